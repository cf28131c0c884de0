"""
The longest-first schedule (lpt_order_kernel, common_kernels.hpp): the order the NEXT solve dispatches its instances in, from the iteration
counts of this one -- a stable counting sort by one wavefront: iteration counts (clipped to 0..63) descending, instances of one count by
ascending index. get_stats("lpt_order") reads it.

  * batches 1025 and 4096 (more than one round of resident wavefronts: the schedule is kept; 1025 leaves the lanes' shares uneven and the
    last lane's short), N = 8: the order equals np.lexsort((arange(B), -clip(qp_iter, 0, 63))) -- exactly, it is a permutation of integers;
  * instances are independent: the solve behind set_schedule(True) and the one behind set_schedule(False) leave bit-identical iterates;
  * a batch of at most 1024 keeps no order: the identity map the capsule starts from stays.

Inputs: x0 spread widely (speeds 5..40 m/s, yaws anywhere, offsets from the reference), so that the iteration counts differ.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.08
N = 8


@functools.lru_cache(maxsize=None)
def _problem(B):
    rng = np.random.default_rng(9100 + B)
    x0 = np.zeros((B, 8))
    x0[:, 0:2] = 50.0 * rng.standard_normal((B, 2))
    x0[:, 2] = rng.uniform(-np.pi, np.pi, B)
    x0[:, 3] = rng.uniform(5.0, 40.0, B)
    x0[:, 4] = 0.3 * rng.standard_normal(B)
    x0[:, 5] = 0.1 * rng.standard_normal(B)
    x0[:, 6] = 0.02 * rng.standard_normal(B)
    x0[:, 7] = 1.0 * rng.standard_normal(B)
    t = DT * np.arange(N + 1)[None, :]
    yref = np.zeros((B, N + 1, 6))
    off = rng.uniform(0.0, 3.0, (B, 1))          # how far the vehicle starts from its reference: what the iteration count follows
    yref[:, :, 0] = x0[:, 0:1] + x0[:, 3:4] * t * np.cos(x0[:, 2:3]) + off * rng.standard_normal((B, 1))
    yref[:, :, 1] = x0[:, 1:2] + x0[:, 3:4] * t * np.sin(x0[:, 2:3]) + off * rng.standard_normal((B, 1))
    yref[:, :, 2] = np.mod(x0[:, 2], 2.0 * np.pi)[:, None]
    yref[:, :, 3] = x0[:, 3:4] + off * rng.standard_normal((B, 1))
    for a in (x0, yref):
        a.setflags(write=False)
    return x0, yref


def _mk(B):
    from tum_control_amd.solver import BatchedOcpSolver
    x0, yref = _problem(B)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B)
    s.install_reference_ocp()
    s.set_x0(x0); s.set_yref_all(yref)
    return s


def _expected(qp_iter):
    B = qp_iter.shape[0]
    return np.lexsort((np.arange(B), -np.clip(qp_iter, 0, 63)))


@pytest.mark.parametrize("B", [1025, 4096])
def test_order_is_the_stable_sort_and_does_not_change_results(B):
    a, n = _mk(B), _mk(B)
    for s in (a, n):
        s.cold_start()
        s.solve()
    it = a.get_stats("qp_iter")
    print(f"B={B}: qp_iter", int(it.min()), "..", int(it.max()), "distinct", np.unique(it).size)
    assert np.unique(it).size > 1          # (an order with one count only would be the identity map)
    order = a.get_stats("lpt_order")
    assert order.dtype == np.int32 and order.shape == (B,)
    assert np.array_equal(order, _expected(it))
    assert np.array_equal(n.get_stats("lpt_order"), order)          # the same counts, the same order: nothing in it is left to chance
    # the following solve: longest-first on one twin, natural order on the other
    a.set_schedule(True); n.set_schedule(False)
    for s in (a, n):
        s.solve()
    (Xa, Ua), (Xn, Un) = a.get_iterate(), n.get_iterate()
    assert np.array_equal(Xa, Xn, equal_nan=True) and np.array_equal(Ua, Un, equal_nan=True)
    assert np.array_equal(a.get_stats("qp_iter"), n.get_stats("qp_iter"))
    # and the order that solve left behind
    assert np.array_equal(a.get_stats("lpt_order"), _expected(a.get_stats("qp_iter")))
    a.synchronize(); n.synchronize()


def test_no_order_up_to_1024_instances():
    s = _mk(1024)
    s.cold_start()
    s.solve()
    assert np.unique(s.get_stats("qp_iter")).size > 1
    assert np.array_equal(s.get_stats("lpt_order"), np.arange(1024))
    s.synchronize()
