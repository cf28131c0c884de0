"""
The SHIFT form of cond_uniform_kernel<5> (options_set("uniform_shift", 1), the default): where the four cost weights of an instance are
the same doubles at the stages 1 .. N - 1, tile (j, I + j) of the condensed Hessian is tile (0, I) as it stood 8 j stages earlier plus the
terminal stage's product, and the stage loop accumulates block row 0 only (pipe_kernels.hpp). The twins of
tests/test_gpu_uniform_powers.py and tests/test_gpu_cond_uniform_edges.py have weights that differ at every stage: they run the fallback.
Here the weights are STAGE-UNIFORM, different from instance to instance, with a W_e that is different again.

Every case is a pair of TWIN capsules on the problem of tests/test_gpu_uniform_powers.py (batch 1025: the smallest that takes the
record-free chain; yaws on both sides of +-pi; a reference that differs at every stage), the same device calls as the cases there.

Bound, everywhere: bit equality (np.array_equal) of X, U, cost, status, qp_iter, qp_status, res, sl, su and lam after the cold-started
solve, and again after a second solve on the then non-uniform iterate. The shift form issues the same matrix instructions on the same
operands in the same order as the stage loop does for each tile; there is no rounding to allow for.

  shift form against column form   uniform_powers 1 / uniform_shift 1 against uniform_powers 0 at N = 1, 7, 8, 9, 15, 16, 17, 24, 25,
                                   32, 33, 39, 40: the horizons where a snapshot stage N - 8 j - 1 is 0, closes a segment or opens one,
                                   and where a shifted tile is all zero. cond_shifted == 1025 on the one side (0 on the other: the
                                   counter speaks of cond_uniform_kernel only). Six and seven tiles (N > 40) do not take the form.
  shift form against its fallback  uniform_shift 1 against 0 at N = 17 and 40; cond_shifted 1025 and 0.
  mixed batch, N = 40 and 17       every third instance has ONE stage's weight changed by one ulp in one of the four rows, at stage 1,
                                   N - 1, N - 9 or N // 2; one instance differs only in the sign of a zero weight (must leave the form),
                                   one only in row 4 (R: must stay), one only at stage 0 (not a stage of the verdict: must stay); W_e
                                   differs from the stages' weights on every instance and must not leave the form. cond_shifted equals
                                   the count computed here from the weights as the sums take them, dt W (the product, rounded as the
                                   kernel rounds it: a change of one ulp in W may round away in dt W, and then the stage IS the same).
  NaN weights                      a NaN among the weights of the verdict (one stage; all stages alike) leaves the form, one in W_e or R
                                   does not: cond_shifted only.
  reset                            X = 0, U = 0 (the linearisation leaves NaN), uniform weights, N = 9 and 17: equal to the column form,
                                   NaN where the column form has it.
"""
import functools

import numpy as np
import pytest

from test_gpu_uniform_powers import B0, DT, _assert_same, _problem, _snap

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _uniform_diag(N):
    """diagonals of W (B, N, 6), the same at every stage of an instance, and of W_e (B, 4): read-only"""
    x0, yref, wf, wef = _problem(N)
    q = _installed_q()
    Wd = np.repeat((0.01 * q * wf[:, 0])[:, None, :], N, axis=1)
    We = 0.01 * q[:4] * wef
    Wd.setflags(write=False); We.setflags(write=False)
    return Wd, We


@functools.lru_cache(maxsize=None)
def _installed_q():
    from tum_control_amd.config import default_config
    mpc = default_config()["mpc"]          # (what a capsule created without a configuration installs)
    return np.array([mpc["q_lon"] / mpc["s_lon"] ** 2, mpc["q_lat"] / mpc["s_lat"] ** 2, mpc["q_yaw"] / mpc["s_yaw"] ** 2,
                     mpc["q_vel"] / mpc["s_vel"] ** 2, mpc["r_jerk"] / mpc["s_jerk"] ** 2, mpc["r_steering_rate"] / mpc["s_steering_rate"] ** 2])


def _diag(d):
    """(B, n) -> (B, n, n) with exact zeros off the diagonal (a product with an identity would spread a NaN over its column)"""
    M = np.zeros(d.shape + d.shape[-1:])
    i = np.arange(d.shape[-1])
    M[:, i, i] = d
    return M


def _mk(N, powers, shift, Wd, We):
    from tum_control_amd.solver import BatchedOcpSolver
    x0, yref, _, _ = _problem(N)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B0)
    s.install_reference_ocp()
    s.options_set("uniform_powers", powers)
    s.options_set("uniform_shift", shift)
    for k in range(N):
        s.cost_set(k, "W", _diag(Wd[:, k]))
    s.cost_set(N, "W", _diag(We))
    s.set_x0(x0); s.set_yref_all(yref)
    if 1025 * (N + 1) * 8 <= 64 * 1024:          # (as tests/test_gpu_cond_uniform_edges.py: the choice that leaves the records out)
        s.set_kernel("lin-lane-per-stage")
    return s


def _twins_agree(N, a_opts, b_opts, Wd, We, shifted_a, shifted_b):
    a, b = _mk(N, *a_opts, Wd, We), _mk(N, *b_opts, Wd, We)
    for s in (a, b):
        s.cold_start()
        s.solve()
    assert a.get_stats("records_skipped") == 1 and b.get_stats("records_skipped") == 1
    na, nb = a.get_stats("cond_shifted"), b.get_stats("cond_shifted")
    print(f"N={N}: cond_shifted", na, nb, "expected", shifted_a, shifted_b)
    assert na == shifted_a and nb == shifted_b
    sa, sb = _snap(a), _snap(b)
    print(f"N={N}: instances solved", int((sa["status"] == 0).sum()), "of", B0, "qp_iter", int(sa["qp_iter"].min()), "..", int(sa["qp_iter"].max()))
    assert (sa["status"] == 0).sum() > B0 // 2          # (the comparison is of solves, not of failures: at every horizon)
    _assert_same(sa, sb, f"N={N}")
    # the second solve: the iterate is uniform no more, cond_kernel runs on both (and nothing took the shift form)
    for s in (a, b):
        s.solve()
    assert a.get_stats("records_skipped") == 1 and b.get_stats("records_skipped") == 1
    assert a.get_stats("cond_shifted") == 0 and b.get_stats("cond_shifted") == 0
    _assert_same(_snap(a), _snap(b), f"N={N}, second solve")
    a.synchronize(); b.synchronize()


@pytest.mark.parametrize("N", [1, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 39, 40])
def test_shift_form_equals_column_form(N):
    Wd, We = _uniform_diag(N)
    _twins_agree(N, (1, 1), (0, 1), Wd, We, B0, 0)


@pytest.mark.parametrize("N", [17, 40])
def test_shift_form_equals_its_fallback(N):
    Wd, We = _uniform_diag(N)
    _twins_agree(N, (1, 1), (1, 0), Wd, We, B0, 0)


def _takes_the_form(Wd, N):
    """the verdict, from the weights as the sums take them: the bit patterns of dt W[1 .. N - 1, 0..3] equal those of stage 1, no NaN"""
    S = np.ascontiguousarray(np.float64(DT) * Wd[:, 1:N, :4])
    bits = S.view(np.int64)
    return (bits == bits[:, :1]).all(axis=(1, 2)) & ~np.isnan(S).any(axis=(1, 2))


@pytest.mark.parametrize("N", [40, 17])
def test_mixed_batch(N):
    Wu, We = _uniform_diag(N)
    Wd = Wu.copy()
    stages = [1, N - 1, N - 9, N // 2]
    changed = np.arange(0, B0, 3)
    for i, b in enumerate(changed):          # ONE stage's weight, one ulp, one of the four rows
        ks, row = stages[i % 4], (i // 4) % 4
        Wd[b, ks, row] = np.nextafter(Wd[b, ks, row], np.inf)
    Wd[1, :, 1] = 0.0; Wd[1, N // 2, 1] = -0.0          # differs only in the sign of a zero weight
    Wd[2, N // 2, 4] = np.nextafter(Wd[2, N // 2, 4], np.inf)          # row 4 only (R)
    Wd[4, 0, :4] *= 1.5          # stage 0 only: not a stage of the verdict
    takes = _takes_the_form(Wd, N)
    # what the test is about: most of the one-ulp changes survive the product with dt, at every one of the four stages; the special ones
    assert not takes[1] and takes[2] and takes[4]
    for j in range(4):
        assert (~takes[changed[j::4]]).sum() > len(changed[j::4]) // 4, (stages[j], int((~takes[changed[j::4]]).sum()))
    assert takes[np.setdiff1d(np.arange(B0), np.append(changed, 1))].all()
    # (W_e differs from the stages' weights on every instance: a change at stage N alone does not leave the form)
    assert (np.float64(DT) * Wd[:, 1, :4] != We).any(axis=1).all()
    n = int(takes.sum())
    print(f"N={N}: expected in the form", n, "of", B0)
    _twins_agree(N, (1, 1), (0, 1), Wd, We, n, 0)


def test_nan_weight_leaves_the_form():
    """a NaN among the cost weights of the stages 1 .. N - 1 sends the instance to the stage loop with all its products -- at one stage, and
    at every stage with one and the same bit pattern (equal bits are not enough); a NaN in W_e or in R alone does not enter the verdict.
    Only the counter is held here: what such an instance computes is NaN on either path."""
    N = 17
    Wu, We = _uniform_diag(N)
    Wd, We = Wu.copy(), We.copy()
    Wd[5, N // 2, 2] = np.nan          # one stage
    Wd[7, :, 0] = np.nan          # every stage, the same NaN
    Wd[9, N - 1, 3] = np.nan          # the last stage of the verdict
    We[11, 1] = np.nan          # stage N: stays
    Wd[13, 3, 5] = np.nan          # R: stays
    takes = _takes_the_form(Wd, N)
    assert not takes[[5, 7, 9]].any() and int(takes.sum()) == B0 - 3
    s = _mk(N, 1, 1, Wd, We)
    s.cold_start(); s.solve()
    assert s.get_stats("records_skipped") == 1
    assert s.get_stats("cond_shifted") == B0 - 3
    s.synchronize()


@pytest.mark.parametrize("N", [9, 17])
def test_reset_equals_column_form(N):
    """reset(): X = 0, U = 0 at every stage -- the vehicle at rest, the linearisation carries NaN"""
    Wd, We = _uniform_diag(N)
    p, c = _mk(N, 1, 1, Wd, We), _mk(N, 0, 1, Wd, We)
    for s in (p, c):
        s.cold_start(); s.solve()
        s.reset(); s.solve()
    assert p.get_stats("records_skipped") == 2 and c.get_stats("records_skipped") == 2
    assert p.get_stats("cond_shifted") == B0 and c.get_stats("cond_shifted") == 0
    _assert_same(_snap(p), _snap(c), "after reset()")
    p.synchronize(); c.synchronize()


def test_uniform_shift_option_validation():
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=8, dt=DT, nsub=3, batch=4)
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception, match="uniform_shift"):
            s.options_set("uniform_shift", bad)
    with pytest.raises(Exception, match="uniform_shift"):          # the "unknown field" message lists the field
        s.options_set("no_such_option", 1)
    s.options_set("uniform_shift", 0); s.options_set("uniform_shift", 1)
    assert s.get_stats("cond_shifted") == 0          # nothing solved yet
