"""
A stage-uniform iterate condensed and expanded WITHOUT stage records (options_set("uniform_records", 0), the default):
lin_uniform_kernel, cond_uniform_kernel, ipm_kernel, expand_uniform_kernel -- lin_fill_kernel is not launched and the record
workspace is not written -- where a whole SQP-RTI step of the nominal OCP runs on a cold-started / reset iterate, nothing behind the
solve reads the records (no store_qp_in) and the expansion is a kernel of its own (more than 1024 instances).

Every case is held against a TWIN capsule with uniform_records 1 (the records are filled, cond_kernel and expand_kernel read them).

Bound: bit equality of everything a solve leaves behind. The two condensing kernels and the two expansion kernels share their
bodies; the record-free forms build each operand by the operation lin_fill_kernel applies to the same numbers (xn - X_0,
X_0 - yref_k with the yaw wrapped), and nothing is summed in another order: there is no rounding to allow for.

get_stats("records_skipped") counts the solves that ran without records; it tells which kernels a solve ran.

Shapes: batch 1025 is the smallest at which the expansion is its own kernel (1024: it is the tail of ipm_kernel and reads records).
Horizons 38, 40 | 41, 48 | 49, 56 are the edges of the five-, six- and seven-tile builds; 38, 41 and 49 leave padded stages.

The safety net (expand_uniform_kernel compares every stage of the old iterate with stage 0, as lin_fill_kernel does where records are
written, and the next synchronous call fails) is never provoked, for the reason tests/test_gpu_lin_uniform.py gives: the cases that
invalidate the iterate end with a synchronize(), which would raise had the path run on an iterate that was not uniform.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.08
B0 = 1025


def _mk(N, B, keep_records, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B, **kw)
    s.install_reference_ocp()
    s.options_set("uniform_records", keep_records)
    return s


@functools.lru_cache(maxsize=None)
def _batch(N, seed=None):
    from tum_control_amd.workloads import nominal_batch
    x0, yref = nominal_batch(B0, N=N) if seed is None else nominal_batch(B0, N=N, seed=seed)
    x0.setflags(write=False); yref.setflags(write=False)
    return x0, yref


def _pair(N, B=B0, **kw):
    """the capsule under test (uniform_records 0) and its twin (uniform_records 1) with the same problem, not yet cold-started"""
    x0, yref = _batch(N)
    pair = _mk(N, B, 0, **kw), _mk(N, B, 1, **kw)
    for s in pair:
        s.set_x0(x0[:B]); s.set_yref_all(yref[:B])
    return pair


def _snap(s, records=False):
    """everything a solve leaves behind: X, U, cost, status, qp_iter, qp_status, res, and per stage sl, su, lam (+ A, B, b)"""
    X, U = s.get_iterate()
    r = dict(X=X, U=U, cost=np.atleast_1d(s.get_cost()), status=s.get_stats("status"), qp_iter=s.get_stats("qp_iter"),
             qp_status=s.get_stats("qp_status"), res=np.atleast_2d(s.get_stats("res")))
    for f in ("sl", "su", "lam"):
        r[f] = np.concatenate([np.atleast_2d(s.get(k, f)).reshape(s.batch, -1) for k in range(s.N + 1)], axis=1)
    if records:
        for f in ("A", "B", "b"):
            r[f] = np.stack([s.get_from_qp_in(k, f) for k in range(s.N)], axis=1)
    return r


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    differ = []
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])          # (a failed instance carries NaN on both sides)
        print(what, k, "max |difference|", float(np.nanmax(np.abs(x.astype(float) - y.astype(float)))) if x.size else 0.0)
        if not (x.shape == y.shape and np.array_equal(x, y, equal_nan=(x.dtype.kind == "f"))):
            differ.append(k)
    assert not differ, (what, differ)


# ------------------------------------------------------------------------------------------------- 1: the record-free path, bit for bit
@pytest.mark.parametrize("N", [38, 40, 41, 48, 49, 56])
def test_cold_start_without_records_equals_with_records(N):
    u, g = _pair(N)
    for s in (u, g):
        s.cold_start()
        assert s.solve() == 0
    assert u.get_stats("records_skipped") == 1 and g.get_stats("records_skipped") == 0
    assert u.get_stats("lin_uniform") == 1 and g.get_stats("lin_uniform") == 1
    _assert_same(_snap(u), _snap(g), f"N={N}")


# ------------------------------------------------------------------------------------------------- 2: reset
def test_reset_without_records_equals_with_records():
    """reset(): X = 0, U = 0 at every stage (the vehicle at rest: whatever the solve makes of it, both paths make the same)"""
    u, g = _pair(40)
    for s in (u, g):
        s.cold_start(); s.solve()
        s.reset(); s.solve()
    assert u.get_stats("records_skipped") == 2 and g.get_stats("records_skipped") == 0
    assert u.get_stats("lin_uniform") == 2 and g.get_stats("lin_uniform") == 2
    _assert_same(_snap(u), _snap(g), "after reset()")


# ------------------------------------------------------------------------------------------------- 3: where the records stay
def test_store_qp_in_keeps_the_records():
    u, g = _pair(40, store_qp_in=True)
    for s in (u, g):
        s.cold_start()
        assert s.solve() == 0
    assert u.get_stats("records_skipped") == 0 and u.get_stats("lin_uniform") == 1
    _assert_same(_snap(u, records=True), _snap(g, records=True), "store_qp_in")


def test_fused_expansion_keeps_the_records():
    """1024 instances: the expansion is the tail of ipm_kernel, which reads the records"""
    u, g = _pair(40, B=1024)
    for s in (u, g):
        s.cold_start()
        assert s.solve() == 0
    assert u.get_stats("records_skipped") == 0 and u.get_stats("lin_uniform") == 1
    _assert_same(_snap(u), _snap(g), "1024 instances")


@pytest.mark.parametrize("first_without_records", [False, True])
def test_second_solve_without_cold_start_keeps_the_records(first_without_records):
    """first_without_records: the solve in front ran record-free -- the second one linearises stage by stage into a workspace that
    nothing has written yet, and counts nothing; otherwise both solves of the capsule under test fill records (count 0)"""
    u, g = _pair(40)
    if not first_without_records:
        u.options_set("uniform_records", 1)
    for s in (u, g):
        s.cold_start()
        assert s.solve() == 0
    first = 1 if first_without_records else 0
    assert u.get_stats("records_skipped") == first
    u.options_set("uniform_records", 0)
    for s in (u, g):
        assert s.solve() == 0
    assert u.get_stats("records_skipped") == first and u.get_stats("lin_uniform") == 1
    _assert_same(_snap(u), _snap(g), "second solve")
    u.synchronize()


@pytest.mark.parametrize("stage,field", [(3, "x"), (0, "u")])
def test_set_after_cold_start_keeps_the_records(stage, field):
    u, g = _pair(40)
    rng = np.random.default_rng(5)
    v = _batch(40)[0] + 1e-3 * rng.standard_normal((B0, 8)) if field == "x" else 1e-2 * rng.standard_normal((B0, 2))
    for s in (u, g):
        s.cold_start(); s.set(stage, field, v)
        assert s.solve() == 0
    assert u.get_stats("records_skipped") == 0 and u.get_stats("lin_uniform") == 0
    _assert_same(_snap(u), _snap(g), f"set({stage}, {field})")
    u.synchronize()


def test_rti_phases_keep_the_records():
    """a preparation is not a whole step: the feedback kernel reads the records"""
    u, g = _pair(40)
    for s in (u, g):
        s.cold_start()
        assert s.prepare() == 0
        assert s.feedback() == 0
    assert u.get_stats("records_skipped") == 0 and u.get_stats("lin_uniform") == 1
    _assert_same(_snap(u), _snap(g), "prepare + feedback")
    u.synchronize()


def test_sqp_mode_keeps_the_records():
    """the residual pass of an SQP solve reads the records"""
    u, g = _pair(40, nlp_solver_type="SQP", nlp_solver_max_iter=4)
    for s in (u, g):
        s.cold_start(); s.solve()
    assert u.get_stats("records_skipped") == 0 and u.get_stats("lin_uniform") == 1
    a, b = _snap(u), _snap(g)
    for s, r in ((u, a), (g, b)):
        r["sqp_iter"] = s.get_stats("sqp_iter"); r["residuals"] = s.get_stats("residuals")
    _assert_same(a, b, "SQP")
    u.synchronize()


# ------------------------------------------------------------------------------------------------- 4: batches in flight
@pytest.mark.parametrize("upload", ["bind_device", "put_device"])
def test_ring_of_three_capsules_two_rounds(upload):
    """three capsules on three streams, two fresh batches each (the reference differs per stage and per instance), the inputs on the
    device: bound in place or copied. The record-free condensing and expansion read the reference while other capsules' batches run"""
    import torch
    from tum_control_amd.streaming import SolverRing
    N = 40
    batches = [_batch(N, seed=300 + k) for k in range(6)]
    dev = [[torch.as_tensor(np.array(v), device="cuda:0") for v in b] for b in batches]          # (a writable copy: the cached batches are read-only)
    torch.cuda.synchronize()
    got = []
    for keep in (0, 1):
        ring = SolverRing(3, lambda i: _mk(N, B0, keep))
        for k in range(6):
            slot, s = ring.acquire()
            getattr(s, upload)("x0", dev[k][0].data_ptr()); getattr(s, upload)("yref", dev[k][1].data_ptr())
            s.cold_start(); s.solve_async()
            ring.request_results(slot, with_iterate=True)
        res = [(slot, [np.array(a) for a in r]) for slot, r in ring.drain()]
        ring.synchronize()
        assert [slot for slot, _ in res] == [0, 1, 2, 0, 1, 2]
        assert [s.get_stats("records_skipped") for s in ring] == [0 if keep else 2] * 3
        assert [s.get_stats("lin_uniform") for s in ring] == [2] * 3
        got.append((res, [_snap(s) for s in ring]))
    (res_u, snap_u), (res_g, snap_g) = got
    for k in range(6):
        for name, a, b in zip(("summary", "X", "U"), res_u[k][1], res_g[k][1]):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (upload, "batch", k, name)
        assert (res_u[k][1][0][:, 3] == 0).all()
    assert not np.array_equal(res_u[0][1][1], res_u[3][1][1])          # (the rounds were different batches)
    for i in range(3):
        _assert_same(snap_u[i], snap_g[i], f"{upload} capsule {i}")


# ------------------------------------------------------------------------------------------------- 5: the option
def test_uniform_records_option_validation():
    s = _mk(8, 4, 0)
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception, match="uniform_records"):
            s.options_set("uniform_records", bad)
    with pytest.raises(Exception, match="uniform_records"):          # the "unknown field" message lists the field
        s.options_set("no_such_option", 1)
    with pytest.raises(Exception, match="lin_dedup"):                # ... and keeps listing lin_dedup
        s.options_set("no_such_option", 1)
