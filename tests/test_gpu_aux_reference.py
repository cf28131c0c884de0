"""
The covariance back-off of the robustified controller (r2_backoff_kernel, K7) and the PCE moments of a scenario group
(pce_moments_kernel, K6b) against the independent references of tests/test_aux_reference.py, within their derived bounds.

Back-off: always after a WARM solve as well -- after a cold start every A_k is the same matrix and a kernel that reads the
wrong stage of the records computes the same covariances. The reference's A_k is the oracle's rk4_sens at the iterate the
solve linearised at, not what get_from_qp_in expands. Shapes: every tile count of the pipeline, uph below / at / beyond N,
batches that leave idle wavefronts in a workgroup. Every test prints the largest |got - reference| / bound it saw.
"""
import numpy as np
import pytest

from test_aux_reference import (COLD_SHAPES, DT, NSUB, SHAPES, backoff_reference, gpu_bounds, moments_reference_groups, r2_matrices,
                                shape_inputs)

pytestmark = pytest.mark.gpu

ROWS = ("lbu", "ubu", "lbx", "ubx", "lh", "uh")
U53 = 2.0 ** -53


def _mk(N, B, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=N, dt=DT, nsub=NSUB, batch=B, store_qp_in=True, **kw)
    s.install_reference_ocp()
    return s


def _limits():
    from tum_control_amd import config
    return config.VEH["delta_f_min"], config.VEH["delta_f_max"]


def _bounds(s):
    """all six bound rows of every instance: (6, N+1, B)"""
    return np.array([[np.atleast_1d(s.constraints_get(k, f)) for k in range(s.N + 1)] for f in ROWS])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _start(N, B):
    x0, yref = shape_inputs(N, B)
    s = _mk(N, B)
    s.set_x0(x0 if B > 1 else x0[0]); s.set_yref_all(yref if B > 1 else yref[0]); s.cold_start()
    return s, x0


def _solve(s):
    s.solve()
    X, U = s.get_iterate()
    return np.atleast_1d(s.get_stats("status")).copy(), X, U


def _hold_backoff(s, Xlin, Ulin, Xnew, uph, tag, skip=()):
    """one r2_backoff call on capsule s against the reference, instance by instance and stage by stage; returns the back-offs"""
    N, B = s.N, s.batch
    S0, BWB = r2_matrices()
    dmin, dmax = _limits()
    before = _bounds(s)
    bo = s.r2_backoff(S0, BWB, uph, dmin, dmax, 1.0, return_backoffs=True)
    after = _bounds(s)
    worst = 0.0
    for b in range(B):
        if b in skip:
            continue
        bd, bh, ebd, ebh = backoff_reference(Xlin[b], Ulin[b], Xnew[b], S0, BWB, uph, N)
        tbd, tbh = gpu_bounds(ebd, ebh)
        dd, dh = np.abs(bo[b, :, 0] - bd), np.abs(bo[b, :, 1] - bh)
        if uph > 1:
            worst = max(worst, (dd[1:] / tbd[1:]).max(), (dh[1:] / tbh[1:]).max())
        assert (dd <= tbd).all() and (dh <= tbh).all(), (tag, b, (dd[1:] / tbd[1:]).max(), (dh[1:] / tbh[1:]).max())
        # the bounds installed for the next solve: the kernel's own back-offs to the bit, hence the reference's within the bound
        # (and the rounding of the sum: the limits are below 1)
        assert _same_bits(after[2, 1:N, b], dmin + bo[b, 1:, 0]) and _same_bits(after[3, 1:N, b], dmax - bo[b, 1:, 0])
        assert _same_bits(after[5, 1:N, b], 1.0 - bo[b, 1:, 1])
        assert (np.abs(after[2, 1:N, b] - (dmin + bd[1:])) <= tbd[1:] + U53).all()
        assert (np.abs(after[3, 1:N, b] - (dmax - bd[1:])) <= tbd[1:] + U53).all()
        assert (np.abs(after[5, 1:N, b] - (1.0 - bh[1:])) <= tbh[1:] + U53).all()
        # stage 0, stage N and the rows the tightening does not own
        assert _same_bits(after[:, 0, b], before[:, 0, b]) and _same_bits(after[:, N, b], before[:, N, b])
        assert _same_bits(after[[0, 1, 4], :, b], before[[0, 1, 4], :, b])
    print(f"{tag}: worst |got - reference| / bound = {worst:.3f}")
    return bo, before, after


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("N,uph,B", SHAPES)
def test_warm_backoff_against_reference(N, uph, B):
    """cold start, solve, solve again at the same x0: the back-off of the SECOND solve (A_k at the first solve's iterate, a
    different matrix at every stage; the gradient at the second solve's iterate)"""
    s, x0 = _start(N, B)
    st, X1, U1 = _solve(s)
    assert (st == 0).all()
    st, X2, U2 = _solve(s)
    assert (st == 0).all()
    assert X1[:, :, 3].min() > 1.0 and X2[:, :, 3].min() > 1.0
    _hold_backoff(s, X1, U1, X2, uph, f"r2 warm N={N} uph={uph} B={B}")


@pytest.mark.parametrize("N,uph,B", COLD_SHAPES)
def test_cold_backoff_against_reference(N, uph, B):
    """the case the suite had, on the independent A and the derived bound: linearised at X_k = x0, U = 0"""
    s, x0 = _start(N, B)
    st, X1, U1 = _solve(s)
    assert (st == 0).all()
    Xl = np.repeat(x0[:, None, :], N + 1, axis=1)
    _hold_backoff(s, Xl, np.zeros((B, N, 2)), X1, uph, f"r2 cold N={N} uph={uph} B={B}")


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("N,B", [(17, 3), (49, 2)])
def test_uph_edges(N, B):
    S0, BWB = r2_matrices()
    dmin, dmax = _limits()
    s, x0 = _start(N, B)
    _solve(s)
    nominal = _bounds(s)
    st, X2, U2 = _solve(s)
    assert (st == 0).all()
    # beyond the horizon: the bits of uph = N
    boN = s.r2_backoff(S0, BWB, N, dmin, dmax, 1.0, return_backoffs=True)
    bN = _bounds(s)
    bo3 = s.r2_backoff(S0, BWB, N + 3, dmin, dmax, 1.0, return_backoffs=True)
    assert _same_bits(bo3, boN) and _same_bits(_bounds(s), bN)
    assert (boN[:, 1:, 1] > 0).all() and not _same_bits(bN, nominal)
    # uph = 1: no covariance is propagated, the nominal bounds on the stages 1..N-1
    bo1 = s.r2_backoff(S0, BWB, 1, dmin, dmax, 1.0, return_backoffs=True)
    assert (bo1 == 0.0).all() and _same_bits(_bounds(s), nominal)
    for bad in (0, -1, -7):
        with pytest.raises(Exception, match="uncertainty propagation horizon < 1"):
            s.r2_backoff(S0, BWB, bad, dmin, dmax, 1.0)
    assert _same_bits(_bounds(s), nominal)
    # attached, then detached with uph = 0: the next solve leaves the bounds alone
    s.r2_attach(S0, BWB, 5, dmin, dmax, 1.0)
    s.solve()
    tight = _bounds(s)
    assert (tight[5, 1:N] < 1.0).all()
    s.r2_attach(S0, BWB, 0, dmin, dmax, 1.0)
    s.r2_backoff(S0, BWB, 1, dmin, dmax, 1.0)
    s.solve()
    assert _same_bits(_bounds(s), nominal)
    with pytest.raises(Exception, match="uncertainty propagation horizon < 1"):
        s.r2_attach(S0, BWB, -2, dmin, dmax, 1.0)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_failed_instance_inside_a_workgroup():
    """six instances = two workgroups of four wavefronts; instance 1 fails (status 4): its six bound rows keep their bits, its
    back-offs read 0, and the wavefronts it shares the barriers with meet the reference"""
    N, uph, B = 40, 5, 6
    S0, BWB = r2_matrices()
    dmin, dmax = _limits()
    s, x0 = _start(N, B)
    st, X1, U1 = _solve(s)
    assert (st == 0).all()
    s.r2_backoff(S0, BWB, uph, dmin, dmax, 1.0)          # (so that the rows instance 1 must keep are not the nominal ones)
    Xp = X1.copy(); Xp[1, 3:7, :] = np.nan
    s.set_iterate(Xp, U1)
    st, X2, U2 = _solve(s)
    assert st[1] == 4 and (np.delete(st, 1) == 0).all(), st
    bo, before, after = _hold_backoff(s, X1, U1, X2, uph, f"r2 failed instance N={N} uph={uph} B={B}", skip=(1,))
    assert _same_bits(after[:, :, 1], before[:, :, 1]) and (before[5, 1:N, 1] < 1.0).all()
    assert (bo[1] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("N,uph,B", [(41, 5, 5), (56, 20, 3)])
def test_attached_equals_one_shot(N, uph, B):
    S0, BWB = r2_matrices()
    dmin, dmax = _limits()
    a, x0 = _start(N, B)
    nominal = _bounds(a)
    for _ in range(2):
        assert a.solve() == 0
        a.r2_backoff(S0, BWB, uph, dmin, dmax, 1.0)
    Xa, Ua = a.get_iterate()
    c, _ = _start(N, B)
    c.r2_attach(S0, BWB, uph, dmin, dmax, 1.0)
    c.bounds_snapshot()
    assert c.solve() == 0 and c.solve() == 0
    Xc, Uc = c.get_iterate()
    assert _same_bits(Xc, Xa) and _same_bits(Uc, Ua)
    ba = _bounds(a)
    assert _same_bits(_bounds(c), ba) and (ba[5, 1:N] < 1.0).all()
    c.bounds_restore()
    assert _same_bits(_bounds(c), nominal)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_r2_bounds_device_loop_against_host_loop():
    """the tightened bounds at the end of a closed loop, all-device loop against the loop on the host (the trajectories are
    compared in tests/test_gpu_pipeline.py, with this tolerance): N = 47, the six-tile pipeline, back-off from its stage records"""
    from tum_control_amd.closed_loop import ClosedLoopBatch
    N, B, steps = 47, 3, 12
    got = {}
    for dev in (False, True):
        cl = ClosedLoopBatch("modena", batch=B, N=N, Tp=3.76, on_device=dev, log_capacity=steps, controller="r2")
        lg = cl.run(steps)
        assert (lg["simSolverDebug"][:, :, 4] == 0).all()
        got[dev] = _bounds(cl.solver)
    worst = 0.0
    for r in (2, 3, 5):
        np.testing.assert_allclose(got[True][r], got[False][r], rtol=1e-8, atol=1e-8, err_msg=ROWS[r])
        worst = max(worst, (np.abs(got[True][r] - got[False][r]) / (1e-8 + 1e-8 * np.abs(got[False][r]))).max())
    # really tightened, and only where the tightening writes: stage 0, stage N and the other rows are the same bits in both loops
    assert (got[True][5, 1:N] < 1.0).all() and (got[True][5, N] == 1.0).all()
    assert _same_bits(got[True][:, [0, N]], got[False][:, [0, N]]) and _same_bits(got[True][[0, 1, 4]], got[False][[0, 1, 4]])
    print(f"r2 device loop vs host loop N={N} B={B}: worst |dev - host| / tolerance = {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ 7
PCE_SL = [(1, 1), (3, 2), (15, 10), (31, 20)]


def _pce_matrix(rng, L, S):
    A = rng.standard_normal((L, S))
    A[1:] -= A[1:].mean(axis=1, keepdims=True)          # rows k >= 1 sum to zero: a common offset of the group cancels in the variance
    return A


@pytest.mark.parametrize("N", [5, 41])
@pytest.mark.parametrize("P", [1, 17])
def test_pce_moments_against_reference(N, P):
    """synthetic iterates (positions of size 1e3, the members of a group 1e-3 .. 1 apart, the nominal instance far off), both
    fields, first / inner / last stage, S and L from 1 up; P = 17: 136 (group, component) pairs, more than one block of 128"""
    import torch
    from tum_control_amd.solver import BatchedOcpSolver
    rng = np.random.default_rng(100 * N + P)
    worst = 0.0
    for S, L in PCE_SL:
        S1 = S + 1
        B = P * S1
        s = BatchedOcpSolver(N=N, dt=DT, nsub=NSUB, batch=B)
        scale = np.array([1e3, 1e3, 3.0, 30.0, 1.0, 0.5, 0.3, 2.0])
        X = (scale * rng.uniform(-1.0, 1.0, (P, 1, N + 1, 8)) + rng.choice([-1.0, 1.0], (P, S1, N + 1, 8)) * 10.0 ** rng.uniform(-3, 0, (P, S1, N + 1, 8)))
        U = (0.3 * rng.uniform(-1.0, 1.0, (P, 1, N, 2)) + rng.choice([-1.0, 1.0], (P, S1, N, 2)) * 10.0 ** rng.uniform(-3, 0, (P, S1, N, 2)))
        X[:, 0] += 500.0; U[:, 0] += 5.0          # the nominal instance of a group is not part of the moments
        s.set_iterate(X.reshape(B, N + 1, 8), U.reshape(B, N, 2))
        A = _pce_matrix(rng, L, S)
        s.pce_attach(A)
        for field, stage in (("x", 0), ("x", 1), ("x", N), ("u", 0), ("u", N - 1)):
            V = (X if field == "x" else U)[:, 1:, stage]          # (P, S, m)
            m = V.shape[-1]
            mean, var = s.pce_moments(field, stage, A)
            rm, rv, em, ev = moments_reference_groups(A, V)
            assert mean.shape == (P, m) and var.shape == (P, m)
            dm, dv = np.abs(mean - rm), np.abs(var - rv)
            assert (dm <= em).all() and (dv <= ev).all(), (field, stage, S, L, (dm / em).max(), (dv[ev > 0] / ev[ev > 0]).max() if L > 1 else 0.0)
            worst = max(worst, (dm / em).max(), (dv[ev > 0] / ev[ev > 0]).max() if L > 1 else 0.0)
            if L == 1:
                assert (var == 0.0).all()
            mv = torch.full((2, P, m), np.nan, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            s.pce_moments_device(field, stage, mv[0].data_ptr(), mv[1].data_ptr())
            s.synchronize()
            assert _same_bits(mv[0].cpu().numpy(), mean) and _same_bits(mv[1].cpu().numpy(), var), (field, stage, S, L)
    print(f"pce moments N={N} P={P}: worst |got - reference| / bound = {worst:.3f}")


def test_pce_moments_refusals():
    import torch
    from tum_control_amd.solver import BatchedOcpSolver
    N, S, L = 5, 3, 2
    s = BatchedOcpSolver(N=N, dt=DT, nsub=NSUB, batch=2 * (S + 1))
    A = _pce_matrix(np.random.default_rng(0), L, S)
    mv = torch.zeros((2, 2, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(Exception, match="no PCE matrix registered"):
        s.pce_moments_device("x", 1, mv[0].data_ptr(), mv[1].data_ptr())
    with pytest.raises(Exception, match="pce_moments: stage"):
        s.pce_moments("u", N, A)
    with pytest.raises(Exception, match="pce_moments: stage"):
        s.pce_moments("x", N + 1, A)
    with pytest.raises(Exception, match="pce_moments: stage"):
        s.pce_moments("x", -1, A)
    with pytest.raises(Exception, match="unknown field"):
        s.pce_moments("z", 0, A)
    with pytest.raises(Exception, match=r"multiple of S\+1"):
        s.pce_moments("x", 1, _pce_matrix(np.random.default_rng(1), 2, 4))          # 8 instances, groups of 5
    with pytest.raises(Exception, match=r"multiple of S\+1"):
        s.pce_attach(_pce_matrix(np.random.default_rng(1), 2, 4))
    s.pce_attach(A)
    with pytest.raises(Exception, match="pce_moments: stage"):
        s.pce_moments_device("u", N, mv[0].data_ptr(), mv[1].data_ptr())
    s.synchronize()
    assert (mv.cpu().numpy() == 0.0).all()          # nothing refused has written
