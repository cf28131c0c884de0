"""
Full SQP solves (nlp_solver_type SQP) on the GPU (-m gpu): config 2 (4096 x N = 40, cold start) against the SQP-RTI path the
mode is built from, against the test-side SQP reference of tests/test_sqp.py, and the refusals.
"""
import os

import numpy as np
import pytest

from test_sqp import N, make_oracle, oracle_sqp, res_eq

pytestmark = pytest.mark.gpu

B = 4096


def _mk(B, N=N, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=N, dt=0.08, nsub=3, batch=B, **kw)
    s.install_reference_ocp()
    return s


def _start(s, x0, yref):
    s.set_x0(x0); s.set_yref_all(yref); s.cold_start()


def _config2():
    from tum_control_amd.workloads import nominal_batch
    return nominal_batch(B, N=N)


def test_sqp_one_iteration_is_one_rti():
    """max_iter = 1: X, U and qp_iter are those of one SQP-RTI solve, to the bit; the residual pass behind the QP reports"""
    x0, yref = _config2()
    r = _mk(B); _start(r, x0, yref); r.solve()
    Xr, Ur = r.get_iterate(); itr, str_ = r.get_stats("qp_iter"), r.get_stats("status")
    s = _mk(B, nlp_solver_type="SQP", nlp_solver_max_iter=1); _start(s, x0, yref)
    s.solve()
    X, U = s.get_iterate()
    np.testing.assert_array_equal(X, Xr)
    np.testing.assert_array_equal(U, Ur)
    np.testing.assert_array_equal(s.get_stats("qp_iter"), itr)
    assert (s.get_stats("sqp_iter") == 1).all()
    st = s.get_stats("status")
    assert ((st == 4) == (str_ == 4)).all() and np.isin(st, (0, 2, 4)).all()
    res = s.get_residuals()
    assert res.shape == (B, 4) and np.isfinite(res).all()


def test_sqp_zero_tolerance_is_five_rti_solves():
    """tolerances 0, max_iter 5: X and U equal five consecutive SQP-RTI solves (QP warm start on in both) to the bit; every
    instance ends at the cap (status 2) with sqp_iter 5 -- or with status 4, frozen at its last good iterate, where the RTI
    sequence had a failed QP as well"""
    x0, yref = _config2()
    r = _mk(B, qp_warm_start=True); _start(r, x0, yref)
    failed = np.zeros(B, bool)
    for _ in range(5):
        r.solve(); failed |= r.get_stats("status") == 4
    Xr, Ur = r.get_iterate()
    tol = dict(nlp_solver_tol_stat=0.0, nlp_solver_tol_eq=0.0, nlp_solver_tol_ineq=0.0, nlp_solver_tol_comp=0.0)
    s = _mk(B, qp_warm_start=True, nlp_solver_type="SQP", nlp_solver_max_iter=5, **tol); _start(s, x0, yref)
    s.solve()
    X, U = s.get_iterate()
    st, it = s.get_stats("status"), s.get_stats("sqp_iter")
    ok = st == 2
    assert np.isin(st, (2, 4)).all()
    assert (it[ok] == 5).all()
    assert failed[st == 4].all() and (~failed[ok]).all()
    np.testing.assert_array_equal(X[ok], Xr[ok])
    np.testing.assert_array_equal(U[ok], Ur[ok])


def _scale_rel(A, Aref):
    """error relative to the scale of each channel over the batch's trajectories (yaw: pi), tests/golden/replay_full_logs.py"""
    sc = np.abs(Aref).reshape(-1, Aref.shape[-1]).max(axis=0)
    if Aref.shape[-1] == 8:
        sc[2] = np.pi
    sc = np.maximum(sc, 1e-3)
    return (np.abs(A - Aref) / sc).reshape(A.shape[0], -1).max(axis=1)


def test_sqp_defaults_parity_with_oracle():
    """Defaults (tolerances 1e-6, 100 QPs) on all 4096 instances: converged instances meet the tolerances; res_eq is the defect of
    the returned iterate as numpy evaluates it; X, U follow the oracle's SQP over the same number of QPs; a further SQP-RTI step
    from a converged iterate barely moves it (median below 1e-5, largest below 1e-4, scale-relative); converged / not converged
    agrees with the oracle's residual test."""
    from oracle.oracle import rk4_sens
    x0, yref = _config2()
    s = _mk(B, nlp_solver_type="SQP"); _start(s, x0, yref)
    s.solve()
    X, U = s.get_iterate()
    st, it, res = s.get_stats("status"), s.get_stats("sqp_iter"), s.get_residuals()
    conv = st == 0
    print(f"converged {conv.sum()} / {B}, cap {(st == 2).sum()}, failed {(st == 4).sum()}; median sqp_iter of the converged {np.median(it[conv])}; "
          f"non-finite residuals by status: {[(int(k), int((~np.isfinite(res[st == k]).all(axis=1)).sum())) for k in (0, 2, 4)]}")
    # (an instance whose full steps diverge can end with a failed QP at an iterate where the model no longer evaluates: status 4)
    assert np.isin(st, (0, 2, 4)).all() and np.isfinite(res[st != 4]).all()
    assert conv.sum() > B // 5
    assert (res[conv] < 1e-6).all()
    assert (it[st == 2] == 100).all()
    # res_eq: numpy's defects at the returned iterate (relative to the size of the state)
    for b in range(0, B, 8):
        d = max([np.abs(x0[b] - X[b, 0]).max()] + [np.abs(rk4_sens(X[b, k], U[b, k], 0.08, 3)[0] - X[b, k + 1]).max() for k in range(N)])
        assert abs(res[b, 1] - d) <= 1e-12 * max(1.0, np.abs(X[b]).max()), (b, res[b, 1], d)
    # the oracle's SQP on a strided subset: the same number of QPs, then the same iterate
    idx = np.arange(3, B, 64)
    o = make_oracle()
    Xo, Uo = np.zeros((len(idx), N + 1, 8)), np.zeros((len(idx), N, 2))
    agree = 0
    for j, b in enumerate(idx):
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        n_o, conv_o, res_o = oracle_sqp(o, 100, tol=1e-6)
        agree += conv_o == conv[b]
        if conv_o != conv[b]:          # (only at the edge of the tolerance: one side converged within an iteration of the other's count)
            assert abs(n_o - it[b]) <= 1 or max(n_o, it[b]) >= 99, (b, n_o, conv_o, it[b], conv[b], res_o, res[b])
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        oracle_sqp(o, int(it[b]), tol=0.0, with_stat=False)
        Xo[j], Uo[j] = o.X, o.U
    assert agree >= len(idx) - 2, agree
    c = conv[idx]
    ex, eu = _scale_rel(X[idx], Xo), _scale_rel(U[idx], Uo)
    print(f"scale-relative X / U against the oracle: converged {ex[c].max():.2e} / {eu[c].max():.2e}, all {ex.max():.2e} / {eu.max():.2e}")
    assert ex[c].max() < 1e-6 and eu[c].max() < 1e-6
    # one more real-time iteration from the converged iterates
    s.options_set("nlp_solver_type", "SQP_RTI")
    s.solve()
    X2, U2 = s.get_iterate()
    mv = np.maximum(_scale_rel(X2[conv], X[conv]), _scale_rel(U2[conv], U[conv]))
    print(f"further SQP-RTI step from the converged iterates: scale-relative {mv.max():.2e}, absolute "
          f"{max(np.abs(X2 - X)[conv].max(), np.abs(U2 - U)[conv].max()):.2e}")
    # (one more Gauss-Newton step is the inverse curvature times a stationarity residual below 1e-6: measured scale-relative median
    #  ~5e-6 and largest 3.8e-5 -- over the input channels, whose curvature is the smallest)
    assert np.median(mv) < 1e-5 and mv.max() < 1e-4, (np.median(mv), mv.max())


def test_sqp_refusals_and_rti_unchanged():
    """SQP is refused with a message for an R2-attached capsule, the coupled SNMPC OCP, the development kernel 'fused' and the
    one-call step; a default solver keeps sqp_iter == 1 and the QP residuals 'res' it always had"""
    from tum_control_amd import config, snmpc as snm
    from tum_control_amd.r2nmpc import r2_setup
    from tum_control_amd.solver import CoupledSnmpcSolver, dev_library
    from tum_control_amd.workloads import nominal_batch
    x0, yref = nominal_batch(8, N=N)
    m, veh = config.MPC, config.VEH
    S0, BWB = r2_setup(m["stds"], 0.08)
    a = _mk(8, store_qp_in=True); _start(a, x0, yref)
    a.r2_attach(S0, BWB, int(m["uncertainty_propagation_horizon"]), veh["delta_f_min"], veh["delta_f_max"], 1.0)
    with pytest.raises(Exception, match="R2NMPC"):
        a.options_set("nlp_solver_type", "SQP")
    w = snm.hammersley_normal(10, 3)
    c = CoupledSnmpcSolver(N=38, batch=1, Apce=snm.pce_matrix(w, snm.alpha_generation(3, 2)), uph=5)
    with pytest.raises(Exception, match="SNMPC"):
        c.options_set("nlp_solver_type", "SQP")
    with dev_library():
        f = _mk(8, qp_warm_start=False); _start(f, x0, yref)
        f.set_kernel("fused")
        f.options_set("nlp_solver_type", "SQP")
        with pytest.raises(Exception, match="fused"):
            f.solve()
    t = _mk(8, nlp_solver_type="SQP"); _start(t, x0, yref)
    with pytest.raises(Exception, match="SQP"):
        t.step(x0, yref)
    for bad in (("nlp_solver_max_iter", 0), ("nlp_solver_step_length", 1.5), ("nlp_solver_tol_stat", -1.0), ("nlp_solver_type", 2)):
        with pytest.raises(Exception):
            t.options_set(*bad)
    # default solver: SQP-RTI as before
    d = _mk(8); _start(d, x0, yref)
    assert d.solve() == 0
    assert (d.get_stats("sqp_iter") == 1).all()
    with pytest.raises(Exception, match="residuals"):
        d.get_residuals()
    e = _mk(8); _start(e, x0, yref)
    e.options_set("nlp_solver_type", "SQP"); e.options_set("nlp_solver_type", "SQP_RTI")
    assert e.solve() == 0
    np.testing.assert_array_equal(e.get_stats("res"), d.get_stats("res"))
    np.testing.assert_array_equal(e.get_iterate()[1], d.get_iterate()[1])
    # an SQP solve, then the same capsule back in SQP-RTI mode: sqp_iter is 1 again
    t.solve(); assert t.get_stats("sqp_iter").max() > 1
    t.options_set("nlp_solver_type", "SQP_RTI"); t.solve()
    assert (t.get_stats("sqp_iter") == 1).all()


def test_sqp_weight_sweep_batch(golden_dir):
    """the 26 weight sets x 2 tracks of kat0.npz as ONE SQP batch (per-instance weights): status 0 or 2, finite residuals; a
    step length below 1 runs as well"""
    from test_gpu_parity import _set_params
    d = np.load(os.path.join(golden_dir, "kat0.npz"))
    Nk, Bk = 38, 52
    for alpha in (1.0, 0.5):
        s = _mk(Bk, N=Nk, nlp_solver_type="SQP", nlp_solver_step_length=alpha)
        _set_params(s, d["params"])
        s.set_x0(d["x0"])
        yref = np.zeros((Bk, Nk + 1, 6)); yref[:, :, :4] = d["yref"]
        s.set_yref_all(yref); s.cold_start()
        s.solve()
        st, res = s.get_stats("status"), s.get_residuals()
        assert np.isin(st, (0, 2)).all(), st
        assert np.isfinite(res).all() and np.isfinite(s.get_cost()).all()
        assert (res[st == 0] < 1e-6).all()
