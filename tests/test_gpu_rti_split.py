"""
Split real-time iteration on the GPU: options_set("rti_phase", 1) -- preparation -- and ("rti_phase", 2) -- feedback. Every case is
held against a TWIN capsule that makes the one-call solve (rti_phase 0) of the same problem; the changed-x0 cases also against the
test-side statement of the update (tests/test_rti_split.py: rti_update / rti_update_dense) and the oracle.

Bounds. Same x0: bit for bit (the feedback kernel adds exact zeros). Changed x0: q | d after the feedback kernel against the one-call
solve's, both read through get_device "qp_vec": ten times the spread a CPU evaluation shows between two summation orders of the update
(forward / adjoint sweep against the dense G, A_k and B_k from get_from_qp_in), the largest over the batch, q and d each -- the precedent
is stat_rounding_spread of tests/test_sqp.py. Iterate, u0 and x1: 1e-6 scale-relative (the metric of tests/golden/replay_full_logs.py
that tests/test_gpu_parity.py gates with: per channel, relative to the channel's largest magnitude in the batch, yaw: pi), against the
twin and against the oracle solved at x0_new from the same iterate; an instance whose interior point method stops one iteration apart
from the oracle's is re-run on the oracle with the GPU's count imposed (force_iter), as test_batch_vs_oracle_config2_full_size does.

Measured (MI355X, test_changed_x0_against_twin_update_and_oracle):
    N x batch   CPU spread q / d        GPU split - twin q / d     |q| / |d|      iterate vs twin / vs oracle (scale-relative)
    40 x 26     2.8e-14 / 2.2e-16       2.8e-14 / 2.2e-16          52 / 1.6       1.8e-08 / 8.9e-09
    38 x 300    5.0e-14 / 6.7e-16       6.4e-14 / 8.9e-16          48 / 5.4       1.5e-08 / 6.5e-10
    48 x 26     5.0e-14 / 2.2e-16       7.1e-14 / 4.4e-16          107 / 1.9      8.9e-09 / 1.6e-08
    56 x 26     1.3e-13 / 2.2e-16       1.8e-13 / 4.4e-16          188 / 2.7      5.9e-10 / 2.0e-09
     8 x 26     5.6e-17 / 2.2e-16       4.9e-17 / 4.4e-16          0.086 / 2.6    3.1e-12 / 3.1e-12
The GPU difference is the rounding of q_prep + dq (an ulp of |q|) and of the two gradients' own sums, between 0.9 and 2.0 times the
CPU spread: inside the factor ten, not by much -- the spread is taken as the batch's largest because single instances show a spread
below an ulp of their q. The kernel's increment alone equals the CPU sweep to 4e-14 of its size. No instance stopped an iteration
apart from the twin or the oracle in these runs. With the shipped terminal weight (W_e = W[:4, :4]) the same cases gave 0.7 .. 2.4
times the spread and an iterate within 2.9e-07 of the twin's (N = 56). The 50-step sequence stays within 2.0e-10 of the one-call solve.
Mutations this file catches (each built into the library and run once): dt missing on the stage weights, W_e used at stage N - 1
(needs the terminal weight of its own above), g5 dropped from the gg row, delta not propagated through the psi column, x0_prep not
saved (all: increment against the CPU sweep, relative error of order one) and a stale preparation accepted (test_stale_preparation_is_refused).
"""
import functools

import numpy as np
import pytest

from test_rti_split import rti_update, rti_update_dense
from test_sqp import apply_case_solver, make_oracle, sqp_case

pytestmark = pytest.mark.gpu

DT = 0.08
WE_FACTORS = np.array([2.0, 0.5, 3.0, 1.5])          # terminal weight of the changed-x0 cases, relative to the stage weight


def _mk(N, B, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B, **kw)
    s.install_reference_ocp()
    return s


@functools.lru_cache(maxsize=None)
def _config2(N, B=4096):
    """config 2 (tum_control_amd.workloads), generated once per horizon: a smaller batch is its head (one sequential stream)"""
    from tum_control_amd.workloads import nominal_batch
    return nominal_batch(B, N=N)


def _inputs(N, B):
    x0, yref = _config2(N, 4096 if B > 300 else 300)
    return x0[:B].copy(), yref[:B].copy()


def _snap(s, rows=True):
    """everything a solve leaves behind: X, U, cost, status, qp_iter (+ qp_status, res) and, per stage, sl, su, lam"""
    X, U = s.get_iterate()
    r = dict(X=X, U=U, cost=np.atleast_1d(s.get_cost()), status=s.get_stats("status"), qp_iter=s.get_stats("qp_iter"),
             qp_status=s.get_stats("qp_status"), res=np.atleast_2d(s.get_stats("res")))
    if rows:
        for f in ("sl", "su", "lam"):
            r[f] = np.concatenate([np.atleast_2d(s.get(k, f)).reshape(s.batch, -1) for k in range(s.N + 1)], axis=1)
    return r


def _assert_same(a, b, what, keys=None):
    for k in keys or a:
        x, y = np.asarray(a[k]), np.asarray(b[k])          # (a failed instance carries NaN on both sides)
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (what, k, float(np.nanmax(np.abs(x.astype(float) - y.astype(float)))))


def _qp_vec(s):
    """q (B, 2N) and d (B, 2N) of the condensed QP in the pipeline's workspace"""
    import torch
    nvp = 80 if s.N <= 40 else (96 if s.N <= 48 else 112)
    t = torch.empty(s.batch, 2 * nvp, dtype=torch.float64, device="cuda:0")
    s.get_device("qp_vec", t.data_ptr())
    s.synchronize()
    v = t.cpu().numpy()
    return v[:, :2 * s.N].copy(), v[:, nvp:nvp + 2 * s.N].copy()


def _scales(u0, x1):
    sc = np.maximum(np.abs(np.concatenate([u0, x1], axis=1)).max(axis=0), 1e-300)
    sc[4] = np.pi
    return sc


def _dev(u0, x1, ru0, rx1, sc):
    """per-instance scale-relative error of (u0, x1) (tests/golden/replay_full_logs.py: solve_errors)"""
    d = np.concatenate([u0 - ru0, x1 - rx1], axis=1)
    d[:, 4] = (d[:, 4] + np.pi) % (2 * np.pi) - np.pi
    return (np.abs(d) / sc[None, :]).max(axis=1)


def _dev_iterate(X, U, RX, RU):
    """the whole iterate in the same metric: per state / input component, relative to its largest magnitude over batch and horizon"""
    sx = np.maximum(np.abs(RX).max(axis=(0, 1)), 1e-300); sx[2] = np.pi
    su = np.maximum(np.abs(RU).max(axis=(0, 1)), 1e-300)
    return max((np.abs(X - RX) / sx).max(), (np.abs(U - RU) / su).max())


# ---------------------------------------------------------------------------------------------------------------- 1: same x0
@pytest.mark.parametrize("B", [1, 26, 300, 4096])
@pytest.mark.parametrize("N", [8, 38, 40, 41, 48, 50, 56])
def test_same_x0_is_the_one_call_solve_bit_for_bit(N, B):
    """cold start, then a five-step warm sequence (qp_warm_start on): prepare + feedback == solve on everything a solve leaves"""
    x0, yref = _inputs(N, B)
    split, twin = _mk(N, B), _mk(N, B)
    for s in (split, twin):
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
    for step in range(6):
        st = twin.solve()
        assert split.prepare() == 0
        assert split.feedback() == st
        a, b = _snap(split, rows=(B <= 300 or step in (0, 5))), _snap(twin, rows=(B <= 300 or step in (0, 5)))
        _assert_same(a, b, (N, B, step))
        xn = b["X"][:, 1].copy()
        for s in (split, twin):
            s.set_x0(xn)


# ---------------------------------------------------------------------------------------------------------------- 2: side effects
@pytest.mark.parametrize("N,B", [(40, 26), (48, 300), (38, 1)])
def test_preparation_is_side_effect_free(N, B):
    x0, yref = _inputs(N, B)
    s = _mk(N, B)
    s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
    s.solve()
    before = _snap(s)
    s.set_x0(before["X"][:, 1].copy())
    assert s.prepare() == 0
    assert s.get_stats("time_tot") > 0.0
    _assert_same(before, _snap(s), (N, B))
    # ... and again on a capsule that has never solved: the cold-started iterate and the zero results stay
    f = _mk(N, B)
    f.set_x0(x0); f.set_yref_all(yref); f.cold_start()
    before = _snap(f)
    assert f.prepare() == 0 and f.get_stats("time_tot") > 0.0
    _assert_same(before, _snap(f), (N, B, "fresh"))


# ---------------------------------------------------------------------------------------------------------------- 3: changed x0
def _gh(X):
    from oracle.oracle import h_con
    return np.array([h_con(x)[1] for x in X])


@pytest.mark.parametrize("N,B", [(40, 26), (38, 300), (48, 26), (56, 26), (8, 26)])
def test_changed_x0_against_twin_update_and_oracle(N, B):
    """x0_new = X_1 of the first solve: what the plant model makes of one control step (metres, not 1e-9). Every instance."""
    x0, yref = _inputs(N, B)
    split, twin = _mk(N, B, qp_warm_start=False, store_qp_in=True), _mk(N, B, qp_warm_start=False, store_qp_in=True)
    # (the shipped OCP has W_e = W[:4, :4]: a terminal weight of its own, or the update could take one for the other unseen)
    o = make_oracle(N)
    o.W[N, :4] *= WE_FACTORS
    for s in (split, twin):
        s.cost_set(N, "W", np.diag(o.W[N, :4]))
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
        assert s.solve() == 0
    X0, U0 = twin.get_iterate()
    assert np.array_equal(split.get_iterate()[0], X0)
    x0n = X0[:, 1].copy()
    assert np.abs(x0n - x0)[:, :2].max(axis=1).min() > 1e-3
    assert split.prepare() == 0
    qp, dp = _qp_vec(split)                                  # the prepared QP, at the old x0
    split.set_x0(x0n); twin.set_x0(x0n)
    st = twin.solve()
    assert split.feedback() == st
    (qs, ds), (qt, dt_) = _qp_vec(split), _qp_vec(twin)
    # ---- q | d: the kernel's update against the CPU statement, and split against twin within ten times the CPU spread
    sq = sd = 0.0
    eq_ref = ed_ref = 0.0
    A = np.stack([twin.get_from_qp_in(k, "A").reshape(B, 8, 8) for k in range(N)], axis=1)
    Bm = np.stack([twin.get_from_qp_in(k, "B").reshape(B, 8, 2) for k in range(N)], axis=1)
    for b in range(B):
        gh = _gh(X0[b])
        d0 = x0n[b] - x0[b]
        q1, d1 = rti_update(A[b], Bm[b], gh, o.W, o.dt, d0)
        q2, d2 = rti_update_dense(A[b], Bm[b], gh, o.W, o.dt, d0)
        sq, sd = max(sq, np.abs(q1 - q2).max()), max(sd, np.abs(d1 - d2).max())
        # (the kernel's increment itself, as far as the sum q_prep + dq still shows it: an ulp of q_prep)
        eq_ref = max(eq_ref, np.abs((qs[b] - qp[b]) - q1).max() / max(np.abs(q1).max(), 1e-300))
        ed_ref = max(ed_ref, np.abs((ds[b] - dp[b]) - d1).max() / max(np.abs(d1).max(), 1e-300))
    eq, ed = np.abs(qs - qt).max(), np.abs(ds - dt_).max()
    print(f"\nN={N} B={B}: CPU spread q {sq:.3e} d {sd:.3e}; GPU split - twin q {eq:.3e} d {ed:.3e}; "
          f"increment vs CPU sweep (relative) q {eq_ref:.3e} d {ed_ref:.3e}; |q| {np.abs(qt).max():.3e} |d| {np.abs(dt_).max():.3e}")
    assert sq > 0.0
    assert eq_ref < 1e-9 and ed_ref < 1e-9                   # (a wrong weight, a dropped gradient entry or column is a relative error of order one)
    assert eq <= 10.0 * sq, (eq, sq)
    assert ed <= 10.0 * sd, (ed, sd)
    # ---- the solve: against the twin
    a, t = _snap(split, rows=False), _snap(twin, rows=False)
    assert np.array_equal(a["status"], t["status"])
    sc = _scales(t["U"][:, 0], t["X"][:, 1])
    dev = _dev(a["U"][:, 0], a["X"][:, 1], t["U"][:, 0], t["X"][:, 1], sc)
    dit = _dev_iterate(a["X"], a["U"], t["X"], t["U"])
    print(f"split vs twin: (u0, x1) {dev.max():.3e}, iterate {dit:.3e}, qp_iter differs on {(a['qp_iter'] != t['qp_iter']).sum()} instances")
    assert dev.max() < 1e-6 and dit < 1e-6
    # ---- ... and against the oracle solved at x0_new from the same iterate
    ou0, ox1, oX, oU, oit, ost = (np.zeros((B, 2)), np.zeros((B, 8)), np.zeros_like(X0), np.zeros_like(U0), np.zeros(B, int), np.zeros(B, int))
    for b in range(B):
        for force in (0, 1):
            o.qp_warm_start(False)
            o.set_iter_force(int(a["qp_iter"][b]) if force else 0)
            o.yref[:] = yref[b]; o.X[:] = X0[b]; o.U[:] = U0[b]; o.x0[:] = x0n[b]
            ost[b] = o.solve(); oit[b] = o.qp_iter
            ou0[b], ox1[b], oX[b], oU[b] = o.U[0], o.X[1], o.X, o.U
            if oit[b] == a["qp_iter"][b] or abs(oit[b] - int(a["qp_iter"][b])) > 1:
                break
        o.set_iter_force(0)
    assert np.array_equal(ost, a["status"])
    assert (oit == a["qp_iter"]).all()
    devo = _dev(a["U"][:, 0], a["X"][:, 1], ou0, ox1, sc)
    dito = _dev_iterate(a["X"], a["U"], oX, oU)
    print(f"split vs oracle: (u0, x1) {devo.max():.3e}, iterate {dito:.3e}")
    assert devo.max() < 1e-6 and dito < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 4: bounds, penalties
@pytest.mark.parametrize("N,B", [(40, 26), (48, 5)])
def test_bounds_and_penalties_changed_between_the_phases(N, B):
    """the bounds of the stages >= 1 and zl / zu / Zl / Zu set between preparation and feedback: the one-call solve with them, bit for bit"""
    x0, yref, cfg = sqp_case("ragged", B, N)
    split, twin = _mk(N, B), _mk(N, B)
    for s in (split, twin):
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
        s.solve()
    assert split.prepare() == 0
    apply_case_solver(split, cfg); apply_case_solver(twin, cfg)
    st = twin.solve()
    assert split.feedback() == st
    a, t = _snap(split), _snap(twin)
    _assert_same(a, t, (N, B))
    assert np.abs(a["sl"]).max() + np.abs(a["su"]).max() > 0.0          # the tight bounds are felt


# ---------------------------------------------------------------------------------------------------------------- 5: staleness
def _stale_ops():
    import torch

    def set_x(s, X, U):
        s.set(3, "x", X[:, 3] + 0.01)

    def set_u(s, X, U):
        s.set(2, "u", U[:, 2] + 0.01)

    def set_yref(s, X, U):
        s.set(5, "yref", np.array([1.0, 2.0, 0.1, 20.0, 0.0, 0.0]))

    def cost_w(s, X, U):
        s.cost_set(2, "W", np.diag([0.02, 0.03, 0.5, 0.01, 1e-3, 1e-1]))

    def put_x(s, X, U):
        t = torch.from_numpy(np.ascontiguousarray(X + 0.005)).to("cuda:0")
        s.put_device("X", t.data_ptr()); s.synchronize()

    return dict(set_x=set_x, set_u=set_u, set_yref=set_yref, cost_set_W=cost_w, cold_start=lambda s, X, U: s.cold_start(),
                reset=lambda s, X, U: s.reset(), put_device_X=put_x, sim_advance=lambda s, X, U: s.loop.advance())


@pytest.mark.parametrize("op", ["set_x", "set_u", "set_yref", "cost_set_W", "cold_start", "reset", "put_device_X", "sim_advance"])
def test_stale_preparation_is_refused(op):
    N, B = 40, 3
    x0, yref = _inputs(N, B)
    split, twin = _mk(N, B), _mk(N, B)
    for s in (split, twin):
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
        if op == "sim_advance":          # the plant of the device closed loop (it writes the iterate and x0): created in rti_phase 0, state as the capsule's
            from tum_control_amd.planner import load_track
            from tum_control_amd.solver import DeviceClosedLoop
            s.loop = DeviceClosedLoop(s, load_track("monteblanco"), N * DT)
            s.loop.set_state(x0[:, :7], x0, cold_start=True)
        assert s.solve() == 0
    X, U = twin.get_iterate()
    assert split.prepare() == 0
    fn = _stale_ops()[op]
    fn(split, X, U); fn(twin, X, U)
    before = _snap(split)
    with pytest.raises(Exception, match="preparation"):
        split.feedback()
    _assert_same(before, _snap(split), op)
    split.options_set("rti_phase", 0)
    assert split.solve() == twin.solve()
    _assert_same(_snap(split), _snap(twin), op)


# ---------------------------------------------------------------------------------------------------------------- 6: sequencing
def test_phase_sequencing():
    N, B = 40, 3
    x0, yref = _inputs(N, B)
    split, twin = _mk(N, B), _mk(N, B)
    for s in (split, twin):
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
    before = _snap(split)
    with pytest.raises(Exception, match="preparation"):
        split.feedback()                                     # no preparation at all
    _assert_same(before, _snap(split), "no preparation")
    assert split.prepare() == 0
    assert split.feedback() == twin.solve()
    _assert_same(_snap(split), _snap(twin), "first")
    with pytest.raises(Exception, match="preparation"):
        split.feedback()                                     # consumed
    with pytest.raises(Exception, match="preparation"):
        split.solve_async()                                  # (the asynchronous entry point as well)
    assert split.prepare() == 0
    split.options_set("rti_phase", 0)                        # a one-call solve discards the pending preparation ...
    assert split.solve() == twin.solve()
    _assert_same(_snap(split), _snap(twin), "phase 0 behind a preparation")
    with pytest.raises(Exception, match="preparation"):
        split.feedback()                                     # ... which is gone
    for bad in (3, -1, 0.5):
        with pytest.raises(Exception, match="rti_phase"):
            split._chk(split._L.tum_ocp_options_set(split._h, b"rti_phase", float(bad)), "options_set")
    with pytest.raises(Exception, match="rti_phase"):
        split._chk(split._L.tum_ocp_options_set(split._h, b"no_such_field", 1.0), "options_set")      # the list of fields names it


# ---------------------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals():
    import tum_control_amd.snmpc as snm
    from tum_control_amd import config
    from tum_control_amd.r2nmpc import r2_setup
    from tum_control_amd.solver import CoupledSnmpcSolver, DeviceClosedLoop, dev_library
    from tum_control_amd.planner import load_track
    m, veh = config.MPC, config.VEH
    N = 38

    def raw(s, v):
        s._chk(s._L.tum_ocp_options_set(s._h, b"rti_phase", float(v)), "options_set")

    # the coupled SNMPC OCP: the binding and the library
    w = snm.hammersley_normal(4, 3)
    c = CoupledSnmpcSolver(N=N, batch=1, Apce=snm.pce_matrix(w, snm.alpha_generation(3, 2)), uph=5)
    with pytest.raises(Exception, match="SNMPC"):
        c.options_set("rti_phase", 1)
    with pytest.raises(Exception, match="SNMPC"):
        raw(c, 2)
    c.options_set("rti_phase", 0)
    # R2 tightening attached: at options_set, and -- attached behind it -- at the solve
    S0, BWB = r2_setup(m["stds"], DT)
    uph = int(m["uncertainty_propagation_horizon"])
    r = _mk(N, 2, store_qp_in=True)
    r.r2_attach(S0, BWB, uph, veh["delta_f_min"], veh["delta_f_max"], 1.0)
    with pytest.raises(Exception, match="R2NMPC"):
        r.options_set("rti_phase", 1)
    r2 = _mk(N, 2, store_qp_in=True)
    r2.options_set("rti_phase", 1)
    r2.r2_attach(S0, BWB, uph, veh["delta_f_min"], veh["delta_f_max"], 1.0)
    with pytest.raises(Exception, match="R2NMPC"):
        r2.solve()
    # a full W
    f = _mk(N, 2)
    W = np.diag([0.02, 0.03, 0.5, 0.01, 1e-3, 1e-1]); W[0, 1] = W[1, 0] = 0.004
    f.cost_set(1, "W", W)
    with pytest.raises(Exception, match="full W"):
        f.options_set("rti_phase", 2)
    f2 = _mk(N, 2)
    f2.options_set("rti_phase", 1)
    f2.cost_set(1, "W", W)
    with pytest.raises(Exception, match="full W"):
        f2.solve()
    # SQP mode, in either order
    q = _mk(N, 2)
    q.options_set("nlp_solver_type", "SQP")
    with pytest.raises(Exception, match="SQP"):
        q.options_set("rti_phase", 1)
    q2 = _mk(N, 2)
    q2.options_set("rti_phase", 1)
    with pytest.raises(Exception, match="rti_phase"):
        q2.options_set("nlp_solver_type", "SQP")
    # the development kernels
    with dev_library():
        for k in ("fused", "pipeline4"):
            d = _mk(N, 2, qp_warm_start=False)
            d.set_kernel(k)
            with pytest.raises(Exception, match="development"):
                d.options_set("rti_phase", 1)
            d2 = _mk(N, 2, qp_warm_start=False)
            d2.options_set("rti_phase", 1)
            d2.set_kernel(k)
            with pytest.raises(Exception, match="development"):
                d2.solve()
    # debug dump, phase timers, the device closed loop
    g = _mk(N, 2)
    g.options_set("rti_phase", 1)
    with pytest.raises(Exception, match="debug dump"):
        g.debug_dump(0)
    with pytest.raises(Exception, match="phase timers"):
        g.profile_phases()
    with pytest.raises(Exception, match="rti_phase"):
        DeviceClosedLoop(g, load_track("monteblanco"), N * DT)
    g.options_set("rti_phase", 0)
    loop = DeviceClosedLoop(g, load_track("monteblanco"), N * DT)
    g.options_set("rti_phase", 2)
    with pytest.raises(Exception, match="rti_phase"):
        loop.run(1)


# ---------------------------------------------------------------------------------------------------------------- 8: step_async
@pytest.mark.parametrize("N,B", [(40, 26), (38, 1), (40, 2000)])
def test_feedback_step_is_the_solve_route(N, B):
    x0, yref = _inputs(N, B)
    a, b = _mk(N, B), _mk(N, B)
    for s in (a, b):
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
        s.solve()
    xn = a.get_iterate()[0][:, 1].copy()
    for s in (a, b):
        assert s.prepare() == 0
    with pytest.raises(Exception, match="preparation"):
        a.step(x0=xn)                                        # rti_phase 1: a preparation has no results
    a.options_set("rti_phase", 2)
    with pytest.raises(Exception, match="preparation"):
        a.step(x0=xn, yref=yref)                             # the reference enters in the preparation
    summ, X, U = a.step(x0=xn)
    summ, X, U = summ.copy(), X.copy(), U.copy()
    st = b.feedback(xn)
    r = _snap(b, rows=False)
    assert np.array_equal(X, r["X"]) and np.array_equal(U, r["U"])
    assert np.array_equal(summ[:, :2], r["U"][:, 0]) and np.array_equal(summ[:, 2], r["cost"])
    assert np.array_equal(summ[:, 3].astype(int), r["status"]) and np.array_equal(summ[:, 4].astype(int), r["qp_iter"])
    assert int(summ[:, 3].max()) == st
    _assert_same(_snap(a), _snap(b), (N, B))
    with pytest.raises(Exception, match="preparation"):
        a.step(x0=xn)                                        # consumed


# ---------------------------------------------------------------------------------------------------------------- 9: a controller's loop
def test_rti_sequence_of_26_vehicles_monteblanco():
    """50 control steps driven as a controller drives them: feedback(x0_t), read u0, set the next reference, prepare. The twin makes
    the one-call solve from the split capsule's iterate at every step. qp_warm_start off on both."""
    from tum_control_amd.planner import load_track, planner_emulator, yref_from_ref
    N, B, steps = 40, 26, 50
    tr = load_track("monteblanco")
    x0, yref = _inputs(N, B)
    split, twin = _mk(N, B, qp_warm_start=False), _mk(N, B, qp_warm_start=False)
    split.set_x0(x0); split.set_yref_all(yref); split.cold_start()
    assert split.prepare() == 0
    worst = 0.0
    for t in range(steps):
        Xi, Ui = split.get_iterate()
        twin.set_iterate(Xi, Ui); twin.set_x0(x0); twin.set_yref_all(yref)
        st = twin.solve()
        assert split.feedback(x0) == st
        a, r = _snap(split, rows=False), _snap(twin, rows=False)
        assert np.array_equal(a["status"], r["status"]), t
        sc = _scales(r["U"][:, 0], r["X"][:, 1])
        dev = max(_dev(a["U"][:, 0], a["X"][:, 1], r["U"][:, 0], r["X"][:, 1], sc).max(), _dev_iterate(a["X"], a["U"], r["X"], r["U"]))
        worst = max(worst, dev)
        assert dev < 1e-6, (t, dev)
        x0 = a["X"][:, 1].copy()                             # the plant model's next state
        for b in range(B):
            _, ref = planner_emulator(tr, x0[b, :2], N + 1, N * DT, True)
            yref[b] = yref_from_ref(ref, N)
        split.set_yref_all(yref)
        assert split.prepare() == 0                          # ... while the next measurement is awaited
    print(f"\n50-step sequence: worst scale-relative deviation from the one-call solve {worst:.3e}")
