"""
Full SQP solves (nlp_solver_type SQP): the CPU side.

`oracle_sqp` is the test-side reference of an SQP solve: OracleOcp.solve() looped with full steps, and the four NLP residuals the
library's residual kernel reports, evaluated the same way -- at the iterate, after its linearisation, with the previous QP's
multipliers. The stationarity residual comes from the condensed QP the oracle builds at the iterate (solve_debug), the equality and
inequality residuals straight from the model (oracle.rk4_sens, oracle.h_con), not from any QP. The GPU tests
(tests/test_gpu_sqp.py) hold the library against it.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DT, NSUB = 40, 0.08, 3


def make_oracle(N=N):
    from oracle.oracle import OracleOcp
    from tum_control_amd import config
    m = config.MPC
    o = OracleOcp(N, DT, NSUB)
    o.set_weights(m["q_lon"], m["q_yaw"], m["q_vel"], m["r_jerk"], m["r_steering_rate"], m["L1_pen"], m["L2_pen"], scale=0.01)
    return o


def _rows(o):
    """row values at the iterate, bounds, penalties (z, Z per side) in the QP's row order [bu_k (N) | (bx_s, h_s) s = 1..N]"""
    from oracle.oracle import h_con
    Nn, dt = o.N, o.dt
    val, lo, hi, zl, zu, Zl, Zu = (np.zeros(3 * Nn) for _ in range(7))
    for i in range(3 * Nn):
        if i < Nn:
            k, slot = i, 0
            val[i], lo[i], hi[i] = o.U[k, 1], o.lbu[k], o.ubu[k]
        else:
            k, slot = 1 + (i - Nn) // 2, 1 + (i - Nn) % 2
            if slot == 1:
                val[i], lo[i], hi[i] = o.X[k, 6], o.lbx[k], o.ubx[k]
            else:
                val[i], lo[i], hi[i] = h_con(o.X[k])[0], o.lh[k], o.uh[k]
        sc = dt if k < Nn else 1.0
        zl[i], zu[i], Zl[i], Zu[i] = (sc * a[k, slot] for a in (o.zl, o.zu, o.Zl, o.Zu))
    return val, lo, hi, zl, zu, Zl, Zu


def res_eq(o):
    """| x0 - X_0 |_inf and the shooting defects at the iterate"""
    from oracle.oracle import rk4_sens
    r = np.abs(o.x0 - o.X[0]).max()
    for k in range(o.N):
        xn = rk4_sens(o.X[k], o.U[k], o.dt, o.nsub)[0]
        r = max(r, np.abs(xn - o.X[k + 1]).max())
    return r


def residuals(o, lam, sl, su, q=None, C=None, rows=None):
    """[stat, eq, ineq, comp] of the iterate (lam, sl, su: the previous QP's multipliers and slacks; q, C: the condensed QP at the
    iterate -- without them stat is NaN; rows: _rows(o) if the caller has it)"""
    val, lo, hi, zl, zu, Zl, Zu = rows or _rows(o)
    m = 3 * o.N
    ll, lu = lam[:m], lam[m:]
    tl, tu = val - lo + sl, hi - val + su
    ml, mu = zl + Zl * sl - ll, zu + Zu * su - lu
    ineq = max(0.0, (-tl).max(), (-tu).max())
    comp = max(np.abs(ll * tl).max(), np.abs(lu * tu).max(), (np.maximum(ml, 0) * np.abs(sl)).max(), (np.maximum(mu, 0) * np.abs(su)).max())
    stat = float("nan")
    if q is not None:
        stat = max(np.abs(q - C.T @ (ll - lu)).max(), (-ml).max(), (-mu).max(), 0.0)
    return np.array([stat, res_eq(o), ineq, comp])


def oracle_sqp(o, max_iter, tol=1e-6, step_tol=None, with_stat=True, alpha=1.0):
    """SQP on one OracleOcp (iterate, x0, yref, weights already in place). Per iteration: linearise (and solve) the QP at
    the iterate, evaluate the residuals, stop if they are all below `tol` (the library's test) -- or, with `step_tol`, if the
    previous step was below it (the step criterion of the study in INTEGRATION.md) -- else take the step: the full one, or with
    `alpha` < 1 the damped one z <- z + alpha (z_qp - z) for X, U, slacks and multipliers (nlp_solver_step_length; the interior
    point method then starts cold in every QP: interpolated multipliers are no warm start).
    Returns (QPs taken, converged, residuals of the returned iterate); o.sl, o.su and o's "lam" are left at the values the
    residuals were evaluated with."""
    m = 3 * o.N
    lam, sl, su = np.zeros(2 * m), np.zeros(m), np.zeros(m)
    step = np.inf
    if alpha != 1.0:
        o.qp_warm_start(False)
    for it in range(max_iter + 1):
        X, U = o.X.copy(), o.U.copy()
        if with_stat:
            st, qp = o.solve_debug()
            # (solve_debug has taken the step already: the rows and defects are those of the iterate in front of it)
            Xn, Un = o.X.copy(), o.U.copy()
            o.X[:] = X; o.U[:] = U
            r = residuals(o, lam, sl, su, qp["q"], qp["C"])
            o.X[:] = Xn; o.U[:] = Un
        else:
            r = None
        if step_tol is not None:
            conv = step < step_tol
        else:          # (without the residuals: exactly max_iter QPs)
            conv = r is not None and bool((r < tol).all())
        if conv or it == max_iter:
            o.X[:] = X; o.U[:] = U
            o._view("lam")[:] = lam; o.sl[:] = sl; o.su[:] = su
            if r is None:
                r = residuals(o, lam, sl, su)
            return it, conv, r
        if not with_stat:
            st = o.solve()
        if st != 0:
            o.X[:] = X; o.U[:] = U
            return it + 1, False, residuals(o, lam, sl, su)
        if alpha != 1.0:
            for view, prev in ((o.X, X), (o.U, U), (o.sl, sl), (o.su, su), (o._view("lam"), lam)):
                view[:] = prev + alpha * (view - prev)
        lam, sl, su = o._view("lam").copy(), o.sl.copy(), o.su.copy()
        step = max(np.abs(o.X - X).max(), np.abs(o.U - U).max())
    raise AssertionError("unreachable")


def residuals_at(o, X, U, lam, sl, su, with_spread=False):
    """The four residuals at a given point -- an iterate, slacks and multipliers read back from the library -- and the scales the
    GPU tests bound the differences with: s_stat = |q|_inf + |C'(lam_l - lam_u)|_inf, s_comp = max |lam| max |t|, s_ineq = the
    largest |bound| or |row value|, s_eq = |X|_inf, and on request stat_spread (stat_rounding_spread). q and C are those of the condensed QP the oracle builds at (X, U): solve_debug
    linearises there before it solves, and the iterate is written back behind it."""
    X, U = np.array(X, dtype=float), np.array(U, dtype=float)
    o.X[:] = X; o.U[:] = U
    _, qp = o.solve_debug()
    q, C = qp["q"].copy(), qp["C"].copy()
    spread = stat_rounding_spread(o, X) if with_spread else None          # (or later: o keeps the linearisation until its next solve)
    o.X[:] = X; o.U[:] = U
    rows = _rows(o)
    r = residuals(o, lam, sl, su, q, C, rows)
    val, lo, hi = rows[:3]
    m = 3 * o.N
    w = lam[:m] - lam[m:]
    t = np.concatenate([val - lo + sl, hi - val + su])
    scales = dict(stat=np.abs(q).max() + np.abs(C.T @ w).max(), stat_spread=spread, eq=max(1.0, np.abs(X).max()),
                  ineq=max(1.0, np.abs(lo).max(), np.abs(hi).max(), np.abs(val).max()), comp=max(1.0, np.abs(lam).max() * np.abs(t).max()))
    return r, scales


def stat_defect_sensitivity(o):
    """M = d (condensed gradient q) / d (defects b_0 .. b_{N-1}), (2N, N, 8), from the A_k, B_k of the oracle's last linearisation:
    q = sum_s G_s' Q_s (r_s + g_s) + ..., g_s = sum_{k < s} Phi(s, k + 1) b_k, G_s = [Phi(s, j + 1) B_j]_j, Q_s the dt-scaled state
    weights. (C, the rows and the multipliers do not depend on the defects.)"""
    Nn, dt = o.N, o.dt
    A, B = o.A, o.B
    Phi = [[None] * (Nn + 1) for _ in range(Nn + 1)]          # Phi[s][k], s >= k: A_{s-1} ... A_k
    for k in range(Nn + 1):
        Phi[k][k] = np.eye(8)
        for s_ in range(k, Nn):
            Phi[s_ + 1][k] = A[s_] @ Phi[s_][k]
    M = np.zeros((2 * Nn, Nn, 8))
    for s_ in range(1, Nn + 1):
        Q = np.zeros((8, 8))
        Q[:4, :4] = (dt if s_ < Nn else 1.0) * (o.Wf[s_, :4, :4] if o.full_w[0] != 0.0 else np.diag(o.W[s_, :4]))
        G = np.zeros((8, 2 * Nn))
        for j in range(s_):
            G[:, 2 * j:2 * j + 2] = Phi[s_][j + 1] @ B[j]
        GQ = G.T @ Q
        for k in range(s_):
            M[:, k] += GQ @ Phi[s_][k + 1]
            if o.full_w[0] != 0.0 and s_ < Nn:          # (a full W couples the inputs of stage s to its state residuals)
                M[2 * s_:2 * s_ + 2, k] += dt * o.Wf[s_, 4:6, :4] @ Phi[s_][k + 1][:4]
    return M


def stat_rounding_spread(o, X):
    """How far the stationarity vector q - C'w of the iterate X moves when the integrator's results f(x_k, u_k) move by one ulp each:
    sum_k |M_k| ulp(|X_{k+1}|), largest component. No FP64 evaluation determines f(x_k, u_k) -- and with it the defect
    b_k = f(x_k, u_k) - x_{k+1}, a difference of two numbers of the size of the state -- more closely than that, so two honest
    evaluations of the same condensed gradient (another order of the sums in the integrator) differ by a good part of this figure:
    at a cold start all b_k carry the SAME rounding error, which g_s = sum_k Phi b_k adds up over the horizon. (Moving the iterate
    itself by an ulp shows a hundredth of it: x_{k+1} enters b_k and b_{k+1} with opposite signs, and the sum telescopes.)
    Needs o's linearisation at X (solve_debug)."""
    M = stat_defect_sensitivity(o)
    return float((np.abs(M) * np.spacing(np.abs(np.asarray(X)[1:]))[None]).sum(axis=(1, 2)).max())


def wrap_yaw(a):
    """the oracle's (and acados' model's) yaw output: into [0, 2 pi)"""
    y = np.fmod(a, 2.0 * np.pi)
    return np.where(y < 0.0, y + 2.0 * np.pi, y)


def cost_at(o, X, U, sl, su):
    """oracle/nmpc_oracle.c::eval_cost in numpy, at a given iterate and slacks (weights, references, penalties: o's): stage terms
    scaled by dt, the terminal one unscaled; diagonal W or, with o.full_w set, the full one; z s + Z s^2 / 2 per row side"""
    Nn, dt = o.N, o.dt
    X, U = np.asarray(X, dtype=float), np.asarray(U, dtype=float)
    c = 0.0
    for k in range(Nn + 1):
        ny = 6 if k < Nn else 4
        y = np.zeros(6)
        y[:4] = X[k, :4]; y[2] = wrap_yaw(X[k, 2])
        if k < Nn:
            y[4:] = U[k]
        r = (y - o.yref[k])[:ny]
        Wk = o.Wf[k, :ny, :ny] if o.full_w[0] != 0.0 else np.diag(o.W[k, :ny])
        c += (dt if k < Nn else 1.0) * 0.5 * (r @ Wk @ r)
    zl, zu, Zl, Zu = _rows(o)[3:]
    return c + (zl * sl + 0.5 * Zl * sl * sl).sum() + (zu * su + 0.5 * Zu * su * su).sum()


# ------------------------------------------------------------------------------------------------- the inputs of the GPU tests
def _pen_factors():
    """36 distinct factors in [0.5, 1.9] on the shipped penalties: [field zl, zu, Zl, Zu][class 0 / 1..N-1 / N][slot bu, bx, h]"""
    return (0.5 + 1.4 * ((7 * np.arange(36)) % 36) / 35.0).reshape(4, 3, 3)


def sqp_case(kind, B, N):
    """x0, yref and the per-stage bounds / penalty factors of the three inputs the SQP tests run:
    'nominal' -- config 2, the shipped bounds and penalties: a batch mixes instances that converge and ones that cycle;
    'tight'   -- accelerating, gg bound 0.05 and steering angle within +-0.002 on the stages 1..N (test_tight_bounds_activate_slacks):
                 the row sides are violated beyond their slacks after the first QPs (ineq > 0);
    'ragged'  -- tight, with bounds that taper over the horizon and differ per side (what the R2 back-off produces) and
                 penalties that differ in zl, zu, Zl, Zu, in each penalty class and in each row type.
    Returns x0, yref, dict(lbx, ubx, uh: (N + 1) or None, pen: (4, 3, 3) factors or None)."""
    from tum_control_amd.workloads import nominal_batch
    if kind == "nominal":
        x0, yref = nominal_batch(B, N=N)
        return x0, yref, dict(lbx=None, ubx=None, uh=None, pen=None)
    x0, yref = nominal_batch(B, N=N, seed=11)
    x0[:, 7] = 1.5
    k = np.arange(N + 1) / N
    if kind == "tight":
        return x0, yref, dict(lbx=np.full(N + 1, -0.002), ubx=np.full(N + 1, 0.002), uh=np.full(N + 1, 0.05), pen=None)
    assert kind == "ragged", kind
    return x0, yref, dict(lbx=-0.003 - 0.005 * k, ubx=0.002 + 0.01 * k, uh=0.05 + 0.1 * k, pen=_pen_factors())


def _classes(N):
    """(penalty class, its stages, its slots)"""
    return [(0, [0], [0])] + ([(1, list(range(1, N)), [0, 1, 2])] if N > 1 else []) + [(2, [N], [1, 2])]


def apply_case_oracle(o, cfg):
    """the bounds and penalties of sqp_case on an OracleOcp that has the shipped ones (make_oracle)"""
    from tum_control_amd import config
    for name in ("lbx", "ubx", "uh"):
        if cfg[name] is not None:
            getattr(o, name)[1:] = cfg[name][1:]
    if cfg["pen"] is not None:
        base = (config.MPC["L1_pen"], config.MPC["L1_pen"], config.MPC["L2_pen"], config.MPC["L2_pen"])
        for f, arr in enumerate((o.zl, o.zu, o.Zl, o.Zu)):
            for cls, stages, slots in _classes(o.N):
                for slot in slots:
                    arr[stages, slot] = base[f] * cfg["pen"][f, cls, slot]


def apply_case_solver(s, cfg):
    """the same on a BatchedOcpSolver behind install_reference_ocp()"""
    N, mpc = s.N, s.cfg["mpc"]
    for name in ("lbx", "ubx", "uh"):
        if cfg[name] is not None:
            for k in range(1, N + 1):
                s.constraints_set(k, name, np.array([cfg[name][k]]))
    if cfg["pen"] is not None:
        base = (mpc["L1_pen"], mpc["L1_pen"], mpc["L2_pen"], mpc["L2_pen"])
        for f, name in enumerate(("zl", "zu", "Zl", "Zu")):
            for cls, stages, slots in _classes(N):
                s.cost_set(stages[0], name, base[f] * cfg["pen"][f, cls, slots])


# ---------------------------------------------------------------------------------------------------------------------------- tests
def test_cabi_exports_options_set():
    """libtumnmpc.so exports tum_ocp_options_set and the binding declares it"""
    import __graft_entry__ as g
    g.build()
    from tum_control_amd import solver
    L = solver.load_library()
    assert hasattr(L, "tum_ocp_options_set")
    assert "tum_ocp_options_set" in solver.C_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "tum_nmpc.h")).read()
    assert "int tum_ocp_options_set(tum_ocp *c, const char *field, double value);" in hdr


def test_sqp_kernels_in_resource_table():
    """the three SQP kernels are in the shipped library, without scratch or spills, and none contains the name of another kernel"""
    import shutil
    import subprocess
    import __graft_entry__ as g
    if not (os.path.exists(g.HIPCC) or shutil.which("hipcc")) and not os.path.exists(g.LIB + ".resources"):
        pytest.skip("no hipcc and no resource table of a previous build on this host")
    g.build()
    rows = {}
    for line in open(g.LIB + ".resources"):
        parts = line.split()
        rows[parts[0]] = [int(x) for x in parts[1:]]
    filt = shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    names = list(rows)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = {d.strip(): rows[n] for n, d in zip(names, dem)}
    kernel_names = {n.split("(")[0].split("<")[0].split("::")[-1] for n in rows}
    for new in ("nlp_residual_kernel", "sqp_snapshot_kernel", "sqp_commit_kernel"):
        assert new in kernel_names, new
        assert not any(k != new and k in new for k in kernel_names), new
    hits = {n: v for n, v in rows.items() if any(k in n for k in ("nlp_residual_kernel", "sqp_snapshot_kernel", "sqp_commit_kernel"))}
    assert len(hits) == 5, sorted(hits)          # the residual kernel for five, six and seven tiles
    for name, (vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ) in hits.items():
        assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, (name, scratch, vgpr_spill, sgpr_spill)


def test_python_options_validation_without_gpu():
    """the binding maps the acados names of nlp_solver_type and rejects the others before the library sees them"""
    from tum_control_amd import solver
    assert solver._NLP_TYPES == {"SQP_RTI": 0, "SQP": 1}
    assert solver._NLP_DEFAULTS["nlp_solver_max_iter"] == 100
    assert all(solver._NLP_DEFAULTS[f"nlp_solver_tol_{k}"] == 1e-6 for k in ("stat", "eq", "ineq", "comp"))
    assert solver._NLP_DEFAULTS["nlp_solver_step_length"] == 1.0


def test_reference_sqp_convergence_split_config2():
    """The study the SQP mode's documentation quotes ("SQP mode"): config 2's first 256 instances, cold-started,
    full-step SQP on the oracle until the largest step is below 1e-6: 93 converge within 40 QPs (median 20), the rest converge
    slowly or cycle -- instance 0 repeats a step of 0.14. The residuals of this reference are consistent: where the step has
    converged, the equality and inequality residuals at the iterate are at the step's level."""
    from tum_control_amd.workloads import nominal_batch
    x0, yref = nominal_batch(256, N=N)
    o = make_oracle()
    its, conv, req = [], [], []
    for b in range(256):
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        it, c, r = oracle_sqp(o, 40, step_tol=1e-6, with_stat=False)
        its.append(it); conv.append(c); req.append(r)
    its, conv, req = np.array(its), np.array(conv), np.array(req)
    assert conv.sum() == 93, conv.sum()
    assert np.median(its[conv]) == 20, np.median(its[conv])
    assert not conv[0]
    # converged by the step: the iterate is feasible for the dynamics and the soft rows to well below the NLP tolerance
    assert req[conv, 1].max() < 1e-6 and req[conv, 2].max() < 1e-6


@pytest.mark.parametrize("Nh", [17, 40, 50])
def test_cost_at_is_the_oracles_cost(Nh):
    """cost_at (numpy) against the C oracle's eval_cost behind a solve: tight and ragged inputs (slacks in use, penalties that differ
    per class and side), diagonal and full W. Both sum the same at most 57 * 6 + 56 * 12 terms in FP64: 1e-13 relative (measured 1.2e-14)."""
    from test_full_w import _spd_weights
    worst = 0.0
    for kind, full in (("nominal", False), ("tight", False), ("ragged", False), ("ragged", True)):
        x0, yref, cfg = sqp_case(kind, 3, Nh)
        used = 0.0
        for b in range(3):
            o = make_oracle(Nh); apply_case_oracle(o, cfg)
            if full:
                o.set_full_W(_spd_weights(np.random.default_rng(Nh + b), o.W.copy()))
            o.cold_start(x0[b]); o.yref[:] = yref[b]
            for _ in range(2):
                assert o.solve() == 0
                c = cost_at(o, o.X, o.U, o.sl, o.su)
                worst = max(worst, abs(c - o.cost) / abs(o.cost))
                assert abs(c - o.cost) <= 1e-13 * abs(o.cost), (kind, full, b, c, o.cost)
                used = max(used, o.sl.max(), o.su.max())
        assert kind == "nominal" or used > 1e-3, used          # (the slack terms are part of what was compared)
    print(f"N = {Nh}: cost_at against the oracle, worst relative difference {worst:.2e}")


@pytest.mark.parametrize("Nh", [17, 40, 50])
def test_oracle_sqp_damped_step(Nh):
    """oracle_sqp(alpha = 0.5): after one QP every variable is half way between the start and the full step's, the second QP starts from
    there (not from the full step), and residuals_at reproduces the residuals oracle_sqp reports at the point it returns"""
    x0, yref, cfg = sqp_case("ragged", 2, Nh)
    m = 3 * Nh
    for b in range(2):
        def fresh():
            o = make_oracle(Nh); apply_case_oracle(o, cfg)
            o.cold_start(x0[b]); o.yref[:] = yref[b]; o.qp_warm_start(False)
            return o
        f = fresh(); assert oracle_sqp(f, 1, tol=0.0)[0] == 1
        h = fresh(); n, conv, r1 = oracle_sqp(h, 1, tol=0.0, alpha=0.5)
        assert n == 1 and not conv
        X0 = np.broadcast_to(x0[b], (Nh + 1, 8))
        for got, full, prev in ((h.X, f.X, X0), (h.U, f.U, 0.0), (h.sl, f.sl, 0.0), (h.su, f.su, 0.0), (h._view("lam"), f._view("lam"), 0.0)):
            np.testing.assert_array_equal(got, prev + 0.5 * (full - prev))
        assert np.abs(f._view("lam")).max() > 1e-3
        r, sc = residuals_at(h, h.X.copy(), h.U.copy(), h._view("lam").copy(), h.sl.copy(), h.su.copy())
        np.testing.assert_allclose(r, r1, rtol=0, atol=1e-12 * max(sc["stat"], sc["comp"], 1.0))
        assert np.isfinite(r).all() and (r[[0, 1, 3]] > 1e-6).all()
        # three damped QPs differ from three full ones and stay finite
        g = fresh(); n, conv, r3 = oracle_sqp(g, 3, tol=0.0, alpha=0.5)
        f3 = fresh(); oracle_sqp(f3, 3, tol=0.0)
        assert n == 3 and np.isfinite(r3).all() and np.abs(g.U - f3.U).max() > 1e-6


def _h_grad_fd_error(X):
    """largest error of a central difference quotient of h_con against its analytic gradient over the stages of X, relative to |grad|"""
    from oracle.oracle import h_con
    worst = 0.0
    for x in X:
        gh = h_con(x)[1]
        fd = np.zeros(8)
        for i in range(8):
            e = np.zeros(8); e[i] = 1e-6 * max(1.0, abs(x[i]))
            fd[i] = (h_con(x + e)[0] - h_con(x - e)[0]) / (2 * e[i])
        worst = max(worst, np.abs(fd - gh).max() / max(1.0, np.abs(gh).max()))
    return worst


def _adjoint_stat(o, X, U, w, A, Bm, b, full=False):
    """q - C'w without condensing: the linearised residuals r_k + g_k (g_0 = x0 - X_0, g_{k+1} = A_k g_k + b_k), then an adjoint sweep
    p_N = grad_x L_N, p_k = A_k' p_{k+1} + grad_x L_k, dL/du_k = B_k' p_{k+1} + grad_u L_k of L = cost - w' rows"""
    from oracle.oracle import h_con
    Nh = o.N
    g = np.zeros((Nh + 1, 8)); g[0] = o.x0 - X[0]
    for k in range(Nh):
        g[k + 1] = A[k] @ g[k] + b[k]
    gx, gu = np.zeros((Nh + 1, 8)), np.zeros((Nh, 2))
    for k in range(Nh + 1):
        ny = 6 if k < Nh else 4
        sc = o.dt if k < Nh else 1.0
        y = np.zeros(6); y[:4] = X[k, :4]; y[2] = wrap_yaw(X[k, 2])
        if k < Nh:
            y[4:] = U[k]
        r = y - o.yref[k]; r[:4] += g[k, :4]
        Wk = o.Wf[k, :ny, :ny] if full else np.diag(o.W[k, :ny])
        gr = sc * Wk @ r[:ny]
        gx[k, :4] += gr[:4]
        if k < Nh:
            gu[k] += gr[4:]
            gu[k, 1] -= w[k]
        if k >= 1:
            gx[k, 6] -= w[Nh + 2 * (k - 1)]
            gx[k] -= w[Nh + 2 * (k - 1) + 1] * h_con(X[k])[1]
    grad = np.zeros((Nh, 2))
    p = gx[Nh].copy()
    for k in range(Nh - 1, -1, -1):
        grad[k] = Bm[k].T @ p + gu[k]
        p = A[k].T @ p + gx[k]
    return grad.reshape(-1)


@pytest.mark.parametrize("Nh,full", [(5, False), (17, False), (40, False), (40, True), (50, False)])
def test_stat_definition_against_an_adjoint_sweep(Nh, full):
    """What `residuals` calls stationarity, q - C'w of the condensed QP, is the reduced gradient of the Lagrangian
    L(U) = cost(X(U), U) - w' rows(X(U), U): at an iterate without defects (X rolled out from U) a plain adjoint sweep over the A_k, B_k of
    rk4_sens (_adjoint_stat) must give the same vector for an arbitrary w, with no condensing recursion and no QP involved. Cost gradient
    W r; rows u[1], x[6], h_con with h_con's analytic gradient (held here to a difference quotient to 1e-6, which is the quotient's own
    error): bound 1e-9 * s_stat."""
    from oracle.oracle import rk4_sens
    from test_full_w import _spd_weights
    x0, yref, cfg = sqp_case("ragged", 2, Nh)
    rng = np.random.default_rng(100 + Nh)
    for b in range(2):
        o = make_oracle(Nh); apply_case_oracle(o, cfg)
        if full:
            o.set_full_W(_spd_weights(np.random.default_rng(Nh + b), o.W.copy()))
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        U = np.stack([0.5 * rng.normal(size=Nh), 0.05 * rng.normal(size=Nh)], axis=1)
        X = np.zeros((Nh + 1, 8)); X[0] = x0[b]
        A, Bm = np.zeros((Nh, 8, 8)), np.zeros((Nh, 8, 2))
        for k in range(Nh):
            X[k + 1], A[k], Bm[k] = rk4_sens(X[k], U[k], o.dt, o.nsub)
        o.X[:] = X; o.U[:] = U
        _, qp = o.solve_debug()
        q, C = qp["q"].copy(), qp["C"].copy()
        w = rng.normal(size=3 * Nh) * np.where(rng.random(3 * Nh) < 0.3, 0.0, 1.0)          # (some rows inactive)
        assert _h_grad_fd_error(X[1:]) < 1e-6
        grad = _adjoint_stat(o, X, U, w, A, Bm, np.zeros((Nh, 8)), full)
        s_stat = np.abs(q).max() + np.abs(C.T @ w).max()
        err = np.abs((q - C.T @ w) - grad).max()
        print(f"N = {Nh}, full W {full}, instance {b}: |condensed - adjoint| = {err:.2e}, s_stat = {s_stat:.2e}")
        assert err <= 1e-9 * s_stat, (err, s_stat)


@pytest.mark.parametrize("Nh,full", [(17, False), (40, True), (56, False)])
def test_stat_sensitivity_to_the_defects(Nh, full):
    """stat_defect_sensitivity / stat_rounding_spread, which the GPU tests bound the stationarity's rounding with: at a cold start (large,
    equal defects in every stage) the adjoint form with the oracle's own A_k, B_k, b_k reproduces the condensed q - C'w (1e-9 s_stat),
    and moving the defects by d moves it by M d (d: 1e4 ulp of the state with random signs; 1e-6 of the move). The spread itself --
    one ulp in every defect, worst signs -- is far below the stationarity tolerance, and above what a 1-ulp move of the ITERATE shows."""
    from test_full_w import _spd_weights
    x0, yref, cfg = sqp_case("ragged", 2, Nh)
    rng = np.random.default_rng(7 + Nh)
    for b in range(2):
        o = make_oracle(Nh); apply_case_oracle(o, cfg)
        if full:
            o.set_full_W(_spd_weights(np.random.default_rng(Nh + b), o.W.copy()))
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        X, U = o.X.copy(), o.U.copy()
        _, qp = o.solve_debug()
        A, Bm, bd = o.A.copy(), o.B.copy(), o.b.copy()
        w = np.abs(rng.normal(size=3 * Nh))
        v = qp["q"] - qp["C"].T @ w
        s_stat = np.abs(qp["q"]).max() + np.abs(qp["C"].T @ w).max()
        v0 = _adjoint_stat(o, X, U, w, A, Bm, bd, full)
        assert np.abs(v - v0).max() <= 1e-9 * s_stat, (np.abs(v - v0).max(), s_stat)
        M = stat_defect_sensitivity(o)
        d = 1e4 * np.spacing(np.abs(X[1:])) * rng.choice([-1.0, 1.0], size=(Nh, 8))
        move = _adjoint_stat(o, X, U, w, A, Bm, bd + d, full) - v0
        want = np.einsum("jki,ki->j", M, d)
        assert np.abs(move - want).max() <= 1e-6 * np.abs(want).max() + 1e-13 * s_stat, (np.abs(move - want).max(), np.abs(want).max())
        spread = stat_rounding_spread(o, X)
        print(f"N = {Nh}, full W {full}, instance {b}: stat {np.abs(v).max():.2e}, one ulp in every defect moves it by at most {spread:.2e}")
        assert 0.0 < spread < 1e-9
