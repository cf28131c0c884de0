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


def residuals(o, lam, sl, su, q=None, C=None):
    """[stat, eq, ineq, comp] of the iterate (lam, sl, su: the previous QP's multipliers and slacks; q, C: the condensed QP at the
    iterate -- without them stat is NaN)"""
    val, lo, hi, zl, zu, Zl, Zu = _rows(o)
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


def oracle_sqp(o, max_iter, tol=1e-6, step_tol=None, with_stat=True):
    """Full-step SQP on one OracleOcp (iterate, x0, yref, weights already in place). Per iteration: linearise (and solve) the QP at
    the iterate, evaluate the residuals, stop if they are all below `tol` (the library's test) -- or, with `step_tol`, if the
    previous step was below it (the step criterion of the study in INTEGRATION.md) -- else take the step.
    Returns (QPs taken, converged, residuals of the returned iterate)."""
    m = 3 * o.N
    lam, sl, su = np.zeros(2 * m), np.zeros(m), np.zeros(m)
    step = np.inf
    for it in range(max_iter + 1):
        X, U = o.X.copy(), o.U.copy()
        if with_stat:
            st, qp = o.solve_debug()
            r = residuals(o, lam, sl, su, qp["q"], qp["C"])
        else:
            r = None
        if step_tol is not None:
            conv = step < step_tol
        else:          # (without the residuals: exactly max_iter QPs)
            conv = r is not None and bool((r < tol).all())
        if conv or it == max_iter:
            o.X[:] = X; o.U[:] = U
            if r is None:
                r = residuals(o, lam, sl, su)
            return it, conv, r
        if not with_stat:
            st = o.solve()
        if st != 0:
            o.X[:] = X; o.U[:] = U
            return it + 1, False, residuals(o, lam, sl, su)
        lam, sl, su = o._view("lam").copy(), o.sl.copy(), o.su.copy()
        step = max(np.abs(o.X - X).max(), np.abs(o.U - U).max())
    raise AssertionError("unreachable")


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
