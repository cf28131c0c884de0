"""
Full SQP solves on the GPU (-m gpu) against the reference of tests/test_sqp.py, at every tile count: the four residuals at the
library's own iterate, slacks and multipliers (get(stage, "lam")), the termination test, the bit-identical restores of finished and
failed instances, damped steps with the residual kernel's own cost, and neighbouring tile counts at one horizon.

Bounds. A reported residual is compared with residuals_at() at the point read back from the library, so both sides evaluate the
same formula on the same numbers: eq 1e-12 max(1, |X|_inf) (the bound of tests/test_gpu_sqp.py), ineq 1e-12 max(1, largest |bound|,
|row value|), comp 1e-12 max(1, max |lam| max |t|) -- a few FP64 sums and products, three orders above their rounding --, stat
1e-11 (|q|_inf + |C'w|_inf) = 1e-11 s_stat, the bound tests/test_snmpc.py holds the condensed gradient to. That the reference's
stationarity is the reduced gradient of the Lagrangian is held on the CPU (tests/test_sqp.py::test_stat_definition_against_an_adjoint_sweep).

Where 1e-11 s_stat lies below FP64 rounding. Measured on the MI355X with that bound alone: tight and ragged inputs pass at every horizon
(largest difference / bound 6e-4 at N = 5, 0.3 at N = 38, 0.9 at N = 56), but the nominal input and pass 0 do not: near convergence q
cancels and s_stat is the residual itself (N = 1: reported 4.7130361186e-09, reference 4.7130361194e-09, bound 4.7e-20), and at a
cold start of a long horizon the difference is 1.5e-11 |q| (N = 56: 3.96e-11 at stat 2.73; N = 40: 7.6e-12 at 0.44). The cause is the
defect b_k = f(x_k, u_k) - x_{k+1}: no FP64 evaluation fixes f, a number of the size of the state, to better than an ulp of it, the
condensing adds the defects up over the horizon, and two evaluations of the same formulas differ accordingly -- the oracle compiled
with its sums regrouped differs from the shipped oracle by 3.95e-11, 7.6e-12 and 8.0e-19 in the three cases above, the library's
figures to two digits. stat_rounding_spread (tests/test_sqp.py, held there against an adjoint sweep) is the move of q - C'w for one
ulp in every f(x_k, u_k), worst signs: 3.6e-11, 6.2e-12 and 4.7e-18 in those cases. Where the difference exceeds 1e-11 s_stat the bound is
ten times that spread, of the instance compared: a few 1e-10 at most on the inputs here, three orders below the default tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_sqp import apply_case_oracle, apply_case_solver, cost_at, make_oracle, oracle_sqp, residuals_at, sqp_case, stat_rounding_spread

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLS = ("nlp_solver_tol_stat", "nlp_solver_tol_eq", "nlp_solver_tol_ineq", "nlp_solver_tol_comp")
ZERO = {k: 0.0 for k in TOLS}
NAMES = ("stat", "eq", "ineq", "comp")
FIELDS = ("X", "U", "sl", "su", "lam", "cost", "residuals", "sqp_iter", "qp_iter", "qp_status", "res", "status")


def _mk(B, N, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=N, dt=0.08, nsub=3, batch=B, nlp_solver_type="SQP", **kw)
    s.install_reference_ocp()
    return s


def _load(s, x0, yref, cfg):
    s.set_x0(x0); s.set_yref_all(yref); apply_case_solver(s, cfg); s.cold_start()


def _set_tols(s, *values):
    for k, v in zip(TOLS, values if len(values) == 4 else values * 4):
        s.options_set(k, v)


def _duals(s):
    """multipliers (B, 6N: lower | upper), lower and upper slacks (B, 3N) in the QP's row order [bu_k (N) | (bx_s, h_s) s = 1..N]"""
    B, N = s.batch, s.N
    lam, sl, su = np.zeros((B, 6 * N)), np.zeros((B, 3 * N)), np.zeros((B, 3 * N))
    for k in range(N + 1):
        cols = ([k] if k < N else []) + ([N + 2 * (k - 1), N + 2 * (k - 1) + 1] if k >= 1 else [])
        n = len(cols)
        sl[:, cols] = np.reshape(s.get(k, "sl"), (B, n)); su[:, cols] = np.reshape(s.get(k, "su"), (B, n))
        l = np.reshape(s.get(k, "lam"), (B, 2 * n))
        lam[:, cols] = l[:, :n]; lam[:, [3 * N + c for c in cols]] = l[:, n:]
    return lam, sl, su


def _read(s):
    B = s.batch
    X, U = s.get_iterate()
    lam, sl, su = _duals(s)
    out = dict(X=X, U=U, lam=lam, sl=sl, su=su, cost=np.reshape(s.get_cost(), (B,)), residuals=np.reshape(s.get_residuals(), (B, 4)),
               res=np.reshape(s.get_stats("res"), (B, 3)))
    for k in ("sqp_iter", "qp_iter", "qp_status", "status"):
        out[k] = np.reshape(s.get_stats(k), (B,))
    return out


def _hold_residuals(out, o, x0, yref, idx, what, worst):
    """reported residuals of the instances idx against residuals_at at the point read back; returns the reference's (len(idx), 4).
    `worst` collects the largest difference / bound per residual."""
    ref = np.zeros((len(idx), 4))
    for j, b in enumerate(idx):
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        r, sc = residuals_at(o, out["X"][b], out["U"][b], out["lam"][b], out["sl"][b], out["su"][b])
        ref[j] = r
        got = out["residuals"][b]
        assert np.isfinite(r).all() == np.isfinite(got).all(), (what, b, got, r)
        if not np.isfinite(r).all():
            continue
        for i, name in enumerate(NAMES):
            bound = (1e-11 if name == "stat" else 1e-12) * sc[name]
            if name == "stat" and abs(got[i] - r[i]) > bound:          # (module docstring; o still holds the linearisation at this point)
                bound = 10.0 * stat_rounding_spread(o, out["X"][b])
            worst[i] = max(worst[i], abs(got[i] - r[i]) / bound)
            assert abs(got[i] - r[i]) <= bound, (what, name, "instance", b, "reported", got[i], "reference", r[i], "bound", bound)
    return ref


# ------------------------------------------------------------------------------------------------------------ 0. the getter
def test_get_lam_order_and_refusals():
    """get(stage, 'lam'): 2 / 6 / 4 values, lower sides then upper sides in the order of sl / su -- what the batch getter of the whole
    array holds --, and a bad stage or length is refused like sl / su"""
    N, B = 17, 3
    x0, yref, cfg = sqp_case("ragged", B, N)
    s = _mk(B, N, nlp_solver_max_iter=2, **ZERO); _load(s, x0, yref, cfg); s.solve()
    assert s.get(0, "lam").shape == (B, 2) and s.get(3, "lam").shape == (B, 6) and s.get(N, "lam").shape == (B, 4)
    lam = _duals(s)[0]
    assert np.abs(lam).max() > 1e-3
    # one instance, one stage through the C-ABI with a stride of its own
    buf = np.full(8, -1.0)
    assert s._L.tum_ocp_get(s._h, 4, b"lam", buf.ctypes.data, 6, 1, 1, 8) == 0
    cols = [4, N + 2 * 3, N + 2 * 3 + 1]
    np.testing.assert_array_equal(buf[:6], np.concatenate([lam[1, cols], lam[1, [3 * N + c for c in cols]]]))
    assert (buf[6:] == -1.0).all()
    for stage, ln in ((0, 6), (3, 3), (N, 6), (N + 1, 4), (-2, 6)):
        assert s._L.tum_ocp_get(s._h, stage, b"lam", buf.ctypes.data, ln, 0, 1, 8) != 0, (stage, ln)
        assert "lam" in s._err()
    with pytest.raises(Exception, match="lam"):
        s.get(N + 1, "lam")
    assert s._L.tum_ocp_get(s._h, 3, b"lam", buf.ctypes.data, 6, 0, 1, 4) != 0          # stride < len


# ------------------------------------------------------------------------------------ 1. residuals at the library's own point
HORIZONS = (1, 5, 17, 38, 40, 41, 44, 48, 49, 50, 56)
CASES = [(N, kind) for N in HORIZONS for kind in ("nominal", "tight", "ragged") if kind == "nominal" or N >= 5]


@pytest.mark.parametrize("N,kind", CASES)
def test_residuals_at_the_librarys_own_point(N, kind):
    """Tolerances 0, max_iter 1, 2, 3, 6: every instance is active to the end and the reported residuals are those of iterate max_iter
    with the multipliers and slacks of QP max_iter. Batches of 1, 67 and (N = 40, 48: the longest-first dispatch order is in use from the
    capsule's second solve on) 1100 instances; every instance is compared, every 17th of the 1100."""
    worst = np.zeros(4)
    stat1 = 0.0
    for B in (1, 67) + ((1100,) if N in (40, 48) else ()):
        x0, yref, cfg = sqp_case(kind, B, N)
        o = make_oracle(N); apply_case_oracle(o, cfg)
        s = _mk(B, N, **ZERO)
        idx = np.arange(B) if B <= 256 else np.arange(0, B, 17)
        for mi in (1, 2, 3, 6):
            s.options_set("nlp_solver_max_iter", mi)
            _load(s, x0, yref, cfg)
            s.solve()
            out = _read(s)
            st, it = out["status"], out["sqp_iter"]
            assert np.isin(st, (2, 4)).all() and (it[st == 2] == mi).all() and (st == 2).mean() >= 0.9, (B, mi, st, it)
            ref = _hold_residuals(out, o, x0, yref, idx, (N, kind, B, mi), worst)
            # the inputs did their job on the reference
            if kind == "nominal":
                stat1 = max(stat1, ref[:, 0].max()) if mi == 1 else stat1
            else:
                used = max(out["sl"][idx].max(), out["su"][idx].max())
                assert ref[:, 2].max() > 1e-3 and used > 1e-3, (B, mi, ref[:, 2].max(), used)
            assert ref[:, 1].max() > 0 and ref[:, 3].max() > 0
    assert kind != "nominal" or stat1 > 1e-3, stat1          # (over the batches: at N = 1 the first instance is converged after one QP)
    print(f"N = {N}, {kind}: largest |reported - reference| / bound for stat, eq, ineq, comp: " + ", ".join(f"{w:.2e}" for w in worst))


def _bits(a, b, fields=FIELDS, mask=None):
    return [f for f in fields if not np.array_equal(a[f] if mask is None else a[f][mask], b[f] if mask is None else b[f][mask], equal_nan=True)]


@pytest.mark.parametrize("N", [5, 40, 48, 56])
def test_pass0_and_cold_start_forget_the_previous_solve(N):
    """Pass 0: after a cold start, with tolerances 1e30, every instance ends with status 0 and sqp_iter 0, X and U untouched to the bit,
    multipliers, slacks and QP statistics zero, the cost that of the cold start, and the residuals are the reference's with zero
    multipliers and slacks -- on a fresh capsule and on one
    that has solved another batch (whose multipliers and slacks are still on the device when cold_start() returns: a full SQP solve
    clears them first, as acados' reset does). Both capsules also return the same bits from a damped three-QP solve, where a stale
    slack or multiplier would enter the iterate itself."""
    B = 24
    x0, yref, cfg = sqp_case("ragged", B, N)
    xp, yp, cfgp = sqp_case("tight", B + 1, N)
    o = make_oracle(N); apply_case_oracle(o, cfg)
    outs = []
    worst = np.zeros(4)
    for reused in (False, True):
        s = _mk(B, N, qp_warm_start=False, nlp_solver_max_iter=3, **ZERO)
        if reused:
            _load(s, xp[1:], yp[1:], cfgp); s.solve()
            lam, sl, su = _duals(s)
            assert np.abs(lam).max() > 1e-3 and max(sl.max(), su.max()) > 1e-3          # (there is something to forget)
        _set_tols(s, 1e30)
        _load(s, x0, yref, cfg); s.solve()
        p0 = _read(s)
        assert (p0["status"] == 0).all() and (p0["sqp_iter"] == 0).all()
        np.testing.assert_array_equal(p0["X"], np.broadcast_to(x0[:, None, :], p0["X"].shape))
        assert not p0["U"].any() and not p0["lam"].any() and not p0["sl"].any() and not p0["su"].any()
        ref = _hold_residuals(p0, o, x0, yref, np.arange(B), (N, "pass 0", reused), worst)
        # no QP was solved for this problem: no statistics of an earlier one, and the cost is that of the cold start
        assert not p0["qp_iter"].any() and not p0["qp_status"].any() and not p0["res"].any()
        for b in range(B):
            o.cold_start(x0[b]); o.yref[:] = yref[b]
            cref = cost_at(o, p0["X"][b], p0["U"][b], p0["sl"][b], p0["su"][b])
            assert abs(p0["cost"][b] - cref) <= 1e-12 * abs(cref), (b, p0["cost"][b], cref)
        assert ref[:, :3].max(axis=0).min() > 1e-3, ref.max(axis=0)          # (ragged: violated at the cold start)
        _set_tols(s, 0.0); s.options_set("nlp_solver_step_length", 0.5)
        _load(s, x0, yref, cfg); s.solve()
        outs.append((p0, _read(s)))
    for a, b in zip(outs[0], outs[1]):
        assert _bits(a, b) == [], _bits(a, b)


# ---------------------------------------------------------------------------------------------------------- 2. termination
@pytest.mark.parametrize("N", [17, 40, 50])
def test_termination_test_decides_every_instance(N):
    """max_iter 1 and ONE finite tolerance (the others 1e30), set between two neighbouring reported residuals of the batch -- of pass 0 or
    of the pass behind the QP -- or exactly on one: every instance's outcome follows from the two residuals the library itself reported
    for it (strict '<', as acados): below at pass 0 -> status 0, sqp_iter 0, X and U untouched; else below behind the QP -> status 0,
    sqp_iter 1; else status 2. From a cold start (pass 0 has zero multipliers and slacks, so its comp is 0 and a comp tolerance alone
    ends every instance there) and from the state one QP has left (pass 0 is then that solve's last pass)."""
    B = 67
    seen, covered = set(), set()
    for kind in ("nominal", "ragged"):
        x0, yref, cfg = sqp_case(kind, B, N)
        s = _mk(B, N, nlp_solver_max_iter=1)
        passes = []
        _set_tols(s, 1e30); _load(s, x0, yref, cfg); s.solve()
        passes.append(_read(s))
        assert (passes[0]["sqp_iter"] == 0).all()
        _set_tols(s, 0.0)
        for mi in (1, 2):
            s.options_set("nlp_solver_max_iter", mi); _load(s, x0, yref, cfg); s.solve()
            passes.append(_read(s))
            assert (passes[mi]["sqp_iter"] == mi).all() and (passes[mi]["status"] == 2).all()
        s.options_set("nlp_solver_max_iter", 1)
        for warm in (0, 1):
            pa, pb = passes[warm], passes[warm + 1]
            r0, r1 = pa["residuals"], pb["residuals"]
            for j in range(4):
                tols = []
                for r in (r0, r1):
                    v = np.unique(r[:, j])
                    if len(v) >= 2:
                        i = len(v) // 2
                        tols += [0.5 * (v[i - 1] + v[i]), v[i]]          # between two neighbours, and on one
                        assert v[i - 1] < tols[-2] < v[i]
                for tol in tols:
                    _load(s, x0, yref, cfg)
                    if warm:
                        _set_tols(s, 0.0); s.solve()
                    t = [1e30] * 4; t[j] = tol
                    _set_tols(s, *t); s.solve()
                    g = _read(s)
                    at0 = r0[:, j] < tol
                    at1 = ~at0 & (r1[:, j] < tol)
                    cap = ~at0 & ~at1
                    what = (kind, warm, NAMES[j], tol)
                    assert (g["status"][at0 | at1] == 0).all() and (g["status"][cap] == 2).all(), what
                    assert (g["sqp_iter"][at0] == 0).all() and (g["sqp_iter"][~at0] == 1).all(), what
                    assert _bits(g, pa, ("X", "U", "residuals"), at0) == [] and _bits(g, pb, ("X", "U", "residuals"), ~at0) == [], what
                    seen |= {n for n, m in (("pass 0", at0), ("pass 1", at1), ("cap", cap)) if m.any()}
                    if at1.any() and cap.any():
                        covered.add(j)
    assert seen == {"pass 0", "pass 1", "cap"} and covered == {0, 1, 2, 3}, (seen, covered)


# ------------------------------------------------------------------------------------------------------------- 3. restores
@pytest.mark.parametrize("kind", ["nominal", "tight"])
@pytest.mark.parametrize("N", [17, 40, 48, 56])
def test_finished_instances_are_restored_to_the_bit(N, kind):
    """Default tolerances. An instance that has converged rides along through every later QP of the batch and is put back by the commit
    kernel: a run capped at c QPs and a run capped at 100 agree TO THE BIT on every instance the capped run reports converged, in every
    output; an instance at the cap of the short run needed more than c QPs in the long one. Solving again from the result changes
    nothing on a converged instance and reports sqp_iter 0. The cost of every finite instance is the reference's at its own point."""
    B = 32
    x0, yref, cfg = sqp_case(kind, B, N)
    long_ = _mk(B, N, nlp_solver_max_iter=100); _load(long_, x0, yref, cfg); long_.solve()
    L = _read(long_)
    s = _mk(B, N)
    for c in (5, 10, 20, 40):
        s.options_set("nlp_solver_max_iter", c); _load(s, x0, yref, cfg); s.solve()
        g = _read(s)
        conv, cap = g["status"] == 0, g["status"] == 2
        assert _bits(g, L, FIELDS, conv) == [], (c, _bits(g, L, FIELDS, conv))
        assert (g["sqp_iter"][conv] <= c).all() and (L["sqp_iter"][cap] > c).all(), (c, g["sqp_iter"], L["sqp_iter"])
        assert (g["residuals"][conv] < 1e-6).all()
        print(f"N = {N}, {kind}, cap {c}: converged {conv.sum()}, at the cap {cap.sum()}, failed {(g['status'] == 4).sum()} of {B}")
    assert conv.sum() >= B // 8 and cap.sum() >= B // 8, (conv.sum(), cap.sum())
    # (Two runs that both carry a finished instance through further QPs repeat the same ride-along QP from the same restored state: a
    #  field the commit kernel forgot would hold that QP's value in both.) A run capped at exactly the n QPs an instance needs ends with
    #  the pass that finds it converged, with no QP behind it: its outputs are the ones the long run must have put back.
    done = L["status"] == 0
    for n in np.unique(L["sqp_iter"][done])[:3]:
        m = done & (L["sqp_iter"] == n)
        s.options_set("nlp_solver_max_iter", int(n)); _load(s, x0, yref, cfg); s.solve()
        g = _read(s)
        assert n >= 1 and (g["status"][m] == 0).all() and _bits(g, L, FIELDS, m) == [], (n, _bits(g, L, FIELDS, m))
    # the cost (step length 1: the expansion's) of converged, capped and restored instances alike
    o = make_oracle(N); apply_case_oracle(o, cfg)
    worst = 0.0
    for b in np.nonzero(np.isin(L["status"], (0, 2)))[0]:
        o.cold_start(x0[b]); o.yref[:] = yref[b]
        cref = cost_at(o, L["X"][b], L["U"][b], L["sl"][b], L["su"][b])
        worst = max(worst, abs(L["cost"][b] - cref) / abs(cref))
        assert abs(L["cost"][b] - cref) <= 1e-12 * abs(cref), (b, L["status"][b], L["cost"][b], cref)
    print(f"N = {N}, {kind}: get_cost against cost_at, worst relative difference {worst:.2e}")
    # once more without a cold start
    long_.solve()
    again = _read(long_)
    assert (again["sqp_iter"][done] == 0).all() and (again["status"][done] == 0).all()
    rest = tuple(f for f in FIELDS if f != "sqp_iter")
    assert _bits(again, L, rest, done) == [], _bits(again, L, rest, done)


# -------------------------------------------------------------------------------------------------------------- 4. failures
def test_nan_input_freezes_its_own_instance_only():
    """a NaN in one instance's yref: its first QP fails -- status 4, sqp_iter 1, X and U those of the cold start to the bit -- and every
    other instance is bit-identical, in every output, to the same batch without the NaN"""
    N, B, bad = 40, 12, 5
    x0, yref, cfg = sqp_case("tight", B, N)
    s = _mk(B, N, nlp_solver_max_iter=6, **ZERO); _load(s, x0, yref, cfg); s.solve()
    good = _read(s)
    assert (good["status"] == 2).all()
    y = yref.copy(); y[bad, 7, 1] = np.nan
    _load(s, x0, y, cfg); s.solve()
    g = _read(s)
    keep = np.arange(B) != bad
    assert g["status"][bad] == 4 and g["sqp_iter"][bad] == 1
    np.testing.assert_array_equal(g["X"][bad], np.broadcast_to(x0[bad], (N + 1, 8)))
    assert not g["U"][bad].any()
    assert _bits(g, good, FIELDS, keep) == [], _bits(g, good, FIELDS, keep)


def test_failed_qp_freezes_the_last_good_iterate():
    """An instance whose QP fails at SQP iteration n keeps, through all later iterations of the batch, the X and U that the same capsule
    returns for max_iter = n - 1, to the bit, and status 4.
    The interior point method's iteration cap cannot provoke this: a QP at qp_iter_max is not a failure (status 0, as acados; the
    oracle agrees: no failure with caps from 1 to 50 on the test inputs). What fails a QP a few iterations into a solve is an iterate
    the model no longer evaluates at: config 2 at 1 m/s with a velocity reference of 0 drives instances through v = 0 -- on the
    oracle 12 of 48 fail, between the 1st and the 22nd QP. The share of failed instances must lie between 5 % and 50 %."""
    N, B, cap = 40, 96, 30
    x0, yref, cfg = sqp_case("nominal", B, N)
    x0[:, 3] = 1.0; yref[:, :, 3] = 0.0
    s = _mk(B, N, nlp_solver_max_iter=cap, **ZERO); _load(s, x0, yref, cfg); s.solve()
    g = _read(s)
    failed = g["status"] == 4
    print(f"failed {failed.sum()} of {B}, at the iterations {sorted(int(v) for v in g['sqp_iter'][failed])}")
    assert np.isin(g["status"], (2, 4)).all() and (g["sqp_iter"][~failed] == cap).all()
    assert 0.05 <= failed.mean() <= 0.5, failed.mean()
    assert (g["sqp_iter"][failed] > 1).any()
    for n in np.unique(g["sqp_iter"][failed]):
        m = failed & (g["sqp_iter"] == n)
        if n == 1:
            X, U = np.broadcast_to(x0[:, None, :], g["X"].shape), np.zeros_like(g["U"])
        else:
            s.options_set("nlp_solver_max_iter", int(n) - 1); _load(s, x0, yref, cfg); s.solve()
            X, U = s.get_iterate()
            assert (s.get_stats("sqp_iter")[m] == n - 1).all()
        assert np.isfinite(X[m]).all() and np.isfinite(U[m]).all()
        assert np.array_equal(g["X"][m], X[m]) and np.array_equal(g["U"][m], U[m]), n


# ---------------------------------------------------------------------------------------------------------- 5. damped steps
def _ulp_close(got, prev, full, alpha, what):
    want = prev + alpha * (full - prev)
    tol = 4 * np.spacing(np.maximum(np.abs(prev), np.abs(full)))
    err = np.abs(got - want)
    assert (err <= tol).all(), (what, float((err / np.maximum(tol, 5e-324)).max()))


@pytest.mark.parametrize("alpha", [0.5, 0.25])
@pytest.mark.parametrize("kind", ["nominal", "ragged"])
@pytest.mark.parametrize("N,full_w", [(17, False), (40, False), (45, False), (50, False), (17, True), (40, True), (45, True)])
def test_damped_steps_and_the_residual_kernels_cost(N, full_w, kind, alpha):
    """nlp_solver_step_length < 1 (interior point warm start off, tolerances 0). After one QP every variable is prev + alpha (full - prev)
    with `full` the step-length-1 run's, to 4 ulp of the larger operand (one subtraction, one multiply-add, possibly contracted). After
    2 and 4 QPs X and U follow oracle_sqp(alpha) (scale-relative 1e-6, the bound of the existing parity test), and get_cost() -- with a
    step length below 1 the residual kernel's own evaluation, diagonal or full W -- is cost_at at the library's own point to 1e-12
    (at most 57 * 6 + 56 * 12 non-negative terms; numpy and the C oracle differ by 1.4e-14 on the same sum)."""
    from test_full_w import _spd_weights
    from test_gpu_sqp import _scale_rel
    B = 8
    x0, yref, cfg = sqp_case(kind, B, N)
    base = make_oracle(N).W.copy()
    Wf = _spd_weights(np.random.default_rng(N), np.broadcast_to(base, (B, N + 1, 6)).copy()) if full_w else None

    def load(s):
        if full_w:
            for k in range(N):
                s.cost_set(k, "W", Wf[:, k])
            s.cost_set(N, "W", Wf[:, N, :4, :4])
        _load(s, x0, yref, cfg)

    def oracle(b):
        o = make_oracle(N); apply_case_oracle(o, cfg)
        if full_w:
            o.set_full_W(Wf[b])
        o.cold_start(x0[b]); o.yref[:] = yref[b]; o.qp_warm_start(False)
        return o

    f = _mk(B, N, qp_warm_start=False, nlp_solver_max_iter=1, **ZERO); load(f); f.solve()
    F = _read(f)
    s = _mk(B, N, qp_warm_start=False, nlp_solver_step_length=alpha, **ZERO)
    worst_c = worst_x = 0.0
    for mi in (1, 2, 4):
        s.options_set("nlp_solver_max_iter", mi); load(s); s.solve()
        g = _read(s)
        assert (g["status"] == 2).all() and (g["sqp_iter"] == mi).all()
        if mi == 1:
            _ulp_close(g["X"], np.broadcast_to(x0[:, None, :], g["X"].shape), F["X"], alpha, "X")
            for k in ("U", "sl", "su", "lam"):
                _ulp_close(g[k], 0.0, F[k], alpha, k)
            assert np.abs(F["lam"]).max() > 1e-3 and (kind == "nominal" or max(F["sl"].max(), F["su"].max()) > 1e-3)
        Xo, Uo = np.zeros_like(g["X"]), np.zeros_like(g["U"])
        for b in range(B):
            o = oracle(b)
            n, conv, r = oracle_sqp(o, mi, tol=0.0, with_stat=False, alpha=alpha)
            assert n == mi
            Xo[b], Uo[b] = o.X, o.U
            cref = cost_at(o, g["X"][b], g["U"][b], g["sl"][b], g["su"][b])
            worst_c = max(worst_c, abs(g["cost"][b] - cref) / abs(cref))
            assert abs(g["cost"][b] - cref) <= 1e-12 * abs(cref), (mi, b, g["cost"][b], cref)
        ex, eu = _scale_rel(g["X"], Xo).max(), _scale_rel(g["U"], Uo).max()
        worst_x = max(worst_x, ex, eu)
        assert ex < 1e-6 and eu < 1e-6, (mi, ex, eu)
    print(f"N = {N}, full W {full_w}, {kind}, alpha {alpha}: cost against cost_at {worst_c:.2e} relative; X, U against oracle_sqp {worst_x:.2e} scale-relative")


# ---------------------------------------------------------------------------------------------- 6. neighbouring tile counts
_CHILD = (
    "import sys, numpy as np\n"
    "sys.path[:0] = [%r, %r]\n"
    "import torch\n"
    "from test_sqp import sqp_case\n"
    "from test_gpu_sqp_reference import _mk, _load, _read, ZERO\n"
    "N, B = int(sys.argv[1]), 48\n"
    "x0, yref, cfg = sqp_case('ragged', B, N)\n"
    "s = _mk(B, N, nlp_solver_max_iter=3, **ZERO); _load(s, x0, yref, cfg); s.solve()\n"
    "np.savez(sys.argv[2], **_read(s))\n" % (ROOT, os.path.join(ROOT, "tests")))


def test_neighbouring_tile_counts_agree_in_sqp_mode(tmp_path):
    """TUM_FORCE_TILES (read once per process) runs nlp_residual_kernel<6> and <7> at a horizon a smaller instantiation covers: N = 40 on
    five (native), six and seven tiles, N = 48 on six (native) and seven, ragged inputs, tolerances 0, three QPs, each in a process of
    its own. Every run's residuals are the reference's at its own point (the bounds above); six and seven tiles return the same X, U,
    multipliers and slacks to the bit (the padding variables do not matter: tests/test_gpu_pipeline.py finds the pipeline so), five
    tiles the same solve to solver accuracy (another factor layout)."""
    out, procs = {}, []
    for N, force in ((40, "0"), (40, "6"), (40, "7"), (48, "0"), (48, "7")):          # (five small processes side by side)
        f = str(tmp_path / f"t{N}_{force}.npz")
        procs.append((N, force, f, subprocess.Popen([sys.executable, "-c", _CHILD, str(N), f], env=dict(os.environ, TUM_FORCE_TILES=force),
                                                    stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
    for N, force, f, pr in procs:
        err = pr.communicate(timeout=600)[1]
        assert pr.returncode == 0, err[-2000:]
        out[(N, force)] = dict(np.load(f))
    worst = np.zeros(4)
    for (N, force), g in out.items():
        x0, yref, cfg = sqp_case("ragged", 48, N)
        o = make_oracle(N); apply_case_oracle(o, cfg)
        assert (g["status"] == 2).all() and (g["sqp_iter"] == 3).all()
        ref = _hold_residuals(g, o, x0, yref, np.arange(48), (N, "tiles", force), worst)
        assert ref.max(axis=0).min() > 1e-3, ref.max(axis=0)
    print("forced tile counts: largest |reported - reference| / bound for stat, eq, ineq, comp: " + ", ".join(f"{w:.2e}" for w in worst))
    same = ("X", "U", "lam", "sl", "su", "qp_iter")
    assert _bits(out[(48, "0")], out[(48, "7")], same) == [], _bits(out[(48, "0")], out[(48, "7")], same)
    assert _bits(out[(40, "6")], out[(40, "7")], same) == [], _bits(out[(40, "6")], out[(40, "7")], same)
    for force in ("6", "7"):
        a, b = out[(40, "0")], out[(40, force)]
        assert np.abs(a["U"] - b["U"]).max() < 1e-6 and np.abs(a["X"] - b["X"]).max() < 1e-6 and np.abs(a["qp_iter"] - b["qp_iter"]).max() <= 1
