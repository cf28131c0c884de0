"""tests/cond_reference.py -- the condensed QP and the expansion restated in numpy, in long double and in binary64 -- against the
oracle's own condensing (OracleOcp.solve_debug, the checker that is pinned to the acados logs), and against itself.

The oracle linearises INSIDE solve_debug and then takes the step: the test reads the oracle's A, B, b after the call and compares
at a copy of the iterate made before it. h and grad h of the comparison are the oracle's own (oracle.h_con): what is tied here is
the condensing, not the model. Agreement is measured in units of u x scale with the long-double run as the truth for both sides
(cond_reference: SCALES) and printed ("cond_bounds cpu ..." lines, `pytest -s`): the CPU half of profiles/cond_bounds.txt.

This module also builds the inputs tests/test_gpu_cond_reference.py shares: the excited iterate, the weights, h and grad h at
an iterate from tests/model_reference.py with that module's bounds.
"""
import functools

import numpy as np
import pytest

import cond_reference as cr
from oracle import oracle as orc

DT, NSUB = 0.08, 3
CASES = [(5, False), (17, False), (40, False), (41, False), (56, False), (12, True), (45, True)]


def base_weights(N):
    """(N + 1, 6): the diagonal W of the reference OCP (0.01 blockdiag(Q, R), the terminal stage its first four)"""
    from tum_control_amd import config
    m = config.MPC
    o = orc.OracleOcp(N, DT, NSUB)
    o.set_weights(m["q_lon"], m["q_yaw"], m["q_vel"], m["r_jerk"], m["r_steering_rate"], m["L1_pen"], m["L2_pen"], scale=0.01)
    return o.W.copy()


def varied_diagonal(rng, base, B):
    """(B, N + 1, 6): stage- and instance-dependent diagonal weights, one state weight of every instance exactly 0"""
    W = base[None] * rng.uniform(0.5, 2.0, (B,) + base.shape)
    N = base.shape[0] - 1
    for b in range(B):
        W[b, (b + N // 2) % (N + 1), 1] = 0.0
    return W


def spd_weights(rng, base, B):
    """(B, N + 1, 6, 6): test_full_w._spd_weights, symmetric to the bit"""
    from test_full_w import _spd_weights
    Wf = _spd_weights(rng, np.broadcast_to(base, (B,) + base.shape).copy())
    return 0.5 * (Wf + np.swapaxes(Wf, -1, -2))


def clear_yaw(yaw, margin=2e-3):
    """yaws closer than `margin` to a multiple of 2 pi are moved to that distance"""
    yaw = np.array(yaw, dtype=np.float64)
    r = np.fmod(yaw, cr.TWO_PI)
    near0 = np.abs(r) < margin
    nearT = cr.TWO_PI - np.abs(r) < margin
    yaw = np.where(near0, yaw - r + np.where(r >= 0, margin, -margin), yaw)
    return np.where(nearT, yaw - np.sign(r) * (margin - (cr.TWO_PI - np.abs(r))), yaw)


def cold_problem(N, B, seed):
    """x0 (B, 8), yref (B, N + 1, 6) of the synthetic workload; the cold start makes X_k = x0, U = 0: large defects at every stage"""
    from tum_control_amd.workloads import nominal_batch
    x0, yref = nominal_batch(B, N=N, seed=seed)
    x0[:, 2] = clear_yaw(x0[:, 2])
    return x0, yref


def excited_problem(N, B, seed):
    """x0, yref, X, U of a stage-varying, inconsistent iterate: inputs of order 1 and 0.05, a rollout of them perturbed by 1e-3 at every
    stage (defects everywhere), x0 != X_0 (g_0 != 0), and the yaw crossing 2 pi between two stages inside the horizon (the
    reference's yaw moved along and wrapped). Every yaw stays 1e-3 away from the multiples of 2 pi (asserted)."""
    x0, yref = cold_problem(N, B, seed)
    rng = np.random.default_rng(seed + 1)
    X = np.zeros((B, N + 1, 8)); U = np.zeros((B, N, 2))
    for b in range(B):
        x0[b, 7] = 0.8; x0[b, 5] = 0.12; x0[b, 4] = 0.3
        U[b] = np.stack([rng.normal(0, 1.0, N), rng.normal(0, 0.05, N)], axis=1)
        X[b, 0] = x0[b]
        for k in range(N):
            X[b, k + 1] = orc.rk4_sens(X[b, k], U[b, k], DT, NSUB)[0]
        m = int(np.argmax(np.abs(np.diff(X[b, :, 2]))))                  # (random inputs: the yaw need not be monotone)
        shift = cr.TWO_PI - 0.5 * (X[b, m, 2] + X[b, m + 1, 2])          # 2 pi half way between the two stages furthest apart in yaw
        X[b, :, 2] += shift
        yref[b, :, 2] = cr.wrap(yref[b, :, 2] + shift)
        X[b] += rng.normal(0, 1e-3, X[b].shape)
        X[b, :, 2] = clear_yaw(X[b, :, 2])
        x0[b] = X[b, 0] + rng.normal(0, 1e-3, 8)
        x0[b, 2] = clear_yaw(x0[b, 2])
        assert np.any(np.diff(np.floor(X[b, :, 2] / cr.TWO_PI)) != 0), "the yaw does not cross 2 pi"
    assert cr.yaw_margin(X[:, :, 2]) >= 1e-3 and cr.yaw_margin(x0[:, 2]) >= 1e-3
    return x0, yref, X, U


def _ld(v):
    """an mpmath number as a long double (two binary64 pieces)"""
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - hi))


def h_exact(X):
    """h (N + 1,) and grad h (N + 1, 8) at the states X in long double, from tests/model_reference.py (60 digits: no state here has an
    entry of 1e-300), and that module's bounds of a binary64 evaluation of them (test_model_reference.allowance): bh, bgh"""
    import model_reference as mr
    from test_model_reference import allowance
    n = X.shape[0]
    h = np.zeros(n, dtype=np.longdouble); gh = np.zeros((n, 8), dtype=np.longdouble); bh = np.zeros(n); bgh = np.zeros((n, 8))
    for k in range(n):
        hv, gv, _ = mr.eval_h(X[k], dps=mr.DPS, raw=True)
        h[k] = _ld(hv); gh[k] = [_ld(t) for t in gv]
        _, bd = allowance(X[k], np.zeros(2), DT, NSUB)
        bh[k] = bd["h"][0]; bgh[k] = bd["gh"]
    return h, gh, bh, bgh


ARRAYS = ("H", "q", "C", "d", "g")


@functools.lru_cache(maxsize=None)
def oracle_case(N, full):
    """the oracle's condensed QP at the excited iterate and both runs of the reference on the oracle's own A, B, b, h, grad h"""
    x0, yref, X, U = excited_problem(N, 1, 300 + N)
    rng = np.random.default_rng(N)
    base = base_weights(N)
    o = orc.OracleOcp(N, DT, NSUB)
    o.W[:] = base
    W = base
    if full:
        W = spd_weights(rng, base, 1)[0]
        o.set_full_W(W)
    else:
        W = varied_diagonal(rng, base, 1)[0]
        o.W[:] = W
    o.cold_start(x0[0]); o.X[:] = X[0]; o.U[:] = U[0]; o.yref[:] = yref[0]
    o.set_iter_max(1)
    X0, U0 = o.X.copy(), o.U.copy()          # (solve_debug takes the step)
    _, qp = o.solve_debug()
    A, B, b = o.A.copy(), o.B.copy(), o.b.copy()
    hh = [orc.h_con(X0[k]) for k in range(N + 1)]
    h = np.array([t[0] for t in hh]); gh = np.stack([t[1] for t in hh])
    args = (A, B, b, X0, U0, x0[0], yref[0], W, DT, h, gh)
    ld, f64 = cr.condense(*args, dtype=np.longdouble), cr.condense(*args, dtype=np.float64)
    want = dict(H=qp["H"], q=qp["q"], C=qp["C"][N:], d=qp["d"][N:], g=qp["g"])
    return dict(N=N, ld=ld, f64=f64, oracle=want, qp=qp, U0=U0)


def agreement(case):
    """per array: (oracle, binary64 run of the reference, its a-priori bound), all in u x scale against the long-double run"""
    ld, f64, want = case["ld"], case["f64"], case["oracle"]
    return {k: (cr.units(want[k], ld[k], ld["s" + k]), cr.units(f64[k], ld[k], ld["s" + k]), f64["n" + k]) for k in ARRAYS}


@pytest.mark.parametrize("N,full", CASES)
def test_reference_equals_the_oracles_condensed_qp(N, full):
    """Oracle and binary64 statement are two orders of the same sums: each is within its count of roundings of the long-double truth
    (the oracle's plain loops have the counts of cond_reference.condense: the same recursion depth, the same sums), so they agree."""
    case = oracle_case(N, full)
    qp = case["qp"]
    # the rows of the input bounds, which the reference does not restate: unit rows and the inputs themselves
    assert np.array_equal(qp["d"][:N], case["U0"][:, 1])
    Cbu = np.zeros((N, 2 * N)); Cbu[np.arange(N), 2 * np.arange(N) + 1] = 1.0
    assert np.array_equal(qp["C"][:N], Cbu)
    for k, (e_or, e_64, n) in agreement(case).items():
        print(f"cond_bounds cpu N={N} {'full' if full else 'diag'} W {k}: oracle {e_or:.2f} fp64 {e_64:.2f} a-priori {n} (u x scale)")
        assert e_or <= n and e_64 <= n, (k, e_or, e_64, n)


@pytest.mark.parametrize("N,full", CASES)
def test_reference_structure(N, full):
    """row 6 of G_s: dt on the odd columns below 2 s, 0 elsewhere; the columns at and beyond 2 s of stage s: 0 -- exactly, in both runs"""
    case = oracle_case(N, full)
    for run in (case["ld"], case["f64"]):
        G, C = run["G"], run["C"]
        for s in range(N + 1):
            want = np.where((np.arange(2 * N) % 2 == 1) & (np.arange(2 * N) < 2 * s), DT, 0.0)
            assert np.array_equal(G[s, 6].astype(np.float64), want) and np.array_equal(G[s, 6], want.astype(G.dtype)), s
            assert not G[s, :, 2 * s:].any(), s
            if s >= 1:
                assert not C[2 * (s - 1):2 * s, 2 * s:].any(), s
        assert np.array_equal(run["H"], run["H"].T) or cr.units(run["H"], run["H"].T, run["sH"]) <= run["nH"]


@pytest.mark.parametrize("N,full", CASES)
def test_long_double_run_is_long_double(N, full):
    """the binary64 run is within its own a-priori bound of the long-double run -- and NOT equal to it: a reference that silently
    computed in binary64 would agree to the bit"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    case = oracle_case(N, full)
    ld, f64 = case["ld"], case["f64"]
    for k in ARRAYS + ("G", "res"):
        assert ld[k].dtype == np.longdouble and f64[k].dtype == np.float64
        e = cr.units(f64[k], ld[k], ld["s" + k])
        assert e <= f64["n" + k], (k, e, f64["n" + k])
    assert all(cr.units(f64[k], ld[k], ld["s" + k]) > 0.0 for k in ("H", "q", "C", "d", "g"))


def test_expansion_and_cost_reproduce_the_oracles_step():
    """the expansion and the cost of the reference on the oracle's own step: X+, U+ and eval_cost, N = 17 (diagonal W) and 12 (full W)"""
    for N, full in ((17, False), (12, True)):
        x0, yref, X, U = excited_problem(N, 1, 300 + N)
        base = base_weights(N)
        o = orc.OracleOcp(N, DT, NSUB)
        o.W[:] = base
        W = base
        if full:
            W = spd_weights(np.random.default_rng(N), base, 1)[0]
            o.set_full_W(W)
        from tum_control_amd import config
        o.zl[:] = o.zu[:] = config.MPC["L1_pen"]; o.Zl[:] = o.Zu[:] = config.MPC["L2_pen"]
        o.cold_start(x0[0]); o.X[:] = X[0]; o.U[:] = U[0]; o.yref[:] = yref[0]
        X0, U0 = o.X.copy(), o.U.copy()
        assert o.solve() == 0
        dv = (o.U - U0).reshape(-1)
        ex = cr.expand(o.A, o.B, o.b, X0, U0, x0[0], dv)
        extra = cr.step_sensitivity(o.A, o.B, np.abs(o.U))          # (dv is recovered from U+ - U: one rounding of U+)
        err = np.abs(o.X.astype(np.longdouble) - ex["X"])
        assert np.all(err <= cr.U53 * ((2 * 9 * N + 4) * ex["sX"] + extra)), float(np.max(err))
        c, sc, n = cr.cost(o.X, o.U, yref[0], W, DT, o.sl, o.su, o.zl, o.zu, o.Zl, o.Zu)
        assert abs(np.longdouble(o.cost) - c) <= n * cr.U53 * sc, (o.cost, float(c), float(sc))
