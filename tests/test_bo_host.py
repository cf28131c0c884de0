"""
The host side of the Bayesian-optimisation step (tum_control_amd/bo.py): the packed model against the textbook GP posterior, the
cell formula of the hypervolume improvement against the area of a union of rectangles, the quadrature of the feasibility factor
against adaptive integration, fit_gp, the front utilities, the CSV format, appending a pick and the driver. No GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_reference as ref          # noqa: E402
from tum_control_amd import bo      # noqa: E402

U = 2.0 ** -53
LD = np.longdouble


def test_cabi_exports_every_declared_bo_symbol():
    """The built library exports every tum_bo_ function include/tum_nmpc.h declares, and solver.BO_SYMBOLS lists exactly those."""
    import re
    import __graft_entry__ as g
    from tum_control_amd import solver
    g.build()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tum_nmpc.h")).read()
    declared = sorted(set(re.findall(r"\b(tum_bo_\w+)\s*\(", hdr)))
    assert len(declared) == 5 and sorted(solver.BO_SYMBOLS) == declared
    L = solver.load_library()
    for sym in declared:
        assert hasattr(L, sym), sym


def _chol_ld(A):
    A = np.asarray(A, dtype=LD)
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(i + 1):
            v = A[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(v) if i == j else v / L[j, j]
    return L


def test_packed_model_reproduces_the_textbook_posterior():
    """n = 6, d = 2. Textbook: mean c + K_bt A^-1 (y - c), covariance K_bb - K_bt A^-1 K_tb, A = K + noise I, by np.linalg.solve.
    Tolerance: the same textbook formulas are evaluated in long double (Cholesky and forward substitution written out); the gate is 4 x
    the error of the FP64 textbook value against it, with a floor of 32 u s -- both FP64 routes round the same ill-conditioned solve."""
    rng = np.random.default_rng(0)
    Xt, Xb = rng.random((6, 2)), rng.random((3, 2))
    y = rng.standard_normal((6, 2))
    hyp, cls = ref.hypers(2)
    Z = bo.sobol_normal(8, 2 * 5, 0).reshape(8, 2, -1).transpose(0, 2, 1)
    m = bo.pack_model(Xt, y, hyp, Xt, np.array([1, 0, 1, 1, 0, 1], dtype=bool), cls, Xb, Z, [-3.0, -3.0], jitter=1e-9)
    x = rng.random((4, 2))
    terms = bo._candidate_terms(m, x)
    for o in range(2):
        h = hyp[o]
        A = bo.rbf(Xt, Xt, h.ils, h.s) + h.noise * np.eye(6)
        Kbt, Kbb = bo.rbf(Xb, Xt, h.ils, h.s), bo.rbf(Xb, Xb, h.ils, h.s)
        mean64 = h.c + Kbt @ np.linalg.solve(A, y[:, o] - h.c)
        cov64 = Kbb - Kbt @ np.linalg.solve(A, Kbt.T)
        # long double
        L = _chol_ld(ref._rbf_ld(Xt, Xt, h.ils, h.s) + LD(h.noise) * np.eye(6, dtype=LD))
        Kbt_l, Kbb_l = ref._rbf_ld(Xb, Xt, h.ils, h.s), ref._rbf_ld(Xb, Xb, h.ils, h.s)
        w = ref.forward_substitution(L, (np.asarray(y[:, o], dtype=LD) - LD(h.c))[:, None])
        Wb = ref.forward_substitution(L, Kbt_l.T)
        mean_l = LD(h.c) + (Wb * w).sum(0)
        cov_l = Kbb_l - ref._mm(Wb.T, Wb)
        tol_mean = max(32 * U * h.s, 4 * float(np.abs(mean64 - mean_l).max()))
        tol_cov = max(32 * U * h.s, 4 * float(np.abs(cov64 - cov_l).max()))
        assert float(np.abs(m.mu_b[o] - mean_l).max()) <= tol_mean
        cov_packed = m.L_b[o] @ m.L_b[o].T - m.jitter[o] * np.eye(3)
        assert float(np.abs(cov_packed - cov_l).max()) <= tol_cov
        assert np.abs(m.R[o] @ m.L_b[o] - np.eye(3)).max() <= 64 * U * np.linalg.cond(m.L_b[o])
        # a candidate: mean, and variance conditional on the baseline draws, d2 = S_xx - S_xb (S_bb + j I)^-1 S_bx
        kx = ref._rbf_ld(Xt, x, h.ils, h.s)
        Wx = ref.forward_substitution(L, kx)
        mu_l = LD(h.c) + (Wx * w).sum(0)
        Sxb = ref._rbf_ld(Xb, x, h.ils, h.s) - ref._mm(Wb.T, Wx)
        Lb = _chol_ld(cov_l + LD(m.jitter[o]) * np.eye(3, dtype=LD))
        lx = ref.forward_substitution(Lb, Sxb)
        d2_l = np.maximum(LD(h.s) - (Wx * Wx).sum(0) - (lx * lx).sum(0), LD(m.jitter[o]))
        mu64 = h.c + bo.rbf(x, Xt, h.ils, h.s) @ np.linalg.solve(A, y[:, o] - h.c)
        assert float(np.abs(terms[o][0] - mu_l).max()) <= max(32 * U * h.s, 4 * float(np.abs(mu64 - mu_l).max()))
        # (the conditional variance goes through the inverse of S_bb + j I: its rounding is amplified by that matrix's condition)
        assert float(np.abs(terms[o][3] - d2_l).max()) <= 64 * U * h.s * np.linalg.cond(cov64 + m.jitter[o] * np.eye(3))


FRONT5 = np.array([[0.1, 0.9], [0.3, 0.7], [0.5, 0.5], [0.7, 0.3], [0.9, 0.1]])


@pytest.mark.parametrize("F", [np.zeros((0, 2)), np.array([[0.4, 0.6]]), FRONT5], ids=["P0", "P1", "P5"])
def test_hvi_cell_formula_is_the_area_of_the_union(F):
    r = np.array([0.0, 0.0])
    rng = np.random.default_rng(len(F))
    pts = [rng.random(2) * 1.2 - 0.1 for _ in range(40)] + [np.array([2.0, 2.0]), np.array([-1.0, 0.5]), np.array([0.5, -1.0])]
    pts += [p.copy() for p in F] + [p - 0.05 for p in F] + [np.array([p[0], 1.5]) for p in F] + [np.array([1.5, p[1]]) for p in F]
    Fs = bo.front_2d(F, r)
    for f in pts:
        want = ref.union_area(F, r, f)
        got = bo.hvi_2d(Fs, r, f)
        assert abs(got - want) <= 16 * U * max(1.0, want), (f, got, want)
    for p in F:
        assert bo.hvi_2d(Fs, r, p) == 0.0 and bo.hvi_2d(Fs, r, p - 0.05) == 0.0          # on the front; dominated by it
    if len(F):
        top = np.array([2.0, 2.0])          # dominates the whole front: the box less the front's own hypervolume
        assert abs(bo.hvi_2d(Fs, r, top) - (4.0 - bo.hypervolume_2d(F, r))) <= 16 * U * 4.0


def test_host_acquisition_uses_the_cell_formula_per_sample():
    m = ref.generate(2, 16, 16, 64, 8, 8, seed=3)
    X = np.random.default_rng(0).random((5, 2))
    _, det = bo.host_acquisition(m, X, detail=True)
    terms = bo._candidate_terms(m, X)
    for c in range(5):
        tot = 0.0
        for s in range(m.S):
            f = [terms[o][0][c] + m.Z(o)[s] @ terms[o][2][:, c] + np.sqrt(terms[o][3][c]) * m.zeta(o)[s] for o in range(2)]
            tot += bo.hvi_2d(m.fronts[s, :m.front_count[s]], m.ref, f)
        assert abs(det[c, 4] - tot / m.S) <= 64 * U * max(1.0, abs(tot))


def _fixture_model(golden_dir):
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"][:300], z["feasible"][:300], z["objectives"][:300]
    Xt = Xn[feas]
    o_h, c_h = ref.hypers(7)
    Z = bo.sobol_normal(16, 2 * (len(Xt) + 2), 4).reshape(16, 2, -1).transpose(0, 2, 1)
    return bo.pack_model(Xt, bo.standardize(obj[feas][:, 0, :])[0], o_h, Xn, feas, c_h, Xt, Z, np.array([-0.5, -0.75]), jitter=1e-6)


@pytest.mark.filterwarnings("ignore::scipy.integrate.IntegrationWarning")
def test_gauss_hermite_moments_against_adaptive_integration(golden_dir):
    """E sigmoid(t) and the standard deviation of sigmoid(t), t ~ N(m, v), over the (m, v) range the fixture's feasibility model produces
    at Sobol candidates and at its own trials. The reference estimates both from 2^14 draws: standard errors sd / 128 and sd / 181. The
    rule must be 100 times finer than that; the smallest K of 8, 16, 32, 48, 64 that is becomes the default (profiles/bo_bounds.txt)."""
    from scipy.integrate import quad
    m = _fixture_model(golden_dir)
    X = np.vstack([bo.sobol_points(64, 7, 5), m.Xc[::5]])
    mk, vk = [], []
    for g in (2, 3):
        kc = bo.rbf(m.Xc, X, m.ils[g], m.s[g])
        q = m.V[g] @ kc
        mk.append(m.c[g] + m.a[g] @ kc); vk.append(m.s[g] - (q * q).sum(0))
    mean, var = mk[1] - mk[0], np.maximum(vk[0] + vk[1], 0)
    grid = [(a, b) for a in np.linspace(mean.min(), mean.max(), 6) for b in np.linspace(var.min(), var.max(), 5)]
    print(f"bo_bounds quadrature grid: mean {mean.min():.3f} .. {mean.max():.3f}, variance {var.min():.3f} .. {var.max():.3f}")
    truth = []
    for a, b in grid:
        sd = np.sqrt(b)
        pdf = lambda t: np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)          # noqa: E731
        p = quad(lambda t: float(bo.sigmoid(a + sd * t)) * pdf(t), -12, 12, epsabs=1e-14, epsrel=1e-14, limit=400)[0]
        v = quad(lambda t: (float(bo.sigmoid(a + sd * t)) - p) ** 2 * pdf(t), -12, 12, epsabs=1e-16, epsrel=1e-14, limit=400)[0]
        truth.append((p, np.sqrt(v)))
    good = []
    for K in (8, 16, 32, 48, 64):
        gx, gw = bo.gauss_hermite(K)
        ep = es = 0.0
        for (a, b), (p, s) in zip(grid, truth):
            sg = bo.sigmoid(a + np.sqrt(b) * gx)
            pk = sg @ gw
            sk = np.sqrt(((sg - pk) ** 2) @ gw)
            ep, es = max(ep, abs(pk - p) / (s / 128 / 100)), max(es, abs(sk - s) / (s / 181 / 100))
        print(f"bo_bounds quadrature K={K}: error of p {ep:.3g}, of sd {es:.3g} (units: a hundredth of the reference's standard error)")
        if ep <= 1.0 and es <= 1.0:
            good.append(K)
    assert good, "no K <= 64 is 100 times finer than the reference's 2^14 draws"
    assert bo.DEFAULT_CONFIG["gh_nodes"] == good[0]


def _fit_data(n=24, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3 * X[:, 0]) + 0.5 * X[:, 1] ** 2 + 0.05 * rng.standard_normal(n)
    return X, (y - y.mean()) / y.std(ddof=1)


def test_fit_gp_gradient_matches_central_differences():
    """h = 1e-5: truncation ~ h^2 |f'''| ~ 1e-9 and rounding ~ u |f| / h ~ 1e-9 on an MLL of order 10: 1e-6 of the gradient's norm."""
    import torch
    X, y = _fit_data()
    Xt, yt, fn = torch.as_tensor(X), torch.as_tensor(y), torch.zeros(len(X), dtype=torch.float64)
    th0 = np.array([np.log(0.4), np.log(0.7), np.log(1.1), np.log(1.3), 0.1, np.log(0.02)])
    th = torch.tensor(th0, requires_grad=True)
    mll, ok = bo._mll_torch(th, Xt, yt, fn, True, 1e-6)
    assert ok
    mll.backward()
    g = th.grad.numpy()
    num = np.zeros_like(g)
    for i in range(len(th0)):
        e = np.zeros_like(th0); e[i] = 1e-5
        num[i] = (float(bo._mll_torch(torch.tensor(th0 + e), Xt, yt, fn, True, 1e-6)[0]) -
                  float(bo._mll_torch(torch.tensor(th0 - e), Xt, yt, fn, True, 1e-6)[0])) / 2e-5
    assert np.abs(g - num).max() <= 1e-6 * np.abs(g).max()


def test_fit_gp_improves_the_likelihood_and_repeats_to_the_bit():
    X, y = _fit_data()
    h1, start, end = bo.fit_gp(X, y, return_trace=True)
    h2 = bo.fit_gp(X, y)
    assert end >= start
    assert abs(bo.gp_mll(X, y, bo.GPHyper(h1.c, h1.s, h1.ls, h1.noise - 1e-6), noise_floor=1e-6) - end) <= 1e-9 * abs(end)
    assert h1.c == h2.c and h1.s == h2.s and h1.noise == h2.noise and (h1.ls == h2.ls).all()


def test_fit_gp_refuses_a_singular_kernel_matrix():
    X, y = _fit_data(12)
    X[5] = X[2]
    with pytest.raises(bo.ModelFittingError):
        bo.fit_gp(X, y, learn_noise=False, noise_floor=0.0)


def test_front_utilities_against_brute_force(golden_dir):
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    obj = z["objectives"][z["feasible"]]
    assert obj.shape == (194, 2, 2)
    refs = np.array(bo.DEFAULT_CONFIG["reference_point_0"]), np.array(bo.DEFAULT_CONFIG["reference_point_1"])
    for g, size in ((0, 73), (1, 20)):
        Y = obj[:, g, :]
        brute = np.array([not any((Y[j] >= Y[i]).all() and (Y[j] > Y[i]).any() for j in range(len(Y))) for i in range(len(Y))])
        mask = bo.pareto_mask(Y)
        assert (mask == brute).all() and mask.sum() == size
        # hypervolume: the elementary rectangles of the grid the points span, each counted if some point dominates its centre
        r = refs[g]
        xs = np.unique(np.concatenate([[r[0]], Y[Y[:, 0] > r[0], 0]]))
        ys = np.unique(np.concatenate([[r[1]], Y[Y[:, 1] > r[1], 1]]))
        cx, cy = 0.5 * (xs[:-1] + xs[1:]), 0.5 * (ys[:-1] + ys[1:])
        dom = ((Y[:, 0][None, None, :] >= cx[:, None, None]) & (Y[:, 1][None, None, :] >= cy[None, :, None])).any(-1)
        area = (np.diff(xs)[:, None] * np.diff(ys)[None, :] * dom).sum()
        assert abs(bo.hypervolume_2d(Y, r) - area) <= 1e-12 * max(area, 1.0)
        assert bo.hypervolume_2d(Y, r) > 0


CSV = ("12.3,1.5,20.0,3.2,150.0,800.5,1500.0;0.390,0.300,0.655,0.533,0.342,0.200,0.667;-0.412,-0.530;-0.201,-0.644;1\n"
       "1.0,0.0,1.0,0.0,20.0,500.0,500.0;0.000,0.000,0.000,0.000,0.000,0.000,0.000;nan,nan;nan,nan;0\n"
       "30.0,5.0,30.0,6.0,400.0,2000.0,2000.0;1.000,1.000,1.000,1.000,1.000,1.000,1.000;-0.100,-1.250;-0.050,-0.900;1\n"
       "7.7,2.2,9.9,4.4,88.8,1234.5,678.9;0.231,0.440,0.307,0.733,0.181,0.490,0.119;-0.333,-0.444;-0.555,-0.666;1\n"
       "15.5,2.5,15.5,3.0,210.0,1250.0,1250.0;0.500,0.500,0.500,0.500,0.500,0.500,0.500;-0.250,-0.750;-0.125,-0.875;1\n")


def test_csv_round_trip():
    trials = bo.load_trials(CSV)
    assert len(trials) == 5 and [t.feasible for t in trials] == [True, False, True, True, True]
    assert np.isnan(trials[1].objectives).all() and trials[3].objectives[1, 1] == -0.666 and trials[3].params_nat[5] == 1234.5
    assert bo.store_trials(trials) == CSV
    again = bo.load_trials(bo.store_trials(trials))
    for a, b in zip(trials, again):
        assert (a.params_nat == b.params_nat).all() and (a.params_nor == b.params_nor).all() and a.feasible == b.feasible
        assert np.array_equal(a.objectives, b.objectives, equal_nan=True)


def test_appending_a_pick_equals_packing_it_into_the_baseline():
    """Appended against packed from scratch with the pick as the last baseline point. The new row of L_b left of the diagonal is the
    same triangular solve: it agrees to that solve's rounding (u times the condition of L_b). The diagonal differs by construction:
    appending takes sqrt(d2) with d2 = max(S_xx - l.l, j), the factorisation of S_bb + j I has sqrt(S_xx + j - l.l) -- the squares
    differ by the jitter, and the pick's draws by that difference times zeta."""
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=21, q=2)
    x = np.random.default_rng(1).random(7)
    app = bo.append_pick(m, x)
    obj, cls = ref.hypers(7)
    feas = np.zeros(65, dtype=bool); feas[:17] = True
    # the targets the model was packed from: a = V^T V (y - c)  ->  y = c + A a, here simply through generate's own arrays
    Ys = np.stack([m.c[o] + np.linalg.solve(m.V[o].T @ m.V[o], m.a[o]) for o in range(2)], axis=1)
    scratch = bo.pack_model(m.Xt, Ys, obj, m.Xc, feas, cls, np.vstack([m.Xb, x]), m.Zfull, m.ref, eps=m.eps, jitter=m.jitter, K=8)
    assert app.n_b == scratch.n_b == 18
    for o in range(2):
        tol = 64 * U * np.linalg.cond(scratch.L_b[o]) * np.abs(scratch.L_b[o]).max()
        assert np.abs(app.L_b[o][:17] - scratch.L_b[o][:17]).max() <= tol
        assert np.abs(app.L_b[o][17, :17] - scratch.L_b[o][17, :17]).max() <= tol
        dd = scratch.L_b[o][17, 17] ** 2 - app.L_b[o][17, 17] ** 2
        assert abs(dd - m.jitter[o]) <= tol and app.L_b[o][17, 17] ** 2 >= m.jitter[o]
        assert np.abs(app.R[o] @ app.L_b[o] - np.eye(18)).max() <= 64 * U * np.linalg.cond(app.L_b[o])
        assert np.abs(app.H[o] - scratch.H[o]).max() <= tol
        assert np.abs(app.F_b[:, :17, o] - scratch.F_b[:, :17, o]).max() <= tol * 18 * np.abs(m.Zfull).max()
        gap = abs(scratch.L_b[o][17, 17] - app.L_b[o][17, 17])
        assert np.abs(app.F_b[:, 17, o] - scratch.F_b[:, 17, o]).max() <= (gap + tol * 18) * np.abs(m.Zfull).max()
    assert (app.zeta(0) == m.Zfull[:, 18, 0]).all() and (app.Z(1)[:, 17] == m.zeta(1)).all()


def _toy_objective(infeasible_everywhere=False):
    def objective(P):
        P = np.atleast_2d(P)
        x = (P - np.array([1.0, 10.0])) / np.array([4.0, 40.0])          # back to [0,1]^2
        f0 = -((x - 0.2) ** 2).sum(1)
        f1 = -((x - 0.8) ** 2).sum(1)
        obj = np.stack([np.stack([f0, f1], 1), np.stack([f0 - 0.1, f1 + 0.05], 1)], axis=1)
        feas = np.zeros(len(P), dtype=bool) if infeasible_everywhere else (x[:, 0] + x[:, 1] < 1.4)
        return obj, feas
    return objective


CFG = dict(n_initial=10, batch_size=2, reference_point_0=[-1.5, -1.5], reference_point_1=[-1.5, -1.5], n_sobol_samples=16, n_restarts=2,
           n_raw_samples=16, max_iter=6, fit_max_iter=15, seed=1)


def test_driver_on_a_synthetic_problem():
    bounds = np.array([[1.0, 10.0], [5.0, 50.0]])
    drv = bo.BayesianOptimization(bounds, CFG, _toy_objective(), acq="host")
    drv.generate_initial_data()
    drv.evaluate_at_boundaries()
    assert len(drv.trials) == 14 and any(t.feasible for t in drv.trials) and not all(t.feasible for t in drv.trials)
    for _ in range(3):
        times = drv.perform_bayesian_optimization_step()
        assert times is not None and len(times) == 3 and all(t >= 0 for t in times)
    assert drv.groups_used == [0, 1, 0] and len(drv.trials) == 20 and drv.fallbacks == 0
    tr = np.array(drv.hv_traces)
    assert (np.diff(tr, axis=0) >= 0).all() and tr[-1].min() > 0
    for t in drv.trials:
        assert ((t.params_nor >= 0) & (t.params_nor <= 1)).all()
        assert ((t.params_nat >= bounds[0]) & (t.params_nat <= bounds[1])).all()
    for g in range(2):
        assert len(drv.pareto_trials[g]) >= 1 and all(t.feasible for t in drv.pareto_trials[g])


def test_driver_falls_back_to_sobol_without_feasible_data():
    drv = bo.BayesianOptimization(np.array([[1.0, 10.0], [5.0, 50.0]]), CFG, _toy_objective(True), acq="host")
    drv.generate_initial_data(4)
    assert drv.perform_bayesian_optimization_step() is None
    assert drv.fallbacks == 1 and len(drv.trials) == 4 + CFG["batch_size"] and drv.active_group == 0
    assert drv.hv_traces[-1] == [0.0, 0.0]
