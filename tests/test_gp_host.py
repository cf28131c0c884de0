"""
The host side of the surrogate fit on the device (tum_control_amd/bo.py gp_mll_grad_host, fit_gp's and pack_model's new keywords, the
tum_gp_ entry points): the numpy statement of the device chain against the long-double reference of tests/gp_reference.py and against
central differences, the defaults against the explicit spelling of the same thing, and the C-ABI. No GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_reference as ref          # noqa: E402
import gp_reference as gref         # noqa: E402
from test_bo_host import _fit_data  # noqa: E402
from tum_control_amd import bo      # noqa: E402

U = 2.0 ** -53
TH0 = np.array([np.log(0.4), np.log(0.7), np.log(1.1), np.log(1.3), 0.1, np.log(0.02)])


def test_cabi_exports_every_declared_gp_symbol():
    """The built library exports every tum_gp_ function include/tum_nmpc.h declares, and solver.GP_SYMBOLS lists exactly those."""
    import re
    import __graft_entry__ as g
    from tum_control_amd import solver
    g.build()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tum_nmpc.h")).read()
    declared = sorted(set(re.findall(r"\b(tum_gp_\w+)\s*\(", hdr)))
    assert len(declared) == 6 and sorted(solver.GP_SYMBOLS) == declared
    L = solver.load_library()
    for sym in declared:
        assert hasattr(L, sym), sym


def _theta(d, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.log(0.4 + 0.8 * rng.random(d)), [np.log(1.3), 0.1, np.log(0.02)]])


@pytest.mark.parametrize("n,d,cls,learn", [(1, 1, False, True), (5, 7, False, True), (24, 3, False, True), (24, 3, True, True),
                                          (65, 16, True, False), (130, 7, True, True)])
def test_host_statement_against_long_double(n, d, cls, learn):
    """Gate of tests/test_gpu_gp.py with the roles turned: the numpy statement is held to 4 x the error of torch's autograd (the other
    FP64 statement), floor 32, in units of u x scale."""
    X, y = gref.fit_data(n, d, seed=n + d)
    fixed = None
    if cls:
        flags = np.zeros(n, dtype=bool); flags[::10] = True
        t, f = bo.dirichlet_targets(flags)
        y, fixed = t[:, 1], f[:, 1]
    th = _theta(d, n)
    want = gref.mll_grad(X, y, th, fixed, learn, 1e-6)
    mll, grad, ok = bo.gp_mll_grad_host(X, y, th, fixed, learn, 1e-6)
    assert ok
    e_host = gref.errors(mll, grad, want)
    e_torch = gref.errors(*gref.torch_mll_grad(X, y, th, fixed, learn, 1e-6)[:2], want)
    print(f"gp_bounds host n={n} d={d} class={cls} learn={learn}: host {e_host[0]:.1f} {e_host[1]:.1f} torch {e_torch[0]:.1f} {e_torch[1]:.1f}")
    for i in range(2):
        assert e_host[i] <= max(4.0 * e_torch[i], 32.0), (i, e_host, e_torch)
    if not learn:
        assert grad[-1] == 0.0


def test_host_gradient_matches_central_differences():
    """h = 1e-5, 1e-6 of the gradient's largest component: the bound test_fit_gp_gradient_matches_central_differences derives."""
    X, y = _fit_data()
    _, g, ok = bo.gp_mll_grad_host(X, y, TH0, None, True, 1e-6)
    assert ok
    num = np.zeros_like(g)
    for i in range(len(TH0)):
        e = np.zeros_like(TH0); e[i] = 1e-5

        def f(th):
            return bo.gp_mll(X, y, bo.GPHyper(c=th[4], s=np.exp(th[3]), ls=np.exp(th[:3]), noise=np.exp(th[5])), noise_floor=1e-6)
        num[i] = (f(TH0 + e) - f(TH0 - e)) / 2e-5
    assert np.abs(g - num).max() <= 1e-6 * np.abs(g).max()


def test_host_statement_reports_a_singular_matrix():
    X, y = _fit_data(12)
    X[5] = X[2]
    th = np.concatenate([np.log(np.full(3, 0.5)), [0.0, 0.0, np.log(1e-2)]])
    assert not bo.gp_mll_grad_host(X, y, th, None, False, 0.0)[2]


def test_block_wise_reference_equals_the_whole_matrix_reference():
    """Clustered data (gp_reference.clustered_data): the sums and concatenations of the clusters' long-double results against the
    long-double results of the whole matrix, within 1 u x scale (both are long double: 2^-11 u per operation; measured 0.001 u for
    the MLL and 0.04 u for the gradient). V is exactly 0 outside the clusters' blocks in both."""
    sizes, d = (37, 70, 23), 3
    LDT = np.longdouble
    for noise, learn in ((False, True), (True, True), (True, False)):
        X, y, fixed = gref.clustered_data(sizes, d, seed=11, noise=noise)
        th = np.concatenate([np.log([0.5, 0.9, 1.2]), [np.log(1.3), 0.1, np.log(0.02)]])
        whole = gref.mll_grad(X, y, th, fixed, learn, 1e-6)
        block = gref.block_mll_grad(sizes, X, y, th, fixed, learn, 1e-6)
        e = gref.errors(block[0], block[1], whole)
        print(f"gp_bounds block-wise against whole noise={noise} learn={learn}: mll {e[0]:.4f} grad {e[1]:.4f} (u x scale)")
        assert e[0] <= 1.0 and e[1] <= 1.0
        assert abs(block[2] - whole[2]) <= 1e-12 * whole[2] and abs(block[3] - whole[3]) <= 1e-12 * whole[3]
        hyp = bo.GPHyper(c=0.1, s=1.3, ls=np.exp(th[:d]), noise=0.05 if fixed is None else fixed + 0.05)
        Vw, aw = gref.factor(X, y, hyp)
        Vb, ab = gref.block_factor(sizes, X, y, hyp)
        assert Vb.dtype == LDT and ab.dtype == LDT
        assert float(np.abs(Vw - Vb).max()) <= U * float(np.abs(Vw).max()) and float(np.abs(aw - ab).max()) <= U * float(np.abs(aw).max())
        inside = np.zeros((len(X), len(X)), dtype=bool)
        for b in gref._blocks(sizes):
            inside[b, b] = True
        assert (Vb[~inside] == 0).all() and (Vw[~inside] == 0).all() and (np.tril(Vb)[inside] != 0).sum() == sum(s * (s + 1) // 2 for s in sizes)
    with pytest.raises(AssertionError):
        gref.clustered_data((64, 70), d, seed=0)          # (a cluster that ends on a tile edge)
    for n in (1409, 4033, 4096):
        assert sum(gref.cluster_sizes(n)) == n
        gref.clustered_data(gref.cluster_sizes(n), 1, seed=0)


def test_campaign_fixture_reloads_and_belongs_to_the_data(golden_dir):
    """tests/golden/gp_campaign.npz (make_gp_golden.py): the split long doubles join exactly, and the stored MLL of every (class,
    theta) is the MLL bo.gp_mll_grad_host gives on the 2050 trials within 1e-9 relative -- a check that the fixture belongs to the
    data, not a bound on the host statement."""
    z = np.load(os.path.join(golden_dir, "gp_campaign.npz"))
    t = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn = t["params_nor"]
    targets, fixed = bo.dirichlet_targets(t["feasible"])
    assert Xn.shape == (2050, 7) and list(z["rows"]) == [63, 64, 1023, 1024, 2047, 2048, 2049]
    for k in range(2):
        for e in range(2):
            tag = f"{k}_{e}"
            th = z["theta_" + tag]
            mll = gref.join(z[f"mll_{tag}_hi"], z[f"mll_{tag}_lo"])
            grad, a, V = (gref.join(z[f"{q}_{tag}_hi"], z[f"{q}_{tag}_lo"]) for q in ("grad", "a", "V"))
            assert th.shape == (10,) and grad.shape == (10,) and a.shape == (2050,) and V.shape == (7, 2050) and z["scale_" + tag].shape == (2,)
            assert mll.dtype == np.longdouble and float(mll) == float(z[f"mll_{tag}_hi"]) and np.isfinite(V.astype(np.float64)).all()
            for i, r in enumerate(z["rows"]):
                assert (V[i, r + 1:] == 0).all() and V[i, r] > 0
            assert float(np.abs(grad).max()) == z["scale_" + tag][1] and float(np.abs(V).max()) <= float(z["vmax_" + tag])
            hm, _, ok = bo.gp_mll_grad_host(Xn, targets[:, k], th, fixed[:, k], True, float(z["noise_floor"]))
            assert ok and abs(hm - float(mll)) <= 1e-9 * abs(float(mll)), (tag, hm, float(mll))
        assert not (z[f"theta_{k}_0"] == z[f"theta_{k}_1"]).all()


def test_defaults_return_what_the_explicit_keywords_return():
    """fit_gp without the keyword against backend="torch", pack_model without it against factor=bo.gp_factor: equal to the bit."""
    X, y = _fit_data()
    h1, s1, e1 = bo.fit_gp(X, y, return_trace=True)
    h2, s2, e2 = bo.fit_gp(X, y, return_trace=True, backend="torch")
    assert (s1, e1, h1.c, h1.s, h1.noise) == (s2, e2, h2.c, h2.s, h2.noise) and (h1.ls == h2.ls).all()
    with pytest.raises(ValueError):
        bo.fit_gp(X, y, backend="hip")
    m1 = ref.generate(7, 17, 17, 65, 16, 8, seed=21)
    rng = np.random.default_rng(21)
    Xc = rng.random((65, 7))          # (generate's own draws, spelled out for the explicit call)
    feas = np.zeros(65, dtype=bool); feas[:17] = True
    Xt = Xc[:17]
    Y = np.stack([-((Xt - 0.3) ** 2).sum(1), -((Xt - 0.7) ** 2).sum(1)], axis=1) * (4.0 / 7) + 0.05 * rng.standard_normal((17, 2))
    Z = bo.sobol_normal(16, 2 * (17 + 2), 21).reshape(16, 2, -1).transpose(0, 2, 1)
    obj, cls = ref.hypers(7)
    m2 = bo.pack_model(Xt, bo.standardize(Y)[0], obj, Xc, feas, cls, Xt, Z, np.array((-1.5, -1.5)), eps=0.8, jitter=1e-6, K=8, factor=bo.gp_factor)
    for g in range(4):
        assert (m1.V[g] == m2.V[g]).all() and (m1.a[g] == m2.a[g]).all()
    for o in range(2):
        assert (m1.H[o] == m2.H[o]).all() and (m1.R[o] == m2.R[o]).all()
    assert (m1.fronts == m2.fronts).all() and (m1.front_count == m2.front_count).all()
    calls = []

    def counting(X, y, hyp):
        calls.append(len(X))
        return bo.gp_factor(X, y, hyp)
    m3 = bo.pack_model(Xt, bo.standardize(Y)[0], obj, Xc, feas, cls, Xt, Z, np.array((-1.5, -1.5)), eps=0.8, jitter=1e-6, K=8, factor=counting)
    assert calls == [17, 17, 65, 65] and (m3.fronts == m1.fronts).all()


def test_driver_refuses_an_unknown_fit_backend():
    with pytest.raises(ValueError):
        bo.BayesianOptimization(np.array([[0.0], [1.0]]), {}, lambda P: None, acq="host", fit_backend="hip")
