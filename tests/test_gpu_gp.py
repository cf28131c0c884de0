"""
The surrogate fit's objective on the device (csrc/gp_kernels.hpp behind tum_gp_mll / tum_gp_factor, bo.DeviceGP) against the
long-double reference of tests/gp_reference.py.

Gate: errors of the MLL and of every gradient component are measured against the long-double value in units of u = 2^-53 times
scale_mll = 1/2 r^T A^-1 r + |sum log L_ii| + 1/2 n log 2 pi and scale_grad = the gradient's largest |component|. The gate of a
quantity is 4 x the larger of the errors of bo.gp_mll_grad_host and of bo._mll_torch with autograd on the CPU (two FP64 statements of
the same sums in other orders), with a floor of 32 -- the standing choice of tests/test_gpu_bo.py. It is measured per case from the
two FP64 references, never from the device, so it scales with the conditioning of the case by itself. The factor (V, a) is held the
same way against the long-double L^-1 and A^-1 r, its FP64 references being bo.gp_factor and torch's cholesky + solve_triangular,
its scale the largest |entry|. The lines the module prints with the prefix gp_bounds are kept in profiles/gp_bounds.txt.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_reference as ref                              # noqa: E402
import gp_reference as gref                             # noqa: E402
from test_bo_host import CFG, _fit_data, _toy_objective  # noqa: E402
from tum_control_amd import bo                          # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
NB = 64          # GP_NB of csrc/gp_kernels.hpp


@pytest.fixture(scope="module")
def gp():
    g = bo.DeviceGP()
    yield g
    g.close()


def _case(n, d, kind, seed=None):
    """Data and hyperparameters of one GP. kind "obj": no fixed noise, a learned one; "cls": the class-1 GP of the Dirichlet
    classification on a 10 % feasible flag vector, with its fixed noise; "fix": as "obj" with learn_noise off."""
    X, y = gref.fit_data(n, d, seed=n + d if seed is None else seed)
    rng = np.random.default_rng(1000 + n + d)
    ls = 0.4 + 0.8 * rng.random(d)
    if kind == "cls":
        flags = np.zeros(n, dtype=bool); flags[::10] = True
        t, f = bo.dirichlet_targets(flags)
        return X, t[:, 1], f[:, 1], np.concatenate([np.log(ls), [np.log(12.0), -3.0, np.log(0.1)]]), True
    return X, y, None, np.concatenate([np.log(ls), [np.log(1.3), 0.1, np.log(0.02)]]), kind == "obj"


def _gate(gp, X, y, fixed, th, learn, floor, label, want=None):
    """want: the long-double (mll, grad, scale_mll, scale_grad) where it does not come from the whole matrix here."""
    want = gref.mll_grad(X, y, th, fixed, learn, floor) if want is None else want
    gp.set_data(X, y, fixed)
    mll, grad, ok = gp.mll_grad(th, learn, floor)
    e_dev = gref.errors(mll, grad, want)
    hm, hg, hok = bo.gp_mll_grad_host(X, y, th, fixed, learn, floor)
    e_host = gref.errors(hm, hg, want)
    tm, tg, tok = gref.torch_mll_grad(X, y, th, fixed, learn, floor)
    e_torch = gref.errors(tm, tg, want)
    gate = [max(32.0, 4.0 * max(e_host[i], e_torch[i])) for i in range(2)]
    for i, name in enumerate(("mll", "grad")):
        print(f"gp_bounds {label} {name}: device {e_dev[i]:.2f} host {e_host[i]:.2f} torch {e_torch[i]:.2f} gate {gate[i]:.2f} "
              f"share {e_dev[i] / gate[i]:.3f} (u x scale)")
    assert ok and hok and tok
    assert np.isfinite(grad).all() and len(grad) == X.shape[1] + 3
    for i in range(2):
        assert e_dev[i] <= gate[i], (label, i, e_dev[i], gate[i])
    if not learn:
        assert grad[-1] == 0.0
    return mll, grad


# every block edge of the factorisation (NB = 64), every d, both kinds of GP; the last size has three block columns behind the first
CASES = [(1, 1, "obj"), (1, 7, "cls"), (5, 7, "obj"), (5, 16, "cls"), (NB - 1, 16, "obj"), (NB - 1, 1, "cls"), (NB, 7, "obj"), (NB, 1, "cls"),
         (NB + 1, 7, "cls"), (NB + 1, 16, "obj"), (2 * NB + 2, 7, "obj"), (2 * NB + 2, 1, "cls"), (2 * NB + 2, 16, "fix"),
         (3 * NB + 8, 2, "cls"), (3 * NB + 8, 7, "obj"), (3 * NB + 8, 16, "cls"), (3 * NB + 8, 1, "fix")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_d%d_%s" % c)
def test_mll_and_gradient_against_long_double(gp, case):
    n, d, kind = case
    X, y, fixed, th, learn = _case(n, d, kind)
    _gate(gp, X, y, fixed, th, learn, 1e-6, "n=%d d=%d %s" % case)


def test_real_shape_first_300_trials(gp, golden_dir):
    """Both class GPs on all 300 trials and both objective GPs on the feasible ones, at fit_gp's initial hyperparameters."""
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"][:300], z["feasible"][:300], z["objectives"][:300]
    Xt = Xn[feas]
    assert 40 <= len(Xt) <= 80
    Ys = bo.standardize(obj[feas][:, 0, :])[0]
    for o in range(2):
        y = Ys[:, o]
        th = np.concatenate([np.log(np.full(7, 0.5)), [np.log(max(float(np.var(y, ddof=1)), 1e-3)), float(y.mean()), np.log(1e-2)]])
        _gate(gp, Xt, y, None, th, True, 1e-6, "fixture[:300] objective %d n=%d" % (o, len(Xt)))
    targets, fixed = bo.dirichlet_targets(feas)
    for k in range(2):
        th = np.concatenate([np.log(np.full(7, 0.5)), [np.log(max(float(np.var(targets[:, k])), 1.0)), 1.0, np.log(1e-2)]])
        _gate(gp, Xn, targets[:, k], fixed[:, k], th, True, 1e-6, "fixture[:300] class %d n=300" % k)


def _factor_gate(V, a, X, y, hyp, Vl, al, label, rows=None, vmax=None):
    """The gate of the factor: (V, a) of the device against the long-double (Vl, al); rows: Vl holds these rows of L^-1 only, vmax
    is then the largest |entry| of the whole of it."""
    def errors(V, a):
        V = V if rows is None else V[list(rows)]
        return (float(np.abs(np.asarray(V, dtype=LD) - Vl).max() / (U * (float(np.abs(Vl).max()) if vmax is None else vmax))),
                float(np.abs(np.asarray(a, dtype=LD) - al).max() / (U * float(np.abs(al).max()))))
    e_dev = errors(V, a)
    e_host = errors(*bo.gp_factor(X, y, hyp))
    e_torch = errors(*gref.torch_factor(X, y, hyp))
    for i, name in enumerate(("V", "a")):
        gate = max(32.0, 4.0 * max(e_host[i], e_torch[i]))
        print(f"gp_bounds factor {label} {name}: device {e_dev[i]:.2f} host {e_host[i]:.2f} torch {e_torch[i]:.2f} gate {gate:.2f} "
              f"share {e_dev[i] / gate:.3f} (u x scale)")
        assert e_dev[i] <= gate, (name, e_dev[i], gate)


@pytest.mark.parametrize("n,d,kind", [(5, 7, "obj"), (NB + 1, 7, "cls"), (3 * NB + 8, 7, "obj"), (3 * NB + 8, 2, "cls")])
def test_factor_against_long_double(gp, n, d, kind):
    X, y, fixed, _, _ = _case(n, d, kind)
    o_h, c_h = ref.hypers(d)
    hyp = o_h[0] if kind == "obj" else bo.GPHyper(c=c_h[1].c, s=c_h[1].s, ls=c_h[1].ls, noise=fixed + c_h[1].noise)
    Vl, al = gref.factor(X, y, hyp)
    V, a = gp.gp_factor(X, y, hyp)
    assert V.shape == (n, n) and (np.triu(V, 1) == 0.0).all() and (np.diag(V) > 0).all()
    _factor_gate(V, a, X, y, hyp, Vl, al, f"n={n} d={d} {kind}")
    # factor(hyp) on data with a fixed noise adds the scalar of hyp to it: the same matrix, the same bits
    if kind == "cls":
        gp.set_data(X, y, fixed)
        V2, a2 = gp.factor(bo.GPHyper(c=hyp.c, s=hyp.s, ls=hyp.ls, noise=0.0))
        gp.set_data(X, y, fixed + c_h[1].noise)
        V3, a3 = gp.factor(bo.GPHyper(c=hyp.c, s=hyp.s, ls=hyp.ls, noise=0.0))
        assert (V3 == V).all() and (a3 == a).all() and V2.shape == V.shape and np.isfinite(a2).all()


def test_packed_model_with_device_factors_against_long_double(gp):
    """pack_model(factor=device) then host_acquisition, against the long-double acquisition, in the units and by the gate of
    tests/test_gpu_bo.py. The reference model is packed from the long-double factors (rounded to FP64), so no FP64 factor is the
    truth; the two FP64 routes the gate is measured from are pack_model's default (bo.gp_factor) under bo.host_acquisition and
    torch's factor under bo_reference.torch_acquisition: both carry their factor's rounding, as the device route does."""
    from test_gpu_bo import NAMES, _errors
    d, n_t, n_b, n_c, S, K, seed = 7, 37, 33, 130, 64, 8, 41
    rng = np.random.default_rng(seed)          # (bo_reference.generate's draws, spelled out to pass factor=)
    Xc = rng.random((n_c, d))
    feas = np.zeros(n_c, dtype=bool); feas[:n_t] = True
    Xt = Xc[:n_t]
    Y = np.stack([-((Xt - 0.3) ** 2).sum(1), -((Xt - 0.7) ** 2).sum(1)], axis=1) * (4.0 / d) + 0.05 * rng.standard_normal((n_t, 2))
    Z = bo.sobol_normal(S, 2 * (n_b + 2), seed).reshape(S, 2, -1).transpose(0, 2, 1)
    obj, cls = ref.hypers(d)

    def pack(factor):
        return bo.pack_model(Xt, bo.standardize(Y)[0], obj, Xc, feas, cls, Xt[:n_b], Z, np.array((-1.5, -1.5)), eps=0.8, jitter=1e-6, K=K, factor=factor)

    def exact(X, y, hyp):
        V, a = gref.factor(X, y, hyp)
        return np.asarray(V, dtype=np.float64), np.asarray(a, dtype=np.float64)
    m_ref, m_host, m_torch, m_dev = pack(exact), pack(None), pack(gref.torch_factor), pack(gp.gp_factor)
    Xq = np.random.default_rng(seed + 1).random((40, d))
    ld_alpha, ld_det = ref.longdouble_acquisition(m_ref, Xq)
    e_dev = _errors(m_ref, *bo.host_acquisition(m_dev, Xq, detail=True), ld_alpha, ld_det)
    e_host = _errors(m_ref, *bo.host_acquisition(m_host, Xq, detail=True), ld_alpha, ld_det)
    e_torch = _errors(m_ref, *ref.torch_acquisition(m_torch, Xq), ld_alpha, ld_det)
    gate = np.maximum(32.0, 4.0 * np.maximum(e_host, e_torch))
    for i, name in enumerate(NAMES):
        print(f"gp_bounds packed model {name}: device {e_dev[i]:.2f} host {e_host[i]:.2f} torch {e_torch[i]:.2f} gate {gate[i]:.2f} "
              f"share {e_dev[i] / gate[i]:.3f} (u x scale)")
    for i, name in enumerate(NAMES):
        assert e_dev[i] <= gate[i], (name, e_dev[i], gate[i])


def test_same_call_same_bits_and_nothing_stale(gp):
    Xb, yb, fb, thb, lb = _case(3 * NB + 8, 7, "cls")
    Xs, ys, fs, ths, ls_ = _case(5, 7, "obj")
    gp.set_data(Xb, yb, fb)
    big = gp.mll_grad(thb, lb, 1e-6)
    again = gp.mll_grad(thb, lb, 1e-6)
    assert big[0] == again[0] and (big[1] == again[1]).all() and big[2] and again[2]
    assert gp.mll_grad(thb, lb, 1e-6, grad=False)[0] == big[0]          # the value alone: the same bits
    gp.set_data(Xs, ys, fs)
    small = gp.mll_grad(ths, ls_, 1e-6)
    small_v = gp.factor(bo.GPHyper(c=0.1, s=1.3, ls=np.exp(ths[:7]), noise=0.05))
    fresh = bo.DeviceGP()
    try:
        fresh.set_data(Xs, ys, fs)
        new = fresh.mll_grad(ths, ls_, 1e-6)
        new_v = fresh.factor(bo.GPHyper(c=0.1, s=1.3, ls=np.exp(ths[:7]), noise=0.05))
    finally:
        fresh.close()
    assert small[0] == new[0] and (small[1] == new[1]).all() and small[2] and new[2]
    assert (small_v[0] == new_v[0]).all() and (small_v[1] == new_v[1]).all()


def _singular():
    X, y = _fit_data(12)
    X[5] = X[2]
    th = np.concatenate([np.log(np.full(3, 0.5)), [np.log(max(float(np.var(y, ddof=1)), 1e-3)), float(y.mean()), np.log(1e-2)]])
    return X, y, th


def test_a_matrix_that_is_not_positive_definite_is_a_result(gp):
    X, y, th = _singular()
    gp.set_data(X, y)
    mll, grad, ok = gp.mll_grad(th, False, 0.0)          # (returns: the call itself did not fail)
    assert not ok and np.isfinite(mll) and np.isfinite(grad).all()
    mll2, _, ok2 = gp.mll_grad(th, False, 0.0, grad=False)
    assert not ok2 and np.isfinite(mll2)
    with pytest.raises(bo.ModelFittingError):
        gp.factor(bo.GPHyper(c=th[4], s=np.exp(th[3]), ls=np.exp(th[:3]), noise=0.0))
    with pytest.raises(bo.ModelFittingError):
        bo.fit_gp(X, y, learn_noise=False, noise_floor=0.0, backend="device", gp=gp)
    with pytest.raises(bo.ModelFittingError):
        bo.fit_gp(X, y, learn_noise=False, noise_floor=0.0)
    # sound data on the same handle: the bits of a fresh handle
    Xs, ys, fs, ths, ls_ = _case(NB + 1, 7, "obj")
    gp.set_data(Xs, ys, fs)
    after = gp.mll_grad(ths, ls_, 1e-6)
    fresh = bo.DeviceGP()
    try:
        fresh.set_data(Xs, ys, fs)
        new = fresh.mll_grad(ths, ls_, 1e-6)
    finally:
        fresh.close()
    assert after[2] and after[0] == new[0] and (after[1] == new[1]).all()


def test_fit_on_the_device(gp):
    """end >= start; a second fit repeats to the bit; gp_mll on the CPU at the fitted theta agrees with the reported end to 1e-9 |end|
    (the bound tests/test_bo_host.py uses for the same comparison); and the device fit ends no lower than torch's on the CPU less
    g = max(4 |end_torch_gpu - end_torch_cpu|, 1e-9 |end_torch_cpu|): the spread of the same algorithm between two FP64 executions."""
    X, y = _fit_data()
    h1, start, end = bo.fit_gp(X, y, return_trace=True, backend="device", gp=gp)
    h2 = bo.fit_gp(X, y, backend="device", gp=gp)
    _, _, end_cpu = bo.fit_gp(X, y, return_trace=True)
    _, _, end_gpu = bo.fit_gp(X, y, return_trace=True, device="cuda")
    g = max(4.0 * abs(end_gpu - end_cpu), 1e-9 * abs(end_cpu))
    print(f"gp_bounds fit n=24 d=3: start {start!r} end device {end!r} torch cpu {end_cpu!r} torch gpu {end_gpu!r} g {g:.3e}")
    assert end >= start
    assert h1.c == h2.c and h1.s == h2.s and h1.noise == h2.noise and (h1.ls == h2.ls).all()
    assert abs(bo.gp_mll(X, y, bo.GPHyper(h1.c, h1.s, h1.ls, h1.noise - 1e-6), noise_floor=1e-6) - end) <= 1e-9 * abs(end)
    assert end >= end_cpu - g


def test_driver_fits_on_the_device():
    bounds = np.array([[1.0, 10.0], [5.0, 50.0]])
    drv = bo.BayesianOptimization(bounds, CFG, _toy_objective(), acq="host", fit_backend="device")
    drv.generate_initial_data()
    drv.evaluate_at_boundaries()
    for _ in range(2):
        assert drv.perform_bayesian_optimization_step() is not None
    assert drv.fallbacks == 0 and len(drv.trials) == 18 and drv.groups_used == [0, 1]
    tr = np.array(drv.hv_traces)
    assert (np.diff(tr, axis=0) >= 0).all() and tr[-1].min() > 0
    drv._gp.close()


def test_refusals():
    from tum_control_amd import solver
    L = solver.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    g = bo.DeviceGP()
    try:
        X, y = _fit_data()
        th = np.concatenate([np.log(np.full(3, 0.5)), [0.0, 0.0, np.log(1e-2)]])
        with pytest.raises(Exception, match="no data"):
            g.mll_grad(th)
        mll, ok = ctypes.c_double(), ctypes.c_int()
        out = np.zeros(24 * 24)
        assert L.tum_gp_factor(g._h, th.ctypes.data_as(dp), 1, 0.0, out.ctypes.data_as(dp), out.ctypes.data_as(dp), ctypes.byref(ok)) != 0
        assert b"no data" in L.tum_ocp_last_error()
        for args in ((None, X.ctypes.data_as(dp), y.ctypes.data_as(dp)), (g._h, None, y.ctypes.data_as(dp)), (g._h, X.ctypes.data_as(dp), None)):
            assert L.tum_gp_data(*args, None, 24, 3) != 0 and b"null" in L.tum_ocp_last_error()
        with pytest.raises(Exception, match="n outside"):
            g.set_data(np.zeros((4097, 1)), np.zeros(4097))
        with pytest.raises(Exception, match="n outside"):
            g.set_data(np.zeros((0, 3)), np.zeros(0))
        with pytest.raises(Exception, match="d outside"):
            g.set_data(np.zeros((4, 17)), np.zeros(4))
        for bad in ("X", "y", "noise"):
            Xb, yb, fb = X.copy(), y.copy(), np.full(24, 0.1)
            {"X": Xb, "y": yb, "noise": fb}[bad][7] = np.nan if bad != "y" else np.inf
            with pytest.raises(Exception, match="NaN"):
                g.set_data(Xb, yb, fb)
            with pytest.raises(Exception, match="no data"):          # refused data leave none behind
                g.mll_grad(th)
        g.set_data(X, y)
        for i in (0, 3, 5):
            t = th.copy(); t[i] = np.nan
            with pytest.raises(Exception, match="NaN"):
                g.mll_grad(t)
        with pytest.raises(Exception, match="NaN"):
            g.mll_grad(th, True, np.inf)
        with pytest.raises(Exception, match="d \\+ 3"):
            g.mll_grad(th[:-1])
        assert L.tum_gp_mll(g._h, None, 1, 0.0, ctypes.byref(mll), None, ctypes.byref(ok)) != 0 and b"null" in L.tum_ocp_last_error()
        assert L.tum_gp_mll(g._h, th.ctypes.data_as(dp), 1, 0.0, None, None, ctypes.byref(ok)) != 0 and b"null" in L.tum_ocp_last_error()
        assert L.tum_gp_factor(g._h, th.ctypes.data_as(dp), 1, 0.0, None, out.ctypes.data_as(dp), ctypes.byref(ok)) != 0
        assert L.tum_gp_profile(None, 1, None) != 0
        m, gr, okk = g.mll_grad(th, True, 1e-6)
        assert okk and np.isfinite(m) and np.isfinite(gr).all()
    finally:
        g.close()


def test_handle_lifetime():
    X, y, f, th, learn = _case(3 * NB + 8, 7, "cls")
    Xs, ys = _fit_data()
    ths = np.concatenate([np.log(np.full(3, 0.5)), [0.0, 0.0, np.log(1e-2)]])
    first = []
    for _ in range(10):
        g = bo.DeviceGP()
        g.set_data(Xs, ys)
        first.append(g.mll_grad(ths, True, 1e-6))
        g.close()
        g.close()
    assert all(r[0] == first[0][0] and (r[1] == first[0][1]).all() for r in first)
    a, b = bo.DeviceGP(), bo.DeviceGP()
    try:
        a.set_data(Xs, ys); b.set_data(X, y, f)
        vb = b.mll_grad(th, learn, 1e-6)
        b.close()          # straight behind its last call: the free waits for the handle's stream
        va = a.mll_grad(ths, True, 1e-6)
        assert va[0] == first[0][0] and (va[1] == first[0][1]).all() and vb[2]
        ms = a.profile(True)
        a.mll_grad(ths, True, 1e-6)
        ms = a.profile(False)
        assert ms.shape == (7,) and (ms >= 0).all() and ms.sum() > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ at the sizes a campaign runs at
# gp_reduce_kernel's threads take a second element from n = 257 and a second tile from nb = 23 (n >= 1409); the logged campaign has
# n = 2050 (33 block columns), the entry points take n = 4096 (64 block columns, no padded row). The whole-matrix long-double
# reference is cubic (minutes at these sizes), so the truth is either block-wise (gp_reference.clustered_data: A is block diagonal,
# exactly) or recorded (tests/golden/gp_campaign.npz).
def _same(a, b):
    return a[2] and b[2] and a[0] == b[0] and (a[1] == b[1]).all()


def _fresh(X, y, fixed, th, learn, floor=1e-6):
    g = bo.DeviceGP()
    try:
        g.set_data(X, y, fixed)
        return g.mll_grad(th, learn, floor)
    finally:
        g.close()


@pytest.mark.parametrize("case", [(257, 7, "obj"), (257, 1, "cls"), (449, 16, "cls"), (449, 2, "fix")], ids=lambda c: "n%d_d%d_%s" % c)
def test_second_trip_of_the_n_loop_against_long_double(gp, case):
    """257: the first n at which a thread of gp_reduce_kernel sums two elements; 449 = 7 x 64 + 1."""
    n, d, kind = case
    X, y, fixed, th, learn = _case(n, d, kind)
    _gate(gp, X, y, fixed, th, learn, 1e-6, "n=%d d=%d %s" % case)


_CLUSTERED = {}


def _clustered(n, d, kind):
    """(sizes, X, y, fixed, theta, learn) of clustered data; "cls": the class-1 targets of a 10 % feasible flag vector, their fixed
    noise plus a per-point one. Length scales 0.4 .. 1.2 as in _case."""
    if (n, d, kind) not in _CLUSTERED:
        sizes = gref.cluster_sizes(n)
        X, y, noise = gref.clustered_data(sizes, d, seed=n + d, noise=kind == "cls")
        ls = 0.4 + 0.8 * np.random.default_rng(1000 + n + d).random(d)
        if kind == "cls":
            flags = np.zeros(n, dtype=bool); flags[::10] = True
            t, f = bo.dirichlet_targets(flags)
            y, fixed, tail = t[:, 1], f[:, 1] + noise, [np.log(12.0), -3.0, np.log(0.1)]
        else:
            fixed, tail = None, [np.log(1.3), 0.1, np.log(0.02)]
        _CLUSTERED[n, d, kind] = (sizes, X, y, fixed, np.concatenate([np.log(ls), tail]), True)
    return _CLUSTERED[n, d, kind]


@pytest.mark.parametrize("case", [(1409, 7, "obj"), (4033, 2, "cls"), (4096, 7, "obj")], ids=lambda c: "n%d_d%d_%s" % c)
def test_clustered_data_against_block_wise_long_double(gp, case):
    """1409: 23 block columns, 276 tiles, the first size with a second trip of gp_reduce_kernel's tile loop. 4033 = 63 x 64 + 1: one
    live row in the last block row, a per-point fixed noise. 4096: the limit, no padded row, 2080 tiles (the slowest case of the
    module: the two FP64 statements of the gate take about 10 s of it)."""
    n, d, kind = case
    sizes, X, y, fixed, th, learn = _clustered(n, d, kind)
    want = gref.block_mll_grad(sizes, X, y, th, fixed, learn, 1e-6)
    _gate(gp, X, y, fixed, th, learn, 1e-6, "clustered n=%d d=%d %s" % case, want=want)


@pytest.mark.parametrize("n", [1409, 4096])
def test_factor_at_size_against_block_wise_long_double(gp, n):
    sizes, X, y, _, _, _ = _clustered(n, 7, "obj")
    hyp = ref.hypers(7)[0][0]
    Vl, al = gref.block_factor(sizes, X, y, hyp)
    V, a = gp.gp_factor(X, y, hyp)
    assert V.shape == (n, n) and (np.triu(V, 1) == 0.0).all() and (np.diag(V) > 0).all()
    assert (V[Vl == 0] == 0.0).all()          # (a tile index off by one brings live numbers between the clusters)
    _factor_gate(V, a, X, y, hyp, Vl, al, f"clustered n={n} d=7 obj")


@pytest.fixture(scope="module")
def campaign(golden_dir):
    """The logged campaign's class GPs on all 2050 trials and their recorded long-double truth (tests/golden/make_gp_golden.py)."""
    t = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    targets, fixed = bo.dirichlet_targets(t["feasible"])
    return t["params_nor"], targets, fixed, np.load(os.path.join(golden_dir, "gp_campaign.npz"))


def _entry(z, k, e):
    tag = f"{k}_{e}"
    j = lambda name: gref.join(z[f"{name}_{tag}_hi"], z[f"{name}_{tag}_lo"])          # noqa: E731
    return z["theta_" + tag], (j("mll"), j("grad"), float(z["scale_" + tag][0]), float(z["scale_" + tag][1])), j("V"), j("a"), float(z["vmax_" + tag])


@pytest.mark.parametrize("k,e", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=lambda v: str(v))
def test_campaign_class_gps_against_recorded_long_double(gp, campaign, k, e):
    """Class k at theta e (0: where the fit starts, 1: where the CPU fit ends) on all 2050 trials: 33 block columns, 561 tiles. The
    likelihood and its gradient, then the factor at the same theta: a and the recorded rows of V."""
    Xn, targets, fixed, z = campaign
    th, want, Vl, al, vmax = _entry(z, k, e)
    floor = float(z["noise_floor"])
    _gate(gp, Xn, targets[:, k], fixed[:, k], th, True, floor, f"campaign n=2050 class {k} theta {e}", want=want)
    hyp = bo.GPHyper(c=float(th[8]), s=float(np.exp(th[7])), ls=np.exp(th[:7]), noise=floor + float(np.exp(th[9])))
    V, a = gp.factor(hyp)          # (raises where ok is 0)
    assert (np.triu(V, 1) == 0.0).all() and (np.diag(V) > 0).all()
    _factor_gate(V, a, Xn, targets[:, k], bo.GPHyper(c=hyp.c, s=hyp.s, ls=hyp.ls, noise=fixed[:, k] + hyp.noise), Vl, al,
                 f"campaign n=2050 class {k} theta {e}", rows=z["rows"], vmax=vmax)


def test_a_pivot_that_fails_in_a_later_block_column_is_a_result(gp):
    """A repeated trial at row 300 (block column 4) without any noise: the bad pivot appears after gp_trsm_kernel and gp_syrk_kernel
    have run over four columns. The kernels' contract is finite numbers and ok = 0."""
    n, d = 321, 3
    X, y = gref.fit_data(n, d)
    X[300] = X[70]
    th = np.concatenate([np.log(np.full(d, 0.5)), [np.log(max(float(np.var(y, ddof=1)), 1e-3)), float(y.mean()), np.log(1e-2)]])
    gp.set_data(X, y)
    mll, grad, ok = gp.mll_grad(th, False, 0.0)
    assert not ok and np.isfinite(mll) and np.isfinite(grad).all()
    mll2, _, ok2 = gp.mll_grad(th, False, 0.0, grad=False)
    assert not ok2 and np.isfinite(mll2)
    with pytest.raises(bo.ModelFittingError):
        gp.factor(bo.GPHyper(c=th[4], s=np.exp(th[3]), ls=np.exp(th[:3]), noise=0.0))
    assert not bo.gp_mll_grad_host(X, y, th, None, False, 0.0)[2]
    Xs, ys, fs, ths, ls_ = _case(449, 2, "fix")          # sound data on the same handle: the bits of a fresh handle
    gp.set_data(Xs, ys, fs)
    assert _same(gp.mll_grad(ths, ls_, 1e-6), _fresh(Xs, ys, fs, ths, ls_))


def test_same_bits_and_nothing_stale_at_size(gp, campaign):
    Xn, targets, fixed, z = campaign
    th = z["theta_1_1"]
    gp.set_data(Xn, targets[:, 1], fixed[:, 1])
    first = gp.mll_grad(th, True, 1e-6)
    assert _same(first, gp.mll_grad(th, True, 1e-6))
    _, Xm, ym, fm, thm, lm = _clustered(1409, 7, "obj")
    gp.set_data(Xm, ym, fm)
    assert gp.mll_grad(thm, lm, 1e-6, grad=False)[0] == gp.mll_grad(thm, lm, 1e-6)[0]          # the value alone: the same bits
    _, Xl, yl, fl, thl, ll = _clustered(4096, 7, "obj")
    Xs, ys, fs, ths, ls_ = _case(257, 7, "obj")
    X5, y5, f5, th5, l5 = _case(5, 7, "obj")
    h5 = bo.GPHyper(c=0.1, s=1.3, ls=np.exp(th5[:7]), noise=0.05)
    big_fresh, small_fresh, five_fresh = _fresh(Xl, yl, fl, thl, ll), _fresh(Xs, ys, fs, ths, ls_), _fresh(X5, y5, f5, th5, l5)
    g = bo.DeviceGP()
    try:
        g.set_data(X5, y5, f5)
        v5 = g.factor(h5)
    finally:
        g.close()
    # after n = 4096 on a handle, n = 257 gives what a fresh handle gives
    gp.set_data(Xl, yl, fl)
    assert _same(gp.mll_grad(thl, ll, 1e-6), big_fresh)
    gp.set_data(Xs, ys, fs)
    assert _same(gp.mll_grad(ths, ls_, 1e-6), small_fresh)
    # 5, 4096, 5, 2050 on one handle: its buffers grow from one tile to 2080 and never shrink
    g = bo.DeviceGP()
    try:
        for step in ("five", "big", "five", "campaign"):
            if step == "five":
                g.set_data(X5, y5, f5)
                v = g.factor(h5)
                assert _same(g.mll_grad(th5, l5, 1e-6), five_fresh) and (v[0] == v5[0]).all() and (v[1] == v5[1]).all()
            elif step == "big":
                g.set_data(Xl, yl, fl)
                assert _same(g.mll_grad(thl, ll, 1e-6), big_fresh)
            else:
                g.set_data(Xn, targets[:, 1], fixed[:, 1])
                assert _same(g.mll_grad(th, True, 1e-6), first)
    finally:
        g.close()


def test_fit_on_the_device_at_the_campaign_objective_shape(gp, golden_dir):
    """bo.fit_gp(backend="device") on the campaign's 194 feasible trials (d = 7), both objectives, by the criteria of
    test_fit_on_the_device."""
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    feas = z["feasible"]
    Xt = z["params_nor"][feas]
    Ys = bo.standardize(z["objectives"][feas][:, 0, :])[0]
    assert Xt.shape == (194, 7)
    for o in range(2):
        y = Ys[:, o]
        h1, start, end = bo.fit_gp(Xt, y, return_trace=True, backend="device", gp=gp)
        h2 = bo.fit_gp(Xt, y, backend="device", gp=gp)
        _, _, end_cpu = bo.fit_gp(Xt, y, return_trace=True)
        _, _, end_gpu = bo.fit_gp(Xt, y, return_trace=True, device="cuda")
        g = max(4.0 * abs(end_gpu - end_cpu), 1e-9 * abs(end_cpu))
        print(f"gp_bounds fit campaign objective {o} n=194 d=7: start {start!r} end device {end!r} torch cpu {end_cpu!r} torch gpu {end_gpu!r} g {g:.3e}")
        assert end >= start
        assert h1.c == h2.c and h1.s == h2.s and h1.noise == h2.noise and (h1.ls == h2.ls).all()
        assert abs(bo.gp_mll(Xt, y, bo.GPHyper(h1.c, h1.s, h1.ls, h1.noise - 1e-6), noise_floor=1e-6) - end) <= 1e-9 * abs(end)
        assert end >= end_cpu - g
