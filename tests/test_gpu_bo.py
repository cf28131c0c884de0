"""
The acquisition value on the device (csrc/bo_kernels.hpp behind tum_bo_evaluate) against the long-double reference of
tests/bo_reference.py.

Gate: errors are measured against the long-double value in units of u = 2^-53 times the scale of the quantity -- s_o for mu and d2,
the batch's largest alpha for alpha and the mean HVI, 1 for p, sd and factor. A quantity's gate is 4 x the larger of the errors of
bo.host_acquisition and bo_reference.torch_acquisition (two FP64 statements of the same sums in other orders), with a floor of 32.
Every candidate and every detail row is compared; none is set aside. Hyperparameters are literal (bo_reference.hypers): nothing here
depends on fit_gp. The lines the module prints are kept in profiles/bo_bounds.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_reference as ref          # noqa: E402
from tum_control_amd import bo      # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
NAMES = ("alpha",) + bo.DETAIL


@pytest.fixture(scope="module")
def acq():
    a = bo.DeviceAcquisition()
    yield a
    a.close()


def _errors(m, alpha, det, ld_alpha, ld_det):
    """Largest error of every quantity over the batch, in its units."""
    amax = float(np.abs(ld_alpha).max())
    amax = amax if amax > 0 else 1.0
    scale = [amax, m.s[0], m.s[1], m.s[0], m.s[1], amax, 1.0, 1.0, 1.0]
    got = np.concatenate([np.asarray(alpha)[:, None], np.asarray(det)], axis=1)
    want = np.concatenate([ld_alpha[:, None], ld_det], axis=1)
    err = np.abs(got.astype(np.longdouble) - want).max(0)
    return np.array([float(err[i] / (U * scale[i])) for i in range(9)])


def _gate(acq, m, X, label):
    ld_alpha, ld_det = ref.longdouble_acquisition(m, X)
    acq.set_model(m)
    e_dev = _errors(m, *acq.evaluate(X, detail=True), ld_alpha, ld_det)
    e_host = _errors(m, *bo.host_acquisition(m, X, detail=True), ld_alpha, ld_det)
    e_torch = _errors(m, *ref.torch_acquisition(m, X), ld_alpha, ld_det)
    gate = np.maximum(32.0, 4.0 * np.maximum(e_host, e_torch))
    for i, n in enumerate(NAMES):
        print(f"bo_bounds {label} {n}: device {e_dev[i]:.2f} host {e_host[i]:.2f} torch {e_torch[i]:.2f} gate {gate[i]:.2f} (u x scale)")
    for i, n in enumerate(NAMES):
        assert e_dev[i] <= gate[i], (label, n, e_dev[i], gate[i])


# d, n_t, n_b, n_c, S, C, K: every tile edge of every kernel once
SHAPES = [(2, 1, 1, 2, 1, 1, 8),
          (7, 3, 2, 15, 64, 15, 64),
          (2, 16, 16, 64, 100, 16, 8),
          (7, 17, 17, 65, 64, 17, 64),
          (7, 37, 33, 130, 100, 200, 8),
          (2, 37, 2, 65, 1, 200, 64),
          (7, 16, 33, 130, 64, 15, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_t%d_b%d_c%d_S%d_C%d_K%d" % s)
def test_acquisition_against_long_double(acq, shape):
    d, n_t, n_b, n_c, S, C, K = shape
    m = ref.generate(d, n_t, n_b, n_c, S, K, seed=sum(shape))
    X = np.random.default_rng(1 + sum(shape)).random((C, d))
    _gate(acq, m, X, "d=%d n_t=%d n_b=%d n_c=%d S=%d C=%d K=%d" % shape)


def test_candidate_on_a_baseline_point_has_the_jitter_as_variance(acq):
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=5)
    acq.set_model(m)
    _, det = acq.evaluate(m.Xb, detail=True)
    assert (det[:, 2] == m.jitter[0]).all() and (det[:, 3] == m.jitter[1]).all()


def test_reference_point_above_every_sample_gives_zero(acq):
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=6, ref=(50.0, 50.0))
    assert (m.front_count == 0).all()
    acq.set_model(m)
    alpha = acq.evaluate(np.random.default_rng(0).random((40, 7)))
    assert (alpha == 0.0).all()


def test_empty_fronts_give_the_box_area(acq):
    """No front point in any sample: HVI_s is the box [ref, f_s]. The long-double reference is held to the box formula on its own
    samples (same numbers, another order of the sum: 4 u relative), the device to the long-double reference by the module's gate."""
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=7)
    m.front_count[:] = 0
    m.fronts[:] = 0.0
    X = np.random.default_rng(2).random((33, 7))
    _, det, f = ref.longdouble_acquisition(m, X, return_samples=True)
    box = (np.maximum(f[0] - m.ref[0], 0) * np.maximum(f[1] - m.ref[1], 0)).mean(0)
    assert box.max() > 0
    assert np.abs(det[:, 4] - box).max() <= 4 * U * float(box.max())
    _gate(acq, m, X, "empty fronts")


@pytest.mark.parametrize("flag", [True, False])
def test_single_class_trial_set(acq, flag):
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=8, single_class=flag)
    X = m.Xc[:20]          # at the trials themselves, where the latent means sit near their targets (log 1.001 against log 0.001)
    _gate(acq, m, X, "single class %s" % flag)
    _, det = acq.evaluate(X, detail=True)
    p, sd, factor = det[:, 5], det[:, 6], det[:, 7]
    assert np.abs(factor - (m.eps * p + (1.0 - m.eps) * sd)).max() <= 2 * U
    assert (p > 0.95).all() if flag else (p < 0.05).all()


def test_real_shape_first_300_trials(acq, golden_dir):
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"][:300], z["feasible"][:300], z["objectives"][:300]
    Xt = Xn[feas]
    assert 40 <= len(Xt) <= 80
    Ys = bo.standardize(obj[feas][:, 0, :])[0]
    o_h, c_h = ref.hypers(7)
    S = 128
    Z = bo.sobol_normal(S, 2 * (len(Xt) + 2), 4).reshape(S, 2, -1).transpose(0, 2, 1)
    m = bo.pack_model(Xt, Ys, o_h, Xn, feas, c_h, Xt, Z, np.array([-0.5, -0.75]), eps=0.8, jitter=1e-6, K=32)
    X = np.vstack([bo.sobol_points(64, 7, 5), Xt])
    _gate(acq, m, X, "fixture[:300] n_t=%d S=128 C=%d" % (len(Xt), len(X)))


_CAMPAIGN = []
S_CAMPAIGN = 1000


def _campaign_model(golden_dir):
    """The model of test_real_shape_first_300_trials from all 2050 trials: n_c = 2050, n_t = n_b = 194, packed once per module."""
    if not _CAMPAIGN:
        z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
        Xn, feas, obj = z["params_nor"], z["feasible"], z["objectives"]
        Xt = Xn[feas]
        assert len(Xn) == 2050 and len(Xt) == 194
        Ys = bo.standardize(obj[feas][:, 0, :])[0]
        o_h, c_h = ref.hypers(7)
        S = S_CAMPAIGN
        Z = bo.sobol_normal(S, 2 * (len(Xt) + 2), 4).reshape(S, 2, -1).transpose(0, 2, 1)
        _CAMPAIGN.append((bo.pack_model(Xt, Ys, o_h, Xn, feas, c_h, Xt, Z, np.array([-0.5, -0.75]), eps=0.8, jitter=1e-6, K=64), Xt))
    return _CAMPAIGN[0]


def test_real_shape_all_2050_trials(acq, golden_dir):
    """The shape every step of the logged campaign has: n_c = 2050 (row-tile chains of 129 tiles over the class factors, offsets into
    them past 2^22 doubles), n_t = n_b = 194, K = 64. S = 1000 samples: no multiple of 16, so the sample mask is live (the
    long-double reference takes about 5 s of the CPU at this S). 17 Sobol candidates and 3 trial points: two column tiles, one
    partial."""
    m, Xt = _campaign_model(golden_dir)
    X = np.vstack([bo.sobol_points(17, 7, 5), Xt[:3]])
    _gate(acq, m, X, "fixture[:2050] n_t=%d S=%d C=%d" % (len(Xt), m.S, len(X)))


def test_alone_and_inside_a_batch_same_bits_at_the_campaign_shape(acq, golden_dir):
    m, _ = _campaign_model(golden_dir)
    acq.set_model(m)
    X = np.random.default_rng(14).random((600, 7))
    a600, d600 = acq.evaluate(X, detail=True)          # (two passes of the chain: 512 + 88)
    assert np.isfinite(a600).all() and np.isfinite(d600).all() and a600.max() > 0
    for i in (0, 15, 16, 511, 512, 599):
        a1, d1 = acq.evaluate(X[i:i + 1], detail=True)
        assert a1[0] == a600[i] and (d1[0] == d600[i]).all(), i


def test_acquisition_at_the_size_limits(acq):
    """n_b = 512 (BO_MAXB) and S = 4096 (BO_MAXS) at once; the baseline repeats draws behind the 40 trials."""
    shape = (7, 40, 512, 130, 4096, 20, 8)
    d, n_t, n_b, n_c, S, C, K = shape
    m = ref.generate(d, n_t, n_b, n_c, S, K, seed=sum(shape))
    X = np.random.default_rng(1 + sum(shape)).random((C, d))
    _gate(acq, m, X, "d=%d n_t=%d n_b=%d n_c=%d S=%d C=%d K=%d" % shape)


def test_alone_and_inside_a_batch_same_bits(acq):
    m = ref.generate(7, 37, 33, 130, 100, 8, seed=9)
    acq.set_model(m)
    X = np.random.default_rng(4).random((600, 7))
    a200, d200 = acq.evaluate(X[:200], detail=True)
    a600, d600 = acq.evaluate(X, detail=True)          # (two passes of the chain: 512 + 88)
    assert (a600[:200] == a200).all() and (d600[:200] == d200).all()
    for i in (0, 15, 16, 199, 511, 512, 599):
        a1, d1 = acq.evaluate(X[i:i + 1], detail=True)
        assert a1[0] == a600[i] and (d1[0] == d600[i]).all(), i
    again = acq.evaluate(X)
    assert (again == a600).all()


class _OneAtATime:
    def __init__(self, acq):
        self.acq = acq

    def set_model(self, m, keep_gp=False):
        self.acq.set_model(m, keep_gp=keep_gp)

    def evaluate(self, X):
        return np.array([self.acq.evaluate(x[None, :])[0] for x in np.atleast_2d(X)])


def test_select_equals_the_search_one_evaluation_at_a_time(acq):
    m = ref.generate(2, 16, 16, 64, 64, 8, seed=10, q=2)
    kw = dict(q=2, n_raw=16, n_restarts=3, max_iter=12, seed=3)
    p1, v1, m1 = bo.select(m, acq=acq, **kw)
    p2, v2, m2 = bo.select(m, acq=_OneAtATime(acq), **kw)
    assert (p1 == p2).all() and (v1 == v2).all()
    assert ((p1 >= 0) & (p1 <= 1)).all() and m1.n_b == m.n_b + 2


def test_appended_model_equals_a_fresh_upload(acq):
    m = ref.generate(7, 17, 17, 65, 64, 8, seed=11, q=2)
    X = np.random.default_rng(5).random((50, 7))
    acq.set_model(m)
    m2 = bo.append_pick(m, X[0])
    acq.set_model(m2, keep_gp=True)
    kept = acq.evaluate(X, detail=True)
    fresh = bo.DeviceAcquisition()
    try:
        fresh.set_model(m2)
        new = fresh.evaluate(X, detail=True)
    finally:
        fresh.close()
    assert (kept[0] == new[0]).all() and (kept[1] == new[1]).all()


def test_refusals():
    a = bo.DeviceAcquisition()
    try:
        with pytest.raises(Exception, match="no model"):
            a.evaluate(np.zeros((1, 2)))
        big = ref.generate(2, 3, 513, 15, 4, 8, seed=12)
        with pytest.raises(Exception, match="n_b"):
            a.set_model(big)
        m = ref.generate(2, 3, 2, 15, 4, 8, seed=12)
        m65 = ref.generate(2, 3, 2, 15, 4, 65, seed=12)
        with pytest.raises(Exception, match="K outside"):
            a.set_model(m65)
        with pytest.raises(Exception, match="no model"):          # a refused model leaves none behind
            a.evaluate(np.zeros((1, 2)))
        a.set_model(m)
        with pytest.raises(Exception, match="d = 2"):
            a.evaluate(np.zeros((1, 3)))
        X = np.full((3, 2), 0.5)
        X[1, 1] = np.nan
        with pytest.raises(Exception, match="NaN"):
            a.evaluate(X)
        with pytest.raises(Exception, match="keep_gp"):
            a.set_model(ref.generate(2, 4, 2, 15, 4, 8, seed=12), keep_gp=True)
        assert np.isfinite(a.evaluate(np.full((3, 2), 0.5))).all()
    finally:
        a.close()


def test_handle_lifetime():
    m1, m2 = ref.generate(2, 16, 16, 64, 64, 8, seed=13), ref.generate(7, 17, 17, 65, 64, 8, seed=14)
    X1, X2 = np.random.default_rng(6).random((20, 2)), np.random.default_rng(7).random((20, 7))
    first = []
    for _ in range(2):
        a = bo.DeviceAcquisition()
        a.set_model(m1)
        first.append(a.evaluate(X1))
        a.close()
    assert (first[0] == first[1]).all()
    a, b = bo.DeviceAcquisition(), bo.DeviceAcquisition()
    try:
        a.set_model(m1); b.set_model(m2)
        va, vb = a.evaluate(X1), b.evaluate(X2)
        assert (a.evaluate(X1) == va).all() and (va == first[0]).all()
        b.close()
        assert (a.evaluate(X1) == va).all() and np.isfinite(vb).all()
    finally:
        a.close(); b.close()
