"""
The parts of the acquisition model the device builds (csrc/bo_model_kernels.hpp behind tum_bom_prune, tum_bom_fronts, tum_bom_build,
tum_bom_append and tum_bom_model_read) against the long-double restatements of tests/bo_model_reference.py.

Gate of every floating-point array (the pruning draws F; H, R, L_b, mu_b, F_b of the built baseline; every output of tum_bo_evaluate
on the built model): the error against the long-double value in units of u = 2^-53 times the array's largest magnitude (the units of
tests/test_gpu_bo.py for the acquisition's outputs); the gate is max(32, 4 x the larger of the errors of the numpy statement in bo.py
and of the same statement in torch float64 on the CPU), measured per shape against the reference, never against the device. The keep
mask is exact: it equals the host rule applied to the device's own draws, and it equals bo.prune_baseline(backend="host") on every
trial, because tests/test_bo_model_host.py shows every trial of every fixture here to be robust (margin further than 1e-6 from zero).
Fronts and counts equal bo.build_fronts of the device's own draws; dominance and fronts of GIVEN draws are compared to the bit. The
lines the module prints are kept in profiles/bo_model_bounds.txt.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_model_reference as mref          # noqa: E402
import bo_reference as ref                 # noqa: E402
from tum_control_amd import bo             # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acq():
    a = bo.DeviceAcquisition()
    yield a
    a.close()


def _prune_gate(acq, fx, label):
    F_ld = mref.longdouble_draws(fx)
    args = (fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    keep, F = acq.prune(*args, draws=True)
    e_dev, e_host, e_torch = mref.error(F, F_ld), mref.error(mref.host_draws(fx), F_ld), mref.error(mref.torch_prune_draws(*args), F_ld)
    gate = max(32.0, 4.0 * max(e_host, e_torch))
    print(f"bo_model_bounds {label} F: device {e_dev:.2f} host {e_host:.2f} torch {e_torch:.2f} gate {gate:.2f} (u x scale)")
    assert e_dev <= gate, (label, e_dev, gate)
    assert (keep == bo.dominance_keep(F)).all()
    host = bo.dominance_keep(mref.host_draws(fx))
    robust = np.abs(mref.margins(mref.host_draws(fx))) > mref.ROBUST
    assert robust.all() and (keep[robust] == host[robust]).all()
    return keep


@pytest.mark.parametrize("shape", mref.PRUNE_SHAPES, ids=lambda s: "n%d_d%d_S%d_seed%d" % s)
def test_pruning_draws_and_mask(acq, shape):
    n, d, S, seed = shape
    fx = mref.prune_fixture(*shape)
    keep = _prune_gate(acq, fx, "n=%d d=%d S=%d" % shape[:3])
    got = bo.prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=S, seed=seed, jitter=fx["jitter"], backend="device", acq=acq)
    want = bo.prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=S, seed=seed, jitter=fx["jitter"], backend="host")
    assert (got == np.flatnonzero(keep)).all() and len(got) == len(want) and (got == want).all()


def test_pruning_at_the_campaign_shape(acq, golden_dir):
    """n = 194 (four block columns), S = 1024, the trials of the logged campaign."""
    fx = mref.campaign_fixture(golden_dir)
    keep = _prune_gate(acq, fx, "campaign n=194 S=%d" % mref.CAMPAIGN_S)
    again, F2 = acq.prune(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"], draws=True)
    small = mref.prune_fixture(*mref.PRUNE_SHAPES[2])
    acq.prune(small["Xt"], small["V"], small["a"], small["obj"], small["Zs"], small["jitter"])
    third, F3 = acq.prune(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"], draws=True)
    assert (again == keep).all() and (third == keep).all() and (F2 == F3).all()          # (the same bits, also behind another problem)


def test_dominance_alone_is_exact(acq):
    same = np.tile(np.array([[0.25, -1.5]]), (3, 19, 1))
    assert acq.prune_given(same).all()
    # a strict chain per sample, in another order each: one trial kept per sample, the union over the samples
    rng = np.random.default_rng(0)
    S, n = 5, 70
    chain = np.stack([np.stack([p, p], axis=1) for p in (rng.permutation(n).astype(np.float64) for _ in range(S))])
    keep = acq.prune_given(chain)
    assert (keep == bo.dominance_keep(chain)).all()
    assert sorted(np.flatnonzero(keep)) == sorted({int(np.argmax(chain[s, :, 0])) for s in range(S)})
    # ties in one objective only: the largest other objective wins, its duplicates with it
    tie = np.zeros((1, 9, 2))
    tie[0, :, 1] = [3, 1, 4, 1, 5, 2, 5, 3, 0]
    assert (np.flatnonzero(acq.prune_given(tie)) == [4, 6]).all()
    assert (np.flatnonzero(acq.prune_given(tie[:, :, ::-1])) == [4, 6]).all()
    # small integers: ties of every kind
    ints = rng.integers(0, 5, size=(7, 130, 2)).astype(np.float64)
    assert (acq.prune_given(ints) == bo.dominance_keep(ints)).all()


def test_dominance_at_the_lds_limit(acq):
    """n = 4096: a sample's draws fill the 64 KB a workgroup may take."""
    F = np.random.default_rng(1).integers(0, 300, size=(2, 4096, 2)).astype(np.float64)
    keep = acq.prune_given(F)
    want = np.zeros(4096, dtype=bool)
    for s in range(2):          # (the front by a sort: bo.dominance_keep would take n^2 memory here)
        order = np.lexsort((-F[s, :, 1], -F[s, :, 0]))
        best, on = -np.inf, []
        for i in order:
            if F[s, i, 1] > best:
                best = F[s, i, 1]
                on.append(i)
        front = {tuple(F[s, i]) for i in on}
        want |= np.array([tuple(F[s, i]) in front for i in range(4096)])
    assert (keep == want).all() and 0 < keep.sum() < 4096


def test_fronts_alone_are_exact(acq):
    rng = np.random.default_rng(2)
    r = np.array([-0.5, 0.25])
    for nb in (1, 16, 17, 512):
        # every point on the front, in a shuffled order
        x = r[0] + 1.0 + np.arange(nb)
        F = np.stack([np.stack([x, r[1] + 1.0 + x[::-1]], axis=1)[rng.permutation(nb)] for _ in range(3)])
        fronts, count = acq.fronts(F, r)
        want_f, want_c = bo.build_fronts(F, r)
        assert (count == nb).all() and (count == want_c).all() and (fronts == want_f).all()
        # the reference point above every draw
        fronts, count = acq.fronts(F, np.array([1e6, 1e6]))
        assert (count == 0).all() and (fronts == 0.0).all()
    for nb, S in ((5, 40), (33, 17), (130, 9), (512, 3)):
        # duplicates, equal objective-0 values, points on and below the reference point
        F = rng.integers(-1, 7, size=(S, nb, 2)).astype(np.float64)
        fronts, count = acq.fronts(F, np.array([0.0, 1.0]))
        want_f, want_c = bo.build_fronts(F, np.array([0.0, 1.0]))
        assert (count == want_c).all() and (fronts == want_f).all()
    m = ref.generate(3, 40, 17, 60, 64, 8, seed=21)
    fronts, count = acq.fronts(m.F_b, m.ref)
    assert (count == m.front_count).all() and (fronts == m.fronts).all() and count.max() > 1


def test_failed_factorisation_is_reported(acq):
    """A `factor` ten times too large makes K - H H^T negative on its diagonal: the pivots fail by arithmetic, the chain finishes with
    the failed pivots replaced, ok is 0 and Python raises ModelFittingError; a valid call on the same handle afterwards is correct."""
    fx = mref.prune_fixture(*mref.PRUNE_SHAPES[4])
    wrong = [10.0 * np.asarray(v) for v in fx["V"]]
    with pytest.raises(bo.ModelFittingError):
        acq.prune(fx["Xt"], wrong, fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    with pytest.raises(bo.ModelFittingError):          # (the host path refuses the same input)
        bo.prune_draws(fx["Xt"], wrong, fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    _prune_gate(acq, fx, "after a failed factorisation n=%d d=%d S=%d" % mref.PRUNE_SHAPES[4][:3])


def test_refusals():
    a = bo.DeviceAcquisition()
    try:
        fx = mref.prune_fixture(*mref.PRUNE_SHAPES[1])
        args = [fx["Xt"], list(fx["V"]), list(fx["a"]), fx["obj"], fx["Zs"], fx["jitter"]]
        F = np.zeros((2, 3, 2))
        F[1, 2, 0] = np.nan
        with pytest.raises(Exception, match="NaN"):
            a.prune_given(F)
        with pytest.raises(Exception, match="S outside"):
            a.prune_given(np.zeros((4097, 1, 2)))
        with pytest.raises(Exception, match="n outside"):
            a.prune_given(np.zeros((1, 4097, 2)))
        bad = [np.array(v) for v in fx["V"]]
        bad[1][3, 2] = np.inf
        with pytest.raises(Exception, match="NaN"):
            a.prune(args[0], bad, *args[2:])
        full = [np.array(v) for v in fx["V"]]
        full[0][2, 9] = 1e-3
        with pytest.raises(Exception, match="above its diagonal"):
            a.prune(args[0], full, *args[2:])
        with pytest.raises(Exception, match="sizes of Xt"):
            a.prune(args[0], [v[:5, :5] for v in fx["V"]], *args[2:])
        with pytest.raises(Exception, match="d outside"):
            a.prune(np.zeros((15, 17)), args[1], args[2], [bo.GPHyper(0.0, 1.0, np.ones(17)), bo.GPHyper(0.0, 1.0, np.ones(17))], *args[4:])
        desc = a._prune_desc()
        assert desc.struct_size == ctypes.sizeof(bo._PruneDesc)
        desc.struct_size -= 8
        keep, ok = np.zeros(3, dtype=np.int32), ctypes.c_int()
        assert a._L.tum_bom_prune(a._h, ctypes.addressof(desc), keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, ctypes.byref(ok)) != 0
        assert b"struct_size" in a._L.tum_ocp_last_error()
        assert a._L.tum_bom_prune(a._h, None, keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, ctypes.byref(ok)) != 0
        assert b"null" in a._L.tum_ocp_last_error()
        with pytest.raises(Exception, match="n_b outside"):
            a.fronts(np.zeros((2, 513, 2)), np.zeros(2))
        with pytest.raises(Exception, match="NaN"):
            a.fronts(F, np.zeros(2))
        with pytest.raises(Exception, match="NaN"):
            a.fronts(np.zeros((2, 3, 2)), np.array([0.0, np.inf]))
        with pytest.raises(Exception, match="no model"):          # pruning installs no model
            a.evaluate(np.zeros((1, 2)))
        assert a.prune(*args)[0].any()
    finally:
        a.close()


def test_handle_lifetime():
    """Two handles give the same bits; closing one leaves the other alone; pruning leaves a handle's acquisition model alone."""
    fx = mref.prune_fixture(*mref.PRUNE_SHAPES[4])
    args = (fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    m = ref.generate(2, 16, 16, 64, 64, 8, seed=13)
    X = np.random.default_rng(6).random((20, 2))
    a, b = bo.DeviceAcquisition(), bo.DeviceAcquisition()
    try:
        a.set_model(m)
        before = a.evaluate(X)
        ka, Fa = a.prune(*args, draws=True)
        kb, Fb = b.prune(*args, draws=True)
        assert (ka == kb).all() and (Fa == Fb).all()
        b.close()
        k2, F2 = a.prune(*args, draws=True)
        assert (k2 == ka).all() and (F2 == Fa).all()
        assert (a.evaluate(X) == before).all()
        ms = a.prune_profile(True)
        a.prune(*args)
        ms = a.prune_profile(False)
        assert ms.shape == (7,) and (ms >= 0).all() and ms.sum() > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ the baseline built on the device
ACQ_NAMES = ("alpha",) + bo.DETAIL


def _acq_errors(m, alpha, det, ld_alpha, ld_det):
    """tests/test_gpu_bo.py's units: the batch's largest alpha for alpha and the mean HVI, s_o for mu and d2, 1 for p, sd, factor."""
    amax = float(np.abs(ld_alpha).max())
    amax = amax if amax > 0 else 1.0
    scale = [amax, m.s[0], m.s[1], m.s[0], m.s[1], amax, 1.0, 1.0, 1.0]
    got = np.concatenate([np.asarray(alpha)[:, None], np.asarray(det)], axis=1)
    want = np.concatenate([ld_alpha[:, None], ld_det], axis=1)
    err = np.abs(got.astype(np.longdouble) - want).max(0)
    return np.array([float(err[i] / (mref.U * scale[i])) for i in range(9)])


def _gate_model(acq, host, got, want, torch_built, label, C):
    """The resident model of acq (arrays `got`) against the long-double arrays `want`; host: the numpy-built model of the same inputs."""
    from dataclasses import replace
    e_dev, e_torch = mref.build_errors(got, want), mref.build_errors(torch_built, want)
    e_host = mref.build_errors(dict(H=host.H, R=host.R, L_b=host.L_b, mu_b=host.mu_b, F_b=host.F_b), want)
    gates = {n: max(32.0, 4.0 * max(e_host[n], e_torch[n])) for n in mref.BUILD_ARRAYS}
    for n in mref.BUILD_ARRAYS:
        print(f"bo_model_bounds {label} {n}: device {e_dev[n]:.2f} host {e_host[n]:.2f} torch {e_torch[n]:.2f} gate {gates[n]:.2f} (u x scale)")
    # the fronts are those of the device's own draws, to the bit
    fronts, count = bo.build_fronts(got["F_b"], host.ref)
    assert (got["front_count"] == count).all() and (got["fronts"] == fronts).all()
    # the acquisition value of the resident model against the long-double acquisition of the long-double model
    X = np.random.default_rng(1 + host.n_b + len(host.Xt)).random((C, host.d))
    ld_alpha, ld_det = ref.longdouble_acquisition(replace(host, **want), X)
    a_dev = _acq_errors(host, *acq.evaluate(X, detail=True), ld_alpha, ld_det)
    a_host = _acq_errors(host, *bo.host_acquisition(host, X, detail=True), ld_alpha, ld_det)
    a_torch = _acq_errors(host, *ref.torch_acquisition(replace(host, **torch_built), X), ld_alpha, ld_det)
    a_gate = np.maximum(32.0, 4.0 * np.maximum(a_host, a_torch))
    for i, n in enumerate(ACQ_NAMES):
        print(f"bo_model_bounds {label} {n}: device {a_dev[i]:.2f} host {a_host[i]:.2f} torch {a_torch[i]:.2f} gate {a_gate[i]:.2f} (u x scale)")
    for n in mref.BUILD_ARRAYS:
        assert e_dev[n] <= gates[n], (label, n, e_dev[n], gates[n])
    for i, n in enumerate(ACQ_NAMES):
        assert a_dev[i] <= a_gate[i], (label, n, a_dev[i], a_gate[i])


def _build_gate(acq, shape, label, C=33):
    """shape: one of mref.BUILD_SHAPES, or the pair (host-built model, the same inputs packed with baseline="device")."""
    host, dev = shape if not isinstance(shape[0], int) else mref.build_fixture(shape)
    acq.set_model(dev)
    got = acq.model_arrays()
    _gate_model(acq, host, got, mref.longdouble_build(host), mref.torch_build(host), label, C)
    return host, dev, got


APPEND_SHAPES = [(3, 40, 15, 60, 33), (7, 130, 63, 300, 100)]          # n_b 15 -> 18 across a 16-row tile edge, 63 -> 66 across a block edge


@pytest.mark.parametrize("shape", APPEND_SHAPES, ids=lambda s: "d%d_t%d_b%d_c%d_S%d" % s)
def test_device_appends(acq, shape):
    """Three picks appended on the device (tum_bom_append), the three columns the base samples leave free. Every state: the arrays and
    tum_bo_evaluate against the long-double statement of append_pick applied to the long-double model, gate from bo.append_pick
    (numpy) and the torch statement, each appended to its own model; fronts to the bit. The same sequence from the same state gives
    the same bits; a fourth append has no column left."""
    host, dev = mref.build_fixture(shape)
    xs = np.random.default_rng(3 + sum(shape)).random((3, host.d))
    X = np.random.default_rng(4).random((40, host.d))
    ld, th, hm = mref.longdouble_build(host), mref.torch_build(host), host
    acq.set_model(dev)
    states = []
    for i, x in enumerate(xs):
        acq.append_pick(x)
        ld, th = mref.longdouble_append(hm, ld, x), mref.torch_append(hm, th, x)
        hm = bo.append_pick(hm, x)
        got = acq.model_arrays()
        assert got["F_b"].shape[1] == host.n_b + i + 1
        _gate_model(acq, hm, got, ld, th, "append %d to n_b=%d (d=%d n_t=%d S=%d)" % (i + 1, host.n_b, shape[0], shape[1], shape[4]), 33)
        states.append((got, acq.evaluate(X, detail=True)))
    with pytest.raises(Exception, match="no column left"):
        acq.append_pick(xs[0])
    acq.set_model(dev)
    for x, (got, ev) in zip(xs, states):
        acq.append_pick(x)
        again, ev2 = acq.model_arrays(), acq.evaluate(X, detail=True)
        assert (ev2[0] == ev[0]).all() and (ev2[1] == ev[1]).all()
        for n in ("F_b", "fronts", "front_count"):
            assert (again[n] == got[n]).all(), n
        for n in ("H", "R", "L_b", "mu_b"):
            assert all((again[n][o] == got[n][o]).all() for o in range(2)), n


class _ReadBackAndInstallFresh:
    """The evaluator of the comparison the device appends are held to: builds and appends on one handle, but after the build and after
    every append reads the model back (model_arrays) and installs it through tum_bo_model on another handle, which evaluates."""

    def __init__(self, acq, fresh):
        self.acq, self.fresh = acq, fresh

    def _install(self):
        self.fresh.set_model(bo.complete_model(self.model, self.acq.model_arrays()))

    def set_model(self, m, keep_gp=False):
        self.acq.set_model(m)
        self.model = m
        self._install()

    def append_pick(self, x):
        from dataclasses import replace
        self.acq.append_pick(x)
        self.model = replace(self.model, Xb=np.vstack([self.model.Xb, np.asarray(x)[None, :]]))
        self._install()

    def model_arrays(self):
        return self.acq.model_arrays()

    def evaluate(self, X, detail=False):
        return self.fresh.evaluate(X, detail=detail)


def test_select_with_device_appends_equals_read_back_and_fresh_install(acq):
    host, dev = mref.build_fixture(APPEND_SHAPES[1])
    kw = dict(q=3, n_raw=16, n_restarts=3, max_iter=12, seed=3)
    p1, v1, m1 = bo.select(dev, acq=acq, **kw)
    fresh = bo.DeviceAcquisition()
    try:
        p2, v2, m2 = bo.select(dev, acq=_ReadBackAndInstallFresh(acq, fresh), **kw)
    finally:
        fresh.close()
    assert (p1 == p2).all() and (v1 == v2).all() and m1.n_b == host.n_b + 3 and not m1.device_baseline
    assert all((m1.H[o] == m2.H[o]).all() and (m1.R[o] == m2.R[o]).all() and (m1.L_b[o] == m2.L_b[o]).all() for o in range(2))
    assert (m1.fronts == m2.fronts).all() and (m1.F_b == m2.F_b).all() and (m1.Xb[-3:] == p1).all()
    p3, v3, m3 = bo.select(dev, acq=acq, device_append=False, **kw)          # (host appends: the same search up to rounding)
    assert m3.n_b == m1.n_b and np.isfinite(v3).all()


def test_append_refusals():
    a = bo.DeviceAcquisition()
    try:
        host, dev = mref.build_fixture(APPEND_SHAPES[0])
        x = np.full(host.d, 0.5)
        with pytest.raises(Exception, match="no model built"):
            a.append_pick(x)
        a.set_model(host)
        with pytest.raises(Exception, match="no model built"):          # a model uploaded from the host is not one the device built
            a.append_pick(x)
        a.set_model(dev)
        with pytest.raises(Exception, match="d = 3"):
            a.append_pick(np.zeros(4))
        bad = x.copy()
        bad[1] = np.nan
        with pytest.raises(Exception, match="NaN"):
            a.append_pick(bad)
        ok = ctypes.c_int()
        assert a._L.tum_bom_append(a._h, None, ctypes.byref(ok)) != 0 and b"null" in a._L.tum_ocp_last_error()
        assert a.model_arrays()["F_b"].shape[1] == host.n_b          # (the refusals left the model as it was)
        full = ref.generate(2, 5, 512, 9, 4, 8, seed=3, q=3)
        from dataclasses import replace
        a.set_model(replace(full, H=[], R=[], L_b=[], mu_b=[], F_b=None, fronts=None, front_count=None, device_baseline=True))
        with pytest.raises(Exception, match="512 already"):
            a.append_pick(np.full(2, 0.5))
    finally:
        a.close()


@pytest.mark.parametrize("shape", mref.BUILD_SHAPES, ids=lambda s: "d%d_t%d_b%d_c%d_S%d" % s)
def test_built_baseline(acq, shape):
    _build_gate(acq, shape, "build d=%d n_t=%d n_b=%d n_c=%d S=%d" % shape)


def test_built_model_equals_its_read_back_installed_fresh(acq):
    """The operand layouts the device packs H and R into are the ones tum_bo_model packs: the arrays read back, installed through
    tum_bo_model on another handle, give the bits of the built model; and select() from the device-built model with host appends
    (device_append=False) is the search from that completed model."""
    host, dev = mref.build_fixture(mref.BUILD_SHAPES[4])
    X = np.random.default_rng(8).random((70, host.d))
    acq.set_model(dev)
    built = acq.evaluate(X, detail=True)
    done = bo.complete_model(dev, acq.model_arrays())
    fresh = bo.DeviceAcquisition()
    try:
        fresh.set_model(done)
        again = fresh.evaluate(X, detail=True)
        assert (built[0] == again[0]).all() and (built[1] == again[1]).all()
        kw = dict(q=3, n_raw=16, n_restarts=3, max_iter=12, seed=3)
        p1, v1, m1 = bo.select(dev, acq=acq, device_append=False, **kw)
        p2, v2, m2 = bo.select(done, acq=fresh, **kw)
        assert (p1 == p2).all() and (v1 == v2).all() and m1.n_b == host.n_b + 3 and not m1.device_baseline
        assert all((m1.H[o] == m2.H[o]).all() and (m1.R[o] == m2.R[o]).all() for o in range(2)) and (m1.fronts == m2.fronts).all()
    finally:
        fresh.close()
    with pytest.raises(Exception, match="keep_gp"):
        acq.set_model(dev, keep_gp=True)
    with pytest.raises(ValueError, match="model_arrays"):
        bo.select(dev, acq=bo.HostAcquisition(), q=1, n_raw=4, n_restarts=1, max_iter=2)


def test_built_baseline_at_the_campaign_shape(acq, golden_dir):
    """n_t = 194, n_c = 2050, the baseline the trials the device's pruning keeps, S = 1024, the campaign's jitter 1e-8: the gates and
    the exact checks of test_built_baseline, through the same function."""
    fx = mref.campaign_fixture(golden_dir)
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn, feas = z["params_nor"], z["feasible"]
    keep = np.flatnonzero(acq.prune(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"])[0])
    o_h, c_h = ref.hypers(7)
    S = mref.CAMPAIGN_S
    Z = bo.sobol_normal(S, 2 * (len(keep) + 2), 4).reshape(S, 2, -1).transpose(0, 2, 1)
    args = (fx["Xt"], fx["Ys"], o_h, Xn, feas, c_h, fx["Xt"][keep], Z, np.array([-0.5, -0.75]))
    host = bo.pack_model(*args, eps=0.8, jitter=1e-8, K=64)
    dev = bo.pack_model(*args, eps=0.8, jitter=1e-8, K=64, baseline="device")
    assert dev.device_baseline and dev.H == [] and dev.F_b is None
    _build_gate(acq, (host, dev), "campaign build n_t=194 n_b=%d n_c=2050 S=%d" % (len(keep), S), C=20)


def test_failed_baseline_is_reported(acq):
    """Singular by arithmetic: V = 0 makes H = 0 and the covariance K(Xb, Xb); s = 4, a duplicated first row and jitter 0 give the
    pivots 2 and sqrt(4 - 2 * 2) = 0. ok is 0, Python raises ModelFittingError and the handle holds no model; a valid build on the
    same handle afterwards is correct."""
    from dataclasses import replace
    host, dev = mref.build_fixture(mref.BUILD_SHAPES[2])
    Xb = dev.Xb.copy()
    Xb[1] = Xb[0]
    s = dev.s.copy()
    s[:2] = 4.0
    bad = replace(dev, Xb=Xb, s=s, V=[np.zeros_like(v) for v in dev.V[:2]] + list(dev.V[2:]), jitter=np.zeros(2))
    with pytest.raises(bo.ModelFittingError):
        acq.set_model(bad)
    with pytest.raises(Exception, match="no model"):
        acq.evaluate(np.zeros((1, dev.d)))
    with pytest.raises(Exception, match="no model"):
        acq.model_arrays()
    _build_gate(acq, mref.BUILD_SHAPES[2], "after a failed build")


def test_build_refusals():
    from dataclasses import replace
    a = bo.DeviceAcquisition()
    try:
        host, dev = mref.build_fixture(mref.BUILD_SHAPES[1])
        with pytest.raises(Exception, match="no model"):
            a.model_arrays()
        a.set_model(host)
        with pytest.raises(Exception, match="no model built"):          # a model uploaded from the host is not one the device built
            a.model_arrays()
        V = [v.copy() for v in dev.V]
        V[2][1, 0] = np.nan
        with pytest.raises(Exception, match="NaN"):
            a.set_model(replace(dev, V=V))
        V = [v.copy() for v in dev.V]
        V[1][0, 1] = 0.5
        with pytest.raises(Exception, match="above its diagonal"):
            a.set_model(replace(dev, V=V))
        with pytest.raises(Exception, match="n_b \\+ 1 columns"):
            a.set_model(replace(dev, Zfull=dev.Zfull[:, :dev.n_b]))
        with pytest.raises(Exception, match="n_b outside"):
            a.set_model(replace(dev, Xb=np.zeros((513, dev.d)), Zfull=np.zeros((dev.S, 514, 2))))
        desc = bo._BuildDesc()
        a._L.tum_bom_build_desc_init(ctypes.addressof(desc))
        assert desc.struct_size == ctypes.sizeof(bo._BuildDesc)
        desc.struct_size += 8
        ok = ctypes.c_int()
        assert a._L.tum_bom_build(a._h, ctypes.addressof(desc), ctypes.byref(ok)) != 0 and b"struct_size" in a._L.tum_ocp_last_error()
        assert a._L.tum_bom_build(a._h, None, ctypes.byref(ok)) != 0 and b"null" in a._L.tum_ocp_last_error()
        a.build_profile(True)
        a.set_model(dev)
        ms = a.build_profile(False)
        assert ms.shape == (9,) and (ms >= 0).all() and ms.sum() > 0
        assert np.isfinite(a.evaluate(np.full((3, dev.d), 0.5))).all()
    finally:
        a.close()


def test_driver_builds_its_model_on_the_device():
    """BayesianOptimization(model_backend="device"): pruning and the baseline of every step on the device, with the host's fit and
    with the device's fit and factors; the steps run without a fallback and the hypervolume grows as on the host path."""
    from test_bo_host import CFG, _toy_objective
    bounds = np.array([[1.0, 10.0], [5.0, 50.0]])
    for fit in ("torch", "device"):
        drv = bo.BayesianOptimization(bounds, CFG, _toy_objective(), acq="device", fit_backend=fit, model_backend="device")
        drv.generate_initial_data()
        drv.evaluate_at_boundaries()
        for _ in range(2):
            assert drv.perform_bayesian_optimization_step() is not None
        assert drv.fallbacks == 0 and len(drv.trials) == 18 and drv.groups_used == [0, 1]
        tr = np.array(drv.hv_traces)
        assert (np.diff(tr, axis=0) >= 0).all() and tr[-1].min() > 0
        drv.close()
        assert drv._model_acq is None and drv._gp is None
