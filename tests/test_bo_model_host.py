"""
The host side of the device-built parts of the acquisition model (tum_bom_prune, tum_bom_fronts): exports, the numpy statements of
bo.py against the long-double restatement of tests/bo_model_reference.py, the unchanged defaults, the refusals that need no device,
and the MARGIN CONDITION of every pruning fixture tests/test_gpu_bo_model.py uses: with the float64 host draws, every trial's margin
m_i = max_s min_{j != i} max_o (F[s,i,o] - F[s,j,o]) is further than 1e-6 from zero, so the keep mask is the same for any draws within
the error gate of the device test (errors of some 1e-12) and the GPU test may compare masks on every trial.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bo_model_reference as mref          # noqa: E402
import bo_reference as ref                 # noqa: E402
from tum_control_amd import bo             # noqa: E402


def test_cabi_exports_every_declared_bom_symbol():
    """The built library exports every tum_bom_ function include/tum_nmpc.h declares, and solver.BOM_SYMBOLS lists exactly those."""
    import re
    import __graft_entry__ as g
    from tum_control_amd import solver
    g.build()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tum_nmpc.h")).read()
    declared = sorted(set(re.findall(r"\b(tum_bom_\w+)\s*\(", hdr)))
    assert len(declared) == 9 and sorted(solver.BOM_SYMBOLS) == declared
    L = solver.load_library()
    for sym in declared:
        assert hasattr(L, sym), sym


@pytest.mark.parametrize("name, cls", [("tum_bom_prune_desc", bo._PruneDesc), ("tum_bom_build_desc", bo._BuildDesc)])
def test_descriptors_match_the_header(name, cls):
    """The ctypes descriptors of bo.py are the header's field for field (the device tests check their sizes against the library's)."""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tum_nmpc.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(int|double)\s+", "", decl.strip())
        names += [re.sub(r"[\*\s]|\[\d+\]", "", p) for p in decl.split(",") if p.strip()]
    assert names == [f[0] for f in cls._fields_]


@pytest.mark.parametrize("shape", mref.PRUNE_SHAPES, ids=lambda s: "n%d_d%d_S%d_seed%d" % s)
def test_numpy_prune_draws_against_long_double(shape):
    """bo.prune_draws and the torch statement against the long-double chain. Both FP64 statements factor a matrix whose condition
    number reaches 1e5: a few thousand u is their own error; 1e6 u (1e-10 of the scale) would be a wrong formula."""
    fx = mref.prune_fixture(*shape)
    F_ld = mref.longdouble_draws(fx)
    e_host = mref.error(mref.host_draws(fx), F_ld)
    e_torch = mref.error(mref.torch_prune_draws(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"]), F_ld)
    print(f"bo_model_host n={shape[0]} d={shape[1]} S={shape[2]} F: host {e_host:.2f} torch {e_torch:.2f} (u x scale)")
    assert e_host < 1e6 and e_torch < 1e6


def _old_prune_baseline(Xt, Y, obj_hyp, S=1024, seed=0, jitter=1e-8):
    """prune_baseline as it stood before its two halves got names: the bits the default must still return."""
    Xt = np.atleast_2d(np.asarray(Xt, dtype=np.float64))
    n = len(Xt)
    Zs = bo.sobol_normal(S, 2 * n, seed).reshape(S, 2, n)
    F = np.zeros((S, n, 2))
    for o in range(2):
        V, a = bo.gp_factor(Xt, Y[:, o], obj_hyp[o])
        K = bo.rbf(Xt, Xt, obj_hyp[o].ils, obj_hyp[o].s)
        Hm = K @ V.T
        Sig = K - Hm @ Hm.T
        L = np.linalg.cholesky(0.5 * (Sig + Sig.T) + max(jitter, 1e-6 * obj_hyp[o].s) * np.eye(n))
        F[:, :, o] = obj_hyp[o].c + K @ a + Zs[:, o] @ L.T
    keep = np.zeros(n, dtype=bool)
    for s in range(S):
        ge = (F[s, None, :, :] >= F[s, :, None, :]).all(-1)
        gt = (F[s, None, :, :] > F[s, :, None, :]).any(-1)
        keep |= ~(ge & gt).any(1)
    return np.flatnonzero(keep), F


@pytest.mark.parametrize("shape", mref.PRUNE_SHAPES[1:], ids=lambda s: "n%d_d%d_S%d_seed%d" % s)
def test_default_is_the_host_path_bit_for_bit(shape):
    n, d, S, seed = shape
    fx = mref.prune_fixture(*shape)
    old, F_old = _old_prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=S, seed=seed, jitter=fx["jitter"])
    default = bo.prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=S, seed=seed, jitter=fx["jitter"])
    host = bo.prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=S, seed=seed, jitter=fx["jitter"], backend="host")
    assert (default == old).all() and (host == old).all() and len(default) == len(old)
    assert (mref.host_draws(fx) == F_old).all()
    assert (np.flatnonzero(bo.dominance_keep(F_old)) == old).all()


def test_unknown_backends_are_refused():
    fx = mref.prune_fixture(*mref.PRUNE_SHAPES[1])
    with pytest.raises(ValueError, match="backend"):
        bo.prune_baseline(fx["Xt"], fx["Ys"], fx["obj"], S=8, backend="gpu")
    with pytest.raises(ValueError, match="model_backend"):
        bo.BayesianOptimization(np.array([[0.0], [1.0]]), {}, lambda x: None, acq="host", model_backend="gpu")
    with pytest.raises(ValueError, match="needs acq"):
        bo.BayesianOptimization(np.array([[0.0], [1.0]]), {}, lambda x: None, acq="host", model_backend="device")
    m = ref.generate(2, 5, 3, 9, 4, 8, seed=1)
    with pytest.raises(ValueError, match="baseline"):
        bo.pack_model(m.Xt, np.zeros((5, 2)), *ref.hypers(2)[:1], m.Xc, np.ones(9, dtype=bool), ref.hypers(2)[1], m.Xb, m.Zfull, m.ref, baseline="gpu")
    b = bo.BayesianOptimization(np.array([[0.0], [1.0]]), {}, lambda x: None, acq="host")
    assert b.model_backend == "host"


def _robust(fx, label):
    m = mref.margins(mref.host_draws(fx))
    keep = bo.dominance_keep(mref.host_draws(fx))
    print(f"bo_model_margin {label}: kept {int(keep.sum())} of {len(m)}, smallest |m_i| {np.abs(m).min():.2e}")
    assert ((m >= 0) == keep).all()
    assert (np.abs(m) > mref.ROBUST).all(), (label, float(np.abs(m).min()))


@pytest.mark.parametrize("shape", mref.PRUNE_SHAPES, ids=lambda s: "n%d_d%d_S%d_seed%d" % s)
def test_margin_condition_of_the_pruning_fixtures(shape):
    _robust(mref.prune_fixture(*shape), "n=%d d=%d S=%d seed=%d" % shape)


def test_margin_condition_of_the_campaign_fixture(golden_dir):
    _robust(mref.campaign_fixture(golden_dir), "campaign n=194 S=%d seed=%d" % (mref.CAMPAIGN_S, mref.CAMPAIGN_SEED))


def test_pack_model_default_is_the_host_baseline_and_the_device_model_carries_inputs_only():
    rng = np.random.default_rng(4)
    Xc = rng.random((30, 3))
    feas = np.arange(30) < 12
    Y = rng.standard_normal((12, 2))
    obj, cls = ref.hypers(3)
    Z = bo.sobol_normal(16, 2 * 9, 1).reshape(16, 2, -1).transpose(0, 2, 1)
    args = (Xc[:12], Y, obj, Xc, feas, cls, Xc[:7], Z, np.array([-1.5, -1.5]))
    default, host, dev = bo.pack_model(*args), bo.pack_model(*args, baseline="host"), bo.pack_model(*args, baseline="device")
    for o in range(2):
        assert (default.H[o] == host.H[o]).all() and (default.R[o] == host.R[o]).all() and (default.L_b[o] == host.L_b[o]).all()
    assert (default.F_b == host.F_b).all() and (default.fronts == host.fronts).all() and not default.device_baseline
    assert dev.device_baseline and dev.H == [] and dev.R == [] and dev.F_b is None and dev.fronts is None
    assert all((dev.V[g] == host.V[g]).all() and (dev.a[g] == host.a[g]).all() for g in range(4)) and (dev.Zfull == host.Zfull).all()
    done = bo.complete_model(dev, dict(H=host.H, R=host.R, L_b=host.L_b, mu_b=host.mu_b, F_b=host.F_b, fronts=host.fronts,
                                       front_count=host.front_count))
    X = rng.random((5, 3))
    assert not done.device_baseline and (bo.host_acquisition(done, X) == bo.host_acquisition(host, X)).all()


@pytest.mark.parametrize("shape", mref.BUILD_SHAPES[:3] + mref.BUILD_SHAPES[5:], ids=lambda s: "d%d_t%d_b%d_c%d_S%d" % s)
def test_numpy_baseline_against_long_double(shape):
    """pack_model's baseline statements and the torch ones against the long-double chain B; the factored covariance has a condition
    number up to s / jitter = 1.3e6: an error of 64 (s / jitter) u would be a wrong formula, not rounding."""
    host, _ = mref.build_fixture(shape)
    want = mref.longdouble_build(host)
    e_host = mref.build_errors(dict(H=host.H, R=host.R, L_b=host.L_b, mu_b=host.mu_b, F_b=host.F_b), want)
    e_torch = mref.build_errors(mref.torch_build(host), want)
    bound = 64.0 * float(host.s[:2].max() / host.jitter.min())
    for n in mref.BUILD_ARRAYS:
        print(f"bo_model_host build {shape} {n}: host {e_host[n]:.2f} torch {e_torch[n]:.2f} (u x scale)")
        assert e_host[n] < bound and e_torch[n] < bound


def test_margins_state_the_dominance_rule():
    """Integer draws with many ties: wherever the margin is not zero its sign is the rule's verdict; equal rows keep each other."""
    F = np.random.default_rng(3).integers(0, 4, size=(5, 12, 2)).astype(np.float64)
    m, keep = mref.margins(F), bo.dominance_keep(F)
    assert (keep[m > 0]).all() and (~keep[m < 0]).all()
    same = np.tile(np.array([[1.0, 2.0]]), (3, 7, 1))
    assert bo.dominance_keep(same).all() and (mref.margins(same) == 0).all()


def test_front_rule_without_a_sort_is_front_2d():
    """The rule csrc/bo_model_kernels.hpp uses (no sort: a point is on the front where no point the sort puts before it has an
    objective 1 at least as large; its row is the number of front points with a smaller objective 0) against bo.front_2d, on integer
    draws with duplicates and equal objective-0 values."""
    rng = np.random.default_rng(11)
    for nb in (1, 2, 5, 16, 17, 40):
        for _ in range(20):
            Y = rng.integers(0, 6, size=(nb, 2)).astype(np.float64)
            r = np.array([0.5, 1.5])
            valid = (Y[:, 0] > r[0]) & (Y[:, 1] > r[1])
            on = valid.copy()
            for i in range(nb):
                for j in range(nb):
                    before = Y[j, 0] > Y[i, 0] or (Y[j, 0] == Y[i, 0] and (Y[j, 1] > Y[i, 1] or (Y[j, 1] == Y[i, 1] and j < i)))
                    if valid[j] and before and Y[j, 1] >= Y[i, 1]:
                        on[i] = False
            out = np.zeros((int(on.sum()), 2))
            for i in np.flatnonzero(on):
                out[int((on & (Y[:, 0] < Y[i, 0])).sum())] = Y[i]
            want = bo.front_2d(Y, r)
            assert out.shape == want.shape and (out == want).all()
