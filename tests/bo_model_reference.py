"""
bo_model_reference.py -- the independent yardsticks of the parts of the acquisition model the device builds (tum_control_amd/bo.py
prune_draws / dominance_keep / build_fronts; csrc/bo_model_kernels.hpp behind tum_bom_prune and tum_bom_fronts).

  longdouble_prune_draws(...)    the pruning chain of include/tum_nmpc.h (K17) in np.longdouble: kernel matrix, H = K V^T, the
                                 symmetrised posterior covariance with its jitter, its Cholesky factor (gp_reference.cholesky, the
                                 column algorithm written out), the mean and the draws. The GP factors V, a are INPUTS, as they are for
                                 the device: their conditioning is not the error of the code under test.
  torch_prune_draws(...)         the second FP64 statement, in torch on the CPU (scaled coordinates, torch.linalg.cholesky, matmul).
  margins(F)                     m_i = max_s min_{j != i} max_o (F[s,i,o] - F[s,j,o]): trial i is kept iff m_i >= 0; a trial with
                                 |m_i| > ROBUST keeps its verdict under any error the draws can carry.
  prune_fixture(n, d, S, seed)   seeded trials in the recipe of bo_reference.generate with bo_reference.hypers, factored on the host.
  campaign_fixture(golden_dir)   the 194 feasible trials of tests/golden/bo_trials_F.npz, S = 1024.
  error(got, want)               largest error in units of u x the array's scale (its largest magnitude in the reference).
"""
import os

import numpy as np

from bo_reference import LD, U, _mm, _rbf_ld, hypers
from gp_reference import cholesky

ROBUST = 1e-6
# n, d, S, seed: one trial; both sides of the 16-row tile and the 64-row block; three block columns; S below and off the wavefront
# size; d at both limits
PRUNE_SHAPES = [(1, 2, 8, 5), (15, 1, 33, 6), (17, 1, 33, 1), (63, 16, 1, 7), (65, 3, 100, 2), (130, 7, 100, 3)]
CAMPAIGN_S, CAMPAIGN_SEED = 1024, 4


def _jitter(jitter, s):
    return max(jitter, 1e-6 * s)


def longdouble_prune_draws(Xt, V, a, obj_hyp, Zs, jitter=1e-8):
    n, S = len(Xt), len(Zs)
    F = np.zeros((S, n, 2), dtype=LD)
    for o in range(2):
        h = obj_hyp[o]
        K = _rbf_ld(Xt, Xt, h.ils, h.s)
        H = _mm(K, np.asarray(V[o], dtype=LD).T)
        Sig = K - _mm(H, H.T)
        A = LD(0.5) * (Sig + Sig.T) + LD(_jitter(jitter, h.s)) * np.eye(n, dtype=LD)
        L = cholesky(A)
        m = LD(h.c) + _mm(K, np.asarray(a[o], dtype=LD)[:, None])[:, 0]
        F[:, :, o] = m[None, :] + _mm(np.asarray(Zs[:, o], dtype=LD), L.T)
    return F


def torch_prune_draws(Xt, V, a, obj_hyp, Zs, jitter=1e-8):
    import torch
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)          # noqa: E731
    n, S = len(Xt), len(Zs)
    F = torch.zeros((S, n, 2), dtype=torch.float64)
    for o in range(2):
        h = obj_hyp[o]
        Xs = t(Xt) * t(h.ils)
        D = Xs[:, None, :] - Xs[None, :, :]
        K = h.s * torch.exp(-0.5 * (D * D).sum(-1))
        H = torch.matmul(K, t(V[o]).T)
        Sig = K - torch.matmul(H, H.T)
        L = torch.linalg.cholesky(0.5 * (Sig + Sig.T) + _jitter(jitter, h.s) * torch.eye(n, dtype=torch.float64))
        F[:, :, o] = (h.c + torch.matmul(K, t(a[o])))[None, :] + torch.matmul(t(Zs[:, o]), L.T)
    return F.numpy()


def margins(F):
    F = np.asarray(F, dtype=np.float64)
    S, n, _ = F.shape
    m = np.full(n, -np.inf)
    for s in range(S):
        D = (F[s, :, None, :] - F[s, None, :, :]).max(-1)
        D[np.diag_indices(n)] = np.inf
        m = np.maximum(m, D.min(1))
    return m


def error(got, want):
    want = np.asarray(want, dtype=LD)
    scale = float(np.abs(want).max())
    scale = scale if scale > 0 else 1.0
    return float(np.abs(np.asarray(got).astype(LD) - want).max() / (U * scale))


_FIXTURES = {}


def _factored(key, Xt, Ys, S, seed, jitter):
    from tum_control_amd import bo
    obj = hypers(Xt.shape[1])[0]
    n = len(Xt)
    Zs = bo.sobol_normal(S, 2 * n, seed).reshape(S, 2, n)
    V, a = zip(*(bo.gp_factor(Xt, Ys[:, o], obj[o]) for o in range(2)))
    _FIXTURES[key] = dict(Xt=Xt, Ys=Ys, obj=obj, Zs=Zs, V=V, a=a, jitter=jitter, S=S, seed=seed)
    return _FIXTURES[key]


def prune_fixture(n, d, S, seed, jitter=1e-8):
    """bo_reference.generate's trials (n_c = n_t = n): uniform points, two smooth objectives with noise, standardised."""
    key = (n, d, S, seed)
    if key in _FIXTURES:
        return _FIXTURES[key]
    from tum_control_amd import bo
    rng = np.random.default_rng(seed)
    Xt = rng.random((n, d))
    Y = np.stack([-((Xt - 0.3) ** 2).sum(1), -((Xt - 0.7) ** 2).sum(1)], axis=1) * (4.0 / d) + 0.05 * rng.standard_normal((n, 2))
    Ys = bo.standardize(Y)[0] if n > 1 else Y
    return _factored(key, Xt, Ys, S, seed, jitter)


def campaign_fixture(golden_dir):
    key = "campaign"
    if key in _FIXTURES:
        return _FIXTURES[key]
    from tum_control_amd import bo
    z = np.load(os.path.join(golden_dir, "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"], z["feasible"], z["objectives"]
    Xt = np.ascontiguousarray(Xn[feas])
    assert len(Xt) == 194
    return _factored(key, Xt, bo.standardize(obj[feas][:, 0, :])[0], CAMPAIGN_S, CAMPAIGN_SEED, 1e-8)


def host_draws(fx):
    """bo.prune_draws of a fixture, computed once."""
    if "F_host" not in fx:
        from tum_control_amd import bo
        fx["F_host"] = bo.prune_draws(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    return fx["F_host"]


def longdouble_draws(fx):
    if "F_ld" not in fx:
        fx["F_ld"] = longdouble_prune_draws(fx["Xt"], fx["V"], fx["a"], fx["obj"], fx["Zs"], fx["jitter"])
    return fx["F_ld"]


# ------------------------------------------------------------------------------------------------ the built baseline (tum_bom_build)
# d, n_t, n_b, n_c, S: one baseline point; both sides of the 16-row tile and of the 64-row block; n_b > n_t once
BUILD_SHAPES = [(2, 5, 1, 9, 1), (3, 40, 15, 60, 33), (3, 40, 17, 60, 64), (7, 130, 64, 300, 100), (7, 130, 65, 300, 100), (2, 9, 20, 30, 16)]
BUILD_ARRAYS = ("H", "R", "L_b", "mu_b", "F_b")


def build_fixture(shape):
    """(the model bo.pack_model builds on the host, the same inputs packed with baseline='device'), once per shape."""
    key = ("build",) + tuple(shape)
    if key not in _FIXTURES:
        from dataclasses import replace
        from bo_reference import generate
        d, n_t, n_b, n_c, S = shape
        host = generate(d, n_t, n_b, n_c, S, 8, seed=sum(shape), q=3)
        dev = replace(host, H=[], R=[], L_b=[], mu_b=[], F_b=None, fronts=None, front_count=None, device_baseline=True)
        _FIXTURES[key] = (host, dev)
    return _FIXTURES[key]


def longdouble_build(m):
    """Chain B of include/tum_nmpc.h (K17) in long double from the inputs of the model m: the fields of PackedModel it fills."""
    from bo_reference import forward_substitution
    from tum_control_amd import bo
    nb = m.n_b
    out = dict(H=[], R=[], L_b=[], mu_b=[], F_b=np.zeros((m.S, nb, 2), dtype=LD))
    for o in range(2):
        Kbt = _rbf_ld(m.Xb, m.Xt, m.ils[o], m.s[o])
        H = _mm(Kbt, np.asarray(m.V[o], dtype=LD).T)
        Sbb = _rbf_ld(m.Xb, m.Xb, m.ils[o], m.s[o]) - _mm(H, H.T)
        L = cholesky(LD(0.5) * (Sbb + Sbb.T) + LD(m.jitter[o]) * np.eye(nb, dtype=LD))
        mu = LD(m.c[o]) + _mm(Kbt, np.asarray(m.a[o], dtype=LD)[:, None])[:, 0]
        out["H"].append(H); out["L_b"].append(L); out["R"].append(forward_substitution(L, np.eye(nb, dtype=LD))); out["mu_b"].append(mu)
        out["F_b"][:, :, o] = mu[None, :] + _mm(np.asarray(m.Z(o), dtype=LD), L.T)
    out["fronts"], out["front_count"] = bo.build_fronts(out["F_b"], m.ref)
    return out


def torch_build(m):
    """The second FP64 statement of chain B, in torch on the CPU."""
    import torch
    from tum_control_amd import bo
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)          # noqa: E731
    nb = m.n_b
    out = dict(H=[], R=[], L_b=[], mu_b=[], F_b=np.zeros((m.S, nb, 2)))

    def kern(A, B, o):
        ils = t(m.ils[o])
        D = (t(A) * ils)[:, None, :] - (t(B) * ils)[None, :, :]
        return m.s[o] * torch.exp(-0.5 * (D * D).sum(-1))
    for o in range(2):
        Kbt = kern(m.Xb, m.Xt, o)
        H = torch.matmul(Kbt, t(m.V[o]).T)
        Sbb = kern(m.Xb, m.Xb, o) - torch.matmul(H, H.T)
        L = torch.linalg.cholesky(0.5 * (Sbb + Sbb.T) + float(m.jitter[o]) * torch.eye(nb, dtype=torch.float64))
        R = torch.linalg.solve_triangular(L, torch.eye(nb, dtype=torch.float64), upper=False)
        mu = m.c[o] + torch.matmul(Kbt, t(m.a[o]))
        out["H"].append(H.numpy()); out["L_b"].append(L.numpy()); out["R"].append(np.tril(R.numpy())); out["mu_b"].append(mu.numpy())
        out["F_b"][:, :, o] = (mu[None, :] + torch.matmul(t(m.Z(o)), L.T)).numpy()
    out["fronts"], out["front_count"] = bo.build_fronts(out["F_b"], m.ref)
    return out


def build_errors(arrays, want):
    """name -> the error of an array of the built baseline (the larger over the two objectives) in units of u x its scale."""
    e = {}
    for name in BUILD_ARRAYS:
        if name == "F_b":
            e[name] = error(arrays[name], want[name])
        else:
            e[name] = max(error(arrays[name][o], want[name][o]) for o in range(2))
    return e


# ------------------------------------------------------------------------------------------------ the appended pick (tum_bom_append)
def _append(m, arr, x, kind):
    """bo.append_pick restated on the arrays `arr` (the fields longdouble_build / torch_build return) of the model m (m.Xb is the baseline
    arr belongs to): kind "ld" in long double, "torch" in torch float64. Returns the arrays of the model with x appended."""
    from tum_control_amd import bo
    if kind == "ld":
        cv, mm = (lambda a: np.asarray(a, dtype=LD)), _mm
        rbf = lambda A, B, o: _rbf_ld(A, B, m.ils[o], m.s[o])          # noqa: E731
        sqrt, back = np.sqrt, (lambda a: a)
    else:
        import torch
        cv = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))          # noqa: E731
        mm, sqrt, back = torch.matmul, torch.sqrt, (lambda a: a.numpy())

        def rbf(A, B, o):
            D = (cv(A) * cv(m.ils[o]))[:, None, :] - (cv(B) * cv(m.ils[o]))[None, :, :]
            return float(m.s[o]) * torch.exp(-0.5 * (D * D).sum(-1))
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    nb, S = m.n_b, m.S
    out = dict(H=[], R=[], L_b=[], mu_b=[], F_b=np.zeros((S, nb + 1, 2), dtype=LD if kind == "ld" else np.float64))
    for o in range(2):
        kt = rbf(m.Xt, x, o)
        q = mm(cv(m.V[o]), kt)
        mu = cv(m.c[o]) + mm(cv(m.a[o])[None, :], kt)[0, 0]
        H, R, L = cv(arr["H"][o]), cv(arr["R"][o]), cv(arr["L_b"][o])
        l = mm(R, rbf(m.Xb, x, o) - mm(H, q))
        d2 = cv(m.s[o]) - (q * q).sum() - (l * l).sum()
        d2 = d2 if d2 > m.jitter[o] else cv(m.jitter[o])
        lam = sqrt(d2)
        Ln = np.zeros((nb + 1, nb + 1), dtype=out["F_b"].dtype); Rn = np.zeros_like(Ln)
        Ln[:nb, :nb], Ln[nb, :nb], Ln[nb, nb] = back(L), back(l[:, 0]), back(lam)
        Rn[:nb, :nb], Rn[nb, :nb], Rn[nb, nb] = back(R), back(-mm(l.T, R)[0] / lam), back(1 / lam)
        out["H"].append(np.vstack([back(H), back(q.T)])); out["L_b"].append(Ln); out["R"].append(Rn)
        out["mu_b"].append(np.append(back(cv(arr["mu_b"][o])), back(mu)))
        Z, zeta = cv(m.Zfull[:, :nb, o]), cv(m.Zfull[:, nb, o])
        out["F_b"][:, :nb, o] = np.asarray(arr["F_b"])[:, :, o]
        out["F_b"][:, nb, o] = back(mu + mm(Z, l)[:, 0] + lam * zeta)
    out["fronts"], out["front_count"] = bo.build_fronts(out["F_b"], m.ref)
    return out


def longdouble_append(m, arr, x):
    return _append(m, arr, x, "ld")


def torch_append(m, arr, x):
    return _append(m, arr, x, "torch")
