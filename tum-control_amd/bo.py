"""
bo.py -- the Bayesian-optimisation half of Learning_To_Adapt/SafeRL_WMPC (bo_optimize.py, BO_WMPC/): surrogate models, the
feasibility-weighted expected hypervolume improvement, candidate selection and the driver, with closed_loop.evaluate_segments as
the objective. The acquisition value of a batch of candidates runs on the device (csrc/bo_kernels.hpp behind tum_bo_evaluate);
everything around it is torch float64 / numpy on the host. botorch and gpytorch are not used: this is the project's own statement
of the same mathematics (INTEGRATION.md lists the differences).

  fit_gp, ObjectiveModel, ConstraintModel      exact GPs with ARD RBF kernels, fitted by L-BFGS on the marginal log-likelihood
  gp_mll_grad_host, DeviceGP                    likelihood, gradient and factor of one GP: numpy statement and the device path
  pack_model, append_pick                       the arrays tum_bo_model takes; a pick appended to the baseline without refactoring
  host_acquisition, HostAcquisition             numpy statement of the acquisition value (the CPU path)
  DeviceAcquisition                             the device path
  select                                        sequential greedy picks: Sobol raw samples, restarts, batched compass search
  pareto_mask, hypervolume_2d, prune_baseline   front utilities; prune_draws / dominance_keep are prune_baseline's two halves, which
                                                DeviceAcquisition.prune runs on the device (csrc/bo_model_kernels.hpp)
  load_trials, store_trials                     the reference's CSV line format
  BayesianOptimization                          the driver
"""
import ctypes
import time
from dataclasses import dataclass, field, replace

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import ndtri
from scipy.stats import qmc

N_MAX, NB_MAX, S_MAX, K_MAX, D_MAX = 4096, 512, 4096, 64, 16
DETAIL = ("mu_0", "mu_1", "d2_0", "d2_1", "hvi", "p", "sd", "factor")


class ModelFittingError(Exception):
    """A surrogate model could not be fitted (the kernel matrix is not numerically positive definite)."""


# ------------------------------------------------------------------------------------------------ kernels and factors
@dataclass
class GPHyper:
    """Hyperparameters of one exact GP: constant mean, output scale, ARD length scales, noise (a scalar or one value per point)."""
    c: float
    s: float
    ls: np.ndarray
    noise: object = 1e-4

    @property
    def ils(self):
        return 1.0 / np.asarray(self.ls, dtype=np.float64)


def rbf(X1, X2, ils, s):
    """k(x,x') = s exp(-1/2 sum_j ((x_j - x'_j) ils_j)^2), the sum in index order."""
    X1, X2 = np.atleast_2d(X1), np.atleast_2d(X2)
    r = np.zeros((X1.shape[0], X2.shape[0]))
    for j in range(X1.shape[1]):
        t = (X1[:, j, None] - X2[None, :, j]) * ils[j]
        r += t * t
    return s * np.exp(-0.5 * r)


def _chol(A, what):
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError as e:
        raise ModelFittingError(f"{what}: {e}") from None
    if not np.isfinite(L).all():
        raise ModelFittingError(f"{what}: non-finite Cholesky factor")
    return L


def _tri_inv(L):
    return np.tril(solve_triangular(L, np.eye(L.shape[0]), lower=True))


def gp_factor(X, y, hyp):
    """A = K + noise = L L^T  ->  V = L^-1 (lower), a = A^-1 (y - c)."""
    A = rbf(X, X, hyp.ils, hyp.s)
    A[np.diag_indices_from(A)] += np.broadcast_to(np.asarray(hyp.noise, dtype=np.float64), (len(X),))
    V = _tri_inv(_chol(A, "GP kernel matrix"))
    return V, V.T @ (V @ (np.asarray(y, dtype=np.float64) - hyp.c))


def gauss_hermite(K):
    """The K-node rule for a standard normal: E g(t) ~ sum w g(m + sd x)."""
    x, w = np.polynomial.hermite.hermgauss(int(K))
    return x * np.sqrt(2.0), w / np.sqrt(np.pi)


def dirichlet_targets(feasible, alpha_eps=0.001):
    """surrogate_models.py:66-160: alpha_ik = alpha_eps + [y_i = k]; fixed noise log(1 / alpha + 1); targets log alpha - noise / 2.
    Returns targets (n x 2) and fixed noise (n x 2)."""
    y = np.asarray(feasible).astype(int)
    alpha = alpha_eps + np.stack([y == 0, y == 1], axis=1).astype(np.float64)
    noise = np.log(1.0 / alpha + 1.0)
    return np.log(alpha) - 0.5 * noise, noise


# ------------------------------------------------------------------------------------------------ front utilities
def pareto_mask(Y):
    """Non-dominated rows of Y (n x m, maximised): no other row is >= everywhere and > somewhere. Equal rows are all kept."""
    Y = np.asarray(Y, dtype=np.float64)
    keep = np.ones(len(Y), dtype=bool)
    for i in range(len(Y)):
        keep[i] = not ((Y >= Y[i]).all(axis=1) & (Y > Y[i]).any(axis=1)).any()
    return keep


def front_2d(Y, ref):
    """The 2-D front of Y above ref: strictly better than ref in both objectives and non-dominated, ascending in objective 0."""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    Y = Y[(Y[:, 0] > ref[0]) & (Y[:, 1] > ref[1])]
    if not len(Y):
        return Y
    Y = Y[np.lexsort((-Y[:, 1], -Y[:, 0]))]          # objective 0 descending, then objective 1 descending
    best = np.maximum.accumulate(np.concatenate([[-np.inf], Y[:-1, 1]]))
    return Y[Y[:, 1] > best][::-1]


def hypervolume_2d(Y, ref):
    """The area dominated by Y and bounded below by ref."""
    F = front_2d(Y, ref)
    hv, xp = 0.0, ref[0]
    for x, y in F:
        hv += (x - xp) * (y - ref[1])
        xp = x
    return float(hv)


def hvi_2d(F, ref, f):
    """The hypervolume improvement of the point f over the front F (as front_2d returns it): the cell formula of the device."""
    hv, xp = 0.0, ref[0]
    for x, h in F:
        hv += max(0.0, min(f[0], x) - xp) * max(0.0, f[1] - h)
        xp = x
    return hv + max(0.0, f[0] - xp) * max(0.0, f[1] - ref[1])


def build_fronts(F_b, ref, P_max=None):
    """F_b: S x n_b x 2 baseline draws -> fronts (S x P_max x 2, rows behind the count repeat nothing: zero) and counts (S)."""
    S, nb, _ = F_b.shape
    P_max = nb if P_max is None else P_max
    fronts, count = np.zeros((S, P_max, 2)), np.zeros(S, dtype=np.int32)
    for s in range(S):
        F = front_2d(F_b[s], ref)
        count[s] = len(F)
        fronts[s, :len(F)] = F
    return fronts, count


def _rng(seed):
    """A numpy Generator from an int or a sequence of ints."""
    return np.random.default_rng(np.random.SeedSequence(seed))


def sobol_points(n, d, seed):
    """n scrambled Sobol points in [0,1]^d (scipy.stats.qmc; n need not be a power of two)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return qmc.Sobol(d=int(d), scramble=True, seed=_rng(seed)).random(int(n))


def sobol_normal(S, ncol, seed):
    """S x ncol standard normals from one scrambled Sobol sequence (scipy.stats.qmc), through the inverse normal CDF."""
    u = sobol_points(S, ncol, seed)
    return ndtri(np.clip(u, 1e-12, 1.0 - 1e-12))


# ------------------------------------------------------------------------------------------------ the packed model
@dataclass
class PackedModel:
    """Everything tum_bo_model takes (names of include/tum_nmpc.h) and what appending a pick needs beside it."""
    d: int
    Xt: np.ndarray
    Xb: np.ndarray
    Xc: np.ndarray
    ils: list          # 4 x (d)
    s: np.ndarray      # 4
    c: np.ndarray      # 4
    a: list            # 4
    V: list            # 4
    jitter: np.ndarray
    H: list
    R: list
    Zfull: np.ndarray  # S x ncol x 2 base samples: columns 0 .. n_b - 1 drive the baseline, column n_b is zeta
    ref: np.ndarray
    eps: float
    gh_x: np.ndarray
    gh_w: np.ndarray
    mu_b: list = field(default_factory=list)
    L_b: list = field(default_factory=list)
    F_b: np.ndarray = None          # S x n_b x 2
    fronts: np.ndarray = None
    front_count: np.ndarray = None
    device_baseline: bool = False          # H, R, L_b, mu_b, F_b and the fronts are not here: DeviceAcquisition.set_model builds them

    @property
    def n_b(self):
        return len(self.Xb)

    @property
    def S(self):
        return self.Zfull.shape[0]

    def Z(self, o):
        return np.ascontiguousarray(self.Zfull[:, :self.n_b, o])

    def zeta(self, o):
        return np.ascontiguousarray(self.Zfull[:, self.n_b, o])


def pack_model(Xt, Y, obj_hyp, Xc, feasible, cls_hyp, Xb, Z, ref, eps=0.8, jitter=1e-8, K=64, alpha_eps=0.001, factor=None, baseline="host"):
    """Xt (n_t x d) feasible trials with Y (n_t x 2, the units the GPs model); obj_hyp two GPHyper; Xc (n_c x d) all trials with their
    feasibility flags; cls_hyp two GPHyper whose noise is the LEARNED extra noise (the fixed Dirichlet noise is added here); Xb the
    baseline; Z (S x ncol x 2, ncol >= n_b + 1) base samples; ref the reference point in the units of Y. factor: what forms the four
    (V, a), gp_factor by default or a callable of its signature such as DeviceGP.gp_factor. baseline "device": the model carries the
    inputs and the flag device_baseline, and no H, R, L_b, mu_b, F_b or fronts: DeviceAcquisition.set_model builds those on the device
    (tum_bom_build) and model_arrays() reads them back; complete_model joins the two."""
    if baseline not in ("host", "device"):
        raise ValueError(f"pack_model: baseline {baseline!r} is neither 'host' nor 'device'")
    Xt, Xb, Xc = (np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64))) for a in (Xt, Xb, Xc))
    Y = np.asarray(Y, dtype=np.float64).reshape(len(Xt), 2)
    d = Xt.shape[1]
    if Z.shape[1] < len(Xb) + 1:
        raise ValueError("pack_model: the base samples need n_b + 1 columns")
    targets, fixed = dirichlet_targets(feasible, alpha_eps)
    hyps = [obj_hyp[0], obj_hyp[1]] + [replace(cls_hyp[k], noise=fixed[:, k] + np.asarray(cls_hyp[k].noise)) for k in range(2)]
    factor = gp_factor if factor is None else factor
    V, a = [], []
    for g, h in enumerate(hyps):
        Vg, ag = factor(Xt if g < 2 else Xc, Y[:, g] if g < 2 else targets[:, g - 2], h)
        V.append(Vg); a.append(ag)
    jit = np.broadcast_to(np.asarray(jitter, dtype=np.float64), (2,)).copy()
    gh_x, gh_w = gauss_hermite(K)
    m = PackedModel(d=d, Xt=Xt, Xb=Xb, Xc=Xc, ils=[np.ascontiguousarray(h.ils) for h in hyps], s=np.array([h.s for h in hyps], dtype=np.float64),
                    c=np.array([h.c for h in hyps], dtype=np.float64), a=a, V=V, jitter=jit, H=[], R=[], Zfull=np.ascontiguousarray(Z, dtype=np.float64),
                    ref=np.asarray(ref, dtype=np.float64).copy(), eps=float(eps), gh_x=gh_x, gh_w=gh_w)
    if baseline == "device":
        m.device_baseline = True
        return m
    nb = len(Xb)
    m.F_b = np.zeros((m.S, nb, 2))
    for o in range(2):
        Kbt = rbf(Xb, Xt, m.ils[o], m.s[o])
        H = Kbt @ V[o].T
        Sbb = rbf(Xb, Xb, m.ils[o], m.s[o]) - H @ H.T
        L = _chol(0.5 * (Sbb + Sbb.T) + jit[o] * np.eye(nb), "baseline posterior covariance")
        m.H.append(np.ascontiguousarray(H)); m.R.append(_tri_inv(L)); m.L_b.append(L)
        m.mu_b.append(m.c[o] + Kbt @ a[o])
        m.F_b[:, :, o] = m.mu_b[o] + m.Z(o) @ L.T
    m.fronts, m.front_count = build_fronts(m.F_b, m.ref)
    return m


def complete_model(m, arrays):
    """A model packed with baseline="device" and the arrays DeviceAcquisition.model_arrays() read back: the model pack_model's host
    path returns, with the device's numbers."""
    return replace(m, device_baseline=False, **arrays)


def _candidate_terms(m, X):
    """Per objective mu, q, l, d2 of the candidates X (C x d) -- the numpy statement of the device's chain."""
    out = []
    for o in range(2):
        kt = rbf(m.Xt, X, m.ils[o], m.s[o])
        q = m.V[o] @ kt
        mu = m.c[o] + m.a[o] @ kt
        sig = rbf(m.Xb, X, m.ils[o], m.s[o]) - m.H[o] @ q
        l = m.R[o] @ sig
        d2 = np.maximum(m.s[o] - (q * q).sum(0) - (l * l).sum(0), m.jitter[o])
        out.append((mu, q, l, d2))
    return out


def sigmoid(t):
    t = np.asarray(t, dtype=np.float64)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def feasibility_factor(m, X):
    """p = E sigmoid(t), sd = sqrt(E (sigmoid(t) - p)^2), factor = eps p + (1 - eps) sd, t ~ N(m_1 - m_0, v_0 + v_1)."""
    mk, vk = [], []
    for g in (2, 3):
        kc = rbf(m.Xc, X, m.ils[g], m.s[g])
        q = m.V[g] @ kc
        mk.append(m.c[g] + m.a[g] @ kc)
        vk.append(m.s[g] - (q * q).sum(0))
    mean, sd_t = mk[1] - mk[0], np.sqrt(np.maximum(vk[0] + vk[1], 0.0))
    sg = sigmoid(mean[:, None] + sd_t[:, None] * m.gh_x[None, :])
    p = sg @ m.gh_w
    sd = np.sqrt(((sg - p[:, None]) ** 2) @ m.gh_w)
    return p, sd, m.eps * p + (1.0 - m.eps) * sd


def host_acquisition(m, X, detail=False, chunk=256):
    """alpha (C) of the candidates X (C x d) and, with detail, the C x 8 rows of tum_bo_evaluate's detail_out."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    C, S = len(X), m.S
    alpha, det = np.zeros(C), np.zeros((C, 8))
    cnt, pmax = m.front_count, int(m.front_count.max()) if len(m.front_count) else 0
    # edges and heights of the cells left of the open one; behind a sample's count the edge repeats: cells of no width
    idx = np.minimum(np.arange(max(pmax, 1))[None, :], np.maximum(cnt[:, None] - 1, 0))
    ex = np.where(cnt[:, None] > 0, np.take_along_axis(m.fronts[:, :, 0], idx, 1), m.ref[0])
    eh = np.take_along_axis(m.fronts[:, :, 1], idx, 1)
    last = ex[:, -1] if pmax else np.full(S, m.ref[0])
    for c0 in range(0, C, chunk):
        Xc = X[c0:c0 + chunk]
        terms = _candidate_terms(m, Xc)
        f = [terms[o][0][None, :] + m.Z(o) @ terms[o][2] + np.sqrt(terms[o][3])[None, :] * m.zeta(o)[:, None] for o in range(2)]
        hv, xp = np.zeros_like(f[0]), np.full((S, 1), m.ref[0])
        for i in range(pmax):
            xn = ex[:, i, None]
            hv += np.maximum(np.minimum(f[0], xn) - xp, 0.0) * np.maximum(f[1] - eh[:, i, None], 0.0)
            xp = xn
        hv += np.maximum(f[0] - last[:, None], 0.0) * np.maximum(f[1] - m.ref[1], 0.0)
        mean_hv = hv.sum(0) / S
        p, sd, factor = feasibility_factor(m, Xc)
        alpha[c0:c0 + chunk] = factor * mean_hv
        det[c0:c0 + chunk] = np.stack([terms[0][0], terms[1][0], terms[0][3], terms[1][3], mean_hv, p, sd, factor], axis=1)
    return (alpha, det) if detail else alpha


def append_pick(m, x):
    """The model with x appended to the baseline, without refactoring: l and sqrt(d2) of x are the new row of L_b, its samples the new
    baseline draws, the next column of the base samples the new zeta; the fronts are rebuilt."""
    x = np.asarray(x, dtype=np.float64).reshape(1, m.d)
    nb = m.n_b
    if m.Zfull.shape[1] < nb + 2:
        raise ValueError("append_pick: the base samples have no column left")
    terms = _candidate_terms(m, x)
    new = replace(m, Xb=np.vstack([m.Xb, x]), H=[], R=[], L_b=[], mu_b=[])
    new.F_b = np.zeros((m.S, nb + 1, 2))
    for o in range(2):
        mu, q, l, d2 = (t[..., 0] if t.ndim > 1 else t[0] for t in terms[o])
        lam = np.sqrt(d2)
        L = np.zeros((nb + 1, nb + 1)); L[:nb, :nb] = m.L_b[o]; L[nb, :nb] = l; L[nb, nb] = lam
        R = np.zeros((nb + 1, nb + 1)); R[:nb, :nb] = m.R[o]; R[nb, :nb] = -(l @ m.R[o]) / lam; R[nb, nb] = 1.0 / lam
        new.H.append(np.ascontiguousarray(np.vstack([m.H[o], q[None, :]])))
        new.R.append(R); new.L_b.append(L); new.mu_b.append(np.append(m.mu_b[o], mu))
        new.F_b[:, :nb, o] = m.F_b[:, :, o]
        new.F_b[:, nb, o] = mu + m.Z(o) @ l + lam * m.zeta(o)
    new.fronts, new.front_count = build_fronts(new.F_b, new.ref)
    return new


def dominance_keep(F):
    """F: S x n x 2 draws -> the boolean mask of the rows that are non-dominated in at least one sample: i is dominated in sample s
    if some j is >= in both objectives and > in one. Equal rows keep each other."""
    keep = np.zeros(F.shape[1], dtype=bool)
    for s in range(F.shape[0]):
        ge = (F[s, None, :, :] >= F[s, :, None, :]).all(-1)
        gt = (F[s, None, :, :] > F[s, :, None, :]).any(-1)
        keep |= ~(ge & gt).any(1)
    return keep


def prune_draws(Xt, V, a, obj_hyp, Zs, jitter=1e-8):
    """The joint posterior draws prune_baseline judges: F (S x n x 2) from the factors (V, a) of the two objective GPs and the base
    samples Zs (S x 2 x n) -- the numpy statement of tum_bom_prune's chain."""
    n, S = len(Xt), len(Zs)
    F = np.zeros((S, n, 2))
    for o in range(2):
        K = rbf(Xt, Xt, obj_hyp[o].ils, obj_hyp[o].s)
        Hm = K @ V[o].T
        Sig = K - Hm @ Hm.T
        L = _chol(0.5 * (Sig + Sig.T) + max(jitter, 1e-6 * obj_hyp[o].s) * np.eye(n), "posterior covariance at the trials")
        F[:, :, o] = obj_hyp[o].c + K @ a[o] + Zs[:, o] @ L.T
    return F


def prune_baseline(Xt, Y, obj_hyp, S=1024, seed=0, jitter=1e-8, backend="host", acq=None, factor=None):
    """Indices of the feasible trials that are non-dominated in at least one of S joint posterior samples at the trials themselves.
    backend "device": the draws and the dominance step run on the device (DeviceAcquisition.prune; acq: the handle to use, created
    and closed here otherwise); the base samples and the two factors (factor: gp_factor or a callable of its signature) stay on the
    host. The host path is the default and returns what it returned."""
    if backend not in ("host", "device"):
        raise ValueError(f"prune_baseline: backend {backend!r} is neither 'host' nor 'device'")
    Xt = np.atleast_2d(np.asarray(Xt, dtype=np.float64))
    n = len(Xt)
    Zs = sobol_normal(S, 2 * n, seed).reshape(S, 2, n)
    factor = gp_factor if factor is None else factor
    V, a = zip(*(factor(Xt, Y[:, o], obj_hyp[o]) for o in range(2)))
    if backend == "host":
        return np.flatnonzero(dominance_keep(prune_draws(Xt, V, a, obj_hyp, Zs, jitter)))
    own = acq is None
    if own:
        acq = DeviceAcquisition()
    try:
        return np.flatnonzero(acq.prune(Xt, V, a, obj_hyp, Zs, jitter)[0])
    finally:
        if own:
            acq.close()


# ------------------------------------------------------------------------------------------------ evaluators
class HostAcquisition:
    """host_acquisition behind the evaluator interface of select()."""

    def set_model(self, model, keep_gp=False):
        self.model = model

    def evaluate(self, X, detail=False):
        return host_acquisition(self.model, X, detail=detail)

    def close(self):
        pass


class _ModelDesc(ctypes.Structure):
    _dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    _fields_ = [(n, ctypes.c_int) for n in ("d", "n_t", "n_b", "n_c", "S", "P_max", "K", "keep_gp")] + \
               [("eps", ctypes.c_double), ("ref", ctypes.c_double * 2), ("jitter", ctypes.c_double * 2),
                ("s", ctypes.c_double * 4), ("c", ctypes.c_double * 4),
                ("Xt", _dp), ("Xb", _dp), ("Xc", _dp), ("ils", _dp * 4), ("a", _dp * 4), ("V", _dp * 4),
                ("H", _dp * 2), ("R", _dp * 2), ("Z", _dp * 2), ("zeta", _dp * 2),
                ("fronts", _dp), ("front_count", _ip), ("gh_x", _dp), ("gh_w", _dp)]


class _BuildDesc(ctypes.Structure):
    _dp = ctypes.POINTER(ctypes.c_double)
    _fields_ = [(n, ctypes.c_int) for n in ("struct_size", "d", "n_t", "n_b", "n_c", "S", "ncol", "K")] + \
               [("eps", ctypes.c_double), ("ref", ctypes.c_double * 2), ("jitter", ctypes.c_double * 2),
                ("s", ctypes.c_double * 4), ("c", ctypes.c_double * 4),
                ("Xt", _dp), ("Xb", _dp), ("Xc", _dp), ("ils", _dp * 4), ("a", _dp * 4), ("V", _dp * 4),
                ("Zfull", _dp * 2), ("gh_x", _dp), ("gh_w", _dp)]


class _PruneDesc(ctypes.Structure):
    _dp = ctypes.POINTER(ctypes.c_double)
    _fields_ = [(n, ctypes.c_int) for n in ("struct_size", "n", "d", "S")] + \
               [("jitter", ctypes.c_double), ("F", _dp), ("Xt", _dp), ("s", ctypes.c_double * 2), ("c", ctypes.c_double * 2),
                ("ils", _dp * 2), ("V", _dp * 2), ("a", _dp * 2), ("Z", _dp * 2)]


class DeviceAcquisition:
    """The acquisition value on the device: tum_bo_create / tum_bo_model / tum_bo_evaluate, and the parts of its model the device
    builds: tum_bom_prune (prune, prune_given), tum_bom_fronts (fronts), tum_bom_build (set_model of a model packed with
    baseline="device"), tum_bom_append (append_pick) and tum_bom_model_read (model_arrays). There is no CPU fallback behind it."""

    def __init__(self, device=0):
        from . import solver
        self._L = solver.load_library()
        self._h = self._L.tum_bo_create(int(device))
        if not self._h:
            raise Exception("tum_bo_create: " + self._L.tum_ocp_last_error().decode())
        self.d = None
        self._built = None          # (S, n_b, n_t) of the resident model where tum_bom_build built it

    def _check(self, rc, what):
        if rc != 0:
            raise Exception(f"{what}: " + self._L.tum_ocp_last_error().decode())

    def set_model(self, m, keep_gp=False):
        dp = ctypes.POINTER(ctypes.c_double)
        hold = []          # the arrays the descriptor points into, alive until the call returns

        def ptr(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            hold.append(a)
            return a.ctypes.data_as(dp)
        if m.device_baseline:
            if keep_gp:
                raise Exception("tum_bom_build: a model whose baseline the device builds installs its GPs too (keep_gp is not for it)")
            return self._build(m, ptr)
        desc = _ModelDesc()
        desc.d, desc.n_t, desc.n_b, desc.n_c, desc.S = m.d, len(m.Xt), m.n_b, len(m.Xc), m.S
        desc.P_max, desc.K, desc.keep_gp, desc.eps = m.fronts.shape[1], len(m.gh_x), int(bool(keep_gp)), m.eps
        for o in range(2):
            desc.ref[o], desc.jitter[o] = m.ref[o], m.jitter[o]
            desc.H[o], desc.R[o], desc.Z[o], desc.zeta[o] = ptr(m.H[o]), ptr(m.R[o]), ptr(m.Z(o)), ptr(m.zeta(o))
        desc.Xb = ptr(m.Xb)
        if not keep_gp:
            desc.Xt, desc.Xc = ptr(m.Xt), ptr(m.Xc)
            for g in range(4):
                desc.s[g], desc.c[g] = m.s[g], m.c[g]
                desc.ils[g], desc.a[g], desc.V[g] = ptr(m.ils[g]), ptr(m.a[g]), ptr(m.V[g])
        desc.fronts, desc.gh_x, desc.gh_w = ptr(m.fronts), ptr(m.gh_x), ptr(m.gh_w)
        cnt = np.ascontiguousarray(m.front_count, dtype=np.int32)
        desc.front_count = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self._built = None
        self._check(self._L.tum_bo_model(self._h, ctypes.addressof(desc)), "tum_bo_model")
        self.d = m.d

    def _build(self, m, ptr):
        desc = _BuildDesc()
        self._L.tum_bom_build_desc_init(ctypes.addressof(desc))
        if desc.struct_size != ctypes.sizeof(_BuildDesc):
            raise Exception("tum_bom_build_desc: the library's descriptor is not the one bo.py declares")
        desc.d, desc.n_t, desc.n_b, desc.n_c, desc.S = m.d, len(m.Xt), m.n_b, len(m.Xc), m.S
        desc.ncol, desc.K, desc.eps = m.Zfull.shape[1], len(m.gh_x), m.eps
        desc.Xt, desc.Xb, desc.Xc, desc.gh_x, desc.gh_w = ptr(m.Xt), ptr(m.Xb), ptr(m.Xc), ptr(m.gh_x), ptr(m.gh_w)
        for o in range(2):
            desc.ref[o], desc.jitter[o], desc.Zfull[o] = m.ref[o], m.jitter[o], ptr(m.Zfull[:, :, o])
        for g in range(4):
            desc.s[g], desc.c[g] = m.s[g], m.c[g]
            desc.ils[g], desc.a[g], desc.V[g] = ptr(m.ils[g]), ptr(m.a[g]), ptr(m.V[g])
        ok = ctypes.c_int()
        self.d = self._built = None
        self._check(self._L.tum_bom_build(self._h, ctypes.addressof(desc), ctypes.byref(ok)), "tum_bom_build")
        if not ok.value:
            raise ModelFittingError("baseline posterior covariance: not positive definite on the device")
        self.d = m.d
        self._built = (m.S, m.n_b, len(m.Xt))

    def append_pick(self, x):
        """bo.append_pick on the device (tum_bom_append): x joins the baseline of the model set_model built there; nothing but x is
        uploaded. model_arrays() reads the appended model."""
        if self.d is None or self._built is None:
            raise Exception("tum_bom_append: no model built on the device (tum_bom_build first)")
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        if len(x) != self.d:
            raise Exception(f"tum_bom_append: x has {len(x)} entries, the model has d = {self.d}")
        ok = ctypes.c_int()
        self._check(self._L.tum_bom_append(self._h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(ok)), "tum_bom_append")
        S, nb, nt = self._built
        self._built = (S, nb + 1, nt)
        if not ok.value:
            raise ModelFittingError("append_pick: the appended point has no positive posterior variance on the device")

    def model_arrays(self):
        """What tum_bom_build left on the device, as the fields of PackedModel: H, R, L_b, mu_b (one per objective), F_b, fronts,
        front_count."""
        dp = ctypes.POINTER(ctypes.c_double)
        if self.d is None or self._built is None:
            raise Exception("tum_bom_model_read: no model built on the device (tum_bom_build first)")
        S, nb, nt = self._built
        H, R, L, mu = ([np.zeros(sh) for _ in range(2)] for sh in ((nb, nt), (nb, nb), (nb, nb), (nb,)))
        F_b, fronts, count, n_b = np.zeros((S, nb, 2)), np.zeros((S, nb, 2)), np.zeros(S, dtype=np.int32), ctypes.c_int()
        pair = lambda arrs: (dp * 2)(*(x.ctypes.data_as(dp) for x in arrs))          # noqa: E731
        pairs = [pair(x) for x in (H, R, L, mu)]
        self._check(self._L.tum_bom_model_read(self._h, *(ctypes.addressof(x) for x in pairs), F_b.ctypes.data_as(dp), fronts.ctypes.data_as(dp),
                                               count.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(n_b)), "tum_bom_model_read")
        assert n_b.value == nb
        return dict(H=H, R=R, L_b=L, mu_b=mu, F_b=F_b, fronts=fronts, front_count=count)

    def evaluate(self, X, detail=False):
        X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        if self.d is not None and X.shape[1] != self.d:
            raise Exception(f"tum_bo_evaluate: X has {X.shape[1]} columns, the model has d = {self.d}")
        dp = ctypes.POINTER(ctypes.c_double)
        alpha = np.zeros(len(X))
        det = np.zeros((len(X), 8)) if detail else None
        self._check(self._L.tum_bo_evaluate(self._h, X.ctypes.data_as(dp), len(X), alpha.ctypes.data_as(dp),
                                            det.ctypes.data_as(dp) if detail else None), "tum_bo_evaluate")
        return (alpha, det) if detail else alpha

    def _prune(self, desc, n, S, want_draws, hold):
        desc.n, desc.S = n, S
        keep, ok = np.zeros(n, dtype=np.int32), ctypes.c_int()
        F = np.zeros((S, n, 2)) if want_draws else None
        self._check(self._L.tum_bom_prune(self._h, ctypes.addressof(desc), keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                          F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if want_draws else None, ctypes.byref(ok)),
                    "tum_bom_prune")
        if not ok.value:
            raise ModelFittingError("posterior covariance at the trials: not positive definite on the device")
        return keep.astype(bool), F

    def _prune_desc(self):
        desc = _PruneDesc()
        self._L.tum_bom_prune_desc_init(ctypes.addressof(desc))
        if desc.struct_size != ctypes.sizeof(_PruneDesc):
            raise Exception("tum_bom_prune_desc: the library's descriptor is not the one bo.py declares")
        return desc

    def prune(self, Xt, V, a, obj_hyp, Zs, jitter=1e-8, draws=False):
        """prune_draws and dominance_keep on the device: (keep mask (n), F (S x n x 2) or None). Zs: S x 2 x n base samples. V: the two
        L^-1 as gp_factor returns them, zero above the diagonal -- the device's products stop at the diagonal tile, so anything else is
        refused, not multiplied."""
        dp = ctypes.POINTER(ctypes.c_double)
        hold = []

        def ptr(x):
            x = np.ascontiguousarray(x, dtype=np.float64)
            hold.append(x)
            return x.ctypes.data_as(dp)
        Xt = np.ascontiguousarray(np.atleast_2d(np.asarray(Xt, dtype=np.float64)))
        n, d = Xt.shape
        Zs = np.asarray(Zs, dtype=np.float64)
        if Zs.ndim != 3 or Zs.shape[1:] != (2, n):
            raise Exception(f"tum_bom_prune: the base samples have the shape {Zs.shape}, not S x 2 x {n}")
        desc = self._prune_desc()
        desc.d, desc.jitter, desc.Xt = d, float(jitter), ptr(Xt)
        for o in range(2):
            if np.shape(V[o]) != (n, n) or np.shape(a[o]) != (n,) or len(obj_hyp[o].ls) != d:
                raise Exception(f"tum_bom_prune: V, a or the length scales of objective {o} do not have the sizes of Xt ({n} x {d})")
            desc.s[o], desc.c[o] = obj_hyp[o].s, obj_hyp[o].c
            desc.ils[o], desc.V[o], desc.a[o], desc.Z[o] = ptr(obj_hyp[o].ils), ptr(V[o]), ptr(a[o]), ptr(Zs[:, o])
        return self._prune(desc, n, len(Zs), draws, hold)

    def prune_given(self, F):
        """dominance_keep of given draws F (S x n x 2) on the device: the keep mask (n)."""
        F = np.ascontiguousarray(np.asarray(F, dtype=np.float64))
        if F.ndim != 3 or F.shape[2] != 2:
            raise Exception(f"tum_bom_prune: the draws have the shape {F.shape}, not S x n x 2")
        desc = self._prune_desc()
        desc.F = F.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return self._prune(desc, F.shape[1], F.shape[0], False, [F])[0]

    def fronts(self, F_b, ref):
        """build_fronts (P_max = n_b) of the baseline draws F_b (S x n_b x 2) on the device: fronts (S x n_b x 2) and counts (S)."""
        dp = ctypes.POINTER(ctypes.c_double)
        F_b = np.ascontiguousarray(np.asarray(F_b, dtype=np.float64))
        if F_b.ndim != 3 or F_b.shape[2] != 2:
            raise Exception(f"tum_bom_fronts: the draws have the shape {F_b.shape}, not S x n_b x 2")
        ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(2))
        S, nb = F_b.shape[:2]
        fronts, count = np.zeros((S, nb, 2)), np.zeros(S, dtype=np.int32)
        self._check(self._L.tum_bom_fronts(self._h, F_b.ctypes.data_as(dp), S, nb, ref.ctypes.data_as(dp), fronts.ctypes.data_as(dp),
                                           count.ctypes.data_as(ctypes.POINTER(ctypes.c_int))), "tum_bom_fronts")
        return fronts, count

    def prune_profile(self, on=True):
        """Time the kernels of the following prune calls; returns the seven times (ms) of the last one, both objectives together:
        kernel matrix, H, covariance, Cholesky, mean, draws, dominance."""
        ms = np.zeros(7)
        self._check(self._L.tum_bom_prune_profile(self._h, int(on), ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tum_bom_prune_profile")
        return ms

    def build_profile(self, on=True):
        """Time the kernels of the following device builds (set_model of a baseline="device" model); returns the nine times (ms) of the
        last one, both objectives together: kernel matrices, H, covariance, Cholesky, R = L_b^-1, mean, draws, packing, fronts."""
        ms = np.zeros(9)
        self._check(self._L.tum_bom_build_profile(self._h, int(on), ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tum_bom_build_profile")
        return ms

    def profile(self, on=True):
        """Time the launches of the following evaluations; returns the seven times (ms) of the last one."""
        ms = np.zeros(7)
        self._check(self._L.tum_bo_profile(self._h, int(on), ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tum_bo_profile")
        return ms

    def close(self):
        if self._h:
            self._L.tum_bo_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ candidate selection
def compass_search(evaluate, X0, h0=0.1, h_min=1e-3, max_iter=400):
    """Batched compass search from the rows of X0 inside [0,1]^d, maximising. Per launch every restart still searching offers its 2 d
    axis points at its step (clipped); it moves to its best point if that is strictly better, otherwise halves the step. Ties go to
    the lowest index. Returns the points, their values and the launches used."""
    X = np.array(X0, dtype=np.float64)
    R, d = X.shape
    val = np.asarray(evaluate(X), dtype=np.float64).copy()
    h = np.full(R, float(h0))
    launches = 1
    steps = np.concatenate([np.eye(d), -np.eye(d)])
    while launches < max_iter and (h >= h_min).any():
        act = np.flatnonzero(h >= h_min)
        P = np.clip(X[act, None, :] + h[act, None, None] * steps[None, :, :], 0.0, 1.0)
        v = np.asarray(evaluate(P.reshape(-1, d)), dtype=np.float64).reshape(len(act), 2 * d)
        launches += 1
        best = np.argmax(v, axis=1)
        bv = v[np.arange(len(act)), best]
        move = bv > val[act]
        X[act[move]] = P[move, best[move]]
        val[act[move]] = bv[move]
        h[act[~move]] *= 0.5
    return X, val, launches


def select(model, q=1, n_raw=512, n_restarts=20, max_iter=400, seed=0, acq=None, h0=0.1, h_min=1e-3, stats=None, device_append=True):
    """q sequential greedy picks (optimize_acqf(..., sequential=True)). Per pick: n_raw scrambled Sobol points in one launch, the best
    n_restarts refined by compass_search, the best restart is the pick and is appended to the baseline. acq: DeviceAcquisition (the
    default, created and closed here) or any object with set_model / evaluate. Returns picks (q x d), their values, the final model.
    A model packed with baseline="device" is built by the evaluator's set_model; where the evaluator has append_pick (and device_append
    is left on) the picks are appended there too and the final model is completed from model_arrays(); otherwise the built model is
    read back once and the picks are appended on the host."""
    own = acq is None
    if own:
        acq = DeviceAcquisition()
    try:
        picks, values = [], []
        on_device = False          # the model was built on the device and the evaluator appends there: nothing is uploaded after the build
        for i in range(int(q)):
            if not on_device:
                acq.set_model(model, keep_gp=i > 0)
            if model.device_baseline:          # (built on the device just now)
                if not hasattr(acq, "model_arrays"):
                    raise ValueError("select: a model packed with baseline='device' needs an evaluator with model_arrays (DeviceAcquisition)")
                on_device = hasattr(acq, "append_pick") and device_append
                if not on_device:          # (the picks are appended on the host to what the device built)
                    model = complete_model(model, acq.model_arrays())
            raw = sobol_points(n_raw, model.d, list(np.atleast_1d(seed)) + [i])
            t0 = time.perf_counter()
            v = np.asarray(acq.evaluate(raw))
            order = np.argsort(-v, kind="stable")[:int(n_restarts)]
            X, val, launches = compass_search(acq.evaluate, raw[order], h0=h0, h_min=h_min, max_iter=max_iter)
            if stats is not None:
                stats.append({"launches": launches + 1, "seconds": time.perf_counter() - t0})
            b = int(np.argmax(val))
            picks.append(X[b].copy()); values.append(float(val[b]))
            if on_device:
                acq.append_pick(X[b])
                model = replace(model, Xb=np.vstack([model.Xb, X[b][None, :]]))
            else:
                model = append_pick(model, X[b])
        if on_device:
            model = complete_model(model, acq.model_arrays())
        return np.array(picks), np.array(values), model
    finally:
        if own:
            acq.close()


# ------------------------------------------------------------------------------------------------ fitting
def _mll_torch(theta, X, y, fixed_noise, learn_noise, noise_floor):
    """Exact marginal log-likelihood of (X, y) at theta = [log ls (d), log s, c, log noise]; returns (mll, info of the Cholesky)."""
    import torch
    d = X.shape[1]
    ils = torch.exp(-theta[:d])
    D = (X[:, None, :] - X[None, :, :]) * ils
    K = torch.exp(theta[d]) * torch.exp(-0.5 * (D * D).sum(-1))
    noise = fixed_noise + noise_floor + (torch.exp(theta[d + 2]) if learn_noise else 0.0)
    A = K + torch.diag(noise * torch.ones(len(X), dtype=X.dtype, device=X.device))
    L, info = torch.linalg.cholesky_ex(A)
    r = (y - theta[d + 1])[:, None]
    w = torch.linalg.solve_triangular(L, r, upper=False)
    mll = -0.5 * (w * w).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * len(X) * np.log(2.0 * np.pi)
    ok = (info == 0) & torch.isfinite(mll) & (torch.diagonal(L).min() > 1e-7 * torch.exp(0.5 * theta[d]))
    return mll, bool(ok)


def gp_mll(X, y, hyp, fixed_noise=None, noise_floor=0.0):
    """The marginal log-likelihood of a GPHyper whose noise is the learned scalar noise (fixed_noise is added per point)."""
    import torch
    X, y = torch.as_tensor(np.asarray(X), dtype=torch.float64), torch.as_tensor(np.asarray(y), dtype=torch.float64)
    fn = torch.zeros(len(X), dtype=torch.float64) if fixed_noise is None else torch.as_tensor(np.asarray(fixed_noise), dtype=torch.float64)
    theta = torch.tensor(np.concatenate([np.log(hyp.ls), [np.log(hyp.s), hyp.c, np.log(hyp.noise)]]), dtype=torch.float64)
    return float(_mll_torch(theta, X, y, fn, True, noise_floor)[0])


def gp_mll_grad_host(X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """The numpy statement of the device chain (csrc/gp_kernels.hpp; include/tum_nmpc.h states the mathematics): the marginal
    log-likelihood at theta = [log ls (d), log s, c, log noise], its analytic gradient from W = alpha alpha^T - A^-1, and ok.
    Returns (mll, grad (d + 3), ok); a matrix numpy's Cholesky refuses gives (nan, nans, False)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    y, theta = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(theta, dtype=np.float64)
    n, d = X.shape
    ils, s, c = np.exp(-theta[:d]), float(np.exp(theta[d])), float(theta[d + 1])
    learned = float(np.exp(theta[d + 2])) if learn_noise else 0.0
    fixed = np.zeros(n) if fixed_noise is None else np.asarray(fixed_noise, dtype=np.float64)
    T2 = [((X[:, j, None] - X[None, :, j]) * ils[j]) ** 2 for j in range(d)]
    R = np.zeros((n, n))
    for t2 in T2:
        R += t2
    K = s * np.exp(-0.5 * R)
    A = K.copy()
    A[np.diag_indices_from(A)] += (fixed + noise_floor) + learned
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return float("nan"), np.full(d + 3, np.nan), False
    V = _tri_inv(L)
    w = V @ (y - c)
    alpha = V.T @ w
    mll = (-0.5 * (w @ w) - np.log(np.diag(L)).sum()) - 0.5 * n * np.log(2.0 * np.pi)
    WK = (np.outer(alpha, alpha) - V.T @ V) * K
    grad = np.array([0.5 * (WK * t2).sum() for t2 in T2] +
                    [0.5 * WK.sum(), alpha.sum(), 0.5 * learned * ((alpha @ alpha) - (V * V).sum()) if learn_noise else 0.0])
    ok = bool(np.isfinite(L).all() and np.isfinite(mll) and np.diag(L).min() > 1e-7 * np.exp(0.5 * theta[d]))
    return float(mll), grad, ok


class DeviceGP:
    """The marginal log-likelihood of one GP, its gradient and its factor on the device: tum_gp_create / tum_gp_data / tum_gp_mll /
    tum_gp_factor (csrc/gp_kernels.hpp). One handle serves any number of GPs one after the other; its three n x n matrices grow on
    demand. There is no CPU fallback behind it."""

    def __init__(self, device=0):
        from . import solver
        self._L = solver.load_library()
        self._h = self._L.tum_gp_create(int(device))
        if not self._h:
            raise Exception("tum_gp_create: " + self._L.tum_ocp_last_error().decode())
        self.n = self.d = None

    def _check(self, rc, what):
        if rc != 0:
            raise Exception(f"{what}: " + self._L.tum_ocp_last_error().decode())

    def set_data(self, X, y, fixed_noise=None):
        dp = ctypes.POINTER(ctypes.c_double)
        X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if len(y) != len(X):
            raise Exception(f"tum_gp_data: y has {len(y)} entries, X has {len(X)} rows")
        fn = None if fixed_noise is None else np.ascontiguousarray(np.broadcast_to(np.asarray(fixed_noise, dtype=np.float64), (len(X),)))
        self.n = self.d = None
        self._check(self._L.tum_gp_data(self._h, X.ctypes.data_as(dp), y.ctypes.data_as(dp), None if fn is None else fn.ctypes.data_as(dp),
                                        X.shape[0], X.shape[1]), "tum_gp_data")
        self.n, self.d = X.shape

    def _theta(self, theta, what):
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1))
        if self.d is not None and len(theta) != self.d + 3:
            raise Exception(f"{what}: theta has {len(theta)} entries, the data have d + 3 = {self.d + 3}")
        return theta

    def mll_grad(self, theta, learn_noise=True, noise_floor=0.0, grad=True):
        """(mll, grad (d + 3), ok) at theta = [log ls (d), log s, c, log noise]; grad=False: (mll, None, ok), A^-1 is not formed."""
        dp = ctypes.POINTER(ctypes.c_double)
        theta = self._theta(theta, "tum_gp_mll")
        mll, ok = ctypes.c_double(), ctypes.c_int()
        g = np.zeros(len(theta)) if grad else None
        self._check(self._L.tum_gp_mll(self._h, theta.ctypes.data_as(dp), int(bool(learn_noise)), float(noise_floor), ctypes.byref(mll),
                                       g.ctypes.data_as(dp) if grad else None, ctypes.byref(ok)), "tum_gp_mll")
        return mll.value, g, bool(ok.value)

    def factor(self, hyp):
        """V = L^-1 and a = A^-1 (y - c) at a GPHyper on the data of set_data; hyp.noise (a scalar) is added to their fixed noise."""
        dp = ctypes.POINTER(ctypes.c_double)
        theta = self._theta(np.concatenate([np.log(hyp.ls), [np.log(hyp.s), hyp.c, 0.0]]), "tum_gp_factor")
        if self.n is None:
            raise Exception("tum_gp_factor: no data (tum_gp_data first)")
        V, a, ok = np.zeros((self.n, self.n)), np.zeros(self.n), ctypes.c_int()
        self._check(self._L.tum_gp_factor(self._h, theta.ctypes.data_as(dp), 0, float(hyp.noise), V.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                          ctypes.byref(ok)), "tum_gp_factor")
        if not ok.value:
            raise ModelFittingError("GP kernel matrix: not positive definite on the device")
        return V, a

    def gp_factor(self, X, y, hyp):
        """gp_factor's signature (pack_model's factor=): hyp.noise is the whole noise, a scalar or one value per point."""
        self.set_data(X, y, fixed_noise=hyp.noise)
        return self.factor(replace(hyp, noise=0.0))

    def profile(self, on=True):
        """Time the kernels of the following calls; returns the seven times (ms) of the last one: kernel matrix, Cholesky, V = L^-1,
        A^-1 = V^T V, w and alpha, gradient tiles, reduction."""
        ms = np.zeros(7)
        self._check(self._L.tum_gp_profile(self._h, int(on), ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tum_gp_profile")
        return ms

    def close(self):
        if self._h:
            self._L.tum_gp_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fit_gp_device(Xn, y, fixed_noise, learn_noise, noise_floor, init, max_iter, return_trace, gp):
    """fit_gp's optimiser around DeviceGP.mll_grad: the same L-BFGS, options, box, start and refusals; theta lives on the host."""
    import torch
    yn = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = Xn.shape
    own = gp is None
    if own:
        gp = DeviceGP()
    try:
        gp.set_data(Xn, yn, fixed_noise)
        if init is None:
            yt = torch.as_tensor(yn, dtype=torch.float64)
            init = GPHyper(c=float(yt.mean()), s=max(float(yt.var()) if len(yt) > 1 else 1.0, 1e-3), ls=np.full(d, 0.5), noise=1e-2)
        theta0 = torch.tensor(np.concatenate([np.log(init.ls), [np.log(init.s), init.c, np.log(init.noise)]]), dtype=torch.float64)
        theta = theta0.clone().requires_grad_(True)
        start, _, ok = gp.mll_grad(theta0.numpy(), learn_noise, noise_floor, grad=False)
        if not ok:
            raise ModelFittingError("fit_gp: the kernel matrix at the initial hyperparameters is not positive definite")
        opt = torch.optim.LBFGS([theta], lr=1.0, max_iter=int(max_iter), tolerance_grad=1e-8, tolerance_change=1e-12, history_size=10,
                                line_search_fn="strong_wolfe")
        lo = torch.tensor([np.log(1e-2)] * d + [np.log(1e-3), -20.0, np.log(1e-8)], dtype=torch.float64)
        hi = torch.tensor([np.log(1e1)] * d + [np.log(1e3), 20.0, np.log(1e2)], dtype=torch.float64)

        def closure():
            opt.zero_grad()
            t = theta.detach()
            th = torch.maximum(torch.minimum(t, hi), lo)
            if not torch.isfinite(th).all():
                return torch.tensor(float("inf"), dtype=torch.float64)
            mll, g, ok = gp.mll_grad(th.numpy(), learn_noise, noise_floor)
            if not ok:
                return torch.tensor(float("inf"), dtype=torch.float64)
            inside = ((t >= lo) & (t <= hi)).to(torch.float64)          # (the clamp passes no gradient to a component outside the box)
            theta.grad = torch.as_tensor(-g / n, dtype=torch.float64) * inside
            return torch.tensor(-mll / n, dtype=torch.float64)
        opt.step(closure)
        th = torch.maximum(torch.minimum(theta.detach(), hi), lo)
        if not torch.isfinite(th).all():
            raise ModelFittingError("fit_gp: the kernel matrix at the fitted hyperparameters is not positive definite")
        end, _, ok = gp.mll_grad(th.numpy(), learn_noise, noise_floor, grad=False)
        if not ok:
            raise ModelFittingError("fit_gp: the kernel matrix at the fitted hyperparameters is not positive definite")
        if float(end) < float(start):          # (a line search that ended on a failed evaluation: keep the start)
            th, end = theta0, start
        t = th.numpy()
        hyp = GPHyper(c=float(t[d + 1]), s=float(np.exp(t[d])), ls=np.exp(t[:d]), noise=float(noise_floor + (np.exp(t[d + 2]) if learn_noise else 0.0)))
        return (hyp, float(start), float(end)) if return_trace else hyp
    finally:
        if own:
            gp.close()


def fit_gp(X, y, fixed_noise=None, learn_noise=True, noise_floor=1e-6, init=None, max_iter=100, device="cpu", return_trace=False,
           backend="torch", gp=None):
    """Maximise the exact marginal log-likelihood over log length scales, log output scale, the constant mean and (learn_noise) the log
    of a scalar noise, by L-BFGS (strong Wolfe) in torch.float64 on `device`. noise = fixed_noise + noise_floor + learned. A kernel
    matrix that is not numerically positive definite raises ModelFittingError. Returns a GPHyper (noise: the learned scalar plus the
    floor; the caller adds its fixed noise). backend "device": likelihood and gradient come from DeviceGP.mll_grad (gp: the handle
    to use; created and closed here otherwise), the optimiser is the same and runs on the host; `device` is not used."""
    import torch
    Xn = np.atleast_2d(np.asarray(X, dtype=np.float64))
    if backend == "device":
        return _fit_gp_device(Xn, y, fixed_noise, learn_noise, noise_floor, init, max_iter, return_trace, gp)
    if backend != "torch":
        raise ValueError(f"fit_gp: backend {backend!r} is neither 'torch' nor 'device'")
    X = torch.as_tensor(Xn, dtype=torch.float64, device=device)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1), dtype=torch.float64, device=device)
    d = X.shape[1]
    fn = torch.zeros(len(X), dtype=torch.float64, device=device) if fixed_noise is None else \
        torch.as_tensor(np.asarray(fixed_noise, dtype=np.float64), dtype=torch.float64, device=device)
    if init is None:
        init = GPHyper(c=float(yt.mean()), s=max(float(yt.var()) if len(yt) > 1 else 1.0, 1e-3), ls=np.full(d, 0.5), noise=1e-2)
    theta0 = torch.tensor(np.concatenate([np.log(init.ls), [np.log(init.s), init.c, np.log(init.noise)]]), dtype=torch.float64, device=device)
    theta = theta0.clone().requires_grad_(True)
    start, ok = _mll_torch(theta.detach(), X, yt, fn, learn_noise, noise_floor)
    if not ok:
        raise ModelFittingError("fit_gp: the kernel matrix at the initial hyperparameters is not positive definite")
    opt = torch.optim.LBFGS([theta], lr=1.0, max_iter=int(max_iter), tolerance_grad=1e-8, tolerance_change=1e-12, history_size=10,
                            line_search_fn="strong_wolfe")
    # the box the parameters are held in (no priors: small data sets would otherwise run off to a flat, huge-scale fit)
    lo = torch.tensor([np.log(1e-2)] * d + [np.log(1e-3), -20.0, np.log(1e-8)], dtype=torch.float64, device=device)
    hi = torch.tensor([np.log(1e1)] * d + [np.log(1e3), 20.0, np.log(1e2)], dtype=torch.float64, device=device)
    failed = []

    def closure():
        opt.zero_grad()
        th = torch.maximum(torch.minimum(theta, hi), lo)
        mll, ok = _mll_torch(th, X, yt, fn, learn_noise, noise_floor)
        if not ok:
            failed.append(True)
            return torch.tensor(float("inf"), dtype=torch.float64, device=device)
        loss = -mll / len(X)
        loss.backward()
        return loss
    opt.step(closure)
    th = torch.maximum(torch.minimum(theta.detach(), hi), lo)
    end, ok = _mll_torch(th, X, yt, fn, learn_noise, noise_floor)
    if not ok or not torch.isfinite(th).all():
        raise ModelFittingError("fit_gp: the kernel matrix at the fitted hyperparameters is not positive definite")
    if float(end) < float(start):          # (a line search that ended on a failed evaluation: keep the start)
        th, end = theta0, start
    t = th.cpu().numpy()
    hyp = GPHyper(c=float(t[d + 1]), s=float(np.exp(t[d])), ls=np.exp(t[:d]), noise=float(noise_floor + (np.exp(t[d + 2]) if learn_noise else 0.0)))
    return (hyp, float(start), float(end)) if return_trace else hyp


def standardize(Y):
    """botorch.utils.transforms.standardize: (Y - mean) / std per column, std with the n - 1 divisor (1 for a single row or zero spread)."""
    Y = np.asarray(Y, dtype=np.float64)
    mean = Y.mean(0)
    std = Y.std(0, ddof=1) if len(Y) > 1 else np.ones(Y.shape[1])
    std = np.where(std > 0, std, 1.0)
    return (Y - mean) / std, mean, std


class ObjectiveModel:
    """One exact GP per objective on the feasible trials, Y standardised."""

    def __init__(self, X, Y, device="cpu", max_iter=100, backend="torch", gp=None):
        self.X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        self.Ys, self.mean, self.std = standardize(Y)
        self.hyp = [fit_gp(self.X, self.Ys[:, o], device=device, max_iter=max_iter, backend=backend, gp=gp) for o in range(2)]


class ConstraintModel:
    """The two-class Dirichlet classification GP on all trials (surrogate_models.py:66-160): one GP per class on the transformed
    targets with their fixed noise and a learned extra noise; constant mean initialised at 1."""

    def __init__(self, X, feasible, device="cpu", max_iter=100, alpha_eps=0.001, backend="torch", gp=None):
        self.X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        self.feasible = np.asarray(feasible).astype(bool)
        targets, fixed = dirichlet_targets(self.feasible, alpha_eps)
        d = self.X.shape[1]
        self.hyp = []
        for k in range(2):
            init = GPHyper(c=1.0, s=max(float(np.var(targets[:, k])), 1.0), ls=np.full(d, 0.5), noise=1e-2)
            self.hyp.append(fit_gp(self.X, targets[:, k], fixed_noise=fixed[:, k], init=init, device=device, max_iter=max_iter,
                                   backend=backend, gp=gp))


# ------------------------------------------------------------------------------------------------ trials
@dataclass
class Trial:
    params_nat: np.ndarray
    params_nor: np.ndarray
    objectives: np.ndarray          # 2 x 2: [group][objective], NaN where infeasible
    feasible: bool


def store_trials(trials):
    """The reference's CSV lines (BO_WMPC/dataclasses.py Trial.to_csv)."""
    return "".join("{};{};{};{};{}\n".format(",".join(f"{e:1.1f}" for e in t.params_nat), ",".join(f"{e:1.3f}" for e in t.params_nor),
                                             ",".join(f"{e:1.3f}" for e in t.objectives[0]), ",".join(f"{e:1.3f}" for e in t.objectives[1]),
                                             1 if t.feasible else 0) for t in trials)


def load_trials(text):
    """Trials from CSV lines (helpers.py load_trials_from_csv)."""
    out = []
    for line in text.splitlines():
        if not line.strip():
            continue
        p = line.strip().split(";")
        out.append(Trial(np.array([float(e) for e in p[0].split(",")]), np.array([float(e) for e in p[1].split(",")]),
                         np.array([[float(e) for e in p[2].split(",")], [float(e) for e in p[3].split(",")]]), bool(int(p[4]))))
    return out


# ------------------------------------------------------------------------------------------------ the driver
DEFAULT_CONFIG = dict(n_initial=50, batch_size=5, reference_point_0=[-0.5, -0.75], reference_point_1=[-0.4, -0.90], n_sobol_samples=1024,
                      n_restarts=20, n_raw_samples=512, max_iter=400, epsilon=0.8, standardize_ref_point=False, fit_max_iter=100,
                      gh_nodes=64, jitter=1e-8, seed=0, prune_baseline=True)


class BayesianOptimization:
    """BO_WMPC/bayesian_optimization.py BayesianOptimization around a batched objective:
        objective(params_nat (P x d)) -> (objectives (P x 2 x 2), feasible (P,))      -- closed_loop.evaluate_segments
    bounds: 2 x d natural lower / upper bounds. acq: "device" (DeviceAcquisition), "host" (host_acquisition) or an evaluator.
    The reference standardises Y for the GP but hands the acquisition the reference point in raw units; that is kept as the default
    (config standardize_ref_point=False); True maps the reference point into the standardised units. model_backend "device": the
    baseline is pruned on the device (prune_baseline(backend="device")) and its posterior, draws and fronts are built there
    (pack_model(baseline="device")); it needs the device acquisition. "host", the default, is the numpy path."""

    def __init__(self, bounds, config, objective, acq="device", fit_device="cpu", fit_backend="torch", model_backend="host"):
        self.bounds = np.asarray(bounds, dtype=np.float64)
        self.d = self.bounds.shape[1]
        self.config = dict(DEFAULT_CONFIG); self.config.update(config or {})
        self.objective, self.acq, self.fit_device = objective, acq, fit_device
        if fit_backend not in ("torch", "device"):
            raise ValueError(f"BayesianOptimization: fit_backend {fit_backend!r} is neither 'torch' nor 'device'")
        self.fit_backend, self._gp = fit_backend, None          # (one DeviceGP for every fit and factor of the campaign)
        if model_backend not in ("host", "device"):
            raise ValueError(f"BayesianOptimization: model_backend {model_backend!r} is neither 'host' nor 'device'")
        if model_backend == "device" and not (acq == "device" or isinstance(acq, DeviceAcquisition)):
            raise ValueError("BayesianOptimization: model_backend 'device' needs acq 'device' or a DeviceAcquisition")
        self.model_backend, self._model_acq = model_backend, None          # (one handle for every pruning of the campaign)
        self.ref = np.array([self.config["reference_point_0"], self.config["reference_point_1"]], dtype=np.float64)
        self.trials, self.active_group = [], 0
        self.hypervolumes, self.hv_traces, self.pareto_trials = [0.0, 0.0], [], [[], []]
        self.times, self.fallbacks, self.groups_used = [], 0, []
        self._draws = 0

    def close(self):
        """Free the device handles the driver created (the surrogate fit's and the model's); one that was handed in stays open."""
        if self._gp is not None:
            self._gp.close()
            self._gp = None
        if self._model_acq is not None and self._model_acq is not self.acq:
            self._model_acq.close()
        self._model_acq = None

    # -- data
    def unnormalize(self, X):
        return self.bounds[0] + np.asarray(X) * (self.bounds[1] - self.bounds[0])

    def _arrays(self):
        Xn = np.array([t.params_nor for t in self.trials]).reshape(-1, self.d)
        feas = np.array([t.feasible for t in self.trials], dtype=bool)
        obj = np.array([t.objectives for t in self.trials]).reshape(-1, 2, 2)
        return Xn, feas, obj

    def _add_trial(self, t):
        self.trials.append(t)
        Xn, feas, obj = self._arrays()
        for g in range(2):
            Y = obj[feas][:, g, :]
            self.hypervolumes[g] = hypervolume_2d(Y, self.ref[g]) if len(Y) else 0.0
            idx = np.flatnonzero(feas)
            self.pareto_trials[g] = [self.trials[i] for i in idx[pareto_mask(Y)]] if len(Y) else []
        self.hv_traces.append(list(self.hypervolumes))

    def _evaluate(self, X_nor):
        X_nor = np.atleast_2d(X_nor)
        nat = self.unnormalize(X_nor)
        obj, feas = self.objective(nat)
        obj, feas = np.array(obj, dtype=np.float64).reshape(-1, 2, 2), np.asarray(feas).astype(bool)
        for i in range(len(nat)):
            o = obj[i] if feas[i] else np.full((2, 2), np.nan)
            self._add_trial(Trial(nat[i], X_nor[i].copy(), o, bool(feas[i])))

    def _sobol(self, n):
        self._draws += 1
        return sobol_points(n, self.d, [int(self.config["seed"]), 7, self._draws])

    def generate_initial_data(self, n=None):
        self._evaluate(self._sobol(self.config["n_initial"] if n is None else n))

    def evaluate_at_boundaries(self):
        """All 2^d corners of the parameter box, as the reference's method of the same name (many of them fail)."""
        import itertools
        self._evaluate(np.array(list(itertools.product((0.0, 1.0), repeat=self.d))))

    # -- one step
    def _fallback(self):
        self.fallbacks += 1
        self._evaluate(self._sobol(self.config["batch_size"]))
        return None

    def build_model(self, group):
        """Fit both surrogates on the current trials and pack the acquisition model of a segment group."""
        cfg = self.config
        Xn, feas, obj = self._arrays()
        Xt, Y = Xn[feas], obj[feas][:, group, :]
        if self.fit_backend == "device" and self._gp is None:
            self._gp = DeviceGP()
        om = ObjectiveModel(Xt, Y, device=self.fit_device, max_iter=cfg["fit_max_iter"], backend=self.fit_backend, gp=self._gp)
        cm = ConstraintModel(Xn, feas, device=self.fit_device, max_iter=cfg["fit_max_iter"], backend=self.fit_backend, gp=self._gp)
        ref = (self.ref[group] - om.mean) / om.std if cfg["standardize_ref_point"] else self.ref[group]
        S, q = int(cfg["n_sobol_samples"]), int(cfg["batch_size"])
        dev = {}
        if self.model_backend == "device" and cfg["prune_baseline"]:
            if self._model_acq is None:
                self._model_acq = self.acq if isinstance(self.acq, DeviceAcquisition) else DeviceAcquisition()
            dev = dict(backend="device", acq=self._model_acq, factor=self._gp.gp_factor if self._gp is not None else None)
        keep = prune_baseline(Xt, om.Ys, om.hyp, S=S, seed=[int(cfg["seed"]), 11, len(self.trials)], jitter=cfg["jitter"], **dev) \
            if cfg["prune_baseline"] else np.arange(len(Xt))
        keep = keep[:NB_MAX - q - 1]
        Z = sobol_normal(S, 2 * (len(keep) + q + 1), [int(cfg["seed"]), 13, len(self.trials)]).reshape(S, 2, -1).transpose(0, 2, 1)
        return pack_model(Xt, om.Ys, om.hyp, Xn, feas, cm.hyp, Xt[keep], Z, ref, eps=cfg["epsilon"], jitter=cfg["jitter"], K=cfg["gh_nodes"],
                          factor=self._gp.gp_factor if self._gp is not None else None, baseline=self.model_backend)

    def perform_bayesian_optimization_step(self):
        """One iteration: fit, select batch_size candidates, evaluate them. Returns (t_fit, t_select, t_evaluate), or None where the
        step fell back to Sobol trials (no feasible data, or the fit failed)."""
        cfg = self.config
        t0 = time.perf_counter()
        if not any(t.feasible for t in self.trials):
            return self._fallback()
        group = self.active_group
        try:
            model = self.build_model(group)
        except ModelFittingError:
            return self._fallback()
        t1 = time.perf_counter()
        acq = {"device": None, "host": HostAcquisition()}.get(self.acq, self.acq) if isinstance(self.acq, str) else self.acq
        try:
            picks, _, _ = select(model, q=cfg["batch_size"], n_raw=cfg["n_raw_samples"], n_restarts=cfg["n_restarts"], max_iter=cfg["max_iter"],
                                 seed=[int(cfg["seed"]), 17, len(self.trials)], acq=acq)
        except ModelFittingError:          # (a baseline the device builds is factored inside select's first set_model)
            if not model.device_baseline:
                raise
            return self._fallback()
        t2 = time.perf_counter()
        self._evaluate(np.clip(picks, 0.0, 1.0))
        t3 = time.perf_counter()
        self.groups_used.append(group)
        self.active_group = (self.active_group + 1) % 2
        self.times.append((t1 - t0, t2 - t1, t3 - t2))
        return self.times[-1]
