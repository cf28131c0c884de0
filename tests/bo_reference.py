"""
bo_reference.py -- the independent yardsticks of the acquisition value (tum_control_amd/bo.py, csrc/bo_kernels.hpp).

  longdouble_acquisition(m, X)   the statement of include/tum_nmpc.h in np.longdouble (x87 extended: 64-bit significand), from the SAME
                                 arrays tum_bo_model takes -- the packed factors V, a, H, R are inputs, so their conditioning is not the
                                 error of the code under test. Returns alpha and the C x 8 detail rows as long doubles.
  torch_acquisition(m, X)        a second FP64 statement in torch, written differently from bo.host_acquisition (kernel through scaled
                                 coordinates and one broadcast sum, products through torch.matmul, the cells as one S x (P + 1) x C
                                 tensor): the gates of tests/test_gpu_bo.py are set from the errors of both FP64 statements.
  forward_substitution(L, B)     hand-written triangular solve in long double (the textbook posterior of tests/test_bo_host.py).
  union_area(F, ref, f)          hypervolume improvement as the area of a union of rectangles, without the cell formula.
  generate(...)                  a seeded synthetic model with literal-style hyperparameters.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def forward_substitution(L, B):
    """X with L X = B, L lower triangular, in long double, row by row."""
    L, B = np.asarray(L, dtype=LD), np.asarray(B, dtype=LD)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        acc = B[i].copy()
        for j in range(i):
            acc = acc - L[i, j] * X[j]
        X[i] = acc / L[i, i]
    return X


def _rbf_ld(X1, X2, ils, s):
    X1, X2, ils = np.asarray(X1, dtype=LD), np.asarray(X2, dtype=LD), np.asarray(ils, dtype=LD)
    r = np.zeros((X1.shape[0], X2.shape[0]), dtype=LD)
    for j in range(X1.shape[1]):
        t = (X1[:, j, None] - X2[None, :, j]) * ils[j]
        r = r + t * t
    return LD(s) * np.exp(LD(-0.5) * r)


def _mm(A, B):
    """Long-double product as a sum of outer products (numpy has no extended-precision BLAS; this keeps it vectorised)."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for k in range(A.shape[1]):
        out += A[:, k, None] * B[None, k, :]
    return out


def _sigmoid_ld(t):
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, LD(1) / (LD(1) + e), e / (LD(1) + e))


def longdouble_acquisition(m, X, return_samples=False):
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    C, S = len(X), m.S
    mu, d2, f = [], [], []
    for o in range(2):
        kt = _rbf_ld(m.Xt, X, m.ils[o], m.s[o])
        q = _mm(m.V[o], kt)
        mu.append(LD(m.c[o]) + _mm(np.asarray(m.a[o])[None, :], kt)[0])
        sig = _rbf_ld(m.Xb, X, m.ils[o], m.s[o]) - _mm(m.H[o], q)
        l = _mm(m.R[o], sig)
        v = LD(m.s[o]) - (q * q).sum(0) - (l * l).sum(0)
        d2.append(np.maximum(v, LD(m.jitter[o])))
        f.append(mu[o][None, :] + _mm(m.Z(o), l) + np.sqrt(d2[o])[None, :] * np.asarray(m.zeta(o), dtype=LD)[:, None])
    hv = np.zeros((S, C), dtype=LD)
    r0, r1 = LD(m.ref[0]), LD(m.ref[1])
    for s in range(S):
        xp = r0
        for i in range(int(m.front_count[s])):
            xn, h = LD(m.fronts[s, i, 0]), LD(m.fronts[s, i, 1])
            hv[s] += np.maximum(np.minimum(f[0][s], xn) - xp, 0) * np.maximum(f[1][s] - h, 0)
            xp = xn
        hv[s] += np.maximum(f[0][s] - xp, 0) * np.maximum(f[1][s] - r1, 0)
    mean_hv = hv.sum(0) / LD(S)
    mk, vk = [], []
    for g in (2, 3):
        kc = _rbf_ld(m.Xc, X, m.ils[g], m.s[g])
        q = _mm(m.V[g], kc)
        mk.append(LD(m.c[g]) + _mm(np.asarray(m.a[g])[None, :], kc)[0])
        vk.append(LD(m.s[g]) - (q * q).sum(0))
    mean, sd_t = mk[1] - mk[0], np.sqrt(np.maximum(vk[0] + vk[1], 0))
    gx, gw = np.asarray(m.gh_x, dtype=LD), np.asarray(m.gh_w, dtype=LD)
    sg = _sigmoid_ld(mean[:, None] + sd_t[:, None] * gx[None, :])
    p = (sg * gw[None, :]).sum(1)
    sd = np.sqrt((((sg - p[:, None]) ** 2) * gw[None, :]).sum(1))
    factor = LD(m.eps) * p + (LD(1) - LD(m.eps)) * sd
    det = np.stack([mu[0], mu[1], d2[0], d2[1], mean_hv, p, sd, factor], axis=1)
    return (factor * mean_hv, det, f) if return_samples else (factor * mean_hv, det)


def torch_acquisition(m, X):
    import torch
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)          # noqa: E731
    X = t(np.atleast_2d(X))
    S = m.S

    def kern(A, g):
        ils = t(m.ils[g])
        D = (t(A) * ils)[:, None, :] - (X * ils)[None, :, :]
        return m.s[g] * torch.exp(-0.5 * (D * D).sum(-1))
    mu, d2, f = [], [], []
    for o in range(2):
        kt = kern(m.Xt, o)
        q = torch.matmul(t(m.V[o]), kt)
        mu.append(m.c[o] + torch.matmul(t(m.a[o]), kt))
        l = torch.matmul(t(m.R[o]), kern(m.Xb, o) - torch.matmul(t(m.H[o]), q))
        d2.append(torch.clamp(m.s[o] - torch.linalg.vector_norm(q, dim=0) ** 2 - torch.linalg.vector_norm(l, dim=0) ** 2, min=float(m.jitter[o])))
        f.append(mu[o] + torch.matmul(t(m.Z(o)), l) + torch.sqrt(d2[o]) * t(m.zeta(o))[:, None])
    P = m.fronts.shape[1]
    cnt = torch.as_tensor(m.front_count.astype(np.int64))
    fr = t(m.fronts)
    valid = torch.arange(P)[None, :] < cnt[:, None]
    inf = torch.full((S, 1), float("inf"), dtype=torch.float64)
    right = torch.cat([torch.where(valid, fr[:, :, 0], inf), inf], dim=1)                              # S x (P + 1): x_{i+1}
    left = torch.cat([torch.full((S, 1), float(m.ref[0]), dtype=torch.float64), right[:, :-1]], dim=1)  # x_i
    # the height of cell i is the front point's objective 1; behind the last point (and in the open cell) the reference point's
    height = torch.cat([torch.where(valid, fr[:, :, 1], torch.full_like(fr[:, :, 1], float(m.ref[1]))),
                        torch.full((S, 1), float(m.ref[1]), dtype=torch.float64)], dim=1)
    # cells behind the open one have left = inf: no width
    w = torch.clamp(torch.minimum(f[0][:, None, :], right[:, :, None]) - left[:, :, None], min=0.0)
    w = torch.where(torch.isfinite(left)[:, :, None], w, torch.zeros_like(w))
    hv = (w * torch.clamp(f[1][:, None, :] - height[:, :, None], min=0.0)).sum(1)
    mean_hv = hv.mean(0)
    mk, vk = [], []
    for g in (2, 3):
        kc = kern(m.Xc, g)
        q = torch.matmul(t(m.V[g]), kc)
        mk.append(m.c[g] + torch.matmul(t(m.a[g]), kc))
        vk.append(m.s[g] - (q * q).sum(0))
    mean, sd_t = mk[1] - mk[0], torch.sqrt(torch.clamp(vk[0] + vk[1], min=0.0))
    sg = torch.sigmoid(mean[:, None] + sd_t[:, None] * t(m.gh_x)[None, :])
    p = torch.matmul(sg, t(m.gh_w))
    sd = torch.sqrt(torch.matmul((sg - p[:, None]) ** 2, t(m.gh_w)))
    factor = m.eps * p + (1.0 - m.eps) * sd
    det = torch.stack([mu[0], mu[1], d2[0], d2[1], mean_hv, p, sd, factor], dim=1)
    return (factor * mean_hv).numpy(), det.numpy()


def union_area(F, ref, f):
    """Area of (box [ref, f]) minus the union of the boxes [ref, p], p in F -- by inclusion of elementary rectangles of the
    coordinate grid all the points span, without sorting the front into cells."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 2)
    if f[0] <= ref[0] or f[1] <= ref[1]:
        return 0.0
    xs = np.unique(np.concatenate([[ref[0], f[0]], np.clip(F[:, 0], ref[0], f[0])]))
    ys = np.unique(np.concatenate([[ref[1], f[1]], np.clip(F[:, 1], ref[1], f[1])]))
    area = 0.0
    for i in range(len(xs) - 1):
        for j in range(len(ys) - 1):
            cx, cy = 0.5 * (xs[i] + xs[i + 1]), 0.5 * (ys[j] + ys[j + 1])
            if not ((F[:, 0] >= cx) & (F[:, 1] >= cy)).any():
                area += (xs[i + 1] - xs[i]) * (ys[j + 1] - ys[j])
    return area


# hyperparameters in the range fitted models of the fixture take (literal: the tests do not depend on fit_gp)
def hypers(d):
    from tum_control_amd.bo import GPHyper
    ls = np.array([0.45, 0.8, 0.6, 1.1, 0.5, 0.9, 0.7, 0.65, 0.75, 0.55, 0.85, 0.95, 0.5, 0.6, 0.7, 0.8])
    obj = [GPHyper(c=0.1, s=1.3, ls=ls[:d].copy(), noise=0.05), GPHyper(c=-0.2, s=0.9, ls=ls[::-1][:d].copy(), noise=0.08)]
    cls = [GPHyper(c=-3.0, s=12.0, ls=0.8 * ls[:d], noise=0.1), GPHyper(c=-4.0, s=15.0, ls=0.7 * ls[::-1][:d], noise=0.2)]
    return obj, cls


def generate(d, n_t, n_b, n_c, S, K, seed, q=1, jitter=1e-6, ref=(-1.5, -1.5), eps=0.8, single_class=None):
    """A seeded synthetic model: n_c trials, the first n_t of them feasible (all or none with single_class), two smooth objectives,
    the baseline the first n_b feasible trials (repeated draws where n_b > n_t)."""
    from tum_control_amd import bo
    rng = np.random.default_rng(seed)
    Xc = rng.random((n_c, d))
    feas = np.zeros(n_c, dtype=bool)
    feas[:min(n_t, n_c)] = True
    if single_class is not None:
        feas[:] = bool(single_class)
    Xt = Xc[:n_t] if n_t <= n_c else rng.random((n_t, d))
    Y = np.stack([-((Xt - 0.3) ** 2).sum(1), -((Xt - 0.7) ** 2).sum(1)], axis=1) * (4.0 / d) + 0.05 * rng.standard_normal((n_t, 2))
    Ys = bo.standardize(Y)[0] if n_t > 1 else Y
    Xb = Xt[:n_b] if n_b <= n_t else np.vstack([Xt, rng.random((n_b - n_t, d))])
    Z = bo.sobol_normal(S, 2 * (n_b + q + 1), seed).reshape(S, 2, -1).transpose(0, 2, 1)
    obj, cls = hypers(d)
    return bo.pack_model(Xt, Ys, obj, Xc, feas, cls, Xb, Z, np.array(ref), eps=eps, jitter=jitter, K=K)
