"""
gp_reference.py -- the independent yardstick of the surrogate fit's objective (tum_control_amd/bo.py gp_mll_grad_host, DeviceGP;
csrc/gp_kernels.hpp): the marginal log-likelihood of include/tum_nmpc.h (K16) and its gradient in np.longdouble (x87 extended).

  mll_grad(X, y, theta, fixed_noise, learn_noise, noise_floor)   MLL, gradient, scale_mll, scale_grad as long doubles / floats
  factor(X, y, hyp)                                               L^-1 and A^-1 (y - c) in long double, hyp a bo.GPHyper
  torch_mll_grad(...)                                             bo._mll_torch and autograd on the CPU: the second FP64 statement
  torch_factor(X, y, hyp)                                         torch's cholesky and solve_triangular: the second FP64 factor
  solve(...)                                                      mll_grad and V = L^-1, A^-1 (y - c) from one Cholesky, one substitution
  clustered_data(sizes, d, seed), cluster_sizes(n)                clusters 100 apart: A is block diagonal to the bit
  block_mll_grad(sizes, ...), block_factor(sizes, X, y, hyp)      their truth cluster by cluster, in the formats of mll_grad and factor:
                                                                  the whole-matrix reference is cubic, 150 s at n = 2050
  split(x), join(hi, lo)                                          a long double as two float64 (tests/golden/gp_campaign.npz)

The Cholesky factor is the column algorithm written out and every solve is forward substitution row by row, as tests/bo_reference.py
does it. The gradient goes through the textbook identity dMLL / dtheta = 1/2 tr((alpha alpha^T - A^-1) dA / dtheta) with A^-1 from
L^-1, all in long double: 11 more bits than the code under test carries.
"""
import numpy as np

from bo_reference import LD, _mm, _rbf_ld, forward_substitution

U = 2.0 ** -53


def cholesky(A):
    """Lower Cholesky factor in long double, column by column."""
    A = np.asarray(A, dtype=LD)
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] * L[j, :j]).sum())
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, None, :j]).sum(1)) / L[j, j]
    return L


def _matrix(X, theta, fixed_noise, learn_noise, noise_floor):
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, d = X.shape
    th = np.asarray(theta, dtype=LD)
    ils, s = np.exp(-th[:d]), np.exp(th[d])
    K = _rbf_ld(X, X, ils, s)
    noise = (np.zeros(n, dtype=LD) if fixed_noise is None else np.asarray(fixed_noise, dtype=LD)) + LD(noise_floor)
    learned = np.exp(th[d + 2]) if learn_noise else LD(0)
    return K, K + np.diag(noise + learned), ils, learned


def solve(X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """Everything of one GP at theta from one Cholesky and one forward substitution (of [I | r]): (mll, grad (d + 3), scale_mll,
    scale_grad, V = L^-1, alpha = A^-1 (y - c)); scale_mll = 1/2 r^T A^-1 r + |sum log L_ii| + 1/2 n log 2 pi, scale_grad the
    largest |component| of the gradient."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, d = X.shape
    K, A, ils, learned = _matrix(X, theta, fixed_noise, learn_noise, noise_floor)
    L = cholesky(A)
    r = np.asarray(y, dtype=LD).reshape(-1) - LD(theta[d + 1])
    Vw = forward_substitution(L, np.concatenate([np.eye(n, dtype=LD), r[:, None]], axis=1))
    V, w = Vw[:, :n], Vw[:, n]
    quad, logdet, const = LD(0.5) * (w * w).sum(), np.log(np.diag(L)).sum(), LD(0.5) * n * np.log(LD(2) * np.pi)
    mll = -quad - logdet - const
    alpha = _mm(V.T, w[:, None])[:, 0]
    W = alpha[:, None] * alpha[None, :] - _mm(V.T, V)
    WK = W * K
    Xl = np.asarray(X, dtype=LD)
    grad = np.zeros(d + 3, dtype=LD)
    for j in range(d):
        t = (Xl[:, j, None] - Xl[None, :, j]) * ils[j]
        grad[j] = LD(0.5) * (WK * t * t).sum()
    grad[d] = LD(0.5) * WK.sum()
    grad[d + 1] = alpha.sum()
    grad[d + 2] = LD(0.5) * learned * np.trace(W) if learn_noise else LD(0)
    return mll, grad, float(quad + abs(logdet) + const), float(np.abs(grad).max()), V, alpha


def mll_grad(X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """(mll, grad (d + 3), scale_mll, scale_grad) of solve."""
    return solve(X, y, theta, fixed_noise, learn_noise, noise_floor)[:4]


def factor(X, y, hyp):
    """(V, a) = (L^-1, A^-1 (y - c)) of bo.gp_factor's matrix in long double; hyp.noise a scalar or one value per point."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n = len(X)
    A = _rbf_ld(X, X, LD(1) / np.asarray(hyp.ls, dtype=LD), hyp.s) + np.diag(np.broadcast_to(np.asarray(hyp.noise, dtype=LD), (n,)))
    L = cholesky(A)
    V = forward_substitution(L, np.eye(n, dtype=LD))
    r = np.asarray(y, dtype=LD).reshape(-1) - LD(hyp.c)
    return V, _mm(V.T, _mm(V, r[:, None]))[:, 0]


def torch_mll_grad(X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """bo._mll_torch with autograd on the CPU: (mll, grad, ok)."""
    import torch
    from tum_control_amd import bo
    Xt, yt = torch.as_tensor(np.atleast_2d(np.asarray(X, dtype=np.float64))), torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1))
    fn = torch.zeros(len(Xt), dtype=torch.float64) if fixed_noise is None else torch.as_tensor(np.asarray(fixed_noise, dtype=np.float64))
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    mll, ok = bo._mll_torch(th, Xt, yt, fn, learn_noise, noise_floor)
    mll.backward()
    return float(mll.detach()), th.grad.numpy().copy(), ok


def torch_factor(X, y, hyp):
    import torch
    from tum_control_amd import bo
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    A = bo.rbf(X, X, hyp.ils, hyp.s)
    A[np.diag_indices_from(A)] += np.broadcast_to(np.asarray(hyp.noise, dtype=np.float64), (len(X),))
    L = torch.linalg.cholesky(torch.as_tensor(A))
    V = torch.linalg.solve_triangular(L, torch.eye(len(X), dtype=torch.float64), upper=False)
    r = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1) - hyp.c)
    return V.numpy(), (V.T @ (V @ r)).numpy()


def errors(mll, grad, ref):
    """(error of the MLL, largest error of a gradient component) against ref = mll_grad(...), in units of u x scale."""
    mll_l, grad_l, s_mll, s_grad = ref
    return float(abs(LD(mll) - mll_l) / (U * s_mll)), float(np.abs(np.asarray(grad, dtype=LD) - grad_l).max() / (U * s_grad))


CLUSTER_PATTERN = (150, 97, 181, 113)


def cluster_sizes(n):
    """CLUSTER_PATTERN repeated up to n; a remainder of fewer than 65 points joins the cluster before it. Every size lies in 65 .. 200."""
    sizes, i = [], 0
    while sum(sizes) + CLUSTER_PATTERN[i % 4] <= n:
        sizes.append(CLUSTER_PATTERN[i % 4]); i += 1
    rest = n - sum(sizes)
    if rest >= 65 or not sizes:
        sizes.append(rest)
    else:
        sizes[-1] += rest
    assert sum(sizes) == n and all(65 <= s <= 200 for s in sizes), sizes
    return tuple(sizes)


def clustered_data(sizes, d, seed, noise=False):
    """(X, y, per-point noise or None): cluster i is drawn in the unit cube and shifted by 100 i in every coordinate, so with length
    scales up to about 1.2 every kernel value between two clusters is exp(-1/2 d (99 / 1.2)^2) or less: exactly 0 in FP64 and below
    1e-1400 in long double (u = 1e-16 of anything it is added to). A is block diagonal and block_mll_grad / block_factor are its
    truth. No cluster ends on a multiple of 64 before n: every 64-wide tile edge then cuts through a cluster, and the tiles the
    factorisation works on hold live and zero entries mixed."""
    ends = np.cumsum(sizes)
    assert all(e % 64 != 0 for e in ends[:-1]), ends
    n = int(ends[-1])
    rng = np.random.default_rng(seed)
    U01 = rng.random((n, d))
    y = np.sin(3 * U01[:, 0]) + 0.5 * U01[:, min(1, d - 1)] ** 2 + 0.05 * rng.standard_normal(n)
    X = U01 + 100.0 * np.repeat(np.arange(len(sizes)), sizes)[:, None]
    fixed = 0.05 + 0.45 * rng.random(n) if noise else None
    return X, (y - y.mean()) / y.std(ddof=1), fixed


def _blocks(sizes):
    ends = np.cumsum(sizes)
    return [slice(int(e - s), int(e)) for s, e in zip(sizes, ends)]


def block_mll_grad(sizes, X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """mll_grad of a block-diagonal A as the sum of the clusters' long-double results: (mll, grad, scale_mll, scale_grad), scale_mll
    the sum of the clusters' scales, scale_grad the largest |component| of the summed gradient."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mll, grad, s_mll = LD(0), np.zeros(X.shape[1] + 3, dtype=LD), 0.0
    for b in _blocks(sizes):
        m, g, sm, _ = mll_grad(X[b], y[b], theta, None if fixed_noise is None else np.asarray(fixed_noise)[b], learn_noise, noise_floor)
        mll, grad, s_mll = mll + m, grad + g, s_mll + sm
    return mll, grad, s_mll, float(np.abs(grad).max())


def block_factor(sizes, X, y, hyp):
    """factor of a block-diagonal A: V with the clusters' long-double L^-1 on its diagonal blocks and exact zeros elsewhere, a their
    concatenation."""
    from dataclasses import replace
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(X)
    noise = np.broadcast_to(np.asarray(hyp.noise, dtype=np.float64), (n,))
    V, a = np.zeros((n, n), dtype=LD), np.zeros(n, dtype=LD)
    for b in _blocks(sizes):
        V[b, b], a[b] = factor(X[b], y[b], replace(hyp, noise=noise[b]))
    return V, a


def split(x):
    """A long double (array) as two float64: hi = float64(x), lo = float64(x - hi); join(hi, lo) gives x back exactly (the 64-bit
    significand fits 53 + 53 bits)."""
    x = np.asarray(x, dtype=LD)
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(LD)).astype(np.float64)


def join(hi, lo):
    return np.asarray(hi, dtype=LD) + np.asarray(lo, dtype=LD)


def fit_data(n=24, d=3, seed=0):
    """tests/test_bo_host.py _fit_data for any d: a smooth target of the first two coordinates plus noise, standardised."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3 * X[:, 0]) + 0.5 * X[:, min(1, d - 1)] ** 2 + 0.05 * rng.standard_normal(n)
    return X, ((y - y.mean()) / y.std(ddof=1) if n > 1 else y - y.mean())
