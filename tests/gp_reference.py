"""
gp_reference.py -- the independent yardstick of the surrogate fit's objective (tum_control_amd/bo.py gp_mll_grad_host, DeviceGP;
csrc/gp_kernels.hpp): the marginal log-likelihood of include/tum_nmpc.h (K16) and its gradient in np.longdouble (x87 extended).

  mll_grad(X, y, theta, fixed_noise, learn_noise, noise_floor)   MLL, gradient, scale_mll, scale_grad as long doubles / floats
  factor(X, y, hyp)                                               L^-1 and A^-1 (y - c) in long double, hyp a bo.GPHyper
  torch_mll_grad(...)                                             bo._mll_torch and autograd on the CPU: the second FP64 statement
  torch_factor(X, y, hyp)                                         torch's cholesky and solve_triangular: the second FP64 factor

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


def mll_grad(X, y, theta, fixed_noise=None, learn_noise=True, noise_floor=0.0):
    """(mll, grad (d + 3), scale_mll, scale_grad): scale_mll = 1/2 r^T A^-1 r + |sum log L_ii| + 1/2 n log 2 pi, scale_grad the
    largest |component| of the gradient."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, d = X.shape
    K, A, ils, learned = _matrix(X, theta, fixed_noise, learn_noise, noise_floor)
    L = cholesky(A)
    r = np.asarray(y, dtype=LD).reshape(-1) - LD(theta[d + 1])
    w = forward_substitution(L, r[:, None])[:, 0]
    quad, logdet, const = LD(0.5) * (w * w).sum(), np.log(np.diag(L)).sum(), LD(0.5) * n * np.log(LD(2) * np.pi)
    mll = -quad - logdet - const
    V = forward_substitution(L, np.eye(n, dtype=LD))
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
    return mll, grad, float(quad + abs(logdet) + const), float(np.abs(grad).max())


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


def fit_data(n=24, d=3, seed=0):
    """tests/test_bo_host.py _fit_data for any d: a smooth target of the first two coordinates plus noise, standardised."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3 * X[:, 0]) + 0.5 * X[:, min(1, d - 1)] ** 2 + 0.05 * rng.standard_normal(n)
    return X, ((y - y.mean()) / y.std(ddof=1) if n > 1 else y - y.mean())
