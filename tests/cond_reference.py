"""
The condensed QP of one SQP real-time iteration of the nominal OCP, and the expansion of its step, once more: written from the
comments of oracle_solve (oracle/nmpc_oracle.c, steps 2-5 and 7) and SURVEY.md section 5, with numpy alone and no code shared
with the kernels or the oracle. Not a test module: tests/test_cond_reference.py holds it against the oracle (CPU),
tests/test_gpu_cond_reference.py holds the condensing and expansion kernels against it.

Every function takes a dtype. In np.longdouble (64-bit significand here: u_ld = 2^-64) it is the truth the others are measured
against; in np.float64 it is the PLAIN STATEMENT of the same sums, whose own distance from the truth sets the gate of the device.

    g_0 = x0 - X_0,  g_{k+1} = A_k g_k + b_k                    G_0 = 0,  G_{k+1} = [A_k G_k | B_k]      (dx_k = G_k v + g_k)
    r_k = [x, y, wrap(yaw), v]_k - yref_k[:4] + g_k[:4]   and, for k < N,   U_k - yref_k[4:]
    H = sum_k sc_k J_k' W_k J_k,  q = sum_k sc_k J_k' W_k r_k    J_k = [G_k[:4]; unit rows of the inputs of stage k],  sc_k = dt (k < N), 1 (k = N)
    rows of stage s = 1..N:  G_s[6] with d = X_s[6] + g_s[6]   |   grad h(X_s) . G_s with d = h(X_s) + grad h(X_s) . g_s
    expansion:  dx_0 = x0 - X_0,  dx_{k+1} = A_k dx_k + B_k dv_k + b_k,  X+ = X + dx,  U+ = U + dv
    cost:  sum_k sc_k (1/2 r' W r at (X+, U+), no g) + sum over the soft rows of sc_k (z s + 1/2 Z s^2), lower and upper side

SCALES. Beside every sum stands the same sum with every term replaced by its absolute value, carried through the recursions
(|A| sG + |B|, |A| sg + |b|, ...): the error of any evaluation order in a binary format with unit roundoff u is at most
(number of roundings on the longest path) x u x scale, entry by entry, to first order. Errors are therefore reported in units of
u x scale with u = 2^-53 (`units`): a small entry of a cancelling sum is neither free nor impossible. `ops` is that number of
roundings for the plain order of this file: `ops x u x scale` is the a-priori bound of its float64 run.

h and grad h are INPUTS (tests/model_reference.py evaluates them exactly); wrap(yaw) is model_reference.wrap: fmod is exact in
binary64, and the one rounding of y + 2 pi for a negative yaw is u |wrap(yaw)|, one unit of the residual's scale, which contains
|wrap(yaw)|. Inputs must keep the yaw 1e-3 away from the multiples of 2 pi (`yaw_margin`), so the branch is not in question.
"""
import math

import numpy as np

U53 = 2.0 ** -53
TWO_PI = 2.0 * math.pi


def wrap(yaw):
    """model_reference.wrap, elementwise on float64 (restated: this module imports nothing of the tests)"""
    y = np.fmod(np.asarray(yaw, dtype=np.float64), TWO_PI)
    return np.where(y < 0.0, y + TWO_PI, y)


def wrap_as(yaw, dtype):
    """the same before the final rounding: fmod of two binary64 numbers is exact, the sum is formed in dtype"""
    y = np.fmod(np.asarray(yaw, dtype=np.float64), TWO_PI).astype(dtype)
    return np.where(y < 0, y + dtype(TWO_PI), y)


def yaw_margin(yaw):
    """smallest distance of a yaw from a multiple of 2 pi"""
    y = np.fmod(np.abs(np.asarray(yaw, dtype=np.float64)), TWO_PI)
    return float(np.min(np.minimum(y, TWO_PI - y)))


def full_w(W, N):
    """W as (N + 1, 6, 6): a diagonal (N + 1, 6) is spread out; the terminal stage uses its leading 4 x 4"""
    W = np.asarray(W)
    if W.ndim == 2:
        out = np.zeros((N + 1, 6, 6), dtype=W.dtype)
        for i in range(6):
            out[:, i, i] = W[:, i]
        W = out
    return W


def condense(A, B, b, X, U, x0, yref, W, dt, h, gh, dtype=np.longdouble):
    """dict of H, q, C (2 N x 2 N: row 2 (s - 1) the steering-angle row of stage s, 2 (s - 1) + 1 its gg row), d, G (N + 1, 8, 2 N),
    g (N + 1, 8), res (N + 1, 6); with "s" in front the scale of each, with "n" in front its number of roundings"""
    T = dtype
    N = A.shape[0]
    nv = 2 * N
    A, B, b, X, U, x0, yref = (np.asarray(a).astype(T) for a in (A, B, b, X, U, x0, yref))
    Wf = full_w(np.asarray(W).astype(T), N)
    diagonal = np.asarray(W).ndim == 2
    h, gh = np.asarray(h).astype(T), np.asarray(gh).astype(T)
    aA, aB, ab = np.abs(A), np.abs(B), np.abs(b)
    G = np.zeros((N + 1, 8, nv), dtype=T); sG = np.zeros_like(G)
    g = np.zeros((N + 1, 8), dtype=T); sg = np.zeros_like(g)
    g[0] = x0 - X[0]; sg[0] = np.abs(x0) + np.abs(X[0])
    for k in range(N):
        G[k + 1, :, :2 * k] = A[k] @ G[k, :, :2 * k]; sG[k + 1, :, :2 * k] = aA[k] @ sG[k, :, :2 * k]
        G[k + 1, :, 2 * k:2 * k + 2] = B[k]; sG[k + 1, :, 2 * k:2 * k + 2] = aB[k]
        g[k + 1] = A[k] @ g[k] + b[k]; sg[k + 1] = aA[k] @ sg[k] + ab[k]
    nG = 9 * np.arange(N + 1)          # a product and a sum of eight terms per stage
    ng = 9 * np.arange(N + 1) + 1
    # residuals of the cost
    yw = wrap_as(X[:, 2].astype(np.float64), T)
    y = np.stack([X[:, 0], X[:, 1], yw, X[:, 3]], axis=1)
    res = np.zeros((N + 1, 6), dtype=T); sres = np.zeros_like(res)
    res[:, :4] = y - yref[:, :4] + g[:, :4]; sres[:, :4] = np.abs(y) + np.abs(yref[:, :4]) + sg[:, :4]
    res[:N, 4:] = U - yref[:N, 4:]; sres[:N, 4:] = np.abs(U) + np.abs(yref[:N, 4:])
    nres = ng + 3
    H = np.zeros((nv, nv), dtype=T); sH = np.zeros_like(H); q = np.zeros(nv, dtype=T); sq = np.zeros_like(q)
    for k in range(N + 1):
        ny, sc = (6, T(dt)) if k < N else (4, T(1))
        J = np.zeros((ny, nv), dtype=T); sJ = np.zeros_like(J)
        J[:4] = G[k, :4]; sJ[:4] = sG[k, :4]
        if k < N:
            J[4, 2 * k] = J[5, 2 * k + 1] = 1; sJ[4, 2 * k] = sJ[5, 2 * k + 1] = 1
        Wk = Wf[k, :ny, :ny]
        WJ = sc * (Wk @ J); sWJ = sc * (np.abs(Wk) @ sJ)
        H += J.T @ WJ; sH += sJ.T @ sWJ
        q += WJ.T @ res[k, :ny]; sq += sWJ.T @ sres[k, :ny]
    nW = 3 if diagonal else 8
    nH = 2 * nG[N] + nW + 6 + 6 * (N + 1)          # two factors, the weight, six rows, N + 1 stages
    nq = nG[N] + nres[N] + nW + 6 + 6 * (N + 1)
    # general rows
    C = np.zeros((2 * N, nv), dtype=T); sC = np.zeros_like(C); d = np.zeros(2 * N, dtype=T); sd = np.zeros_like(d)
    for s in range(1, N + 1):
        C[2 * (s - 1)] = G[s, 6]; sC[2 * (s - 1)] = sG[s, 6]
        d[2 * (s - 1)] = X[s, 6] + g[s, 6]; sd[2 * (s - 1)] = np.abs(X[s, 6]) + sg[s, 6]
        C[2 * (s - 1) + 1] = gh[s] @ G[s]; sC[2 * (s - 1) + 1] = np.abs(gh[s]) @ sG[s]
        d[2 * (s - 1) + 1] = h[s] + gh[s] @ g[s]; sd[2 * (s - 1) + 1] = np.abs(h[s]) + np.abs(gh[s]) @ sg[s]
    nC = nG[N] + 9; nd = ng[N] + 10
    return dict(H=H, q=q, C=C, d=d, G=G, g=g, res=res, sH=sH, sq=sq, sC=sC, sd=sd, sG=sG, sg=sg, sres=sres,
                nH=int(nH), nq=int(nq), nC=int(nC), nd=int(nd), nG=int(nG[N]), ng=int(ng[N]), nres=int(nres[N]))


def expand(A, B, b, X, U, x0, dv, dtype=np.longdouble):
    """X+ (N + 1, 8), U+ (N, 2) of the full step dv (2 N,), with their scales sX, sU and roundings nX, nU"""
    T = dtype
    N = A.shape[0]
    A, B, b, X, U, x0 = (np.asarray(a).astype(T) for a in (A, B, b, X, U, x0))
    dv = np.asarray(dv).astype(T).reshape(N, 2)
    aA, aB, ab, adv = np.abs(A), np.abs(B), np.abs(b), np.abs(dv)
    dx = np.zeros((N + 1, 8), dtype=T); sdx = np.zeros_like(dx)
    dx[0] = x0 - X[0]; sdx[0] = np.abs(x0) + np.abs(X[0])
    for k in range(N):
        dx[k + 1] = A[k] @ dx[k] + B[k] @ dv[k] + b[k]
        sdx[k + 1] = aA[k] @ sdx[k] + aB[k] @ adv[k] + ab[k]
    return dict(X=X + dx, U=U + dv, dx=dx, sX=np.abs(X) + sdx, sU=np.abs(U) + adv, sdx=sdx, nX=12 * N + 2, nU=1)


def step_sensitivity(A, B, w, dtype=np.longdouble):
    """sum over the stages of |Phi B_k| w_k as the scale recursion forms it: what a perturbation of dv of size w (N, 2) can move dx by"""
    T = dtype
    N = A.shape[0]
    aA, aB, w = np.abs(np.asarray(A).astype(T)), np.abs(np.asarray(B).astype(T)), np.abs(np.asarray(w).astype(T)).reshape(N, 2)
    s = np.zeros((N + 1, 8), dtype=T)
    for k in range(N):
        s[k + 1] = aA[k] @ s[k] + aB[k] @ w[k]
    return s


def cost(X, U, yref, W, dt, sl, su, zl, zu, Zl, Zu, dtype=np.longdouble):
    """eval_cost of the oracle at (X, U) with the slack values sl, su (3 N each: [bu_k k = 0..N-1 | (bx_k, h_k) k = 1..N]) and the
    penalties z, Z (N + 1, 3: slots bu, bx, h of every stage). Returns (cost, scale, roundings)."""
    T = dtype
    N = U.shape[0]
    Xf = np.asarray(X, dtype=np.float64)
    X, U, yref, sl, su, zl, zu, Zl, Zu = (np.asarray(a).astype(T) for a in (X, U, yref, sl, su, zl, zu, Zl, Zu))
    Wf = full_w(np.asarray(W).astype(T), N)
    c = T(0); s = T(0)
    half = T(0.5)
    for k in range(N + 1):
        ny, sc = (6, T(dt)) if k < N else (4, T(1))
        y = np.zeros(6, dtype=T); y[:2] = X[k, :2]; y[2] = wrap_as(Xf[k, 2], T); y[3] = X[k, 3]
        if k < N:
            y[4:] = U[k]
        r = (y - yref[k])[:ny]; sr = (np.abs(y) + np.abs(yref[k]))[:ny]
        c += sc * half * (r @ (Wf[k, :ny, :ny] @ r)); s += sc * half * (sr @ (np.abs(Wf[k, :ny, :ny]) @ sr))
    for i in range(3 * N):
        k, slot = (i, 0) if i < N else (1 + (i - N) // 2, 1 + (i - N) % 2)
        sc = T(dt) if k < N else T(1)
        for z, Z, v in ((zl, Zl, sl), (zu, Zu, su)):
            t = sc * (z[k, slot] * v[i] + half * Z[k, slot] * v[i] * v[i])
            c += t; s += sc * (np.abs(z[k, slot] * v[i]) + half * np.abs(Z[k, slot]) * v[i] * v[i])
    return c, s, 6 * (N + 1) + 6 * N + 20


def units(got, truth, scale):
    """largest |got - truth| / (u x scale) over the entries, u = 2^-53; an entry of scale 0 must be equal (inf otherwise)"""
    got = np.asarray(got).astype(np.longdouble); truth = np.asarray(truth).astype(np.longdouble); scale = np.asarray(scale).astype(np.longdouble)
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, np.longdouble(0), err / (np.longdouble(U53) * scale))
    return float(np.max(r)) if r.size else 0.0
