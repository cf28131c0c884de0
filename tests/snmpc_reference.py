"""
The condensed QP of one SQP real-time iteration of the COUPLED SNMPC OCP, and the expansion of its step, once more: written from the
comments of snmpc_solve / snmpc_step / snmpc_h (oracle/nmpc_oracle.c) in the DENSE STACKED form -- 8 (n_s + 1)-state stage matrices
and dense condensing -- with numpy alone and no code shared with the kernels or the oracle. The device exploits the block structure
(snmpc_kernels.hpp); this file does not, so it is an independent statement of the same operation. Not a test module:
tests/test_snmpc_reference.py holds it against the oracle (CPU), tests/test_gpu_snmpc_reference.py holds the kernels against it.

Every function takes a dtype, as in tests/cond_reference.py: np.longdouble is the truth, np.float64 the PLAIN STATEMENT whose own
distance from the truth sets the gate of the device; beside every sum stands the same sum of absolute values, carried through the
recursions (cond_reference: SCALES), and errors are reported in units of u x scale, u = 2^-53 (cond_reference.units).

    stacked state: copy 0 the nominal one, copies 1 .. n_s the samples; a = A_pce[0]
    k <  uph:  block i of A_k, B_k, b_k is As[k, i], Bs[k, i], bs[k, i]; the nominal rows are a_i As[k, i] at the columns of sample i,
               B_nom = sum_i a_i Bs[k, i], b_nom = sum_i a_i (bs[k, i] + X^(i)_{k+1}) - X_nom,k+1
    k >= uph:  the nominal block is An, Bn, bn; the samples are the identity with zero defect
    g_0 = x0 - X_0,  G_{k+1} = [A_k G_k | B_k],  g_{k+1} = A_k g_k + b_k
    cost on the nominal copy, outputs [x, y, wrap(yaw), |v|, u]: the |v| row is cl G[3] + ct G[4], cl = vl / |v|, ct = vt / |v| formed in
               the dtype from X, its residual |v| - yref + cl g[3] + ct g[4]; diagonal weights
    rows of stage s: G_s[6] with d = X_s[6] + g_s[6] | the gg row: for s >= uph ghn[s] . G_s (nominal block), d = hn[s] + ghn[s] . g_s;
               for 1 <= s < uph the chance row: c = A_pce hs[s], sd = sqrt(sum_{l>=1} c_l^2), h = c_0 + kappa sd,
               w_i = a_i + kappa (sum_{l>=1} c_l A_pce[l, i]) / sd (a_i where sd == 0), gradient block of sample i: w_i ghs[s, i]
    scales of the two non-linear steps, to first order: s_var = sum 2 |c_l| s_c_l, s_sd = s_var / (2 sd),
               s_w_i = |a_i| + kappa (s_acc / sd + |acc| s_sd / sd^2)
    expansion: dx_0 = x0 - X_0, dx_{k+1} = A_k dx_k + B_k dv_k + b_k, X+ = X + dx, U+ = U + dv; sample copies beyond uph are FROZEN:
               X^(i)_k = X^(i)_uph; cost as snmpc_eval_cost at (X+, U+) with the slacks handed in

h and grad h (hs, ghs, hn, ghn) are INPUTS (tests/model_reference.py: eval_h_vabs evaluates them exactly); kappa is the binary64
number sqrt((1 - gamma) / gamma).
"""
import numpy as np

from cond_reference import U53, units, wrap_as, yaw_margin          # noqa: F401  (re-exported: the tests take them from here)


def kappa_of(gamma):
    return float(np.sqrt(np.float64((1.0 - gamma) / gamma)))


def stage_matrices(As, Bs, bs, An, Bn, bn, X, Apce, dtype=np.longdouble):
    """A (N, nxs, nxs), B (N, nxs, 2), b (N, nxs) and the scale of b (|A|, |B| are the scales of A, B but for the nominal rows: sA, sB)
    X (N + 1, n_s + 1, 8); As (uph, n_s, 8, 8) ...; An (N - uph, 8, 8) ..."""
    T = dtype
    N, ns = X.shape[0] - 1, X.shape[1] - 1
    uph = As.shape[0]
    nxs = 8 * (ns + 1)
    As, Bs, bs, An, Bn, bn, X, Apce = (np.asarray(v).astype(T) for v in (As, Bs, bs, An, Bn, bn, X, Apce))
    a = Apce[0]; aa = np.abs(a)
    A = np.zeros((N, nxs, nxs), dtype=T); B = np.zeros((N, nxs, 2), dtype=T); b = np.zeros((N, nxs), dtype=T)
    sA = np.zeros_like(A); sB = np.zeros_like(B); sb = np.zeros_like(b)
    for k in range(N):
        if k < uph:
            for i in range(ns):
                r = slice(8 * (i + 1), 8 * (i + 2))
                A[k, r, r] = As[k, i]; B[k, r] = Bs[k, i]; b[k, r] = bs[k, i]
                sA[k, r, r] = np.abs(As[k, i]); sB[k, r] = np.abs(Bs[k, i]); sb[k, r] = np.abs(bs[k, i])
                A[k, :8, r] = a[i] * As[k, i]; sA[k, :8, r] = aa[i] * np.abs(As[k, i])
                B[k, :8] += a[i] * Bs[k, i]; sB[k, :8] += aa[i] * np.abs(Bs[k, i])
                b[k, :8] += a[i] * (bs[k, i] + X[k + 1, i + 1]); sb[k, :8] += aa[i] * (np.abs(bs[k, i]) + np.abs(X[k + 1, i + 1]))
            b[k, :8] -= X[k + 1, 0]; sb[k, :8] += np.abs(X[k + 1, 0])
        else:
            A[k, :8, :8] = An[k - uph]; B[k, :8] = Bn[k - uph]; b[k, :8] = bn[k - uph]
            sA[k, :8, :8] = np.abs(An[k - uph]); sB[k, :8] = np.abs(Bn[k - uph]); sb[k, :8] = np.abs(bn[k - uph])
            for j in range(8, nxs):
                A[k, j, j] = 1; sA[k, j, j] = 1
    return dict(A=A, B=B, b=b, sA=sA, sB=sB, sb=sb, uph=uph, ns=ns, N=N)


def chance_row(Apce, hs, ghs, kappa, dtype=np.longdouble):
    """value h, gradient (n_s, 8) w.r.t. the sample copies, their scales, and sd, of one stage: hs (n_s,), ghs (n_s, 8)"""
    T = dtype
    Apce, hs, ghs = (np.asarray(v).astype(T) for v in (Apce, hs, ghs))
    kap = T(kappa)
    a = Apce[0]
    c = Apce @ hs; s_c = np.abs(Apce) @ np.abs(hs)
    var = np.sum(c[1:] * c[1:]); s_var = np.sum(2 * np.abs(c[1:]) * s_c[1:])
    sd = np.sqrt(var)
    h = c[0] + kap * sd
    if sd > 0:
        s_sd = s_var / (2 * sd)
        acc = c[1:] @ Apce[1:]; s_acc = s_c[1:] @ np.abs(Apce[1:])
        w = a + kap * acc / sd
        s_w = np.abs(a) + kap * (s_acc / sd + np.abs(acc) * s_sd / (sd * sd))
    else:
        s_sd = T(0)
        w = a.copy(); s_w = np.abs(a)
    s_h = s_c[0] + kap * s_sd
    return dict(h=h, s_h=s_h, grad=w[:, None] * ghs, s_grad=s_w[:, None] * np.abs(ghs), sd=sd, w=w)


def condense(lin, X, U, x0, yref, W, dt, Apce, kappa, dtype=np.longdouble):
    """lin: dict As, Bs, bs, hs (uph, n_s), ghs (uph, n_s, 8), hn (N + 1,), ghn (N + 1, 8), An, Bn, bn. X (N + 1, n_s + 1, 8),
    U (N, 2), x0 (n_s + 1, 8), yref (N + 1, 6), W (N + 1, 6) diagonal. Returns H, q, C (2 N x 2 N: row 2 (s - 1) the steering-angle row
    of stage s, 2 (s - 1) + 1 its gg / chance row), d, G, g, with "s" in front their scales, and sdmin (smallest sd of the chance rows)"""
    T = dtype
    M = stage_matrices(lin["As"], lin["Bs"], lin["bs"], lin["An"], lin["Bn"], lin["bn"], X, Apce, T)
    N, ns, uph = M["N"], M["ns"], M["uph"]
    nxs, nv = 8 * (ns + 1), 2 * N
    Xf = np.asarray(X, dtype=np.float64)
    X, U, x0, yref, W = (np.asarray(v).astype(T) for v in (X, U, x0, yref, W))
    Xs = X.reshape(N + 1, nxs)
    G = np.zeros((N + 1, nxs, nv), dtype=T); sG = np.zeros_like(G)
    g = np.zeros((N + 1, nxs), dtype=T); sg = np.zeros_like(g)
    g[0] = x0.reshape(nxs) - Xs[0]; sg[0] = np.abs(x0.reshape(nxs)) + np.abs(Xs[0])
    for k in range(N):
        G[k + 1, :, :2 * k] = M["A"][k] @ G[k, :, :2 * k]; sG[k + 1, :, :2 * k] = M["sA"][k] @ sG[k, :, :2 * k]
        G[k + 1, :, 2 * k:2 * k + 2] = M["B"][k]; sG[k + 1, :, 2 * k:2 * k + 2] = M["sB"][k]
        g[k + 1] = M["A"][k] @ g[k] + M["b"][k]; sg[k + 1] = M["sA"][k] @ sg[k] + M["sb"][k]
    # cost on the nominal copy
    H = np.zeros((nv, nv), dtype=T); sH = np.zeros_like(H); q = np.zeros(nv, dtype=T); sq = np.zeros_like(q)
    yw = wrap_as(Xf[:, 0, 2], T)
    for k in range(N + 1):
        ny, sc = (6, T(dt)) if k < N else (4, T(1))
        vl, vt = X[k, 0, 3], X[k, 0, 4]
        vabs = np.sqrt(vl * vl + vt * vt)
        cl, ct = (vl / vabs, vt / vabs) if vabs > 0 else (T(0), T(0))
        J = np.zeros((ny, nv), dtype=T); sJ = np.zeros_like(J); r = np.zeros(ny, dtype=T); sr = np.zeros_like(r)
        J[:3] = G[k, :3]; sJ[:3] = sG[k, :3]
        J[3] = cl * G[k, 3] + ct * G[k, 4]; sJ[3] = np.abs(cl) * sG[k, 3] + np.abs(ct) * sG[k, 4]
        y = np.array([X[k, 0, 0], X[k, 0, 1], yw[k], vabs], dtype=T)
        r[:4] = y - yref[k, :4]; sr[:4] = np.abs(y) + np.abs(yref[k, :4])
        r[:3] += g[k, :3]; sr[:3] += sg[k, :3]
        r[3] += cl * g[k, 3] + ct * g[k, 4]; sr[3] += np.abs(cl) * sg[k, 3] + np.abs(ct) * sg[k, 4]
        if k < N:
            J[4, 2 * k] = J[5, 2 * k + 1] = 1; sJ[4, 2 * k] = sJ[5, 2 * k + 1] = 1
            r[4:] = U[k] - yref[k, 4:]; sr[4:] = np.abs(U[k]) + np.abs(yref[k, 4:])
        WJ = sc * (W[k, :ny, None] * J); sWJ = sc * (np.abs(W[k, :ny, None]) * sJ)
        H += J.T @ WJ; sH += sJ.T @ sWJ
        q += WJ.T @ r; sq += sWJ.T @ sr
    # rows
    C = np.zeros((2 * N, nv), dtype=T); sC = np.zeros_like(C); d = np.zeros(2 * N, dtype=T); sd = np.zeros_like(d)
    hn, ghn = np.asarray(lin["hn"]).astype(T), np.asarray(lin["ghn"]).astype(T)
    sdmin = np.inf
    for s in range(1, N + 1):
        C[2 * (s - 1)] = G[s, 6]; sC[2 * (s - 1)] = sG[s, 6]
        d[2 * (s - 1)] = Xs[s, 6] + g[s, 6]; sd[2 * (s - 1)] = np.abs(Xs[s, 6]) + sg[s, 6]
        grad = np.zeros(nxs, dtype=T); sgrad = np.zeros_like(grad)
        if s >= uph:
            grad[:8] = ghn[s]; sgrad[:8] = np.abs(ghn[s]); h, s_h = hn[s], np.abs(hn[s])
        else:
            cr = chance_row(Apce, lin["hs"][s], lin["ghs"][s], kappa, T)
            grad[8:] = cr["grad"].reshape(-1); sgrad[8:] = cr["s_grad"].reshape(-1); h, s_h = cr["h"], cr["s_h"]
            sdmin = min(sdmin, float(cr["sd"]))
        C[2 * (s - 1) + 1] = grad @ G[s]; sC[2 * (s - 1) + 1] = sgrad @ sG[s]
        d[2 * (s - 1) + 1] = h + grad @ g[s]; sd[2 * (s - 1) + 1] = s_h + sgrad @ sg[s]
    return dict(H=H, q=q, C=C, d=d, G=G, g=g, sH=sH, sq=sq, sC=sC, sd=sd, sG=sG, sg=sg, sdmin=sdmin, M=M)


def expand(M, X, U, x0, dv, dtype=np.longdouble):
    """X+ (N + 1, n_s + 1, 8) and U+ (N, 2) of the full step dv (2 N,) with their scales; M: stage_matrices in the same dtype.
    The sample copies of the stages beyond uph are those of stage uph (frozen)."""
    T = dtype
    N, ns, uph = M["N"], M["ns"], M["uph"]
    nxs = 8 * (ns + 1)
    X, U, x0 = (np.asarray(v).astype(T) for v in (X, U, x0))
    dv = np.asarray(dv).astype(T).reshape(N, 2); adv = np.abs(dv)
    Xs = X.reshape(N + 1, nxs)
    dx = np.zeros((N + 1, nxs), dtype=T); sdx = np.zeros_like(dx)
    dx[0] = x0.reshape(nxs) - Xs[0]; sdx[0] = np.abs(x0.reshape(nxs)) + np.abs(Xs[0])
    for k in range(N):
        dx[k + 1] = M["A"][k] @ dx[k] + M["B"][k] @ dv[k] + M["b"][k]
        sdx[k + 1] = M["sA"][k] @ sdx[k] + M["sB"][k] @ adv[k] + M["sb"][k]
    Xp = (Xs + dx).reshape(N + 1, ns + 1, 8); sX = (np.abs(Xs) + sdx).reshape(N + 1, ns + 1, 8)
    for k in range(uph + 1, N + 1):
        Xp[k, 1:] = Xp[uph, 1:]; sX[k, 1:] = sX[uph, 1:]
    return dict(X=Xp, U=U + dv, sX=sX, sU=np.abs(U) + adv)


def cost(Xn, U, yref, W, dt, sl, su, zl, zu, Zl, Zu, dtype=np.longdouble):
    """snmpc_eval_cost at the nominal copy Xn (N + 1, 8) and U, slacks sl, su (3 N each: [bu_k k = 0..N-1 | (bx_k, h_k) k = 1..N]),
    penalties (N + 1, 3). Returns (cost, scale)."""
    T = dtype
    N = U.shape[0]
    Xf = np.asarray(Xn, dtype=np.float64)
    Xn, U, yref, W, sl, su, zl, zu, Zl, Zu = (np.asarray(v).astype(T) for v in (Xn, U, yref, W, sl, su, zl, zu, Zl, Zu))
    c = T(0); s = T(0); half = T(0.5)
    for k in range(N + 1):
        ny, sc = (6, T(dt)) if k < N else (4, T(1))
        y = np.zeros(6, dtype=T)
        y[:2] = Xn[k, :2]; y[2] = wrap_as(Xf[k, 2], T); y[3] = np.sqrt(Xn[k, 3] * Xn[k, 3] + Xn[k, 4] * Xn[k, 4])
        if k < N:
            y[4:] = U[k]
        r = (y - yref[k])[:ny]; sr = (np.abs(y) + np.abs(yref[k]))[:ny]
        c += sc * half * np.sum(W[k, :ny] * r * r); s += sc * half * np.sum(np.abs(W[k, :ny]) * sr * sr)
    for i in range(3 * N):
        k, slot = (i, 0) if i < N else (1 + (i - N) // 2, 1 + (i - N) % 2)
        sc = T(dt) if k < N else T(1)
        for z, Z, v in ((zl, Zl, sl), (zu, Zu, su)):
            c += sc * (z[k, slot] * v[i] + half * Z[k, slot] * v[i] * v[i])
            s += sc * (np.abs(z[k, slot] * v[i]) + half * np.abs(Z[k, slot]) * v[i] * v[i])
    return c, s


def step_sensitivity(M, w):
    """what a perturbation of dv of size w (N, 2) can move dx by: the scale recursion with |dv| = w and nothing else"""
    N = M["N"]
    w = np.abs(np.asarray(w).astype(M["sA"].dtype)).reshape(N, 2)
    s = np.zeros((N + 1, M["sA"].shape[1]), dtype=M["sA"].dtype)
    for k in range(N):
        s[k + 1] = M["sA"][k] @ s[k] + M["sB"][k] @ w[k]
    return s
