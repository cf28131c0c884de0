// bo_kernels.hpp -- K15: the acquisition value of the Bayesian-optimisation step (Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/acquisition.py:
// feasibility-weighted expected hypervolume improvement over two exact GPs on the feasible trials and a two-class Dirichlet
// classification GP on all trials; include/tum_nmpc.h states the mathematics). One evaluation of C candidates is this chain:
//   bo_kern_kernel      k(X, x) of every candidate against the six point sets (objective 0 / 1 on X_t, class 0 / 1 on X_c, objective
//                       0 / 1 on X_b), plain vector code, into column-tile buffers [tile of 16 candidates][point][16].
//   bo_tri_kernel       q = V k (and, a second launch, l = R sig): one wavefront per 16-row tile of a packed lower-triangular factor and
//                       BO_NCT column tiles, on v_mfma_f64_16x16x4_f64; the blocks right of the diagonal tile are neither stored nor
//                       multiplied. Writes the product, the tile's column sums of squares and the tile's share of k . a.
//   bo_moments_kernel   per (model, candidate): mean = c + k . a and |q|^2 from the tile sums.
//   bo_cross_kernel     sig = k(X_b, x) - H q: one wavefront per 16 baseline rows and BO_NCT column tiles, K = n_t.
//   bo_hvi_kernel       one wavefront per (16 samples, 16 candidates): Z l of both objectives on the matrix cores, the sample
//                       f = mu + Z l + sqrt(d2) zeta, its hypervolume improvement over that sample's front, summed over the 16 samples.
//                       The S x C samples never reach memory.
//   bo_final_kernel     per candidate: the mean over the sample tiles, the feasibility factor by Gauss-Hermite quadrature, alpha.
// Determinism: no floating-point atomics; every sum is one chain or one fixed tree whose order is a function of the model's sizes
// alone, and no sum runs across candidates: a candidate's bits do not depend on its neighbours in the launch.
#pragma once
#include "nmpc_device.hpp"

namespace tum {

constexpr int BO_NCT = 4;              // column tiles (of 16 candidates) one wavefront of the product kernels carries: one A read, four products
constexpr int BO_MAXD = 16;
constexpr int BO_MAXK = 64;            // quadrature nodes
constexpr int BO_GP = 4;               // GP models: objective 0, 1, class 0, 1
constexpr int BO_SETS = 6;             // point sets of bo_kern_kernel: the four above and the baseline under objective 0, 1
enum { BO_D_MU0, BO_D_MU1, BO_D_D20, BO_D_D21, BO_D_HVI, BO_D_P, BO_D_SD, BO_D_FACTOR, BO_DETAIL };

// blocks of 64 doubles in front of row tile t of a packed lower-triangular factor: tile t holds its 4 (t + 1) blocks q = 0 .. 4 t + 3
__host__ __device__ __forceinline__ size_t bo_tri_off(int t) { return (size_t)2 * t * (t + 1); }

struct BoKernArgs {
    int d, C, nct;                              // dimension, candidates of this launch, column tiles written (a multiple of BO_NCT)
    const double *x;                            // [C][d]
    int n[BO_SETS], np[BO_SETS];                // points, padded to a multiple of 16
    const double *X[BO_SETS], *ils[BO_SETS];    // [n][d], [d] inverse length scales
    double s[BO_SETS];
    double *k[BO_SETS];                         // [nct][np][16]
};

// grid (row tiles of the largest set, nct, BO_SETS), 256 threads: thread (row = tid >> 4, column = tid & 15)
__global__ void __launch_bounds__(256) bo_kern_kernel(const BoKernArgs a)
{
#pragma clang fp contract(off)
    const int g = blockIdx.z, ct = blockIdx.y, i = blockIdx.x * 16 + (threadIdx.x >> 4), col = threadIdx.x & 15, c = ct * 16 + col;
    if (i >= a.np[g]) return;
    double v = 0.0;
    if (i < a.n[g] && c < a.C) {
        const double *X = a.X[g] + (size_t)i * a.d, *x = a.x + (size_t)c * a.d, *ils = a.ils[g];
        double r = 0.0;
        for (int j = 0; j < a.d; j++) {
            const double t = (X[j] - x[j]) * ils[j];
            r = r + t * t;
        }
        v = a.s[g] * exp(-0.5 * r);
    }
    a.k[g][((size_t)ct * a.np[g] + i) * 16 + col] = v;
}

// the column sums of squares of one 16 x 16 D tile: over the four rows of the lane, then over the four quads; every lane of a column
// ends with the same bits (the two exchanges add the same pair in either order)
__device__ __forceinline__ double bo_colsq(const d4 acc)
{
#pragma clang fp contract(off)
    double p = (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
    p = p + __shfl_xor(p, 16);
    p = p + __shfl_xor(p, 32);
    return p;
}

struct BoTriArgs {
    int n_units, nct;
    int first[BO_GP + 1];                       // first workgroup (row tile) of unit u; the total behind the last
    int np[BO_GP];
    const double *T[BO_GP];                     // packed factor: tile t at bo_tri_off(t) * 64, block q: lane holds T[16 t + (lane & 15)][4 q + (lane >> 4)]
    const double *in[BO_GP];                    // [nct][np][16]
    double *out[BO_GP];                         // [nct][np][16] or null
    double *part[BO_GP];                        // [nct][np / 16][16]: the tile's column sums of squares of the product
    const double *a[BO_GP];                     // [np] or null: with it, the tile's share of in . a (its 16 rows of `in`) goes to dot
    double *dot[BO_GP];                         // [nct][np / 16][16]
};

// grid (row tiles of all units, nct / BO_NCT), 64 threads. The last four blocks of a row tile are its diagonal tile: their B operands
// are the tile's own 16 rows of `in`, one per (quad, block) -- the dot product with a rides on them.
__global__ void __launch_bounds__(64) bo_tri_kernel(const BoTriArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    int u = 0;
    while (u + 1 < a.n_units && (int)blockIdx.x >= a.first[u + 1]) u++;
    const int np = a.np[u], nt = np >> 4;
    const int t = nt - 1 - ((int)blockIdx.x - a.first[u]);          // the long rows first
    const int ct0 = blockIdx.y * BO_NCT, nq = 4 * (t + 1);
    const double *T = a.T[u] + bo_tri_off(t) * 64 + lane;
    const double *x = a.in[u] + ((size_t)ct0 * np + quad) * 16 + col;
    const size_t cs = (size_t)np * 16;
    d4 acc[BO_NCT];
#pragma unroll
    for (int g = 0; g < BO_NCT; g++) acc[g] = d4{0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < nq - 4; q++) {
        const double w = T[(size_t)q * 64];
#pragma unroll
        for (int g = 0; g < BO_NCT; g++) acc[g] = mfma(w, x[g * cs + (size_t)q * 64], acc[g]);
    }
    const double *av = a.a[u];
    double dot[BO_NCT] = {};
    for (int q = nq - 4; q < nq; q++) {
        const double w = T[(size_t)q * 64], ar = av ? av[4 * q + quad] : 0.0;
#pragma unroll
        for (int g = 0; g < BO_NCT; g++) {
            const double b = x[g * cs + (size_t)q * 64];
            acc[g] = mfma(w, b, acc[g]);
            dot[g] = dot[g] + b * ar;
        }
    }
#pragma unroll
    for (int g = 0; g < BO_NCT; g++) {
        const int ct = ct0 + g;
        if (av) {
            double dsum = dot[g] + __shfl_xor(dot[g], 16);
            dsum = dsum + __shfl_xor(dsum, 32);
            if (quad == 0) a.dot[u][((size_t)ct * nt + t) * 16 + col] = dsum;
        }
        if (a.out[u]) {
#pragma unroll
            for (int j = 0; j < 4; j++) a.out[u][((size_t)ct * np + 16 * t + quad + 4 * j) * 16 + col] = acc[g][j];
        }
        const double p = bo_colsq(acc[g]);
        if (quad == 0) a.part[u][((size_t)ct * nt + t) * 16 + col] = p;
    }
}

struct BoMomArgs {
    int C;
    int n[BO_GP], np[BO_GP];
    const double *part[BO_GP], *dot[BO_GP];        // bo_tri_kernel's tile sums
    double c[BO_GP];
    double *mom;                                // [BO_GP][C padded to 16][2]: mean, |q|^2
    int cp;
};

// grid (ceil(C / 64), BO_GP), 64 threads: one lane per (model, candidate), both sums one chain over the row tiles in index order
__global__ void __launch_bounds__(64) bo_moments_kernel(const BoMomArgs a)
{
#pragma clang fp contract(off)
    const int g = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.C) return;
    const int ct = c >> 4, col = c & 15, np = a.np[g], nt = np >> 4;
    const double *p = a.part[g] + (size_t)ct * nt * 16 + col, *dp = a.dot[g] + (size_t)ct * nt * 16 + col;
    double m = 0.0, qq = 0.0;
    for (int t = 0; t < nt; t++) { m = m + dp[t * 16]; qq = qq + p[t * 16]; }
    double *o = a.mom + ((size_t)g * a.cp + c) * 2;
    o[0] = a.c[g] + m; o[1] = qq;
}

struct BoCrossArgs {
    int nct, npt, npb;                          // column tiles, n_t and n_b padded to multiples of 16
    const double *H[2];                         // [npb / 16][npt / 4][64]: lane holds H[16 t + (lane & 15)][4 q + (lane >> 4)]
    const double *q[2], *kb[2];                 // [nct][npt][16], [nct][npb][16]
    double *sig[2];                             // [nct][npb][16]
};

// grid (npb / 16, nct / BO_NCT, 2), 64 threads
__global__ void __launch_bounds__(64) bo_cross_kernel(const BoCrossArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int t = blockIdx.x, ct0 = blockIdx.y * BO_NCT, o = blockIdx.z, nq = a.npt >> 2;
    const double *H = a.H[o] + (size_t)t * nq * 64 + lane;
    const double *x = a.q[o] + ((size_t)ct0 * a.npt + quad) * 16 + col;
    const size_t cs = (size_t)a.npt * 16;
    d4 acc[BO_NCT];
#pragma unroll
    for (int g = 0; g < BO_NCT; g++) acc[g] = d4{0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < nq; q++) {
        const double w = H[(size_t)q * 64];
#pragma unroll
        for (int g = 0; g < BO_NCT; g++) acc[g] = mfma(w, x[g * cs + (size_t)q * 64], acc[g]);
    }
#pragma unroll
    for (int g = 0; g < BO_NCT; g++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t at = ((size_t)(ct0 + g) * a.npb + 16 * t + quad + 4 * j) * 16 + col;
            a.sig[o][at] = a.kb[o][at] - acc[g][j];
        }
}

// d2 = max(s - |q|^2 - |l|^2, jitter) of one candidate: the one statement of it, for bo_hvi_kernel and bo_final_kernel alike
__device__ __forceinline__ double bo_d2(double s, double qq, const double *llpart, int ntb, double jitter)
{
#pragma clang fp contract(off)
    double ll = 0.0;
    for (int t = 0; t < ntb; t++) ll = ll + llpart[t * 16];
    const double v = (s - qq) - ll;
    return v > jitter ? v : jitter;
}

struct BoHviArgs {
    int C, cp, S, npb, nts, P_max;              // candidates, mom's stride, samples, n_b padded, sample tiles, rows of a front
    const double *Z[2];                         // [nts][npb / 4][64]: lane holds Z[16 t + (lane & 15)][4 q + (lane >> 4)], zero where padded
    const double *zeta[2];                      // [16 nts]
    const double *l[2], *llpart[2];             // [nct][npb][16], [nct][npb / 16][16]
    const double *mom;
    double s[2], jitter[2], ref[2];
    const double *fronts; const int *count;     // [S][P_max][2] ascending in objective 0, [S]
    double *part;                               // [nct][nts][16]
};

// The hypervolume improvement of the point f over a front of P points (ascending in objective 0, so descending in objective 1):
// cell i spans objective 0 from the previous front point (the reference point for i = 0) to front point i and is open above that
// point's objective 1; the last cell is open to the right, above the reference point.
__device__ __forceinline__ double bo_hvi(const double *fr, int P, double r0, double r1, double f0, double f1)
{
#pragma clang fp contract(off)
    double hv = 0.0, xp = r0;
    for (int i = 0; i < P; i++) {
        const double xn = fr[2 * i], h = fr[2 * i + 1];
        const double w = (f0 < xn ? f0 : xn) - xp, e = f1 - h;
        hv = hv + (w > 0.0 ? w : 0.0) * (e > 0.0 ? e : 0.0);
        xp = xn;
    }
    const double w = f0 - xp, e = f1 - r1;
    return hv + (w > 0.0 ? w : 0.0) * (e > 0.0 ? e : 0.0);
}

// grid (nts, column tiles), 64 threads
__global__ void __launch_bounds__(64) bo_hvi_kernel(const BoHviArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int ts = blockIdx.x, ct = blockIdx.y, nq = a.npb >> 2, ntb = a.npb >> 4;
    const int c = ct * 16 + col, cc = c < a.C ? c : a.C - 1;          // (the columns behind the last candidate compute on it and are dropped)
    d4 acc[2];
    double mu[2], sd[2];
#pragma unroll
    for (int o = 0; o < 2; o++) {
        const double *Z = a.Z[o] + (size_t)ts * nq * 64 + lane, *x = a.l[o] + ((size_t)ct * a.npb + quad) * 16 + col;
        acc[o] = d4{0.0, 0.0, 0.0, 0.0};
        for (int q = 0; q < nq; q++) acc[o] = mfma(Z[(size_t)q * 64], x[(size_t)q * 64], acc[o]);
        const double *m = a.mom + ((size_t)o * a.cp + cc) * 2;
        mu[o] = m[0];
        sd[o] = sqrt(bo_d2(a.s[o], m[1], a.llpart[o] + (size_t)ct * ntb * 16 + col, ntb, a.jitter[o]));
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int s = 16 * ts + quad + 4 * j;
        double hv = 0.0;
        if (s < a.S) {
            const double f0 = (mu[0] + acc[0][j]) + sd[0] * a.zeta[0][s], f1 = (mu[1] + acc[1][j]) + sd[1] * a.zeta[1][s];
            hv = bo_hvi(a.fronts + (size_t)s * a.P_max * 2, a.count[s], a.ref[0], a.ref[1], f0, f1);
        }
        sum = sum + hv;
    }
    sum = sum + __shfl_xor(sum, 16);
    sum = sum + __shfl_xor(sum, 32);
    if (quad == 0) a.part[((size_t)ct * a.nts + ts) * 16 + col] = sum;
}

__device__ __forceinline__ double bo_sigmoid(double t)
{
#pragma clang fp contract(off)
    if (t >= 0.0) return 1.0 / (1.0 + exp(-t));
    const double e = exp(t);
    return e / (1.0 + e);
}

struct BoFinalArgs {
    int C, cp, S, nts, npb, K;
    const double *mom, *llpart[2], *hvpart;
    double s[BO_GP], jitter[2], eps;
    const double *gh_x, *gh_w;                  // the rule for a standard normal: E g(t) = sum w g(m + sd x)
    double *alpha, *detail;                     // [C], [C][BO_DETAIL]
};

// grid (ceil(C / 64)), 64 threads: one lane per candidate
__global__ void __launch_bounds__(64) bo_final_kernel(const BoFinalArgs a)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.C) return;
    const int ct = c >> 4, col = c & 15, ntb = a.npb >> 4;
    double mu[BO_GP], qq[BO_GP];
#pragma unroll
    for (int g = 0; g < BO_GP; g++) {
        const double *m = a.mom + ((size_t)g * a.cp + c) * 2;
        mu[g] = m[0]; qq[g] = m[1];
    }
    double d2[2];
#pragma unroll
    for (int o = 0; o < 2; o++) d2[o] = bo_d2(a.s[o], qq[o], a.llpart[o] + (size_t)ct * ntb * 16 + col, ntb, a.jitter[o]);
    const double *hp = a.hvpart + (size_t)ct * a.nts * 16 + col;
    double hv = 0.0;
    for (int t = 0; t < a.nts; t++) hv = hv + hp[t * 16];
    hv = hv / (double)a.S;
    // the feasibility factor: t ~ N(m_1 - m_0, v_0 + v_1), p = E sigmoid(t), sd^2 = E (sigmoid(t) - p)^2
    const double m = mu[3] - mu[2];
    double var = (a.s[2] - qq[2]) + (a.s[3] - qq[3]);
    var = var > 0.0 ? var : 0.0;
    const double st = sqrt(var);
    double p = 0.0;
    for (int i = 0; i < a.K; i++) p = p + a.gh_w[i] * bo_sigmoid(m + st * a.gh_x[i]);
    double v2 = 0.0;
    for (int i = 0; i < a.K; i++) {
        const double e = bo_sigmoid(m + st * a.gh_x[i]) - p;
        v2 = v2 + a.gh_w[i] * (e * e);
    }
    const double sdv = sqrt(v2), factor = a.eps * p + (1.0 - a.eps) * sdv;
    a.alpha[c] = factor * hv;
    if (a.detail) {
        double *o = a.detail + (size_t)c * BO_DETAIL;
        o[BO_D_MU0] = mu[0]; o[BO_D_MU1] = mu[1]; o[BO_D_D20] = d2[0]; o[BO_D_D21] = d2[1];
        o[BO_D_HVI] = hv; o[BO_D_P] = p; o[BO_D_SD] = sdv; o[BO_D_FACTOR] = factor;
    }
}

}  // namespace tum
