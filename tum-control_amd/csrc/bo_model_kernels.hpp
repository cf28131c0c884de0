// bo_model_kernels.hpp -- K17: the parts of the acquisition MODEL that are built on the device (bo.prune_baseline, the baseline part of
// bo.pack_model and bo.build_fronts; include/tum_nmpc.h states the mathematics). Matrices are row-major with the leading dimension np = n padded to a multiple of GP_NB,
// as in gp_kernels.hpp, whose product (gp_mm) and blocked Cholesky these chains reuse.
// Chain P, per objective (tum_bom_prune):
//   bom_kern_kernel     K = k(Xt, Xt), every tile (the product behind it reads whole rows); zero behind the points
//   bom_h_kernel        H = K V^T on v_mfma_f64_16x16x4_f64; V is lower triangular: the sum over k ends with block column j of the tile
//   bom_sig_kernel      the lower tiles of K - H H^T + jitter I; the identity behind n. (Tile (i, j) and its mirror image are the same
//                       sums in the same order, so the symmetrised matrix IS its lower triangle; the factorisation reads nothing else.)
//   gp_potrf / gp_trsm / gp_syrk   its Cholesky factor L_p in place (gp.hpp's loop)
//   bom_mean_kernel     m = c + K a, one wavefront per row
//   bom_draw_kernel     F[s][j][o] = m_j + sum_{k <= j} Z[s][k] L_p[j][k], again without the zero tiles
// and once:
//   bom_dom_kernel      one workgroup per sample, its n x 2 draws in LDS: trial i is kept where no j is >= in both objectives and > in
//                       one. The samples are combined by storing a 1: an OR of integers, which has no order.
// Fronts (tum_bom_fronts):
//   bom_front_kernel    one workgroup per sample: bo.front_2d of its n_b <= 512 draws without a sort -- a point is on the front where
//                       no point that the sort (objective 0 descending, then objective 1 descending, then index) puts before it
//                       has an objective 1 at least as large; its row is the number of front points with a smaller objective 0.
// Chain B, per objective (tum_bom_build): the same kernels on K(Xb, Xt) and K(Xb, Xb) -- the leading dimension and the length of the
// products are arguments --, the Cholesky, gp_lhat / gp_trinv for R = L_b^-1, the mean, the draws; then bom_front_kernel and
//   bom_pack_kernel     H, R and Z from their dense form into the A-operand layouts bo_cross_kernel, bo_tri_kernel and bo_hvi_kernel read
// Chain A (tum_bom_append), after the evaluation chain of bo_kernels.hpp has run on the one point:
//   bom_append_kernel   row n_b of the dense H (q), L_b (l, lam) and R (-(l R) / lam, 1 / lam), mu_b, the point into Xb; lam = sqrt(d2)
//   bom_appdraw_kernel  column n_b of F_b: (mu + Z l) + lam zeta, zeta the next column of the resident Zfull
// then bom_pack_kernel on H, R, Z and bom_front_kernel again.
// Every kernel is a template of a parameter nobody sets, for the reason gp_kernels.hpp gives. No floating-point atomics; the order of
// every sum depends on the sizes alone; every tile that is read was written by a kernel of the same call (or uploaded by it).
#pragma once
#include "bo_kernels.hpp"
#include "gp_kernels.hpp"

namespace tum {

constexpr int BOM_MAXB = 512;          // points of one sample's front (BO_MAXB)

struct BomKernArgs {
    int nr, nc, ld, d;                          // rows (points of Xr), columns (points of Xc), the leading dimension
    const double *Xr, *Xc;                      // [nr][d], [nc][d]
    double ils[GP_MAXD], s;
    double *K;                                  // [nr padded][ld]
};

// grid (column blocks, row blocks), 256 threads; tile (i, j) = (blockIdx.y, blockIdx.x). Thread: column tid & 63, rows (tid >> 6) + 4 e.
template <int = 0> __global__ void __launch_bounds__(256) bom_kern_kernel(const BomKernArgs a)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * GP_NB + (threadIdx.x & 63);
    for (int e = 0; e < 16; e++) {
        const int i = blockIdx.y * GP_NB + (threadIdx.x >> 6) + 4 * e;
        double v = 0.0;
        if (i < a.nr && k < a.nc) {
            const double *xi = a.Xr + (size_t)i * a.d, *xk = a.Xc + (size_t)k * a.d;
            double rr = 0.0;
            for (int j = 0; j < a.d; j++) {
                const double t = (xi[j] - xk[j]) * a.ils[j];
                rr = rr + t * t;
            }
            v = a.s * exp(-0.5 * rr);
        }
        a.K[(size_t)i * a.ld + k] = v;
    }
}

struct BomMatArgs {
    int n, np, ld;                              // points of the covariance, padded; leading dimension of Kx, V and H (a multiple of GP_NB)
    const double *Kx, *V;                       // [..][ld]: the kernel matrix against the trials; L^-1 of the GP, zero right of the diagonal
    const double *K;                            // [np][np]: the kernel matrix of the points themselves
    double *H, *A;                              // [..][ld]: Kx V^T; [np][np]: the posterior covariance, later its factor
    double jitter;
};

// grid (ld / 64, row blocks), 256 threads: tile (i, j) = (blockIdx.y, blockIdx.x) of H; wavefront w its rows 16 w .. 16 w + 15
template <int = 0> __global__ void __launch_bounds__(256) bom_h_kernel(const BomMatArgs a)
{
    const int i = blockIdx.y, j = blockIdx.x, w = threadIdx.x >> 6;
    const size_t r0 = (size_t)i * GP_NB + 16 * w;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, true, 4>(a.Kx + r0 * a.ld, a.V + (size_t)(j * GP_NB) * a.ld, a.ld, GP_NB * (j + 1), acc);
    gp_store<GP_ST_SET>(a.H + r0 * a.ld + j * GP_NB, a.ld, acc);
}

// grid (np / 64, np / 64), 256 threads: tile (i, j) = (blockIdx.y, blockIdx.x), j <= i
template <int = 0> __global__ void __launch_bounds__(256) bom_sig_kernel(const BomMatArgs a)
{
#pragma clang fp contract(off)
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y, j = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, quad = lane >> 4;
    const int r0 = i * GP_NB + 16 * w;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, true, 4>(a.H + (size_t)r0 * a.ld, a.H + (size_t)(j * GP_NB) * a.ld, a.ld, a.ld, acc);
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int r = r0 + quad + 4 * e, c = j * GP_NB + 16 * g + col;
            const size_t at = (size_t)r * a.np + c;
            double v = (r < a.n && c < a.n) ? a.K[at] - acc[g][e] : 0.0;
            if (r == c) v = r < a.n ? v + a.jitter : 1.0;
            a.A[at] = v;
        }
}

struct BomDrawArgs {
    int n, np, S, o, ldk, ldf;                  // points, leading dimension of L and Z; samples; objective; leading dimension (and row length) of Kx; rows of a sample in F
    const double *Kx, *a;                       // [np][ldk]; [ldk] zero behind the trials
    const double *L, *Z;                        // the factor [np][np]; [S padded to 16][np], zero where padded
    double c;
    double *m, *F;                              // [np]; [S][ldf][2]
};

// grid (np / 4), 256 threads: one wavefront per row i: lane l sums K_ik a_k over k = l, l + 64, .. in order, then one butterfly
template <int = 0> __global__ void __launch_bounds__(256) bom_mean_kernel(const BomDrawArgs a)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const double *k = a.Kx + (size_t)i * a.ldk;
    double sum = 0.0;
    for (int p = lane; p < a.ldk; p += 64) sum = sum + k[p] * a.a[p];
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) sum = sum + __shfl_xor(sum, h);
    if (lane == 0) a.m[i] = a.c + sum;
}

// grid (nb, S padded / 16), 64 threads: samples 16 blockIdx.y .. + 15 against the trials of block blockIdx.x
template <int = 0> __global__ void __launch_bounds__(64) bom_draw_kernel(const BomDrawArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x, lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, true, 4>(a.Z + (size_t)(16 * blockIdx.y) * a.np, a.L + (size_t)(j * GP_NB) * a.np, a.np, GP_NB * (j + 1), acc);
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int s = 16 * blockIdx.y + quad + 4 * e, t = j * GP_NB + 16 * g + col;
            if (s < a.S && t < a.n) a.F[((size_t)s * a.ldf + t) * 2 + a.o] = a.m[t] + acc[g][e];
        }
}

struct BomDomArgs {
    int n;
    const double *F;                            // [S][n][2]
    int *keep;                                  // [n], zero before the launch
};

// grid (S), 256 threads, 16 n bytes of dynamic LDS: thread t judges the trials t, t + 256, ..
template <int = 0> __global__ void __launch_bounds__(256) bom_dom_kernel(const BomDomArgs a)
{
    extern __shared__ double bom_f[];
    const double *F = a.F + (size_t)blockIdx.x * a.n * 2;
    for (int p = threadIdx.x; p < 2 * a.n; p += 256) bom_f[p] = F[p];
    __syncthreads();
    for (int i = threadIdx.x; i < a.n; i += 256) {
        const double f0 = bom_f[2 * i], f1 = bom_f[2 * i + 1];
        bool dominated = false;
        for (int j = 0; j < a.n; j++) {
            const double g0 = bom_f[2 * j], g1 = bom_f[2 * j + 1];
            dominated |= (g0 >= f0) & (g1 >= f1) & ((g0 > f0) | (g1 > f1));
        }
        if (!dominated) a.keep[i] = 1;
    }
}

struct BomFrontArgs {
    int nb, ldf;                                // points; rows of a sample in F and in fronts (>= nb)
    const double *F;                            // [S][nb][2]
    double ref[2];
    double *fronts; int *count;                 // [S][nb][2] ascending in objective 0, zero rows behind the count; [S]
};

// grid (S), 256 threads: thread t judges the points t and t + 256
template <int = 0> __global__ void __launch_bounds__(256) bom_front_kernel(const BomFrontArgs a)
{
    __shared__ double f[2 * BOM_MAXB];
    __shared__ int on[BOM_MAXB];
    __shared__ int total;
    const int nb = a.nb;
    const double *F = a.F + (size_t)blockIdx.x * a.ldf * 2;
    double *out = a.fronts + (size_t)blockIdx.x * a.ldf * 2;
    for (int p = threadIdx.x; p < 2 * nb; p += 256) f[p] = F[p];
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const double f0 = f[2 * i], f1 = f[2 * i + 1];
        bool keep = f0 > a.ref[0] && f1 > a.ref[1];
        for (int j = 0; j < nb; j++) {
            const double g0 = f[2 * j], g1 = f[2 * j + 1];
            const bool valid = g0 > a.ref[0] && g1 > a.ref[1];
            const bool before = g0 > f0 || (g0 == f0 && (g1 > f1 || (g1 == f1 && j < i)));
            if (valid && before && g1 >= f1) keep = false;
        }
        on[i] = keep ? 1 : 0;
        if (keep) atomicAdd(&total, 1);          // (an integer count: it has no order)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        if (on[i]) {
            int rank = 0;          // (front points have distinct objective 0: the ranks are unique and below `total`, the rows zeroed below lie behind them)
            for (int j = 0; j < nb; j++) rank += (on[j] && f[2 * j] < f[2 * i]) ? 1 : 0;
            out[2 * rank] = f[2 * i]; out[2 * rank + 1] = f[2 * i + 1];
        }
        if (i >= total) { out[2 * i] = 0.0; out[2 * i + 1] = 0.0; }
    }
    if (threadIdx.x == 0) a.count[blockIdx.x] = total;
}

struct BomAppendArgs {
    int n, nt, ntp, ldb, ntb, S, ncol, ldf, d;  // baseline points before the append; trials, padded to 64; leading dimension of L_b, R; row tiles of l; samples; columns of Zfull; rows of a sample in F
    const double *q[2], *l[2], *llpart[2];      // the evaluation chain's column 0 of its first column tile: [i][16] each
    const double *mom, *x;                      // [BO_GP][cp][2] with cp in `cp`; the point [d]
    int cp;
    double s[2], jitter[2];
    double *H[2], *L[2], *R[2], *mu[2];         // dense: [..][ntp], [..][ldb], [..][ldb], [..]
    const double *Zf[2];                        // [S][ncol]
    double *F, *Xb;                             // [S][ldf][2]; [..][d]
    int *ok;                                    // [2]
};

// grid (2), 256 threads: objective blockIdx.x. Row n of H is q, of L_b (l, lam), of R (-(l R) / lam, 1 / lam), lam = sqrt(d2) with
// bo_d2's own d2; every sum in index order, one thread per column
template <int = 0> __global__ void __launch_bounds__(256) bom_append_kernel(const BomAppendArgs a)
{
#pragma clang fp contract(off)
    const int o = blockIdx.x, n = a.n;
    const double *m = a.mom + ((size_t)o * a.cp) * 2;
    const double lam = sqrt(bo_d2(a.s[o], m[1], a.llpart[o], a.ntb, a.jitter[o]));
    for (int k = threadIdx.x; k < a.ntp; k += 256) a.H[o][(size_t)n * a.ntp + k] = k < a.nt ? a.q[o][(size_t)k * 16] : 0.0;
    for (int k = threadIdx.x; k < a.ldb; k += 256) {
        a.L[o][(size_t)n * a.ldb + k] = k < n ? a.l[o][(size_t)k * 16] : (k == n ? lam : 0.0);
        double r = 0.0;
        if (k < n) {
            double sum = 0.0;
            for (int i = k; i < n; i++) sum = sum + a.l[o][(size_t)i * 16] * a.R[o][(size_t)i * a.ldb + k];
            r = -(sum / lam);
        } else if (k == n) r = 1.0 / lam;
        a.R[o][(size_t)n * a.ldb + k] = r;
    }
    if (threadIdx.x == 0) {
        a.mu[o][n] = m[0];
        a.ok[o] = (lam > 0.0 && lam <= GP_DBL_MAX) ? 1 : 0;
    }
    if (o == 0 && threadIdx.x < a.d) a.Xb[(size_t)n * a.d + threadIdx.x] = a.x[threadIdx.x];
}

// grid (ceil(S / 256), 2), 256 threads: the new baseline draw of sample s: (mu + Z[s] . l) + lam zeta[s], zeta the column n of Zfull
template <int = 0> __global__ void __launch_bounds__(256) bom_appdraw_kernel(const BomAppendArgs a)
{
#pragma clang fp contract(off)
    const int o = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, n = a.n;
    if (s >= a.S) return;
    const double *m = a.mom + ((size_t)o * a.cp) * 2;
    const double lam = sqrt(bo_d2(a.s[o], m[1], a.llpart[o], a.ntb, a.jitter[o]));
    const double *z = a.Zf[o] + (size_t)s * a.ncol;
    double sum = 0.0;
    for (int k = 0; k < n; k++) sum = sum + z[k] * a.l[o][(size_t)k * 16];
    a.F[((size_t)s * a.ldf + n) * 2 + o] = (m[0] + sum) + lam * z[n];
}

struct BomPackArgs {
    int rows, cols, ld, tri;                    // tri: the lower triangle only, in bo_tri_kernel's layout
    const double *M;                            // [rows padded to 64][ld]
    double *out;
};

// grid (blocks of a row tile, row tiles of 16), 64 threads: block (t, q) of the A-operand layouts of bo_kernels.hpp -- lane holds
// M[16 t + (lane & 15)][4 q + (lane >> 4)], zero outside rows x cols (tri: and right of the diagonal; a tile t has 4 (t + 1) blocks)
template <int = 0> __global__ void __launch_bounds__(64) bom_pack_kernel(const BomPackArgs a)
{
    const int t = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
    if (a.tri && q >= 4 * (t + 1)) return;
    const int r = 16 * t + (lane & 15), k = 4 * q + (lane >> 4);
    const bool in = r < a.rows && k < a.cols && (!a.tri || k <= r);
    const size_t blk = a.tri ? bo_tri_off(t) + q : (size_t)t * gridDim.x + q;
    a.out[blk * 64 + lane] = in ? a.M[(size_t)r * a.ld + k] : 0.0;
}

}  // namespace tum
