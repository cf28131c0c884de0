// gp_kernels.hpp -- K16: the marginal log-likelihood of one exact GP and its gradient (bo.fit_gp's objective; include/tum_nmpc.h states
// the mathematics), and the two things bo.pack_model needs of a fitted GP, V = L^-1 and a = A^-1 (y - c). All matrices are row-major
// with the leading dimension np = n padded to a multiple of GP_NB = 64; only the lower 64 x 64 tiles are written and read. One call is
// this chain, plain launches on one stream:
//   gp_kern_kernel      the lower tiles of A = K + diag(noise) from X; rows and columns behind n are the identity; r = y - c.
//   per block column k: gp_potrf_kernel  A_kk = L_kk L_kk^T in LDS in one workgroup, then L_kk^-1 (the diagonal tile of V) in the
//                                        free upper triangle; a pivot that is not positive and finite is replaced by 1 and recorded
//                       gp_trsm_kernel   L_ik = A_ik L_kk^-T for the tiles below                       (v_mfma_f64_16x16x4_f64)
//                       gp_syrk_kernel   A_ij -= L_ik L_jk^T for the lower tiles behind the column     (v_mfma_f64_16x16x4_f64)
//   gp_lhat_kernel      M_im = L_ii^-1 L_im for the tiles below the diagonal (into the buffer A^-1 takes later)
//   gp_trinv_kernel     V = L^-1 by block diagonals: stage s forms V_(j+s)j = -sum_{m = j .. j+s-1} M_(j+s)m V_mj, one product of K = 64 s
//   gp_ainv_kernel      the lower tiles of A^-1 = V^T V; the sum starts at the tile's block row: the zero tiles of V above are skipped
//   gp_w_kernel         w = V r, one wavefront per row
//   gp_alpha_kernel     the block-row partials of alpha = V^T w
//   gp_asum_kernel      alpha from them, in block-row order
//   gp_grad_kernel      per lower tile the d + 1 sums over W_ik K_ik [1, t_ikj^2], W = alpha alpha^T - A^-1, K recomputed from X
//   gp_reduce_kernel    one workgroup: the MLL, the gradient and the ok word
// The kernels are templates (of a parameter nobody sets) for one reason: the compiler emits a template's code behind all plain
// functions of the translation unit, in the order of first use. So these kernels land behind every older kernel of the library and
// move none of them: the interior point kernels are larger than the instruction cache and their speed depends on where they lie.
// Determinism: no floating-point atomics; every sum is one chain or one fixed tree whose order depends on n and d alone. Every tile a
// kernel reads was written by a kernel of the same call: nothing a larger, earlier problem left in the buffers is read.
#pragma once
#include "nmpc_device.hpp"

namespace tum {

constexpr int GP_NB = 64;              // block size of the factorisation: one diagonal block (padded rows) is 33 KB of LDS
constexpr int GP_LDS = GP_NB + 1;      // row stride of the block in LDS: a column's 64 rows lie in 64 different banks
constexpr int GP_MAXD = 16;
constexpr int GP_NG = GP_MAXD + 1;     // sums of gp_grad_kernel per tile: W K, W K t_j^2
constexpr double GP_DBL_MAX = 1.7976931348623157e308;

// acc[g] += A(16 rows x K) B(K x 16 columns of column tile g), g < NCT, K a multiple of 64. A points at (first row, k = 0), B at
// (k = 0, first column); T*: the operand is stored transposed (element (i, k) at [k][i]). The operands come straight from global
// memory (L2): the loads of the next CH k-steps are issued before the products of the current ones, so a wavefront waits for memory
// once per chunk and not once per k-step.
template <bool TA, bool TB, int NCT>
__device__ __forceinline__ void gp_mm(const double *A, const double *B, int ld, int K, d4 (&acc)[NCT])
{
    constexpr int CH = NCT == 1 ? 16 : 8;          // k-steps per chunk: 16 or 8 x (1 + NCT) doubles in flight, twice
    const int lane = threadIdx.x & 63, col = lane & 15, quad = lane >> 4;
    const double *pa = TA ? A + (size_t)quad * ld + col : A + (size_t)col * ld + quad;
    const double *pb = TB ? B + (size_t)col * ld + quad : B + (size_t)quad * ld + col;
    const size_t sa = TA ? (size_t)4 * ld : 4, sb = TB ? 4 : (size_t)4 * ld, cb = TB ? (size_t)16 * ld : 16;
    double a0[CH], b0[CH][NCT], a1[CH], b1[CH][NCT];
#pragma unroll
    for (int u = 0; u < CH; u++) {
        a0[u] = pa[u * sa];
#pragma unroll
        for (int g = 0; g < NCT; g++) b0[u][g] = pb[u * sb + g * cb];
    }
    for (int k = 4 * CH; k <= K; k += 4 * CH) {
        pa += CH * sa; pb += CH * sb;
        if (k < K) {
#pragma unroll
            for (int u = 0; u < CH; u++) {
                a1[u] = pa[u * sa];
#pragma unroll
                for (int g = 0; g < NCT; g++) b1[u][g] = pb[u * sb + g * cb];
            }
        }
#pragma unroll
        for (int u = 0; u < CH; u++)
#pragma unroll
            for (int g = 0; g < NCT; g++) acc[g] = mfma(a0[u], b0[u][g], acc[g]);
        if (k < K) {
#pragma unroll
            for (int u = 0; u < CH; u++) {
                a0[u] = a1[u];
#pragma unroll
                for (int g = 0; g < NCT; g++) b0[u][g] = b1[u][g];
            }
        }
    }
}

// the sum of v over the 256 threads of the workgroup in one fixed tree; every thread returns it. sh: 256 doubles.
__device__ __forceinline__ double gp_block_sum(double v, double *sh)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) sh[t] = sh[t] + sh[t + h];
        __syncthreads();
    }
    return sh[0];
}

struct GpKernArgs {
    int n, np, d, learn;
    const double *X, *y, *fixed;                // [n][d], [n], [n]
    double ils[GP_MAXD], s, c, floor, learned;  // 1 / ls_j; output scale; mean; noise floor; e^theta_noise
    double *A, *r;                              // [np][np], [np]
};

// grid (nb, nb), 256 threads; tile (i, j) = (blockIdx.y, blockIdx.x), j <= i. Thread: column tid & 63, rows (tid >> 6) + 4 e.
template <int = 0> __global__ void __launch_bounds__(256) gp_kern_kernel(const GpKernArgs a)
{
#pragma clang fp contract(off)
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int k = bj * GP_NB + (threadIdx.x & 63);
    for (int e = 0; e < 16; e++) {
        const int i = bi * GP_NB + (threadIdx.x >> 6) + 4 * e;
        double v = i == k ? 1.0 : 0.0;
        if (i < a.n && k < a.n) {
            const double *xi = a.X + (size_t)i * a.d, *xk = a.X + (size_t)k * a.d;
            double rr = 0.0;
            for (int j = 0; j < a.d; j++) {
                const double t = (xi[j] - xk[j]) * a.ils[j];
                rr = rr + t * t;
            }
            v = a.s * exp(-0.5 * rr);
            if (i == k) v = v + ((a.fixed[i] + a.floor) + (a.learn ? a.learned : 0.0));
        }
        a.A[(size_t)i * a.np + k] = v;
    }
    if (bi == bj && threadIdx.x < GP_NB) {
        const int i = bi * GP_NB + threadIdx.x;
        a.r[i] = i < a.n ? a.y[i] - a.c : 0.0;
    }
}

struct GpFacArgs {
    int n, np, k, s;                            // k: block column (potrf, trsm, syrk); s: block diagonal (trinv)
    double *A, *V, *M;                          // [np][np] each: A becomes L; V = L^-1; M = L_ii^-1 L_im, later A^-1
    double *minpiv; int *bad;                   // [nb] each
};

// grid 1, 256 threads: the diagonal block k; thread (row = tid & 63, grp = tid >> 6). Left-looking column Cholesky of the lower
// triangle in LDS: column j is A_ij - sum_{p < j} L_ip L_jp, the sum split over the four groups and added in group order. Then
// X = L_kk^-1 by forward substitution of L X = I, row by row, every column on its own: X_ij = -(sum_{m = j .. i-1} L_im X_mj) / L_ii.
// (L X = I and not X L = I: the panel L_ik = A_ik X^T and the blocks of V need a RIGHT inverse of L_kk, one with a small L X - I;
// the other recursion leaves a small X L - I, and that costs the likelihood several times the error of the right inverse.) X_mj (m > j)
// lives at S[j][m], in the upper triangle the factor leaves free.
template <int = 0> __global__ void __launch_bounds__(256) gp_potrf_kernel(const GpFacArgs a)
{
#pragma clang fp contract(off)
    __shared__ double S[GP_NB * GP_LDS];
    __shared__ double piv[GP_NB], dinv[GP_NB], comb[4 * GP_NB];
    __shared__ int badp[GP_NB];
    const int t = threadIdx.x, row = t & 63, grp = t >> 6, k0 = a.k * GP_NB;
    double *Ak = a.A + (size_t)k0 * a.np + k0, *Vk = a.V + (size_t)k0 * a.np + k0;
    for (int e = 0; e < 16; e++) {
        const int i = grp + 4 * e;                  // (global accesses: this thread's COLUMN is `row`, its rows are i)
        S[i * GP_LDS + row] = row <= i ? Ak[(size_t)i * a.np + row] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < GP_NB; j++) {
        // row `row` against row j over the finished columns p = grp, grp + 4, .. < j: no write to LDS in the loop, its reads pipeline
        double part = 0.0;
#pragma unroll 4
        for (int p = grp; p < j; p += 4) part = part + S[row * GP_LDS + p] * S[j * GP_LDS + p];
        comb[grp * GP_NB + row] = part;
        __syncthreads();
        if (grp == 0 && row >= j) {
            // every row forms the pivot itself (the same bits in every lane); the diagonal stays in piv until the loop is through
            double vj = S[j * GP_LDS + j] - (((comb[j] + comb[GP_NB + j]) + comb[2 * GP_NB + j]) + comb[3 * GP_NB + j]);
            const bool good = vj > 0.0 && vj <= GP_DBL_MAX;
            if (!good) vj = 1.0;
            const double l = sqrt(vj);
            if (row == j) { piv[j] = l; dinv[j] = 1.0 / l; badp[j] = good ? 0 : 1; }
            else {
                const double v = S[row * GP_LDS + j] - (((comb[row] + comb[GP_NB + row]) + comb[2 * GP_NB + row]) + comb[3 * GP_NB + row]);
                S[row * GP_LDS + j] = v / l;
            }
        }
        __syncthreads();
    }
    if (t < GP_NB) S[t * GP_LDS + t] = piv[t];
    __syncthreads();
    for (int e = 0; e < 16; e++) {
        const int i = grp + 4 * e;
        Ak[(size_t)i * a.np + row] = S[i * GP_LDS + row];          // (zero above the diagonal)
    }
    if (t == 0) {
        double mn = GP_DBL_MAX; int bad = 0;
        for (int j = 0; j < GP_NB; j++)
            if (k0 + j < a.n) { mn = piv[j] < mn ? piv[j] : mn; bad |= badp[j]; }
        a.minpiv[a.k] = mn; a.bad[a.k] = bad;
    }
    __syncthreads();                               // (the upper triangle is read back above before it is written below)
    // thread (column c = row, grp): rows i downwards; the share m = grp, grp + 4, .. < i of the sum, m >= c (a trip count the
    // wavefront shares); the four shares are added in group order
    const int c = row;
    const double dc = dinv[c];
    for (int i = 1; i < GP_NB; i++) {
        double part = 0.0;
#pragma unroll 4
        for (int m = grp; m < i; m += 4) {
            const int mm = m > c ? m : c;
            const double term = S[i * GP_LDS + m] * (m == c ? dc : S[c * GP_LDS + mm]);
            if (m >= c) part = part + term;
        }
        comb[grp * GP_NB + c] = part;
        __syncthreads();
        if (grp == 0 && c < i) {
            const double sum = ((comb[c] + comb[GP_NB + c]) + comb[2 * GP_NB + c]) + comb[3 * GP_NB + c];
            S[c * GP_LDS + i] = -(sum / piv[i]);
        }
        __syncthreads();
    }
    for (int e = 0; e < 16; e++) {
        const int i = grp + 4 * e;                  // V[i][row]
        Vk[(size_t)i * a.np + row] = row < i ? S[row * GP_LDS + i] : (row == i ? dinv[i] : 0.0);
    }
}

// the 16 x 64 strip of a wavefront, rows r0 + quad + 4 j of the accumulators, to C (or C - acc, or -acc)
enum { GP_ST_SET, GP_ST_SUB, GP_ST_NEG };
template <int MODE, int NCT>
__device__ __forceinline__ void gp_store(double *C, int ld, const d4 (&acc)[NCT])
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, col = lane & 15, quad = lane >> 4;
#pragma unroll
    for (int g = 0; g < NCT; g++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double *p = C + (size_t)(quad + 4 * j) * ld + 16 * g + col;
            *p = MODE == GP_ST_SET ? acc[g][j] : (MODE == GP_ST_SUB ? *p - acc[g][j] : -acc[g][j]);
        }
}

template <int NCT>
__device__ __forceinline__ void gp_zero(d4 (&acc)[NCT])
{
#pragma unroll
    for (int g = 0; g < NCT; g++) acc[g] = d4{0.0, 0.0, 0.0, 0.0};
}

// grid (tiles below the diagonal block k), 256 threads: wavefront w takes rows 16 w .. 16 w + 15 of the tile, in place (it reads
// its own 16 rows only, all of them before it writes)
template <int = 0> __global__ void __launch_bounds__(256) gp_trsm_kernel(const GpFacArgs a)
{
    const int i = a.k + 1 + blockIdx.x, w = threadIdx.x >> 6, k0 = a.k * GP_NB;
    double *Aik = a.A + (size_t)(i * GP_NB + 16 * w) * a.np + k0;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, true, 4>(Aik, a.V + (size_t)k0 * a.np + k0, a.np, GP_NB, acc);
    gp_store<GP_ST_SET>(Aik, a.np, acc);
}

// grid (m, m), m = nb - k - 1, 256 threads: tile (i, j) = k + 1 + (blockIdx.y, blockIdx.x), j <= i
template <int = 0> __global__ void __launch_bounds__(256) gp_syrk_kernel(const GpFacArgs a)
{
    if (blockIdx.x > blockIdx.y) return;
    const int i = a.k + 1 + blockIdx.y, j = a.k + 1 + blockIdx.x, w = threadIdx.x >> 6, k0 = a.k * GP_NB;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, true, 4>(a.A + (size_t)(i * GP_NB + 16 * w) * a.np + k0, a.A + (size_t)(j * GP_NB) * a.np + k0, a.np, GP_NB, acc);
    gp_store<GP_ST_SUB>(a.A + (size_t)(i * GP_NB + 16 * w) * a.np + j * GP_NB, a.np, acc);
}

// grid (nb, nb, 4), 64 threads: tile (i, m) = (blockIdx.y, blockIdx.x), m < i; blockIdx.z the 16-row strip. M_im = V_ii L_im.
template <int = 0> __global__ void __launch_bounds__(64) gp_lhat_kernel(const GpFacArgs a)
{
    if (blockIdx.x >= blockIdx.y) return;
    const int i = blockIdx.y, m = blockIdx.x, r0 = i * GP_NB + 16 * blockIdx.z;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<false, false, 4>(a.V + (size_t)r0 * a.np + i * GP_NB, a.A + (size_t)(i * GP_NB) * a.np + m * GP_NB, a.np, GP_NB, acc);
    gp_store<GP_ST_SET>(a.M + (size_t)r0 * a.np + m * GP_NB, a.np, acc);
}

// grid (nb - s, 4, 4), 64 threads: tile (j + s, j), j = blockIdx.x; one wavefront per 16 x 16 piece (blockIdx.y rows, blockIdx.z
// columns): the stages run one behind the other, so a stage is as short as its longest wavefront
template <int = 0> __global__ void __launch_bounds__(64) gp_trinv_kernel(const GpFacArgs a)
{
    const int j = blockIdx.x, i = j + a.s, r0 = i * GP_NB + 16 * blockIdx.y, c0 = j * GP_NB + 16 * blockIdx.z;
    d4 acc[1];
    gp_zero(acc);
    gp_mm<false, false, 1>(a.M + (size_t)r0 * a.np + j * GP_NB, a.V + (size_t)(j * GP_NB) * a.np + c0, a.np, GP_NB * a.s, acc);
    gp_store<GP_ST_NEG>(a.V + (size_t)r0 * a.np + c0, a.np, acc);
}

// grid (nb, nb), 256 threads: tile (i, j) = (blockIdx.y, blockIdx.x), j <= i, of M = V^T V: rows i 64 .. np - 1 of V
template <int = 0> __global__ void __launch_bounds__(256) gp_ainv_kernel(const GpFacArgs a)
{
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y, j = blockIdx.x, w = threadIdx.x >> 6;
    const double *Vi = a.V + (size_t)(i * GP_NB) * a.np;
    d4 acc[4];
    gp_zero(acc);
    gp_mm<true, false, 4>(Vi + i * GP_NB + 16 * w, Vi + j * GP_NB, a.np, a.np - i * GP_NB, acc);
    gp_store<GP_ST_SET>(a.M + (size_t)(i * GP_NB + 16 * w) * a.np + j * GP_NB, a.np, acc);
}

struct GpVecArgs {
    int n, np, nb, d, learn, want_grad;
    const double *V, *M, *L, *X, *r;
    double *w, *alpha, *apart, *gpart;          // [np], [np], [nb][np], [tiles][GP_NG]
    const double *minpiv; const int *bad;
    double ils[GP_MAXD], s, learned, thr;       // thr: the smallest pivot the host accepts, 1e-7 sqrt(s)
    double *out;                                // [d + 5]: MLL, the d + 3 gradient components, ok (1.0 / 0.0)
};

// grid (np / 4), 256 threads: wavefront per row i: lane l sums V_ik r_k over k = l, l + 64, .. <= i in order, then one butterfly
template <int = 0> __global__ void __launch_bounds__(256) gp_w_kernel(const GpVecArgs a)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const double *v = a.V + (size_t)i * a.np;
    double sum = 0.0;
    for (int k = lane; k <= i; k += 64) sum = sum + v[k] * a.r[k];
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) sum = sum + __shfl_xor(sum, h);
    if (lane == 0) a.w[i] = sum;
}

// grid (nb, nb), 64 threads: column j = 64 blockIdx.x + tid, block row blockIdx.y >= blockIdx.x: its 64 rows in order
template <int = 0> __global__ void __launch_bounds__(64) gp_alpha_kernel(const GpVecArgs a)
{
#pragma clang fp contract(off)
    if (blockIdx.x > blockIdx.y) return;
    const int j = blockIdx.x * GP_NB + threadIdx.x, i0 = blockIdx.y * GP_NB;
    double sum = 0.0;
    for (int i = i0; i < i0 + GP_NB; i++) sum = sum + (i >= j ? a.V[(size_t)i * a.np + j] : 0.0) * a.w[i];
    a.apart[(size_t)blockIdx.y * a.np + j] = sum;
}

// grid (nb), 64 threads
template <int = 0> __global__ void __launch_bounds__(64) gp_asum_kernel(const GpVecArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * GP_NB + threadIdx.x;
    double sum = 0.0;
    for (int b = blockIdx.x; b < a.nb; b++) sum = sum + a.apart[(size_t)b * a.np + j];
    a.alpha[j] = sum;
}

// grid (nb, nb), 256 threads: tile (i, j) = (blockIdx.y, blockIdx.x), j <= i; thread: column tid & 63, rows (tid >> 6) + 4 e. The
// tile's sums go to gpart[i (i + 1) / 2 + j]; a tile below the diagonal stands for its mirror image too: its sums are doubled.
template <int = 0> __global__ void __launch_bounds__(256) gp_grad_kernel(const GpVecArgs a)
{
#pragma clang fp contract(off)
    __shared__ double sh[256];
    if (blockIdx.x > blockIdx.y) return;
    const int bi = blockIdx.y, bj = blockIdx.x, k = bj * GP_NB + (threadIdx.x & 63);
    double acc[GP_NG];
#pragma unroll
    for (int j = 0; j < GP_NG; j++) acc[j] = 0.0;
    const double ak = a.alpha[k];
    for (int e = 0; e < 16; e++) {
        const int i = bi * GP_NB + (threadIdx.x >> 6) + 4 * e;
        if (i < a.n && k < a.n) {
            const double *xi = a.X + (size_t)i * a.d, *xk = a.X + (size_t)k * a.d;
            double t2[GP_MAXD], rr = 0.0;
#pragma unroll
            for (int j = 0; j < GP_MAXD; j++) {
                t2[j] = 0.0;
                if (j < a.d) {
                    const double t = (xi[j] - xk[j]) * a.ils[j];
                    t2[j] = t * t;
                    rr = rr + t2[j];
                }
            }
            const double wk = (a.alpha[i] * ak - a.M[(size_t)i * a.np + k]) * (a.s * exp(-0.5 * rr));
            acc[0] = acc[0] + wk;
#pragma unroll
            for (int j = 0; j < GP_MAXD; j++) acc[1 + j] = acc[1 + j] + wk * t2[j];
        }
    }
    const double twice = bi == bj ? 1.0 : 2.0;
    double *o = a.gpart + (size_t)(bi * (bi + 1) / 2 + bj) * GP_NG;
#pragma unroll
    for (int j = 0; j < GP_NG; j++) {
        const double sum = j <= a.d ? gp_block_sum(acc[j], sh) : 0.0;          // (uniform over the workgroup)
        if (threadIdx.x == 0) o[j] = twice * sum;
    }
}

// grid 1, 256 threads. Every sum: thread t takes the elements t, t + 256, .. in order, then the fixed tree of gp_block_sum.
template <int = 0> __global__ void __launch_bounds__(256) gp_reduce_kernel(const GpVecArgs a)
{
#pragma clang fp contract(off)
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double ww = 0.0, ll = 0.0, sa = 0.0, saa = 0.0, tr = 0.0;
    for (int i = t; i < a.n; i += 256) {
        ww = ww + a.w[i] * a.w[i];
        ll = ll + log(a.L[(size_t)i * a.np + i]);
        if (a.want_grad) {
            sa = sa + a.alpha[i];
            saa = saa + a.alpha[i] * a.alpha[i];
            tr = tr + a.M[(size_t)i * a.np + i];
        }
    }
    ww = gp_block_sum(ww, sh); ll = gp_block_sum(ll, sh);
    const double mll = (-0.5 * ww - ll) - 0.5 * (double)a.n * 1.8378770664093454836;          // log 2 pi
    double mn = GP_DBL_MAX; int bad = 0;
    for (int b = 0; b < a.nb; b++) { mn = a.minpiv[b] < mn ? a.minpiv[b] : mn; bad |= a.bad[b]; }
    const bool ok = !bad && mll >= -GP_DBL_MAX && mll <= GP_DBL_MAX && mn > a.thr;
    if (t == 0) { a.out[0] = mll; a.out[a.d + 4] = ok ? 1.0 : 0.0; }
    if (!a.want_grad) return;
    sa = gp_block_sum(sa, sh); saa = gp_block_sum(saa, sh); tr = gp_block_sum(tr, sh);
    const int tiles = a.nb * (a.nb + 1) / 2;
    for (int j = 0; j <= a.d; j++) {
        double g = 0.0;
        for (int i = t; i < tiles; i += 256) g = g + a.gpart[(size_t)i * GP_NG + j];
        g = gp_block_sum(g, sh);
        if (t == 0) a.out[1 + (j == 0 ? a.d : j - 1)] = 0.5 * g;          // W K -> d / d log s; W K t_j^2 -> d / d log ls_j
    }
    if (t == 0) {
        a.out[1 + a.d + 1] = sa;
        a.out[1 + a.d + 2] = a.learn ? 0.5 * a.learned * (saa - tr) : 0.0;
    }
}

}  // namespace tum
