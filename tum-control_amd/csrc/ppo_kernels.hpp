// ppo_kernels.hpp -- K14: the PPO update on the nets that policy_kernel / policy_ac_kernel act with (stable_baselines3 PPO.train as
// Learning_To_Adapt/SafeRL_WMPC/rl_training.py:133-155 configures it: normalize_advantage, no clip_range_vf, no target_kl, separate
// tanh nets for policy and value). One minibatch is this chain on the capsule's stream:
//   ppo_stats_kernel   mean and std (n - 1 divisor) of the minibatch's advantages.
//   ppo_tile_kernel    one workgroup per tile of 16 minibatch rows, gathered through the index list: both nets forward through
//                      policy_layers (the sums of policy_ac_kernel, to the bit), the hidden activations kept in memory; the per-row
//                      loss terms and diagnostics, dL/dz and dL/dV; then the deltas backwards, delta_{l-1} = (W_l^T delta_l) (1 - h^2)
//                      on v_mfma_f64_16x16x4_f64 with a second, transposed packing of every matrix. Activations and deltas of every
//                      layer go to memory as [row][width]: at [128, 256, 128] they do not fit LDS beside the two ping-pong buffers.
//   ppo_wgrad_kernel   dW_l = sum_rows delta_l h_{l-1}^T and db_l = sum_rows delta_l: one wavefront per 16 x 16 tile of a gradient,
//                      the minibatch rows in index order, 4 per product, one dependent chain. Rows behind the end of the minibatch
//                      carry delta = 0 exactly.
//   ppo_norm_kernel    partial sums of g^2 over fixed slices of the flat gradient, and (one more workgroup) the means of the loss terms.
//   ppo_adam_kernel    the gradient norm from the partial sums, the clip, Adam in FP64 on FP64 moments, the parameter rounded ONCE to
//                      float32, written to the float32 master and -- as that float32 value -- into the packed matrices policy_kernel and
//                      policy_ac_kernel read and into the transposed ones.
// Determinism: no floating-point atomics anywhere; every sum is a strided per-thread chain and a fixed tree, or one chain of products,
// whose order is a function of the minibatch size and the widths alone.
#pragma once
#include "collect_kernels.hpp"

namespace tum {

// what one minibatch reports (include/tum_nmpc.h: TUM_PPO_*)
enum { PPO_LOSS, PPO_POLICY_LOSS, PPO_VALUE_LOSS, PPO_ENTROPY_LOSS, PPO_APPROX_KL, PPO_CLIP_FRACTION, PPO_GRAD_NORM, PPO_N, PPO_STATS };
// per-row record of ppo_tile_kernel: -min(A r, A clip r), entropy, squared value error, (r - 1) - log r, clipped flag, log_prob, value
enum { PPO_R_POLICY, PPO_R_ENTROPY, PPO_R_VALUE, PPO_R_KL, PPO_R_CLIPPED, PPO_R_LOGP, PPO_R_V, PPO_R_PAD, PPO_ROW };
constexpr int PPO_RED = 256;           // threads of the reduction kernels
constexpr int PPO_SLICE = 2048;        // gradient entries per partial sum of the norm

// the training view of one net beside its PolicyArgs. The flat parameter vector is torch's: W_0 (out x in, row-major), b_0, W_1, ...
struct PpoNet {
    int n_mat;
    int in[POL_MAXMAT], out[POL_MAXMAT];          // true widths of matrix l
    int kp[POL_MAXMAT], mp[POL_MAXMAT];           // as PolicyArgs
    int hs[POL_MAXMAT];                           // row stride of h[l]: in[l] padded to a multiple of 16 (mp[l - 1] for l > 0)
    int kt[POL_MAXMAT];                           // K of the transposed product: out[l] padded to a multiple of 4
    int off[POL_MAXMAT];                          // W_l in the flat vector; b_l follows at off[l] + out[l] * in[l]
    double *W[POL_MAXMAT], *b[POL_MAXMAT];        // the packed matrices of PolicyArgs, writable
    double *WT[POL_MAXMAT];                       // [hs / 16][kt / 4][64]: lane holds W[4 q + (lane >> 4)][16 t + (lane & 15)]; l >= 1
    double *h[POL_MAXMAT], *d[POL_MAXMAT];        // [rows][hs[l]]: the input of matrix l; [rows][mp[l]]: dL/d(output of matrix l)
};

// a fixed tree over PPO_RED values in LDS; the result in red[0]
__device__ __forceinline__ double ppo_tree(double *red, double v, int tid)
{
    red[tid] = v;
    __syncthreads();
    for (int w = PPO_RED / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

struct PpoStatsArgs {
    int n, normalize;
    const int *idx;              // [n] rows of the buffer, null: 0 .. n - 1
    const double *adv;
    double *out;                 // [2]: mean, std + 1e-8 (0, 1 where the advantages are taken as they are)
};

__global__ void __launch_bounds__(PPO_RED) ppo_stats_kernel(const PpoStatsArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[PPO_RED];
    const int tid = threadIdx.x;
    if (!a.normalize || a.n < 2) {
        if (tid == 0) { a.out[0] = 0.0; a.out[1] = 1.0; }
        return;
    }
    double s = 0.0;
    for (int i = tid; i < a.n; i += PPO_RED) s = s + a.adv[a.idx ? a.idx[i] : i];
    const double mean = ppo_tree(red, s, tid) / (double)a.n;
    double q = 0.0;
    for (int i = tid; i < a.n; i += PPO_RED) {
        const double e = a.adv[a.idx ? a.idx[i] : i] - mean;
        q = q + e * e;
    }
    const double var = ppo_tree(red, q, tid) / (double)(a.n - 1);
    if (tid == 0) { a.out[0] = mean; a.out[1] = sqrt(var) + 1e-8; }
}

struct PpoTileArgs {
    PolicyArgs pi, vf;           // n = the minibatch's rows, obs / obs_stride = the buffer's observations
    PpoNet tp, tv;
    int rows;                    // rows of one LDS buffer: the larger of the two nets'
    const int *idx;              // [n] rows of the buffer, null: 0 .. n - 1
    const double *act, *old_logp, *adv, *ret;          // the buffer's columns (actions as doubles, as tum_sim_env_collect leaves them)
    const double *advstat;       // ppo_stats_kernel's
    double clip, ent_coef, vf_coef;
    double *rowrec;              // [rows of the tiles][PPO_ROW]
};

// The observation of a tile, rounded to float32 as policy_load_obs rounds it, into an LDS buffer and as h[0] into memory (zero up to hs)
__device__ __forceinline__ void ppo_load_obs(const PolicyArgs &a, const int *idx, double *dst, double *h0, int hs, int i0, int tid)
{
    for (int i = tid; i < hs * POL_TILE; i += 64 * POL_WAVES) {
        const int inst = i / hs, k = i - inst * hs;
        double v = 0.0;
        if (i0 + inst < a.n && k < a.n_in) {
            const size_t row = idx ? idx[i0 + inst] : i0 + inst;
            v = (double)(float)a.obs[row * a.obs_stride + k];
        }
        if (k < a.kp[0]) dst[k * POL_TILE + inst] = v;
        h0[(size_t)(i0 + inst) * hs + k] = v;
    }
}

// The deltas of one net backwards. In: dL/d(output of the last matrix) of the tile in buf[cur] as [mp][16], zero in the padded rows.
// Every delta goes to memory as [row][mp[l]]; delta_{l-1} = (W_l^T delta_l) (1 - h_l^2), h_l the kept input of matrix l.
__device__ __forceinline__ void ppo_backward(const PolicyArgs &a, const PpoNet &t, double *const *buf, int cur, int i0, int tid)
{
    const int lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
    for (int l = a.n_mat - 1; l >= 0; l--) {
        const double *src = buf[cur];
        double *dst = buf[cur ^ 1];
        const int mp = a.mp[l];
        for (int i = tid; i < mp * POL_TILE; i += 64 * POL_WAVES) {
            const int inst = i / mp, r = i - inst * mp;
            t.d[l][(size_t)(i0 + inst) * mp + r] = src[r * POL_TILE + inst];
        }
        if (l == 0) break;
        const int nt = t.hs[l] >> 4, nq = t.kt[l] >> 2;
        for (int tt = wave; tt < nt; tt += POL_WAVES) {
            const double *Wt = t.WT[l] + (size_t)tt * nq * 64 + lane, *x = src + quad * POL_TILE + col;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < nq; q++) acc = mfma(Wt[(size_t)q * 64], x[q * 4 * POL_TILE], acc);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = 16 * tt + quad + 4 * j;
                const double hv = t.h[l][(size_t)(i0 + col) * t.hs[l] + k];
                dst[k * POL_TILE + col] = acc[j] * (1.0 - hv * hv);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64 * POL_WAVES) ppo_tile_kernel(const PpoTileArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double pol_lds[];          // [2][rows][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * POL_TILE, n = a.pi.n;
    double *buf[2] = {pol_lds, pol_lds + (size_t)a.rows * POL_TILE};
    const bool mine = tid < POL_TILE && i0 + tid < n;
    const size_t row = mine ? (a.idx ? a.idx[i0 + tid] : i0 + tid) : 0;
    double *rec = a.rowrec + (size_t)(i0 + tid) * PPO_ROW;          // (tid < POL_TILE)

    // ---- the value net: forward, dL/dV = vf_coef 2 (V - ret) / n, backward
    ppo_load_obs(a.vf, a.idx, buf[0], a.tv.h[0], a.tv.hs[0], i0, tid);
    __syncthreads();
    policy_layers<true>(a.vf, buf, lane, wave, a.tv.h, i0);
    {
        double *z = buf[a.vf.n_mat & 1];
        if (tid < POL_TILE) {
            const double v = z[tid];          // row 0 of the one-row last matrix
            double dv = 0.0, sq = 0.0;
            if (mine) {
                const double e = v - a.ret[row];
                sq = e * e;
                dv = a.vf_coef * (2.0 * e) / (double)n;
            }
            rec[PPO_R_VALUE] = sq; rec[PPO_R_V] = mine ? v : 0.0;
            for (int j = 0; j < a.vf.mp[a.vf.n_mat - 1]; j++) z[j * POL_TILE + tid] = j == 0 ? dv : 0.0;
        }
        __syncthreads();
    }
    ppo_backward(a.vf, a.tv, buf, a.vf.n_mat & 1, i0, tid);

    // ---- the policy net: forward, the row's loss terms and dL/dz, backward
    ppo_load_obs(a.pi, a.idx, buf[0], a.tp.h[0], a.tp.hs[0], i0, tid);
    __syncthreads();
    policy_layers<true>(a.pi, buf, lane, wave, a.tp.h, i0);
    if (tid < POL_TILE) {
        double *z = buf[a.pi.n_mat & 1] + tid;
        const int A = a.pi.n_act, mpl = a.pi.mp[a.pi.n_mat - 1];
        double pol = 0.0, H = 0.0, kl = 0.0, clipped = 0.0, lp = 0.0;
        if (mine) {
            // m, S and log_prob exactly as policy_sample computes them
            double m = z[0];
            for (int j = 1; j < A; j++) {
                const double v = z[j * POL_TILE];
                if (v > m) m = v;
            }
            double S = 0.0;
            for (int j = 0; j < A; j++) S = S + exp(z[j * POL_TILE] - m);
            const double logS = log(S);
            const int act = (int)a.act[row];
            lp = (z[act * POL_TILE] - m) - logS;
            for (int j = 0; j < A; j++) {
                const double lj = (z[j * POL_TILE] - m) - logS;
                H = H - exp(lj) * lj;
            }
            const double Ad = (a.adv[row] - a.advstat[0]) / a.advstat[1];
            const double lr = lp - a.old_logp[row], r = exp(lr);
            const double rc = r < 1.0 - a.clip ? 1.0 - a.clip : (r > 1.0 + a.clip ? 1.0 + a.clip : r);
            const double s1 = Ad * r, s2 = Ad * rc;
            pol = -(s1 <= s2 ? s1 : s2);
            kl = (r - 1.0) - lr;
            clipped = fabs(r - 1.0) > a.clip ? 1.0 : 0.0;
            // d(-min)/d log_prob: the unclipped term carries the gradient where it is the smaller one (or both are equal)
            const double glp = s1 <= s2 ? -s1 : 0.0;
            for (int j = 0; j < A; j++) {
                const double lj = (z[j * POL_TILE] - m) - logS, pj = exp(lj);
                const double g = glp * ((j == act ? 1.0 : 0.0) - pj) + a.ent_coef * (pj * (lj + H));
                z[j * POL_TILE] = g / (double)n;
            }
            for (int j = A; j < mpl; j++) z[j * POL_TILE] = 0.0;
        } else {
            for (int j = 0; j < mpl; j++) z[j * POL_TILE] = 0.0;
        }
        rec[PPO_R_POLICY] = pol; rec[PPO_R_ENTROPY] = H; rec[PPO_R_KL] = kl; rec[PPO_R_CLIPPED] = clipped; rec[PPO_R_LOGP] = lp;
        rec[PPO_R_PAD] = 0.0;
    }
    __syncthreads();
    ppo_backward(a.pi, a.tp, buf, a.pi.n_mat & 1, i0, tid);
}

struct PpoGradArgs {
    PpoNet net[2];                                // policy, value
    int first[2 * POL_MAXMAT + 1];                // first workgroup of matrix (net, l) at [net * POL_MAXMAT + l]; the total behind the last
    int rows;                                     // minibatch rows padded to whole tiles
    double *G;                                    // the flat gradient, policy net then value net
    int goff[2];                                  // where each net begins in it
};

// One wavefront per 16 x 16 tile of dW_l (tile column u < hs / 16) or the 16 entries of db_l (u == hs / 16): A = delta_l^T, B = h_l or
// ones, K the minibatch rows in index order
__global__ void __launch_bounds__(64) ppo_wgrad_kernel(const PpoGradArgs a)
{
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    int m = 0;
    while (m + 1 < 2 * POL_MAXMAT && (int)blockIdx.x >= a.first[m + 1]) m++;
    const int ni = m / POL_MAXMAT, l = m - ni * POL_MAXMAT;
    const PpoNet &t = a.net[ni];
    const int nu = t.hs[l] >> 4, id = blockIdx.x - a.first[m], tt = id / (nu + 1), u = id - tt * (nu + 1);
    const int mp = t.mp[l], hs = t.hs[l], nq = a.rows >> 2;
    const bool bias = u == nu;
    const double *dp = t.d[l] + (size_t)quad * mp + 16 * tt + col, *hp = t.h[l] + (size_t)quad * hs + (bias ? 0 : 16 * u + col);
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    // one dependent chain in q; the operands of four products are loaded before the first is issued (rows is a multiple of 16)
    for (int q = 0; q < nq; q += 4) {
        double x[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[i] = dp[(size_t)(q + i) * 4 * mp];
            y[i] = bias ? 1.0 : hp[(size_t)(q + i) * 4 * hs];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) acc = mfma(x[i], y[i], acc);
    }
    double *g = a.G + a.goff[ni] + t.off[l];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = 16 * tt + quad + 4 * j, k = 16 * u + col;
        if (r >= t.out[l]) continue;
        if (bias) { if (col == 0) g[(size_t)t.out[l] * t.in[l] + r] = acc[j]; }
        else if (k < t.in[l]) g[(size_t)r * t.in[l] + k] = acc[j];
    }
}

struct PpoNormArgs {
    int P, n_parts, n;                 // parameters, slices of PPO_SLICE of them, minibatch rows
    const double *G, *rowrec;
    double ent_coef, vf_coef;
    double *parts, *stats;             // [n_parts], [PPO_STATS]
};

__global__ void __launch_bounds__(PPO_RED) ppo_norm_kernel(const PpoNormArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[PPO_RED];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < a.n_parts) {
        const int base = blockIdx.x * PPO_SLICE;
        double s = 0.0;
        for (int i = tid; i < PPO_SLICE && base + i < a.P; i += PPO_RED) s = s + a.G[base + i] * a.G[base + i];
        s = ppo_tree(red, s, tid);
        if (tid == 0) a.parts[blockIdx.x] = s;
        return;
    }
    // the last workgroup: the means of the loss terms over the minibatch's rows
    // (the first five fields of a row record, in the record's order)
    double mean[5];
#pragma unroll
    for (int f = 0; f < 5; f++) {
        double s = 0.0;
        for (int i = tid; i < a.n; i += PPO_RED) s = s + a.rowrec[(size_t)i * PPO_ROW + f];
        mean[f] = ppo_tree(red, s, tid) / (double)a.n;
    }
    if (tid == 0) {
        const double pl = mean[PPO_R_POLICY], el = -mean[PPO_R_ENTROPY], vl = mean[PPO_R_VALUE];
        a.stats[PPO_POLICY_LOSS] = pl; a.stats[PPO_ENTROPY_LOSS] = el; a.stats[PPO_VALUE_LOSS] = vl;
        a.stats[PPO_LOSS] = (pl + a.ent_coef * el) + a.vf_coef * vl;
        a.stats[PPO_APPROX_KL] = mean[PPO_R_KL]; a.stats[PPO_CLIP_FRACTION] = mean[PPO_R_CLIPPED];
        a.stats[PPO_N] = (double)a.n;
    }
}

struct PpoAdamArgs {
    PpoNet net[2];
    int goff[2], P, n_parts, mode;     // mode 0: the norm alone; 1: clip and Adam; 2: the float32 master and the transposes from the packed nets
    const double *G, *parts;
    double max_grad_norm, step, bc2_sqrt, beta1, beta2, eps;          // step = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
    float *theta;                      // [P] the float32 master
    double *m, *v;                     // [P] Adam's moments
    double *stats;
};

__global__ void __launch_bounds__(PPO_RED) ppo_adam_kernel(const PpoAdamArgs a)
{
#pragma clang fp contract(off)
    __shared__ double coef_s;
    const int tid = threadIdx.x, p = blockIdx.x * PPO_RED + tid;
    if (a.mode != 2) {
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < a.n_parts; i++) s = s + a.parts[i];
            const double total = sqrt(s), c = a.max_grad_norm / (total + 1e-6);
            coef_s = c < 1.0 ? c : 1.0;
            if (blockIdx.x == 0) a.stats[PPO_GRAD_NORM] = total;
        }
        __syncthreads();
        if (a.mode == 0) return;
    }
    if (p >= a.P) return;
    // where parameter p lives: net, matrix, weight (r, k) or bias r
    const int ni = p >= a.goff[1] ? 1 : 0;
    const PpoNet &t = a.net[ni];
    const int q = p - a.goff[ni];
    int l = 0;
    while (l + 1 < t.n_mat && q >= t.off[l + 1]) l++;
    const int e = q - t.off[l], in = t.in[l], nw = t.out[l] * in;
    const bool bias = e >= nw;
    const int r = bias ? e - nw : e / in, k = bias ? 0 : e - r * in;
    double *fwd = bias ? t.b[l] + r : t.W[l] + ((size_t)(r >> 4) * (t.kp[l] >> 2) + (k >> 2)) * 64 + ((k & 3) << 4) + (r & 15);
    float th;
    if (a.mode == 2) th = (float)*fwd;
    else {
        const double g = a.G[p] * coef_s;
        const double m = a.beta1 * a.m[p] + (1.0 - a.beta1) * g;
        const double v = a.beta2 * a.v[p] + ((1.0 - a.beta2) * g) * g;
        a.m[p] = m; a.v[p] = v;
        th = (float)((double)a.theta[p] - (a.step * m) / (sqrt(v) / a.bc2_sqrt + a.eps));
        *fwd = (double)th;
    }
    a.theta[p] = th;
    if (!bias && l > 0) t.WT[l][((size_t)(k >> 4) * (t.kt[l] >> 2) + (r >> 2)) * 64 + ((r & 3) << 4) + (k & 15)] = (double)th;
}

}  // namespace tum
