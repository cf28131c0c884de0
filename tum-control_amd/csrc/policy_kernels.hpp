// policy_kernels.hpp -- K12: the weight-scheduling agent of the reference on the device (Learning_To_Adapt/SafeRL_WMPC: enable_WMPC of the
// controller classes, RL_WMPC/evaluation.py:65-105 run_policy; both call model.predict(obs, deterministic=True)) and what strings its
// decisions and the environment of env_kernels.hpp into whole episodes without the host.
//   policy_kernel        batched inference of the policy net: h = tanh(W h + b) per hidden layer, a linear action layer, softmax, argmax.
//                        FP64 on the float32 weights (converted exactly at attach time), the observation rounded to float32 first as
//                        stable_baselines3 does. One WORKGROUP of POL_WAVES wavefronts owns a tile of 16 instances: D[output][instance]
//                        accumulates on v_mfma_f64_16x16x4_f64 over K in steps of 4, A a 16 x 4 block of W, B the activations
//                        h[k][instance] from LDS; the activations ping-pong between two LDS buffers; the 16-output tiles of a layer are
//                        spread over the wavefronts, a barrier between layers. Every weight read serves 16 instances. The load of
//                        the observation and the layer loop are device functions (policy_load_obs, policy_layers) that
//                        policy_ac_kernel of collect_kernels.hpp runs as well: one order of sums for both.
//   rollout_next_kernel  one lane per instance, behind env_finish_kernel inside a rollout: the record into the rollout's log, the next
//                        step's reset mask / start index and the policy's next input, the live flag and the counter of live instances.
#pragma once
#include "nmpc_device.hpp"

namespace tum {

constexpr int POL_TILE = 16;           // instances per workgroup: the N of the 16 x 16 x 4 product
#ifndef TUM_POL_WAVES
#define TUM_POL_WAVES 4                // (scripts/probes/probe_policy_waves.cpp builds the kernel with 1, 2, 4 and 8)
#endif
constexpr int POL_WAVES = TUM_POL_WAVES;          // wavefronts per workgroup (the output tiles of a layer are dealt round robin)
#ifndef TUM_POL_AHEAD
#define TUM_POL_AHEAD 1
#endif
constexpr int POL_AHEAD = TUM_POL_AHEAD;          // operands of this many products are loaded before the first of them is issued
constexpr int POL_MAXMAT = 5;          // matrices: up to 4 hidden layers and the action layer
constexpr int POL_MAXWIDTH = 256;      // widest hidden layer: 2 x 256 x 16 doubles of LDS
constexpr int POL_MAXIN = 128;
constexpr int POL_MAXACT = 64;

struct PolicyArgs {
    int n, n_mat, n_in, n_act, rows;            // instances, matrices, true input width, true action count, rows of one LDS buffer
    int kp[POL_MAXMAT], mp[POL_MAXMAT];         // per matrix: inputs padded to a multiple of 4, outputs padded to a multiple of 16
    // W[l]: [mp / 16][kp / 4][64] doubles, the A operand of one product per 64 (lane l holds W[16 t + (l & 15)][4 q + (l >> 4)]), zero
    // where padded; b[l]: [mp], zero where padded
    const double *W[POL_MAXMAT], *b[POL_MAXMAT];
    const double *obs; int obs_stride;          // [n][obs_stride] doubles, the first n_in of a row
    double *logits, *probs; int *actions;       // [n][n_act], [n][n_act], [n]: any may be null
};

// tanh of the hidden layers: the device library's. Its error against the exact value is MEASURED, over 1e-300 <= |x| <= 40, the signed
// zeros and the neighbourhoods of its branch points -- 2^-27 (tanh x = x below), 19.0625 (1 above) and the breaks of the exponential's
// range reduction in between: tests/test_gpu_policy.py, profiles/policy_bounds.txt
__device__ __forceinline__ double policy_tanh(double x) { return tanh(x); }

// softmax and argmax of one instance, plain C++: z[j * 16] its logits in LDS. The first index of the largest logit wins (numpy / torch
// argmax on an exact tie)
__device__ __forceinline__ void policy_decide(const PolicyArgs &a, const double *z, int inst)
{
#pragma clang fp contract(off)
    const size_t row = (size_t)inst * a.n_act;
    int best = 0;
    double zmax = z[0];
    for (int j = 1; j < a.n_act; j++) {
        const double v = z[j * POL_TILE];
        if (v > zmax) { zmax = v; best = j; }
    }
    if (a.actions) a.actions[inst] = best;
    if (a.logits)
        for (int j = 0; j < a.n_act; j++) a.logits[row + j] = z[j * POL_TILE];
    if (a.probs) {
        double s = 0.0;
        for (int j = 0; j < a.n_act; j++) s = s + exp(z[j * POL_TILE] - zmax);
        for (int j = 0; j < a.n_act; j++) a.probs[row + j] = exp(z[j * POL_TILE] - zmax) / s;
    }
}

// The observation of a tile into one LDS buffer, rounded to float32 (stable_baselines3: obs_as_tensor -> float32 before the first
// Linear); zero rows up to kp[0], zero columns behind the last instance of a partial tile. The caller puts the barrier behind it.
__device__ __forceinline__ void policy_load_obs(const PolicyArgs &a, double *dst, int i0, int tid)
{
    for (int i = tid; i < a.kp[0] * POL_TILE; i += 64 * POL_WAVES) {
        const int inst = i / a.kp[0], k = i - inst * a.kp[0];
        double v = 0.0;
        if (i0 + inst < a.n && k < a.n_in) v = (double)(float)a.obs[(size_t)(i0 + inst) * a.obs_stride + k];
        dst[k * POL_TILE + inst] = v;
    }
}

// The layers of one net on the tile whose input is in buf[0]: the result of matrix l is in buf[(l + 1) & 1], a barrier behind every
// layer. policy_kernel and policy_ac_kernel both run this loop and nothing else on the matrices: one order of sums.
// KEEP (ppo_tile_kernel of ppo_kernels.hpp, the same loop and the same sums): the hidden activations also go to memory for the
// backward pass, instance i0 + column of the tile at keep[l + 1] + (i0 + column) * mp[l].
template <bool KEEP = false>
__device__ __forceinline__ void policy_layers(const PolicyArgs &a, double *const *buf, int lane, int wave, double *const *keep = nullptr, int i0 = 0)
{
    const int col = lane & 15, quad = lane >> 4;
    for (int l = 0; l < a.n_mat; l++) {
        const double *src = buf[l & 1];
        double *dst = buf[(l + 1) & 1];
        const int nq = a.kp[l] >> 2, nt = a.mp[l] >> 4;
        const bool hidden = l + 1 < a.n_mat;
        for (int t = wave; t < nt; t += POL_WAVES) {
            const double *Wt = a.W[l] + (size_t)t * nq * 64 + lane, *bt = a.b[l] + 16 * t + quad;
            d4 acc = {bt[0], bt[4], bt[8], bt[12]};          // D row (lane >> 4) + 4 j, column lane & 15
            const double *h = src + quad * POL_TILE + col;
            // the products of a tile form one dependent chain in q, in this order whatever POL_AHEAD is: the same sums to the bit
            int q = 0;
            for (; q + POL_AHEAD <= nq; q += POL_AHEAD) {
                double w[POL_AHEAD], x[POL_AHEAD];
#pragma unroll
                for (int i = 0; i < POL_AHEAD; i++) { w[i] = Wt[(size_t)(q + i) * 64]; x[i] = h[(q + i) * 4 * POL_TILE]; }
#pragma unroll
                for (int i = 0; i < POL_AHEAD; i++) acc = mfma(w[i], x[i], acc);
            }
            for (; q < nq; q++) acc = mfma(Wt[(size_t)q * 64], h[q * 4 * POL_TILE], acc);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double v = hidden ? policy_tanh(acc[j]) : acc[j];
                dst[(16 * t + quad + 4 * j) * POL_TILE + col] = v;
                if (KEEP && hidden) keep[l + 1][(size_t)(i0 + col) * a.mp[l] + 16 * t + quad + 4 * j] = v;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64 * POL_WAVES) policy_kernel(const PolicyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double pol_lds[];          // [2][rows][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * POL_TILE;
    double *buf[2] = {pol_lds, pol_lds + (size_t)a.rows * POL_TILE};
    policy_load_obs(a, buf[0], i0, tid);
    __syncthreads();
    policy_layers(a, buf, lane, wave);
    if (tid < POL_TILE && i0 + tid < a.n) policy_decide(a, buf[a.n_mat & 1] + tid, i0 + tid);
}

struct RolloutArgs {
    int batch, rec, head, n_obs, e, n_env_steps, on_end;          // rec = head + n_obs doubles per record (head: ENV_REC of env_kernels.hpp)
    const double *out;                // [b][rec]: what env_finish_kernel wrote
    int *in;                          // [3][batch]: the next step's reset mask and start index (the policy writes the actions)
    const int *start_table;           // [n_env_steps][batch] or null
    double *pol_obs;                  // [b][n_obs]: the policy's next input
    int *live, *n_live;               // [b], [1]
    double *log; int *act_log, *live_log;          // [e][b][rec], [e][b], [e][b]
};

__global__ void __launch_bounds__(64) rollout_next_kernel(const RolloutArgs a)
{
    const int b = blockIdx.x * 64 + threadIdx.x, B = a.batch;
    if (b >= B) return;
    const double *o = a.out + (size_t)b * a.rec;
    double *lg = a.log + ((size_t)a.e * B + b) * a.rec;
    for (int i = 0; i < a.rec; i++) lg[i] = o[i];
    const int live = a.live[b];
    a.act_log[(size_t)a.e * B + b] = a.in[b];
    a.live_log[(size_t)a.e * B + b] = live;
    const bool ended = o[1] != 0.0 || o[2] != 0.0;
    const bool reset = a.on_end == 1 && ended && a.e + 1 < a.n_env_steps;
    a.in[B + b] = reset ? 1 : 0;
    a.in[2 * B + b] = reset ? a.start_table[(size_t)(a.e + 1) * B + b] : 0;
    // environment.py:230-233: the observation a reset returns is all zeros
    for (int i = 0; i < a.n_obs; i++) a.pol_obs[(size_t)b * a.n_obs + i] = (a.on_end == 1 && ended) ? 0.0 : o[a.head + i];
    if (a.on_end == 0 && live && ended) {
        a.live[b] = 0;
        atomicSub(a.n_live, 1);
    }
}

}  // namespace tum
