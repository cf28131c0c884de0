// collect_kernels.hpp -- K13: what PPO's data collection needs beside the environment of env_kernels.hpp and the policy net of
// policy_kernels.hpp (stable_baselines3: OnPolicyAlgorithm.collect_rollouts + RolloutBuffer.compute_returns_and_advantage, driven by
// Learning_To_Adapt/SafeRL_WMPC/rl_training.py model.learn). The PPO update itself is not here.
//   policy_ac_kernel      the actor-critic evaluation of a tile of 16 instances in ONE workgroup: the value net, then the policy net, back
//                         to back through the same two LDS buffers and the same layer loop as policy_kernel (policy_layers); then one
//                         Philox4x32-10 draw per instance, the sampled action, its log-probability and the value.
//   collect_next_kernel   one lane per instance, behind env_finish_kernel and the value of the step's own observation: the buffer row,
//                         the crash bootstrap, the next step's reset mask / start index / policy input.
//   gae_kernel            one lane per instance, backwards over the [E][B] buffers.
// The sampling rule is this project's own: the distribution of stable_baselines3, not the draws of torch.multinomial.
#pragma once
#include "policy_kernels.hpp"

namespace tum {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., Random123): counter c[4], key k[2] -> c[4]
__host__ __device__ inline void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c[0], p1 = (unsigned long long)PHILOX_M1 * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
}

// the uniform of instance b at decision t: 53 bits of the first two output words, exact in a double, in [0, 1)
__host__ __device__ inline double philox_uniform(unsigned long long seed, unsigned b, unsigned long long t)
{
    unsigned c[4] = {b, (unsigned)t, (unsigned)(t >> 32), 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned long long m = ((unsigned long long)(c[0] >> 5) << 26) + (unsigned long long)(c[1] >> 6);
    return (double)m * 0x1p-53;
}

struct AcArgs {
    PolicyArgs pi, vf;                 // the two nets; obs / obs_stride / n of both are the same; vf.n_mat == 0: no value net
    int rows, do_pi;                   // rows of one LDS buffer (the larger of the two nets'); do_pi == 0: the value alone
    unsigned long long seed, t;
    unsigned first;                    // counter word 0 of instance i is first + i
    double *values, *log_probs, *uniforms;          // [n]: any may be null (pi.actions too)
};

// the draw and the decision of one instance, plain C++: z[j * 16] its logits in LDS. e_j = exp(z_j - m), prefix sums c_j in index
// order, S = c_{A-1}; the action is the smallest j with u S < c_j (A - 1 if none); log_prob = (z_a - m) - log S
__device__ __forceinline__ void policy_sample(const AcArgs &a, const double *z, int inst)
{
#pragma clang fp contract(off)
    const int A = a.pi.n_act;
    double m = z[0];
    for (int j = 1; j < A; j++) {
        const double v = z[j * POL_TILE];
        if (v > m) m = v;
    }
    double S = 0.0;
    for (int j = 0; j < A; j++) S = S + exp(z[j * POL_TILE] - m);
    const double u = philox_uniform(a.seed, a.first + (unsigned)inst, a.t);
    const double thr = u * S;
    int act = A - 1;
    double c = 0.0;
    for (int j = 0; j < A; j++) {
        c = c + exp(z[j * POL_TILE] - m);          // the same sums in the same order as S: c_{A-1} == S
        if (thr < c) { act = j; break; }
    }
    if (a.pi.actions) a.pi.actions[inst] = act;
    if (a.log_probs) a.log_probs[inst] = (z[act * POL_TILE] - m) - log(S);
    if (a.uniforms) a.uniforms[inst] = u;
}

__global__ void __launch_bounds__(64 * POL_WAVES) policy_ac_kernel(const AcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double pol_lds[];          // [2][rows][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * POL_TILE;
    double *buf[2] = {pol_lds, pol_lds + (size_t)a.rows * POL_TILE};
    double v = 0.0;
    if (a.vf.n_mat > 0) {
        policy_load_obs(a.vf, buf[0], i0, tid);
        __syncthreads();
        policy_layers(a.vf, buf, lane, wave);
        if (tid < POL_TILE) v = buf[a.vf.n_mat & 1][tid];          // row 0 of the one-row last matrix
        __syncthreads();                                           // (the policy net's input goes over the value net's buffers)
    }
    if (a.do_pi) {
        policy_load_obs(a.pi, buf[0], i0, tid);
        __syncthreads();
        policy_layers(a.pi, buf, lane, wave);
        if (tid < POL_TILE && i0 + tid < a.pi.n) policy_sample(a, buf[a.pi.n_mat & 1] + tid, i0 + tid);
    }
    if (a.values && tid < POL_TILE && i0 + tid < a.pi.n) a.values[i0 + tid] = v;
}

// fields of the collection buffer, each [E][B] doubles, in this order; behind them the observations [E][B][n_obs], last_values [B],
// last_dones [B], next_obs [B][n_obs] (include/tum_nmpc.h: TUM_COLLECT_*)
enum { COL_ACTION, COL_VALUE, COL_LOGP, COL_REWARD, COL_REWARD_RAW, COL_START, COL_ADV, COL_RET, COL_TERMINATED, COL_TRUNCATED,
       COL_STEP_LENGTH, COL_QP_FAILURES, COL_ERR, COL_FIELDS };

struct CollectArgs {
    int batch, rec, head, n_obs, e, n_env_steps;          // rec = head + n_obs doubles per record of env_finish_kernel
    double gamma;
    const double *out;                // [b][rec]: what env_finish_kernel wrote
    int *in;                          // [3][batch]: the sampled actions; the next step's reset mask and start index
    const int *start_table;           // [n_env_steps][batch]
    double *pol_obs;                  // [b][n_obs]: what the policy saw this step; then its next input
    const double *term_val;           // [b]: the value net on the step's own observation
    const double *first_starts;       // [b]: the episode-start flags of step 0
    double *buf;                      // the collection buffer
};

__global__ void __launch_bounds__(64) collect_next_kernel(const CollectArgs a)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x, B = a.batch;
    if (b >= B) return;
    const size_t EB = (size_t)a.n_env_steps * B, row = (size_t)a.e * B + b;
    const double *o = a.out + (size_t)b * a.rec;
    double *f = a.buf + row, *obs_log = a.buf + COL_FIELDS * EB + row * a.n_obs, *po = a.pol_obs + (size_t)b * a.n_obs;
    const bool terminated = o[1] != 0.0, truncated = o[2] != 0.0, ended = terminated || truncated;
    // TimeLimit.truncated of stable_baselines3 is truncated && !terminated, and in the reference's naming truncated is the CRASH
    // (environment.py:152-165): the crash is bootstrapped, the episode length is not
    double reward = o[0];
    if (truncated && !terminated) reward = reward + a.gamma * a.term_val[b];
    f[COL_ACTION * EB] = (double)a.in[b];
    f[COL_REWARD * EB] = reward; f[COL_REWARD_RAW * EB] = o[0];
    f[COL_START * EB] = a.e == 0 ? a.first_starts[b]
                                 : ((f[COL_TERMINATED * EB - B] != 0.0 || f[COL_TRUNCATED * EB - B] != 0.0) ? 1.0 : 0.0);
    f[COL_TERMINATED * EB] = o[1]; f[COL_TRUNCATED * EB] = o[2]; f[COL_STEP_LENGTH * EB] = o[3]; f[COL_QP_FAILURES * EB] = o[4];
    f[COL_ERR * EB] = o[5];
    const bool reset = ended && a.e + 1 < a.n_env_steps;
    a.in[B + b] = reset ? 1 : 0;
    a.in[2 * B + b] = reset ? a.start_table[(size_t)(a.e + 1) * B + b] : 0;
    // environment.py:230-233: the observation a reset returns is all zeros
    double *next_obs = a.buf + (COL_FIELDS + a.n_obs) * EB + 2 * B + (size_t)b * a.n_obs;
    for (int i = 0; i < a.n_obs; i++) {
        const double nx = ended ? 0.0 : o[a.head + i];
        obs_log[i] = po[i];
        po[i] = nx;
        if (a.e + 1 == a.n_env_steps) next_obs[i] = nx;
    }
    a.buf[(COL_FIELDS + a.n_obs) * EB + B + b] = ended ? 1.0 : 0.0;          // last_dones: the last step's stands
}

struct GaeArgs {
    int E, B;
    double gamma, lambda;
    const double *rewards, *values, *episode_starts, *last_values, *last_dones;          // [E][B] x 3, [B] x 2
    double *adv, *ret;                                                                    // [E][B]
};

// RolloutBuffer.compute_returns_and_advantage, FP64, in exactly this association
__global__ void __launch_bounds__(64) gae_kernel(const GaeArgs a)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x, B = a.B, E = a.E;
    if (b >= B) return;
    double last = 0.0;
    for (int t = E - 1; t >= 0; t--) {
        const size_t i = (size_t)t * B + b;
        const double nnt = 1.0 - (t == E - 1 ? a.last_dones[b] : a.episode_starts[i + B]);
        const double nv = t == E - 1 ? a.last_values[b] : a.values[i + B];
        const double delta = (a.rewards[i] + (a.gamma * nv) * nnt) - a.values[i];
        last = delta + ((a.gamma * a.lambda) * nnt) * last;
        a.adv[i] = last;
        a.ret[i] = last + a.values[i];
    }
}

}  // namespace tum
