// wmpc_kernels.hpp -- K19: the learned weight schedule of the reference's controller classes (enable_WMPC: NMPC_class.py:120-160,208-239,
// SNMPC_class.py:224-255, Reduced_Robustified_NMPC_class.py:206-245,373-404) inside the device closed loop.
//   wmpc_schedule_kernel  once per control step between the solve and plant_advance_kernel (where env_score_kernel sits), inside captured
//                         chunks too. Every `period` control steps an instance is DUE: its observation is formed from the state the solve
//                         started at and this step's reference window, the policy net picks a row of the parameter table, the row is
//                         installed as the cost setter would (env_begin_kernel). An instance whose solve failed gets the weights the
//                         loop held at attach time back (on_failure "base": the reference builds a fresh solver from the YAML weights).
// One WORKGROUP of POL_WAVES wavefronts owns a tile of POL_TILE = 16 instances, as in policy_kernel: the forward pass is policy_layers and
// policy_decide unchanged, one order of sums for every kernel that evaluates the net.
// Which step is a decision step is decided HERE (a captured chunk replays constant arguments, and 25 is no multiple of 20): instance b
// holds since[b], the control step of its last decision (the step the schedule was attached at before the first); its counter -- the
// reference's self.counter before the test -- is step - since[b], and it is due where that is >= period. The decision writes
// since[b] = step, which IS "counter = 0, then counter += 1"; a step without a decision writes nothing at all. (A stored counter that
// every launch bumps would be written by the first wavefront of a tile while the last one may still be reading it for the exit test
// below, which has no barrier in front of it: the wavefronts could then disagree on whether the tile is due.)
// The exit test: lane i < 16 of EVERY wavefront reads since[] and status[] of instance i0 + i, a ballot makes the tile's masks. Nothing
// this kernel writes before its first barrier feeds them, so all wavefronts of a workgroup take the same branch. 19 launches out of 20
// end there.
#pragma once
#include "env_kernels.hpp"
#include "policy_kernels.hpp"

namespace tum {

struct WmpcArgs {
    int N, batch, n_actions, n_samples, period, restore, log_cap;
    double Ts;
    const double *table;                              // [n_actions][7]
    const int *obs_idx;                               // [2][n_samples]: sample indices into ref_v and into the averaged yaw rate
    const double *obs_bounds;                         // [2][2 + 2 n_samples]: lower, upper
    const double *base_W, *base_pen;                  // [b][(N + 1) * 6], [b][36]: what the loop held when the schedule was attached
    // the loop's state
    const double *x0, *yref, *ref0; const int *status, *step_counter;
    double *W, *pen;
    // the schedule's state, per instance
    int *since, *n_dec;                               // control step of the last decision; decisions taken
    int *log_step, *log_act; double *log_obs;         // [b][log_cap], [b][log_cap], [b][log_cap][2 + 2 n_samples]: the first log_cap decisions
    PolicyArgs pol;                                   // the attached policy net; pol.actions: [batch], the action of the last decision
};

// LDS of one workgroup: the policy's two activation buffers, then the tile's windows yaw[N + 1][16] | v[N + 1][16] (instance fastest:
// the 16 lanes that unwrap side by side hit 16 different banks)
__host__ __device__ inline size_t wmpc_lds_doubles(int rows, int N) { return (size_t)2 * rows * POL_TILE + (size_t)2 * (N + 1) * POL_TILE; }

__global__ void __launch_bounds__(64 * POL_WAVES) wmpc_schedule_kernel(const WmpcArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double wm_lds[];
    __shared__ int sMode[POL_TILE];          // per instance of the tile: bit 0 install the decided row, bit 1 restore the snapshot
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * POL_TILE, N = a.N, B = a.batch;
    const int step = a.step_counter[0];               // control steps done before this one
    bool due = false, failed = false;
    if (lane < POL_TILE && i0 + lane < B) {
        due = step - a.since[i0 + lane] >= a.period;
        failed = a.restore && a.status[i0 + lane] != 0;
    }
    const unsigned dmask = (unsigned)__ballot(due), fmask = (unsigned)__ballot(failed);
    if (!(dmask | fmask)) return;

    double *buf[2] = {wm_lds, wm_lds + (size_t)a.pol.rows * POL_TILE};
    double *sYaw = wm_lds + (size_t)2 * a.pol.rows * POL_TILE, *sV = sYaw + (size_t)(N + 1) * POL_TILE;
    if (dmask) {          // (the same for every wavefront of the workgroup: the barriers below are met by all or by none)
        const int ns = a.n_samples, no = 2 + 2 * ns;
        const double *lo = a.obs_bounds, *hi = a.obs_bounds + no;
        // the reference windows of the due instances, and a zero input buffer (policy_load_obs: zero rows up to kp[0], zero columns
        // of the instances that are not evaluated)
        for (int i = tid; i < (N + 1) * POL_TILE; i += 64 * POL_WAVES) {
            const int inst = i / (N + 1), j = i - inst * (N + 1);
            if (!((dmask >> inst) & 1u)) continue;
            const double *y = a.yref + ((size_t)(i0 + inst) * (N + 1) + j) * 6;
            sYaw[j * POL_TILE + inst] = y[2];
            sV[j * POL_TILE + inst] = y[3];
        }
        for (int i = tid; i < a.pol.kp[0] * POL_TILE; i += 64 * POL_WAVES) buf[0][i] = 0.0;
        __syncthreads();
        // np.unwrap(period = 2 pi): a sequential cumulative correction, one lane per instance, 16 instances side by side
        if (tid < POL_TILE && ((dmask >> tid) & 1u)) {
            double prev = sYaw[tid], cum = 0.0;
            for (int j = 1; j <= N; j++) {
                const double p = sYaw[j * POL_TILE + tid];
                const double dd = p - prev;
                double md = fmod(dd + M_PI, 2.0 * M_PI);
                if (md != 0.0 && md < 0.0) md += 2.0 * M_PI;
                double ddmod = md - M_PI;
                if (ddmod == -M_PI && dd > 0.0) ddmod = M_PI;
                double corr = ddmod - dd;
                if (fabs(dd) < M_PI) corr = 0.0;
                cum += corr;
                sYaw[j * POL_TILE + tid] = p + cum;
                prev = p;
            }
        }
        __syncthreads();
        // the observation (observation.py:28-75), the operations of env_finish_kernel in its order; rounded to float32 into the
        // policy's input, unrounded into the decision log while that has room
        for (int i = tid; i < (ns + 1) * POL_TILE; i += 64 * POL_WAVES) {
            const int inst = i & (POL_TILE - 1), j = i / POL_TILE - 1, b = i0 + inst;
            if (!((dmask >> inst) & 1u)) continue;
            const int slot = a.n_dec[b];
            double *lg = slot < a.log_cap ? a.log_obs + ((size_t)b * a.log_cap + slot) * no : nullptr;
            if (j < 0) {
                // LonLatDeviations (Utils/MPC_sim_utils.py:102-112), lateral component, of the state the solve started at against the
                // first point of this step's reference; velocity against the window's first speed
                const double *xs = a.x0 + (size_t)b * NX, *rf = a.ref0 + (size_t)b * 4;
                double sn, cs;
                fast_sincos(-xs[2], &sn, &cs);
                const double lat = sn * (rf[0] - xs[0]) + cs * (rf[1] - xs[1]);
                const double vel = xs[3] - sV[inst];
                const double o0 = (lat - lo[0]) / (hi[0] - lo[0]), o1 = (vel - lo[1]) / (hi[1] - lo[1]);
                buf[0][inst] = (double)(float)o0;
                buf[0][POL_TILE + inst] = (double)(float)o1;
                if (lg) { lg[0] = o0; lg[1] = o1; }
            } else {
                const int iv = a.obs_idx[j], ir = a.obs_idx[ns + j];
                double s = 0.0;
                for (int k = 0; k < ENV_MA; k++) {          // np.convolve(np.diff(yaw) / Ts, ones(10) / 10, 'valid')
                    const double rate = (sYaw[(ir + k + 1) * POL_TILE + inst] - sYaw[(ir + k) * POL_TILE + inst]) / a.Ts;
                    s = s + rate * (1.0 / ENV_MA);
                }
                const double ov = (sV[iv * POL_TILE + inst] - lo[2 + j]) / (hi[2 + j] - lo[2 + j]);
                const double orr = (s - lo[2 + ns + j]) / (hi[2 + ns + j] - lo[2 + ns + j]);
                buf[0][(2 + j) * POL_TILE + inst] = (double)(float)ov;
                buf[0][(2 + ns + j) * POL_TILE + inst] = (double)(float)orr;
                if (lg) { lg[2 + j] = ov; lg[2 + ns + j] = orr; }
            }
        }
        __syncthreads();
        policy_layers(a.pol, buf, lane, wave);          // (a barrier behind the last layer)
    }
    if (tid < POL_TILE) {
        const int b = i0 + tid;
        int mode = 0;
        if ((dmask >> tid) & 1u) {
            policy_decide(a.pol, buf[a.pol.n_mat & 1] + tid, b);          // -> pol.actions[b]
            const int slot = a.n_dec[b];
            if (slot < a.log_cap) { a.log_step[(size_t)b * a.log_cap + slot] = step; a.log_act[(size_t)b * a.log_cap + slot] = a.pol.actions[b]; }
            a.n_dec[b] = slot + 1;
            a.since[b] = step;          // counter = 0 now, 1 at the next step's test
            mode = 1;
        }
        // main.py:59-61: a failed solve is followed by a fresh solver with the constructor's weights -- a row decided at this very step is lost
        if ((fmask >> tid) & 1u) mode = 2;
        sMode[tid] = mode;
    }
    __syncthreads();
    // update_cost_function_weights as env_begin_kernel writes it, or the snapshot
    const int nw = N * 6 + 4, recW = (N + 1) * 6;
    for (int i = tid; i < POL_TILE * recW; i += 64 * POL_WAVES) {
        const int inst = i / recW, k = i - inst * recW, mode = sMode[inst];
        const size_t at = (size_t)(i0 + inst) * recW + k;
        if (mode == 2) a.W[at] = a.base_W[at];
        else if (mode == 1 && k < nw) {
            const double *p = a.table + (size_t)7 * a.pol.actions[i0 + inst];
            const int q = k % 6;
            a.W[at] = q < 2 ? p[0] : q == 2 ? p[1] : q == 3 ? p[2] : q == 4 ? p[3] : p[4];
        }
    }
    for (int i = tid; i < POL_TILE * 36; i += 64 * POL_WAVES) {
        const int inst = i / 36, k = i - inst * 36, mode = sMode[inst];
        const size_t at = (size_t)(i0 + inst) * 36 + k;
        if (mode == 2) a.pen[at] = a.base_pen[at];
        else if (mode == 1) {
            // pen[b][class][slot][zl, zu, Zl, Zu]: class 0 (stage 0) slot 0, class 1 (stages 1..N-1) slots 0..2, class 2 (stage N) slots 1, 2
            const int cls = k / 12, slot = (k >> 2) % 3, which = k & 3;
            const bool used = cls == 0 ? slot == 0 : cls == 1 ? true : slot >= 1;
            const double *p = a.table + (size_t)7 * a.pol.actions[i0 + inst];
            if (used) a.pen[at] = which < 2 ? p[5] : p[6];
        }
    }
}

}  // namespace tum
