// env_kernels.hpp -- K11: the weight-scheduling RL environment of the reference around the device closed loop
// (Learning_To_Adapt/SafeRL_WMPC/RL_WMPC/environment.py:112-240, reward.py, observation.py).
//   env_begin_kernel   once per environment step: per-instance reset (environment.py:191-237), the agent's row of the parameter table
//                      (NMPC_class.py:269-317 update_cost_function_weights), episode_steps++ (environment.py:115)
//   env_score_kernel   once per control step between the solve and plant_advance_kernel: lat_dev / vel_dev
//                      (Utils/Logging_Plotting.py:152-159), truncated / terminated (environment.py:152-169), the reference window
//   env_finish_kernel  once per environment step: reward (reward.py:15-33), observation (observation.py:28-75), one record per instance
// One WAVEFRONT per instance in all three. What costs here is not arithmetic: the begin kernel writes (N + 1) * 8 + N * 8 words of one
// instance, the score kernel copies 2 (N + 1) words of its reference window, the finish kernel unwraps N + 1 yaw angles -- a sequential
// cumulative sum of N dependent additions, once per ENVIRONMENT step, on lane 0 from LDS -- and then differentiates, averages and samples
// with one lane per point. With one lane per instance every one of those loops would be 64 instances wide and uncoalesced.
#pragma once
#include "loop_kernels.hpp"

namespace tum {

constexpr int ENV_TERMINATED = 1;      // environment.py:161-165
constexpr int ENV_TRUNCATED = 2;       // environment.py:153-158: lat_dev > max_lat_dev, signed
constexpr int ENV_MAXPTS = 128;        // longest reference window (N + 1) the finish kernel's LDS holds
constexpr int ENV_REC = 6;             // head of a result record: reward, terminated, truncated, step_length, qp_failures, planner error word; then the observation
constexpr int ENV_MA = 10;             // taps of the moving average of the yaw rate (observation.py:52)

struct EnvArgs {
    int N, batch, n_track, n_actions, n_samples, episode_length, full_lap, obs_last_step, log_cap;
    double max_lat_dev, Ts;
    double sig[2], lim[4];                            // reward.py: sigmas; lims[0][lat, vel], lims[1][lat, vel]
    const double *track, *table;                      // [n_track][4], [n_actions][7]
    const int *track_of, *track_rows;                 // a track set (null: one track): [batch] track of an instance, [n_tracks + 1] first rows in `track`
    const int *in;                                    // [3][batch]: actions, reset mask, start index (one upload per environment step)
    const int *obs_idx;                               // [2][n_samples]: sample indices into ref_v and into the averaged yaw rate
    const double *obs_bounds;                         // [2][2 + 2 n_samples]: lower, upper
    // the loop's state
    double *X, *U, *x0, *W, *pen, *qp_lam, *x_sim, *pose, *hist;
    const double *yref, *ref0; const int *closest, *status, *step_counter, *err;
    double *lCiLX, *lSimX;
    // the environment's state, per instance
    int *ep_steps, *count, *flags, *qpf, *samples;    // episode_steps, scored control steps / flags / failed solves of this environment step, estimator samples
    double *acc;                                      // [b][4]: sum lat_dev^2, sum vel_dev^2, lat_dev and vel_dev of the last scored control step
    double *win;                                      // [b][2][N + 1]: ref_yaw, ref_v of the last scored control step
    double *out;                                      // [b][ENV_REC + 2 + 2 n_samples]
};

// the table and the length of the track instance b drives on (a.track / a.n_track where the loop holds one track)
__device__ __forceinline__ const double *env_track(const EnvArgs &a, int b, int &n)
{
    n = a.n_track;
    if (!a.track_of) return a.track;
    const int t = a.track_of[b], r0 = a.track_rows[t];
    n = a.track_rows[t + 1] - r0;
    return a.track + (size_t)4 * r0;
}

// with_actions = 0: resets only (tum_sim_env_reset)
__global__ void __launch_bounds__(64) env_begin_kernel(const EnvArgs a, int with_actions)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch) return;
    const int N = a.N, B = a.batch;
    const int idx = a.in[2 * B + b];
    int n_track;
    const double *track = env_track(a, b, n_track);          // (start indices are local to the instance's own track)
    if (a.in[B + b] != 0 && idx >= 0 && idx < n_track) {
        // environment.py:191-237: a fresh MPC_Sim at idx_ref_start (SimulationMode_main_class.py:60-75: position, yaw mod 2 pi, reference
        // speed, everything else 0), MPC.reset(X0_MPC) (NMPC_class.py:256-267: x_k = x0, u = 0), a fresh Logger. What tum_sim_set_state
        // and cold_start_kernel do, for this instance only
        const double *t = track + (size_t)4 * idx;
        const double xv[4] = {t[0], t[1], pymod_2pi(t[2]), t[3]};
        for (int i = lane; i < (N + 1) * NX; i += 64) {
            const int q = i & 7;
            a.X[(size_t)b * (N + 1) * NX + i] = q == 0 ? xv[0] : q == 1 ? xv[1] : q == 2 ? xv[2] : q == 3 ? xv[3] : 0.0;
        }
        for (int i = lane; i < N * NU; i += 64) a.U[(size_t)b * N * NU + i] = 0.0;
        if (lane < 32) a.hist[(size_t)b * 32 + lane] = 0.0;
        if (lane < 8) {
            const double v = lane == 0 ? xv[0] : lane == 1 ? xv[1] : lane == 2 ? xv[2] : lane == 3 ? xv[3] : 0.0;
            a.x0[(size_t)b * NX + lane] = v;
            if (lane < 7) a.x_sim[(size_t)b * 7 + lane] = v;
            if (lane < 2) a.pose[(size_t)b * 2 + lane] = v;
            // the logs stay indexed by the loop's global step: row s keeps being the plant state BEFORE control step s
            const int s = a.step_counter[0];
            if (a.lCiLX && s <= a.log_cap) {
                if (lane < 7) a.lCiLX[((size_t)s * B + b) * 7 + lane] = v;
                a.lSimX[((size_t)s * B + b) * 8 + lane] = v;
            }
        }
        if (lane == 0) {
            a.qp_lam[(size_t)b * (6 * N + 2) + 6 * N] = 0.0;          // (the interior point method of the next solve starts cold as well)
            a.samples[b] = 0;
            a.ep_steps[b] = 0;
        }
    }
    if (lane < 4) a.acc[(size_t)b * 4 + lane] = 0.0;
    if (lane == 0) { a.count[b] = 0; a.flags[b] = 0; a.qpf[b] = 0; }
    if (!with_actions) return;
    const int act = a.in[b];
    if (act < 0 || act >= a.n_actions) return;          // (the host has refused the step: nothing is launched with such an action)
    // update_cost_function_weights (NMPC_class.py:269-317): W = diag(q_xy, q_xy, q_yaw, q_vel, r_jerk, r_steer) at the stages 0..N-1, its
    // first four entries at stage N (the two words behind them stay), zl = zu = L1 and Zl = Zu = L2 for the slacks each class has
    const double *p = a.table + (size_t)7 * act;
    const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], L1 = p[5], L2 = p[6];
    for (int i = lane; i < N * 6 + 4; i += 64) {
        const int q = i % 6;
        a.W[(size_t)b * (N + 1) * 6 + i] = q < 2 ? p0 : q == 2 ? p1 : q == 3 ? p2 : q == 4 ? p3 : p4;
    }
    if (lane < 36) {
        // pen[b][class][slot][zl, zu, Zl, Zu]: class 0 (stage 0) slot 0, class 1 (stages 1..N-1) slots 0..2, class 2 (stage N) slots 1, 2
        const int cls = lane / 12, slot = (lane >> 2) % 3, which = lane & 3;
        const bool used = cls == 0 ? slot == 0 : cls == 1 ? true : slot >= 1;
        if (used) a.pen[(size_t)b * 36 + lane] = which < 2 ? L1 : L2;
    }
    if (lane == 0) a.ep_steps[b] += 1;                     // environment.py:115
}

__global__ void __launch_bounds__(64) env_score_kernel(const EnvArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch) return;
    if (a.flags[b] != 0) return;                        // this environment step has ended for the instance: it keeps driving unscored
    const int N = a.N;
    // the reference window of this control step: what the observation is made of if this is the last scored one
    for (int j = lane; j <= N; j += 64) {
        const double *y = a.yref + ((size_t)b * (N + 1) + j) * 6;
        a.win[(size_t)b * 2 * (N + 1) + j] = y[2];
        a.win[(size_t)b * 2 * (N + 1) + (N + 1) + j] = y[3];
    }
    if (lane != 0) return;
    const double *xs = a.x_sim + (size_t)b * 7, *rf = a.ref0 + (size_t)b * 4;
    // LonLatDeviations (Utils/MPC_sim_utils.py:102-112), lateral component; velocity deviation (Logging_Plotting.py:152-159)
    double sn, cs;
    fast_sincos(-xs[2], &sn, &cs);
    const double lat = sn * (rf[0] - xs[0]) + cs * (rf[1] - xs[1]);
    const double vel = xs[3] - rf[3];
    double *acc = a.acc + (size_t)b * 4;
    a.count[b] += 1;
    acc[0] = acc[0] + lat * lat;
    acc[1] = acc[1] + vel * vel;
    acc[2] = lat; acc[3] = vel;
    if (a.status[b] != 0) a.qpf[b] += 1;
    int f = 0;
    if (lat > a.max_lat_dev) f |= ENV_TRUNCATED;
    int n_track = 0;
    if (a.full_lap) (void)env_track(a, b, n_track);          // (the last-but-one waypoint of the instance's own track)
    if (a.full_lap ? a.closest[b] == n_track - 2 : a.ep_steps[b] == a.episode_length) f |= ENV_TERMINATED;
    if (f) a.flags[b] = f;
}

__global__ void __launch_bounds__(64) env_finish_kernel(const EnvArgs a)
{
#pragma clang fp contract(off)
    __shared__ double sYaw[ENV_MAXPTS], sRate[ENV_MAXPTS];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch) return;
    const int N = a.N, ns = a.n_samples, no = 2 + 2 * ns;
    const double *yaw = a.win + (size_t)b * 2 * (N + 1), *vref = yaw + (N + 1);
    double *o = a.out + (size_t)b * (ENV_REC + no);
    const double *lo = a.obs_bounds, *hi = a.obs_bounds + no;
    if (lane == 0) {
        // reward.py:15-33
        const int n = a.count[b];
        const double *acc = a.acc + (size_t)b * 4;
        double h = 0.0;
        if (n > 0) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const double m = sqrt(acc[i] / (double)n);
                const double v = fmin(fmax((m - a.lim[i]) / (a.lim[2 + i] - a.lim[i]), 0.0), 1.0);
                h = h + (v * v) / (2.0 * a.sig[i]);
            }
        }
        const int f = a.flags[b];
        o[0] = n > 0 ? exp(-h) : 0.0;
        o[1] = (f & ENV_TERMINATED) ? 1.0 : 0.0; o[2] = (f & ENV_TRUNCATED) ? 1.0 : 0.0;
        o[3] = (double)n; o[4] = (double)a.qpf[b]; o[5] = (double)a.err[0];
        // Logger.get_observation_states reads the row BEHIND the last one written: 0, 0 in the reference (obs_last_step = 0)
        const double l = a.obs_last_step ? acc[2] : 0.0, v = a.obs_last_step ? acc[3] : 0.0;
        o[ENV_REC] = (l - lo[0]) / (hi[0] - lo[0]);
        o[ENV_REC + 1] = (v - lo[1]) / (hi[1] - lo[1]);
        // np.unwrap(period = 2 pi): sequential cumulative correction
        double prev = yaw[0], cum = 0.0;
        sYaw[0] = prev;
        for (int j = 1; j <= N; j++) {
            const double p = yaw[j];
            const double dd = p - prev;
            double md = fmod(dd + M_PI, 2.0 * M_PI);
            if (md != 0.0 && md < 0.0) md += 2.0 * M_PI;
            double ddmod = md - M_PI;
            if (ddmod == -M_PI && dd > 0.0) ddmod = M_PI;
            double corr = ddmod - dd;
            if (fabs(dd) < M_PI) corr = 0.0;
            cum += corr;
            sYaw[j] = p + cum;
            prev = p;
        }
    }
    __syncthreads();
    // np.diff / Ts: the loop's Ts although the points are Tp / N apart (observation.py:49, environment.py:180)
    for (int j = lane; j < N; j += 64) sRate[j] = (sYaw[j + 1] - sYaw[j]) / a.Ts;
    __syncthreads();
    for (int j = lane; j < ns; j += 64) {
        const int iv = a.obs_idx[j], ir = a.obs_idx[ns + j];
        double s = 0.0;
        for (int k = 0; k < ENV_MA; k++) s = s + sRate[ir + k] * (1.0 / ENV_MA);          // np.convolve(rate, ones(10) / 10, 'valid')
        o[ENV_REC + 2 + j] = (vref[iv] - lo[2 + j]) / (hi[2 + j] - lo[2 + j]);
        o[ENV_REC + 2 + ns + j] = (s - lo[2 + ns + j]) / (hi[2 + ns + j] - lo[2 + ns + j]);
    }
}

}  // namespace tum
