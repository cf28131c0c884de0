// sim_loop.hpp -- host side of the device closed loop (K8 / K9) and of segment scoring: tum_sim, the owners of its memory, the control
// step, tum_sim_run, the disturbance generator (K18), the segments and the getters. Host code only, included by tum_nmpc.hip behind the capsule it drives (tum_ocp,
// invalidate, flush_inputs, launch ...): the library stays one translation unit. The RL layers on top of it are sim_rl.hpp.
#pragma once

// Owner of one array, on the device or in pinned host memory: move-only, freed with its owner; get() is what goes into the kernel arguments.
//   alloc(n)    a fresh array of n elements; device arrays zero-filled and waited for as dalloc does, or (zero = false) left as hipMalloc
//               hands them out, without a device-wide wait: temporaries that are uploaded to in full
//   reserve(n)  grow only: at least n elements afterwards. Growing frees and allocates anew; the contents are NOT kept
// Both return the HIP error and leave the buffer empty where they fail.
template <typename T, bool PINNED>
class Buf {
    T *p = nullptr; size_t n = 0;
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }          // (o's destructor frees what we held)
    ~Buf() { reset(); }
    void reset() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; n = 0; }
    hipError_t alloc(size_t count, bool zero = true)
    {
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p, sizeof(T) * count, hipHostMallocDefault) :
                             zero ? dalloc(&p, count) : hipMalloc((void **)&p, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) n = count; else reset();
        return e;
    }
    hipError_t reserve(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    T *get() const { return p; }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// a kernel launch and the check behind it (returns from the caller where the launch was refused)
#define LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); HIPCHK(hipGetLastError()); } while (0)

// n ints on the device, handed out as doubles (the getters' one number format)
static int fetch_ints(const int *src, size_t n, double *out)
{
    std::vector<int> t(n);
    HIPCHK(hipMemcpy(t.data(), src, sizeof(int) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) out[i] = t[i];
    return 0;
}

// ---------------------------------------------------------------------------------------------- the state of a loop, by what is attached together
// Every sub-state holds its settings, its buffers and whether it is attached (on); releasing one is assigning it a fresh value.
// the loop itself (tum_sim_create): settings, plant / estimator / planner state, logs, the disturbance realisation played back
struct SimCore {
    int n_track = 0, loop_circuit = 0, n_elem = 0, step = 0, log_cap = 0, win[8] = {};
    double Tp = 0, Ts = 0;
    DevBuf<double> track, xsim, pose, hist, ref0, lCiLX, lSimX, lU, lREF, lDBG;
    DevBuf<int> closest, err, step_counter;
    DevBuf<double> dw, de; int dist_len = 0;          // (tum_sim_set_disturbances)
    // the generator that draws the realisation instead (tum_sim_disturbances_attach): kinds, magnitudes and seed as the kernel takes
    // them, and the one-step slab (batch x 7 per stream that is on) a control step draws into and its plant step reads
    bool gen_on = false; DistArgs gen{}; DevBuf<double> slab_w, slab_e;
    // the track set (tum_sim_create_tracks): `track` holds the tables one behind the other, rows[t] is the first row of track t
    // (n_tracks + 1 entries), track_of[b] the track of instance b. One track (tum_sim_create): rows = {0, n_track}, track_of all 0 and
    // NO device copies -- the kernels take their single-track path on the null pointers. n_track is the row count of the whole table.
    int n_tracks = 1; std::vector<int> rows, track_of; DevBuf<int> d_rows, d_track_of;
    int rows_of(size_t b) const { const int t = track_of[b]; return rows[t + 1] - rows[t]; }          // length of instance b's own track
};
// segment scoring (tum_sim_segments_attach): end index and accumulators per instance, groups of contiguous instances
struct SimSegments {
    bool on = false; int groups = 0; double max_lat = 0, max_acomb = 0;
    DevBuf<int> end, off, steps, state, qpf;
    DevBuf<double> lat, ssq, acomb, ggv, out;
};
// RL environment (tum_sim_env_attach): the settings as the kernels take them, the table / indices / bounds and the per-instance state
// on the device, pinned staging of the one upload and the one download of an environment step, and which episodes have ended (host)
struct SimEnv {
    bool on = false; int mpc_steps = 0, rec = 0; EnvArgs a{};
    DevBuf<double> table, bounds, acc, win, out;
    DevBuf<int> idx, in, ep, count, flags, qpf, samples;
    PinBuf<double> hout; PinBuf<int> hin; std::vector<unsigned char> ended;
};
// one net of the agent in the order policy_kernel reads it (tum_sim_policy_attach, tum_sim_policy_attach_value), and its true widths
struct SimNet {
    bool on = false; PolicyArgs a{};
    DevBuf<double> W[POL_MAXMAT], b[POL_MAXMAT]; int widths[POL_MAXMAT + 1] = {};
};
// with the policy net: its input inside a rollout, the live flags and their counter; the device-side log of a rollout
// (tum_sim_env_rollout: records, then actions | live | start table), grown on demand
struct SimRollout { DevBuf<double> obs, log; DevBuf<int> live, n_live, ints; };
// with the value net: the value of a step's own observation and the episode-start flags of a collection's first step; the device-side
// buffer of a collection with its start table (tum_sim_env_collect), grown on demand, and the rows the last collection left in it
struct SimCollect { DevBuf<double> term, starts, buf; DevBuf<int> tab; size_t rows = 0; };
// the trainer (tum_sim_ppo_attach): the settings and Adam's step counter, the training views of the nets as the kernels take them and the
// owners of what those views add (transposed matrices; activations and deltas of a minibatch), the float32 master / moments / gradient over
// the flat parameter vector (policy net then value net), and workspaces grown on demand: row records, diagnostics, an uploaded buffer, index lists
struct SimTrainer {
    bool on = false; double clip = 0, ent = 0, vf = 0, max_norm = 0; int normalize = 0, P = 0, parts = 0; long long t = 0;
    PpoNet net[2] = {};
    struct Layers { DevBuf<double> WT[POL_MAXMAT], h[POL_MAXMAT], d[POL_MAXMAT]; } layers[2];
    DevBuf<float> theta; DevBuf<double> m, v, G, part, advstat, rowrec, stats, data; DevBuf<int> idx;
};

// the learned weight schedule (tum_sim_wmpc_attach): the settings as the kernel takes them, the table / indices / bounds, the snapshot of
// W and the penalties, and per instance the step of the last decision, the decision count and the decision log
struct SimWmpc {
    bool on = false; int n_obs = 0; size_t lds = 0; WmpcArgs a{};
    DevBuf<double> table, bounds, base_W, base_pen, log_obs;
    DevBuf<int> idx, since, n_dec, log_step, log_act, act;
};

struct tum_sim {
    tum_ocp *c = nullptr;
    SimCore core;
    hipGraphExec_t graph = nullptr; int graph_steps = 0;            // captured chunk of control steps (tum_sim_run)
    unsigned graph_epoch = 0; bool graph_fanout = false;            // configuration of the capsule the chunk was captured with
    hipStream_t s2 = nullptr; hipEvent_t evF = nullptr, evJ = nullptr;          // side stream of the linearisation that runs beside the planner, fork / join events
    SimSegments seg; SimEnv env;
    SimNet pol, val; SimRollout roll; SimCollect col; SimTrainer ppo;          // (env_release and the chain behind it: sim_rl.hpp)
    SimWmpc wm;                                                                // (stands on the policy: policy_release drops it)
};

// a captured chunk holds kernel arguments and launches by value: whoever changes one of them drops it (the loop's stream is idle)
static void graph_drop(tum_sim *s) { if (s->graph) { (void)hipGraphExecDestroy(s->graph); s->graph = nullptr; } }

// a new evaluation: accumulators and state words of every segment back to zero (fills on the NULL stream: the caller synchronises)
static int seg_zero(tum_sim *s)
{
    const size_t B = s->c->batch; SimSegments &g = s->seg;
    HIPCHK(hipMemset(g.steps.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(g.state.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(g.qpf.get(), 0, sizeof(int) * B));
    HIPCHK(hipMemset(g.lat.get(), 0, sizeof(double) * B)); HIPCHK(hipMemset(g.ssq.get(), 0, sizeof(double) * B)); HIPCHK(hipMemset(g.acomb.get(), 0, sizeof(double) * B));
    return 0;
}

// What the loop does for an attached environment (sim_rl.hpp): it zeroes its counters with the state, scores every control step, and
// serves its per-instance words.
// episode counters, step accumulators, flags and the estimator's sample numbers back to zero (fills on the NULL stream: the caller synchronises)
static int env_zero(tum_sim *s)
{
    const size_t B = s->c->batch; SimEnv &v = s->env;
    HIPCHK(hipMemset(v.ep.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(v.count.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(v.flags.get(), 0, sizeof(int) * B));
    HIPCHK(hipMemset(v.qpf.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(v.samples.get(), 0, sizeof(int) * B));
    HIPCHK(hipMemset(v.acc.get(), 0, sizeof(double) * B * 4));
    std::fill(v.ended.begin(), v.ended.end(), 0);
    return 0;
}
// the capsule's arrays as they are NOW (tum_ocp_bind_device moves x0 / yref; a captured chunk is dropped with the epoch then)
static void env_bind(tum_sim *s)
{
    tum_ocp *c = s->c; EnvArgs &a = s->env.a;
    a.X = c->dX; a.U = c->dU; a.x0 = c->dx0; a.W = c->dW; a.pen = c->dpen; a.qp_lam = c->dqplam; a.yref = c->dyref; a.status = c->dstatus;
}
static int env_get(tum_sim *s, const std::string &f, double *out, long long len)
{
    const long long B = s->c->batch; const SimEnv &v = s->env;
    if (!v.on) return fail("sim_get " + f + ": no environment attached (tum_sim_env_attach)");
    if (len != B) return fail("sim_get " + f + ": len != batch");
    if (f == "env_ended") { for (long long i = 0; i < B; i++) out[i] = v.ended[i]; return 0; }
    const int *src = f == "env_episode_steps" ? v.ep.get() : f == "env_step_length" ? v.count.get() : f == "env_flags" ? v.flags.get() :
                     f == "env_qp_failures" ? v.qpf.get() : f == "env_samples" ? v.samples.get() : nullptr;
    if (!src) return fail("sim_get: unknown field '" + f + "'");
    return fetch_ints(src, B, out);
}

// What the loop does for an attached weight schedule (sim_rl.hpp): it refuses what the schedule cannot run on, at attach time and
// again at every run (a capsule can change behind an attached schedule), and launches its kernel behind every solve.
static int wmpc_refuse(const tum_sim *s, const char *who)
{
    const tum_ocp *c = s->c;
    const std::string w(who);
    if (s->env.on) return fail(w + ": this loop is an RL environment (tum_sim_env_attach), which installs the weights by its own rules; detach it first");
    if (c->dWf) return fail(w + ": the weight schedule installs a diagonal W (update_cost_function_weights); this capsule keeps a full W");
    if (c->nlp_type) return fail(w + ": the weight schedule runs behind one SQP-RTI iteration per control step; this capsule is in SQP mode (nlp_solver_type 1)");
    if (c->rti_phase) return fail(w + ": the weight schedule runs behind whole SQP-RTI steps; this capsule splits them (rti_phase 1 / 2): set rti_phase 0");
    if (c->kmode == KMode::FUSED || (c->ka.flags & KF_DEBUG)) return fail(w + ": the weight schedule runs on the pipeline, not on the development kernel 'fused'");
    return 0;
}
// the schedule's kernel behind the solve that is on the stream (the capsule's arrays as they are NOW, as env_bind takes them)
static int wmpc_enqueue(tum_sim *s)
{
    tum_ocp *c = s->c; SimWmpc &m = s->wm; WmpcArgs &a = m.a;
    invalidate(c, CH_W | CH_BOUNDS);          // (what the kernel may write: W and the slack penalties)
    a.x0 = c->dx0; a.yref = c->dyref; a.status = c->dstatus; a.W = c->dW; a.pen = c->dpen;
    LAUNCH(wmpc_schedule_kernel, dim3((c->batch + POL_TILE - 1) / POL_TILE), dim3(64 * POL_WAVES), m.lds, c->stream, a);
    return 0;
}
// a new run of the loop (tum_sim_set_state zeroes the step counter): no decision yet, the counters at 0, an empty log
static int wmpc_zero(tum_sim *s)
{
    const size_t B = s->c->batch; SimWmpc &m = s->wm; const size_t L = (size_t)m.a.log_cap * B;
    HIPCHK(hipMemset(m.since.get(), 0, sizeof(int) * B)); HIPCHK(hipMemset(m.n_dec.get(), 0, sizeof(int) * B));
    if (L) {
        HIPCHK(hipMemset(m.log_step.get(), 0xff, sizeof(int) * L)); HIPCHK(hipMemset(m.log_act.get(), 0xff, sizeof(int) * L));
        HIPCHK(hipMemset(m.log_obs.get(), 0, sizeof(double) * L * m.n_obs));
    }
    return 0;
}

// what a track set must satisfy (tum_sim_create_tracks, tum_planner_emulate_tracks): ascending offsets from 0, at least 2 rows per
// track, one track id in 0 .. n_tracks - 1 per instance, in any order
static int track_set_check(const std::string &w, const int *track_rows, int n_tracks, const int *track_of, size_t count)
{
    if (!track_rows || !track_of) return fail("null argument");
    if (n_tracks < 1) return fail(w + ": n_tracks < 1");
    if (track_rows[0] != 0) return fail(w + ": track_rows must start at 0");
    for (int t = 0; t < n_tracks; t++)
        if (track_rows[t + 1] - track_rows[t] < 2)
            return fail(w + ": track_rows must ascend and every track needs at least 2 rows (track " + std::to_string(t) + ")");
    for (size_t b = 0; b < count; b++)
        if (track_of[b] < 0 || track_of[b] >= n_tracks)
            return fail(w + ": track_of[" + std::to_string(b) + "] = " + std::to_string(track_of[b]) + " is outside 0.." + std::to_string(n_tracks - 1));
    return 0;
}

static int planner_emulate(const double *track, int n_track, const int *track_rows, int n_tracks, const int *track_of, const double *pose, int P,
                           int n_points, double Tp, int loop_circuit, double *ref_out, int *closest_out, int device)
{
    if (!track || !pose || !ref_out) return fail("null argument");
    if (n_track < 2 || P < 1 || n_points < 2) return fail("planner_emulate: bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device: libtumnmpc has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("planner_emulate: device ordinal out of range");
    DevGuard guard(device); GUARD_OK(guard);
    DevBuf<double> tt, tp, tout; DevBuf<int> tcl, terr, tof, trows;
    if (track_of) {
        HIPCHK(tof.alloc(P, false)); HIPCHK(trows.alloc((size_t)n_tracks + 1, false));
        HIPCHK(hipMemcpy(tof.get(), track_of, sizeof(int) * P, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(trows.get(), track_rows, sizeof(int) * ((size_t)n_tracks + 1), hipMemcpyHostToDevice));
    }
    HIPCHK(tt.alloc((size_t)4 * n_track, false)); HIPCHK(tp.alloc((size_t)2 * P, false));
    HIPCHK(tout.alloc((size_t)4 * P * n_points, false)); HIPCHK(tcl.alloc(P, false)); HIPCHK(terr.alloc(1, false));
    HIPCHK(hipMemset(terr.get(), 0, sizeof(int)));
    HIPCHK(hipMemcpy(tt.get(), track, sizeof(double) * 4 * n_track, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tp.get(), pose, sizeof(double) * 2 * P, hipMemcpyHostToDevice));
    LAUNCH(planner_kernel, dim3(P), dim3(64), 0, 0, tt.get(), n_track, tp.get(), 2, n_points, Tp, loop_circuit, tout.get(), 4, (double *)nullptr,
           tcl.get(), terr.get(), P, (int *)nullptr, (const int *)tof.get(), (const int *)trows.get());
    HIPCHK(hipDeviceSynchronize());
    int err = 0;
    HIPCHK(hipMemcpy(&err, terr.get(), sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ref_out, tout.get(), sizeof(double) * 4 * (size_t)P * n_points, hipMemcpyDeviceToHost));
    if (closest_out) HIPCHK(hipMemcpy(closest_out, tcl.get(), sizeof(int) * P, hipMemcpyDeviceToHost));
    if (err) return fail("planner_emulate: extracted segment longer than PLAN_MAXM points");
    return 0;
}
extern "C" int tum_planner_emulate(const double *track, int n_track, const double *pose, int P, int n_points, double Tp,
                                   int loop_circuit, double *ref_out, int *closest_out, int device)
{
    return planner_emulate(track, n_track, nullptr, 1, nullptr, pose, P, n_points, Tp, loop_circuit, ref_out, closest_out, device);
}
extern "C" int tum_planner_emulate_tracks(const double *tracks, const int *track_rows, int n_tracks, const int *track_of, const double *pose,
                                          int P, int n_points, double Tp, int loop_circuit, double *ref_out, int *closest_out, int device)
{
    if (P < 1) return fail("planner_emulate: bad sizes");
    if (track_set_check("planner_emulate_tracks", track_rows, n_tracks, track_of, P)) return 1;
    return planner_emulate(tracks, track_rows[n_tracks], track_rows, n_tracks, track_of, pose, P, n_points, Tp, loop_circuit, ref_out,
                           closest_out, device);
}

// (the owners free with the loop: all of it under the capsule's device)
extern "C" void tum_sim_free(tum_sim *s)
{
    if (!s) return;
    DevGuard guard(s->c->d.device);
    graph_drop(s);
    if (s->s2) { (void)hipStreamSynchronize(s->s2); (void)hipStreamDestroy(s->s2); (void)hipEventDestroy(s->evF); (void)hipEventDestroy(s->evJ); }
    delete s;
}

// track_of == NULL: one track of n_track rows (tum_sim_create); else the set (checked by the caller), n_track = track_rows[n_tracks]
static tum_sim *sim_create(tum_ocp *c, const double *track, int n_track, const int *track_rows, int n_tracks, const int *track_of, double Tp,
                           int loop_circuit, double Ts, int n_elem, const int *windows, int log_capacity)
{
    if (!c || !track || !windows) { fail("null argument"); return nullptr; }
    if (n_track < 2 || !(Tp > 0) || !(Ts > 0) || n_elem < 1 || log_capacity < 0) { fail("sim_create: bad arguments"); return nullptr; }
    for (int i = 0; i < 8; i++) if (windows[i] < 1 || windows[i] > 4) { fail("sim_create: estimator windows must be 1..4"); return nullptr; }
    if (c->nlp_type) { fail("sim_create: the device closed loop runs one SQP-RTI iteration per control step; this capsule is in SQP mode (nlp_solver_type 1)"); return nullptr; }
    if (c->rti_phase) { fail("sim_create: the device closed loop runs whole SQP-RTI steps; this capsule splits them (rti_phase 1 / 2): set rti_phase 0"); return nullptr; }
    DevGuard guard(c->d.device); if (!guard.ok) { fail("hipSetDevice failed"); return nullptr; }
    if (c->sn) {   // the state estimator writes the nominal x0 only: the samples follow by fan-out
        if (!c->have_offs) { fail("sim_create: an SNMPC capsule needs its sample offsets (tum_ocp_snmpc_set_offsets)"); return nullptr; }
        c->fanout = true;
    }
    tum_sim *s = new tum_sim();
    SimCore &k = s->core;
    s->c = c; k.n_track = n_track; k.loop_circuit = loop_circuit; k.n_elem = n_elem; k.Tp = Tp; k.Ts = Ts; k.log_cap = log_capacity;
    for (int i = 0; i < 8; i++) k.win[i] = windows[i];
    const size_t B = c->batch, L = log_capacity;
    bool ok = true;
    if (track_of) {
        k.n_tracks = n_tracks; k.rows.assign(track_rows, track_rows + n_tracks + 1); k.track_of.assign(track_of, track_of + B);
        ok &= k.d_rows.alloc(k.rows.size()) == hipSuccess && k.d_track_of.alloc(B) == hipSuccess;
        ok = ok && hipMemcpy(k.d_rows.get(), k.rows.data(), sizeof(int) * k.rows.size(), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(k.d_track_of.get(), k.track_of.data(), sizeof(int) * B, hipMemcpyHostToDevice) == hipSuccess;
    } else { k.rows = {0, n_track}; k.track_of.assign(B, 0); }
    ok &= k.track.alloc((size_t)4 * n_track) == hipSuccess;
    ok &= k.xsim.alloc(B * 7) == hipSuccess && k.pose.alloc(B * 2) == hipSuccess && k.hist.alloc(B * 32) == hipSuccess;
    ok &= k.ref0.alloc(B * 4) == hipSuccess && k.closest.alloc(B) == hipSuccess && k.err.alloc(1) == hipSuccess && k.step_counter.alloc(2) == hipSuccess;
    if (L > 0) {
        ok &= k.lCiLX.alloc((L + 1) * B * 7) == hipSuccess && k.lSimX.alloc((L + 1) * B * 8) == hipSuccess;
        ok &= k.lU.alloc(L * B * 2) == hipSuccess && k.lREF.alloc(L * B * 4) == hipSuccess && k.lDBG.alloc(L * B * 5) == hipSuccess;
    }
    ok = ok && hipMemcpy(k.track.get(), track, sizeof(double) * 4 * n_track, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { fail("sim_create: device allocation failed"); tum_sim_free(s); return nullptr; }
    return s;
}
extern "C" tum_sim *tum_sim_create(tum_ocp *c, const double *track, int n_track, double Tp, int loop_circuit, double Ts, int n_elem,
                                   const int *windows, int log_capacity)
{
    return sim_create(c, track, n_track, nullptr, 1, nullptr, Tp, loop_circuit, Ts, n_elem, windows, log_capacity);
}
extern "C" tum_sim *tum_sim_create_tracks(tum_ocp *c, const double *tracks, const int *track_rows, int n_tracks, const int *track_of, double Tp,
                                          int loop_circuit, double Ts, int n_elem, const int *windows, int log_capacity)
{
    if (!c) { fail("null argument"); return nullptr; }
    if (track_set_check("sim_create_tracks", track_rows, n_tracks, track_of, c->batch)) return nullptr;
    return sim_create(c, tracks, track_rows[n_tracks], track_rows, n_tracks, track_of, Tp, loop_circuit, Ts, n_elem, windows, log_capacity);
}

// initial plant state (batch x 7) and controller state (batch x 8): X0_sim / X0_MPC of SimulationMode_main_class.py:60-75
extern "C" int tum_sim_set_state(tum_sim *s, const double *x_sim, const double *x_mpc, int cold_start)
{
    if (!s || !x_sim || !x_mpc) return fail("null argument");
    tum_ocp *c = s->c; const size_t B = c->batch; SimCore &k = s->core;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    invalidate(c, CH_X0 | CH_REF | CH_UPLOAD);
    if (flush_inputs(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(k.xsim.get(), x_sim, sizeof(double) * B * 7, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->dx0, x_mpc, sizeof(double) * B * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy2D(k.pose.get(), 2 * 8, x_mpc, 8 * 8, 2 * 8, B, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(k.hist.get(), 0, sizeof(double) * B * 32));
    HIPCHK(hipMemset(k.step_counter.get(), 0, 2 * sizeof(int)));
    if (s->seg.on && seg_zero(s)) return 1;
    if (s->env.on && env_zero(s)) return 1;
    if (s->wm.on && wmpc_zero(s)) return 1;
    HIPCHK(hipDeviceSynchronize());          // (the fills run on the NULL stream, the loop on the capsule's non-blocking one)
    k.step = 0;
    if (k.log_cap > 0) {
        HIPCHK(hipMemcpy(k.lCiLX.get(), x_sim, sizeof(double) * B * 7, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(k.lSimX.get(), x_mpc, sizeof(double) * B * 8, hipMemcpyHostToDevice));
    }
    if (cold_start) return tum_ocp_cold_start(c);
    return 0;
}

extern "C" int tum_sim_plan(tum_sim *s)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c; const SimCore &k = s->core;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;
    invalidate(c, CH_REF);
    LAUNCH(planner_kernel, dim3(c->batch), dim3(64), 0, c->stream, k.track.get(), k.n_track, k.pose.get(), 2, c->N + 1, k.Tp,
           k.loop_circuit, c->dyref, 6, k.ref0.get(), k.closest.get(), k.err.get(), c->batch, (int *)nullptr,
           (const int *)k.d_track_of.get(), (const int *)k.d_rows.get());
    return 0;
}

extern "C" int tum_sim_advance(tum_sim *s)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c; SimCore &k = s->core;
    if (!c->solved) return fail("sim_advance: no solve yet");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    invalidate(c, CH_ITERATE | CH_X0);          // (the plant re-initialises the iterate of an instance whose solve failed, and writes the next x0)
    if (flush_inputs(c)) return 1;
    SimArgs sa{};
    sa.N = c->N; sa.batch = c->batch; sa.n_elem = k.n_elem; sa.step_counter = k.step_counter.get(); sa.log_cap = k.log_cap; sa.Ts = k.Ts;
    for (int i = 0; i < 8; i++) sa.win[i] = k.win[i];
    vehicle_constants(sa.pm, c->d);
    sa.X = c->dX; sa.U = c->dU; sa.cost = c->dcost; sa.status = c->dstatus; sa.qp_iter = c->dqpiter;
    sa.ns = c->sn ? c->sa.ns : 0; sa.XS = c->dXS; sa.xs0 = c->dxs0;
    sa.bnd = c->dbnd; sa.r2 = c->r2 ? 1 : 0; sa.r2_dmin = c->r2_dmin; sa.r2_dmax = c->r2_dmax; sa.r2_uh = c->r2_uh;
    sa.x_sim = k.xsim.get(); sa.x0 = c->dx0; sa.pose = k.pose.get(); sa.hist = k.hist.get(); sa.ref0 = k.ref0.get();
    sa.lCiLX = k.lCiLX.get(); sa.lSimX = k.lSimX.get(); sa.lU = k.lU.get(); sa.lREF = k.lREF.get(); sa.lDBG = k.lDBG.get();
    sa.dist_w = k.dw.get(); sa.dist_e = k.de.get(); sa.dist_len = k.dist_len;
    if (k.gen_on) {
        // the realisation of THIS step, drawn into the slab in front of the plant: the step comes from the loop's counter on the
        // device (a captured chunk replays with constant arguments). Here, not in sim_enqueue_step_body, so that a loop driven by
        // tum_sim_plan / solve / tum_sim_advance draws as well
        DistArgs da = k.gen;
        da.batch = c->batch; da.n_steps = 1; da.step_counter = k.step_counter.get(); da.out[0] = k.slab_w.get(); da.out[1] = k.slab_e.get();
        LAUNCH(disturbance_draw_kernel, dim3((c->batch + 63) / 64, 2), dim3(64), 0, c->stream, da);
        sa.dist_w = k.slab_w.get(); sa.dist_e = k.slab_e.get(); sa.dist_len = 0; sa.dist_live = 1;
    }
    sa.samples = s->env.samples.get();          // (null without an environment)
    LAUNCH(plant_advance_kernel, dim3((c->batch * PLANT_LANES + 63) / 64), dim3(64), 0, c->stream, sa);
    k.step++;
    return 0;
}

// scores the control step whose solve is on the stream and whose plant step is not yet (tum_sim_segments_attach)
static int sim_enqueue_segment_score(tum_sim *s)
{
    tum_ocp *c = s->c; const SimSegments &g = s->seg;
    SegArgs a{};
    a.N = c->N; a.batch = c->batch; a.n_ggv = c->d.n_ggv;
    a.X = c->dX; a.status = c->dstatus; a.x_sim = s->core.xsim.get(); a.ref0 = s->core.ref0.get(); a.closest = s->core.closest.get();
    a.end_idx = g.end.get(); a.ggv = g.ggv.get();
    a.acc_min = c->d.acc_min; a.max_lat_dev = g.max_lat; a.max_a_comb = g.max_acomb;
    a.steps = g.steps.get(); a.state = g.state.get(); a.qp_failures = g.qpf.get();
    a.max_abs_lat = g.lat.get(); a.sumsq_vel = g.ssq.get(); a.max_acomb = g.acomb.get();
    LAUNCH(segment_score_kernel, dim3((c->batch + 63) / 64), dim3(64), 0, c->stream, a);
    return 0;
}
static int sim_enqueue_step_body(tum_sim *s, bool events)
{
    tum_ocp *c = s->c;
    if (lin_ahead_ok(c)) {
        // fork: the linearisation of this step's solve on the side stream, behind everything the capsule's stream holds (the plant
        // of the previous step may have re-initialised the iterate); the planner on the capsule's stream; join in front of the
        // condensing kernel. Inside a stream capture this becomes two branches of the graph.
        HIPCHK(hipEventRecord(s->evF, c->stream));
        HIPCHK(hipStreamWaitEvent(s->s2, s->evF, 0));
        launch_lin_ahead(c, s->s2);
        HIPCHK(hipEventRecord(s->evJ, s->s2));
        if (tum_sim_plan(s)) return 1;
        HIPCHK(hipStreamWaitEvent(c->stream, s->evJ, 0));
    } else if (tum_sim_plan(s)) return 1;
    if (launch(c, events)) return 1;
    if (s->seg.on && sim_enqueue_segment_score(s)) return 1;
    if (s->env.on) {          // scores the control step whose solve is on the stream and whose plant step is not yet (tum_sim_env_attach)
        env_bind(s);
        LAUNCH(env_score_kernel, dim3(c->batch), dim3(64), 0, c->stream, s->env.a);
    }
    if (s->wm.on && wmpc_enqueue(s)) return 1;          // the learned weight schedule, in the same place (tum_sim_wmpc_attach)
    return tum_sim_advance(s);
}
static int sim_enqueue_step(tum_sim *s, bool events)
{
    // whatever goes wrong between the forked linearisation and the solve that consumes it (planner, join, a failed capture): the
    // capsule must not keep the "linearisation already done" mark for a LATER solve, which would run on stale stage records
    const int rc = sim_enqueue_step_body(s, events);
    if (rc) s->c->lin_ahead = false;
    return rc;
}

// nsteps x (planner, SQP-RTI solve, plant + estimator) on the capsule's stream; returns after the last one. The loop is
// launch-bound for small batches (3 short kernels per control step), so chunks of GRAPH_STEPS steps are captured once into
// a hipGraph and replayed; all per-step state (step counter, ring buffers, logs) lives in device memory, so the captured
// kernel arguments never change.
static const int GRAPH_STEPS = 25;
// the control steps of tum_sim_run on the capsule's stream, without the wait behind them
static int sim_run_enqueue(tum_sim *s, int nsteps)
{
    tum_ocp *c = s->c;
    if (c->nlp_type) return fail("sim_run: the device closed loop runs one SQP-RTI iteration per control step; this capsule is in SQP mode (nlp_solver_type 1)");
    if (c->rti_phase) return fail("sim_run: the device closed loop runs whole SQP-RTI steps; this capsule splits them (rti_phase 1 / 2): set rti_phase 0");
    if (s->wm.on && wmpc_refuse(s, "sim_run")) return 1;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    invalidate(c, CH_ITERATE);          // (the closed loop keeps the general linearisation: its chunks are captured and replayed)
    if (flush_inputs(c)) return 1;            // (pending host setters go up before anything is captured)
    if (resolve_kernel(c)) return 1;          // (workspace allocation must not happen inside the capture below)
    // ... nor the reallocation / synchronisation a changed SNMPC parameter vector can trigger, nor the deferred freeze
    if (c->sn && (sn_apply_p(c) || sn_materialise(c))) return 1;
    if (lin_ahead_ok(c) && !s->s2) {          // (created here: not inside the capture below)
        HIPCHK(hipStreamCreateWithFlags(&s->s2, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s->evF, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&s->evJ, hipEventDisableTiming));
    }
    int done = 0;
    if (nsteps >= 2 * GRAPH_STEPS) {
        // a captured chunk holds the kernel variant, the schedule flag, the SNMPC horizon / risk parameter / work-buffer
        // pointers and the R2 attachment BY VALUE: after any of them changed the chunk is captured again
        if (s->graph_epoch != c->epoch || s->graph_fanout != c->fanout) graph_drop(s);
        if (!s->graph) {
            s->graph_epoch = c->epoch; s->graph_fanout = c->fanout;
            hipGraph_t g = nullptr;
            const int step0 = s->core.step;
            bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            c->capturing = ok;
            if (ok) {
                c->solved = true;                                      // the captured solve precedes every captured advance
                for (int i = 0; i < GRAPH_STEPS && ok; i++) ok = sim_enqueue_step(s, false) == 0;
                ok = (hipStreamEndCapture(c->stream, &g) == hipSuccess) && ok;
                c->capturing = false;
                s->core.step = step0;                                  // nothing ran yet
            }
            if (ok && g) ok = hipGraphInstantiate(&s->graph, g, nullptr, nullptr, 0) == hipSuccess;
            if (g) (void)hipGraphDestroy(g);
            if (!ok) { s->graph = nullptr; c->lin_ahead = false; (void)hipGetLastError(); }  // fall back to plain launches
            s->graph_steps = GRAPH_STEPS;
        }
        while (s->graph && nsteps - done >= s->graph_steps) {
            HIPCHK(hipGraphLaunch(s->graph, c->stream));
            done += s->graph_steps; s->core.step += s->graph_steps;
            if (solve_done(c, SOLVE_REPLAY, false)) return 1;
        }
    }
    for (; done < nsteps; done++)
        if (sim_enqueue_step(s, true)) return 1;
    return 0;
}

extern "C" int tum_sim_run(tum_sim *s, int nsteps)
{
    if (!s || nsteps < 0) return fail("bad argument");
    tum_ocp *c = s->c;
    if (sim_run_enqueue(s, nsteps)) return 1;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    int err = 0;
    HIPCHK(hipMemcpy(&err, s->core.err.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (err) return fail("sim_run: planner segment longer than PLAN_MAXM points");
    return 0;
}

extern "C" int tum_sim_steps(const tum_sim *s) { return s ? s->core.step : -1; }

static void gen_release(SimCore &k) { k.gen_on = false; k.gen = DistArgs{}; k.slab_w.reset(); k.slab_e.reset(); }

// Disturbance realisation of the loop (Utils/SimulationMode_main_class.py:121-143 with disturbance_playback, and what
// Utils/MPC_sim_utils.py:54-67 generate_disturbances draws otherwise -- drawn on the host, closed_loop.DisturbanceModel): w_deriv
// (additive on the state derivatives, constant over a control step) and e_est (additive state estimation error), n_steps x batch x 7
// each (host, step-major), either may be null. Control step i >= n_steps runs undisturbed. n_steps = 0 removes the realisation.
extern "C" int tum_sim_set_disturbances(tum_sim *s, const double *w_deriv, const double *e_est, int n_steps)
{
    if (!s || n_steps < 0) return fail("bad argument");
    tum_ocp *c = s->c; SimCore &k = s->core;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    k.dw.reset(); k.de.reset(); k.dist_len = 0;
    graph_drop(s);          // (the pointers are kernel arguments of a captured chunk)
    if (n_steps > 0 && (w_deriv || e_est)) gen_release(k);          // (a table takes the generator's place)
    if (n_steps == 0 || (!w_deriv && !e_est)) return 0;
    const size_t n = (size_t)n_steps * c->batch * 7;
    if (w_deriv) { HIPCHK(k.dw.alloc(n, false)); HIPCHK(hipMemcpy(k.dw.get(), w_deriv, sizeof(double) * n, hipMemcpyHostToDevice)); }
    if (e_est) { HIPCHK(k.de.alloc(n, false)); HIPCHK(hipMemcpy(k.de.get(), e_est, sizeof(double) * n, hipMemcpyHostToDevice)); }
    k.dist_len = n_steps;
    return 0;
}

// The same realisation DRAWN on the device (disturbance_kernels.hpp; the definition of a draw: include/tum_nmpc.h): kind 0 switches a
// stream off, 1..4 are 'uniform' (the ellipsoid), 'gaussian', 'absolute' and the box; both 0 detaches. A generator and a played-back
// table exclude each other: attaching one removes the other.
extern "C" int tum_sim_disturbances_attach(tum_sim *s, int kind_w, const double *bound_w, int kind_e, const double *bound_e, unsigned long long seed)
{
    if (!s) return fail("null argument");
    const int kinds[2] = {kind_w, kind_e}; const double *bounds[2] = {bound_w, bound_e};
    for (int q = 0; q < 2; q++) {
        const std::string who = q ? "state estimation error" : "derivative disturbance";
        if (kinds[q] < DIST_OFF || kinds[q] > DIST_BOX)
            return fail("disturbances_attach: kind " + std::to_string(kinds[q]) + " of the " + who + " is outside 0..4 (off, uniform, gaussian, absolute, box)");
        if (kinds[q] == DIST_OFF) continue;
        if (!bounds[q]) return fail("disturbances_attach: the " + who + " is on and has no bounds");
        for (int i = 0; i < 7; i++)
            if (!(bounds[q][i] >= 0.0) || std::isinf(bounds[q][i]))
                return fail("disturbances_attach: bound " + std::to_string(i) + " of the " + who + " is negative or not finite");
    }
    tum_ocp *c = s->c; SimCore &k = s->core; const size_t B = c->batch;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    graph_drop(s);          // (a captured chunk holds the extra launch, or lacks it)
    gen_release(k);
    if (kind_w == DIST_OFF && kind_e == DIST_OFF) return 0;
    k.dw.reset(); k.de.reset(); k.dist_len = 0;          // (the generator takes a table's place)
    bool ok = true;
    if (kind_w != DIST_OFF) ok &= k.slab_w.alloc(B * 7) == hipSuccess;
    if (kind_e != DIST_OFF) ok &= k.slab_e.alloc(B * 7) == hipSuccess;
    if (!ok) { gen_release(k); (void)hipGetLastError(); return fail("disturbances_attach: device allocation failed"); }
    k.gen.seed = seed;
    for (int q = 0; q < 2; q++) {
        k.gen.kind[q] = kinds[q];
        for (int i = 0; i < 7 && kinds[q] != DIST_OFF; i++) { k.gen.bound[q][i] = bounds[q][i]; k.gen.root[q][i] = std::sqrt(bounds[q][i]); }
    }
    k.gen_on = true;
    return 0;
}

// The realisation of the control steps first_step .. first_step + n_steps - 1 as the attached generator draws it, n_steps x batch x 7
// doubles per stream (host, step-major), either output may be null; a stream that is off gives zeros. Drawn into a temporary table in
// chunks: the loop's step counter, slab and captured chunk are not touched.
extern "C" int tum_sim_disturbances_table(tum_sim *s, long long first_step, int n_steps, double *w_out, double *e_out)
{
    if (!s) return fail("null argument");
    if (first_step < 0 || n_steps < 0) return fail("disturbances_table: first_step < 0 or n_steps < 0");
    tum_ocp *c = s->c; const SimCore &k = s->core; const size_t B = c->batch;
    if (!k.gen_on) return fail("disturbances_table: no generator attached (tum_sim_disturbances_attach)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    double *outs[2] = {w_out, e_out};
    const int chunk = (int)std::max<size_t>(1, ((size_t)1 << 22) / (B * 7));          // steps per launch: 32 MB of table per stream
    DevBuf<double> tmp[2];
    for (int q = 0; q < 2; q++) {
        if (!outs[q]) continue;
        if (k.gen.kind[q] == DIST_OFF) { std::fill(outs[q], outs[q] + (size_t)n_steps * B * 7, 0.0); outs[q] = nullptr; continue; }
        HIPCHK(tmp[q].alloc((size_t)std::min(chunk, std::max(n_steps, 1)) * B * 7, false));
    }
    if (!outs[0] && !outs[1]) return 0;
    for (int done = 0; done < n_steps; done += chunk) {
        const int n = std::min(chunk, n_steps - done);
        DistArgs da = k.gen;
        da.batch = c->batch; da.n_steps = n; da.first_step = first_step + done; da.step_counter = nullptr;
        da.out[0] = outs[0] ? tmp[0].get() : nullptr; da.out[1] = outs[1] ? tmp[1].get() : nullptr;
        const size_t rows = (size_t)n * B;
        LAUNCH(disturbance_draw_kernel, dim3((unsigned)((rows + 63) / 64), 2), dim3(64), 0, c->stream, da);
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int q = 0; q < 2; q++)
            if (outs[q]) HIPCHK(hipMemcpy(outs[q] + (size_t)done * B * 7, tmp[q].get(), sizeof(double) * rows * 7, hipMemcpyDeviceToHost));
    }
    return 0;
}

// Track segments of a weight sweep (Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/objective_function.py:57-200): instance b is scored every control
// step until the planner's index equals end_idx[b] or a crash test fires; groups are contiguous runs of instances.
extern "C" int tum_sim_segments_attach(tum_sim *s, const int *end_idx, const int *group_offsets, int n_groups, double max_lat_dev, double max_a_comb)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c; const int B = c->batch;
    if (end_idx && s->env.on) return fail("segments_attach: this loop is an RL environment (tum_sim_env_attach): an instance is scored by one set of rules; detach the environment first");
    if (end_idx) {
        if (max_lat_dev != max_lat_dev || max_a_comb != max_a_comb) return fail("segments_attach: a threshold is NaN (an infinite one disables its crash test)");
        // on a track set an end index is a waypoint of the instance's OWN track: one past it (valid on a longer track of the set, say)
        // could never be reached. A single-track loop keeps taking any index, as it always has (one it cannot reach: never done)
        if (s->core.d_track_of.get())
            for (int b = 0; b < B; b++)
                if (end_idx[b] >= s->core.rows_of(b))
                    return fail("segments_attach: end index " + std::to_string(end_idx[b]) + " of instance " + std::to_string(b) + " is outside its own track (track " +
                                std::to_string(s->core.track_of[b]) + ", " + std::to_string(s->core.rows_of(b)) + " rows)");
        if (group_offsets) {
            if (n_groups < 1) return fail("segments_attach: n_groups < 1");
            if (group_offsets[0] != 0 || group_offsets[n_groups] != B) return fail("segments_attach: group_offsets must start at 0 and end at batch");
            for (int g = 0; g < n_groups; g++)
                if (group_offsets[g + 1] <= group_offsets[g]) return fail("segments_attach: group_offsets must increase (no empty group)");
        }
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    graph_drop(s);          // (a captured chunk holds the extra launch, or lacks it)
    s->seg = SimSegments{};
    if (!end_idx) return 0;
    std::vector<int> off;
    if (group_offsets) off.assign(group_offsets, group_offsets + n_groups + 1);
    else { n_groups = B; off.resize(B + 1); for (int i = 0; i <= B; i++) off[i] = i; }
    double ggv[48];
    for (int i = 0; i < 16; i++) { ggv[i] = c->d.ggv_v[i]; ggv[16 + i] = c->d.ggv_ax[i]; ggv[32 + i] = c->d.ggv_ay[i]; }
    SimSegments &g = s->seg;
    bool ok = true;
    ok &= g.end.alloc(B) == hipSuccess && g.off.alloc((size_t)n_groups + 1) == hipSuccess;
    ok &= g.steps.alloc(B) == hipSuccess && g.state.alloc(B) == hipSuccess && g.qpf.alloc(B) == hipSuccess;
    ok &= g.lat.alloc(B) == hipSuccess && g.ssq.alloc(B) == hipSuccess && g.acomb.alloc(B) == hipSuccess;
    ok &= g.ggv.alloc(48) == hipSuccess && g.out.alloc((size_t)4 * n_groups) == hipSuccess;
    ok = ok && hipMemcpy(g.end.get(), end_idx, sizeof(int) * B, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(g.off.get(), off.data(), sizeof(int) * (n_groups + 1), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(g.ggv.get(), ggv, sizeof(ggv), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { s->seg = SimSegments{}; (void)hipGetLastError(); return fail("segments_attach: device allocation failed"); }
    g.on = true; g.groups = n_groups; g.max_lat = max_lat_dev; g.max_acomb = max_a_comb;
    return 0;
}

// segments whose state word is still 0 (the loop's stream is idle)
static int seg_count_active(tum_sim *s, double *active)
{
    std::vector<double> st(s->c->batch);
    if (fetch_ints(s->seg.state.get(), st.size(), st.data())) return 1;
    *active = (double)std::count(st.begin(), st.end(), 0.0);
    return 0;
}

// tum_sim_run in chunks of check_every control steps until no segment is active or max_steps have run. The reference's
// `while not done and not crash` has no cap; segments still active at the end have timed out (neither done nor crashed).
extern "C" int tum_sim_run_segments(tum_sim *s, int max_steps, int check_every)
{
    if (!s || max_steps < 0) return fail("bad argument");
    if (!s->seg.on) return fail("sim_run_segments: no segments attached (tum_sim_segments_attach)");
    if (check_every <= 0) check_every = 100;
    DevGuard guard(s->c->d.device); GUARD_OK(guard);
    for (int done = 0; done < max_steps;) {
        const int n = std::min(check_every, max_steps - done);
        if (tum_sim_run(s, n)) return 1;
        done += n;
        double active = 0;
        if (seg_count_active(s, &active)) return 1;
        if (active == 0) break;
    }
    return 0;
}

static int seg_get(tum_sim *s, const std::string &f, double *out, long long len)
{
    tum_ocp *c = s->c; const long long B = c->batch; const SimSegments &g = s->seg;
    if (!g.on) return fail("sim_get " + f + ": no segments attached (tum_sim_segments_attach)");
    if (f == "seg_active") return len != 1 ? fail("sim_get seg_active: len != 1") : seg_count_active(s, out);
    if (f == "seg_groups") {
        if (len != 4LL * g.groups) return fail("sim_get seg_groups: len != 4 * n_groups");
        LAUNCH(segment_group_kernel, dim3(g.groups), dim3(64), 0, c->stream, g.off.get(), g.groups, g.steps.get(), g.state.get(), g.lat.get(), g.ssq.get(), g.out.get());
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(out, g.out.get(), sizeof(double) * len, hipMemcpyDeviceToHost));
        return 0;
    }
    if (len != B) return fail("sim_get " + f + ": len != batch");
    const int *isrc = f == "seg_steps" ? g.steps.get() : f == "seg_state" ? g.state.get() : f == "seg_qp_failures" ? g.qpf.get() : nullptr;
    if (isrc) return fetch_ints(isrc, B, out);
    if (f == "seg_max_lat_dev") { HIPCHK(hipMemcpy(out, g.lat.get(), sizeof(double) * B, hipMemcpyDeviceToHost)); return 0; }
    if (f == "seg_max_a_comb") { HIPCHK(hipMemcpy(out, g.acomb.get(), sizeof(double) * B, hipMemcpyDeviceToHost)); return 0; }
    if (f == "seg_rms_vel_dev") {          // sqrt(sumsq_vel / steps): get_root_mean_square of objective_function.py:184 (0 before the first step)
        std::vector<double> t(B);
        if (fetch_ints(g.steps.get(), B, t.data())) return 1;
        HIPCHK(hipMemcpy(out, g.ssq.get(), sizeof(double) * B, hipMemcpyDeviceToHost));
        for (long long i = 0; i < B; i++) out[i] = t[i] > 0 ? std::sqrt(out[i] / t[i]) : 0.0;
        return 0;
    }
    return fail("sim_get: unknown field '" + f + "'");
}

extern "C" int tum_sim_get(tum_sim *s, const char *field, double *out, long long len)
{
    if (!s || !field || !out) return fail("null argument");
    tum_ocp *c = s->c; const long long B = c->batch; const SimCore &k = s->core;
    const long long L = k.step < k.log_cap ? k.step : k.log_cap;
    const std::string f(field);
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (f.compare(0, 4, "seg_") == 0) return seg_get(s, f, out, len);
    if (f.compare(0, 4, "env_") == 0) return env_get(s, f, out, len);
    if (f == "graph_steps") {         // control steps per captured hipGraph chunk (0: plain launches)
        if (len != 1) return fail("sim_get graph_steps: len != 1");
        out[0] = s->graph ? s->graph_steps : 0;
        return 0;
    }
    if (f == "closest") return len != B ? fail("sim_get closest: len != batch") : fetch_ints(k.closest.get(), B, out);
    if (f == "track_of") {          // the track of every instance (all 0 on a single-track loop)
        if (len != B) return fail("sim_get track_of: len != batch");
        for (long long i = 0; i < B; i++) out[i] = k.track_of[i];
        return 0;
    }
    if (f == "track_rows") {        // first row of every track in the concatenated table, then the total: n_tracks + 1 values
        if (len != k.n_tracks + 1) return fail("sim_get track_rows: len != n_tracks + 1");
        for (long long i = 0; i <= k.n_tracks; i++) out[i] = k.rows[i];
        return 0;
    }
    const struct { const char *name; const double *src; long long want; } arrays[] = {
        {"x_sim", k.xsim.get(), B * 7}, {"x_mpc", c->dx0, B * 8}, {"pose", k.pose.get(), B * 2}, {"ref0", k.ref0.get(), B * 4},
        {"yref", c->dyref, B * (c->N + 1) * 6},          // (the reference window of the last planned step, [x, y, yaw, v, 0, 0] per point)
        {"CiLX", k.lCiLX.get(), (L + 1) * B * 7}, {"MPC_SimX", k.lSimX.get(), (L + 1) * B * 8}, {"simU", k.lU.get(), L * B * 2},
        {"simREF", k.lREF.get(), L * B * 4}, {"simSolverDebug", k.lDBG.get(), L * B * 5}};
    for (const auto &a : arrays) {
        if (f != a.name) continue;
        if (!a.src) return fail("sim_get: logging disabled (log_capacity 0)");
        if (len != a.want) return fail("sim_get " + f + ": len mismatch");
        if (a.want > 0) HIPCHK(hipMemcpy(out, a.src, sizeof(double) * a.want, hipMemcpyDeviceToHost));
        return 0;
    }
    return fail("sim_get: unknown field '" + f + "'");
}
