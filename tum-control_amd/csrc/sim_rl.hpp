// sim_rl.hpp -- host side of the RL layers on the device closed loop (sim_loop.hpp): the environment (K11), the agent and whole
// episodes (K12), collecting PPO training rollouts (K13) and the PPO update (K14). Host code only, included by tum_nmpc.hip.
#pragma once

// What is attached on top of what: the policy reads the environment's observation and writes its actions, the value net takes the
// policy's inputs, the trainer updates both nets. Detaching one detaches what stands on it, in this order.
static void ppo_release(tum_sim *s) { s->ppo = SimTrainer{}; }
static void value_release(tum_sim *s) { ppo_release(s); s->val = SimNet{}; s->col = SimCollect{}; }
static void wmpc_release(tum_sim *s) { s->wm = SimWmpc{}; }          // (the weight schedule of the controller classes runs the policy net)
static void policy_release(tum_sim *s) { value_release(s); wmpc_release(s); s->pol = SimNet{}; s->roll = SimRollout{}; }
static void env_release(tum_sim *s) { policy_release(s); s->env = SimEnv{}; }

// ---------------------------------------------------------------------------------------------- K11: RL environment
// what the environment cannot run on, at attach time and again at every step (a capsule can change behind an attached environment)
static int env_refuse(const tum_sim *s, const char *who)
{
    const tum_ocp *c = s->c;
    const std::string w(who);
    if (c->sn) return fail(w + ": the RL environment runs the nominal OCP; this is a coupled SNMPC capsule");
    if (c->r2) return fail(w + ": the RL environment runs the nominal OCP; this capsule has the R2 back-off attached (its reset restores bounds the environment does not know)");
    if (c->dWf) return fail(w + ": the RL environment installs a diagonal W (update_cost_function_weights); this capsule keeps a full W");
    if (c->nlp_type) return fail(w + ": the RL environment runs one SQP-RTI iteration per control step; this capsule is in SQP mode (nlp_solver_type 1)");
    if (c->rti_phase) return fail(w + ": the RL environment runs whole SQP-RTI steps; this capsule splits them (rti_phase 1 / 2): set rti_phase 0");
    if (c->kmode == KMode::FUSED || (c->ka.flags & KF_DEBUG)) return fail(w + ": the RL environment runs on the pipeline, not on the development kernel 'fused'");
    if (s->seg.on) return fail(w + ": this loop has track segments attached (tum_sim_segments_attach): an instance is scored by one set of rules; detach them first");
    return 0;
}

extern "C" int tum_sim_env_attach(tum_sim *s, const double *table, int n_actions, int n_mpc_steps, double max_lat_dev, int episode_length, int full_lap,
                                  const double *sigmas, const double *lims, const double *obs_lo, const double *obs_hi,
                                  const int *idx_v, const int *idx_yawrate, int n_samples, int obs_states)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c; const size_t B = c->batch; const int N = c->N;
    if (table) {
        if (!sigmas || !lims || !obs_lo || !obs_hi || !idx_v || !idx_yawrate) return fail("null argument");
        if (env_refuse(s, "env_attach")) return 1;
        if (s->wm.on) return fail("env_attach: this loop runs a learned weight schedule (tum_sim_wmpc_attach), which installs the weights by its own rule; detach it first");
        if (n_actions < 1 || n_mpc_steps < 1 || episode_length < 1 || n_samples < 1) return fail("env_attach: n_actions, n_mpc_steps, episode_length and n_samples must be >= 1");
        if (N < ENV_MA || N + 1 > ENV_MAXPTS) return fail("env_attach: the observation's 10-tap moving average of the yaw rate needs 10 <= N <= 127");
        if (max_lat_dev != max_lat_dev) return fail("env_attach: max_lat_dev is NaN (an infinite one disables the crash test)");
        if (obs_states != 0 && obs_states != 1) return fail("env_attach: obs_states must be 0 (reference) or 1 (last_step)");
        for (int i = 0; i < 2; i++) {
            if (!(sigmas[i] > 0.0)) return fail("env_attach: sigmas must be positive");
            if (!(lims[2 + i] != lims[i])) return fail("env_attach: lims[1] must differ from lims[0]");
        }
        for (int i = 0; i < n_samples; i++) {
            if (idx_v[i] < 0 || idx_v[i] > N) return fail("env_attach: a velocity sample index is outside 0..N");
            if (idx_yawrate[i] < 0 || idx_yawrate[i] > N - ENV_MA) return fail("env_attach: a yaw rate sample index is outside 0..N-10");
        }
        for (int i = 0; i < 2 + 2 * n_samples; i++)
            if (!(obs_hi[i] != obs_lo[i])) return fail("env_attach: an observation bound has no width");
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    graph_drop(s);          // (a captured chunk holds the extra launch and the sample counters, or lacks them)
    env_release(s);
    if (!table) return 0;
    const int no = 2 + 2 * n_samples, rec = ENV_REC + no;
    std::vector<double> bounds(2 * (size_t)no);
    for (int i = 0; i < no; i++) { bounds[i] = obs_lo[i]; bounds[no + i] = obs_hi[i]; }
    std::vector<int> idx(2 * (size_t)n_samples), samples(B, s->core.step);
    for (int i = 0; i < n_samples; i++) { idx[i] = idx_v[i]; idx[n_samples + i] = idx_yawrate[i]; }
    SimEnv &v = s->env; const SimCore &k = s->core;
    bool ok = true;
    ok &= v.table.alloc((size_t)n_actions * 7) == hipSuccess && v.bounds.alloc(bounds.size()) == hipSuccess;
    ok &= v.acc.alloc(B * 4) == hipSuccess && v.win.alloc(B * 2 * (N + 1)) == hipSuccess && v.out.alloc(B * rec) == hipSuccess;
    ok &= v.idx.alloc(idx.size()) == hipSuccess && v.in.alloc(B * 3) == hipSuccess && v.ep.alloc(B) == hipSuccess;
    ok &= v.count.alloc(B) == hipSuccess && v.flags.alloc(B) == hipSuccess && v.qpf.alloc(B) == hipSuccess && v.samples.alloc(B) == hipSuccess;
    ok = ok && v.hout.alloc(B * rec) == hipSuccess && v.hin.alloc(B * 3) == hipSuccess;
    v.ended.assign(B, 0);
    ok = ok && hipMemcpy(v.table.get(), table, sizeof(double) * 7 * n_actions, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(v.bounds.get(), bounds.data(), sizeof(double) * bounds.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(v.idx.get(), idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice) == hipSuccess;
    // the estimator of every instance has seen as many samples as the loop has run control steps: attaching changes nothing the loop computes
    ok = ok && hipMemcpy(v.samples.get(), samples.data(), sizeof(int) * B, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { env_release(s); (void)hipGetLastError(); return fail("env_attach: allocation failed"); }
    EnvArgs &a = v.a;
    a.N = N; a.batch = c->batch; a.n_track = k.n_track; a.n_actions = n_actions; a.n_samples = n_samples; a.episode_length = episode_length;
    a.full_lap = full_lap ? 1 : 0; a.obs_last_step = obs_states; a.log_cap = k.log_cap;
    a.max_lat_dev = max_lat_dev; a.Ts = k.Ts;
    for (int i = 0; i < 2; i++) a.sig[i] = sigmas[i];
    for (int i = 0; i < 4; i++) a.lim[i] = lims[i];
    a.track = k.track.get(); a.track_of = k.d_track_of.get(); a.track_rows = k.d_rows.get(); a.table = v.table.get(); a.in = v.in.get(); a.obs_idx = v.idx.get(); a.obs_bounds = v.bounds.get();
    a.x_sim = k.xsim.get(); a.pose = k.pose.get(); a.hist = k.hist.get(); a.ref0 = k.ref0.get(); a.closest = k.closest.get();
    a.step_counter = k.step_counter.get(); a.err = k.err.get(); a.lCiLX = k.lCiLX.get(); a.lSimX = k.lSimX.get();
    a.ep_steps = v.ep.get(); a.count = v.count.get(); a.flags = v.flags.get(); a.qpf = v.qpf.get(); a.samples = v.samples.get();
    a.acc = v.acc.get(); a.win = v.win.get(); a.out = v.out.get();
    v.on = true; v.mpc_steps = n_mpc_steps; v.rec = rec;
    return 0;
}

// The begin kernel of an environment step on the capsule's stream. `changed`: what it writes, for invalidate() -- W and the penalties
// where it installs actions; the iterate, x0 and the pose the planner reads of the instances it resets. Never CH_RESTART: a partly reset
// batch is not stage-uniform. The caller holds the device guard.
enum : unsigned { ENV_CH_ACTIONS = CH_W | CH_BOUNDS, ENV_CH_RESET = CH_ITERATE | CH_X0 | CH_REF };
static int env_enqueue_begin(tum_sim *s, unsigned changed, int with_actions)
{
    tum_ocp *c = s->c;
    invalidate(c, changed);
    env_bind(s);
    LAUNCH(env_begin_kernel, dim3(c->batch), dim3(64), 0, c->stream, s->env.a, with_actions);
    return 0;
}
// One environment step on the capsule's stream, nothing waited for: the begin kernel on the actions in env.in, n_mpc_steps control
// steps, the finish kernel. Where the DEVICE marks the instances to reset (rollout, collect) the host does not know which they are:
// `changed` is ENV_CH_ACTIONS | ENV_CH_RESET then, as if any had been.
static int env_enqueue_step(tum_sim *s, unsigned changed)
{
    tum_ocp *c = s->c;
    if (env_enqueue_begin(s, changed, 1)) return 1;
    if (sim_run_enqueue(s, s->env.mpc_steps)) return 1;
    env_bind(s);
    LAUNCH(env_finish_kernel, dim3(c->batch), dim3(64), 0, c->stream, s->env.a);
    return 0;
}

// on a track set an index is held against the instance's own track: the tail of a refusal that says which one that is
static std::string env_own_track(const tum_sim *s, size_t b)
{
    const SimCore &k = s->core;
    if (!k.d_track_of.get()) return "";
    return " it drives on (track " + std::to_string(k.track_of[b]) + " of the set, " + std::to_string(k.rows_of(b)) + " rows)";
}
// checks and uploads actions | reset mask | start indices (any may be null: none) of a host-driven step or reset; *changed: what the
// begin kernel behind it will write. The caller holds the device guard.
static int env_stage(tum_sim *s, const int *actions, const int *reset_mask, const int *start_idx, const char *who, unsigned *changed)
{
    tum_ocp *c = s->c; const int B = c->batch; SimEnv &v = s->env;
    const std::string w(who);
    bool any_reset = false;
    for (int b = 0; b < B; b++) {
        const bool r = reset_mask && reset_mask[b] == 1, go_on = reset_mask && reset_mask[b] == 2;
        if (reset_mask && !r && !go_on && reset_mask[b] != 0) return fail(w + ": a reset mask holds 0 (nothing), 1 (reset) or 2 (an ended episode drives on)");
        if (r && (!start_idx || start_idx[b] < 0 || start_idx[b] >= s->core.rows_of(b))) return fail(w + ": start index of instance " + std::to_string(b) + " is outside the track" + env_own_track(s, b));
        if (actions && (actions[b] < 0 || actions[b] >= v.a.n_actions))
            return fail(w + ": action " + std::to_string(actions[b]) + " of instance " + std::to_string(b) + " is outside the table of " + std::to_string(v.a.n_actions) + " rows");
        if (actions && v.ended[b] && !r && !go_on) return fail(w + ": the episode of instance " + std::to_string(b) + " has ended and it is not marked for reset");
        any_reset |= r;
    }
    if (flush_inputs(c)) return 1;          // (older setters of x0 / yref in the pinned shadow go first: the begin kernel writes behind them)
    int *hin = v.hin.get();
    for (int b = 0; b < B; b++) {
        const bool r = reset_mask && reset_mask[b] == 1;
        if (reset_mask && reset_mask[b] == 2) v.ended[b] = 0;
        hin[b] = actions ? actions[b] : 0; hin[B + b] = r ? 1 : 0; hin[2 * B + b] = r ? start_idx[b] : 0;
        if (r) v.ended[b] = 0;
    }
    HIPCHK(hipMemcpyAsync(v.in.get(), hin, sizeof(int) * 3 * B, hipMemcpyHostToDevice, c->stream));
    *changed = (actions ? ENV_CH_ACTIONS : 0u) | (any_reset ? ENV_CH_RESET : 0u);
    return 0;
}

extern "C" int tum_sim_env_reset(tum_sim *s, const int *mask, const int *start_idx)
{
    if (!s || !start_idx) return fail("null argument");
    if (!s->env.on) return fail("env_reset: no environment attached (tum_sim_env_attach)");
    if (env_refuse(s, "env_reset")) return 1;
    tum_ocp *c = s->c;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    std::vector<int> all;
    if (!mask) { all.assign(c->batch, 1); mask = all.data(); }
    unsigned changed = 0;
    if (env_stage(s, nullptr, mask, start_idx, "env_reset", &changed) || env_enqueue_begin(s, changed, 0)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the planner's error flag of n environment steps, flag[e * stride]
static int env_plan_check(const char *who, const double *flag, size_t stride, int n)
{
    for (int e = 0; e < n; e++)
        if (flag[e * stride] != 0.0) return fail(std::string(who) + ": planner segment longer than PLAN_MAXM points");
    return 0;
}
// env.ended[] from the last step that ran: instance b has ended where one of the n flags at flag[b * stride] is set
static void env_mark_ended(tum_sim *s, const double *flag, size_t stride, int n)
{
    for (size_t b = 0; b < s->env.ended.size(); b++) {
        bool e = false;
        for (int i = 0; i < n; i++) e |= flag[b * stride + i] != 0.0;
        s->env.ended[b] = e ? 1 : 0;
    }
}

extern "C" int tum_sim_env_step(tum_sim *s, const int *actions, const int *reset_mask, const int *start_idx, double *out)
{
    if (!s || !actions || !out) return fail("null argument");
    if (!s->env.on) return fail("env_step: no environment attached (tum_sim_env_attach)");
    if (env_refuse(s, "env_step")) return 1;
    tum_ocp *c = s->c; const size_t B = c->batch; SimEnv &v = s->env;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    unsigned changed = 0;
    if (env_stage(s, actions, reset_mask, start_idx, "env_step", &changed) || env_enqueue_step(s, changed)) return 1;
    HIPCHK(hipMemcpyAsync(v.hout.get(), v.out.get(), sizeof(double) * B * v.rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (env_plan_check("env_step", v.hout.get() + 5, 0, 1)) return 1;
    memcpy(out, v.hout.get(), sizeof(double) * B * v.rec);
    for (size_t b = 0; b < B; b++)          // (an instance that has ended stays so until it is reset or told to drive on)
        if (out[b * v.rec + 1] != 0.0 || out[b * v.rec + 2] != 0.0) v.ended[b] = 1;
    return lin_uniform_check(c);
}

// ---------------------------------------------------------------------------------------------- K12: the agent, whole episodes
// The policy net of the reference's agent (a stable_baselines3 MlpPolicy with tanh activations; inference only: model.predict(obs,
// deterministic=True) and helpers.py:100-105 get_action_probabilities) in the layout policy_kernel reads. widths[n_layers + 1]: inputs,
// hidden widths..., actions; W[l] row-major (out, in) as torch stores it. W == NULL detaches. On a loop with an environment the widths
// must fit it; on one without, the policy serves tum_sim_policy_eval alone (attaching an environment detaches it). Nothing a captured
// chunk of control steps holds changes: the policy runs outside sim_run_enqueue.
// What both nets must satisfy; what differs is passed in: the name of the call and of the last layer, the rule for the input width and
// the rule for the last layer's (each fails with its own message and returns non-zero).
template <typename InputRule, typename LastRule>
static int net_check(const std::string &w, const char *last_layer, int n_layers, const int *widths, const float *const *W, const float *const *b,
                     InputRule input_rule, LastRule last_rule)
{
    if (n_layers < 2 || n_layers > POL_MAXMAT) return fail(w + ": 1 to 4 hidden layers (n_layers 2..5 with the " + last_layer + " layer)");
    for (int l = 0; l < n_layers; l++) if (!W[l] || !b[l]) return fail("null argument");
    if (input_rule(widths[0])) return 1;
    for (int l = 1; l < n_layers; l++)
        if (widths[l] < 1 || widths[l] > POL_MAXWIDTH) return fail(w + ": hidden layers are 1 to 256 wide");
    return last_rule(widths[n_layers]);
}
// a net in the layout policy_layers reads, on the device; false where an allocation or a copy failed (the caller releases)
static bool net_upload(SimNet &net, int n_layers, const int *widths, const float *const *W, const float *const *b)
{
    PolicyArgs &a = net.a;
    memset(&a, 0, sizeof(a));
    a.n_mat = n_layers; a.n_in = widths[0]; a.n_act = widths[n_layers];
    for (int l = 0; l <= n_layers; l++) net.widths[l] = widths[l];
    bool ok = true;
    for (int l = 0; l < n_layers && ok; l++) {
        const int in = widths[l], out = widths[l + 1], kp = (in + 3) & ~3, mp = (out + 15) & ~15;
        a.kp[l] = kp; a.mp[l] = mp; a.rows = std::max(a.rows, std::max(kp, mp));
        // float -> double is exact; the A operand of product (t, q) is 64 consecutive doubles: lane holds W[16 t + (lane & 15)][4 q + (lane >> 4)]
        std::vector<double> Wp((size_t)mp * kp, 0.0), bp(mp, 0.0);
        for (int t = 0; t < mp / 16; t++)
            for (int q = 0; q < kp / 4; q++)
                for (int lane = 0; lane < 64; lane++) {
                    const int r = 16 * t + (lane & 15), k = 4 * q + (lane >> 4);
                    if (r < out && k < in) Wp[((size_t)t * (kp / 4) + q) * 64 + lane] = (double)W[l][(size_t)r * in + k];
                }
        for (int r = 0; r < out; r++) bp[r] = (double)b[l][r];
        ok = ok && net.W[l].alloc(Wp.size()) == hipSuccess && net.b[l].alloc(bp.size()) == hipSuccess;
        ok = ok && hipMemcpy(net.W[l].get(), Wp.data(), sizeof(double) * Wp.size(), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(net.b[l].get(), bp.data(), sizeof(double) * bp.size(), hipMemcpyHostToDevice) == hipSuccess;
        a.W[l] = net.W[l].get(); a.b[l] = net.b[l].get();
    }
    return ok;
}

extern "C" int tum_sim_policy_attach(tum_sim *s, int n_layers, const int *widths, const float *const *W, const float *const *b)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c;
    if (W) {
        if (!widths || !b) return fail("null argument");
        const std::string w("policy_attach");
        if (net_check(w, "action", n_layers, widths, W, b,
                      [&](int in) { return (in < 1 || in > POL_MAXIN) ? fail(w + ": 1 to 128 inputs") : 0; },
                      [&](int out) { return (out < 1 || out > POL_MAXACT) ? fail(w + ": 1 to 64 actions") : 0; })) return 1;
        // without an environment the policy serves tum_sim_policy_eval alone; with one it reads its observation and picks rows of its table
        if (s->env.on && widths[0] != s->env.rec - ENV_REC)
            return fail("policy_attach: the policy takes " + std::to_string(widths[0]) + " inputs, the environment's observation has " + std::to_string(s->env.rec - ENV_REC) + " entries");
        if (s->env.on && widths[n_layers] != s->env.a.n_actions)
            return fail("policy_attach: the policy has " + std::to_string(widths[n_layers]) + " actions, the environment's table has " + std::to_string(s->env.a.n_actions) + " rows");
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (s->wm.on) graph_drop(s);          // (a captured chunk holds the schedule's launch, which goes with the policy)
    policy_release(s);
    if (!W) return 0;
    const size_t B = c->batch; SimRollout &r = s->roll;
    bool ok = net_upload(s->pol, n_layers, widths, W, b);
    ok = ok && r.obs.alloc(B * s->pol.a.n_in) == hipSuccess && r.live.alloc(B) == hipSuccess && r.n_live.alloc(1) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)policy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)policy_ac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { policy_release(s); (void)hipGetLastError(); return fail("policy_attach: allocation failed"); }
    s->pol.on = true;
    return 0;
}

// one launch of the policy on the capsule's stream: n instances, observations [n][stride] on the device
static int policy_launch(tum_sim *s, const double *dobs, int stride, int n, double *dlogits, double *dprobs, int *dactions)
{
    PolicyArgs a = s->pol.a;
    a.n = n; a.obs = dobs; a.obs_stride = stride; a.logits = dlogits; a.probs = dprobs; a.actions = dactions;
    LAUNCH(policy_kernel, dim3((n + POL_TILE - 1) / POL_TILE), dim3(64 * POL_WAVES), sizeof(double) * 2 * a.rows * POL_TILE, s->c->stream, a);
    return 0;
}

// the policy alone on n host observations (n x widths[0]), independent of the loop's batch: logits and probabilities n x actions, actions n
extern "C" int tum_sim_policy_eval(tum_sim *s, const double *obs, int n, double *logits, double *probs, int *actions)
{
    if (!s || !obs) return fail("null argument");
    if (!s->pol.on) return fail("policy_eval: no policy attached (tum_sim_policy_attach)");
    if (n < 1) return fail("policy_eval: n < 1");
    tum_ocp *c = s->c;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const size_t ni = (size_t)n * s->pol.a.n_in, na = (size_t)n * s->pol.a.n_act;
    DevBuf<double> to, tl, tp; DevBuf<int> ta;
    HIPCHK(to.alloc(ni, false)); HIPCHK(tl.alloc(na, false)); HIPCHK(tp.alloc(na, false)); HIPCHK(ta.alloc(n, false));
    HIPCHK(hipMemcpy(to.get(), obs, sizeof(double) * ni, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    if (policy_launch(s, to.get(), s->pol.a.n_in, n, logits ? tl.get() : nullptr, probs ? tp.get() : nullptr, actions ? ta.get() : nullptr)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (logits) HIPCHK(hipMemcpy(logits, tl.get(), sizeof(double) * na, hipMemcpyDeviceToHost));
    if (probs) HIPCHK(hipMemcpy(probs, tp.get(), sizeof(double) * na, hipMemcpyDeviceToHost));
    if (actions) HIPCHK(hipMemcpy(actions, ta.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------- K19: the learned weight schedule
// enable_WMPC of the reference's controller classes inside the loop (wmpc_kernels.hpp; the rule: include/tum_nmpc.h). The kernel's
// launch is part of every control step from here on (wmpc_enqueue of sim_loop.hpp), of a captured chunk too.
extern "C" int tum_sim_wmpc_attach(tum_sim *s, const double *table, int n_actions, int period, int on_failure, int n_samples,
                                   const int *idx_v, const int *idx_yawrate, const double *obs_lo, const double *obs_hi, int log_capacity)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c; const size_t B = c->batch; const int N = c->N;
    if (table) {
        if (!idx_v || !idx_yawrate || !obs_lo || !obs_hi) return fail("null argument");
        if (!s->pol.on) return fail("wmpc_attach: no policy attached (tum_sim_policy_attach)");
        if (wmpc_refuse(s, "wmpc_attach")) return 1;
        if (n_actions < 1 || n_samples < 1) return fail("wmpc_attach: n_actions and n_samples must be >= 1");
        if (period < 0) return fail("wmpc_attach: weights_update_period is negative (0 decides at every control step)");
        if (on_failure != 0 && on_failure != 1) return fail("wmpc_attach: on_failure is 0 (keep the weights) or 1 (back to the weights held at attach time)");
        if (log_capacity < 0) return fail("wmpc_attach: log_capacity < 0");
        if (N < ENV_MA || N + 1 > ENV_MAXPTS) return fail("wmpc_attach: the observation's 10-tap moving average of the yaw rate needs 10 <= N <= 127");
        if (s->pol.a.n_in != 2 + 2 * n_samples)
            return fail("wmpc_attach: the policy takes " + std::to_string(s->pol.a.n_in) + " inputs, the observation has " + std::to_string(2 + 2 * n_samples) + " entries");
        if (s->pol.a.n_act != n_actions)
            return fail("wmpc_attach: the policy has " + std::to_string(s->pol.a.n_act) + " actions, the table has " + std::to_string(n_actions) + " rows");
        for (int i = 0; i < n_samples; i++) {
            if (idx_v[i] < 0 || idx_v[i] > N) return fail("wmpc_attach: a velocity sample index is outside 0..N");
            if (idx_yawrate[i] < 0 || idx_yawrate[i] > N - ENV_MA) return fail("wmpc_attach: a yaw rate sample index is outside 0..N-10");
        }
        for (int i = 0; i < 2 + 2 * n_samples; i++)
            if (!(obs_hi[i] != obs_lo[i])) return fail("wmpc_attach: an observation bound has no width");
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    graph_drop(s);          // (a captured chunk holds the extra launch, or lacks it)
    wmpc_release(s);
    if (!table) return 0;
    const int no = 2 + 2 * n_samples; const size_t L = (size_t)log_capacity * B, recW = (size_t)(N + 1) * 6;
    std::vector<double> bounds(2 * (size_t)no);
    for (int i = 0; i < no; i++) { bounds[i] = obs_lo[i]; bounds[no + i] = obs_hi[i]; }
    std::vector<int> idx(2 * (size_t)n_samples), since(B, s->core.step);
    for (int i = 0; i < n_samples; i++) { idx[i] = idx_v[i]; idx[n_samples + i] = idx_yawrate[i]; }
    SimWmpc &m = s->wm; const SimCore &k = s->core;
    m.lds = sizeof(double) * wmpc_lds_doubles(s->pol.a.rows, N);
    bool ok = true;
    ok &= m.table.alloc((size_t)n_actions * 7) == hipSuccess && m.bounds.alloc(bounds.size()) == hipSuccess && m.idx.alloc(idx.size()) == hipSuccess;
    ok &= m.base_W.alloc(B * recW) == hipSuccess && m.base_pen.alloc(B * 36) == hipSuccess;
    ok &= m.since.alloc(B) == hipSuccess && m.n_dec.alloc(B) == hipSuccess && m.act.alloc(B) == hipSuccess;
    if (L) ok &= m.log_step.alloc(L) == hipSuccess && m.log_act.alloc(L) == hipSuccess && m.log_obs.alloc(L * no) == hipSuccess;
    ok = ok && hipMemcpy(m.table.get(), table, sizeof(double) * 7 * n_actions, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(m.bounds.get(), bounds.data(), sizeof(double) * bounds.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(m.idx.get(), idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice) == hipSuccess;
    // the snapshot a failed solve goes back to: W and the penalties as the loop holds them now
    ok = ok && hipMemcpy(m.base_W.get(), c->dW, sizeof(double) * B * recW, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipMemcpy(m.base_pen.get(), c->dpen, sizeof(double) * B * 36, hipMemcpyDeviceToDevice) == hipSuccess;
    // the counter of every instance is 0 at the step the loop stands at
    ok = ok && hipMemcpy(m.since.get(), since.data(), sizeof(int) * B, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && L) {
        ok = hipMemset(m.log_step.get(), 0xff, sizeof(int) * L) == hipSuccess && hipMemset(m.log_act.get(), 0xff, sizeof(int) * L) == hipSuccess;
    }
    ok = ok && hipFuncSetAttribute((const void *)wmpc_schedule_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m.lds) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { wmpc_release(s); (void)hipGetLastError(); return fail("wmpc_attach: allocation failed"); }
    WmpcArgs &a = m.a;
    a.N = N; a.batch = c->batch; a.n_actions = n_actions; a.n_samples = n_samples; a.period = period; a.restore = on_failure; a.log_cap = log_capacity;
    a.Ts = k.Ts;
    a.table = m.table.get(); a.obs_idx = m.idx.get(); a.obs_bounds = m.bounds.get(); a.base_W = m.base_W.get(); a.base_pen = m.base_pen.get();
    a.ref0 = k.ref0.get(); a.step_counter = k.step_counter.get();
    a.since = m.since.get(); a.n_dec = m.n_dec.get(); a.log_step = m.log_step.get(); a.log_act = m.log_act.get(); a.log_obs = m.log_obs.get();
    a.pol = s->pol.a;
    a.pol.n = c->batch; a.pol.obs = nullptr; a.pol.obs_stride = 0; a.pol.logits = a.pol.probs = nullptr; a.pol.actions = m.act.get();
    m.n_obs = no; m.on = true;
    return 0;
}

// counter (B: the reference's self.counter as the next control step will test it), n_decisions (B), the first log_capacity decisions
// of every instance -- steps, actions (B x log_capacity, -1 where none), observations (B x log_capacity x n_obs) --, the snapshot
// base_W (B x (N + 1) x 6) and base_pen (B x 36), and the weights as they are now: W, pen (the same shapes)
extern "C" int tum_sim_wmpc_get(tum_sim *s, const char *field, double *out, long long len)
{
    if (!s || !field || !out) return fail("null argument");
    tum_ocp *c = s->c; const long long B = c->batch, recW = (long long)(c->N + 1) * 6; const SimWmpc &m = s->wm;
    const std::string f(field);
    if (!m.on) return fail("wmpc_get " + f + ": no weight schedule attached (tum_sim_wmpc_attach)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    const long long L = (long long)m.a.log_cap * B;
    const struct { const char *name; const int *isrc; const double *dsrc; long long want; } arrays[] = {
        {"counter", m.since.get(), nullptr, B}, {"n_decisions", m.n_dec.get(), nullptr, B},
        {"steps", m.log_step.get(), nullptr, L}, {"actions", m.log_act.get(), nullptr, L}, {"observations", nullptr, m.log_obs.get(), L * m.n_obs},
        {"base_W", nullptr, m.base_W.get(), B * recW}, {"base_pen", nullptr, m.base_pen.get(), B * 36},
        {"W", nullptr, c->dW, B * recW}, {"pen", nullptr, c->dpen, B * 36}};
    for (const auto &a : arrays) {
        if (f != a.name) continue;
        if (len != a.want) return fail("wmpc_get " + f + ": len mismatch");
        if (a.want == 0) return 0;
        if (a.isrc) { if (fetch_ints(a.isrc, (size_t)a.want, out)) return 1; }
        else HIPCHK(hipMemcpy(out, a.dsrc, sizeof(double) * a.want, hipMemcpyDeviceToHost));
        if (f == "counter") for (long long b = 0; b < B; b++) out[b] = (double)s->core.step - out[b];
        return 0;
    }
    return fail("wmpc_get: unknown field '" + f + "'");
}

// what tum_sim_env_rollout and tum_sim_env_collect share beside env_enqueue_step: every entry of a start table (E x B) is a point of the track
static int env_check_start_table(const tum_sim *s, const char *who, const int *start_table, size_t E)
{
    const size_t B = s->c->batch;
    for (size_t i = 0; i < E * B; i++)
        if (start_table[i] < 0 || start_table[i] >= s->core.rows_of(i % B))
            return fail(std::string(who) + ": start index of instance " + std::to_string(i % B) + " at step " + std::to_string(i / B) + " is outside the track" + env_own_track(s, i % B));
    return 0;
}
// step 0, what the host knows: an instance whose episode has ended is reset to start_table[0][b] (reset_ended) and the policy sees zeros
// for it; the others see first_obs (B x n_obs, NULL: zeros). Uploads env.in and the policy's input; the caller waits for the device
static int env_stage_first(tum_sim *s, const double *first_obs, bool reset_ended, const int *start_table)
{
    const size_t B = s->c->batch; const int no = s->pol.a.n_in; SimEnv &v = s->env;
    std::vector<double> obs0(B * no, 0.0);
    int *hin = v.hin.get();
    for (size_t b = 0; b < B; b++) {
        const bool r = reset_ended && v.ended[b];
        hin[b] = 0; hin[B + b] = r ? 1 : 0; hin[2 * B + b] = r ? start_table[b] : 0;
        if (first_obs && !r) memcpy(&obs0[b * no], first_obs + b * no, sizeof(double) * no);
    }
    HIPCHK(hipMemcpy(v.in.get(), hin, sizeof(int) * 3 * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->roll.obs.get(), obs0.data(), sizeof(double) * B * no, hipMemcpyHostToDevice));
    return 0;
}

// n_env_steps x (policy, begin, n_mpc_steps control steps, finish, next) on the capsule's stream without a host wait in between; one
// download behind the last step (and the 4-byte counter of live instances every check_every steps where asked for).
//   first_obs (B x n_obs, NULL: zeros -- what a reset returns) is what the policy sees first.
//   on_end 0: an instance whose episode ends is frozen out: it drives on as with reset mask 2 of tum_sim_env_step, live = 0 from the
//             next step on and its later rows are not results. An instance whose episode had ended BEFORE the call starts with live = 0.
//   on_end 1: it is reset at the start of step e + 1 to start_table[e + 1][b] and the policy sees zeros for it; an instance whose
//             episode had ended before the call is reset to start_table[0][b] at step 0. start_table: n_env_steps x B.
// env.ended[] afterwards: the flags of the last step that ran, which is what tum_sim_env_step leaves when an ended instance drives on.
extern "C" int tum_sim_env_rollout(tum_sim *s, int n_env_steps, const double *first_obs, int on_end, const int *start_table,
                                   int check_every, double *out, int *actions_out, int *live_out, int *steps_run)
{
    if (!s || !out || !actions_out || !live_out || !steps_run) return fail("null argument");
    if (!s->env.on) return fail("env_rollout: no environment attached (tum_sim_env_attach)");
    if (env_refuse(s, "env_rollout")) return 1;
    if (!s->pol.on) return fail("env_rollout: no policy attached (tum_sim_policy_attach)");
    if (n_env_steps < 1) return fail("env_rollout: n_env_steps < 1");
    if (on_end != 0 && on_end != 1) return fail("env_rollout: on_end is 0 (an ended instance is frozen out) or 1 (it is reset)");
    if (on_end == 1 && !start_table) return fail("env_rollout: on_end 1 resets ended instances and needs a start table (n_env_steps x batch)");
    tum_ocp *c = s->c; const size_t B = c->batch, E = n_env_steps, rec = s->env.rec; const int no = s->pol.a.n_in;
    SimEnv &v = s->env; SimRollout &r = s->roll;
    if (start_table && env_check_start_table(s, "env_rollout", start_table, E)) return 1;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;          // (older setters of x0 / yref in the pinned shadow go first: the begin kernel writes behind them)
    HIPCHK(hipStreamSynchronize(c->stream));
    if (r.log.reserve(E * B * rec) != hipSuccess || r.ints.reserve(3 * E * B) != hipSuccess) { (void)hipGetLastError(); return fail("env_rollout: allocation failed"); }
    int *dact = r.ints.get(), *dlive = dact + E * B, *dtab = dlive + E * B;
    if (env_stage_first(s, first_obs, on_end == 1, start_table)) return 1;
    std::vector<int> live0(B);
    int n_live = 0;
    for (size_t b = 0; b < B; b++) n_live += live0[b] = (on_end == 0 && v.ended[b]) ? 0 : 1;
    HIPCHK(hipMemcpy(r.live.get(), live0.data(), sizeof(int) * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(r.n_live.get(), &n_live, sizeof(int), hipMemcpyHostToDevice));
    if (start_table) HIPCHK(hipMemcpy(dtab, start_table, sizeof(int) * E * B, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    RolloutArgs ra{};
    ra.batch = (int)B; ra.rec = (int)rec; ra.head = ENV_REC; ra.n_obs = no; ra.n_env_steps = n_env_steps; ra.on_end = on_end;
    ra.out = v.out.get(); ra.in = v.in.get(); ra.start_table = start_table ? dtab : nullptr; ra.pol_obs = r.obs.get();
    ra.live = r.live.get(); ra.n_live = r.n_live.get(); ra.log = r.log.get(); ra.act_log = dact; ra.live_log = dlive;
    int ran = 0;
    *steps_run = 0;
    if (!(check_every > 0 && n_live == 0))
        for (int e = 0; e < n_env_steps; e++) {
            if (policy_launch(s, r.obs.get(), no, (int)B, nullptr, nullptr, v.in.get())) return 1;
            if (env_enqueue_step(s, ENV_CH_ACTIONS | ENV_CH_RESET)) return 1;
            ra.e = e;
            LAUNCH(rollout_next_kernel, dim3((B + 63) / 64), dim3(64), 0, c->stream, ra);
            ran = e + 1;
            if (check_every > 0 && ran % check_every == 0 && ran < n_env_steps) {
                int nl = 0;
                HIPCHK(hipStreamSynchronize(c->stream));
                HIPCHK(hipMemcpy(&nl, r.n_live.get(), sizeof(int), hipMemcpyDeviceToHost));
                if (nl == 0) break;
            }
        }
    HIPCHK(hipStreamSynchronize(c->stream));
    *steps_run = ran;
    if (ran == 0) return 0;
    HIPCHK(hipMemcpy(out, r.log.get(), sizeof(double) * ran * B * rec, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(actions_out, dact, sizeof(int) * ran * B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(live_out, dlive, sizeof(int) * ran * B, hipMemcpyDeviceToHost));
    env_mark_ended(s, out + (size_t)(ran - 1) * B * rec + 1, rec, 2);
    if (env_plan_check("env_rollout", out + 5, B * rec, ran)) return 1;
    return lin_uniform_check(c);
}

// ---------------------------------------------------------------------------------------------- K13: collecting PPO training rollouts
// The value net of the agent (mlp_extractor.value_net.<i>, value_net of a stable_baselines3 MlpPolicy) beside the attached policy:
// widths[n_layers + 1] = inputs, hidden widths..., 1; the inputs are the policy's. W == NULL detaches. Detaching or re-attaching the
// policy or the environment detaches it.
extern "C" int tum_sim_policy_attach_value(tum_sim *s, int n_layers, const int *widths, const float *const *W, const float *const *b)
{
    if (!s) return fail("null argument");
    tum_ocp *c = s->c;
    if (W) {
        if (!widths || !b) return fail("null argument");
        if (!s->pol.on) return fail("policy_attach_value: no policy attached (tum_sim_policy_attach): the value net takes the policy's inputs");
        const std::string w("policy_attach_value");
        const int n_in = s->pol.a.n_in;
        if (net_check(w, "value", n_layers, widths, W, b,
                      [&](int in) { return in != n_in ? fail(w + ": the value net takes " + std::to_string(in) + " inputs, the policy " + std::to_string(n_in)) : 0; },
                      [&](int out) { return out != 1 ? fail(w + ": the last matrix of a value net has one row") : 0; })) return 1;
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    value_release(s);
    if (!W) return 0;
    const size_t B = c->batch;
    bool ok = net_upload(s->val, n_layers, widths, W, b);
    ok = ok && s->col.term.alloc(B) == hipSuccess && s->col.starts.alloc(B) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)policy_ac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { value_release(s); (void)hipGetLastError(); return fail("policy_attach_value: allocation failed"); }
    s->val.on = true;
    return 0;
}

// one launch of the actor-critic evaluation on the capsule's stream: n instances, observations [n][stride] on the device. do_pi 0: the
// value net alone. with_value 0: the policy net alone (dvalues must be null then)
static int ac_launch(tum_sim *s, const double *dobs, int stride, int n, int do_pi, bool with_value, unsigned long long seed, unsigned long long t,
                     unsigned first, int *dactions, double *dvalues, double *dlogp, double *du)
{
    AcArgs a{};
    a.pi = s->pol.a;
    if (with_value) a.vf = s->val.a;
    a.pi.n = a.vf.n = n; a.pi.obs = a.vf.obs = dobs; a.pi.obs_stride = a.vf.obs_stride = stride;
    a.pi.logits = a.pi.probs = nullptr; a.pi.actions = dactions;
    a.rows = std::max(do_pi ? s->pol.a.rows : 0, with_value ? s->val.a.rows : 0);
    a.do_pi = do_pi; a.seed = seed; a.t = t; a.first = first;
    a.values = dvalues; a.log_probs = dlogp; a.uniforms = du;
    LAUNCH(policy_ac_kernel, dim3((n + POL_TILE - 1) / POL_TILE), dim3(64 * POL_WAVES), sizeof(double) * 2 * a.rows * POL_TILE, s->c->stream, a);
    return 0;
}

// the two nets and one draw on n host observations (n x widths[0]), independent of the loop's batch; instance i draws with counter word
// first_instance + i at decision t. Any output may be NULL; values needs the value net, the others do not.
extern "C" int tum_sim_policy_eval_ac(tum_sim *s, const double *obs, int n, unsigned long long seed, unsigned long long t, unsigned first_instance,
                                      int *actions, double *values, double *log_probs, double *uniforms)
{
    if (!s || !obs) return fail("null argument");
    if (!s->pol.on) return fail("policy_eval_ac: no policy attached (tum_sim_policy_attach)");
    if (values && !s->val.on) return fail("policy_eval_ac: values asked for and no value net attached (tum_sim_policy_attach_value)");
    if (n < 1) return fail("policy_eval_ac: n < 1");
    tum_ocp *c = s->c;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const size_t ni = (size_t)n * s->pol.a.n_in;
    DevBuf<double> to, td; DevBuf<int> ta;
    HIPCHK(to.alloc(ni, false)); HIPCHK(td.alloc((size_t)3 * n, false)); HIPCHK(ta.alloc(n, false));
    double *dv = td.get(), *dl = dv + n, *du = dl + n;
    HIPCHK(hipMemcpy(to.get(), obs, sizeof(double) * ni, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    const int do_pi = (actions || log_probs || uniforms) ? 1 : 0;
    if (!do_pi && !values) return 0;
    if (ac_launch(s, to.get(), s->pol.a.n_in, n, do_pi, values != nullptr, seed, t, first_instance, actions ? ta.get() : nullptr,
                  values ? dv : nullptr, log_probs ? dl : nullptr, uniforms ? du : nullptr)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (actions) HIPCHK(hipMemcpy(actions, ta.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    if (values) HIPCHK(hipMemcpy(values, dv, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (log_probs) HIPCHK(hipMemcpy(log_probs, dl, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (uniforms) HIPCHK(hipMemcpy(uniforms, du, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

// generalised advantage estimation alone, on host arrays: rewards, values, episode_starts E x B, last_values and last_dones B -> adv, ret E x B
extern "C" int tum_sim_gae(tum_sim *s, int E, int B, const double *rewards, const double *values, const double *episode_starts,
                           const double *last_values, const double *last_dones, double gamma, double lambda, double *adv, double *ret)
{
    if (!s || !rewards || !values || !episode_starts || !last_values || !last_dones || !adv || !ret) return fail("null argument");
    if (E < 1 || B < 1) return fail("gae: E and B must be >= 1");
    tum_ocp *c = s->c;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const size_t EB = (size_t)E * B;
    DevBuf<double> tb;
    HIPCHK(tb.alloc(5 * EB + 2 * B, false));
    double *d = tb.get();
    HIPCHK(hipMemcpy(d, rewards, sizeof(double) * EB, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + EB, values, sizeof(double) * EB, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + 2 * EB, episode_starts, sizeof(double) * EB, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + 5 * EB, last_values, sizeof(double) * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + 5 * EB + B, last_dones, sizeof(double) * B, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    GaeArgs g;
    g.E = E; g.B = B; g.gamma = gamma; g.lambda = lambda;
    g.rewards = d; g.values = d + EB; g.episode_starts = d + 2 * EB; g.last_values = d + 5 * EB; g.last_dones = d + 5 * EB + B;
    g.adv = d + 3 * EB; g.ret = d + 4 * EB;
    LAUNCH(gae_kernel, dim3((B + 63) / 64), dim3(64), 0, c->stream, g);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(adv, g.adv, sizeof(double) * EB, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ret, g.ret, sizeof(double) * EB, hipMemcpyDeviceToHost));
    return 0;
}

// tum_sim_env_rollout with on_end 1, SAMPLED actions and the record of a stable_baselines3 RolloutBuffer: per step the actor-critic
// evaluation (decision counter t0 + e), begin, n_mpc_steps control steps, finish, the value net on the step's own observation, the record;
// behind the last step the value net on what the policy would see next (last_values) and gae_kernel. One wait, one download.
//   first_obs (B x n_obs, NULL: zeros), first_episode_starts (B, NULL: ones): what the policy sees first, and whether that begins an episode
//   out: TUM_COLLECT_FIELDS fields of E x B doubles each (TUM_COLLECT_* in tum_nmpc.h), the observations E x B x n_obs, last_values B,
//        last_dones B, and what the policy would see next B x n_obs (the first_obs of a following call)
extern "C" int tum_sim_env_collect(tum_sim *s, int n_env_steps, const double *first_obs, const double *first_episode_starts, const int *start_table,
                                   unsigned long long seed, unsigned long long t0, double gamma, double gae_lambda, double *out)
{
    if (!s || !out) return fail("null argument");
    if (!s->env.on) return fail("env_collect: no environment attached (tum_sim_env_attach)");
    if (env_refuse(s, "env_collect")) return 1;
    if (!s->pol.on) return fail("env_collect: no policy attached (tum_sim_policy_attach)");
    if (!s->val.on) return fail("env_collect: no value net attached (tum_sim_policy_attach_value)");
    if (n_env_steps < 1) return fail("env_collect: n_env_steps < 1");
    if (!start_table) return fail("env_collect: ended instances are reset and need a start table (n_env_steps x batch)");
    tum_ocp *c = s->c; const size_t B = c->batch, E = n_env_steps, EB = E * B, rec = s->env.rec; const int no = s->pol.a.n_in;
    SimEnv &v = s->env; SimCollect &k = s->col; double *const pol_obs = s->roll.obs.get();
    if (env_check_start_table(s, "env_collect", start_table, E)) return 1;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;          // (older setters of x0 / yref in the pinned shadow go first: the begin kernel writes behind them)
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t total = EB * (COL_FIELDS + no) + 2 * B + B * no;
    k.rows = 0;          // (what tum_sim_ppo_update may train on: set behind a collection that ran to its end)
    if (k.buf.reserve(total) != hipSuccess || k.tab.reserve(EB) != hipSuccess) { (void)hipGetLastError(); return fail("env_collect: allocation failed"); }
    // step 0: beside the first observation, its episode-start flags
    if (env_stage_first(s, first_obs, true, start_table)) return 1;
    std::vector<double> st0(B, 1.0);
    if (first_episode_starts) for (size_t b = 0; b < B; b++) st0[b] = first_episode_starts[b] != 0.0 ? 1.0 : 0.0;
    HIPCHK(hipMemcpy(k.starts.get(), st0.data(), sizeof(double) * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.tab.get(), start_table, sizeof(int) * EB, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    double *buf = k.buf.get();
    CollectArgs ca{};
    ca.batch = (int)B; ca.rec = (int)rec; ca.head = ENV_REC; ca.n_obs = no; ca.n_env_steps = n_env_steps; ca.gamma = gamma;
    ca.out = v.out.get(); ca.in = v.in.get(); ca.start_table = k.tab.get(); ca.pol_obs = pol_obs; ca.term_val = k.term.get();
    ca.first_starts = k.starts.get(); ca.buf = buf;
    for (int e = 0; e < n_env_steps; e++) {
        if (ac_launch(s, pol_obs, no, (int)B, 1, true, seed, t0 + (unsigned long long)e, 0u, v.in.get(),
                      buf + COL_VALUE * EB + e * B, buf + COL_LOGP * EB + e * B, nullptr)) return 1;
        if (env_enqueue_step(s, ENV_CH_ACTIONS | ENV_CH_RESET)) return 1;
        // the value of the step's own observation: the bootstrap of an instance that crashed, and -- to the bit -- the next step's value of one that goes on
        if (ac_launch(s, v.out.get() + ENV_REC, (int)rec, (int)B, 0, true, 0ull, 0ull, 0u, nullptr, k.term.get(), nullptr, nullptr)) return 1;
        ca.e = e;
        LAUNCH(collect_next_kernel, dim3((B + 63) / 64), dim3(64), 0, c->stream, ca);
    }
    double *last_values = buf + EB * (COL_FIELDS + no), *last_dones = last_values + B;
    if (ac_launch(s, pol_obs, no, (int)B, 0, true, 0ull, 0ull, 0u, nullptr, last_values, nullptr, nullptr)) return 1;
    GaeArgs g;
    g.E = n_env_steps; g.B = (int)B; g.gamma = gamma; g.lambda = gae_lambda;
    g.rewards = buf + COL_REWARD * EB; g.values = buf + COL_VALUE * EB; g.episode_starts = buf + COL_START * EB;
    g.last_values = last_values; g.last_dones = last_dones; g.adv = buf + COL_ADV * EB; g.ret = buf + COL_RET * EB;
    LAUNCH(gae_kernel, dim3((B + 63) / 64), dim3(64), 0, c->stream, g);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, buf, sizeof(double) * total, hipMemcpyDeviceToHost));
    env_mark_ended(s, out + EB * (COL_FIELDS + no) + B, 1, 1);
    if (env_plan_check("env_collect", out + COL_ERR * EB, B, n_env_steps)) return 1;
    k.rows = EB;
    return lin_uniform_check(c);
}

// ---------------------------------------------------------------------------------------------- K14: the PPO update
// parameters of a net in the flat vector (W_0, b_0, W_1, ...): the value net's entries begin behind the policy net's
static int ppo_net_params(const PpoNet &t) { const int l = t.n_mat - 1; return t.off[l] + (t.in[l] + 1) * t.out[l]; }
static int ppo_value_offset(const tum_sim *s) { return ppo_net_params(s->ppo.net[0]); }

// the training view of one attached net: widths, strides and offsets in the flat parameter vector; the transposed matrices are allocated
// here (zero: the padding stays zero) and filled by ppo_adam_kernel
static bool ppo_net(PpoNet &t, SimTrainer::Layers &own, const SimNet &net)
{
    const PolicyArgs &a = net.a; const int *widths = net.widths;
    memset(&t, 0, sizeof(t));
    t.n_mat = a.n_mat;
    int off = 0;
    bool ok = true;
    for (int l = 0; l < a.n_mat && ok; l++) {
        t.in[l] = widths[l]; t.out[l] = widths[l + 1]; t.kp[l] = a.kp[l]; t.mp[l] = a.mp[l];
        t.hs[l] = (widths[l] + 15) & ~15; t.kt[l] = (widths[l + 1] + 3) & ~3;
        t.off[l] = off; off += widths[l + 1] * widths[l] + widths[l + 1];
        t.W[l] = net.W[l].get(); t.b[l] = net.b[l].get();
        if (l > 0) { ok = own.WT[l].alloc((size_t)t.hs[l] * t.kt[l]) == hipSuccess; t.WT[l] = own.WT[l].get(); }
    }
    return ok;
}

static PpoAdamArgs ppo_adam_args(const tum_sim *s, int mode)
{
    const SimTrainer &p = s->ppo;
    PpoAdamArgs a{};
    a.net[0] = p.net[0]; a.net[1] = p.net[1]; a.goff[0] = 0; a.goff[1] = ppo_value_offset(s);
    a.P = p.P; a.n_parts = p.parts; a.mode = mode;
    a.G = p.G.get(); a.parts = p.part.get(); a.theta = p.theta.get(); a.m = p.m.get(); a.v = p.v.get();
    a.max_grad_norm = p.max_norm; a.beta1 = 0.9; a.beta2 = 0.999; a.eps = 1e-5; a.step = 0.0; a.bc2_sqrt = 1.0;
    return a;
}

extern "C" int tum_sim_ppo_detach(tum_sim *s)
{
    if (!s) return fail("null argument");
    DevGuard guard(s->c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(s->c->stream));
    ppo_release(s);
    return 0;
}

// The trainer on the attached nets: settings of stable_baselines3's PPO (rl_training.py:133-155), Adam's moments and step counter at
// zero. The float32 master is read back from the packed policy and value nets -- their entries ARE float32 values -- so what is trained
// is exactly what acts.
extern "C" int tum_sim_ppo_attach(tum_sim *s, double clip_range, double ent_coef, double vf_coef, double max_grad_norm, int normalize_advantage)
{
    if (!s) return fail("null argument");
    if (!s->pol.on) return fail("ppo_attach: no policy attached (tum_sim_policy_attach)");
    if (!s->val.on) return fail("ppo_attach: no value net attached (tum_sim_policy_attach_value)");
    if (!(clip_range > 0.0) || !(max_grad_norm > 0.0)) return fail("ppo_attach: clip_range and max_grad_norm must be > 0");
    tum_ocp *c = s->c; SimTrainer &p = s->ppo;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    ppo_release(s);
    bool ok = ppo_net(p.net[0], p.layers[0], s->pol) && ppo_net(p.net[1], p.layers[1], s->val);
    const size_t P = (size_t)ppo_net_params(p.net[0]) + ppo_net_params(p.net[1]);
    p.P = (int)P; p.parts = (int)((P + PPO_SLICE - 1) / PPO_SLICE);
    ok = ok && p.theta.alloc(P) == hipSuccess && p.m.alloc(P) == hipSuccess && p.v.alloc(P) == hipSuccess;
    ok = ok && p.G.alloc(P) == hipSuccess && p.part.alloc(p.parts) == hipSuccess && p.advstat.alloc(2) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)ppo_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    if (ok) {
        const PpoAdamArgs a = ppo_adam_args(s, 2);
        hipLaunchKernelGGL(ppo_adam_kernel, dim3((unsigned)((P + PPO_RED - 1) / PPO_RED)), dim3(PPO_RED), 0, c->stream, a);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
    }
    if (!ok) { ppo_release(s); (void)hipGetLastError(); return fail("ppo_attach: allocation failed"); }
    p.clip = clip_range; p.ent = ent_coef; p.vf = vf_coef; p.max_norm = max_grad_norm; p.normalize = normalize_advantage ? 1 : 0;
    p.on = true;
    return 0;
}

// a workspace of the trainer, grown on demand
template <typename T>
static int ppo_reserve(DevBuf<T> &buf, size_t n)
{
    if (buf.reserve(n) == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail("ppo: allocation failed");
}
// workspaces of a minibatch of up to `rows` rows (a multiple of 16): activations and deltas of every layer, the row records
static int ppo_reserve_rows(tum_sim *s, size_t rows)
{
    SimTrainer &p = s->ppo;
    int rc = ppo_reserve(p.rowrec, rows * PPO_ROW);
    for (int ni = 0; ni < 2; ni++)
        for (int l = 0; l < p.net[ni].n_mat; l++) {
            PpoNet &t = p.net[ni]; SimTrainer::Layers &own = p.layers[ni];
            rc = rc || ppo_reserve(own.h[l], rows * t.hs[l]) || ppo_reserve(own.d[l], rows * t.mp[l]);
            t.h[l] = own.h[l].get(); t.d[l] = own.d[l].get();          // (the views follow their owners)
        }
    return rc;
}

// the columns of a training buffer on the device
struct PpoData { const double *obs; int stride; const double *act, *old_logp, *adv, *ret; };

// One minibatch on the capsule's stream, nothing waited for: rows idx[0 .. n) of the buffer (idx null: 0 .. n - 1); its diagnostics to
// dstats. apply 0: loss, gradients and their norm alone.
static int ppo_minibatch_enqueue(tum_sim *s, const PpoData &d, const int *idx, int n, double lr, int apply, double *dstats)
{
    tum_ocp *c = s->c; SimTrainer &p = s->ppo;
    const int rows = (n + POL_TILE - 1) & ~(POL_TILE - 1);
    PpoStatsArgs sa;
    sa.n = n; sa.normalize = p.normalize; sa.idx = idx; sa.adv = d.adv; sa.out = p.advstat.get();
    LAUNCH(ppo_stats_kernel, dim3(1), dim3(PPO_RED), 0, c->stream, sa);
    PpoTileArgs ta{};
    ta.pi = s->pol.a; ta.vf = s->val.a; ta.tp = p.net[0]; ta.tv = p.net[1];
    ta.pi.n = ta.vf.n = n; ta.pi.obs = ta.vf.obs = d.obs; ta.pi.obs_stride = ta.vf.obs_stride = d.stride;
    ta.rows = std::max(s->pol.a.rows, s->val.a.rows); ta.idx = idx;
    ta.act = d.act; ta.old_logp = d.old_logp; ta.adv = d.adv; ta.ret = d.ret; ta.advstat = p.advstat.get();
    ta.clip = p.clip; ta.ent_coef = p.ent; ta.vf_coef = p.vf; ta.rowrec = p.rowrec.get();
    LAUNCH(ppo_tile_kernel, dim3(rows / POL_TILE), dim3(64 * POL_WAVES), sizeof(double) * 2 * ta.rows * POL_TILE, c->stream, ta);
    PpoGradArgs ga{};
    ga.net[0] = p.net[0]; ga.net[1] = p.net[1]; ga.rows = rows; ga.G = p.G.get();
    ga.goff[0] = 0; ga.goff[1] = ppo_value_offset(s);
    int tiles = 0;
    for (int ni = 0; ni < 2; ni++)
        for (int l = 0; l < POL_MAXMAT; l++) {
            const PpoNet &t = ga.net[ni];
            ga.first[ni * POL_MAXMAT + l] = tiles;
            if (l < t.n_mat) tiles += (t.mp[l] / 16) * (t.hs[l] / 16 + 1);
        }
    ga.first[2 * POL_MAXMAT] = tiles;
    LAUNCH(ppo_wgrad_kernel, dim3(tiles), dim3(64), 0, c->stream, ga);
    PpoNormArgs na;
    na.P = p.P; na.n_parts = p.parts; na.n = n; na.G = p.G.get(); na.rowrec = p.rowrec.get();
    na.ent_coef = p.ent; na.vf_coef = p.vf; na.parts = p.part.get(); na.stats = dstats;
    LAUNCH(ppo_norm_kernel, dim3(p.parts + 1), dim3(PPO_RED), 0, c->stream, na);
    PpoAdamArgs aa = ppo_adam_args(s, apply ? 1 : 0);
    aa.stats = dstats;
    if (apply) {
        const double t = (double)(p.t + 1);
        aa.step = lr / (1.0 - std::pow(aa.beta1, t)); aa.bc2_sqrt = std::sqrt(1.0 - std::pow(aa.beta2, t));
    }
    LAUNCH(ppo_adam_kernel, dim3(apply ? (p.P + PPO_RED - 1) / PPO_RED : 1), dim3(PPO_RED), 0, c->stream, aa);
    if (apply) p.t++;
    return 0;
}

// a host buffer of N rows into the trainer's own device copy: observations N x n_obs, then actions (as doubles), old log-probabilities,
// advantages and returns, N each
static int ppo_upload(tum_sim *s, size_t N, const double *obs, const int *actions, const double *old_logp, const double *adv, const double *ret, PpoData *d)
{
    const size_t no = s->pol.a.n_in; const int n_act = s->pol.a.n_act;
    if (ppo_reserve(s->ppo.data, N * (no + 4))) return 1;
    std::vector<double> act(N);
    for (size_t i = 0; i < N; i++) {
        if (actions[i] < 0 || actions[i] >= n_act) return fail("ppo: action of row " + std::to_string(i) + " is outside the policy's " + std::to_string(n_act));
        act[i] = (double)actions[i];
    }
    double *p = s->ppo.data.get();
    HIPCHK(hipMemcpy(p, obs, sizeof(double) * N * no, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p + N * no, act.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p + N * (no + 1), old_logp, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p + N * (no + 2), adv, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p + N * (no + 3), ret, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    d->obs = p; d->stride = (int)no; d->act = p + N * no; d->old_logp = p + N * (no + 1); d->adv = p + N * (no + 2); d->ret = p + N * (no + 3);
    return 0;
}

// One minibatch of n host rows. apply 0 computes loss and gradients only: parameters, moments and the step counter stay as they are.
// stats_out: TUM_PPO_STATS doubles. grads_out (optional): the UNCLIPPED gradients, the flat parameter vector in torch's layout (per net
// W_0 row-major (out, in), b_0, W_1, ...; policy net then value net). rows_out (optional): n x 2, the log-probability of the row's
// action and its value as the tile kernel computed them.
extern "C" int tum_sim_ppo_step(tum_sim *s, int n, const double *obs, const int *actions, const double *old_log_probs, const double *advantages,
                                const double *returns, double lr, int apply, double *stats_out, double *grads_out, double *rows_out)
{
    if (!s || !obs || !actions || !old_log_probs || !advantages || !returns || !stats_out) return fail("null argument");
    if (!s->ppo.on) return fail("ppo_step: no trainer attached (tum_sim_ppo_attach)");
    if (n < 1) return fail("ppo_step: n < 1");
    tum_ocp *c = s->c; SimTrainer &p = s->ppo;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t rows = ((size_t)n + POL_TILE - 1) & ~(size_t)(POL_TILE - 1);
    PpoData d;
    if (ppo_upload(s, n, obs, actions, old_log_probs, advantages, returns, &d)) return 1;
    if (ppo_reserve_rows(s, rows) || ppo_reserve(p.stats, (size_t)PPO_STATS)) return 1;
    if (ppo_minibatch_enqueue(s, d, nullptr, n, lr, apply, p.stats.get())) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(stats_out, p.stats.get(), sizeof(double) * PPO_STATS, hipMemcpyDeviceToHost));
    if (grads_out) HIPCHK(hipMemcpy(grads_out, p.G.get(), sizeof(double) * p.P, hipMemcpyDeviceToHost));
    if (rows_out) {
        std::vector<double> rec((size_t)n * PPO_ROW);
        HIPCHK(hipMemcpy(rec.data(), p.rowrec.get(), sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) { rows_out[2 * i] = rec[(size_t)i * PPO_ROW + PPO_R_LOGP]; rows_out[2 * i + 1] = rec[(size_t)i * PPO_ROW + PPO_R_V]; }
    }
    return 0;
}

// One whole update: n_epochs passes over the N buffer rows, pass e in the order perm[e][0 .. N), cut into minibatches of batch_size
// rows (the last one may be short); every minibatch's chain is enqueued, one wait, one download of n_epochs x ceil(N / batch_size) x
// TUM_PPO_STATS diagnostics. obs .. returns all NULL: the buffer the last tum_sim_env_collect left on the device (row e B + b).
extern "C" int tum_sim_ppo_update(tum_sim *s, int N, const double *obs, const int *actions, const double *old_log_probs, const double *advantages,
                                  const double *returns, const int *perm, int n_epochs, int batch_size, double lr, double *stats_out)
{
    if (!s || !perm || !stats_out) return fail("null argument");
    if (!s->ppo.on) return fail("ppo_update: no trainer attached (tum_sim_ppo_attach)");
    if (N < 1 || n_epochs < 1) return fail("ppo_update: N and n_epochs must be >= 1");
    if (batch_size < 1) return fail("ppo_update: batch_size < 1");
    const bool resident = !obs && !actions && !old_log_probs && !advantages && !returns;
    if (!resident && (!obs || !actions || !old_log_probs || !advantages || !returns)) return fail("ppo_update: a buffer is all five arrays, or none of them");
    if (resident && s->col.rows == 0) return fail("ppo_update: no buffer given and no collection on the device (tum_sim_env_collect)");
    if (resident && s->col.rows != (size_t)N) return fail("ppo_update: the collection on the device has " + std::to_string(s->col.rows) + " rows, not " + std::to_string(N));
    for (size_t i = 0; i < (size_t)n_epochs * N; i++)
        if (perm[i] < 0 || perm[i] >= N) return fail("ppo_update: perm[" + std::to_string(i / N) + "][" + std::to_string(i % N) + "] is outside the buffer");
    tum_ocp *c = s->c; SimTrainer &p = s->ppo;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    const int bs = std::min(batch_size, N), n_mb = (N + bs - 1) / bs;
    PpoData d;
    if (resident) {
        const size_t EB = N; const double *col = s->col.buf.get();
        d.obs = col + COL_FIELDS * EB; d.stride = s->pol.a.n_in; d.act = col + COL_ACTION * EB; d.old_logp = col + COL_LOGP * EB;
        d.adv = col + COL_ADV * EB; d.ret = col + COL_RET * EB;
    } else if (ppo_upload(s, N, obs, actions, old_log_probs, advantages, returns, &d)) return 1;
    const size_t n_stats = (size_t)n_epochs * n_mb * PPO_STATS;
    if (ppo_reserve_rows(s, ((size_t)bs + POL_TILE - 1) & ~(size_t)(POL_TILE - 1)) || ppo_reserve(p.stats, n_stats) ||
        ppo_reserve(p.idx, (size_t)n_epochs * N)) return 1;
    HIPCHK(hipMemcpy(p.idx.get(), perm, sizeof(int) * (size_t)n_epochs * N, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    for (int e = 0; e < n_epochs; e++)
        for (int k = 0; k < n_mb; k++)
            if (ppo_minibatch_enqueue(s, d, p.idx.get() + (size_t)e * N + (size_t)k * bs, std::min(bs, N - k * bs), lr, 1,
                                      p.stats.get() + ((size_t)e * n_mb + k) * PPO_STATS)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(stats_out, p.stats.get(), sizeof(double) * n_stats, hipMemcpyDeviceToHost));
    return 0;
}

// the float32 parameters the device acts with, per matrix as the attach functions take them (W[l]: (out, in) row-major)
extern "C" int tum_sim_ppo_params(tum_sim *s, float *const *W, float *const *b, float *const *VW, float *const *Vb)
{
    if (!s || !W || !b || !VW || !Vb) return fail("null argument");
    if (!s->ppo.on) return fail("ppo_params: no trainer attached (tum_sim_ppo_attach)");
    DevGuard guard(s->c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(s->c->stream));
    std::vector<float> th(s->ppo.P);
    HIPCHK(hipMemcpy(th.data(), s->ppo.theta.get(), sizeof(float) * th.size(), hipMemcpyDeviceToHost));
    for (int ni = 0; ni < 2; ni++) {
        const PpoNet &t = s->ppo.net[ni];
        float *const *Wo = ni ? VW : W, *const *bo = ni ? Vb : b;
        const size_t base = ni ? ppo_value_offset(s) : 0;
        for (int l = 0; l < t.n_mat; l++) {
            if (!Wo[l] || !bo[l]) return fail("null argument");
            const size_t nw = (size_t)t.out[l] * t.in[l];
            memcpy(Wo[l], &th[base + t.off[l]], sizeof(float) * nw);
            memcpy(bo[l], &th[base + t.off[l] + nw], sizeof(float) * t.out[l]);
        }
    }
    return 0;
}

// Adam's state: the moments over the flat parameter vector (n_params doubles each; either may be NULL) and the step counter
extern "C" int tum_sim_ppo_state(tum_sim *s, double *m, double *v, long long *t, int *n_params)
{
    if (!s) return fail("null argument");
    const SimTrainer &p = s->ppo;
    if (!p.on) return fail("ppo_state: no trainer attached (tum_sim_ppo_attach)");
    DevGuard guard(s->c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(s->c->stream));
    if (m) HIPCHK(hipMemcpy(m, p.m.get(), sizeof(double) * p.P, hipMemcpyDeviceToHost));
    if (v) HIPCHK(hipMemcpy(v, p.v.get(), sizeof(double) * p.P, hipMemcpyDeviceToHost));
    if (t) *t = p.t;
    if (n_params) *n_params = p.P;
    return 0;
}
