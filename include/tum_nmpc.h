/*
 * include/tum_nmpc.h -- C-ABI of libtumnmpc.so, the MI355X-native batched SQP-RTI solver.
 *
 * Drop-in boundary: the reference drives its solver through acados_template.AcadosOcpSolver
 * (a ctypes wrapper around the generated libacados_ocp_solver_<name>.so). Every entry point
 * below replaces one AcadosOcpSolver method the reference calls; the reference call sites are
 * cited per function (paths relative to bzarr/TUM-CONTROL). All functions take plain pointers
 * and sizes; no torch / C++ types cross the boundary.
 *
 * New relative to acados: a leading BATCH dimension. A capsule owns `batch` independent OCP
 * instances (perturbed-x0 / sigma-point / Monte-Carlo / weight-sweep fan-outs); one wavefront
 * solves one instance. Host buffers passed to set/get hold `nb` consecutive instances
 * [b0, b0+nb), `stride` doubles apart (stride 0 on a set = broadcast one record to all nb).
 *
 * Conventions: doubles everywhere; matrices column-major like acados; every set/get COPIES
 * (caller owns host buffers, capsule owns device memory); return 0 on success, non-zero on
 * error with the message available from tum_ocp_last_error(). One host thread per capsule.
 */
#ifndef TUM_NMPC_H
#define TUM_NMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define TUM_NX 8          /* [posx,posy,yaw,vlong,vlat,yawrate,delta_f,a]  pred_model_dynamic_stm_pacejka.py:80-93 */
#define TUM_NU 2          /* [jerk, steering_rate]                                                        :96-98   */
#define TUM_NY 6          /* cost_y_expr = [x0,x1,wrap(yaw),vlong,u]        NMPC_STM_acados_settings.py:51 */
#define TUM_NYE 4
#define TUM_N_MAX 56      /* horizon limit of this build: N <= 40 (five 16-wide MFMA tiles of condensed variables) on every kernel
                             variant, 41..48 (six tiles) on the pipeline variant only (nominal and coupled SNMPC OCP), 49..56 (seven
                             tiles, round 6: Tp = 4.0 s at Ts_MPC = 0.08 s is N = 50) with a diagonal W (nominal, R2 and coupled SNMPC OCP) */
#define TUM_ALL_STAGES (-1)

/* acados return codes the callers test (NMPC_class.py:183-206, main.py:59-61) */
#define TUM_SUCCESS 0
#define TUM_QP_FAILURE 4

typedef struct tum_ocp tum_ocp;           /* opaque capsule (acados: nlp_solver_capsule) */

/* Problem description = what NMPC_STM_acados_settings.py:16-245 bakes into the generated solver. */
typedef struct tum_ocp_desc {
    int N;                 /* shooting intervals, ocp.dims.N                     :34  */
    int nsub;              /* sim_method_num_steps (ERK4 sub-steps)              :240 */
    double dt;             /* Tf / N                                             :230 */
    int batch;             /* number of independent OCP instances                     */
    int device;            /* HIP device ordinal                                      */
    /* single-track / Pacejka constants, Config/EDGAR/veh_params_pred.yaml, pacejka_params.yaml,
       pred_model_dynamic_stm_pacejka.py:33-46 */
    double lf, lr, m, Iz, ro, S, Cd;
    double Bf, Cf, Df, Ef, Br, Cr, Dr, Er;
    double g, fr0, fr1, fr4;
    double acc_min;        /* braking limit used as ax_max when a < 0            NMPC_STM_acados_settings.py:74 */
    /* velocity-dependent gg limits, Config/EDGAR/ggv.csv via NMPC_class.py:322-335 */
    int n_ggv;
    double ggv_v[16], ggv_ax[16], ggv_ay[16];
    /* QP solver options (acados: qp_solver_iter_max :232, HPIPM tolerances json:904-950) */
    int qp_iter_max;
    double qp_tol_stat, qp_tol_ineq, qp_tol_comp;
    double qp_mu0;         /* initial complementarity target of the interior point method (default 0.05) */
    double qp_t0;          /* floor of the initial constraint residuals (default 0.05) */
    int store_qp_in;       /* keep A_k,B_k,b_k of the last linearisation for tum_ocp_get_from_qp_in */
    /* acados: qp_solver_warm_start (1 in Stochastic_NMPC/SNMPC_acados_settings.py:307, unset = 0 for the nominal solver). != 0: in a
     * sequence of solves the interior point method of an instance starts from the multipliers and violation slacks its previous QP
     * ended with -- when that QP converged and the new problem is close to it (at most 16 row sides changed their activity, no new
     * violation above 0.1; otherwise it starts cold); tum_ocp_cold_start / tum_ocp_reset forget them -- pushed back into the interior and
     * re-centred to the complementarity target qp_warm_mu (0: the default 1e-2). The QP solution is the same to the solver's
     * tolerances; 9 % fewer interior point iterations over the reference's logged closed loops (profiles/r05_ipm_iterations.txt).
     * The Python binding switches it on by default for every controller -- for the nominal and R2 solvers a documented deviation from
     * the reference's setting ("Interior point warm start"). */
    int qp_warm_start;
    double qp_warm_mu;
    /* the proximity gate of the warm start: an instance starts warm only when at most qp_warm_flips row sides changed their activity
     * against the previous QP (0: the default 16; < 0: no gate -- a development aid, measured to stall solves at the iteration cap on
     * jumping sequences, profiles/r05_warm_gate.txt) and no new violation exceeds qp_warm_viol (0: the default 0.1). */
    int qp_warm_flips;
    double qp_warm_viol;
} tum_ocp_desc;

/* AcadosOcpSolver(ocp, json_file=..., generate=..., build=...)   NMPC_STM_acados_settings.py:243 */
tum_ocp *tum_ocp_create(const tum_ocp_desc *desc);
void tum_ocp_free(tum_ocp *c);
const char *tum_ocp_last_error(void);
int tum_ocp_batch(const tum_ocp *c);
int tum_ocp_horizon(const tum_ocp *c);

/* acados_solver.set(stage, field, value)   NMPC_class.py:172,178,254; SNMPC_class.py:124,130
 * field: "x" (8), "u" (2), "yref" (6 for stage<N, 4 for stage N); on an SNMPC capsule also
 * "p" (L*ns + 2 values = [A_pce.flatten(), risk_parameter, stop_flag], SNMPC_class.py:124,185,193; b0 = 0, nb = batch,
 * stride 0: the parameter vector is shared by the batch). A_pce and the risk parameter are shared by all stages (the
 * reference sends every stage the same values; a differing risk parameter is an error at the next solve); the stop flags
 * must be 0 on the stages < uph and 1 from stage uph on (SNMPC_class.py:103-104) and DEFINE the uncertainty propagation
 * horizon of the next solve (any other pattern is an error at the next solve).
 * stage == TUM_ALL_STAGES: v holds all stages back to back ("x": (N+1)*8, "u": N*2, "yref": (N+1)*6
 * with the terminal record padded to 6). */
int tum_ocp_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride);
/* acados_solver.get(stage, field)          NMPC_class.py:193,198; Reduced_Robustified_NMPC_class.py:280,298
 * field: "x", "u" (and the soft-constraint slacks of the last QP: "sl", "su", 3 per stage in acados order);
 * "lam": the multipliers of the last QP's rows, per stage the lower sides in the order of "sl", then the upper sides in the order of
 * "su" -- 2 / 6 / 4 values at stage 0 / 1..N-1 / N. (acados appends the multipliers of the slack bounds; this getter does not.)
 * After a full SQP solve they are the multipliers the reported residuals were evaluated with. */
int tum_ocp_get(tum_ocp *c, int stage, const char *field, double *v, int len, int b0, int nb, int stride);

/* acados_solver.constraints_set(stage, field, value)   NMPC_class.py:111-112,245-246;
 * Reduced_Robustified_NMPC_class.py:335-336,359,362-365
 * stage 0 "lbx"/"ubx" (8 values) = initial state x0 (initial-value embedding);
 * stage>=1 "lbx"/"ubx" (1 value) = steering-angle bound; "lbu"/"ubu" (1) = steering-rate bound;
 * "lh"/"uh" (1) = bounds of the gg-circle constraint. */
int tum_ocp_constraints_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride);

/* acados_solver.cost_set(stage, field, value)   NMPC_class.py:295-317
 * "W": ny*ny (stage<N: 36, stage N: 16) column-major. Any matrix, as in acados (its symmetric part is what the cost sees and what is kept). The
 * reference only installs blockdiag(Q,R) with diagonal Q, R: a capsule whose W have always been diagonal stores the diagonal and condenses with the
 * kernels of the headline; the first W with an off-diagonal entry switches the capsule to a full 6 x 6 per stage (nominal / R2 OCP on the pipeline;
 * the condensing then runs as the six-wavefront kernel's full-W instantiation whatever the batch size; refused by the coupled SNMPC OCP, whose cost
 * rows come from the prologue kernel, and by the development build's fused kernel). Per STAGE, as in acados: the reference sets every stage in a loop (NMPC_class.py:294-296), and a caller may
 * give every stage its own weights. stage == TUM_ALL_STAGES with a 6 x 6 W: all the stages 0..N-1 in one call. (The development
 * build's fused kernel reads stage 0's W for all stages < N; the shipped pipeline honours every stage.)
 * "zl","zu","Zl","Zu": 1 value at stage 0 [sbu], 3 at stages 1..N-1 [sbu,sbx,sh], 2 at stage N [sbx,sh]. */
int tum_ocp_cost_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride);

/* status = acados_solver.solve()   NMPC_class.py:183, SNMPC_class.py:198, Reduced_Robustified_NMPC_class.py:264
 * One SQP real-time iteration for every instance. Returns the max status over the batch
 * (0 ok, 4 QP failure); per-instance values via tum_ocp_get_stats("status"). Synchronous.
 * The reference's LITERAL per-step call sequence on a small capsule (batch x (N+1) x 8 <= 32768 doubles, N <= 63) -- N+1 x
 * set(j,"yref"), constraints_set(0,"lbx"|"ubx"), solve(), get(0,"u"), N x get(j,"x"), get_cost(), 3 x get_stats, NMPC_class.py:169-206,
 * 243-246 -- costs ONE device round trip: the per-stage "yref" setters and the stage-0 "lbx"/"ubx" land in a pinned shadow the capsule
 * owns (with a map of the stages touched) and go up in one kernel in front of the solve; the solve ends with one kernel that writes
 * u0 / cost / status / qp_iter and the whole iterate into pinned slabs; get "x" / "u", get_cost and get_stats "qp_iter" / "status" are
 * then host copies until something changes the iterate (a set "x"/"u", reset, cold start, device upload, another solve). Same numbers as
 * the one-call step (tum_ocp_step_async) and as the uncached getters, bit for bit (tests/test_gpu_call_sequence.py). On such a capsule
 * the solve is timed by the device's wall clock (get_stats "time_tot") and the events around the interior point kernel are left out
 * (get_stats "time_ipm" needs tum_ocp_set_kernel(c, "time-ipm")). */
int tum_ocp_solve(tum_ocp *c);
/* Asynchronous flavour for benchmarking / pipelining: enqueue on the capsule's stream, no host sync.
 * In SQP mode (tum_ocp_options_set) it returns behind the enqueue of the last iteration: the host reads the number of active
 * instances between two iterations. */
int tum_ocp_solve_async(tum_ocp *c);
/* acados_solver.options_set(field, value) for the NLP solver (acados_ocp_SNMPC.json: nlp_solver_*) and its globalization:
 * "nlp_solver_type"        0 SQP_RTI (default: one QP per solve, as before), 1 SQP (full solves)
 * "nlp_solver_max_iter"    1..10000 QPs per SQP solve (default 100)
 * "nlp_solver_tol_stat" | "nlp_solver_tol_eq" | "nlp_solver_tol_ineq" | "nlp_solver_tol_comp"   >= 0 (default 1e-6 each)
 * "nlp_solver_step_length" in (0, 1] (default 1)
 * An SQP solve evaluates the four NLP residuals of every instance at each iterate (after its linearisation, with the previous QP's
 * multipliers), stops an instance whose residuals are all below their tolerances and ends when none is active or after max_iter QPs.
 * Per-instance status: 0 converged, 2 max_iter reached (ACADOS_MAXITER), 4 a QP failed (the iterate stays at the last good one).
 * SQP is refused for a capsule with the R2NMPC tightening attached, for the coupled SNMPC OCP, for the development kernels "fused" /
 * "pipeline4", by tum_ocp_step_async and by the device closed loop (tum_sim_*): those stay SQP-RTI.
 *
 * "globalization"          0 FIXED_STEP (default: every instance moves by nlp_solver_step_length), 1 MERIT_BACKTRACKING: a step length per
 *                          instance and per iteration, chosen by a line search on an L1 merit function. Read by an SQP solve only (an
 *                          SQP-RTI solve and rti_phase are unaffected).
 * "alpha_min"              in (0, 1] (default 0.05, acados')      "alpha_reduction"   in (0, 1) (default 0.7, acados')
 * "merit_weight_eq"        finite, >= 0 (default 1): the weight mu_eq of the shooting defects. Not an acados name: acados weights them
 *                          with the multipliers of the dynamics, which condensing does not keep.
 * The candidates are alpha_j = alpha_reduction^j (formed as j products), j = 0 .. K - 1, K = 1 + floor(log alpha_min / log alpha_reduction):
 *   9 with the defaults, the smallest 0.7^8 = 0.0576. A solve with K > 16 is refused, and so is one with MERIT_BACKTRACKING and
 *   nlp_solver_step_length != 1.
 * Merit function at z = (X, U, sl, su):  phi(z) = cost(z) + mu_eq E(z) + mu_in V(z), with cost the value get_cost reports (wrapped yaw,
 *   stage terms scaled by dt, diagonal or full W, z s + Z s^2 / 2 per row side), E = |x0 - X_0|_1 + sum_k |f(X_k, U_k) - X_{k+1}|_1 with f the
 *   ERK4 x nsub integrator of the model, V = the sum over the row sides of max(0, -t), t = value - lo + s_l (lower) or hi - value + s_u
 *   (upper), with the row's value -- U[k][1], X[s][6], the gg expression at X_s -- AT z, not its linearisation. mu_in is kept per
 *   instance: 0 at the start of every SQP solve, then the largest |multiplier| of the rows over the QPs of this solve, the QP just solved
 *   included.
 * Line search: with z_prev the iterate in front of the QP and z_qp what the interior point method and the expansion return,
 *   z(alpha) = z_prev + alpha (z_qp - z_prev). Accepted is the first j with phi(z(alpha_j)) < phi(z(0)) (simple decrease, acados'
 *   line_search_use_sufficient_descent = 0), else alpha_{K-1}. X, U, slacks and multipliers move by the accepted alpha; an instance that
 *   took alpha < 1 starts its next QP cold (interpolated multipliers are no warm start). All candidates of all instances are evaluated
 *   by ONE kernel launch per iteration (sqp_merit_kernel). Finished instances and failed QPs are treated as under FIXED_STEP. The
 *   reported cost is that of the returned iterate.
 *
 * "rti_phase"              acados' split of the real-time iteration: 0 preparation and feedback in one solve (default, as before),
 *                          1 PREPARATION, 2 FEEDBACK; any other value is an error.
 * rti_phase 1: tum_ocp_solve / tum_ocp_solve_async upload the pending inputs and run what does not need the measured state -- the
 *   linearisation and the condensing, the kernels a one-call solve of this capsule would run -- at the x0 the capsule holds, and keep
 *   a device copy of that x0. Iterate, cost, status, qp_iter, qp_status, res, slacks and multipliers are untouched. Returns 0 (acados
 *   >= 0.3 returns ACADOS_READY = 5 here; the reference's callers take every non-zero status for a failure). get_stats "time_tot" is
 *   the preparation's device time.
 * rti_phase 2: the pending x0 goes up, rti_feedback_kernel applies x0 - x0_prep to the gradient q and the row constants d of the
 *   prepared QP (both affine in x0; nothing else of the QP depends on it), then the interior point method and the expansion run as in
 *   a one-call solve (longest-first order, fused expansion, warm start, "time_tot" / "time_ipm", the single device round trip of a
 *   small capsule's tum_ocp_solve). Returns the maximum status. At an unchanged x0 the result is the one-call solve's, bit for bit.
 *   A feedback CONSUMES its preparation: without one -- or a second time -- it fails and leaves the iterate alone.
 * Between the two the caller may change x0 by every route (constraints_set(0, "lbx" | "ubx"), put_device "x0", set_x0_fanout), read
 *   anything, and change the bounds of the stages >= 1 and the penalties zl / zu / Zl / Zu (the interior point kernel reads them, in
 *   the feedback). Whatever else the preparation has read makes it STALE and the feedback fail: set "x" | "u" | "yref", cost_set "W",
 *   put_device "X" | "U" | "yref", bind_device, cold_start, reset, set_kernel. A solve in rti_phase 0 discards a pending preparation.
 * tum_ocp_step_async: rti_phase 2 with yref = NULL is the one-call feedback step; with a yref (the reference enters in the
 *   preparation) and in rti_phase 1 (a preparation has no results) it is an error.
 * Refused, here where the condition is known and again by the solve: the coupled SNMPC OCP, a capsule with the R2NMPC tightening
 *   attached or with a full W, SQP mode (in either order of setting), the development kernels "fused" / "pipeline4", the debug dump
 *   and the phase timers, and tum_sim_create / tum_sim_run on a capsule whose rti_phase is not 0.
 *
 * "lin_dedup"              1 (default): while the iterate is the same at every stage -- after cold_start() or reset(), until anything
 *                          writes it: set "x" | "u", put_device "X" | "U", a solve that expands, the device closed loop -- the
 *                          linearisation runs the Runge-Kutta pass once per instance instead of once per stage and fills the stage
 *                          records from it (lin_uniform_kernel + lin_fill_kernel). The records, and every result, are bit-identical to
 *                          the general linearisation's. 0: always the general linearisation (A/B runs, tests). Applies where the
 *                          lane-per-stage kernel of the nominal OCP would run: not on the eight-lane latency path, not to the
 *                          coupled SNMPC OCP, not in the device closed loop (tum_sim_run captures and replays its steps). A caller who
 *                          captures solves into a graph of their own captures the cold_start() with them, or sets 0. The fill kernel compares every stage with stage 0: should the
 *                          library ever take the path on a non-uniform iterate, every synchronous call fails and says so until the next
 *                          cold_start() / reset(), which re-initialise the iterate and re-arm the check.
 * "uniform_records"        0 (default): a solve on the "lin_dedup" path does not materialise the stage records where nothing reads them:
 *                          the condensing and the expansion form their operands from the once-per-instance linearisation and the
 *                          reference (cond_uniform_kernel, expand_uniform_kernel; lin_fill_kernel is not launched, and the expansion
 *                          holds the check of every stage against stage 0). Taken by a whole SQP-RTI step (rti_phase 0) of the nominal
 *                          OCP with a diagonal W, created without store_qp_in, at batch sizes where the condensing runs one wavefront
 *                          per OCP and the expansion is a kernel of its own (more than 1024 instances), without the debug dump or the
 *                          phase timers; every other solve fills the records as before. Results are bit-identical either way.
 *                          1: always fill the records (A/B runs, tests).
 * "uniform_powers"         1 (default): the condensing of that record-free path computes what is the same on every lane once per
 *                          instance -- the sequences A^m B and g_{s+1} = A g_s + defect -- and its stages read them from tables
 *                          (cond_uniform_kernel). 0: every lane carries its column of G through every stage
 *                          (cond_uniform_columns_kernel; A/B runs, tests). Results are bit-identical either way.
 * "uniform_shift"          1 (default): cond_uniform_kernel at N <= 40 decides per instance whether the four cost weights of W are the
 *                          same doubles (bit patterns; no NaN) at the stages 1 .. N - 1. Where they are, tile (j, I + j) of the
 *                          condensed Hessian is tile (0, I) as it stood 8 j stages earlier plus the terminal stage's product, and
 *                          only block row 0 is accumulated: 130 matrix products at N = 40, not 280. Every other instance runs the
 *                          stage loop with all its products, as does 0 (A/B runs, tests). Results are bit-identical either way. */
int tum_ocp_options_set(tum_ocp *c, const char *field, double value);
int tum_ocp_synchronize(tum_ocp *c);

/* acados_solver.get_cost()   NMPC_class.py:202 */
int tum_ocp_get_cost(tum_ocp *c, double *out, int b0, int nb);
/* acados_solver.get_stats(field)   NMPC_class.py:203-205
 * "time_tot" -> 1 double, device seconds of the last solve (HIP events on the capsule's stream)
 * "sqp_iter" -> nb ints (1 after an SQP-RTI solve; the QPs each instance solved after an SQP solve), "qp_iter" -> nb ints,
 * "status" -> nb ints, "qp_status" -> nb ints
 * "res" -> nb x 3 doubles (stat, ineq, comp residuals of the last QP)
 * "residuals" -> nb x 4 doubles (stat, eq, ineq, comp residuals of the NLP at the returned iterate; after an SQP solve only).
 * After an SQP solve with globalization MERIT_BACKTRACKING only (refused otherwise):
 * "merit_dims" -> 2 ints: K, the number of candidates, and M, the nlp_solver_max_iter of that solve
 * "alpha" -> nb x M doubles: row b holds the accepted alpha of its QPs 1 .. sqp_iter[b], then zeros (a QP that failed has no line
 *   search: its entry stays 0)
 * "merit" -> nb x (K + 1) x 3 doubles: cost, E, V of the instance's own LAST line search at the candidates j = 0 .. K - 1 and, in row K,
 *   at alpha = 0 (zeros for an instance that never searched)
 * "merit_weights" -> nb x 2 doubles: mu_eq, mu_in
 * "lin_uniform" -> 1 int: linearisations of this capsule that took the uniform path (options_set "lin_dedup") since it was created.
 * "records_skipped" -> 1 int: solves of this capsule that ran without stage records (options_set "uniform_records") since it was created.
 * "cond_shifted" -> 1 int: instances of the LAST solve whose condensing took the shift form (options_set "uniform_shift"); 0 where the
 *   last condensing was not cond_uniform_kernel.
 * "lpt_order" -> nb ints: entries b0 .. b0 + nb - 1 of the longest-first order the NEXT solve dispatches in (tum_ocp_set_schedule): the
 *   last solve's iteration counts, clipped to 0..63, descending; instances of one count by ascending index. The identity map while no
 *   order is kept (a batch of at most 1024, before the first solve). */
int tum_ocp_get_stats(tum_ocp *c, const char *field, void *out, int b0, int nb);
/* acados_solver.reset()   NMPC_class.py:251 -- zero the iterate of every instance */
int tum_ocp_reset(tum_ocp *c);
/* acados_solver.get_from_qp_in(stage, "A")   Reduced_Robustified_NMPC_class.py:295
 * "A" (64, column-major 8x8), "B" (16, column-major 8x2), "b" (8) of the LAST linearisation. */
int tum_ocp_get_from_qp_in(tum_ocp *c, int stage, const char *field, double *out, int len, int b0, int nb, int stride);

/* Device-side plumbing (no reference counterpart): use an external HIP stream (e.g. torch's current
 * stream) and copy results device-to-device into caller-owned HBM (for the RCCL gather). */
int tum_ocp_set_stream(tum_ocp *c, void *hip_stream);
/* field: "u0" (nb x 2), "x1" (nb x 8), "cost" (nb), "X" (nb x (N+1)*8), "U" (nb x N*2),
 * "status" / "qp_iter" (nb int32), "summary" (nb x 5 doubles: u0[2], cost, status, qp_iter -- the slab of the rooted gather),
 * "qp_vec" (nb x 2 NVP doubles, NVP = 80 / 96 / 112 for N <= 40 / 48 / 56: gradient q | row constants d of the condensed QP as the
 * interior point kernel of the last solve -- or the next feedback -- reads them; d[2 (s - 1)], d[2 (s - 1) + 1]: steering angle and gg row of stage s) */
int tum_ocp_get_device(tum_ocp *c, const char *field, void *dev_dst, int b0, int nb);
/* Results on the HOST without stalling the stream (no reference counterpart; the caller it serves reads u0 / pred_X / cost /
 * status after every solve, NMPC_class.py:193-206). tum_ocp_results_async enqueues, on the capsule's stream and behind the
 * solve already enqueued there: the result summary packed on the device (5 doubles per instance: u0[2], cost, status,
 * qp_iter) and its copy into a PINNED host slab the capsule owns -- with_iterate != 0: also the whole iterate X ((N+1)*8
 * doubles per instance) and U (N*2) -- then records an event. It returns at once: a caller that keeps several capsules in
 * flight (streaming.SolverRing) enqueues the next batches while this one's results cross PCIe.
 * A capsule owns TWO sets of slabs and events, used in turn: up to two requests may be outstanding, so a caller can enqueue the
 * next batch and its request BEFORE it reads the previous batch's results (the stream then never runs dry waiting for the host).
 * tum_ocp_results_wait blocks until the event of the OLDEST outstanding request has passed and hands out its pinned slabs
 * (valid until the second-next tum_ocp_results_async on this capsule; X / U are null when that request was made without the
 * iterate). A third request without a wait in between is an error. */
int tum_ocp_results_async(tum_ocp *c, int with_iterate);
int tum_ocp_results_wait(tum_ocp *c, const double **summary, const double **X, const double **U);
/* number of result requests outstanding on this capsule (0, 1 or 2; tum_ocp_step_async makes one): a synchronous caller drains what
 * an earlier, abandoned request left behind before it trusts tum_ocp_results_wait to deliver ITS solve (solver.py: step) */
int tum_ocp_results_outstanding(const tum_ocp *c);
/* One control step of a HOST-driven loop in one call (what NMPC_class.py:163-241 does with 2 + (N+1) setters, solve() and
 * 2 N + 5 getters, each a synchronous round trip): x0 (nb = batch instances x 8; SNMPC capsules: as tum_ocp_put_device "x0") and
 * yref (batch x (N+1) x 6) -- either may be null: the capsule keeps what it has -- are copied into PINNED staging memory the capsule
 * owns and uploaded on its stream, one SQP-RTI is enqueued behind them and a results request (tum_ocp_results_async) behind
 * the solve. Returns after enqueuing; tum_ocp_results_wait delivers summary / X / U. The caller's x0 / yref buffers are free on
 * return. Two steps may be outstanding, like two result requests. Small batches: one kernel reads the staging area, one writes
 * summary and iterate into the pinned slabs, and the step's device time (get_stats "time_tot") is read from the device's wall clock
 * by these two kernels -- no copy command and no event on the stream; get_stats "time_ipm" is not available after a step. One instance, N = 38, warm: 0.34 -> 0.15 ms per control step
 * of the mirrored controller class. */
int tum_ocp_step_async(tum_ocp *c, const double *x0, const double *yref, int with_iterate);
/* The other direction: per-instance inputs from caller-owned DEVICE memory (asynchronous D2D on the capsule's stream).
 * field: "x0" (nb x 8, = constraints_set(0,"lbx")), "yref" (nb x (N+1)*6), "X" (nb x (N+1)*8), "U" (nb x N*2). */
int tum_ocp_put_device(tum_ocp *c, const char *field, const void *dev_src, int b0, int nb);
/* Zero-copy flavour of the above for "x0" / "yref" (whole batch): the capsule USES the caller's device array as its own -- kernels read
 * it in place, setters and the device closed loop write through to it -- until dev_ptr = NULL hands the capsule's own array back. The
 * memory must stay valid, and unchanged by others, while solves that use it are in flight. For callers that rotate batches resident in
 * HBM (bench.py --bind-inputs). Measured (profiles/r05_bind_inputs.txt): the copy kernels of tum_ocp_put_device cost 1.2 % on one stream
 * and disappear behind another capsule's solve with three capsules in flight (4.037 against 4.032 M solves/s). */
int tum_ocp_bind_device(tum_ocp *c, const char *field, void *dev_ptr);
/* cold start every instance on the device: X_k = x0 for all k, U = 0 (acados create / reset + set x;
 * NMPC_class.py:250-254) using the x0 already uploaded with constraints_set(0,"lbx"). */
int tum_ocp_cold_start(tum_ocp *c);
/* Scheduling of the instances onto wavefronts (no reference counterpart). longest_first = 1 (default): workgroup i solves
 * the instance with the i-th largest IPM iteration count of the PREVIOUS solve, so the few long instances of a batch start
 * first instead of leaving the GPU idle at the end (a batch is only a few rounds of resident wavefronts); 0: natural order.
 * Results do not depend on the schedule. Environment override at create time: TUM_NMPC_SCHEDULE=natural. */
int tum_ocp_set_schedule(tum_ocp *c, int longest_first);
/* Kernel variant of the solve (no reference counterpart). The shipped library has ONE: "pipeline" (= "auto", the default):
 * linearise / condense / interior point / expand as four kernels, each at its own occupancy, handing over through an
 * L2-resident workspace; the coupled SNMPC OCP runs its prologue / epilogue kernels around it. get_stats("time_ipm") reports
 * the interior point kernel. The development build (libtumnmpc_dev.so, tests and experiments only) adds the two other
 * implementations the pipeline is held against: "fused" (round 1's single kernel, N <= 40, uph <= 31) and "pipeline4" (the
 * pipeline with the four-wavefront interior point kernel); the shipped library refuses these names. Environment override at
 * create time: TUM_NMPC_KERNEL.
 * Two further names choose the PROLOGUE of a coupled SNMPC capsule without touching the rest: "prologue-mfma" (the column
 * recursions of the samples as v_mfma_f64_4x4x4_4b products; n_samples <= 10, where it is the library's own choice) and
 * "prologue-passes" (the column-slot / pass kernels of rounds 1-3, the only ones for n_samples > 10): two implementations of
 * the same hand-over the tests hold against each other.
 * Small batches are bound by the length of ONE pass of a kernel, not by throughput; for them the library launches wider forms of
 * the first two kernels of the pipeline, and four more names pin the choice (tests, A/B runs):
 *   "lin-eight-lanes" / "lin-lane-per-stage"      linearisation with eight lanes per (instance, stage) -- one sensitivity column per
 *       lane, the tyre chains of the model split over a DPP quad -- or one; default: eight while batch x (N+1) x 8 lanes are one
 *       round of wavefronts (batch <= 199 at N = 40). b_k identical, A_k / B_k to 3e-15 relative (FMA contraction).
 *   "cond-six-wavefronts" / "cond-one-wavefront"  condensing with a workgroup of six (N > 40: seven) wavefronts per OCP -- column
 *       recursion with four lanes per column, Hessian tiles dealt to four wavefronts, gradient on two -- or one wavefront;
 *       default: the workgroup while batch <= 256 (one per CU). Bit-identical results. The nominal OCP only.
 *   "loop-fork" / "loop-serial"   device closed loops (tum_sim_run) of the nominal OCP on the latency path: the linearisation of a
 *       control step's solve runs BESIDE the planner of that step, on a side stream of the simulation (the Runge-Kutta pass needs
 *       the iterate, not the reference; the four residuals of the cost are formed by the condensing kernel) -- or behind it as in
 *       a plain solve. Default: serial (the fork is bit-identical and measured slower: the cross-stream dependencies cost more
 *       than the overlap gains). Environment: TUM_SIM_FORK = 0 | 1.
 * "auto" hands all these choices back to the library. Environment overrides (read once): TUM_LIN_COLS, TUM_COND_WIDE = 0 | 1.
 * Two names are timing options, not kernels: "time-ipm" keeps the two HIP events around the interior point kernel on EVERY solve
 * (get_stats "time_ipm"), also where the library leaves them out -- steps, and synchronous solves of small capsules: every event on the
 * stream is a gap of several microseconds between two kernels; "no-time-ipm" (default) hands that back. */
int tum_ocp_set_kernel(tum_ocp *c, const char *name);
/* last kernel launch time in milliseconds (HIP events on the launch stream) */
double tum_ocp_last_kernel_ms(tum_ocp *c);
/* debug: one solve, then the condensed QP of instance b as the condensing kernel handed it to the interior point kernel
 * (N <= 40): out = [H 80x80 | q 80 | steering-angle row and gg row of every stage, 2N x 80 | their constants 2N]; see
 * csrc/tum_nmpc.hip */
int tum_ocp_debug_dump(tum_ocp *c, int b, double *out, int len);
/* read-only: the condensed QP of the instances b0 .. b0 + nb - 1 as the LAST preparation or solve left it in the hand-over buffers of the
 * pipeline -- every horizon (NVP = 80 | 96 | 112 condensed variables incl. the padding for N <= 40 | 48 | 56), whichever condensing
 * kernel ran. Launches nothing, changes nothing.
 *   info[3]: NVP, 2 N, and 1 where dv is the step of this QP (0: the expansion ran as the tail of the interior point kernel, which
 *            hands no step over -- batches of at most 1024 instances below seven tiles)
 *   H nb x NVP x NVP (diagonal tiles as stored, both triangles) | q, d, dv nb x NVP | C nb x 2 N x NVP
 *   rows: 2 (s - 1) the steering-angle row of stage s (synthesised: dt on the odd columns below 2 s), 2 (s - 1) + 1 its gg row
 * Null array pointers are skipped (all null: info only). Refused before the first pipeline preparation / solve, on the development
 * kernel 'fused' (no hand-over buffers) and for an instance range out of bounds. */
int tum_ocp_get_condensed_qp(tum_ocp *c, int b0, int nb, double *H, double *q, double *C, double *d, double *dv, int *info);
/* read-only: the linearisation of the coupled SNMPC OCP of the instances b0 .. b0 + nb - 1 as the LAST pipeline solve left it. Launches
 * nothing, changes nothing.
 *   info[3]: n_samples, uph, N
 *   stages k < uph, every sample:  As nb x uph x ns x 64, Bs nb x uph x ns x 16 (column-major, expanded like tum_ocp_get_from_qp_in's),
 *                                  bs nb x uph x ns x 8 | gg value hs nb x uph x ns and gradient ghs nb x uph x ns x 8 (entries 3, 4, 5, 7;
 *                                  zeros at stage 0)
 *   nominal copy, every stage:     hn nb x (N + 1), ghn nb x (N + 1) x 8 (entries 3, 4, 5, 7), cv nb x (N + 1) x 2 ((vl, vt) / |v|)
 *   nominal copy, stages k >= uph: An nb x (N - uph) x 64, Bn nb x (N - uph) x 16, bn nb x (N - uph) x 8
 * Null array pointers are skipped (all null: info only). Refused on a capsule that is not the coupled SNMPC one, before the first
 * pipeline solve, on the development kernel 'fused' and for an instance range out of bounds. */
int tum_ocp_get_snmpc_linearisation(tum_ocp *c, int b0, int nb, double *As, double *Bs, double *bs, double *hs, double *ghs,
                                    double *hn, double *ghn, double *cv, double *An, double *Bn, double *bn, int *info);

/* ---- the small kernels either side of the solve ---------------------------------
 * Scenario fan-out of the initial state (Stochastic_NMPC/stochastic_mpc_utils.py:78-91 compute_x0dist as a
 * batch axis): batch must equal P*(S+1); instance p*(S+1) is pose p, instance p*(S+1)+s is pose p + offs[s-1].
 * pose: P x 8, offs: S x 8 (host). Writes lbx_0 = ubx_0 of every instance. */
int tum_ocp_set_x0_fanout(tum_ocp *c, const double *pose, const double *offs, int P, int S);
/* PCE moments over each scenario group (Stochastic_NMPC/SNMPC_acados_settings.py:116-133): coefficients
 * c = A v with the L x S least-squares PCE matrix A (row-major, host), mean = c_0, var = sum_{k>=1} c_k^2, for
 * every component of field "x" (8) / "u" (2) at `stage` of the current iterate. mean, var: P x m (host). */
int tum_pce_moments(tum_ocp *c, const char *field, int stage, const double *A, int L, int S, double *mean, double *var);
/* The same reduction without a host round trip: tum_pce_attach keeps A (L x S, row-major, host) on the device,
 * tum_pce_moments_device enqueues the reduction on the capsule's stream and writes P x m doubles each into caller-owned
 * DEVICE buffers (the slab of the rooted gather of BASELINE config 3). */
int tum_pce_attach(tum_ocp *c, const double *A, int L, int S);
int tum_pce_moments_device(tum_ocp *c, const char *field, int stage, double *mean_dev, double *var_dev);
/* The coupled SNMPC OCP (Stochastic_NMPC/SNMPC_acados_settings.py:19-320 with the DISCRETE stacked dynamics
 * of Stochastic_NMPC/pred_model_dynamic_disc.py:121-220): turns the capsule (created with nsub = 1) into the solver the
 * reference builds at SNMPC_acados_settings.py:318 and calls at SNMPC_class.py:198. The stacked state is the nominal
 * copy followed by `ns` sample copies (nx = 8 (ns+1)); Apce (L x ns, row-major, host) and `uph` replace the per-stage
 * parameter vector p = [A_pce.flatten(), risk_parameter, stop_flag] (SNMPC_class.py:103-104,124: stop_flag = 1 from
 * stage uph on); gamma is the chance-constraint level (kappa = sqrt((1-gamma)/gamma), SNMPC_acados_settings.py:187).
 * Afterwards set/get "x" and constraints_set "lbx"/"ubx" at stage 0 also accept 8 (ns+1) values, cold_start copies the
 * stacked x0 to every stage (SNMPC_class.py:126-127), and solve runs prologue + fused kernel + epilogue. The cost acts
 * on the nominal copy with |v| as the speed row; the gg limits are looked up at |v|. 0 <= uph <= N (the reference ran
 * uph = N; beyond 31 stages the sample columns no longer fit one wavefront: pipeline kernels only). 1 <= ns <= 32 and
 * 1 <= L <= 32 (MPC_params.yaml's n_samples / expansion_degree, SNMPC_class.py:78-94; beyond 16 of either: pipeline kernels
 * only, and ns x uph bounded by the prologue's 128 KiB of LDS -- uph <= 28 / 26 / 18 / 16 at 17 / 20 / 24 / 32 samples --
 * otherwise refused here). */
int tum_ocp_snmpc_attach(tum_ocp *c, int ns, int L, const double *Apce, int uph, double gamma);
int tum_ocp_snmpc_samples(const tum_ocp *c);   /* ns, or 0 for a nominal capsule */
/* Offsets of the sample initial conditions from the nominal one (compute_x0dist, Stochastic_NMPC/stochastic_mpc_utils.py:78-91;
 * SNMPC_class.py:259-264 recomputes x0_samples from x0 before every solve): ns x 8 (host). Once registered, an 8-value
 * lbx_0 / ubx_0 -- and the device closed loop (tum_sim_*), whose state estimator writes the nominal x0 -- fans out to the
 * sample copies on the device at every solve; a stacked 8 (ns+1) lbx_0 switches back to explicit samples. */
int tum_ocp_snmpc_set_offsets(tum_ocp *c, const double *offs);
/* R2NMPC constraint tightening after a solve (Reduced_Robustified_NMPC_class.py:286-366): propagates
 * Sigma_{k+1} = A_k Sigma_k A_k' + B W B' with the A_k of the last linearisation (needs store_qp_in) and rewrites the
 * capsule's lbx/ubx (steering angle) and uh (gg circle) of stages 1..N-1 for the NEXT solve.
 * Sigma0, BWB: 8x8 row-major (host); backoff (optional, host): batch x N x 2 (steering, gg) back-offs.
 * uph >= 1, the reference's uncertainty_propagation_horizon: the stages 1..min(uph, N)-1 get the back-offs of their own
 * Sigma_k, the stages from uph on repeat the last pair, and a uph beyond N acts as N. uph = 1 propagates nothing: both
 * back-offs are 0 and the stages 1..N-1 get the nominal delta_min / delta_max / uh_nom. uph < 1 is refused. An instance whose
 * last solve failed keeps all its bounds; its rows of `backoff` read 0. */
int tum_ocp_r2_backoff(tum_ocp *c, const double *Sigma0, const double *BWB, int uph,
                       double delta_min, double delta_max, double uh_nom, double *backoff);
/* The same tightening as part of EVERY solve (Reduced_Robustified_NMPC_class.py:276-378 runs it after each successful acados
 * call, and counts it in the reported solver time, :379-381): after the SQP-RTI kernel the back-off kernel rewrites the bounds
 * for the next solve on the capsule's stream; instances whose solve failed keep their bounds. Needs store_qp_in. This is what
 * lets the robustified controller run in the device closed loop (tum_sim_*). uph = 0 detaches. */
int tum_ocp_r2_attach(tum_ocp *c, const double *Sigma0, const double *BWB, int uph,
                      double delta_min, double delta_max, double uh_nom);
/* Snapshot / restore (asynchronous) of ALL per-stage bounds on the device: the tightening rewrites them after every solve,
 * a sweep or a benchmark that restarts from the nominal problem puts them back without a host copy. */
int tum_ocp_bounds_snapshot(tum_ocp *c);
int tum_ocp_bounds_restore(tum_ocp *c);
/* read back a bound installed with constraints_set / r2_backoff (one value per instance) */
int tum_ocp_constraints_get(tum_ocp *c, int stage, const char *field, double *v, int b0, int nb);

/* ---- the producer and the consumer of the solve, on the device --------------------------
 * PlannerEmulator(ref_traj, pose, n_points, Tp, loop_circuit)   Utils/MPC_sim_utils.py:137-194, called from
 * main.py:52-54 / get_baseline_performances.py:105: stateless batched form. track: n_track x 4 row-major
 * [pos_x,pos_y,ref_yaw,ref_v]; pose: P x 2; ref_out: P x n_points x 4; closest_out (optional): P. All host pointers. */
int tum_planner_emulate(const double *track, int n_track, const double *pose, int P, int n_points, double Tp,
                        int loop_circuit, double *ref_out, int *closest_out, int device);
/* The same on a TRACK SET: tracks holds the tables of n_tracks race lines one behind the other ([sum n_t][4]), track_rows the
 * n_tracks + 1 ascending row offsets (0 first, every track at least 2 rows), track_of[p] in 0..n_tracks-1 the track of pose p (any
 * order). closest_out and every index behind it are local to the pose's own track; the arithmetic is the single-track call's. */
int tum_planner_emulate_tracks(const double *tracks, const int *track_rows, int n_tracks, const int *track_of, const double *pose,
                               int P, int n_points, double Tp, int loop_circuit, double *ref_out, int *closest_out, int device);

/* A batch of closed loops kept in HBM: planner -> solve -> plant step + state estimation
 * (main.py:48-78; Utils/SimulationMode_main_class.py:106-156 sim_step simMode 0 / StateEstimation;
 * Vehicle_Simulator/sim_model_dynamic_stm_pacejka.py:137-195 + VehicleSimulator.py:73-77: RK4 with n_elem elements over Ts).
 * windows: the 8 moving-average lengths (1..4). log_capacity: control steps of logs kept on the device (0 = none). */
typedef struct tum_sim tum_sim;
tum_sim *tum_sim_create(tum_ocp *c, const double *track, int n_track, double Tp, int loop_circuit, double Ts, int n_elem,
                        const int *windows, int log_capacity);
/* The same loop on a track set (tum_planner_emulate_tracks: tracks, track_rows, n_tracks), track_of[b] the track of instance b, batch
 * ints in any order (need not be sorted or contiguous). Every index of an instance -- "closest", a segment's end, a start index of the
 * environment, the full_lap waypoint n - 2 -- is local to that instance's own track, and the host checks hold it against that track:
 * an index that exists on a longer track of the set but not on the instance's own is refused before anything is launched. Instance b
 * computes what it computes in a single-track loop of the same batch on track_of[b], bit for bit. The set is fixed for the life of
 * the loop (a captured chunk holds its pointers by value). */
tum_sim *tum_sim_create_tracks(tum_ocp *c, const double *tracks, const int *track_rows, int n_tracks, const int *track_of, double Tp,
                               int loop_circuit, double Ts, int n_elem, const int *windows, int log_capacity);
void tum_sim_free(tum_sim *s);
/* x_sim: batch x 7 plant states, x_mpc: batch x 8 controller states (host); resets the estimator and the step counter */
int tum_sim_set_state(tum_sim *s, const double *x_sim, const double *x_mpc, int cold_start);
/* Disturbance realisation played back by the loop (Utils/SimulationMode_main_class.py:121-143: simulate_disturbances /
 * simulate_state_estimation, as with disturbance_playback; the draws of Utils/MPC_sim_utils.py:54-86 are made on the host): w_deriv is
 * added to the state derivatives of the plant for the whole control step (Vehicle_Simulator/sim_model_dynamic_stm_pacejka.py:196) in a
 * SECOND plant step from the same state -- the true state stays the undisturbed step, as in the reference --, e_est is added to that
 * disturbed state before the estimator. n_steps x batch x 7 doubles each (host, step-major), either may be null; control steps beyond
 * n_steps run undisturbed; n_steps = 0 removes the realisation. tum_sim_set_state restarts the playback. */
int tum_sim_set_disturbances(tum_sim *s, const double *w_deriv, const double *e_est, int n_steps);
/* ---- Disturbance draws: the same realisation DRAWN on the device, one launch per control step in front of the plant, instead of
 * played back from a table. The distributions are the reference's (Utils/MPC_sim_utils.py:54-86); the random stream is this
 * project's own. A draw depends on (seed, instance b, global control step t, stream s, kind, bounds) alone -- not on the batch, the
 * window, the launch shape or the path that asks for it -- so every realisation can be regenerated after the fact without being stored.
 *
 * Key and counter. Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32). Block j of stream s (s = 0: derivative disturbance,
 * s = 1: state estimation error) for instance b at step t has the counter (b, t & 0xffffffff, t >> 32, 0x100 * (1 + s) + j). The last
 * word is never 0: these draws never meet the policy's (last word 0) under the same seed.
 * Uniforms from a block. Its four words x0..x3 give uA = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 and uB likewise from (x2, x3): both in
 * [0, 1), integer work plus an exact conversion.
 * Normals. Block j = 0..3 gives z[2j] = R cos(theta) and z[2j+1] = R sin(theta) with R = sqrt(-2 ln(1 - uA)), theta = 2 pi uB;
 * 1 - uA is exact and lies in (0, 1], so the logarithm never sees 0. Channel i = 0..6 uses z[i]; z[7] is unused.
 * Kinds, with the bounds w[i] >= 0 (the seven magnitudes of the stream):
 *   1 'uniform'   the reference's ellipsoid with shape matrix diag(w): sqrt(w[i]) * r * z[i] / |z|, |z| the 2-norm of z[0..6] summed
 *                 in index order, r = uA(block 4) ** (1/7); a zero norm gives zeros
 *   2 'gaussian'  w[i] * z[i]
 *   3 'absolute'  w[i]
 *   4 the box     -w[i] + u_i * (2 w[i]), u_i = uA (i even) or uB (i odd) of block i >> 1
 * All kinds: fp contract(off), sums in index order. 'absolute' and the box are exact statements (device and host agree to the bit);
 * the two normal kinds go through log, sqrt, sin, cos and a power, whose last bits are the math library's.
 * Difference from the reference: it draws from numpy's legacy Mersenne-Twister stream (one rand(), then randn()s), which no counter
 * reproduces; closed_loop.DisturbanceModel.draw keeps doing that on the host for playback.
 *
 * kind_w / kind_e: 0 switches a stream off, 1..4 as above; both 0 detaches. bound_w / bound_e: 7 doubles each (may be null for a stream
 * that is off), negative or non-finite ones are refused. Attaching waits for the loop's stream, drops the captured chunk of the run
 * function (it holds the extra launch, or lacks it) and removes a played-back table; the table setter above, given a table, removes
 * the generator. The draws are indexed by the loop's GLOBAL control step, as playback is: the state function restarts them at step 0
 * with the counter, an environment reset or a per-instance restart does not touch them. */
int tum_sim_disturbances_attach(tum_sim *s, int kind_w, const double *bound_w, int kind_e, const double *bound_e, unsigned long long seed);
/* The realisation of the control steps first_step .. first_step + n_steps - 1 as the attached generator draws it (the same device
 * function as the live draw: equal to the bit), n_steps x batch x 7 doubles per stream (host, step-major). Either output may be null;
 * a stream that is off gives zeros. Read-only for the loop: step counter, slab and captured chunk are untouched. */
int tum_sim_disturbances_table(tum_sim *s, long long first_step, int n_steps, double *w_out, double *e_out);
int tum_sim_plan(tum_sim *s);        /* yref of every instance from its pose (async on the capsule's stream) */
/* plant step with (x1[7], u0[1]) of the iterate, estimator -> next x0 (async). An instance whose solve FAILED (status != 0)
 * is then treated as main.py:59-61 treats it (MPC.reintialize_solver(x_next)): its iterate is cold-started at the state the
 * failed solve started from (sample copies included), an R2 capsule gets its nominal bounds back. */
int tum_sim_advance(tum_sim *s);
/* nsteps x (plan, solve, advance), then synchronises; chunks of 25 steps are captured once into a hipGraph and replayed
 * (tum_sim_get "graph_steps" tells whether the capture succeeded) */
int tum_sim_run(tum_sim *s, int nsteps);
int tum_sim_steps(const tum_sim *s);
/* field: "x_sim" (B*7), "x_mpc" (B*8), "pose" (B*2), "ref0" (B*4), "closest" (B), "graph_steps" (1), "track_of" (B: all 0 on one
 * track), "track_rows" (n_tracks + 1: the row offsets; {0, n_track} on one track); logs with the npz schema of
 * Utils/Logging_Plotting.py:357-372, step-major: "CiLX" ((steps+1)*B*7), "MPC_SimX" ((steps+1)*B*8), "simU" (steps*B*2),
 * "simREF" (steps*B*4), "simSolverDebug" (steps*B*5: cost, 0, sqp_iter, qp_iter, status). len must match. */
int tum_sim_get(tum_sim *s, const char *field, double *out, long long len);

/* ---- track segments: what a weight sweep runs the loop for (Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/objective_function.py:57-200,
 * the same termination rules as RL_WMPC/environment.py:152-165,239-240) ------------------------------------------------
 * Once attached, every control step scores every instance whose segment is still active, between the solve and the plant step, from
 * what the loop holds there (Utils/Logging_Plotting.py:152-179): lat_dev and vel_dev of the plant state against the first reference
 * point, a_comb from the gg table of the capsule. It accumulates steps, max |lat_dev|, sum vel_dev^2, max a_comb and the failed solves,
 * then sets the bits of the segment's state word, which are never cleared: 1 done (planner index == end_idx[b], an equality;
 * end_idx[b] < 0: never), 2 crash by lat_dev > max_lat_dev (signed), 4 crash by a_comb > max_a_comb. The step that sets a bit is
 * counted; an instance with a non-zero state is not scored any further but keeps driving. An infinite threshold disables its test.
 * end_idx: batch ints (host). group_offsets: n_groups + 1 ints, 0 = first < ... < last = batch (contiguous groups of instances;
 * NULL: one group per instance). end_idx == NULL detaches. Either way a captured chunk of the run function is dropped and captured again.
 * The state function (set_state) zeroes scores and state words: a new run is a new evaluation. */
int tum_sim_segments_attach(tum_sim *s, const int *end_idx, const int *group_offsets, int n_groups, double max_lat_dev, double max_a_comb);
/* the run function in chunks of check_every control steps (<= 0: 100) until no segment is active or max_steps have run. Segments still
 * active then have timed out: they are neither done nor crashed (the reference's loop has no cap, a batched one needs it).
 * More fields of the get function, B values each unless noted, an error when nothing is attached: "seg_steps", "seg_state",
 * "seg_max_lat_dev", "seg_rms_vel_dev" (sqrt(sum vel_dev^2 / steps)), "seg_max_a_comb", "seg_qp_failures", "seg_active" (1 value),
 * "seg_groups" (n_groups x 4: mean of -max|lat_dev|, mean of -rms(vel_dev), segments, segments not cleanly done -- crashed or
 * still active; one reduction kernel per read, fixed summation order). */
int tum_sim_run_segments(tum_sim *s, int max_steps, int check_every);

/* ---- the weight-scheduling RL environment (Learning_To_Adapt/SafeRL_WMPC/RL_WMPC/environment.py:112-240, reward.py:15-33,
 * observation.py:28-75) around the loop: every n_mpc_steps control steps an agent picks, per instance, one row
 * [q_xy, q_yaw, q_vel, r_jerk, r_steer, L1, L2] of `table` (n_actions x 7, host; NMPC_class.py:269-317 update_cost_function_weights:
 * the words written are those of the cost setter -- diag W at the stages 0..N-1, its first four entries at stage N, zl = zu = L1 and
 * Zl = Zu = L2 of every slack). Once attached, every control step scores every instance whose environment step has not ended, between
 * the solve and the plant step (Utils/Logging_Plotting.py:152-159: lat_dev signed, vel_dev), then latches truncated = lat_dev >
 * max_lat_dev (environment.py:153-158,239-240) and terminated = full_lap ? planner index == n_track - 2 (an equality) :
 * episode_steps == episode_length (environment.py:160-165). The step that sets a flag is counted, nothing after it is; the instance
 * keeps driving unscored. episode_steps counts ENVIRONMENT steps (environment.py:115), so the last environment step of an episode ends
 * after its first control step.
 * sigmas: 2, lims: 4 = lims[0][lat, vel], lims[1][lat, vel] (reward.py: exp(-sum(clip((rms - lims[0]) / (lims[1] - lims[0]), 0, 1)^2 /
 * (2 sigmas)))). Observation of 2 + 2 n_samples entries: [lat_dev, vel_dev], ref_v at idx_v, the 10-tap average of
 * diff(unwrap(ref_yaw)) / Ts at idx_yawrate (np.linspace(0, len - 1, n_samples, dtype=int) of observation.py:58-59, computed by the
 * caller; Ts is the loop's although the points are Tp / N apart), normalised with obs_lo / obs_hi (observation.py:16-24). obs_states 0:
 * the first two entries are 0 before normalisation, as in the reference (Logging_Plotting.py:307-312 reads the row BEHIND the last one
 * written); 1: those of the last scored control step. Needs 10 <= N <= 127.
 * Refused: SNMPC, R2 and full-W capsules, SQP mode, rti_phase 1 / 2, the development kernel 'fused', a loop with segments attached (and
 * segments on a loop with an environment). table == NULL detaches. Either way a captured chunk of the run function is dropped. While
 * attached the state estimator counts its samples per instance (a reset empties one instance's buffers); disturbance playback and the
 * logs stay indexed by the loop's global step. The state function (set_state) zeroes the environment's counters. */
int tum_sim_env_attach(tum_sim *s, const double *table, int n_actions, int n_mpc_steps, double max_lat_dev, int episode_length, int full_lap,
                       const double *sigmas, const double *lims, const double *obs_lo, const double *obs_hi,
                       const int *idx_v, const int *idx_yawrate, int n_samples, int obs_states);
/* environment.py:191-237 for the instances with mask[b] != 0 (mask == NULL: all): plant and controller state of waypoint start_idx[b]
 * (yaw mod 2 pi, everything else 0), empty estimator, cold iterate (X_k = x0, U = 0, cold interior point method), episode counters 0.
 * Nothing else of the batch changes. */
int tum_sim_env_reset(tum_sim *s, const int *mask, const int *start_idx);
/* environment.py:112-189 for the whole batch: one upload (actions, reset mask, start indices: batch ints each; the last two may be
 * NULL), the resets, the actions, n_mpc_steps control steps, one download. out: batch x (6 + 2 + 2 n_samples) doubles -- reward,
 * terminated, truncated, step_length, failed solves among the scored steps, planner error word, observation. An action outside the
 * table, and stepping an instance whose episode has ended without marking it for reset, are errors; nothing runs then. reset_mask[b]:
 * 0 nothing, 1 reset, 2 an instance whose episode has ended drives on as it is (scoring a loop nothing restarts: episode_steps keeps
 * counting, so `terminated`, an equality, is not set again). */
int tum_sim_env_step(tum_sim *s, const int *actions, const int *reset_mask, const int *start_idx, double *out);
/* More fields of the get function, B values each, an error when no environment is attached: "env_episode_steps", "env_step_length",
 * "env_flags" (1 terminated, 2 truncated), "env_qp_failures", "env_samples" (samples the estimator has seen), "env_ended". */

/* --- K12: the agent of the environment on the device (enable_WMPC of the reference's controller classes, RL_WMPC/evaluation.py:65-105
 * run_policy: model.predict(obs, deterministic=True) of a stable_baselines3 MlpPolicy with tanh activations). Inference; sampling and the value net are K13 below.
 * The policy net is evaluated in FP64 on the float32 weights, the observation rounded to float32 first as stable_baselines3 does:
 * h = tanh(W h + b) per hidden layer, a linear action layer, the action the first index of the largest logit, the probabilities the
 * softmax of the logits (helpers.py:100-105).
 * widths[n_layers + 1]: inputs, hidden widths..., actions (n_layers matrices: 2..5, that is 1 to 4 hidden layers; 1..128 inputs,
 * hidden layers 1..256 wide, 1..64 actions); W[l] row-major (out, in) as torch stores it; W == NULL detaches.
 * On a loop with an attached environment the observation must have widths[0] entries and the table widths[n_layers] rows. On a
 * loop without one the policy serves tum_sim_policy_eval alone (a rollout is refused). Attaching, re-attaching or detaching the
 * environment detaches the policy. */
int tum_sim_policy_attach(tum_sim *s, int n_layers, const int *widths, const float *const *W, const float *const *b);
/* the policy alone on n host observations (n >= 1, independent of the loop's batch; n x widths[0] doubles): logits and probs
 * n x actions doubles, actions n ints; any of the outputs may be NULL */
int tum_sim_policy_eval(tum_sim *s, const double *obs, int n, double *logits, double *probs, int *actions);
/* n_env_steps environment steps with the policy choosing every action, enqueued without a host wait in between:
 * first_obs (B x n_obs, NULL = zeros, what a reset returns) is what the policy sees first.
 * on_end 0: an ended instance is frozen out: it drives on as with reset mask 2 of tum_sim_env_step, live = 0 from the next step on,
 *           and its later rows are not results. An instance whose episode had ended before the call starts with live = 0.
 * on_end 1: it is reset at the start of step e + 1 to start_table[e + 1][b] and the policy sees zeros for it; an instance whose
 *           episode had ended before the call is reset to start_table[0][b] at step 0. start_table: n_env_steps x B ints, every one
 *           checked against the track before anything is launched.
 * check_every > 0: the counter of live instances is read back every check_every steps and the rollout stops when it is 0.
 * out: n_env_steps x B records as tum_sim_env_step writes them; actions_out, live_out: n_env_steps x B ints; steps_run: how many
 * steps ran (the rows behind them are not written). Everything tum_sim_env_step refuses is refused, and a rollout without a policy.
 * "env_ended" afterwards: the flags of the last step that ran. tum_sim_env_step works unchanged after a rollout. */
int tum_sim_env_rollout(tum_sim *s, int n_env_steps, const double *first_obs, int on_end, const int *start_table,
                        int check_every, double *out, int *actions_out, int *live_out, int *steps_run);

/* --- K19: the learned weight schedule INSIDE the loop: enable_WMPC of the reference's controller classes (NMPC_class.py:120-160,208-239,
 * SNMPC_class.py:224-255, Reduced_Robustified_NMPC_class.py:206-245,373-404) with the attached policy as the agent. One more kernel
 * per control step between the solve and the plant step (wmpc_schedule_kernel), inside captured chunks too. Per instance, with a
 * counter c that is 0 at attach time: after the solve of a control step, if c >= period then c = 0, DECIDE and INSTALL; then, in every
 * case, c += 1. period 20: decisions after the solves of the steps 20, 40, 60 counted from attach time; 1: from step 1 on; 0: every
 * step; negative: refused. Until the first decision the loop keeps the weights it has.
 * DECIDE: the observation of tum_sim_env_attach (2 + 2 n_samples entries, idx_v / idx_yawrate / obs_lo / obs_hi as there) with
 * lat_dev the lateral deviation of the state the solve STARTED at (x0) from the first point of this step's reference and
 * vel_dev = x0[3] - ref_v[0], rounded to float32, through the policy net; the first index of the largest logit.
 * INSTALL: row `action` of table (n_actions x 7), the words tum_sim_env_step writes.
 * on_failure 1 ("base"): an instance whose solve failed (status != 0) gets back, behind the decision logic of that step, the W and the
 * slack penalties it held when the schedule was attached -- the reference builds a fresh solver from the YAML weights then
 * (main.py:59-61), so a row decided at that very step is lost; the counter is not touched. 0 ("keep"): the weights stay.
 * The first log_capacity decisions of every instance are stored (step, action, observation before the rounding); later ones are counted.
 * Needs an attached policy whose input width is 2 + 2 n_samples and whose action count is n_actions, and 10 <= N <= 127. Runs on
 * nominal, coupled SNMPC and R2 capsules, beside segments and drawn disturbances. Refused, each with its own message: a loop that is
 * an RL environment (and an environment on a loop with a schedule), a full-W capsule, SQP mode, rti_phase 1 / 2, the development
 * kernel 'fused', bad indices or bounds. table == NULL detaches: the weights stay as last installed. Attaching again takes a new
 * snapshot and starts counters and log afresh; detaching the policy detaches the schedule; the state function (set_state) zeroes
 * counters and log. Either way a captured chunk of the run function is dropped. Only the run function launches the kernel: a loop
 * driven by tum_sim_plan / solve / tum_sim_advance is not scheduled. */
int tum_sim_wmpc_attach(tum_sim *s, const double *table, int n_actions, int period, int on_failure, int n_samples,
                        const int *idx_v, const int *idx_yawrate, const double *obs_lo, const double *obs_hi, int log_capacity);
/* "counter" (B: c as the next control step tests it), "n_decisions" (B), "steps" and "actions" (B x log_capacity, -1 where none),
 * "observations" (B x log_capacity x (2 + 2 n_samples)), the snapshot "base_W" (B x (N + 1) x 6: the diagonal of W per stage) and
 * "base_pen" (B x 36), and the same arrays as the capsule holds them now: "W", "pen". */
int tum_sim_wmpc_get(tum_sim *s, const char *field, double *out, long long len);

/* --- K13: collecting PPO training rollouts on the device (stable_baselines3 collect_rollouts + compute_returns_and_advantage as
 * rl_training.py's model.learn drives them). The PPO update is not here.
 * The value net of the agent beside the attached policy (mlp_extractor.value_net.<i>, value_net): widths[n_layers + 1] = inputs,
 * hidden widths..., 1, with widths[0] the attached policy's inputs; 1 to 4 hidden layers up to 256 wide, its own depth and widths.
 * W == NULL detaches. Refused without a policy; detaching or re-attaching the policy or the environment detaches it. */
int tum_sim_policy_attach_value(tum_sim *s, int n_layers, const int *widths, const float *const *W, const float *const *b);
/* The two nets and ONE draw per observation on n host observations (n x widths[0] doubles). The draw of observation i is the uniform
 * u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (first_instance + i, t & 0xffffffff, t >> 32, 0); with e_j = exp(z_j - max z) and prefix sums c_j in index order, S = c_{A-1}, the
 * action is the smallest j with u S < c_j (A - 1 if none) and log_probs = (z_a - max z) - log S. This is the project's own sampling
 * rule: the distribution of stable_baselines3, not the draws of torch.multinomial. Any output may be NULL; values needs the value net. */
int tum_sim_policy_eval_ac(tum_sim *s, const double *obs, int n, unsigned long long seed, unsigned long long t, unsigned first_instance,
                           int *actions, double *values, double *log_probs, double *uniforms);
/* Generalised advantage estimation alone on host arrays (rewards, values, episode_starts: E x B; last_values, last_dones: B), FP64:
 *   nnt = 1 - (t == E-1 ? last_dones : episode_starts[t+1]);  nv = t == E-1 ? last_values : values[t+1]
 *   delta = (rewards[t] + (gamma nv) nnt) - values[t];  last = delta + ((gamma lambda) nnt) last;  adv[t] = last;  ret[t] = adv[t] + values[t] */
int tum_sim_gae(tum_sim *s, int E, int B, const double *rewards, const double *values, const double *episode_starts,
                const double *last_values, const double *last_dones, double gamma, double lambda, double *adv, double *ret);
/* tum_sim_env_rollout with on_end 1, SAMPLED actions (decision counter t0 + e at step e, counter word 0 the instance's index) and the
 * record of a RolloutBuffer, GAE included; everything is enqueued, one wait and one download at the end.
 * first_obs (B x n_obs, NULL = zeros) and first_episode_starts (B, NULL = ones): what the policy sees first and whether that begins an
 * episode. start_table: n_env_steps x B, as for the rollout.
 * rewards = rewards_raw + gamma V(the step's own observation) where truncated && !terminated (stable_baselines3's TimeLimit.truncated;
 * in the reference's naming that is the crash, not the episode length).
 * out: TUM_COLLECT_FIELDS fields of n_env_steps x B doubles each, in the order of the enum below, then the observations the policy
 * saw (n_env_steps x B x n_obs), then last_values (B) -- the value of what the policy would see next, zeros for an instance that just
 * ended -- last_dones (B) and what the policy would see next (B x n_obs: the first_obs of a following call). Refuses what the rollout
 * refuses, and a missing value net. */
enum { TUM_COLLECT_ACTION, TUM_COLLECT_VALUE, TUM_COLLECT_LOG_PROB, TUM_COLLECT_REWARD, TUM_COLLECT_REWARD_RAW, TUM_COLLECT_EPISODE_START,
       TUM_COLLECT_ADVANTAGE, TUM_COLLECT_RETURN, TUM_COLLECT_TERMINATED, TUM_COLLECT_TRUNCATED, TUM_COLLECT_STEP_LENGTH,
       TUM_COLLECT_QP_FAILURES, TUM_COLLECT_PLANNER_ERROR, TUM_COLLECT_FIELDS };
int tum_sim_env_collect(tum_sim *s, int n_env_steps, const double *first_obs, const double *first_episode_starts, const int *start_table,
                        unsigned long long seed, unsigned long long t0, double gamma, double gae_lambda, double *out);

/* --- K14: the PPO update on the device (stable_baselines3 PPO.train as rl_training.py:133-155 configures it: normalize_advantage,
 * clip_range_vf None, target_kl None, separate tanh nets). One minibatch of n rows (obs, a, old_log_prob, adv, ret):
 *   A = (adv - mean adv) / (std adv + 1e-8), std with the n - 1 divisor (A = adv for n == 1 or normalize_advantage == 0)
 *   z the policy net's logits on float32(obs); logp = (z - max z) - log sum exp(z - max z) (index order); p = exp(logp)
 *   H = -sum p logp; lp = logp[a]; r = exp(lp - old_log_prob)
 *   policy_loss = -mean min(A r, A clip(r, 1 - c, 1 + c)) (the unclipped term carries the gradient where A r <= A clip(r))
 *   value_loss = mean (ret - V(obs))^2; entropy_loss = -mean H; loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 *   approx_kl = mean((r - 1) - log r); clip_fraction = mean(|r - 1| > c); grad_norm = sqrt(sum g^2) over every weight and bias
 *   g <- min(1, max_grad_norm / (grad_norm + 1e-6)) g
 *   Adam (beta 0.9 / 0.999, eps 1e-5, no weight decay), t the step counter:  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;
 *   theta <- theta - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * Precision: the parameters are float32 values (what policy_kernel / policy_ac_kernel act with); everything else -- forward, backward,
 * reductions, moments -- is FP64; the new parameter is the FP64 result of the Adam line rounded ONCE to float32 (nearest even) and is
 * written in place into the packed nets: the nets that act are the updated nets, without an upload. No floating-point atomics; the
 * order of every sum depends on the minibatch size and the widths alone: the same call from the same state gives the same bits.
 * tum_sim_ppo_attach needs an attached policy WITH a value net; it zeroes the moments and the step counter. Detaching or re-attaching
 * the policy, the value net or the environment detaches the trainer; tum_sim_ppo_detach does so alone. */
enum { TUM_PPO_LOSS, TUM_PPO_POLICY_LOSS, TUM_PPO_VALUE_LOSS, TUM_PPO_ENTROPY_LOSS, TUM_PPO_APPROX_KL, TUM_PPO_CLIP_FRACTION,
       TUM_PPO_GRAD_NORM, TUM_PPO_N, TUM_PPO_STATS };
int tum_sim_ppo_attach(tum_sim *s, double clip_range, double ent_coef, double vf_coef, double max_grad_norm, int normalize_advantage);
int tum_sim_ppo_detach(tum_sim *s);
/* One minibatch of n host rows (obs n x widths[0]; actions n ints inside the policy's range). apply 0: loss, gradients and grad_norm
 * only -- parameters, moments and the step counter stay untouched. stats_out: TUM_PPO_STATS doubles (TUM_PPO_N: the rows).
 * grads_out (NULL or n_params doubles): the UNCLIPPED gradients over the flat parameter vector in torch's layout -- per net W_0 (out x
 * in, row-major), b_0, W_1, b_1, ...; the policy net, then the value net. rows_out (NULL or n x 2): the log-probability of each row's
 * action and its value as the update computed them: the bits of tum_sim_policy_eval_ac on the same rows. */
int tum_sim_ppo_step(tum_sim *s, int n, const double *obs, const int *actions, const double *old_log_probs, const double *advantages,
                     const double *returns, double lr, int apply, double *stats_out, double *grads_out, double *rows_out);
/* One update: n_epochs passes over the N buffer rows; pass e visits them in the order perm[e][0 .. N) (n_epochs x N ints in [0, N),
 * the caller's), cut into minibatches [k batch_size, min((k + 1) batch_size, N)) -- the last may be short. Every minibatch is the
 * chain of tum_sim_ppo_step with apply 1; all of them are enqueued, one wait, one download. stats_out: n_epochs x ceil(N /
 * min(batch_size, N)) x TUM_PPO_STATS. obs, actions, old_log_probs, advantages, returns all NULL: the rows tum_sim_env_collect last left
 * on the device (row e B + b); refused when there are none or their number is not N. */
int tum_sim_ppo_update(tum_sim *s, int N, const double *obs, const int *actions, const double *old_log_probs, const double *advantages,
                       const double *returns, const int *perm, int n_epochs, int batch_size, double lr, double *stats_out);
/* The float32 parameters the device acts with, per matrix as the attach functions take them (policy W / b, value net VW / Vb). */
int tum_sim_ppo_params(tum_sim *s, float *const *W, float *const *b, float *const *VW, float *const *Vb);
/* Adam's state: the moments over the flat parameter vector (n_params doubles each), the step counter, n_params. Any may be NULL. */
int tum_sim_ppo_state(tum_sim *s, double *m, double *v, long long *t, int *n_params);

/* --- K15: candidate selection of the Bayesian-optimisation step (Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/acquisition.py): the
 * feasibility-weighted expected hypervolume improvement of C candidates x in [0,1]^d, two objectives, both maximised.
 * Four exact GPs g (objective 0, 1 on the n_t feasible trials Xt; class 0, 1 of the Dirichlet classification GP on all n_c trials Xc),
 * each with k_g(x,x') = s_g exp(-1/2 sum_j ((x_j - x'_j) ils_gj)^2), constant mean c_g, a_g = A_g^-1 (y_g - c_g) and V_g = L_A^-1
 * (A_g = K_g + noise = L_A L_A^T; n x n row-major, the lower triangle is read). Per objective o the baseline Xb (n_b points) with
 * H_o = K_o(Xb,Xt) V_o^T (n_b x n_t), R_o = chol(K_o(Xb,Xb) - H_o H_o^T + jitter_o I)^-1 (lower), the base samples Z_o (S x n_b) and
 * zeta_o (S), and per sample s the front of the baseline draw: front_count[s] points of fronts[s] (P_max x 2, ascending in objective
 * 0), non-dominated and strictly better than ref. For a candidate x and each o:
 *   k_t = k_o(Xt, x); q = V_o k_t; mu = c_o + k_t . a_o; sig = k_o(Xb, x) - H_o q; l = R_o sig
 *   d2 = max(s_o - q.q - l.l, jitter_o); f_s,o = mu + Z_o[s] . l + sqrt(d2) zeta_o[s]
 *   HVI_s = sum_{i=0..P} max(0, min(f_s,0, x_{i+1}) - x_i) max(0, f_s,1 - h_i), x_0 = ref_0, x_i = p_i,0, x_{P+1} = +inf, h_i = p_{i+1},1, h_P = ref_1
 * and for the classes m_k = c_k + k_c . a_k, v_k = s_k - |V_k k_c|^2, t ~ N(m_1 - m_0, max(v_0 + v_1, 0)):
 *   p = E sigmoid(t), sd = sqrt(E (sigmoid(t) - p)^2), both by the K-node rule (gh_x, gh_w) for a standard normal: E g = sum w g(m + sd_t x)
 *   factor = eps p + (1 - eps) sd;  alpha(x) = factor (1 / S) sum_s HVI_s
 * All pointers are host pointers; the matrices stay on the device across evaluations. keep_gp != 0: the four GPs of the last
 * tum_bo_model stay (d, n_t, n_c must match; Xt, Xc, ils, a, V, s, c are not read) and only the baseline, the samples, the fronts and
 * the scalars are replaced -- what appending a pick changes. Limits: d 1..16, n_t and n_c 1..4096, n_b 1..512, S 1..4096,
 * P_max 1..n_b, K 1..64, any C >= 1 (candidates are processed 512 at a time). No floating-point atomics: the order of every sum
 * depends on the model's sizes alone, the same call gives the same bits, and a candidate's value does not depend on the others. */
typedef struct tum_bo tum_bo;
typedef struct tum_bo_model_desc {
    int d, n_t, n_b, n_c, S, P_max, K, keep_gp;
    double eps, ref[2], jitter[2];
    double s[4], c[4];                  /* objective 0, 1, class 0, 1 */
    const double *Xt, *Xb, *Xc;         /* n_t x d, n_b x d, n_c x d */
    const double *ils[4];               /* d inverse length scales each */
    const double *a[4];                 /* n_t, n_t, n_c, n_c */
    const double *V[4];                 /* n x n */
    const double *H[2], *R[2];          /* n_b x n_t, n_b x n_b */
    const double *Z[2], *zeta[2];       /* S x n_b, S */
    const double *fronts;               /* S x P_max x 2 */
    const int *front_count;             /* S */
    const double *gh_x, *gh_w;          /* K */
} tum_bo_model_desc;
enum { TUM_BO_MU0, TUM_BO_MU1, TUM_BO_D20, TUM_BO_D21, TUM_BO_HVI, TUM_BO_P, TUM_BO_SD, TUM_BO_FACTOR, TUM_BO_DETAIL };
tum_bo *tum_bo_create(int device);
void tum_bo_free(tum_bo *b);
int tum_bo_model(tum_bo *b, const tum_bo_model_desc *m);
/* X: C x d; alpha_out: C; detail_out: NULL or C x TUM_BO_DETAIL. Refused: no model, C < 1, a NaN or an infinity in X. */
int tum_bo_evaluate(tum_bo *b, const double *X, int C, double *alpha_out, double *detail_out);
/* Measurement aid: on != 0 times the seven launches of the following evaluations with events; ms_out (NULL or 7 doubles): the
 * milliseconds of the last evaluation -- kernel values, V products, moments, H product, R product, samples and HVI, final. */
int tum_bo_profile(tum_bo *b, int on, double *ms_out);

/* --- K17: parts of the acquisition model built on the device (bo.prune_baseline, the baseline part of bo.pack_model, bo.append_pick,
 * bo.build_fronts). All work on a tum_bo handle. tum_bom_prune and tum_bom_fronts need no model and leave the handle's model alone;
 * tum_bom_build installs a model (it replaces the one there), tum_bom_append extends it, tum_bom_model_read downloads it.
 * tum_bom_prune: which of the n feasible trials are non-dominated in at least one of S joint posterior samples at the trials
 * themselves. Per objective o, from the fitted GP (Xt, ils_o, s_o, c_o, V_o = L_A^-1 lower, a_o) and base samples Z_o (S x n):
 *   K = k_o(Xt, Xt); H = K V_o^T; Sig = K - H H^T (symmetrised) + max(jitter, 1e-6 s_o) I = L_p L_p^T; m = c_o + K a_o
 *   F[s][i][o] = m_i + sum_k Z_o[s][k] L_p[i][k]
 * then keep_out[i] = 1 where in some sample s no j has F[s][j] >= F[s][i] in both objectives and > in one (equal rows keep each
 * other), 0 otherwise. With desc->F (S x n x 2) set, the GP inputs are not read and only this step runs on the given draws.
 * ok_out: 1 where both factorisations met positive finite pivots only (always 1 with given draws); otherwise 0, and keep_out and
 * F_out hold the result of the chain with each failed pivot replaced by 1 -- a result, not an error. The Cholesky is gp_kernels'
 * blocked chain; products run on the matrix cores and skip the zero tiles of V and L_p. No floating-point atomics: the order of
 * every sum depends on n, d and S alone. struct_size: sizeof(tum_bom_prune_desc) as the caller compiled it (tum_bom_prune_desc_init
 * sets it and zeroes the rest). Limits: n 1..4096, S 1..4096, d 1..16. Refused: a null argument, a struct_size that is not this
 * library's, sizes out of range, a NaN or an infinity in any input, a V with a nonzero above its diagonal (the products stop at the
 * diagonal tile; tum_bom_build refuses the same of the two objective V). */
typedef struct tum_bom_prune_desc {
    int struct_size;
    int n, d, S;
    double jitter;
    const double *F;                    /* NULL, or S x n x 2 given draws */
    const double *Xt;                   /* n x d */
    double s[2], c[2];
    const double *ils[2];               /* d */
    const double *V[2], *a[2];          /* n x n, zero above the diagonal (as tum_gp_factor returns it); n */
    const double *Z[2];                 /* S x n */
} tum_bom_prune_desc;
void tum_bom_prune_desc_init(tum_bom_prune_desc *desc);
/* keep_out: n ints; F_out: NULL or S x n x 2, the draws the mask was formed from. */
int tum_bom_prune(tum_bo *b, const tum_bom_prune_desc *desc, int *keep_out, double *F_out, int *ok_out);
/* The fronts of given baseline draws F_b (S x n_b x 2): per sample the points strictly above ref in both objectives, sorted by
 * objective 0 descending, then objective 1 descending, kept where objective 1 exceeds the running maximum, stored ascending in
 * objective 0 into fronts_out (S x n_b x 2, zero rows behind the count) with count_out (S) -- what tum_bo_model takes as fronts
 * (P_max = n_b) and front_count. Limits: S 1..4096, n_b 1..512. Refused: a null argument, sizes out of range, a NaN or an infinity. */
int tum_bom_fronts(tum_bo *b, const double *F_b, int S, int n_b, const double *ref, double *fronts_out, int *count_out);
/* tum_bom_build: tum_bo_model with the baseline part built on the device. The four GPs are installed as tum_bo_model installs them;
 * then per objective o, with Z_o = Zfull_o[:, 0 .. n_b) and zeta_o = Zfull_o[:, n_b] (Zfull_o: S x ncol, ncol >= n_b + 1):
 *   H_o = K_o(Xb,Xt) V_o^T; L_b = chol(sym(K_o(Xb,Xb) - H_o H_o^T) + jitter_o I); R_o = L_b^-1; mu_b = c_o + K_o(Xb,Xt) a_o
 *   F_b[s][i][o] = mu_b,i + sum_k Z_o[s][k] L_b[i][k]
 * and per sample the front of F_b[s] above ref as tum_bom_fronts states it (P_max = n_b). It takes no H, R, fronts or counts. ok_out: 1
 * where both factorisations met positive finite pivots only; otherwise 0 and the handle holds NO model. Limits and refusals as
 * tum_bo_model's, and a struct_size that is not this library's. tum_bom_model_read downloads what the build left on the device: per
 * objective H (n_b x n_t), R and L_b (n_b x n_b, zero above the diagonal), mu_b (n_b); F_b and fronts (S x n_b x 2), counts (S),
 * n_b. Any pointer (or entry of a pointer pair) may be NULL. Refused where the resident model was not built by tum_bom_build. */
typedef struct tum_bom_build_desc {
    int struct_size;
    int d, n_t, n_b, n_c, S, ncol, K;
    double eps, ref[2], jitter[2];
    double s[4], c[4];                  /* objective 0, 1, class 0, 1 */
    const double *Xt, *Xb, *Xc;         /* n_t x d, n_b x d, n_c x d */
    const double *ils[4];               /* d inverse length scales each */
    const double *a[4];                 /* n_t, n_t, n_c, n_c */
    const double *V[4];                 /* n x n, zero above the diagonal */
    const double *Zfull[2];             /* S x ncol */
    const double *gh_x, *gh_w;          /* K */
} tum_bom_build_desc;
void tum_bom_build_desc_init(tum_bom_build_desc *desc);
int tum_bom_build(tum_bo *b, const tum_bom_build_desc *desc, int *ok_out);
int tum_bom_model_read(tum_bo *b, double *const *H_out, double *const *R_out, double *const *L_out, double *const *mu_out,
                       double *F_b_out, double *fronts_out, int *count_out, int *n_b_out);
/* tum_bom_append: the point x (d doubles) joins the baseline of the model tum_bom_build left, without refactoring, as bo.append_pick
 * states it: with mu, q, l, d2 of x from the evaluation chain and lam = sqrt(d2), q is the new row of H_o, (l, lam) of L_b,
 * (-(l R_o) / lam, 1 / lam) of R_o, the new baseline draw is mu + Z_o l + lam zeta_o, the next column of Zfull_o becomes zeta_o and the
 * fronts are rebuilt -- all on the device; nothing is uploaded but x. tum_bom_build keeps room for one append per column of Zfull behind
 * zeta's, up to n_b = 512. ok_out: 0 where a lam is not positive and finite (jitter 0 on a baseline point). Refused: a null argument, a
 * model not built by tum_bom_build, no free column of Zfull (n_b + 2 > ncol), n_b = 512 already, a NaN or an infinity in x. */
int tum_bom_append(tum_bo *b, const double *x, int *ok_out);
/* Measurement aid: on != 0 times the kernels of the following tum_bom_build calls with events; ms_out (NULL or 9 doubles): the
 * milliseconds of the last call, both objectives together -- kernel matrices, H, covariance, Cholesky, R = L_b^-1, mean, draws, packing
 * of H and R, fronts. */
int tum_bom_build_profile(tum_bo *b, int on, double *ms_out);
/* Measurement aid: on != 0 times the kernels of the following tum_bom_prune calls with events; ms_out (NULL or 7 doubles): the
 * milliseconds of the last call, both objectives together -- kernel matrix, H, covariance, Cholesky, mean, draws, dominance. */
int tum_bom_prune_profile(tum_bo *b, int on, double *ms_out);

/* --- K16: fitting the surrogates of the Bayesian-optimisation step: the exact marginal log-likelihood of one GP and its gradient.
 * Data X (n x d), y (n) and a fixed noise per point (NULL: none); hyperparameters theta = [log ls (d), log s, c, log noise]:
 *   A = s exp(-1/2 sum_j ((x_ij - x_kj) / ls_j)^2) + diag(fixed + noise_floor + [learn_noise] e^theta_noise) = L L^T
 *   MLL = -1/2 r^T A^-1 r - sum_i log L_ii - 1/2 n log 2 pi,  r = y - c
 * and, with alpha = A^-1 r and W = alpha alpha^T - A^-1, the gradient in the order of theta:
 *   d / d log ls_j = 1/2 sum_ik W_ik K_ik ((x_ij - x_kj) / ls_j)^2     (K: the kernel alone, without the noise)
 *   d / d log s    = 1/2 sum_ik W_ik K_ik
 *   d / d c        = sum_i alpha_i
 *   d / d log noise = 1/2 e^theta_noise tr W                            (0 where learn_noise is 0)
 * ok: 1 where the factorisation met positive finite pivots only, the MLL is finite and min L_ii > 1e-7 sqrt(s); a matrix that is not
 * positive definite is a result, not an error: a failed pivot is replaced by 1, the chain finishes and ok is 0.
 * The factorisation is a blocked right-looking Cholesky (64 x 64 blocks, panel and trailing update on the matrix cores), V = L^-1 is
 * formed block-wise and A^-1 = V^T V. No floating-point atomics: the order of every sum depends on n and d alone; the same call
 * gives the same bits, also after a larger problem on the same handle. All pointers are host pointers. Limits: n 1..4096, d 1..16;
 * three n x n matrices (n padded to 64) live on the device, allocated at the first tum_gp_data that needs them and grown on demand.
 * Refused: a null argument, n or d out of range, a NaN or an infinity in X, y, the noise or theta, an evaluation before the data. */
typedef struct tum_gp tum_gp;
tum_gp *tum_gp_create(int device);
void tum_gp_free(tum_gp *g);
int tum_gp_data(tum_gp *g, const double *X, const double *y, const double *fixed_noise, int n, int d);
/* grad_out: NULL (the value only: A^-1 is not formed) or d + 3 doubles. */
int tum_gp_mll(tum_gp *g, const double *theta, int learn_noise, double noise_floor, double *mll_out, double *grad_out, int *ok_out);
/* What tum_bo_model takes of a fitted GP: V_out = L^-1 (n x n row-major, zero above the diagonal), a_out = A^-1 (y - c). */
int tum_gp_factor(tum_gp *g, const double *theta, int learn_noise, double noise_floor, double *V_out, double *a_out, int *ok_out);
/* Measurement aid: on != 0 times the following calls with events; ms_out (NULL or 7 doubles): the milliseconds of the last call --
 * kernel matrix, Cholesky, V = L^-1, A^-1 = V^T V, w and alpha, gradient tiles, reduction. */
int tum_gp_profile(tum_gp *g, int on, double *ms_out);

/* development aid: one solve with in-kernel phase timers; out = batch x 12 shader-cycle counters
 * [linearise, condense, ipm-residuals, M assembly, Cholesky, rhs, tri-solves, row updates, (iteration tail), expand+cost] */
int tum_ocp_profile_phases(tum_ocp *c, long long *out);

#ifdef __cplusplus
}
#endif
#endif /* TUM_NMPC_H */
