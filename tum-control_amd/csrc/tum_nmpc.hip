// tum_nmpc.hip -- host side of libtumnmpc.so: the C-ABI declared in include/tum_nmpc.h.
// Owns device memory for `batch` OCP instances and launches the SQP-RTI pipeline (lin / cond / ipm / expand kernels).
// -DTUM_DEV_KERNELS (libtumnmpc_dev.so, tests and experiments only) adds the two other implementations of the solve the
// pipeline is held against: round 1's fused kernel and the four-wavefront interior point kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tum_nmpc.h"
#include "pipe_kernels.hpp"
#ifdef TUM_DEV_KERNELS
#include "nmpc_kernel.hpp"
#include "ipm4_kernel.hpp"
#endif
#include "aux_kernels.hpp"
#include "loop_kernels.hpp"
#include "env_kernels.hpp"
#include "policy_kernels.hpp"
#include "wmpc_kernels.hpp"
#include "collect_kernels.hpp"
#include "ppo_kernels.hpp"
#include "disturbance_kernels.hpp"
#include "sqp_kernels.hpp"
#include "rti_kernels.hpp"
#include "bo_kernels.hpp"
#include "gp_kernels.hpp"
#include "bo_model_kernels.hpp"

using namespace tum;

// the integer switches of the environment (include/tum_nmpc.h lists them), read once
static int env_int(const char *name, int fallback) { const char *e = getenv(name); return e ? atoi(e) : fallback; }
struct Env {
    PlanEnv plan;          // TUM_LIN_COLS, TUM_COND_WIDE, TUM_SIM_FORK, TUM_FUSED_EXPAND: -1 the library's choice, 0 never, 1 always (pipe_plan.hpp)
    int ipm_lds;           // TUM_IPM_LDS (development aid: a larger LDS request lowers the number of OCPs that share a CU), 0: the kernel's own
    int force_tiles;       // TUM_FORCE_TILES (development aid, tiles_of)
};
static const Env &env()
{
    static const Env e = [] {
        const int lds = env_int("TUM_IPM_LDS", 0);
        return Env{{env_int("TUM_LIN_COLS", -1), env_int("TUM_COND_WIDE", -1), env_int("TUM_SIM_FORK", -1), env_int("TUM_FUSED_EXPAND", -1)},
                   (lds > 0 && lds <= 64 * 1024) ? lds : 0, env_int("TUM_FORCE_TILES", 0)};
    }();
    return e;
}

static thread_local std::string g_err;
static int fail(const std::string &m) { g_err = m; return 1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

struct tum_ocp {
    tum_ocp_desc d{};
    int N = 0, batch = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KArgs ka{};
    double *dx0_own = nullptr, *dyref_own = nullptr;        // the capsule's own x0 / yref arrays; dx0 / dyref below are what is IN USE (tum_ocp_bind_device: the caller's)
    double *dX = nullptr, *dU = nullptr, *dx0 = nullptr, *dyref = nullptr, *dW = nullptr, *dpen = nullptr, *dbnd = nullptr, *dcost = nullptr, *dres = nullptr,
           *dslack = nullptr, *dqpin = nullptr, *ddbg = nullptr, *dqplam = nullptr;
    double *dWf = nullptr;             // full W per stage, [b][N+1][36] (allocated by the first cost_set 'W' with an off-diagonal entry; null: diagonal W)
    int *dstatus = nullptr, *dqpiter = nullptr, *dqpstatus = nullptr, *dorder = nullptr;
    bool lpt = true, order_valid = false;
    long long *dprof = nullptr;
    double *dws = nullptr, *dhws = nullptr;
    KMode kmode = KMode::AUTO;     // auto (= the pipeline), fused, pipeline, pipeline with the four-wavefront interior point kernel (pipe_plan.hpp)
    unsigned epoch = 0;            // bumped by everything a captured launch bakes into its kernel arguments (kernel variant, schedule,
                                   // SNMPC horizon / risk parameter / work buffers, R2 attachment): tum_sim_run re-captures its graph
    bool pipe = false;             // this solve runs the four-kernel pipeline (resolved from kmode at launch)
    bool solved_pipe = false;      // the LAST solve ran the pipeline: its linearisation is in the stage records, not in qpin
    double *drec = nullptr, *dcws = nullptr, *dvec = nullptr;    // pipeline workspace: stage records, gg rows in operand layout, q | d | dv
    hipEvent_t evi0 = nullptr, evi1 = nullptr;         // around the interior point kernel of the pipeline
    bool skip_ipm_events = false, ipm_timed = false;   // a step leaves them out (tum_ocp_step_async); was the LAST solve timed with them
    float last_ms = 0;
    bool solved = false;
    std::vector<double> stage;     // host staging
    // coupled SNMPC OCP (tum_ocp_snmpc_attach)
    bool sn = false;
    SnArgs sa{};
    double *dXS = nullptr, *dxs0 = nullptr, *dApce = nullptr, *dws2 = nullptr, *dpro = nullptr, *ddv = nullptr, *doffs = nullptr;
    int *dxs_dirty = nullptr; bool xs_lazy = false;          // sample copies of the stages > uph not yet frozen (snmpc_freeze_kernel)
    bool have_offs = false, fanout = false;        // sample initial conditions derived from the nominal x0 at every solve
    int sim_fork = -1; bool lin_ahead = false;      // device closed loop: linearisation beside the planner (-1 the library's choice, 0 never, 1 where possible); state of one step
    int cond_wide = -1;                // condensing with six wavefronts per OCP: -1 the library's choice (at most one workgroup per CU), 0 never, 1 always
    int lin_cols = -1;                 // linearisation with eight lanes per (instance, stage): -1 the library's choice (small batches), 0 never, 1 always (tum_ocp_set_kernel)
    int sn_prologue = -1;              // prologue of the SNMPC OCP: -1 the library's choice, 2 the matrix-core kernel, 0 column slots and passes (tum_ocp_set_kernel)
    // R2NMPC tightening after every solve (tum_ocp_r2_attach)
    bool r2 = false; int r2_uph = 0; double r2_dmin = 0, r2_dmax = 0, r2_uh = 0; double *dr2S = nullptr, *dr2B = nullptr;
    // per-stage parameter vector of the SNMPC OCP as the caller last set it (tum_ocp_set "p")
    std::vector<double> hApce, p_gamma, p_stop; bool p_dirty = false; int uph_cap = 0; size_t pro_cap = 0; double gamma = 0.0;
    // PCE matrix of the scenario fan-out (tum_pce_attach), snapshot of the bounds (tum_ocp_bounds_snapshot)
    double *dpceA = nullptr; int pce_L = 0, pce_S = 0; double *dbnd_snap = nullptr;
    // results on the host without a stream stall (tum_ocp_results_async / _wait): device slab of the packed summary, pinned
    // host slabs, the event behind the copies
    // two sets, used in turn: the request for the NEXT batch can be enqueued before the previous batch's results have been read
    double *dsum = nullptr, *hsum[2] = {}, *hX[2] = {}, *hU[2] = {}; hipEvent_t evres[2] = {}; bool res_iter[2] = {}; int res_head = 0, res_count = 0;
    double *hin[2] = {};               // pinned staging of x0 | yref of a step (tum_ocp_step_async), one per result slot
    unsigned long long *hts[2] = {};   // device wall clock at the start / end of a step timed without events (pinned, one pair per result slot)
    int ts_slot = -1; double ts_khz = 0.0;   // slot whose clock pair times the LAST solve (-1: the events ev0 / ev1 do; 2: the synchronous slot below)
    // The reference's LITERAL call pattern on a small capsule (NMPC_class.py:169-206: N+1 x set yref, solve, 1 + N x get, get_cost,
    // 3 x get_stats -- every one a synchronous call): the per-step setters land in a pinned shadow of x0 | yref with a dirty map and go
    // up in ONE kernel in front of the next solve; a synchronous solve ends with ONE kernel that writes summary, X and U into pinned
    // slabs, and the getters that follow are served from those slabs until something changes the iterate. 83 calls of ~21 us each
    // (a stream synchronisation per call) become one solve and 82 host copies.
    double *hin_s = nullptr; unsigned long long in_mask = 0; bool in_x0 = false, in_inflight = false; hipEvent_t ev_in = nullptr;      // shadow of x0 | yref, dirty stages, upload in flight
    double *hsum_s = nullptr, *hX_s = nullptr, *hU_s = nullptr; unsigned long long *hts_s = nullptr; bool cache_valid = false;     // results of the last synchronous solve
    double *hXS_s = nullptr; bool xs_cached = false;                                           // ... and the sample copies of an SNMPC capsule, read back on first use
    bool time_ipm = false;             // keep the events around the interior point kernel also where the library leaves them out (tum_ocp_set_kernel "time-ipm")
    // full SQP solves (tum_ocp_options_set): the options, the device state of the loop (allocated by the first SQP solve), whether the
    // LAST solve was one
    // (defaults of the reference's generated solver, acados_ocp_SNMPC.json: SQP_RTI; for SQP 100 iterations, tolerances 1e-6, full steps)
    int nlp_type = 0, nlp_max_iter = 100; double nlp_tol[4] = {1e-6, 1e-6, 1e-6, 1e-6}, nlp_alpha = 1.0;
    double *dnlpres = nullptr, *dsnap = nullptr; int *dsqpstate = nullptr, *dsqpiter = nullptr, *dsnapi = nullptr;
    unsigned *dactive = nullptr, *hactive = nullptr; int active_cap = 0; hipEvent_t evpoll[2] = {};
    bool solved_sqp = false;
    // globalization of an SQP solve (tum_ocp_options_set "globalization"): 0 FIXED_STEP (nlp_alpha), 1 MERIT_BACKTRACKING -- a line search
    // per instance and iteration (sqp_merit_kernel) over the candidates merit_alpha_reduction^j >= merit_alpha_min. Device state of the
    // line search (allocated by the first such solve): accepted alpha, weight mu_in, merit table, alpha history [b][merit_hist_cap];
    // whether the LAST solve was one, and its number of candidates K and history length M (the nlp_solver_max_iter it ran with)
    int globalization = 0; double merit_alpha_min = 0.05, merit_alpha_reduction = 0.7, merit_weight_eq = 1.0;
    double *dmalpha = nullptr, *dmmu = nullptr, *dmtable = nullptr, *dmhist = nullptr; int merit_hist_cap = 0;
    bool solved_merit = false; int merit_K = 0, merit_M = 0; double merit_weight_eq_used = 1.0;
    // no solve since the last cold start / reset: the multipliers and slacks on the device are those of an EARLIER problem. An SQP-RTI
    // solve never reads them (the warm-start word is 0); a full SQP solve evaluates pass 0 with them and damps towards them, so it clears
    // them first (acados' reset() zeroes them)
    bool cold = true;
    // split real-time iteration (tum_ocp_options_set "rti_phase"): 0 preparation and feedback in one solve, 1 the next solves are
    // PREPARATIONS (linearisation and condensing), 2 FEEDBACKS (rti_feedback_kernel, interior point method, expansion).
    // prep: 0 no preparation pending, 1 the workspace holds the condensed QP of a preparation at dx0prep, 2 that preparation is
    // STALE: something it had read (iterate, reference, W, kernel variant, bound arrays) changed behind it
    int rti_phase = 0, prep = 0; double *dx0prep = nullptr; bool prep_timed = false;
    // linearisation of a STAGE-UNIFORM iterate once per instance (lin_uniform_kernel + lin_fill_kernel, pipe_kernels.hpp).
    // iter_uniform: X_k = X_0 and U_k = U_0 for every k -- set by cold_start() and reset(), cleared by everything that writes dX / dU
    // (invalidate below). lin_dedup: options_set "lin_dedup", 1 by default. n_lin_uniform: linearisations that took the
    // uniform path (get_stats "lin_uniform"). hlin_bad: pinned word lin_fill_kernel sets when it finds a stage that differs from
    // stage 0 -- an invalidation missed here; checked at the synchronous entry points (lin_uniform_check).
    // capturing: tum_sim_run is recording a chunk of the closed loop into a graph (a captured launch is replayed on other iterates)
    bool iter_uniform = false, capturing = false; int lin_dedup = 1; int n_lin_uniform = 0; double *dlin1 = nullptr; int *hlin_bad = nullptr;
    // uniform_records: options_set "uniform_records", 0 by default -- a whole SQP-RTI step on a stage-uniform iterate writes NO stage
    // records where nothing behind it reads them (pipe_plan.hpp: plan_pipeline; cond_uniform_kernel and expand_uniform_kernel take lin1 and the
    // reference; the expansion holds the safety net then); 1: lin_fill_kernel always. n_records_skipped: get_stats "records_skipped"
    int uniform_records = 0; int n_records_skipped = 0;
    // uniform_powers: options_set "uniform_powers", 1 by default -- the record-free condensing forms the sequences A^m B and g_s once per
    // instance (cond_uniform_kernel); 0: every lane carries its column through every stage (cond_uniform_columns_kernel). Same results, to the bit.
    int uniform_powers = 1;
    // uniform_shift: options_set "uniform_shift", 1 by default -- cond_uniform_kernel<5> forms the Hessian tiles below block row 0 from those of
    // block row 0 where the cost weights are the same at every stage (pipe_kernels.hpp: the SHIFT form); 0: every tile from its own products.
    // Same results, to the bit. dshift: one int per instance, 1 where the last cond_uniform_kernel took the form (get_stats "cond_shifted",
    // summed on the host when asked); shift_counted: the last condensing was that kernel
    int uniform_shift = 1; int *dshift = nullptr; bool shift_counted = false;
    // tum_ocp_get_condensed_qp: the hand-over buffers hold a condensed QP (a pipeline preparation or solve has run); PV_DV holds the
    // step of that QP (the interior point kernel wrote it for an expansion kernel behind it: its own tail keeps the step in LDS)
    bool qp_handed = false, dv_handed = false;
};

// cold_start() / reset() re-initialise the iterate: a capsule the safety net has failed works again from there. The word may only be
// written once the kernels that could still set it have finished (they never do in a correct library: the wait is paid after an error only)
static void lin_uniform_rearm(tum_ocp *c)
{
    if (!c->hlin_bad || !*(volatile int *)c->hlin_bad) return;
    (void)hipStreamSynchronize(c->stream);
    *(volatile int *)c->hlin_bad = 0;
}
// the safety net of the uniform linearisation, at the points where the host has waited for the stream anyway
static int lin_uniform_check(const tum_ocp *c)
{
    // (the text is part of the interface and keeps its wording: the call it names is invalidate(c, CH_ITERATE) below)
    if (c->hlin_bad && *(volatile int *)c->hlin_bad)
        return fail("the uniform linearisation (lin_dedup) ran on an iterate that was NOT the same at every stage: the results since the last "
                    "cold_start() / reset() are wrong. This is a bug of the library (a writer of the iterate that does not call iterate_changed). "
                    "Every synchronous call fails until the next cold_start() / reset(); options_set('lin_dedup', 0) before it avoids the path");
    return 0;
}

// What an entry point WROTE. It says so to invalidate() and sets none of the flags below itself.
enum : unsigned {
    CH_ITERATE = 1,       // dX / dU (the sample copies with them)
    CH_RESTART = 2,       // cold_start() / reset() have enqueued their re-initialisation: the iterate is the same at every stage now, and
                          // there has been no solve since. Passed on its own, behind the CH_ITERATE of the same entry point
    CH_REF = 4,           // the reference (tum_sim_set_state: the pose the planner derives the next one from)
    CH_W = 8,             // W, diagonal or full
    CH_X0 = 16,           // x0, of the nominal copy or the samples
    CH_BOUNDS = 32,       // bounds of the stages >= 1, slack penalties
    CH_VARIANT = 64,      // the kernel variant, the array x0 / yref is bound to
    CH_CAPTURED = 128,    // something a captured launch holds by value (tum_ocp::epoch)
    CH_RESULTS = 256,     // cost, status and iteration counts: a solve is being enqueued
    CH_UPLOAD = 512       // tum_ocp_put_device / tum_sim_set_state uploaded an input. Nothing the getters serve changed, but both have
                          // always dropped the cache, and that is kept
};
// The one place that knows what a write invalidates. Per row:
//   prep     a pending preparation has read it: 1 -> 2, the feedback is refused (x0, the bounds of the stages >= 1 and the slack
//            penalties are read by the feedback itself: they do not -- their rows say so and do nothing else)
//   cache    the pinned slabs the getters are served from (tum_ocp_solve) and the SNMPC sample copies beside them are dropped. The host
//            setters of yref / W / x0 / bounds leave them: the 83-call control step sets the next step's inputs behind its getters
//   uniform  -1 the next linearisation is the general one, +1 it may be the uniform one (and the multipliers are an earlier problem's)
//   epoch    tum_sim_run captures its chunk again
static void invalidate(tum_ocp *c, unsigned what)
{
    static const struct { unsigned bit; bool prep, cache; int uniform; bool epoch; } table[] = {
        {CH_ITERATE,  true,  true,  -1, false},
        {CH_RESTART,  false, false, +1, false},
        {CH_REF,      true,  false,  0, false},
        {CH_W,        true,  false,  0, false},
        {CH_X0,       false, false,  0, false},
        {CH_BOUNDS,   false, false,  0, false},
        {CH_VARIANT,  true,  false,  0, false},
        {CH_CAPTURED, false, false,  0, true},
        {CH_RESULTS,  false, true,   0, false},
        {CH_UPLOAD,   false, true,   0, false},
    };
    for (const auto &r : table) {
        if (!(what & r.bit)) continue;
        if (r.prep && c->prep == 1) c->prep = 2;
        if (r.cache) c->cache_valid = c->xs_cached = false;
        if (r.uniform) c->iter_uniform = r.uniform > 0;
        if (r.uniform > 0) { c->cold = true; lin_uniform_rearm(c); }
        if (r.epoch) c->epoch++;
    }
}

static const int DBG_STRIDE = 20480;
static const int DBG_INST = 4;

extern "C" const char *tum_ocp_last_error(void) { return g_err.c_str(); }
extern "C" int tum_ocp_batch(const tum_ocp *c) { return c->batch; }
extern "C" int tum_ocp_horizon(const tum_ocp *c) { return c->N; }

// Every entry point that touches the device runs under the capsule's device and leaves the caller's (torch's) current
// device as it found it: two capsules on different GPUs may live in one process.
struct DevGuard {
    int prev = -1, dev; bool changed = false, ok = true;
    explicit DevGuard(int d) : dev(d)
    {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != d) { changed = hipSetDevice(d) == hipSuccess; ok = changed; }
    }
    ~DevGuard() { if (changed) (void)hipSetDevice(prev); }
};
// entry points that allocate or launch refuse to run on the caller's device when the switch failed
#define GUARD_OK(g) do { if (!(g).ok) return fail("hipSetDevice failed"); } while (0)

// temporary device buffer that cannot leak on an early error return
struct DevTmp {
    void *p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <typename T> T *as() const { return (T *)p; }
};

template <typename T>
static hipError_t dalloc(T **p, size_t n)
{
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(T));
    // hipMemset on device memory returns before the fill has run, and the fill runs on the NULL stream -- which the capsule's
    // non-blocking stream does not wait for. Without this wait the first solve after a large allocation races the fill: at
    // 65 536 instances the fill of the pipeline's 4.4 GB of workspace was still zeroing what the first eighth of the instances
    // had already handed from kernel to kernel (wrong first solves at batches >= 32 768; scripts/probes/large_batch_variants.py).
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

// the vehicle constants the OCP's model (Model) and the plant of the closed loop (PlantModel) share
template <typename M>
static void vehicle_constants(M &m, const tum_ocp_desc &d)
{
    m.lf = d.lf; m.lr = d.lr; m.m = d.m; m.inv_m = 1.0 / d.m; m.inv_Iz = 1.0 / d.Iz;
    m.ka = 0.5 * d.ro * d.S * d.Cd;
    m.Bf = d.Bf; m.Cf = d.Cf; m.Df = d.Df; m.Ef = d.Ef;
    m.Br = d.Br; m.Cr = d.Cr; m.Dr = d.Dr; m.Er = d.Er;
    m.Fz_f = d.m * d.lr * d.g / (d.lf + d.lr);
    m.Fz_r = d.m * d.lf * d.g / (d.lf + d.lr);
    m.invFmax_f = 1.0 / std::sqrt(m.Fz_f * m.Fz_f + (d.Cf * m.Fz_f) * (d.Cf * m.Fz_f));
    m.invFmax_r = 1.0 / std::sqrt(m.Fz_r * m.Fz_r + (d.Cr * m.Fz_r) * (d.Cr * m.Fz_r));
    m.fr0 = d.fr0; m.fr1 = d.fr1; m.fr4 = d.fr4;
}

extern "C" tum_ocp *tum_ocp_create(const tum_ocp_desc *desc)
{
    if (!desc) { fail("null desc"); return nullptr; }
    if (desc->N < 1 || desc->N > TUM_N_MAX) { fail("N out of range (1..56)"); return nullptr; }
    if (desc->batch < 1) { fail("batch < 1"); return nullptr; }
    if (desc->nsub < 1 || !(desc->dt > 0)) { fail("bad nsub/dt"); return nullptr; }
    if (desc->n_ggv < 2 || desc->n_ggv > 16) { fail("n_ggv out of range (2..16)"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device: libtumnmpc has no CPU fallback"); return nullptr; }
    if (desc->device < 0 || desc->device >= ndev) { fail("device ordinal out of range"); return nullptr; }
    DevGuard guard(desc->device); if (!guard.ok) { fail("hipSetDevice failed"); return nullptr; }
    tum_ocp *c = new tum_ocp();
    c->d = *desc; c->N = desc->N; c->batch = desc->batch;
    const int N = c->N; const size_t B = c->batch;
    bool ok = true;
    ok &= hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess; c->own_stream = true;
    ok &= hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
    ok &= dalloc(&c->dX, B * (N + 1) * NX) == hipSuccess;
    ok &= dalloc(&c->dU, B * N * NU) == hipSuccess;
    ok &= dalloc(&c->dlin1, B * LIN1) == hipSuccess;
    ok &= hipMalloc((void **)&c->dshift, sizeof(int) * B) == hipSuccess;
    ok &= hipHostMalloc((void **)&c->hlin_bad, sizeof(int), hipHostMallocDefault) == hipSuccess;
    if (c->hlin_bad) *c->hlin_bad = 0;
    ok &= dalloc(&c->dx0, B * NX) == hipSuccess;
    ok &= dalloc(&c->dyref, B * (N + 1) * 6) == hipSuccess;
    c->dx0_own = c->dx0; c->dyref_own = c->dyref;
    ok &= dalloc(&c->dW, B * (size_t)(N + 1) * 6) == hipSuccess;          // diagonal of W per stage (stage N: the first 4 = W_e)
    ok &= dalloc(&c->dpen, B * 36) == hipSuccess;
    ok &= dalloc(&c->dbnd, B * 6 * (N + 1)) == hipSuccess;
    ok &= dalloc(&c->dcost, B) == hipSuccess;
    ok &= dalloc(&c->dres, B * 3) == hipSuccess;
    ok &= dalloc(&c->dslack, B * 6 * N) == hipSuccess;
    ok &= dalloc(&c->dstatus, B) == hipSuccess;
    ok &= dalloc(&c->dqpiter, B) == hipSuccess;
    ok &= dalloc(&c->dqpstatus, B) == hipSuccess;
    ok &= dalloc(&c->dorder, B) == hipSuccess;
    ok &= dalloc(&c->dqplam, B * (6 * (size_t)N + 2)) == hipSuccess;      // warm start of the interior point method: multipliers | converged flag
    { const char *e = getenv("TUM_NMPC_SCHEDULE"); c->lpt = !(e && std::string(e) == "natural"); }
    if (ok) {   // start from the identity map: the schedule is always a valid permutation
        std::vector<int> id(B);
        for (size_t i = 0; i < B; i++) id[i] = (int)i;
        ok &= hipMemcpy(c->dorder, id.data(), sizeof(int) * B, hipMemcpyHostToDevice) == hipSuccess;
        c->order_valid = true;
    }
#ifdef TUM_DEV_KERNELS      // (only the fused kernel writes A | B | b per stage; the pipeline's stage records hold them)
    if (desc->store_qp_in) ok &= dalloc(&c->dqpin, B * N * 88) == hipSuccess;
#endif
    ok &= dalloc(&c->ddbg, (size_t)DBG_STRIDE * DBG_INST) == hipSuccess;
    ok &= dalloc(&c->dprof, B * 12) == hipSuccess;
#ifdef TUM_DEV_KERNELS      // (linearisation records parked by the fused kernel during its interior point loop)
    ok &= dalloc(&c->dws, B * WS_DOUBLES) == hipSuccess;
#endif
    { const char *e = getenv("TUM_NMPC_KERNEL"); const std::string k(e ? e : "auto"); c->kmode = (k == "pipeline") ? KMode::PIPELINE : KMode::AUTO;
#ifdef TUM_DEV_KERNELS
      if (k == "fused") c->kmode = KMode::FUSED; else if (k == "pipeline4") c->kmode = KMode::PIPELINE4;
#endif
    }
    ok &= hipEventCreate(&c->evi0) == hipSuccess && hipEventCreate(&c->evi1) == hipSuccess;
    if (!ok) { fail("device allocation failed"); tum_ocp_free(c); return nullptr; }

    KArgs &ka = c->ka;
    memset(&ka, 0, sizeof(ka));
    ka.N = N; ka.nsub = desc->nsub; ka.batch = c->batch; ka.flags = desc->store_qp_in ? KF_STORE_QP_IN : 0; ka.dt = desc->dt;
    ka.iter_max = desc->qp_iter_max > 0 ? desc->qp_iter_max : 50;
    ka.tol_stat = desc->qp_tol_stat > 0 ? desc->qp_tol_stat : 1e-8;
    ka.tol_ineq = desc->qp_tol_ineq > 0 ? desc->qp_tol_ineq : 1e-8;
    ka.tol_comp = desc->qp_tol_comp > 0 ? desc->qp_tol_comp : 1e-8;
    ka.mu0 = desc->qp_mu0 > 0 ? desc->qp_mu0 : 0.05;
    ka.t0 = desc->qp_t0 > 0 ? desc->qp_t0 : 0.05;
    ka.reg = 0.0;
    // qp_solver_warm_start (SNMPC_acados_settings.py:307): the interior point method starts from the previous QP's multipliers
    ka.warm_mu = desc->qp_warm_start ? (desc->qp_warm_mu > 0 ? desc->qp_warm_mu : 1e-2) : 0.0;
    ka.qp_lam = c->dqplam;
    // (the gate of the warm start: constants of the oracle study, scripts/study/warm_gate.py; TUM_WARM_GATE=0 removes it -- development aid)
    // tum_ocp_desc.qp_warm_flips / qp_warm_viol override them (flips < 0: no gate)
    { const char *e = getenv("TUM_WARM_GATE");
      ka.warm_flips = (e && e[0] == '0') ? -1 : (desc->qp_warm_flips != 0 ? desc->qp_warm_flips : 16);
      ka.warm_viol = desc->qp_warm_viol > 0 ? desc->qp_warm_viol : 0.1; }
    Model &m = ka.mp;
    vehicle_constants(m, *desc);
    m.ax_brake = -desc->acc_min;
    m.n_ggv = desc->n_ggv;
    for (int i = 0; i < 16; i++) { m.ggv_v[i] = desc->ggv_v[i]; m.ggv_ax[i] = desc->ggv_ax[i]; m.ggv_ay[i] = desc->ggv_ay[i]; }
    ka.X = c->dX; ka.U = c->dU; ka.x0 = c->dx0; ka.yref = c->dyref; ka.W = c->dW; ka.pen = c->dpen; ka.bnd = c->dbnd;
    ka.cost = c->dcost; ka.res = c->dres; ka.slack = c->dslack;
    ka.status = c->dstatus; ka.qp_iter = c->dqpiter; ka.qp_status = c->dqpstatus;
    ka.qpin = c->dqpin; ka.dbg = c->ddbg; ka.dbg_stride = DBG_STRIDE; ka.prof = c->dprof; ka.ws = c->dws;

    if (hipFuncSetAttribute((const void *)ipm_kernel<false, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)ipm_kernel<true, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)ipm_kernel<false, 6>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)ipm_kernel<false, 5, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)ipm_kernel<false, 6, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess
#ifdef TUM_DEV_KERNELS
        || hipFuncSetAttribute((const void *)ipm4_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)ipm4_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)nmpc_rti_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute((const void *)nmpc_rti_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute((const void *)nmpc_rti_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute((const void *)nmpc_rti_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess
#endif
        ) {
        fail("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"); tum_ocp_free(c); return nullptr;
    }
    return c;
}

extern "C" void tum_ocp_free(tum_ocp *c)
{
    if (!c) return;
    DevGuard guard(c->d.device);
    (void)hipFree(c->dX); (void)hipFree(c->dU); (void)hipFree(c->dx0_own); (void)hipFree(c->dyref_own); (void)hipFree(c->dW); if (c->dWf) (void)hipFree(c->dWf); (void)hipFree(c->dpen); (void)hipFree(c->dbnd);
    (void)hipFree(c->dqplam);
    (void)hipFree(c->dcost); (void)hipFree(c->dres); (void)hipFree(c->dslack); (void)hipFree(c->dstatus); (void)hipFree(c->dqpiter); (void)hipFree(c->dqpstatus); (void)hipFree(c->dorder);
    if (c->dqpin) (void)hipFree(c->dqpin);
    (void)hipFree(c->ddbg); (void)hipFree(c->dprof); (void)hipFree(c->dws); (void)hipFree(c->dhws); (void)hipFree(c->drec); (void)hipFree(c->dcws); (void)hipFree(c->dvec);
    if (c->evi0) (void)hipEventDestroy(c->evi0);
    if (c->evi1) (void)hipEventDestroy(c->evi1);
    (void)hipFree(c->dXS); (void)hipFree(c->dxs0); (void)hipFree(c->dApce); (void)hipFree(c->dws2); (void)hipFree(c->dpro); (void)hipFree(c->ddv); (void)hipFree(c->doffs); (void)hipFree(c->dxs_dirty);
    (void)hipFree(c->dr2S); (void)hipFree(c->dr2B); (void)hipFree(c->dpceA); (void)hipFree(c->dbnd_snap);
    (void)hipFree(c->dsum); (void)hipFree(c->dx0prep); (void)hipFree(c->dlin1); (void)hipFree(c->dshift);
    if (c->hlin_bad) (void)hipHostFree(c->hlin_bad);
    (void)hipFree(c->dnlpres); (void)hipFree(c->dsnap); (void)hipFree(c->dsqpstate); (void)hipFree(c->dsqpiter); (void)hipFree(c->dsnapi); (void)hipFree(c->dactive);
    if (c->hactive) (void)hipHostFree(c->hactive);
    (void)hipFree(c->dmalpha); (void)hipFree(c->dmmu); (void)hipFree(c->dmtable); (void)hipFree(c->dmhist);
    for (hipEvent_t e : c->evpoll) if (e) (void)hipEventDestroy(e);
    if (c->hin_s) (void)hipHostFree(c->hin_s);
    if (c->hsum_s) (void)hipHostFree(c->hsum_s);
    if (c->hX_s) (void)hipHostFree(c->hX_s);
    if (c->hU_s) (void)hipHostFree(c->hU_s);
    if (c->hts_s) (void)hipHostFree(c->hts_s);
    if (c->hXS_s) (void)hipHostFree(c->hXS_s);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (int i = 0; i < 2; i++) {
        if (c->hsum[i]) (void)hipHostFree(c->hsum[i]);
        if (c->hin[i]) (void)hipHostFree(c->hin[i]);
        if (c->hts[i]) (void)hipHostFree(c->hts[i]);
        if (c->hX[i]) (void)hipHostFree(c->hX[i]);
        if (c->hU[i]) (void)hipHostFree(c->hU[i]);
        if (c->evres[i]) (void)hipEventDestroy(c->evres[i]);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// dynamic LDS (doubles) of the prologue kernel that `want` (a capsule's choice, < 0: the library's) selects for (uph, ns)
// (nsb: the compile-time bound of the kernels' sample / PCE-term sums: 16, or 32 where either count exceeds 16)
static int sn_nsb(int ns, int L) { return (ns > SN_B16 || L > SN_B16) ? SN_NSMAX : SN_B16; }
static size_t sn_prologue_lds(int uph, int ns, int want, int nsb = SN_B16)
{
    const int kind = sn_prologue_kind(uph, ns, want);
    if (kind == 2 && nsb == SN_B16) return sn_mfma_lds_doubles(uph, ns);
    return sn_prologue_lds_doubles(uph, ns, nsb == SN_B16 ? sn_prologue_variant(uph, ns) : 0, nsb);
}

// Turn the capsule into the coupled SNMPC OCP: the stacked state is the nominal copy followed by `ns`
// sample copies; A_pce (L x ns, row-major) and the uncertainty propagation horizon replace the per-stage parameter
// vector p = [A_pce.flatten(), risk_parameter, stop_flag] of the reference (SNMPC_class.py:103-104,124).
extern "C" int tum_ocp_snmpc_attach(tum_ocp *c, int ns, int L, const double *Apce, int uph, double gamma)
{
    if (!c || !Apce) return fail("null argument");
    if (c->sn) return fail("snmpc_attach: already attached");
    if (c->dWf) return fail("snmpc_attach: the capsule holds a full W; the coupled SNMPC OCP takes a diagonal one");
    if (ns < 1 || ns > SN_NSMAX) return fail("snmpc_attach: n_samples out of range (1..32)");
    if (L < 1 || L > SN_LMAX) return fail("snmpc_attach: number of PCE terms out of range (1..32)");
    if (uph < 0 || uph > c->N || uph > SN_UPHMAX) return fail("snmpc_attach: uncertainty propagation horizon out of range (0..N)");
    if (!(gamma > 0.0 && gamma <= 1.0)) return fail("snmpc_attach: gamma out of range (0,1]");
    if (c->d.nsub != 1) return fail("snmpc_attach: the SNMPC model is DISCRETE with one RK4 step per stage: create the capsule with nsub = 1");
    if (c->d.store_qp_in) return fail("snmpc_attach: store_qp_in is not available for the stacked state");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    {
        const size_t lds = sizeof(double) * (sn_prologue_lds(uph, ns, c->sn_prologue, sn_nsb(ns, L)));
        if (lds > 128 * 1024) return fail("snmpc_attach: n_samples x uph too large for the prologue kernel's LDS");
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_mfma_kernel<SN_MFMA_NSW, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<0, SN_NSMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<6>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<9>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<13>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)snmpc_prologue_kernel<17>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    }
    const size_t B = c->batch; const int N = c->N;
    bool ok = true;
    ok &= dalloc(&c->dXS, B * (N + 1) * ns * NX) == hipSuccess;
    ok &= dalloc(&c->dxs0, B * ns * NX) == hipSuccess;
    ok &= dalloc(&c->dApce, (size_t)L * ns) == hipSuccess;
    ok &= dalloc(&c->dws2, B * (size_t)(uph > 0 ? uph : 1) * ns * (ABS + 5)) == hipSuccess;      // records, then the gg values / gradients
    ok &= dalloc(&c->dpro, B * (size_t)(uph > 0 ? uph : 1) * sn_pro_stage(uph)) == hipSuccess;
    ok &= dalloc(&c->ddv, B * NVP) == hipSuccess;
    ok &= dalloc(&c->doffs, (size_t)ns * NX) == hipSuccess;
    if (ok) { (void)hipFree(c->dxs_dirty); c->dxs_dirty = nullptr; ok &= hipMalloc((void **)&c->dxs_dirty, sizeof(int) * B) == hipSuccess; }
    if (!ok) return fail("snmpc_attach: device allocation failed");
    HIPCHK(hipMemset(c->dxs_dirty, 0, sizeof(int) * B)); HIPCHK(hipDeviceSynchronize()); c->xs_lazy = false;
    HIPCHK(hipMemcpy(c->dApce, Apce, sizeof(double) * L * ns, hipMemcpyHostToDevice));
    SnArgs &sa = c->sa;
    memset(&sa, 0, sizeof(sa));
    sa.N = N; sa.batch = c->batch; sa.ns = ns; sa.L = L; sa.uph = uph; sa.dt = c->ka.dt;
    sa.kappa = std::sqrt((1.0 - gamma) / gamma);      // SNMPC_acados_settings.py:187
    sa.mp = c->ka.mp;
    sa.X = c->dX; sa.U = c->dU; sa.XS = c->dXS; sa.xs0 = c->dxs0; sa.Apce = c->dApce; sa.ws2 = c->dws2; sa.pro = c->dpro;
    sa.gh = c->dws2 + B * (size_t)(uph > 0 ? uph : 1) * ns * ABS;
    sa.dv = c->ddv; sa.dv_stride = NVP; sa.status = c->dstatus; sa.xs_dirty = c->dxs_dirty;
    sa.dbg = c->ddbg + 20000;                            // tail of instance 0's dump area (tum_ocp_debug_dump), unused by the fused kernel
    c->ka.uph = uph; c->ka.pro = c->dpro; c->ka.dv = c->ddv;
    c->sn = true;
    c->hApce.assign(Apce, Apce + (size_t)L * ns);
    c->gamma = gamma; c->uph_cap = uph > 0 ? uph : 1; c->pro_cap = (size_t)(uph > 0 ? uph : 1) * sn_pro_stage(uph);
    c->p_gamma.assign(N + 1, gamma); c->p_stop.assign(N + 1, 0.0);
    for (int k = uph; k <= N; k++) c->p_stop[k] = 1.0;
    c->p_dirty = false;
    invalidate(c, CH_CAPTURED);
    return 0;
}

// acados_solver.set(stage, "p", [A_pce.flatten(), risk_parameter, stop_flag])   SNMPC_class.py:124,185,193.
// A_pce and the risk parameter are shared by all stages of the stacked model (the reference sends the same values to every
// stage); the stop flags must form the pattern the model is built for -- 0 on the stages < uph, 1 from stage uph on
// (SNMPC_class.py:103-104) -- and define the uncertainty propagation horizon. Applied at the next solve.
static int sn_set_p(tum_ocp *c, int stage, const double *v, int len, int nb, int stride)
{
    if (!c->sn) return fail("set p: not an SNMPC capsule (tum_ocp_snmpc_attach)");
    const int L = c->sa.L, ns = c->sa.ns, N = c->N;
    if (stage < 0 || stage > N) return fail("set p: stage out of range");
    if (len != L * ns + 2) return fail("set p: mismatching dimension for field \"p\" with dimension " + std::to_string(L * ns + 2) +
                                       " (you have " + std::to_string(len) + ")");
    if (stride != 0)
        for (int i = 1; i < nb; i++)
            if (memcmp(v, v + (size_t)i * stride, sizeof(double) * len) != 0) return fail("set p: the parameter vector is shared by all instances of the batch");
    const double g = v[L * ns], sf = v[L * ns + 1];
    if (!(g > 0.0 && g <= 1.0)) return fail("set p: risk parameter out of range (0,1]");
    if (sf != 0.0 && sf != 1.0) return fail("set p: stop_flag must be 0 or 1");
    if (memcmp(v, c->hApce.data(), sizeof(double) * L * ns) != 0) {
        DevGuard guard(c->d.device); GUARD_OK(guard);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(c->dApce, v, sizeof(double) * L * ns, hipMemcpyHostToDevice));
        c->hApce.assign(v, v + (size_t)L * ns);
    }
    c->p_gamma[stage] = g; c->p_stop[stage] = sf;
    c->p_dirty = true;
    return 0;
}
// linearisation of the sample stages (K-S1), in front of the prologue kernel
static void sn_launch_lin(tum_ocp *c)
{
    const long long items = (long long)c->batch * c->sa.uph * c->sa.ns;
    if (items <= 0) return;
    // eight lanes per item while that still is one round of wavefronts on the chip (the same rule as plan_pipeline's for lin_cols_kernel, pipe_plan.hpp)
    const int want = (c->lin_cols >= 0) ? c->lin_cols : env().plan.lin_cols;
    if (want > 0 || (want < 0 && items * SLC_LANES <= 64LL * 1024))
        hipLaunchKernelGGL(snmpc_lin_cols_kernel, dim3((unsigned)((items + SLC_ITEMS - 1) / SLC_ITEMS)), dim3(64), 0, c->stream, c->sa);
    else hipLaunchKernelGGL(snmpc_lin_kernel, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, c->stream, c->sa);
}

// the epilogue leaves the sample copies of the stages > uph for later (snmpc_epilogue_kernel); this brings them up to date
static int sn_materialise(tum_ocp *c)
{
    if (!c->sn || !c->xs_lazy) return 0;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    hipLaunchKernelGGL(snmpc_freeze_kernel, dim3(c->batch), dim3(256), 0, c->stream, c->dXS, c->dxs_dirty, c->N, c->sa.ns, c->sa.uph, c->batch);
    HIPCHK(hipGetLastError());
    c->xs_lazy = false;
    return 0;
}

// the stacked state behind a synchronous solve of a small SNMPC capsule: the reference reads get(j, "x")[0:8] on every stage
// (SNMPC_class.py:205-209) -- the sample copies of all stages come back in ONE copy on the first such read
static int sn_cache_samples(tum_ocp *c)
{
    if (!c->sn || !c->cache_valid || c->xs_cached) return 0;
    if (sn_materialise(c)) return 1;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const size_t n = (size_t)c->batch * (c->N + 1) * c->sa.ns * NX;
    if (!c->hXS_s) HIPCHK(hipHostMalloc((void **)&c->hXS_s, sizeof(double) * n, hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(c->hXS_s, c->dXS, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->xs_cached = true;
    return 0;
}

// resolve the per-stage parameters into (uph, kappa) before a solve
static int sn_apply_p(tum_ocp *c)
{
    if (!c->p_dirty) return 0;
    const int N = c->N, ns = c->sa.ns;
    for (int k = 1; k <= N; k++)
        if (c->p_gamma[k] != c->p_gamma[0]) return fail("solve: the risk parameter p[-2] differs between stages (stage " + std::to_string(k) + ")");
    int uph = N + 1;
    for (int k = 0; k <= N; k++) if (c->p_stop[k] == 1.0) { uph = k; break; }
    for (int k = uph; k <= N; k++)
        if (c->p_stop[k] != 1.0) return fail("solve: stop_flag pattern not supported: it must be 0 on the stages < uph and 1 from stage uph on (stage " + std::to_string(k) + " is 0 after a 1)");
    if (uph > N) uph = N;                      // no stop flag at all: the samples are propagated over the whole horizon
    if (uph > SN_UPHMAX) return fail("solve: uncertainty propagation horizon from the stop flags exceeds " + std::to_string(SN_UPHMAX));
    if (sizeof(double) * (sn_prologue_lds(uph, ns, c->sn_prologue, sn_nsb(ns, c->sa.L))) > 128 * 1024)      // (the variant sn_launch_prologue will pick)
        return fail("solve: n_samples x uph too large for the prologue kernel's LDS");
    // (the hand-over buffer of the prologue is sized uph x sn_pro_stage(uph): its row pitch doubles beyond uph = 31)
    if (uph > c->uph_cap || (size_t)uph * sn_pro_stage(uph) > c->pro_cap) {
        DevGuard guard(c->d.device); GUARD_OK(guard);
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipFree(c->dws2); (void)hipFree(c->dpro); c->dws2 = c->dpro = nullptr;
        const size_t B = c->batch;
        c->pro_cap = (size_t)uph * sn_pro_stage(uph);
        if (dalloc(&c->dws2, B * (size_t)uph * ns * (ABS + 5)) != hipSuccess || dalloc(&c->dpro, B * c->pro_cap) != hipSuccess)
            return fail("solve: device allocation failed for the longer uncertainty propagation horizon");
        c->uph_cap = uph; c->sa.ws2 = c->dws2; c->sa.gh = c->dws2 + B * (size_t)uph * ns * ABS; c->sa.pro = c->dpro; c->ka.pro = c->dpro;
    }
    if (uph != c->sa.uph) {
        if (sn_materialise(c)) return 1;          // (the frozen copies belong to the horizon they were solved with)
        // the prologue only writes the live columns of a stage (2k+3 of them) and relies on the rest of its hand-over
        // buffers being zero; the per-instance stride of both buffers depends on uph, so a new horizon starts from zeros
        DevGuard guard(c->d.device); GUARD_OK(guard);
        HIPCHK(hipMemsetAsync(c->dws2, 0, sizeof(double) * (size_t)c->batch * c->uph_cap * ns * ABS, c->stream));
        HIPCHK(hipMemsetAsync(c->dpro, 0, sizeof(double) * (size_t)c->batch * c->pro_cap, c->stream));
    }
    c->gamma = c->p_gamma[0];
    c->sa.kappa = std::sqrt((1.0 - c->gamma) / c->gamma);
    c->sa.uph = uph; c->ka.uph = uph;
    c->p_dirty = false;
    invalidate(c, CH_CAPTURED);                   // (uph, kappa and the work buffers are kernel arguments of a captured launch)
    return 0;
}
extern "C" int tum_ocp_snmpc_samples(const tum_ocp *c) { return (c && c->sn) ? c->sa.ns : 0; }

// Offsets of the sample initial conditions from the nominal one (compute_x0dist, stochastic_mpc_utils.py:78-91:
// row s = x0 + stds * w_s), ns x 8 (host). Once registered, an 8-value lbx_0 / ubx_0 (and the device closed loop, whose
// state estimator writes the nominal x0) fans out to the sample copies on the device at every solve.
extern "C" int tum_ocp_snmpc_set_offsets(tum_ocp *c, const double *offs)
{
    if (!c || !offs) return fail("null argument");
    if (!c->sn) return fail("snmpc_set_offsets: not an SNMPC capsule (tum_ocp_snmpc_attach)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipMemcpy(c->doffs, offs, sizeof(double) * c->sa.ns * NX, hipMemcpyHostToDevice));
    c->have_offs = true;
    return 0;
}
static int sn_fanout(tum_ocp *c)
{
    const int n = c->batch * c->sa.ns * NX;
    hipLaunchKernelGGL(snmpc_fanout_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->dxs0, c->dx0, c->doffs, c->sa.ns, c->batch);
    HIPCHK(hipGetLastError());
    return 0;
}

static int chk_range(tum_ocp *c, int b0, int nb)
{
    if (!c) return fail("null capsule");
    if (b0 < 0 || nb < 1 || b0 + nb > c->batch) return fail("instance range out of bounds");
    return 0;
}

// the summary (and, for small batches, the iterate) is written by the packing kernel STRAIGHT into the pinned slab; TUM_RESULTS_ZERO_COPY=0
// (development aid) goes through a device slab and copy commands instead
static bool results_zero_copy()
{
    static const bool zc = [] { const char *e = getenv("TUM_RESULTS_ZERO_COPY"); return !(e && e[0] == '0'); }();
    return zc;
}
// does a results request of this capsule run as ONE kernel that writes summary, X and U into the pinned slabs (pack_results_kernel:
// the kernel that also reads the device clock at the end of a clocked step, tum_ocp_step_async)
static bool results_pack_all(const tum_ocp *c, int with_iterate)
{
    return results_zero_copy() && with_iterate && (size_t)c->batch * (size_t)(c->N + 1) * NX <= 32768;
}

// ---- the pinned shadow of the per-step inputs (x0 | yref) of a SMALL capsule
static bool small_inputs(const tum_ocp *c) { return (size_t)c->batch * (NX + (size_t)(c->N + 1) * 6) <= 32768 && c->N + 1 <= 64; }
static int shadow_ready(tum_ocp *c)
{
    if (!c->hin_s) {
        HIPCHK(hipHostMalloc((void **)&c->hin_s, sizeof(double) * (size_t)c->batch * (NX + (size_t)(c->N + 1) * 6), hipHostMallocDefault));
        // (a stage-N reference has four entries: the two behind it in its six-double record are uploaded with it and must not be garbage)
        memset(c->hin_s, 0, sizeof(double) * (size_t)c->batch * (NX + (size_t)(c->N + 1) * 6));
        HIPCHK(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    }
    // the upload kernel of an asynchronous solve may still be reading the shadow
    if (c->in_inflight) { HIPCHK(hipEventSynchronize(c->ev_in)); c->in_inflight = false; }
    return 0;
}
// host records (batch x len, `stride` apart; 0 = one record for all) into the shadow: x0 (stage < 0) or the yref record of a stage
static int shadow_write(tum_ocp *c, int stage, const double *v, int len, int stride)
{
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (shadow_ready(c)) return 1;
    const size_t B = c->batch, rec = (size_t)(c->N + 1) * 6;
    for (size_t b = 0; b < B; b++) {
        const double *src = v + b * (size_t)stride;
        double *dst = (stage < 0) ? c->hin_s + b * NX : c->hin_s + B * NX + b * rec + (size_t)stage * 6;
        memcpy(dst, src, sizeof(double) * len);
    }
    if (stage < 0) c->in_x0 = true; else c->in_mask |= 1ull << stage;
    invalidate(c, stage < 0 ? CH_X0 : CH_REF);
    return 0;
}
// pending setters -> device, one kernel on the capsule's stream (ts: the device clock at its start goes to ts[0])
static int flush_inputs(tum_ocp *c, unsigned long long *ts = nullptr, bool force = false)
{
    if (!c->in_x0 && !c->in_mask && !force) return 0;
    const size_t B = c->batch;
    hipLaunchKernelGGL(stage_in_masked_kernel, dim3(4), dim3(256), 0, c->stream, c->hin_s, c->dx0, (int)(B * NX), c->dyref, (int)(B * (c->N + 1) * 6),
                       c->N + 1, c->in_x0 ? 1 : 0, c->in_mask, ts);
    HIPCHK(hipGetLastError());
    if (c->in_x0 || c->in_mask) { HIPCHK(hipEventRecord(c->ev_in, c->stream)); c->in_inflight = true; }
    c->in_x0 = false; c->in_mask = 0;
    return 0;
}

// strided scatter: host records (nb x len, `stride` apart; stride 0 = broadcast) -> device rows; what: CH_* of the array written
static int put(tum_ocp *c, unsigned what, double *dbase, size_t rec, size_t off, const double *v, int len, int b0, int nb, int stride)
{
    if (stride != 0 && stride < len) return fail("stride < len");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if ((what & (CH_X0 | CH_REF)) && flush_inputs(c)) return 1;          // (older setters still in the shadow go first)
    invalidate(c, what);
    const double *src = v;
    size_t spitch = (size_t)stride * sizeof(double);
    if (stride == 0) {
        c->stage.assign((size_t)nb * len, 0.0);
        for (int i = 0; i < nb; i++) memcpy(&c->stage[(size_t)i * len], v, sizeof(double) * len);
        src = c->stage.data(); spitch = (size_t)len * sizeof(double);
    }
    HIPCHK(hipMemcpy2DAsync(dbase + (size_t)b0 * rec + off, rec * sizeof(double), src, spitch,
                            (size_t)len * sizeof(double), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
static int fetch(tum_ocp *c, const double *dbase, size_t rec, size_t off, double *v, int len, int b0, int nb, int stride)
{
    if (stride < len) return fail("stride < len");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipMemcpy2DAsync(v, (size_t)stride * sizeof(double), dbase + (size_t)b0 * rec + off, rec * sizeof(double),
                            (size_t)len * sizeof(double), nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return lin_uniform_check(c);
}

extern "C" int tum_ocp_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !v) return fail("null argument");
    const int N = c->N;
    const std::string f(field);
    if (f == "x") {
        if (stage == TUM_ALL_STAGES) { if (len != (N + 1) * NX) return fail("set x: len != (N+1)*8"); return put(c, CH_ITERATE, c->dX, (N + 1) * NX, 0, v, len, b0, nb, stride); }
        if (stage < 0 || stage > N) return fail("set x: stage out of range");
        if (c->sn && len == NX * (c->sa.ns + 1)) {   // stacked state: nominal copy, then the sample copies (SNMPC_class.py:126-127)
            if (stride != 0 && stride < len) return fail("stride < len");
            const int ns = c->sa.ns;
            // (a write to stage uph would change what the deferred freeze copies into the stages behind it: freeze first)
            if (stage >= c->sa.uph && sn_materialise(c)) return 1;
            if (put(c, CH_ITERATE, c->dX, (N + 1) * NX, (size_t)stage * NX, v, NX, b0, nb, stride)) return 1;
            return put(c, CH_ITERATE, c->dXS, (size_t)(N + 1) * ns * NX, (size_t)stage * ns * NX, v + NX, ns * NX, b0, nb, stride);
        }
        if (len != NX) return fail("set x: mismatching dimension, expected 8");
        return put(c, CH_ITERATE, c->dX, (N + 1) * NX, (size_t)stage * NX, v, len, b0, nb, stride);
    }
    if (f == "u") {
        if (stage == TUM_ALL_STAGES) { if (len != N * NU) return fail("set u: len != N*2"); return put(c, CH_ITERATE, c->dU, N * NU, 0, v, len, b0, nb, stride); }
        if (stage < 0 || stage >= N) return fail("set u: stage out of range");
        if (len != NU) return fail("set u: mismatching dimension, expected 2");
        return put(c, CH_ITERATE, c->dU, N * NU, (size_t)stage * NU, v, len, b0, nb, stride);
    }
    if (f == "yref") {
        if (stage == TUM_ALL_STAGES) { if (len != (N + 1) * 6) return fail("set yref: len != (N+1)*6"); return put(c, CH_REF, c->dyref, (N + 1) * 6, 0, v, len, b0, nb, stride); }
        if (stage < 0 || stage > N) return fail("set yref: stage out of range");
        const int want = (stage < N) ? TUM_NY : TUM_NYE;
        if (len != want) return fail("set yref: mismatching dimension for this stage");
        // the reference sets one stage per call, N + 1 calls per control step (NMPC_class.py:169-180): into the shadow, up with the solve
        if (b0 == 0 && nb == c->batch && small_inputs(c) && (stride == 0 || stride >= len)) return shadow_write(c, stage, v, len, stride);
        return put(c, CH_REF, c->dyref, (N + 1) * 6, (size_t)stage * 6, v, len, b0, nb, stride);
    }
    if (f == "p") {
        if (b0 != 0 || nb != c->batch) return fail("set p: the parameter vector is shared by all instances (b0 = 0, nb = batch)");
        return sn_set_p(c, stage, v, len, nb, stride);
    }
    return fail("set: unknown field '" + f + "'");
}

extern "C" int tum_ocp_get(tum_ocp *c, int stage, const char *field, double *v, int len, int b0, int nb, int stride)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !v) return fail("null argument");
    const int N = c->N;
    const std::string f(field);
    // after a synchronous solve of a small capsule the iterate is in the capsule's pinned slabs (tum_ocp_solve): the N + 1 getters the
    // reference issues per control step (NMPC_class.py:193-198) are host copies
    auto cached = [&](const double *slab, size_t rec, size_t off) {
        if (stride < len) return fail("stride < len");
        for (int i = 0; i < nb; i++) memcpy(v + (size_t)i * stride, slab + (size_t)(b0 + i) * rec + off, sizeof(double) * len);
        return 0;
    };
    if (f == "x") {
        if (stage == TUM_ALL_STAGES) {
            if (len != (N + 1) * NX) return fail("get x: len");
            if (c->cache_valid) return cached(c->hX_s, (size_t)(N + 1) * NX, 0);
            return fetch(c, c->dX, (N + 1) * NX, 0, v, len, b0, nb, stride);
        }
        if (c->sn && stage >= 0 && stage <= N && len == NX * (c->sa.ns + 1)) {
            const int ns = c->sa.ns;
            if (stride < len) return fail("stride < len");
            if (sn_cache_samples(c)) return 1;
            if (c->cache_valid && c->hXS_s) {          // the stacked state of every stage, read back ONCE after the solve
                for (int i = 0; i < nb; i++) {
                    memcpy(v + (size_t)i * stride, c->hX_s + ((size_t)(b0 + i) * (N + 1) + stage) * NX, sizeof(double) * NX);
                    memcpy(v + (size_t)i * stride + NX, c->hXS_s + ((size_t)(b0 + i) * (N + 1) + stage) * ns * NX, sizeof(double) * ns * NX);
                }
                return 0;
            }
            if (stage > c->sa.uph && sn_materialise(c)) return 1;
            if (fetch(c, c->dX, (N + 1) * NX, (size_t)stage * NX, v, NX, b0, nb, stride)) return 1;
            return fetch(c, c->dXS, (size_t)(N + 1) * ns * NX, (size_t)stage * ns * NX, v + NX, ns * NX, b0, nb, stride);
        }
        if (stage < 0 || stage > N || len != NX) return fail("get x: bad stage/len");
        if (c->cache_valid) return cached(c->hX_s, (size_t)(N + 1) * NX, (size_t)stage * NX);
        return fetch(c, c->dX, (N + 1) * NX, (size_t)stage * NX, v, len, b0, nb, stride);
    }
    if (f == "u") {
        if (stage == TUM_ALL_STAGES) {
            if (len != N * NU) return fail("get u: len");
            if (c->cache_valid) return cached(c->hU_s, (size_t)N * NU, 0);
            return fetch(c, c->dU, N * NU, 0, v, len, b0, nb, stride);
        }
        if (stage < 0 || stage >= N || len != NU) return fail("get u: bad stage/len");
        if (c->cache_valid) return cached(c->hU_s, (size_t)N * NU, (size_t)stage * NU);
        return fetch(c, c->dU, N * NU, (size_t)stage * NU, v, len, b0, nb, stride);
    }
    if (f == "sl" || f == "su") {
        // acados order per stage: stage 0 [sbu], stages 1..N-1 [sbu,sbx,sh], stage N [sbx,sh]
        const int want = (stage == 0) ? 1 : (stage == N ? 2 : 3);
        if (stage < 0 || stage > N || len != want) return fail("get sl/su: bad stage/len");
        std::vector<double> all((size_t)nb * 6 * N);
        if (fetch(c, c->dslack, 6 * N, 0, all.data(), 6 * N, b0, nb, 6 * N)) return 1;
        const int side = (f == "su") ? 3 * N : 0;
        for (int i = 0; i < nb; i++) {
            const double *s = &all[(size_t)i * 6 * N + side];
            double *o = v + (size_t)i * stride; int n = 0;
            if (stage < N) o[n++] = s[stage];
            if (stage >= 1) { o[n++] = s[N + 2 * (stage - 1)]; o[n++] = s[N + 2 * (stage - 1) + 1]; }
        }
        return 0;
    }
    if (f == "lam") {
        // multipliers of the last QP's rows (acados appends those of the slack bounds; not kept here): per stage the lower sides in the
        // order of sl, then the upper sides in the order of su
        const int want = (stage == 0) ? 2 : (stage == N ? 4 : 6);
        if (stage < 0 || stage > N || len != want) return fail("get lam: bad stage/len");
        if (stride < len) return fail("stride < len");
        const int nl = 6 * N + 2;
        std::vector<double> all((size_t)nb * nl);
        if (fetch(c, c->dqplam, nl, 0, all.data(), nl, b0, nb, nl)) return 1;
        for (int i = 0; i < nb; i++) {
            double *o = v + (size_t)i * stride; int n = 0;
            for (int side = 0; side < 2; side++) {
                const double *s = &all[(size_t)i * nl + (size_t)side * 3 * N];
                if (stage < N) o[n++] = s[stage];
                if (stage >= 1) { o[n++] = s[N + 2 * (stage - 1)]; o[n++] = s[N + 2 * (stage - 1) + 1]; }
            }
        }
        return 0;
    }
    return fail("get: unknown field '" + f + "'");
}

extern "C" int tum_ocp_constraints_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !v) return fail("null argument");
    const int N = c->N, NB = N + 1;
    const std::string f(field);
    if (stage < 0 || stage > N) return fail("constraints_set: stage out of range");
    if (f == "lbx" || f == "ubx") {
        if (stage == 0) {   // x0 equality: lbx_0 = ubx_0 = x0 (NMPC_class.py:243-246)
            if (c->sn && len == NX * (c->sa.ns + 1)) {   // x0 of all copies (SNMPC_class.py:262-264)
                if (stride != 0 && stride < len) return fail("stride < len");
                c->fanout = false;
                if (put(c, CH_X0, c->dx0, NX, 0, v, NX, b0, nb, stride)) return 1;
                return put(c, CH_X0, c->dxs0, (size_t)c->sa.ns * NX, 0, v + NX, c->sa.ns * NX, b0, nb, stride);
            }
            if (len != NX) return fail("constraints_set lbx/ubx at stage 0: expected 8 values (x0)");
            if (c->sn) {
                if (!c->have_offs) return fail("constraints_set lbx/ubx at stage 0: an SNMPC capsule takes 8 (n_samples+1) values, or 8 after tum_ocp_snmpc_set_offsets");
                c->fanout = true;
            }
            // (set twice per control step, lbx and ubx: NMPC_class.py:243-246)
            if (b0 == 0 && nb == c->batch && small_inputs(c) && (stride == 0 || stride >= len)) return shadow_write(c, -1, v, len, stride);
            return put(c, CH_X0, c->dx0, NX, 0, v, len, b0, nb, stride);
        }
        if (len != 1) return fail("constraints_set lbx/ubx: expected 1 value (steering angle)");
        return put(c, CH_BOUNDS, c->dbnd, 6 * NB, (size_t)(f == "lbx" ? 2 : 3) * NB + stage, v, 1, b0, nb, stride);
    }
    if (f == "lbu" || f == "ubu") {
        if (stage >= N) return fail("constraints_set lbu/ubu: stage out of range");
        if (len != 1) return fail("constraints_set lbu/ubu: expected 1 value (steering rate)");
        return put(c, CH_BOUNDS, c->dbnd, 6 * NB, (size_t)(f == "lbu" ? 0 : 1) * NB + stage, v, 1, b0, nb, stride);
    }
    if (f == "lh" || f == "uh") {
        if (stage == 0) return fail("constraints_set lh/uh: no nonlinear constraint at stage 0 (nh_0 = 0)");
        if (len != 1) return fail("constraints_set lh/uh: expected 1 value");
        return put(c, CH_BOUNDS, c->dbnd, 6 * NB, (size_t)(f == "lh" ? 4 : 5) * NB + stage, v, 1, b0, nb, stride);
    }
    return fail("constraints_set: unknown field '" + f + "'");
}

extern "C" int tum_ocp_cost_set(tum_ocp *c, int stage, const char *field, const double *v, int len, int b0, int nb, int stride)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !v) return fail("null argument");
    const int N = c->N;
    const std::string f(field);
    if ((stage < 0 || stage > N) && !(stage == TUM_ALL_STAGES && f == "W")) return fail("cost_set: stage out of range");
    if (f == "W") {
        // per stage, like acados (NMPC_class.py:294-296 sets every stage in a loop); stage == TUM_ALL_STAGES: one 6 x 6 W for all
        // the stages 0..N-1 in one call
        const bool all = stage == TUM_ALL_STAGES;
        const int ny = (all || stage < N) ? TUM_NY : TUM_NYE;
        if (len != ny * ny) return fail("cost_set W: mismatching dimension");
        const int cnt = stride == 0 ? 1 : nb;
        const int rep = all ? N : 1;
        std::vector<double> diag((size_t)cnt * rep * ny);
        bool offdiag = false;
        for (int i = 0; i < cnt; i++) {
            const double *Wm = v + (size_t)i * stride;
            for (int r = 0; r < ny; r++)
                for (int q = 0; q < ny; q++) {
                    if (r == q) { for (int k = 0; k < rep; k++) diag[((size_t)i * rep + k) * ny + r] = Wm[r * ny + r]; }
                    else if (Wm[q * ny + r] != 0.0) offdiag = true;
                }
        }
        // A W with off-diagonal entries (acados takes any matrix, NMPC_class.py:290-296; the reference installs diagonal ones): from the first such
        // call on the capsule keeps a full symmetric 6 x 6 per stage (its symmetric part: the cost only sees that) beside the diagonal, and the
        // pipeline condenses with the full-W instantiation of the six-wavefront condensing kernel. Nominal / R2 OCP through the pipeline only.
        if (offdiag && !c->dWf) {
            if (c->N > 48) return fail("cost_set W: horizons beyond 48 take a diagonal W (the full-W condensing kernel's row store does not fit there)");
            if (c->sn) return fail("cost_set W: the coupled SNMPC OCP takes a diagonal W (its cost rows come from the prologue kernel)");
            DevGuard guard(c->d.device); GUARD_OK(guard);
            HIPCHK(hipStreamSynchronize(c->stream));
            if (dalloc(&c->dWf, (size_t)c->batch * (N + 1) * 36) != hipSuccess) return fail("cost_set W: device allocation failed");
            const size_t n = (size_t)c->batch * (N + 1);
            hipLaunchKernelGGL(wf_from_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->dW, c->dWf, (long long)n);
            HIPCHK(hipGetLastError());
            c->ka.Wf = c->dWf; invalidate(c, CH_CAPTURED);
        }
        if (c->dWf) {
            std::vector<double> full((size_t)cnt * rep * 36, 0.0);
            for (int i = 0; i < cnt; i++) {
                const double *Wm = v + (size_t)i * stride;
                for (int k = 0; k < rep; k++)
                    for (int r = 0; r < ny; r++)
                        for (int q = 0; q < ny; q++) full[((size_t)i * rep + k) * 36 + r * 6 + q] = 0.5 * (Wm[q * ny + r] + Wm[r * ny + q]);
            }
            if (put(c, CH_W, c->dWf, (size_t)(N + 1) * 36, all ? 0 : (size_t)stage * 36, full.data(), rep * 36, b0, nb, stride == 0 ? 0 : rep * 36)) return 1;
        }
        return put(c, CH_W, c->dW, (size_t)(N + 1) * 6, all ? 0 : (size_t)stage * 6, diag.data(), rep * ny, b0, nb, stride == 0 ? 0 : rep * ny);
    }
    int which = -1;
    if (f == "zl") which = 0; else if (f == "zu") which = 1; else if (f == "Zl") which = 2; else if (f == "Zu") which = 3;
    if (which < 0) return fail("cost_set: unknown field '" + f + "'");
    // penalty classes: 0 = stage 0 [sbu], 1 = stages 1..N-1 [sbu,sbx,sh], 2 = stage N [sbx,sh]
    const int cls = (stage == 0) ? 0 : (stage < N ? 1 : 2);
    const int want = (cls == 0) ? 1 : (cls == 1 ? 3 : 2);
    if (len != want) return fail("cost_set " + f + ": mismatching dimension for this stage");
    const int slot0 = (cls == 2) ? 1 : 0;
    for (int j = 0; j < want; j++) {
        const int slot = slot0 + j;
        // element (cls, slot, which) of pen[b][3][3][4]; one strided put per slot
        const int cnt = stride == 0 ? 1 : nb;
        std::vector<double> col(cnt);
        for (int i = 0; i < cnt; i++) col[i] = v[(size_t)i * stride + j];
        if (put(c, CH_BOUNDS, c->dpen, 36, (size_t)(cls * 3 + slot) * 4 + which, col.data(), 1, b0, nb, stride == 0 ? 0 : 1)) return 1;
    }
    return 0;
}

// MFMA tiles of condensed variables this capsule's pipeline runs with: five (N <= 40), six (41..48), seven (49..56).
// (TUM_FORCE_TILES: development aid -- a larger instantiation at a horizon a smaller one covers: the padding variables must not change the answer.)
static int tiles_of(const tum_ocp *c)
{
    const int force = env().force_tiles;
    const int need = c->N > 48 ? 7 : (c->N > NMAX ? 6 : 5);
    return (force > need && force <= 7 && !c->sn) ? force : need;
}
// the one dispatch on it: f(std::integral_constant<int, NT>) with the capsule's tile count; sizes and offsets are PD<NT>'s
template <typename F>
static auto with_tiles(const tum_ocp *c, F &&f)
{
    const int nt = tiles_of(c);
    if (nt == 7) return f(std::integral_constant<int, 7>());
    if (nt == 6) return f(std::integral_constant<int, 6>());
    return f(std::integral_constant<int, 5>());
}
// what the kernels of the pipeline are given
static PArgs pargs(const tum_ocp *c)
{
    PArgs pa;
    pa.ka = c->ka; pa.rec = c->drec; pa.hws = c->dhws; pa.cws = c->dcws; pa.vec = c->dvec;
    return pa;
}
// workspaces of the kernel variants, allocated when a variant is first used
static int ensure_workspace(tum_ocp *c)
{
    if (!c->pipe) return 0;
    return with_tiles(c, [&](auto ntc) {          // horizons beyond 40: six MFMA tiles (PD<6>), beyond 48: seven (PD<7>)
        using D = PD<decltype(ntc)::value>;
        const size_t B = c->batch;
        if (!c->dhws && dalloc(&c->dhws, B * D::NTT * 256) != hipSuccess) return fail("workspace allocation failed (H tiles)");
        if (!c->drec && (dalloc(&c->drec, B * (size_t)(c->N + 1) * PREC) != hipSuccess || dalloc(&c->dcws, B * D::NCH * 64) != hipSuccess ||
                         dalloc(&c->dvec, B * D::PVEC) != hipSuccess)) return fail("workspace allocation failed (pipeline)");
        return 0;
    });
}

// "fused": one kernel per solve; "pipeline": linearise / condense / interior point / expand as four kernels, each at its own
// occupancy, handing over through the L2-resident workspace. Since the pipeline's interior point kernel has the factorisation
// without LDS round trips it is the faster one at every batch size (device time per solve 0.334 against 0.346 ms at one
// instance, 1.51 against 1.71 ms at 4096; wall time of a solve() call likewise): "auto" (default) runs the pipeline; the fused
// kernel stays selectable and is what the condensed-QP debug dump runs. The coupled SNMPC OCP follows the same rule
// (prologue / epilogue around either).
extern "C" int tum_ocp_set_kernel(tum_ocp *c, const char *name)
{
    if (!c || !name) return fail("null argument");
    const std::string n(name);
    if (n == "time-ipm") { c->time_ipm = true; return 0; }            // (timing options, not kernels: the events around the interior point kernel on EVERY solve)
    if (n == "no-time-ipm") { c->time_ipm = false; return 0; }
    if (n == "auto") { c->kmode = KMode::AUTO; c->lin_cols = -1; c->cond_wide = -1; c->sim_fork = -1; }        // (the wide kernels of the latency path: the library decides by batch size again)
    else if (n == "pipeline") c->kmode = KMode::PIPELINE;
    // the prologue of the coupled SNMPC OCP: the matrix-core kernel (default where n_samples <= 10) or the column-slot / pass variants
    // the linearisation: one lane per (instance, stage) or eight (default: eight while the batch is one round of wavefronts)
    else if (n == "loop-serial") c->sim_fork = 0;
    else if (n == "loop-fork") c->sim_fork = 1;
    else if (n == "cond-one-wavefront") c->cond_wide = 0;
    else if (n == "cond-six-wavefronts") c->cond_wide = 1;
    else if (n == "lin-lane-per-stage") c->lin_cols = 0;
    else if (n == "lin-eight-lanes") c->lin_cols = 1;
    else if (n == "prologue-passes" || n == "prologue-mfma") {
        if (c->sn) {
            const int want = (n == "prologue-passes") ? 0 : 2;
            const size_t lds = sizeof(double) * sn_prologue_lds(c->sa.uph, c->sa.ns, want, sn_nsb(c->sa.ns, c->sa.L));
            if (lds > 128 * 1024) return fail("set_kernel: n_samples x uph too large for that prologue kernel's LDS");
        }
        c->sn_prologue = (n == "prologue-passes") ? 0 : 2;
    }
#ifdef TUM_DEV_KERNELS
    else if (n == "fused") c->kmode = KMode::FUSED;
    else if (n == "pipeline4") c->kmode = KMode::PIPELINE4;
#else
    else if (n == "fused" || n == "pipeline4")
        return fail("set_kernel: kernel '" + n + "' exists in the development build only (libtumnmpc_dev.so); this library is the pipeline");
#endif
    else return fail("set_kernel: unknown kernel '" + n + "' (auto | pipeline | lin-lane-per-stage | lin-eight-lanes | cond-one-wavefront | cond-six-wavefronts | loop-fork | loop-serial | prologue-mfma | prologue-passes; development build: fused | pipeline4)");
    invalidate(c, CH_VARIANT | CH_CAPTURED);
    return 0;
}

// which kernel variant this solve runs, and its workspace (allocated on first use; never inside a stream capture)
static int resolve_kernel(tum_ocp *c)
{
#ifdef TUM_DEV_KERNELS
    c->pipe = !(c->ka.flags & KF_DEBUG) && c->kmode != KMode::FUSED;
    if (c->dWf && c->kmode == KMode::FUSED) return fail("solve: a full W (cost_set 'W' with off-diagonal entries) runs on the pipeline only, not on the development kernel 'fused'");
    if (c->ka.warm_mu > 0.0 && (c->kmode == KMode::FUSED || c->kmode == KMode::PIPELINE4))
        return fail("solve: the development kernels 'fused' / 'pipeline4' always cold-start the interior point method: create the capsule with qp_warm_start = 0");
    if (c->N > NMAX) {      // the fused kernel covers N <= 40; longer horizons exist as a pipeline instantiation only
        if (c->ka.flags & KF_DEBUG) return fail("debug_dump: the condensed-QP dump is built for N <= 40");
        if (c->kmode == KMode::FUSED) return fail("solve: kernel 'fused' is built for N <= 40 (use 'auto' or 'pipeline')");
        c->pipe = true;
    }
#else
    c->pipe = true;
#endif
    return ensure_workspace(c);
}

// the prologue of the coupled SNMPC OCP: column state of its recursions in registers (instantiation by the number of passes of the
// last stage) or, for short propagation horizons and beyond the largest instantiation, in LDS
static void sn_launch_prologue(tum_ocp *c)
{
    if (sn_nsb(c->sa.ns, c->sa.L) != SN_B16) {      // more than 16 samples or PCE terms: the column-slot kernel, column state in LDS, 32-wide bounds
        const size_t lds32 = sizeof(double) * sn_prologue_lds_doubles(c->sa.uph, c->sa.ns, 0, SN_NSMAX);
        hipLaunchKernelGGL((snmpc_prologue_kernel<0, SN_NSMAX>), dim3(c->batch), dim3(64), lds32, c->stream, c->sa);
        return;
    }
    const int kind = sn_prologue_kind(c->sa.uph, c->sa.ns, c->sn_prologue);
    if (kind == 2) {      // the column recursions on the matrix cores, the samples split over the two wavefronts of a workgroup
        const size_t lds = sizeof(double) * sn_mfma_lds_doubles(c->sa.uph, c->sa.ns);
        // (one wavefront with all ten samples instead: 178 spilled registers, 3.6 against 2.55 ms per solve at UPH = Tp)
        hipLaunchKernelGGL((snmpc_prologue_mfma_kernel<SN_MFMA_NSW, 2>), dim3(c->batch), dim3(128), lds, c->stream, c->sa);
        return;
    }
    const int v = sn_prologue_variant(c->sa.uph, c->sa.ns);
    const size_t lds = sizeof(double) * sn_prologue_lds_doubles(c->sa.uph, c->sa.ns, v);
    const dim3 g(c->batch), blk(64);
    switch (v) {
    case 6: hipLaunchKernelGGL(snmpc_prologue_kernel<6>, g, blk, lds, c->stream, c->sa); break;
    case 9: hipLaunchKernelGGL(snmpc_prologue_kernel<9>, g, blk, lds, c->stream, c->sa); break;
    case 13: hipLaunchKernelGGL(snmpc_prologue_kernel<13>, g, blk, lds, c->stream, c->sa); break;
    case 17: hipLaunchKernelGGL(snmpc_prologue_kernel<17>, g, blk, lds, c->stream, c->sa); break;
    default: hipLaunchKernelGGL(snmpc_prologue_kernel<0>, g, blk, lds, c->stream, c->sa); break;
    }
}

// the facts plan_pipeline decides on (pipe_plan.hpp), as this capsule holds them now
static PlanIn plan_in(const tum_ocp *c, Part part)
{
    PlanIn in;
    in.N = c->N; in.tiles = tiles_of(c); in.batch = c->batch; in.sn = c->sn; in.uph = c->sa.uph;
    in.full_w = c->dWf != nullptr; in.store_qp_in = c->d.store_qp_in != 0; in.debug = (c->ka.flags & KF_DEBUG) != 0; in.prof = (c->ka.flags & KF_PROF) != 0;
    in.kmode = c->kmode; in.lin_cols = c->lin_cols; in.cond_wide = c->cond_wide; in.sim_fork = c->sim_fork; in.env = env().plan;
    in.iter_uniform = c->iter_uniform; in.lin_dedup = c->lin_dedup != 0; in.uniform_records = c->uniform_records != 0; in.capturing = c->capturing;
    in.nlp_type = c->nlp_type; in.ran_ahead = c->lin_ahead; in.part = part;
    in.uniform_powers = c->uniform_powers != 0;
    return in;
}
// the device closed loop: the linearisation of a step beside its planner (plan_lin_ahead, pipe_plan.hpp)
static bool lin_ahead_ok(const tum_ocp *c)
{
    PlanIn in = plan_in(c, Part::WHOLE);
    in.ran_ahead = false;
    return c->pipe && plan_lin_ahead(in);
}
static void launch_lin_ahead(tum_ocp *c, hipStream_t st)
{
    PArgs pa = pargs(c);
    pa.ka.flags |= KF_LIN_AHEAD;
    const long long items = (long long)c->batch * (c->N + 1);
    hipLaunchKernelGGL(lin_cols_kernel<false>, dim3((unsigned)((items + LC_ITEMS - 1) / LC_ITEMS)), dim3(64), 0, st, pa);
    c->lin_ahead = true;          // the next launch_pipeline skips its linearisation and tells the condensing kernel (consumed there)
}

// One part of a solve on the pipeline kernels: plan_pipeline (pipe_plan.hpp) says which kernel every stage runs, this launches them.
// ipm_events: the events around the interior point kernel (get_stats "time_ipm") are recorded
static int launch_pipeline(tum_ocp *c, bool ipm_events, Part part)
{
    const PlanIn in = plan_in(c, part);
    const PipePlan plan = plan_pipeline(in);
    PArgs pa = pargs(c);
    const long long items = (long long)c->batch * (c->N + 1);
    const dim3 g_cols((unsigned)((items + LC_ITEMS - 1) / LC_ITEMS)), g_lane((unsigned)((items + 63) / 64)), g_ocp(c->batch), wave(64);
    if (part != Part::FEEDBACK) c->lin_ahead = false;
    if (plan.cond != Cond::NONE) { c->qp_handed = true; c->dv_handed = false; c->shift_counted = plan.cond == Cond::ONE_WAVE_UNIFORM && plan.cond_powers; }
    if (plan.ipm != Ipm::NONE) c->dv_handed = plan.ipm != Ipm::FUSED_TAIL;
    if (plan.lin_ahead_flag) pa.ka.flags |= KF_LIN_AHEAD;          // (launch_lin_ahead ran it on another stream; the caller has joined that stream)
    if (plan.lin == Lin::SN_LANE || plan.lin == Lin::SN_COLS) {   // coupled SNMPC OCP: sample fan-out and prologue first, the QP solution goes to the epilogue through the workspace
        if (c->fanout && sn_fanout(c)) return 1;
        sn_launch_lin(c);
        sn_launch_prologue(c);
    }
    switch (plan.lin) {
    case Lin::NONE: break;
    case Lin::LANE: hipLaunchKernelGGL(lin_kernel<false>, g_lane, wave, 0, c->stream, pa); break;
    case Lin::COLS: hipLaunchKernelGGL(lin_cols_kernel<false>, g_cols, wave, 0, c->stream, pa); break;
    case Lin::SN_LANE: hipLaunchKernelGGL(lin_kernel<true>, g_lane, wave, 0, c->stream, pa); break;
    case Lin::SN_COLS: hipLaunchKernelGGL(lin_cols_kernel<true>, g_cols, wave, 0, c->stream, pa); break;
    case Lin::UNIFORM_FILL: case Lin::UNIFORM:
        // a stage-uniform iterate (cold_start(), reset()): the Runge-Kutta pass once per instance, then the records of every stage
        // (UNIFORM: nobody reads them, cond_uniform_kernel and expand_uniform_kernel take lin1 and the reference)
        hipLaunchKernelGGL(lin_uniform_kernel, dim3((unsigned)((c->batch + 63) / 64)), wave, 0, c->stream, pa, c->dlin1);
        if (plan.lin == Lin::UNIFORM_FILL) hipLaunchKernelGGL(lin_fill_kernel, dim3((unsigned)((c->batch + LF_WAVES - 1) / LF_WAVES)), dim3(64 * LF_WAVES), 0, c->stream, pa, c->dlin1, c->hlin_bad);
        c->n_lin_uniform++;
        if (plan.lin == Lin::UNIFORM) c->n_records_skipped++;
        break;
    }
    with_tiles(c, [&](auto ntc) {
        constexpr int NTv = decltype(ntc)::value;
        switch (plan.cond) {
        case Cond::NONE: break;
        case Cond::ONE_WAVE: hipLaunchKernelGGL((cond_kernel<NTv, false>), g_ocp, wave, 0, c->stream, pa); break;
        case Cond::ONE_WAVE_UNIFORM:
            if (plan.cond_powers) hipLaunchKernelGGL((cond_uniform_kernel<NTv>), g_ocp, wave, 0, c->stream, pa, c->dlin1, c->uniform_shift, c->dshift);
            else hipLaunchKernelGGL((cond_uniform_columns_kernel<NTv>), g_ocp, wave, 0, c->stream, pa, c->dlin1);
            break;
        case Cond::SN_REGISTER: hipLaunchKernelGGL((cond_kernel<NTv, true, true>), g_ocp, wave, 0, c->stream, pa); break;
        case Cond::SN_LDS: hipLaunchKernelGGL((cond_kernel<NTv, true, false>), g_ocp, wave, 0, c->stream, pa); break;
        case Cond::WIDE: case Cond::WIDE_FULLW: case Cond::SN_WIDE:
            if constexpr (NTv != 7) {      // (never planned at seven tiles: the instantiation does not exist)
                const dim3 blk(64 * cw_waves<NTv>());
                if (plan.cond == Cond::SN_WIDE) hipLaunchKernelGGL((cond_wide_kernel<NTv, true>), g_ocp, blk, 0, c->stream, pa);
                else if (plan.cond == Cond::WIDE_FULLW) hipLaunchKernelGGL((cond_wide_kernel<NTv, false, true>), g_ocp, blk, 0, c->stream, pa);
                else hipLaunchKernelGGL((cond_wide_kernel<NTv, false>), g_ocp, blk, 0, c->stream, pa);
            }
            break;
        }
        if (plan.ipm == Ipm::NONE) return;
        const int ipm_lds = env().ipm_lds > PD<NTv>::I_LDS_BYTES ? env().ipm_lds : PD<NTv>::I_LDS_BYTES;
        if (ipm_events) (void)hipEventRecord(c->evi0, c->stream);
        switch (plan.ipm) {
        case Ipm::NONE: break;
        case Ipm::PLAIN: hipLaunchKernelGGL((ipm_kernel<false, NTv>), g_ocp, wave, ipm_lds, c->stream, pa); break;
        case Ipm::FUSED_TAIL:      // the nominal OCP: the expansion runs as the tail of the interior point kernel
            if constexpr (NTv != 7) hipLaunchKernelGGL((ipm_kernel<false, NTv, true>), g_ocp, wave, ipm_lds, c->stream, pa);
            break;
        case Ipm::INSTRUMENTED:      // (five tiles only, as the four-wavefront kernel)
            if constexpr (NTv == 5) hipLaunchKernelGGL((ipm_kernel<true, 5>), g_ocp, wave, ipm_lds, c->stream, pa);
            break;
        case Ipm::FOUR_WAVE:
#ifdef TUM_DEV_KERNELS
            if (in.prof) hipLaunchKernelGGL((ipm4_kernel<true>), g_ocp, dim3(256), I4::BYTES, c->stream, pa);
            else hipLaunchKernelGGL((ipm4_kernel<false>), g_ocp, dim3(256), I4::BYTES, c->stream, pa);
#endif
            break;
        }
        if (ipm_events) (void)hipEventRecord(c->evi1, c->stream);
        switch (plan.expand) {
        case Expand::NONE: break;
        case Expand::RECORDS: hipLaunchKernelGGL((expand_kernel<NTv, false>), g_ocp, wave, 0, c->stream, pa); break;
        case Expand::UNIFORM: hipLaunchKernelGGL((expand_uniform_kernel<NTv>), g_ocp, wave, 0, c->stream, pa, c->dlin1, c->hlin_bad); break;
        case Expand::SN_RECORDS: {
            // the epilogue steps the sample copies AND the nominal copy of the stages 1..uph (their PCE mean); the expansion
            // kernel behind it takes the nominal recursion from stage uph to the end of the horizon and evaluates the cost
            SnArgs sa = c->sa;
            sa.dv = c->dvec + PD<NTv>::PV_DV; sa.dv_stride = PD<NTv>::PVEC;
            sa.Xn = c->dX; sa.dxu = c->dvec + PD<NTv>::PV_SC + 8;
            if (sn_nsb(sa.ns, sa.L) != SN_B16) hipLaunchKernelGGL((snmpc_epilogue_kernel<SN_NSMAX>), g_ocp, wave, 0, c->stream, sa);
            else hipLaunchKernelGGL((snmpc_epilogue_kernel<>), g_ocp, wave, 0, c->stream, sa);
            c->xs_lazy = true;
            hipLaunchKernelGGL((expand_kernel<NTv, true>), g_ocp, wave, 0, c->stream, pa);
            break;
        }
        }
    });
    return 0;
}

// ---- split real-time iteration (tum_ocp_options_set "rti_phase")
// what the split is not built for: the reason, or null
static const char *rti_unsupported(const tum_ocp *c)
{
    if (c->sn) return "the split real-time iteration is not available for the coupled SNMPC OCP (its prologue and epilogue kernels read x0 themselves): rti_phase 0 only";
    if (c->r2) return "the split real-time iteration is not available for a capsule with the R2NMPC tightening attached (the back-off follows every whole solve): rti_phase 0 only";
    if (c->dWf) return "the split real-time iteration is not available for a capsule with a full W (cost_set 'W' with off-diagonal entries: x0 then enters the input rows of the gradient as well): rti_phase 0 only";
    if (c->nlp_type) return "the split real-time iteration is one SQP-RTI step; this capsule is in SQP mode (nlp_solver_type 1)";
    if (c->kmode == KMode::FUSED || c->kmode == KMode::PIPELINE4) return "the split real-time iteration runs on the pipeline only, not on the development kernels 'fused' / 'pipeline4'";
    if (c->ka.flags & (KF_DEBUG | KF_PROF)) return "the split real-time iteration does not run with the debug dump or the phase timers";
    return nullptr;
}
// may a solve in the capsule's phase start: nothing is touched when it may not
static int rti_gate(tum_ocp *c)
{
    if (!c->rti_phase) return 0;
    if (const char *why = rti_unsupported(c)) return fail(std::string("solve: ") + why);
    if (c->rti_phase == 2 && c->prep == 0)
        return fail("solve: rti_phase 2 (feedback) without a preparation: solve with rti_phase 1 first (every feedback consumes its preparation)");
    if (c->rti_phase == 2 && c->prep == 2)
        return fail("solve: rti_phase 2 (feedback): the preparation is stale -- the iterate, the reference, W, the kernel choice or a bound array changed "
                    "behind it (between the phases: x0, the bounds of the stages >= 1 and the slack penalties only); prepare again");
    return 0;
}
static void launch_rti_feedback(tum_ocp *c)
{
    with_tiles(c, [&](auto ntc) { hipLaunchKernelGGL(rti_feedback_kernel<decltype(ntc)::value>, dim3(c->batch), dim3(64), 0, c->stream, pargs(c), c->dx0prep); });
}
// ---- what every solve has in common, whichever way its kernels get onto the stream
enum SolveKind { SOLVE_RTI, SOLVE_SQP, SOLVE_REPLAY };          // launch(), launch_sqp(), a solve inside a replayed chunk of tum_sim_run
// the opening: the results of the last solve are on their way out, pending setters go up, the clock starts
static int solve_begin(tum_ocp *c, bool events)
{
    invalidate(c, CH_RESULTS);
    if (flush_inputs(c)) return 1;          // setters still in the pinned shadow (small capsules)
    if (events) HIPCHK(hipEventRecord(c->ev0, c->stream));
    // longest-first schedule from the previous solve's iteration counts (only matters when the batch is more than one
    // round of resident wavefronts)
    c->ka.order = (c->lpt && c->order_valid && c->batch > 1024) ? c->dorder : nullptr;
    return 0;
}
// a solve of this kind has been enqueued. A replayed one was enqueued by the graph: its kernels (the schedule's among them) are in
// the chunk, nothing is launched here, and nothing was timed -- what the last timed solve left behind stays
static int solve_done(tum_ocp *c, SolveKind kind, bool ipm_timed)
{
    if (c->lpt && c->batch > 1024) {
        if (kind != SOLVE_REPLAY) {
            hipLaunchKernelGGL(lpt_order_kernel, dim3(1), dim3(64), 0, c->stream, c->dqpiter, c->dorder, c->batch);
            HIPCHK(hipGetLastError());
        }
        c->order_valid = true;
    }
    c->solved = true; c->solved_pipe = c->pipe; c->solved_sqp = kind == SOLVE_SQP; c->solved_merit = false; c->cold = false;
    invalidate(c, CH_ITERATE);          // (whichever kernel variant ran: the solve wrote the new iterate)
    c->prep = 0; c->prep_timed = false;          // (a feedback consumes its preparation; a one-call solve discards a pending one)
    if (kind == SOLVE_REPLAY) { if (c->sn) c->xs_lazy = true; return 0; }          // (the epilogue kernel of the chunk, as launch_pipeline records it)
    c->ipm_timed = ipm_timed;
    c->ts_slot = -1;          // (tum_ocp_step_async sets it behind this call)
    return 0;
}

// PREPARATION (rti_phase 1): pending inputs up, part 1 of the pipeline as a one-call solve of this capsule would run it, and the x0 it
// condensed at. Iterate, results, multipliers, slacks and the getters' cache stay as they are.
static int launch_prepare(tum_ocp *c)
{
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (rti_gate(c)) return 1;
    if (resolve_kernel(c)) return 1;
    if (!c->dx0prep && dalloc(&c->dx0prep, (size_t)c->batch * NX) != hipSuccess) return fail("solve: device allocation failed (rti_phase 1)");
    c->prep = 0;
    if (flush_inputs(c)) return 1;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (launch_pipeline(c, false, Part::PREPARE)) return 1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->dx0prep, c->dx0, sizeof(double) * (size_t)c->batch * NX, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    c->prep = 1; c->prep_timed = true;
    c->ts_slot = -1;          // (get_stats "time_tot": the events of the preparation)
    return 0;
}

static int launch(tum_ocp *c, bool events = true)
{
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (rti_gate(c)) return 1;
    const bool feedback = c->rti_phase == 2;
    if (resolve_kernel(c)) return 1;
    if (solve_begin(c, events)) return 1;
    const bool ipm_events = (events && !c->skip_ipm_events) || c->time_ipm;
    // the instrumented instantiation carries the phase timers (flag 4) and the debug dump (flag 2)
    if (c->sn && sn_apply_p(c)) return 1;
#ifdef TUM_DEV_KERNELS
    const bool prof = (c->ka.flags & (KF_DEBUG | KF_PROF)) != 0;
    auto fused = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(c->batch), dim3(64), LDS_BYTES, c->stream, c->ka); };
    if (c->sn && !c->pipe && sn_nsb(c->sa.ns, c->sa.L) != SN_B16)
        return fail("solve: kernel 'fused' takes at most 16 samples / PCE terms (use 'auto' or 'pipeline')");
    if (c->sn && !c->pipe && c->sa.uph > SN_UPHMAX_FUSED)
        return fail("solve: kernel 'fused' reads the sample columns of one wavefront: uncertainty propagation horizon <= 31 (use 'auto' or 'pipeline')");
    if (!c->pipe) {
        if (c->sn) {
            if (c->fanout && sn_fanout(c)) return 1;
            sn_launch_lin(c);
            sn_launch_prologue(c);
            if (prof) fused(nmpc_rti_kernel<true, true>); else fused(nmpc_rti_kernel<false, true>);
            hipLaunchKernelGGL((snmpc_epilogue_kernel<>), dim3(c->batch), dim3(64), 0, c->stream, c->sa); c->xs_lazy = true;
        }
        else { if (prof) fused(nmpc_rti_kernel<true>); else fused(nmpc_rti_kernel<false>); }
        HIPCHK(hipMemsetAsync(c->dqplam, 0, sizeof(double) * (size_t)c->batch * (6 * (size_t)c->N + 2), c->stream));      // (the fused kernel leaves no multipliers behind)
    } else
#endif
    {
        if (feedback) launch_rti_feedback(c);
        if (launch_pipeline(c, ipm_events, feedback ? Part::FEEDBACK : Part::WHOLE)) return 1;
    }
    HIPCHK(hipGetLastError());
    if (c->r2) {   // constraint tightening for the NEXT solve from this one's linearisation (skipped per instance on failure)
        hipLaunchKernelGGL(r2_backoff_kernel, dim3((c->batch + 3) / 4), dim3(256), 0, c->stream, c->dqpin, c->dX, c->dbnd, c->ka.mp,
                           c->dr2S, c->dr2B, c->N, c->r2_uph, c->batch, c->r2_dmin, c->r2_dmax, c->r2_uh, (double *)nullptr, c->dstatus,
                           c->pipe ? c->drec : (const double *)nullptr, PREC);
        HIPCHK(hipGetLastError());
    }
    if (events) HIPCHK(hipEventRecord(c->ev1, c->stream));
    return solve_done(c, SOLVE_RTI, ipm_events);
}

// ---- full SQP solves (nlp_solver_type SQP)
// acados' option fields (acados_ocp_SNMPC.json: nlp_solver_type, nlp_solver_max_iter, nlp_solver_tol_*, nlp_solver_step_length) and its
// globalization: FIXED_STEP (the default) or MERIT_BACKTRACKING with alpha_min, alpha_reduction and -- not an acados name: the weight of the
// shooting defects in the merit function, where acados takes the multipliers of the dynamics that condensing does not keep -- merit_weight_eq
extern "C" int tum_ocp_options_set(tum_ocp *c, const char *field, double value)
{
    if (!c || !field) return fail("null argument");
    const std::string f(field);
    if (!(value == value)) return fail("options_set " + f + ": NaN");
    if (f == "nlp_solver_type") {
        if (value != 0.0 && value != 1.0) return fail("options_set nlp_solver_type: 0 (SQP_RTI) or 1 (SQP)");
        if (value == 1.0) {
            if (c->rti_phase) return fail("options_set nlp_solver_type: SQP is not available while the capsule splits the real-time iteration (rti_phase 1 / 2 is one SQP-RTI step): set rti_phase 0 first");
            if (c->r2) return fail("options_set nlp_solver_type: SQP is not available for a capsule with the R2NMPC tightening attached (SQP_RTI only, as Reduced_Robustified_NMPC_class.py requires)");
            if (c->sn) return fail("options_set nlp_solver_type: SQP is not available for the coupled SNMPC OCP (SQP_RTI only)");
        }
        c->nlp_type = (int)value;
        return 0;
    }
    if (f == "nlp_solver_max_iter") {
        if (!(value >= 1.0 && value <= 10000.0) || value != std::floor(value)) return fail("options_set nlp_solver_max_iter: an integer in 1..10000");
        c->nlp_max_iter = (int)value;
        return 0;
    }
    const char *tols[4] = {"nlp_solver_tol_stat", "nlp_solver_tol_eq", "nlp_solver_tol_ineq", "nlp_solver_tol_comp"};
    for (int i = 0; i < 4; i++)
        if (f == tols[i]) {
            if (!(value >= 0.0) || std::isinf(value)) return fail("options_set " + f + ": a finite value >= 0");
            c->nlp_tol[i] = value;
            return 0;
        }
    if (f == "nlp_solver_step_length") {
        if (!(value > 0.0 && value <= 1.0)) return fail("options_set nlp_solver_step_length: in (0, 1]");
        c->nlp_alpha = value;
        return 0;
    }
    if (f == "globalization") {      // read by an SQP solve only; what does not go together with it is refused there
        if (value != 0.0 && value != 1.0) return fail("options_set globalization: 0 (FIXED_STEP) or 1 (MERIT_BACKTRACKING)");
        c->globalization = (int)value;
        return 0;
    }
    if (f == "alpha_min") {
        if (!(value > 0.0 && value <= 1.0)) return fail("options_set alpha_min: in (0, 1]");
        c->merit_alpha_min = value;
        return 0;
    }
    if (f == "alpha_reduction") {
        if (!(value > 0.0 && value < 1.0)) return fail("options_set alpha_reduction: in (0, 1)");
        c->merit_alpha_reduction = value;
        return 0;
    }
    if (f == "merit_weight_eq") {
        if (!(value >= 0.0) || std::isinf(value)) return fail("options_set merit_weight_eq: a finite value >= 0");
        c->merit_weight_eq = value;
        return 0;
    }
    if (f == "rti_phase") {      // acados: 0 PREPARATION_AND_FEEDBACK, 1 PREPARATION, 2 FEEDBACK
        if (value != 0.0 && value != 1.0 && value != 2.0) return fail("options_set rti_phase: 0 (preparation and feedback), 1 (preparation) or 2 (feedback)");
        if (value != 0.0) { if (const char *why = rti_unsupported(c)) return fail(std::string("options_set rti_phase: ") + why); }
        c->rti_phase = (int)value;
        return 0;
    }
    if (f == "lin_dedup") {      // 1: a stage-uniform iterate is linearised once per instance (default); 0: lin_kernel always (A/B runs, tests)
        if (value != 0.0 && value != 1.0) return fail("options_set lin_dedup: 0 or 1");
        c->lin_dedup = (int)value;
        return 0;
    }
    if (f == "uniform_records") {      // 0: a stage-uniform iterate is condensed and expanded without stage records where nothing else reads them (default); 1: lin_fill_kernel always
        if (value != 0.0 && value != 1.0) return fail("options_set uniform_records: 0 or 1");
        c->uniform_records = (int)value;
        return 0;
    }
    if (f == "uniform_powers") {      // 1: the record-free condensing computes the sequences A^m B, g_s once per instance (default); 0: every lane carries its column (A/B runs, tests)
        if (value != 0.0 && value != 1.0) return fail("options_set uniform_powers: 0 or 1");
        c->uniform_powers = (int)value;
        return 0;
    }
    if (f == "uniform_shift") {      // 1: cond_uniform_kernel<5> takes the shift form where an instance's cost weights are the same at every stage (default); 0: never (A/B runs, tests)
        if (value != 0.0 && value != 1.0) return fail("options_set uniform_shift: 0 or 1");
        c->uniform_shift = (int)value;
        return 0;
    }
    return fail("options_set: unknown field '" + f + "' (lin_dedup | uniform_records | uniform_powers | uniform_shift | nlp_solver_type | nlp_solver_max_iter | nlp_solver_tol_stat | nlp_solver_tol_eq | "
                "nlp_solver_tol_ineq | nlp_solver_tol_comp | nlp_solver_step_length | rti_phase), of the SQP globalization (globalization | "
                "alpha_min | alpha_reduction | merit_weight_eq)");
}

// One full SQP solve: [lin, cond, residuals] then, while an instance is active and the cap is not reached, [snapshot, ipm, expand,
// commit, lin, cond, residuals]. The host reads the number of active instances of every residual pass (a 4-byte copy into pinned
// memory behind an event), one iteration behind the GPU; the kernels of the pipeline are the RTI's, launched as an SQP-RTI solve
// launches them. With globalization MERIT_BACKTRACKING sqp_merit_kernel stands between the expansion and the commit: all candidates
// of every instance in ONE launch (the host reads the active count an iteration late; a backtracking loop on the host would stall the
// stream), and the commit kernel accepts a step length for every instance from that table and moves the instance by it.

// number of candidates alpha_reduction^j >= alpha_min, j = 0 ..: 1 + floor(log alpha_min / log alpha_reduction) (9 with acados' defaults)
static int merit_candidates(const tum_ocp *c)
{
    const double k = std::floor(std::log(c->merit_alpha_min) / std::log(c->merit_alpha_reduction));
    return (k < 1e6) ? 1 + (int)k : 1000000;
}

static int launch_sqp(tum_ocp *c)
{
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (c->r2) return fail("solve: SQP is not available for a capsule with the R2NMPC tightening attached (nlp_solver_type SQP_RTI only)");
    if (c->sn) return fail("solve: SQP is not available for the coupled SNMPC OCP (nlp_solver_type SQP_RTI only)");
    if (c->ka.flags & (KF_DEBUG | KF_PROF)) return fail("solve: SQP does not run with the debug dump or the phase timers");
    if (resolve_kernel(c)) return 1;
    if (!c->pipe) return fail("solve: SQP runs on the pipeline only, not on the development kernel 'fused'");
#ifdef TUM_DEV_KERNELS
    if (c->kmode == KMode::PIPELINE4) return fail("solve: SQP runs on the pipeline only, not on the development kernel 'pipeline4'");
#endif
    const size_t B = c->batch; const int N = c->N;
    const bool merit = c->globalization == 1;
    const int K = merit ? merit_candidates(c) : 0;
    if (merit) {
        if (c->nlp_alpha != 1.0)
            return fail("solve: globalization MERIT_BACKTRACKING chooses every step length itself and does not go together with "
                        "nlp_solver_step_length != 1 (it is " + std::to_string(c->nlp_alpha) + "): set one of the two back");
        if (K > MERIT_KMAX)
            return fail("solve: globalization MERIT_BACKTRACKING: alpha_min " + std::to_string(c->merit_alpha_min) + " and alpha_reduction " +
                        std::to_string(c->merit_alpha_reduction) + " give " + std::to_string(K) + " candidate step lengths; at most " +
                        std::to_string(MERIT_KMAX) + " (1 + floor(log alpha_min / log alpha_reduction))");
    }
    const int snap_len = (N + 1) * NX + N * NU + (6 * N + 2) + 6 * N + 4;
    if (merit && !c->dmalpha) {
        if (dalloc(&c->dmalpha, B) != hipSuccess || dalloc(&c->dmmu, B) != hipSuccess || dalloc(&c->dmtable, B * (MERIT_KMAX + 1) * 3) != hipSuccess)
            return fail("solve: device allocation failed (SQP, MERIT_BACKTRACKING)");
    }
    if (merit && c->merit_hist_cap < c->nlp_max_iter) {
        (void)hipFree(c->dmhist); c->dmhist = nullptr; c->merit_hist_cap = 0;
        if (dalloc(&c->dmhist, B * (size_t)c->nlp_max_iter) != hipSuccess) return fail("solve: device allocation failed (SQP, MERIT_BACKTRACKING)");
        c->merit_hist_cap = c->nlp_max_iter;
    }
    if (!c->dnlpres) {
        if (dalloc(&c->dnlpres, B * 4) != hipSuccess || dalloc(&c->dsnap, B * snap_len) != hipSuccess || dalloc(&c->dsqpstate, B) != hipSuccess ||
            dalloc(&c->dsqpiter, B) != hipSuccess || dalloc(&c->dsnapi, B * 3) != hipSuccess) return fail("solve: device allocation failed (SQP)");
        HIPCHK(hipEventCreateWithFlags(&c->evpoll[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->evpoll[1], hipEventDisableTiming));
    }
    if (c->active_cap < c->nlp_max_iter + 1) {
        (void)hipFree(c->dactive); c->dactive = nullptr;
        if (c->hactive) { (void)hipHostFree(c->hactive); c->hactive = nullptr; }
        if (dalloc(&c->dactive, (size_t)c->nlp_max_iter + 1) != hipSuccess) return fail("solve: device allocation failed (SQP)");
        HIPCHK(hipHostMalloc((void **)&c->hactive, 2 * sizeof(unsigned), hipHostMallocDefault));
        c->active_cap = c->nlp_max_iter + 1;
    }
    if (solve_begin(c, true)) return 1;
    HIPCHK(hipMemsetAsync(c->dsqpstate, 0, sizeof(int) * B, c->stream));
    HIPCHK(hipMemsetAsync(c->dsqpiter, 0, sizeof(int) * B, c->stream));
    HIPCHK(hipMemsetAsync(c->dactive, 0, sizeof(unsigned) * (size_t)(c->nlp_max_iter + 1), c->stream));
    const bool cold = c->cold;
    if (cold) {
        // pass 0 of a cold-started solve: zero multipliers and slacks, whatever this capsule solved before -- and no QP statistics of an
        // earlier problem for an instance that converges before its first QP (its cost is evaluated by pass 0)
        HIPCHK(hipMemsetAsync(c->dqplam, 0, sizeof(double) * B * (6 * (size_t)N + 2), c->stream));
        HIPCHK(hipMemsetAsync(c->dslack, 0, sizeof(double) * B * 6 * (size_t)N, c->stream));
        HIPCHK(hipMemsetAsync(c->dres, 0, sizeof(double) * B * 3, c->stream));
        HIPCHK(hipMemsetAsync(c->dqpiter, 0, sizeof(int) * B, c->stream));
        HIPCHK(hipMemsetAsync(c->dqpstatus, 0, sizeof(int) * B, c->stream));
    }
    SqpArgs sq;
    sq.res_nlp = c->dnlpres; sq.state = c->dsqpstate; sq.sqp_iter = c->dsqpiter; sq.active = c->dactive;
    sq.snap = c->dsnap; sq.snapi = c->dsnapi; sq.snap_len = snap_len;
    sq.tol_stat = c->nlp_tol[0]; sq.tol_eq = c->nlp_tol[1]; sq.tol_ineq = c->nlp_tol[2]; sq.tol_comp = c->nlp_tol[3];
    sq.alpha = c->nlp_alpha;
    MeritArgs ma{};          // (ma.alpha null: FIXED_STEP)
    if (merit) {
        // every solve starts with mu_in = 0, an empty table and an empty history
        HIPCHK(hipMemsetAsync(c->dmmu, 0, sizeof(double) * B, c->stream));
        HIPCHK(hipMemsetAsync(c->dmtable, 0, sizeof(double) * B * (size_t)(K + 1) * 3, c->stream));
        HIPCHK(hipMemsetAsync(c->dmhist, 0, sizeof(double) * B * (size_t)c->nlp_max_iter, c->stream));
        ma.alpha = c->dmalpha; ma.mu_in = c->dmmu; ma.table = c->dmtable; ma.hist = c->dmhist;
        ma.K = K; ma.hist_len = c->nlp_max_iter; ma.mu_eq = c->merit_weight_eq;
        ma.cand[0] = 1.0;
        for (int j = 1; j < K; j++) ma.cand[j] = ma.cand[j - 1] * c->merit_alpha_reduction;          // (alpha_reduction^j as j products)
    }
    const PArgs pa = pargs(c);
    auto residuals = [&](int pass) {
        sq.pass = pass; sq.last = (pass == c->nlp_max_iter) ? 1 : 0;
        sq.cost = (c->nlp_alpha != 1.0 || merit || (pass == 0 && cold)) ? 1 : 0;
        if (launch_pipeline(c, false, Part::PREPARE)) return 1;
        with_tiles(c, [&](auto ntc) { hipLaunchKernelGGL(nlp_residual_kernel<decltype(ntc)::value>, dim3(c->batch), dim3(64), 0, c->stream, pa, sq); });
        HIPCHK(hipGetLastError());
        return 0;
    };
    // the count of residual pass p goes to the pinned word p & 1 behind event p & 1
    auto count_copy = [&](int p) {
        HIPCHK(hipMemcpyAsync(c->hactive + (p & 1), c->dactive + p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->evpoll[p & 1], c->stream));
        return 0;
    };
    if (residuals(0) || count_copy(0)) return 1;
    // The host reads the count of pass `it` while the GPU runs iteration `it`, which is enqueued in front of the read: the stream never
    // waits for the host. When the count says that no instance was active any more, that iteration was a ride-along of finished
    // instances only -- the commit kernel has put every one of them back -- and the solve ends behind it.
    for (int it = 0; it < c->nlp_max_iter; it++) {
        hipLaunchKernelGGL(sqp_snapshot_kernel, dim3(c->batch), dim3(256), 0, c->stream, c->ka, sq);
        if (launch_pipeline(c, c->time_ipm, Part::FEEDBACK)) return 1;
        invalidate(c, CH_ITERATE);          // (the expansion wrote a new iterate: the residual pass below linearises the general way)
        if (merit) hipLaunchKernelGGL(sqp_merit_kernel, dim3(c->batch, K + 1), dim3(64), 0, c->stream, c->ka, sq, ma);          // (one wavefront per trial point)
        hipLaunchKernelGGL(sqp_commit_kernel, dim3(c->batch), dim3(256), 0, c->stream, c->ka, sq, ma);
        HIPCHK(hipGetLastError());
        if (residuals(it + 1) || count_copy(it + 1)) return 1;
        HIPCHK(hipEventSynchronize(c->evpoll[it & 1]));
        if (c->hactive[it & 1] == 0) break;
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    if (solve_done(c, SOLVE_SQP, c->time_ipm)) return 1;
    c->solved_merit = merit; c->merit_K = K; c->merit_M = c->nlp_max_iter; c->merit_weight_eq_used = c->merit_weight_eq;
    return 0;
}

// 1: dispatch instances longest-first using the previous solve's iteration counts (default), 0: natural order
extern "C" int tum_ocp_set_schedule(tum_ocp *c, int longest_first)
{
    if (!c) return fail("null capsule");
    if (c->lpt != (longest_first != 0)) invalidate(c, CH_CAPTURED);
    c->lpt = longest_first != 0;
    return 0;
}

extern "C" int tum_ocp_solve_async(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    if (c->nlp_type) return launch_sqp(c);          // (the host reads the active count between iterations: returns behind the last QP)
    if (c->rti_phase == 1) return launch_prepare(c);
    return launch(c);
}
extern "C" int tum_ocp_synchronize(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    return lin_uniform_check(c);
}

// the end of a synchronous solve: wait, the safety net, the largest status of the batch (-1: the call failed). A preparation has no
// results: 0 (acados >= 0.3 returns ACADOS_READY here; the reference's callers take any non-zero status for a failure)
static int wait_status(tum_ocp *c, bool results = true)
{
    if (hipStreamSynchronize(c->stream) != hipSuccess) { fail("kernel execution failed"); return -1; }
    if (lin_uniform_check(c)) return -1;
    if (!results) return 0;
    std::vector<int> st(c->batch);
    if (hipMemcpy(st.data(), c->dstatus, sizeof(int) * c->batch, hipMemcpyDeviceToHost) != hipSuccess) { fail("status copy failed"); return -1; }
    int mx = 0;
    for (int s : st) if (s > mx) mx = s;
    return mx;
}

extern "C" int tum_ocp_solve(tum_ocp *c)
{
    if (!c) { fail("null capsule"); return -1; }
    DevGuard guard(c->d.device); if (!guard.ok) { fail("hipSetDevice failed"); return -1; }
    if (c->nlp_type) return launch_sqp(c) ? -1 : wait_status(c);
    if (rti_gate(c)) return -1;          // (before anything is uploaded or invalidated)
    if (c->rti_phase == 1) return launch_prepare(c) ? -1 : wait_status(c, false);
    if (small_inputs(c) && results_pack_all(c, 1)) {
        // small capsule: [pending setters up + device clock] -> solve -> [summary, X, U into pinned slabs + device clock], ONE wait. No
        // event and no copy command on the stream; the getters that follow read the slabs (cache_valid).
        const size_t B = c->batch; const int N = c->N;
        auto hm = [&](auto **pp, size_t bytes) { return *pp || hipHostMalloc((void **)pp, bytes, hipHostMallocDefault) == hipSuccess; };
        if (shadow_ready(c)) return -1;
        if (!hm(&c->hsum_s, sizeof(double) * B * 5) || !hm(&c->hX_s, sizeof(double) * B * (N + 1) * NX) || !hm(&c->hU_s, sizeof(double) * B * N * NU) ||
            !hm(&c->hts_s, 2 * sizeof(unsigned long long))) { fail("solve: pinned allocation failed"); return -1; }
        if (c->ts_khz == 0.0) { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->d.device) != hipSuccess) khz = 0; c->ts_khz = khz > 0 ? (double)khz : 1e5; }
        if (flush_inputs(c, c->hts_s, true)) return -1;
        c->skip_ipm_events = true;
        const int rc = launch(c, false);
        c->skip_ipm_events = false;
        if (rc) return -1;
        hipLaunchKernelGGL(pack_results_kernel, dim3(8), dim3(256), 0, c->stream, c->dX, c->dU, c->dcost, c->dstatus, c->dqpiter, N, (int)B,
                           c->hsum_s, c->hX_s, c->hU_s, c->hts_s);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { fail("kernel execution failed"); return -1; }
        if (lin_uniform_check(c)) return -1;
        c->in_inflight = false;
        c->ts_slot = 2; c->cache_valid = true;          // (xs_cached went with the cache at the start of the solve)
        int mx = 0;
        for (size_t b = 0; b < B; b++) { const int st = (int)c->hsum_s[b * 5 + 3]; if (st > mx) mx = st; }
        return mx;
    }
    return launch(c) ? -1 : wait_status(c);
}

extern "C" double tum_ocp_last_kernel_ms(tum_ocp *c)
{
    if (!c || !(c->solved || c->prep_timed)) return 0.0;
    DevGuard guard(c->d.device); if (!guard.ok) return 0.0;
    if (c->ts_slot == 2) {      // the synchronous solve of a small capsule: clocked by its first and last kernel, already waited for
        c->last_ms = (float)((double)(c->hts_s[1] - c->hts_s[0]) / c->ts_khz);
        return c->last_ms;
    }
    if (c->ts_slot >= 0) {      // a step timed by the device's wall clock (tum_ocp_step_async): valid once its results have been waited for
        const int w = c->ts_slot;
        if (c->evres[w] && hipEventSynchronize(c->evres[w]) != hipSuccess) return 0.0;
        const unsigned long long t0 = c->hts[w][0], t1 = c->hts[w][1];
        c->last_ms = (float)((double)(t1 - t0) / c->ts_khz);
        return c->last_ms;
    }
    if (hipEventSynchronize(c->ev1) != hipSuccess) return 0.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return 0.0;
    c->last_ms = ms;
    return ms;
}

extern "C" int tum_ocp_get_cost(tum_ocp *c, double *out, int b0, int nb)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!out) return fail("null argument");
    if (c->cache_valid) { for (int i = 0; i < nb; i++) out[i] = c->hsum_s[(size_t)(b0 + i) * 5 + 2]; return 0; }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));        // (the copy below runs on the NULL stream, which the capsule's non-blocking stream is not ordered with)
    if (lin_uniform_check(c)) return 1;
    HIPCHK(hipMemcpy(out, c->dcost + b0, sizeof(double) * nb, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tum_ocp_get_stats(tum_ocp *c, const char *field, void *out, int b0, int nb)
{
    if (!c || !field || !out) return fail("null argument");
    const std::string f(field);
    if (f == "time_tot") { *(double *)out = tum_ocp_last_kernel_ms(c) * 1e-3; return 0; }
    if (f == "time_ipm") {    // pipeline only: device seconds of the interior point kernel of the last solve
        if (!c->solved || !c->solved_pipe || !c->ipm_timed)
            return fail("get_stats time_ipm: pipeline kernel only, after a solve() / solve_async() (a step, and the synchronous solve of a small capsule, leave these "
                        "events out unless tum_ocp_set_kernel(c, \"time-ipm\") asked for them)");
        DevGuard guard(c->d.device); GUARD_OK(guard);
        float ms = 0;
        if (hipEventSynchronize(c->evi1) != hipSuccess || hipEventElapsedTime(&ms, c->evi0, c->evi1) != hipSuccess) return fail("get_stats time_ipm: no timing");
        *(double *)out = ms * 1e-3; return 0;
    }
    if (f == "records_skipped") { *(int *)out = c->n_records_skipped; return 0; }      // solves that ran without stage records (one int)
    if (f == "lin_uniform") { *(int *)out = c->n_lin_uniform; return 0; }      // linearisations that took the uniform path (one int)
    if (f == "cond_shifted") {      // instances of the last solve whose condensing took the shift form (one int): the kernel's per-instance flags, summed here
        *(int *)out = 0;
        if (!c->shift_counted) return 0;
        DevGuard guard(c->d.device); GUARD_OK(guard);
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<int> h((size_t)c->batch);
        HIPCHK(hipMemcpy(h.data(), c->dshift, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
        int n = 0;
        for (int v : h) n += v;
        *(int *)out = n;
        return 0;
    }
    if (chk_range(c, b0, nb)) return 1;
    if (f == "sqp_iter" && !c->solved_sqp) { int *o = (int *)out; for (int i = 0; i < nb; i++) o[i] = 1; return 0; }      // (SQP-RTI: one QP per solve)
    if (f == "residuals" && !c->solved_sqp) return fail("get_stats residuals: computed by a full SQP solve only (options_set nlp_solver_type 1)");
    const bool merit_field = f == "alpha" || f == "merit" || f == "merit_weights" || f == "merit_dims";
    if (merit_field && !(c->solved_sqp && c->solved_merit))
        return fail("get_stats " + f + ": written by the line search of a full SQP solve with globalization MERIT_BACKTRACKING only "
                    "(options_set nlp_solver_type 1, globalization 1)");
    if (f == "merit_dims") { int *o = (int *)out; o[0] = c->merit_K; o[1] = c->merit_M; return 0; }
    if (c->cache_valid && (f == "qp_iter" || f == "status")) {
        int *o = (int *)out; const int col = (f == "status") ? 3 : 4;
        for (int i = 0; i < nb; i++) o[i] = (int)c->hsum_s[(size_t)(b0 + i) * 5 + col];
        return 0;
    }
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));        // (after tum_ocp_solve_async: the copies below are on the NULL stream)
    if (lin_uniform_check(c)) return 1;
    if (f == "qp_iter") { HIPCHK(hipMemcpy(out, c->dqpiter + b0, sizeof(int) * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "status") { HIPCHK(hipMemcpy(out, c->dstatus + b0, sizeof(int) * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "qp_status") { HIPCHK(hipMemcpy(out, c->dqpstatus + b0, sizeof(int) * nb, hipMemcpyDeviceToHost)); return 0; }
    // the longest-first order the next solve dispatches in (entries b0 .. b0 + nb - 1 of the permutation); the identity map while no
    // order is kept: a batch of at most 1024, or before the first solve
    if (f == "lpt_order") { HIPCHK(hipMemcpy(out, c->dorder + b0, sizeof(int) * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "res") { HIPCHK(hipMemcpy(out, c->dres + (size_t)b0 * 3, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "sqp_iter") { HIPCHK(hipMemcpy(out, c->dsqpiter + b0, sizeof(int) * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "residuals") { HIPCHK(hipMemcpy(out, c->dnlpres + (size_t)b0 * 4, sizeof(double) * 4 * nb, hipMemcpyDeviceToHost)); return 0; }
    if (f == "alpha") {
        HIPCHK(hipMemcpy(out, c->dmhist + (size_t)b0 * c->merit_M, sizeof(double) * (size_t)c->merit_M * nb, hipMemcpyDeviceToHost));
        return 0;
    }
    if (f == "merit") {
        const size_t row = (size_t)(c->merit_K + 1) * 3;
        HIPCHK(hipMemcpy(out, c->dmtable + (size_t)b0 * row, sizeof(double) * row * nb, hipMemcpyDeviceToHost));
        return 0;
    }
    if (f == "merit_weights") {
        std::vector<double> mu(nb);
        HIPCHK(hipMemcpy(mu.data(), c->dmmu + b0, sizeof(double) * nb, hipMemcpyDeviceToHost));
        double *o = (double *)out;
        for (int i = 0; i < nb; i++) { o[2 * i] = c->merit_weight_eq_used; o[2 * i + 1] = mu[i]; }
        return 0;
    }
    return fail("get_stats: unknown field '" + f + "'");
}

extern "C" int tum_ocp_reset(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    invalidate(c, CH_ITERATE);
    HIPCHK(hipMemsetAsync(c->dqplam, 0, sizeof(double) * (size_t)c->batch * (6 * (size_t)c->N + 2), c->stream));
    HIPCHK(hipMemsetAsync(c->dX, 0, sizeof(double) * (size_t)c->batch * (c->N + 1) * NX, c->stream));
    HIPCHK(hipMemsetAsync(c->dU, 0, sizeof(double) * (size_t)c->batch * c->N * NU, c->stream));
    HIPCHK(hipMemsetAsync(c->dslack, 0, sizeof(double) * (size_t)c->batch * 6 * (size_t)c->N, c->stream));
    invalidate(c, CH_RESTART);          // (X = 0, U = 0 at every stage)
    if (c->sn) HIPCHK(hipMemsetAsync(c->dXS, 0, sizeof(double) * (size_t)c->batch * (c->N + 1) * c->sa.ns * NX, c->stream));
    if (c->sn) { HIPCHK(hipMemsetAsync(c->dxs_dirty, 0, sizeof(int) * (size_t)c->batch, c->stream)); c->xs_lazy = false; }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int tum_ocp_cold_start(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    invalidate(c, CH_ITERATE);
    if (flush_inputs(c)) return 1;          // (the x0 it copies may still be in the pinned shadow)
    hipLaunchKernelGGL(cold_start_kernel, dim3(c->batch), dim3(64), 0, c->stream, c->dX, c->dU, c->dx0, c->N, c->batch, c->dqplam);
    if (c->sn && c->fanout && sn_fanout(c)) return 1;
    if (c->sn) hipLaunchKernelGGL(snmpc_cold_start_kernel, dim3(c->batch), dim3(256), 0, c->stream, c->dXS, c->dxs0, c->N, c->sa.ns, c->batch);
    if (c->sn) { HIPCHK(hipMemsetAsync(c->dxs_dirty, 0, sizeof(int) * (size_t)c->batch, c->stream)); c->xs_lazy = false; }
    HIPCHK(hipGetLastError());
    invalidate(c, CH_RESTART);          // (X_k = x0, U_k = 0 at every stage)
    return 0;
}

// A_k (column-major 8 x 8), B_k (column-major 8 x 2) and b_k (8) of one compact linearisation record ([0,1] Sp | [2..43] S[6][7] |
// [44..51] defect: the first 52 doubles of a stage record and of a sample record of the coupled SNMPC OCP alike); null pointers are skipped
static void expand_record(const double *q, double dt, double *A, double *B, double *b)
{
    if (A) {
        for (int e = 0; e < 64; e++) A[e] = 0.0;
        for (int d : {0, 1, 2, 6, 7}) A[d * 8 + d] = 1.0;
        A[2 * 8 + 0] = q[0]; A[2 * 8 + 1] = q[1];
        for (int ri = 0; ri < 6; ri++) for (int cc = 0; cc < 5; cc++) A[(3 + cc) * 8 + ri] = q[2 + ri * 7 + cc];
    }
    if (B) {
        for (int e = 0; e < 16; e++) B[e] = 0.0;
        for (int ri = 0; ri < 6; ri++) { B[0 * 8 + ri] = q[2 + ri * 7 + 5]; B[1 * 8 + ri] = q[2 + ri * 7 + 6]; }
        B[1 * 8 + 6] = dt; B[0 * 8 + 7] = dt;
    }
    if (b) for (int ri = 0; ri < 8; ri++) b[ri] = q[44 + ri];
}

extern "C" int tum_ocp_get_from_qp_in(tum_ocp *c, int stage, const char *field, double *out, int len, int b0, int nb, int stride)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!c->d.store_qp_in) return fail("get_from_qp_in: capsule created without store_qp_in");
    if (!c->solved) return fail("get_from_qp_in: no solve yet");
    if (stage < 0 || stage >= c->N) return fail("get_from_qp_in: stage out of range");
    const std::string f(field ? field : "");
    int off, n, rows, cols;
    if (f == "A") { off = 0; n = 64; rows = 8; cols = 8; }
    else if (f == "B") { off = 64; n = 16; rows = 8; cols = 2; }
    else if (f == "b") { off = 80; n = 8; rows = 8; cols = 1; }
    else return fail("get_from_qp_in: unknown field '" + f + "'");
    if (len != n || stride < n) return fail("get_from_qp_in: bad len/stride");
    if (c->solved_pipe) {   // the pipeline keeps the linearisation as compact stage records (pipe_kernels.hpp): expand on the host
        std::vector<double> r((size_t)nb * PREC);
        if (fetch(c, c->drec, (size_t)(c->N + 1) * PREC, (size_t)stage * PREC, r.data(), PREC, b0, nb, PREC)) return 1;
        for (int i = 0; i < nb; i++) {
            double *o = out + (size_t)i * stride;
            expand_record(&r[(size_t)i * PREC], c->ka.dt, f == "A" ? o : nullptr, f == "B" ? o : nullptr, f == "b" ? o : nullptr);
        }
        return 0;
    }
    std::vector<double> tmp((size_t)nb * n);
    if (fetch(c, c->dqpin, (size_t)c->N * 88, (size_t)stage * 88 + off, tmp.data(), n, b0, nb, n)) return 1;
    for (int i = 0; i < nb; i++)          // device keeps row-major, acados hands out column-major
        for (int r = 0; r < rows; r++)
            for (int q = 0; q < cols; q++) out[(size_t)i * stride + q * rows + r] = tmp[(size_t)i * n + r * cols + q];
    return 0;
}

extern "C" int tum_ocp_set_stream(tum_ocp *c, void *hip_stream)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    // whatever is still pending on the old stream (asynchronous uploads, a bounds snapshot, a solve) must not be overtaken
    // by work enqueued on the new one
    if (c->stream) HIPCHK(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)hip_stream; c->own_stream = false;
    return 0;
}

extern "C" int tum_ocp_get_device(tum_ocp *c, const char *field, void *dst, int b0, int nb)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !dst) return fail("null argument");
    const int N = c->N;
    const std::string f(field);
    DevGuard guard(c->d.device); GUARD_OK(guard);
    hipStream_t s = c->stream;
    if (f == "summary") {
        hipLaunchKernelGGL(pack_summary_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, c->dU, c->dcost, c->dstatus, c->dqpiter, N, b0, nb, (double *)dst);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (f == "u0") { HIPCHK(hipMemcpy2DAsync(dst, 2 * 8, c->dU + (size_t)b0 * N * NU, (size_t)N * NU * 8, 2 * 8, nb, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "x1") { HIPCHK(hipMemcpy2DAsync(dst, 8 * 8, c->dX + (size_t)b0 * (N + 1) * NX + NX, (size_t)(N + 1) * NX * 8, 8 * 8, nb, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "cost") { HIPCHK(hipMemcpyAsync(dst, c->dcost + b0, 8 * (size_t)nb, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "X") { HIPCHK(hipMemcpyAsync(dst, c->dX + (size_t)b0 * (N + 1) * NX, 8 * (size_t)nb * (N + 1) * NX, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "U") { HIPCHK(hipMemcpyAsync(dst, c->dU + (size_t)b0 * N * NU, 8 * (size_t)nb * N * NU, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "status") { HIPCHK(hipMemcpyAsync(dst, c->dstatus + b0, 4 * (size_t)nb, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "qp_iter") { HIPCHK(hipMemcpyAsync(dst, c->dqpiter + b0, 4 * (size_t)nb, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "qp_vec") {      // gradient q and row constants d of the condensed QP in the pipeline's workspace, read-only
        if (!c->dvec) return fail("get_device qp_vec: no pipeline solve or preparation yet");
        return with_tiles(c, [&](auto ntc) {
            using D = PD<decltype(ntc)::value>;
            const size_t nvp = D::NVP, pvec = D::PVEC;
            HIPCHK(hipMemcpy2DAsync(dst, 2 * nvp * 8, c->dvec + (size_t)b0 * pvec, pvec * 8, 2 * nvp * 8, nb, hipMemcpyDeviceToDevice, s));
            return 0;
        });
    }
    return fail("get_device: unknown field '" + f + "'");
}

// Results on the host behind an event instead of a stream synchronisation (include/tum_nmpc.h). The slabs are allocated on first
// use: pinned memory is a scarce host resource and most capsules (closed loops on the device, the RCCL gather) never ask.
// from_step: the request closes a tum_ocp_step_async whose clock pair hts[w] the packing kernel completes; a plain request never
// touches a clock pair (it would change the time_tot of the last step after the fact)
static int results_enqueue(tum_ocp *c, int with_iterate, bool from_step)
{
    const size_t B = c->batch; const int N = c->N;
    // Two sets of slabs / events used in turn: a caller keeps one request outstanding per capsule while it enqueues the next batch
    // and its request, and only then reads the older one -- the stream never runs dry between two batches waiting for the host.
    if (c->res_count == 2) return fail("results_async: two requests outstanding on this capsule (call tum_ocp_results_wait first)");
    const int w = (c->res_head + c->res_count) & 1;
    if (!c->evres[w]) HIPCHK(hipEventCreateWithFlags(&c->evres[w], hipEventDisableTiming));
    if (!c->dsum) { if (dalloc(&c->dsum, B * 5) != hipSuccess) return fail("results_async: device allocation failed"); }
    if (!c->hsum[w]) HIPCHK(hipHostMalloc((void **)&c->hsum[w], sizeof(double) * B * 5, hipHostMallocDefault));
    if (with_iterate && !c->hX[w]) {
        HIPCHK(hipHostMalloc((void **)&c->hX[w], sizeof(double) * B * (N + 1) * NX, hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&c->hU[w], sizeof(double) * B * N * NU, hipHostMallocDefault));
    }
    // The copies stay on the capsule's own stream. (Tried: a copy stream per capsule behind an event of the solve. Three capsules
    // then own six streams, more than the four hardware queues the runtime multiplexes streams onto: the capsules' compute
    // streams start to share queues and their batches no longer overlap -- 2.6 instead of 3.8 M solves/s on config 2.)
    hipStream_t s = c->stream;
    // the summary (40 B per instance) is written by the packing kernel STRAIGHT into the pinned slab (host memory mapped into the
    // device's address space): no copy command, no DMA engine and no signal round trip between the kernels of two batches
    const bool zero_copy = results_zero_copy();
    // small batches with the iterate: ONE kernel writes summary, X and U into the pinned slabs (a copy command costs 4-5 us on the
    // stream whatever its size; the two of the iterate were a tenth of a host-driven control step of one instance)
    const bool pack_all = results_pack_all(c, with_iterate);
    if (pack_all) {
        hipLaunchKernelGGL(pack_results_kernel, dim3(8), dim3(256), 0, s, c->dX, c->dU, c->dcost, c->dstatus, c->dqpiter, N, (int)B,
                           c->hsum[w], c->hX[w], c->hU[w], (from_step && c->ts_slot == w) ? c->hts[w] : (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    } else {
    hipLaunchKernelGGL(pack_summary_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, c->dU, c->dcost, c->dstatus, c->dqpiter, N, 0, (int)B,
                       zero_copy ? c->hsum[w] : c->dsum);
    HIPCHK(hipGetLastError());
    }
    if (!zero_copy) HIPCHK(hipMemcpyAsync(c->hsum[w], c->dsum, sizeof(double) * B * 5, hipMemcpyDeviceToHost, s));
    if (with_iterate && !pack_all) {
        HIPCHK(hipMemcpyAsync(c->hX[w], c->dX, sizeof(double) * B * (N + 1) * NX, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(c->hU[w], c->dU, sizeof(double) * B * N * NU, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(c->evres[w], s));
    c->res_iter[w] = with_iterate != 0;
    c->res_count++;
    return 0;
}

extern "C" int tum_ocp_results_async(tum_ocp *c, int with_iterate)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    return results_enqueue(c, with_iterate, false);
}

extern "C" int tum_ocp_results_outstanding(const tum_ocp *c) { return c ? c->res_count : -1; }

extern "C" int tum_ocp_results_wait(tum_ocp *c, const double **summary, const double **X, const double **U)
{
    if (!c) return fail("null capsule");
    if (c->res_count == 0) return fail("results_wait: no tum_ocp_results_async before it");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const int r = c->res_head;          // the OLDEST outstanding request
    HIPCHK(hipEventSynchronize(c->evres[r]));
    if (summary) *summary = c->hsum[r];
    if (X) *X = c->res_iter[r] ? c->hX[r] : nullptr;
    if (U) *U = c->res_iter[r] ? c->hU[r] : nullptr;
    c->res_head ^= 1; c->res_count--;
    return lin_uniform_check(c);
}

extern "C" int tum_ocp_step_async(tum_ocp *c, const double *x0, const double *yref, int with_iterate)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (c->nlp_type) return fail("step_async: one SQP-RTI iteration per step; a capsule in SQP mode (nlp_solver_type 1) takes tum_ocp_solve");
    if (c->res_count == 2) return fail("step_async: two requests outstanding on this capsule (call tum_ocp_results_wait first)");
    if (c->rti_phase == 1) return fail("step_async: a preparation (rti_phase 1) has no results: prepare with tum_ocp_solve / tum_ocp_solve_async");
    if (c->rti_phase == 2 && yref) return fail("step_async: the reference enters in the preparation; a feedback step (rti_phase 2) takes x0 only (yref = NULL)");
    if (rti_gate(c)) return 1;
    if (flush_inputs(c)) return 1;          // (setters older than this step's inputs)
    const size_t B = c->batch, nx0 = B * NX, nyr = B * (size_t)(c->N + 1) * 6;
    // the staging area of the result slot this step will use: its previous step has been waited for, so its uploads are done
    const int w = (c->res_head + c->res_count) & 1;
    if ((x0 || yref) && !c->hin[w]) HIPCHK(hipHostMalloc((void **)&c->hin[w], sizeof(double) * (nx0 + nyr), hipHostMallocDefault));
    if (x0) {
        if (c->sn) { if (!c->have_offs) return fail("step_async x0: an SNMPC capsule needs its sample offsets (tum_ocp_snmpc_set_offsets)"); c->fanout = true; }
        memcpy(c->hin[w], x0, sizeof(double) * nx0);
    }
    if (yref) memcpy(c->hin[w] + nx0, yref, sizeof(double) * nyr);
    // small batches with inputs and the iterate: the step is timed by the device's wall clock, read by its first and its last kernel
    // (stage_in_kernel, pack_results_kernel), instead of by events around the solve -- every event on the stream is a gap of 5 us
    const bool small_in = (x0 || yref) && nx0 + nyr <= 32768;
    // (the packing kernel is what reads the clock at the end: the same predicate as its launch, results_pack_all)
    const bool clocked = small_in && results_pack_all(c, with_iterate);
    if (clocked) {
        if (!c->hts[w]) HIPCHK(hipHostMalloc((void **)&c->hts[w], 2 * sizeof(unsigned long long), hipHostMallocDefault));
        if (c->ts_khz == 0.0) { int khz = 0; HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->d.device)); c->ts_khz = khz > 0 ? (double)khz : 1e5; }
    }
    if (small_in) {      // one kernel reads the staging area (host memory mapped into the device's address space)
        hipLaunchKernelGGL(stage_in_kernel, dim3(4), dim3(256), 0, c->stream, c->hin[w], c->dx0, (int)nx0, c->dyref, (int)nyr, x0 ? 1 : 0, yref ? 1 : 0,
                           clocked ? c->hts[w] : (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    } else {
        if (x0) HIPCHK(hipMemcpyAsync(c->dx0, c->hin[w], sizeof(double) * nx0, hipMemcpyHostToDevice, c->stream));
        if (yref) HIPCHK(hipMemcpyAsync(c->dyref, c->hin[w] + nx0, sizeof(double) * nyr, hipMemcpyHostToDevice, c->stream));
    }
    // (the two events around the interior point kernel -- get_stats "time_ipm" -- are left out of a step: every event on the stream
    //  is a gap of a few microseconds between two kernels; "time_tot" keeps its events)
    c->skip_ipm_events = true;
    const int rc = launch(c, !clocked);
    c->skip_ipm_events = false;
    if (rc) return 1;
    c->ts_slot = clocked ? w : -1;
    const int rr = results_enqueue(c, with_iterate, true);
    if (rr) c->ts_slot = -1;
    return rr;
}

// device-to-device upload of per-instance inputs from caller-owned HBM (asynchronous, on the capsule's stream)
extern "C" int tum_ocp_put_device(tum_ocp *c, const char *field, const void *src, int b0, int nb)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !src) return fail("null argument");
    const int N = c->N;
    const std::string f(field);
    DevGuard guard(c->d.device); GUARD_OK(guard);
    hipStream_t s = c->stream;
    const unsigned what = f == "x0" ? CH_X0 : f == "yref" ? CH_REF : (f == "X" || f == "U") ? CH_ITERATE : 0u;
    if (!what) return fail("put_device: unknown field '" + f + "'");
    invalidate(c, what | CH_UPLOAD);
    if (flush_inputs(c)) return 1;          // (setters older than this upload)
    if (f == "x0") {
        if (c->sn) { if (!c->have_offs) return fail("put_device x0: an SNMPC capsule needs its sample offsets (tum_ocp_snmpc_set_offsets)"); c->fanout = true; }
        HIPCHK(hipMemcpyAsync(c->dx0 + (size_t)b0 * NX, src, 8 * (size_t)nb * NX, hipMemcpyDeviceToDevice, s)); return 0;
    }
    if (f == "yref") { HIPCHK(hipMemcpyAsync(c->dyref + (size_t)b0 * (N + 1) * 6, src, 8 * (size_t)nb * (N + 1) * 6, hipMemcpyDeviceToDevice, s)); return 0; }
    if (f == "X") { HIPCHK(hipMemcpyAsync(c->dX + (size_t)b0 * (N + 1) * NX, src, 8 * (size_t)nb * (N + 1) * NX, hipMemcpyDeviceToDevice, s)); return 0; }
    HIPCHK(hipMemcpyAsync(c->dU + (size_t)b0 * N * NU, src, 8 * (size_t)nb * N * NU, hipMemcpyDeviceToDevice, s));
    return 0;
}

// Zero-copy inputs for callers whose batches are resident in HBM already (scenario fan-outs, sweeps: bench.py rotates resident batches):
// the capsule USES the caller's array as its x0 / yref array -- kernels read it in place, setters and the device closed loop write
// through to it -- instead of copying it into its own (tum_ocp_put_device: a blit kernel per field and step, 8 MB for yref at 16384 x
// N = 40; measured 1.2 % of a step on one stream, nothing with three capsules in flight, profiles/r05_bind_inputs.txt). Whole batch
// only; the memory must stay valid and unchanged while solves that use it are in flight. dev_ptr = NULL hands the capsule's own array back (its contents are what they were before the binding).
extern "C" int tum_ocp_bind_device(tum_ocp *c, const char *field, void *dev_ptr)
{
    if (!c || !field) return fail("null argument");
    const std::string f(field);
    if (f != "x0" && f != "yref") return fail("bind_device: field must be 'x0' or 'yref'");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;          // (setters parked in the pinned shadow belong to the array in use until now)
    if (f == "x0") {
        if (c->sn && dev_ptr) { if (!c->have_offs) return fail("bind_device x0: an SNMPC capsule needs its sample offsets (tum_ocp_snmpc_set_offsets)"); c->fanout = true; }
        c->dx0 = dev_ptr ? (double *)dev_ptr : c->dx0_own; c->ka.x0 = c->dx0;
    } else { c->dyref = dev_ptr ? (double *)dev_ptr : c->dyref_own; c->ka.yref = c->dyref; }
    invalidate(c, (f == "x0" ? CH_X0 : CH_REF) | CH_VARIANT | CH_CAPTURED);          // (a captured closed-loop chunk holds the pointers by value)
    return 0;
}

// One solve, then the condensed QP of instance b as the solve built it. Layout of `out` (doubles, N <= 40):
//   [0, 6400) H (80 x 80, symmetric, incl. the input cost and the unit padding) | [6400, 6480) q |
//   [6480, 6480 + 2 N 80) the steering-angle row and the gg row of every stage 1..N | [12880, 12880 + 2 N) their constants.
// The shipped library reads it back from the hand-over buffers of the pipeline (H tiles, gg rows in MFMA operand layout,
// q | d) -- so the dump shows what the interior point kernel is given; the development build keeps the fused kernel's own
// dump, which continues with g, the KKT matrix and the first right-hand side / step of the first iteration.
extern "C" int tum_ocp_debug_dump(tum_ocp *c, int b, double *out, int len)
{
    if (!c) return fail("null capsule");
    if (b < 0 || b >= DBG_INST || b >= c->batch) return fail("debug_dump: instance out of range");
    if (c->rti_phase) return fail("debug_dump: the split real-time iteration does not run with the debug dump or the phase timers (set rti_phase 0)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (len > DBG_STRIDE) len = DBG_STRIDE;
#ifdef TUM_DEV_KERNELS
    if (c->kmode != KMode::PIPELINE && c->kmode != KMode::PIPELINE4) {
        c->ka.flags |= KF_DEBUG;
        const int rc = launch(c);
        c->ka.flags &= ~KF_DEBUG;
        if (rc) return 1;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(out, c->ddbg + (size_t)b * DBG_STRIDE, sizeof(double) * len, hipMemcpyDeviceToHost));
        return 0;
    }
#endif
    if (c->N > NMAX) return fail("debug_dump: the condensed-QP dump is built for N <= 40");
    if (launch(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return with_tiles(c, [&](auto ntc) {          // (the 80 variables of N <= 40, whichever instantiation TUM_FORCE_TILES made the solve run)
        using D = PD<decltype(ntc)::value>;
        const int N = c->N;
        std::vector<double> hw((size_t)D::NTT * 256), cw((size_t)D::NCH * 64), vv(D::PVEC), o(DBG_STRIDE, 0.0);
        HIPCHK(hipMemcpy(hw.data(), c->dhws + (size_t)b * D::NTT * 256, sizeof(double) * hw.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cw.data(), c->dcws + (size_t)b * D::NCH * 64, sizeof(double) * cw.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(vv.data(), c->dvec + (size_t)b * D::PVEC, sizeof(double) * vv.size(), hipMemcpyDeviceToHost));
        for (int K = 0; K < 5; K++)
            for (int I = K; I < 5; I++)
                for (int l = 0; l < 64; l++)
                    for (int jj = 0; jj < 4; jj++) {         // accumulator layout: row (l >> 4) + 4 jj, column l & 15
                        const int row = 16 * K + (l >> 4) + 4 * jj, col = 16 * I + (l & 15);
                        const double v = hw[((size_t)D::tidx(K, I) * 64 + l) * 4 + jj];
                        o[row * 80 + col] = v; o[col * 80 + row] = v;
                    }
        for (int i = 0; i < 80; i++) o[6400 + i] = vv[D::PV_Q + i];
        for (int s = 1; s <= N; s++)
            for (int col = 0; col < 80; col++) {
                o[6480 + (2 * (s - 1)) * 80 + col] = ((col & 1) && col < 2 * s) ? c->ka.dt : 0.0;
                const int cc = (s - 1) >> 2, lq = (s - 1) & 3, T = col >> 4;       // operand layout: chunk cc, DPP row lq, tile column T
                o[6480 + (2 * (s - 1) + 1) * 80 + col] = (cc >= 2 * T) ? cw[(size_t)D::cidx(cc, T) * 64 + 16 * lq + (col & 15)] : 0.0;
            }
        for (int i = 0; i < 2 * N; i++) o[12880 + i] = vv[D::PV_D + i];
        // (development aid: the tail of the dump area carries the phase cycle counters of the SNMPC prologue kernels, SnArgs::dbg)
        HIPCHK(hipMemcpy(o.data() + 20000, c->ddbg + (size_t)b * DBG_STRIDE + 20000, sizeof(double) * (DBG_STRIDE - 20000), hipMemcpyDeviceToHost));
        memcpy(out, o.data(), sizeof(double) * len);
        return 0;
    });
}

// The condensed QP of the instances b0 .. b0 + nb - 1 as the LAST preparation or solve left it in the hand-over buffers of the
// pipeline, at every tile count and whichever condensing kernel ran. Launches nothing and writes nothing on the device.
//   info[0] = NVP (16 x tiles: condensed variables incl. the padding), info[1] = 2 N (rows), info[2] = 1 where dv is the step of
//   this QP (see below), 0 where the buffer does not hold it
//   H  nb x NVP x NVP, symmetric, unpacked from the accumulator-layout tiles (PD<NT>::tidx)
//   q  nb x NVP | d  nb x NVP: d[2 (s - 1)] the steering-angle row of stage s, d[2 (s - 1) + 1] its gg row
//   C  nb x 2 N x NVP: the same rows; the gg rows from the operand layout (PD<NT>::cidx), the steering-angle rows synthesised (dt on
//      the odd columns below 2 s) as the debug dump does -- no kernel stores them
//   dv nb x NVP: what PV_DV holds. The interior point kernel writes it for an expansion KERNEL behind it (batches beyond 1024, seven
//      tiles, the record-free chain, the coupled SNMPC OCP); where the expansion is its own tail the step stays in LDS: info[2] = 0
// Any of the array pointers may be null (skipped); with all of them null the call only answers info.
extern "C" int tum_ocp_get_condensed_qp(tum_ocp *c, int b0, int nb, double *H, double *q, double *C, double *d, double *dv, int *info)
{
    if (!c) return fail("null capsule");
#ifdef TUM_DEV_KERNELS
    if (c->kmode == KMode::FUSED) return fail("get_condensed_qp: the development kernel 'fused' condenses in registers and LDS and has no hand-over buffers (use 'auto' or 'pipeline')");
#endif
    if (!c->qp_handed || !c->dhws || !c->dcws || !c->dvec) return fail("get_condensed_qp: no preparation or solve has run on the pipeline yet: there is no condensed QP to read");
    if (b0 < 0 || nb < 0 || (long long)b0 + nb > c->batch) return fail("get_condensed_qp: instance range out of bounds");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (lin_uniform_check(c)) return 1;
    return with_tiles(c, [&](auto ntc) {
        using D = PD<decltype(ntc)::value>;
        constexpr int NT = D::NT, NVP = D::NVP;
        const int N = c->N, m = 2 * N;
        if (info) { info[0] = NVP; info[1] = m; info[2] = c->dv_handed ? 1 : 0; }
        std::vector<double> hw((size_t)D::NTT * 256), cw((size_t)D::NCH * 64), vv(D::PVEC);
        for (int i = 0; i < nb; i++) {
            const size_t b = (size_t)b0 + i;
            if (H) {
                HIPCHK(hipMemcpy(hw.data(), c->dhws + b * D::NTT * 256, sizeof(double) * hw.size(), hipMemcpyDeviceToHost));
                double *o = H + (size_t)i * NVP * NVP;
                for (int K = 0; K < NT; K++)
                    for (int I = K; I < NT; I++)
                        for (int l = 0; l < 64; l++)
                            for (int jj = 0; jj < 4; jj++) {         // accumulator layout: row (l >> 4) + 4 jj, column l & 15
                                const int row = 16 * K + (l >> 4) + 4 * jj, col = 16 * I + (l & 15);
                                const double v = hw[((size_t)D::tidx(K, I) * 64 + l) * 4 + jj];
                                o[(size_t)row * NVP + col] = v;
                                if (K != I) o[(size_t)col * NVP + row] = v;          // (a diagonal tile holds both triangles: they go out as stored, so that an asymmetry shows)
                            }
            }
            if (q || d || dv) {
                HIPCHK(hipMemcpy(vv.data(), c->dvec + b * D::PVEC, sizeof(double) * vv.size(), hipMemcpyDeviceToHost));
                if (q) memcpy(q + (size_t)i * NVP, vv.data() + D::PV_Q, sizeof(double) * NVP);
                if (d) memcpy(d + (size_t)i * NVP, vv.data() + D::PV_D, sizeof(double) * NVP);
                if (dv) memcpy(dv + (size_t)i * NVP, vv.data() + D::PV_DV, sizeof(double) * NVP);
            }
            if (C) {
                HIPCHK(hipMemcpy(cw.data(), c->dcws + b * D::NCH * 64, sizeof(double) * cw.size(), hipMemcpyDeviceToHost));
                double *o = C + (size_t)i * m * NVP;
                for (int s = 1; s <= N; s++)
                    for (int col = 0; col < NVP; col++) {
                        o[(size_t)(2 * (s - 1)) * NVP + col] = ((col & 1) && col < 2 * s) ? c->ka.dt : 0.0;
                        const int cc = (s - 1) >> 2, lq = (s - 1) & 3, T = col >> 4;       // operand layout: chunk cc, DPP row lq, tile column T
                        o[(size_t)(2 * (s - 1) + 1) * NVP + col] = (cc >= 2 * T) ? cw[(size_t)D::cidx(cc, T) * 64 + 16 * lq + (col & 15)] : 0.0;
                    }
            }
        }
        return 0;
    });
}

// The linearisation of the coupled SNMPC OCP of the instances b0 .. b0 + nb - 1 as the LAST pipeline solve left it: the sample records and
// gg values of the stages below the uncertainty propagation horizon (ws2 / gh: snmpc_lin_kernel or snmpc_lin_cols_kernel), the nominal
// stage records (lin_kernel<true> or lin_cols_kernel<true>). Launches nothing and writes nothing on the device.
//   info[0] = n_samples, info[1] = uph, info[2] = N
//   As nb x uph x ns x 64 | Bs nb x uph x ns x 16 (column-major, expand_record) | bs nb x uph x ns x 8
//   hs nb x uph x ns | ghs nb x uph x ns x 8: entries 3, 4, 5, 7 (the device writes zeros at stage 0)
//   hn nb x (N + 1) | ghn nb x (N + 1) x 8: entries 3, 4 (PR_G4), 5, 7 | cv nb x (N + 1) x 2 (PR_CV)
//   An nb x (N - uph) x 64 | Bn nb x (N - uph) x 16 | bn nb x (N - uph) x 8: the nominal records of the stages uph .. N - 1
// Any of the array pointers may be null (skipped); with all of them null the call only answers info.
extern "C" int tum_ocp_get_snmpc_linearisation(tum_ocp *c, int b0, int nb, double *As, double *Bs, double *bs, double *hs, double *ghs,
                                               double *hn, double *ghn, double *cv, double *An, double *Bn, double *bn, int *info)
{
    if (!c) return fail("null capsule");
    if (!c->sn) return fail("get_snmpc_linearisation: not an SNMPC capsule (tum_ocp_snmpc_attach)");
#ifdef TUM_DEV_KERNELS
    if (c->kmode == KMode::FUSED) return fail("get_snmpc_linearisation: the development kernel 'fused' keeps no stage records (use 'auto' or 'pipeline')");
#endif
    if (!c->qp_handed || !c->solved_pipe || !c->drec || !c->dws2) return fail("get_snmpc_linearisation: no solve has run on the pipeline yet: there is no linearisation to read");
    if (b0 < 0 || nb < 0 || (long long)b0 + nb > c->batch) return fail("get_snmpc_linearisation: instance range out of bounds");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    const int N = c->N, ns = c->sa.ns, uph = c->sa.uph, nitem = uph * ns, nn = N - uph;
    if (info) { info[0] = ns; info[1] = uph; info[2] = N; }
    const double dt = c->ka.dt;
    std::vector<double> w((size_t)nitem * ABS), g((size_t)nitem * 5), r((size_t)(N + 1) * PREC);
    for (int i = 0; i < nb; i++) {
        const size_t b = (size_t)b0 + i;
        if (nitem > 0 && (As || Bs || bs)) {
            HIPCHK(hipMemcpy(w.data(), c->sa.ws2 + b * nitem * ABS, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
            for (int it = 0; it < nitem; it++) {
                const size_t o = (size_t)i * nitem + it;
                expand_record(&w[(size_t)it * ABS], dt, As ? As + o * 64 : nullptr, Bs ? Bs + o * 16 : nullptr, bs ? bs + o * 8 : nullptr);
            }
        }
        if (nitem > 0 && (hs || ghs)) {
            HIPCHK(hipMemcpy(g.data(), c->sa.gh + b * nitem * 5, sizeof(double) * g.size(), hipMemcpyDeviceToHost));
            for (int it = 0; it < nitem; it++) {
                const size_t o = (size_t)i * nitem + it;
                const double *q = &g[(size_t)it * 5];
                if (hs) hs[o] = q[0];
                if (ghs) { double *v = ghs + o * 8; for (int e = 0; e < 8; e++) v[e] = 0.0; v[3] = q[1]; v[4] = q[2]; v[5] = q[3]; v[7] = q[4]; }
            }
        }
        if (hn || ghn || cv || An || Bn || bn) {
            HIPCHK(hipMemcpy(r.data(), c->drec + b * (size_t)(N + 1) * PREC, sizeof(double) * r.size(), hipMemcpyDeviceToHost));
            for (int k = 0; k <= N; k++) {
                const double *q = &r[(size_t)k * PREC];
                const size_t o = (size_t)i * (N + 1) + k;
                if (hn) hn[o] = q[PR_GH + 3];
                if (ghn) { double *v = ghn + o * 8; for (int e = 0; e < 8; e++) v[e] = 0.0; v[3] = q[PR_GH]; v[4] = q[PR_G4]; v[5] = q[PR_GH + 1]; v[7] = q[PR_GH + 2]; }
                if (cv) { cv[o * 2] = q[PR_CV]; cv[o * 2 + 1] = q[PR_CV + 1]; }
                if (k >= uph && k < N) {
                    const size_t on = (size_t)i * nn + (k - uph);
                    expand_record(q, dt, An ? An + on * 64 : nullptr, Bn ? Bn + on * 16 : nullptr, bn ? bn + on * 8 : nullptr);
                }
            }
        }
    }
    return 0;
}

// development aid: one solve with the in-kernel phase timers on; out = batch x 12 cycle counters
extern "C" int tum_ocp_profile_phases(tum_ocp *c, long long *out)
{
    if (!c || !out) return fail("null argument");
    if (c->N > NMAX) return fail("profile_phases: the instrumented kernels are built for N <= 40");
    if (c->rti_phase) return fail("profile_phases: the split real-time iteration does not run with the debug dump or the phase timers (set rti_phase 0)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    c->ka.flags |= KF_PROF;
    int rc = launch(c);
    c->ka.flags &= ~KF_PROF;
    if (rc) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->dprof, sizeof(long long) * 12 * (size_t)c->batch, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------- K6 / K7
extern "C" int tum_ocp_set_x0_fanout(tum_ocp *c, const double *pose, const double *offs, int P, int S)
{
    if (!c || !pose || (S > 0 && !offs)) return fail("null argument");
    const int S1 = S + 1;
    if (P < 1 || S < 0 || (long long)P * S1 != c->batch) return fail("set_x0_fanout: P*(S+1) must equal the batch size");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (flush_inputs(c)) return 1;
    DevTmp tp, to;
    HIPCHK(tp.alloc(sizeof(double) * P * NX));
    HIPCHK(to.alloc(sizeof(double) * (S > 0 ? S : 1) * NX));
    double *dp = tp.as<double>(), *dofs = to.as<double>();
    HIPCHK(hipMemcpyAsync(dp, pose, sizeof(double) * P * NX, hipMemcpyHostToDevice, c->stream));
    if (S > 0) HIPCHK(hipMemcpyAsync(dofs, offs, sizeof(double) * S * NX, hipMemcpyHostToDevice, c->stream));
    const int n = P * S1 * NX;
    hipLaunchKernelGGL(sigma_fanout_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->dx0, dp, dofs, P, S1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// PCE matrix of the scenario fan-out kept on the device (L x S, row-major, host) for tum_pce_moments_device
extern "C" int tum_pce_attach(tum_ocp *c, const double *A, int L, int S)
{
    if (!c || !A) return fail("null argument");
    if (S < 1 || L < 1 || c->batch % (S + 1) != 0) return fail("pce_attach: batch must be a multiple of S+1");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(c->dpceA); c->dpceA = nullptr;
    if (dalloc(&c->dpceA, (size_t)L * S) != hipSuccess) return fail("pce_attach: device allocation failed");
    HIPCHK(hipMemcpy(c->dpceA, A, sizeof(double) * L * S, hipMemcpyHostToDevice));
    c->pce_L = L; c->pce_S = S;
    return 0;
}

static int pce_launch(tum_ocp *c, const std::string &f, int stage, const double *dA, int L, int S, double *dmean, double *dvar)
{
    const int S1 = S + 1, N = c->N, P = c->batch / S1;
    int m; const double *src; size_t rec, off;
    if (f == "x") { if (stage < 0 || stage > N) return fail("pce_moments: stage"); m = NX; src = c->dX; rec = (size_t)(N + 1) * NX; off = (size_t)stage * NX; }
    else if (f == "u") { if (stage < 0 || stage >= N) return fail("pce_moments: stage"); m = NU; src = c->dU; rec = (size_t)N * NU; off = (size_t)stage * NU; }
    else return fail("pce_moments: unknown field '" + f + "'");
    hipLaunchKernelGGL(pce_moments_kernel, dim3((P * m + 127) / 128), dim3(128), 0, c->stream, src + off, rec, dA, P, S1, m, L, dmean, dvar);
    HIPCHK(hipGetLastError());
    return 0;
}

// Asynchronous, device-to-device flavour (the reduction of BASELINE config 3 inside the timed step): mean_dev / var_dev are
// caller-owned device buffers of P x m doubles; the matrix is the one registered with tum_pce_attach.
extern "C" int tum_pce_moments_device(tum_ocp *c, const char *field, int stage, double *mean_dev, double *var_dev)
{
    if (!c || !field || !mean_dev || !var_dev) return fail("null argument");
    if (!c->dpceA) return fail("pce_moments_device: no PCE matrix registered (tum_pce_attach)");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    return pce_launch(c, field, stage, c->dpceA, c->pce_L, c->pce_S, mean_dev, var_dev);
}

extern "C" int tum_pce_moments(tum_ocp *c, const char *field, int stage, const double *A, int L, int S, double *mean, double *var)
{
    if (!c || !field || !A || !mean || !var) return fail("null argument");
    const int S1 = S + 1;
    if (S < 1 || L < 1 || c->batch % S1 != 0) return fail("pce_moments: batch must be a multiple of S+1");
    const int P = c->batch / S1;
    const int m = (std::string(field) == "u") ? NU : NX;
    DevGuard guard(c->d.device); GUARD_OK(guard);
    DevTmp tA, tm, tv;
    HIPCHK(tA.alloc(sizeof(double) * L * S));
    HIPCHK(tm.alloc(sizeof(double) * P * m)); HIPCHK(tv.alloc(sizeof(double) * P * m));
    double *dA = tA.as<double>(), *dm = tm.as<double>(), *dv = tv.as<double>();
    HIPCHK(hipMemcpyAsync(dA, A, sizeof(double) * L * S, hipMemcpyHostToDevice, c->stream));
    if (pce_launch(c, field, stage, dA, L, S, dm, dv)) return 1;
    HIPCHK(hipMemcpyAsync(mean, dm, sizeof(double) * P * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(var, dv, sizeof(double) * P * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Snapshot / restore of all per-stage bounds (lbu, ubu, lbx, ubx, lh, uh) on the device. The R2NMPC tightening rewrites the
// bounds after every solve; a benchmark or a sweep that restarts from the nominal problem restores them without a host copy.
extern "C" int tum_ocp_bounds_snapshot(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const size_t n = (size_t)c->batch * 6 * (c->N + 1);
    if (!c->dbnd_snap && dalloc(&c->dbnd_snap, n) != hipSuccess) return fail("bounds_snapshot: device allocation failed");
    HIPCHK(hipMemcpyAsync(c->dbnd_snap, c->dbnd, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int tum_ocp_bounds_restore(tum_ocp *c)
{
    if (!c) return fail("null capsule");
    if (!c->dbnd_snap) return fail("bounds_restore: no snapshot taken");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    HIPCHK(hipMemcpyAsync(c->dbnd, c->dbnd_snap, sizeof(double) * (size_t)c->batch * 6 * (c->N + 1), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int tum_ocp_r2_backoff(tum_ocp *c, const double *Sigma0, const double *BWB, int uph,
                                  double delta_min, double delta_max, double uh_nom, double *backoff)
{
    if (!c || !Sigma0 || !BWB) return fail("null argument");
    if (!c->d.store_qp_in) return fail("r2_backoff: capsule created without store_qp_in");
    if (!c->solved) return fail("r2_backoff: no solve yet");
    if (uph < 1) return fail("r2_backoff: uncertainty propagation horizon < 1");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    const int N = c->N;
    DevTmp tS, tB, tbo;
    HIPCHK(tS.alloc(64 * 8)); HIPCHK(tB.alloc(64 * 8));
    double *dS = tS.as<double>(), *dB = tB.as<double>(), *dbo = nullptr;
    if (backoff) {
        HIPCHK(tbo.alloc(sizeof(double) * (size_t)c->batch * N * 2)); dbo = tbo.as<double>();
        HIPCHK(hipMemsetAsync(dbo, 0, sizeof(double) * (size_t)c->batch * N * 2, c->stream));
    }
    HIPCHK(hipMemcpyAsync(dS, Sigma0, 64 * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dB, BWB, 64 * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(r2_backoff_kernel, dim3((c->batch + 3) / 4), dim3(256), 0, c->stream, c->dqpin, c->dX, c->dbnd, c->ka.mp,
                       dS, dB, N, uph, c->batch, delta_min, delta_max, uh_nom, dbo, c->dstatus,
                       c->solved_pipe ? c->drec : (const double *)nullptr, PREC);
    HIPCHK(hipGetLastError());
    if (backoff) HIPCHK(hipMemcpyAsync(backoff, dbo, sizeof(double) * (size_t)c->batch * N * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Make the R2NMPC tightening part of every solve (what Reduced_Robustified_NMPC_class.py:276-378 does after each successful
// acados call): after the SQP-RTI kernel the back-off kernel rewrites lbx / ubx / uh of the stages 1..N-1 for the NEXT solve,
// on the capsule's stream, inside the time `get_stats("time_tot")` reports (:379-381). uph = 0 detaches.
extern "C" int tum_ocp_r2_attach(tum_ocp *c, const double *Sigma0, const double *BWB, int uph,
                                 double delta_min, double delta_max, double uh_nom)
{
    if (!c) return fail("null capsule");
    if (uph == 0) { if (c->r2) invalidate(c, CH_CAPTURED); c->r2 = false; return 0; }
    if (!Sigma0 || !BWB) return fail("null argument");
    if (!c->d.store_qp_in) return fail("r2_attach: capsule created without store_qp_in");
    if (c->sn) return fail("r2_attach: not available for an SNMPC capsule");
    if (uph < 1) return fail("r2_attach: uncertainty propagation horizon < 1");
    DevGuard guard(c->d.device); GUARD_OK(guard);
    if (!c->dr2S && (dalloc(&c->dr2S, 64) != hipSuccess || dalloc(&c->dr2B, 64) != hipSuccess)) return fail("r2_attach: device allocation failed");
    HIPCHK(hipMemcpy(c->dr2S, Sigma0, 64 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->dr2B, BWB, 64 * 8, hipMemcpyHostToDevice));
    c->r2_uph = uph; c->r2_dmin = delta_min; c->r2_dmax = delta_max; c->r2_uh = uh_nom;
    c->r2 = true;
    invalidate(c, CH_CAPTURED);
    return 0;
}

extern "C" int tum_ocp_constraints_get(tum_ocp *c, int stage, const char *field, double *v, int b0, int nb)
{
    if (chk_range(c, b0, nb)) return 1;
    if (!field || !v) return fail("null argument");
    const int N = c->N, NB = N + 1;
    const std::string f(field);
    int row;
    if (f == "lbu") row = 0; else if (f == "ubu") row = 1; else if (f == "lbx") row = 2; else if (f == "ubx") row = 3;
    else if (f == "lh") row = 4; else if (f == "uh") row = 5; else return fail("constraints_get: unknown field '" + f + "'");
    if (stage < 0 || stage > N) return fail("constraints_get: stage out of range");
    return fetch(c, c->dbnd, (size_t)6 * NB, (size_t)row * NB + stage, v, 1, b0, nb, 1);
}

// the device closed loop on the capsule above, host code like the rest of this file in headers of its own
#include "sim_loop.hpp"          // K8 / K9 / K18: tum_sim, the control step, the disturbance generator, segment scoring, the getters
#include "sim_rl.hpp"            // K11 to K14: the RL environment, the agent, collection, the trainer
#include "bo.hpp"                // K15: tum_bo, the acquisition value of the Bayesian-optimisation step
#include "gp.hpp"                // K16: tum_gp, the marginal log-likelihood of a surrogate and its factor
#include "bo_model.hpp"          // K17: tum_bom_prune / fronts / build / append / model_read: the acquisition model built on the device
