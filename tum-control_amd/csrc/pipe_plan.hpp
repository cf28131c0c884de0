// pipe_plan.hpp -- WHICH kernel of every pipeline stage a solve launches: the decision, apart from the launching.
// plan_pipeline() is a pure function of the facts in PlanIn; tum_nmpc.hip: launch_pipeline fills them in from the capsule, asks once
// and launches what the plan names. Nothing of HIP in here: tests/host/pipe_plan_check.cpp builds this header with a plain host
// compiler, enumerates the whole input space and checks that no plan reads stage records (drec) that were not written.
#pragma once

namespace tum {

constexpr int LC_LANES = 8;          // lanes lin_cols_kernel spreads one (instance, stage) over (pipe_kernels.hpp)

// tum_ocp_set_kernel / TUM_NMPC_KERNEL: auto is the pipeline; FUSED (round 1's one-kernel solve) and PIPELINE4 (the pipeline with the
// four-wavefront interior point kernel) exist in the development build only
enum class KMode : int { AUTO = 0, FUSED = 1, PIPELINE = 2, PIPELINE4 = 3 };
// PREPARE: linearisation and condensing; FEEDBACK: interior point method and expansion; WHOLE: an SQP-RTI step. (A full SQP solve puts
// its residual pass between the two, the split real-time iteration its feedback kernel in front of the second.)
enum class Part : int { PREPARE = 1, FEEDBACK = 2, WHOLE = 3 };

// integer switches of the environment (include/tum_nmpc.h lists them), -1: the library's choice. A capsule's own word
// (tum_ocp_set_kernel) goes first.
struct PlanEnv { int lin_cols = -1, cond_wide = -1, sim_fork = -1, fused_expand = -1; };

struct PlanIn {
    int N = 0, tiles = 5, batch = 0;          // horizon, MFMA tiles of the instantiation (5: N <= 40, 6: <= 48, 7: <= 56), instances
    bool sn = false; int uph = 0;             // coupled SNMPC OCP, its uncertainty propagation horizon
    bool full_w = false, store_qp_in = false; // W with off-diagonal entries; the capsule serves get_from_qp_in / the R2 back-off from drec
    bool debug = false, prof = false;         // KF_DEBUG, KF_PROF
    KMode kmode = KMode::AUTO;
    int lin_cols = -1, cond_wide = -1, sim_fork = -1;          // the capsule's overrides: -1 the library's choice, 0 never, 1 always
    PlanEnv env;
    bool iter_uniform = false, lin_dedup = true, uniform_records = false, capturing = false;
    int nlp_type = 0;                         // 1: a full SQP solve (its residual pass reads drec)
    bool ran_ahead = false;                   // launch_lin_ahead has run this solve's linearisation on another stream
    Part part = Part::WHOLE;
    bool uniform_powers = true;               // options_set "uniform_powers": which body condenses a stage-uniform iterate without records
};

// NONE: the stage is not part of this call (or, Lin: it ran ahead; Expand: it is the tail of the interior point kernel)
enum class Lin { NONE, LANE, COLS, UNIFORM_FILL, UNIFORM, SN_LANE, SN_COLS };          // SN_*: behind the sample linearisation and the prologue
enum class Cond { NONE, ONE_WAVE, ONE_WAVE_UNIFORM, WIDE, WIDE_FULLW, SN_REGISTER, SN_LDS, SN_WIDE };
enum class Ipm { NONE, PLAIN, FUSED_TAIL, INSTRUMENTED, FOUR_WAVE };
enum class Expand { NONE, RECORDS, UNIFORM, SN_RECORDS };          // SN_RECORDS: behind the epilogue

struct PipePlan {
    Lin lin = Lin::NONE; Cond cond = Cond::NONE; Ipm ipm = Ipm::NONE; Expand expand = Expand::NONE;
    bool records_written = true;          // drec holds this linearisation's records for whoever reads it, in this call or behind it
    bool lin_ahead_flag = false;          // KF_LIN_AHEAD for the condensing kernel: it forms the residuals of the cost itself
    // Cond::ONE_WAVE_UNIFORM only: cond_uniform_kernel (the sequences A^m B and g_s once per instance, the stages read them) or
    // cond_uniform_columns_kernel (every lane carries its column through every stage); the same hand-over, to the bit
    bool cond_powers = true;
};

// who reads drec (the CPU check holds every plan against this)
constexpr bool reads_records(Cond k) { return k != Cond::NONE && k != Cond::ONE_WAVE_UNIFORM; }
constexpr bool reads_records(Ipm k) { return k == Ipm::FUSED_TAIL; }
constexpr bool reads_records(Expand k) { return k == Expand::RECORDS || k == Expand::SN_RECORDS; }

inline PipePlan plan_pipeline(const PlanIn &in)
{
    const bool prepare = in.part != Part::FEEDBACK, feedback = in.part != Part::PREPARE;
    // The wide kernels of the latency path. Linearisation: eight lanes per (instance, stage) while that still is one round of
    // wavefronts on the chip (256 CUs x 4 SIMDs). Condensing: six wavefronts per OCP while every OCP can have a CU's LDS to itself;
    // a full W exists as an instantiation of that kernel only; never at seven tiles (its row store does not fit a CU's LDS there).
    const int want_cols = in.lin_cols >= 0 ? in.lin_cols : in.env.lin_cols;
    const bool cols = want_cols > 0 || (want_cols < 0 && (long long)in.batch * (in.N + 1) * LC_LANES <= 64LL * 1024);
    const int want_wide = in.cond_wide >= 0 ? in.cond_wide : in.env.cond_wide;
    const bool wide = in.tiles != 7 && (want_wide > 0 || (want_wide < 0 && in.batch <= 256) || in.full_w);
    // The expansion as the tail of the interior point kernel pays where a batch is at most one round of resident wavefronts (one
    // launch less: 0.424 against 0.432 ms per solve() call at 26 instances, 0.457 against 0.469 at 1024); beyond that its
    // loads run at the interior point kernel's occupancy -- one wavefront per SIMD, four OCPs per CU -- and hold that slot:
    // 3.72 against 3.96 M solves/s on config 2 (three streams). TUM_FUSED_EXPAND=0 / 1 forces it off / on (development aid).
    const bool tail_wanted = in.env.fused_expand > 0 || (in.env.fused_expand < 0 && in.batch <= 1024);
    // The uniform linearisation replaces lin_kernel<false> only: the nominal OCP beyond the latency path, and never inside the capture
    // of a closed-loop chunk (a captured launch is replayed on iterates that are uniform no more).
    const bool lin_uniform = !in.ran_ahead && !in.sn && !cols && in.iter_uniform && in.lin_dedup && !in.capturing;
    // The record-free chain of a stage-uniform iterate: lin_uniform_kernel, cond_uniform_kernel, ipm_kernel, expand_uniform_kernel --
    // drec is not written. Every stage must have its uniform form (one wavefront per OCP in the condensing, a diagonal W, the
    // expansion a kernel of its own behind the pipeline's own interior point kernel) and nobody else may read drec: the residual pass
    // of an SQP solve, the feedback kernel of the split iteration or the other half of a split call, get_from_qp_in and the R2 back-off
    // (store_qp_in), the instrumented kernels.
    const bool record_free = lin_uniform && in.part == Part::WHOLE && !in.uniform_records && in.nlp_type == 0 && !in.full_w && !in.store_qp_in &&
                             !in.debug && !in.prof && !tail_wanted && !wide && in.kmode != KMode::PIPELINE4;
    PipePlan p;
    p.records_written = !record_free;
    if (prepare) {
        if (in.ran_ahead) p.lin_ahead_flag = true;
        else if (in.sn) p.lin = cols ? Lin::SN_COLS : Lin::SN_LANE;
        else if (cols) p.lin = Lin::COLS;
        else if (lin_uniform) p.lin = record_free ? Lin::UNIFORM : Lin::UNIFORM_FILL;
        else p.lin = Lin::LANE;

        if (wide) p.cond = in.sn ? Cond::SN_WIDE : (in.full_w ? Cond::WIDE_FULLW : Cond::WIDE);
        // (coupled SNMPC: the register form of the stage record pays behind stage uph and costs in front of it, pipe_kernels.hpp)
        else if (in.sn) p.cond = 2 * in.uph <= in.N ? Cond::SN_REGISTER : Cond::SN_LDS;
        else p.cond = record_free ? Cond::ONE_WAVE_UNIFORM : Cond::ONE_WAVE;
        p.cond_powers = in.uniform_powers;
    }
    if (feedback) {
        // the four-wavefront kernel and the instrumented instantiation exist for the five-tile build only: other tile counts get the
        // plain kernel. The fused tail: the nominal OCP only (SN keeps the expansion kernel behind its epilogue), never at seven tiles.
        if (in.kmode == KMode::PIPELINE4 && in.tiles == 5) p.ipm = Ipm::FOUR_WAVE;
        else if (in.prof && in.tiles == 5) p.ipm = Ipm::INSTRUMENTED;
        else if (in.sn || in.tiles == 7 || !tail_wanted) p.ipm = Ipm::PLAIN;
        else p.ipm = Ipm::FUSED_TAIL;

        if (in.sn) p.expand = Expand::SN_RECORDS;
        else if (record_free) p.expand = Expand::UNIFORM;
        else if (p.ipm != Ipm::FUSED_TAIL) p.expand = Expand::RECORDS;
    }
    return p;
}

// The device closed loop (tum_sim_run) can run the linearisation of a solve BESIDE the planner of the same control step: the
// Runge-Kutta pass needs the iterate, not the reference -- only the four residuals of the cost do, and cond_wide_kernel forms those
// while it loads the records (KF_LIN_AHEAD). Nominal OCP on the latency path only (lin_cols_kernel + cond_wide_kernel).
// (off unless asked for: measured SLOWER -- 0.169 against 0.160 ms per control step at 26 vehicles, 0.158-0.162 against 0.156 at one:
//  the two cross-stream dependencies of a step cost more than the 15 us of planner the linearisation hides behind; HISTORY.md (round-4 document, section 7))
// `in`: the whole step as launch_pipeline would be asked for it, nothing run ahead yet
inline bool plan_lin_ahead(const PlanIn &in)
{
    const int want = in.sim_fork >= 0 ? in.sim_fork : in.env.sim_fork;
    if (want <= 0 || in.sn || in.debug || in.prof) return false;
    const PipePlan p = plan_pipeline(in);
    return p.lin == Lin::COLS && (p.cond == Cond::WIDE || p.cond == Cond::WIDE_FULLW);
}

}  // namespace tum
