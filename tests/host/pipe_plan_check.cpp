// pipe_plan_check.cpp -- plan_pipeline (csrc/pipe_plan.hpp) over its whole input space, on the CPU.
// Built by tests/test_pipe_plan.py with the host compiler and -fsanitize=address,undefined and run as a child process.
// Exit code 0: every invariant holds for every input and every named case gives the kernels listed; otherwise the first
// failures are printed and the exit code is 1.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "pipe_plan.hpp"

using namespace tum;

// (the checks that copy a PlanIn stay out of check(): its frame is set up 25 million times under the address sanitizer)
#define NOINLINE __attribute__((noinline))

static long long n_checked = 0;
static int n_failed = 0;

static void describe(const PlanIn &in, const PipePlan &p)
{
    std::printf("    N %d tiles %d batch %d sn %d uph %d fullW %d qp_in %d debug %d prof %d kmode %d overrides %d %d %d env %d %d %d %d "
                "uniform %d dedup %d urec %d capturing %d nlp %d ahead %d part %d -> lin %d cond %d ipm %d expand %d records %d flag %d\n",
                in.N, in.tiles, in.batch, in.sn, in.uph, in.full_w, in.store_qp_in, in.debug, in.prof, (int)in.kmode, in.lin_cols, in.cond_wide,
                in.sim_fork, in.env.lin_cols, in.env.cond_wide, in.env.sim_fork, in.env.fused_expand, in.iter_uniform, in.lin_dedup,
                in.uniform_records, in.capturing, in.nlp_type, in.ran_ahead, (int)in.part, (int)p.lin, (int)p.cond, (int)p.ipm, (int)p.expand,
                p.records_written, p.lin_ahead_flag);
}
static void failed(const char *what, const PlanIn &in, const PipePlan &p)
{
    if (n_failed++ < 20) { std::printf("FAILED: %s\n", what); describe(in, p); }
}
#define expect(ok, what, in, p) do { if (!(ok)) failed(what, in, p); } while (0)
static bool same(const PipePlan &a, const PipePlan &b)
{
    return a.lin == b.lin && a.cond == b.cond && a.ipm == b.ipm && a.expand == b.expand && a.records_written == b.records_written &&
           a.lin_ahead_flag == b.lin_ahead_flag;
}
static bool uniform_stage(const PipePlan &p)
{
    return p.lin == Lin::UNIFORM || p.lin == Lin::UNIFORM_FILL || p.cond == Cond::ONE_WAVE_UNIFORM || p.expand == Expand::UNIFORM;
}

// PART 2: a FEEDBACK does not depend on ran-ahead, on the linearisation / condensing overrides or on what the iterate looks like
NOINLINE static void check_feedback(const PlanIn &in, const PipePlan &p)
{
    PlanIn o = in;
    o.ran_ahead = false; o.lin_cols = o.cond_wide = o.sim_fork = -1; o.env.lin_cols = o.env.cond_wide = o.env.sim_fork = -1;
    o.iter_uniform = false; o.lin_dedup = true; o.uniform_records = false; o.capturing = false;
    expect(same(p, plan_pipeline(o)), "a FEEDBACK plan depends on ran-ahead, a linearisation override or the iterate's uniformity", in, p);
}
// the capsule's word goes before the environment's
NOINLINE static void check_precedence(const PlanIn &in, const PipePlan &p)
{
    PlanIn o = in;
    if (in.lin_cols >= 0) o.env.lin_cols = -1;
    if (in.cond_wide >= 0) o.env.cond_wide = -1;
    expect(same(p, plan_pipeline(o)), "the environment overrides a word of the capsule", in, p);
}
// the linearisation beside the planner: only where it was asked for, and only in front of the kernels that can take it
NOINLINE static void check_lin_ahead(const PlanIn &in, const PipePlan &p)
{
    if (!plan_lin_ahead(in)) return;
    PlanIn o = in; o.ran_ahead = true;
    const PipePlan q = plan_pipeline(o);
    expect(p.lin == Lin::COLS && !in.sn && !in.debug && !in.prof && (in.sim_fork > 0 || (in.sim_fork < 0 && in.env.sim_fork > 0)),
           "lin-ahead: asked for, the nominal OCP on lin_cols_kernel, no debug bits", in, p);
    expect(q.lin_ahead_flag && (q.cond == Cond::WIDE || q.cond == Cond::WIDE_FULLW) && q.records_written, "lin-ahead: cond_wide_kernel consumes it", o, q);
}

static void check(const PlanIn &in)
{
    const PipePlan p = plan_pipeline(in);
    n_checked++;
    const bool prepare = in.part != Part::FEEDBACK, feedback = in.part != Part::PREPARE;
    // the parts: a stage is planned exactly where its part is asked for (the linearisation may have run ahead instead)
    expect((p.cond != Cond::NONE) == prepare, "condensing planned with PREPARE / WHOLE and only there", in, p);
    expect((p.ipm != Ipm::NONE) == feedback, "interior point method planned with FEEDBACK / WHOLE and only there", in, p);
    expect(prepare || (p.lin == Lin::NONE && !p.lin_ahead_flag), "a FEEDBACK has no linearisation", in, p);
    expect(feedback || p.expand == Expand::NONE, "a PREPARE has no expansion", in, p);
    expect(!prepare || (p.lin == Lin::NONE) == in.ran_ahead, "no linearisation kernel exactly where it ran ahead", in, p);
    expect(p.lin_ahead_flag == (prepare && in.ran_ahead), "the condensing kernel is told exactly where the linearisation ran ahead", in, p);
    expect(!feedback || in.sn || (p.expand == Expand::NONE) == (p.ipm == Ipm::FUSED_TAIL), "the nominal OCP is expanded once: by the tail or by a kernel", in, p);

    // RECORDS: whoever reads drec finds it written
    expect(!(reads_records(p.cond) || reads_records(p.ipm) || reads_records(p.expand)) || p.records_written, "a planned kernel reads records that were not written", in, p);
    expect(in.part == Part::WHOLE || p.records_written, "half a solve: the other half, the residual pass or the feedback kernel reads the records", in, p);
    expect(!in.store_qp_in || p.records_written, "store_qp_in: get_from_qp_in and the R2 back-off read the records", in, p);
    expect(in.nlp_type == 0 || p.records_written, "SQP: the residual pass reads the records", in, p);
    expect(!(in.debug || in.prof) || p.records_written, "the instrumented kernels read the records", in, p);
    expect(!in.ran_ahead || p.records_written, "a linearisation that ran ahead wrote the records", in, p);
    expect(p.lin != Lin::UNIFORM || (p.cond == Cond::ONE_WAVE_UNIFORM && p.expand == Expand::UNIFORM && in.part == Part::WHOLE),
           "the linearisation goes without the fill only in the record-free chain of a whole step", in, p);
    expect(p.records_written == !(p.lin == Lin::UNIFORM), "records are written by every linearisation but the uniform one without fill", in, p);
    expect((p.cond == Cond::ONE_WAVE_UNIFORM || p.expand == Expand::UNIFORM) ? p.lin == Lin::UNIFORM : true, "the uniform condensing / expansion take lin1 of THIS solve's uniform linearisation", in, p);
    expect((p.lin == Lin::UNIFORM || p.lin == Lin::UNIFORM_FILL) ? (in.iter_uniform && in.lin_dedup) : true, "the uniform linearisation needs a stage-uniform iterate and lin_dedup", in, p);

    // TILES
    const bool wide = p.cond == Cond::WIDE || p.cond == Cond::WIDE_FULLW || p.cond == Cond::SN_WIDE;
    expect(in.tiles != 7 || (!wide && p.ipm != Ipm::FUSED_TAIL), "seven tiles: never wide, never the fused tail", in, p);
    expect(in.tiles == 5 || (p.ipm != Ipm::INSTRUMENTED && p.ipm != Ipm::FOUR_WAVE), "the instrumented and the four-wavefront kernel exist at five tiles only", in, p);
    expect(p.ipm != Ipm::FOUR_WAVE || in.kmode == KMode::PIPELINE4, "the four-wavefront kernel only where it was asked for", in, p);
    expect(p.ipm != Ipm::INSTRUMENTED || in.prof, "the instrumented kernel only with the phase timers", in, p);

    // SN and full W
    if (in.sn) {
        expect(!uniform_stage(p), "SN never takes a uniform stage", in, p);
        expect(!feedback || p.expand == Expand::SN_RECORDS, "SN always has a separate expansion, behind its epilogue", in, p);
        expect(p.ipm != Ipm::FUSED_TAIL, "SN never takes the fused tail", in, p);
        expect(!prepare || wide || (p.cond == Cond::SN_REGISTER) == (2 * in.uph <= in.N), "SN: the register form if and only if 2 uph <= N", in, p);
        expect(!prepare || p.cond == Cond::SN_REGISTER || p.cond == Cond::SN_LDS || p.cond == Cond::SN_WIDE, "SN condenses with its own instantiations", in, p);
        expect(!prepare || in.ran_ahead || p.lin == Lin::SN_LANE || p.lin == Lin::SN_COLS, "SN linearises with its own instantiations", in, p);
    } else {
        expect(p.lin != Lin::SN_LANE && p.lin != Lin::SN_COLS && p.cond != Cond::SN_REGISTER && p.cond != Cond::SN_LDS && p.cond != Cond::SN_WIDE &&
               p.expand != Expand::SN_RECORDS, "the nominal OCP takes no SN instantiation", in, p);
        // (a capsule with a full W is refused by snmpc_attach: the nominal OCP only)
        expect(!(prepare && in.full_w && in.tiles != 7) || p.cond == Cond::WIDE_FULLW, "a full W (tiles != 7) always takes wide-fullW", in, p);
        expect(p.cond != Cond::WIDE_FULLW || in.full_w, "wide-fullW only for a full W", in, p);
    }

    expect(!in.capturing || !uniform_stage(p), "capturing never yields a uniform stage", in, p);
    if (in.part == Part::FEEDBACK) check_feedback(in, p);
    if ((in.lin_cols >= 0 && in.env.lin_cols >= 0) || (in.cond_wide >= 0 && in.env.cond_wide >= 0)) check_precedence(in, p);
    if (in.part == Part::WHOLE && !in.ran_ahead && (in.sim_fork > 0 || in.env.sim_fork > 0)) check_lin_ahead(in, p);
}

static void enumerate()
{
    const int shapes[3][2] = {{40, 5}, {48, 6}, {56, 7}};          // (N, tiles)
    const int batches[] = {1, 199, 200, 256, 257, 1024, 1025, 4096};
    const int tri[] = {-1, 0, 1};
    // the whole product, the overrides as the capsule's words
    PlanIn in;
    for (const auto &sh : shapes)
    for (int batch : batches)
    for (int snm = 0; snm < 3; snm++)          // nominal, SN with 2 uph <= N, SN with 2 uph > N
    for (int bits = 0; bits < 16; bits++)      // full W, store_qp_in, debug, prof
    for (int km = 0; km < 4; km++)
    for (int lc : tri) for (int cw : tri) for (int efe : tri)
    for (int ub = 0; ub < 16; ub++)            // iter_uniform, lin_dedup, uniform_records, capturing
    for (int nlp = 0; nlp < 2; nlp++)
    for (int ahead = 0; ahead < 2; ahead++)
    for (Part part : {Part::PREPARE, Part::FEEDBACK, Part::WHOLE}) {
        in.N = sh[0]; in.tiles = sh[1]; in.batch = batch;
        in.sn = snm != 0; in.uph = snm == 0 ? 0 : (snm == 1 ? 5 : in.N - 2);
        in.full_w = bits & 1; in.store_qp_in = bits & 2; in.debug = bits & 4; in.prof = bits & 8;
        in.kmode = (KMode)km;
        in.lin_cols = lc; in.cond_wide = cw; in.env.fused_expand = efe;
        in.iter_uniform = ub & 1; in.lin_dedup = ub & 2; in.uniform_records = ub & 4; in.capturing = ub & 8;
        in.nlp_type = nlp; in.ran_ahead = ahead; in.part = part;
        check(in);
    }
    // (capsule, environment) of an override: each alone at -1 / 0 / 1, and every word of the one against every word of the other;
    // with them the fork beside the planner and a forced larger instantiation (TUM_FORCE_TILES) at N = 40
    const int words[9][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {-1, 1}, {0, 1}, {1, 0}, {0, 0}, {1, 1}};
    for (int tiles : {5, 6, 7}) for (int batch : batches) for (const auto &sf : words) for (const auto &lc : words) for (const auto &cw : words)
    for (int bits = 0; bits < 16; bits++)      // full W, prof, SN, iter_uniform
    for (Part part : {Part::PREPARE, Part::FEEDBACK, Part::WHOLE}) {
        PlanIn f;
        f.N = 40; f.tiles = tiles; f.batch = batch; f.sim_fork = sf[0]; f.env.sim_fork = sf[1];
        f.lin_cols = lc[0]; f.env.lin_cols = lc[1]; f.cond_wide = cw[0]; f.env.cond_wide = cw[1];
        f.full_w = bits & 1; f.prof = bits & 2; f.sn = bits & 4; f.uph = 5; f.iter_uniform = bits & 8; f.part = part;
        check(f);
    }
}

// ---- named cases, read off launch_pipeline as it stood before the plan was separated from it. Defaults: no environment override,
// kernel mode auto, diagonal W, flags 0.
static PlanIn nominal(int batch, int N, bool uniform)
{
    PlanIn in;
    in.N = N; in.tiles = N > 48 ? 7 : (N > 40 ? 6 : 5); in.batch = batch; in.iter_uniform = uniform;
    return in;
}
static void named(const char *name, const PlanIn &in, Lin lin, Cond cond, Ipm ipm, Expand expand, bool records, bool flag = false)
{
    const PipePlan p = plan_pipeline(in);
    n_checked++;
    const bool ok = p.lin == lin && p.cond == cond && p.ipm == ipm && p.expand == expand && p.records_written == records && p.lin_ahead_flag == flag;
    if (!ok) {
        std::printf("expected lin %d cond %d ipm %d expand %d records %d flag %d\n", (int)lin, (int)cond, (int)ipm, (int)expand, records, flag);
        expect(false, name, in, p);
    }
}
static void named_cases()
{
    PlanIn in = nominal(4096, 40, true);
    named("4096 x 40, uniform, whole", in, Lin::UNIFORM, Cond::ONE_WAVE_UNIFORM, Ipm::PLAIN, Expand::UNIFORM, false);
    in.uniform_records = true;
    named("4096 x 40, uniform, uniform_records 1", in, Lin::UNIFORM_FILL, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
    named("4096 x 40, iterate not uniform", nominal(4096, 40, false), Lin::LANE, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
    in = nominal(4096, 40, true); in.store_qp_in = true;
    named("4096 x 40, uniform, store_qp_in", in, Lin::UNIFORM_FILL, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
    in = nominal(4096, 40, true); in.part = Part::PREPARE;
    named("4096 x 40, uniform, part 1", in, Lin::UNIFORM_FILL, Cond::ONE_WAVE, Ipm::NONE, Expand::NONE, true);
    in.part = Part::FEEDBACK;
    named("4096 x 40, uniform, part 2", in, Lin::NONE, Cond::NONE, Ipm::PLAIN, Expand::RECORDS, true);
    in = nominal(4096, 40, true); in.nlp_type = 1;
    named("4096 x 40, uniform, nlp_type 1", in, Lin::UNIFORM_FILL, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
    for (bool uniform : {false, true})
        named("26 x 40 (any iterate)", nominal(26, 40, uniform), Lin::COLS, Cond::WIDE, Ipm::FUSED_TAIL, Expand::NONE, true);
    named("199 x 40, not uniform", nominal(199, 40, false), Lin::COLS, Cond::WIDE, Ipm::FUSED_TAIL, Expand::NONE, true);
    named("200 x 40, not uniform", nominal(200, 40, false), Lin::LANE, Cond::WIDE, Ipm::FUSED_TAIL, Expand::NONE, true);
    named("512 x 40, uniform", nominal(512, 40, true), Lin::UNIFORM_FILL, Cond::ONE_WAVE, Ipm::FUSED_TAIL, Expand::NONE, true);
    named("1025 x 40, uniform", nominal(1025, 40, true), Lin::UNIFORM, Cond::ONE_WAVE_UNIFORM, Ipm::PLAIN, Expand::UNIFORM, false);
    in = nominal(26, 40, false); in.prof = true;
    named("26 x 40, prof bit", in, Lin::COLS, Cond::WIDE, Ipm::INSTRUMENTED, Expand::RECORDS, true);
    in = nominal(26, 40, false); in.ran_ahead = true;
    named("26 x 40, ran ahead", in, Lin::NONE, Cond::WIDE, Ipm::FUSED_TAIL, Expand::NONE, true, true);
    in = nominal(4096, 40, false); in.full_w = true;
    named("4096 x 40, full W", in, Lin::LANE, Cond::WIDE_FULLW, Ipm::PLAIN, Expand::RECORDS, true);
    in.iter_uniform = true;
    named("4096 x 40, full W, uniform", in, Lin::UNIFORM_FILL, Cond::WIDE_FULLW, Ipm::PLAIN, Expand::RECORDS, true);
    named("26 x 50", nominal(26, 50, false), Lin::COLS, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
    named("4096 x 50, uniform", nominal(4096, 50, true), Lin::UNIFORM, Cond::ONE_WAVE_UNIFORM, Ipm::PLAIN, Expand::UNIFORM, false);
    in = nominal(4096, 38, true); in.sn = true; in.uph = 5;
    named("SN 4096 x 38, uph 5", in, Lin::SN_LANE, Cond::SN_REGISTER, Ipm::PLAIN, Expand::SN_RECORDS, true);
    in.uph = 38;
    named("SN 4096 x 38, uph 38", in, Lin::SN_LANE, Cond::SN_LDS, Ipm::PLAIN, Expand::SN_RECORDS, true);
    in = nominal(26, 38, false); in.sn = true; in.uph = 5;
    named("SN 26 x 38", in, Lin::SN_COLS, Cond::SN_WIDE, Ipm::PLAIN, Expand::SN_RECORDS, true);
    in = nominal(4096, 40, true); in.capturing = true;
    named("4096 x 40, uniform, capturing", in, Lin::LANE, Cond::ONE_WAVE, Ipm::PLAIN, Expand::RECORDS, true);
}

int main()
{
    named_cases();
    enumerate();
    std::printf("pipe_plan_check: %lld plans checked, %d failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
