// sqp_kernels.hpp -- the kernels a full SQP solve adds around the unchanged SQP-RTI pipeline (tum_nmpc.hip: launch_sqp).
//
// One SQP iteration is   [lin, cond] -> nlp_residual_kernel -> sqp_snapshot_kernel -> [ipm, expand] -> sqp_commit_kernel
// (globalization MERIT_BACKTRACKING: sqp_merit_kernel between the expansion and the commit chooses every instance's step length)
// and behind the last QP one more [lin, cond] -> nlp_residual_kernel describes the iterate the solve returns (acados' order:
// linearise, evaluate the residuals, test for termination, then solve the QP). The kernels of the pipeline are the RTI's own,
// launched with the RTI's arguments: instances that have converged or failed ride along and are put back by the commit kernel.
//
// Per instance the SQP state is 0 (active), 1 (converged) or 2 (a QP failed; the iterate stays at the last good one).
#pragma once
#include "pipe_kernels.hpp"

namespace tum {

struct SqpArgs {
    double *res_nlp;        // [b][4]  stat, eq, ineq, comp of the iterate
    int *state;             // [b]     0 active, 1 converged, 2 QP failed
    int *sqp_iter;          // [b]     QPs solved by this instance
    unsigned *active;       // [max_iter + 1]  instances still active behind each residual pass
    double *snap;           // [b][snap_len]   X | U | qp_lam | slack | cost | res (the QP's) in front of the QP
    int *snapi;             // [b][3]          status | qp_iter | qp_status
    int snap_len;
    double tol_stat, tol_eq, tol_ineq, tol_comp;
    double alpha;           // step length (nlp_solver_step_length)
    int pass;               // which counter of `active` this residual pass adds to
    int last;               // 1: no QP follows this pass (iteration cap): the instances still active end with status 2
    int cost;               // 1: the cost of the iterate is evaluated here (alpha != 1: the expansion's is that of the full step; pass 0
                            //    of a cold-started solve: an instance that converges there has no expansion)
};

// globalization MERIT_BACKTRACKING: what sqp_merit_kernel reads and writes beside the SQP state
constexpr int MERIT_KMAX = 16;          // candidates alpha_j = alpha_reduction^j, j < K <= MERIT_KMAX
struct MeritArgs {
    double *alpha;          // [b]              step length the line search of this iteration accepted (null: FIXED_STEP)
    double *mu_in;          // [b]              weight of the row violations: largest |multiplier| of the QPs of this solve so far
    double *table;          // [b][K + 1][3]    cost, E, V at the candidates j = 0 .. K - 1 and (row K) at alpha = 0, of the instance's last line search
    double *hist;           // [b][hist_len]    accepted alpha of the QPs 1 .. sqp_iter (a failed QP leaves its 0)
    int K, hist_len;
    double mu_eq;           // weight of the shooting defects (merit_weight_eq)
    double cand[MERIT_KMAX];
};

// Residuals of the NLP at the current iterate, with the multipliers of the previous QP, in the condensed form the pipeline
// builds (one wavefront per instance):
//   stat  | q - C'(lam_l - lam_u) |_inf over the inputs, where q is the condensing kernel's gradient and C the rows of the QP --
//         steering-rate boxes (1 on column 2k+1), steering-angle rows (dt on the columns 2j+1, j < s) and the gg rows of cws --,
//         and the stationarity in the slacks, z + Z s - lam - mu = 0 with mu >= 0 the multiplier of s >= 0: what is left of it
//         is max(lam - z - Z s, 0). The rows of the states vanish: condensing eliminates dx, i.e. the multipliers of the
//         dynamics are those the backward recursion recovers, which make the state part of the Lagrangian's gradient zero.
//   eq    | x0 - X_0 |_inf and the defects f(x_k, u_k) - x_{k+1} of the stage records
//   ineq  the largest violation of a row side beyond its slack (row values at the iterate, not the QP's linear prediction)
//   comp  the largest lam t (t: the row side's margin plus its slack) and mu s over the row sides
template <int NT_>
__global__ void __launch_bounds__(64) nlp_residual_kernel(const PArgs pa, const SqpArgs sq)
{
    PD_LOCALS
    __shared__ double sW[3][NMAX + 1];      // lam_l - lam_u per row type (box: stage k, steering angle / gg: stage s)
    __shared__ double sPart[4][NVP];        // gg part of C'w per DPP row of the operand layout
    __shared__ double sCost[64];
    const KArgs &ka = pa.ka;
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= ka.batch) return;
    const int N = ka.N, nv = 2 * N, NB = N + 1;
    const double dt = ka.dt;
    const double *grec = pa.rec + (size_t)b * NB * PREC;
    const double *glm = ka.qp_lam + (size_t)b * (6 * N + 2);
    const double *gsl = ka.slack + (size_t)b * 6 * N;
    const double *gbnd = ka.bnd + (size_t)b * 6 * NB;
    const double *gpen = ka.pen + (size_t)b * 36;
    const double *gU = ka.U + (size_t)b * N * NU, *gX = ka.X + (size_t)b * NB * NX, *gx0 = ka.x0 + (size_t)b * NX;
    const double *gvec = pa.vec + (size_t)b * PVEC;

    double rs = 0.0, re = 0.0, ri = 0.0, rc = 0.0, cl = 0.0;
    for (int k = lane; k < N; k += 64) {
#pragma unroll
        for (int ty = 0; ty < 3; ty++) {
            // row type 0: steering-rate box of stage k; 1: steering angle of stage k + 1; 2: gg row of stage k + 1
            const int st = (ty == 0) ? k : k + 1;
            const int idx = (ty == 0) ? k : N + 2 * k + ((ty == 2) ? 1 : 0);          // (layout of `slack` / `qp_lam`)
            const double val = (ty == 0) ? gU[2 * k + 1] : grec[(size_t)st * PREC + ((ty == 1) ? PR_XD : PR_GH + 3)];
            const double lo = gbnd[(2 * ty) * NB + st], hi = gbnd[(2 * ty + 1) * NB + st];
            const int pc = (ty == 0) ? ((k == 0) ? 0 : 1) : ((st < N) ? 1 : 2);          // penalty class
            const double sc = (ty == 0 || st < N) ? dt : 1.0;
            double w = 0.0;
#pragma unroll
            for (int sd = 0; sd < 2; sd++) {
                const double lam = glm[sd * 3 * N + idx], s = gsl[sd * 3 * N + idx];
                const double z = sc * gpen[(pc * 3 + ty) * 4 + sd], Z = sc * gpen[(pc * 3 + ty) * 4 + 2 + sd];
                const double t = sd ? hi - val + s : val - lo + s;
                const double m = z + Z * s - lam;
                ri = fmax(ri, -t);
                rs = fmax(rs, -m);
                rc = fmax(rc, fmax(fabs(lam * t), fmax(m, 0.0) * fabs(s)));
                w += sd ? -lam : lam;
                cl += z * s + 0.5 * Z * s * s;
            }
            sW[ty][st] = w;
        }
#pragma unroll
        for (int i = 0; i < NX; i++) re = fmax(re, fabs(grec[(size_t)k * PREC + 44 + i]));
    }
    if (lane < NX) re = fmax(re, fabs(gx0[lane] - gX[lane]));
    wsync();
    // the gg rows: chunk c of the operand layout holds the rows 4c+1..4c+4 (DPP row lq of the wavefront: row 4c+lq+1), tile T
    // the columns 16T..16T+15 (lane column lc); only the chunks c >= 2T are stored, the rest of a row is zero
    {
        const int lq = lane >> 4, lc = lane & 15;
        const double *gcw = pa.cws + (size_t)b * NCH * 64 + lane;
#pragma unroll
        for (int T = 0; T < NT; T++) {
            double acc = 0.0;
#pragma unroll
            for (int c = 2 * T; c < NC; c++) {
                const int s = 4 * c + lq + 1;
                if (s <= N) acc += gcw[cidx(c, T) * 64] * sW[2][s];
            }
            sPart[lq][16 * T + lc] = acc;
        }
    }
    wsync();
    for (int j = lane; j < nv; j += 64) {
        double ct = sPart[0][j] + sPart[1][j] + sPart[2][j] + sPart[3][j];
        if (j & 1) {
            const int k = j >> 1;
            double sfx = 0.0;
            for (int s = k + 1; s <= N; s++) sfx += sW[1][s];
            ct += sW[0][k] + dt * sfx;
        }
        rs = fmax(rs, fabs(gvec[PV_Q + j] - ct));
    }
    if (sq.cost) {
        // least-squares cost of the iterate (the stage records hold its state residuals) plus the slack cost above
        for (int k = lane; k <= N; k += 64) {
            const double *yr = ka.yref + ((size_t)b * NB + k) * 6;
            double rr[6];
#pragma unroll
            for (int i = 0; i < 4; i++) rr[i] = grec[(size_t)k * PREC + PR_RES + i];
            rr[4] = (k < N) ? gU[2 * k] - yr[4] : 0.0; rr[5] = (k < N) ? gU[2 * k + 1] - yr[5] : 0.0;
            const int ny = (k < N) ? 6 : 4;
            double acc = 0.0;
            if (ka.Wf) {
                const double *Wk = ka.Wf + ((size_t)b * NB + k) * 36;
                for (int i = 0; i < ny; i++)
                    for (int i2 = 0; i2 < ny; i2++) acc += Wk[i * 6 + i2] * rr[i] * rr[i2];
            } else {
                const double *Wd = ka.W + ((size_t)b * NB + k) * 6;
                for (int i = 0; i < ny; i++) acc += Wd[i] * rr[i] * rr[i];
            }
            cl += 0.5 * ((k < N) ? dt : 1.0) * acc;
        }
        sCost[lane] = cl;
        wsync();
        if (lane == 0) {
            double sum = 0.0;
            for (int i = 0; i < 64; i++) sum += sCost[i];
            ka.cost[b] = sum;
        }
    }
    rs = wave_max(rs); re = wave_max(re); ri = wave_max(ri); rc = wave_max(rc);
    if (lane == 0) {
        double *o = sq.res_nlp + (size_t)b * 4;
        o[0] = rs; o[1] = re; o[2] = ri; o[3] = rc;
        int st = sq.state[b];
        if (st == 0) {
            // (acados' test: every residual strictly below its tolerance; all tolerances 0 never converge)
            if (rs < sq.tol_stat && re < sq.tol_eq && ri < sq.tol_ineq && rc < sq.tol_comp) { st = 1; sq.state[b] = 1; ka.status[b] = 0; }
            else if (sq.last) ka.status[b] = 2;          // ACADOS_MAXITER
        }
        if (st == 0) atomicAdd(sq.active + sq.pass, 1u);
    }
}

// One shooting interval without sensitivities: the state part of rk4_sens (nmpc_device.hpp), operation for operation.
__device__ __forceinline__ void rk4_state(const Model &p, const double x0[8], const double u[2], double dt, int nsub, double xn[8])
{
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = x0[i];
    const double h = dt / nsub;
    for (int sub = 0; sub < nsub; sub++) {
        double xacc[6], kp[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { xacc[i] = 0.0; kp[i] = 0.0; }
#pragma unroll 1
        for (int st = 0; st < 4; st++) {
            const double ci = (st == 0) ? 0.0 : (st == 3 ? 1.0 : 0.5);
            const double bi = (st == 0 || st == 3) ? (1.0 / 6.0) : (2.0 / 6.0);
            const double ch = ci * h;
            const double psi = x[2] + ch * kp[2];
            const double vl = x[3] + ch * kp[3], vt = x[4] + ch * kp[4], r = x[5] + ch * kp[5];
            const double de = x[6] + ch * u[1], a = x[7] + ch * u[0];
            double f[3], J[3][5];          // (the partials are dead code here)
            stm_core(p, vl, vt, r, de, a, f, J);
            double sn, cs;
            fast_sincos(psi, &sn, &cs);
            double k[6];
            k[0] = vl * cs - vt * sn; k[1] = vl * sn + vt * cs; k[2] = r;
            k[3] = f[0]; k[4] = f[1]; k[5] = f[2];
#pragma unroll
            for (int i = 0; i < 6; i++) { xacc[i] += bi * k[i]; kp[i] = k[i]; }
        }
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] += h * xacc[i];
        x[6] += h * u[1]; x[7] += h * u[0];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) xn[i] = x[i];
}

// The trial points of MERIT_BACKTRACKING, between the expansion and the commit kernel: one wavefront per (instance, candidate), lane =
// stage. With z_prev the snapshot in front of the QP and z_qp what the interior point method and the expansion left, the trial point
// is z(alpha) = z_prev + alpha (z_qp - z_prev) in X, U and the slacks, and the wavefront j of an instance evaluates there, for
// alpha = cand[j] (j < K) or alpha = 0 (j = K),
//   cost  the cost as nlp_residual_kernel forms it: wrapped yaw, dt scaling, diagonal or full W, z s + Z s^2 / 2 per row side
//   E     | x0 - X_0 |_1 + sum_k | f(X_k, U_k) - X_{k+1} |_1   (f: ERK4 x nsub of the model, rk4_state)
//   V     sum over the row sides of max(0, -t), t = value - lo + s_l or hi - value + s_u with the row's value AT the trial point
//         (steering-rate box of stage k: U[k][1]; steering angle and gg row of stage s: X[s][6], h_con(X_s))
// into row j of the instance's table. The commit kernel, behind it on the stream, reads the table and decides (merit_accept). An
// instance that has finished, or whose QP failed, is left alone: its table stays.
__global__ void __launch_bounds__(64) sqp_merit_kernel(const KArgs ka, const SqpArgs sq, const MeritArgs ma)
{
    const int b = blockIdx.x, j = blockIdx.y;
    if (b >= ka.batch || j > ma.K) return;
    if (sq.state[b] != 0 || ka.status[b] != 0) return;          // (uniform over the wavefront)
    const int lane = threadIdx.x;
    // the model's constants in LDS: held in scalar registers across the Runge-Kutta loop they do not fit (18 spilled)
    __shared__ Model sM;
    static_assert(sizeof(Model) % sizeof(double) == 0, "copied in doubles");
    for (int i = lane; i < (int)(sizeof(Model) / sizeof(double)); i += 64)
        reinterpret_cast<double *>(&sM)[i] = reinterpret_cast<const double *>(&ka.mp)[i];
    wsync();
    const int N = ka.N, NB = N + 1;
    const int nx = NB * NX, nu = N * NU, nl = 6 * N + 2;
    const double dt = ka.dt;
    const double a = (j < ma.K) ? ma.cand[j] : 0.0;
    // lane = stage. The lanes behind the horizon work on copies of the last stage and contribute nothing
    const int s = (lane < NB) ? lane : N, k = (lane < N) ? lane : N - 1;
    const bool has_x = lane < NB, has_u = lane < N, has_rows = lane >= 1 && lane < NB;
    double x[8], u[2];
    double cl = 0.0, e = 0.0, v = 0.0;
    {
        const double *snap = sq.snap + (size_t)b * sq.snap_len;
        const double *Xq = ka.X + (size_t)b * nx + s * NX, *Uq = ka.U + (size_t)b * nu + k * NU, *Sq = ka.slack + (size_t)b * 6 * N;
        const double *Xp = snap + s * NX, *Up = snap + nx + k * NU, *Sp = snap + nx + nu + nl;
#pragma unroll
        for (int i = 0; i < 8; i++) { const double p = Xp[i]; x[i] = p + a * (Xq[i] - p); }
#pragma unroll
        for (int i = 0; i < 2; i++) { const double p = Up[i]; u[i] = p + a * (Uq[i] - p); }
        if (lane == 0) {
            const double *gx0 = ka.x0 + (size_t)b * NX;
#pragma unroll
            for (int i = 0; i < 8; i++) e += fabs(gx0[i] - x[i]);
        }
        // rows and slack cost: the box of stage k on the lanes < N, the steering angle and the gg row of stage s on the lanes 1 .. N
        const double *gbnd = ka.bnd + (size_t)b * 6 * NB, *gpen = ka.pen + (size_t)b * 36;
        double h, g3, g5, g7;
        h_con(sM, x[3], x[5], x[7], h, g3, g5, g7);
#pragma unroll
        for (int ty = 0; ty < 3; ty++) {
            const int st = (ty == 0) ? k : s;
            const int idx = (ty == 0) ? k : N + 2 * (s - 1) + ((ty == 2) ? 1 : 0);
            const bool on = (ty == 0) ? has_u : has_rows;
            const double val = (ty == 0) ? u[1] : ((ty == 1) ? x[6] : h);
            const double lo = gbnd[(2 * ty) * NB + st], hi = gbnd[(2 * ty + 1) * NB + st];
            const int pc = (ty == 0) ? ((k == 0) ? 0 : 1) : ((st < N) ? 1 : 2);
            const double sc = (ty == 0 || st < N) ? dt : 1.0;
#pragma unroll
            for (int sd = 0; sd < 2; sd++) {
                const int si = on ? sd * 3 * N + idx : 0;
                const double s0 = Sp[si], sl = s0 + a * (Sq[si] - s0);
                const double z = sc * gpen[(pc * 3 + ty) * 4 + sd], Z = sc * gpen[(pc * 3 + ty) * 4 + 2 + sd];
                const double t = sd ? hi - val + sl : val - lo + sl;
                if (on) { v += fmax(-t, 0.0); cl += z * sl + 0.5 * Z * sl * sl; }
            }
        }
        // least-squares cost of the stage
        const double *yr = ka.yref + ((size_t)b * NB + s) * 6;
        double rr[6];
        rr[0] = x[0] - yr[0]; rr[1] = x[1] - yr[1]; rr[2] = wrap_yaw(x[2]) - yr[2]; rr[3] = x[3] - yr[3];
        rr[4] = u[0] - yr[4]; rr[5] = u[1] - yr[5];
        const int ny = (s < N) ? 6 : 4;
        double acc = 0.0;
        if (ka.Wf) {
            const double *Wk = ka.Wf + ((size_t)b * NB + s) * 36;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int i2 = 0; i2 < 6; i2++) if (i < ny && i2 < ny) acc += Wk[i * 6 + i2] * rr[i] * rr[i2];
        } else {
            const double *Wd = ka.W + ((size_t)b * NB + s) * 6;
#pragma unroll
            for (int i = 0; i < 6; i++) if (i < ny) acc += Wd[i] * rr[i] * rr[i];
        }
        if (has_x) cl += 0.5 * ((s < N) ? dt : 1.0) * acc;
    }
    // shooting defects: the lane's interval against the trial state of the lane above
    {
        double xn[8];
        rk4_state(sM, x, u, dt, ka.nsub, xn);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const double nxt = lane_gather(x[i], ((lane + 1) & 63) * 4);
            if (has_u) e += fabs(xn[i] - nxt);
        }
    }
    cl = wave_sum(cl); e = wave_sum(e); v = wave_sum(v);
    if (lane == 0) {
        double *t = ma.table + ((size_t)b * (ma.K + 1) + j) * 3;
        t[0] = cl; t[1] = e; t[2] = v;
    }
}

// The decision of the line search, by the first wavefront of the commit kernel for an instance that takes its step: the weight mu_in
// becomes the largest |multiplier| of the QPs of this solve so far, this one included; the merit function is
// phi = cost + mu_eq E + mu_in V on the rows of the table; accepted is the first j with phi(alpha_j) < phi(0), else the smallest
// candidate. Writes alpha, mu_in and the history entry of this QP; returns alpha (on every lane).
__device__ __forceinline__ double merit_accept(const KArgs &ka, const MeritArgs &ma, int b, int it, int lane)
{
    const int N = ka.N, K = ma.K;
    const double *glm = ka.qp_lam + (size_t)b * (6 * N + 2);
    double m = 0.0;
    for (int i = lane; i < 6 * N; i += 64) m = fmax(m, fabs(glm[i]));
    const double mu = fmax(ma.mu_in[b], wave_max(m));
    const double *t = ma.table + (size_t)b * (K + 1) * 3;
    const double phi0 = t[3 * K] + ma.mu_eq * t[3 * K + 1] + mu * t[3 * K + 2];
    int acc = K - 1;
    for (int j = 0; j < K; j++)
        if (t[3 * j] + ma.mu_eq * t[3 * j + 1] + mu * t[3 * j + 2] < phi0) { acc = j; break; }
    const double a = ma.cand[acc];
    if (lane == 0) {
        ma.alpha[b] = a; ma.mu_in[b] = mu;
        if (it < ma.hist_len) ma.hist[(size_t)b * ma.hist_len + it] = a;
    }
    return a;
}

// what the commit kernel may have to put back: the iterate and the QP's outputs, in front of the QP
__global__ void __launch_bounds__(256) sqp_snapshot_kernel(const KArgs ka, const SqpArgs sq)
{
    const int b = blockIdx.x;
    if (b >= ka.batch) return;
    const int N = ka.N, nx = (N + 1) * NX, nu = N * NU, nl = 6 * N + 2, ns = 6 * N;
    double *o = sq.snap + (size_t)b * sq.snap_len;
    for (int i = threadIdx.x; i < nx; i += blockDim.x) o[i] = ka.X[(size_t)b * nx + i];
    o += nx;
    for (int i = threadIdx.x; i < nu; i += blockDim.x) o[i] = ka.U[(size_t)b * nu + i];
    o += nu;
    for (int i = threadIdx.x; i < nl; i += blockDim.x) o[i] = ka.qp_lam[(size_t)b * nl + i];
    o += nl;
    for (int i = threadIdx.x; i < ns; i += blockDim.x) o[i] = ka.slack[(size_t)b * ns + i];
    o += ns;
    if (threadIdx.x == 0) {
        o[0] = ka.cost[b]; o[1] = ka.res[b * 3]; o[2] = ka.res[b * 3 + 1]; o[3] = ka.res[b * 3 + 2];
        int *oi = sq.snapi + (size_t)b * 3;
        oi[0] = ka.status[b]; oi[1] = ka.qp_iter[b]; oi[2] = ka.qp_status[b];
    }
}

// Behind the QP and its expansion. An instance that had converged or failed before this iteration gets back everything the
// snapshot holds (bit-identical); an active one whose QP failed gets back its iterate (status 4 and the QP's statistics stay) and
// stops; an active one that took the step moves by alpha: z <- z_prev + alpha (z_new - z_prev) for X, U, slacks and multipliers.
// alpha is sq.alpha, or with globalization MERIT_BACKTRACKING (ma.alpha set) the instance's own, which the first wavefront decides here
// from the table sqp_merit_kernel has written (merit_accept): an instance that took less than the full step also starts its next QP
// cold (its warm-start word is cleared: interpolated multipliers are no warm start).
__global__ void __launch_bounds__(256) sqp_commit_kernel(const KArgs ka, const SqpArgs sq, const MeritArgs ma)
{
    __shared__ int mode;          // 0 restore all, 1 restore the iterate (QP failed), 2 step
    __shared__ double step;       // its length
    const int b = blockIdx.x;
    if (b >= ka.batch) return;
    if (threadIdx.x < 64) {
        const int st = sq.state[b];
        const int m = (st != 0) ? 0 : ((ka.status[b] != 0) ? 1 : 2);
        double al = sq.alpha;
        if (ma.alpha && m == 2) al = merit_accept(ka, ma, b, sq.sqp_iter[b], threadIdx.x);
        if (threadIdx.x == 0) {
            if (st == 0) {
                sq.sqp_iter[b] += 1;
                if (m == 1) sq.state[b] = 2;
            }
            mode = m; step = al;
        }
    }
    __syncthreads();
    const int m = mode;
    const double a = step;
    if (m == 2 && a == 1.0) return;
    const int N = ka.N, nx = (N + 1) * NX, nu = N * NU, nl = 6 * N + 2, ns = 6 * N;
    const double *o = sq.snap + (size_t)b * sq.snap_len;
    auto put = [&](double *dst, const double *prev, int n) {
        if (m == 2) { for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = prev[i] + a * (dst[i] - prev[i]); }
        else for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = prev[i];
    };
    put(ka.X + (size_t)b * nx, o, nx);
    put(ka.U + (size_t)b * nu, o + nx, nu);
    put(ka.qp_lam + (size_t)b * nl, o + nx + nu, nl - 2);          // (the warm-start flag behind the multipliers: the QP's own)
    put(ka.slack + (size_t)b * ns, o + nx + nu + nl, ns);
    if (m == 2 && ma.alpha && threadIdx.x == 0) ka.qp_lam[(size_t)b * nl + 6 * N] = 0.0;
    if (m != 2 && threadIdx.x == 0) {
        ka.qp_lam[(size_t)b * nl + 6 * N] = o[nx + nu + 6 * N];
        ka.cost[b] = o[nx + nu + nl + ns];
    }
    if (m == 0 && threadIdx.x == 0) {
        const double *r = o + nx + nu + nl + ns + 1;
        ka.res[b * 3] = r[0]; ka.res[b * 3 + 1] = r[1]; ka.res[b * 3 + 2] = r[2];
        const int *oi = sq.snapi + (size_t)b * 3;
        ka.status[b] = oi[0]; ka.qp_iter[b] = oi[1]; ka.qp_status[b] = oi[2];
    }
}

}  // namespace tum
