// rti_kernels.hpp -- the FEEDBACK phase of a split real-time iteration (tum_ocp_options_set "rti_phase" 2).
//
// The preparation (rti_phase 1) ran the linearisation and the condensing at the initial state x0_prep. x0 enters the condensed QP
// through the constant column g of the recursion alone (g_0 = x0 - X_0, g_{k+1} = A_k g_k + b_k; cond_kernel / cond_wide_kernel), and
// g enters the gradient q and the row constants d alone -- both affine in x0. H, the gg rows C, bounds and penalties do not see it.
// With delta_0 = x0 - x0_prep and delta_{k+1} = A_k delta_k:
//     d[2 (s - 1)]     += delta_s[6]                                                (steering angle row of stage s = 1..N)
//     d[2 (s - 1) + 1] += g3 delta_s[3] + g5 delta_s[5] + g7 delta_s[7]             (gg row; g3, g5, g7: PR_GH of record s)
//     q[2 k + r]       += (B_k' lambda_{k+1})[r],   lambda_N = W_e o delta_N[0..3],   lambda_k = A_k' lambda_{k+1} + dt W_k o delta_k[0..3]
// (the weights as cond_kernel's sWt scales them: dt W_s below stage N, W_e at N; the cost rows are the states 0..3). Written as the
// DIFFERENCE against the preparation the update needs neither the reference nor the residuals nor the yaw wrap, and a feedback at
// an unchanged x0 adds exact zeros: prepare + feedback then IS the one-call solve, bit for bit.
//
// One wavefront per instance; two serial chains of N 8 x 8 matrix-vector products, latency-bound:
//   * the stage records of the whole horizon are requested at once (16 bytes a lane and load, all loads in flight together: ONE
//     memory round trip, where expand_instance keeps EX_AHEAD = 8 stages in flight) and parked in LDS -- the adjoint sweep reads
//     them a second time, backwards;
//   * a product is spread over the lanes of a DPP row: lane i holds component i of the vector and forms row i of A_k delta (column i
//     of A_k' lambda; the lanes 8, 9: the two columns of B_k) with the vector's other components as `row_newbcast` operands of
//     v_fmac_f64_dpp (RecRows' instruction): no readlane, no LDS round trip and no reduction on the chain -- six / eight FMAs a stage
//     in two accumulators. The four DPP rows of the wavefront carry the same values; the coefficients of a stage are read from
//     LDS one stage ahead of their use (two register sets);
//   * delta_0..delta_N and the increments of q wait in LDS; d and q are updated by all lanes behind the sweeps.
// No lane-dependent branch: every lane stores (to its own slot or to one that is never read), so EXEC is never written in front
// of a DPP operation (tests/test_host_logic.py scans the shipped code object for that hazard).
#pragma once
#include "pipe_kernels.hpp"

namespace tum {

// acc += (lane L of the row of v) * x
template <int L> __device__ __forceinline__ void fmac_bcast(double &acc, double v, double x)
{
    static_assert(L >= 0 && L < 16, "lane of the row");
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(x), "n"(L));
}
// (a DPP operand must not be read within two wait states of the vector instruction that wrote it; the compiler does not look into the asm)
__device__ __forceinline__ void dpp_settle(double &v) { asm volatile("s_nop 1" : "+v"(v)); }

template <int NT_>
__global__ void __launch_bounds__(64) rti_feedback_kernel(const PArgs pa, const double *x0_prep)
{
    PD_LOCALS
    constexpr int NL = (NMAX + 2) / 2;          // 16-byte loads per lane that cover the records 0..NMAX
    __shared__ __attribute__((aligned(16))) double sRec[NL * 128];
    __shared__ double sD[(NMAX + 1) * NX], sW[(NMAX + 1) * 4], sQ[NVP + 64];          // (sQ[NVP ..]: slots of the lanes that hold no column of B)
    const KArgs &ka = pa.ka;
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= ka.batch) return;
    const int N = ka.N, nv = 2 * N;
    const double dt = ka.dt;
    const double *grec = pa.rec + (size_t)b * (N + 1) * PREC;
    const double *gW = ka.W + (size_t)b * (N + 1) * 6;
    double *gvec = pa.vec + (size_t)b * PVEC;
    const int lc = lane & 15, ri = lc & 7;

    // ---- every record of the horizon: all loads first, one round trip
    {
        typedef double d2 __attribute__((ext_vector_type(2)));
        const int nrec = (N + 1) * PREC;
        d2 t[NL];
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = 128 * j + 2 * lane;
            t[j] = (i < nrec) ? *reinterpret_cast<const d2 *>(grec + i) : d2{0.0, 0.0};
        }
        const double d0 = ka.x0[(size_t)b * NX + ri] - x0_prep[(size_t)b * NX + ri];
        for (int i = lane; i < (N + 1) * 4; i += 64) sW[i] = ((i < 4 * N) ? dt : 1.0) * gW[(i >> 2) * 6 + (i & 3)];
        sD[ri] = d0;
#pragma unroll
        for (int j = 0; j < NL; j++) *reinterpret_cast<d2 *>(sRec + 128 * j + 2 * lane) = t[j];
    }
    wsync();

    // ---- forward: delta_{k+1} = A_k delta_k (apply_A_rec's semantics), component ri on the lanes ri and ri + 8 of every row
    {
        const bool core = ri < 6;
        const double diag = (ri < 3 || ri >= 6) ? 1.0 : 0.0;
        const int osp = (ri < 2) ? ri : 0, os = 2 + (core ? ri : 0) * 7;
        // (an entry a lane's row does not have is a product with 0.0 of a field that exists, not a select: a select of a loaded value
        //  becomes a branch round the load, and the wait for it lands in front of THIS stage's chain instead of the next one's)
        const double mpsi = (ri < 2) ? 1.0 : 0.0, mcore = core ? 1.0 : 0.0;
        // row ri of [Sp | S] of record k: the psi column and the five state columns
        auto coef = [&](int k, double c[6]) __attribute__((always_inline)) {
            const double *rec = sRec + k * PREC;
            c[0] = mpsi * rec[osp];
#pragma unroll
            for (int j = 0; j < 5; j++) c[1 + j] = mcore * rec[os + j];
        };
        double d = sD[ri];
        auto stage = [&](int k, const double c[6], double cn[6]) __attribute__((always_inline)) {
            coef(k + 1 < N ? k + 1 : k, cn);          // (the next stage's, in flight behind this stage's chain)
            double a0 = diag * d, a1 = 0.0;
            dpp_settle(d);
            fmac_bcast<2>(a0, d, c[0]); fmac_bcast<3>(a1, d, c[1]);
            fmac_bcast<4>(a0, d, c[2]); fmac_bcast<5>(a1, d, c[3]);
            fmac_bcast<6>(a0, d, c[4]); fmac_bcast<7>(a1, d, c[5]);
            d = a0 + a1;
            sD[(k + 1) * NX + ri] = d;          // (all lanes that hold component ri store the same value)
        };
        double ca[6], cb[6];
        coef(0, ca);
        for (int k = 0; k < N; k += 2) {
            stage(k, ca, cb);
            if (k + 1 < N) stage(k + 1, cb, ca);
        }
    }
    wsync();

    // ---- adjoint: lane c < 8 column c of A_k' lambda, the lanes 8, 9 the columns of B_k
    {
        // entry (i, column) of [A_k | B_k]: rows i < 6 from S (columns 3..7 of A, then B's two), the psi column from Sp, the unit
        // diagonal of px, py, psi and of the two integrators, whose input entries are dt (rows 6, 7 of B: b6c / b7c of cond_kernel)
        const bool scol = lc >= 3 && lc < 10, pcol = lc == 2;
        const int os = 2 + (scol ? lc - 3 : 0);
        const double c6 = (lc == 6) ? 1.0 : (lc == 9) ? dt : 0.0, c7 = (lc == 7) ? 1.0 : (lc == 8) ? dt : 0.0;
        const double u0 = (lc == 0) ? 1.0 : 0.0, u1 = (lc == 1) ? 1.0 : 0.0, u2 = pcol ? 1.0 : 0.0;
        const bool wl = lc < 4;
        const double ms = scol ? 1.0 : 0.0, mp = pcol ? 1.0 : 0.0, mw = wl ? 1.0 : 0.0;          // (products, not selects: as in the forward sweep)
        const int ow = wl ? lc : 0, od = (lc < 8) ? lc : 0;
        // c[0..5]: rows 0..5 of the lane's column; c[6]: the weighted delta_k of the lane's component
        auto coef = [&](int k, double c[7]) __attribute__((always_inline)) {
            const double *rec = sRec + k * PREC;
#pragma unroll
            for (int i = 0; i < 6; i++) c[i] = ms * rec[os + 7 * i];
            c[0] += mp * rec[0] + u0;
            c[1] += mp * rec[1] + u1;
            c[2] += u2;
            c[6] = mw * (sW[k * 4 + ow] * sD[k * NX + od]);
        };
        double lam = wl ? sW[N * 4 + ow] * sD[N * NX + od] : 0.0;
        const bool qcol = lc == 8 || lc == 9;
        auto stage = [&](int k, const double c[7], double cn[7]) __attribute__((always_inline)) {
            coef(k > 0 ? k - 1 : 0, cn);
            double a0 = c[6], a1 = 0.0;
            dpp_settle(lam);
            fmac_bcast<0>(a0, lam, c[0]); fmac_bcast<1>(a1, lam, c[1]);
            fmac_bcast<2>(a0, lam, c[2]); fmac_bcast<3>(a1, lam, c[3]);
            fmac_bcast<4>(a0, lam, c[4]); fmac_bcast<5>(a1, lam, c[5]);
            fmac_bcast<6>(a0, lam, c6); fmac_bcast<7>(a1, lam, c7);
            lam = a0 + a1;
            sQ[qcol ? 2 * k + (lc - 8) : NVP + lane] = lam;          // (B_k' lambda_{k+1}; the other lanes: lambda_k, to a slot nobody reads)
        };
        double ca[7], cb[7];
        coef(N - 1, ca);
        for (int k = N - 1; k >= 0; k -= 2) {
            stage(k, ca, cb);
            if (k >= 1) stage(k - 1, cb, ca);
        }
    }
    wsync();
    // ---- the rows (stage s = lane + 1) and the gradient: behind the sweeps, where a lane-dependent branch is in front of no DPP operation
    {
        const int s = (lane < N) ? lane + 1 : N;
        const double *ds = sD + s * NX, *gh = sRec + s * PREC + PR_GH;
        const double e0 = ds[6], e1 = gh[0] * ds[3] + gh[1] * ds[5] + gh[2] * ds[7];
        double *gd = gvec + PV_D + 2 * (s - 1);
        const double o0 = gd[0], o1 = gd[1];
        if (lane < N) { gd[0] = o0 + e0; gd[1] = o1 + e1; }
    }
    for (int i = lane; i < nv; i += 64) gvec[PV_Q + i] += sQ[i];
}

}  // namespace tum
