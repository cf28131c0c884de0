// disturbance_kernels.hpp -- K18: the disturbance realisation of the closed loop, drawn on the device (what Utils/MPC_sim_utils.py:54-86
// generate_disturbances / sample_from_ellipsoid draw per control step for SimulationMode_main_class.py:121-143). The distributions are
// the reference's; the random stream is this project's own: a Philox4x32-10 draw that depends on (seed, instance, step, stream, kind)
// alone -- the definition stands in include/tum_nmpc.h ("Disturbance draws"), closed_loop.DisturbanceModel.draw_counter is its host
// statement.
//   disturbance_draw_kernel   one lane per (step, instance) row, blockIdx.y the stream (0: derivative disturbance, 1: estimation error),
//                             so the kind is wave-uniform. Launched once per control step in front of plant_advance_kernel (one row per
//                             instance into the loop's slab, the step read from the loop's counter on the device), or on request for
//                             any window into a table. Both go through disturbance_draw: a live draw and a regenerated table are the
//                             same bits.
#pragma once
#include "collect_kernels.hpp"

namespace tum {

constexpr int DIST_OFF = 0, DIST_UNIFORM = 1, DIST_GAUSSIAN = 2, DIST_ABSOLUTE = 3, DIST_BOX = 4;

// The seven values of stream s for instance b at control step t. bound: the magnitudes w[i] >= 0, root: sqrt(w[i]) (host, IEEE).
// This runs once per control step beside three short kernels, so its time is instruction fetch as plant_advance_kernel's is: the blocks
// are a loop that is NOT unrolled around the one inlined copy of Philox and of the Box-Muller body (log, sqrt, sincos); a block's two
// values reach their slots of z by selects (a dynamic index would put z into scratch).
__device__ __forceinline__ void disturbance_draw(unsigned long long seed, unsigned b, unsigned long long t, int s, int kind,
                                                 const double *bound, const double *root, double out[7])
{
#pragma clang fp contract(off)
    if (kind == DIST_ABSOLUTE) {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = bound[i];
        return;
    }
    const bool normal = kind == DIST_UNIFORM || kind == DIST_GAUSSIAN;
    const int n_blocks = kind == DIST_UNIFORM ? 5 : 4;
    double z[8], u4 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) z[i] = 0.0;
#pragma unroll 1
    for (int j = 0; j < n_blocks; j++) {
        unsigned c[4] = {b, (unsigned)t, (unsigned)(t >> 32), 0x100u * (1u + (unsigned)s) + (unsigned)j};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        const double uA = (double)(((unsigned long long)(c[0] >> 5) << 26) + (unsigned long long)(c[1] >> 6)) * 0x1p-53;
        const double uB = (double)(((unsigned long long)(c[2] >> 5) << 26) + (unsigned long long)(c[3] >> 6)) * 0x1p-53;
        double va = uA, vb = uB;
        if (normal) {
            const double R = sqrt(-2.0 * log(1.0 - uA));          // (1 - uA is exact and in (0, 1])
            double sn, cs;
            fast_sincos((2.0 * M_PI) * uB, &sn, &cs);
            va = R * cs; vb = R * sn;
        }
        if (j == 4) u4 = uA;          // (the radius of the ellipsoid; slots 8, 9 do not exist)
#pragma unroll
        for (int i = 0; i < 8; i++) z[i] = (i == 2 * j) ? va : (i == 2 * j + 1) ? vb : z[i];
    }
    if (kind == DIST_GAUSSIAN) {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = bound[i] * z[i];
    } else if (kind == DIST_UNIFORM) {
        double n2 = z[0] * z[0];
#pragma unroll
        for (int i = 1; i < 7; i++) n2 = n2 + z[i] * z[i];
        const double nz = sqrt(n2), r = pow(u4, 1.0 / 7.0);
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = (nz == 0.0) ? 0.0 : root[i] * r * z[i] / nz;
    } else {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = -bound[i] + z[i] * (2.0 * bound[i]);
    }
}

struct DistArgs {
    int batch, n_steps;                               // rows = n_steps * batch, layout [step][b][7] (the playback layout)
    int kind[2];                                      // per stream (DIST_OFF: nothing is written)
    unsigned long long seed;
    long long first_step;                             // global control step of row 0 ...
    const int *step_counter;                          // ... or (non-null) read from the loop's counter on the device: [0] steps completed
    double bound[2][7], root[2][7];
    double *out[2];                                   // per stream, nullable
};

__global__ void __launch_bounds__(64) disturbance_draw_kernel(const DistArgs a)
{
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= (long long)a.n_steps * a.batch || a.kind[s] == DIST_OFF || !a.out[s]) return;
    const long long first = a.step_counter ? (long long)a.step_counter[0] : a.first_step;
    const long long step = row / a.batch;
    const unsigned b = (unsigned)(row - step * a.batch);
    double v[7];
    disturbance_draw(a.seed, b, (unsigned long long)(first + step), s, a.kind[s], a.bound[s], a.root[s], v);
    double *o = a.out[s] + (size_t)row * 7;
#pragma unroll
    for (int i = 0; i < 7; i++) o[i] = v[i];
}

}  // namespace tum
