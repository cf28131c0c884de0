// common_kernels.hpp -- what every kernel variant shares: phase timers, the acados status code, the row-state accessor of the
// interior point kernels, the longest-first schedule and the cold start.
#pragma once
#include "nmpc_device.hpp"

namespace tum {

// optional in-kernel phase timers (KF_PROF): cycles per phase accumulated into ka.prof[b][12]
#define TUM_TICK(slot) do { asm volatile("; TUM_MARK " #slot); if (PROF) { const long long t_ = __builtin_readcyclecounter(); pacc[slot] += t_ - tprev; tprev = t_; } } while (0)

__device__ __forceinline__ int acados_status(int qp_status) { return (qp_status == 0 || qp_status == 1) ? 0 : 4; }

// row-side state of the interior point kernels: rowst[field][slot * 2 + side], fields s, t, lam, mu, rs, rt
#define ROWF(f, k) rowst[f][k]

// Longest-first schedule for the NEXT solve: workgroup i gets the instance with the i-th largest iteration count of THIS
// solve (counting sort, one wavefront). A batch is only a few rounds of resident wavefronts (4096 instances = 4 rounds of
// 1024), and the time of an instance is proportional to its iteration count (4..15), so in natural order the last round
// leaves most of the GPU idle while a few long instances finish: measured 2.62 ms natural order, 2.17 ms longest-first,
// 2.34 ms shortest-first for the same 4096 instances. Iteration counts of consecutive solves of an MPC are strongly
// correlated (and identical for a repeated batch), which makes the last solve a good predictor.
// ONE wavefront with few registers: the kernel runs at the end of a solve's chain while the interior point kernels of the other
// streams hold (almost) every register of every SIMD -- a workgroup of 1024 threads had to wait for a compute unit without any of
// their wavefronts, a single small wavefront is placed beside them. The order is deterministic: iteration counts descending,
// instances of one count by ascending index (a stable counting sort). Lane l owns the instances [l chunk, (l + 1) chunk):
//   pass 1  its histogram, cnt[k][l] (a column of its own: no lane touches another's)
//   scan    per count k, longest first: the exclusive prefix of cnt[k][.] over the lanes behind the running total -- the position
//           of lane l's first instance of that count
//   pass 2  the lane walks its instances again in ascending order and takes the positions one by one
constexpr int LPT_K = 64;          // iteration counts are clipped to 0..63
__global__ void __launch_bounds__(64) lpt_order_kernel(const int *qp_iter, int *order, int batch)
{
    __shared__ int cnt[LPT_K * 64];
    const int lane = threadIdx.x;
    const int chunk = (batch + 63) >> 6;
    const int i0 = lane * chunk < batch ? lane * chunk : batch, i1 = i0 + chunk < batch ? i0 + chunk : batch;
#pragma unroll
    for (int k = 0; k < LPT_K; k++) cnt[k * 64 + lane] = 0;
    // (a lane's instances eight at a time: the loads of a block are in flight together -- one at a time, each waited for, the two
    //  passes were 128 trips to memory one behind the other -- and the counters move by LDS adds that nobody waits for)
    constexpr int BLK = 8;
    auto load_block = [&](const int i, int (&kk)[BLK]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < BLK; j++) {
            const int k = qp_iter[(i + j < i1) ? i + j : i1 - 1];          // (i < i1: the index is valid)
            kk[j] = k < 0 ? 0 : (k > LPT_K - 1 ? LPT_K - 1 : k);
        }
    };
    for (int i = i0; i < i1; i += BLK) {
        int kk[BLK];
        load_block(i, kk);
#pragma unroll
        for (int j = 0; j < BLK; j++) if (i + j < i1) atomicAdd(&cnt[kk[j] * 64 + lane], 1);
    }
    int acc = 0;
#pragma unroll 8
    for (int k = LPT_K - 1; k >= 0; k--) {
        const int own = cnt[k * 64 + lane];
        int incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); incl += (lane >= d) ? up : 0; }
        cnt[k * 64 + lane] = acc + incl - own;
        acc += __shfl(incl, 63);
    }
    for (int i = i0; i < i1; i += BLK) {
        int kk[BLK];
        load_block(i, kk);
#pragma unroll
        for (int j = 0; j < BLK; j++) if (i + j < i1) order[atomicAdd(&cnt[kk[j] * 64 + lane], 1)] = i + j;          // (one lane's adds: in order)
    }
}

// cold start on the device: X_k = x0, U = 0 (acados create / reset + set(i,'x',x0); NMPC_class.py:250-254)
__global__ void cold_start_kernel(double *X, double *U, const double *x0, int N, int batch, double *qp_lam)
{
    const int b = blockIdx.x;
    if (b >= batch) return;
    if (qp_lam && threadIdx.x == 0) qp_lam[(size_t)b * (6 * N + 2) + 6 * N] = 0.0;          // (the interior point method of the next solve starts cold as well)
    for (int i = threadIdx.x; i < (N + 1) * NX; i += blockDim.x) X[(size_t)b * (N + 1) * NX + i] = x0[(size_t)b * NX + (i & 7)];
    for (int i = threadIdx.x; i < N * NU; i += blockDim.x) U[(size_t)b * N * NU + i] = 0.0;
}

}  // namespace tum
