// Probe: policy_kernel of csrc/policy_kernels.hpp with TUM_POL_WAVES wavefronts per tile of 16 instances (compile once per value:
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -DTUM_POL_WAVES=<1|2|4|8> -I tum-control_amd/csrc -o probe_policy_waves_<n> probe_policy_waves.cpp).
// The shipped agent's shape 22-128-256-128-26 with seeded weights, 16 and 4096 instances, the time of one launch from events around 200.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "policy_kernels.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main()
{
    const int widths[5] = {22, 128, 256, 128, 26};
    tum::PolicyArgs a = {};
    a.n_mat = 4; a.n_in = 22; a.n_act = 26;
    srand(1);
    std::vector<std::vector<double>> Wh(4);          // the same weights row-major, for the check on the host
    for (int l = 0; l < 4; l++) {
        const int in = widths[l], out = widths[l + 1], kp = (in + 3) & ~3, mp = (out + 15) & ~15;
        a.kp[l] = kp; a.mp[l] = mp; if (kp > a.rows) a.rows = kp; if (mp > a.rows) a.rows = mp;
        std::vector<double> W((size_t)mp * kp, 0.0), b(mp, 0.0);
        Wh[l].assign((size_t)out * in, 0.0);
        for (int t = 0; t < mp / 16; t++) for (int q = 0; q < kp / 4; q++) for (int lane = 0; lane < 64; lane++) {
            const int r = 16 * t + (lane & 15), k = 4 * q + (lane >> 4);
            if (r < out && k < in) Wh[l][(size_t)r * in + k] = W[((size_t)t * (kp / 4) + q) * 64 + lane] = (double)(float)((rand() / (double)RAND_MAX - 0.5) * 0.2);
        }
        double *dW, *db;
        CK(hipMalloc((void **)&dW, W.size() * 8)); CK(hipMalloc((void **)&db, b.size() * 8));
        CK(hipMemcpy(dW, W.data(), W.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b.data(), b.size() * 8, hipMemcpyHostToDevice));
        a.W[l] = dW; a.b[l] = db;
    }
    const int NMAX = 4096;
    std::vector<double> obs((size_t)NMAX * 22);
    for (auto &v : obs) v = rand() / (double)RAND_MAX;
    double *dobs, *dlog; int *dact;
    CK(hipMalloc((void **)&dobs, obs.size() * 8)); CK(hipMalloc((void **)&dact, NMAX * 4)); CK(hipMalloc((void **)&dlog, (size_t)NMAX * 26 * 8));
    CK(hipMemcpy(dobs, obs.data(), obs.size() * 8, hipMemcpyHostToDevice));
    a.obs = dobs; a.obs_stride = 22; a.actions = dact; a.logits = dlog;
    CK(hipFuncSetAttribute((const void *)tum::policy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    const size_t lds = sizeof(double) * 2 * a.rows * tum::POL_TILE;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    long sum = 0;
    for (int n : {16, 4096}) {
        a.n = n;
        const int iters = 200;
        for (int rep = 0; rep < 3; rep++) {          // (the first repetition warms up)
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < iters; i++) hipLaunchKernelGGL(tum::policy_kernel, dim3((n + 15) / 16), dim3(64 * tum::POL_WAVES), lds, 0, a);
            CK(hipEventRecord(e1, 0));
            CK(hipDeviceSynchronize());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep) printf("waves %d  instances %4d  %.2f us per launch (back to back, %d launches)\n", tum::POL_WAVES, n, ms * 1e3 / iters, iters);
        }
        std::vector<int> act(n);
        CK(hipMemcpy(act.data(), dact, n * 4, hipMemcpyDeviceToHost));
        long part = 0;
        for (int v : act) part += v;
        // against the same network in plain double loops on the host
        std::vector<double> lg((size_t)n * 26);
        CK(hipMemcpy(lg.data(), dlog, lg.size() * 8, hipMemcpyDeviceToHost));
        double worst = 0.0; int wrong = 0;
        for (int i = 0; i < n; i++) {
            std::vector<double> h(22), z;
            for (int k = 0; k < 22; k++) h[k] = (double)(float)obs[(size_t)i * 22 + k];
            for (int l = 0; l < 4; l++) {
                z.assign(widths[l + 1], 0.0);
                for (int r = 0; r < widths[l + 1]; r++) { double s = 0.0; for (int k = 0; k < widths[l]; k++) s += Wh[l][(size_t)r * widths[l] + k] * h[k]; z[r] = l < 3 ? tanh(s) : s; }
                h = z;
            }
            int best = 0;
            for (int r = 0; r < 26; r++) { worst = fmax(worst, fabs(z[r] - lg[(size_t)i * 26 + r])); if (z[r] > z[best]) best = r; }
            wrong += best != act[i];
        }
        printf("waves %d  instances %4d  sum of actions %ld  largest |logit - host| %.3g  actions that differ from the host's %d\n", tum::POL_WAVES, n, part, worst, wrong);
        sum += part;
    }
    printf("waves %d  checksum of the actions %ld\n", tum::POL_WAVES, sum);
    return 0;
}
