// plant_probe.hip -- TEST ONLY (tests/test_gpu_plant_reference.py): plant_xdot of csrc/loop_kernels.hpp applied to an array of points,
// four lanes (one DPP quad) per point as plant_advance_kernel deals them, every lane's result stored. Includes that header and
// nothing else of the library; not part of the shipped build. vehicle_constants (tum_nmpc.hip) is a static function of the
// library's own translation unit: the folded constants come from the test, which restates the folding, in the order of the
// members of PlantModel.
#include "loop_kernels.hpp"

using namespace tum;

namespace {

constexpr int TPB = 64;

// x [n][7], au [n][2] = a, sr; xd [n][4][7]. Lanes of quads beyond the last point shadow it and store nothing.
__global__ void __launch_bounds__(TPB) k_plant_xdot(PlantModel pm, const double *x, const double *au, double *xd, int n)
{
    const int tid = blockIdx.x * TPB + threadIdx.x;
    const int item = tid >> 2, role = tid & 3;
    const int it = item < n ? item : n - 1;
    PlantLane tl;
    tl.role = role; tl.front = !(role & 1);
    tl.B = tl.front ? pm.Bf : pm.Br; tl.C = tl.front ? pm.Cf : pm.Cr; tl.D = tl.front ? pm.Df : pm.Dr;
    tl.E = tl.front ? pm.Ef : pm.Er; tl.invFmax = tl.front ? pm.invFmax_f : pm.invFmax_r;
    double xv[7], k[7];
    for (int i = 0; i < 7; i++) xv[i] = x[(size_t)it * 7 + i];
    plant_xdot(pm, tl, xv, au[(size_t)it * 2], au[(size_t)it * 2 + 1], k);
    if (item >= n) return;
    for (int i = 0; i < 7; i++) xd[((size_t)item * 4 + role) * 7 + i] = k[i];
}

}  // namespace

// pm: the 21 doubles of PlantModel in the order of its members. A nonzero return value is the first HIP error met.
extern "C" int probe_plant_xdot(const double *pm, const double *x, const double *au, double *xd, int n)
{
    static_assert(sizeof(PlantModel) == 21 * sizeof(double), "PlantModel is 21 doubles");
    if (n < 1 || !pm || !x || !au || !xd) return -1;
    PlantModel m;
    __builtin_memcpy(&m, pm, sizeof(m));
    double *dx = nullptr, *da = nullptr, *dd = nullptr;
    hipError_t e = hipMalloc((void **)&dx, sizeof(double) * 7 * n);
    if (e == hipSuccess) e = hipMalloc((void **)&da, sizeof(double) * 2 * n);
    if (e == hipSuccess) e = hipMalloc((void **)&dd, sizeof(double) * 28 * n);
    if (e == hipSuccess) e = hipMemcpy(dx, x, sizeof(double) * 7 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(da, au, sizeof(double) * 2 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dd, 0xff, sizeof(double) * 28 * n);          // (NaN: a lane that does not store shows)
    if (e == hipSuccess) {
        k_plant_xdot<<<(int)(((long long)n * 4 + TPB - 1) / TPB), TPB>>>(m, dx, da, dd, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(xd, dd, sizeof(double) * 28 * n, hipMemcpyDeviceToHost);
    (void)hipFree(dx); (void)hipFree(da); (void)hipFree(dd);
    return (int)e;
}
