// policy_probe.hip -- TEST ONLY (tests/test_gpu_policy.py): policy_tanh of csrc/policy_kernels.hpp, the activation policy_kernel applies,
// element by element on an array, so that it can be held to the exact value on its own. Compiled by the test, never part of the library.
#include <hip/hip_runtime.h>
#include "policy_kernels.hpp"

__global__ void probe_tanh_kernel(const double *x, double *y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tum::policy_tanh(x[i]);
}

extern "C" int probe_policy_tanh(const double *x, double *y, int n)
{
    double *dx = nullptr, *dy = nullptr;
    hipError_t e = hipMalloc((void **)&dx, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void **)&dy, sizeof(double) * n);
    if (e == hipSuccess) e = hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(probe_tanh_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void)hipFree(dx); (void)hipFree(dy);
    return (int)e;
}
