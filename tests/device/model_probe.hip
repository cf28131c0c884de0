// model_probe.hip -- TEST ONLY (tests/test_gpu_model_reference.py): the device functions of csrc/nmpc_device.hpp applied, one by one, to
// arrays of inputs. Includes that header and nothing else of the library; not part of the shipped build. One extern "C" host entry per
// function group; every entry copies its inputs to the device, launches a one-dimensional kernel, checks hipGetLastError and
// hipDeviceSynchronize, and copies the outputs back. A nonzero return value is the first HIP error met.
#include "nmpc_device.hpp"

#include <cmath>
#include <cstring>
#include <vector>

using namespace tum;

static Model g_model;

// the vehicle constants as the library derives them from its description (tum_nmpc.hip: vehicle_constants, tum_ocp_create)
// p: lf lr m Iz ro S Cd Bf Cf Df Ef Br Cr Dr Er g fr0 fr1 fr4 acc_min
extern "C" int probe_set_model(const double *p, int n_ggv, const double *v, const double *ax, const double *ay)
{
    if (n_ggv < 2 || n_ggv > 16) return -1;
    Model &m = g_model;
    std::memset(&m, 0, sizeof(m));
    const double lf = p[0], lr = p[1], mass = p[2], Iz = p[3], ro = p[4], S = p[5], Cd = p[6], g = p[15];
    m.lf = lf; m.lr = lr; m.m = mass; m.inv_m = 1.0 / mass; m.inv_Iz = 1.0 / Iz;
    m.ka = 0.5 * ro * S * Cd;
    m.Bf = p[7]; m.Cf = p[8]; m.Df = p[9]; m.Ef = p[10];
    m.Br = p[11]; m.Cr = p[12]; m.Dr = p[13]; m.Er = p[14];
    m.Fz_f = mass * lr * g / (lf + lr);
    m.Fz_r = mass * lf * g / (lf + lr);
    m.invFmax_f = 1.0 / std::sqrt(m.Fz_f * m.Fz_f + (m.Cf * m.Fz_f) * (m.Cf * m.Fz_f));
    m.invFmax_r = 1.0 / std::sqrt(m.Fz_r * m.Fz_r + (m.Cr * m.Fz_r) * (m.Cr * m.Fz_r));
    m.fr0 = p[16]; m.fr1 = p[17]; m.fr4 = p[18];
    m.ax_brake = -p[19];
    m.n_ggv = n_ggv;
    for (int i = 0; i < n_ggv; i++) { m.ggv_v[i] = v[i]; m.ggv_ax[i] = ax[i]; m.ggv_ay[i] = ay[i]; }
    return 0;
}

namespace {

// device buffers of one call: inputs copied in, outputs copied back, everything freed on every path
struct Bufs {
    std::vector<void *> dev;
    hipError_t err = hipSuccess;
    ~Bufs() { for (void *p : dev) (void)hipFree(p); }
    double *in(const double *h, size_t n)
    {
        double *d = out(n);
        if (err == hipSuccess && n) err = hipMemcpy(d, h, n * sizeof(double), hipMemcpyHostToDevice);
        return d;
    }
    double *out(size_t n)
    {
        void *d = nullptr;
        if (err == hipSuccess) { err = hipMalloc(&d, (n ? n : 1) * sizeof(double)); if (err == hipSuccess) dev.push_back(d); }
        return (double *)d;
    }
    void launched()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    void back(double *h, const double *d, size_t n)
    {
        if (err == hipSuccess && n) err = hipMemcpy(h, d, n * sizeof(double), hipMemcpyDeviceToHost);
    }
};

constexpr int TPB = 64;
inline int blocks(long long threads) { return (int)((threads + TPB - 1) / TPB); }

// which: 0 fast_sincos (o0 sin, o1 cos)  1 fast_atan  2 fast_sqrt_pos  3 frcp  4 raw rcp seed  5 raw rsq seed
__global__ void k_primitive(int which, const double *x, double *o0, double *o1, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double a = 0.0, b = 0.0;
    switch (which) {
    case 0: fast_sincos(v, &a, &b); break;
    case 1: a = fast_atan(v); break;
    case 2: a = fast_sqrt_pos(v); break;
    case 3: a = frcp(v); break;
    case 4: a = __builtin_amdgcn_rcp(v); break;
    default: a = __builtin_amdgcn_rsq(v); break;
    }
    o0[i] = a; o1[i] = b;
}

__global__ void k_wrap_yaw(const double *x, double *o, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) o[i] = wrap_yaw(x[i]);
}

__global__ void k_pacejka(Model mp, int front, const double *al, double *Fy, double *dFy, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double a, b;
    if (front) pacejka(mp.Bf, mp.Cf, mp.Df, mp.Ef, al[i], a, b);
    else pacejka(mp.Br, mp.Cr, mp.Dr, mp.Er, al[i], a, b);
    Fy[i] = a; dFy[i] = b;
}

// in [n][5] = vl vt r delta a; f [n][3]; J [n][15]
__global__ void k_stm_core(Model mp, const double *in, double *f, double *J, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double *v = in + (size_t)i * 5;
    double ff[3], JJ[3][5];
    stm_core(mp, v[0], v[1], v[2], v[3], v[4], ff, JJ);
    for (int r = 0; r < 3; r++) {
        f[(size_t)i * 3 + r] = ff[r];
        for (int c = 0; c < 5; c++) J[(size_t)i * 15 + r * 5 + c] = JJ[r][c];
    }
}

// four lanes (one DPP quad) per item; in [n][6] = vl vt r delta a psi; every lane of the quad stores what it ends with:
// f [n][4][3], J [n][4][15], sc [n][4][2] = sin psi, cos psi. Lanes beyond the last item shadow it and store nothing.
__global__ void k_stm_core_quad(Model mp, const double *in, double *f, double *J, double *sc, int n)
{
    const int tid = blockIdx.x * TPB + threadIdx.x;
    const int item = tid >> 2, ql = tid & 3;
    const int it = item < n ? item : n - 1;
    const double *v = in + (size_t)it * 6;
    const TyreLane t = tyre_lane(mp, ql);
    double ff[3], JJ[3][5], sn, cs;
    stm_core_quad(mp, t, v[0], v[1], v[2], v[3], v[4], v[5], ff, JJ, sn, cs);
    if (item >= n) return;
    const size_t o = (size_t)item * 4 + ql;
    for (int r = 0; r < 3; r++) {
        f[o * 3 + r] = ff[r];
        for (int c = 0; c < 5; c++) J[o * 15 + r * 5 + c] = JJ[r][c];
    }
    sc[o * 2] = sn; sc[o * 2 + 1] = cs;
}

// table 0: ggv_ax, 1: ggv_ay
__global__ void k_interp_lin(Model mp, const double *tab, const double *x, double *y, double *dy, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double a, b;
    interp_lin(mp.n_ggv, mp.ggv_v, tab[i] == 0.0 ? mp.ggv_ax : mp.ggv_ay, x[i], a, b);
    y[i] = a; dy[i] = b;
}

// in [n][3] = vl r a; out [n][4] = h g3 g5 g7
__global__ void k_h_con(Model mp, const double *in, double *out, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double h, g3, g5, g7;
    h_con(mp, in[(size_t)i * 3], in[(size_t)i * 3 + 1], in[(size_t)i * 3 + 2], h, g3, g5, g7);
    double *o = out + (size_t)i * 4;
    o[0] = h; o[1] = g3; o[2] = g5; o[3] = g7;
}

// x [n][8], u [n][2]; xn [n][8], Sp [n][2], S [n][42]
__global__ void k_rk4_sens(Model mp, const double *x, const double *u, double dt, int nsub, double *xn, double *Sp, double *S, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double x0[8], uu[2], xo[8], sp[2], s[6][7];
    for (int k = 0; k < 8; k++) x0[k] = x[(size_t)i * 8 + k];
    uu[0] = u[(size_t)i * 2]; uu[1] = u[(size_t)i * 2 + 1];
    rk4_sens(mp, x0, uu, dt, nsub, xo, sp, s);
    for (int k = 0; k < 8; k++) xn[(size_t)i * 8 + k] = xo[k];
    Sp[(size_t)i * 2] = sp[0]; Sp[(size_t)i * 2 + 1] = sp[1];
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 7; c++) S[(size_t)i * 42 + r * 7 + c] = s[r][c];
}

// eight lanes per item, lane = column (lin_cols_kernel's division); xn [n][8][8] (every lane's copy), Sc [n][8][6]
__global__ void k_rk4_sens_col(Model mp, const double *x, const double *u, double dt, int nsub, double *xn, double *Sc, int n)
{
    const int tid = blockIdx.x * TPB + threadIdx.x;
    const int item = tid >> 3, col = tid & 7;
    const int it = item < n ? item : n - 1;
    const TyreLane t = tyre_lane(mp, col);
    double x0[8], uu[2], xo[8], sc[6];
    for (int k = 0; k < 8; k++) x0[k] = x[(size_t)it * 8 + k];
    uu[0] = u[(size_t)it * 2]; uu[1] = u[(size_t)it * 2 + 1];
    rk4_sens_col(mp, t, col, x0, uu, dt, nsub, xo, sc);
    if (item >= n) return;
    const size_t o = (size_t)item * 8 + col;
    for (int k = 0; k < 8; k++) xn[o * 8 + k] = xo[k];
    for (int k = 0; k < 6; k++) Sc[o * 6 + k] = sc[k];
}

}  // namespace

extern "C" int probe_primitive(int which, const double *x, double *o0, double *o1, int n)
{
    if (n < 1 || which < 0 || which > 5) return -1;
    Bufs b;
    double *dx = b.in(x, n), *d0 = b.out(n), *d1 = b.out(n);
    if (b.err == hipSuccess) k_primitive<<<blocks(n), TPB>>>(which, dx, d0, d1, n);
    b.launched();
    b.back(o0, d0, n); b.back(o1, d1, n);
    return (int)b.err;
}

extern "C" int probe_wrap_yaw(const double *x, double *o, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dx = b.in(x, n), *d0 = b.out(n);
    if (b.err == hipSuccess) k_wrap_yaw<<<blocks(n), TPB>>>(dx, d0, n);
    b.launched();
    b.back(o, d0, n);
    return (int)b.err;
}

extern "C" int probe_pacejka(int front, const double *al, double *Fy, double *dFy, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dx = b.in(al, n), *d0 = b.out(n), *d1 = b.out(n);
    if (b.err == hipSuccess) k_pacejka<<<blocks(n), TPB>>>(g_model, front, dx, d0, d1, n);
    b.launched();
    b.back(Fy, d0, n); b.back(dFy, d1, n);
    return (int)b.err;
}

extern "C" int probe_stm_core(const double *in, double *f, double *J, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dx = b.in(in, (size_t)n * 5), *d0 = b.out((size_t)n * 3), *d1 = b.out((size_t)n * 15);
    if (b.err == hipSuccess) k_stm_core<<<blocks(n), TPB>>>(g_model, dx, d0, d1, n);
    b.launched();
    b.back(f, d0, (size_t)n * 3); b.back(J, d1, (size_t)n * 15);
    return (int)b.err;
}

extern "C" int probe_stm_core_quad(const double *in, double *f, double *J, double *sc, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dx = b.in(in, (size_t)n * 6), *d0 = b.out((size_t)n * 12), *d1 = b.out((size_t)n * 60), *d2 = b.out((size_t)n * 8);
    if (b.err == hipSuccess) k_stm_core_quad<<<blocks((long long)n * 4), TPB>>>(g_model, dx, d0, d1, d2, n);
    b.launched();
    b.back(f, d0, (size_t)n * 12); b.back(J, d1, (size_t)n * 60); b.back(sc, d2, (size_t)n * 8);
    return (int)b.err;
}

extern "C" int probe_interp_lin(const double *tab, const double *x, double *y, double *dy, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dt = b.in(tab, n), *dx = b.in(x, n), *d0 = b.out(n), *d1 = b.out(n);
    if (b.err == hipSuccess) k_interp_lin<<<blocks(n), TPB>>>(g_model, dt, dx, d0, d1, n);
    b.launched();
    b.back(y, d0, n); b.back(dy, d1, n);
    return (int)b.err;
}

extern "C" int probe_h_con(const double *in, double *out, int n)
{
    if (n < 1) return -1;
    Bufs b;
    double *dx = b.in(in, (size_t)n * 3), *d0 = b.out((size_t)n * 4);
    if (b.err == hipSuccess) k_h_con<<<blocks(n), TPB>>>(g_model, dx, d0, n);
    b.launched();
    b.back(out, d0, (size_t)n * 4);
    return (int)b.err;
}

extern "C" int probe_rk4_sens(const double *x, const double *u, double dt, int nsub, double *xn, double *Sp, double *S, int n)
{
    if (n < 1 || nsub < 1) return -1;
    Bufs b;
    double *dx = b.in(x, (size_t)n * 8), *du = b.in(u, (size_t)n * 2), *d0 = b.out((size_t)n * 8), *d1 = b.out((size_t)n * 2), *d2 = b.out((size_t)n * 42);
    if (b.err == hipSuccess) k_rk4_sens<<<blocks(n), TPB>>>(g_model, dx, du, dt, nsub, d0, d1, d2, n);
    b.launched();
    b.back(xn, d0, (size_t)n * 8); b.back(Sp, d1, (size_t)n * 2); b.back(S, d2, (size_t)n * 42);
    return (int)b.err;
}

extern "C" int probe_rk4_sens_col(const double *x, const double *u, double dt, int nsub, double *xn, double *Sc, int n)
{
    if (n < 1 || nsub < 1) return -1;
    Bufs b;
    double *dx = b.in(x, (size_t)n * 8), *du = b.in(u, (size_t)n * 2), *d0 = b.out((size_t)n * 64), *d1 = b.out((size_t)n * 48);
    if (b.err == hipSuccess) k_rk4_sens_col<<<blocks((long long)n * 8), TPB>>>(g_model, dx, du, dt, nsub, d0, d1, n);
    b.launched();
    b.back(xn, d0, (size_t)n * 64); b.back(Sc, d1, (size_t)n * 48);
    return (int)b.err;
}
