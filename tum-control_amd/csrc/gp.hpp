// gp.hpp -- host side of K16 (gp_kernels.hpp): tum_gp, the data of one GP on the device, and the chain that evaluates its marginal
// log-likelihood with the gradient, or its factor V = L^-1 with a = A^-1 (y - c). Host code only, included by tum_nmpc.hip behind
// bo.hpp (DevBuf, LAUNCH, bo_finite).
#pragma once

constexpr int GP_MAXN = 4096;
enum { GP_T_KERN, GP_T_CHOL, GP_T_TRINV, GP_T_AINV, GP_T_ALPHA, GP_T_GRAD, GP_T_REDUCE, GP_TIMERS };

struct tum_gp {
    int device = 0;
    hipStream_t stream = nullptr;
    bool have_data = false, profile = false;
    int n = 0, d = 0;
    size_t cap = 0;                                 // np the three matrices were allocated for
    DevBuf<double> X, y, fixed, A, V, M, r, w, alpha, apart, gpart, minpiv, out;
    DevBuf<int> bad;
    hipEvent_t ev[GP_TIMERS + 1] = {};
    double ms[GP_TIMERS] = {};
};

static int gp_pad(int n) { return (n + GP_NB - 1) / GP_NB * GP_NB; }

extern "C" tum_gp *tum_gp_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device: libtumnmpc has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= ndev) { fail("tum_gp_create: device ordinal out of range"); return nullptr; }
    DevGuard guard(device); if (!guard.ok) { fail("hipSetDevice failed"); return nullptr; }
    tum_gp *g = new tum_gp();
    g->device = device;
    bool ok = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i <= GP_TIMERS; i++) ok = hipEventCreate(&g->ev[i]) == hipSuccess;
    if (!ok) { fail("tum_gp_create: stream or events"); tum_gp_free(g); return nullptr; }
    return g;
}

extern "C" void tum_gp_free(tum_gp *g)
{
    if (!g) return;
    DevGuard guard(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (int i = 0; i <= GP_TIMERS; i++)
        if (g->ev[i]) (void)hipEventDestroy(g->ev[i]);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;          // (the buffers free under the guard)
}

extern "C" int tum_gp_data(tum_gp *g, const double *X, const double *y, const double *fixed_noise, int n, int d)
{
    if (!g || !X || !y) return fail("null argument");
    if (n < 1 || n > GP_MAXN) return fail("tum_gp_data: n outside 1..4096");
    if (d < 1 || d > GP_MAXD) return fail("tum_gp_data: d outside 1..16");
    if (!bo_finite(X, (size_t)n * d) || !bo_finite(y, n) || (fixed_noise && !bo_finite(fixed_noise, n)))
        return fail("tum_gp_data: X, y or the noise holds a NaN or an infinity");
    DevGuard guard(g->device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(g->stream));
    g->have_data = false;
    const size_t np = gp_pad(n), nb = np / GP_NB;
    if (np > g->cap) {          // the three matrices grow on demand and never shrink; the chain writes every tile it reads
        g->cap = 0;
        HIPCHK(g->A.alloc(np * np, false)); HIPCHK(g->V.alloc(np * np, false)); HIPCHK(g->M.alloc(np * np, false));
        g->cap = np;
    }
    BOCHK(bo_upload(g->X, X, (size_t)n * d));
    BOCHK(bo_upload(g->y, y, n));
    HIPCHK(g->fixed.alloc(n));          // (zero-filled)
    if (fixed_noise) HIPCHK(hipMemcpy(g->fixed.get(), fixed_noise, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(g->r.reserve(np)); HIPCHK(g->w.reserve(np)); HIPCHK(g->alpha.reserve(np));
    HIPCHK(g->apart.reserve(nb * np)); HIPCHK(g->gpart.reserve(nb * (nb + 1) / 2 * GP_NG));
    HIPCHK(g->minpiv.reserve(nb)); HIPCHK(g->bad.reserve(nb)); HIPCHK(g->out.reserve(GP_MAXD + 5));
    HIPCHK(hipDeviceSynchronize());
    g->n = n; g->d = d; g->have_data = true;
    return 0;
}

// the blocked right-looking Cholesky of the lower tiles of f.A, in place: per block column the diagonal block (with its inverse into the
// diagonal tile of f.V), the panel below it and the trailing update. Shared with the posterior covariance of bo_model.hpp. (Defined
// behind gp_chain: the kernels keep the order of first use they had.)
static int gp_cholesky(GpFacArgs f, int nb, hipStream_t st);

// the chain on the handle's stream. grad: A^-1 and the gradient; alpha: a = V^T w (implied by grad).
static int gp_chain(tum_gp *g, const double *theta, int learn, double floor_, bool want_alpha, bool want_grad)
{
    const int n = g->n, d = g->d, np = gp_pad(n), nb = np / GP_NB;
    hipStream_t st = g->stream;
    int ti = 0;
    auto mark = [&]() { if (g->profile) (void)hipEventRecord(g->ev[ti], st); ti++; };
    const double s = std::exp(theta[d]), learned = std::exp(theta[d + 2]);
    mark();
    {
        GpKernArgs a{};
        a.n = n; a.np = np; a.d = d; a.learn = learn; a.X = g->X.get(); a.y = g->y.get(); a.fixed = g->fixed.get();
        for (int j = 0; j < d; j++) a.ils[j] = std::exp(-theta[j]);
        a.s = s; a.c = theta[d + 1]; a.floor = floor_; a.learned = learned; a.A = g->A.get(); a.r = g->r.get();
        LAUNCH(gp_kern_kernel<>, dim3(nb, nb), dim3(256), 0, st, a);
    }
    mark();
    GpFacArgs f{};
    f.n = n; f.np = np; f.A = g->A.get(); f.V = g->V.get(); f.M = g->M.get(); f.minpiv = g->minpiv.get(); f.bad = g->bad.get();
    BOCHK(gp_cholesky(f, nb, st));
    mark();
    if (nb > 1) LAUNCH(gp_lhat_kernel<>, dim3(nb, nb, 4), dim3(64), 0, st, f);
    for (int sdiag = 1; sdiag < nb; sdiag++) {
        f.s = sdiag;
        LAUNCH(gp_trinv_kernel<>, dim3(nb - sdiag, 4, 4), dim3(64), 0, st, f);
    }
    mark();
    if (want_grad) LAUNCH(gp_ainv_kernel<>, dim3(nb, nb), dim3(256), 0, st, f);
    mark();
    GpVecArgs v{};
    v.n = n; v.np = np; v.nb = nb; v.d = d; v.learn = learn; v.want_grad = want_grad;
    v.V = g->V.get(); v.M = g->M.get(); v.L = g->A.get(); v.X = g->X.get(); v.r = g->r.get();
    v.w = g->w.get(); v.alpha = g->alpha.get(); v.apart = g->apart.get(); v.gpart = g->gpart.get();
    v.minpiv = g->minpiv.get(); v.bad = g->bad.get();
    for (int j = 0; j < d; j++) v.ils[j] = std::exp(-theta[j]);
    v.s = s; v.learned = learned; v.thr = 1e-7 * std::exp(0.5 * theta[d]); v.out = g->out.get();
    LAUNCH(gp_w_kernel<>, dim3(np / 4), dim3(256), 0, st, v);
    if (want_alpha || want_grad) {
        LAUNCH(gp_alpha_kernel<>, dim3(nb, nb), dim3(64), 0, st, v);
        LAUNCH(gp_asum_kernel<>, dim3(nb), dim3(64), 0, st, v);
    }
    mark();
    if (want_grad) LAUNCH(gp_grad_kernel<>, dim3(nb, nb), dim3(256), 0, st, v);
    mark();
    LAUNCH(gp_reduce_kernel<>, dim3(1), dim3(256), 0, st, v);
    mark();
    return 0;
}

// (Keep this definition BEHIND gp_chain: a template kernel's code is emitted where it is first used, and gp_chain's first uses fix
// the order the K16 kernels have in the code object. Moving it in front would put potrf / trsm / syrk before gp_kern_kernel.)
static int gp_cholesky(GpFacArgs f, int nb, hipStream_t st)
{
    for (int k = 0; k < nb; k++) {
        f.k = k;
        LAUNCH(gp_potrf_kernel<>, dim3(1), dim3(256), 0, st, f);
        const int m = nb - k - 1;
        if (m > 0) {
            LAUNCH(gp_trsm_kernel<>, dim3(m), dim3(256), 0, st, f);
            LAUNCH(gp_syrk_kernel<>, dim3(m, m), dim3(256), 0, st, f);
        }
    }
    return 0;
}

static int gp_times(tum_gp *g)
{
    if (g->profile)
        for (int i = 0; i < GP_TIMERS; i++) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, g->ev[i], g->ev[i + 1]));
            g->ms[i] = ms;
        }
    return 0;
}

static int gp_check(tum_gp *g, const double *theta, double floor_, const char *who)
{
    if (!g->have_data) return fail(std::string(who) + ": no data (tum_gp_data first)");
    if (!bo_finite(theta, g->d + 3) || !std::isfinite(floor_)) return fail(std::string(who) + ": theta or the noise floor holds a NaN or an infinity");
    return 0;
}

extern "C" int tum_gp_mll(tum_gp *g, const double *theta, int learn_noise, double noise_floor, double *mll_out, double *grad_out, int *ok_out)
{
    if (!g || !theta || !mll_out || !ok_out) return fail("null argument");
    BOCHK(gp_check(g, theta, noise_floor, "tum_gp_mll"));
    DevGuard guard(g->device); GUARD_OK(guard);
    BOCHK(gp_chain(g, theta, learn_noise != 0, noise_floor, false, grad_out != nullptr));
    double out[GP_MAXD + 5];
    HIPCHK(hipMemcpyAsync(out, g->out.get(), sizeof(double) * (g->d + 5), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    BOCHK(gp_times(g));
    *mll_out = out[0]; *ok_out = out[g->d + 4] != 0.0;
    if (grad_out)
        for (int j = 0; j < g->d + 3; j++) grad_out[j] = out[1 + j];
    return 0;
}

extern "C" int tum_gp_factor(tum_gp *g, const double *theta, int learn_noise, double noise_floor, double *V_out, double *a_out, int *ok_out)
{
    if (!g || !theta || !V_out || !a_out || !ok_out) return fail("null argument");
    BOCHK(gp_check(g, theta, noise_floor, "tum_gp_factor"));
    DevGuard guard(g->device); GUARD_OK(guard);
    BOCHK(gp_chain(g, theta, learn_noise != 0, noise_floor, true, false));
    const size_t n = g->n, np = gp_pad(g->n);
    double out[GP_MAXD + 5];
    HIPCHK(hipMemcpyAsync(out, g->out.get(), sizeof(double) * (g->d + 5), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpy2DAsync(V_out, sizeof(double) * n, g->V.get(), sizeof(double) * np, sizeof(double) * n, n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(a_out, g->alpha.get(), sizeof(double) * n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    BOCHK(gp_times(g));
    for (size_t i = 0; i < n; i++)          // (the tiles right of the diagonal tile are never written on the device)
        for (size_t k = i + 1; k < n; k++) V_out[i * n + k] = 0.0;
    *ok_out = out[g->d + 4] != 0.0;
    return 0;
}

extern "C" int tum_gp_profile(tum_gp *g, int on, double *ms_out)
{
    if (!g) return fail("null argument");
    g->profile = on != 0;
    if (ms_out)
        for (int i = 0; i < GP_TIMERS; i++) ms_out[i] = g->ms[i];
    return 0;
}
