// bo.hpp -- host side of K15 (bo_kernels.hpp): tum_bo, the upload of a model in the operand layouts of the product kernels, and one
// evaluation of C candidates in chunks of BO_CHUNK. Host code only, included by tum_nmpc.hip behind sim_loop.hpp (DevBuf, LAUNCH).
#pragma once

constexpr int BO_CHUNK = 512;          // candidates per pass of the kernel chain: bounds the column-tile buffers, not C
constexpr int BO_MAXN = 4096, BO_MAXB = 512, BO_MAXS = 4096;
enum { BO_T_KERN, BO_T_TRI, BO_T_MOM, BO_T_CROSS, BO_T_TRI2, BO_T_HVI, BO_T_FINAL, BO_TIMERS };

// what tum_bom_prune, tum_bom_fronts, tum_bom_build and tum_bom_append (bo_model.hpp) keep on the device: grown on demand, never read before the call wrote it
enum { BOM_T_KERN, BOM_T_H, BOM_T_SIG, BOM_T_CHOL, BOM_T_MEAN, BOM_T_DRAW, BOM_T_DOM, BOM_TIMERS };
constexpr int BOM_EVENTS = 2 * (BOM_T_DOM + 1) + 2;
enum { BOMB_T_KERN, BOMB_T_H, BOMB_T_SIG, BOMB_T_CHOL, BOMB_T_TRINV, BOMB_T_MEAN, BOMB_T_DRAW, BOMB_T_PACK, BOMB_T_FRONT, BOMB_TIMERS };
constexpr int BOMB_EVENTS = 2 * (BOMB_T_FRONT + 1) + 2;
struct BomWork {
    DevBuf<double> X, K, W, H, A, Z, a, m, F, minpiv, Fb, fronts;
    DevBuf<int> keep, bad, count;
    // tum_bom_build: the dense baseline posterior of the resident model, per objective, for tum_bom_model_read
    bool built = false;
    DevBuf<double> Kbb, Mt, Hd[2], Ld[2], Rd[2], mub[2], Fbm, Zf[2];
    DevBuf<int> okapp;
    int cap = 0, ldb = 0, ncol = 0;          // baseline points the resident arrays hold room for; their leading dimension; columns of Zfull
    hipEvent_t ev[BOM_EVENTS] = {};
    double ms[BOM_TIMERS] = {};
    bool profile = false;
    hipEvent_t evb[BOMB_EVENTS] = {};          // tum_bom_build's timers
    double msb[BOMB_TIMERS] = {};
    bool profile_build = false;
};

struct tum_bo {
    BomWork work;
    int device = 0;
    hipStream_t stream = nullptr;
    bool have_model = false, profile = false;
    int d = 0, n[BO_SETS] = {}, np[BO_SETS] = {}, S = 0, nts = 0, P_max = 0, K = 0;
    double s[BO_GP] = {}, c[BO_GP] = {}, jitter[2] = {}, ref[2] = {}, eps = 0;
    DevBuf<double> X[3], ils[BO_GP], a[BO_GP], V[BO_GP], H[2], R[2], Z[2], zeta[2], fronts, gh;
    DevBuf<int> count;
    // per chunk
    DevBuf<double> x, k[BO_SETS], q[2], part[BO_GP], dot[BO_GP], sig[2], l[2], llpart[2], mom, hvpart, alpha, detail;
    hipEvent_t ev[BO_TIMERS + 1] = {};
    double ms[BO_TIMERS] = {};
};

#define BOCHK(x) do { if (x) return 1; } while (0)

static int bo_pad16(int n) { return (n + 15) & ~15; }

// the lower triangle of the n x n row-major M in the A-operand layout of bo_tri_kernel
static std::vector<double> bo_pack_tri(const double *M, int n)
{
    const int nt = bo_pad16(n) >> 4;
    std::vector<double> out(bo_tri_off(nt) * 64, 0.0);
    for (int t = 0; t < nt; t++)
        for (int q = 0; q < 4 * (t + 1); q++) {
            double *blk = out.data() + (bo_tri_off(t) + q) * 64;
            for (int lane = 0; lane < 64; lane++) {
                const int r = 16 * t + (lane & 15), k = 4 * q + (lane >> 4);
                if (r < n && k <= r) blk[lane] = M[(size_t)r * n + k];
            }
        }
    return out;
}

// the rows x cols row-major M as [rows padded / 16][cols padded to 16 / 4][64]
static std::vector<double> bo_pack_dense(const double *M, int rows, int cols)
{
    const int nt = bo_pad16(rows) >> 4, nq = bo_pad16(cols) >> 2;
    std::vector<double> out((size_t)nt * nq * 64, 0.0);
    for (int t = 0; t < nt; t++)
        for (int q = 0; q < nq; q++) {
            double *blk = out.data() + ((size_t)t * nq + q) * 64;
            for (int lane = 0; lane < 64; lane++) {
                const int r = 16 * t + (lane & 15), k = 4 * q + (lane >> 4);
                if (r < rows && k < cols) blk[lane] = M[(size_t)r * cols + k];
            }
        }
    return out;
}

static int bo_upload(DevBuf<double> &buf, const double *src, size_t n, size_t padded = 0)
{
    if (padded < n) padded = n;
    HIPCHK(buf.alloc(padded));          // (zero-filled: what lies behind n stays zero)
    if (n) HIPCHK(hipMemcpy(buf.get(), src, sizeof(double) * n, hipMemcpyHostToDevice));
    return 0;
}

static bool bo_finite(const double *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

extern "C" tum_bo *tum_bo_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device: libtumnmpc has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= ndev) { fail("tum_bo_create: device ordinal out of range"); return nullptr; }
    DevGuard guard(device); if (!guard.ok) { fail("hipSetDevice failed"); return nullptr; }
    tum_bo *b = new tum_bo();
    b->device = device;
    bool ok = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i <= BO_TIMERS; i++) ok = hipEventCreate(&b->ev[i]) == hipSuccess;
    if (!ok) { fail("tum_bo_create: stream or events"); tum_bo_free(b); return nullptr; }
    return b;
}

extern "C" void tum_bo_free(tum_bo *b)
{
    if (!b) return;
    DevGuard guard(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (int i = 0; i <= BO_TIMERS; i++)
        if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
    for (int i = 0; i < BOM_EVENTS; i++)
        if (b->work.ev[i]) (void)hipEventDestroy(b->work.ev[i]);
    for (int i = 0; i < BOMB_EVENTS; i++)
        if (b->work.evb[i]) (void)hipEventDestroy(b->work.evb[i]);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;          // (the buffers free under the guard)
}

static int bo_model_gp(tum_bo *b, const tum_bo_model_desc *m)
{
    const double *Xs[3] = {m->Xt, m->Xb, m->Xc};
    const int ns[3] = {m->n_t, m->n_b, m->n_c};
    for (int i = 0; i < 3; i += 2) BOCHK(bo_upload(b->X[i], Xs[i], (size_t)ns[i] * m->d));
    for (int g = 0; g < BO_GP; g++) {
        const int n = g < 2 ? m->n_t : m->n_c;
        BOCHK(bo_upload(b->ils[g], m->ils[g], m->d));
        BOCHK(bo_upload(b->a[g], m->a[g], n, bo_pad16(n)));
        const std::vector<double> V = bo_pack_tri(m->V[g], n);
        BOCHK(bo_upload(b->V[g], V.data(), V.size()));
        b->s[g] = m->s[g]; b->c[g] = m->c[g];
    }
    return 0;
}

// the sizes of a model, as tum_bo_model and tum_bom_build (bo_model.hpp) set them
static void bo_model_sizes(tum_bo *b, int d, int n_t, int n_c, int n_b, int S, int P_max, int K, double eps)
{
    b->d = d;
    const int ns[BO_SETS] = {n_t, n_t, n_c, n_c, n_b, n_b};
    for (int g = 0; g < BO_SETS; g++) { b->n[g] = ns[g]; b->np[g] = bo_pad16(ns[g]); }
    b->S = S; b->nts = bo_pad16(S) >> 4; b->P_max = P_max; b->K = K; b->eps = eps;
}

// the quadrature rule and the chunk's buffers of a model whose sizes are set
static int bo_model_chunk(tum_bo *b, const double *gh_x, const double *gh_w)
{
    std::vector<double> gh(2 * BO_MAXK, 0.0);
    for (int i = 0; i < b->K; i++) { gh[i] = gh_x[i]; gh[BO_MAXK + i] = gh_w[i]; }
    BOCHK(bo_upload(b->gh, gh.data(), gh.size()));
    // the chunk's buffers: every element of them is written by the chain before it is read
    const size_t nct = BO_CHUNK / 16;
    HIPCHK(b->x.reserve((size_t)BO_CHUNK * BO_MAXD));
    for (int g = 0; g < BO_SETS; g++) HIPCHK(b->k[g].alloc(nct * b->np[g] * 16, false));
    for (int g = 0; g < BO_GP; g++) { HIPCHK(b->part[g].alloc(nct * b->np[g], false)); HIPCHK(b->dot[g].alloc(nct * b->np[g], false)); }
    for (int o = 0; o < 2; o++) {
        HIPCHK(b->q[o].alloc(nct * b->np[0] * 16, false));
        HIPCHK(b->sig[o].alloc(nct * b->np[4] * 16, false));
        HIPCHK(b->l[o].alloc(nct * b->np[4] * 16, false));
        HIPCHK(b->llpart[o].alloc(nct * b->np[4], false));
    }
    HIPCHK(b->mom.reserve((size_t)BO_GP * BO_CHUNK * 2));
    HIPCHK(b->hvpart.alloc(nct * b->nts * 16, false));
    HIPCHK(b->alpha.reserve(BO_CHUNK)); HIPCHK(b->detail.reserve((size_t)BO_CHUNK * BO_DETAIL));
    return 0;
}

extern "C" int tum_bo_model(tum_bo *b, const tum_bo_model_desc *m)
{
    if (!b || !m) return fail("null argument");
    if (m->d < 1 || m->d > BO_MAXD) return fail("tum_bo_model: d outside 1..16");
    if (m->n_t < 1 || m->n_t > BO_MAXN) return fail("tum_bo_model: n_t outside 1..4096");
    if (m->n_c < 1 || m->n_c > BO_MAXN) return fail("tum_bo_model: n_c outside 1..4096");
    if (m->n_b < 1 || m->n_b > BO_MAXB) return fail("tum_bo_model: n_b outside 1..512");
    if (m->S < 1 || m->S > BO_MAXS) return fail("tum_bo_model: S outside 1..4096");
    if (m->P_max < 1 || m->P_max > m->n_b) return fail("tum_bo_model: P_max outside 1..n_b");
    if (m->K < 1 || m->K > BO_MAXK) return fail("tum_bo_model: K outside 1..64");
    if (!m->Xb || !m->fronts || !m->front_count || !m->gh_x || !m->gh_w) return fail("tum_bo_model: null array");
    for (int o = 0; o < 2; o++)
        if (!m->H[o] || !m->R[o] || !m->Z[o] || !m->zeta[o]) return fail("tum_bo_model: null array");
    if (m->keep_gp) {
        if (!b->have_model || b->d != m->d || b->n[0] != m->n_t || b->n[2] != m->n_c)
            return fail("tum_bo_model: keep_gp needs a model of the same d, n_t and n_c");
    } else {
        if (!m->Xt || !m->Xc) return fail("tum_bo_model: null array");
        for (int g = 0; g < BO_GP; g++)
            if (!m->ils[g] || !m->a[g] || !m->V[g]) return fail("tum_bo_model: null array");
    }
    for (int s = 0; s < m->S; s++)
        if (m->front_count[s] < 0 || m->front_count[s] > m->P_max) return fail("tum_bo_model: front_count outside 0..P_max");
    DevGuard guard(b->device); GUARD_OK(guard);
    HIPCHK(hipStreamSynchronize(b->stream));
    b->have_model = false; b->work.built = false;
    if (!m->keep_gp) BOCHK(bo_model_gp(b, m));
    bo_model_sizes(b, m->d, m->n_t, m->n_c, m->n_b, m->S, m->P_max, m->K, m->eps);
    BOCHK(bo_upload(b->X[1], m->Xb, (size_t)m->n_b * m->d));
    for (int o = 0; o < 2; o++) {
        b->jitter[o] = m->jitter[o]; b->ref[o] = m->ref[o];
        const std::vector<double> H = bo_pack_dense(m->H[o], m->n_b, m->n_t), R = bo_pack_tri(m->R[o], m->n_b),
                                  Z = bo_pack_dense(m->Z[o], m->S, m->n_b);
        BOCHK(bo_upload(b->H[o], H.data(), H.size()));
        BOCHK(bo_upload(b->R[o], R.data(), R.size()));
        BOCHK(bo_upload(b->Z[o], Z.data(), Z.size()));
        BOCHK(bo_upload(b->zeta[o], m->zeta[o], m->S, (size_t)16 * b->nts));
    }
    BOCHK(bo_upload(b->fronts, m->fronts, (size_t)m->S * m->P_max * 2));
    HIPCHK(b->count.alloc(m->S));
    HIPCHK(hipMemcpy(b->count.get(), m->front_count, sizeof(int) * m->S, hipMemcpyHostToDevice));
    BOCHK(bo_model_chunk(b, m->gh_x, m->gh_w));
    HIPCHK(hipDeviceSynchronize());
    b->have_model = true;
    return 0;
}

// one chunk of C <= BO_CHUNK candidates, already on the device in b->x
static int bo_chain(tum_bo *b, int C)
{
    const int nct = ((C + 16 * BO_NCT - 1) / (16 * BO_NCT)) * BO_NCT, ctr = (C + 15) / 16;
    hipStream_t st = b->stream;
    int ti = 0;
    auto mark = [&]() { if (b->profile) (void)hipEventRecord(b->ev[ti], st); ti++; };
    mark();
    {
        BoKernArgs a{};
        a.d = b->d; a.C = C; a.nct = nct; a.x = b->x.get();
        int npmax = 0;
        for (int g = 0; g < BO_SETS; g++) {
            a.n[g] = b->n[g]; a.np[g] = b->np[g]; a.k[g] = b->k[g].get();
            a.X[g] = b->X[g < 2 ? 0 : (g < 4 ? 2 : 1)].get();
            a.ils[g] = b->ils[g < 4 ? g : g - 4].get(); a.s[g] = b->s[g < 4 ? g : g - 4];
            npmax = std::max(npmax, b->np[g]);
        }
        LAUNCH(bo_kern_kernel, dim3(npmax / 16, nct, BO_SETS), dim3(256), 0, st, a);
    }
    mark();
    {
        BoTriArgs a{};
        a.n_units = BO_GP; a.nct = nct;
        int first = 0;
        for (int g = 0; g < BO_GP; g++) {
            a.first[g] = first; first += b->np[g] / 16;
            a.np[g] = b->np[g]; a.T[g] = b->V[g].get(); a.in[g] = b->k[g].get(); a.out[g] = g < 2 ? b->q[g].get() : nullptr;
            a.part[g] = b->part[g].get(); a.a[g] = b->a[g].get(); a.dot[g] = b->dot[g].get();
        }
        a.first[BO_GP] = first;
        LAUNCH(bo_tri_kernel, dim3(first, nct / BO_NCT), dim3(64), 0, st, a);
    }
    mark();
    {
        BoMomArgs a{};
        a.C = C; a.cp = BO_CHUNK; a.mom = b->mom.get();
        for (int g = 0; g < BO_GP; g++) {
            a.n[g] = b->n[g]; a.np[g] = b->np[g]; a.part[g] = b->part[g].get(); a.dot[g] = b->dot[g].get(); a.c[g] = b->c[g];
        }
        LAUNCH(bo_moments_kernel, dim3((C + 63) / 64, BO_GP), dim3(64), 0, st, a);
    }
    mark();
    {
        BoCrossArgs a{};
        a.nct = nct; a.npt = b->np[0]; a.npb = b->np[4];
        for (int o = 0; o < 2; o++) { a.H[o] = b->H[o].get(); a.q[o] = b->q[o].get(); a.kb[o] = b->k[4 + o].get(); a.sig[o] = b->sig[o].get(); }
        LAUNCH(bo_cross_kernel, dim3(a.npb / 16, nct / BO_NCT, 2), dim3(64), 0, st, a);
    }
    mark();
    {
        BoTriArgs a{};
        a.n_units = 2; a.nct = nct;
        for (int o = 0; o < 2; o++) {
            a.first[o] = o * (b->np[4] / 16);
            a.np[o] = b->np[4]; a.T[o] = b->R[o].get(); a.in[o] = b->sig[o].get(); a.out[o] = b->l[o].get(); a.part[o] = b->llpart[o].get();
        }
        a.first[2] = 2 * (b->np[4] / 16);
        LAUNCH(bo_tri_kernel, dim3(a.first[2], nct / BO_NCT), dim3(64), 0, st, a);
    }
    mark();
    {
        BoHviArgs a{};
        a.C = C; a.cp = BO_CHUNK; a.S = b->S; a.npb = b->np[4]; a.nts = b->nts; a.P_max = b->P_max;
        for (int o = 0; o < 2; o++) {
            a.Z[o] = b->Z[o].get(); a.zeta[o] = b->zeta[o].get(); a.l[o] = b->l[o].get(); a.llpart[o] = b->llpart[o].get();
            a.s[o] = b->s[o]; a.jitter[o] = b->jitter[o]; a.ref[o] = b->ref[o];
        }
        a.mom = b->mom.get(); a.fronts = b->fronts.get(); a.count = b->count.get(); a.part = b->hvpart.get();
        LAUNCH(bo_hvi_kernel, dim3(b->nts, ctr), dim3(64), 0, st, a);
    }
    mark();
    {
        BoFinalArgs a{};
        a.C = C; a.cp = BO_CHUNK; a.S = b->S; a.nts = b->nts; a.npb = b->np[4]; a.K = b->K;
        a.mom = b->mom.get(); a.hvpart = b->hvpart.get();
        for (int o = 0; o < 2; o++) { a.llpart[o] = b->llpart[o].get(); a.jitter[o] = b->jitter[o]; }
        for (int g = 0; g < BO_GP; g++) a.s[g] = b->s[g];
        a.eps = b->eps; a.gh_x = b->gh.get(); a.gh_w = b->gh.get() + BO_MAXK;
        a.alpha = b->alpha.get(); a.detail = b->detail.get();
        LAUNCH(bo_final_kernel, dim3((C + 63) / 64), dim3(64), 0, st, a);
    }
    mark();
    return 0;
}

extern "C" int tum_bo_evaluate(tum_bo *b, const double *X, int C, double *alpha_out, double *detail_out)
{
    if (!b || !X || !alpha_out) return fail("null argument");
    if (!b->have_model) return fail("tum_bo_evaluate: no model (tum_bo_model first)");
    if (C < 1) return fail("tum_bo_evaluate: C < 1");
    if (!bo_finite(X, (size_t)C * b->d)) return fail("tum_bo_evaluate: X holds a NaN or an infinity");
    DevGuard guard(b->device); GUARD_OK(guard);
    for (int g = 0; g < BO_TIMERS; g++) b->ms[g] = 0.0;
    for (int c0 = 0; c0 < C; c0 += BO_CHUNK) {
        const int n = std::min(BO_CHUNK, C - c0);
        HIPCHK(hipMemcpyAsync(b->x.get(), X + (size_t)c0 * b->d, sizeof(double) * n * b->d, hipMemcpyHostToDevice, b->stream));
        if (bo_chain(b, n)) return 1;
        HIPCHK(hipMemcpyAsync(alpha_out + c0, b->alpha.get(), sizeof(double) * n, hipMemcpyDeviceToHost, b->stream));
        if (detail_out)
            HIPCHK(hipMemcpyAsync(detail_out + (size_t)c0 * BO_DETAIL, b->detail.get(), sizeof(double) * n * BO_DETAIL, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (b->profile)
            for (int g = 0; g < BO_TIMERS; g++) {
                float ms = 0;
                HIPCHK(hipEventElapsedTime(&ms, b->ev[g], b->ev[g + 1]));
                b->ms[g] += ms;
            }
    }
    return 0;
}

extern "C" int tum_bo_profile(tum_bo *b, int on, double *ms_out)
{
    if (!b) return fail("null argument");
    b->profile = on != 0;
    if (ms_out)
        for (int g = 0; g < BO_TIMERS; g++) ms_out[g] = b->ms[g];
    return 0;
}
