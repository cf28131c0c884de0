// bo_model.hpp -- host side of K17 (bo_model_kernels.hpp): tum_bom_prune, tum_bom_fronts, tum_bom_build, tum_bom_append and tum_bom_model_read on a
// tum_bo handle's stream and work buffers (BomWork, bo.hpp). Host code only, included by tum_nmpc.hip behind gp.hpp (gp_pad, gp_cholesky).
#pragma once

// the products with V stop at the diagonal tile: a V with anything above its diagonal would silently give another result than K V^T
static bool bom_lower(const double *V, size_t n)
{
    for (size_t i = 0; i < n; i++)
        for (size_t k = i + 1; k < n; k++)
            if (V[i * n + k] != 0.0) return false;
    return true;
}

// the rows x cols row-major host matrix into the [prows][ld] device matrix, zero around it
static int bom_upload(DevBuf<double> &buf, const double *src, size_t rows, size_t cols, size_t prows, size_t ld, hipStream_t st)
{
    HIPCHK(buf.reserve(prows * ld));
    HIPCHK(hipMemsetAsync(buf.get(), 0, sizeof(double) * prows * ld, st));
    HIPCHK(hipMemcpy2DAsync(buf.get(), sizeof(double) * ld, src, sizeof(double) * cols, sizeof(double) * cols, rows, hipMemcpyHostToDevice, st));
    return 0;
}

extern "C" void tum_bom_prune_desc_init(tum_bom_prune_desc *desc)
{
    if (!desc) return;
    *desc = tum_bom_prune_desc{};
    desc->struct_size = (int)sizeof(tum_bom_prune_desc);
}

// chain P of one objective on the stream: F[:, :, o] and the pivot flags of its factorisation into bad[o * nb ..]
static int bom_draws(tum_bo *b, const tum_bom_prune_desc *p, int o, int mark0)
{
    BomWork &w = b->work;
    const int n = p->n, d = p->d, S = p->S, np = gp_pad(n), nb = np / GP_NB, Sp = bo_pad16(S);
    hipStream_t st = b->stream;
    int ti = mark0;
    auto mark = [&]() { if (w.profile) (void)hipEventRecord(w.ev[ti], st); ti++; };
    BOCHK(bom_upload(w.W, p->V[o], n, n, np, np, st));
    BOCHK(bom_upload(w.Z, p->Z[o], S, n, Sp, np, st));
    BOCHK(bom_upload(w.a, p->a[o], 1, n, 1, np, st));
    mark();
    {
        BomKernArgs a{};
        a.nr = n; a.nc = n; a.ld = np; a.d = d; a.Xr = w.X.get(); a.Xc = w.X.get(); a.s = p->s[o]; a.K = w.K.get();
        for (int j = 0; j < d; j++) a.ils[j] = p->ils[o][j];
        LAUNCH(bom_kern_kernel<>, dim3(nb, nb), dim3(256), 0, st, a);
    }
    mark();
    BomMatArgs m{};
    m.n = n; m.np = np; m.ld = np; m.Kx = w.K.get(); m.K = w.K.get(); m.V = w.W.get(); m.H = w.H.get(); m.A = w.A.get();
    m.jitter = std::max(p->jitter, 1e-6 * p->s[o]);
    LAUNCH(bom_h_kernel<>, dim3(nb, nb), dim3(256), 0, st, m);
    mark();
    LAUNCH(bom_sig_kernel<>, dim3(nb, nb), dim3(256), 0, st, m);
    mark();
    GpFacArgs f{};          // (the diagonal blocks of L_p^-1 go where V was: H is formed, V is not read again)
    f.n = n; f.np = np; f.A = w.A.get(); f.V = w.W.get(); f.M = nullptr; f.minpiv = w.minpiv.get() + (size_t)o * nb; f.bad = w.bad.get() + (size_t)o * nb;
    BOCHK(gp_cholesky(f, nb, st));
    mark();
    BomDrawArgs a{};
    a.n = n; a.np = np; a.S = S; a.o = o; a.ldk = np; a.ldf = n; a.Kx = w.K.get(); a.a = w.a.get(); a.L = w.A.get(); a.Z = w.Z.get(); a.c = p->c[o];
    a.m = w.m.get(); a.F = w.F.get();
    LAUNCH(bom_mean_kernel<>, dim3(np / 4), dim3(256), 0, st, a);
    mark();
    LAUNCH(bom_draw_kernel<>, dim3(nb, Sp / 16), dim3(64), 0, st, a);
    mark();
    return 0;
}

extern "C" int tum_bom_prune(tum_bo *b, const tum_bom_prune_desc *p, int *keep_out, double *F_out, int *ok_out)
{
    if (!b || !p || !keep_out || !ok_out) return fail("null argument");
    if (p->struct_size != (int)sizeof(tum_bom_prune_desc)) return fail("tum_bom_prune: struct_size is not this library's sizeof(tum_bom_prune_desc)");
    if (p->n < 1 || p->n > BO_MAXN) return fail("tum_bom_prune: n outside 1..4096");
    if (p->S < 1 || p->S > BO_MAXS) return fail("tum_bom_prune: S outside 1..4096");
    const size_t n = p->n, S = p->S;
    if (p->F) {
        if (!bo_finite(p->F, S * n * 2)) return fail("tum_bom_prune: F holds a NaN or an infinity");
    } else {
        if (p->d < 1 || p->d > BO_MAXD) return fail("tum_bom_prune: d outside 1..16");
        if (!p->Xt) return fail("tum_bom_prune: null array");
        for (int o = 0; o < 2; o++)
            if (!p->ils[o] || !p->V[o] || !p->a[o] || !p->Z[o]) return fail("tum_bom_prune: null array");
        bool fin = bo_finite(p->Xt, n * p->d) && bo_finite(p->s, 2) && bo_finite(p->c, 2) && std::isfinite(p->jitter);
        for (int o = 0; fin && o < 2; o++)
            fin = bo_finite(p->ils[o], p->d) && bo_finite(p->V[o], n * n) && bo_finite(p->a[o], n) && bo_finite(p->Z[o], S * n);
        if (!fin) return fail("tum_bom_prune: an input holds a NaN or an infinity");
        if (!bom_lower(p->V[0], n) || !bom_lower(p->V[1], n)) return fail("tum_bom_prune: V is not zero above its diagonal");
    }
    DevGuard guard(b->device); GUARD_OK(guard);
    BomWork &w = b->work;
    hipStream_t st = b->stream;
    HIPCHK(hipStreamSynchronize(st));
    const size_t np = gp_pad(p->n), nb = np / GP_NB;
    if (w.profile)
        for (int i = 0; i < BOM_EVENTS; i++)
            if (!w.ev[i]) HIPCHK(hipEventCreate(&w.ev[i]));
    HIPCHK(w.F.reserve(S * n * 2)); HIPCHK(w.keep.reserve(n));
    std::vector<int> bad;
    if (p->F) {
        HIPCHK(hipMemcpyAsync(w.F.get(), p->F, sizeof(double) * S * n * 2, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(w.K.reserve(np * np)); HIPCHK(w.H.reserve(np * np)); HIPCHK(w.A.reserve(np * np));
        HIPCHK(w.m.reserve(np)); HIPCHK(w.minpiv.reserve(2 * nb)); HIPCHK(w.bad.reserve(2 * nb));
        BOCHK(bo_upload(w.X, p->Xt, n * p->d));
        for (int o = 0; o < 2; o++) BOCHK(bom_draws(b, p, o, o * (BOM_T_DOM + 1)));
        bad.resize(2 * nb);
        HIPCHK(hipMemcpyAsync(bad.data(), w.bad.get(), sizeof(int) * 2 * nb, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemsetAsync(w.keep.get(), 0, sizeof(int) * n, st));
    const int e0 = 2 * (BOM_T_DOM + 1);
    if (w.profile) (void)hipEventRecord(w.ev[e0], st);
    {
        BomDomArgs a{};
        a.n = p->n; a.F = w.F.get(); a.keep = w.keep.get();
        LAUNCH(bom_dom_kernel<>, dim3(p->S), dim3(256), sizeof(double) * 2 * n, st, a);
    }
    if (w.profile) (void)hipEventRecord(w.ev[e0 + 1], st);
    HIPCHK(hipMemcpyAsync(keep_out, w.keep.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    if (F_out) HIPCHK(hipMemcpyAsync(F_out, w.F.get(), sizeof(double) * S * n * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int ok = 1;
    for (int v : bad) ok &= v == 0;
    *ok_out = ok;
    if (w.profile) {
        for (int g = 0; g < BOM_TIMERS; g++) w.ms[g] = 0.0;
        float ms = 0;
        if (!p->F)
            for (int o = 0; o < 2; o++)
                for (int g = 0; g < BOM_T_DOM; g++) {
                    HIPCHK(hipEventElapsedTime(&ms, w.ev[o * (BOM_T_DOM + 1) + g], w.ev[o * (BOM_T_DOM + 1) + g + 1]));
                    w.ms[g] += ms;
                }
        HIPCHK(hipEventElapsedTime(&ms, w.ev[e0], w.ev[e0 + 1]));
        w.ms[BOM_T_DOM] = ms;
    }
    return 0;
}

extern "C" int tum_bom_fronts(tum_bo *b, const double *F_b, int S, int n_b, const double *ref, double *fronts_out, int *count_out)
{
    if (!b || !F_b || !ref || !fronts_out || !count_out) return fail("null argument");
    if (S < 1 || S > BO_MAXS) return fail("tum_bom_fronts: S outside 1..4096");
    if (n_b < 1 || n_b > BO_MAXB) return fail("tum_bom_fronts: n_b outside 1..512");
    const size_t len = (size_t)S * n_b * 2;
    if (!bo_finite(F_b, len) || !bo_finite(ref, 2)) return fail("tum_bom_fronts: F_b or ref holds a NaN or an infinity");
    DevGuard guard(b->device); GUARD_OK(guard);
    BomWork &w = b->work;
    hipStream_t st = b->stream;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(w.Fb.reserve(len)); HIPCHK(w.fronts.reserve(len)); HIPCHK(w.count.reserve(S));
    HIPCHK(hipMemcpyAsync(w.Fb.get(), F_b, sizeof(double) * len, hipMemcpyHostToDevice, st));
    BomFrontArgs a{};
    a.nb = n_b; a.ldf = n_b; a.F = w.Fb.get(); a.ref[0] = ref[0]; a.ref[1] = ref[1]; a.fronts = w.fronts.get(); a.count = w.count.get();
    LAUNCH(bom_front_kernel<>, dim3(S), dim3(256), 0, st, a);
    HIPCHK(hipMemcpyAsync(fronts_out, w.fronts.get(), sizeof(double) * len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(count_out, w.count.get(), sizeof(int) * S, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" void tum_bom_build_desc_init(tum_bom_build_desc *desc)
{
    if (!desc) return;
    *desc = tum_bom_build_desc{};
    desc->struct_size = (int)sizeof(tum_bom_build_desc);
}

// chain B of one objective on the stream: the dense H, L_b, R, mu_b of the baseline stay in the work buffers; H and R go to the
// model in the operand layouts of bo_kernels.hpp (Z too, from the dense copy the draws use), the draws to Fbm
static int bom_baseline(tum_bo *b, const tum_bom_build_desc *p, int o)
{
    BomWork &w = b->work;
    // np: the leading dimension of everything n_b x n_b, for the capacity appends may fill; nb: the blocks the n_b points take now
    const int nt = p->n_t, n = p->n_b, S = p->S, ntp = gp_pad(nt), np = w.ldb, nb = gp_pad(n) / GP_NB, Sp = bo_pad16(S);
    hipStream_t st = b->stream;
    int ti = o * (BOMB_T_FRONT + 1);
    auto mark = [&]() { if (w.profile_build) (void)hipEventRecord(w.evb[ti], st); ti++; };
    BOCHK(bom_upload(w.W, p->V[o], nt, nt, ntp, ntp, st));
    BOCHK(bom_upload(w.a, p->a[o], 1, nt, 1, ntp, st));
    HIPCHK(w.Z.reserve((size_t)Sp * np));
    HIPCHK(hipMemsetAsync(w.Z.get(), 0, sizeof(double) * Sp * np, st));
    HIPCHK(hipMemcpy2DAsync(w.Z.get(), sizeof(double) * np, p->Zfull[o], sizeof(double) * p->ncol, sizeof(double) * n, S, hipMemcpyHostToDevice, st));
    mark();
    BomKernArgs k{};
    k.d = p->d; k.s = p->s[o];
    for (int j = 0; j < p->d; j++) k.ils[j] = p->ils[o][j];
    k.nr = n; k.nc = nt; k.ld = ntp; k.Xr = b->X[1].get(); k.Xc = b->X[0].get(); k.K = w.K.get();
    LAUNCH(bom_kern_kernel<>, dim3(ntp / GP_NB, nb), dim3(256), 0, st, k);
    k.nc = n; k.ld = np; k.Xc = b->X[1].get(); k.K = w.Kbb.get();
    LAUNCH(bom_kern_kernel<>, dim3(nb, nb), dim3(256), 0, st, k);
    mark();
    BomMatArgs m{};
    m.n = n; m.np = np; m.ld = ntp; m.Kx = w.K.get(); m.K = w.Kbb.get(); m.V = w.W.get(); m.H = w.Hd[o].get(); m.A = w.Ld[o].get();
    m.jitter = p->jitter[o];
    LAUNCH(bom_h_kernel<>, dim3(ntp / GP_NB, nb), dim3(256), 0, st, m);
    mark();
    LAUNCH(bom_sig_kernel<>, dim3(nb, nb), dim3(256), 0, st, m);
    mark();
    GpFacArgs f{};
    f.n = n; f.np = np; f.A = w.Ld[o].get(); f.V = w.Rd[o].get(); f.M = w.Mt.get(); f.minpiv = w.minpiv.get() + (size_t)o * nb; f.bad = w.bad.get() + (size_t)o * nb;
    BOCHK(gp_cholesky(f, nb, st));
    mark();
    if (nb > 1) LAUNCH(gp_lhat_kernel<>, dim3(nb, nb, 4), dim3(64), 0, st, f);
    for (int sdiag = 1; sdiag < nb; sdiag++) {
        f.s = sdiag;
        LAUNCH(gp_trinv_kernel<>, dim3(nb - sdiag, 4, 4), dim3(64), 0, st, f);
    }
    mark();
    BomDrawArgs a{};
    a.n = n; a.np = np; a.S = S; a.o = o; a.ldk = ntp; a.ldf = w.cap; a.Kx = w.K.get(); a.a = w.a.get(); a.L = w.Ld[o].get(); a.Z = w.Z.get(); a.c = p->c[o];
    a.m = w.mub[o].get(); a.F = w.Fbm.get();
    LAUNCH(bom_mean_kernel<>, dim3(nb * GP_NB / 4), dim3(256), 0, st, a);
    mark();
    LAUNCH(bom_draw_kernel<>, dim3(nb, Sp / 16), dim3(64), 0, st, a);
    mark();
    BomPackArgs pk{};
    pk.rows = n; pk.cols = nt; pk.ld = ntp; pk.tri = 0; pk.M = w.Hd[o].get(); pk.out = b->H[o].get();
    LAUNCH(bom_pack_kernel<>, dim3(b->np[0] / 4, b->np[4] / 16), dim3(64), 0, st, pk);
    pk.cols = n; pk.ld = np; pk.tri = 1; pk.M = w.Rd[o].get(); pk.out = b->R[o].get();
    LAUNCH(bom_pack_kernel<>, dim3(b->np[4] / 4, b->np[4] / 16), dim3(64), 0, st, pk);
    pk.rows = S; pk.tri = 0; pk.M = w.Z.get(); pk.out = b->Z[o].get();          // (the dense Z of the draws: one upload serves both)
    LAUNCH(bom_pack_kernel<>, dim3(b->np[4] / 4, b->nts), dim3(64), 0, st, pk);
    mark();
    return 0;
}

extern "C" int tum_bom_build(tum_bo *b, const tum_bom_build_desc *p, int *ok_out)
{
    if (!b || !p || !ok_out) return fail("null argument");
    if (p->struct_size != (int)sizeof(tum_bom_build_desc)) return fail("tum_bom_build: struct_size is not this library's sizeof(tum_bom_build_desc)");
    if (p->d < 1 || p->d > BO_MAXD) return fail("tum_bom_build: d outside 1..16");
    if (p->n_t < 1 || p->n_t > BO_MAXN) return fail("tum_bom_build: n_t outside 1..4096");
    if (p->n_c < 1 || p->n_c > BO_MAXN) return fail("tum_bom_build: n_c outside 1..4096");
    if (p->n_b < 1 || p->n_b > BO_MAXB) return fail("tum_bom_build: n_b outside 1..512");
    if (p->S < 1 || p->S > BO_MAXS) return fail("tum_bom_build: S outside 1..4096");
    if (p->K < 1 || p->K > BO_MAXK) return fail("tum_bom_build: K outside 1..64");
    if (p->ncol < p->n_b + 1) return fail("tum_bom_build: the base samples need n_b + 1 columns");
    if (!p->Xt || !p->Xb || !p->Xc || !p->gh_x || !p->gh_w || !p->Zfull[0] || !p->Zfull[1]) return fail("tum_bom_build: null array");
    for (int g = 0; g < BO_GP; g++)
        if (!p->ils[g] || !p->a[g] || !p->V[g]) return fail("tum_bom_build: null array");
    const size_t d = p->d, nt = p->n_t, nc = p->n_c, n = p->n_b, S = p->S;
    bool fin = bo_finite(p->Xt, nt * d) && bo_finite(p->Xb, n * d) && bo_finite(p->Xc, nc * d) && bo_finite(p->s, 4) && bo_finite(p->c, 4) &&
               bo_finite(p->ref, 2) && bo_finite(p->jitter, 2) && std::isfinite(p->eps) && bo_finite(p->gh_x, p->K) && bo_finite(p->gh_w, p->K) &&
               bo_finite(p->Zfull[0], S * p->ncol) && bo_finite(p->Zfull[1], S * p->ncol);
    for (int g = 0; fin && g < BO_GP; g++) {
        const size_t m = g < 2 ? nt : nc;
        fin = bo_finite(p->ils[g], d) && bo_finite(p->a[g], m) && bo_finite(p->V[g], m * m);
    }
    if (!fin) return fail("tum_bom_build: an input holds a NaN or an infinity");
    if (!bom_lower(p->V[0], nt) || !bom_lower(p->V[1], nt)) return fail("tum_bom_build: V of an objective is not zero above its diagonal");
    DevGuard guard(b->device); GUARD_OK(guard);
    BomWork &w = b->work;
    hipStream_t st = b->stream;
    HIPCHK(hipStreamSynchronize(st));
    b->have_model = false; w.built = false;
    if (w.profile_build)
        for (int i = 0; i < BOMB_EVENTS; i++)
            if (!w.evb[i]) HIPCHK(hipEventCreate(&w.evb[i]));
    tum_bo_model_desc gp{};          // the four GPs as tum_bo_model installs them
    gp.d = p->d; gp.n_t = p->n_t; gp.n_b = p->n_b; gp.n_c = p->n_c; gp.Xt = p->Xt; gp.Xb = p->Xb; gp.Xc = p->Xc;
    for (int g = 0; g < BO_GP; g++) { gp.ils[g] = p->ils[g]; gp.a[g] = p->a[g]; gp.V[g] = p->V[g]; gp.s[g] = p->s[g]; gp.c[g] = p->c[g]; }
    BOCHK(bo_model_gp(b, &gp));
    // every resident array is sized for the baseline points appends may add: one per free column of Zfull behind zeta's
    const size_t cap = std::min<size_t>(BO_MAXB, (size_t)p->ncol - 1);
    w.cap = (int)cap; w.ldb = gp_pad((int)cap); w.ncol = p->ncol;
    bo_model_sizes(b, p->d, p->n_t, p->n_c, (int)cap, p->S, (int)cap, p->K, p->eps);
    BOCHK(bo_model_chunk(b, p->gh_x, p->gh_w));
    bo_model_sizes(b, p->d, p->n_t, p->n_c, p->n_b, p->S, (int)cap, p->K, p->eps);
    BOCHK(bo_upload(b->X[1], p->Xb, n * d, cap * d));
    const size_t ntp = gp_pad(p->n_t), np = w.ldb, nb = gp_pad(p->n_b) / GP_NB, ntb = bo_pad16((int)cap) / 16;
    HIPCHK(w.K.reserve(np * ntp)); HIPCHK(w.Kbb.reserve(np * np)); HIPCHK(w.Mt.reserve(np * np));
    HIPCHK(w.minpiv.reserve(2 * nb)); HIPCHK(w.bad.reserve(2 * nb)); HIPCHK(w.Fbm.reserve(S * cap * 2)); HIPCHK(w.okapp.reserve(2));
    for (int o = 0; o < 2; o++) {
        b->jitter[o] = p->jitter[o]; b->ref[o] = p->ref[o];
        HIPCHK(w.Hd[o].reserve(np * ntp)); HIPCHK(w.Ld[o].reserve(np * np)); HIPCHK(w.Rd[o].reserve(np * np)); HIPCHK(w.mub[o].reserve(np));
        HIPCHK(b->H[o].alloc(ntb * (b->np[0] / 4) * 64, false)); HIPCHK(b->R[o].alloc(bo_tri_off((int)ntb) * 64, false));
        // the base samples: Z (the first n_b columns) goes up once, dense, and the chain packs it; zeta is column n_b
        HIPCHK(b->Z[o].alloc((size_t)b->nts * (ntb * 4) * 64, false));
        BOCHK(bo_upload(w.Zf[o], p->Zfull[o], S * p->ncol));
        std::vector<double> zeta(S);
        for (size_t s = 0; s < S; s++) zeta[s] = p->Zfull[o][s * p->ncol + n];
        BOCHK(bo_upload(b->zeta[o], zeta.data(), S, (size_t)16 * b->nts));
    }
    HIPCHK(b->fronts.alloc(S * cap * 2, false)); HIPCHK(b->count.alloc(S, false));
    for (int o = 0; o < 2; o++) BOCHK(bom_baseline(b, p, o));
    const int e0 = 2 * (BOMB_T_FRONT + 1);
    if (w.profile_build) (void)hipEventRecord(w.evb[e0], st);
    {
        BomFrontArgs a{};
        a.nb = p->n_b; a.ldf = w.cap; a.F = w.Fbm.get(); a.ref[0] = p->ref[0]; a.ref[1] = p->ref[1]; a.fronts = b->fronts.get(); a.count = b->count.get();
        LAUNCH(bom_front_kernel<>, dim3(p->S), dim3(256), 0, st, a);
    }
    if (w.profile_build) (void)hipEventRecord(w.evb[e0 + 1], st);
    std::vector<int> bad(2 * nb);
    HIPCHK(hipMemcpyAsync(bad.data(), w.bad.get(), sizeof(int) * 2 * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipDeviceSynchronize());
    if (w.profile_build) {
        for (int g = 0; g < BOMB_TIMERS; g++) w.msb[g] = 0.0;
        float ms = 0;
        for (int o = 0; o < 2; o++)
            for (int g = 0; g < BOMB_T_FRONT; g++) {
                HIPCHK(hipEventElapsedTime(&ms, w.evb[o * (BOMB_T_FRONT + 1) + g], w.evb[o * (BOMB_T_FRONT + 1) + g + 1]));
                w.msb[g] += ms;
            }
        HIPCHK(hipEventElapsedTime(&ms, w.evb[e0], w.evb[e0 + 1]));
        w.msb[BOMB_T_FRONT] = ms;
    }
    int ok = 1;
    for (int v : bad) ok &= v == 0;
    *ok_out = ok;
    b->have_model = w.built = ok != 0;          // (a baseline that could not be factored leaves no model behind)
    return 0;
}

// the n x n lower-triangular device matrix (leading dimension ld) to the host, zero above the diagonal
static int bom_read_tri(const double *src, size_t n, size_t ld, double *out, hipStream_t st)
{
    HIPCHK(hipMemcpy2DAsync(out, sizeof(double) * n, src, sizeof(double) * ld, sizeof(double) * n, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++)          // (the tiles right of the diagonal tile are never written on the device)
        for (size_t k = i + 1; k < n; k++) out[i * n + k] = 0.0;
    return 0;
}

extern "C" int tum_bom_model_read(tum_bo *b, double *const *H_out, double *const *R_out, double *const *L_out, double *const *mu_out,
                                  double *F_b_out, double *fronts_out, int *count_out, int *n_b_out)
{
    if (!b) return fail("null argument");
    if (!b->have_model || !b->work.built) return fail("tum_bom_model_read: no model built on the device (tum_bom_build first)");
    DevGuard guard(b->device); GUARD_OK(guard);
    BomWork &w = b->work;
    hipStream_t st = b->stream;
    const size_t n = b->n[4], nt = b->n[0], S = b->S, np = w.ldb, ntp = gp_pad((int)nt), row = sizeof(double) * 2 * n, pitch = sizeof(double) * 2 * w.cap;
    for (int o = 0; o < 2; o++) {
        if (H_out && H_out[o])
            HIPCHK(hipMemcpy2DAsync(H_out[o], sizeof(double) * nt, w.Hd[o].get(), sizeof(double) * ntp, sizeof(double) * nt, n, hipMemcpyDeviceToHost, st));
        if (R_out && R_out[o]) BOCHK(bom_read_tri(w.Rd[o].get(), n, np, R_out[o], st));
        if (L_out && L_out[o]) BOCHK(bom_read_tri(w.Ld[o].get(), n, np, L_out[o], st));
        if (mu_out && mu_out[o]) HIPCHK(hipMemcpyAsync(mu_out[o], w.mub[o].get(), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    if (F_b_out) HIPCHK(hipMemcpy2DAsync(F_b_out, row, w.Fbm.get(), pitch, row, S, hipMemcpyDeviceToHost, st));
    if (fronts_out) HIPCHK(hipMemcpy2DAsync(fronts_out, row, b->fronts.get(), pitch, row, S, hipMemcpyDeviceToHost, st));
    if (count_out) HIPCHK(hipMemcpyAsync(count_out, b->count.get(), sizeof(int) * S, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_b_out) *n_b_out = (int)n;
    return 0;
}

// Chain A: the point x joins the baseline of the model tum_bom_build left, without refactoring: the evaluation chain gives q, l and d2
// of x; they are the new rows of H, L_b and R, the new draw is mu + Z l + sqrt(d2) zeta, the next column of Zfull becomes zeta, the
// fronts are rebuilt and H, R, Z are packed again. Nothing is uploaded but x.
extern "C" int tum_bom_append(tum_bo *b, const double *x, int *ok_out)
{
    if (!b || !x || !ok_out) return fail("null argument");
    if (!b->have_model || !b->work.built) return fail("tum_bom_append: no model built on the device (tum_bom_build first)");
    BomWork &w = b->work;
    const int n = b->n[4], nt = b->n[0], S = b->S;
    if (n >= BO_MAXB) return fail("tum_bom_append: n_b is 512 already");
    if (n + 2 > w.ncol) return fail("tum_bom_append: the base samples have no column left");
    if (!bo_finite(x, b->d)) return fail("tum_bom_append: x holds a NaN or an infinity");
    DevGuard guard(b->device); GUARD_OK(guard);
    hipStream_t st = b->stream;
    HIPCHK(hipMemcpyAsync(b->x.get(), x, sizeof(double) * b->d, hipMemcpyHostToDevice, st));
    const bool prof = b->profile;
    b->profile = false;
    const int rc = bo_chain(b, 1);
    b->profile = prof;
    BOCHK(rc);
    BomAppendArgs a{};
    a.n = n; a.nt = nt; a.ntp = gp_pad(nt); a.ldb = w.ldb; a.ntb = b->np[4] / 16; a.S = S; a.ncol = w.ncol; a.ldf = w.cap; a.d = b->d;
    a.mom = b->mom.get(); a.x = b->x.get(); a.cp = BO_CHUNK; a.F = w.Fbm.get(); a.Xb = b->X[1].get(); a.ok = w.okapp.get();
    for (int o = 0; o < 2; o++) {
        a.q[o] = b->q[o].get(); a.l[o] = b->l[o].get(); a.llpart[o] = b->llpart[o].get(); a.s[o] = b->s[o]; a.jitter[o] = b->jitter[o];
        a.H[o] = w.Hd[o].get(); a.L[o] = w.Ld[o].get(); a.R[o] = w.Rd[o].get(); a.mu[o] = w.mub[o].get(); a.Zf[o] = w.Zf[o].get();
    }
    LAUNCH(bom_append_kernel<>, dim3(2), dim3(256), 0, st, a);
    LAUNCH(bom_appdraw_kernel<>, dim3((S + 255) / 256, 2), dim3(256), 0, st, a);
    bo_model_sizes(b, b->d, nt, b->n[2], n + 1, S, w.cap, b->K, b->eps);
    for (int o = 0; o < 2; o++) {
        BomPackArgs pk{};
        pk.rows = n + 1; pk.cols = nt; pk.ld = a.ntp; pk.tri = 0; pk.M = w.Hd[o].get(); pk.out = b->H[o].get();
        LAUNCH(bom_pack_kernel<>, dim3(b->np[0] / 4, b->np[4] / 16), dim3(64), 0, st, pk);
        pk.cols = n + 1; pk.ld = w.ldb; pk.tri = 1; pk.M = w.Rd[o].get(); pk.out = b->R[o].get();
        LAUNCH(bom_pack_kernel<>, dim3(b->np[4] / 4, b->np[4] / 16), dim3(64), 0, st, pk);
        pk.rows = S; pk.ld = w.ncol; pk.tri = 0; pk.M = w.Zf[o].get(); pk.out = b->Z[o].get();
        LAUNCH(bom_pack_kernel<>, dim3(b->np[4] / 4, b->nts), dim3(64), 0, st, pk);
        HIPCHK(hipMemcpy2DAsync(b->zeta[o].get(), sizeof(double), w.Zf[o].get() + n + 1, sizeof(double) * w.ncol, sizeof(double), S, hipMemcpyDeviceToDevice, st));
    }
    {
        BomFrontArgs f{};
        f.nb = n + 1; f.ldf = w.cap; f.F = w.Fbm.get(); f.ref[0] = b->ref[0]; f.ref[1] = b->ref[1]; f.fronts = b->fronts.get(); f.count = b->count.get();
        LAUNCH(bom_front_kernel<>, dim3(S), dim3(256), 0, st, f);
    }
    int ok[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(ok, w.okapp.get(), sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *ok_out = ok[0] && ok[1];
    return 0;
}

extern "C" int tum_bom_build_profile(tum_bo *b, int on, double *ms_out)
{
    if (!b) return fail("null argument");
    b->work.profile_build = on != 0;
    if (ms_out)
        for (int g = 0; g < BOMB_TIMERS; g++) ms_out[g] = b->work.msb[g];
    return 0;
}

extern "C" int tum_bom_prune_profile(tum_bo *b, int on, double *ms_out)
{
    if (!b) return fail("null argument");
    b->work.profile = on != 0;
    if (ms_out)
        for (int g = 0; g < BOM_TIMERS; g++) ms_out[g] = b->work.ms[g];
    return 0;
}
