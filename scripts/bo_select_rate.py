"""
bo_select_rate.py -- what one Bayesian-optimisation step costs at the end of the reference's campaign, part by part
(profiles/bo_select_rate.txt).

Workload: all 2050 trials of tests/golden/bo_trials_F.npz (194 feasible), segment group 0, bo_config.yaml's settings: 1024 Sobol
samples, 512 raw samples, 20 restarts, q = 5, max_iter 400. Per repetition, interleaved:
  (f) fit       ObjectiveModel + ConstraintModel (fit_gp, torch float64 on --fit-device)
  (g) fit       the same four fits with backend="device": likelihood and gradient from tum_gp_mll (csrc/gp_kernels.hpp)
  (s) select    bo.select on the device (tum_bo_evaluate behind the compass search)
  (h) select    the same search, bo.host_acquisition on this box's threads (numpy / BLAS); --host-reps of them
  (e) evaluate  closed_loop.evaluate_segments of the q picks, 8 segments of Monteblanco each
(s) and (h) run the same seeds on the same packed model: their picks are compared. Then one tum_bo_evaluate of 512 candidates with
the launches timed by events (tum_bo_profile), the FP64 rate of the matrix products against the 78.6 TFLOP/s peak, and the share of
(s) that is not kernel time: round trips, uploads of the appended model, the host's move / halve step and front rebuild.
Then the surrogate fit's chain (profiles/bo_fit_rate.txt): one tum_gp_mll at n = 2050 and at n = 194 kernel group by kernel group
(tum_gp_profile), the matrix-core kernels against the FP64 peak, the device's MLL and gradient at n = 2050 against the two FP64
statements on the host, and how prune + pack on the host splits with the host's factors and with factor= on the device. Digests
(sha256 of the bytes) of the default fit, the picks and one evaluation let two builds be compared to the bit; --no-gp runs the lines
a library without the tum_gp_ entry points has. botorch cannot be run here, so nothing is quoted against it.

    python scripts/bo_select_rate.py [--reps 6] [--host-reps 6] [--fit-device cuda] [--fit-max-iter 50] [--no-gp] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 78.6e12


def stat(x):
    x = np.asarray(x, dtype=float)
    return f"median {np.median(x):10.3f} ms  range {x.min():10.3f} .. {x.max():10.3f}  (n = {len(x)})"


def overlap(a, b):
    return "ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "ranges DO NOT overlap"


def product_flops(m, C):
    """FLOPs of the four matrix products of one evaluation of C candidates as the kernels run them (padded tiles, zero tiles of the
    triangular factors skipped): V k for the four GPs, H q, R sig, Z l."""
    p16 = lambda n: (n + 15) // 16 * 16          # noqa: E731
    ct = (C + 63) // 64 * 4
    blk = 2 * 16 * 16 * 4
    tri = lambda n: sum(4 * (t + 1) for t in range(p16(n) // 16))          # noqa: E731
    nt, nb, nc = len(m.Xt), m.n_b, len(m.Xc)
    v = (2 * tri(nt) + 2 * tri(nc)) * blk * ct
    h = 2 * (p16(nb) // 16) * (p16(nt) // 4) * blk * ct
    r = 2 * tri(nb) * blk * ct
    z = 2 * (p16(m.S) // 16) * (p16(nb) // 4) * blk * ((C + 15) // 16)
    return v, h, r, z


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()[:16]


def gp_flops(n):
    """FLOPs of the matrix-core kernels of one tum_gp_mll as they run them (64 x 64 tiles, n padded): panel + trailing update,
    M = L_ii^-1 L_im and the block diagonals of V, the lower tiles of V^T V from their block row on."""
    nb, t = (n + 63) // 64, 2 * 64 ** 3
    chol = sum((nb - k - 1) * t + (nb - k - 1) * (nb - k) // 2 * t for k in range(nb))
    trinv = nb * (nb - 1) // 2 * t + sum((nb - s) * s * t for s in range(1, nb))
    ainv = sum((i + 1) * (nb - i) * t for i in range(nb))
    return chol, trinv, ainv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--host-reps", type=int, default=6)
    ap.add_argument("--fit-device", default="cuda")
    ap.add_argument("--fit-max-iter", type=int, default=50)
    ap.add_argument("--max-steps", type=int, default=500)
    ap.add_argument("--no-gp", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import bo
    from tum_control_amd import closed_loop as clm
    from tum_control_amd.planner import load_track

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    z = np.load(os.path.join(ROOT, "tests", "golden", "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"], z["feasible"], z["objectives"]
    Xt, Y = Xn[feas], obj[feas][:, 0, :]
    cfg = dict(bo.DEFAULT_CONFIG)
    S, q = cfg["n_sobol_samples"], cfg["batch_size"]
    say(f"# scripts/bo_select_rate.py --reps {a.reps} --host-reps {a.host_reps} --fit-device {a.fit_device} --fit-max-iter {a.fit_max_iter}")
    say(f"# {len(Xn)} trials, {len(Xt)} feasible, group 0; S = {S}, {cfg['n_raw_samples']} raw samples, {cfg['n_restarts']} restarts, q = {q}, "
        f"max_iter {cfg['max_iter']}, K = {cfg['gh_nodes']} quadrature nodes")
    torch.zeros(1, device="cuda:0")

    def fit():
        om = bo.ObjectiveModel(Xt, Y, device=a.fit_device, max_iter=a.fit_max_iter)
        cm = bo.ConstraintModel(Xn, feas, device=a.fit_device, max_iter=a.fit_max_iter)
        return om, cm

    dgp = None if a.no_gp else bo.DeviceGP()

    def fit_dev():
        om = bo.ObjectiveModel(Xt, Y, max_iter=a.fit_max_iter, backend="device", gp=dgp)
        cm = bo.ConstraintModel(Xn, feas, max_iter=a.fit_max_iter, backend="device", gp=dgp)
        return om, cm

    def prune(om):
        return bo.prune_baseline(Xt, om.Ys, om.hyp, S=S, seed=[0, 11], jitter=cfg["jitter"])[:bo.NB_MAX - q - 1]

    def pack(om, cm, keep=None, **kw):
        keep = prune(om) if keep is None else keep
        Z = bo.sobol_normal(S, 2 * (len(keep) + q + 1), [0, 13]).reshape(S, 2, -1).transpose(0, 2, 1)
        return bo.pack_model(Xt, om.Ys, om.hyp, Xn, feas, cm.hyp, Xt[keep], Z, np.array(cfg["reference_point_0"]), eps=cfg["epsilon"],
                             jitter=cfg["jitter"], K=cfg["gh_nodes"], **kw)

    # segments of the objective: 8 on Monteblanco, two groups of four, about six seconds of race-line travel each
    track = load_track("monteblanco")
    n = len(track)
    starts = (np.arange(8) * (n // 8)).astype(np.int64)
    dt = np.hypot(*(np.roll(track[:, :2], -1, axis=0) - track[:, :2]).T) / np.roll(track[:, 3], -1)
    ends = []
    for s0 in starts:
        t, i = 0.0, int(s0)
        while t < 6.0:
            t += dt[i % n]; i += 1
        ends.append(i % n)
    groups = [[(int(starts[i]), int(ends[i])) for i in range(0, 4)], [(int(starts[i]), int(ends[i])) for i in range(4, 8)]]
    bounds = np.array([[1, 0, 1, 0, 20, 500, 500], [30, 5, 30, 6, 400, 2000, 2000]], dtype=float)

    om, cm = fit()          # warm-up of every path, and the model all repetitions of (s) / (h) search on
    t0 = time.perf_counter()
    model = pack(om, cm)
    t_pack = (time.perf_counter() - t0) * 1e3
    say(f"# packed model: n_t {len(model.Xt)}, n_c {len(model.Xc)}, n_b {model.n_b} after pruning, fronts up to {int(model.front_count.max())} points; "
        f"prune + pack on the host {t_pack:.0f} ms (once per step, not in the lines below)")
    acq = bo.DeviceAcquisition()
    kw = dict(q=q, n_raw=cfg["n_raw_samples"], n_restarts=cfg["n_restarts"], max_iter=cfg["max_iter"], seed=5)
    picks, vals, _ = bo.select(model, acq=acq, **kw)
    clm.evaluate_segments("monteblanco", bounds[0] + picks * (bounds[1] - bounds[0]), groups, 2.0, 1.02, a.max_steps)

    if dgp is not None:
        om_d, cm_d = fit_dev()
    tf, tg, ts, th, te, launches, host_picks, same_fit = [], [], [], [], [], [], None, []
    for rep in range(a.reps):
        t0 = time.perf_counter(); om_r, cm_r = fit(); torch.cuda.synchronize(); tf.append((time.perf_counter() - t0) * 1e3)
        same_fit.append(digest(*[[h.c, h.s, h.noise] + list(h.ls) for h in om_r.hyp + cm_r.hyp]) == digest(*[[h.c, h.s, h.noise] + list(h.ls) for h in om.hyp + cm.hyp]))
        if dgp is not None:
            t0 = time.perf_counter(); fit_dev(); tg.append((time.perf_counter() - t0) * 1e3)
        st = []
        t0 = time.perf_counter(); p_dev, v_dev, _ = bo.select(model, acq=acq, stats=st, **kw); ts.append((time.perf_counter() - t0) * 1e3)
        launches.append(sum(s["launches"] for s in st))
        if rep < a.host_reps:
            t0 = time.perf_counter(); host_picks, v_host, _ = bo.select(model, acq=bo.HostAcquisition(), **kw); th.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        clm.evaluate_segments("monteblanco", bounds[0] + p_dev * (bounds[1] - bounds[0]), groups, 2.0, 1.02, a.max_steps)
        torch.cuda.synchronize(); te.append((time.perf_counter() - t0) * 1e3)
        assert (p_dev == picks).all() and (v_dev == vals).all(), "select is not repeatable"
    say(f"  (f) fit, torch float64 on {a.fit_device}, max_iter {a.fit_max_iter}: {stat(tf)}")
    if tg:
        say(f"  (g) fit, backend=\"device\" (tum_gp_mll), max_iter {a.fit_max_iter}: {stat(tg)}   (g) against (f): {overlap(tg, tf)}, "
            f"ratio of medians (f) / (g) {np.median(tf) / np.median(tg):.2f}")
        for nm, hs, hd in (("objective 0", om.hyp[0], om_d.hyp[0]), ("objective 1", om.hyp[1], om_d.hyp[1]), ("class 0", cm.hyp[0], cm_d.hyp[0]),
                           ("class 1", cm.hyp[1], cm_d.hyp[1])):
            say(f"      {nm}: largest relative difference of the fitted hyperparameters, (g) against (f): "
                f"{max(abs(hd.c - hs.c) / max(abs(hs.c), 1e-300), abs(hd.s / hs.s - 1), abs(hd.noise / hs.noise - 1), float(np.abs(hd.ls / hs.ls - 1).max())):.2e}")
    say(f"  (s) select on the device                  : {stat(ts)}   {launches[0]} launches of tum_bo_evaluate")
    if th:
        say(f"  (h) select, host_acquisition, {os.cpu_count()} CPUs seen, {torch.get_num_threads()} threads: {stat(th)}   (s) against (h): {overlap(ts, th)}, "
            f"ratio of medians {np.median(th) / np.median(ts):.1f}")
        same = np.abs(host_picks - picks).max()
        say(f"      picks of (h) against (s): largest coordinate difference {same:.3e}; values {np.array2string(v_host, precision=6)} against "
            f"{np.array2string(vals, precision=6)}")
    say(f"  (e) evaluate_segments of the {q} picks x 8 segments: {stat(te)}")

    # one evaluation of 512 candidates, launch by launch
    X = bo.sobol_points(512, 7, 9)
    acq.set_model(model)
    acq.profile(True)
    names = ("bo_kern_kernel", "bo_tri_kernel (V k, 4 GPs)", "bo_moments_kernel", "bo_cross_kernel (H q)", "bo_tri_kernel (R sig)", "bo_hvi_kernel (Z l, HVI)",
             "bo_final_kernel")
    per, wall = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter(); acq.evaluate(X); wall.append((time.perf_counter() - t0) * 1e3)
        per.append(acq.profile(True))
    per, wall = np.array(per[1:]), wall[1:]
    v, h, r, zf = product_flops(model, 512)
    fl = {1: v, 3: h, 4: r, 5: zf}
    say(f"  one tum_bo_evaluate of 512 candidates: wall {stat(wall)}")
    for i, nm in enumerate(names):
        med = np.median(per[:, i])
        rate = f"   {fl[i] / 1e9:8.2f} GFLOP of products = {fl[i] / (med * 1e-3) / 1e12:6.2f} TFLOP/s = {fl[i] / (med * 1e-3) / PEAK:.3f} of the FP64 peak" if i in fl else ""
        say(f"      {nm:28s}: {stat(per[:, i])}{rate}")
    ksum = np.median(per.sum(1))
    say(f"      the seven launches together {ksum:.3f} ms of {np.median(wall):.3f} ms wall")
    acq.profile(False)
    # the share of select outside kernels: time the same launches' kernels through one profiled select
    acq.profile(True)
    kernel_ms = [0.0]
    orig = acq.evaluate

    def counted(Xe, detail=False):
        out = orig(Xe, detail=detail)
        kernel_ms[0] += float(acq.profile(True).sum())
        return out
    acq.evaluate = counted
    t0 = time.perf_counter(); bo.select(model, acq=acq, **kw); t_sel = (time.perf_counter() - t0) * 1e3
    acq.evaluate = orig
    acq.profile(False)
    say(f"  one profiled select: {t_sel:.1f} ms, of which kernels {kernel_ms[0]:.1f} ms; outside kernels (round trips, uploads of the appended "
        f"model, move / halve and front rebuild on the host) {100.0 * (1.0 - kernel_ms[0] / t_sel):.1f} %")
    h_cpu = bo.fit_gp(Xt, om.Ys[:, 0], max_iter=a.fit_max_iter)
    say(f"  the default fit on {a.fit_device} repeated to the bit in {sum(same_fit)} of {len(same_fit)} repetitions")
    say(f"  digests: default fit of objective 0 on the cpu {digest([h_cpu.c, h_cpu.s, h_cpu.noise], h_cpu.ls)}  default fit on {a.fit_device} {digest(*[[h.c, h.s, h.noise] + list(h.ls) for h in om.hyp + cm.hyp])}  picks and values {digest(picks, vals)}  "
        f"one evaluation of 512 candidates {digest(*acq.evaluate(X, detail=True))}")
    acq.close()
    if dgp is not None:
        gp_lines(a, say, bo, dgp, Xn, feas, Xt, om, cm, prune, pack)
        dgp.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def gp_lines(a, say, bo, dgp, Xn, feas, Xt, om, cm, prune, pack):
    import torch
    targets, fixed = bo.dirichlet_targets(feas)
    names = ("gp_kern_kernel", "potrf + trsm + syrk (Cholesky)", "gp_lhat + gp_trinv (V = L^-1)", "gp_ainv_kernel (V^T V)", "gp_w + gp_alpha + gp_asum",
             "gp_grad_kernel", "gp_reduce_kernel")
    theta = lambda h, fl: np.concatenate([np.log(h.ls), [np.log(h.s), h.c, np.log(h.noise - fl)]])          # noqa: E731
    for label, X, y, fn, h in (("class 0, n = %d" % len(Xn), Xn, targets[:, 0], fixed[:, 0], cm.hyp[0]), ("objective 0, n = %d" % len(Xt), Xt, om.Ys[:, 0], None, om.hyp[0])):
        th = theta(h, 1e-6)
        dgp.set_data(X, y, fn)
        dgp.profile(True)
        per, wall, wall_v = [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter(); dgp.mll_grad(th, True, 1e-6); wall.append((time.perf_counter() - t0) * 1e3)
            per.append(dgp.profile(True))
            t0 = time.perf_counter(); dgp.mll_grad(th, True, 1e-6, grad=False); wall_v.append((time.perf_counter() - t0) * 1e3)
        per, wall, wall_v = np.array(per[1:]), wall[1:], wall_v[1:]
        nb = (len(X) + 63) // 64
        launches = 1 + nb + 2 * (nb - 1) + (1 if nb > 1 else 0) + (nb - 1) + 1 + 3 + 1 + 1
        say(f"  one tum_gp_mll with the gradient, {label} at the fitted hyperparameters, {launches} launches: wall {stat(wall)}")
        say(f"      the value alone (no V^T V, no gradient tiles): wall {stat(wall_v)}")
        fl = dict(zip((1, 2, 3), gp_flops(len(X))))
        for i, nm in enumerate(names):
            med = np.median(per[:, i])
            rate = f"   {fl[i] / 1e9:8.2f} GFLOP on the matrix cores = {fl[i] / (med * 1e-3) / 1e12:6.2f} TFLOP/s = {fl[i] / (med * 1e-3) / PEAK:.3f} of the FP64 peak" \
                if i in fl and fl[i] else ""
            say(f"      {nm:32s}: {stat(per[:, i])}{rate}")
        say(f"      the kernels together {np.median(per.sum(1)):.3f} ms of {np.median(wall):.3f} ms wall")
        dgp.profile(False)
    # agreement at full size, recorded and not gated: no long-double reference is affordable at n = 2050
    n, d = Xn.shape
    th = np.concatenate([np.log(np.full(d, 0.5)), [np.log(max(float(np.var(targets[:, 0])), 1.0)), 1.0, np.log(1e-2)]])
    dgp.set_data(Xn, targets[:, 0], fixed[:, 0])
    m_d, g_d, ok = dgp.mll_grad(th, True, 1e-6)
    m_h, g_h, _ = bo.gp_mll_grad_host(Xn, targets[:, 0], th, fixed[:, 0], True, 1e-6)
    tt = torch.tensor(th, requires_grad=True)
    m_t, _ = bo._mll_torch(tt, torch.as_tensor(Xn), torch.as_tensor(targets[:, 0]), torch.as_tensor(fixed[:, 0]), True, 1e-6)
    m_t.backward()
    g_t, m_t = tt.grad.numpy(), float(m_t.detach())
    L = np.linalg.cholesky(bo.rbf(Xn, Xn, np.exp(-th[:d]), np.exp(th[d])) + np.diag(fixed[:, 0] + 1e-6 + np.exp(th[d + 2])))
    scale_m = abs(m_h + np.log(np.diag(L)).sum() + 0.5 * n * np.log(2 * np.pi)) + abs(np.log(np.diag(L)).sum()) + 0.5 * n * np.log(2 * np.pi)
    scale_g, u = np.abs(g_h).max(), 2.0 ** -53
    say(f"  agreement at n = {n}, class 0 at fit_gp's initial hyperparameters (ok {int(ok)}), in u x scale (scale_mll {scale_m:.1f}, scale_grad {scale_g:.1f}; "
        "scales from the host statement, no long-double reference at this size; recorded, not gated):")
    say(f"      MLL      device - torch autograd (CPU) {abs(m_d - m_t) / (u * scale_m):9.1f}   device - gp_mll_grad_host {abs(m_d - m_h) / (u * scale_m):9.1f}   "
        f"host - torch {abs(m_h - m_t) / (u * scale_m):9.1f}")
    say(f"      gradient device - torch autograd (CPU) {np.abs(g_d - g_t).max() / (u * scale_g):9.1f}   device - gp_mll_grad_host {np.abs(g_d - g_h).max() / (u * scale_g):9.1f}   "
        f"host - torch {np.abs(g_h - g_t).max() / (u * scale_g):9.1f}")
    # prune + pack on the host, part by part
    hyps4 = lambda: [(Xt, om.Ys[:, 0], om.hyp[0]), (Xt, om.Ys[:, 1], om.hyp[1])] + \
        [(Xn, targets[:, k], bo.GPHyper(cm.hyp[k].c, cm.hyp[k].s, cm.hyp[k].ls, fixed[:, k] + cm.hyp[k].noise)) for k in range(2)]          # noqa: E731
    t_pr, t_fh, t_fd, t_ph, t_pd, t_fr = [], [], [], [], [], []
    for rep in range(a.reps):
        t0 = time.perf_counter(); keep = prune(om); t_pr.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); [bo.gp_factor(*h) for h in hyps4()]; t_fh.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); [dgp.gp_factor(*h) for h in hyps4()]; t_fd.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); m_h = pack(om, cm, keep=keep); t_ph.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); m_d = pack(om, cm, keep=keep, factor=dgp.gp_factor); t_pd.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); bo.build_fronts(m_h.F_b, m_h.ref); t_fr.append((time.perf_counter() - t0) * 1e3)
    say("  prune + pack on the host, part by part:")
    say(f"      prune_baseline                          : {stat(t_pr)}")
    say(f"      the four factors (V, a), bo.gp_factor   : {stat(t_fh)}")
    say(f"      the four factors (V, a), tum_gp_factor  : {stat(t_fd)}   {overlap(t_fd, t_fh)}, ratio of medians {np.median(t_fh) / np.median(t_fd):.2f}")
    say(f"      pack_model, host factors                : {stat(t_ph)}   of it fronts {np.median(t_fr):.1f} ms, baseline posterior and the rest "
        f"{np.median(t_ph) - np.median(t_fh) - np.median(t_fr):.1f} ms")
    say(f"      pack_model, factor= on the device       : {stat(t_pd)}")
    Xq = bo.sobol_points(64, d, 9)
    a_h, a_d = bo.host_acquisition(m_h, Xq), bo.host_acquisition(m_d, Xq)
    say(f"      acquisition of 64 Sobol points, device factors against host factors: largest difference {np.abs(a_d - a_h).max():.3e} of {np.abs(a_h).max():.3e}")


if __name__ == "__main__":
    main()
