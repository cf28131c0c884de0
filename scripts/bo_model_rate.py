"""
bo_model_rate.py -- what building the acquisition model costs on the host and on the device at the end of the reference's campaign
(profiles/bo_model_rate.txt).

Workload: all 2050 trials of tests/golden/bo_trials_F.npz (194 feasible), segment group 0, S = 1024, q = 5, K = 64, the literal
hyperparameters of tests/bo_reference.hypers (nothing here depends on a fit). Six repetitions, interleaved:
  (p) prune_baseline          backend="host" against backend="device" (tum_bom_prune), the two factors (V, a) formed once outside
  (b) baseline of pack_model  pack_model + DeviceAcquisition.set_model with baseline="host" (numpy posterior, draws, fronts, upload)
                              against baseline="device" (tum_bom_build), the four factors formed once outside; model_arrays() apart
  (s) select                  from the host-built model with host appends (append_pick, upload with keep_gp) against the device-built
                              model with device appends (tum_bom_append: nothing uploaded but the pick)
then chain P and chain B kernel group by kernel group (tum_bom_prune_profile, tum_bom_build_profile), and for both (s) variants one
profiled select with the share of its time that is not kernel time (the launches of tum_bo_evaluate and, for the device-built model,
of tum_bom_build, timed by events; the few launches of tum_bom_append have no timers and count as outside).
With --parent LIB (a build of the parent commit): tum_bo_evaluate, select, tum_gp_mll and tum_gp_factor on their defaults in fresh
processes, alternating between the two libraries; times as medians and ranges, results as digests (sha256 of the bytes).

    python scripts/bo_model_rate.py [--reps 6] [--parent exp_libs/libtumnmpc_parent.so] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stat(x):
    x = np.asarray(x, dtype=float)
    return f"median {np.median(x):10.3f} ms  range {x.min():10.3f} .. {x.max():10.3f}  (n = {len(x)})"


def overlap(a, b):
    return "ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "ranges DO NOT overlap"


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()[:16]


def ms(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def workload():
    from bo_reference import hypers
    from tum_control_amd import bo
    z = np.load(os.path.join(ROOT, "tests", "golden", "bo_trials_F.npz"))
    Xn, feas, obj = z["params_nor"], z["feasible"], z["objectives"]
    Xt = np.ascontiguousarray(Xn[feas])
    Ys = bo.standardize(obj[feas][:, 0, :])[0]
    o_h, c_h = hypers(7)
    return bo, Xn, feas, Xt, Ys, o_h, c_h


class CachedFactor:
    """gp_factor's signature; every (V, a) is formed once: the lines time what is built FROM the factors."""

    def __init__(self, bo):
        self.bo, self.memo = bo, {}

    def __call__(self, X, y, hyp):
        key = digest(X, y, hyp.ls, [hyp.c, hyp.s], hyp.noise)
        if key not in self.memo:
            self.memo[key] = self.bo.gp_factor(X, y, hyp)
        return self.memo[key]


def child():
    """The defaults of the parent commit's entry points on the library TUM_NMPC_LIB names: one JSON line."""
    bo, Xn, feas, Xt, Ys, o_h, c_h = workload()
    S, q = 1024, 5
    keep = bo.prune_baseline(Xt, Ys, o_h, S=S, seed=[0, 11])[:bo.NB_MAX - q - 1]
    Z = bo.sobol_normal(S, 2 * (len(keep) + q + 1), [0, 13]).reshape(S, 2, -1).transpose(0, 2, 1)
    model = bo.pack_model(Xt, Ys, o_h, Xn, feas, c_h, Xt[keep], Z, np.array([-0.5, -0.75]), eps=0.8, jitter=1e-8, K=64)
    acq, gp = bo.DeviceAcquisition(), bo.DeviceGP()
    kw = dict(q=q, n_raw=512, n_restarts=20, max_iter=400, seed=5)
    bo.select(model, acq=acq, **kw)
    t_sel, (picks, vals, _) = ms(lambda: bo.select(model, acq=acq, **kw))
    X = bo.sobol_points(512, 7, 9)
    acq.set_model(model)
    acq.evaluate(X)
    t_ev = float(np.median([ms(lambda: acq.evaluate(X))[0] for _ in range(20)]))
    ev = acq.evaluate(X, detail=True)
    th = np.concatenate([np.log(o_h[0].ls), [np.log(o_h[0].s), o_h[0].c, np.log(1e-2)]])
    gp.set_data(Xt, Ys[:, 0])
    gp.mll_grad(th, True, 1e-6)
    t_mll = float(np.median([ms(lambda: gp.mll_grad(th, True, 1e-6))[0] for _ in range(10)]))
    mll, grad, _ = gp.mll_grad(th, True, 1e-6)
    gp.gp_factor(Xt, Ys[:, 0], o_h[0])
    t_fac = float(np.median([ms(lambda: gp.gp_factor(Xt, Ys[:, 0], o_h[0]))[0] for _ in range(10)]))
    V, a = gp.gp_factor(Xt, Ys[:, 0], o_h[0])
    acq.close(); gp.close()
    print("CHILD " + json.dumps(dict(select=t_sel, evaluate=t_ev, mll=t_mll, factor=t_fac, d_select=digest(picks, vals), d_evaluate=digest(*ev),
                                     d_mll=digest([mll], grad), d_factor=digest(V, a))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    bo, Xn, feas, Xt, Ys, o_h, c_h = workload()
    S, q = 1024, 5
    say(f"# scripts/bo_model_rate.py --reps {a.reps}" + (f" --parent {a.parent}" if a.parent else ""))
    say(f"# {len(Xn)} trials, {len(Xt)} feasible, group 0; S = {S}, q = {q}, K = 64, literal hyperparameters (tests/bo_reference.hypers)")
    factor = CachedFactor(bo)
    acq = bo.DeviceAcquisition()
    seed = [0, 11]
    prune = lambda backend: bo.prune_baseline(Xt, Ys, o_h, S=S, seed=seed, factor=factor, backend=backend, acq=acq)          # noqa: E731
    keep = prune("host")[:bo.NB_MAX - q - 1]
    assert (prune("device")[:bo.NB_MAX - q - 1] == keep).all(), "the device prunes other trials than the host"
    Z = bo.sobol_normal(S, 2 * (len(keep) + q + 1), [0, 13]).reshape(S, 2, -1).transpose(0, 2, 1)
    t_sob = np.median([ms(lambda: bo.sobol_normal(S, 2 * len(Xt), seed))[0] for _ in range(3)])

    def pack(baseline):
        m = bo.pack_model(Xt, Ys, o_h, Xn, feas, c_h, Xt[keep], Z, np.array([-0.5, -0.75]), eps=0.8, jitter=1e-8, K=64, factor=factor, baseline=baseline)
        acq.set_model(m)
        return m
    m_host, m_dev = pack("host"), pack("device")
    m_done = bo.complete_model(m_dev, acq.model_arrays())
    kw = dict(q=q, n_raw=512, n_restarts=20, max_iter=400, seed=5)
    bo.select(m_host, acq=acq, **kw); bo.select(m_dev, acq=acq, **kw)
    tp_h, tp_d, tb_h, tb_d, tr, ts_h, ts_d = [], [], [], [], [], [], []
    for rep in range(a.reps):
        tp_h.append(ms(lambda: prune("host"))[0]); tp_d.append(ms(lambda: prune("device"))[0])
        tb_h.append(ms(lambda: pack("host"))[0]); tb_d.append(ms(lambda: pack("device"))[0])
        tr.append(ms(acq.model_arrays)[0])
        t, (p_h, v_h, _) = ms(lambda: bo.select(m_host, acq=acq, **kw)); ts_h.append(t)
        t, (p_d, v_d, _) = ms(lambda: bo.select(m_dev, acq=acq, **kw)); ts_d.append(t)
    say(f"# n_b {len(keep)} of {len(Xt)} trials after pruning (host and device keep the same trials); the Sobol base samples of one pruning, "
        f"formed on the host in both paths: {t_sob:.1f} ms of each (p) line")
    say(f"  (p) prune_baseline, host                       : {stat(tp_h)}")
    say(f"  (p) prune_baseline, device (tum_bom_prune)     : {stat(tp_d)}   {overlap(tp_d, tp_h)}, ratio of medians {np.median(tp_h) / np.median(tp_d):.1f}")
    say(f"  (b) pack_model + set_model, baseline on host   : {stat(tb_h)}")
    say(f"  (b) pack_model + set_model, baseline on device : {stat(tb_d)}   {overlap(tb_d, tb_h)}, ratio of medians {np.median(tb_h) / np.median(tb_d):.1f}")
    say(f"      model_arrays() (the download that completes the final model of select): {stat(tr)}")
    say(f"  (s) select, host-built model, host appends     : {stat(ts_h)}")
    say(f"  (s) select, device-built model, device appends : {stat(ts_d)}   {overlap(ts_d, ts_h)}, ratio of medians {np.median(ts_h) / np.median(ts_d):.2f} "
        "(the build is inside this line, the host model's pack_model is not inside the other)")
    say(f"      picks, device-built against host-built: largest coordinate difference {np.abs(p_d - p_h).max():.3e}; values "
        f"{np.array2string(v_d, precision=6)} against {np.array2string(v_h, precision=6)}")
    Xq = bo.sobol_points(64, 7, 9)
    a_h, a_d = bo.host_acquisition(m_host, Xq), bo.host_acquisition(m_done, Xq)
    say(f"      acquisition of 64 Sobol points, device-built against host-built model: largest difference {np.abs(a_d - a_h).max():.3e} of {np.abs(a_h).max():.3e}")
    V, av = zip(*(factor(Xt, Ys[:, o], o_h[o]) for o in range(2)))
    Zs = bo.sobol_normal(S, 2 * len(Xt), seed).reshape(S, 2, len(Xt))
    names = ("bom_kern_kernel (K)", "bom_h_kernel (K V^T)", "bom_sig_kernel (K - H H^T)", "potrf + trsm + syrk (Cholesky)", "bom_mean_kernel", "bom_draw_kernel (Z L^T)",
             "bom_dom_kernel")
    acq.prune_profile(True)
    per, wall = [], []
    for rep in range(a.reps + 1):
        wall.append(ms(lambda: acq.prune(Xt, V, av, o_h, Zs))[0])
        per.append(acq.prune_profile(True))
    per, wall = np.array(per[1:]), wall[1:]
    say(f"  one tum_bom_prune, n = {len(Xt)}, S = {S}, both objectives: wall {stat(wall)}")
    for i, nm in enumerate(names):
        say(f"      {nm:32s}: {stat(per[:, i])}")
    say(f"      the kernels together {np.median(per.sum(1)):.3f} ms of {np.median(wall):.3f} ms wall (the rest: checks, uploads of V, Z and a, downloads)")
    acq.prune_profile(False)
    bnames = ("bom_kern_kernel (K(Xb,Xt), K(Xb,Xb))", "bom_h_kernel (K V^T)", "bom_sig_kernel (K - H H^T)", "potrf + trsm + syrk (Cholesky)",
              "gp_lhat + gp_trinv (R = L_b^-1)", "bom_mean_kernel", "bom_draw_kernel (Z L_b^T)", "bom_pack_kernel (H, R, Z)", "bom_front_kernel")
    acq.build_profile(True)
    per, wall = [], []
    for rep in range(a.reps + 1):
        wall.append(ms(lambda: acq.set_model(m_dev))[0])
        per.append(acq.build_profile(True))
    per, wall = np.array(per[1:]), wall[1:]
    say(f"  one tum_bom_build, n_t = {len(Xt)}, n_b = {len(keep)}, n_c = {len(Xn)}, S = {S}, both objectives: wall {stat(wall)}")
    for i, nm in enumerate(bnames):
        say(f"      {nm:36s}: {stat(per[:, i])}")
    say(f"      the kernels together {np.median(per.sum(1)):.3f} ms of {np.median(wall):.3f} ms wall (the rest: checks, packing and upload of the four V, "
        "upload of Z and zeta, allocation of the chunk buffers)")
    # the share of select outside kernels, for both models: the kernels of every tum_bo_evaluate and of the device build, by events
    for label, model in (("host-built model with host appends", m_host), ("device-built model with device appends", m_dev)):
        acq.profile(True)
        kernel_ms = [0.0]
        orig = acq.evaluate

        def counted(Xe, detail=False):
            out = orig(Xe, detail=detail)
            kernel_ms[0] += float(acq.profile(True).sum())
            return out
        acq.evaluate = counted
        t_sel = ms(lambda: bo.select(model, acq=acq, **kw))[0]
        acq.evaluate = orig
        acq.profile(False)
        if model.device_baseline:
            kernel_ms[0] += float(acq.build_profile(True).sum())
        say(f"  one profiled select from the {label}: {t_sel:.1f} ms, of which kernels {kernel_ms[0]:.1f} ms; outside kernels (round trips, "
            f"uploads, appends, move / halve) {100.0 * (1.0 - kernel_ms[0] / t_sel):.1f} %")
    acq.build_profile(False)
    acq.close()
    if a.parent:
        libs = {"this build": os.path.join(ROOT, "tum-control_amd", "libtumnmpc.so"), "parent": os.path.abspath(a.parent)}
        res = {k: [] for k in libs}
        for rep in range(a.reps):
            for k, path in libs.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, TUM_NMPC_LIB=path),
                                     capture_output=True, text=True, timeout=300)
                hit = [ln for ln in out.stdout.splitlines() if ln.startswith("CHILD ")]
                if out.returncode != 0 or not hit:
                    say(f"  child on {k} failed (rc {out.returncode}): {out.stderr[-400:]}")
                    return finish(a, lines)
                res[k].append(json.loads(hit[0][6:]))
        say("  the parent commit's entry points on their defaults, fresh processes alternating between the two builds:")
        for key, label in (("evaluate", "tum_bo_evaluate, 512 candidates"), ("select", "select, q = 5"), ("mll", "tum_gp_mll, n = 194, with gradient"),
                           ("factor", "DeviceGP.gp_factor, n = 194")):
            t = {k: [r[key] for r in res[k]] for k in libs}
            d = {k: sorted({r["d_" + key] for r in res[k]}) for k in libs}
            same = d["this build"] == d["parent"] and len(d["parent"]) == 1
            say(f"      {label:36s} this build: {stat(t['this build'])}")
            say(f"      {'':36s} parent    : {stat(t['parent'])}   {overlap(t['this build'], t['parent'])}; results "
                f"{'equal to the bit' if same else 'DIFFER'} (digests {d['this build']} / {d['parent']})")
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
