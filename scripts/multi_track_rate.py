"""
multi_track_rate.py -- what a track set costs (profiles/multi_track_rate.txt). Medians and ranges of `--reps` interleaved repetitions
behind one warm-up repetition; every wall time ends in a device synchronise.

With --parent-lib FILE (libtumnmpc.so of a build of the parent commit) the UNCHANGED single-track paths, same job on both builds,
interleaved, results compared to the bit:
  (1) a control step of a Monteblanco loop at 16 and at 4096 vehicles (run(K), chunks replayed)
  (2) an environment step (n_mpc_steps 20, random actions from the 26-row table) at both sizes
  (3) evaluate_segments on 26 weight sets x 8 Monteblanco segments (the workload of scripts/segment_scores.py)
On this build alone, a mixed Monteblanco / Modena loop (instance i on track i % 2) against the single-track loop of the same batch:
  (4) a control step at 16 and at 4096 vehicles, and the planner launch alone (tum_sim_plan, K launches and one wait)
And the two workloads of the reference that need a track set:
  (5) one evaluation of 26 weight sets on the 20 training segments of closed_loop.train_segments() (520 loops, both tracks)
  (6) one collect(512) and one update (8192 rows, batch_size 4096, 5 epochs) on 8 + 8 environments

    python scripts/multi_track_rate.py [--reps 6] [--parent-lib FILE] [--n-steps 512] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rl_collect_rate import GAMMA, LAM, M, library, overlap, stat  # noqa: E402

TWO = ("monteblanco", "modena")
RESTART = (0, 100, 200, 400, 500, 700, 800)          # environment.py:196


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--n-steps", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm
    from tum_control_amd.planner import load_track

    gold = os.path.join(ROOT, "tests", "golden")
    table = np.load(os.path.join(gold, "rl_env.npz"))["F"]
    P26 = np.load(os.path.join(gold, "closed_loop_monteblanco_150.npz"))["params"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def pair(tag, fa, fb, names, per=1.0, scale=1e3, unit="ms", same=None):
        """fa / fb interleaved, in alternating order; `same(ra, rb)` holds their results to each other"""
        ta, tb = [], []
        for r in range(a.reps + 1):
            if r % 2:          # (the order within a pair alternates: neither side always runs behind the other)
                da, ra = timed(fa); db, rb = timed(fb)
            else:
                db, rb = timed(fb); da, ra = timed(fa)
            if same is not None:
                assert same(ra, rb), tag + ": the results differ"
            if r:
                ta.append(da / per); tb.append(db / per)
        say(f"  {tag} {names[0]:<12}: {stat(ta, scale, unit)}")
        say(f"  {' ' * len(tag)} {names[1]:<12}: {stat(tb, scale, unit)}   {overlap(ta, tb)}; ratio of the medians {np.median(ta) / np.median(tb):.4f}"
            + ("; results equal to the bit" if same is not None else ""))

    say(f"# scripts/multi_track_rate.py --reps {a.reps} --n-steps {a.n_steps}" + (" --parent-lib <build of the parent commit>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")
    K = 200
    starts = lambda B, n: (np.arange(B) * 37) % n

    def loop(B, names=None, lib=None):
        with library(lib):
            if names is None:
                return clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, idx_start=starts(B, 1190), on_device=True)
            return clm.ClosedLoopBatch(list(names), batch=B, N=38, Tp=3.04, idx_start=starts(B, 1002), on_device=True)

    def run_k(cl):
        def f():
            cl.dev.set_state(cl.x_sim0, cl.x_mpc0, cold_start=True)
            cl.dev.run(50)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cl.dev.run(K)
            f.t = time.perf_counter() - t0
            return cl.dev.get("x_sim")
        return f

    def run_pair(tag, ca, cb, names, same):
        """run(K) of two loops interleaved, the time of run(K) alone"""
        for c in (ca, cb):
            c.x_sim0, c.x_mpc0 = c.x_sim.copy(), c.x_mpc.copy()
        fa, fb = run_k(ca), run_k(cb)
        ta, tb = [], []
        for r in range(a.reps + 1):
            if r % 2:          # (the order within a pair alternates)
                ra = fa(); rb = fb()
            else:
                rb = fb(); ra = fa()
            if same:
                assert np.array_equal(ra, rb), tag + ": the results differ"
            if r:
                ta.append(fa.t / K); tb.append(fb.t / K)
        say(f"  {tag} {names[0]:<12}: {stat(ta, 1e6, 'us')}")
        say(f"  {' ' * len(tag)} {names[1]:<12}: {stat(tb, 1e6, 'us')}   {overlap(ta, tb)}; ratio of the medians {np.median(ta) / np.median(tb):.4f}"
            + ("; results equal to the bit" if same else ""))

    def env(B, names="monteblanco", lib=None, **kw):
        n = 1190 if isinstance(names, str) else 1002
        with library(lib):
            return clm.WeightScheduleEnv(names, B, table, n_mpc_steps=M, auto_reset=True, restart_indices=RESTART,
                                         idx_start=np.asarray(RESTART)[np.arange(B) % len(RESTART)] % n, N=38, Tp=3.04, seed=1, **kw)

    # the README's segment workload (scripts/segment_scores.py): 26 weight sets x 8 Monteblanco segments, ends 6 s of race-line time away
    track = load_track("monteblanco")
    n = len(track)
    seg_starts = (np.arange(8) * (n // 8)).astype(np.int64)
    dt = np.hypot(*(np.roll(track[:, :2], -1, axis=0) - track[:, :2]).T) / np.roll(track[:, 3], -1)
    ends = []
    for s0 in seg_starts:
        t, i = 0.0, int(s0)
        while t < 6.0:
            t += dt[i % n]; i += 1
        ends.append(i % n)
    pairs8 = np.stack([seg_starts, np.array(ends)], axis=1)

    def evaluate8(lib):
        def f():
            with library(lib):
                o, fe, seg = clm.evaluate_segments("monteblanco", P26, [pairs8[:4], pairs8[4:]], np.inf, np.inf, 500, check_every=100)
            return o, fe, seg["max_lat_dev"], seg["rms_vel_dev"], seg["steps"]
        return f

    same_all = lambda x, y: all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))
    if a.parent_lib:
        plib = os.path.abspath(a.parent_lib)
        say("single-track paths, this build against a build of the parent commit:")
        for B in (16, 4096):
            run_pair(f"(1) control step, {B:4d} vehicles, run({K}):", loop(B), loop(B, lib=plib), ("this build", "parent"), True)
        for B in (16, 4096):
            ea, eb = env(B), env(B, lib=plib)
            Es = 8
            acts = np.random.RandomState(2).randint(0, len(table), size=(Es, B))

            def steps(e):
                def f():
                    for act in acts:
                        out = e.step(act)
                    return [out[0], out[1], e.dev.get("x_sim")]
                return f
            pair(f"(2) environment step, {B:4d} vehicles:", steps(ea), steps(eb), ("this build", "parent"), per=Es, same=same_all)
            del ea, eb
        pair("(3) evaluate_segments, 26 x 8 Monteblanco:", evaluate8(None), evaluate8(plib), ("this build", "parent"), same=same_all)
    say("a mixed Monteblanco / Modena loop (instance i on track i % 2) against the single-track loop of the same batch, this build:")
    for B in (16, 4096):
        cm, cs = loop(B, TWO), loop(B)
        run_pair(f"(4) control step, {B:4d} vehicles, run({K}):", cm, cs, ("mixed", "single track"), False)

        def plans(c):
            def f():
                for _ in range(K):
                    c.dev.plan()
                return c.dev.get("closest")
            return f
        pair(f"    planner launch alone, {B:4d} vehicles:", plans(cm), plans(cs), ("mixed", "single track"), per=K, scale=1e6, unit="us")
        del cm, cs
    say("the reference's own workloads (they need a track set):")
    groups = clm.train_segments()
    t5 = []
    for r in range(a.reps + 1):
        d, (o, fe, seg) = timed(lambda: clm.evaluate_segments(None, P26, groups, 2.0, 1.02, 4000, check_every=100))
        if r:
            t5.append(d)
    say(f"  (5) evaluate_segments, 26 weight sets x 20 training segments of modena + monteblanco = {len(seg['steps'])} loops, max_lat_dev 2.0, "
        f"max_a_comb 1.02, cap 4000 steps: {stat(t5)}; feasible {int(fe.sum())}/26, longest segment {int(seg['steps'].max())} steps, "
        f"timed out {int(seg['timed_out'].sum())}")
    import policy_reference as pr
    PI, VFN = (22, 128, 256, 128, 26), (22, 128, 256, 128, 1)
    W, b = pr.synthetic_policy(PI, 11)
    V, c = pr.synthetic_policy(VFN, 12)
    E, B = a.n_steps, 16
    e16 = env(B, list(TWO))
    trainer = clm.PPOTrainer(e16, clm.WeightPolicy(W, b, V, c), clip_range=0.2, ent_coef=0.006, vf_coef=0.5, max_grad_norm=0.5)
    e1 = env(B)
    trainer1 = clm.PPOTrainer(e1, clm.WeightPolicy(W, b, V, c), clip_range=0.2, ent_coef=0.006, vf_coef=0.5, max_grad_norm=0.5)
    rng = np.random.RandomState(0)
    tc, tu, tc1 = [], [], []
    for r in range(a.reps + 1):
        perm = np.stack([rng.permutation(E * B) for _ in range(5)])
        d0, _ = timed(lambda: e16.collect(trainer, E, GAMMA, LAM))
        d1, s = timed(lambda: trainer.update(None, perm, 5, 4096, 3e-4))
        d2, _ = timed(lambda: e1.collect(trainer1, E, GAMMA, LAM))
        assert np.isfinite(s["loss"]).all()
        if r:
            tc.append(d0); tu.append(d1); tc1.append(d2)
    say(f"  (6) 8 + 8 environments on monteblanco and modena, n_mpc_steps {M}, nets {list(PI[1:-1])}:")
    say(f"      collect({E})                               : {stat(tc)}")
    say(f"      update, {E * B} rows, batch_size 4096, 5 epochs : {stat(tu)}")
    say(f"      collect({E}), 16 environments on monteblanco : {stat(tc1)}   {overlap(tc, tc1)}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
