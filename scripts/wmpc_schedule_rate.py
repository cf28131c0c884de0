"""
wmpc_schedule_rate.py -- what the learned weight schedule inside the device loop costs (profiles/wmpc_schedule_rate.txt). Medians and
ranges of `--reps` interleaved repetitions behind one warm-up repetition; every wall time ends in a device synchronise. Monteblanco,
N = 38, the shipped agent and table.

  (1) per control step, nominal controller, 16 and 4096 vehicles, run(K) with chunks replayed: the schedule attached with period 20
      against nothing attached
  (2) the kernel alone, 16 and 4096 vehicles: K control steps with period 0 (every tile due at every step) and with a period no run
      reaches (every launch takes the early exit), each against nothing attached -- the difference per step is the kernel's own time
      plus its launch
  (3) against the host-driven alternative at 16 vehicles, all three controllers: run(K) with the schedule attached against K x
      (run(1), read x_mpc / ref0 / the window, decide on the host, set_weights for the due instances), period 20
With --parent-lib FILE (libtumnmpc.so of a build of the parent commit):
  (0) a loop with NOTHING attached on this build against the parent's, same job, interleaved, results compared to the bit

    python scripts/wmpc_schedule_rate.py [--reps 6] [--parent-lib FILE] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rl_collect_rate import library, overlap, stat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm

    gold = os.path.join(ROOT, "tests", "golden")
    table = np.load(os.path.join(gold, "rl_env.npz"))["F"]
    agent = clm.WeightPolicy.from_npz(os.path.join(gold, "wmpc_policy.npz"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# scripts/wmpc_schedule_rate.py --reps {a.reps}" + (" --parent-lib <build of the parent commit>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")
    K = 200
    starts = lambda B: (np.arange(B) * 37) % 1190

    def loop(B, lib=None, controller="nominal", period=None, tab=None):
        kw = {} if period is None else dict(wmpc=(agent, table if tab is None else tab), weights_update_period=period)
        with library(lib):
            return clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, idx_start=starts(B), on_device=True, controller=controller, **kw)

    def run_k(cl, k=K):
        def f():
            cl.dev.set_state(cl.x_sim0, cl.x_mpc0, cold_start=True)
            cl.dev.run(50)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cl.dev.run(k)
            f.t = time.perf_counter() - t0
            return cl.dev.get("x_sim")
        return f

    def host_driven(cl, k):
        """the alternative without the kernel: stop after every control step"""
        def f():
            cl.dev.set_state(cl.x_sim0, cl.x_mpc0, cold_start=True)
            cl.set_weights(cl.p0)
            cl.dev.run(50)
            sched = clm.WmpcSchedule(agent, table, 20, cl.B)
            cur = cl.p0.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(k):
                x0 = cl.dev.get("x_mpc")
                cl.dev.run(1)
                due, actions = sched.after_solve(i, x0, cl.dev.get("ref0"), cl.dev.get("yref"))
                if len(due):
                    cur[due] = table[actions]
                    cl.set_weights(cur)
            f.t = time.perf_counter() - t0
            return cl.dev.get("x_sim")
        return f

    def run_pair(tag, fa, fb, names, same, k=K):
        ta, tb = [], []
        for r in range(a.reps + 1):
            if r % 2:          # (the order within a pair alternates: neither side always runs behind the other)
                ra = fa(); rb = fb()
            else:
                rb = fb(); ra = fa()
            if same:
                assert np.array_equal(ra, rb), tag + ": the results differ"
            if r:
                ta.append(fa.t / k); tb.append(fb.t / k)
        say(f"  {tag} {names[0]:<14}: {stat(ta, 1e6, 'us')}")
        say(f"  {' ' * len(tag)} {names[1]:<14}: {stat(tb, 1e6, 'us')}   {overlap(ta, tb)}; difference of the medians "
            f"{(np.median(ta) - np.median(tb)) * 1e6:+.3f} us, ratio {np.median(ta) / np.median(tb):.4f}" + ("; results equal to the bit" if same else ""))

    def prepared(cl):
        cl.x_sim0, cl.x_mpc0 = cl.x_sim.copy(), cl.x_mpc.copy()
        return cl

    if a.parent_lib:
        plib = os.path.abspath(a.parent_lib)
        say("(0) nothing attached, this build against a build of the parent commit:")
        for B in (16, 4096):
            ca, cb = prepared(loop(B)), prepared(loop(B, lib=plib))
            run_pair(f"control step, {B:4d} vehicles, run({K}):", run_k(ca), run_k(cb), ("this build", "parent"), True)
            del ca, cb
    say("(1) the schedule attached with period 20 against nothing attached (nominal controller):")
    for B in (16, 4096):
        ca, cb = prepared(loop(B, period=20)), prepared(loop(B))
        run_pair(f"control step, {B:4d} vehicles, run({K}):", run_k(ca), run_k(cb), ("period 20", "nothing"), False)
        del ca, cb
    say("    ... and with a table whose 26 rows are the weights the loop has anyway: the same decisions, installs that change nothing the")
    say("    solver sees -- the kernel without what the agent's weights do to the solves:")
    from tum_control_amd import config
    m = config.default_config()["mpc"]          # (q_lon = q_lat in the shipped YAML: the defaults ARE a row of the table's form)
    same_rows = np.tile([0.01 * m["q_lon"] / m["s_lon"] ** 2, 0.01 * m["q_yaw"] / m["s_yaw"] ** 2, 0.01 * m["q_vel"] / m["s_vel"] ** 2,
                         0.01 * m["r_jerk"] / m["s_jerk"] ** 2, 0.01 * m["r_steering_rate"] / m["s_steering_rate"] ** 2,
                         m["L1_pen"], m["L2_pen"]], (len(table), 1))
    for B in (16, 4096):
        ca, cb = prepared(loop(B, period=20, tab=same_rows)), prepared(loop(B))
        run_pair(f"control step, {B:4d} vehicles, run({K}):", run_k(ca), run_k(cb), ("period 20", "nothing"), False)
        del ca, cb
    say("(2) the kernel alone: every tile due at every step (period 0), and every launch on the early exit (period 1000000):")
    for B in (16, 4096):
        cn = prepared(loop(B))
        for period, name in ((0, "all due"), (1000000, "early exit")):
            ca = prepared(loop(B, period=period))
            run_pair(f"control step, {B:4d} vehicles, run({K}):", run_k(ca), run_k(cn), (name, "nothing"), False)
            del ca
        del cn
    say("(3) attached against the host-driven alternative (run(1), three reads, numpy, set_weights), 16 vehicles, period 20:")
    Kh = 100
    for controller in ("nominal", "snmpc", "r2"):
        ca, cb = prepared(loop(16, controller=controller, period=20)), prepared(loop(16, controller=controller))
        cb.p0 = np.tile(table[0], (16, 1)); ca.set_weights(cb.p0)
        ca.dev.attach_wmpc(table, 20)          # (the snapshot is row 0 on both sides)
        fa = run_k(ca, Kh)

        def fa0(fa=fa, ca=ca, cb=cb):
            ca.set_weights(cb.p0)
            r = fa()
            fa0.t = fa.t
            return r
        run_pair(f"{controller:8s} control step, run({Kh}) | {Kh} x run(1):", fa0, host_driven(cb, Kh), ("attached", "host-driven"), False, k=Kh)          # (tests/test_gpu_wmpc_schedule.py holds the two to each other, to the bit)
        del ca, cb
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
