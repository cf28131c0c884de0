"""
rl_env_rate.py -- what the RL environment on the device buys over driving the loop as one from the host (profiles/rl_env_rate.txt).

Workload: B copies of the reference's RL environment on Monteblanco (N = 38, n_mpc_steps = 20, the 26 rows of the reference's action
table from tests/golden/rl_env.npz, random actions), B = 16 (the reference's n_environments) and B = 4096. Two paths on the same build,
interleaved, one environment step per repetition:
  (a) WeightScheduleEnv.step                     (one upload, begin kernel, 20 control steps with the score kernel, finish kernel, one download)
  (b) ClosedLoopBatch.set_weights(table[actions]) + dev.run(20) + dev.logs() + closed_loop.rl_env_steps_from_logs
      (the loop of (b) keeps 20 steps of logs; between repetitions, untimed, its step counter is put back with set_state so that
      logs() copies those 20 steps and no more)
Then the time of a bare control step, run(K), of one loop with the environment attached and detached, interleaved -- and, with
--parent-lib, of the same loop (same start states, same weights) on a library built from the parent commit, loaded beside this one.

    python scripts/rl_env_rate.py [--reps 6] [--batches 16,4096] [--steps 500] [--parent-lib FILE] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 20


def stat(v, scale=1e3, unit="ms"):
    v = np.asarray(v) * scale
    return f"median {np.median(v):9.3f} {unit}  range {v.min():9.3f} .. {v.max():9.3f}  (n = {len(v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--batches", default="16,4096")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm
    from tum_control_amd import solver

    table = np.load(os.path.join(ROOT, "tests", "golden", "rl_env.npz"))["F"]
    restart = (0, 100, 200, 400, 500, 700, 800)          # environment.py:196
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# scripts/rl_env_rate.py --reps {a.reps} --batches {a.batches} --steps {a.steps}" + (" --parent-lib <parent build>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")
    for B in [int(b) for b in a.batches.split(",")]:
        rng = np.random.RandomState(B)
        starts = np.asarray(restart)[np.arange(B) % len(restart)]
        env = clm.WeightScheduleEnv("monteblanco", B, table, n_mpc_steps=M, episode_length=128, restart_indices=restart, seed=0,
                                    idx_start=starts, N=38, Tp=3.04)
        lb = clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, idx_start=starts, on_device=True, log_capacity=M)
        ta, tb, parts = [], [], []
        for r in range(a.reps + 1):          # (repetition 0 warms both paths up)
            act = rng.randint(0, len(table), size=B)
            t0 = time.perf_counter()
            env.step(act)
            t1 = time.perf_counter()
            lb.set_weights(table[act])
            t2 = time.perf_counter()
            lb.dev.run(M)
            t3 = time.perf_counter()
            logs = lb.dev.logs()
            t4 = time.perf_counter()
            clm.rl_env_steps_from_logs(logs, lb.track, act[None], M)
            t5 = time.perf_counter()
            lb.dev.set_state(lb.dev.get("x_sim"), lb.dev.get("x_mpc"), cold_start=False)          # untimed: logs() copies 20 steps again
            if r:
                ta.append(t1 - t0); tb.append(t5 - t1); parts.append((t2 - t1, t3 - t2, t4 - t3, t5 - t4))
        parts = np.array(parts)
        say(f"B = {B}, n_mpc_steps = {M}: one environment step")
        say(f"  (a) WeightScheduleEnv.step                : {stat(ta)}   = {1.0 / np.median(ta):9.1f} environment steps/s, {B / np.median(ta):11.1f} instance steps/s")
        say(f"  (b) setters + run + logs + numpy          : {stat(tb)}   = {1.0 / np.median(tb):9.1f} environment steps/s")
        for name, col in (("set_weights (13 cost_set)", 0), (f"run({M})", 1), ("logs() copy", 2), ("rl_env_steps_from_logs", 3)):
            say(f"      of (b): {name:<28}: {stat(parts[:, col])}")
        # the bare control step: attached / detached (/ parent build), interleaved
        K = a.steps
        kw = dict(n_mpc_steps=M, max_lat_dev=2.0, episode_length=128, sigmas=clm.RL_SIGMAS, lims=clm.RL_LIMS)
        loops = {"attached": lb, "detached": lb}
        if a.parent_lib:
            old = solver._default_path
            solver._default_path = os.path.abspath(a.parent_lib)
            try:
                loops["parent"] = clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, idx_start=starts, on_device=True, log_capacity=M)
                loops["parent"].set_weights(table[act])          # (the weights the other loop was left with: they decide the iteration counts)
            finally:
                solver._default_path = old
        x_sim, x_mpc = lb.x_sim.copy(), lb.x_mpc.copy()
        t = {k: [] for k in loops}
        for r in range(a.reps + 1):
            for which, lp in loops.items():
                if which == "attached":
                    lp.dev.attach_env(table, **kw)
                elif which == "detached":
                    lp.dev.detach_env()
                lp.dev.set_state(x_sim, x_mpc, cold_start=True)
                lp.dev.run(50)          # (captures the chunk again)
                t0 = time.perf_counter(); lp.dev.run(K); t1 = time.perf_counter()
                if r:
                    t[which].append((t1 - t0) / K)
        say(f"  time per control step, run({K}): " + "; ".join(f"{k} {stat(v, 1e6, 'us')}" for k, v in t.items()))
        say(f"      attached - detached {(np.median(t['attached']) - np.median(t['detached'])) * 1e6:+.2f} us"
            + (f"; detached - parent {(np.median(t['detached']) - np.median(t['parent'])) * 1e6:+.2f} us" if "parent" in t else ""))
        del env, lb, loops
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
