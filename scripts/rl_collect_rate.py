"""
rl_collect_rate.py -- what collecting PPO training data on the device buys against one host round trip per environment step, and
whether the paths that existed before take what they took (profiles/rl_collect_rate.txt).

Workload: B copies of the reference's RL environment on Monteblanco (N = 38, n_mpc_steps = 20, the 26 rows of the reference's action
table from tests/golden/rl_env.npz), the trained agent of tests/golden/wmpc_policy.npz + wmpc_value.npz SAMPLING every action, 32
environment steps, B = 16 (the reference's n_environments) and B = 4096. Two environments that start alike, interleaved:
  (c) WeightScheduleEnv.collect(policy, 32, gamma, lambda)      policy_ac_kernel + environment + control steps + record + GAE, one wait
  (h) 32 x [policy_eval_ac(obs) -> step() -> policy_eval_ac(terminal observations)] and closed_loop.gae: the same kernels, three host
      round trips per environment step
Episodes are 128 steps long as in the reference's rl_config.yaml, so none ends inside the first repetitions; the two paths must return
the same buffers: asserted on actions, values and advantages.

With --parent-lib FILE (libtumnmpc.so of a build of the parent commit) also the UNCHANGED paths, same job on both builds, interleaved,
no value net attached:
  (s) 32 x step(fixed actions)            (r) rollout(policy, 32)
"Unchanged" means the two ranges overlap.

    python scripts/rl_collect_rate.py [--reps 6] [--batches 16,4096] [--steps 32] [--parent-lib FILE] [--out FILE]
"""
import argparse
import contextlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 20
GAMMA, LAM = 0.99, 0.95          # rl_config.yaml


def stat(v, scale=1e3, unit="ms"):
    v = np.asarray(v) * scale
    return f"median {np.median(v):9.3f} {unit}  range {v.min():9.3f} .. {v.max():9.3f}  (n = {len(v)})"


def overlap(a, b):
    return "ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "ranges DO NOT overlap"


@contextlib.contextmanager
def library(path):
    """solvers created inside bind to the library at `path` (None: the shipped one)"""
    from tum_control_amd import solver
    old = solver._default_path
    solver._default_path = path
    try:
        yield
    finally:
        solver._default_path = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--batches", default="16,4096")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm

    gold = os.path.join(ROOT, "tests", "golden")
    table = np.load(os.path.join(gold, "rl_env.npz"))["F"]
    agent = clm.WeightPolicy.from_npz(os.path.join(gold, "wmpc_policy.npz"), os.path.join(gold, "wmpc_value.npz"))
    bare = clm.WeightPolicy(agent.weights, agent.biases)
    restart = (0, 100, 200, 400, 500, 700, 800)          # environment.py:196
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    E = a.steps
    say(f"# scripts/rl_collect_rate.py --reps {a.reps} --batches {a.batches} --steps {E}" + (" --parent-lib <build of the parent commit>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")

    def make(B, lib=None):
        starts = np.asarray(restart)[np.arange(B) % len(restart)]
        with library(lib):
            return clm.WeightScheduleEnv("monteblanco", B, table, n_mpc_steps=M, auto_reset=True, restart_indices=restart, idx_start=starts,
                                         N=38, Tp=3.04, seed=1)

    for B in [int(b) for b in a.batches.split(",")]:
        envs = [make(B), make(B)]
        envs[1].dev.attach_policy(agent)
        obs = np.zeros((B, 22))
        t = [[], []]
        parts = [[], [], []]
        for r in range(a.reps + 1):          # (repetition 0 warms every path up)
            t0 = time.perf_counter()
            c = envs[0].collect(agent, E, GAMMA, LAM)
            t1 = time.perf_counter()
            env, dev = envs[1], envs[1].dev
            rows = {k: [] for k in ("actions", "values", "rewards", "starts")}
            es = env._episode_starts.copy()
            tp = tv = 0.0
            for e in range(E):
                tq = time.perf_counter()
                ac = dev.policy_eval_ac(obs, env._seed, env._t)
                tp += time.perf_counter() - tq
                obs, rew, te, tr, info = env.step(ac["actions"])
                tq = time.perf_counter()
                term_v = dev.policy_eval_ac(info["terminal_observation"], 0, 0)["values"]
                tv += time.perf_counter() - tq
                crash = tr & ~te
                rew = np.where(crash, rew + GAMMA * term_v, rew)
                for k, v in (("actions", ac["actions"]), ("values", ac["values"]), ("rewards", rew), ("starts", es)):
                    rows[k].append(v)
                es = (te | tr).astype(float)
            tq = time.perf_counter()
            last_v = dev.policy_eval_ac(obs, 0, 0)["values"]
            adv, _ = clm.gae(np.stack(rows["rewards"]), np.stack(rows["values"]), np.stack(rows["starts"]), last_v, es, GAMMA, LAM)
            tg = time.perf_counter() - tq
            t2 = time.perf_counter()
            if r:
                t[0].append((t1 - t0) / E); t[1].append((t2 - t1) / E)
                parts[0].append(tp / E); parts[1].append(tv / E); parts[2].append(tg / E)
            # the same buffers as long as no instance was reset (step() and collect() draw their start waypoints differently)
            if not (c["episode_starts"][1:].any() or np.stack(rows["starts"])[1:].any()) and r == 0:
                assert np.array_equal(c["actions"], np.stack(rows["actions"])) and np.array_equal(c["values"], np.stack(rows["values"]))
                assert np.array_equal(c["advantages"], adv), "collect() and the host-driven loop disagree"
        say(f"B = {B}, n_mpc_steps = {M}, {E} environment steps per repetition: time per environment step")
        say(f"  (c) collect() on the device                      : {stat(t[0])}   = {1.0 / np.median(t[0]):9.1f} environment steps/s, {B / np.median(t[0]):11.1f} instance steps/s")
        say(f"  (h) eval_ac -> step -> eval_ac(values) + numpy GAE : {stat(t[1])}")
        say(f"      of which eval_ac {stat(parts[0])}")
        say(f"               values of the terminal observations {stat(parts[1])}")
        say(f"               last values + GAE (per step) {stat(parts[2])}")
        say(f"      (h) - (c) {(np.median(t[1]) - np.median(t[0])) * 1e3:+.3f} ms per environment step; {overlap(t[0], t[1])}")
        del envs
        if a.parent_lib:
            libs = (None, os.path.abspath(a.parent_lib))
            pair = [make(B, lib) for lib in libs]
            roll = [make(B, lib) for lib in libs]
            acts = np.random.RandomState(2).randint(0, len(table), size=(E, B))
            ts, tr_ = [[], []], [[], []]
            for r in range(a.reps + 1):
                for j in (0, 1):
                    tq = time.perf_counter()
                    for e in range(E):
                        pair[j].step(acts[e])
                    tm = time.perf_counter()
                    roll[j].rollout(bare, E)
                    te = time.perf_counter()
                    if r:
                        ts[j].append((tm - tq) / E); tr_[j].append((te - tm) / E)
            assert np.array_equal(pair[0].dev.get("x_sim"), pair[1].dev.get("x_sim")), "step() differs between the two builds"
            assert np.array_equal(roll[0].dev.get("x_sim"), roll[1].dev.get("x_sim")), "rollout() differs between the two builds"
            say(f"  unchanged paths, no value net attached, this build against the parent commit's (final plant states equal to the bit):")
            say(f"  (s) step(fixed actions)   this build : {stat(ts[0])}")
            say(f"                            parent     : {stat(ts[1])}   {overlap(ts[0], ts[1])}")
            say(f"  (r) rollout(policy)       this build : {stat(tr_[0])}")
            say(f"                            parent     : {stat(tr_[1])}   {overlap(tr_[0], tr_[1])}")
            del pair, roll
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
