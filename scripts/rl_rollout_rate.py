"""
rl_rollout_rate.py -- what running the agent on the device buys: whole episodes enqueued at once against one host round trip per
environment step (profiles/rl_rollout_rate.txt).

Workload: B copies of the reference's RL environment on Monteblanco (N = 38, n_mpc_steps = 20, the 26 rows of the reference's action
table from tests/golden/rl_env.npz), driven by the trained agent of tests/golden/wmpc_policy.npz for 32 environment steps, B = 16
(the reference's n_environments) and B = 4096. Three paths on the same build, three environments that start alike, interleaved:
  (r) WeightScheduleEnv.rollout(policy, 32)                 policy_kernel + environment + control steps, one wait, one download
  (a) 32 x step(WeightPolicy.predict(obs))                  float64 numpy forward pass on the host
  (b) 32 x step(argmax of a torch float32 forward pass)     what stable_baselines3's model.predict computes, on the host's CPU
No episode ends inside the measurement (episode_length is out of reach). The three paths must pick the same actions: asserted.

    python scripts/rl_rollout_rate.py [--reps 6] [--batches 16,4096] [--steps 32] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm

    table = np.load(os.path.join(ROOT, "tests", "golden", "rl_env.npz"))["F"]
    policy = clm.WeightPolicy.from_npz(os.path.join(ROOT, "tests", "golden", "wmpc_policy.npz"))
    layers = []
    for i, (w, b) in enumerate(zip(policy.weights, policy.biases)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w)); lin.bias.copy_(torch.from_numpy(b))
        layers += [lin] + ([torch.nn.Tanh()] if i + 1 < len(policy.weights) else [])
    net = torch.nn.Sequential(*layers)

    def torch_predict(obs):
        with torch.no_grad():
            return net(torch.from_numpy(obs.astype(np.float32))).argmax(dim=1).numpy()

    restart = (0, 100, 200, 400, 500, 700, 800)          # environment.py:196
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    E = a.steps
    say(f"# scripts/rl_rollout_rate.py --reps {a.reps} --batches {a.batches} --steps {E}")
    torch.zeros(1, device="cuda:0")
    for B in [int(b) for b in a.batches.split(",")]:
        starts = np.asarray(restart)[np.arange(B) % len(restart)]
        envs = [clm.WeightScheduleEnv("monteblanco", B, table, n_mpc_steps=M, episode_length=10 ** 8, auto_reset=False, idx_start=starts,
                                      N=38, Tp=3.04) for _ in range(3)]
        obs = [np.zeros((B, 22)) for _ in range(3)]
        t = [[], [], []]
        pred = [[], []]
        differ = 0
        for r in range(a.reps + 1):          # (repetition 0 warms every path up)
            t0 = time.perf_counter()
            ro = envs[0].rollout(policy, E)
            t1 = time.perf_counter()
            acts = [[], []]
            for j, f in ((1, policy.predict), (2, torch_predict)):
                tp = 0.0
                ts = time.perf_counter()
                for _ in range(E):
                    tq = time.perf_counter()
                    act = f(obs[j])
                    tp += time.perf_counter() - tq
                    obs[j] = envs[j].step(act)[0]
                    acts[j - 1].append(act)
                te = time.perf_counter()
                if r:
                    t[j].append((te - ts) / E); pred[j - 1].append(tp / E)
            if r:
                t[0].append((t1 - t0) / E)
            assert np.array_equal(ro["action"].data, np.stack(acts[0])), "rollout and host float64 pick different actions"
            differ += int((np.stack(acts[0]) != np.stack(acts[1])).sum())
        say(f"B = {B}, n_mpc_steps = {M}, {E} environment steps per repetition: time per environment step")
        say(f"  (r) rollout on the device                 : {stat(t[0])}   = {1.0 / np.median(t[0]):9.1f} environment steps/s, {B / np.median(t[0]):11.1f} instance steps/s")
        say(f"  (a) step(WeightPolicy.predict), float64   : {stat(t[1])}   of which predict {stat(pred[0])}")
        say(f"  (b) step(torch float32 forward, CPU)      : {stat(t[2])}   of which forward {stat(pred[1])}")
        say(f"      (a) - (r) {(np.median(t[1]) - np.median(t[0])) * 1e3:+.3f} ms, (b) - (r) {(np.median(t[2]) - np.median(t[0])) * 1e3:+.3f} ms per environment step; "
            f"decisions where torch float32 and float64 differ: {differ} of {(a.reps + 1) * E * B}")
        del envs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
