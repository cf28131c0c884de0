"""
rl_update_rate.py -- what one PPO update on the device takes, against the same update in torch on the same GPU, and what share of a
training iteration it is (profiles/rl_update_rate.txt).

Workload: the reference's training iteration (rl_config.yaml): 16 environments on Monteblanco (N = 38, n_mpc_steps = 20, the 26 rows of
tests/golden/rl_env.npz), n_steps 512 -> 8192 buffer rows, batch_size 4096, n_epochs 5, nets [128, 256, 128] for policy and value
(seeded: tests/policy_reference.synthetic_policy), clip 0.2, ent_coef 0.006, vf_coef 0.5, max_grad_norm 0.5. Per repetition, interleaved:
  (c)   env.collect(trainer, 512)                     the collection, the resident nets acting
  (d)   trainer.update(None, perm, 5, 4096, lr)       the update on the buffer collect left on the device: 10 minibatches, one wait
  (t32) the same 10 minibatches in torch on the same GPU, float32 (what stable_baselines3 runs), Adam eps 1e-5, clip_grad_norm_
  (t64) the same in torch float64
The torch updates train their own copy of the nets on the buffer of the same repetition (downloaded once, uploaded before the clock
starts). Nothing is claimed beyond what the ranges support.

With --parent-lib FILE (libtumnmpc.so of a build of the parent commit) also the UNCHANGED paths, same job on both builds, interleaved:
  (s) 32 x step(fixed actions)     (r) rollout(policy, 32)     (p) collect(policy, 32)
"Unchanged" means the two ranges overlap.

    python scripts/rl_update_rate.py [--reps 6] [--n-steps 512] [--parent-lib FILE] [--out FILE]
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

B, BATCH, EPOCHS, LR = 16, 4096, 5, 3e-4
CLIP, ENT, VF, MAXNORM = 0.2, 0.006, 0.5, 0.5
PI, VFN = (22, 128, 256, 128, 26), (22, 128, 256, 128, 1)


def torch_update(torch, nets, opt, buf, perm, dtype):
    """PPO.train of stable_baselines3 on (pi, vf) Sequential nets: one update over perm (n_epochs, N)"""
    pi, vf = nets
    obs, act, olp, adv, ret = buf
    params = list(pi.parameters()) + list(vf.parameters())
    for p in perm:
        for k in range(0, len(p), BATCH):
            i = p[k:k + BATCH]
            a = adv[i]
            if len(i) > 1:
                a = (a - a.mean()) / (a.std() + 1e-8)
            dist = torch.distributions.Categorical(logits=pi(obs[i]))
            ratio = torch.exp(dist.log_prob(act[i]) - olp[i])
            pl = -torch.min(a * ratio, a * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
            vl = torch.nn.functional.mse_loss(ret[i], vf(obs[i]).flatten())
            loss = pl + ENT * -dist.entropy().mean() + VF * vl
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, MAXNORM)
            opt.step()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--n-steps", type=int, default=512)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import policy_reference as pr
    from tum_control_amd import closed_loop as clm

    gold = os.path.join(ROOT, "tests", "golden")
    table = np.load(os.path.join(gold, "rl_env.npz"))["F"]
    restart = (0, 100, 200, 400, 500, 700, 800)          # environment.py:196
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    E = a.n_steps
    N = E * B
    say(f"# scripts/rl_update_rate.py --reps {a.reps} --n-steps {E}" + (" --parent-lib <build of the parent commit>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")

    def make(lib=None):
        starts = np.asarray(restart)[np.arange(B) % len(restart)]
        with library(lib):
            return clm.WeightScheduleEnv("monteblanco", B, table, n_mpc_steps=M, auto_reset=True, restart_indices=restart, idx_start=starts,
                                         N=38, Tp=3.04, seed=1)

    W, b = pr.synthetic_policy(PI, 11)
    V, c = pr.synthetic_policy(VFN, 12)
    env = make()
    trainer = clm.PPOTrainer(env, clm.WeightPolicy(W, b, V, c), clip_range=CLIP, ent_coef=ENT, vf_coef=VF, max_grad_norm=MAXNORM)

    def torch_nets(dtype):
        out = []
        for Ws, bs in ((W, b), (V, c)):
            layers = []
            for l, (w, bb) in enumerate(zip(Ws, bs)):
                lin = torch.nn.Linear(w.shape[1], w.shape[0])
                with torch.no_grad():
                    lin.weight.copy_(torch.tensor(w)); lin.bias.copy_(torch.tensor(bb))
                layers += [lin] + ([torch.nn.Tanh()] if l + 1 < len(Ws) else [])
            out.append(torch.nn.Sequential(*layers).to("cuda:0", dtype))
        return out, torch.optim.Adam([p for n in out for p in n.parameters()], lr=LR, eps=1e-5)
    tn = {dt: torch_nets(dt) for dt in (torch.float32, torch.float64)}
    t = {k: [] for k in ("c", "d", "t32", "t64")}
    rng = np.random.RandomState(0)
    for r in range(a.reps + 1):          # (repetition 0 warms every path up)
        perm = np.stack([rng.permutation(N) for _ in range(EPOCHS)])
        t0 = time.perf_counter()
        d = env.collect(trainer, E, GAMMA, LAM)
        t1 = time.perf_counter()
        s = trainer.update(None, perm, EPOCHS, BATCH, LR)
        t2 = time.perf_counter()
        assert np.isfinite(s["loss"]).all() and s["n"].sum() == EPOCHS * N
        tt = {}
        for key, dt in (("t32", torch.float32), ("t64", torch.float64)):
            buf = [torch.tensor(d["observations"].reshape(N, -1).astype(np.float32), device="cuda:0").to(dt),
                   torch.tensor(d["actions"].reshape(N), device="cuda:0")] + \
                  [torch.tensor(d[k].reshape(N), device="cuda:0").to(dt) for k in ("log_probs", "advantages", "returns")]
            p = torch.tensor(perm, device="cuda:0")
            torch.cuda.synchronize()
            tq = time.perf_counter()
            torch_update(torch, *tn[dt], buf, p, dt)
            tt[key] = time.perf_counter() - tq
        if r:
            t["c"].append(t1 - t0); t["d"].append(t2 - t1); t["t32"].append(tt["t32"]); t["t64"].append(tt["t64"])
    n_mb = EPOCHS * ((N + BATCH - 1) // BATCH)
    say(f"{B} environments, n_steps {E} = {N} rows, batch_size {BATCH}, n_epochs {EPOCHS} = {n_mb} minibatches, nets {list(PI[1:-1])}: time per call")
    say(f"  (c)   collect(trainer, {E})               : {stat(t['c'])}")
    say(f"  (d)   update on the device, FP64          : {stat(t['d'])}   = {np.median(t['d']) / n_mb * 1e3:7.3f} ms per minibatch")
    say(f"  (t32) torch on the same GPU, float32      : {stat(t['t32'])}   (d) against (t32): {overlap(t['d'], t['t32'])}")
    say(f"  (t64) torch on the same GPU, float64      : {stat(t['t64'])}   (d) against (t64): {overlap(t['d'], t['t64'])}")
    say(f"  the update's share of a training iteration (c) + (d): {100 * np.median(t['d']) / (np.median(t['c']) + np.median(t['d'])):.2f} %")
    del env, trainer
    if a.parent_lib:
        from tum_control_amd.closed_loop import WeightPolicy
        agent = WeightPolicy.from_npz(os.path.join(gold, "wmpc_policy.npz"), os.path.join(gold, "wmpc_value.npz"))
        bare = WeightPolicy(agent.weights, agent.biases)
        Es = 32
        libs = (None, os.path.abspath(a.parent_lib))
        pair, roll, coll = ([make(lib) for lib in libs] for _ in range(3))
        acts = np.random.RandomState(2).randint(0, len(table), size=(Es, B))
        ts, tr_, tc = [[], []], [[], []], [[], []]
        for r in range(a.reps + 1):
            for j in (0, 1):
                tq = time.perf_counter()
                for e in range(Es):
                    pair[j].step(acts[e])
                tm = time.perf_counter()
                roll[j].rollout(bare, Es)
                te = time.perf_counter()
                cj = coll[j].collect(agent, Es, GAMMA, LAM)
                tf = time.perf_counter()
                if j == 0:
                    c0 = cj
                if r:
                    ts[j].append((tm - tq) / Es); tr_[j].append((te - tm) / Es); tc[j].append((tf - te) / Es)
            assert all(np.array_equal(c0[k], cj[k]) for k in c0), "collect(policy) differs between the two builds"
        assert np.array_equal(pair[0].dev.get("x_sim"), pair[1].dev.get("x_sim")), "step() differs between the two builds"
        assert np.array_equal(roll[0].dev.get("x_sim"), roll[1].dev.get("x_sim")), "rollout() differs between the two builds"
        say(f"  unchanged paths, {B} vehicles, per environment step, this build against the parent commit's (results equal to the bit):")
        for tag, tv in (("(s) step(fixed actions)", ts), ("(r) rollout(policy)    ", tr_), ("(p) collect(policy)    ", tc)):
            say(f"  {tag} this build : {stat(tv[0])}")
            say(f"  {' ' * len(tag)} parent     : {stat(tv[1])}   {overlap(tv[0], tv[1])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
