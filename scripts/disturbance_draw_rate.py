"""
disturbance_draw_rate.py -- what drawing the closed loop's disturbance realisation on the device costs and buys
(profiles/disturbance_draw_rate.txt).

Workload: B closed loops on Monteblanco (N = 38, nominal controller, the shipped magnitudes with both streams on: 'uniform' derivative
disturbances, 'gaussian' estimation errors), B = 16 and B = 4096.
  (1) the time of a control step, run(K) after run(50) has captured the chunk, of loops with the same start states, interleaved:
        none      nothing attached            parent    the same on a library built from the parent commit (--parent-lib), loaded
        live      the generator attached                beside this one; its final states are compared with `none` bit for bit
        playback  the regenerated table of the same steps played back (so `live` and `playback` run the same numbers)
  (2) producing the realisation of B = 4096 vehicles x 500 steps, three ways:
        legacy    DisturbanceModel.draw, timed for 64 vehicles and scaled by 4096 / 64 (it is a Python loop over vehicles)
        counter   DisturbanceModel.draw_counter
        table     DeviceClosedLoop.disturbance_table (device draw + copy to the host)

    python scripts/disturbance_draw_rate.py [--reps 6] [--batches 16,4096] [--steps 500] [--parent-lib FILE] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x1234567890abcdef


def stat(v, scale=1e3, unit="ms"):
    v = np.asarray(v) * scale
    return f"median {np.median(v):9.3f} {unit}  range {v.min():9.3f} .. {v.max():9.3f}  (n = {len(v)})"


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


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

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# scripts/disturbance_draw_rate.py --reps {a.reps} --batches {a.batches} --steps {a.steps}" + (" --parent-lib <parent build>" if a.parent_lib else ""))
    torch.zeros(1, device="cuda:0")
    model = clm.DisturbanceModel(dict(simulate_disturbances=True, simulate_state_estimation=True))
    restart = (0, 100, 200, 400, 500, 700, 800)
    for B in [int(b) for b in a.batches.split(",")]:
        K = a.steps if B <= 256 else max(50, a.steps // 5)          # (a control step of 4096 vehicles takes milliseconds)
        starts = np.asarray(restart)[np.arange(B) % len(restart)]
        make = lambda: clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, idx_start=starts, on_device=True)
        loops = {"none": make()}
        if a.parent_lib:
            old = solver._default_path
            solver._default_path = os.path.abspath(a.parent_lib)
            try:
                loops["parent"] = make()
            finally:
                solver._default_path = old
        loops["live"] = make()
        loops["live"].dev.attach_disturbances(model, SEED)
        loops["playback"] = make()
        loops["playback"].set_disturbances(*loops["live"].dev.disturbance_table(0, 50 + K))
        x_sim, x_mpc = loops["none"].x_sim.copy(), loops["none"].x_mpc.copy()
        t = {k: [] for k in loops}
        end = {}
        for r in range(a.reps + 1):          # (repetition 0 warms every loop up)
            for which, lp in loops.items():
                lp.dev.set_state(x_sim, x_mpc, cold_start=True)
                lp.dev.run(50)
                t0 = time.perf_counter(); lp.dev.run(K); t1 = time.perf_counter()
                if r:
                    t[which].append((t1 - t0) / K)
                end[which] = (lp.dev.get("x_sim"), lp.dev.get("x_mpc"))
        say(f"B = {B}: time per control step, run({K})")
        for k, v in t.items():
            say(f"  {k:<9}: {stat(v, 1e6, 'us')}")
        med = {k: np.median(v) for k, v in t.items()}
        say(f"  live - playback {(med['live'] - med['playback']) * 1e6:+.2f} us = {100 * (med['live'] - med['playback']) / med['playback']:+.2f} % of the played-back step; "
            f"live - none {(med['live'] - med['none']) * 1e6:+.2f} us (two plant passes and the draw)")
        say(f"  live and playback end in the same states, bit for bit: {all(same_bits(x, y) for x, y in zip(end['live'], end['playback']))}")
        if "parent" in t:
            overlap = min(t["none"]) <= max(t["parent"]) and min(t["parent"]) <= max(t["none"])
            say(f"  none - parent {(med['none'] - med['parent']) * 1e6:+.2f} us, ranges overlap: {overlap}; "
                f"same states, bit for bit: {all(same_bits(x, y) for x, y in zip(end['none'], end['parent']))}")
        del loops
    # ---- (2) producing a realisation
    B, S, Bl = 4096, 500, 64
    lp = clm.ClosedLoopBatch("monteblanco", batch=B, N=38, Tp=3.04, on_device=True)
    lp.dev.attach_disturbances(model, SEED)
    t = dict(legacy=[], counter=[], table=[])
    for r in range(a.reps + 1):
        t0 = time.perf_counter(); model.draw(S, Bl, seed=r)
        t1 = time.perf_counter(); model.draw_counter(S, B, seed=r)
        t2 = time.perf_counter(); lp.dev.disturbance_table(0, S)
        t3 = time.perf_counter()
        if r:
            t["legacy"].append((t1 - t0) * (B / Bl)); t["counter"].append(t2 - t1); t["table"].append(t3 - t2)
    say(f"the realisation of {B} vehicles x {S} steps, both streams ({2 * B * S * 7 * 8 / 1e6:.0f} MB of table; the live draw keeps {2 * B * 7} doubles = {2 * B * 7 * 8 / 1e3:.0f} kB)")
    say(f"  legacy   DisturbanceModel.draw, {Bl} vehicles timed, x {B // Bl}: {stat(t['legacy'], 1.0, 's ')}")
    say(f"  counter  DisturbanceModel.draw_counter           : {stat(t['counter'], 1.0, 's ')}")
    say(f"  table    DeviceClosedLoop.disturbance_table      : {stat(t['table'], 1.0, 's ')}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
