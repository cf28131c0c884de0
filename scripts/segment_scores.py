"""
segment_scores.py -- what scoring track segments on the device buys over scoring logs on the host (profiles/segment_scores.txt).

Workload: 26 weight sets (tests/golden/closed_loop_monteblanco_150.npz) x 8 segments of Monteblanco = 208 closed loops, N = 38,
every segment's end about `--seconds` of race-line travel time after its start. Two paths on the same build, interleaved:
  (a) DeviceClosedLoop.run_segments + segment_groups              (scores kept on the device, early stop)
  (b) run(max_steps) with log_capacity = max_steps, logs(), closed_loop.segment_scores_from_logs + segment_objectives
Every repetition is a whole evaluation of the 26 candidates: weights, start states, loop, objectives. Wall times end in a device
synchronise (both paths read results back). Also: the time per control step of the same loop with and without the extra kernel.

    python scripts/segment_scores.py [--reps 6] [--max-steps 500] [--seconds 6.0] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--max-steps", type=int, default=500)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd import closed_loop as clm
    from tum_control_amd.planner import load_track

    P = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop_monteblanco_150.npz"))["params"]
    track = load_track("monteblanco")
    n = len(track)
    seg_starts = (np.arange(8) * (n // 8)).astype(np.int64)
    # end of a segment: the waypoint reached after `seconds` at the race line's own speeds
    dt = np.hypot(*(np.roll(track[:, :2], -1, axis=0) - track[:, :2]).T) / np.roll(track[:, 3], -1)
    ends = []
    for s0 in seg_starts:
        t, i = 0.0, int(s0)
        while t < a.seconds:
            t += dt[i % n]; i += 1
        ends.append(i % n)
    ends = np.array(ends)
    S, C = len(seg_starts), len(P)
    B = S * C
    params = np.repeat(P, S, axis=0)
    starts, end_idx = np.tile(seg_starts, C), np.tile(ends, C)
    offsets = np.arange(C * S + 1)[::4]          # groups of four segments: two per candidate
    sizes = [4, 4]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    say(f"# scripts/segment_scores.py --reps {a.reps} --max-steps {a.max_steps} --seconds {a.seconds}")
    say(f"# {C} weight sets x {S} segments of monteblanco = {B} loops, N = 38; segment starts {seg_starts.tolist()}, ends {ends.tolist()}")
    torch.zeros(1, device="cuda:0")
    f0 = free()
    la = clm.ClosedLoopBatch("monteblanco", batch=B, params=params, N=38, Tp=3.04, idx_start=starts, on_device=True, log_capacity=0)
    f1 = free()
    la.dev.attach_segments(end_idx, np.inf, np.inf, group_offsets=offsets)
    f2 = free()
    lb = clm.ClosedLoopBatch("monteblanco", batch=B, params=params, N=38, Tp=3.04, idx_start=starts, on_device=True, log_capacity=a.max_steps)
    f3 = free()
    seg_bytes = B * (4 * 4 + 3 * 8) + (len(offsets) + 4 * (len(offsets) - 1) + 48) * 8
    log_bytes = 8 * B * ((a.max_steps + 1) * 15 + a.max_steps * 11)
    say(f"device memory (free memory before - after, allocation granularity included): loop without logs {(f0 - f1) / 2**20:.1f} MiB, "
        f"+ segments {(f1 - f2) / 2**20:.3f} MiB (buffers: {seg_bytes} B), loop with log_capacity {a.max_steps}: {(f2 - f3) / 2**20:.1f} MiB "
        f"(logs: {log_bytes / 2**20:.1f} MiB = 26 doubles per instance and step)")

    def eval_a():
        la.set_weights(params)
        la.dev.set_state(la.x_sim, la.x_mpc, cold_start=True)
        la.dev.run_segments(a.max_steps, 100)
        obj, feas = clm._objectives_from_groups(la.dev.segment_groups().reshape(C, len(sizes), 4))
        return obj, feas, la.dev.steps

    def eval_b():
        t0 = time.perf_counter()
        lb.set_weights(params)
        lb.dev.set_state(lb.x_sim, lb.x_mpc, cold_start=True)
        lb.dev.run(a.max_steps)
        t1 = time.perf_counter()
        logs = lb.dev.logs()
        t2 = time.perf_counter()
        seg = clm.segment_scores_from_logs(logs, lb.track, end_idx, np.inf, np.inf, lb.cfg)
        obj, feas = clm.segment_objectives(seg, C, sizes)
        t3 = time.perf_counter()
        return obj, feas, (t1 - t0, t2 - t1, t3 - t2)

    ta, tb, parts = [], [], []
    for r in range(a.reps + 1):          # (repetition 0 warms both paths up: graph capture, code objects)
        t0 = time.perf_counter(); oa, fa, steps_a = eval_a(); t1 = time.perf_counter()
        ob, fb, pt = eval_b(); t2 = time.perf_counter()
        if r:
            ta.append(t1 - t0); tb.append(t2 - t1); parts.append(pt)
    err = np.nanmax(np.abs(oa - ob)) if fa.any() else float("nan")
    say(f"same evaluation: feasible {int(fa.sum())}/{C} (a), {int(fb.sum())}/{C} (b), equal {bool((fa == fb).all())}; "
        f"largest objective difference {err:.3e}; (a) stopped after {steps_a} of {a.max_steps} steps")

    def stat(v):
        v = np.asarray(v) * 1e3
        return f"median {np.median(v):8.2f} ms  range {v.min():8.2f} .. {v.max():8.2f}  (n = {len(v)})"
    say(f"(a) run_segments + segment_groups          : {stat(ta)}")
    say(f"(b) run + logs + host scoring              : {stat(tb)}")
    parts = np.array(parts)
    say(f"    of (b): loop {stat(parts[:, 0])}")
    say(f"            logs() copy {stat(parts[:, 1])}")
    say(f"            host scoring {stat(parts[:, 2])}")
    # per-step cost of the extra kernel: the same loop, attached / detached, interleaved
    K = a.max_steps
    att, det = [], []
    for r in range(a.reps + 1):
        for which in ("att", "det"):
            if which == "att":
                la.dev.attach_segments(end_idx, np.inf, np.inf, group_offsets=offsets)
            else:
                la.dev.detach_segments()
            la.dev.set_state(la.x_sim, la.x_mpc, cold_start=True)
            la.dev.run(50)          # (captures the chunk again)
            t0 = time.perf_counter(); la.dev.run(K); t1 = time.perf_counter()
            if r:
                (att if which == "att" else det).append((t1 - t0) / K)
    us = lambda v: f"median {np.median(v) * 1e6:7.2f} us  range {min(v) * 1e6:7.2f} .. {max(v) * 1e6:7.2f}"
    say(f"time per control step, {B} loops, run({K}): attached {us(att)}; detached {us(det)}; "
        f"difference of the medians {(np.median(att) - np.median(det)) * 1e6:+.2f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
