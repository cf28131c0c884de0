"""
rti_split_latency.py -- what the split real-time iteration buys on the latency path and what it costs.

Per size (N x batch; default N = 40, 38 x 1, 26, 4096 instances): a one-call capsule and a split capsule (twins: same problem,
config 2, cold-started before every repetition) alternate in ONE process -- one-call solve, preparation, feedback -- after a
warm-up; medians and the 5 % / 95 % quantiles of get_stats("time_tot") (device time) of the three, the ratio feedback / one-call
and the price of the split (preparation + feedback against the one-call solve); then the host wall time of step() (x0 in, solve,
results out) on the one-call capsule against the feedback step() on the split one (its preparation outside the timed span).
(time_tot of a small capsule's synchronous solve / feedback is read from the device's wall clock by its first and last kernel; a
preparation, and every solve of a large capsule, is timed by events on the stream.)

    python scripts/rti_split_latency.py [--sizes 40x1,40x26,...] [--reps 200] [--warmup 20] [--no-wall] [--out FILE]

A kernel trace of its own gives the feedback kernel's time:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/rti_split_latency.py --sizes 40x26 --reps 50 --no-wall
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tum_control_amd.solver import BatchedOcpSolver  # noqa: E402
from tum_control_amd.workloads import nominal_batch  # noqa: E402


def q(a):
    a = np.asarray(a) * 1e3
    return f"{np.median(a):8.4f} ms [{np.quantile(a, 0.05):.4f} .. {np.quantile(a, 0.95):.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40x1,40x26,40x4096,38x1,38x26,38x4096")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-wall", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# split real-time iteration, config 2, cold-started problem; {a.reps} repetitions behind {a.warmup} warm-up, one process, alternated")
    for size in a.sizes.split(","):
        N, B = (int(v) for v in size.split("x"))
        x0, yref = nominal_batch(B, N=N)
        one, split = BatchedOcpSolver(N=N, batch=B), BatchedOcpSolver(N=N, batch=B)
        for s in (one, split):
            s.install_reference_ocp(); s.set_x0(x0); s.set_yref_all(yref)
        t_one, t_prep, t_fb = [], [], []
        for r in range(a.warmup + a.reps):
            one.cold_start(); split.cold_start()
            st = one.solve(); t1 = one.get_stats("time_tot")
            split.prepare(); t2 = split.get_stats("time_tot")
            assert split.feedback() == st; t3 = split.get_stats("time_tot")
            if r >= a.warmup:
                t_one.append(t1); t_prep.append(t2); t_fb.append(t3)
        Xa, Ua = one.get_iterate(); Xb, Ub = split.get_iterate()
        assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub)          # (same x0: the same solve, bit for bit)
        m1, m2, m3 = np.median(t_one), np.median(t_prep), np.median(t_fb)
        say(f"N={N} batch={B}: device time_tot   one-call {q(t_one)}   preparation {q(t_prep)}   feedback {q(t_fb)}")
        say(f"N={N} batch={B}: feedback / one-call = {m3 / m1:.3f}   (preparation + feedback) / one-call = {(m2 + m3) / m1:.3f}")
        if not a.no_wall:
            w_one, w_fb = [], []
            for r in range(a.warmup + a.reps):
                one.cold_start(); split.cold_start(); one.synchronize()
                t = time.perf_counter(); one.step(x0=x0); w1 = time.perf_counter() - t
                split.prepare()
                split.options_set("rti_phase", 2)
                t = time.perf_counter(); split.step(x0=x0); w2 = time.perf_counter() - t
                if r >= a.warmup:
                    w_one.append(w1); w_fb.append(w2)
            say(f"N={N} batch={B}: host wall of step()   one-call {q(w_one)}   feedback {q(w_fb)}   ratio {np.median(w_fb) / np.median(w_one):.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
