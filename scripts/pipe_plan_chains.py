#!/usr/bin/env python3
"""Which kernels a solve launches, capsule by capsule: one capsule per branch of plan_pipeline (csrc/pipe_plan.hpp), at the smallest
shape that reaches the branch -- the named cases of tests/host/pipe_plan_check.cpp, on the GPU.

    pipe_plan_chains.py run <out dir>
        every capsule in turn: cold start and two solves (an SQP solve, a prepare + feedback pair, the instrumented solve and two
        closed loops of 60 steps among them); X, U, cost and status of each go to <out dir>/<capsule>.npz. Run under
        `rocprofv3 --kernel-trace` the trace holds the kernels of capsule i between the i-th and the (i + 1)-th fill kernel of torch
        (the one torch kernel this script launches, as a separator).
    pipe_plan_chains.py compare <out dir A> <trace dir A> <out dir B> <trace dir B>
        per capsule: the ordered kernel names of A, whether B's are the same, and whether every array of B equals A's bit for bit.
        Exit code 1 where anything differs. (The closed loop with the linearisation forked onto a second stream is compared as a
        multiset: two streams have no order.)

scripts/pipe_plan_chains.sh runs both libraries (the working tree's and a saved build through TUM_NMPC_LIB) and writes the report.
"""
import collections
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.08


def _nominal(N, B, uniform=True, **kw):
    from tum_control_amd.solver import BatchedOcpSolver
    from tum_control_amd.workloads import nominal_batch
    x0, yref = nominal_batch(B, N=N)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B, **kw)
    s.install_reference_ocp()
    s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
    if not uniform:
        s.set(3, "x", x0 + 1e-3)          # (a writer of the iterate: the general linearisation)
    return s


def _keep_records():
    s = _nominal(40, 4096)
    s.options_set("uniform_records", 1)
    return s


def _full_w(N, B, uniform):
    s = _nominal(N, B, uniform)
    W = np.diag([1.0, 1.0, 2.0, 0.5, 0.05, 0.05]) * 0.01
    W[0, 1] = W[1, 0] = 2e-3; W[2, 3] = W[3, 2] = -1e-3
    for k in range(N):
        s.cost_set(k, "W", W)
    s.cost_set(N, "W", W[:4, :4])
    return s


def _snmpc(N, B, uph):
    from tum_control_amd import config, snmpc as snm
    from tum_control_amd.solver import CoupledSnmpcSolver
    from tum_control_amd.workloads import nominal_batch
    w = snm.hammersley_normal(10, 3)
    A = snm.pce_matrix(w, snm.alpha_generation(3, 2))
    offs = snm.x0_offsets(w, np.asarray(config.MPC["stds"], dtype=float))
    x0, yref = nominal_batch(B, N=N)
    s = CoupledSnmpcSolver(N=N, dt=DT, batch=B, Apce=A, uph=uph, gamma=config.MPC["gamma"], x0_offsets=offs)
    s.install_reference_ocp()
    s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
    return s


def _two_solves(s):
    s.solve(); s.solve()


def _split(s):
    s.prepare(); s.feedback(); s.prepare(); s.feedback()


def _instrumented(s):
    s.profile_phases(); s.profile_phases()


def _results(s):
    X, U = s.get_iterate()
    return dict(X=X, U=U, cost=np.atleast_1d(s.get_cost()), status=s.get_stats("status"))


def _loop(kernel):
    def run():
        from tum_control_amd.closed_loop import ClosedLoopBatch
        cl = ClosedLoopBatch("monteblanco", batch=26, on_device=True, log_capacity=60)
        if kernel:
            cl.solver.set_kernel(kernel)
        logs = cl.run(60)
        return dict(logs, status=cl.solver.get_stats("status"), cost=np.atleast_1d(cl.solver.get_cost()))
    return run


def _case(make, solve=_two_solves):
    def run():
        s = make()
        solve(s)
        return _results(s)
    return run


CAPSULES = [
    ("4096x40_uniform", _case(lambda: _nominal(40, 4096))),
    ("4096x40_uniform_records_1", _case(_keep_records)),
    ("4096x40_not_uniform", _case(lambda: _nominal(40, 4096, uniform=False))),
    ("4096x40_uniform_store_qp_in", _case(lambda: _nominal(40, 4096, store_qp_in=True))),
    ("4096x40_uniform_prepare_feedback", _case(lambda: _nominal(40, 4096), _split)),
    ("4096x40_uniform_sqp_3", _case(lambda: _nominal(40, 4096, nlp_solver_type="SQP", nlp_solver_max_iter=3), lambda s: s.solve())),
    ("26x40_uniform", _case(lambda: _nominal(40, 26))),
    ("26x40_not_uniform", _case(lambda: _nominal(40, 26, uniform=False))),
    ("199x40_not_uniform", _case(lambda: _nominal(40, 199, uniform=False))),
    ("200x40_not_uniform", _case(lambda: _nominal(40, 200, uniform=False))),
    ("512x40_uniform", _case(lambda: _nominal(40, 512))),
    ("1025x40_uniform", _case(lambda: _nominal(40, 1025))),
    ("26x40_prof", _case(lambda: _nominal(40, 26, uniform=False), _instrumented)),
    ("4096x40_full_w", _case(lambda: _full_w(40, 4096, False))),
    ("4096x40_full_w_uniform", _case(lambda: _full_w(40, 4096, True))),
    ("26x50", _case(lambda: _nominal(50, 26, uniform=False))),
    ("4096x50_uniform", _case(lambda: _nominal(50, 4096))),
    ("sn_4096x38_uph5", _case(lambda: _snmpc(38, 4096, 5))),
    ("sn_4096x38_uph38", _case(lambda: _snmpc(38, 4096, 38))),
    ("sn_26x38", _case(lambda: _snmpc(38, 26, 5))),
    ("loop_26_60_steps_captured", _loop(None)),
    ("loop_26_60_steps_fork", _loop("loop-fork")),          # (the linearisation ran ahead; two streams)
]


def run(out):
    import torch
    os.makedirs(out, exist_ok=True)
    mark = torch.empty(64, device="cuda:0")
    for i, (name, fn) in enumerate(CAPSULES):
        torch.cuda.synchronize(); mark.fill_(float(i)); torch.cuda.synchronize()
        np.savez(os.path.join(out, "%02d_%s.npz" % (i, name)), **fn())
        print("ran", i, name, flush=True)
    torch.cuda.synchronize()


def _chains(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    chains = []
    for _, k in sorted(rows):
        if "at::native" in k:
            chains.append([])
        elif chains:
            chains[-1].append(k.split("(")[0].replace("void ", "").replace("tum::", ""))
    return [c for c in chains if c]          # (torch may fill a tensor of its own before the first capsule)


def _runs(chain):
    """the chain with repetitions folded: `k x3`, `(a | b | c) x25`"""
    out, i = [], 0
    while i < len(chain):
        best = (1, 1)          # (period, repetitions) of what repeats longest from here
        for p in range(1, 9):
            r = 1
            while chain[i + r * p:i + (r + 1) * p] == chain[i:i + p]:
                r += 1
            if r > 1 and r * p > best[0] * best[1]:
                best = (p, r)
        p, r = best
        block = " | ".join(chain[i:i + p])
        out.append(block if r == 1 else ("%s x%d" % (block, r) if p == 1 else "(%s) x%d" % (block, r)))
        i += p * r
    return " | ".join(out)


def compare(out_a, trace_a, out_b, trace_b):
    ca, cb = _chains(trace_a), _chains(trace_b)
    bad = 0
    if not (len(ca) == len(cb) == len(CAPSULES)):
        print("separators found: %d and %d, capsules %d" % (len(ca), len(cb), len(CAPSULES)))
        return 1
    for i, (name, _) in enumerate(CAPSULES):
        a, b = ca[i], cb[i]
        same_k = (collections.Counter(a) == collections.Counter(b)) if name.endswith("_fork") else a == b
        fa, fb = (np.load(os.path.join(d, "%02d_%s.npz" % (i, name))) for d in (out_a, out_b))
        same_o = sorted(fa.files) == sorted(fb.files) and all(fa[k].shape == fb[k].shape and fa[k].tobytes() == fb[k].tobytes() for k in fa.files)
        print("%-34s %3d kernels: %s; outputs (%s): %s" % (name, len(a), "same chain" if same_k else "CHAIN DIFFERS", ", ".join(sorted(fa.files)),
                                                          "bit-identical" if same_o else "DIFFERENT"))
        print("    " + _runs(a))
        if not same_k:
            print("  B " + _runs(b))
        bad += (not same_k) + (not same_o)
    print("capsules %d, differences %d" % (len(CAPSULES), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
