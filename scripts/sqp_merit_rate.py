"""
scripts/sqp_merit_rate.py -- full SQP solves (nlp_solver_type SQP) on config 2 (4096 x N = 40, cold start, one GPU) under both
globalizations, FIXED_STEP and MERIT_BACKTRACKING, interleaved in one process (sibling of scripts/sqp_rate.py, whose figures the
FIXED_STEP leg repeats).

Reports per globalization: converged / capped / failed instances, the median QPs of the converged, ms per SQP solve and per SQP
iteration (wall time of a solve over the iterations it ran, i.e. the largest sqp_iter), the same with every instance active
(tolerances 0, --k iterations: the per-iteration cost without early stops), and for the line search the share of damped steps.
The kernel-trace time of sqp_merit_kernel comes from a run of this script under rocprofv3 --kernel-trace --stats with --reps 1.

    python scripts/sqp_merit_rate.py [--batch 4096] [--reps 5] [--max-iter 100] [--k 20] [--no-qp-warm-start] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 40
GLOBS = ("FIXED_STEP", "MERIT_BACKTRACKING")
ZERO = dict(nlp_solver_tol_stat=0.0, nlp_solver_tol_eq=0.0, nlp_solver_tol_ineq=0.0, nlp_solver_tol_comp=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--no-qp-warm-start", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tum_control_amd.solver import BatchedOcpSolver
    from tum_control_amd.workloads import nominal_batch
    torch.zeros(1, device="cuda:0")
    B = a.batch
    x0, yref = nominal_batch(B, N=N)
    warm = False if a.no_qp_warm_start else None

    def mk(**kw):
        s = BatchedOcpSolver(N=N, dt=0.08, nsub=3, batch=B, nlp_solver_type="SQP", qp_warm_start=warm, **kw)
        s.install_reference_ocp()
        s.set_x0(x0); s.set_yref_all(yref)
        return s

    def timed(solvers, reps):
        """median wall ms of a cold-started solve per solver, the solvers taking turns (the first round: warm-up, allocation)"""
        ts = {g: [] for g in solvers}
        for _ in range(reps + 1):
            for g, s in solvers.items():
                s.cold_start(); s.synchronize()
                t = time.perf_counter(); s.solve(); ts[g].append(time.perf_counter() - t)
        return {g: float(np.median(v[1:])) * 1e3 for g, v in ts.items()}

    full = {g: mk(nlp_solver_max_iter=a.max_iter, globalization=g) for g in GLOBS}
    ms = timed(full, a.reps)
    active = {g: mk(nlp_solver_max_iter=a.k, globalization=g, **ZERO) for g in GLOBS}
    ms_k = timed(active, a.reps)
    res = dict(batch=B, N=N, max_iter=a.max_iter, qp_warm_start=not a.no_qp_warm_start, k_iterations=a.k)
    for g in GLOBS:
        s = full[g]
        it, st = s.get_stats("sqp_iter"), s.get_stats("status")
        n_it = int(it.max())
        r = dict(converged=int((st == 0).sum()), capped=int((st == 2).sum()), failed=int((st == 4).sum()),
                 median_qps_of_converged=float(np.median(it[st == 0])) if (st == 0).any() else None,
                 ms_per_sqp_solve=ms[g], sqp_iterations_run=n_it, ms_per_sqp_iteration=ms[g] / max(n_it, 1),
                 ms_per_sqp_iteration_all_active=ms_k[g] / a.k, sqp_solves_per_s=B / (ms[g] * 1e-3))
        if g == "MERIT_BACKTRACKING":
            al = s.get_alpha()
            done = (np.arange(al.shape[1])[None, :] < it[:, None]) & (al > 0)
            r.update(steps=int(done.sum()), damped_steps=int((al[done] < 1.0).sum()), steps_at_smallest_candidate=int((al[done] == al[done].min()).sum()),
                     smallest_alpha=float(al[done].min()))
        res[g] = r
    res["merit_over_fixed_per_iteration_all_active"] = res[GLOBS[1]]["ms_per_sqp_iteration_all_active"] / res[GLOBS[0]]["ms_per_sqp_iteration_all_active"]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
