"""
make_bo_golden.py -- records the reference's logged Bayesian-optimisation campaign as a test fixture.

    python tests/golden/make_bo_golden.py <reference checkout>

reads <reference checkout>/Learning_To_Adapt/SafeRL_WMPC/_logs/F/F.csv (one trial per line: natural parameters; normalised
parameters; objectives of group 0; objectives of group 1; feasible -- BO_WMPC/dataclasses.py Trial.to_csv) and writes
tests/golden/bo_trials_F.npz: params_nat (n x 7), params_nor (n x 7), objectives (n x 2 x 2, NaN where infeasible), feasible (n).
Recorded results only; run by hand where the reference is checked out, never by a test.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    path = os.path.join(ref, "Learning_To_Adapt", "SafeRL_WMPC", "_logs", "F", "F.csv")
    nat, nor, obj, feas = [], [], [], []
    with open(path) as f:
        for line in f:
            parts = line.strip().split(";")
            if len(parts) != 5:
                continue
            nat.append([float(e) for e in parts[0].split(",")])
            nor.append([float(e) for e in parts[1].split(",")])
            obj.append([[float(e) for e in parts[2].split(",")], [float(e) for e in parts[3].split(",")]])
            feas.append(bool(int(parts[4])))
    nat, nor, obj, feas = np.array(nat), np.array(nor), np.array(obj), np.array(feas)
    assert nat.shape[1] == 7 and nor.shape == nat.shape and obj.shape == (len(nat), 2, 2)
    assert np.isnan(obj[~feas]).all() and np.isfinite(obj[feas]).all()
    out = os.path.join(HERE, "bo_trials_F.npz")
    np.savez_compressed(out, params_nat=nat, params_nor=nor, objectives=obj, feasible=feas)
    print(f"{out}: {len(nat)} trials, {int(feas.sum())} feasible, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
