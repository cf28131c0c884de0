"""
make_gp_golden.py -- the long-double truth of the two class GPs of the logged campaign at its full size, as a test fixture.

    python tests/golden/make_gp_golden.py

reads tests/golden/bo_trials_F.npz (2050 trials, d = 7) and writes tests/golden/gp_campaign.npz. Per class k = 0, 1 of the Dirichlet
classification (targets and fixed noise of bo.dirichlet_targets, noise floor 1e-6, a learned noise) and per hyperparameter vector
t = 0 (the theta bo.ConstraintModel starts fit_gp at) and t = 1 (the theta bo.fit_gp on the CPU, torch, max_iter=50, ends at) it
stores, from one Cholesky and one forward substitution of tests/gp_reference.py solve in np.longdouble:

    theta_k_t                          the d + 3 hyperparameters (data: the tests read them from here)
    mll_k_t, grad_k_t                  the marginal log-likelihood and its d + 3 gradient components
    scale_k_t                          scale_mll, scale_grad
    a_k_t                              A^-1 (y - c)
    V_k_t                              the rows ROWS of V = L^-1
    vmax_k_t                           the largest |entry| of V (the scale of the factor's gate)

Every long double is kept as two float64 arrays <name>_hi = float64(x) and <name>_lo = float64(x - hi); gp_reference.join gives x
back exactly. Numbers only. The four (class, theta) entries run in four processes, about three minutes each; run by hand, never by a
test.
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gp_reference as gref         # noqa: E402

ROWS = (63, 64, 1023, 1024, 2047, 2048, 2049)
FLOOR = 1e-6
MAX_ITER = 50


def data():
    from tum_control_amd import bo
    z = np.load(os.path.join(HERE, "bo_trials_F.npz"))
    Xn, feas = z["params_nor"], z["feasible"]
    targets, fixed = bo.dirichlet_targets(feas)
    return Xn, targets, fixed


def thetas(k):
    """(initial theta, fitted theta) of class k."""
    from tum_control_amd import bo
    Xn, targets, fixed = data()
    d = Xn.shape[1]
    init = bo.GPHyper(c=1.0, s=max(float(np.var(targets[:, k])), 1.0), ls=np.full(d, 0.5), noise=1e-2)
    th0 = np.concatenate([np.log(init.ls), [np.log(init.s), init.c, np.log(init.noise)]])
    h = bo.fit_gp(Xn, targets[:, k], fixed_noise=fixed[:, k], init=init, max_iter=MAX_ITER, noise_floor=FLOOR)
    th1 = np.concatenate([np.log(h.ls), [np.log(h.s), h.c, np.log(h.noise - FLOOR)]])
    return th0, th1


def entry(job):
    k, t, theta = job
    Xn, targets, fixed = data()
    mll, grad, s_mll, s_grad, V, a = gref.solve(Xn, targets[:, k], theta, fixed[:, k], True, FLOOR)
    out = {f"theta_{k}_{t}": theta, f"scale_{k}_{t}": np.array([s_mll, s_grad]), f"vmax_{k}_{t}": np.array(float(np.abs(V).max()))}
    for name, x in (("mll", mll), ("grad", grad), ("a", a), ("V", V[list(ROWS)])):
        out[f"{name}_{k}_{t}_hi"], out[f"{name}_{k}_{t}_lo"] = gref.split(x)
    print(f"class {k} theta {t}: mll {float(mll)!r} scale_mll {s_mll:.6e} scale_grad {s_grad:.6e}", flush=True)
    return out


def main():
    import torch
    torch.set_num_threads(4)
    jobs = []
    for k in range(2):
        th0, th1 = thetas(k)
        print(f"class {k}: theta0 {th0.tolist()}\n         theta1 {th1.tolist()}", flush=True)
        jobs += [(k, 0, th0), (k, 1, th1)]
    with multiprocessing.get_context("spawn").Pool(4) as pool:
        parts = pool.map(entry, jobs)
    out = {"rows": np.array(ROWS), "noise_floor": np.array(FLOOR)}
    for p in parts:
        out.update(p)
    path = os.path.join(HERE, "gp_campaign.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
