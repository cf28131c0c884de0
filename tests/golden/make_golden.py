#!/usr/bin/env python3
"""
tests/golden/make_golden.py -- regenerates the golden fixtures in this directory.

Runs ONLY in the build container (needs /root/reference, which never travels to the
GPU box). It imports the pure-numpy pieces of the reference with stub `casadi` /
`chaospy` modules and reads the reference's logged acados outputs; what it writes is
DATA (inputs + expected outputs), never reference source:

  kat0.npz            step 0 (cold start) of all 52 _baseline/F/{monteblanco,lvms}/{k}.npz
  replay_<t>_<k>_<a>_<b>.npz   sequential closed-loop windows (x0_i, yref_i, expected u0/x1/cost/qp_iter)
  replay_hard.npz     windows of the weight sets on which acados hit its 50-iteration QP cap (2, 13, 16, 18; both tracks):
                      x0_i, planner pose_i and the logged u0/x1/cost/qp_iter around the first capped solve of each loop
  planner.npz         PlannerEmulator input/output pairs
  pce.npz             alphaGeneration / polyChaosExpansion / compute_x0dist / sigma points of acados_ocp_SNMPC.json
  snmpc_expr.npz      stacked dynamics / cost output / chance constraint of the exported SNMPC OCP evaluated at random points
  snmpc_json.npz      dimensions, weights, penalties, bounds and solver options of the exported SNMPC OCP (acados_ocp_SNMPC.json)
  r2.npz              P_propagation input/output pairs
  disturbances.npz    the harness's disturbance set-up (initDisturbanceSim on the shipped sim_main_params.yaml) and seeded realisations of
                      generate_disturbances for every distribution type, in sim_step's draw order; LonLatDeviations / postprocess_yaw pairs
  closed_loop_<t>_<n>.npz   first n steps of the 26 logged closed loops of one track (plant states, inputs, predictions)
  closed_loop_<t>_full_sub<k>.npz   the complete 5499-step loops, every k-th plant state + per-loop statistics
  log_file_<t>_<k>.npz   one logged loop's _baseline/F/<t>/<k>.npz as Logger.save_logs wrote it (every key, full length)

Reference call sites reproduced by the replay protocol:
  get_baseline_performances.py:101-131 (loop), Utils/SimulationMode_main_class.py:106-156
  (sim_step / StateEstimation), Utils/MPC_sim_utils.py:137-194 (PlannerEmulator),
  Utils/Logging_Plotting.py:124-146,341-343 (what the logs hold; yaw is stored wrapped).
"""
import json
import re
import os
import sys
import types
from collections import deque

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

# --- stub the absent third-party modules so the reference's numpy code imports
for name in ("casadi", "chaospy", "matplotlib", "matplotlib.pyplot", "matplotlib.cm", "matplotlib.colors", "pylab"):
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
sys.modules["casadi"].__dict__.setdefault("__all__", [])
sys.path.insert(0, REF)

from Utils.MPC_sim_utils import PlannerEmulator, postprocess_yaw  # noqa: E402
from Utils.SimulationMode_main_class import moving_average_filter  # noqa: E402

BASE = os.path.join(REF, "Learning_To_Adapt/SafeRL_WMPC/_baseline/F")
F = np.loadtxt(os.path.join(REF, "Learning_To_Adapt/SafeRL_WMPC/_parameters/F.csv"), delimiter=",")
N, TP = 38, 3.04
WINDOWS = np.array([1, 1, 4, 2, 2, 3, 4, 2])


def load_traj(track):
    with open(os.path.join(REF, "Trajectories", f"reftraj_{track}_edgar.json")) as f:
        return json.load(f)


def yref_of(traj, pose):
    _, t = PlannerEmulator(traj, pose, N + 1, TP, True)
    return np.stack([np.asarray(t["pos_x"], float), np.asarray(t["pos_y"], float),
                     np.asarray(t["ref_yaw"], float), np.asarray(t["ref_v"], float)], axis=1)


def replay_inputs(track, k, nsteps):
    """(x0_i, yref_i, expected) for steps 0..nsteps-1 of one logged closed loop."""
    d = np.load(os.path.join(BASE, track, f"{k}.npz"))
    traj = load_traj(track)
    CiLX = d["CiLX"].copy()
    CiLX[:, 2] = np.unwrap(CiLX[:, 2])        # logs hold yaw mod 2pi, the live state is continuous
    SimX = d["MPC_SimX"]
    buf = [deque(maxlen=15) for _ in range(8)]
    x0s, yrefs = [], []
    X0 = np.array([traj["pos_x"][0], traj["pos_y"][0], postprocess_yaw(traj["ref_yaw"][0]), traj["ref_v"][0], 0, 0, 0, 0.0])
    for i in range(nsteps):
        if i == 0:
            x0 = X0.copy()
            pose = X0[:4].copy()
        else:
            xn = np.append(CiLX[i], SimX[i][7])
            for j in range(8):
                buf[j].append(xn[j])
                xn[j] = moving_average_filter(np.array(buf[j]), WINDOWS[j])
            x0 = xn
            pose = CiLX[i][:4]
        x0s.append(x0)
        yrefs.append(yref_of(traj, pose))
    exp = dict(u0=d["simU"][:nsteps], x1=SimX[1:nsteps + 1], cost=d["simSolverDebug"][:nsteps, 0],
               qp_iter=d["simSolverDebug"][:nsteps, 3], status=d["simSolverDebug"][:nsteps, 4])
    return np.array(x0s), np.array(yrefs), exp


def make_kat0():
    rows = []
    for track in ("monteblanco", "lvms"):
        for k in range(26):
            x0s, yrefs, exp = replay_inputs(track, k, 1)
            rows.append((track, k, x0s[0], yrefs[0], exp))
    np.savez_compressed(
        os.path.join(OUT, "kat0.npz"),
        track=np.array([r[0] for r in rows]), k=np.array([r[1] for r in rows]),
        params=np.array([F[r[1]] for r in rows]),
        x0=np.array([r[2] for r in rows]), yref=np.array([r[3] for r in rows]),
        u0=np.array([r[4]["u0"][0] for r in rows]), x1=np.array([r[4]["x1"][0] for r in rows]),
        cost=np.array([r[4]["cost"][0] for r in rows]), qp_iter=np.array([r[4]["qp_iter"][0] for r in rows]))


def make_replay(track, k, nsteps):
    x0s, yrefs, exp = replay_inputs(track, k, nsteps)
    np.savez_compressed(os.path.join(OUT, f"replay_{track}_{k}_0_{nsteps}.npz"),
                        params=F[k], x0=x0s, yref=yrefs, **exp)


# (track, weight set, first step, one-past-last step). Windows that start at 0 replay the log from its cold start; the
# lvms/2 window starts in the middle of the log (cold restart there: the first ~20 steps are warm-up).
HARD_WINDOWS = [("monteblanco", 2, 0, 380), ("monteblanco", 13, 0, 135), ("monteblanco", 16, 0, 290), ("monteblanco", 18, 0, 60),
                ("lvms", 2, 1195, 1295), ("lvms", 13, 0, 425), ("lvms", 16, 0, 450), ("lvms", 18, 0, 375)]


def make_replay_hard():
    """Per-solve pins on the weight sets whose logged closed loops contain QP solves that acados stopped at its iteration cap
    (qp_iter == 50, status still 0: `simSolverDebug[:, 3:5]`). Stored per step: the x0 the logged solve started from, the
    pose handed to the planner (yref is re-derived by the golden-pinned planner restatement), and what acados returned."""
    out = {}
    meta = []
    for track, k, a, b in HARD_WINDOWS:
        d = np.load(os.path.join(BASE, track, f"{k}.npz"))
        x0s, _, exp = replay_inputs(track, k, b)
        traj = load_traj(track)
        CiLX = d["CiLX"]
        pose = np.array([[traj["pos_x"][0], traj["pos_y"][0]] if i == 0 else CiLX[i][:2] for i in range(b)])
        key = f"{track}_{k}"
        out[key + "_x0"] = x0s[a:b]; out[key + "_pose"] = pose[a:b]
        for f in ("u0", "x1", "cost", "qp_iter"):
            out[key + "_" + f] = np.asarray(exp[f][a:b], dtype=np.float64)
        assert (exp["status"][a:b] == 0).all()
        meta.append((track, k, a, b))
    np.savez_compressed(os.path.join(OUT, "replay_hard.npz"), params=F, track=np.array([m[0] for m in meta]),
                        k=np.array([m[1] for m in meta]), start=np.array([m[2] for m in meta]), **out)


def make_closed_loop(track="monteblanco", nsteps=150):
    """First `nsteps` control steps of the 26 logged closed loops on one track (one per weight set of F.csv):
    what the plant, the inputs and the stage-1 predictions were. Yaw columns are stored as logged (mod 2pi)."""
    C, S, U = [], [], []
    for k in range(26):
        d = np.load(os.path.join(BASE, track, f"{k}.npz"))
        C.append(d["CiLX"][:nsteps + 1]); S.append(d["MPC_SimX"][:nsteps + 1]); U.append(d["simU"][:nsteps])
    np.savez_compressed(os.path.join(OUT, f"closed_loop_{track}_{nsteps}.npz"), params=F,
                        CiLX=np.array(C, dtype=np.float64), MPC_SimX=np.array(S), simU=np.array(U))


def make_closed_loop_full(track="monteblanco", sub=25):
    """The complete logged closed loops (5499 control steps, 26 weight sets), subsampled: plant state every `sub` steps,
    the inputs at those steps, and per-loop statistics of the solver (mean / max QP iterations, worst status, lap cost)."""
    C, U, st = [], [], []
    for k in range(26):
        d = np.load(os.path.join(BASE, track, f"{k}.npz"))
        C.append(d["CiLX"][::sub]); U.append(d["simU"][::sub])
        dbg = d["simSolverDebug"]
        st.append([dbg[:, 3].mean(), dbg[:, 3].max(), dbg[:, 4].max(), dbg[:, 0].mean(),
                   np.abs(d["dev_lat"]).max(), np.abs(d["dev_vel"]).max()])
    np.savez_compressed(os.path.join(OUT, f"closed_loop_{track}_full_sub{sub}.npz"), params=F, sub=sub,
                        CiLX=np.array(C), simU=np.array(U), stats=np.array(st))


def make_planner():
    rng = np.random.default_rng(7)
    out = {}
    for track in ("monteblanco", "lvms", "modena"):
        traj = load_traj(track)
        n = len(traj["pos_x"])
        idx = np.concatenate([np.arange(0, n, 53), [n - 1, n - 2, n - 5, n - 12, n - 25]])
        poses = np.stack([np.asarray(traj["pos_x"])[idx], np.asarray(traj["pos_y"])[idx]], 1) + rng.normal(0, 0.7, (len(idx), 2))
        res39, res41, cidx = [], [], []
        for p in poses:
            c, t = PlannerEmulator(traj, p, 39, 3.04, True)
            res39.append(np.stack([t["pos_x"], t["pos_y"], t["ref_yaw"], t["ref_v"]], 1))
            c2, t2 = PlannerEmulator(traj, p, 41, 3.2, True)
            res41.append(np.stack([t2["pos_x"], t2["pos_y"], t2["ref_yaw"], t2["ref_v"]], 1))
            cidx.append(c)
        out[f"{track}_pose"] = poses
        out[f"{track}_idx"] = np.array(cidx)
        out[f"{track}_n39"] = np.array(res39)
        out[f"{track}_n41"] = np.array(res41)
    np.savez_compressed(os.path.join(OUT, "planner.npz"), **out)


def make_pce():
    from Model_Predictive_Controller.Stochastic_NMPC.stochastic_mpc_utils import (
        alphaGeneration, polyChaosExpansion, compute_x0dist, hermiteGeneration)
    alphas = alphaGeneration(3, 2)
    rng = np.random.default_rng(3)
    w = rng.normal(size=(3, 15))
    phi = np.array([polyChaosExpansion(w[:, i], alphas, "gaussian") for i in range(15)])
    herm = np.array([[hermiteGeneration(x, n) for n in range(4)] for x in (-1.3, 0.0, 0.4, 2.2)])
    x0 = np.array([1.0, 2.0, 0.3, 20.0, 0.1, 0.02, 0.01, 0.5])
    stds = np.array([0, 0, 0, 0.8, 0.35, 0.035, 0, 0])
    x0d = compute_x0dist(x0.copy(), w, 15, stds)
    with open(os.path.join(REF, "acados_ocp_SNMPC.json")) as f:
        js = json.load(f)
    lbx0 = np.array(js["constraints"]["lbx_0"], float).reshape(11, 8)
    np.savez_compressed(os.path.join(OUT, "pce.npz"), alphas=alphas, w=w, phi=phi, herm=herm,
                        x0=x0, stds=stds, x0dist=x0d, json_lbx0=lbx0)


def make_snmpc_json():
    """Problem data of the exported SNMPC OCP (acados_ocp_SNMPC.json): dimensions, weights, slack penalties, bounds and the
    solver options the coupled solver has to agree with. Data only."""
    with open(os.path.join(REF, "acados_ocp_SNMPC.json")) as f:
        js = json.load(f)
    d, c, k, so = js["dims"], js["cost"], js["constraints"], js["solver_options"]
    dims = {q: int(d[q]) for q in ("N", "nx", "nu", "np", "nh", "nh_0", "nh_e", "ns", "ns_0", "ns_e", "nbx", "nbu", "nbx_0", "nbx_e",
                                   "nsbx", "nsbu", "nsh", "nsh_e", "nsbx_e", "ny", "ny_e")}
    opts = {q: so[q] for q in ("integrator_type", "nlp_solver_type", "qp_solver", "hessian_approx", "qp_solver_iter_max",
                               "qp_solver_warm_start", "nlp_solver_step_length", "tf", "levenberg_marquardt", "regularize_method",
                               "hpipm_mode")}
    np.savez_compressed(os.path.join(OUT, "snmpc_json.npz"),
                        dims=json.dumps(dims), opts=json.dumps(opts),
                        W=np.array(c["W"], float), W_e=np.array(c["W_e"], float),
                        Zl=np.array(c["Zl"], float), Zu=np.array(c["Zu"], float), zl=np.array(c["zl"], float), zu=np.array(c["zu"], float),
                        Zl_0=np.array(c["Zl_0"], float), zl_0=np.array(c["zl_0"], float), Zl_e=np.array(c["Zl_e"], float), zl_e=np.array(c["zl_e"], float),
                        lbx=np.array(k["lbx"], float), ubx=np.array(k["ubx"], float), lbu=np.array(k["lbu"], float), ubu=np.array(k["ubu"], float),
                        lh=np.array(k["lh"], float), uh=np.array(k["uh"], float), lh_e=np.array(k["lh_e"], float), uh_e=np.array(k["uh_e"], float),
                        lbx_e=np.array(k["lbx_e"], float), ubx_e=np.array(k["ubx_e"], float),
                        idxbx=np.array(k["idxbx"], int), idxbu=np.array(k["idxbu"], int), idxbx_e=np.array(k["idxbx_e"], int),
                        cost_type=c["cost_type"], cost_type_e=c["cost_type_e"], n_param=len(js["parameter_values"]))


def make_snmpc_expr(n=48):
    """The model functions of the exported SNMPC OCP evaluated at random points: acados_ocp_SNMPC.json carries the CasADi
    expressions of the stacked discrete dynamics, the cost output and the chance constraint as text; casadi_expr.py
    evaluates them numerically (gg tables from Config/EDGAR/ggv.csv). Stored: inputs (x 88, u 2, A_pce 10x10, stop_flag) and
    outputs (f_disc 88, y 6, y_e 4, h). The printed constants have 6 significant digits."""
    import csv
    import casadi_expr as ce
    with open(os.path.join(REF, "acados_ocp_SNMPC.json")) as f:
        js = json.load(f)
    model = js["model"]
    xnames = [t.strip() for t in re.match(r"vertcat\((.*)\)$", model["x"]).group(1).split(",")]
    ns, L = len(xnames) // 8 - 1, 10
    with open(os.path.join(REF, "Config", "EDGAR", "ggv.csv")) as f:
        rows = list(csv.DictReader(f))
    gv = np.array([float(r["vel_max_mps"]) for r in rows]); gax = np.array([float(r["ax_max_mps2"]) for r in rows])
    gay = np.array([float(r["ay_max_mps2"]) for r in rows])
    progs = {k: ce.parse_program(model[k]) for k in ("disc_dyn_expr", "cost_y_expr", "cost_y_expr_e", "con_h_expr")}
    ddefs = progs["disc_dyn_expr"][0]
    xdot_id = [k for k, a in ddefs.items() if a[0] == "call" and a[1] == "vertcat" and len(a[2]) == 8 and a[2][-1] == ("id", "jerk")][0]

    def reshape(arg_ast, val):
        val = np.asarray(val, dtype=float)
        if arg_ast == ("id", "A_pce"):
            return val.reshape((ns, L), order="F")            # reshape(A_pce, n_samples, num_poly_terms)
        return val.reshape((8, ns), order="F")                 # reshape(f_disc, 8, n_samples)

    def ode(ev, X, U):
        env = dict(ev.env)
        for i, nm in enumerate(xnames[:8]):
            env[nm] = float(X[i])
        env["jerk"], env["steering_rate"] = float(U[0]), float(U[1])
        return ev.child(env).ev(("tmp", xdot_id))

    funcs = {"f": ode,
             "ax_max_interpolant": lambda ev, v: float(np.interp(v, gv, gax)),
             "ay_max_interpolant": lambda ev, v: float(np.interp(v, gv, gay))}
    rng = np.random.default_rng(2024)
    from Model_Predictive_Controller.Stochastic_NMPC.stochastic_mpc_utils import alphaGeneration, polyChaosExpansion
    X = np.zeros((n, 8 * (ns + 1))); U = np.zeros((n, 2)); A = np.zeros((n, L, ns)); stop = np.zeros(n)
    F = np.zeros((n, 8 * (ns + 1))); Y = np.zeros((n, 6)); Ye = np.zeros((n, 4)); H = np.zeros(n)
    for j in range(n):
        base = np.array([rng.uniform(-200, 200), rng.uniform(-200, 200), rng.uniform(-7, 7), rng.uniform(5, 40) if j % 3 else rng.uniform(9, 13),
                         rng.uniform(-1.5, 1.5), rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2), rng.uniform(-3, 3)])
        xs = np.tile(base, (ns + 1, 1)); xs[1:] += rng.normal(0, 1, (ns, 8)) * np.array([1, 1, .05, .8, .35, .035, .01, .3])
        if j % 4 == 0:
            xs[:, 3] = np.abs(xs[:, 3]) * 1e-4                 # the vlong <= 0.001 branch of the slip angles
        a = rng.normal(0, 0.3, (L, ns)); a[0] = np.abs(a[0]) + 0.05; a[0] /= a[0].sum()
        X[j] = xs.reshape(-1); U[j] = [rng.uniform(-5, 5), rng.uniform(-0.3, 0.3)]; A[j] = a; stop[j] = float(j % 2)
        env = {nm: float(X[j, i]) for i, nm in enumerate(xnames)}
        env.update(jerk=float(U[j, 0]), steering_rate=float(U[j, 1]), A_pce=a.reshape(-1), risk_parameter=0.8, stop_flag=stop[j])
        F[j] = ce.Evaluator(progs["disc_dyn_expr"][0], env, funcs, reshape).ev(progs["disc_dyn_expr"][1])
        Y[j] = ce.Evaluator(progs["cost_y_expr"][0], env, funcs, reshape).ev(progs["cost_y_expr"][1])
        Ye[j] = ce.Evaluator(progs["cost_y_expr_e"][0], env, funcs, reshape).ev(progs["cost_y_expr_e"][1])
        H[j] = ce.Evaluator(progs["con_h_expr"][0], env, funcs, reshape).ev(progs["con_h_expr"][1])
    np.savez_compressed(os.path.join(OUT, "snmpc_expr.npz"), X=X, U=U, A=A, stop=stop, F=F, Y=Y, Ye=Ye, H=H, Ts=0.08, gamma=0.8)


def make_r2():
    from Model_Predictive_Controller.Reduced_Robustified_NMPC.Robust_NMPC_pred_model_utils import P_propagation
    rng = np.random.default_rng(11)
    P = rng.normal(size=(6, 8, 8)); P = P @ P.transpose(0, 2, 1)
    A = rng.normal(size=(6, 8, 8)); B = rng.normal(size=(6, 8, 4)); W = np.diag([0.1, 0.2, 0.3, 0.4])
    Pn = np.array([P_propagation(P[i], A[i], B[i], W) for i in range(6)])
    np.savez_compressed(os.path.join(OUT, "r2.npz"), P=P, A=A, B=B, W=W, Pn=Pn)


def make_disturbances():
    """Utils/MPC_sim_utils.py:15-99 (initDisturbanceSim, generate_disturbances, sampleFromEllipsoid) and :103-134 (LonLatDeviations,
    postprocess_yaw) on the shipped Config/EDGAR/sim_main_params.yaml, with numpy's global generator seeded: what
    tum_control_amd.closed_loop.DisturbanceModel / generate_disturbances / lon_lat_deviations / wrap_yaw must reproduce."""
    import yaml
    from Utils.MPC_sim_utils import LonLatDeviations, generate_disturbances, initDisturbanceSim
    with open(os.path.join(REF, "Config/EDGAR/sim_main_params.yaml")) as f:
        p = yaml.safe_load(f)
    p = dict(p, simulate_disturbances=True, simulate_state_estimation=True, disturbance_playback=False)
    (_, _, _, bd, be, types, _, _) = initDisturbanceSim(p, "", 10, 7)
    out = dict(bounds_derivatives=np.array(bd, float), bounds_state_estimation=np.array(be, float), types=np.array(types))
    for kind in ("uniform", "gaussian", "absolute", "box"):
        np.random.seed(7)
        out[f"deriv_{kind}"] = np.array([np.array(generate_disturbances(bd, kind), float) for _ in range(5)])
        np.random.seed(8)
        out[f"est_{kind}"] = np.array([np.array(generate_disturbances(be, kind), float) for _ in range(5)])
    # one run in sim_step's order (SimulationMode_main_class.py:121-143): per control step the derivative draw, then the estimation draw
    np.random.seed(3)
    W, E = [], []
    for _ in range(6):
        W.append(np.array(generate_disturbances(bd, types[0]), float)); E.append(np.array(generate_disturbances(be, types[1]), float))
    out["run_w"], out["run_e"] = np.array(W), np.array(E)
    rng = np.random.default_rng(12)
    yaw = rng.uniform(-7, 7, 20); ex, ey, rx, ry = rng.normal(size=(4, 20)) * 30
    dl, dt_ = LonLatDeviations(yaw, ex, ey, rx, ry)
    out.update(dev_in=np.stack([yaw, ex, ey, rx, ry]), dev_long=dl, dev_lat=dt_, wrapped=postprocess_yaw(yaw.copy()))
    np.savez_compressed(os.path.join(OUT, "disturbances.npz"), **out)


def make_log_file(track="lvms", k=3):
    """Utils/Logging_Plotting.py:321-395: the file Logger.save_logs wrote for one logged loop, every array as stored (the five raw
    logs and the channels derived from them): what tum_control_amd.closed_loop.log_file_arrays must reproduce."""
    with np.load(os.path.join(BASE, track, f"{k}.npz")) as r:
        np.savez_compressed(os.path.join(OUT, f"log_file_{track}_{k}.npz"), **{key: r[key] for key in r.files})


if __name__ == "__main__":
    what = sys.argv[1:] or ["kat0", "replay", "replay_hard", "planner", "pce", "snmpc_json", "snmpc_expr", "r2", "closed_loop", "disturbances",
                            "log_file"]
    if "log_file" in what:
        make_log_file()
    if "disturbances" in what:
        make_disturbances()
    if "replay_hard" in what:
        make_replay_hard()
    if "kat0" in what:
        make_kat0()
    if "replay" in what:
        make_replay("lvms", 0, 450)
        make_replay("monteblanco", 0, 400)
    if "planner" in what:
        make_planner()
    if "pce" in what:
        make_pce()
    if "snmpc_json" in what:
        make_snmpc_json()
    if "snmpc_expr" in what:
        make_snmpc_expr()
    if "r2" in what:
        make_r2()
    if "closed_loop" in what:
        make_closed_loop()
        make_closed_loop_full("monteblanco")
        make_closed_loop_full("lvms")
    print("golden fixtures written to", OUT)
