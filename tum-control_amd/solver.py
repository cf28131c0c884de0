"""
solver.py -- ctypes binding of libtumnmpc.so with the AcadosOcpSolver method surface.

`BatchedOcpSolver` mirrors the methods of acados_template.AcadosOcpSolver that the reference's
controller classes call (complete list):
    solve, set, get, cost_set, constraints_set, get_cost, get_stats, reset, get_from_qp_in
  call sites: Model_Predictive_Controller/Nominal_NMPC/NMPC_class.py:111-112,172,178,183,193,198,202-205,
  245-246,251,254,295-317; Stochastic_NMPC/SNMPC_class.py:124,130,198;
  Reduced_Robustified_NMPC/Reduced_Robustified_NMPC_class.py:264,280,295,298,335-336,359.
With batch == 1 every method takes / returns exactly the shapes acados does, so the reference's
controller code runs unchanged on it. With batch > 1 values gain a leading batch axis; a value
without it is broadcast to all instances.

There is NO CPU fallback: if the HIP library or a GPU is missing, construction raises.
"""
import contextlib
import ctypes
import os

import numpy as np

from . import config as _config

_HERE = os.path.dirname(os.path.abspath(__file__))
# development build (tests / experiments): the same C-ABI plus the kernel variants "fused" and "pipeline4" (tum_ocp_set_kernel)
DEV_LIB_PATH = os.path.join(_HERE, "libtumnmpc_dev.so")
# overrides: TUM_NMPC_LIB=<path> (A/B testing of builds), TUM_NMPC_DEV=1 (a whole script on the development build)
LIB_PATH = os.environ.get("TUM_NMPC_LIB", DEV_LIB_PATH if os.environ.get("TUM_NMPC_DEV") == "1" else os.path.join(_HERE, "libtumnmpc.so"))
ALL_STAGES = -1


class TumOcpDesc(ctypes.Structure):
    _fields_ = (
        [("N", ctypes.c_int), ("nsub", ctypes.c_int), ("dt", ctypes.c_double),
         ("batch", ctypes.c_int), ("device", ctypes.c_int)]
        + [(n, ctypes.c_double) for n in
           ("lf", "lr", "m", "Iz", "ro", "S", "Cd", "Bf", "Cf", "Df", "Ef", "Br", "Cr", "Dr", "Er",
            "g", "fr0", "fr1", "fr4", "acc_min")]
        + [("n_ggv", ctypes.c_int),
           ("ggv_v", ctypes.c_double * 16), ("ggv_ax", ctypes.c_double * 16), ("ggv_ay", ctypes.c_double * 16),
           ("qp_iter_max", ctypes.c_int),
           ("qp_tol_stat", ctypes.c_double), ("qp_tol_ineq", ctypes.c_double), ("qp_tol_comp", ctypes.c_double),
           ("qp_mu0", ctypes.c_double), ("qp_t0", ctypes.c_double), ("store_qp_in", ctypes.c_int),
           ("qp_warm_start", ctypes.c_int), ("qp_warm_mu", ctypes.c_double),
           ("qp_warm_flips", ctypes.c_int), ("qp_warm_viol", ctypes.c_double)]
    )


_lib = None
_libs = {}              # path -> loaded library
_default_path = None    # None: LIB_PATH


@contextlib.contextmanager
def dev_library():
    """Solvers created inside this context bind to the development build (libtumnmpc_dev.so: the shipped pipeline plus the
    kernel variants "fused" and "pipeline4"). Tests and experiments only."""
    global _default_path
    old = _default_path
    _default_path = DEV_LIB_PATH
    try:
        yield
    finally:
        _default_path = old


# every symbol include/tum_nmpc.h declares (tests/test_cabi.py checks the .so exports them all)
C_SYMBOLS = ["tum_ocp_create", "tum_ocp_free", "tum_ocp_last_error", "tum_ocp_batch", "tum_ocp_horizon",
             "tum_ocp_set", "tum_ocp_get", "tum_ocp_constraints_set", "tum_ocp_cost_set",
             "tum_ocp_solve", "tum_ocp_solve_async", "tum_ocp_synchronize", "tum_ocp_options_set",
             "tum_ocp_get_cost", "tum_ocp_get_stats", "tum_ocp_reset", "tum_ocp_get_from_qp_in",
             "tum_ocp_set_stream", "tum_ocp_get_device", "tum_ocp_put_device", "tum_ocp_bind_device", "tum_ocp_results_async", "tum_ocp_results_wait", "tum_ocp_results_outstanding", "tum_ocp_step_async", "tum_ocp_cold_start", "tum_ocp_last_kernel_ms",
             "tum_ocp_debug_dump", "tum_ocp_get_condensed_qp", "tum_ocp_get_snmpc_linearisation", "tum_ocp_profile_phases", "tum_ocp_set_schedule", "tum_ocp_set_kernel",
             "tum_ocp_set_x0_fanout", "tum_pce_moments", "tum_pce_attach", "tum_pce_moments_device",
             "tum_ocp_bounds_snapshot", "tum_ocp_bounds_restore", "tum_ocp_r2_backoff", "tum_ocp_r2_attach", "tum_ocp_constraints_get",
             "tum_ocp_snmpc_attach", "tum_ocp_snmpc_samples", "tum_ocp_snmpc_set_offsets",
             "tum_planner_emulate", "tum_planner_emulate_tracks", "tum_sim_create", "tum_sim_create_tracks", "tum_sim_free", "tum_sim_set_state", "tum_sim_plan", "tum_sim_advance",
             "tum_sim_run", "tum_sim_steps", "tum_sim_get", "tum_sim_set_disturbances",
             "tum_sim_disturbances_attach", "tum_sim_disturbances_table",
             "tum_sim_segments_attach", "tum_sim_run_segments", "tum_sim_env_attach", "tum_sim_env_reset", "tum_sim_env_step",
             "tum_sim_policy_attach", "tum_sim_policy_eval", "tum_sim_env_rollout", "tum_sim_wmpc_attach", "tum_sim_wmpc_get",
             "tum_sim_policy_attach_value", "tum_sim_policy_eval_ac", "tum_sim_gae", "tum_sim_env_collect",
             "tum_sim_ppo_attach", "tum_sim_ppo_detach", "tum_sim_ppo_step", "tum_sim_ppo_update", "tum_sim_ppo_params", "tum_sim_ppo_state"]
# the entry points of the Bayesian-optimisation step (bo.py), declared in the same header; a list of their own because
# tests/test_host_logic.py::test_cabi_exports_every_declared_symbol holds C_SYMBOLS to the tum_ocp / tum_pce / tum_sim / tum_planner names
BO_SYMBOLS = ["tum_bo_create", "tum_bo_free", "tum_bo_model", "tum_bo_evaluate", "tum_bo_profile"]
# the entry points of the surrogate fit (bo.DeviceGP), a list of their own for the same reason
GP_SYMBOLS = ["tum_gp_create", "tum_gp_free", "tum_gp_data", "tum_gp_mll", "tum_gp_factor", "tum_gp_profile"]
# the entry points that build parts of the acquisition model on the device (bo.prune_baseline, bo.build_fronts): they work on a tum_bo
# handle; their prefix is their own because tests/test_bo_host.py holds the tum_bo_ names of the header to BO_SYMBOLS
BOM_SYMBOLS = ["tum_bom_prune_desc_init", "tum_bom_prune", "tum_bom_fronts", "tum_bom_prune_profile",
               "tum_bom_build_desc_init", "tum_bom_build", "tum_bom_model_read", "tum_bom_build_profile", "tum_bom_append"]


def load_library(path=None):
    """dlopen libtumnmpc.so (built by __graft_entry__.build()); raises if it is missing."""
    global _lib
    p = path or _default_path or LIB_PATH
    if p in _libs:
        return _libs[p]
    try:
        # torch ships its own HIP runtime: let it load first so that libtumnmpc.so binds to the same
        # libamdhip64 (two runtimes in one process lose the device)
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the solver has no CPU fallback)")
    L = ctypes.CDLL(p)
    dp = ctypes.POINTER(ctypes.c_double)
    vp, ci, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
    L.tum_ocp_create.restype = vp; L.tum_ocp_create.argtypes = [ctypes.POINTER(TumOcpDesc)]
    L.tum_ocp_free.restype = None; L.tum_ocp_free.argtypes = [vp]
    L.tum_ocp_last_error.restype = cs; L.tum_ocp_last_error.argtypes = []
    L.tum_ocp_batch.argtypes = [vp]; L.tum_ocp_horizon.argtypes = [vp]
    # (the data pointer of the per-call setters / getters goes over as a plain address -- `a.ctypes.data` -- : building a typed ctypes
    #  pointer per call costs 1.9 us, twice the rest of a call; the reference issues 83 of them per control step)
    for name in ("tum_ocp_set", "tum_ocp_constraints_set", "tum_ocp_cost_set"):
        getattr(L, name).argtypes = [vp, ci, cs, vp, ci, ci, ci, ci]
    L.tum_ocp_get.argtypes = [vp, ci, cs, vp, ci, ci, ci, ci]
    L.tum_ocp_get_from_qp_in.argtypes = [vp, ci, cs, dp, ci, ci, ci, ci]
    L.tum_ocp_solve.argtypes = [vp]; L.tum_ocp_solve_async.argtypes = [vp]; L.tum_ocp_synchronize.argtypes = [vp]
    if hasattr(L, "tum_ocp_options_set"):
        L.tum_ocp_options_set.argtypes = [vp, cs, ctypes.c_double]
    L.tum_ocp_get_cost.argtypes = [vp, dp, ci, ci]
    L.tum_ocp_get_stats.argtypes = [vp, cs, vp, ci, ci]
    L.tum_ocp_reset.argtypes = [vp]; L.tum_ocp_cold_start.argtypes = [vp]
    L.tum_ocp_set_stream.argtypes = [vp, vp]
    L.tum_ocp_set_schedule.argtypes = [vp, ci]
    L.tum_ocp_set_kernel.argtypes = [vp, cs]
    L.tum_ocp_get_device.argtypes = [vp, cs, vp, ci, ci]
    L.tum_ocp_put_device.argtypes = [vp, cs, vp, ci, ci]
    if hasattr(L, "tum_ocp_bind_device"):
        L.tum_ocp_bind_device.argtypes = [vp, cs, vp]
    if hasattr(L, "tum_ocp_results_async"):          # (absent from the libraries of earlier revisions that scripts/dev/ab2.py loads beside this one)
        L.tum_ocp_results_async.argtypes = [vp, ci]
        L.tum_ocp_results_wait.argtypes = [vp, ctypes.POINTER(dp), ctypes.POINTER(dp), ctypes.POINTER(dp)]
    if hasattr(L, "tum_ocp_results_outstanding"):
        L.tum_ocp_results_outstanding.argtypes = [vp]
    if hasattr(L, "tum_ocp_step_async"):
        L.tum_ocp_step_async.argtypes = [vp, vp, vp, ci]
    L.tum_ocp_last_kernel_ms.restype = ctypes.c_double; L.tum_ocp_last_kernel_ms.argtypes = [vp]
    L.tum_ocp_debug_dump.argtypes = [vp, ci, dp, ci]
    if hasattr(L, "tum_ocp_get_condensed_qp"):
        L.tum_ocp_get_condensed_qp.argtypes = [vp, ci, ci, dp, dp, dp, dp, dp, ctypes.POINTER(ci)]
    if hasattr(L, "tum_ocp_get_snmpc_linearisation"):
        L.tum_ocp_get_snmpc_linearisation.argtypes = [vp, ci, ci] + [dp] * 11 + [ctypes.POINTER(ci)]
    L.tum_ocp_profile_phases.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    L.tum_ocp_set_x0_fanout.argtypes = [vp, dp, dp, ci, ci]
    L.tum_pce_moments.argtypes = [vp, cs, ci, dp, ci, ci, dp, dp]
    L.tum_pce_attach.argtypes = [vp, dp, ci, ci]
    L.tum_pce_moments_device.argtypes = [vp, cs, ci, vp, vp]
    L.tum_ocp_bounds_snapshot.argtypes = [vp]; L.tum_ocp_bounds_restore.argtypes = [vp]
    L.tum_ocp_r2_backoff.argtypes = [vp, dp, dp, ci, ctypes.c_double, ctypes.c_double, ctypes.c_double, dp]
    L.tum_ocp_constraints_get.argtypes = [vp, ci, cs, dp, ci, ci]
    L.tum_ocp_r2_attach.argtypes = [vp, dp, dp, ci, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.tum_ocp_snmpc_attach.argtypes = [vp, ci, ci, dp, ci, ctypes.c_double]
    L.tum_ocp_snmpc_samples.argtypes = [vp]
    L.tum_ocp_snmpc_set_offsets.argtypes = [vp, dp]
    ip = ctypes.POINTER(ctypes.c_int); cd = ctypes.c_double
    L.tum_planner_emulate.argtypes = [dp, ci, dp, ci, ci, cd, ci, dp, ip, ci]
    L.tum_sim_create.restype = vp; L.tum_sim_create.argtypes = [vp, dp, ci, cd, ci, cd, ci, ip, ci]
    if hasattr(L, "tum_sim_create_tracks"):
        L.tum_planner_emulate_tracks.argtypes = [dp, ip, ci, ip, dp, ci, ci, cd, ci, dp, ip, ci]
        L.tum_sim_create_tracks.restype = vp; L.tum_sim_create_tracks.argtypes = [vp, dp, ip, ci, ip, cd, ci, cd, ci, ip, ci]
    L.tum_sim_free.restype = None; L.tum_sim_free.argtypes = [vp]
    L.tum_sim_set_state.argtypes = [vp, dp, dp, ci]
    L.tum_sim_plan.argtypes = [vp]; L.tum_sim_advance.argtypes = [vp]; L.tum_sim_run.argtypes = [vp, ci]
    L.tum_sim_steps.argtypes = [vp]
    L.tum_sim_get.argtypes = [vp, cs, dp, ctypes.c_longlong]
    if hasattr(L, "tum_sim_set_disturbances"):
        L.tum_sim_set_disturbances.argtypes = [vp, dp, dp, ci]
    if hasattr(L, "tum_sim_disturbances_attach"):
        L.tum_sim_disturbances_attach.argtypes = [vp, ci, dp, ci, dp, ctypes.c_ulonglong]
        L.tum_sim_disturbances_table.argtypes = [vp, ctypes.c_longlong, ci, dp, dp]
    if hasattr(L, "tum_sim_segments_attach"):
        L.tum_sim_segments_attach.argtypes = [vp, ip, ip, ci, cd, cd]
        L.tum_sim_run_segments.argtypes = [vp, ci, ci]
    if hasattr(L, "tum_sim_env_attach"):
        L.tum_sim_env_attach.argtypes = [vp, dp, ci, ci, cd, ci, ci, dp, dp, dp, dp, ip, ip, ci, ci]
        L.tum_sim_env_reset.argtypes = [vp, ip, ip]
        L.tum_sim_env_step.argtypes = [vp, ip, ip, ip, dp]
    if hasattr(L, "tum_sim_policy_attach"):
        L.tum_sim_policy_attach.argtypes = [vp, ci, ip, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.tum_sim_policy_eval.argtypes = [vp, dp, ci, dp, dp, ip]
        L.tum_sim_env_rollout.argtypes = [vp, ci, dp, ci, ip, ci, dp, ip, ip, ip]
    if hasattr(L, "tum_sim_wmpc_attach"):
        L.tum_sim_wmpc_attach.argtypes = [vp, dp, ci, ci, ci, ci, ip, ip, dp, dp, ci]
        L.tum_sim_wmpc_get.argtypes = [vp, cs, dp, ctypes.c_longlong]
    if hasattr(L, "tum_sim_env_collect"):
        u64 = ctypes.c_ulonglong
        L.tum_sim_policy_attach_value.argtypes = [vp, ci, ip, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.tum_sim_policy_eval_ac.argtypes = [vp, dp, ci, u64, u64, ctypes.c_uint, ip, dp, dp, dp]
        L.tum_sim_gae.argtypes = [vp, ci, ci, dp, dp, dp, dp, dp, cd, cd, dp, dp]
        L.tum_sim_env_collect.argtypes = [vp, ci, dp, dp, ip, u64, u64, cd, cd, dp]
    if hasattr(L, "tum_sim_ppo_attach"):
        pvp = ctypes.POINTER(vp)
        L.tum_sim_ppo_attach.argtypes = [vp, cd, cd, cd, cd, ci]
        L.tum_sim_ppo_detach.argtypes = [vp]
        L.tum_sim_ppo_step.argtypes = [vp, ci, dp, ip, dp, dp, dp, cd, ci, dp, dp, dp]
        L.tum_sim_ppo_update.argtypes = [vp, ci, dp, ip, dp, dp, dp, ip, ci, ci, cd, dp]
        L.tum_sim_ppo_params.argtypes = [vp, pvp, pvp, pvp, pvp]
        L.tum_sim_ppo_state.argtypes = [vp, dp, dp, ctypes.POINTER(ctypes.c_longlong), ip]
    if hasattr(L, "tum_bo_create"):
        L.tum_bo_create.restype = vp; L.tum_bo_create.argtypes = [ci]
        L.tum_bo_free.restype = None; L.tum_bo_free.argtypes = [vp]
        L.tum_bo_model.argtypes = [vp, vp]
        L.tum_bo_evaluate.argtypes = [vp, dp, ci, dp, dp]
        L.tum_bo_profile.argtypes = [vp, ci, dp]
    if hasattr(L, "tum_bom_prune"):
        L.tum_bom_prune_desc_init.restype = None; L.tum_bom_prune_desc_init.argtypes = [vp]
        L.tum_bom_prune.argtypes = [vp, vp, ip, dp, ip]
        L.tum_bom_fronts.argtypes = [vp, dp, ci, ci, dp, dp, ip]
        L.tum_bom_prune_profile.argtypes = [vp, ci, dp]
        L.tum_bom_build_desc_init.restype = None; L.tum_bom_build_desc_init.argtypes = [vp]
        L.tum_bom_build.argtypes = [vp, vp, ip]
        L.tum_bom_build_profile.argtypes = [vp, ci, dp]
        L.tum_bom_append.argtypes = [vp, dp, ip]
        L.tum_bom_model_read.argtypes = [vp, vp, vp, vp, vp, dp, dp, ip, ip]
    if hasattr(L, "tum_gp_create"):
        L.tum_gp_create.restype = vp; L.tum_gp_create.argtypes = [ci]
        L.tum_gp_free.restype = None; L.tum_gp_free.argtypes = [vp]
        L.tum_gp_data.argtypes = [vp, dp, dp, dp, ci, ci]
        L.tum_gp_mll.argtypes = [vp, dp, ci, ctypes.c_double, dp, dp, ip]
        L.tum_gp_factor.argtypes = [vp, dp, ci, ctypes.c_double, dp, dp, ip]
        L.tum_gp_profile.argtypes = [vp, ci, dp]
    _libs[p] = L
    if p == LIB_PATH:
        _lib = L
    return L


def make_desc(N, dt, nsub, batch, device=0, cfg=None, store_qp_in=False, qp_iter_max=50,
              qp_tol=(1e-8, 1e-8, 1e-8), qp_mu0=0.05, qp_t0=0.05, qp_warm_start=True, qp_warm_mu=0.0,
              qp_warm_flips=0, qp_warm_viol=0.0):
    cfg = cfg or _config.default_config()
    d = TumOcpDesc()
    d.N, d.nsub, d.dt, d.batch, d.device = int(N), int(nsub), float(dt), int(batch), int(device)
    for k in ("lf", "lr", "m", "Iz", "ro", "S", "Cd", "acc_min"):
        setattr(d, k, float(cfg["veh"][k]))
    for k in ("Bf", "Cf", "Df", "Ef", "Br", "Cr", "Dr", "Er"):
        setattr(d, k, float(cfg["tire"][k]))
    for k in ("g", "fr0", "fr1", "fr4"):
        setattr(d, k, float(cfg["phys"][k]))
    n = len(cfg["ggv"]["v"])
    if n > 16:
        raise ValueError("ggv table longer than 16 rows")
    d.n_ggv = n
    for i in range(n):
        d.ggv_v[i], d.ggv_ax[i], d.ggv_ay[i] = cfg["ggv"]["v"][i], cfg["ggv"]["ax"][i], cfg["ggv"]["ay"][i]
    d.qp_iter_max = int(qp_iter_max)
    d.qp_tol_stat, d.qp_tol_ineq, d.qp_tol_comp = (float(t) for t in qp_tol)
    d.qp_mu0 = float(qp_mu0)
    d.qp_t0 = float(qp_t0)
    d.store_qp_in = 1 if store_qp_in else 0
    d.qp_warm_start = 1 if qp_warm_start else 0
    d.qp_warm_mu = float(qp_warm_mu)
    d.qp_warm_flips, d.qp_warm_viol = int(qp_warm_flips), float(qp_warm_viol)      # (0: the library's defaults 16 / 0.1)
    return d


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


_FIELD_BYTES = {}          # field name -> bytes, encoded once
# acados' defaults of the NLP solver options as the reference's generated solver carries them (acados_ocp_SNMPC.json)
_NLP_DEFAULTS = dict(nlp_solver_max_iter=100, nlp_solver_tol_stat=1e-6, nlp_solver_tol_eq=1e-6, nlp_solver_tol_ineq=1e-6,
                     nlp_solver_tol_comp=1e-6, nlp_solver_step_length=1.0, alpha_min=0.05, alpha_reduction=0.7, merit_weight_eq=1.0)
_NLP_TYPES = {"SQP_RTI": 0, "SQP": 1}
# acados' globalization of an SQP solve: the step length of nlp_solver_step_length, or a line search per instance on an L1 merit function
_GLOBALIZATIONS = {"FIXED_STEP": 0, "MERIT_BACKTRACKING": 1}
# acados' rti_phase values: 0 preparation and feedback in one solve(), 1 preparation, 2 feedback
_RTI_PHASES = {0: "PREPARATION_AND_FEEDBACK", 1: "PREPARATION", 2: "FEEDBACK"}


def _rti_phase_value(value):
    """rti_phase as acados takes it: the integer 0, 1 or 2 (anything else is refused before the library sees it)"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer, float, np.floating)) or value not in _RTI_PHASES:
        raise Exception(f"BatchedOcpSolver.options_set: rti_phase must be 0 (preparation and feedback), 1 (preparation) or 2 (feedback), got {value!r}")
    return int(value)


def _globalization_value(value):
    """globalization as acados takes it, by name (or the library's 0 / 1); anything else is refused before the library sees it"""
    if isinstance(value, str):
        if value not in _GLOBALIZATIONS:
            raise Exception(f"BatchedOcpSolver.options_set: globalization must be one of {sorted(_GLOBALIZATIONS)}, got '{value}'")
        return _GLOBALIZATIONS[value]
    if isinstance(value, bool) or not isinstance(value, (int, np.integer, float, np.floating)) or value not in _GLOBALIZATIONS.values():
        raise Exception(f"BatchedOcpSolver.options_set: globalization must be one of {sorted(_GLOBALIZATIONS)} (0 / 1), got {value!r}")
    return int(value)


class BatchedOcpSolver:
    """`batch` independent copies of the nominal NMPC OCP on one MI355X; acados method names."""

    def __init__(self, N=38, dt=0.08, nsub=3, batch=1, device=0, cfg=None, store_qp_in=False,
                 qp_iter_max=50, qp_tol=(1e-8, 1e-8, 1e-8), qp_mu0=0.05, qp_t0=0.05, qp_warm_start=None, qp_warm_mu=0.0,
                 qp_warm_flips=0, qp_warm_viol=0.0, nlp_solver_type="SQP_RTI", nlp_solver_max_iter=100, nlp_solver_tol_stat=1e-6,
                 nlp_solver_tol_eq=1e-6, nlp_solver_tol_ineq=1e-6, nlp_solver_tol_comp=1e-6, nlp_solver_step_length=1.0,
                 globalization="FIXED_STEP", alpha_min=0.05, alpha_reduction=0.7, merit_weight_eq=1.0):
        self._L = load_library()
        self.N, self.dt, self.nsub, self.batch = int(N), float(dt), int(nsub), int(batch)
        self.cfg = cfg or _config.default_config()
        if qp_warm_start is None:
            # (acados: qp_solver_warm_start) ON by default for every controller, whichever library is loaded -- a deliberate, documented
            # deviation for the nominal and R2 solvers, where the reference leaves the option at acados' default 0 (INTEGRATION.md,
            # "Interior point warm start"; qp_warm_start=False gives the cold-started method). The development build's extra kernels
            # ("fused", "pipeline4") always cold-start the method and ignore the flag.
            qp_warm_start = True
        self._desc = make_desc(N, dt, nsub, batch, device, self.cfg, store_qp_in, qp_iter_max, qp_tol, qp_mu0, qp_t0, qp_warm_start, qp_warm_mu,
                               qp_warm_flips, qp_warm_viol)
        self._h = self._L.tum_ocp_create(ctypes.byref(self._desc))
        if not self._h:
            raise RuntimeError("tum_ocp_create failed: " + self._err())
        self.status = 0
        # NLP solver options (acados_ocp_SNMPC.json: nlp_solver_*); the defaults leave the capsule as created -- SQP_RTI
        nlp = dict(nlp_solver_max_iter=nlp_solver_max_iter, nlp_solver_tol_stat=nlp_solver_tol_stat, nlp_solver_tol_eq=nlp_solver_tol_eq,
                   nlp_solver_tol_ineq=nlp_solver_tol_ineq, nlp_solver_tol_comp=nlp_solver_tol_comp, nlp_solver_step_length=nlp_solver_step_length,
                   alpha_min=alpha_min, alpha_reduction=alpha_reduction, merit_weight_eq=merit_weight_eq)
        for k, v in nlp.items():
            if v != _NLP_DEFAULTS[k]:
                self.options_set(k, v)
        if globalization != "FIXED_STEP":
            self.options_set("globalization", globalization)
        if nlp_solver_type != "SQP_RTI":
            self.options_set("nlp_solver_type", nlp_solver_type)

    # ------------------------------------------------------------------ plumbing
    def _err(self):
        e = self._L.tum_ocp_last_error()
        return e.decode() if e else ""

    def _chk(self, rc, what):
        if rc != 0:
            raise Exception(f"BatchedOcpSolver.{what}: {self._err()}")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.tum_ocp_free(self._h)
                self._h = None
        except Exception:
            pass

    def _put(self, fn, stage, field, value, what):
        v = np.ascontiguousarray(value, dtype=np.float64)
        fb = _FIELD_BYTES.get(field) or _FIELD_BYTES.setdefault(field, field.encode())
        if v.ndim >= 2 and v.shape[0] == self.batch and self.batch > 1:
            v = v.reshape(self.batch, -1)
            ln = v.shape[1]
            self._chk(fn(self._h, stage, fb, v.ctypes.data, ln, 0, self.batch, ln), what)
        else:
            scalar_field = field in ("uh", "lh", "lbu", "ubu") or (field in ("lbx", "ubx") and stage != 0)
            if self.batch > 1 and v.ndim >= 1 and v.shape[0] == self.batch and scalar_field:   # one value per instance
                v = v.reshape(self.batch, 1)
                self._chk(fn(self._h, stage, fb, v.ctypes.data, 1, 0, self.batch, 1), what)
                return
            self._chk(fn(self._h, stage, fb, v.ctypes.data, v.size, 0, self.batch, 0), what)

    def _out(self, a):
        return a[0] if self.batch == 1 else a

    # ------------------------------------------------------------------ acados surface
    def set(self, stage, field, value):
        """acados_solver.set(stage, 'x'|'u'|'yref', value)"""
        self._put(self._L.tum_ocp_set, stage, field, value, "set")

    def get(self, stage, field):
        """acados_solver.get(stage, 'x'|'u'|'sl'|'su'|'lam'); 'lam': the multipliers of the last QP's rows, lower sides in the order of
        'sl', then upper sides in the order of 'su' (without acados' trailing multipliers of the slack bounds)"""
        N = self.N
        if field == "x":
            ln = 8
        elif field == "u":
            ln = 2
        elif field in ("sl", "su"):
            ln = 1 if stage == 0 else (2 if stage == N else 3)
        elif field == "lam":
            ln = 2 if stage == 0 else (4 if stage == N else 6)
        else:
            raise Exception(f"BatchedOcpSolver.get: unknown field '{field}'")
        out = np.empty((self.batch, ln))
        fb = _FIELD_BYTES.get(field) or _FIELD_BYTES.setdefault(field, field.encode())
        self._chk(self._L.tum_ocp_get(self._h, stage, fb, out.ctypes.data, ln, 0, self.batch, ln), "get")
        return out[0] if self.batch == 1 else out

    def constraints_set(self, stage, field, value):
        self._put(self._L.tum_ocp_constraints_set, stage, field, value, "constraints_set")

    def cost_set(self, stage, field, value):
        """acados_solver.cost_set (NMPC_class.py:294-317). 'W' is PER STAGE, as in acados: cost_set(i, 'W', W) touches stage i only
        (stage N: the 4 x 4 terminal weight); cost_set(ALL_STAGES, 'W', W6x6) sets the stages 0..N-1 in one call. W may be any
        (symmetric) matrix, as in acados: diagonal ones -- all the reference installs -- keep the capsule on the headline's kernels, the first W with
        an off-diagonal entry switches it to the full-W form (include/tum_nmpc.h). 'zl' | 'zu' | 'Zl' | 'Zu': per penalty class (stage 0 / 1..N-1 / N)."""
        v = np.asarray(value, dtype=np.float64)
        if field == "W":
            ny = 6 if (stage < self.N) else 4          # (stage == ALL_STAGES = -1: one 6 x 6 W for all the stages 0..N-1)
            if v.ndim == 3:     # (batch, ny, ny): column-major per instance
                v = np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(v.shape[0], ny * ny)
            else:
                v = np.ascontiguousarray(v.T).reshape(-1)
        self._put(self._L.tum_ocp_cost_set, stage, field, v, "cost_set")

    def solve(self):
        st = self._L.tum_ocp_solve(self._h)
        if st < 0:
            raise Exception("BatchedOcpSolver.solve: " + self._err())
        self.status = st
        return st

    def options_set(self, field, value):
        """acados_solver.options_set(field, value) for the NLP solver: 'nlp_solver_type' ('SQP_RTI' | 'SQP'), 'nlp_solver_max_iter',
        'nlp_solver_tol_stat' | '_eq' | '_ineq' | '_comp', 'nlp_solver_step_length', 'globalization' ('FIXED_STEP' | 'MERIT_BACKTRACKING')
        with 'alpha_min', 'alpha_reduction' and 'merit_weight_eq' (include/tum_nmpc.h, tum_ocp_options_set);
        'rti_phase' 0 | 1 | 2: the following solve() calls are whole SQP-RTI steps (default), preparations or feedbacks;
        'lin_dedup' 1 | 0: linearise a stage-uniform iterate (after cold_start() / reset()) once per instance (default) or per stage;
        'uniform_records' 0 | 1: such a solve writes no stage records where nothing reads them (default), or always fills them;
        'uniform_powers' 1 | 0: its condensing computes the sequences A^m B once per instance (default) or carries every column through every stage;
        'uniform_shift' 1 | 0: that condensing (N <= 40) forms the Hessian tiles below block row 0 from those of block row 0 where an instance's
        cost weights are the same at every stage (default), or every tile from its own products; get_stats('cond_shifted') counts the instances"""
        if field == "rti_phase":
            value = _rti_phase_value(value)
        if field == "globalization":
            value = _globalization_value(value)
        if field == "nlp_solver_type" and isinstance(value, str):
            if value not in _NLP_TYPES:
                raise Exception(f"BatchedOcpSolver.options_set: nlp_solver_type must be one of {sorted(_NLP_TYPES)}, got '{value}'")
            value = _NLP_TYPES[value]
        self._chk(self._L.tum_ocp_options_set(self._h, field.encode(), float(value)), "options_set")

    def prepare(self):
        """PREPARATION of a split real-time iteration (options_set('rti_phase', 1) + solve()): linearisation and condensing at the
        current iterate, reference and x0 -- everything that can run before the measured state is known. Leaves iterate and results
        untouched, returns 0; get_stats('time_tot') is its device time. The capsule stays in rti_phase 1."""
        self.options_set("rti_phase", 1)
        return self.solve()

    def feedback(self, x0=None):
        """FEEDBACK of a split real-time iteration (options_set('rti_phase', 2) + solve()): x0 (None: keep) enters the prepared QP, then
        the interior point method and the expansion. Raises without a (fresh) preparation. The capsule stays in rti_phase 2."""
        self.options_set("rti_phase", 2)
        if x0 is not None:
            self.set_x0(x0)
        return self.solve()

    def get_residuals(self):
        """acados_solver.get_residuals(): [stat, eq, ineq, comp] of the NLP at the iterate of the last SQP solve; (batch, 4) for a batch"""
        return self.get_stats("residuals")

    def _merit_dims(self):
        """(K, M) of the last solve: candidates of its line search, its nlp_solver_max_iter (refused unless it was MERIT_BACKTRACKING)"""
        o = (ctypes.c_int * 2)()
        self._chk(self._L.tum_ocp_get_stats(self._h, b"merit_dims", o, 0, 1), "get_stats")
        return int(o[0]), int(o[1])

    def get_alpha(self):
        """step lengths the line search of the last SQP solve accepted (globalization MERIT_BACKTRACKING): (batch, max_iter), row b
        holds those of its QPs 1 .. sqp_iter[b], then zeros"""
        return self.get_stats("alpha")

    def get_merit(self):
        """(table, weights) of each instance's own last line search: table (batch, K + 1, 3) with the columns cost, E, V at the
        candidates alpha_reduction^j, j < K, and in row K at alpha = 0; weights (batch, 2): mu_eq, mu_in"""
        return self.get_stats("merit"), self.get_stats("merit_weights")

    def get_cost(self):
        out = np.zeros(self.batch)
        self._chk(self._L.tum_ocp_get_cost(self._h, _dp(out), 0, self.batch), "get_cost")
        return float(out[0]) if self.batch == 1 else out

    def get_stats(self, field):
        if field in ("time_tot", "time_ipm"):
            o = ctypes.c_double(0.0)
            self._chk(self._L.tum_ocp_get_stats(self._h, field.encode(), ctypes.byref(o), 0, 1), "get_stats")
            return o.value
        if field in ("sqp_iter", "qp_iter", "status", "qp_status", "lpt_order"):
            out = np.zeros(self.batch, dtype=np.int32)
            self._chk(self._L.tum_ocp_get_stats(self._h, field.encode(), out.ctypes.data_as(ctypes.c_void_p), 0, self.batch), "get_stats")
            if field == "sqp_iter" and self.batch == 1:
                return int(out[0])
            return out            # acados returns an array for qp_iter; callers take np.max
        # linearisations that took the uniform path (options_set('lin_dedup', 0 | 1)); solves without stage records ('uniform_records');
        # instances of the last solve whose condensing took the shift form ('uniform_shift')
        if field in ("lin_uniform", "records_skipped", "cond_shifted"):
            o = ctypes.c_int(0)
            self._chk(self._L.tum_ocp_get_stats(self._h, field.encode(), ctypes.byref(o), 0, 1), "get_stats")
            return o.value
        if field == "res":
            out = np.zeros((self.batch, 3))
            self._chk(self._L.tum_ocp_get_stats(self._h, b"res", out.ctypes.data_as(ctypes.c_void_p), 0, self.batch), "get_stats")
            return self._out(out)
        if field == "residuals":
            out = np.zeros((self.batch, 4))
            self._chk(self._L.tum_ocp_get_stats(self._h, b"residuals", out.ctypes.data_as(ctypes.c_void_p), 0, self.batch), "get_stats")
            return self._out(out)
        if field in ("alpha", "merit", "merit_weights"):
            K, M = self._merit_dims()
            out = np.zeros({"alpha": (self.batch, M), "merit": (self.batch, K + 1, 3), "merit_weights": (self.batch, 2)}[field])
            self._chk(self._L.tum_ocp_get_stats(self._h, field.encode(), out.ctypes.data_as(ctypes.c_void_p), 0, self.batch), "get_stats")
            return self._out(out)
        raise Exception(f"BatchedOcpSolver.get_stats: unknown field '{field}'")

    def reset(self):
        self._chk(self._L.tum_ocp_reset(self._h), "reset")

    def get_from_qp_in(self, stage, field):
        shp = {"A": (8, 8), "B": (8, 2), "b": (8,)}.get(field)
        if shp is None:
            raise Exception(f"BatchedOcpSolver.get_from_qp_in: unknown field '{field}'")
        n = int(np.prod(shp))
        out = np.zeros((self.batch, n))
        self._chk(self._L.tum_ocp_get_from_qp_in(self._h, stage, field.encode(), _dp(out), n, 0, self.batch, n), "get_from_qp_in")
        if len(shp) == 2:     # the C-ABI hands matrices out column-major (acados convention)
            out = np.ascontiguousarray(out.reshape(self.batch, shp[1], shp[0]).transpose(0, 2, 1))
        return self._out(out)

    # ------------------------------------------------------------------ batch conveniences (no acados counterpart)
    def set_x0(self, x0):
        """lbx_0 = ubx_0 = x0 for every instance; x0: (8,) or (batch, 8)."""
        self.constraints_set(0, "lbx", x0)

    def set_yref_all(self, yref):
        """yref: (N+1, 6) or (batch, N+1, 6); the terminal record uses its first 4 entries."""
        y = np.ascontiguousarray(yref, dtype=np.float64)
        if y.ndim == 3:
            y = y.reshape(y.shape[0], -1)
        else:
            y = y.reshape(-1)
        self._put(self._L.tum_ocp_set, ALL_STAGES, "yref", y, "set_yref_all")

    def set_iterate(self, X=None, U=None):
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64)
            self._put(self._L.tum_ocp_set, ALL_STAGES, "x", X.reshape(X.shape[0], -1) if X.ndim == 3 else X.reshape(-1), "set_iterate")
        if U is not None:
            U = np.ascontiguousarray(U, dtype=np.float64)
            self._put(self._L.tum_ocp_set, ALL_STAGES, "u", U.reshape(U.shape[0], -1) if U.ndim == 3 else U.reshape(-1), "set_iterate")

    def get_iterate(self):
        N = self.N
        X = np.zeros((self.batch, (N + 1) * 8)); U = np.zeros((self.batch, N * 2))
        self._chk(self._L.tum_ocp_get(self._h, ALL_STAGES, b"x", X.ctypes.data, X.shape[1], 0, self.batch, X.shape[1]), "get")
        self._chk(self._L.tum_ocp_get(self._h, ALL_STAGES, b"u", U.ctypes.data, U.shape[1], 0, self.batch, U.shape[1]), "get")
        return X.reshape(self.batch, N + 1, 8), U.reshape(self.batch, N, 2)

    def cold_start(self):
        """X_k = x0 for all k, U = 0 on the device (acados create/reset semantics)."""
        self._chk(self._L.tum_ocp_cold_start(self._h), "cold_start")

    def solve_async(self):
        self._chk(self._L.tum_ocp_solve_async(self._h), "solve_async")

    def synchronize(self):
        self._chk(self._L.tum_ocp_synchronize(self._h), "synchronize")

    def set_stream(self, hip_stream_ptr):
        self._chk(self._L.tum_ocp_set_stream(self._h, ctypes.c_void_p(hip_stream_ptr)), "set_stream")

    def get_device(self, field, dev_ptr, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        self._chk(self._L.tum_ocp_get_device(self._h, field.encode(), ctypes.c_void_p(dev_ptr), b0, nb), "get_device")

    def put_device(self, field, dev_ptr, b0=0, nb=None):
        """'x0' | 'yref' | 'X' | 'U' from caller-owned device memory (asynchronous D2D on the capsule's stream)"""
        nb = self.batch - b0 if nb is None else nb
        self._chk(self._L.tum_ocp_put_device(self._h, field.encode(), ctypes.c_void_p(dev_ptr), b0, nb), "put_device")

    def bind_device(self, field, dev_ptr):
        """'x0' | 'yref': use the caller's device array (whole batch) IN PLACE as the capsule's own -- no copy; dev_ptr None / 0 hands the
        capsule's own array back. The memory must stay valid and unchanged while solves that use it are in flight."""
        self._chk(self._L.tum_ocp_bind_device(self._h, field.encode(), ctypes.c_void_p(dev_ptr or 0)), "bind_device")

    def results_async(self, with_iterate=False):
        """Enqueue, behind the solve on this capsule's stream, the copy of the results into the capsule's pinned host slabs
        (summary: u0[2], cost, status, qp_iter per instance; with_iterate: also X and U). Returns at once."""
        self._chk(self._L.tum_ocp_results_async(self._h, int(bool(with_iterate))), "results_async")

    def results_wait(self):
        """Block until the copies of the last results_async have landed. Returns numpy VIEWS of the pinned slabs (valid until
        the next results_async on this capsule): (summary (batch, 5), X (batch, N+1, 8) or None, U (batch, N, 2) or None)."""
        dp = ctypes.POINTER(ctypes.c_double)
        ps, px, pu = dp(), dp(), dp()
        self._chk(self._L.tum_ocp_results_wait(self._h, ctypes.byref(ps), ctypes.byref(px), ctypes.byref(pu)), "results_wait")
        B, N = self.batch, self.N
        summ = np.ctypeslib.as_array(ps, shape=(B, 5))
        X = np.ctypeslib.as_array(px, shape=(B, N + 1, 8)) if px else None
        U = np.ctypeslib.as_array(pu, shape=(B, N, 2)) if pu else None
        return summ, X, U

    def step_async(self, x0=None, yref=None, with_iterate=True):
        """One control step of a host-driven loop in one call (tum_ocp_step_async): x0 (batch, 8) and yref (batch, N+1, 6) -- None:
        keep -- uploaded through pinned staging on the capsule's stream, one SQP-RTI behind them, the results request behind the
        solve. Returns at once; results_wait() delivers. In rti_phase 2 it is the one-call FEEDBACK step (x0 in, feedback, results;
        yref must be None: the reference enters in the preparation); in rti_phase 1 it is an error."""
        def arr(a, n):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != n:
                raise Exception(f"BatchedOcpSolver.step: expected {n} values, got {a.size}")
            return a, ctypes.c_void_p(a.ctypes.data)
        a0, p0 = arr(x0, self.batch * 8)
        a1, p1 = arr(yref, self.batch * (self.N + 1) * 6)
        self._chk(self._L.tum_ocp_step_async(self._h, p0, p1, int(bool(with_iterate))), "step_async")

    def results_outstanding(self):
        """result requests enqueued on this capsule and not yet waited for (0, 1 or 2)"""
        if not hasattr(self._L, "tum_ocp_results_outstanding"):      # (a saved build of an earlier round, scripts/dev/ab2.py)
            return 0
        return int(self._L.tum_ocp_results_outstanding(self._h))

    def step(self, x0=None, yref=None, with_iterate=True):
        """step_async + results_wait: (summary (batch, 5): u0[2], cost, status, qp_iter; X; U) as views of the capsule's pinned slabs.
        SYNCHRONOUS: the results returned are those of THIS step. results_wait delivers the OLDEST outstanding request, so requests an
        earlier caller left behind on this capsule (a results_async never waited for, a step whose wait was interrupted) are drained
        and dropped first -- otherwise every later step would hand out the previous step's results, one control step late."""
        while self.results_outstanding() > 0:
            self.results_wait()
        self.step_async(x0, yref, with_iterate)
        return self.results_wait()

    def set_schedule(self, longest_first=True):
        """Dispatch instances longest-first by the previous solve's iteration counts (default) or in natural order."""
        self._chk(self._L.tum_ocp_set_schedule(self._h, int(bool(longest_first))), "set_schedule")

    def set_kernel(self, name):
        """'auto' | 'fused' | 'pipeline' (include/tum_nmpc.h, tum_ocp_set_kernel)"""
        self._chk(self._L.tum_ocp_set_kernel(self._h, name.encode()), "set_kernel")

    def last_kernel_ms(self):
        return float(self._L.tum_ocp_last_kernel_ms(self._h))

    # ------------------------------------------------------------------ K6 / K7
    def set_x0_fanout(self, pose, offsets):
        """x0 of instance p*(S+1)+s = pose[p] (+ offsets[s-1] for s >= 1); batch must be P*(S+1)."""
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 8)
        offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 8)
        self._chk(self._L.tum_ocp_set_x0_fanout(self._h, _dp(pose), _dp(offsets), pose.shape[0], offsets.shape[0]), "set_x0_fanout")

    def pce_moments(self, field, stage, A):
        """mean / variance over every scenario group of `field` ('x' or 'u') at `stage`; A is the L x S PCE matrix."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        L_, S = A.shape
        m = 8 if field == "x" else 2
        P = self.batch // (S + 1)
        mean = np.zeros((P, m)); var = np.zeros((P, m))
        self._chk(self._L.tum_pce_moments(self._h, field.encode(), stage, _dp(A), L_, S, _dp(mean), _dp(var)), "pce_moments")
        return mean, var

    def pce_attach(self, A):
        """keep the L x S PCE matrix on the device for pce_moments_device"""
        A = np.ascontiguousarray(A, dtype=np.float64)
        self._chk(self._L.tum_pce_attach(self._h, _dp(A), A.shape[0], A.shape[1]), "pce_attach")

    def pce_moments_device(self, field, stage, mean_ptr, var_ptr):
        """asynchronous PCE mean / variance into caller-owned device buffers (P x m doubles each)"""
        self._chk(self._L.tum_pce_moments_device(self._h, field.encode(), int(stage), ctypes.c_void_p(mean_ptr),
                                                 ctypes.c_void_p(var_ptr)), "pce_moments_device")

    def bounds_snapshot(self):
        self._chk(self._L.tum_ocp_bounds_snapshot(self._h), "bounds_snapshot")

    def bounds_restore(self):
        """put back the bounds of the last snapshot (asynchronous, on the capsule's stream)"""
        self._chk(self._L.tum_ocp_bounds_restore(self._h), "bounds_restore")

    def r2_backoff(self, Sigma0, BWB, uph, delta_min, delta_max, uh_nom=1.0, return_backoffs=False):
        """R2NMPC tightening of lbx/ubx/uh for the next solve from the last linearisation (store_qp_in capsules)."""
        S0 = np.ascontiguousarray(Sigma0, dtype=np.float64).reshape(64)
        BW = np.ascontiguousarray(BWB, dtype=np.float64).reshape(64)
        bo = np.zeros((self.batch, self.N, 2)) if return_backoffs else None
        self._chk(self._L.tum_ocp_r2_backoff(self._h, _dp(S0), _dp(BW), int(uph), float(delta_min), float(delta_max),
                                             float(uh_nom), _dp(bo) if bo is not None else None), "r2_backoff")
        return bo

    def r2_attach(self, Sigma0, BWB, uph, delta_min, delta_max, uh_nom=1.0):
        """make the R2NMPC tightening part of every solve (device closed loops); uph = 0 detaches"""
        S = np.ascontiguousarray(Sigma0, dtype=np.float64).reshape(64); B = np.ascontiguousarray(BWB, dtype=np.float64).reshape(64)
        self._chk(self._L.tum_ocp_r2_attach(self._h, _dp(S), _dp(B), int(uph), float(delta_min), float(delta_max), float(uh_nom)), "r2_attach")

    def constraints_get(self, stage, field):
        out = np.zeros(self.batch)
        self._chk(self._L.tum_ocp_constraints_get(self._h, stage, field.encode(), _dp(out), 0, self.batch), "constraints_get")
        return float(out[0]) if self.batch == 1 else out

    def profile_phases(self):
        """One solve with the in-kernel phase timers on: (batch, 12) shader-cycle counters."""
        out = np.zeros((self.batch, 12), dtype=np.int64)
        self._chk(self._L.tum_ocp_profile_phases(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))), "profile_phases")
        return out

    def debug_dump(self, b=0, n=20480):
        out = np.zeros(n)
        self._chk(self._L.tum_ocp_debug_dump(self._h, b, _dp(out), n), "debug_dump")
        return out

    def get_condensed_qp(self, b0=0, nb=None):
        """The condensed QP of the instances b0 .. b0 + nb - 1 as the last preparation or solve handed it to the interior point kernel
        (read-only, launches nothing; every horizon, whichever condensing kernel ran): dict with H (nb, NVP, NVP), q (nb, NVP),
        C (nb, 2 N, NVP), d (nb, 2 N), dv (nb, NVP) and dv_valid. NVP = 16 x tiles: the 2 N condensed inputs and the padding. Row
        2 (s - 1) is the steering-angle row of stage s, row 2 (s - 1) + 1 its gg row. dv_valid False: the expansion ran as the tail of
        the interior point kernel (at most 1024 instances, N <= 48), which hands no step over -- dv is not that of this QP."""
        nb = self.batch - b0 if nb is None else int(nb)
        info = (ctypes.c_int * 3)()
        null = ctypes.POINTER(ctypes.c_double)()
        self._chk(self._L.tum_ocp_get_condensed_qp(self._h, int(b0), nb, null, null, null, null, null, info), "get_condensed_qp")
        nvp, m = int(info[0]), int(info[1])
        H = np.zeros((nb, nvp, nvp)); q = np.zeros((nb, nvp)); C = np.zeros((nb, m, nvp)); d = np.zeros((nb, nvp)); dv = np.zeros((nb, nvp))
        self._chk(self._L.tum_ocp_get_condensed_qp(self._h, int(b0), nb, _dp(H), _dp(q), _dp(C), _dp(d), _dp(dv), info), "get_condensed_qp")
        return dict(H=H, q=q, C=C, d=d[:, :m].copy(), dv=dv, dv_valid=bool(info[2]))

    # ------------------------------------------------------------------ reference defaults
    def install_reference_ocp(self, Q=None, R=None, Qe=None, L1=None, L2=None, w_scale=0.01):
        """What NMPC_STM_acados_settings.py:48-60,126-139,161-224 bakes into the solver at creation:
        W = 0.01*blockdiag(Q,R), W_e = 0.01*Qe, bounds on delta_f / steering rate, 0 <= h <= 1,
        slack penalties L1/L2 on every soft bound."""
        mpc, veh = self.cfg["mpc"], self.cfg["veh"]
        if Q is None:
            Q = np.diag([mpc["q_lon"] / mpc["s_lon"] ** 2, mpc["q_lat"] / mpc["s_lat"] ** 2,
                         mpc["q_yaw"] / mpc["s_yaw"] ** 2, mpc["q_vel"] / mpc["s_vel"] ** 2])
        if R is None:
            R = np.diag([mpc["r_jerk"] / mpc["s_jerk"] ** 2, mpc["r_steering_rate"] / mpc["s_steering_rate"] ** 2])
        Qe = Q if Qe is None else Qe
        L1 = mpc["L1_pen"] if L1 is None else L1
        L2 = mpc["L2_pen"] if L2 is None else L2
        N = self.N
        W = np.zeros((6, 6)); W[:4, :4] = Q; W[4:, 4:] = R
        self.cost_set(ALL_STAGES, "W", w_scale * W)          # the same W on every stage < N (per-stage: cost_set(i, "W", ...))
        self.cost_set(N, "W", w_scale * np.asarray(Qe))
        classes = ((0, 1), (1, 3), (N, 2)) if N > 1 else ((0, 1), (N, 2))
        for st, n in classes:                        # one representative stage per penalty class
            for f, val in (("zl", L1), ("zu", L1), ("Zl", L2), ("Zu", L2)):
                self.cost_set(st, f, np.ones(n) * val)
        for k in range(N):
            self.constraints_set(k, "lbu", np.array([veh["delta_f_dot_min"]]))
            self.constraints_set(k, "ubu", np.array([veh["delta_f_dot_max"]]))
        for k in range(1, N + 1):
            self.constraints_set(k, "lbx", np.array([veh["delta_f_min"]]))
            self.constraints_set(k, "ubx", np.array([veh["delta_f_max"]]))
            self.constraints_set(k, "lh", np.array([0.0]))
            self.constraints_set(k, "uh", np.array([1.0]))


class CoupledSnmpcSolver(BatchedOcpSolver):
    """`batch` copies of the reference's coupled SNMPC OCP: what
    Stochastic_NMPC/SNMPC_acados_settings.py:318 builds and SNMPC_class.py:198 solves, acados method names.

    The stacked state is the nominal copy followed by n_s sample copies (nx = 8 (n_s+1)). `Apce` (L x n_s) and `uph`
    stand for the per-stage parameter vector p = [A_pce.flatten(), risk_parameter, stop_flag]; set(stage, "p", ...)
    is accepted and checked against them (the reference re-sends the same p before every solve, SNMPC_class.py:184-193).
    """

    def __init__(self, N=38, dt=0.08, batch=1, Apce=None, uph=5, gamma=0.8, device=0, cfg=None,
                 qp_iter_max=50, qp_tol=(1e-8, 1e-8, 1e-8), qp_mu0=0.05, qp_t0=0.05, x0_offsets=None, qp_warm_start=None, qp_warm_mu=0.0,
                 qp_warm_flips=0, qp_warm_viol=0.0):
        super().__init__(N=N, dt=dt, nsub=1, batch=batch, device=device, cfg=cfg, qp_iter_max=qp_iter_max,
                         qp_tol=qp_tol, qp_mu0=qp_mu0, qp_t0=qp_t0, qp_warm_start=qp_warm_start, qp_warm_mu=qp_warm_mu,
                         qp_warm_flips=qp_warm_flips, qp_warm_viol=qp_warm_viol)
        self.Apce = np.ascontiguousarray(Apce, dtype=np.float64)
        if self.Apce.ndim != 2:
            raise Exception("CoupledSnmpcSolver: Apce must be (num_poly_terms, n_samples)")
        self.L, self.ns = self.Apce.shape
        self.uph, self.gamma = int(uph), float(gamma)
        self.nx = 8 * (self.ns + 1)
        self._chk(self._L.tum_ocp_snmpc_attach(self._h, self.ns, self.L, _dp(self.Apce), self.uph, self.gamma), "snmpc_attach")
        if x0_offsets is not None:
            self.set_x0_offsets(x0_offsets)

    def set_x0_offsets(self, offsets):
        """(n_s, 8) offsets of the sample initial conditions (stds * w_s): afterwards set_x0 / constraints_set(0, 'lbx', x0)
        with the 8 nominal values fan out to the samples on the device (compute_x0dist as a kernel)."""
        o = np.ascontiguousarray(offsets, dtype=np.float64)
        if o.shape != (self.ns, 8):
            raise Exception(f"CoupledSnmpcSolver.set_x0_offsets: expected shape ({self.ns}, 8)")
        self._chk(self._L.tum_ocp_snmpc_set_offsets(self._h, _dp(o)), "set_x0_offsets")

    def set(self, stage, field, value):
        if field == "p":
            # [A_pce.flatten(), risk_parameter, stop_flag] (SNMPC_class.py:124,185,193): handled by the C-ABI -- A_pce and the
            # risk parameter are shared by all stages, the stop flags define the uncertainty propagation horizon of the
            # next solve (include/tum_nmpc.h, tum_ocp_set)
            v = np.ascontiguousarray(value, dtype=np.float64).reshape(-1)
            if v.size != self.L * self.ns + 2:
                raise Exception(f"CoupledSnmpcSolver.set: mismatching dimension for field \"p\" with dimension "
                                f"{self.L * self.ns + 2} (you have {v.size})")
            self._chk(self._L.tum_ocp_set(self._h, int(stage), b"p", v.ctypes.data, v.size, 0, self.batch, 0), "set")
            return
        super().set(stage, field, value)

    def options_set(self, field, value):
        if field == "rti_phase" and _rti_phase_value(value) != 0:
            raise Exception("CoupledSnmpcSolver.options_set: the split real-time iteration (rti_phase 1 / 2) is not available for the coupled "
                            "SNMPC OCP: its prologue and epilogue kernels read x0 themselves")
        super().options_set(field, value)

    def get(self, stage, field):
        if field == "x":
            out = np.zeros((self.batch, self.nx))
            self._chk(self._L.tum_ocp_get(self._h, stage, b"x", out.ctypes.data, self.nx, 0, self.batch, self.nx), "get")
            return self._out(out)
        return super().get(stage, field)

    def get_from_qp_in(self, stage, field):
        raise Exception("CoupledSnmpcSolver.get_from_qp_in: not available for the stacked state")

    def get_snmpc_linearisation(self, b0=0, nb=None):
        """The linearisation of the instances b0 .. b0 + nb - 1 as the last pipeline solve left it (read-only, launches nothing): dict with
        As (nb, uph, ns, 8, 8), Bs (nb, uph, ns, 8, 2), bs (nb, uph, ns, 8), the gg values hs (nb, uph, ns) and gradients ghs (nb, uph, ns, 8)
        of the sample copies of the stages below the uncertainty propagation horizon (zeros at stage 0); hn (nb, N + 1), ghn (nb, N + 1, 8) and
        the speed row's gradient cv (nb, N + 1, 2) of the nominal copy of every stage; An (nb, N - uph, 8, 8), Bn, bn of its stages >= uph."""
        nb = self.batch - b0 if nb is None else int(nb)
        info = (ctypes.c_int * 3)()
        null = ctypes.POINTER(ctypes.c_double)()
        self._chk(self._L.tum_ocp_get_snmpc_linearisation(self._h, int(b0), nb, *([null] * 11), info), "get_snmpc_linearisation")
        ns, uph, N = int(info[0]), int(info[1]), int(info[2])
        shapes = dict(As=(nb, uph, ns, 8, 8), Bs=(nb, uph, ns, 2, 8), bs=(nb, uph, ns, 8), hs=(nb, uph, ns), ghs=(nb, uph, ns, 8),
                      hn=(nb, N + 1), ghn=(nb, N + 1, 8), cv=(nb, N + 1, 2), An=(nb, N - uph, 8, 8), Bn=(nb, N - uph, 2, 8), bn=(nb, N - uph, 8))
        out = {k: np.zeros(v) for k, v in shapes.items()}
        self._chk(self._L.tum_ocp_get_snmpc_linearisation(self._h, int(b0), nb, *[_dp(out[k]) for k in shapes], info), "get_snmpc_linearisation")
        for k in ("As", "Bs", "An", "Bn"):      # the C-ABI hands matrices out column-major (acados convention)
            out[k] = np.ascontiguousarray(np.swapaxes(out[k], -1, -2))
        return out


def planner_emulate(track, poses, n_points, Tp, loop_circuit=True, device=0):
    """Batched PlannerEmulator on the GPU (Utils/MPC_sim_utils.py:137-194): track (n,4) [x,y,yaw,v], poses (P,2).
    Returns (closest_index (P,), ref (P, n_points, 4))."""
    L = load_library()
    track = np.ascontiguousarray(track, dtype=np.float64); poses = np.ascontiguousarray(np.atleast_2d(poses), dtype=np.float64)
    if track.ndim != 2 or track.shape[1] != 4 or poses.shape[1] != 2:
        raise Exception("planner_emulate: track must be (n,4), poses (P,2)")
    P = poses.shape[0]
    ref = np.empty((P, n_points, 4)); idx = np.empty(P, dtype=np.int32)
    rc = L.tum_planner_emulate(_dp(track), track.shape[0], _dp(poses), P, int(n_points), float(Tp), int(bool(loop_circuit)),
                               _dp(ref), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(device))
    if rc != 0:
        raise Exception("planner_emulate: " + L.tum_ocp_last_error().decode())
    return idx, ref


def track_set(tracks, track_of, count, track_rows=None):
    """A track set as the C-ABI takes it (tum_sim_create_tracks, tum_planner_emulate_tracks), checked on the host: `tracks` a sequence
    of (n_t, 4) tables -- or, with track_rows, ONE table of all of them one behind the other and its n_tracks + 1 ascending row offsets
    (0 first, at least 2 rows per track); track_of: `count` track ids in 0 .. n_tracks - 1 in any order (None: i % n_tracks).
    Returns (table (sum n_t, 4) float64, track_rows (n_tracks + 1,) int32, track_of (count,) int32)."""
    if track_rows is None:
        tabs = [np.asarray(t, dtype=np.float64) for t in tracks]
        if not tabs or any(t.ndim != 2 or t.shape[1] != 4 for t in tabs):
            raise ValueError("track_set: tracks is a non-empty sequence of (n, 4) tables")
        table = np.ascontiguousarray(np.concatenate(tabs))
        rows = np.concatenate([[0], np.cumsum([len(t) for t in tabs])])
    else:
        table = np.ascontiguousarray(tracks, dtype=np.float64)
        rows = np.asarray(track_rows)
        if table.ndim != 2 or table.shape[1] != 4:
            raise ValueError("track_set: with track_rows, tracks is one (sum n_t, 4) table")
        if rows.ndim != 1 or len(rows) < 2 or not np.issubdtype(rows.dtype, np.integer) or rows[0] != 0 or rows[-1] != len(table):
            raise ValueError("track_set: track_rows is n_tracks + 1 integer offsets from 0 to the length of the table")
    if (np.diff(rows) < 2).any():
        raise ValueError("track_set: track_rows must ascend and every track needs at least 2 rows")
    T = len(rows) - 1
    if track_of is None:
        track_of = np.arange(int(count)) % T
    of = np.asarray(track_of)
    if of.shape != (int(count),) or not np.issubdtype(of.dtype, np.integer):
        raise ValueError(f"track_set: track_of is one integer track id per instance ({int(count)})")
    if ((of < 0) | (of >= T)).any():
        raise ValueError(f"track_set: track_of holds ids outside 0..{T - 1}")
    return table, np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(of, dtype=np.int32)


def planner_emulate_tracks(tracks, track_of, poses, n_points, Tp, loop_circuit=True, device=0, track_rows=None):
    """planner_emulate on a track set (track_set): pose p is planned on tracks[track_of[p]], its index is local to that track.
    Returns (closest_index (P,), ref (P, n_points, 4))."""
    L = load_library()
    poses = np.ascontiguousarray(np.atleast_2d(poses), dtype=np.float64)
    if poses.shape[1] != 2:
        raise Exception("planner_emulate_tracks: poses (P,2)")
    P = poses.shape[0]
    table, rows, of = track_set(tracks, track_of, P, track_rows)
    ref = np.empty((P, n_points, 4)); idx = np.empty(P, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = L.tum_planner_emulate_tracks(_dp(table), rows.ctypes.data_as(ip), len(rows) - 1, of.ctypes.data_as(ip), _dp(poses), P, int(n_points),
                                      float(Tp), int(bool(loop_circuit)), _dp(ref), idx.ctypes.data_as(ip), int(device))
    if rc != 0:
        raise Exception("planner_emulate_tracks: " + L.tum_ocp_last_error().decode())
    return idx, ref


class DeviceClosedLoop:
    """Closed loops of every instance of a solver kept on the GPU: planner -> SQP-RTI -> plant + estimator
    (main.py:48-78, SimulationMode_main_class.py:106-156). The logs use the reference's npz field names.
    One race line `track` (n, 4) for all instances, or (track=None) a track set: tracks, a sequence of (n_t, 4) tables, and track_of,
    the track of every instance (None: i % n_tracks) -- every index of an instance is then local to its own track (track_set)."""

    def __init__(self, solver, track, Tp, Ts=0.02, n_elem=4, windows=(1, 1, 4, 2, 2, 3, 4, 2), loop_circuit=True, log_capacity=0,
                 tracks=None, track_of=None):
        self.solver, self._L = solver, solver._L
        win = (ctypes.c_int * 8)(*[int(w) for w in windows])
        if tracks is None:
            if track_of is not None:
                raise ValueError("DeviceClosedLoop: track_of goes with tracks=[...]")
            track = np.ascontiguousarray(track, dtype=np.float64)
            self.track_rows, self.track_of = np.array([0, track.shape[0]]), np.zeros(solver.batch, dtype=np.int64)
            self._s = self._L.tum_sim_create(solver._h, _dp(track), track.shape[0], float(Tp), int(bool(loop_circuit)), float(Ts),
                                             int(n_elem), win, int(log_capacity))
        else:
            if track is not None:
                raise ValueError("DeviceClosedLoop: one track or tracks=[...], not both")
            table, rows, of = track_set(tracks, track_of, solver.batch)
            ip = ctypes.POINTER(ctypes.c_int)
            self.track_rows, self.track_of = rows.astype(np.int64), of.astype(np.int64)
            self._s = self._L.tum_sim_create_tracks(solver._h, _dp(table), rows.ctypes.data_as(ip), len(rows) - 1, of.ctypes.data_as(ip), float(Tp),
                                                    int(bool(loop_circuit)), float(Ts), int(n_elem), win, int(log_capacity))
        if not self._s:
            raise Exception("tum_sim_create: " + self._L.tum_ocp_last_error().decode())
        self.B = solver.batch
        self.log_capacity = int(log_capacity)

    def __del__(self):
        if getattr(self, "_s", None):
            self._L.tum_sim_free(self._s); self._s = None

    def _chk(self, rc, what):
        if rc != 0:
            raise Exception(f"{what}: " + self._L.tum_ocp_last_error().decode())

    def set_state(self, x_sim, x_mpc, cold_start=True):
        x_sim = np.ascontiguousarray(np.broadcast_to(x_sim, (self.B, 7)), dtype=np.float64)
        x_mpc = np.ascontiguousarray(np.broadcast_to(x_mpc, (self.B, 8)), dtype=np.float64)
        self._chk(self._L.tum_sim_set_state(self._s, _dp(x_sim), _dp(x_mpc), int(cold_start)), "sim_set_state")

    def set_disturbances(self, w_deriv=None, e_est=None):
        """disturbance realisation played back by the loop: (n_steps, B, 7) additive disturbances of the state derivatives and / or
        (n_steps, B, 7) state estimation errors (closed_loop.DisturbanceModel.draw); both None: none"""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (w_deriv, e_est)]
        n = 0
        for a in arrs:
            if a is not None:
                if a.ndim != 3 or a.shape[1:] != (self.B, 7) or (n and a.shape[0] != n):
                    raise Exception("DeviceClosedLoop.set_disturbances: expected (n_steps, batch, 7) arrays of equal length")
                n = a.shape[0]
        if n:
            self.disturbance_streams = (False, False)          # (a table takes an attached generator's place)
        self._chk(self._L.tum_sim_set_disturbances(self._s, None if arrs[0] is None else _dp(arrs[0]), None if arrs[1] is None else _dp(arrs[1]), n),
                  "sim_set_disturbances")

    DIST_KINDS = dict(uniform=1, gaussian=2, absolute=3)          # (anything else: 4, the box -- generate_disturbances' last branch)

    def attach_disturbances(self, model, seed=0):
        """Draw the realisation ON THE DEVICE from now on, one launch per control step (disturbance_draw_kernel): `model` a
        closed_loop.DisturbanceModel -- its switches, kinds and magnitudes --, `seed` the key of the counter-based draws
        (DisturbanceModel.draw_counter is the host statement; include/tum_nmpc.h the definition). Removes a played-back table;
        model=None (or a model with both switches off) detaches. The attached streams are kept in .disturbance_streams."""
        on = [False, False] if model is None else [bool(model.derivatives), bool(model.state_estimation)]
        kinds = [self.DIST_KINDS.get(model.types[q], 4) if on[q] else 0 for q in range(2)]
        bounds = [None, None]
        if model is not None:
            bounds = [np.ascontiguousarray(np.asarray(b, dtype=np.float64)[:, 1]) for b in (model.bounds_derivatives, model.bounds_state_estimation)]
        self._chk(self._L.tum_sim_disturbances_attach(self._s, kinds[0], None if not on[0] else _dp(bounds[0]), kinds[1],
                                                      None if not on[1] else _dp(bounds[1]), int(seed) & (2 ** 64 - 1)), "sim_disturbances_attach")
        self.disturbance_streams = tuple(on)

    def disturbance_table(self, first_step, n_steps):
        """(w_deriv, e_est) of the control steps first_step .. first_step + n_steps - 1 as the attached generator draws them:
        (n_steps, B, 7) arrays, None for a stream that is off -- what set_disturbances plays back. Regenerated on the device by the
        function the live draw uses (equal to the bit); the loop is not touched."""
        on = getattr(self, "disturbance_streams", (False, False))
        out = [np.empty((int(n_steps), self.B, 7)) if f else None for f in on]
        self._chk(self._L.tum_sim_disturbances_table(self._s, int(first_step), int(n_steps), None if out[0] is None else _dp(out[0]),
                                                     None if out[1] is None else _dp(out[1])), "sim_disturbances_table")
        return out[0], out[1]

    def plan(self):
        self._chk(self._L.tum_sim_plan(self._s), "sim_plan")

    def advance(self):
        self._chk(self._L.tum_sim_advance(self._s), "sim_advance")

    def run(self, nsteps):
        self._chk(self._L.tum_sim_run(self._s, int(nsteps)), "sim_run")

    @property
    def steps(self):
        return self._L.tum_sim_steps(self._s)

    _DIMS = dict(x_sim=7, x_mpc=8, pose=2, ref0=4, closest=1, CiLX=7, MPC_SimX=8, simU=2, simREF=4, simSolverDebug=5)

    def get(self, field):
        if field in ("track_of", "track_rows"):          # the loop's track set as the library holds it (one track: zeros, [0, n])
            out = np.empty(self.B if field == "track_of" else len(self.track_rows))
            self._chk(self._L.tum_sim_get(self._s, field.encode(), _dp(out), out.size), "sim_get " + field)
            return out.astype(np.int64)
        if field == "yref":          # the reference window of the last planned control step: (B, N + 1, 6)
            out = np.empty((self.B, self.solver.N + 1, 6))
            self._chk(self._L.tum_sim_get(self._s, b"yref", _dp(out), out.size), "sim_get yref")
            return out
        d = self._DIMS[field]
        if field in ("x_sim", "x_mpc", "pose", "ref0", "closest"):
            shape = (self.B, d)
        else:
            if self.log_capacity == 0:
                raise Exception(f"DeviceClosedLoop.get('{field}'): created with log_capacity=0 (no logs kept on the device)")
            n = min(self.steps, self.log_capacity) + (1 if field in ("CiLX", "MPC_SimX") else 0)   # the first log_capacity steps
            shape = (n, self.B, d)
        out = np.empty(shape)
        self._chk(self._L.tum_sim_get(self._s, field.encode(), _dp(out), out.size), "sim_get " + field)
        return out[:, 0].astype(np.int64) if field == "closest" else out

    @property
    def graph_steps(self):
        out = np.zeros(1)
        self._chk(self._L.tum_sim_get(self._s, b"graph_steps", _dp(out), 1), "sim_get graph_steps")
        return int(out[0])

    def logs(self):
        return {k: self.get(k) for k in ("CiLX", "MPC_SimX", "simU", "simREF", "simSolverDebug")}

    # ---- track segments: what a weight sweep runs the loop for (BO_WMPC/objective_function.py:57-200)
    SEG_DONE, SEG_CRASH_LAT, SEG_CRASH_ACOMB = 1, 2, 4          # bits of a segment's state word (0: active)

    def attach_segments(self, end_idx, max_lat_dev, max_a_comb, group_offsets=None):
        """Score every instance on its own track segment from now on: end_idx (B,) planner index that ends it (< 0: never),
        crash thresholds of the signed lateral deviation and of the combined acceleration (inf: no test), group_offsets
        (n_groups + 1,) contiguous groups of instances for segment_groups() (None: one group per instance)."""
        end = np.ascontiguousarray(np.broadcast_to(end_idx, (self.B,)), dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        off, ng = None, 0
        if group_offsets is not None:
            off = np.ascontiguousarray(group_offsets, dtype=np.int32).reshape(-1)
            ng = len(off) - 1
        self._chk(self._L.tum_sim_segments_attach(self._s, end.ctypes.data_as(ip), None if off is None else off.ctypes.data_as(ip), ng,
                                                  float(max_lat_dev), float(max_a_comb)), "sim_segments_attach")
        self.n_groups = ng if off is not None else self.B

    def detach_segments(self):
        self._chk(self._L.tum_sim_segments_attach(self._s, None, None, 0, 0.0, 0.0), "sim_segments_attach")
        self.n_groups = 0

    def run_segments(self, max_steps, check_every=0):
        """run() in chunks of check_every steps (0: 100) until every segment is done or crashed, or max_steps have run"""
        self._chk(self._L.tum_sim_run_segments(self._s, int(max_steps), int(check_every)), "sim_run_segments")

    def _seg_get(self, field, n):
        out = np.empty(n)
        self._chk(self._L.tum_sim_get(self._s, field.encode(), _dp(out), out.size), "sim_get " + field)
        return out

    @property
    def segments_active(self):
        return int(self._seg_get("seg_active", 1)[0])

    def segments(self):
        """Per-instance scores: steps, state, max_lat_dev (max |lat_dev|), rms_vel_dev, max_a_comb, qp_failures, and the booleans
        derived from the state word -- crashed (any crash bit; wins over done), done, timed_out (still active)."""
        B = self.B
        d = {k: self._seg_get("seg_" + k, B) for k in ("max_lat_dev", "rms_vel_dev", "max_a_comb")}
        for k in ("steps", "state", "qp_failures"):
            d[k] = self._seg_get("seg_" + k, B).astype(np.int64)
        d.update(segment_flags(d["state"]))
        return d

    def segment_groups(self):
        """(n_groups, 4): mean of -max|lat_dev|, mean of -rms(vel_dev), segments, segments not cleanly done (crashed or active)"""
        return self._seg_get("seg_groups", 4 * self.n_groups).reshape(self.n_groups, 4)

    # ---- the weight-scheduling RL environment (RL_WMPC/environment.py:112-240)
    ENV_HEAD = 6          # reward, terminated, truncated, step_length, qp_failures, planner error word; then the observation
    _OBS_STATES = {"reference": 0, "last_step": 1}

    def attach_env(self, table, n_mpc_steps, max_lat_dev, episode_length, sigmas, lims, n_samples=10, full_lap=False,
                   obs_states="reference", obs_bounds=None):
        """Turn the loop into the reference's RL environment: `table` (A, 7) rows [q_xy, q_yaw, q_vel, r_jerk, r_steer, L1, L2] an
        agent picks from every n_mpc_steps control steps; sigmas (2,) and lims (lims[0] lower, lims[1] upper, broadcast over
        [lat_dev, vel_dev] as reward.py does) of the reward; n_samples anticipation points of the observation; obs_states
        "reference" (first two observation entries 0 before normalisation, as the reference computes them) or "last_step";
        obs_bounds (2, 2 + 2 n_samples) lower / upper (None: observation.py:16-24)."""
        if obs_states not in self._OBS_STATES:
            raise Exception("attach_env: obs_states must be 'reference' or 'last_step'")
        N, n = self.solver.N, int(n_samples)
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 7:
            raise Exception("attach_env: table must be (n_actions, 7)")
        if N < 10 or n < 1:
            raise Exception("attach_env: the observation's 10-tap moving average of the yaw rate needs N >= 10 (and n_samples >= 1)")
        lims = np.asarray(lims, dtype=np.float64)
        lo_hi = np.ascontiguousarray(np.concatenate([np.broadcast_to(lims[0], (2,)), np.broadcast_to(lims[1], (2,))]))
        sig = np.ascontiguousarray(np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (2,)))
        if obs_bounds is None:
            obs_bounds = env_observation_bounds(n)
        ob = np.ascontiguousarray(obs_bounds, dtype=np.float64).reshape(2, 2 + 2 * n)
        # observation.py:58-59: the sample indices into ref_v (N + 1 points) and into the averaged yaw rate (N - 9 points)
        iv = np.ascontiguousarray(np.linspace(0, N, n, dtype=int), dtype=np.int32)
        ir = np.ascontiguousarray(np.linspace(0, N - 10, n, dtype=int), dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        self._chk(self._L.tum_sim_env_attach(self._s, _dp(table), table.shape[0], int(n_mpc_steps), float(max_lat_dev), int(episode_length),
                                             int(bool(full_lap)), _dp(sig), _dp(lo_hi), _dp(ob[0]), _dp(ob[1]), iv.ctypes.data_as(ip),
                                             ir.ctypes.data_as(ip), n, self._OBS_STATES[obs_states]), "sim_env_attach")
        self.env_n_obs = 2 + 2 * n
        self.policy_widths = self.value_widths = None          # (attaching an environment detaches the policy of the one before)

    def detach_env(self):
        self._chk(self._L.tum_sim_env_attach(self._s, None, 0, 0, 0.0, 0, 0, None, None, None, None, None, None, 0, 0), "sim_env_attach")
        self.env_n_obs = 0
        self.policy_widths = self.value_widths = None

    def _ints(self, a):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a), (self.B,)))
        if not (np.issubdtype(a.dtype, np.integer) or a.dtype == bool):
            raise Exception("env: actions, masks and start indices are integers")
        return np.ascontiguousarray(a, dtype=np.int32)

    def env_reset(self, start_idx, mask=None):
        """environment.py:191-237 for the instances of `mask` (None: all): plant and controller at waypoint start_idx[b], empty
        estimator, cold iterate, episode counters 0. The rest of the batch is untouched."""
        ip = ctypes.POINTER(ctypes.c_int)
        st = self._ints(start_idx)
        m = None if mask is None else self._ints(mask)
        self._chk(self._L.tum_sim_env_reset(self._s, None if m is None else m.ctypes.data_as(ip), st.ctypes.data_as(ip)), "sim_env_reset")

    def env_step(self, actions, reset_mask=None, start_idx=None):
        """One environment step of every instance (environment.py:112-189): reset_mask[b] 1 resets instance b to start_idx[b] first,
        2 lets an instance whose episode has ended drive on without a reset (episode_steps keeps counting), 0 neither -- an error
        if its episode has ended. Returns a dict of batched arrays: reward, terminated, truncated, step_length, qp_failures,
        observation (B, 2 + 2 n_samples)."""
        ip = ctypes.POINTER(ctypes.c_int)
        act = self._ints(actions)
        m = None if reset_mask is None else self._ints(reset_mask)
        st = None if start_idx is None else self._ints(start_idx)
        out = np.empty((self.B, self.ENV_HEAD + getattr(self, "env_n_obs", 0)))
        self._chk(self._L.tum_sim_env_step(self._s, act.ctypes.data_as(ip), None if m is None else m.ctypes.data_as(ip),
                                           None if st is None else st.ctypes.data_as(ip), _dp(out)), "sim_env_step")
        return dict(reward=out[:, 0].copy(), terminated=out[:, 1] != 0, truncated=out[:, 2] != 0, step_length=out[:, 3].astype(np.int64),
                    qp_failures=out[:, 4].astype(np.int64), observation=out[:, self.ENV_HEAD:].copy())

    def env_get(self, field):
        """per-instance integers of the environment: episode_steps, step_length, flags, qp_failures, samples, ended"""
        out = np.empty(self.B)
        self._chk(self._L.tum_sim_get(self._s, ("env_" + field).encode(), _dp(out), out.size), "sim_get env_" + field)
        return out.astype(np.int64)

    # ---- the agent of the environment (enable_WMPC of the controller classes, RL_WMPC/evaluation.py:65-105)
    @staticmethod
    def _net(weights, biases, who):
        """(widths, pointer arrays, the arrays they point into) of a float32 net for the attach calls"""
        Ws = [np.ascontiguousarray(w) for w in weights]
        bs = [np.ascontiguousarray(b) for b in biases]
        if len(Ws) != len(bs) or len(Ws) < 1:
            raise Exception(who + ": one bias per weight matrix")
        for w, b in zip(Ws, bs):
            if w.dtype != np.float32 or b.dtype != np.float32 or w.ndim != 2 or b.shape != (w.shape[0],):
                raise Exception(who + ": weights are float32 (out, in) matrices, biases float32 (out,) vectors")
        for w0, w1 in zip(Ws, Ws[1:]):
            if w1.shape[1] != w0.shape[0]:
                raise Exception(who + ": the layers do not chain")
        widths = np.array([Ws[0].shape[1]] + [w.shape[0] for w in Ws], dtype=np.int32)
        pw = (ctypes.c_void_p * len(Ws))(*[w.ctypes.data for w in Ws])
        pb = (ctypes.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
        return widths, pw, pb, (Ws, bs)

    def attach_policy(self, policy):
        """The policy net that picks the environment's actions on the device: `policy` has .weights / .biases, lists of float32 arrays
        (out, in) / (out,) -- closed_loop.WeightPolicy. 1 to 4 hidden layers up to 256 wide, tanh, up to 128 inputs and 64 actions; its
        input width is the environment's observation, its action count the rows of the environment's table. A policy that carries a
        value net (.value_weights / .value_biases) brings it along (attach_value); one that does not leaves none attached."""
        widths, pw, pb, _keep = self._net(policy.weights, policy.biases, "attach_policy")
        self._chk(self._L.tum_sim_policy_attach(self._s, len(pw), widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), pw, pb), "sim_policy_attach")
        self.policy_widths = tuple(int(w) for w in widths)
        self.value_widths = None          # (attaching a policy detaches the value net of the one before)
        if getattr(policy, "value_weights", None) is not None:
            self.attach_value(policy.value_weights, policy.value_biases)

    def detach_policy(self):
        """(an attached weight schedule goes with it)"""
        self._chk(self._L.tum_sim_policy_attach(self._s, 0, None, None, None), "sim_policy_attach")
        self.policy_widths = self.value_widths = None

    # ---- the learned weight schedule inside the loop (enable_WMPC of the controller classes)
    _ON_FAILURE = {"keep": 0, "base": 1}

    def attach_wmpc(self, table, period=20, on_failure="base", n_samples=10, log_capacity=0, obs_bounds=None):
        """Let the attached policy (attach_policy) replace the cost weights inside the loop, as enable_WMPC does in the reference's
        controller classes: per instance a counter c, 0 now; after the solve of every control step `if c >= period: c = 0, decide,
        install`, then c += 1 (closed_loop.WmpcSchedule is the host statement). The observation is closed_loop.wmpc_observation of the
        state the solve started at and the step's reference window, the row installed is table[action] ((A, 7), as attach_env takes
        it). on_failure "base": an instance whose solve failed gets back the weights the loop holds NOW (the reference builds a fresh
        solver from the YAML weights; a row decided at that step is lost); "keep": nothing. log_capacity: decisions stored per instance
        (wmpc_get). Runs on nominal, SNMPC and R2 loops, inside captured chunks, beside segments and drawn disturbances."""
        if on_failure not in self._ON_FAILURE:
            raise Exception("attach_wmpc: on_failure must be 'base' or 'keep'")
        N, n = self.solver.N, int(n_samples)
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 7:
            raise Exception("attach_wmpc: table must be (n_actions, 7)")
        if N < 10 or n < 1:
            raise Exception("attach_wmpc: the observation's 10-tap moving average of the yaw rate needs N >= 10 (and n_samples >= 1)")
        if obs_bounds is None:
            obs_bounds = env_observation_bounds(n)
        ob = np.ascontiguousarray(obs_bounds, dtype=np.float64).reshape(2, 2 + 2 * n)
        iv = np.ascontiguousarray(np.linspace(0, N, n, dtype=int), dtype=np.int32)
        ir = np.ascontiguousarray(np.linspace(0, N - 10, n, dtype=int), dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        self._chk(self._L.tum_sim_wmpc_attach(self._s, _dp(table), table.shape[0], int(period), self._ON_FAILURE[on_failure], n,
                                              iv.ctypes.data_as(ip), ir.ctypes.data_as(ip), _dp(ob[0]), _dp(ob[1]), int(log_capacity)), "sim_wmpc_attach")
        self.wmpc_log_capacity, self.wmpc_n_obs = int(log_capacity), 2 + 2 * n

    def detach_wmpc(self):
        """the loop goes on as a plain loop with the weights last installed"""
        self._chk(self._L.tum_sim_wmpc_attach(self._s, None, 0, 0, 0, 0, None, None, None, None, 0), "sim_wmpc_attach")

    def wmpc_get(self, field):
        """of the attached schedule: counter, n_decisions (B,) ints; steps, actions (B, log_capacity) ints, -1 where none; observations
        (B, log_capacity, n_obs); base_W / W (B, N + 1, 6) the diagonal of W per stage at attach time / now (stage N: its first four
        entries); base_pen / pen (B, 36) the slack penalties"""
        B, N, L, no = self.B, self.solver.N, getattr(self, "wmpc_log_capacity", 0), getattr(self, "wmpc_n_obs", 0)
        shapes = dict(counter=(B,), n_decisions=(B,), steps=(B, L), actions=(B, L), observations=(B, L, no),
                      base_W=(B, N + 1, 6), W=(B, N + 1, 6), base_pen=(B, 36), pen=(B, 36))
        if field not in shapes:
            raise Exception(f"wmpc_get: unknown field '{field}'")
        out = np.zeros(shapes[field])
        self._chk(self._L.tum_sim_wmpc_get(self._s, field.encode(), _dp(out), out.size), "sim_wmpc_get " + field)
        return out.astype(np.int64) if field in ("counter", "n_decisions", "steps", "actions") else out

    # ---- collecting PPO training rollouts (stable_baselines3 collect_rollouts + compute_returns_and_advantage)
    COLLECT_FIELDS = ("actions", "values", "log_probs", "rewards", "rewards_raw", "episode_starts", "advantages", "returns",
                      "terminated", "truncated", "step_length", "qp_failures", "planner_error")          # TUM_COLLECT_* of tum_nmpc.h

    def attach_value(self, weights, biases):
        """The value net beside the attached policy: float32 (out, in) matrices / (out,) vectors, its own 1 to 4 hidden layers up to
        256 wide, the policy's inputs, one output."""
        widths, pw, pb, _keep = self._net(weights, biases, "attach_value")
        self._chk(self._L.tum_sim_policy_attach_value(self._s, len(pw), widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), pw, pb),
                  "sim_policy_attach_value")
        self.value_widths = tuple(int(w) for w in widths)

    def detach_value(self):
        self._chk(self._L.tum_sim_policy_attach_value(self._s, 0, None, None, None), "sim_policy_attach_value")
        self.value_widths = None

    def policy_eval_ac(self, obs, seed, t, first_instance=0, values=None):
        """the attached nets and ONE draw per row on (n, n_obs) observations, independent of the loop's batch: dict of actions (n,)
        sampled with the uniform of (seed, first_instance + i, t), log_probs, uniforms and -- with a value net attached (values=None) or
        asked for (values=True: an error without one) -- values"""
        w = getattr(self, "policy_widths", None)
        if not w:
            raise Exception("policy_eval_ac: no policy attached (attach_policy)")
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != w[0] or obs.shape[0] < 1:
            raise Exception(f"policy_eval_ac: observations are (n, {w[0]}), n >= 1")
        n = obs.shape[0]
        want_v = bool(getattr(self, "value_widths", None)) if values is None else bool(values)
        act, val, lp, u = np.empty(n, dtype=np.int32), np.empty(n), np.empty(n), np.empty(n)
        self._chk(self._L.tum_sim_policy_eval_ac(self._s, _dp(obs), n, int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1), int(first_instance) & 0xffffffff,
                                                 act.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(val) if want_v else None, _dp(lp), _dp(u)),
                  "sim_policy_eval_ac")
        out = dict(actions=act.astype(np.int64), log_probs=lp, uniforms=u)
        if want_v:
            out["values"] = val
        return out

    def gae(self, rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
        """gae_kernel alone on (E, B) host arrays: (advantages, returns)"""
        r = np.ascontiguousarray(rewards, dtype=np.float64)
        if r.ndim != 2 or r.size < 1:
            raise Exception("gae: rewards, values and episode_starts are (E, B)")
        E, B = r.shape
        v, es = (np.ascontiguousarray(a, dtype=np.float64) for a in (values, episode_starts))
        lv, ld = (np.ascontiguousarray(a, dtype=np.float64) for a in (last_values, last_dones))
        if v.shape != (E, B) or es.shape != (E, B) or lv.shape != (B,) or ld.shape != (B,):
            raise Exception("gae: rewards, values and episode_starts are (E, B), last_values and last_dones (B,)")
        adv, ret = np.empty((E, B)), np.empty((E, B))
        self._chk(self._L.tum_sim_gae(self._s, E, B, _dp(r), _dp(v), _dp(es), _dp(lv), _dp(ld), float(gamma), float(gae_lambda), _dp(adv), _dp(ret)), "sim_gae")
        return adv, ret

    def env_collect(self, n_env_steps, start_table, seed, t0, gamma, gae_lambda, first_obs=None, first_episode_starts=None):
        """n_env_steps environment steps with SAMPLED actions and everything a RolloutBuffer holds after collect_rollouts and
        compute_returns_and_advantage, one wait at the end (tum_sim_env_collect). Returns a dict of (E, B) arrays named as
        COLLECT_FIELDS (without planner_error), observations (E, B, n_obs), last_values and last_dones (B,), and next_observation
        (B, n_obs): what the policy would see next."""
        ip = ctypes.POINTER(ctypes.c_int)
        E, B, no = int(n_env_steps), self.B, getattr(self, "env_n_obs", 0)
        if E < 1:
            raise Exception("env_collect: n_env_steps < 1")
        fo = fs = None
        if first_obs is not None:
            fo = np.ascontiguousarray(first_obs, dtype=np.float64)
            if fo.shape != (B, no):
                raise Exception(f"env_collect: first_obs is ({B}, {no})")
        if first_episode_starts is not None:
            fs = np.ascontiguousarray(first_episode_starts, dtype=np.float64)
            if fs.shape != (B,):
                raise Exception(f"env_collect: first_episode_starts is ({B},)")
        tab = np.asarray(start_table)
        if tab.shape != (E, B) or not np.issubdtype(tab.dtype, np.integer):
            raise Exception(f"env_collect: start_table is an integer array ({E}, {B})")
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        F = len(self.COLLECT_FIELDS)
        out = np.zeros(E * B * (F + no) + 2 * B + B * no)
        self._chk(self._L.tum_sim_env_collect(self._s, E, None if fo is None else _dp(fo), None if fs is None else _dp(fs), tab.ctypes.data_as(ip),
                                              int(seed) & (2 ** 64 - 1), int(t0) & (2 ** 64 - 1), float(gamma), float(gae_lambda), _dp(out)),
                  "sim_env_collect")
        f = out[:F * E * B].reshape(F, E, B)
        r = {k: f[i].copy() for i, k in enumerate(self.COLLECT_FIELDS) if k != "planner_error"}
        r["actions"] = r["actions"].astype(np.int64)
        for k in ("step_length", "qp_failures"):
            r[k] = r[k].astype(np.int64)
        for k in ("terminated", "truncated"):
            r[k] = r[k] != 0
        r["observations"] = out[F * E * B:(F + no) * E * B].reshape(E, B, no).copy()
        tail = out[(F + no) * E * B:]
        r["last_values"], r["last_dones"], r["next_observation"] = tail[:B].copy(), tail[B:2 * B].copy(), tail[2 * B:].reshape(B, no).copy()
        return r

    # ---- the PPO update (stable_baselines3 PPO.train)
    PPO_STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm", "n")          # TUM_PPO_* of tum_nmpc.h

    def ppo_attach(self, clip_range=0.2, ent_coef=0.006, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True):
        """The trainer on the attached policy and value net (tum_sim_ppo_attach): Adam's moments and step counter at zero. Detaching or
        re-attaching the policy or the value net detaches it."""
        self._chk(self._L.tum_sim_ppo_attach(self._s, float(clip_range), float(ent_coef), float(vf_coef), float(max_grad_norm),
                                             int(bool(normalize_advantage))), "sim_ppo_attach")

    def ppo_detach(self):
        self._chk(self._L.tum_sim_ppo_detach(self._s), "sim_ppo_detach")

    def _ppo_shapes(self):
        """[(out, in), ...] of the policy net and of the value net"""
        pw, vw = getattr(self, "policy_widths", None), getattr(self, "value_widths", None)
        if not pw or not vw:
            raise Exception("ppo: no policy with a value net attached (attach_policy)")
        return [(o, i) for i, o in zip(pw[:-1], pw[1:])], [(o, i) for i, o in zip(vw[:-1], vw[1:])]

    def _ppo_split(self, flat):
        """the flat parameter vector (per net W_0, b_0, W_1, ...; policy then value) -> (weights, biases, value_weights, value_biases)"""
        out, p = [], 0
        for shapes in self._ppo_shapes():
            Ws, bs = [], []
            for o, i in shapes:
                Ws.append(flat[p:p + o * i].reshape(o, i).copy()); p += o * i
                bs.append(flat[p:p + o].copy()); p += o
            out += [Ws, bs]
        return tuple(out)

    def _ppo_rows(self, who, n, obs, actions, old_log_probs, advantages, returns):
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.shape != (n, self.policy_widths[0]):
            raise Exception(f"{who}: observations are ({n}, {self.policy_widths[0]})")
        act = np.asarray(actions)
        if act.shape != (n,) or not np.issubdtype(act.dtype, np.integer):
            raise Exception(f"{who}: actions is an integer array ({n},)")
        cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (old_log_probs, advantages, returns)]
        if any(a.shape != (n,) for a in cols):
            raise Exception(f"{who}: old_log_probs, advantages and returns are ({n},)")
        return [obs, np.ascontiguousarray(act, dtype=np.int32)] + cols

    def ppo_step(self, obs, actions, old_log_probs, advantages, returns, lr, apply=True, want_grads=False, want_rows=False):
        """One minibatch from host arrays (tum_sim_ppo_step). apply=False: loss and gradients only, nothing changes. Returns the dict of
        PPO_STATS; with want_grads `grads`: (weights, biases, value_weights, value_biases) lists of float64 arrays, UNCLIPPED; with
        want_rows `log_probs` and `values` (n,) as the update computed them."""
        shapes = self._ppo_shapes()
        n = len(np.asarray(actions))
        if n < 1:
            raise Exception("ppo_step: n < 1")
        obs, act, lp, adv, ret = self._ppo_rows("ppo_step", n, obs, actions, old_log_probs, advantages, returns)
        P = sum(o * i + o for sh in shapes for o, i in sh)
        stats, grads, rows = np.zeros(len(self.PPO_STATS)), np.zeros(P), np.zeros((n, 2))
        self._chk(self._L.tum_sim_ppo_step(self._s, n, _dp(obs), act.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(lp), _dp(adv), _dp(ret),
                                           float(lr), int(bool(apply)), _dp(stats), _dp(grads) if want_grads else None,
                                           _dp(rows) if want_rows else None), "sim_ppo_step")
        out = dict(zip(self.PPO_STATS, stats))
        out["n"] = int(out["n"])
        if want_grads:
            out["grads"] = self._ppo_split(grads)
        if want_rows:
            out["log_probs"], out["values"] = rows[:, 0].copy(), rows[:, 1].copy()
        return out

    def ppo_update(self, N, perm, batch_size, lr, buffer=None):
        """One update (tum_sim_ppo_update): perm (n_epochs, N) integers in [0, N); buffer None: the rows the last env_collect left on
        the device, else (obs (N, n_obs), actions, old_log_probs, advantages, returns (N,)). Returns a dict of PPO_STATS arrays
        (n_epochs, minibatches)."""
        ip = ctypes.POINTER(ctypes.c_int)
        N = int(N)
        perm = np.asarray(perm)
        if perm.ndim != 2 or perm.shape[1] != N or perm.shape[0] < 1 or not np.issubdtype(perm.dtype, np.integer):
            raise Exception(f"ppo_update: perm is an integer array (n_epochs, {N})")
        if int(batch_size) < 1:
            raise Exception("ppo_update: batch_size < 1")
        if np.any(perm < 0) or np.any(perm >= N):
            raise Exception("ppo_update: perm is outside the buffer")
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        n_epochs, bs = perm.shape[0], min(int(batch_size), N)
        n_mb = (N + bs - 1) // bs
        stats = np.zeros((n_epochs, n_mb, len(self.PPO_STATS)))
        if buffer is None:
            args = [None] * 5
        else:
            self._ppo_shapes()
            rows = self._ppo_rows("ppo_update", N, *buffer)
            args = [_dp(rows[0]), rows[1].ctypes.data_as(ip)] + [_dp(a) for a in rows[2:]]
        self._chk(self._L.tum_sim_ppo_update(self._s, N, *args, perm.ctypes.data_as(ip), n_epochs, int(batch_size), float(lr), _dp(stats)),
                  "sim_ppo_update")
        out = {k: stats[:, :, i].copy() for i, k in enumerate(self.PPO_STATS)}
        out["n"] = out["n"].astype(np.int64)
        return out

    def ppo_params(self):
        """(weights, biases, value_weights, value_biases): the float32 parameters the device acts with"""
        nets = []
        for shapes in self._ppo_shapes():
            nets += [[np.zeros((o, i), dtype=np.float32) for o, i in shapes], [np.zeros(o, dtype=np.float32) for o, i in shapes]]
        ptrs = [(ctypes.c_void_p * len(a))(*[x.ctypes.data for x in a]) for a in nets]
        self._chk(self._L.tum_sim_ppo_params(self._s, *ptrs), "sim_ppo_params")
        return tuple(nets)

    def ppo_state(self):
        """Adam's state: dict of m and v -- each (weights, biases, value_weights, value_biases) of float64 arrays -- and t, the step counter"""
        shapes = self._ppo_shapes()
        P = sum(o * i + o for sh in shapes for o, i in sh)
        m, v, t, n = np.zeros(P), np.zeros(P), ctypes.c_longlong(0), ctypes.c_int(0)
        self._chk(self._L.tum_sim_ppo_state(self._s, _dp(m), _dp(v), ctypes.byref(t), ctypes.byref(n)), "sim_ppo_state")
        if n.value != P:
            raise Exception(f"ppo_state: the device holds {n.value} parameters, the attached widths say {P}")
        return dict(m=self._ppo_split(m), v=self._ppo_split(v), t=int(t.value))

    def policy_eval(self, obs):
        """the attached policy alone on (n, n_obs) observations, independent of the loop's batch: dict of logits (n, A), probabilities
        (n, A) -- the softmax of the logits -- and actions (n,), the first index of the largest logit"""
        w = getattr(self, "policy_widths", None)
        if not w:
            raise Exception("policy_eval: no policy attached (attach_policy)")
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != w[0] or obs.shape[0] < 1:
            raise Exception(f"policy_eval: observations are (n, {w[0]}), n >= 1")
        n = obs.shape[0]
        logits, probs, act = np.empty((n, w[-1])), np.empty((n, w[-1])), np.empty(n, dtype=np.int32)
        self._chk(self._L.tum_sim_policy_eval(self._s, _dp(obs), n, _dp(logits), _dp(probs), act.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
                  "sim_policy_eval")
        return dict(logits=logits, probabilities=probs, actions=act.astype(np.int64))

    def env_rollout(self, n_env_steps, first_obs=None, on_end=0, start_table=None, check_every=0):
        """n_env_steps environment steps with the attached policy choosing every action, without a host wait in between. first_obs
        (B, n_obs) what the policy sees first (None: zeros, what a reset returns). on_end 0: an ended instance is frozen out (live 0
        from the next step on; its later rows are not results); on_end 1: it is reset at the start of step e + 1 to
        start_table[e + 1][b] -- (n_env_steps, B) -- and the policy sees zeros for it. check_every > 0: the rollout stops when no
        instance is live, looked at every check_every steps. Returns a dict of (E, B[, ...]) arrays over the E steps that ran: the
        fields of env_step, action and live."""
        ip = ctypes.POINTER(ctypes.c_int)
        E, B, no = int(n_env_steps), self.B, getattr(self, "env_n_obs", 0)
        if E < 1:
            raise Exception("env_rollout: n_env_steps < 1")
        fo = None
        if first_obs is not None:
            fo = np.ascontiguousarray(first_obs, dtype=np.float64)
            if fo.shape != (B, no):
                raise Exception(f"env_rollout: first_obs is ({B}, {no})")
        tab = None
        if start_table is not None:
            tab = np.asarray(start_table)
            if tab.shape != (E, B) or not np.issubdtype(tab.dtype, np.integer):
                raise Exception(f"env_rollout: start_table is an integer array ({E}, {B})")
            tab = np.ascontiguousarray(tab, dtype=np.int32)
        out = np.zeros((E, B, self.ENV_HEAD + no))
        act, live, ran = np.zeros((E, B), dtype=np.int32), np.zeros((E, B), dtype=np.int32), ctypes.c_int(0)
        self._chk(self._L.tum_sim_env_rollout(self._s, E, None if fo is None else _dp(fo), int(on_end), None if tab is None else tab.ctypes.data_as(ip),
                                              int(check_every), _dp(out), act.ctypes.data_as(ip), live.ctypes.data_as(ip), ctypes.byref(ran)),
                  "sim_env_rollout")
        n = ran.value
        out = out[:n]
        return dict(action=act[:n].astype(np.int64), live=live[:n] != 0, reward=out[:, :, 0].copy(), terminated=out[:, :, 1] != 0,
                    truncated=out[:, :, 2] != 0, step_length=out[:, :, 3].astype(np.int64), qp_failures=out[:, :, 4].astype(np.int64),
                    observation=out[:, :, self.ENV_HEAD:].copy())


def env_observation_bounds(n_samples):
    """(2, 2 + 2 n) lower / upper normalisation bounds of the RL observation (RL_WMPC/observation.py:16-24): lateral deviation,
    velocity deviation, n future velocities, n future yaw rates"""
    n = int(n_samples)
    return np.concatenate((np.array([[-3., 3.], [-5, 5]]), np.tile([0., 39.], (n, 1)), np.tile([-3.2, 3.2], (n, 1)))).transpose()


def segment_flags(state):
    """crashed / done / timed_out of segment state words: crash wins over done, a segment still active has timed out"""
    state = np.asarray(state)
    crashed = (state & (DeviceClosedLoop.SEG_CRASH_LAT | DeviceClosedLoop.SEG_CRASH_ACOMB)) != 0
    return dict(crashed=crashed, done=((state & DeviceClosedLoop.SEG_DONE) != 0) & ~crashed, timed_out=state == 0)
