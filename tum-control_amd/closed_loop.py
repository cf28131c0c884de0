"""
closed_loop.py -- counterpart of the reference's closed-loop harness for a BATCH of independent vehicles
(SURVEY.md 8(f2), 8(f4)): planner -> batched SQP-RTI solve on the GPU -> plant step -> state estimation.

Restates, for the code around the hot path only what is needed to drive it the way the reference does:
  main.py:48-78 / Learning_To_Adapt/SafeRL_WMPC/get_baseline_performances.py:101-131   the loop
  Utils/SimulationMode_main_class.py:106-156                                            sim_step (simMode 0), StateEstimation
  Vehicle_Simulator/sim_model_dynamic_stm_pacejka.py:137-195 + VehicleSimulator.py:73-77 plant: 7-state single track
                                                                                         (input = acceleration, steering rate),
                                                                                         CasADi 'rk' with 4 finite elements = RK4 x 4
  Utils/Logging_Plotting.py:124-146,321-372                                             what gets logged, and the npz file (save)
  Utils/MPC_sim_utils.py:15-99                                                          disturbance set-up and generators
Every instance may carry its own cost weights / penalties (the BO / RL weight sweep as one batch).
"""
import numpy as np

from . import config as _config
from .planner import closest_index, load_track, planner_emulator, yref_from_ref
from .solver import BatchedOcpSolver, CoupledSnmpcSolver, DeviceClosedLoop, env_observation_bounds, segment_flags

WINDOWS = (1, 1, 4, 2, 2, 3, 4, 2)          # SimulationMode_main_class.py:86


def plant_xdot(x, a, sr, cfg):
    """xdot of the 7-state plant [posx,posy,yaw,vlong,vlat,yawrate,delta_f]; x: (B,7), a, sr: (B,)."""
    veh, tire, ph = cfg["veh"], cfg["tire"], cfg["phys"]
    lf, lr, m, Iz = veh["lf"], veh["lr"], veh["m"], veh["Iz"]
    yaw, vl, vt, r, de = x[:, 2], x[:, 3], x[:, 4], x[:, 5], x[:, 6]
    v = np.sqrt(vl ** 2 + vt ** 2) * 3.6
    fr = ph["fr0"] + ph["fr1"] * v / 100 + ph["fr4"] * (v / 100) ** 4
    Fz_f = m * lr * ph["g"] / (lf + lr); Fz_r = m * lf * ph["g"] / (lf + lr)
    Fx_f = -fr * Fz_f
    Fx_r = m * a - fr * Fz_r
    Faero = 0.5 * veh["ro"] * veh["S"] * veh["Cd"] * vl ** 2
    ok = vl > 0.001
    vls = np.where(ok, vl, 1.0)
    al_f = np.where(ok, de - np.arctan((vt + lf * r) / vls), 0.0)
    al_r = np.where(ok, np.arctan((lr * r - vt) / vls), 0.0)
    Bf, Cf, Df, Ef = tire["Bf"], tire["Cf"], tire["Df"], tire["Ef"]
    Br, Cr, Dr, Er = tire["Br"], tire["Cr"], tire["Dr"], tire["Er"]
    Fy_f_lat = Df * np.sin(Cf * np.arctan(Bf * al_f - Ef * (Bf * al_f - np.arctan(Bf * al_f))))
    Fy_r_lat = Dr * np.sin(Cr * np.arctan(Br * al_r - Er * (Br * al_r - np.arctan(Br * al_r))))
    Fmax_f = np.sqrt(Fz_f ** 2 + (Cf * Fz_f) ** 2); Fmax_r = np.sqrt(Fz_r ** 2 + (Cr * Fz_r) ** 2)
    Gy_f = np.clip(Fx_f / Fmax_f, -0.98, 0.98); Gy_r = np.clip(Fx_r / Fmax_r, -0.98, 0.98)
    Fy_f = Fy_f_lat * np.cos(np.arcsin(Gy_f)); Fy_r = Fy_r_lat * np.cos(np.arcsin(Gy_r))
    xd = np.empty_like(x)
    xd[:, 0] = vl * np.cos(yaw) - vt * np.sin(yaw)
    xd[:, 1] = vl * np.sin(yaw) + vt * np.cos(yaw)
    xd[:, 2] = r
    xd[:, 3] = (Fx_r - Faero - Fy_f * np.sin(de) + Fx_f * np.cos(de) + m * vt * r) / m
    xd[:, 4] = (Fy_r + Fy_f * np.cos(de) + Fx_f * np.sin(de) - m * vl * r) / m
    xd[:, 5] = (lf * (Fy_f * np.cos(de) + Fx_f * np.sin(de)) - lr * Fy_r) / Iz
    xd[:, 6] = sr
    return xd


def plant_step(x, a, sr, cfg, Ts=0.02, n_elem=4, w=None):
    """One simulator step: classic RK4 with `n_elem` equal sub-steps over Ts, inputs held constant. w (B,7): additive disturbance
    of the state derivatives, constant over the step (simulator_step_disturbed: xdot + w, sim_model_dynamic_stm_pacejka.py:196)."""
    h = Ts / n_elem
    x = x.copy()
    f = (lambda y: plant_xdot(y, a, sr, cfg)) if w is None else (lambda y: plant_xdot(y, a, sr, cfg) + w)
    for _ in range(n_elem):
        k1 = f(x)
        k2 = f(x + 0.5 * h * k1)
        k3 = f(x + 0.5 * h * k2)
        k4 = f(x + h * k3)
        x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


STATE_NAMES = ("posx", "posy", "yaw", "vlong", "vlat", "yawrate", "delta_f")


def sample_from_ellipsoid(w, Z, rng):
    """Utils/MPC_sim_utils.py:70-86: a point of the ellipsoid with centre w and shape matrix Z -- radius rand()^(1/n), direction a
    normalised Gaussian vector, mapped through the eigen-decomposition of Z. Same order of random draws as the reference (one rand(),
    then n randn())."""
    n = w.shape[0]
    lam, v = np.linalg.eig(Z)
    r = rng.rand() ** (1 / n)
    x = rng.randn(n)
    x = x / np.linalg.norm(x)
    x *= r
    return v @ (np.sqrt(lam) * x) + w


def generate_disturbances(bounds, kind, rng):
    """Utils/MPC_sim_utils.py:54-67: one realisation for the n channels of `bounds` ([-b, b] pairs). 'uniform' draws from the ELLIPSOID
    with semi-axes sqrt(b) (the reference passes diag(b) as the shape matrix), 'gaussian' has standard deviation b, 'absolute'
    returns b; anything else is uniform in the box."""
    b = np.asarray(bounds, dtype=float)
    if kind == 'uniform':
        return sample_from_ellipsoid(np.zeros(len(b)), np.diag(b.T[1, :]), rng)
    if kind == 'gaussian':
        return np.array([rng.normal(0, b[j][1]) for j in range(len(b))])
    if kind == 'absolute':
        return np.array([b[j][1] for j in range(len(b))])
    return np.array([rng.uniform(b[j][0], b[j][1]) for j in range(len(b))])


class DisturbanceModel:
    """The disturbance set-up of the reference's harness (initDisturbanceSim, Utils/MPC_sim_utils.py:15-51; switches and magnitudes:
    Config/EDGAR/sim_main_params.yaml:44-80) and the realisations sim_step draws from it (SimulationMode_main_class.py:121-143).
    `draw` pre-draws a whole run: the device loop plays a realisation back (as the reference does with disturbance_playback),
    the host loop applies the same arrays step by step."""

    def __init__(self, sim_main_params=None, **override):
        p = dict(_config.SIM)
        p.update(sim_main_params or {})
        p.update(override)
        self.derivatives = bool(p["simulate_disturbances"])
        self.state_estimation = bool(p["simulate_state_estimation"])
        self.types = [p["disturbance_type_derivatives"], p["disturbance_type_state_estimation"]]
        self.bounds_derivatives = [[-p[f"w_{n}_dot"], p[f"w_{n}_dot"]] for n in STATE_NAMES]
        self.bounds_state_estimation = [[-p[f"w_{n}"], p[f"w_{n}"]] for n in STATE_NAMES]

    def draw(self, n_steps, batch=1, seed=0):
        """(w_deriv, e_est): (n_steps, batch, 7) arrays or None. Vehicle b uses numpy's legacy generator seeded with seed + b and
        draws in the reference's order -- per control step the derivative disturbance first, then the estimation error -- so
        batch = 1 reproduces what main.py produces after np.random.seed(seed)."""
        w = np.zeros((n_steps, batch, 7)) if self.derivatives else None
        e = np.zeros((n_steps, batch, 7)) if self.state_estimation else None
        for b in range(batch):
            rng = np.random.RandomState(seed + b)
            for i in range(n_steps):
                if w is not None:
                    w[i, b] = generate_disturbances(self.bounds_derivatives, self.types[0], rng)
                if e is not None:
                    e[i, b] = generate_disturbances(self.bounds_state_estimation, self.types[1], rng)
        return w, e

    def draw_counter(self, n_steps, batch=1, seed=0, first_step=0, first_instance=0):
        """(w_deriv, e_est) like `draw`, from the project's COUNTER-BASED stream (include/tum_nmpc.h, "Disturbance draws"): row
        [i, k] is the realisation of instance first_instance + k at global control step first_step + i, and depends on (seed,
        instance, step, stream, kind, bounds) alone -- any window and any batch that contain a row return the same bits for it.
        The host statement of what disturbance_draw_kernel draws on the device (DeviceClosedLoop.attach_disturbances): the box
        and 'absolute' kinds agree with it to the bit, the two normal kinds to the math library's last bits. Vectorised over steps
        and vehicles (windows of more than 2^16 rows are drawn in slabs of steps, to bound the memory of the Philox words). NOT
        numpy's Mersenne-Twister stream of `draw`: the distributions are the same, the numbers are not."""
        n_steps, batch, first_step = int(n_steps), int(batch), int(first_step)
        seed = int(seed) & (2 ** 64 - 1)
        key = np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64)
        b = ((int(first_instance) + np.arange(batch)) & 0xffffffff).astype(np.uint64)
        out = []
        for s, (on, kind, bounds) in enumerate(((self.derivatives, self.types[0], self.bounds_derivatives),
                                                (self.state_estimation, self.types[1], self.bounds_state_estimation))):
            if not on:
                out.append(None)
                continue
            w = np.asarray(bounds, dtype=float)[:, 1]
            res = np.zeros((n_steps, batch, 7))
            slab = max(1, (1 << 16) // max(batch, 1))
            for i0 in range(0, n_steps, slab):
                t = np.uint64(first_step + i0) + np.arange(min(slab, n_steps - i0), dtype=np.uint64)
                ctr = np.zeros((len(t), batch, DISTURBANCE_BLOCKS, 4), dtype=np.uint64)
                ctr[..., 0] = b[None, :, None]
                ctr[..., 1] = (t & np.uint64(0xffffffff))[:, None, None]
                ctr[..., 2] = (t >> np.uint64(32))[:, None, None]
                ctr[..., 3] = np.uint64(0x100 * (1 + s)) + np.arange(DISTURBANCE_BLOCKS, dtype=np.uint64)
                x = philox4x32(ctr, key)
                res[i0:i0 + len(t)] = disturbance_from_uniforms(kind, w, uniform_from_words(x[..., 0], x[..., 1]),
                                                                uniform_from_words(x[..., 2], x[..., 3]))
            out.append(res)
        return out[0], out[1]


DISTURBANCE_BLOCKS = 5          # Philox blocks of one draw: four of normals / box uniforms, one for the ellipsoid's radius


def disturbance_from_uniforms(kind, w, uA, uB):
    """One draw per leading index from the uniforms of its Philox blocks: uA, uB (..., 5) in [0, 1), w (7,) bounds >= 0 -> (..., 7).
    The statement of include/tum_nmpc.h in plain binary64 numpy, in the device function's order of operations (products and sums
    rounded one by one, the norm summed in index order)."""
    w = np.asarray(w, dtype=float)
    uA, uB = np.asarray(uA, dtype=float), np.asarray(uB, dtype=float)
    lead = uA.shape[:-1]
    if kind == 'absolute':
        return np.broadcast_to(w, lead + (7,)).copy()
    if kind in ('uniform', 'gaussian'):
        R = np.sqrt(-2.0 * np.log(1.0 - uA[..., :4]))
        th = (2.0 * np.pi) * uB[..., :4]
        z = np.stack([R * np.cos(th), R * np.sin(th)], axis=-1).reshape(lead + (8,))[..., :7]
        if kind == 'gaussian':
            return w * z
        n2 = z[..., 0] * z[..., 0]
        for i in range(1, 7):
            n2 = n2 + z[..., i] * z[..., i]
        nz = np.sqrt(n2)[..., None]
        r = (uA[..., 4] ** (1.0 / 7.0))[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(nz == 0.0, 0.0, np.sqrt(w) * r * z / nz)
    u = np.stack([uA[..., :4], uB[..., :4]], axis=-1).reshape(lead + (8,))[..., :7]
    return -w + u * (2.0 * w)


def lon_lat_deviations(ego_yaw, ego_x, ego_y, ref_x, ref_y):
    """Utils/MPC_sim_utils.py:103-112: the deviation vector rotated into the vehicle frame"""
    c, s_ = np.cos(-ego_yaw), np.sin(-ego_yaw)
    return c * (ref_x - ego_x) - s_ * (ref_y - ego_y), s_ * (ref_x - ego_x) + c * (ref_y - ego_y)


def wrap_yaw(yaw):
    """postprocess_yaw (Utils/MPC_sim_utils.py:124-134): fmod into (-2 pi, 2 pi), negatives shifted up"""
    y = np.fmod(np.asarray(yaw, dtype=float), 2 * np.pi)
    return np.where(y < 0, y + 2 * np.pi, y)


LOG_KEYS = ("MPC_SimX", "CiLX", "simU", "simREF", "simSolverDebug", "sim_disturbance_derivatives", "sim_disturbance_state_estimation",
            "a_lat", "dev_lat", "dev_long", "dev_vel", "dev_yaw", "t")


def log_file_arrays(logs, b, w_deriv=None, e_est=None, T=None, Ts=0.02, drop_last_step=True):
    """The arrays of one vehicle's `full_logs.npz` as Logger.save_logs writes them (Utils/Logging_Plotting.py:321-395): the five raw
    logs of instance b (yaw columns wrapped to [0, 2 pi) as the reference stores them), the disturbance realisation, and the derived
    channels a_lat = vlong * yawrate, dev_lat / dev_long (vehicle frame), dev_vel, dev_yaw, t.
    drop_last_step: Logger.truncate cuts at `current_step`, the INDEX of the last control step -- a run of n steps is stored as n - 1
    rows of simU / simREF / simSolverDebug and n rows of CiLX / MPC_SimX (the reference's own files: 5500 steps run, 5499 stored), while
    the disturbance arrays keep all n rows and t = linspace(0, T, n - 1). True reproduces that layout; False keeps every step."""
    simU = np.array(logs["simU"][:, b])
    n_run = len(simU)
    n = n_run - 1 if (drop_last_step and n_run > 1) else n_run
    CiLX = np.array(logs["CiLX"][:n + 1, b]); SimX = np.array(logs["MPC_SimX"][:n + 1, b])
    simU = simU[:n]; simREF = np.array(logs["simREF"][:n, b]); dbg = np.array(logs["simSolverDebug"][:n, b])
    dev_vel = np.abs(CiLX[1:, 3] - simREF[:, 3])
    CiLX[:, 2] = wrap_yaw(CiLX[:, 2]); SimX[:, 2] = wrap_yaw(SimX[:, 2])
    dev_yaw = np.abs(CiLX[1:, 2] - simREF[:, 2])
    dev_long, dev_lat = lon_lat_deviations(CiLX[1:, 2], CiLX[1:, 0], CiLX[1:, 1], simREF[:, 0], simREF[:, 1])

    def realisation(a):
        out = np.zeros((n_run, 7))
        if a is not None:
            a = np.asarray(a)[:n_run, b]
            out[:len(a)] = a
        return out
    return dict(MPC_SimX=SimX, CiLX=CiLX, simU=simU, simREF=simREF, simSolverDebug=dbg,
                sim_disturbance_derivatives=realisation(w_deriv), sim_disturbance_state_estimation=realisation(e_est),
                a_lat=CiLX[:, 3] * CiLX[:, 5], dev_lat=dev_lat, dev_long=dev_long, dev_vel=dev_vel, dev_yaw=dev_yaw,
                t=np.linspace(0.0, _config.SIM["T"] if T is None else T, n))      # (Logging_Plotting.py:348-349: always sim_main_params['T'], whatever the run length)


class MovingAverageEstimator:
    """StateEstimation (SimulationMode_main_class.py:152-156): per-state moving average over the last
    WINDOWS[i] samples (fewer while the buffer fills), buffers start empty."""

    def __init__(self, batch):
        self.hist = [[] for _ in range(8)]
        self.batch = batch

    def __call__(self, x_next):
        out = np.empty_like(x_next)
        for i in range(8):
            self.hist[i].append(x_next[:, i].copy())
            if len(self.hist[i]) > 15:
                self.hist[i].pop(0)
            out[:, i] = np.mean(self.hist[i][-WINDOWS[i]:], axis=0)
        return out


def resolve_tracks(track_name, batch, track_of=None):
    """(names, tables, track_of) of a loop's tracks: track_name one name of planner.TRACKS -- track_of must be None then and every
    instance drives on it -- or a sequence of names, instance i on names[track_of[i]] (None: i % T, as RL_WMPC/environment.py:283
    deals trajectories to environments). An unknown name is a KeyError (load_track), a bad track_of a ValueError."""
    if isinstance(track_name, str):
        if track_of is not None:
            raise ValueError("track_of goes with a sequence of track names")
        return [track_name], [load_track(track_name)], np.zeros(int(batch), dtype=np.int64)
    names = [str(n) for n in track_name]
    if not names:
        raise ValueError("track_name: a name or a non-empty sequence of names")
    tables = [load_track(n) for n in names]
    of = np.arange(int(batch)) % len(names) if track_of is None else np.asarray(track_of)
    if of.shape != (int(batch),) or not np.issubdtype(of.dtype, np.integer):
        raise ValueError(f"track_of: one integer track id per instance ({int(batch)})")
    if ((of < 0) | (of >= len(names))).any():
        raise ValueError(f"track_of holds ids outside 0..{len(names) - 1}")
    return names, tables, of.astype(np.int64)


def start_states(track, idx_start, batch, track_of=None):
    """X0_MPC (batch, 8) of loops that start on the race line at waypoint idx_start (SimulationMode_main_class.py:60-75 with
    idx_ref_start): position, yaw in [0, 2 pi), reference speed, everything else 0. idx_start: one index or (batch,) indices.
    With track_of (batch,): `track` is a sequence of tables and instance b starts at waypoint idx_start[b] of track[track_of[b]]; an
    index outside that instance's own track is an IndexError, whatever the longer tracks of the set hold."""
    if track_of is not None:
        of = np.asarray(track_of)
        idx = np.broadcast_to(np.asarray(idx_start), (batch,))
        if of.shape != (batch,) or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("idx_start: one index or an integer array of length batch; track_of: one track id per instance")
        x = np.zeros((batch, 8))
        for b in range(batch):
            t = track[of[b]]
            if not -len(t) <= idx[b] < len(t):
                raise IndexError(f"idx_start[{b}] = {idx[b]} is outside the instance's own track ({len(t)} rows)")
            x[b, :4] = t[idx[b], 0], t[idx[b], 1], np.mod(t[idx[b], 2], 2 * np.pi), t[idx[b], 3]
        return x
    idx = np.asarray(idx_start)
    if idx.ndim == 0:
        i = idx_start
        x0 = np.array([track[i, 0], track[i, 1], np.mod(track[i, 2], 2 * np.pi), track[i, 3], 0, 0, 0, 0.0])
        return np.tile(x0, (batch, 1))
    if idx.shape != (batch,) or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("idx_start: one index or an integer array of length batch")
    x = np.zeros((batch, 8))
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = track[idx, 0], track[idx, 1], np.mod(track[idx, 2], 2 * np.pi), track[idx, 3]
    return x


class ClosedLoopBatch:
    """B independent closed loops, one OCP instance each; `params` (B,7) are per-instance
    [q_xy, q_yaw, q_vel, r_jerk, r_steer, L1, L2] as in update_cost_function_weights (None: YAML defaults x0.01).
    track_name: one track for all instances, or a sequence of names with instance i on track_name[track_of[i]] (None: i % T) -- on the
    device and on the host path alike; .tracks / .track_of hold what was resolved, .track the one table of a single-track batch.
    idx_start: the waypoint all loops start at, or one per instance -- a waypoint of the instance's own track."""

    def __init__(self, track_name, batch=1, params=None, N=38, Tp=3.04, Ts=0.02, idx_start=0, cfg=None, device=0,
                 on_device=False, log_capacity=0, controller="nominal", disturbances=None, disturbance_steps=0, seed=0,
                 qp_warm_start=None, qp_tol=None, track_of=None, draw="legacy", wmpc=None, weights_update_period=20,
                 wmpc_on_failure="base", wmpc_log_capacity=0):
        """wmpc = (policy, table): the learned weight schedule of the reference's controller classes (enable_WMPC) -- a WeightPolicy
        and the (A, 7) parameter table it picks rows of; after the solve of every control step the rule of WmpcSchedule, with
        weights_update_period control steps between decisions. on_device=True: inside the device loop (DeviceClosedLoop.attach_wmpc);
        on_device=False: in step(), the host statement the device is held to. wmpc_on_failure "base": an instance whose solve failed
        gets the weights of this constructor back (`params`, or the YAML's x 0.01); "keep": it keeps what it has.
        wmpc_log_capacity: decisions stored per instance (wmpc_decisions)."""
        if draw not in ("legacy", "counter", "device"):
            raise ValueError("ClosedLoopBatch: draw must be 'legacy', 'counter' or 'device'")
        if draw != "legacy" and disturbances is not None and not isinstance(disturbances, DisturbanceModel):
            raise ValueError(f"ClosedLoopBatch: draw='{draw}' draws from a DisturbanceModel; a (w_deriv, e_est) pair is played back (draw='legacy')")
        if draw == "device" and disturbances is not None and not on_device:
            raise ValueError("ClosedLoopBatch: draw='device' draws inside the device loop (on_device=True); draw='counter' plays the same stream back on the host")
        self.cfg = cfg or _config.default_config()
        kw = {} if qp_tol is None else dict(qp_tol=tuple(qp_tol))          # (termination tolerances of the interior point method; default: the solver's 1e-8)
        self.track_names, self.tracks, self.track_of = resolve_tracks(track_name, batch, track_of)
        single = isinstance(track_name, str)
        self.track = self.tracks[0] if single else None
        self.B, self.N, self.Tp, self.Ts = batch, N, Tp, Ts
        self.x_mpc = start_states(self.track, idx_start, batch) if single else start_states(self.tracks, idx_start, batch, self.track_of)  # X0_MPC
        self.x_sim = self.x_mpc[:, :7].copy()                    # X0_sim
        self.pose = self.x_mpc[:, :2].copy()
        self.controller = controller
        if controller == "nominal":       # main.py:33-36 picks the controller class by MPC_params['MPC_type']
            self.solver = BatchedOcpSolver(N=N, dt=Tp / N, nsub=3, batch=batch, device=device, cfg=self.cfg, qp_warm_start=qp_warm_start, **kw)
        elif controller == "snmpc":       # the coupled SNMPC OCP; x0_samples = compute_x0dist(x0) before every solve
            from . import snmpc as _snm
            m = self.cfg["mpc"]
            stds = np.asarray(m["stds"], dtype=float)
            nvar = int(np.count_nonzero(stds))
            w = _snm.hammersley_normal(m["n_samples"], nvar)
            A = _snm.pce_matrix(w, _snm.alpha_generation(nvar, m["expansion_degree"]))
            self._x0_offsets = _snm.x0_offsets(w, stds)
            self.solver = CoupledSnmpcSolver(N=N, dt=Tp / N, batch=batch, Apce=A, uph=min(int(m["uncertainty_propagation_horizon"]), N),
                                             gamma=m["gamma"], device=device, cfg=self.cfg, x0_offsets=self._x0_offsets, qp_warm_start=qp_warm_start, **kw)
        elif controller == "r2":          # nominal OCP + covariance back-off after every solve (K7 attached to the solve)
            from .r2nmpc import r2_setup
            m, veh = self.cfg["mpc"], self.cfg["veh"]
            self.solver = BatchedOcpSolver(N=N, dt=Tp / N, nsub=3, batch=batch, device=device, cfg=self.cfg, store_qp_in=True,
                                           qp_warm_start=qp_warm_start, **kw)
            S0, BWB = r2_setup(m["stds"], Tp / N)
            self.solver.r2_attach(S0, BWB, int(m["uncertainty_propagation_horizon"]), veh["delta_f_min"], veh["delta_f_max"], 1.0)
        else:
            raise ValueError("controller must be 'nominal', 'snmpc' or 'r2'")
        self.solver.install_reference_ocp()
        # the weights the solver holds, per instance: diag W of the stages < N, diag W_e, [L1, L2] (install_reference_ocp's defaults)
        m = self.cfg["mpc"]
        w6 = 0.01 * np.array([m["q_lon"] / m["s_lon"] ** 2, m["q_lat"] / m["s_lat"] ** 2, m["q_yaw"] / m["s_yaw"] ** 2, m["q_vel"] / m["s_vel"] ** 2,
                              m["r_jerk"] / m["s_jerk"] ** 2, m["r_steering_rate"] / m["s_steering_rate"] ** 2])
        self._weights = [np.tile(w6, (batch, 1)), np.tile(w6[:4], (batch, 1)), np.tile([float(m["L1_pen"]), float(m["L2_pen"])], (batch, 1))]
        if params is not None:
            self.set_weights(np.asarray(params, dtype=float).reshape(batch, 7))
        self._base_weights = [a.copy() for a in self._weights]          # (what wmpc_on_failure="base" goes back to)
        self.solver.set_x0(self.x_mpc)
        self.solver.cold_start()
        self.est = MovingAverageEstimator(batch)
        # on_device: planner, plant and estimator run as kernels next to the solve (no host round trip per step)
        self.dev = None
        if on_device:
            set_kw = {} if single else dict(tracks=self.tracks, track_of=self.track_of)
            self.dev = DeviceClosedLoop(self.solver, self.track, Tp, Ts=Ts, n_elem=4, windows=WINDOWS, log_capacity=log_capacity, **set_kw)
            self.dev.set_state(self.x_sim, self.x_mpc, cold_start=True)
        self.log = dict(CiLX=[self.x_sim.copy()], MPC_SimX=[self.x_mpc.copy()], simU=[], simREF=[], simSolverDebug=[])
        # disturbance realisation (sim_step's simulate_disturbances / simulate_state_estimation): a DisturbanceModel -- `disturbance_steps`
        # control steps are drawn with `seed` -- or a (w_deriv, e_est) pair of (n_steps, B, 7) arrays / None to play back.
        # draw: which stream a DisturbanceModel is drawn from -- "legacy": numpy's Mersenne-Twister, the reference's (draw);
        # "counter": the project's counter-based stream, drawn on the host and played back (draw_counter); "device": the same stream
        # drawn by the device loop itself, one launch per control step, for as long as the loop runs (disturbance_steps is ignored)
        self.w_deriv = self.e_est = None
        self._i = 0
        self._last_logs = None
        self.draw = draw
        if disturbances is not None:
            if draw == "device":
                self.dev.attach_disturbances(disturbances, seed)
            else:
                w, e = disturbances if not isinstance(disturbances, DisturbanceModel) else \
                    (disturbances.draw if draw == "legacy" else disturbances.draw_counter)(disturbance_steps, batch, seed)
                self.set_disturbances(w, e)
        self.wmpc = None
        if wmpc is not None:
            policy, table = wmpc
            self.wmpc = WmpcSchedule(policy, table, weights_update_period, batch, Ts=Ts, log_capacity=wmpc_log_capacity)
            if wmpc_on_failure not in ("base", "keep"):
                raise ValueError("ClosedLoopBatch: wmpc_on_failure must be 'base' or 'keep'")
            self.wmpc_on_failure = wmpc_on_failure
            if self.dev is not None:
                self.dev.attach_policy(policy)
                self.dev.attach_wmpc(self.wmpc.table, weights_update_period, wmpc_on_failure, self.wmpc.n_samples, wmpc_log_capacity)

    def wmpc_decisions(self):
        """the decisions of the learned weight schedule so far: dict of n_decisions (B,), and of the first wmpc_log_capacity of every
        instance steps, actions (B, capacity; -1 where none) and observations (B, capacity, n_obs) -- on either path"""
        if self.wmpc is None:
            raise Exception("ClosedLoopBatch.wmpc_decisions: no weight schedule (wmpc=(policy, table))")
        if self.dev is not None:
            return {k: self.dev.wmpc_get(k) for k in ("n_decisions", "steps", "actions", "observations")}
        w = self.wmpc
        return dict(n_decisions=w.n_decisions.copy(), steps=w.steps.copy(), actions=w.actions.copy(), observations=w.observations.copy())

    def _put_weights(self):
        """self._weights through the cost setters (the calls of set_weights)"""
        s, B, N = self.solver, self.B, self.N
        w6, we, L = self._weights
        W = np.zeros((B, 6, 6)); We = np.zeros((B, 4, 4))
        for j in range(B):
            W[j] = np.diag(w6[j]); We[j] = np.diag(we[j])
        s.cost_set(-1, "W", W if B > 1 else W[0])
        s.cost_set(N, "W", We if B > 1 else We[0])
        for st, n in ((0, 1), (1, 3), (N, 2)):
            for f, col in (("zl", 0), ("zu", 0), ("Zl", 1), ("Zu", 1)):
                v = np.repeat(L[:, col:col + 1], n, axis=1)
                s.cost_set(st, f, v if B > 1 else v[0])

    def _wmpc_after_solve(self, yref, ref0, status):
        """the WMPC branch at the end of the controller classes' solve(), for every instance, and main.py:59-61 behind it"""
        due, actions = self.wmpc.after_solve(self._i, self.x_mpc, ref0, yref)
        changed = len(due) > 0
        for b, a in zip(due, actions):
            p = self.wmpc.table[a]
            self._weights[0][b] = [p[0], p[0], p[1], p[2], p[3], p[4]]; self._weights[1][b] = [p[0], p[0], p[1], p[2]]; self._weights[2][b] = p[5:7]
        failed = np.nonzero(np.asarray(status) != 0)[0]
        if self.wmpc_on_failure == "base" and len(failed):
            for cur, base in zip(self._weights, self._base_weights):
                cur[failed] = base[failed]
            changed = True
        if changed:
            self._put_weights()

    def set_disturbances(self, w_deriv=None, e_est=None):
        self.w_deriv = None if w_deriv is None else np.ascontiguousarray(w_deriv, dtype=float).reshape(-1, self.B, 7)
        self.e_est = None if e_est is None else np.ascontiguousarray(e_est, dtype=float).reshape(-1, self.B, 7)
        if self.dev is not None:
            self.dev.set_disturbances(self.w_deriv, self.e_est)

    def set_weights(self, p):
        s, B, N = self.solver, self.B, self.N
        p = np.asarray(p, dtype=float).reshape(-1, 7)          # (one row for all, or one per instance)
        p = np.broadcast_to(p, (B, 7))
        self._weights = [p[:, [0, 0, 1, 2, 3, 4]].copy(), p[:, [0, 0, 1, 2]].copy(), p[:, 5:7].copy()]
        W = np.zeros((B, 6, 6))
        for j in range(B):
            W[j] = np.diag([p[j, 0], p[j, 0], p[j, 1], p[j, 2], p[j, 3], p[j, 4]])
        s.cost_set(-1, "W", W if B > 1 else W[0])          # (-1 = ALL_STAGES: the stages 0..N-1)
        s.cost_set(N, "W", W[:, :4, :4] if B > 1 else W[0, :4, :4])
        for st, n in ((0, 1), (1, 3), (N, 2)):
            for f, col in (("zl", 5), ("zu", 5), ("Zl", 6), ("Zu", 6)):
                v = np.repeat(p[:, col:col + 1], n, axis=1)
                s.cost_set(st, f, v if B > 1 else v[0])

    def step(self):
        s, B, N = self.solver, self.B, self.N
        yref = np.zeros((B, N + 1, 6)); ref0 = np.zeros((B, 4))
        for b in range(B):
            _, ref = planner_emulator(self.tracks[self.track_of[b]], self.pose[b], N + 1, self.Tp, True)
            yref[b] = yref_from_ref(ref, N); ref0[b] = ref[0]
        s.set_yref_all(yref if B > 1 else yref[0])
        status = s.solve()
        X, U = s.get_iterate()
        u0, x1 = U[:, 0], X[:, 1]
        stats = np.stack([np.atleast_1d(s.get_cost()), np.full(B, s.get_stats("time_tot")), np.ones(B),
                          s.get_stats("qp_iter").astype(float), s.get_stats("status").astype(float)], axis=1)
        # sim_step, simMode 0: the plant takes the predicted acceleration of stage 1 and the steering rate
        a_in, sr_in = x1[:, 7].copy(), u0[:, 1].copy()
        if self.wmpc is not None:
            self._wmpc_after_solve(yref, ref0, stats[:, 4])
        failed = np.nonzero(stats[:, 4] != 0)[0]
        if len(failed):
            self._reinitialise(failed, X, U)
        x_sim_next = plant_step(self.x_sim, a_in, sr_in, self.cfg, self.Ts)
        # SimulationMode_main_class.py:121-143: the TRUE state follows the undisturbed step; what the estimator is fed is a second step
        # with disturbed derivatives (if simulated) plus the state estimation error (if simulated)
        i = self._i
        x_meas = x_sim_next
        if self.w_deriv is not None and i < len(self.w_deriv):
            x_meas = plant_step(self.x_sim, a_in, sr_in, self.cfg, self.Ts, w=self.w_deriv[i])
        if self.e_est is not None and i < len(self.e_est):
            x_meas = x_meas + self.e_est[i]
        self._i += 1
        x_next = np.concatenate([x_meas, a_in[:, None]], axis=1)
        self.pose = x_sim_next[:, :2].copy()
        self.x_sim = x_sim_next
        self.x_mpc = self.est(x_next)
        s.set_x0(self.x_mpc if B > 1 else self.x_mpc[0])
        lg = self.log
        lg["simU"].append(u0.copy()); lg["simREF"].append(ref0); lg["simSolverDebug"].append(stats)
        lg["CiLX"].append(x_sim_next.copy()); lg["MPC_SimX"].append(x1.copy())
        return status

    def _reinitialise(self, failed, X, U):
        """main.py:59-61: `if MPC_stats[-1] != 0: MPC.reintialize_solver(x_next)` -- the failed instances get a fresh solver,
        cold-started at the state the failed solve started from (NMPC_class.py:256-267; sample copies included for the SNMPC
        controller, SNMPC_class.py:274-281; nominal bounds again for R2NMPC). The control of this step is still the failed
        solver's u0 and the last good prediction. Host mirror of what plant_advance_kernel does on the device."""
        s, N, B = self.solver, self.N, self.B
        X = X.copy(); U = U.copy()
        X[failed] = self.x_mpc[failed][:, None, :]
        U[failed] = 0.0
        s.set_iterate(X if B > 1 else X[0], U if B > 1 else U[0])
        if self.controller == "snmpc":
            ns = s.ns
            x0s = self.x_mpc[failed][:, None, :] + np.concatenate([np.zeros((1, 8)), self._x0_offsets])[None]    # (F, ns+1, 8)
            for k in range(N + 1):
                xk = np.asarray(s.get(k, "x")).reshape(B, 8 * (ns + 1))
                xk[failed] = x0s.reshape(len(failed), -1)
                s.set(k, "x", xk if B > 1 else xk[0])
        if self.controller == "r2":
            veh = self.cfg["veh"]
            for k in range(1, N):
                for f, val in (("lbx", veh["delta_f_min"]), ("ubx", veh["delta_f_max"]), ("uh", 1.0)):
                    v = np.atleast_1d(s.constraints_get(k, f)).copy()
                    v[failed] = val
                    s.constraints_set(k, f, v if B > 1 else v[:1])

    def run(self, n_steps):
        if self.dev is not None:
            self.dev.run(n_steps)
            self.x_sim, self.x_mpc, self.pose = self.dev.get("x_sim"), self.dev.get("x_mpc"), self.dev.get("pose")
            self._last_logs = self.dev.logs() if self.dev.log_capacity else None
            return self._last_logs
        for _ in range(n_steps):
            self.step()
        self._last_logs = {k: np.array(v) for k, v in self.log.items()}          # arrays are (steps[+1], B, dim)
        return self._last_logs

    def save(self, path, instance=None, T=None, drop_last_step=True):
        """Write the loop's logs as the reference's Logger.save_logs does (Utils/Logging_Plotting.py:321-372: np.savez with the keys
        LOG_KEYS, yaw wrapped, derived deviation channels). instance = b: one file `path` for vehicle b -- what Papers_Plots and the
        RL / BO tooling read; instance = None: one file per vehicle, `path` formatted with the vehicle index ('logs/{}.npz' ->
        logs/0.npz, ... -- the layout of Learning_To_Adapt/SafeRL_WMPC/_baseline/F/<track>/<k>.npz). drop_last_step: as Logger.truncate
        does (log_file_arrays). Returns the paths written."""
        logs = self._last_logs
        if logs is None:
            raise Exception("ClosedLoopBatch.save: no logs (run() first; a device loop needs log_capacity > 0)")
        out = []
        w_deriv, e_est = self.w_deriv, self.e_est
        if self.dev is not None and any(getattr(self.dev, "disturbance_streams", ())):
            # a realisation drawn on the device is not stored anywhere: the logged steps' rows are regenerated (the same bits)
            w_deriv, e_est = self.dev.disturbance_table(0, len(logs["simU"]))
        for b in (range(self.B) if instance is None else [int(instance)]):
            f = path.format(b) if instance is None else path
            np.savez(f, **log_file_arrays(logs, b, w_deriv, e_est, T=T, Ts=self.Ts, drop_last_step=drop_last_step))
            out.append(f)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# Track segments: what the weight sweep runs the loop for (Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/objective_function.py:57-200;
# the RL environment ends an episode by the same rules, RL_WMPC/environment.py:152-165,239-240)

def gg_limits(vlong, cfg):
    """(ax_lim, ay_lim) of the gg table at vlong: piecewise linear, the outer pieces extended (the interpolant the OCP's
    constraint uses, NMPC_class.py:322-335; the same arithmetic as interp_lin of csrc/nmpc_device.hpp)"""
    g = cfg["ggv"]
    v, ax, ay = (np.asarray(g[k], dtype=float) for k in ("v", "ax", "ay"))
    vlong = np.asarray(vlong, dtype=float)
    i = np.clip(np.searchsorted(v, vlong, side="right") - 1, 0, len(v) - 2)
    out = []
    for y in (ax, ay):
        sl = (y[i + 1] - y[i]) / (v[i + 1] - v[i])
        out.append(y[i] + sl * (vlong - v[i]))
    return out[0], out[1]


def segment_step_channels(CiLX_s, simREF_s, a_next, cfg):
    """What Logger.logging_step derives in control step s (Utils/Logging_Plotting.py:152-179) from the plant state BEFORE the step
    (CiLX[s]), the first reference point of the step (simREF[s]) and x_next_MPC[7] (MPC_SimX[s + 1][7]): lat_dev (signed), vel_dev
    (signed), a_comb. Arrays over a leading batch axis."""
    _, lat = lon_lat_deviations(CiLX_s[..., 2], CiLX_s[..., 0], CiLX_s[..., 1], simREF_s[..., 0], simREF_s[..., 1])
    vel = CiLX_s[..., 3] - simREF_s[..., 3]
    ax, ay = gg_limits(CiLX_s[..., 3], cfg)
    ax = np.where(a_next > 0, ax, cfg["veh"]["acc_min"])
    alat = CiLX_s[..., 3] * CiLX_s[..., 5]
    return lat, vel, np.sqrt((a_next / ax) ** 2 + (alat / ay) ** 2)


def segment_scores_from_logs(logs, track, end_idx, max_lat_dev, max_a_comb, cfg=None, first_step=0):
    """The scores DeviceClosedLoop.segments() keeps on the device, from the five raw logs of a run -- the host statement of the same
    rules, and the path a caller without attach_segments has: per control step s >= first_step and instance b still active, the
    channels of segment_step_channels, the accumulators (steps, max |lat_dev|, sum vel_dev^2, max a_comb, failed solves), then the
    state bits, never cleared: 1 done (planner_emulator's index of the logged pose == end_idx[b]; end_idx[b] < 0: never),
    2 lat_dev > max_lat_dev (signed), 4 a_comb > max_a_comb (objective_function.py:139-146,188-200). The step that sets a bit is
    counted; nothing after it is. rms_vel_dev = sqrt(sum / steps) (0 before the first step)."""
    cfg = cfg or _config.default_config()
    CiLX, REF, SimX, DBG = (np.asarray(logs[k]) for k in ("CiLX", "simREF", "MPC_SimX", "simSolverDebug"))
    S, B = REF.shape[0], REF.shape[1]
    end_idx = np.broadcast_to(np.asarray(end_idx), (B,))
    steps = np.zeros(B, dtype=np.int64); state = np.zeros(B, dtype=np.int64); qpf = np.zeros(B, dtype=np.int64)
    max_lat = np.zeros(B); sumsq = np.zeros(B); max_ac = np.zeros(B)
    for s in range(first_step, S):
        act = state == 0
        if not act.any():
            break
        lat, vel, ac = segment_step_channels(CiLX[s], REF[s], SimX[s + 1][:, 7], cfg)
        closest = closest_index(track, CiLX[s][:, :2])
        steps[act] += 1
        max_lat[act] = np.maximum(max_lat[act], np.abs(lat[act]))
        sumsq[act] = sumsq[act] + vel[act] ** 2
        max_ac[act] = np.maximum(max_ac[act], ac[act])
        qpf[act] += (DBG[s][act, 4] != 0)
        bits = 1 * ((end_idx >= 0) & (closest == end_idx)) + 2 * (lat > max_lat_dev) + 4 * (ac > max_a_comb)
        state[act] = bits[act]
    rms = np.sqrt(np.divide(sumsq, steps, out=np.zeros(B), where=steps > 0))
    d = dict(steps=steps, state=state, max_lat_dev=max_lat, rms_vel_dev=rms, max_a_comb=max_ac, qp_failures=qpf)
    d.update(segment_flags(state))
    return d


def _objectives_from_groups(groups):
    """groups (P, n_groups, 4) as DeviceClosedLoop.segment_groups() orders them -> objectives (P, n_groups, 2), feasible (P,):
    a candidate with any segment not cleanly done is infeasible and ALL its objectives are NaN (objective_function.py:162-172)"""
    groups = np.asarray(groups, dtype=float)
    feasible = (groups[:, :, 3] == 0).all(axis=1)
    objectives = groups[:, :, :2].copy()
    objectives[~feasible] = np.nan
    return objectives, feasible


def segment_objectives(seg, n_candidates, group_sizes):
    """(objectives (P, n_groups, 2), feasible (P,)) from a per-segment dict (segments() / segment_scores_from_logs) of a
    candidate-major batch P x sum(group_sizes): per group the means of -max|lat_dev| and -rms(vel_dev)
    (objective_function.py:163,178-185), NaN rows for infeasible candidates."""
    P, sizes = int(n_candidates), [int(n) for n in group_sizes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    lat = np.asarray(seg["max_lat_dev"], dtype=float).reshape(P, off[-1])
    rms = np.asarray(seg["rms_vel_dev"], dtype=float).reshape(P, off[-1])
    bad = (np.asarray(seg["crashed"]) | np.asarray(seg["timed_out"])).reshape(P, off[-1])
    groups = np.zeros((P, len(sizes), 4))
    for g in range(len(sizes)):
        sl = slice(off[g], off[g + 1])
        groups[:, g, 0] = -lat[:, sl].mean(axis=1); groups[:, g, 1] = -rms[:, sl].mean(axis=1)
        groups[:, g, 2] = sizes[g]; groups[:, g, 3] = bad[:, sl].sum(axis=1)
    return _objectives_from_groups(groups)


def curvature_segments(track, name, curv_threshold_lo, curv_threshold_hi, overlap):
    """BO_WMPC/track_segmentation.py:8-49 curvature_segmentation on one race line (n, 4): the curvature |diff(unwrap(yaw))| / v of
    every waypoint but the last; a two-threshold switch over it -- on from a sample >= curv_threshold_hi, off from one
    <= curv_threshold_lo, unchanged in between, off at first (helpers.py:41-50 hysteresis) --; a segment between consecutive switching
    points, the last one closing on the FIRST again (so it wraps past the end of the line: its end is smaller than its start), widened
    by `overlap` waypoints on both sides and dropped when shorter than 20. type 0 (curve) where the curvature behind the switching
    point is above curv_threshold_lo, else 1 (straight). Returns (curves, straights), lists of dicts start, end, type, trajectory."""
    track = np.asarray(track, dtype=float)
    curv = np.abs(np.diff(np.unwrap(track[:, 2]))) / track[:-1, 3]
    on = np.zeros(len(curv), dtype=bool)
    state = False
    for i, k in enumerate(curv):
        if k >= curv_threshold_hi:
            state = True
        elif k <= curv_threshold_lo:
            state = False
        on[i] = state
    switch = np.nonzero(on[1:] != on[:-1])[0]
    groups = ([], [])
    for j in range(len(switch)):
        a, b = int(switch[j]), int(switch[(j + 1) % len(switch)])
        start, end = a - int(overlap), b + int(overlap)
        if abs(end - start) < 20:
            continue
        kind = 0 if curv[a + 1] > curv_threshold_lo else 1
        groups[kind].append(dict(start=start, end=end, type=kind, trajectory=name))
    return groups


def train_segments(curv_threshold_lo=2e-5, curv_threshold_hi=1e-3, overlap=10, tracks=("modena", "monteblanco")):
    """BO_WMPC/track_segmentation.py:52-83 get_train_segments: the two segment groups the reference's Bayesian optimisation drives --
    [curves, straights], each the segments of every track of `tracks` in that order (curvature_segments) -- in the reference's
    structure, which evaluate_segments takes as it is."""
    groups = [[], []]
    for name in tracks:
        for g, segs in enumerate(curvature_segments(load_track(name), name, curv_threshold_lo, curv_threshold_hi, overlap)):
            groups[g].extend(segs)
    return groups


def evaluate_segments(track_name, params, segment_groups, max_lat_dev, max_a_comb, max_steps, N=38, Tp=3.04, controller="nominal",
                      check_every=0, disturbances=None, seed=0, draw="legacy", **loop_kw):
    """objective_function (BO_WMPC/objective_function.py:57-175) for P candidate weight sets at once: params (P, 7) as in
    update_cost_function_weights, segment_groups a list of groups of (start, end) waypoint index pairs on the one track track_name, or
    -- the reference's structure, train_segments() -- of dicts with start, end and trajectory, every segment on its own track
    (track_name: None, or the sequence of names that fixes the order of the loop's track set; None: first appearance). One device loop
    of P x (number of segments) instances, candidate-major, then group, then the segments in the order given, every instance started at
    its segment's start and scored until the planner's index equals its end, it crashes, or max_steps have run. Returns (objectives
    (P, n_groups, 2), feasible (P,), per-segment dict).
    A candidate with a crashed or timed-out segment is infeasible and all its objectives are NaN. (The reference stops a candidate
    at its first crash; here all its segments run, the returned values are the same.)
    disturbances, seed, draw: as ClosedLoopBatch takes them -- draw="device" disturbs every segment for as long as it runs, with no
    disturbance_steps to guess (the other two need it among loop_kw).
    wmpc=(policy, table), weights_update_period, wmpc_on_failure among loop_kw: every segment drives under the learned weight
    schedule from the candidate's weights on (ClosedLoopBatch) -- a schedule scored on the training segments."""
    params = np.asarray(params, dtype=float).reshape(-1, 7)
    P = len(params)
    flat = [p for grp in segment_groups for p in grp]
    set_kw = {}
    if flat and isinstance(flat[0], dict):
        names = list(dict.fromkeys(p["trajectory"] for p in flat)) if track_name is None else \
            ([track_name] if isinstance(track_name, str) else list(track_name))
        missing = sorted({p["trajectory"] for p in flat} - set(names))
        if missing:
            raise ValueError(f"evaluate_segments: segments on {missing}, which track_name does not list")
        set_kw = dict(track_of=np.tile([names.index(p["trajectory"]) for p in flat], P))
        track_name = names
        flat = [(p["start"], p["end"]) for p in flat]
    pairs = np.array(flat, dtype=np.int64).reshape(-1, 2)
    sizes = [len(grp) for grp in segment_groups]
    S = len(pairs)
    off = np.concatenate([[0], np.cumsum(sizes)])
    offsets = np.concatenate([c * S + off[:-1] for c in range(P)] + [[P * S]])
    cl = ClosedLoopBatch(track_name, batch=P * S, params=np.repeat(params, S, axis=0), N=N, Tp=Tp, idx_start=np.tile(pairs[:, 0], P),
                         on_device=True, controller=controller, disturbances=disturbances, seed=seed, draw=draw, **set_kw, **loop_kw)
    cl.dev.attach_segments(np.tile(pairs[:, 1], P), max_lat_dev, max_a_comb, group_offsets=offsets)
    cl.dev.run_segments(max_steps, check_every)
    objectives, feasible = _objectives_from_groups(cl.dev.segment_groups().reshape(P, len(sizes), 4))
    return objectives, feasible, cl.dev.segments()


# ---------------------------------------------------------------------------------------------------------------------------
# The weight-scheduling RL environment (Learning_To_Adapt/SafeRL_WMPC/RL_WMPC/environment.py:112-240): every n_mpc_steps control
# steps an agent installs one row of a parameter table per vehicle; the environment answers with a reward and an observation.
# Host statements of what env_finish_kernel computes, and the environment itself.

def rl_observation(ref_yaw, ref_v, Ts, n_samples, lat_dev, vel_dev):
    """ObservationGenerator.get_observation (RL_WMPC/observation.py:28-75) of one local reference: [lat_dev, vel_dev], n_samples points
    of ref_v and of the yaw rate -- diff(unwrap(ref_yaw)) / Ts smoothed by a 10-tap moving average ('valid') -- at
    np.linspace(0, len - 1, n_samples, dtype=int) of each, normalised with the bounds of observation.py:16-24. Ts is the loop's
    sampling time although the points of the window are Tp / N apart: the reference's choice (environment.py:180)."""
    ref_v = np.asarray(ref_v, dtype=float)
    yaw_rate = np.diff(np.unwrap(np.asarray(ref_yaw, dtype=float))) / Ts
    yaw_rate = np.convolve(yaw_rate, np.ones(10) / 10, mode='valid')
    iv = np.linspace(0, len(ref_v) - 1, n_samples, dtype=int)
    ir = np.linspace(0, len(yaw_rate) - 1, n_samples, dtype=int)
    obs = np.concatenate((np.array([lat_dev, vel_dev]), ref_v[iv], yaw_rate[ir]))
    b = env_observation_bounds(n_samples)
    return (obs - b[0]) / (b[1] - b[0])


def wmpc_observation(x0, ref0, ref_yaw, ref_v, Ts, n_samples):
    """The observation the controller classes form for their agent at the end of solve() (NMPC_class.py:213-222, the same lines in the
    SNMPC and R2NMPC classes): lat_dev the lateral component of LonLatDeviations of the state the solve STARTED at (x0, what
    set_initial_state was handed) against the first point of this step's reference, vel_dev = x0[3] - ref_v[0], then
    rl_observation of the step's window (N + 1 points). Unlike the RL environment's, whose first two entries are always 0."""
    _, lat_dev = lon_lat_deviations(x0[2], x0[0], x0[1], ref0[0], ref0[1])
    vel_dev = x0[3] - ref_v[0]
    return rl_observation(ref_yaw, ref_v, Ts, n_samples, lat_dev, vel_dev)


class WmpcSchedule:
    """The learned weight schedule of the reference's controller classes (enable_WMPC; NMPC_class.py:208-239 and the same branch of
    the SNMPC and R2NMPC classes), stated once for `batch` instances: a counter c per instance, 0 at the start. After the solve of
    control step k: `if c >= period: c = 0; decide`, then -- in every case -- c += 1. period 20 decides after the solves of the steps
    20, 40, 60 (0-based); 1 from step 1 on; 0 at every step; a negative period is refused. Decide is policy.predict (deterministic:
    the first index of the largest logit, the observation rounded to float32) on wmpc_observation; the caller installs
    table[action] (update_cost_function_weights). A failed solve does not touch the counter. The first log_capacity decisions of
    every instance are stored (steps, actions, observations), every decision is counted: what wmpc_schedule_kernel keeps on the device.
    n_obs_stack > 1 of rl_config.yaml is not supported: the policy takes one observation of 2 + 2 n_samples entries."""

    def __init__(self, policy, table, period, batch=1, Ts=0.02, log_capacity=0):
        self.policy = policy
        self.table = np.ascontiguousarray(table, dtype=float)
        if self.table.ndim != 2 or self.table.shape[1] != 7:
            raise ValueError("WmpcSchedule: table must be (n_actions, 7)")
        if int(period) < 0:
            raise ValueError("WmpcSchedule: weights_update_period is negative (0 decides at every control step)")
        if policy.n_actions != len(self.table):
            raise ValueError(f"WmpcSchedule: the policy has {policy.n_actions} actions, the table {len(self.table)} rows")
        if policy.n_observations < 4 or policy.n_observations % 2:
            raise ValueError(f"WmpcSchedule: the policy takes {policy.n_observations} inputs; an observation has 2 + 2 n_samples entries")
        self.period, self.B, self.Ts = int(period), int(batch), float(Ts)
        self.n_samples = (policy.n_observations - 2) // 2
        self.counter = np.zeros(self.B, dtype=np.int64)
        L = int(log_capacity)
        self.n_decisions = np.zeros(self.B, dtype=np.int64)
        self.steps = np.full((self.B, L), -1, dtype=np.int64); self.actions = np.full((self.B, L), -1, dtype=np.int64)
        self.observations = np.zeros((self.B, L, policy.n_observations))
        self.current_action = [None] * self.B          # (self.current_action of the controller classes)

    def after_solve(self, k, x0, ref0, yref):
        """the branch behind the solve of control step k: x0 (B, 8) the states the solves started at, ref0 (B, 4) and yref
        (B, N + 1, 6) this step's reference (columns 2, 3 of yref: ref_yaw, ref_v). Returns (due instances, their actions)."""
        x0, ref0, yref = np.reshape(x0, (self.B, -1)), np.reshape(ref0, (self.B, -1)), np.asarray(yref).reshape(self.B, -1, 6)
        due = np.nonzero(self.counter >= self.period)[0]
        self.counter[due] = 0
        actions = []
        for b in due:
            obs = wmpc_observation(x0[b], ref0[b], yref[b, :, 2], yref[b, :, 3], self.Ts, self.n_samples)
            a = int(self.policy.predict(obs))
            n = self.n_decisions[b]
            if n < self.steps.shape[1]:
                self.steps[b, n], self.actions[b, n], self.observations[b, n] = k, a, obs
            self.n_decisions[b] += 1
            self.current_action[b] = a
            actions.append(a)
        self.counter += 1
        return due, np.array(actions, dtype=np.int64)


def rl_reward(lat_devs, vel_devs, sigmas, lims):
    """RewardGenerator.get_reward (RL_WMPC/reward.py:15-33) of the scored control steps of one environment step:
    exp(-sum(clip((m - lims[0]) / (lims[1] - lims[0]), 0, 1)^2 / (2 sigmas))), m = [rms(lat_devs), rms(vel_devs)]. lims[0] / lims[1]
    broadcast over m as numpy does: (2, 2) rows lower / upper per metric; the FLAT list environment.py:79-82 builds from the shipped
    rl_config.yaml, [0, 0.4, 0, 1], normalises both metrics with 0 .. 0.4."""
    lat_devs, vel_devs = np.asarray(lat_devs, dtype=float), np.asarray(vel_devs, dtype=float)
    sigmas, lims = np.array(sigmas), np.array(lims)
    m = np.array([np.sqrt(np.mean(lat_devs ** 2)), np.sqrt(np.mean(vel_devs ** 2))])
    m_nor = np.clip((m - lims[0]) / (lims[1] - lims[0]), 0., 1.)
    return 1.0 * np.exp(-np.sum(np.power(m_nor, 2) / (2 * sigmas)))


RL_SIGMAS = (0.1, 0.5)                       # _config/rl_config.yaml:33
RL_LIMS = (0.0, 0.4, 0.0, 1.0)               # rew_lims_lat_dev + rew_lims_vel_dev as environment.py:79-82 concatenates them (flat: see rl_reward)


def rl_env_steps_from_logs(logs, track, actions_per_step, n_mpc_steps, max_lat_dev=2.0, episode_length=128, sigmas=RL_SIGMAS,
                           lims=RL_LIMS, n_samples=10, full_lap=False, obs_states="reference", N=38, Tp=3.04, Ts=0.02, first_step=0):
    """The episode rules of RLEnvironment.step (environment.py:112-189) replayed on the five raw logs of a run that nothing reset: the
    host statement of what the device environment returns. Environment step e (one row of actions_per_step, (E, B); only its length is
    used -- the weights are in the logs already) covers the control steps first_step + e n_mpc_steps .. + n_mpc_steps - 1.
    Per instance: episode_steps += 1 (once per ENVIRONMENT step), then per control step lat_dev / vel_dev of
    segment_step_channels, truncated = lat_dev > max_lat_dev (signed), terminated = (planner index of the pose == len(track) - 2)
    with full_lap, else (episode_steps == episode_length); the step that sets a flag is counted, nothing after it is. Reward over the
    counted steps; observation from the planner's window at the last counted step, its first two entries 0 before normalisation with
    obs_states 'reference' (Logger.get_observation_states reads the row behind the last one written) or the last counted step's
    lat_dev / vel_dev with 'last_step'.
    Returns a dict of (E, B[, 2 + 2 n_samples]) arrays: reward, observation, terminated, truncated, step_length, qp_failures."""
    if obs_states not in ("reference", "last_step"):
        raise ValueError("obs_states must be 'reference' or 'last_step'")
    CiLX, REF, DBG = (np.asarray(logs[k]) for k in ("CiLX", "simREF", "simSolverDebug"))
    E, B = len(actions_per_step), REF.shape[1]
    if first_step + E * n_mpc_steps > REF.shape[0]:
        raise ValueError("rl_env_steps_from_logs: the logs are shorter than the environment steps asked for")
    out = dict(reward=np.zeros((E, B)), observation=np.zeros((E, B, 2 + 2 * n_samples)), terminated=np.zeros((E, B), dtype=bool),
               truncated=np.zeros((E, B), dtype=bool), step_length=np.zeros((E, B), dtype=np.int64), qp_failures=np.zeros((E, B), dtype=np.int64))
    episode_steps = np.zeros(B, dtype=np.int64)
    for e in range(E):
        episode_steps += 1
        s0 = first_step + e * n_mpc_steps
        for b in range(B):
            lats, vels = [], []
            terminated = truncated = False
            for s in range(s0, s0 + n_mpc_steps):
                _, lat = lon_lat_deviations(CiLX[s, b, 2], CiLX[s, b, 0], CiLX[s, b, 1], REF[s, b, 0], REF[s, b, 1])
                lats.append(lat); vels.append(CiLX[s, b, 3] - REF[s, b, 3])
                out["qp_failures"][e, b] += DBG[s, b, 4] != 0
                truncated = bool(lat > max_lat_dev)
                if full_lap:
                    terminated = bool(closest_index(track, CiLX[s, b, :2]) == len(track) - 2)
                else:
                    terminated = bool(episode_steps[b] == episode_length)
                if terminated or truncated:
                    break
            _, ref = planner_emulator(track, CiLX[s, b, :2], N + 1, Tp, True)
            last = (lats[-1], vels[-1]) if obs_states == "last_step" else (0.0, 0.0)
            out["reward"][e, b] = rl_reward(lats, vels, sigmas, lims)
            out["observation"][e, b] = rl_observation(ref[:, 2], ref[:, 3], Ts, n_samples, *last)
            out["terminated"][e, b], out["truncated"][e, b], out["step_length"][e, b] = terminated, truncated, len(lats)
    return out


def restart_lists(restart_indices, n_tracks):
    """restart_indices of a WeightScheduleEnv as one int64 array per track: one list serves every track, a sequence of n_tracks
    sequences gives each track its own"""
    seq = list(restart_indices) if not np.isscalar(restart_indices) else [restart_indices]
    if seq and all(np.ndim(r) == 1 for r in seq):
        if len(seq) != int(n_tracks):
            raise ValueError(f"restart_indices: one list, or one list per track ({int(n_tracks)})")
        lists = [np.asarray(r, dtype=np.int64) for r in seq]
    else:
        lists = [np.atleast_1d(np.asarray(restart_indices, dtype=np.int64))] * int(n_tracks)
    if any(r.ndim != 1 or len(r) < 1 for r in lists):
        raise ValueError("restart_indices: every list holds at least one waypoint")
    return lists


def draw_restarts(rng, lists, tracks):
    """environment.py:195-198 for the instances whose tracks are `tracks`, in that order: one rng.randint per instance into the list
    of its own track. Where every list has the same length the draws are ONE randint call of that size -- the stream a single list
    has always consumed -- and each instance indexes its own list with its draw."""
    tracks = np.asarray(tracks, dtype=np.int64)
    if len({len(r) for r in lists}) == 1:
        k = rng.randint(0, len(lists[0]), size=len(tracks))
    else:
        k = np.array([rng.randint(0, len(lists[t])) for t in tracks], dtype=np.int64)
    return np.array([lists[t][i] for t, i in zip(tracks, k)], dtype=np.int64)


class WeightScheduleEnv:
    """n_envs copies of the reference's RLEnvironment (RL_WMPC/environment.py) as ONE batched environment whose state stays
    on the device: reset() -> (obs, info), step(actions) -> (obs, reward, terminated, truncated, info), arrays over the n_envs axis.
    actions: the (A, 7) parameter table the integer actions index (rows as in update_cost_function_weights; the reference's
    actions_file). info: terminal_observation (the observation of the step itself, also where obs was replaced by a reset's zeros),
    step_length, qp_failures.
    auto_reset (as a VecEnv): an instance whose episode ended is reset at the start of the next step() to a waypoint drawn from
    restart_indices with numpy.random.RandomState(seed) (environment.py:195-198; one randint per reset instance, in instance order,
    reset() draws n_envs first), and the observation step() returns for it is already the zeros of reset(). auto_reset=False never
    resets: an ended instance drives on and is scored on -- for scoring a run; restart instances with reset(mask) where wanted.
    track_name: one track, or a sequence of T names with instance i on track_name[i % T] -- the reference's
    trajectories[i % n_trajs] (environment.py:283; rl_training.py:66 trains 16 environments on monteblanco and modena, 8 each) -- or on
    track_name[track_of[i]]; ONE object, one rollout buffer and one update over all tracks. restart_indices: one list for all tracks or
    one list per track (a sequence of T sequences); a reset instance draws from the list of its own track, still one randint per reset
    instance in instance order (equal lists: the stream of the single list). A full_lap episode ends at the last-but-one waypoint of
    the instance's own track. No gymnasium / stable_baselines3 needed."""

    def __init__(self, track_name, n_envs, actions, n_mpc_steps=20, max_lat_dev=2.0, episode_length=128, rew_sigmas=RL_SIGMAS,
                 rew_lims=RL_LIMS, obs_n_anticipation_points=10, full_lap=False, restart_indices=(0,), auto_reset=True, seed=0,
                 obs_states="reference", track_of=None, disturbances=None, draw="legacy", disturbance_seed=None, **loop_kw):
        self.table = np.ascontiguousarray(actions, dtype=float).reshape(-1, 7)
        self.n_envs, self.n_actions, self.n_mpc_steps = int(n_envs), len(self.table), int(n_mpc_steps)
        self.n_observations = 2 + 2 * int(obs_n_anticipation_points)
        n_tracks = 1 if isinstance(track_name, str) else len(track_name)
        self.track_of = np.zeros(self.n_envs, dtype=np.int64) if isinstance(track_name, str) else \
            (np.arange(self.n_envs) % n_tracks if track_of is None else np.asarray(track_of, dtype=np.int64))
        self.restart_lists = restart_lists(restart_indices, n_tracks)
        self.restart_indices = self.restart_lists[0]          # (the list of the first track: the only one of a single-track environment)
        self.auto_reset = bool(auto_reset)
        self._rng = np.random.RandomState(seed)
        for k in ("on_device", "controller", "batch", "params"):
            if k in loop_kw:
                raise ValueError(f"WeightScheduleEnv: '{k}' is the environment's to set")
        # (idx_start among loop_kw: where the loops stand until the first reset() -- one waypoint or one per instance)
        loop_kw.setdefault("idx_start", int(self.restart_indices[0]) if n_tracks == 1 else
                           np.array([self.restart_lists[t][0] for t in self.track_of], dtype=np.int64))
        if n_tracks > 1:
            loop_kw["track_of"] = self.track_of
        # disturbances / draw: as ClosedLoopBatch takes them, drawn with disturbance_seed (None: `seed`). draw="device" is what a
        # training run needs: the environment's global step only grows, and no table has a last step to be sized for
        self.loop = ClosedLoopBatch(track_name, batch=self.n_envs, on_device=True, controller="nominal", disturbances=disturbances, draw=draw,
                                    seed=int(seed if disturbance_seed is None else disturbance_seed), **loop_kw)
        self.dev = self.loop.dev
        self.dev.attach_env(self.table, n_mpc_steps, max_lat_dev, episode_length, rew_sigmas, rew_lims, obs_n_anticipation_points,
                            full_lap=full_lap, obs_states=obs_states)
        self._ended = np.zeros(self.n_envs, dtype=bool)
        self._next_obs = np.zeros((self.n_envs, self.n_observations))          # what an agent sees next (rollout)
        self._policy = None
        # collect(): the seed of the draws, the decision counter (one per environment step, whoever drives it) and whether what the
        # agent sees next begins an episode (_last_episode_starts of stable_baselines3)
        self._seed, self._t = int(seed), 0
        self._episode_starts = np.ones(self.n_envs)

    def _draw(self, instances):
        """start waypoints of the instances listed (with repeats: a start table), one randint each in the order given"""
        return draw_restarts(self._rng, self.restart_lists, self.track_of[np.asarray(instances, dtype=np.int64)])

    def reset(self, mask=None):
        """environment.py:191-237 for every instance (or those of the boolean mask): start waypoints drawn from restart_indices;
        the observation of a reset is all zeros (environment.py:230-233)."""
        m = np.ones(self.n_envs, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(self.n_envs)
        start = np.zeros(self.n_envs, dtype=np.int64)
        start[m] = self._draw(np.nonzero(m)[0])
        self.dev.env_reset(start, m)
        self._ended[m] = False
        self.last_start = start
        self._next_obs[m] = 0.0
        self._episode_starts[m] = 1.0
        return np.zeros((self.n_envs, self.n_observations)), {}

    def step(self, actions):
        mask = np.zeros(self.n_envs, dtype=np.int32)
        start = np.zeros(self.n_envs, dtype=np.int64)
        if self.auto_reset:
            mask[self._ended] = 1
            start[self._ended] = self._draw(np.nonzero(self._ended)[0])
        else:
            mask[self._ended] = 2
        r = self.dev.env_step(actions, mask, start)
        self.last_start = start
        self._ended = r["terminated"] | r["truncated"]
        obs = r["observation"]
        info = dict(terminal_observation=obs.copy(), step_length=r["step_length"], qp_failures=r["qp_failures"])
        if self.auto_reset:
            obs[self._ended] = 0.0
        self._next_obs = obs.copy()
        self._episode_starts = self._ended.astype(float)
        self._t += 1
        return obs, r["reward"], r["terminated"], r["truncated"], info

    def rollout(self, policy, n_steps, stop_when_done=False):
        """n_steps environment steps with `policy` (a WeightPolicy) choosing every action ON THE DEVICE: policy_kernel, the environment's
        kernels and the control steps are enqueued back to back, the host waits once at the end. What the policy sees first is what
        the last reset() / step() / rollout() returned (zeros after a reset). Equal, bit for bit, to step() driven with
        policy.predict(obs) on the host.
        auto_reset: an instance whose episode ends is reset at the next step and the policy sees zeros for it. The start waypoints are
        drawn BEFORE the rollout, one per step and instance -- self._draw(n_steps * n_envs), row e for the resets at the start of step
        e -- so the generator is consumed differently from step(), which draws one number per reset that happens: after a rollout the
        two no longer draw the same sequence.
        auto_reset=False: an ended instance is frozen out -- it drives on, live is False from the next step on and its rows are masked;
        stop_when_done ends the rollout once no instance is live (looked at after every step).
        Returns a dict of (E, B[, n_obs]) arrays over the E steps that ran: live (bool) and, as numpy masked arrays whose mask is
        ~live, action, reward, observation (of the step itself, as info['terminal_observation'] of step()), terminated, truncated,
        step_length, qp_failures."""
        E, B = int(n_steps), self.n_envs
        if self._policy is not policy:
            self.dev.attach_policy(policy)
            self._policy = policy
        table = self._draw(np.tile(np.arange(B), E)).reshape(E, B) if self.auto_reset else None
        r = self.dev.env_rollout(E, first_obs=self._next_obs, on_end=1 if self.auto_reset else 0, start_table=table,
                                 check_every=1 if stop_when_done else 0)
        live = r["live"]
        if len(live):
            self._ended = r["terminated"][-1] | r["truncated"][-1]
            self._episode_starts = self._ended.astype(float)
            self._t += len(live)
            self._next_obs = r["observation"][-1].copy()
            if self.auto_reset:
                self._next_obs[self._ended] = 0.0
                self.last_start = table[len(live) - 1]
        out = dict(live=live)
        for k, v in r.items():
            if k != "live":
                out[k] = np.ma.masked_array(v, mask=np.broadcast_to((~live).reshape(live.shape + (1,) * (v.ndim - 2)), v.shape))
        return out

    def collect(self, policy, n_steps, gamma, gae_lambda, seed=None):
        """What stable_baselines3's collect_rollouts and compute_returns_and_advantage leave in a RolloutBuffer, for n_steps environment
        steps ON THE DEVICE with one wait at the end: `policy` (a WeightPolicy WITH a value net) samples every action -- one Philox
        draw per instance and step, WeightPolicy.sample -- policy_ac_kernel, the environment, collect_next_kernel and gae_kernel are
        enqueued back to back. Equal, bit for bit, to the host-driven loop: dev.policy_eval_ac on the observation just returned,
        step(), the value of the terminal observations, gae().
        seed: of the draws (None: the environment's); the decision counter is the environment's: it advances by one per environment
        step (step() and rollout() included), so consecutive calls continue one stream, and one episode bookkeeping: episode_starts of
        the first row is what the last reset() / step() / rollout() / collect() left. The policy is attached anew at every call:
        changed weights between two calls are what a training loop has. Needs auto_reset=True; the start waypoints are drawn before
        the call as rollout() draws them. A PPOTrainer in place of the policy: the nets resident on the device -- the trainer's, as
        its updates left them -- act, and nothing is attached.
        Returns a dict of (E, B[, n_obs]) arrays: observations (what the policy saw), actions, log_probs, values, rewards (with
        gamma V(terminal observation) added where truncated and not terminated: the CRASH, environment.py:152-165), rewards_raw,
        episode_starts, advantages, returns, terminated, truncated, step_length, qp_failures; and last_values, last_dones (B,).
        Everything is float64 (stable_baselines3 keeps float32 buffers)."""
        E, B = int(n_steps), self.n_envs
        if not self.auto_reset:
            raise ValueError("WeightScheduleEnv.collect: needs auto_reset=True (an ended instance is reset, as in a VecEnv)")
        if isinstance(policy, PPOTrainer):
            if policy.dev is not self.dev:
                raise ValueError("WeightScheduleEnv.collect: the trainer belongs to another loop")
        elif getattr(policy, "value_weights", None) is None:
            raise ValueError("WeightScheduleEnv.collect: the policy carries no value net")
        if E < 1:
            raise ValueError("WeightScheduleEnv.collect: n_steps < 1")
        if not isinstance(policy, PPOTrainer):
            self.dev.attach_policy(policy)
        self._policy = policy
        table = self._draw(np.tile(np.arange(B), E)).reshape(E, B)
        r = self.dev.env_collect(E, table, self._seed if seed is None else int(seed), self._t, gamma, gae_lambda,
                                 first_obs=self._next_obs, first_episode_starts=self._episode_starts)
        self._t += E
        self._collected = E * B
        self._ended = r["terminated"][-1] | r["truncated"][-1]
        self._episode_starts = self._ended.astype(float)
        self._next_obs = r.pop("next_observation")
        self.last_start = table[-1]
        return r


# ---------------------------------------------------------------------------------------------------------------------------
# The random numbers of collect(): the project's own rule -- torch.multinomial's stream cannot be reproduced.

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., Random123): counter (..., 4) and key (..., 2) of 32-bit words -> (..., 4) uint32"""
    c = np.array(np.broadcast_arrays(*[np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]), dtype=np.uint64)
    k = [np.asarray(key, dtype=np.uint64)[..., i] for i in range(2)]
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M[0]) * c[0], np.uint64(PHILOX_M[1]) * c[2]
        c = np.array([(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32], dtype=np.uint64)
        k = [(k[0] + np.uint64(PHILOX_W[0])) & m32, (k[1] + np.uint64(PHILOX_W[1])) & m32]
    return np.moveaxis(c, 0, -1).astype(np.uint32)


def uniform_from_words(x0, x1):
    """u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 in [0, 1): integer work and an exact conversion"""
    m = (np.asarray(x0, dtype=np.uint64) >> np.uint64(5)) * np.uint64(1 << 26) + (np.asarray(x1, dtype=np.uint64) >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def policy_uniforms(seed, t, n, first_instance=0):
    """(n,) uniforms of the instances first_instance .. first_instance + n - 1 at decision t: key (seed & 0xffffffff, seed >> 32),
    counter (b, t & 0xffffffff, t >> 32, 0). A draw depends on (seed, b, t) alone."""
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    ctr = np.zeros((int(n), 4), dtype=np.uint64)
    ctr[:, 0] = (int(first_instance) + np.arange(int(n), dtype=np.uint64)) & np.uint64(0xffffffff)
    ctr[:, 1], ctr[:, 2] = t & 0xffffffff, t >> 32
    x = philox4x32(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    return uniform_from_words(x[:, 0], x[:, 1])


def gae(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """RolloutBuffer.compute_returns_and_advantage on (E, B) float64 arrays, in the association gae_kernel uses: (advantages, returns)"""
    rewards, values, episode_starts = (np.asarray(a, dtype=np.float64) for a in (rewards, values, episode_starts))
    E = rewards.shape[0]
    adv = np.zeros_like(rewards)
    last = np.zeros(rewards.shape[1:])
    for t in range(E - 1, -1, -1):
        nnt = 1.0 - (np.asarray(last_dones, dtype=np.float64) if t == E - 1 else episode_starts[t + 1])
        nv = np.asarray(last_values, dtype=np.float64) if t == E - 1 else values[t + 1]
        delta = (rewards[t] + (gamma * nv) * nnt) - values[t]
        last = delta + ((gamma * gae_lambda) * nnt) * last
        adv[t] = last
    return adv, adv + values


class WeightPolicy:
    """The trained agent of the reference as DATA: the policy net of a stable_baselines3 MlpPolicy -- Linear / Tanh hidden layers
    (mlp_extractor.policy_net, rl_training.py:116-121) and the linear action layer (action_net) -- and its deterministic decision,
    model.predict(obs, deterministic=True): the first index of the largest logit. This is the HOST statement, in float64 numpy on
    the float32 weights, the observation rounded to float32 first as stable_baselines3 does; policy_kernel computes the same on the
    device (DeviceClosedLoop.attach_policy). No training.
    weights: float32 (out, in) matrices as torch stores them, biases: float32 (out,) vectors; the last pair is the action layer.
    value_weights / value_biases (optional): the value net of the same archive (mlp_extractor.value_net, value_net) with its own
    hidden layers, the same inputs and a last matrix of one row. With it the object also states what collecting training data needs:
    values, log_prob and sample -- the sampling rule of policy_ac_kernel. Without it the object is the inference-only one."""

    def __init__(self, weights, biases, value_weights=None, value_biases=None):
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
        if len(self.weights) < 2 or len(self.weights) != len(self.biases):
            raise ValueError("WeightPolicy: at least one hidden layer and the action layer, one bias per weight matrix")
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],) or (i and w.shape[1] != self.weights[i - 1].shape[0]):
                raise ValueError(f"WeightPolicy: layer {i} does not fit: weight {w.shape}, bias {b.shape}")
        self.n_observations, self.n_actions = self.weights[0].shape[1], self.weights[-1].shape[0]
        self.value_weights = self.value_biases = None
        if (value_weights is None) != (value_biases is None):
            raise ValueError("WeightPolicy: a value net is value_weights AND value_biases")
        if value_weights is not None:
            vw = [np.ascontiguousarray(w, dtype=np.float32) for w in value_weights]
            vb = [np.ascontiguousarray(b, dtype=np.float32) for b in value_biases]
            if len(vw) < 2 or len(vw) != len(vb):
                raise ValueError("WeightPolicy: the value net has at least one hidden layer and the value layer, one bias per weight matrix")
            for i, (w, b) in enumerate(zip(vw, vb)):
                if w.ndim != 2 or b.shape != (w.shape[0],) or (i and w.shape[1] != vw[i - 1].shape[0]):
                    raise ValueError(f"WeightPolicy: value layer {i} does not fit: weight {w.shape}, bias {b.shape}")
            if vw[0].shape[1] != self.n_observations:
                raise ValueError(f"WeightPolicy: the value net takes {vw[0].shape[1]} inputs, the policy net {self.n_observations}")
            if vw[-1].shape[0] != 1:
                raise ValueError("WeightPolicy: the last matrix of the value net has one row")
            self.value_weights, self.value_biases = vw, vb

    @classmethod
    def from_npz(cls, path, value_path=None):
        """the fixture format: W0, W1, ... and b0, b1, ... (tests/golden/wmpc_policy.npz); the value net V0, V1, ... and c0, c1, ...
        where `path` -- or value_path, a second file (tests/golden/wmpc_value.npz) -- holds them"""
        d = np.load(path)
        n = 0
        while f"W{n}" in d.files:
            n += 1
        missing = [f"b{i}" for i in range(n) if f"b{i}" not in d.files]
        if n == 0 or missing:
            raise ValueError(f"WeightPolicy.from_npz: {path} holds no W0, W1, ... / lacks {missing}")
        v = d if value_path is None else np.load(value_path)
        m = 0
        while f"V{m}" in v.files:
            m += 1
        missing = [f"c{i}" for i in range(m) if f"c{i}" not in v.files]
        if missing or (value_path is not None and m == 0):
            raise ValueError(f"WeightPolicy.from_npz: {value_path or path} holds no V0, V1, ... / lacks {missing}")
        value = ([v[f"V{i}"] for i in range(m)], [v[f"c{i}"] for i in range(m)]) if m else (None, None)
        return cls([d[f"W{i}"] for i in range(n)], [d[f"b{i}"] for i in range(n)], *value)

    @classmethod
    def from_sb3_zip(cls, path):
        """a stable_baselines3 archive (model.save: best_model.zip): its policy.pth is a plain state dict, read with zipfile and
        torch.load(weights_only=True) -- stable_baselines3 is not needed. Takes mlp_extractor.policy_net.<i>.weight / .bias and
        action_net.weight / .bias, and -- when the archive has them -- mlp_extractor.value_net.<i> and value_net as the value net; a
        shared trunk (mlp_extractor.shared_net) is refused, and so are missing keys."""
        import io
        import re
        import zipfile

        import torch
        with zipfile.ZipFile(path) as z:
            if "policy.pth" not in z.namelist():
                raise ValueError(f"WeightPolicy.from_sb3_zip: {path} holds no policy.pth")
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        if any(k.startswith("mlp_extractor.shared_net") for k in sd):
            raise ValueError("WeightPolicy.from_sb3_zip: the policy has a shared trunk (mlp_extractor.shared_net): not supported")
        idx = sorted(int(m.group(1)) for m in (re.fullmatch(r"mlp_extractor\.policy_net\.(\d+)\.weight", k) for k in sd) if m)
        names = [f"mlp_extractor.policy_net.{i}" for i in idx] + ["action_net"]
        missing = [f"{n}.{p}" for n in names for p in ("weight", "bias") if f"{n}.{p}" not in sd]
        if not idx or missing:
            raise ValueError(f"WeightPolicy.from_sb3_zip: missing keys {missing or ['mlp_extractor.policy_net.*.weight']}")
        vidx = sorted(int(m.group(1)) for m in (re.fullmatch(r"mlp_extractor\.value_net\.(\d+)\.weight", k) for k in sd) if m)
        value = (None, None)
        if vidx or "value_net.weight" in sd:
            vnames = [f"mlp_extractor.value_net.{i}" for i in vidx] + ["value_net"]
            missing = [f"{n}.{p}" for n in vnames for p in ("weight", "bias") if f"{n}.{p}" not in sd]
            if not vidx or missing:
                raise ValueError(f"WeightPolicy.from_sb3_zip: missing keys {missing or ['mlp_extractor.value_net.*.weight']}")
            value = ([sd[n + ".weight"].numpy() for n in vnames], [sd[n + ".bias"].numpy() for n in vnames])
        return cls([sd[n + ".weight"].numpy() for n in names], [sd[n + ".bias"].numpy() for n in names], *value)

    def _forward(self, obs, weights, biases):
        x = np.asarray(obs, dtype=np.float64)
        h = np.atleast_2d(x).astype(np.float32).astype(np.float64)          # obs_as_tensor: float32 before the first layer
        if h.shape[1] != self.n_observations:
            raise ValueError(f"WeightPolicy: observations have {self.n_observations} entries")
        for i, (w, b) in enumerate(zip(weights, biases)):
            h = h @ w.astype(np.float64).T + b.astype(np.float64)
            if i + 1 < len(weights):
                h = np.tanh(h)
        return h[0] if x.ndim == 1 else h

    def logits(self, obs):
        """(n, n_actions) float64 (or (n_actions,) for one observation)"""
        return self._forward(obs, self.weights, self.biases)

    def values(self, obs):
        """(n,) float64 (a scalar for one observation): the value net"""
        if self.value_weights is None:
            raise ValueError("WeightPolicy.values: no value net")
        return self._forward(obs, self.value_weights, self.value_biases)[..., 0]

    def _prefix_sums(self, obs):
        """z - max z and the prefix sums, in index order, of exp(z - max z): (n, A) each"""
        z = np.atleast_2d(self.logits(obs))
        d = z - z.max(axis=-1, keepdims=True)
        return d, np.cumsum(np.exp(d), axis=-1)

    def log_prob(self, obs, actions):
        """(n,) log-probability of the given actions: (z_a - max z) - log S, S the sum of exp(z - max z) in index order"""
        d, c = self._prefix_sums(obs)
        a = np.broadcast_to(np.asarray(actions, dtype=np.int64), (len(d),))
        return d[np.arange(len(d)), a] - np.log(c[:, -1])

    def sample(self, obs, seed, t, first_instance=0):
        """(n,) sampled actions, row i with the uniform u of (seed, first_instance + i, t) (policy_uniforms): the smallest j with
        u S < c_j, c the prefix sums of exp(z - max z) in index order and S the last of them; n_actions - 1 if there is none"""
        d, c = self._prefix_sums(obs)
        u = policy_uniforms(seed, t, len(d), first_instance)
        below = (u * c[:, -1])[:, None] < c
        return np.where(below.any(axis=1), np.argmax(below, axis=1), self.n_actions - 1)

    def probabilities(self, obs):
        """get_action_probabilities (helpers.py:100-105): the softmax of the logits"""
        z = self.logits(obs)
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    def predict(self, obs):
        """model.predict(obs, deterministic=True): the first index of the largest logit"""
        return np.argmax(self.logits(obs), axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# The PPO update (stable_baselines3 PPO.train as rl_training.py:133-155 configures it). ppo_loss_and_grads and adam_step are the HOST
# statements -- float64 numpy, the role WeightPolicy._forward has for the nets -- of what ppo_tile_kernel / ppo_wgrad_kernel /
# ppo_adam_kernel compute on the device.

def learning_rate_schedule(initial, final, k):
    """helpers.py:88-97: remaining (1 at the start of training, 0 at its end) -> initial (final / initial)^((1 - remaining) k)"""
    initial, final, k = float(initial), float(final), float(k)

    def func(remaining):
        return initial * (final / initial) ** ((1.0 - float(remaining)) * k)
    return func


def minibatch_slices(N, batch_size):
    """[k batch_size, min((k + 1) batch_size, N)) for k = 0, 1, ...: the last minibatch may be short, as in stable_baselines3"""
    N, bs = int(N), int(batch_size)
    if N < 1 or bs < 1:
        raise ValueError("minibatch_slices: N and batch_size must be >= 1")
    bs = min(bs, N)
    return [slice(k, min(k + bs, N)) for k in range(0, N, bs)]


def _tanh_net(h, weights, biases):
    """the layers of _forward with the input of every matrix kept: (output (n, out), [h_0, h_1, ...])"""
    hs = []
    for i, (w, b) in enumerate(zip(weights, biases)):
        hs.append(h)
        h = h @ w.astype(np.float64).T + b.astype(np.float64)
        if i + 1 < len(weights):
            h = np.tanh(h)
    return h, hs


def _tanh_net_grads(delta, weights, hs):
    """delta = dL/d(output) (n, out) back through the layers: ([dW_l], [db_l])"""
    gW, gb = [None] * len(weights), [None] * len(weights)
    for l in range(len(weights) - 1, -1, -1):
        gW[l], gb[l] = delta.T @ hs[l], delta.sum(axis=0)
        if l:
            delta = (delta @ weights[l].astype(np.float64)) * (1.0 - hs[l] * hs[l])
    return gW, gb


def ppo_loss_and_grads(policy, obs, actions, old_log_probs, advantages, returns, clip_range=0.2, ent_coef=0.006, vf_coef=0.5,
                       normalize_advantage=True):
    """Loss, diagnostics and the gradient of every weight and bias of one minibatch, float64: the host statement of the device's
    ppo_step(apply=False). `policy`: a WeightPolicy with a value net. Returns a dict: loss, policy_loss, value_loss, entropy_loss,
    approx_kl, clip_fraction, grad_norm (before clipping), ratio (n,), log_probs (n,), values (n,) and grads = (weights, biases,
    value_weights, value_biases) lists of float64 arrays shaped as the parameters."""
    obs = np.atleast_2d(np.asarray(obs, dtype=np.float64))
    n = len(obs)
    a = np.asarray(actions, dtype=np.int64).reshape(n)
    old, adv, ret = (np.asarray(x, dtype=np.float64).reshape(n) for x in (old_log_probs, advantages, returns))
    if policy.value_weights is None:
        raise ValueError("ppo_loss_and_grads: the policy carries no value net")
    A = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8) if normalize_advantage and n > 1 else adv
    h0 = obs.astype(np.float32).astype(np.float64)
    z, hs = _tanh_net(h0, policy.weights, policy.biases)
    V, vhs = _tanh_net(h0, policy.value_weights, policy.value_biases)
    V = V[:, 0]
    d = z - z.max(axis=-1, keepdims=True)
    logp = d - np.log(np.cumsum(np.exp(d), axis=-1)[:, -1:])          # (the sum in index order: WeightPolicy.log_prob)
    p = np.exp(logp)
    H = -(p * logp).sum(axis=-1)
    rows = np.arange(n)
    lp = logp[rows, a]
    lr = lp - old
    r = np.exp(lr)
    s1, s2 = A * r, A * np.clip(r, 1.0 - clip_range, 1.0 + clip_range)
    policy_loss, value_loss, entropy_loss = -np.minimum(s1, s2).mean(), ((ret - V) ** 2).mean(), -H.mean()
    # backwards: the unclipped term carries the gradient where it is the smaller one (or both are equal)
    glp = np.where(s1 <= s2, -s1, 0.0)
    onehot = np.zeros_like(z)
    onehot[rows, a] = 1.0
    dz = (glp[:, None] * (onehot - p) + ent_coef * (p * (logp + H[:, None]))) / n
    dV = (vf_coef * (2.0 * (V - ret)) / n)[:, None]
    gW, gb = _tanh_net_grads(dz, policy.weights, hs)
    gVW, gVb = _tanh_net_grads(dV, policy.value_weights, vhs)
    norm = np.sqrt(sum(float((g * g).sum()) for g in gW + gb + gVW + gVb))
    return dict(loss=policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss=policy_loss, value_loss=value_loss,
                entropy_loss=entropy_loss, approx_kl=((r - 1.0) - lr).mean(), clip_fraction=(np.abs(r - 1.0) > clip_range).mean(),
                grad_norm=norm, ratio=r, log_probs=lp, values=V, grads=(gW, gb, gVW, gVb))


def adam_step(params, grads, m, v, t, lr, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5):
    """Gradient clipping and one Adam step, float64, on lists of arrays: the host statement of ppo_adam_kernel BEFORE the rounding to
    float32. total = sqrt(sum g^2) over all tensors, g <- min(1, max_grad_norm / (total + 1e-6)) g; then, with t the number of this
    step (1 for the first), m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2, theta <- theta - (lr / (1 - b1^t)) m / (sqrt(v) /
    sqrt(1 - b2^t) + eps). Returns (new params, new m, new v, total), params and moments float64; the caller rounds."""
    b1, b2 = betas
    g64 = [np.asarray(g, dtype=np.float64) for g in grads]
    total = np.sqrt(sum(float((g * g).sum()) for g in g64))
    coef = min(1.0, max_grad_norm / (total + 1e-6))
    step, bc2 = lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)
    P, M, V = [], [], []
    for th, g, m0, v0 in zip(params, g64, m, v):
        g = coef * g
        m1 = b1 * np.asarray(m0, dtype=np.float64) + (1.0 - b1) * g
        v1 = b2 * np.asarray(v0, dtype=np.float64) + ((1.0 - b2) * g) * g
        P.append(np.asarray(th, dtype=np.float64) - (step * m1) / (np.sqrt(v1) / bc2 + eps))
        M.append(m1); V.append(v1)
    return P, M, V, total


class PPOTrainer:
    """The PPO update of `policy` (a WeightPolicy WITH a value net) on the device of `env_or_loop` (a WeightScheduleEnv, a
    ClosedLoopBatch with on_device=True or a DeviceClosedLoop): attaches the policy and the trainer. From then on the nets live on the
    device: step() and update() change them in place, WeightScheduleEnv.collect(trainer, ...) acts with them, policy() downloads them.
    Parameters are float32, everything else FP64, the new parameter the FP64 Adam result rounded once."""

    def __init__(self, env_or_loop, policy, clip_range=0.2, ent_coef=0.006, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True):
        if getattr(policy, "value_weights", None) is None:
            raise ValueError("PPOTrainer: the policy carries no value net")
        self.env = env_or_loop if isinstance(env_or_loop, WeightScheduleEnv) else None
        self.dev = getattr(env_or_loop, "dev", env_or_loop)
        self.settings = dict(clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                             normalize_advantage=normalize_advantage)
        self.dev.attach_policy(policy)
        self.dev.ppo_attach(**self.settings)
        if self.env is not None:
            self.env._policy = self

    def step(self, obs, actions, old_log_probs, advantages, returns, lr, apply=True, want_grads=False, want_rows=False):
        """one minibatch from host arrays: the dict of diagnostics (DeviceClosedLoop.ppo_step)"""
        return self.dev.ppo_step(obs, actions, old_log_probs, advantages, returns, lr, apply=apply, want_grads=want_grads, want_rows=want_rows)

    def update(self, buffer=None, perm=None, n_epochs=5, batch_size=4096, lr=3e-4, seed=0):
        """One update: n_epochs passes over the buffer in minibatches of batch_size, one wait. buffer: what collect() returned (its
        (E, B) arrays are flattened in C order), or None: the rows the last collect() left on the device. perm (n_epochs, N), or None:
        numpy.random.RandomState(seed).permutation(N) per epoch, drawn in epoch order from one generator."""
        if buffer is None:
            if self.env is None:
                raise ValueError("PPOTrainer.update: without a buffer the trainer needs a WeightScheduleEnv whose collect() left one on the device")
            N = getattr(self.env, "_collected", 0)
            if N < 1:
                raise ValueError("PPOTrainer.update: no buffer given and nothing collected yet")
            rows = None
        else:
            acts = np.asarray(buffer["actions"])
            N = acts.size
            rows = (np.asarray(buffer["observations"], dtype=np.float64).reshape(N, -1), acts.reshape(N),
                    *(np.asarray(buffer[k], dtype=np.float64).reshape(N) for k in ("log_probs", "advantages", "returns")))
        if perm is None:
            rng = np.random.RandomState(seed)
            perm = np.stack([rng.permutation(N) for _ in range(int(n_epochs))])
        return self.dev.ppo_update(N, perm, batch_size, lr, buffer=rows)

    def policy(self):
        """the nets the device acts with, as a WeightPolicy"""
        return WeightPolicy(*self.dev.ppo_params())

    def state(self):
        """Adam's moments and step counter (DeviceClosedLoop.ppo_state)"""
        return self.dev.ppo_state()


def learn(env, trainer, n_updates, n_steps, batch_size, n_epochs, gamma, gae_lambda, lr_schedule, seed=0):
    """The loop of stable_baselines3's model.learn on the device: n_updates x (collect n_steps environment steps with the trainer's
    resident nets, one update on the buffer collect left on the device). lr_schedule: a number, or a function of the remaining
    progress (1 -> 0, learning_rate_schedule), evaluated before each update as stable_baselines3 does. The permutations of update u
    come from RandomState(seed + u). Returns the list of per-update diagnostics (PPOTrainer.update)."""
    out = []
    for u in range(int(n_updates)):
        env.collect(trainer, n_steps, gamma, gae_lambda)
        # (_update_current_progress_remaining: 1 - num_timesteps / total_timesteps, after the collection)
        remaining = 1.0 - (u + 1) / float(n_updates)
        lr = lr_schedule(remaining) if callable(lr_schedule) else float(lr_schedule)
        out.append(trainer.update(None, None, n_epochs, batch_size, lr, seed=seed + u))
    return out


def run_policy(track_name, policy, table, starts, max_steps=400, n_mpc_steps=20, check_every=1, n_obs_stack=1, **env_kw):
    """RL_WMPC/evaluation.py:65-105 run_policy for MANY start waypoints at once: one vehicle per entry of `starts` on `track_name` -- or,
    with a sequence of names and track_of (one track id per start; None: i % T) among env_kw, each on its own track --,
    full_lap=True and no restarts -- an episode ends at the last-but-one waypoint of ITS track or when the vehicle leaves it -- with
    `policy` (a WeightPolicy) picking rows of `table` (A, 7) every n_mpc_steps control steps, on the device, until every instance has
    ended or max_steps environment steps have run. env_kw: further arguments of WeightScheduleEnv (N, Tp, max_lat_dev, log_capacity ...;
    by default the five logs of all control steps are kept).
    Returns a dict: actions (E, B) and probabilities (E, B, A) -- get_action_probabilities of what the policy saw at each decision,
    through the device policy -- masked where the instance had ended; live (E, B); n_decisions (B,); rollout: everything
    WeightScheduleEnv.rollout returned; logs: the loop's logs (None with log_capacity=0); env: the environment."""
    if int(n_obs_stack) != 1:
        raise ValueError("run_policy: n_obs_stack > 1 (VecFrameStack) is not supported; every shipped config has 1")
    starts = np.atleast_1d(np.asarray(starts))
    if starts.ndim != 1 or not np.issubdtype(starts.dtype, np.integer):
        raise ValueError("run_policy: starts is a list of waypoint indices")
    for k in ("full_lap", "auto_reset", "restart_indices", "idx_start"):
        if k in env_kw:
            raise ValueError(f"run_policy: '{k}' is run_policy's to set")
    B = len(starts)
    env_kw.setdefault("log_capacity", int(max_steps) * int(n_mpc_steps))
    env = WeightScheduleEnv(track_name, B, table, n_mpc_steps=n_mpc_steps, full_lap=True, auto_reset=False, idx_start=starts.astype(np.int64), **env_kw)
    r = env.rollout(policy, int(max_steps), stop_when_done=check_every > 0)
    live = r["live"]
    E = len(live)
    seen = np.concatenate([np.zeros((1, B, env.n_observations)), r["observation"].data[:-1]])          # environment.py:230-233: reset() returns zeros
    probs = env.dev.policy_eval(seen.reshape(E * B, -1))["probabilities"].reshape(E, B, -1)
    probs = np.ma.masked_array(probs, mask=np.broadcast_to(~live[:, :, None], probs.shape))
    return dict(actions=r["action"], probabilities=probs, live=live, n_decisions=live.sum(axis=0), rollout=r,
                logs=env.dev.logs() if env.dev.log_capacity > 0 else None, env=env)
