#!/usr/bin/env python3
"""
tests/golden/make_rl_env_golden.py -- regenerates rl_env.npz in this directory.

Runs only where the reference tree exists (REF below; the fixture is committed, the tests never need this script). It imports the
reference's ObservationGenerator and RewardGenerator (Learning_To_Adapt/SafeRL_WMPC/RL_WMPC/observation.py, reward.py) with stubs for
the third-party modules that are absent, as make_golden.py does, and writes DATA only -- inputs and the outputs the reference computes:

  F                       the 26 rows of Learning_To_Adapt/SafeRL_WMPC/_parameters/F.csv (the RL agent's action table)
  obs_<i>_ref_yaw / _ref_v / _args / _out   PlannerEmulator windows (N + 1 points; N = 38 and N = 12, n_samples = 10, so indices
                          repeat at N = 12), args = [Ts, n_samples, lat_dev, vel_dev], out = get_observation(...). At least one
                          window crosses the yaw seam (asserted here: |diff(ref_yaw)| > pi somewhere)
  rew_<i>_lat / _vel / _sigmas / _lims / _out   lat_devs / vel_devs series of 1, 5 and 20 control steps, sigmas, lims as
                          environment.py:79-82 builds them, out = get_reward(logger, step_length)
"""
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


class _Stub(types.ModuleType):
    """an absent third-party module: any name imported from it is a placeholder nothing here calls"""
    __path__ = []

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return type(item, (), {})


sys.path.insert(0, REF)


def _import_with_stubs(module, names):
    """import `names` from a reference module; every third-party module that is absent here becomes a stub, one at a time"""
    for _ in range(64):
        try:
            m = __import__(module, fromlist=list(names))
            return [getattr(m, n) for n in names]
        except ModuleNotFoundError as e:
            if not e.name or e.name.split(".")[0] in ("Utils", "Learning_To_Adapt", "Model_Predictive_Controller", "Vehicle_Simulator"):
                raise
            sys.modules[e.name] = _Stub(e.name)
            if e.name == "casadi":
                sys.modules[e.name].__dict__["__all__"] = []
    raise ImportError(module)


PlannerEmulator, = _import_with_stubs("Utils.MPC_sim_utils", ["PlannerEmulator"])
ObservationGenerator, = _import_with_stubs("Learning_To_Adapt.SafeRL_WMPC.RL_WMPC.observation", ["ObservationGenerator"])
RewardGenerator, = _import_with_stubs("Learning_To_Adapt.SafeRL_WMPC.RL_WMPC.reward", ["RewardGenerator"])


def main():
    out = {"F": np.loadtxt(os.path.join(REF, "Learning_To_Adapt/SafeRL_WMPC/_parameters/F.csv"), delimiter=",")}
    assert out["F"].shape == (26, 7)
    with open(os.path.join(REF, "Trajectories", "reftraj_monteblanco_edgar.json")) as f:
        traj = json.load(f)
    px, py, yaw = (np.asarray(traj[k], float) for k in ("pos_x", "pos_y", "ref_yaw"))
    seam = np.nonzero(np.abs(np.diff(yaw)) > np.pi)[0]
    assert len(seam), "the race line never crosses the yaw seam"
    rng = np.random.RandomState(7)
    # poses: a few waypoints (slightly off the line), and one a handful of points in front of the seam
    starts = [0, 137, 800, int(seam[0]) - 6, int(seam[0]) - 1]
    gen = ObservationGenerator(anticipation_horizon=38, n_anticipation_points=10)
    i, crossed = 0, False
    for N, Tp in ((38, 3.04), (12, 3.04)):
        for w in starts:
            pose = np.array([px[w], py[w]]) + 0.3 * rng.randn(2)
            _, ref = PlannerEmulator(traj, pose, N + 1, Tp, True)
            ref_yaw, ref_v = np.asarray(ref["ref_yaw"], float), np.asarray(ref["ref_v"], float)
            crossed |= bool((np.abs(np.diff(ref_yaw)) > np.pi).any())
            lat, vel = (0.0, 0.0) if i % 2 == 0 else (float(rng.uniform(-2, 2)), float(rng.uniform(-4, 4)))
            obs = gen.get_observation(0.0, lat, vel, {"ref_yaw": ref_yaw, "ref_v": ref_v}, 0.02)
            out[f"obs_{i}_ref_yaw"], out[f"obs_{i}_ref_v"] = ref_yaw, ref_v
            out[f"obs_{i}_args"], out[f"obs_{i}_out"] = np.array([0.02, 10, lat, vel]), np.asarray(obs, float)
            i += 1
    assert crossed, "no window crosses the yaw seam"
    out["n_obs"] = np.array(i)
    # rewards: lims in the two shapes environment.py:79-82 can produce -- (2, 2) from [[lo, hi]] entries, flat from the shipped
    # rl_config.yaml's [lo, hi] entries -- and series whose rms lies below lims[0], between, and above lims[1]
    lims22 = np.concatenate([[[0.05, 0.4]], [[0.2, 1.0]]]).transpose()
    limsflat = np.concatenate([[0.0, 0.4], [0.0, 1.0]]).transpose()
    j = 0
    for lims in (lims22, limsflat):
        for n in (1, 5, 20):
            for scale_lat, scale_vel in ((0.01, 0.05), (0.2, 0.6), (1.5, 3.0)):
                lat, vel = scale_lat * rng.randn(n), scale_vel * rng.randn(n)
                sig = np.array([0.1, 0.5])
                logger = types.SimpleNamespace(lat_devs=np.concatenate([rng.randn(3), lat]), vel_devs=np.concatenate([rng.randn(3), vel]),
                                               current_step=3 + n)
                r = RewardGenerator(sig, lims).get_reward(logger, step_length=n)
                out[f"rew_{j}_lat"], out[f"rew_{j}_vel"], out[f"rew_{j}_sigmas"], out[f"rew_{j}_lims"] = lat, vel, sig, lims
                out[f"rew_{j}_out"] = np.array(float(r))
                j += 1
    out["n_rew"] = np.array(j)
    np.savez(os.path.join(OUT, "rl_env.npz"), **out)
    print(f"rl_env.npz: {i} observations, {j} rewards")


if __name__ == "__main__":
    main()
