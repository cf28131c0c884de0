#!/usr/bin/env python3
"""
tests/golden/make_wmpc_schedule_golden.py -- regenerates wmpc_schedule.npz in this directory.

Runs only where the reference tree exists (REF below; the fixture is committed, the tests never need this script). It imports the
reference's ObservationGenerator (Learning_To_Adapt/SafeRL_WMPC/RL_WMPC/observation.py) and LonLatDeviations (Utils/MPC_sim_utils.py)
with stubs for the third-party modules that are absent, as make_rl_env_golden.py does, and writes DATA only -- inputs and the outputs
the reference computes for them, the statements NMPC_class.py:213-222 makes at a decision step:

  n                       number of cases
  case_<i>_x0             the state the solve started at (8,): a point of the race line moved sideways by up to +- 2 m, its speed by
                          up to +- 3 m/s, its yaw by up to +- 0.05 rad
  case_<i>_ref            this step's window (N + 1, 4) [pos_x, pos_y, ref_yaw, ref_v] from the PROJECT's planner emulator
                          (tum_control_amd.planner.planner_emulator) on Monteblanco and Modena; N = 38, one case with N = 10
  case_<i>_args           [Ts, n_samples]
  case_<i>_dev            [lat_dev, vel_dev] as LonLatDeviations and the subtraction give them
  case_<i>_obs            ObservationGenerator(38, 10).get_observation(v, lat_dev, vel_dev, window, Ts)
Windows in front of every yaw seam of both race lines are among the cases (asserted here: |diff(ref_yaw)| > pi in at least four).
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))


class _Stub(types.ModuleType):
    """an absent third-party module: any name imported from it is a placeholder nothing here calls"""
    __path__ = []

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return type(item, (), {})


sys.path.insert(0, REF)
sys.path.insert(0, ROOT)


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


LonLatDeviations, = _import_with_stubs("Utils.MPC_sim_utils", ["LonLatDeviations"])
ObservationGenerator, = _import_with_stubs("Learning_To_Adapt.SafeRL_WMPC.RL_WMPC.observation", ["ObservationGenerator"])


def main():
    from tum_control_amd.planner import load_track, planner_emulator
    rng = np.random.RandomState(11)
    gen = ObservationGenerator(anticipation_horizon=38, n_anticipation_points=10)
    out, i, crossed = {}, 0, 0
    cases = []
    for name in ("monteblanco", "modena"):
        track = load_track(name)
        seams = np.nonzero(np.abs(np.diff(track[:, 2])) > np.pi)[0]
        assert len(seams), name
        starts = list(rng.randint(0, len(track), 12)) + [int(s) - d for s in seams for d in (1, 8)]
        cases += [(track, w, 38, 3.04) for w in starts]
    cases.append((load_track("monteblanco"), 300, 10, 0.8))          # the smallest horizon the ten-tap average takes
    for track, w, N, Tp in cases:
        p = track[w % len(track)]
        yaw = np.mod(p[2], 2 * np.pi)
        side = rng.uniform(-2.0, 2.0)
        x0 = np.zeros(8)
        x0[0], x0[1] = p[0] - side * np.sin(yaw), p[1] + side * np.cos(yaw)
        x0[2], x0[3] = yaw + rng.uniform(-0.05, 0.05), p[3] + rng.uniform(-3.0, 3.0)
        _, ref = planner_emulator(track, x0[:2], N + 1, Tp, True)
        ref = np.asarray(ref, float)[:N + 1]
        crossed += bool((np.abs(np.diff(ref[:, 2])) > np.pi).any())
        _, lat = LonLatDeviations(x0[2], x0[0], x0[1], ref[0, 0], ref[0, 1])
        vel = x0[3] - ref[0, 3]
        obs = gen.get_observation(x0[3], lat, vel, {"ref_yaw": ref[:, 2], "ref_v": ref[:, 3]}, 0.02)
        out[f"case_{i}_x0"], out[f"case_{i}_ref"] = x0, ref
        out[f"case_{i}_args"], out[f"case_{i}_dev"], out[f"case_{i}_obs"] = np.array([0.02, 10]), np.array([lat, vel], float), np.asarray(obs, float)
        i += 1
    assert crossed >= 4, crossed
    out["n"] = np.array(i)
    np.savez(os.path.join(OUT, "wmpc_schedule.npz"), **out)
    print(f"wmpc_schedule.npz: {i} cases, {crossed} windows across a yaw seam")


if __name__ == "__main__":
    main()
