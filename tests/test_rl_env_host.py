"""
Host statements of the RL environment (closed_loop.rl_observation, rl_reward, rl_env_steps_from_logs) against what the reference's
ObservationGenerator / RewardGenerator computed (tests/golden/rl_env.npz, written by tests/golden/make_rl_env_golden.py) and against
hand-stated outcomes of the episode rules (RL_WMPC/environment.py:112-189) on synthetic logs. No GPU.

Gate of the two formulas, 1e-12 absolute + relative: the same numpy operations as the reference on the same inputs; differences are a
few ulp of O(1) numbers.
"""
import os

import numpy as np
import pytest

from tum_control_amd import closed_loop as cl
from tum_control_amd.planner import closest_index, load_track, planner_emulator

TOL = 1e-12


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and bool((np.abs(a - b) <= TOL + TOL * np.abs(b)).all())


def test_action_table_is_the_26_weight_sets(gold, golden_dir):
    F = gold["F"]
    assert F.shape == (26, 7) and np.isfinite(F).all() and (F >= 0).all()
    # the same 26 weight sets the logged closed loops of the reference ran with
    assert np.array_equal(F, np.load(os.path.join(golden_dir, "closed_loop_monteblanco_150.npz"))["params"])


def test_observation_matches_reference(gold):
    n = int(gold["n_obs"])
    assert n >= 10
    lengths, seam, nonzero_states = set(), False, False
    for i in range(n):
        yaw, v, (Ts, ns, lat, vel) = gold[f"obs_{i}_ref_yaw"], gold[f"obs_{i}_ref_v"], gold[f"obs_{i}_args"]
        lengths.add(len(yaw))
        seam |= bool((np.abs(np.diff(yaw)) > np.pi).any())
        nonzero_states |= lat != 0.0
        obs = cl.rl_observation(yaw, v, Ts, int(ns), lat, vel)
        assert obs.shape == (2 + 2 * int(ns),)
        assert _close(obs, gold[f"obs_{i}_out"]), (i, np.abs(obs - gold[f"obs_{i}_out"]).max())
        if lat == 0.0 and vel == 0.0:          # the reference's quirk: the first two entries are always 0 -> 0.5
            assert obs[0] == 0.5 and obs[1] == 0.5
    assert lengths == {39, 13} and seam and nonzero_states
    # at N = 12 the yaw rate has 3 points: the 10 sample indices repeat
    assert len(np.unique(np.linspace(0, 12 - 10, 10, dtype=int))) == 3


def test_reward_matches_reference(gold):
    n = int(gold["n_rew"])
    lengths, below, above, inside, shapes = set(), False, False, False, set()
    for j in range(n):
        lat, vel, sig, lims = (gold[f"rew_{j}_{k}"] for k in ("lat", "vel", "sigmas", "lims"))
        lengths.add(len(lat)); shapes.add(lims.shape)
        r = cl.rl_reward(lat, vel, sig, lims)
        assert _close(r, gold[f"rew_{j}_out"]), (j, r, gold[f"rew_{j}_out"])
        m = np.array([np.sqrt(np.mean(lat ** 2)), np.sqrt(np.mean(vel ** 2))])
        u = (m - lims[0]) / (lims[1] - lims[0])
        below |= bool((u < 0).any()); above |= bool((u > 1).any()); inside |= bool(((u > 0) & (u < 1)).any())
    assert lengths == {1, 5, 20} and below and above and inside and shapes == {(2, 2), (4,)}
    # the flat lims of the shipped rl_config.yaml normalise BOTH metrics with the lateral limits 0 .. 0.4
    assert cl.rl_reward([0.0], [0.4], (0.1, 0.5), cl.RL_LIMS) == np.exp(-1.0 / (2 * 0.5))


# --------------------------------------------------------------------------------------------- the episode rules on synthetic logs
N_MPC = 4


def _synthetic(track, idx, lat, failed=None):
    """logs of one vehicle that sits on waypoint idx[s] at control step s with yaw 0, its first reference point `lat[s]` to the left
    (lat_dev = lat[s] exactly: sin(-0) = -0, cos(-0) = 1) and 0.5 m/s faster than it drives"""
    S = len(idx)
    CiLX = np.zeros((S + 1, 1, 7)); REF = np.zeros((S, 1, 4)); DBG = np.zeros((S, 1, 5))
    CiLX[:S, 0, :2] = track[idx, :2]; CiLX[:S, 0, 3] = 10.0
    REF[:, 0, 0] = track[idx, 0]; REF[:, 0, 1] = track[idx, 1] + np.asarray(lat, float); REF[:, 0, 3] = 10.5
    if failed is not None:
        DBG[:, 0, 4] = failed
    return dict(CiLX=CiLX, simREF=REF, simSolverDebug=DBG, MPC_SimX=np.zeros((S + 1, 1, 8)))


def _run(track, logs, E, **kw):
    kw = dict(dict(max_lat_dev=2.0, episode_length=3, sigmas=(0.1, 0.5), lims=((0.0, 0.0), (0.4, 1.0))), **kw)
    return cl.rl_env_steps_from_logs(logs, track, np.zeros((E, 1), dtype=int), N_MPC, **kw)


@pytest.fixture(scope="module")
def track():
    return load_track("monteblanco")


def test_rules_crash_first_last_and_never(track):
    E = 3
    idx = 100 + np.arange(E * N_MPC)
    lat = np.full(E * N_MPC, 0.1)
    lat[0] = 2.5                      # environment step 0: crash in its first control step
    lat[2 * N_MPC - 1] = 2.0001       # environment step 1: crash in its last
    lat[2 * N_MPC + 1] = -7.0         # environment step 2: far off to the RIGHT: the test is signed, no crash
    failed = np.zeros(E * N_MPC); failed[1] = 1; failed[N_MPC] = 1
    d = _run(track, _synthetic(track, idx, lat, failed), E, episode_length=100)
    assert d["truncated"][:, 0].tolist() == [True, True, False]
    assert d["terminated"][:, 0].tolist() == [False, False, False]
    assert d["step_length"][:, 0].tolist() == [1, N_MPC, N_MPC]
    assert d["qp_failures"][:, 0].tolist() == [0, 1, 0]          # the failed solve of control step 1 came after the crash: not counted
    # reward of the first environment step: one scored step, lat 2.5 -> clipped to 1, vel -0.5 -> 0.5
    assert _close(d["reward"][0, 0], np.exp(-(1.0 / (2 * 0.1) + 0.25 / (2 * 0.5))))
    lats = lat[N_MPC:2 * N_MPC]
    assert _close(d["reward"][1, 0], cl.rl_reward(lats, np.full(N_MPC, -0.5), (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))))
    # observation: from the planner's window at the LAST SCORED control step (step 0 of environment step 0)
    _, ref = planner_emulator(track, track[100, :2], 39, 3.04)
    assert np.array_equal(d["observation"][0, 0], cl.rl_observation(ref[:, 2], ref[:, 3], 0.02, 10, 0.0, 0.0))
    d2 = _run(track, _synthetic(track, idx, lat, failed), E, episode_length=100, obs_states="last_step")
    assert _close(d2["observation"][0, 0], cl.rl_observation(ref[:, 2], ref[:, 3], 0.02, 10, 2.5, -0.5))          # (lat_dev = (y + 2.5) - y: 2.5 to rounding)
    assert np.array_equal(d2["observation"][:, :, 2:], d["observation"][:, :, 2:])
    assert (d["observation"][:, :, :2] == 0.5).all()


def test_rules_last_episode_step_has_length_one(track):
    """episode_steps counts ENVIRONMENT steps and is compared after every control step: in environment step `episode_length` the
    flag is set after the first control step already; past it the equality never holds again"""
    E = 5
    idx = 200 + np.arange(E * N_MPC)
    d = _run(track, _synthetic(track, idx, np.zeros(E * N_MPC)), E, episode_length=3)
    assert d["terminated"][:, 0].tolist() == [False, False, True, False, False]
    assert d["step_length"][:, 0].tolist() == [N_MPC, N_MPC, 1, N_MPC, N_MPC]
    assert not d["truncated"].any()


def test_rules_full_lap_is_an_equality(track):
    n = len(track)
    E = 3
    idx = np.array([n - 6, n - 5, n - 4, n - 3,   n - 3, n - 2, 0, 1,   0, 1, 2, 3])          # (waypoint n - 1 repeats waypoint 0: the planner never returns it)
    assert (closest_index(track, track[idx, :2]) == idx).all()
    d = _run(track, _synthetic(track, idx, np.zeros(len(idx))), E, full_lap=True, episode_length=1)
    assert d["terminated"][:, 0].tolist() == [False, True, False]          # (episode_length plays no part with full_lap)
    assert d["step_length"][:, 0].tolist() == [N_MPC, 2, N_MPC]            # beyond n - 2 nothing terminates: passed, not reached
    # a vehicle that jumps over n - 2 never terminates
    idx2 = np.array([n - 5, n - 4, n - 3, 0, 1, 2, 3, 4])
    d = _run(track, _synthetic(track, idx2, np.zeros(len(idx2))), 2, full_lap=True)
    assert not d["terminated"].any() and d["step_length"][:, 0].tolist() == [N_MPC, N_MPC]


def test_rules_refuse_short_logs_and_unknown_mode(track):
    logs = _synthetic(track, 100 + np.arange(N_MPC), np.zeros(N_MPC))
    with pytest.raises(ValueError, match="shorter"):
        _run(track, logs, 2)
    with pytest.raises(ValueError, match="obs_states"):
        _run(track, logs, 1, obs_states="current")


def test_interface_is_documented():
    """the C interface, its refusals and the two quirks are written down where a user looks for them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tum_nmpc.h")).read()
    for word in ("tum_sim_env_attach", "tum_sim_env_reset", "tum_sim_env_step", '"env_episode_steps"', "environment.py:112-189"):
        assert word in hdr, word
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for word in ("WeightScheduleEnv", "obs_states", "step_length", "VecEnv", "reintialize_solver"):
        assert word in doc, word
    from tum_control_amd import solver
    for name in ("attach_env", "env_reset", "env_step"):
        assert callable(getattr(solver.DeviceClosedLoop, name))


def test_env_kernels_in_resource_table():
    """the three kernels are in the shipped library and the compiler reports no spills and no scratch for them"""
    import shutil
    import __graft_entry__ as g
    if not (os.path.exists(g.HIPCC) or shutil.which("hipcc")) and not os.path.exists(g.LIB + ".resources"):
        pytest.skip("no hipcc and no resource table of a previous build on this host")
    g.build()
    rows = [line.split() for line in open(g.LIB + ".resources")]
    for name in ("env_begin_kernel", "env_score_kernel", "env_finish_kernel"):
        hit = [r for r in rows if name in r[0]]
        assert len(hit) == 1, name
        vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ = (int(x) for x in hit[0][1:])
        assert (sgpr_spill, vgpr_spill, scratch) == (0, 0, 0) and vgpr <= 64 and lds <= 4096, (name, hit[0])
