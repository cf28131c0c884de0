"""
Closed loops, segment evaluations and RL environments on several tracks at once (tum_sim_create_tracks, tum_planner_emulate_tracks;
planner_kernel, env_begin_kernel and env_score_kernel select the instance's own table and length from the loop's track set).

A mixed loop is held against SINGLE-TRACK LOOPS OF THE SAME BATCH SIZE WITH THE SAME INSTANCE PLACEMENT: instance b of the mixed loop
against instance b of a loop that runs entirely on track_of[b] with the same start state at b (the other instances of that loop start
at their own index taken modulo the track's length: nothing they compute reaches instance b). Both run the same kernel chain and there
is no arithmetic across instances, so the gate is BIT EQUALITY throughout; the one exception, the group objectives, is stated where it
is used. Every test also asserts that the single-track runs themselves show the event it is about.
The shipped race lines have 1190 (monteblanco), 921 (lvms) and 1002 (modena) waypoints: an index taken against the wrong length shows.
Shipped tracks, N = 38, the 26-row table of tests/golden/rl_env.npz, the agent of wmpc_policy.npz + wmpc_value.npz.
"""
import os

import numpy as np
import pytest

import ppo_reference as ppo_ref
from test_gpu_collect import ALL_KEYS, GAMMA, LAM, _assert_same, _host_loop
from test_gpu_policy import FIELDS, _assert_same_steps, _decided
from test_multi_track_host import seam_pose

pytestmark = pytest.mark.gpu

N, TP = 38, 3.04
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))
ROWS = {"monteblanco": 1190, "lvms": 921, "modena": 1002}
TWO = ("monteblanco", "modena")
LOGS = ("CiLX", "MPC_SimX", "simU", "simREF", "simSolverDebug")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


@pytest.fixture(scope="module")
def agent(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"), os.path.join(golden_dir, "wmpc_value.npz"))


def _own(names, of, idx, t):
    """the indices a single-track loop on names[t] takes: the instance's own where it drives on that track, else modulo its length"""
    idx = np.asarray(idx, dtype=np.int64)
    return np.where(np.asarray(of) == t, idx, idx % ROWS[names[t]])


# ----------------------------------------------------------------------------------------------------------------------- 1. planner
def test_planner_on_a_track_set():
    from tum_control_amd.planner import TRACKS, load_track
    from tum_control_amd.solver import planner_emulate, planner_emulate_tracks
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner.npz"))
    names = list(TRACKS)
    tabs = [load_track(n) for n in names]
    poses, of = [], []
    for t, n in enumerate(names):
        for p in (tabs[t][-1, :2], tabs[t][-2, :2], tabs[t][-3, :2], seam_pose(g, n, tabs[t])):
            poses.append(p); of.append(t)
    poses.append(tabs[0][1100, :2] + 0.2); of.append(0)
    order = np.random.RandomState(0).permutation(len(of))          # interleaved over the three tracks
    poses, of = np.array(poses)[order], np.array(of)[order]
    assert len(of) == 13 and (np.diff(of) < 0).any()
    for npts, tp in ((39, 3.04), (41, 3.2)):
        idx, ref = planner_emulate_tracks(tabs, of, poses, npts, tp)
        wraps = seams = 0
        for t in range(3):
            m = of == t
            i1, r1 = planner_emulate(tabs[t], poses[m], npts, tp)
            assert np.array_equal(idx[m], i1), (names[t], idx[m], i1)
            assert r1.shape == ref[m].shape and r1.tobytes() == ref[m].tobytes(), names[t]
            # what the single-track calls show: walks that pass the last waypoint of the pose's own track, windows across the yaw seam
            wraps += int((i1 >= len(tabs[t]) - 3).sum())
            seams += int((np.abs(np.diff(r1[:, :, 2], axis=1)) > 3.0).any(axis=1).sum())
            assert (i1 < len(tabs[t])).all()
        assert wraps == 6 and seams >= 3 and (idx[of == 0] >= 1002).any()
    # the concatenated form of the set, and the refusals of the C entry point itself
    from tum_control_amd.solver import track_set
    table, rows, _ = track_set(tabs, of, len(of))
    idx2, ref2 = planner_emulate_tracks(table, of, poses, 41, 3.2, track_rows=rows)
    assert np.array_equal(idx2, idx) and ref2.tobytes() == ref.tobytes()
    import ctypes
    from tum_control_amd.solver import load_library
    L = load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out, cl = np.empty((13, 39, 4)), np.empty(13, dtype=np.int32)
    call = lambda r, o: L.tum_planner_emulate_tracks(table.ctypes.data_as(dp), r.ctypes.data_as(ip), 3, o.ctypes.data_as(ip), poses.ctypes.data_as(dp),
                                                     13, 39, 3.04, 1, out.ctypes.data_as(dp), cl.ctypes.data_as(ip), 0)
    of32 = of.astype(np.int32)
    assert call(rows, of32) == 0
    bad_of = of32.copy(); bad_of[4] = 3
    assert call(rows, bad_of) != 0 and b"track_of[4]" in L.tum_ocp_last_error()
    bad_rows = rows.copy(); bad_rows[1] = bad_rows[2]
    assert call(bad_rows, of32) != 0 and b"ascend" in L.tum_ocp_last_error()


# -------------------------------------------------------------------------------------------------------------------------- 2. loop
def _loop(names, B, starts, cap, controller="nominal", track_of=None):
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(names, batch=B, N=N, Tp=TP, idx_start=starts, on_device=True, log_capacity=cap, controller=controller, track_of=track_of)


def _run_mixed_and_single(names, of, starts, runs, controller="nominal"):
    """(mixed, [single per track]) after run(k) for k in runs: each a dict logs / closest / graph_steps / loop"""
    B, cap = len(of), sum(runs)
    out = []
    for t in [None] + list(range(len(names))):
        cl = _loop(list(names), B, starts, cap, controller, of) if t is None else _loop(names[t], B, _own(names, of, starts, t), cap, controller)
        for k in runs:
            cl.dev.run(k)
        out.append(dict(logs=cl.dev.logs(), closest=cl.dev.get("closest"), graph_steps=cl.dev.graph_steps, loop=cl))
    return out[0], out[1:]


def _assert_instances_equal(names, of, mixed, single, steps):
    for t in range(len(names)):
        m = np.asarray(of) == t
        assert m.any()
        for k in LOGS:
            a, b = mixed["logs"][k], single[t]["logs"][k]
            assert a.shape == b.shape and a.shape[0] in (steps, steps + 1) and np.array_equal(a[:, m], b[:, m]), (names[t], k)
        assert np.array_equal(mixed["closest"][m], single[t]["closest"][m]), names[t]
        assert (mixed["closest"][m] < ROWS[names[t]]).all()
    assert np.isfinite(mixed["logs"]["simU"]).all()


def test_loop_batch_4_plain_launches_and_captured_chunk():
    of, starts = np.array([0, 1, 1, 0]), np.array([1100, 990, 400, 1180])
    mixed, single = _run_mixed_and_single(TWO, of, starts, (30, 50))          # 30 steps by plain launches, then 50 through the chunk
    _assert_instances_equal(TWO, of, mixed, single, 80)
    dev = mixed["loop"].dev
    assert dev.steps == 80 and mixed["graph_steps"] == 25 and all(s["graph_steps"] == 25 for s in single)
    assert dev.get("track_of").tolist() == of.tolist() and dev.get("track_rows").tolist() == [0, 1190, 2192]
    assert single[0]["loop"].dev.get("track_of").tolist() == [0] * 4 and single[0]["loop"].dev.get("track_rows").tolist() == [0, 1190]
    # the single-track runs show what the set is for: a Monteblanco index no Modena table has, and two laps that close -- the planner
    # walked past the last waypoint of the instance's OWN track (990 + and 1180 + 80 steps end behind waypoint 0)
    assert single[0]["closest"][0] >= 1002 and single[1]["closest"][1] < 100 and single[0]["closest"][3] < 100
    # the same instance on the two tracks does differ
    assert not np.array_equal(single[0]["logs"]["simU"][:, 2], single[1]["logs"]["simU"][:, 2])


def test_loop_batch_17_three_tracks():
    from tum_control_amd.planner import TRACKS
    B = 17
    of = np.arange(B) % 3
    starts = np.array([[1180, 912, 992][t] if b < 3 else (61 * b) % ROWS[TRACKS[t]] for b, t in enumerate(of)])
    mixed, single = _run_mixed_and_single(TRACKS, of, starts, (10,))
    _assert_instances_equal(TRACKS, of, mixed, single, 10)
    # each of the first three starts a few waypoints before the end of its own line: the window the planner extracts at the pose of the
    # last control step starts there and ends behind waypoint 0 of the same line
    from tum_control_amd.planner import closest_index, planner_emulator
    for t in range(3):
        track = single[t]["loop"].track
        i0, ref = planner_emulator(track, single[t]["logs"]["CiLX"][9, t, :2], N + 1, TP)
        assert i0 == single[t]["closest"][t] >= len(track) - 12 and closest_index(track, ref[-1, :2]) < 100


def test_loop_snmpc_one_track_each():
    of, starts = np.array([0, 1]), np.array([1100, 995])
    mixed, single = _run_mixed_and_single(TWO, of, starts, (10,), controller="snmpc")
    _assert_instances_equal(TWO, of, mixed, single, 10)
    assert single[0]["closest"][0] >= 1002


def test_create_tracks_refusals():
    from tum_control_amd.closed_loop import ClosedLoopBatch
    from tum_control_amd.solver import DeviceClosedLoop
    cl = ClosedLoopBatch("monteblanco", batch=3, N=N, Tp=TP, on_device=False)
    tabs = [cl.track, cl.track[:500]]
    with pytest.raises(ValueError, match="outside 0..1"):
        DeviceClosedLoop(cl.solver, None, TP, tracks=tabs, track_of=[0, 2, 1])
    with pytest.raises(ValueError, match="not both"):
        DeviceClosedLoop(cl.solver, cl.track, TP, tracks=tabs)
    with pytest.raises(ValueError, match="goes with tracks"):
        DeviceClosedLoop(cl.solver, cl.track, TP, track_of=[0, 0, 0])
    with pytest.raises(KeyError, match="unknown track"):
        ClosedLoopBatch(("monteblanco", "monza"), batch=2, N=N, Tp=TP, on_device=True)
    dev = DeviceClosedLoop(cl.solver, None, TP, tracks=tabs, track_of=[1, 0, 1])
    assert dev.get("track_of").tolist() == [1, 0, 1] and dev.get("track_rows").tolist() == [0, 1190, 1690]
    # an end index is a waypoint of the instance's own track
    with pytest.raises(Exception, match="outside its own track"):
        dev.attach_segments(np.array([400, 600, 600]), np.inf, np.inf)
    dev.attach_segments(np.array([400, 600, 499]), np.inf, np.inf)


# ---------------------------------------------------------------------------------------------------------------------- 3. segments
SEG_CAP, SEG_CHECK = 4000, 100
MAX_LAT = 2.0          # the lateral crash threshold of the reference's bo_config.yaml
SEG_KEYS = ("max_lat_dev", "rms_vel_dev", "steps", "state")


@pytest.fixture(scope="module")
def segment_runs(golden_dir, table):
    """the fixture's 20 training segments x 2 weight sets, single-track evaluations first (they set max_steps), then ONE mixed loop"""
    from tum_control_amd import closed_loop as clm
    g = np.load(os.path.join(golden_dir, "train_segments.npz"))
    groups = [[dict(start=int(s), end=int(e), type=int(k), trajectory=str(n)) for s, e, k, n, gg in
               zip(g["start"], g["end"], g["type"], g["trajectory"], g["group"]) if gg == grp] for grp in (0, 1)]
    assert groups == clm.train_segments()
    # the default weight set as a row of update_cost_function_weights: what install_reference_ocp installs (0.01 q / s^2; L1, L2 as they are)
    mpc = clm._config.default_config()["mpc"]
    default = np.array([0.01 * mpc[q] / mpc[s_] ** 2 for q, s_ in (("q_lon", "s_lon"), ("q_yaw", "s_yaw"), ("q_vel", "s_vel"), ("r_jerk", "s_jerk"),
                                                                   ("r_steering_rate", "s_steering_rate"))] + [mpc["L1_pen"], mpc["L2_pen"]])
    params = np.stack([default, table[7]])
    flat = [s for grp in groups for s in grp]
    names = ["modena", "monteblanco"]
    of = np.array([names.index(s["trajectory"]) for s in flat])
    start, end = np.array([s["start"] for s in flat]), np.array([s["end"] for s in flat])

    def single_track(max_a_comb):
        """two single-track evaluations of the same 40 instances; of each instance what the evaluation on its own track gave"""
        single = []
        for t, n in enumerate(names):
            pairs = np.stack([_own(names, of, start, t), _own(names, of, end, t)], axis=1)
            single.append(clm.evaluate_segments(n, params, [pairs[:10], pairs[10:]], MAX_LAT, max_a_comb, SEG_CAP, N=N, Tp=TP, check_every=SEG_CHECK)[2])
        return {k: np.where(np.tile(of, 2) == 0, single[0][k], single[1][k]) for k in single[0]}

    # The threshold of the combined acceleration: the reference's 1.02 stops the DEFAULT weights on both wrapped segments (they start on
    # the straights at full speed; states 4 after 45 and 238 steps), and a finished wrapped segment is what this test is about. So it is
    # taken from the single-track runs themselves, as tests/test_gpu_rl_env.py takes its crash threshold: above everything the default
    # weights reach and -- where the other weight set reaches further -- below that, which makes the other candidate infeasible.
    own = single_track(np.inf)
    top_default, top_other = own["max_a_comb"][:20].max(), own["max_a_comb"][20:].max()
    max_a_comb = 0.5 * (top_default + top_other) if top_other > top_default * (1.0 + 1e-9) else np.inf
    if np.isfinite(max_a_comb):
        own = single_track(max_a_comb)
    # max_steps from the single-track runs: every segment that ended there ends below it (where one did not, the cap they ran with)
    ended = own["state"] != 0
    max_steps = SEG_CAP if not ended.all() else int(-(-own["steps"].max() // SEG_CHECK) * SEG_CHECK)
    mixed = clm.evaluate_segments(None, params, groups, MAX_LAT, max_a_comb, max_steps, N=N, Tp=TP, check_every=SEG_CHECK)
    return dict(own=own, mixed=mixed, of=of, flat=flat, max_steps=max_steps, default=default, max_a_comb=max_a_comb)


def test_segments_one_loop_over_both_tracks(segment_runs):
    from tum_control_amd import closed_loop as clm
    own, (objectives, feasible, seg), of, flat = (segment_runs[k] for k in ("own", "mixed", "of", "flat"))
    print("max_a_comb", segment_runs["max_a_comb"], "max_steps", segment_runs["max_steps"], "steps (default weights)", own["steps"][:20].tolist(), "state", own["state"].tolist())
    assert len(seg["steps"]) == 40 and objectives.shape == (2, 2, 2) and feasible.shape == (2,)
    # the single-track runs: with the default weights every segment is driven to its end -- no time-out, no crash -- the two that wrap
    # past the end of their track among them
    assert not own["timed_out"][:20].any() and (own["state"][:20] == 1).all() and (own["steps"][:20] <= segment_runs["max_steps"]).all()
    wrapped = [i for i, s in enumerate(flat) if s["end"] < s["start"]]
    assert [(flat[i]["trajectory"], flat[i]["start"], flat[i]["end"]) for i in wrapped] == [("modena", 876, 65), ("monteblanco", 931, 209)]
    assert all(own["done"][i] and own["steps"][i] > 200 for i in wrapped)
    for k in SEG_KEYS:
        assert seg[k].dtype == own[k].dtype and np.array_equal(seg[k], own[k]), k
    # group objectives: the device's sum of ten non-negative terms in its own order and one division, against numpy's: 16 u relative
    want_obj, want_feas = clm.segment_objectives(own, 2, [10, 10])
    assert np.array_equal(feasible, want_feas) and feasible[0]
    assert np.array_equal(np.isnan(objectives), np.isnan(want_obj))
    ok = ~np.isnan(want_obj)
    err = np.abs(objectives[ok] - want_obj[ok]) / np.abs(want_obj[ok])
    print("objectives", objectives.tolist(), "relative error / u", (err / U).tolist())
    assert (err <= 16 * U).all()


# ------------------------------------------------------------------------------------------------------------------- 4. environment
M = 5


def _env(names, B, table, starts, track_of=None, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    kw = dict(dict(rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=starts, n_mpc_steps=M, auto_reset=False), **kw)
    return WeightScheduleEnv(names, B, table, track_of=track_of, **kw)


def _records(env, actions):
    out = []
    for a in actions:
        obs, rew, te, tr, info = env.step(a)
        out.append(dict(reward=rew, terminated=te, truncated=tr, observation=info["terminal_observation"], step_length=info["step_length"],
                        qp_failures=info["qp_failures"], x_sim=env.dev.get("x_sim"), x_mpc=env.dev.get("x_mpc")))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def _mixed_and_single_envs(table, starts, actions, **kw):
    of = np.arange(4) % 2
    mixed = _env(list(TWO), 4, table, starts, **kw)
    assert mixed.track_of.tolist() == of.tolist() and mixed.dev.get("track_of").tolist() == of.tolist()
    rm = _records(mixed, actions)
    rs = [_records(_env(TWO[t], 4, table, _own(TWO, of, starts, t), **kw), actions) for t in range(2)]
    for t in range(2):
        for k in rm:
            assert rm[k].shape == rs[t][k].shape and np.array_equal(rm[k][:, of == t], rs[t][k][:, of == t]), (TWO[t], k)
    return rm, rs, of


def test_env_steps_on_two_tracks(table):
    actions = np.random.RandomState(1).randint(0, len(table), size=(3, 4))
    starts = np.array([1100, 995, 300, 40])
    rm, rs, of = _mixed_and_single_envs(table, starts, actions, episode_length=2, max_lat_dev=np.inf)
    # what the single-track environments show: scored steps, an episode that ends by its length, and instances that differ by track
    assert (rs[0]["step_length"][0] == M).all() and rs[0]["terminated"][1].all() and not rs[0]["terminated"][0].any()
    assert (rm["reward"] > 0).all() and not np.array_equal(rs[0]["observation"][:, 2], rs[1]["observation"][:, 2])


def test_full_lap_ends_at_the_last_but_one_waypoint_of_the_own_track(table):
    actions = np.zeros((1, 4), dtype=np.int64)
    starts = np.array([998, 998, 300, 300])
    rm, rs, of = _mixed_and_single_envs(table, starts, actions, n_mpc_steps=20, full_lap=True, episode_length=1, max_lat_dev=np.inf)
    # Modena ends at waypoint 1000 of its 1002: the instance started two waypoints before it terminates within the first environment
    # step, in the single-track environment and in the mixed one; the Monteblanco instance started at the same index has 190 to go
    assert rs[1]["terminated"][0, 1] and 1 <= rs[1]["step_length"][0, 1] < 20
    assert not rs[0]["terminated"][0, 0] and rs[0]["step_length"][0, 0] == 20
    assert rm["terminated"][0].tolist() == [False, True, False, False] and rm["step_length"][0, 1] == rs[1]["step_length"][0, 1]


def test_start_index_is_held_against_the_own_track(table, agent):
    """1100 is a waypoint of Monteblanco (instances 0, 2) and of no Modena table (instances 1, 3): accepted there, refused here, by
    reset, by step and by the start tables of rollout and collect, before anything is launched"""
    env = _env(list(TWO), 4, table, 0, auto_reset=True, episode_length=2, max_lat_dev=np.inf)
    dev = env.dev
    dev.attach_policy(agent)

    def state():
        return [dev.steps] + [dev.get(f) for f in ("x_sim", "x_mpc", "pose")] + [dev.env_get(f) for f in ("episode_steps", "samples", "ended")]

    def unchanged(s0):
        return all(np.array_equal(a, b) for a, b in zip(s0, state()))

    dev.env_reset(np.array([1100, 1001, 1189, 0]))
    assert dev.get("x_mpc")[0, 0] == env.loop.tracks[0][1100, 0] and dev.get("x_mpc")[1, 0] == env.loop.tracks[1][1001, 0]
    s0 = state()
    act = np.zeros(4, dtype=np.int64)
    for bad, who in ((np.array([1100, 1100, 0, 0]), 1), (np.array([0, 0, 0, 1002]), 3)):
        msg = f"start index of instance {who} is outside the track it drives on \\(track 1 of the set, 1002 rows\\)"
        with pytest.raises(Exception, match="env_reset: " + msg):
            dev.env_reset(bad)
        with pytest.raises(Exception, match="env_step: " + msg):
            dev.env_step(act, np.ones(4, dtype=np.int64), bad)
        tab = np.zeros((3, 4), dtype=np.int64); tab[2] = bad
        with pytest.raises(Exception, match=f"env_rollout: start index of instance {who} at step 2 is outside the track it drives on"):
            dev.env_rollout(3, first_obs=None, on_end=1, start_table=tab)
        with pytest.raises(Exception, match=f"env_collect: start index of instance {who} at step 2 is outside the track it drives on"):
            dev.env_collect(3, tab, 1, 0, GAMMA, LAM)
        assert unchanged(s0)
    with pytest.raises(Exception, match="instance 0 is outside the track it drives on \\(track 0 of the set, 1190 rows\\)"):
        dev.env_reset(np.array([1190, 0, 0, 0]))
    assert unchanged(s0)
    # accepted where the instance's own track has the waypoint: a step that resets instances 0 and 2 to 1100 runs
    r = dev.env_step(act, np.array([1, 0, 1, 0]), np.array([1100, 1100, 1100, 1100]))
    assert dev.steps == M and (r["step_length"] == M).all()
    # a single-track environment says what it always said
    one = _env("modena", 2, table, 0)
    with pytest.raises(Exception, match="is outside the track$"):
        one.dev.env_reset(np.array([0, 1002]))


# -------------------------------------------------------------------------------------------------------- 5. rollout, collect, update
RESTARTS = ((0, 200, 640, 1100), (7, 350, 950))          # Monteblanco's list holds a waypoint Modena does not have
SEED = 0x1234567890abcdef


def _agent_env(table, **kw):
    kw = dict(dict(n_mpc_steps=3, auto_reset=True, episode_length=2, max_lat_dev=np.inf, restart_indices=RESTARTS, seed=9), **kw)
    return _env(list(TWO), 4, table, np.array([1100, 995, 300, 40]), **kw)


def _drawn_table(E, B):
    """what a fresh _agent_env draws for the E steps of a rollout or a collection: every instance from the list of its own track"""
    from tum_control_amd import closed_loop as clm
    tab = clm.draw_restarts(np.random.RandomState(9), clm.restart_lists(RESTARTS, 2), np.tile(np.arange(B) % 2, E)).reshape(E, B)
    assert set(tab[:, 0::2].ravel()) <= set(RESTARTS[0]) and set(tab[:, 1::2].ravel()) <= set(RESTARTS[1])
    return tab


def _host_rollout(env, policy, start_table, E):
    """the step of step(), driven by policy.predict on the observation just returned, with the rollout's start table (step() itself
    draws one number per reset that happens, rollout() one per step and instance before it starts); dict of (E, B, ...) arrays"""
    dev, B = env.dev, env.n_envs
    obs, ended = np.zeros((B, env.n_observations)), np.zeros(B, dtype=bool)
    out = {k: [] for k in FIELDS + ("action",)}
    for e in range(E):
        _decided(policy, obs)
        a = policy.predict(obs)
        h = dev.env_step(a, ended.astype(np.int32), np.where(ended, start_table[e], 0))
        for k in FIELDS:
            out[k].append(h[k])
        out["action"].append(a)
        ended = h["terminated"] | h["truncated"]
        obs = np.where(ended[:, None], 0.0, h["observation"])
    return {k: np.stack(v) for k, v in out.items()}


def test_rollout_is_step_driven_by_predict(table, agent):
    from tum_control_amd.closed_loop import WeightPolicy
    policy = WeightPolicy(agent.weights, agent.biases)
    a, b = _agent_env(table, log_capacity=9), _agent_env(table, log_capacity=9)
    r = a.rollout(policy, 3)
    drawn = _drawn_table(3, 4)
    b.dev.attach_policy(policy)
    h = _host_rollout(b, policy, drawn, 3)
    assert r["live"].shape == (3, 4) and r["live"].all()
    _assert_same_steps(r, h)
    la, lb = a.dev.logs(), b.dev.logs()
    assert all(np.array_equal(la[k], lb[k]) for k in la)
    for f in ("episode_steps", "samples", "ended"):
        assert np.array_equal(a.dev.env_get(f), b.dev.env_get(f)), f
    # the episodes of two steps ended and the third step began with a reset of every instance, each to a waypoint of its own list
    assert h["terminated"][1].all() and (h["step_length"][2] == 3).all() and np.array_equal(a.last_start, drawn[2])


def test_collect_is_the_host_driven_loop_and_update_repeats(table, agent):
    from tum_control_amd import closed_loop as clm
    E, B = 3, 4
    a, b = _agent_env(table, log_capacity=9), _agent_env(table, log_capacity=9)
    r = a.collect(agent, E, GAMMA, LAM, seed=SEED)
    drawn = _drawn_table(E, B)
    h, _ = _host_loop(b, agent, drawn, E, SEED)
    assert set(r) == set(ALL_KEYS) and r["observations"].shape == (E, B, 22)
    _assert_same(r, h)
    la, lb = a.dev.logs(), b.dev.logs()
    assert all(np.array_equal(la[k], lb[k]) for k in la)
    assert r["terminated"][1].all() and (r["episode_starts"][2] == 1).all() and np.array_equal(a.last_start, drawn[-1])
    # one update on the buffer each collection left on its device: it runs, and the same call from the same state gives the same bits
    c, d = _agent_env(table), _agent_env(table)
    outs = []
    for env in (c, d):
        tr = clm.PPOTrainer(env, agent, **ppo_ref.SETTINGS)
        buf = env.collect(tr, E, GAMMA, LAM, seed=SEED)
        assert all(np.array_equal(buf[k], r[k]) for k in ALL_KEYS)
        outs.append((tr.update(None, None, n_epochs=2, batch_size=6, lr=1e-3, seed=3), tr.policy(), tr.state()))
    (sa, pa, ta), (sb, pb, tb) = outs
    assert set(sa) == set(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert np.isfinite(sa["loss"]).all() and sa["n"].sum() == 2 * E * B
    for x, y in zip(pa.weights + pa.biases + pa.value_weights + pa.value_biases, pb.weights + pb.biases + pb.value_weights + pb.value_biases):
        assert np.array_equal(x, y)
    assert np.abs(pa.weights[0] - agent.weights[0]).max() > 0 and ta["t"] == tb["t"] == 4
