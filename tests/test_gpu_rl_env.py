"""
The weight-scheduling RL environment on the device (env_begin_kernel / env_score_kernel / env_finish_kernel, tum_sim_env_attach /
_reset / _step, closed_loop.WeightScheduleEnv) against loops that never had an environment and against the host statement of the
episode rules on their logs (closed_loop.rl_env_steps_from_logs, held to the reference's ObservationGenerator / RewardGenerator by
tests/test_rl_env_host.py). Shipped track, N = 38, the 26 rows of the reference's action table (tests/golden/rl_env.npz).

The floating-point gate of reward and observation, 1e-12 absolute + relative, is that of tests/test_gpu_segments.py: kernel and host
read bit-identical inputs (the logs store exactly the words the kernel reads; the planner's window is recomputed on the host, which the
planner tests hold to the kernel), so what differs is the device's sin / cos / sqrt / exp, a few ulp, and the order of roundings in sums
of at most 20 terms of size O(1): of the order 1e-15. Everything else -- logs, plant and controller states, flags, step lengths -- is
compared bit for bit.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12
TRACK, N, TP = "monteblanco", 38, 3.04
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


def _loop(B, starts, log_capacity=0, controller="nominal"):
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(TRACK, batch=B, N=N, Tp=TP, idx_start=starts, on_device=True, log_capacity=log_capacity, controller=controller)


def _env(B, table, starts=0, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    kw = dict(dict(rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=starts), **kw)
    return WeightScheduleEnv(TRACK, B, table, **kw)


def _host_driven(loop, table, actions, n_mpc_steps, states=None):
    """the path a caller had before: per environment step the weights through the setters, then run(); optionally the plant and
    controller states after every environment step"""
    for a in actions:
        loop.set_weights(table[a])
        loop.dev.run(n_mpc_steps)
        if states is not None:
            states.append((loop.dev.get("x_sim"), loop.dev.get("x_mpc")))
    return loop


def _between(values, lo, hi):
    """a threshold in (lo, hi): the middle of the widest gap between neighbouring values of the series in [lo, hi]"""
    v = np.unique(values[(values >= lo) & (values <= hi)])
    assert len(v) >= 2 and v[0] == lo and v[-1] == hi
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1])


def _assert_same_logs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _assert_close(name, dev, host):
    err = np.abs(dev - host) / (1.0 + np.abs(host))
    print(name, "max err", err.max())
    assert dev.shape == host.shape and (np.abs(dev - host) <= TOL + TOL * np.abs(host)).all(), (name, err.max())


def _host_rules(loop, logs, E, n_mpc_steps, **kw):
    from tum_control_amd.closed_loop import rl_env_steps_from_logs
    return rl_env_steps_from_logs(logs, loop.track, np.zeros((E, loop.B), dtype=int), n_mpc_steps, sigmas=SIGMAS, lims=LIMS, N=N, Tp=TP, **kw)


def _stack(steps):
    """[(obs, reward, terminated, truncated, info)] of E steps -> dict of (E, B, ...) arrays"""
    return dict(observation=np.stack([s[4]["terminal_observation"] for s in steps]), returned=np.stack([s[0] for s in steps]),
                reward=np.stack([s[1] for s in steps]), terminated=np.stack([s[2] for s in steps]), truncated=np.stack([s[3] for s in steps]),
                step_length=np.stack([s[4]["step_length"] for s in steps]), qp_failures=np.stack([s[4]["qp_failures"] for s in steps]))


def _assert_env_steps(dev, host):
    for k in ("terminated", "truncated", "step_length", "qp_failures"):
        assert np.array_equal(dev[k], host[k]), (k, dev[k], host[k])
    _assert_close("reward", dev["reward"], host["reward"])
    _assert_close("observation", dev["observation"], host["observation"])


# --------------------------------------------------------------------------------------------------------- 1: no resets, B = 70
B1, M1, L1, E1 = 70, 5, 4, 6


@pytest.fixture(scope="module")
def scored(table):
    """the host-driven loop with logs; a crash threshold chosen from its series; an identical loop as an environment"""
    from tum_control_amd import closed_loop as clm
    rng = np.random.RandomState(1)
    actions = rng.randint(0, len(table), size=(E1, B1))
    starts = np.array([0, 350, 800])[np.arange(B1) % 3]
    ref = _host_driven(_loop(B1, starts, log_capacity=E1 * M1), table, actions, M1)
    logs0 = ref.dev.logs()
    S = E1 * M1
    lat, _, _ = clm.segment_step_channels(logs0["CiLX"][:S], logs0["simREF"], logs0["MPC_SimX"][1:S + 1, :, 7], ref.cfg)
    v = np.sort(lat.reshape(-1))
    thr = _between(lat, v[int(0.75 * len(v))], v[int(0.9 * len(v))])
    assert np.abs(lat - thr).min() > 1e-9
    env = _env(B1, table, starts, n_mpc_steps=M1, episode_length=L1, max_lat_dev=thr, auto_reset=False, log_capacity=S)
    steps = [env.step(a) for a in actions]
    return dict(ref=ref, logs0=logs0, env=env, dev=_stack(steps), thr=thr, lat=lat)


def test_attaching_changes_nothing_the_loop_computes(scored):
    """the begin kernel leaves exactly the words set_weights leaves, the score kernel only reads, and the estimator's per-instance
    sample counter is the global step counter while nothing is reset: the five logs are bit-identical"""
    _assert_same_logs(scored["env"].dev.logs(), scored["logs0"])
    assert scored["env"].dev.steps == E1 * M1
    assert np.array_equal(scored["env"].dev.env_get("samples"), np.full(B1, E1 * M1))
    assert np.array_equal(scored["env"].dev.env_get("episode_steps"), np.full(B1, E1))


def test_env_steps_match_the_rules_on_the_logs(scored):
    host = _host_rules(scored["ref"], scored["logs0"], E1, M1, max_lat_dev=scored["thr"], episode_length=L1)
    dev = scored["dev"]
    _assert_env_steps(dev, host)
    assert np.array_equal(dev["returned"], dev["observation"])          # auto_reset=False: nothing is replaced by a reset's zeros
    assert (dev["observation"][:, :, :2] == 0.5).all()                  # obs_states "reference"
    # what the run shows
    tr, te, n = dev["truncated"], dev["terminated"], dev["step_length"]
    assert tr.any() and te.any() and (~tr & ~te).any()
    assert (~tr & ~te)[:L1 - 1].any() and (n[~tr & ~te] == M1).all()
    assert ((tr | te) & (n == 1)).any()                                  # a flag set in the first control step
    # the last environment step of an episode has step_length 1; the equality never holds again without a reset
    assert te[L1 - 1].all() and (n[L1 - 1] == 1).all() and not te[:L1 - 1].any() and not te[L1:].any()
    assert (dev["reward"] > 0).all() and (dev["reward"] <= 1).all()


# ------------------------------------------------------------------------------------------------- 2: per-instance reset, B = 6
B2, M2 = 6, 4


def _states(dev):
    return dev.get("x_sim"), dev.get("x_mpc")


def test_reset_of_single_instances(table):
    rng = np.random.RandomState(2)
    actions = rng.randint(0, len(table), size=(5, B2))
    who = np.array([0, 1, 0, 0, 1, 0])
    env = _env(B2, table, 0, n_mpc_steps=M2, episode_length=100, max_lat_dev=np.inf, auto_reset=False)
    got = []
    for e, a in enumerate(actions):
        r = env.dev.env_step(a, who if e == 2 else None, np.full(B2, 350) if e == 2 else None)
        assert not r["terminated"].any() and not r["truncated"].any() and (r["step_length"] == M2).all()
        got.append(_states(env.dev))
    never, fresh = [], []
    _host_driven(_loop(B2, 0), table, actions, M2, never)
    _host_driven(_loop(B2, 350), table, actions[2:], M2, fresh)
    keep = who == 0
    for e in range(5):
        for k in range(2):
            assert np.array_equal(got[e][k][keep], never[e][k][keep]), (e, k)
    for e in range(2, 5):
        for k in range(2):
            assert np.array_equal(got[e][k][~keep], fresh[e - 2][k][~keep]), (e, k)
            assert not np.array_equal(got[e][k][~keep], never[e][k][~keep])
    assert np.array_equal(env.dev.env_get("samples"), np.where(keep, 5 * M2, 3 * M2))
    assert np.array_equal(env.dev.env_get("episode_steps"), np.where(keep, 5, 3))
    assert env.dev.steps == 5 * M2


def test_auto_reset_draws_and_restarts(table):
    seed, restart = 5, (0, 350)
    rng = np.random.RandomState(3)
    actions = rng.randint(0, len(table), size=(4, B2))
    env = _env(B2, table, n_mpc_steps=M2, episode_length=2, max_lat_dev=np.inf, auto_reset=True, restart_indices=restart, seed=seed)
    draws = np.random.RandomState(seed)
    obs0, info0 = env.reset()
    start0 = np.asarray(restart)[draws.randint(0, 2, size=B2)]
    assert np.array_equal(env.last_start, start0) and obs0.shape == (B2, 22) and not obs0.any() and info0 == {}
    got, steps = [], []
    for a in actions:
        steps.append(env.step(a))
        got.append(_states(env.dev) + (env.last_start.copy(),))
    d = _stack(steps)
    # episodes of two environment steps: the second ends after its first control step, the observation returned is a reset's zeros,
    # the step's own observation is in info; the third step starts with the reset of every instance
    assert d["terminated"][:, 0].tolist() == [False, True, False, True] and (d["terminated"] == d["terminated"][:, :1]).all()
    assert d["step_length"][:, 0].tolist() == [M2, 1, M2, 1] and not d["truncated"].any()
    assert not d["returned"][1].any() and not d["returned"][3].any() and d["observation"][1].all() and d["observation"][3].all()
    assert np.array_equal(d["returned"][0], d["observation"][0])
    start2 = np.asarray(restart)[draws.randint(0, 2, size=B2)]
    assert np.array_equal(got[2][2], start2) and len(np.unique(np.concatenate([start0, start2]))) == 2
    first, second = [], []
    _host_driven(_loop(B2, start0), table, actions[:2], M2, first)
    _host_driven(_loop(B2, start2), table, actions[2:], M2, second)
    for e in range(4):
        want = first[e] if e < 2 else second[e - 2]
        for k in range(2):
            assert np.array_equal(got[e][k], want[k]), (e, k)


# --------------------------------------------------------------------------------------------- 3: obs_states modes and full_lap
def test_obs_states_modes(table):
    B, M, E = 4, 5, 2
    actions = np.random.RandomState(4).randint(0, len(table), size=(E, B))
    starts = np.array([0, 350, 800, 1000])
    out = {}
    for mode in ("reference", "last_step"):
        env = _env(B, table, starts, n_mpc_steps=M, episode_length=100, max_lat_dev=np.inf, auto_reset=False, obs_states=mode, log_capacity=E * M)
        out[mode] = _stack([env.step(a) for a in actions])
        host = _host_rules(env.loop, env.dev.logs(), E, M, max_lat_dev=np.inf, episode_length=100, obs_states=mode)
        _assert_env_steps(out[mode], host)
    ref, last = out["reference"]["observation"], out["last_step"]["observation"]
    assert (ref[:, :, :2] == 0.5).all() and (last[:, :, :2] != 0.5).all()
    assert np.array_equal(ref[:, :, 2:], last[:, :, 2:]) and np.array_equal(out["reference"]["reward"], out["last_step"]["reward"])


def test_full_lap_terminates_at_the_last_but_one_waypoint(table):
    from tum_control_amd.planner import closest_index
    B, M, E = 3, 5, 4
    actions = np.random.RandomState(6).randint(0, len(table), size=(E, B))
    env = _env(B, table, 0, n_mpc_steps=M, episode_length=1, max_lat_dev=np.inf, auto_reset=False, full_lap=True, log_capacity=E * M)
    n = len(env.loop.track)
    starts = np.array([n - 6, n - 5, 0])          # two vehicles a few metres in front of waypoint n - 2, one that has a lap to go
    env.dev.env_reset(starts)
    d = _stack([env.step(a) for a in actions])
    logs = env.dev.logs()
    idx = closest_index(env.loop.track, logs["CiLX"][:E * M, :, :2])
    assert (idx[:, :2] == n - 2).any(axis=0).all() and not (idx[:, 2] == n - 2).any()          # passed within the run / never reached
    host = _host_rules(env.loop, logs, E, M, max_lat_dev=np.inf, episode_length=1, full_lap=True)
    _assert_env_steps(d, host)
    first = (idx == n - 2).argmax(axis=0)
    for b in range(2):
        e, i = divmod(int(first[b]), M)
        assert d["terminated"][e, b] and d["step_length"][e, b] == i + 1 and not d["terminated"][:e, b].any()
    assert not d["terminated"][:, 2].any() and (d["step_length"][:, 2] == M).all()          # (episode_length 1 plays no part)


# ----------------------------------------------------------------------------------------------------------------- 4: lifecycle
ENV_KW = dict(n_mpc_steps=3, max_lat_dev=2.0, episode_length=2, sigmas=SIGMAS, lims=LIMS)


def test_refusals(table):
    snm = _loop(2, 0, controller="snmpc")
    with pytest.raises(Exception, match="SNMPC"):
        snm.dev.attach_env(table, **ENV_KW)
    r2 = _loop(2, 0, controller="r2")
    with pytest.raises(Exception, match="R2"):
        r2.dev.attach_env(table, **ENV_KW)
    fw = _loop(2, 0)
    W = np.diag([1.0, 1.0, 2.0, 3.0, 4.0, 5.0]); W[0, 1] = W[1, 0] = 0.1
    fw.solver.cost_set(3, "W", np.stack([W, W]))
    with pytest.raises(Exception, match="full W"):
        fw.dev.attach_env(table, **ENV_KW)
    sqp = _loop(2, 0)
    sqp.solver.options_set("nlp_solver_type", "SQP")
    with pytest.raises(Exception, match="SQP mode"):
        sqp.dev.attach_env(table, **ENV_KW)
    sqp.solver.options_set("nlp_solver_type", "SQP_RTI")
    sqp.solver.options_set("rti_phase", 1)
    with pytest.raises(Exception, match="rti_phase"):
        sqp.dev.attach_env(table, **ENV_KW)
    seg = _loop(2, 0)
    seg.dev.attach_segments(np.array([10, 20]), 2.0, 2.0)
    with pytest.raises(Exception, match="segments attached"):
        seg.dev.attach_env(table, **ENV_KW)
    seg.dev.detach_segments()
    seg.dev.attach_env(table, **ENV_KW)
    with pytest.raises(Exception, match="RL environment"):
        seg.dev.attach_segments(np.array([10, 20]), 2.0, 2.0)
    with pytest.raises(Exception, match="obs_states"):
        seg.dev.attach_env(table, obs_states="current", **ENV_KW)
    none = _loop(2, 0)
    with pytest.raises(Exception, match="no environment attached"):
        none.dev.env_step(np.zeros(2, dtype=int))
    with pytest.raises(Exception, match="no environment attached"):
        none.dev.env_get("episode_steps")
    # a capsule that changes behind an attached environment is refused at the step
    seg.solver.cost_set(3, "W", np.stack([W, W]))
    with pytest.raises(Exception, match="full W"):
        seg.dev.env_step(np.zeros(2, dtype=int))


def test_bad_actions_and_ended_instances(table):
    cl = _loop(3, 0)
    cl.dev.attach_env(table, **ENV_KW)
    x = _states(cl.dev)
    for bad in ([0, len(table), 0], [0, 0, -1]):
        with pytest.raises(Exception, match="outside the table"):
            cl.dev.env_step(np.array(bad))
    with pytest.raises(Exception, match="outside the track"):
        cl.dev.env_step(np.zeros(3, dtype=int), np.array([0, 1, 0]), np.array([0, len(cl.track), 0]))
    with pytest.raises(Exception, match="integers"):
        cl.dev.env_step(np.array([0.0, 1.0, 2.0]))
    assert cl.dev.steps == 0 and all(np.array_equal(a, b) for a, b in zip(x, _states(cl.dev)))          # nothing ran
    assert not cl.dev.env_step(np.array([0, 1, 2]))["terminated"].any()
    r = cl.dev.env_step(np.array([3, 4, 5]))
    assert r["terminated"].all() and (r["step_length"] == 1).all() and cl.dev.env_get("ended").all()
    with pytest.raises(Exception, match="has ended and it is not marked for reset"):
        cl.dev.env_step(np.array([0, 0, 0]), np.array([1, 0, 1]), np.array([5, 5, 5]))
    assert cl.dev.steps == 6
    r = cl.dev.env_step(np.array([0, 0, 0]), np.array([1, 2, 1]), np.array([5, 5, 5]))
    assert not r["terminated"].any() and cl.dev.env_get("episode_steps").tolist() == [1, 3, 1] and not cl.dev.env_get("ended").any()


def test_detach_and_set_state(table):
    from tum_control_amd.closed_loop import start_states
    actions = np.random.RandomState(8).randint(0, len(table), size=(2, 3))
    cl = _loop(3, 0, log_capacity=60)
    cl.dev.attach_env(table, **ENV_KW)
    cl.dev.env_step(actions[0]); cl.dev.env_step(actions[1])
    assert cl.dev.env_get("episode_steps").tolist() == [2, 2, 2] and cl.dev.env_get("ended").all()
    # set_state zeroes the environment with everything else
    x0 = start_states(cl.track, 350, 3)
    cl.dev.set_state(x0[:, :7], x0, cold_start=True)
    for f in ("episode_steps", "step_length", "flags", "qp_failures", "samples", "ended"):
        assert not cl.dev.env_get(f).any(), f
    # detached: run() is bit for bit a loop that never had an environment (55 steps: two replays of the captured chunk and 5 launches)
    cl.dev.detach_env()
    cl.set_weights(table[actions[0]])
    cl.dev.run(55)
    ref = _loop(3, 350, log_capacity=60)
    ref.set_weights(table[actions[0]])
    ref.dev.run(55)
    _assert_same_logs(cl.dev.logs(), ref.dev.logs())
    with pytest.raises(Exception, match="no environment attached"):
        cl.dev.env_step(actions[0])
