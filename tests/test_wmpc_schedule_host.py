"""
The host statement of the learned weight schedule (closed_loop.wmpc_observation, WmpcSchedule): the observation the controller
classes form at a decision step against what the reference's LonLatDeviations and ObservationGenerator computed for the same inputs
(tests/golden/wmpc_schedule.npz, written by tests/golden/make_wmpc_schedule_golden.py), and the counter rule against a literal
transcription of NMPC_class.py:208-239. No GPU.

Gate of the observation, 1e-12 absolute + relative, that of tests/test_rl_env_host.py: the same numpy operations as the reference on the
same inputs; differences are a few ulp of O(1) numbers.
"""
import os

import numpy as np
import pytest

from tum_control_amd import closed_loop as cl

TOL = 1e-12


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "wmpc_schedule.npz"))


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and bool((np.abs(a - b) <= TOL + TOL * np.abs(b)).all())


def test_observation_matches_reference(gold):
    n = int(gold["n"])
    assert n >= 35
    lengths, seams, sides = set(), 0, set()
    for i in range(n):
        x0, ref, (Ts, ns), (lat, vel) = gold[f"case_{i}_x0"], gold[f"case_{i}_ref"], gold[f"case_{i}_args"], gold[f"case_{i}_dev"]
        lengths.add(len(ref))
        seams += bool((np.abs(np.diff(ref[:, 2])) > np.pi).any())
        sides.add(bool(lat > 0))
        assert abs(lat) <= 2.5 and abs(vel) <= 3.5 and abs(lat) + abs(vel) > 0          # unlike the environment's, whose entries are 0, 0
        obs = cl.wmpc_observation(x0, ref[0], ref[:, 2], ref[:, 3], Ts, int(ns))
        assert obs.shape == (2 + 2 * int(ns),)
        assert _close(obs, gold[f"case_{i}_obs"]), (i, np.abs(obs - gold[f"case_{i}_obs"]).max())
        # the two deviations themselves, and that they are what fills the first two entries
        _, lat_h = cl.lon_lat_deviations(x0[2], x0[0], x0[1], ref[0, 0], ref[0, 1])
        assert _close([lat_h, x0[3] - ref[0, 3]], [lat, vel])
        assert _close(obs, cl.rl_observation(ref[:, 2], ref[:, 3], Ts, int(ns), lat, vel))
    assert lengths == {39, 11} and seams >= 4 and sides == {True, False}


def _transcription(period, steps):
    """NMPC_class.py:208-239 with everything but the counter taken out"""
    steps_since_weight_update, decided = 0, []
    for k in range(steps):
        if steps_since_weight_update >= period:
            steps_since_weight_update = 0
            decided.append(k)
        steps_since_weight_update += 1
    return decided


class _Agent:
    """an agent whose action is a function of the observation's first entry"""
    n_observations, n_actions = 22, 26

    def predict(self, obs):
        return int(np.floor(np.asarray(obs)[..., 0] * 1e3)) % 26


@pytest.mark.parametrize("period", [0, 1, 2, 7, 20])
def test_schedule_is_the_counter_rule(period, gold):
    steps, B = 100, 3
    table = np.arange(26 * 7, dtype=float).reshape(26, 7)
    s = cl.WmpcSchedule(_Agent(), table, period, batch=B, log_capacity=steps)
    refs = [gold[f"case_{i}_ref"] for i in range(B)]
    x0 = np.stack([gold[f"case_{i}_x0"] for i in range(B)])
    yref = np.zeros((B, 39, 6)); yref[:, :, :4] = np.stack(refs)
    ref0 = np.stack([r[0] for r in refs])
    decided = []
    for k in range(steps):
        due, actions = s.after_solve(k, x0, ref0, yref)
        assert len(due) == len(actions) and (len(due) in (0, B))
        if len(due):
            decided.append(k)
            want = [_Agent().predict(cl.wmpc_observation(x0[b], ref0[b], refs[b][:, 2], refs[b][:, 3], 0.02, 10)) for b in range(B)]
            assert actions.tolist() == want and s.current_action == want
    want = _transcription(period, steps)
    assert decided == want
    if period == 20:
        assert want == [20, 40, 60, 80]
    if period == 1:
        assert want == list(range(1, 100))
    if period == 0:
        assert want == list(range(100))
    assert (s.n_decisions == len(want)).all() and (s.steps[:, :len(want)] == np.array(want)).all() and (s.steps[:, len(want):] == -1).all()
    assert (s.counter == (steps - want[-1])).all()


def test_schedule_refusals_and_log_capacity():
    table = np.zeros((26, 7))
    with pytest.raises(ValueError, match="negative"):
        cl.WmpcSchedule(_Agent(), table, -1)
    with pytest.raises(ValueError, match="25 rows"):
        cl.WmpcSchedule(_Agent(), table[:25], 20)
    with pytest.raises(ValueError, match="n_actions, 7"):
        cl.WmpcSchedule(_Agent(), table[:, :6], 20)
    stacked = _Agent()
    stacked.n_observations = 45          # (n_obs_stack > 1 cannot give an even width above... 2 x 22 + 1: not an observation)
    with pytest.raises(ValueError, match="2 \\+ 2 n_samples"):
        cl.WmpcSchedule(stacked, table, 20)
    s = cl.WmpcSchedule(_Agent(), table, 0, batch=1, log_capacity=2)
    x0, ref = np.zeros((1, 8)), np.zeros((1, 39, 6))
    ref[0, :, 2] = np.linspace(0, 1, 39)
    for k in range(5):
        s.after_solve(k, x0, ref[:, 0, :4], ref)
    assert s.n_decisions[0] == 5 and s.steps.tolist() == [[0, 1]]          # past capacity: counted, not stored
