"""
The disturbance realisation drawn on the device (disturbance_draw_kernel, csrc/disturbance_kernels.hpp; tum_sim_disturbances_attach,
tum_sim_disturbances_table) against the exact restatement of tests/disturbance_reference.py, against its own regenerated table played
back through tum_sim_set_disturbances, and through every path that enqueues control steps: run (captured chunks and plain launches),
the segments, the environment's step / rollout / collect. Shipped tracks, N = 38, the shipped magnitudes with both streams on.

The gate of the two normal kinds is test_disturbance_reference.gate_units: max(32, 4 x the plain statement's own error), in the units of
disturbance_reference; nothing in it comes from a device result. 'absolute' and the box kind are equal to draw_counter to the bit.
The table test prints what the device needed of its gate beside the plain statement's share ("disturbance_bounds ..." lines):
profiles/disturbance_bounds.txt.
"""
import ctypes
import os

import numpy as np
import pytest

import disturbance_reference as dr
from disturbance_reference import same_bits
from test_disturbance_reference import gate_units

pytestmark = pytest.mark.gpu

TRACK, N, TP = "monteblanco", 38, 3.04
TWO = ("monteblanco", "modena")
LOGS = ("CiLX", "MPC_SimX", "simU", "simREF", "simSolverDebug")
SEED = 0x1234567890abcdef          # both words of the key in use
_dp = ctypes.POINTER(ctypes.c_double)


def _model(kind_w="uniform", kind_e="gaussian", **kw):
    from tum_control_amd.closed_loop import DisturbanceModel
    return DisturbanceModel(dict(simulate_disturbances=True, simulate_state_estimation=True, disturbance_type_derivatives=kind_w,
                                 disturbance_type_state_estimation=kind_e, **kw))


def _starts(B):
    return np.array([0, 350, 800, 137, 1000])[np.arange(B) % 5]


def _loop(B, log_capacity=0, controller="nominal", **kw):
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(TRACK, batch=B, N=N, Tp=TP, idx_start=_starts(B), on_device=True, log_capacity=log_capacity,
                           controller=controller, **kw)


def _assert_same_logs(a, b, what=""):
    for k in LOGS:
        assert same_bits(a[k], b[k]), (what, k, int(np.argmax((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1))))


# ---------------------------------------------------------------------------------------------- 1: the table against the exact reference
@pytest.fixture(scope="module")
def loop33():
    return _loop(33)


def _shares(got, kind, w, seed, first_step, s):
    """largest error of a table (n, B, 7) in units of its gate, and the plain statement's on the same rows"""
    from tum_control_amd import closed_loop as clm
    gate = gate_units(kind)
    dev = plain = 0.0
    for i in range(got.shape[0]):
        for b in range(got.shape[1]):
            mA, mB = dr.mantissas(seed, b, first_step + i, s)
            ref = dr.exact(kind, w, mA, mB)
            dev = max(dev, dr.errors(got[i, b], ref).max() / gate)
            plain = max(plain, dr.errors(clm.disturbance_from_uniforms(kind, w, *dr.uniforms(mA, mB)), ref).max() / gate)
    return dev, plain


@pytest.mark.parametrize("kinds,seed", ((("uniform", "gaussian"), SEED), (("gaussian", "uniform"), 77),
                                        (("absolute", "box"), SEED), (("box", "absolute"), 3)))
def test_table_against_the_exact_reference(kinds, seed, loop33):
    """disturbance_table(0, 8) at batch 33, every kind once on each stream; and three steps from 2^31 - 4 (the step word widens)"""
    m = _model(*kinds)
    dev = loop33.dev
    dev.attach_disturbances(m, seed)
    for first, n in ((0, 8), (2 ** 31 - 4, 3)):
        tab = dev.disturbance_table(first, n)
        host = m.draw_counter(n, batch=33, seed=seed, first_step=first)
        for s, (kind, bounds) in enumerate(zip(kinds, (m.bounds_derivatives, m.bounds_state_estimation))):
            assert tab[s].shape == (n, 33, 7)
            if kind in ("absolute", "box"):
                assert same_bits(tab[s], host[s]), (kind, s, first)
                continue
            share, plain = _shares(tab[s], kind, np.array(bounds)[:, 1], seed, first, s)
            print(f"disturbance_bounds device {kind} stream {s} first_step {first}: device needed {share:.4g} of its gate, "
                  f"the plain statement {plain:.4g}")
            assert share < 1.0, (kind, s, first, share)
    dev.attach_disturbances(None)


def test_table_of_a_stream_that_is_off_and_of_a_zero_bound(loop33):
    dev = loop33.dev
    m = _model("uniform", "gaussian", w_yaw_dot=0.0, w_vlat=0.0)
    m.state_estimation = False
    dev.attach_disturbances(m, 5)
    w, e = dev.disturbance_table(2, 4)
    assert e is None and (w[..., 2] == 0.0).all() and (w[..., 3] != 0.0).all()
    bw = np.array(m.bounds_derivatives)[:, 1]
    pos = bw > 0
    assert (np.sum(w[..., pos] ** 2 / bw[pos], axis=-1) <= 1 + 1e-12).all()
    # the C entry hands zeros out for the stream that is off
    buf = np.full((4, 33, 7), 3.0)
    assert dev._L.tum_sim_disturbances_table(dev._s, 2, 4, None, buf.ctypes.data_as(_dp)) == 0 and (buf == 0.0).all()
    m.state_estimation, m.derivatives = True, False
    dev.attach_disturbances(m, 5)
    w, e = dev.disturbance_table(2, 4)
    assert w is None and (e[..., 4] == 0.0).all() and (e[..., 3] != 0.0).all()
    dev.attach_disturbances(None)


# ---------------------------------------------------------------------------------------------- 2: window and batch
def test_a_row_does_not_depend_on_the_window_or_the_batch(loop33):
    m = _model()
    loop33.dev.attach_disturbances(m, SEED)
    full = loop33.dev.disturbance_table(0, 8)
    part = loop33.dev.disturbance_table(3, 3)
    loop33.dev.attach_disturbances(None)
    for s in range(2):
        assert same_bits(part[s], full[s][3:6])
    for B in (17, 1):
        small = _loop(B)
        small.dev.attach_disturbances(m, SEED)
        tab = small.dev.disturbance_table(0, 8)
        for s in range(2):
            assert same_bits(tab[s], full[s][:, :B]), (B, s)


# ---------------------------------------------------------------------------------------------- 3: live equals playback
def _live_and_playback(B, n, controller="nominal"):
    m = _model()
    live = _loop(B, log_capacity=n, controller=controller, disturbances=m, draw="device", seed=SEED)
    logs = live.run(n)
    w, e = live.dev.disturbance_table(0, n)
    back = _loop(B, log_capacity=n, controller=controller, disturbances=(w, e))
    return live, logs, back, back.run(n)


@pytest.mark.parametrize("B,controller", ((1, "nominal"), (17, "nominal"), (33, "nominal"), (17, "snmpc"), (17, "r2")))
def test_live_draw_equals_playback_of_its_table(B, controller):
    """run(60): two replays of the 25-step captured chunk and 10 plain launches, the step read from the loop's counter on the device"""
    live, logs, back, logs_b = _live_and_playback(B, 60, controller)
    assert live.dev.graph_steps == 25 and back.dev.graph_steps == 25
    assert logs["simU"].shape[0] == 60
    _assert_same_logs(logs, logs_b, (B, controller))
    if (B, controller) == (17, "nominal"):
        # the second run continues the realisation at step 60 (it does not restart at 0): against playback of steps 0..119
        w, e = live.dev.disturbance_table(0, 120)
        back.set_disturbances(w, e)
        live.run(60); back.run(60)
        for f in ("x_sim", "x_mpc"):
            assert same_bits(live.dev.get(f), back.dev.get(f)), f
        again = _loop(B, disturbances=(np.concatenate([w[:60], w[:60]]), np.concatenate([e[:60], e[:60]])))
        again.run(120)
        assert not same_bits(again.dev.get("x_mpc"), live.dev.get("x_mpc"))


# ---------------------------------------------------------------------------------------------- 4: exclusivity, refusals
@pytest.fixture(scope="module")
def runs20():
    """20 control steps at batch 17: undisturbed, and with the live generator"""
    plain = _loop(17, log_capacity=20)
    live = _loop(17, log_capacity=20, disturbances=_model(), draw="device", seed=SEED)
    return dict(plain=plain.run(20), live=live.run(20), table=live.dev.disturbance_table(0, 20))


def test_generator_and_table_exclude_each_other(runs20):
    m = _model()
    junk = _model("box", "box").draw_counter(20, batch=17, seed=1)
    # a table, then the generator: the generator's bits
    a = _loop(17, log_capacity=20, disturbances=junk)
    a.dev.attach_disturbances(m, SEED)
    _assert_same_logs(a.run(20), runs20["live"], "generator over table")
    # the generator, then a table: the table's bits, and no generator left to ask
    b = _loop(17, log_capacity=20, disturbances=_model("box", "box"), draw="device", seed=1)
    b.set_disturbances(*runs20["table"])
    with pytest.raises(Exception, match="no generator attached"):
        b.dev.disturbance_table(0, 1)
    _assert_same_logs(b.run(20), runs20["live"], "table over generator")
    # detached: the undisturbed loop's bits
    c = _loop(17, log_capacity=20, disturbances=m, draw="device", seed=SEED)
    c.dev.attach_disturbances(None)
    _assert_same_logs(c.run(20), runs20["plain"], "detached")


def test_bad_kinds_and_bounds_are_refused(runs20):
    cl = _loop(17, log_capacity=20)
    dev = cl.dev
    L, s = dev._L, dev._s
    good = np.array(_model().bounds_derivatives)[:, 1].copy()
    err = lambda: L.tum_ocp_last_error().decode()
    assert L.tum_sim_disturbances_attach(s, 5, good.ctypes.data_as(_dp), 0, None, 1) != 0 and "outside 0..4" in err()
    assert L.tum_sim_disturbances_attach(s, 0, None, -1, good.ctypes.data_as(_dp), 1) != 0 and "outside 0..4" in err()
    assert L.tum_sim_disturbances_attach(s, 1, None, 0, None, 1) != 0 and "no bounds" in err()
    for bad in (-0.1, np.nan, np.inf):
        w = good.copy(); w[3] = bad
        assert L.tum_sim_disturbances_attach(s, 0, None, 2, w.ctypes.data_as(_dp), 1) != 0
        assert "bound 3 of the state estimation error is negative or not finite" in err()
    with pytest.raises(Exception, match="no generator attached"):
        dev.disturbance_table(0, 1)
    assert L.tum_sim_disturbances_table(s, -1, 1, None, None) != 0 and "first_step < 0" in err()
    # the loop is as usable as before
    _assert_same_logs(cl.run(20), runs20["plain"], "after refusals")


# ---------------------------------------------------------------------------------------------- 5: segments
def test_segments_live_equals_playback(golden_dir):
    from tum_control_amd import closed_loop as clm
    P = np.load(os.path.join(golden_dir, "closed_loop_monteblanco_150.npz"))["params"][[0, 9]]
    groups = [[(0, 16)], [(350, 366)]]
    m, max_steps = _model(), 80
    live = clm.evaluate_segments(TRACK, P, groups, 2.0, np.inf, max_steps, N=N, Tp=TP, check_every=40, disturbances=m, seed=SEED, draw="device")
    probe = _loop(4)
    probe.dev.attach_disturbances(m, SEED)
    back = clm.evaluate_segments(TRACK, P, groups, 2.0, np.inf, max_steps, N=N, Tp=TP, check_every=40,
                                 disturbances=probe.dev.disturbance_table(0, max_steps))
    plain = clm.evaluate_segments(TRACK, P, groups, 2.0, np.inf, max_steps, N=N, Tp=TP, check_every=40)
    assert same_bits(live[0], back[0]) and np.array_equal(live[1], back[1])
    assert set(live[2]) == set(back[2])
    for k in live[2]:
        assert same_bits(np.asarray(live[2][k], dtype=float), np.asarray(back[2][k], dtype=float)), k
    assert (live[2]["steps"] > 20).all() and live[2]["done"].any()
    assert not same_bits(live[2]["rms_vel_dev"], plain[2]["rms_vel_dev"])


# ---------------------------------------------------------------------------------------------- 6: the environment
M_ENV, B_ENV = 20, 16
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))
RESTARTS = ((0, 200, 640, 1100), (7, 350, 950))


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


@pytest.fixture(scope="module")
def agent(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"), os.path.join(golden_dir, "wmpc_value.npz"))


def _env(table, n_mpc_steps=M_ENV, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    starts = np.array([0, 7, 200, 350, 640, 950, 1100, 7])[np.arange(B_ENV) % 8]
    return WeightScheduleEnv(list(TWO), B_ENV, table, rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=starts, n_mpc_steps=n_mpc_steps,
                             auto_reset=True, episode_length=2, max_lat_dev=np.inf, restart_indices=RESTARTS, seed=9, **kw)


def _env_pair(table, n_control_steps, **kw):
    """an environment with the live generator, and one that plays the regenerated table of its first n_control_steps back"""
    live = _env(table, disturbances=_model(), draw="device", disturbance_seed=SEED, **kw)
    back = _env(table, disturbances=live.dev.disturbance_table(0, n_control_steps), **kw)
    return live, back


def _same(a, b, what):
    if isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], (what, k))
    elif isinstance(a, np.ma.MaskedArray):
        assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), what
        _same(np.asarray(a.data), np.asarray(b.data), what)
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), what


def test_env_step_live_equals_playback(table):
    live, back = _env_pair(table, 3 * M_ENV)
    rng = np.random.RandomState(3)
    outs = []
    for env in (live, back):
        env.reset()
    assert np.array_equal(live.last_start, back.last_start)
    for e in range(3):
        actions = rng.randint(0, len(table), size=B_ENV)
        got = [env.step(actions) for env in (live, back)]
        for x, y, name in zip(got[0], got[1], ("obs", "reward", "terminated", "truncated", "info")):
            _same(x, y, (e, name))
        outs.append(got[0])
    assert live.dev.steps == 3 * M_ENV
    # and it is disturbed: an undisturbed environment earns other rewards
    plain = _env(table)
    plain.reset()
    rng = np.random.RandomState(3)
    rewards = [plain.step(rng.randint(0, len(table), size=B_ENV))[1] for _ in range(3)]
    assert not same_bits(np.array(rewards), np.array([o[1] for o in outs]))


def test_env_rollout_and_collect_live_equal_playback(table, agent):
    live, back = _env_pair(table, 3 * M_ENV)
    for env in (live, back):
        env.reset()
    _same(live.rollout(agent, 3), back.rollout(agent, 3), "rollout")
    live, back = _env_pair(table, 2 * M_ENV)
    for env in (live, back):
        env.reset()
    _same(live.collect(agent, 2, 0.99, 0.95), back.collect(agent, 2, 0.99, 0.95), "collect")


# ---------------------------------------------------------------------------------------------- 7: disturbed, and only where the reference is
def test_a_disturbed_loop_is_disturbed_where_the_reference_is(runs20):
    """the estimator is fed the disturbed step, so the controller's states differ; the plant's TRUE first step is the undisturbed one
    (SimulationMode_main_class.py:112-143, kept by plant_advance_kernel): CiLX[1] is equal to the bit"""
    live, plain = runs20["live"], runs20["plain"]
    assert not same_bits(live["MPC_SimX"], plain["MPC_SimX"])
    assert same_bits(live["CiLX"][:2], plain["CiLX"][:2])
    assert not same_bits(live["CiLX"][2:], plain["CiLX"][2:])
    w, e = runs20["table"]
    assert w.shape == e.shape == (20, 17, 7) and np.abs(w).max() > 0 and np.abs(e).max() > 0


def test_save_fetches_the_realisation_of_a_device_loop(tmp_path, runs20):
    cl = _loop(17, log_capacity=20, disturbances=_model(), draw="device", seed=SEED)
    cl.run(20)
    f = cl.save(str(tmp_path / "v3.npz"), instance=3, drop_last_step=False)[0]
    z = np.load(f)
    assert same_bits(z["sim_disturbance_derivatives"], runs20["table"][0][:, 3])
    assert same_bits(z["sim_disturbance_state_estimation"], runs20["table"][1][:, 3])


def test_counter_mode_plays_the_same_stream_back(runs20):
    """draw="counter": the host statement of the stream, played back -- on the device loop the live loop's bits wherever the kinds are
    exact statements (box, 'absolute'); with on_device=False the host loop gets the same arrays"""
    m = _model("box", "absolute")
    live = _loop(17, log_capacity=20, disturbances=m, draw="device", seed=SEED)
    back = _loop(17, log_capacity=20, disturbances=m, draw="counter", seed=SEED, disturbance_steps=20)
    _assert_same_logs(live.run(20), back.run(20), "counter against device")
    assert not same_bits(live._last_logs["MPC_SimX"], runs20["plain"]["MPC_SimX"])
    from tum_control_amd.closed_loop import ClosedLoopBatch
    host = ClosedLoopBatch(TRACK, batch=2, N=N, Tp=TP, idx_start=_starts(2), disturbances=_model(), draw="counter", seed=SEED, disturbance_steps=3)
    w, e = _model().draw_counter(3, batch=2, seed=SEED)
    assert same_bits(host.w_deriv, w) and same_bits(host.e_est, e)
    host.run(2)
    assert len(host.log["simU"]) == 2
