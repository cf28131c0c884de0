"""
Lifetimes of what a device closed loop owns (csrc/sim_loop.hpp, csrc/sim_rl.hpp): buffers that grow on demand and sub-states that are
released and attached again must leave NO trace in what the loop computes. Nothing here is new behaviour -- every comparison is bit for
bit against a loop that allocated once -- so the module passes on a library from before the owners existed as well.
  growth   the rollout log, the collection buffer and the trainer's workspaces are used small first, then larger
  cycles   environment, policy, value net and trainer attached; one of them detached or re-attached, which detaches what stands on it:
           the calls that need what is gone are refused BY THE LIBRARY (the wrapper's own bookkeeping is put back so that they get there);
           everything attached again, and the collect and the minibatch are those of a loop that attached once. Twice round.
B = 3 vehicles, one control step per environment step, at most 3 environment steps: the shapes at which ownership can still go wrong.
A loop is put into a known state by set_state() on its initial state and env_reset() on fixed waypoints.
"""
import numpy as np
import pytest

import ppo_reference as ref
from test_gpu_collect import GAMMA, LAM, LIMS, RESTARTS, SEED, SIGMAS, _env, _starts, agent, table          # noqa: F401 (agent, table: fixtures)
from test_gpu_ppo import _rows, _same_lists, _trainer, dev          # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu

B, M, E = 3, 1, 3
TAB = np.array(RESTARTS)[np.random.RandomState(3).randint(0, len(RESTARTS), size=E * B)].reshape(E, B)
STEP = dict(lr=1e-3, apply=False, want_grads=True, want_rows=True)


def _loop(table, agent=None):
    """(device loop of a fresh environment, its initial state); with the agent's two nets attached where given"""
    d = _env(B, table, n_mpc_steps=M).dev
    if agent is not None:
        d.attach_policy(agent)
    return d, (d.get("x_sim").copy(), d.get("x_mpc").copy())


def _restart(d, x0):
    d.set_state(*x0)
    d.env_reset(_starts(B))


def _minibatch(n_obs, n_act, n=5):
    rng = np.random.RandomState(8)
    return rng.rand(n, n_obs), rng.randint(0, n_act, n), -3.0 + 0.3 * rng.randn(n), rng.randn(n), rng.randn(n)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "grads":
            assert _same_lists(a[k], b[k]), k
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), k


def _same_loop(a, b):
    for f in ("x_sim", "x_mpc", "pose", "ref0"):
        assert np.array_equal(a.get(f), b.get(f)), f
    for f in ("episode_steps", "step_length", "samples", "ended"):
        assert np.array_equal(a.env_get(f), b.env_get(f)), f
    assert a.steps == b.steps


# ---------------------------------------------------------------------------------------------------------------- growth
def test_rollout_log_grows(table, agent):
    (a, xa), (b, xb) = _loop(table, agent), _loop(table, agent)
    assert all(np.array_equal(p, q) for p, q in zip(xa, xb))
    _restart(a, xa)
    first = a.env_rollout(1, on_end=1, start_table=TAB[:1])
    _restart(a, xa)
    ra = a.env_rollout(E, on_end=1, start_table=TAB)
    _restart(b, xb)
    rb = b.env_rollout(E, on_end=1, start_table=TAB)
    assert ra["live"].shape == (E, B) and ra["live"].all() and (ra["terminated"] | ra["truncated"]).any()
    _same(ra, rb)
    _same_loop(a, b)
    _same(first, {k: v[:1] for k, v in rb.items()})          # (and the one-step log held the first of the three steps)


def test_collection_buffer_grows(table, agent):
    (a, xa), (b, xb) = _loop(table, agent), _loop(table, agent)
    _restart(a, xa)
    a.env_collect(1, TAB[:1], SEED, 0, GAMMA, LAM)
    _restart(a, xa)
    ra = a.env_collect(E, TAB, SEED, 0, GAMMA, LAM)
    _restart(b, xb)
    rb = b.env_collect(E, TAB, SEED, 0, GAMMA, LAM)
    assert ra["observations"].shape == (E, B, 22) and ra["episode_starts"][1:].any()          # (episodes end inside: resets from the table)
    _same(ra, rb)
    _same_loop(a, b)


def test_trainer_workspaces_grow(dev):
    """5 rows (one tile of 16) and then 40 (three): the minibatch workspaces, the uploaded buffer and the row records all grow. The
    second trainer is attached anew -- everything it owns is fresh -- and apply=False has left the parameters alone"""
    small, big = ref.case("odd", 5), ref.case("odd", 40)
    a = _trainer(dev, "odd")
    a.step(*_rows(small), **STEP)
    ga = a.step(*_rows(big), **STEP)
    gb = _trainer(dev, "odd").step(*_rows(big), **STEP)
    assert ga["n"] == 40 and ga["log_probs"].shape == ga["values"].shape == (40,) and np.isfinite(ga["loss"])
    _same(ga, gb)


# ---------------------------------------------------------------------------------------------------------------- cycles
@pytest.fixture(scope="module")
def attached_once(table, agent):
    """the collect and the minibatch of a loop that attached everything once: what every cycle must reproduce; not to be changed"""
    d, x0 = _loop(table, agent)
    d.ppo_attach(**ref.SETTINGS)
    _restart(d, x0)
    return d.env_collect(E, TAB, SEED, 0, GAMMA, LAM), d.ppo_step(*_minibatch(22, len(table)), **STEP)


@pytest.mark.parametrize("start", ["env", "policy", "value"])
def test_detach_and_attach_again(start, table, agent, attached_once):
    d, x0 = _loop(table, agent)
    d.ppo_attach(**ref.SETTINGS)
    rows = _minibatch(22, len(table))
    obs = np.random.RandomState(4).rand(2, 22)
    acted = d.policy_eval(obs)
    for _ in range(2):
        widths = d.policy_widths, d.value_widths
        if start == "env":          # re-attaching the environment detaches the policy, that the value net, that the trainer
            d.attach_env(table, M, 2.0, 2, SIGMAS, LIMS, 10, full_lap=False, obs_states="reference")
        elif start == "policy":
            d.detach_policy()
        else:
            d.detach_value()
        d.policy_widths, d.value_widths = widths          # (the wrapper would refuse on its own bookkeeping: the library is asked)
        if start == "value":          # the policy stands: it acts as before, alone and in a rollout
            _same(d.policy_eval(obs), acted)
            _restart(d, x0)
            assert d.env_rollout(1, on_end=1, start_table=TAB[:1])["live"].shape == (1, B)
            gone = "no value net attached"
        else:
            with pytest.raises(Exception, match="policy_eval: no policy attached"):
                d.policy_eval(obs)
            with pytest.raises(Exception, match="env_rollout: no policy attached"):
                d.env_rollout(1, on_end=1, start_table=TAB[:1])
            gone = "no policy attached"
        with pytest.raises(Exception, match="env_collect: " + gone):
            d.env_collect(E, TAB, SEED, 0, GAMMA, LAM)
        with pytest.raises(Exception, match="ppo_step: no trainer attached"):
            d.ppo_step(*rows, **STEP)
        d.attach_policy(agent)
        d.ppo_attach(**ref.SETTINGS)
        _restart(d, x0)
        _same(d.env_collect(E, TAB, SEED, 0, GAMMA, LAM), attached_once[0])
        _same(d.ppo_step(*rows, **STEP), attached_once[1])
        _same(d.policy_eval(obs), acted)
