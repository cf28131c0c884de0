"""
Collecting PPO training data on the device: policy_ac_kernel (tum_sim_policy_attach_value / _eval_ac) against the long-double
references of tests/collect_reference.py within their bounds and against the host's uniforms to the bit; gae_kernel (tum_sim_gae)
against the literal loop bit for bit; tum_sim_env_collect / WeightScheduleEnv.collect against the host-driven loop -- policy_eval_ac on
the observation just returned, env_step, policy_eval_ac values of the terminal observations, the literal GAE loop -- BIT FOR BIT on every
returned array: both paths run the same kernels on the same words.
Shipped track, N = 38, n_mpc_steps 3, the 26-row table of tests/golden/rl_env.npz, the agent of wmpc_policy.npz + wmpc_value.npz.
"""
import os

import numpy as np
import pytest

import collect_reference as cr
import policy_reference as pr
from test_gpu_policy import C_TANH, NETS, _assert_same_steps, _host_driven, _pool

pytestmark = pytest.mark.gpu

TRACK, N, TP, M = "monteblanco", 38, 3.04, 3
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))
SEED, T = 0x1234567890abcdef, 2 ** 32 + 5          # both words of the key and of the decision counter in use
GAMMA, LAM = 0.99, 0.95
RESTARTS = (0, 200, 640, 900)
STEP_KEYS = ("observations", "actions", "log_probs", "values", "rewards", "rewards_raw", "episode_starts", "terminated", "truncated",
             "step_length", "qp_failures")
ALL_KEYS = STEP_KEYS + ("advantages", "returns", "last_values", "last_dones")
# value nets of another depth and other widths than the policy net they go with; "tiny" gets one WIDER than its policy net (the LDS
# buffers are sized by the larger of the two)
VALUE_NETS = {"fixture": (22, 37, 1), "odd": (23, 7, 50, 9, 30, 1), "tiny": (3, 200, 17, 1), "widest": (128, 256, 200, 1)}


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


@pytest.fixture(scope="module")
def agent(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"), os.path.join(golden_dir, "wmpc_value.npz"))


@pytest.fixture(scope="module")
def bare_loop():
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(TRACK, batch=2, N=N, Tp=TP, on_device=True)


def _starts(B):
    return np.array([0, 350, 800, 137, 1000])[np.arange(B) % 5]


def _env(B, table, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    kw = dict(dict(rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=_starts(B), n_mpc_steps=M, auto_reset=True, episode_length=2,
                   restart_indices=RESTARTS, seed=9), **kw)
    return WeightScheduleEnv(TRACK, B, table, **kw)


def _drawn_table(E, B, seed=9):
    """what WeightScheduleEnv draws for E steps when nothing has been drawn before"""
    return np.array(RESTARTS)[np.random.RandomState(seed).randint(0, len(RESTARTS), size=E * B)].reshape(E, B)


# ---------------------------------------------------------------------------------------------------------------- policy_eval_ac
@pytest.mark.parametrize("net", list(VALUE_NETS))
def test_eval_ac_within_the_bounds(net, agent, bare_loop):
    from tum_control_amd.closed_loop import WeightPolicy, policy_uniforms
    W, b = (agent.weights, agent.biases) if NETS[net] is None else pr.synthetic_policy(NETS[net], 11)
    V, c = pr.synthetic_policy(VALUE_NETS[net], 12)
    assert len(V) != len(W) and [w.shape[0] for w in V[:-1]] != [w.shape[0] for w in W[:-1]]
    dev = bare_loop.dev
    dev.attach_policy(WeightPolicy(W, b, V, c))
    x = _pool(W[0].shape[1], np.random.RandomState(2))
    vref, vbound = cr.value(V, c, x, c_tanh=C_TANH)
    FI = 3
    rows = aside = 0
    res = {}
    for n in (1, 15, 16, 17, 33, 5):
        r = res[n] = dev.policy_eval_ac(x[:n], SEED, T, first_instance=FI)
        u = cr.uniforms(SEED, T, n, first_instance=FI)
        assert np.array_equal(r["uniforms"], u) and np.array_equal(policy_uniforms(SEED, T, n, FI), u)
        verr = np.abs(r["values"].astype(pr.LD) - vref[:n]).astype(np.float64)
        lp, lbound = cr.log_prob(W, b, x[:n], r["actions"], c_tanh=C_TANH)
        lerr = np.abs(r["log_probs"].astype(pr.LD) - lp).astype(np.float64)
        want, decided = cr.sample(W, b, x[:n], u, c_tanh=C_TANH)
        print(net, n, "values err / bound", (verr / vbound[:n]).max(), "log_probs err / bound", (lerr / lbound).max(), "set aside", int((~decided).sum()))
        assert r["actions"].shape == r["values"].shape == r["log_probs"].shape == (n,)
        assert (verr <= vbound[:n]).all() and (lerr <= lbound).all()
        assert np.array_equal(r["actions"][decided], want[decided])
        assert ((r["actions"] >= 0) & (r["actions"] < W[-1].shape[0])).all()
        rows += n; aside += int((~decided).sum())
    assert aside <= rows // 1000
    # the stream depends on (seed, first_instance + i, t) alone: rows 0 to 4 of n = 17 are n = 5; a shifted batch; another t, another seed
    for k in ("actions", "values", "log_probs", "uniforms"):
        assert np.array_equal(res[17][k][:5], res[5][k]), k
    r = dev.policy_eval_ac(x[4:12], SEED, T, first_instance=FI + 4)
    for k in ("actions", "values", "log_probs", "uniforms"):
        assert np.array_equal(r[k], res[17][k][4:12]), k
    for seed, t in ((SEED, T + 1), (SEED, T - 2 ** 32), (SEED + 1, T), (SEED - 0x1234567800000000, T)):
        r = dev.policy_eval_ac(x[:17], seed, t, first_instance=FI)
        assert np.array_equal(r["uniforms"], cr.uniforms(seed, t, 17, first_instance=FI)) and not np.array_equal(r["uniforms"], res[17]["uniforms"])
        assert np.array_equal(r["values"], res[17]["values"])
    # the policy net alone: no values without a value net, everything else as before
    dev.detach_value()
    r = dev.policy_eval_ac(x[:17], SEED, T, first_instance=FI)
    assert "values" not in r
    for k in ("actions", "log_probs", "uniforms"):
        assert np.array_equal(r[k], res[17][k]), k
    with pytest.raises(Exception, match="no value net attached"):
        dev.policy_eval_ac(x[:17], SEED, T, values=True)
    # and the deterministic path beside it is untouched
    z, bound = pr.forward(W, b, x, c_tanh=C_TANH)
    assert np.array_equal(dev.policy_eval(x)["actions"], pr.actions(z))


def test_eval_ac_fixture_agent(agent, bare_loop):
    """the trained value net itself, on seeded rows: within the bound; the sampled actions follow the long-double CDF"""
    dev = bare_loop.dev
    dev.attach_policy(agent)
    x = pr.seeded_observations()[0][:256]
    r = dev.policy_eval_ac(x, SEED, T)
    v, vb = cr.value(agent.value_weights, agent.value_biases, x, c_tanh=C_TANH)
    assert (np.abs(r["values"].astype(pr.LD) - v).astype(np.float64) <= vb).all()
    want, decided = cr.sample(agent.weights, agent.biases, x, cr.uniforms(SEED, T, 256), c_tanh=C_TANH)
    assert decided.all() and np.array_equal(r["actions"], want) and np.array_equal(r["actions"], agent.sample(x, SEED, T))
    assert len(np.unique(r["actions"])) > 3


# ---------------------------------------------------------------------------------------------------------------- GAE
@pytest.mark.parametrize("E,B", [(1, 1), (3, 65), (6, 17)])
def test_gae_kernel_equals_the_loop(E, B, bare_loop):
    rng = np.random.RandomState(E * 100 + B)
    r, v, es = rng.randn(E, B), rng.randn(E, B), (rng.rand(E, B) < 0.4).astype(float)
    lv, ld = rng.randn(B), (rng.rand(B) < 0.5).astype(float)
    adv, ret = bare_loop.dev.gae(r, v, es, lv, ld, GAMMA, LAM)
    a0, r0 = cr.gae_loop(r, v, es, lv, ld, GAMMA, LAM)
    assert np.array_equal(adv, a0) and np.array_equal(ret, r0)


# ---------------------------------------------------------------------------------------------------------------- collect
def _host_loop(env, policy, start_table, E, seed, t0=0, state=None):
    """the host-driven collection on env.dev; state = (obs, episode_starts, ended) to continue from (None: after a reset)"""
    dev, B = env.dev, env.n_envs
    dev.attach_policy(policy)
    obs, es, ended = state if state is not None else (np.zeros((B, env.n_observations)), np.ones(B), np.zeros(B, dtype=bool))
    rows = {k: [] for k in STEP_KEYS}
    for e in range(E):
        a = dev.policy_eval_ac(obs, seed, t0 + e)
        h = dev.env_step(a["actions"], ended.astype(np.int32), np.where(ended, start_table[e], 0))
        tv = dev.policy_eval_ac(h["observation"], 0, 0)["values"]
        crash = h["truncated"] & ~h["terminated"]
        rew = h["reward"].copy()
        rew[crash] = h["reward"][crash] + GAMMA * tv[crash]
        for k, v in (("observations", obs), ("actions", a["actions"]), ("log_probs", a["log_probs"]), ("values", a["values"]), ("rewards", rew),
                     ("rewards_raw", h["reward"]), ("episode_starts", es), ("terminated", h["terminated"]), ("truncated", h["truncated"]),
                     ("step_length", h["step_length"]), ("qp_failures", h["qp_failures"])):
            rows[k].append(np.array(v))
        ended = h["terminated"] | h["truncated"]
        es = ended.astype(float)
        obs = np.where(ended[:, None], 0.0, h["observation"])
    out = {k: np.stack(v) for k, v in rows.items()}
    out["last_values"], out["last_dones"] = dev.policy_eval_ac(obs, 0, 0)["values"], es
    out["advantages"], out["returns"] = cr.gae_loop(out["rewards"], out["values"], out["episode_starts"], out["last_values"], out["last_dones"], GAMMA, LAM)
    return out, (obs, es, ended)


def _assert_same(a, b, keys=ALL_KEYS, rows=slice(None)):
    for k in keys:
        x, y = (a[k], b[k]) if k.startswith("last_") else (a[k][rows], b[k][rows])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), k


def _crash_threshold(B, table, agent):
    """a crash threshold from the lateral deviations of a first environment step: between the instances' largest values, so that some
    instances crash in the FIRST step of an episode (where the episode length does not end it as well) and some do not"""
    from tum_control_amd import closed_loop as clm
    env = _env(B, table, log_capacity=M)
    env.collect(agent, 1, GAMMA, LAM, seed=SEED)
    lg = env.dev.logs()
    lat, _, _ = clm.segment_step_channels(lg["CiLX"][:M], lg["simREF"], lg["MPC_SimX"][1:M + 1, :, 7], env.loop.cfg)
    top = np.sort(lat.max(axis=0))
    gaps = np.diff(top)
    i = int(np.argmax(gaps[len(top) // 3:])) + len(top) // 3          # the widest gap in the upper two thirds
    thr = 0.5 * (top[i] + top[i + 1])
    assert np.abs(lat - thr).min() > 1e-9 and 0 < (lat.max(axis=0) > thr).sum() < B
    return thr


@pytest.mark.parametrize("B", [5, 17])
def test_collect_equals_the_host_driven_loop(B, table, agent):
    E = 6
    thr = _crash_threshold(B, table, agent)
    a = _env(B, table, max_lat_dev=thr, log_capacity=E * M)
    b = _env(B, table, max_lat_dev=thr, log_capacity=E * M)
    r = a.collect(agent, E, GAMMA, LAM, seed=SEED)
    h, _ = _host_loop(b, agent, _drawn_table(E, B), E, SEED)
    assert set(r) == set(ALL_KEYS) and r["observations"].shape == (E, B, 22) and r["advantages"].shape == (E, B) and r["last_values"].shape == (B,)
    _assert_same(r, h)
    crash, limit = r["truncated"] & ~r["terminated"], r["terminated"]
    print("crashes bootstrapped", int(crash.sum()), "time limits", int(limit.sum()), "of", E * B)
    assert crash.any() and limit.any() and (~crash & ~limit).any()
    assert np.array_equal(r["rewards"] != r["rewards_raw"], crash)
    # the bookkeeping: a row starts an episode exactly where the row before ended one, the first rows after the reset all do
    ended = r["terminated"] | r["truncated"]
    assert (r["episode_starts"][0] == 1).all() and np.array_equal(r["episode_starts"][1:], ended[:-1].astype(float))
    assert np.array_equal(r["last_dones"], ended[-1].astype(float))
    assert (r["observations"][r["episode_starts"] == 1] == 0).all() and (r["observations"][0] == 0).all()
    assert len(np.unique(r["actions"])) > 3
    # the loop itself: the same control steps, the same resets
    la, lb = a.dev.logs(), b.dev.logs()
    for k in la:
        assert np.array_equal(la[k], lb[k]), k
    for f in ("episode_steps", "samples", "ended"):
        assert np.array_equal(a.dev.env_get(f), b.dev.env_get(f)), f
    # an instance that goes on: the value of the step's own observation is the next row's value, to the bit
    go_on = ~ended[:-1]
    tv = a.dev.policy_eval_ac(r["observations"][1:][go_on], 0, 0)["values"]
    assert go_on.any() and np.array_equal(tv, r["values"][1:][go_on])


def test_two_collects_continue_one_stream(table, agent):
    B = 5
    thr = _crash_threshold(B, table, agent)
    a = _env(B, table, max_lat_dev=thr, episode_length=3)          # (rows 2 and 5 end every episode the crashes have not)
    b = _env(B, table, max_lat_dev=thr, episode_length=3)
    r1 = a.collect(agent, 3, GAMMA, LAM, seed=SEED)
    r2 = a.collect(agent, 3, GAMMA, LAM, seed=SEED)
    r = b.collect(agent, 6, GAMMA, LAM, seed=SEED)
    both = {k: np.concatenate([r1[k], r2[k]]) for k in STEP_KEYS}
    _assert_same(both, r, keys=STEP_KEYS)
    assert r["terminated"][2].any() and (r["truncated"] & ~r["terminated"])[:3].any()          # the second call begins on episodes the first one ended
    assert np.array_equal(r2["last_values"], r["last_values"]) and np.array_equal(r2["last_dones"], r["last_dones"])
    adv, ret = cr.gae_loop(both["rewards"], both["values"], both["episode_starts"], r2["last_values"], r2["last_dones"], GAMMA, LAM)
    assert np.array_equal(adv, r["advantages"]) and np.array_equal(ret, r["returns"])
    # each call's own advantages are GAE over its own rows
    adv, ret = cr.gae_loop(r1["rewards"], r1["values"], r1["episode_starts"], r1["last_values"], r1["last_dones"], GAMMA, LAM)
    assert np.array_equal(adv, r1["advantages"]) and np.array_equal(ret, r1["returns"])
    assert a._t == b._t == 6


def test_changed_weights_between_two_collects(table, agent):
    from tum_control_amd.closed_loop import WeightPolicy
    B = 5
    other = WeightPolicy(agent.weights[:-1] + [0.5 * agent.weights[-1]], agent.biases,
                         agent.value_weights, agent.value_biases[:-1] + [agent.value_biases[-1] + np.float32(0.25)])
    a, b = _env(B, table), _env(B, table)
    tab = _drawn_table(6, B)
    a.collect(agent, 3, GAMMA, LAM, seed=SEED)
    r2 = a.collect(other, 3, GAMMA, LAM, seed=SEED)
    _, state = _host_loop(b, agent, tab[:3], 3, SEED)
    h2, _ = _host_loop(b, other, tab[3:], 3, SEED, t0=3, state=state)
    _assert_same(r2, h2)
    go_on = r2["episode_starts"] == 0
    assert go_on.any() and np.abs(r2["values"][go_on] - other.values(r2["observations"][go_on])).max() < 1e-9
    assert np.abs(r2["values"][go_on] - agent.values(r2["observations"][go_on])).min() > 0.2


def test_step_and_rollout_after_a_collect(table, agent):
    """one case of tests/test_gpu_policy.py::test_rollout_equals_the_host_driven_path behind a collect(): rollout() with the
    deterministic policy against step() with WeightPolicy.predict, both on environments that collected two steps first (one on the
    device, one host-driven through step())"""
    B, E = 5, 4
    kw = dict(episode_length=128, restart_indices=(200,), log_capacity=(2 + E) * M)
    a, b = _env(B, table, **kw), _env(B, table, **kw)
    r = a.collect(agent, 2, GAMMA, LAM, seed=SEED)
    b.dev.attach_policy(agent)
    obs = np.zeros((B, 22))
    for e in range(2):
        act = b.dev.policy_eval_ac(obs, SEED, b._t)["actions"]
        assert np.array_equal(act, r["actions"][e])
        obs = b.step(act)[0]
    assert a._t == b._t == 2 and np.array_equal(a._next_obs, obs) and np.array_equal(a._episode_starts, b._episode_starts)
    ro = a.rollout(agent, E)
    h = _host_driven(b, agent, E, obs=obs)
    assert ro["live"].all()
    _assert_same_steps(ro, h)
    la, lb = a.dev.logs(), b.dev.logs()
    for k in la:
        assert np.array_equal(la[k], lb[k]), k
    act = np.arange(B) % len(table)
    for x, y in zip(a.step(act)[:4], b.step(act)[:4]):
        assert np.array_equal(x, y)
    assert a._t == b._t == 2 + E + 1


def test_collect_refusals(table, agent, bare_loop):
    from tum_control_amd.closed_loop import WeightPolicy
    B = 2
    env = _env(B, table)
    dev = env.dev

    def state():
        return [dev.get("x_sim"), dev.get("x_mpc"), dev.env_get("episode_steps"), dev.env_get("samples"), dev.env_get("ended"), np.array(dev.steps)]

    def unchanged(s0):
        for x, y in zip(s0, state()):
            assert np.array_equal(x, y)
    env.step(np.zeros(B, dtype=int))
    s0 = state()
    bare = WeightPolicy(agent.weights, agent.biases)
    with pytest.raises(ValueError, match="no value net"):
        env.collect(bare, 2, GAMMA, LAM)
    dev.attach_policy(bare)
    with pytest.raises(Exception, match="no value net attached"):
        dev.env_collect(2, np.zeros((2, B), dtype=int), 0, 0, GAMMA, LAM)
    V, c = pr.synthetic_policy((21, 8, 1), 1)
    with pytest.raises(Exception, match="takes 21 inputs, the policy 22"):
        dev.attach_value(V, c)
    V, c = pr.synthetic_policy((22, 8, 2), 1)
    with pytest.raises(Exception, match="one row"):
        dev.attach_value(V, c)
    dev.detach_policy()
    with pytest.raises(Exception, match="no policy attached"):
        dev.attach_value(agent.value_weights, agent.value_biases)
    dev.attach_policy(agent)
    tab = np.zeros((2, B), dtype=int)
    tab[1, 1] = len(env.loop.track)
    with pytest.raises(Exception, match="instance 1 at step 1 is outside the track"):
        dev.env_collect(2, tab, 0, 0, GAMMA, LAM)
    unchanged(s0)
    frozen = _env(B, table, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        frozen.collect(agent, 2, GAMMA, LAM)
    assert frozen.dev.steps == 0
    # the value net goes with the policy, and the policy with the environment
    dev.attach_policy(bare)
    with pytest.raises(Exception, match="no value net attached"):
        dev.policy_eval_ac(np.zeros((1, 22)), 0, 0, values=True)
    dev.attach_policy(agent)
    dev.detach_env()
    with pytest.raises(Exception, match="no environment attached"):
        dev.env_collect(2, np.zeros((2, B), dtype=int), 0, 0, GAMMA, LAM)
    with pytest.raises(Exception, match="no policy attached"):
        dev.policy_eval_ac(np.zeros((1, 22)), 0, 0)
    # a loop without an environment: the two nets serve policy_eval_ac alone
    bare_loop.dev.attach_policy(agent)
    with pytest.raises(Exception, match="no environment attached"):
        bare_loop.dev.env_collect(2, np.zeros((2, 2), dtype=int), 0, 0, GAMMA, LAM)
