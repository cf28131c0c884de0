"""
The agent on the device: policy_kernel (tum_sim_policy_attach / _eval) against the long-double forward pass within the forward rounding
bound of tests/policy_reference.py, and tum_sim_env_rollout / WeightScheduleEnv.rollout / closed_loop.run_policy against the host-driven
path -- step() with WeightPolicy.predict on the observation just returned -- BIT FOR BIT: both paths run the same kernels on the same
words, and the two decide alike on every observation whose two largest logits are further apart than twice the bound (asserted).
Shipped track, N = 38, n_mpc_steps 3, the 26-row table of tests/golden/rl_env.npz, the agent of tests/golden/wmpc_policy.npz.

C_TANH: the device tanh against the exact value measured 0.81 ulp (profiles/policy_bounds.txt; test_device_tanh prints the figure);
the allowance is that rounded up to the next integer plus one.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import policy_reference as pr

pytestmark = pytest.mark.gpu

C_TANH = 2.0          # profiles/policy_bounds.txt: largest error 0.81 ulp -> 1 + 1
TRACK, N, TP, M = "monteblanco", 38, 3.04, 3
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


@pytest.fixture(scope="module")
def policy(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"))


def _env(B, table, starts=0, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    kw = dict(dict(rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=starts, n_mpc_steps=M, auto_reset=False), **kw)
    return WeightScheduleEnv(TRACK, B, table, **kw)


def _starts(B):
    return np.array([0, 350, 800, 137, 1000])[np.arange(B) % 5]


# ---------------------------------------------------------------------------------------------------------------- the activation
def test_device_tanh(tmp_path):
    """policy_tanh against tanh in long double (whose own error, 2^-11 ulp of a double, is added to the figure): |x| from 1e-300 to 40
    log-spaced, both signs, the signed zeros, and 200 neighbours on either side of every branch point of the implementation -- 2^-27,
    19.0625 and (n + 1/2) ln 2 / 2 .. of the exponential's range reduction between them"""
    import __graft_entry__ as ge
    out = str(tmp_path / "libpolicy_probe.so")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device", "policy_probe.hip")
    r = subprocess.run([ge.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", ge.CSRC, "-o", out, src],
                       capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(out), "the probe does not compile:\n" + r.stdout + r.stderr
    L = ctypes.CDLL(out)
    L.probe_policy_tanh.argtypes = [_dp, _dp, ctypes.c_int]
    rng = np.random.RandomState(5)
    x = [10.0 ** rng.uniform(-300, np.log10(40.0), 20000), 10.0 ** rng.uniform(-9, np.log10(40.0), 20000), rng.uniform(0, 40.0, 20000)]
    branch = [2.0 ** -27, 19.0625] + [(n + 0.5) * np.log(2.0) * s for n in range(0, 56) for s in (0.5, 1.0)]
    for p in branch:
        v = [p]
        for _ in range(200):
            v.append(np.nextafter(v[-1], np.inf))
        w = [p]
        for _ in range(200):
            w.append(np.nextafter(w[-1], -np.inf))
        x.append(np.array(v + w))
    x = np.concatenate(x)
    x = np.concatenate([x, -x, [0.0, -0.0, 1e-300, -1e-300, 40.0, -40.0]])
    y = np.empty_like(x)
    assert L.probe_policy_tanh(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(x)) == 0
    exact = np.tanh(x.astype(pr.LD))
    ulp = np.spacing(np.abs(exact).astype(np.float64))
    nz = x != 0.0
    err = (np.abs(y[nz].astype(pr.LD) - exact[nz]) / ulp[nz]).astype(np.float64) + 2.0 ** -11
    i = int(np.argmax(err))
    print(f"PB policy_tanh points {len(x)} max_ulp {err.max():.4f} at x = {x[nz][i]!r}")
    # odd to the bit, the sign of a zero included; never above 1
    assert np.array_equal(y[~nz], x[~nz]) and np.array_equal(np.signbit(y[~nz]), np.signbit(x[~nz]))
    h = len(x) // 2 - 3
    assert np.array_equal(y[:h], -y[h:2 * h]) and (np.abs(y) <= 1.0).all()
    assert err.max() <= C_TANH - 1.0


# ---------------------------------------------------------------------------------------------------------------- policy_eval
def _pool(n_in, rng):
    """33 observations: the zeros of a reset, entries far outside [0, 1] that saturate tanh, the seeded kinds, doubles that are no
    float32 values (all of rand / randn, and a few next to a float32 tie)"""
    x = np.zeros((33, n_in))
    x[1] = 50.0
    x[2] = 50.0 * (-1.0) ** np.arange(n_in)
    x[3:14] = rng.rand(11, n_in)
    x[14:24] = 2.0 * rng.randn(10, n_in)
    x[24:29] = rng.rand(5, n_in).astype(np.float32).astype(np.float64) * (1.0 + 2.0 ** -25)          # just above the middle of two float32
    x[29:33] = np.array([-50.0, 50.0, 0.0, 1.0, 1e-30, -3.0])[rng.randint(0, 6, size=(4, n_in))]
    return x


NETS = {"fixture": None,
        "odd": (23, 20, 36, 12, 5),                        # widths that are multiples of neither 16 nor 4
        "tiny": (3, 1, 2),                                 # one hidden layer, one unit
        "widest": (128, 256, 256, 256, 256, 64),           # the largest supported: 4 hidden layers, 64 KB of LDS
        "one": (1, 1, 1)}


@pytest.fixture(scope="module")
def bare_loop():
    """a loop WITHOUT an environment: a policy of any supported widths attaches for policy_eval alone"""
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(TRACK, batch=2, N=N, Tp=TP, on_device=True)


@pytest.mark.parametrize("net", list(NETS))
def test_policy_eval_within_the_bound(net, policy, bare_loop):
    """logits within B_logit, probabilities within their bound and summing to 1, actions equal on every row; n = 1, 15, 16, 17, 33"""
    from tum_control_amd.closed_loop import WeightPolicy
    W, b = (policy.weights, policy.biases) if NETS[net] is None else pr.synthetic_policy(NETS[net], 11)
    dev = bare_loop.dev
    dev.attach_policy(WeightPolicy(W, b))
    x = _pool(W[0].shape[1], np.random.RandomState(2))
    z, bound = pr.forward(W, b, x, c_tanh=C_TANH)
    gap = pr.top_gap(z)
    print(net, "smallest gap", gap.min(), "largest bound", bound.max())
    assert (gap >= 2.0 * bound.max(axis=1)).all()          # the precondition: no row is excused
    pref, pb = pr.probabilities(z), pr.probability_bound(z, bound)
    n_act = W[-1].shape[0]
    for n in (1, 15, 16, 17, 33):
        r = dev.policy_eval(x[:n])
        err = np.abs(r["logits"].astype(pr.LD) - z[:n]).astype(np.float64)
        rel = (np.abs(r["probabilities"].astype(pr.LD) - pref[:n]) / pref[:n]).astype(np.float64)
        print(net, n, "logits err / bound", (err / bound[:n]).max(), "probabilities err / bound", (rel / pb[:n, None]).max())
        assert r["logits"].shape == (n, n_act) and r["actions"].shape == (n,)
        assert (err <= bound[:n]).all()
        assert (rel <= pb[:n, None]).all()
        assert (np.abs(r["probabilities"].sum(axis=1) - 1.0) <= (n_act + 4) * pr.EPS).all()
        assert np.array_equal(r["actions"], pr.actions(z[:n]))


def test_policy_eval_seeded_rows_and_ties(policy, bare_loop):
    """the first 256 seeded rows of the fixture on the device: within the bound of the long-double pass, the recorded decisions; and an
    exact tie goes to the lowest index"""
    from tum_control_amd.closed_loop import WeightPolicy
    dev = bare_loop.dev
    dev.attach_policy(policy)
    x = pr.seeded_observations()[0][:256]
    z, bound = pr.forward(policy.weights, policy.biases, x, c_tanh=C_TANH)
    assert (pr.top_gap(z) >= 2.0 * bound.max(axis=1)).all()
    r = dev.policy_eval(x)
    assert (np.abs(r["logits"].astype(pr.LD) - z).astype(np.float64) <= bound).all()
    assert np.array_equal(r["actions"], pr.actions(z)) and np.array_equal(r["actions"], policy.predict(x))
    tie = WeightPolicy([np.zeros((4, 3), np.float32), np.zeros((5, 4), np.float32)], [np.zeros(4, np.float32), np.array([0.0, 1.0, 0.5, 1.0, 1.0], np.float32)])
    dev.attach_policy(tie)
    r = dev.policy_eval(np.random.RandomState(3).randn(17, 3))
    assert np.array_equal(r["actions"], np.ones(17, dtype=int)) and np.array_equal(r["logits"], np.tile(tie.biases[1].astype(float), (17, 1)))
    dev.detach_policy()
    with pytest.raises(Exception, match="no policy attached"):
        dev.policy_eval(np.zeros((1, 3)))


def test_attach_refuses_unsupported_shapes(bare_loop):
    from tum_control_amd.closed_loop import WeightPolicy
    for widths, msg in (((129, 4, 3), "1 to 128 inputs"), ((4, 257, 3), "1 to 256 wide"), ((4, 8, 65), "1 to 64 actions"),
                        ((4, 3, 3, 3, 3, 3, 2), "1 to 4 hidden layers")):
        with pytest.raises(Exception, match=msg):
            bare_loop.dev.attach_policy(WeightPolicy(*pr.synthetic_policy(widths, 1)))


# ---------------------------------------------------------------------------------------------------------------- rollouts
FIELDS = ("reward", "observation", "terminated", "truncated", "step_length", "qp_failures")


def _decided(policy, obs):
    """the precondition of every equality below: host and device decide alike on these observations"""
    z, bound = pr.forward(policy.weights, policy.biases, obs, c_tanh=C_TANH)
    assert (pr.top_gap(z) >= 2.0 * bound.max(axis=1)).all()


def _host_driven(env, policy, E, obs=None):
    """step() with the host picking each action on the observation just returned; dict of (E, B, ...) arrays"""
    obs = np.zeros((env.n_envs, env.n_observations)) if obs is None else obs
    out = {k: [] for k in FIELDS + ("action",)}
    for _ in range(E):
        _decided(policy, obs)
        a = policy.predict(obs)
        obs, rew, te, tr, info = env.step(a)
        for k, v in (("action", a), ("reward", rew), ("observation", info["terminal_observation"]), ("terminated", te), ("truncated", tr),
                     ("step_length", info["step_length"]), ("qp_failures", info["qp_failures"])):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def _assert_same_steps(dev, host, rows=slice(None)):
    for k in FIELDS + ("action",):
        d = dev[k].data if isinstance(dev[k], np.ma.MaskedArray) else dev[k]
        assert d[rows].shape == host[k][rows].shape and np.array_equal(d[rows], host[k][rows]), k


def _assert_same_logs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("B", [5, 18])
def test_rollout_equals_the_host_driven_path(B, table, policy):
    """E = 4 at B = 5 (one partial tile) and B = 18 (two tiles, the second partial): actions, every record field, the five logs"""
    E = 4
    a = _env(B, table, _starts(B), log_capacity=E * M)
    b = _env(B, table, _starts(B), log_capacity=E * M)
    r = a.rollout(policy, E)
    h = _host_driven(b, policy, E)
    assert r["live"].shape == (E, B) and r["live"].all() and not r["action"].mask.any()
    _assert_same_steps(r, h)
    _assert_same_logs(a.dev.logs(), b.dev.logs())
    assert a.dev.steps == b.dev.steps == E * M
    assert len(np.unique(r["action"].data)) > 1          # (the agent does schedule: not one row throughout)
    for f in ("episode_steps", "samples", "ended"):
        assert np.array_equal(a.dev.env_get(f), b.dev.env_get(f)), f


def test_attached_policy_changes_nothing_step_computes(table, policy):
    """an environment with a policy attached but driven through step() against one without: logs bit-identical"""
    B, E = 5, 3
    a = _env(B, table, _starts(B), log_capacity=E * M)
    b = _env(B, table, _starts(B), log_capacity=E * M)
    a.dev.attach_policy(policy)
    acts = np.random.RandomState(4).randint(0, len(table), size=(E, B))
    for row in acts:
        ra, rb = a.step(row), b.step(row)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    _assert_same_logs(a.dev.logs(), b.dev.logs())


def test_rollout_auto_reset(table, policy):
    """episode_length 2, on_end 1 and a given start table against step(reset_mask, start_idx) with the same starts: an instance that
    ended is reset at the start of the next step, and the policy sees zeros for it"""
    B, E = 5, 5
    start_table = np.random.RandomState(6).choice([0, 200, 640, 900], size=(E, B))
    a = _env(B, table, _starts(B), episode_length=2, log_capacity=E * M)
    b = _env(B, table, _starts(B), episode_length=2, log_capacity=E * M)
    a.dev.attach_policy(policy)
    r = a.dev.env_rollout(E, on_end=1, start_table=start_table)
    obs, ended = np.zeros((B, 22)), np.zeros(B, dtype=bool)
    for e in range(E):
        _decided(policy, obs)
        act = policy.predict(obs)
        h = b.dev.env_step(act, ended.astype(np.int32), np.where(ended, start_table[e], 0))
        assert np.array_equal(r["action"][e], act), e
        for k in FIELDS:
            assert np.array_equal(r[k][e], h[k]), (k, e)
        ended = h["terminated"] | h["truncated"]
        obs = np.where(ended[:, None], 0.0, h["observation"])
    assert r["live"].all()
    assert r["terminated"][1].all() and r["terminated"][3].all() and not r["terminated"][[0, 2, 4]].any()          # reset twice
    _assert_same_logs(a.dev.logs(), b.dev.logs())
    for f in ("episode_steps", "samples", "ended"):
        assert np.array_equal(a.dev.env_get(f), b.dev.env_get(f)), f
    # the wrapper: an (E, B) table drawn from restart_indices before the rollout
    c = _env(B, table, _starts(B), episode_length=2, auto_reset=True, restart_indices=(0, 200, 640), seed=9)
    rc = c.rollout(policy, 3)
    assert rc["terminated"].data[1].all() and not rc["terminated"].data[[0, 2]].any() and rc["live"].all()
    want = np.array([0, 200, 640])[np.random.RandomState(9).randint(0, 3, size=3 * B)].reshape(3, B)
    assert np.array_equal(c.last_start, want[2])


def test_rollout_freeze_and_early_stop(table, policy):
    """on_end 0, check_every 1: two groups whose episodes (length 3) end one step apart -- the second group was reset one step later.
    The rollout stops at the step after the last instance ended; live is right; "ended" and a following step behave as after
    host-driven steps"""
    B = 5
    late = np.array([False, True, False, True, True])

    def prelude():
        env = _env(B, table, _starts(B), episode_length=3)
        obs, *_ = env.step(np.zeros(B, dtype=int))
        env.reset(mask=late)
        obs[late] = 0.0
        return env, obs
    a, obs_a = prelude()
    b, obs_b = prelude()
    assert np.array_equal(obs_a, obs_b)
    r = a.rollout(policy, 6, stop_when_done=True)
    h = _host_driven(b, policy, 3, obs=obs_b)
    assert r["live"].shape == (3, B)          # the early group ends in step 1, the late one in step 2: stopped after 3 of 6
    assert np.array_equal(r["live"], np.array([[True] * B, [True] * B, list(late)]))
    _assert_same_steps(r, h)
    assert np.array_equal(r["terminated"].data, np.array([[False] * B, list(~late), list(late)]))
    assert np.array_equal(r["action"].mask, ~r["live"]) and np.array_equal(r["observation"].mask[:, :, 0], ~r["live"])
    for f in ("episode_steps", "samples", "ended", "flags"):
        assert np.array_equal(a.dev.env_get(f), b.dev.env_get(f)), f
    assert np.array_equal(a.dev.env_get("ended"), late.astype(int))
    # an ended instance that is not marked is refused on both, and nothing has run
    with pytest.raises(Exception, match="has ended"):
        a.dev.env_step(np.zeros(B, dtype=int))
    act = np.arange(B) % len(table)
    sa, sb = a.step(act), b.step(act)
    for x, y in zip(sa[:4], sb[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(a.dev.get("x_sim"), b.dev.get("x_sim")) and np.array_equal(a.dev.get("x_mpc"), b.dev.get("x_mpc"))


def test_rollout_continues_from_first_obs(table, policy):
    """a rollout continued from the previous rollout's last observation equals one longer rollout"""
    B = 5
    a = _env(B, table, _starts(B), log_capacity=4 * M)
    b = _env(B, table, _starts(B), log_capacity=4 * M)
    r1 = a.rollout(policy, 2)
    r2 = a.rollout(policy, 2)
    r = b.rollout(policy, 4)
    for k in FIELDS + ("action",):
        assert np.array_equal(np.concatenate([r1[k].data, r2[k].data]), r[k].data), k
    _assert_same_logs(a.dev.logs(), b.dev.logs())
    # and through the C interface: first_obs given explicitly
    c = _env(B, table, _starts(B))
    c.dev.attach_policy(policy)
    q1 = c.dev.env_rollout(2)
    q2 = c.dev.env_rollout(2, first_obs=q1["observation"][-1])
    assert np.array_equal(q2["action"], r["action"].data[2:]) and np.array_equal(q2["observation"], r["observation"].data[2:])


def test_run_policy_full_lap(table, policy):
    """full_lap from a start 60 waypoints before the end of the track: terminates at len(track) - 2, with the actions of the
    host-driven loop"""
    from tum_control_amd.closed_loop import closest_index, load_track, run_policy
    track = load_track(TRACK)
    start = len(track) - 60
    r = run_policy(TRACK, policy, table, [start, start - 40], max_steps=120, n_mpc_steps=M, rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP)
    n = r["n_decisions"]
    ro = r["rollout"]
    E = len(r["live"])
    assert E == n.max() < 120 and n[0] < n[1]          # stopped when the last instance ended
    for i in range(2):
        assert ro["terminated"].data[n[i] - 1, i] and not ro["truncated"].data[:n[i], i].any() and not ro["terminated"].data[:n[i] - 1, i].any()
        # the control step that ended the episode stood at the last-but-one waypoint
        s = (n[i] - 1) * M + ro["step_length"].data[n[i] - 1, i] - 1
        assert closest_index(track, r["logs"]["CiLX"][s, i, :2]) == len(track) - 2
        assert r["actions"].mask[n[i]:, i].all() and not r["actions"].mask[:n[i], i].any()
    p = r["probabilities"]
    assert p.shape == (E, 2, 26) and np.allclose(p.data.sum(axis=2), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(np.argmax(p.data, axis=2)[r["live"]], r["actions"].data[r["live"]])
    # the host-driven loop of evaluation.py:84-96, the first vehicle alone
    env = _env(1, table, np.array([start]), full_lap=True)
    obs, done, acts = np.zeros((1, 22)), False, []
    while not done and len(acts) < 120:
        _decided(policy, obs)
        a = policy.predict(obs)
        obs, _, te, tr, _ = env.step(a)
        acts.append(int(a[0]))
        done = bool(te[0] or tr[0])
    assert acts == list(r["actions"].data[:n[0], 0])


def test_rollout_refusals(table, policy):
    from tum_control_amd.closed_loop import ClosedLoopBatch, WeightPolicy
    B = 2
    env = _env(B, table, _starts(B))
    dev = env.dev

    def state():
        return [dev.get("x_sim"), dev.get("x_mpc"), dev.env_get("episode_steps"), dev.env_get("samples"), dev.env_get("ended"), np.array(dev.steps)]

    def unchanged(s0):
        for x, y in zip(s0, state()):
            assert np.array_equal(x, y)
    env.step(np.zeros(B, dtype=int))
    s0 = state()
    with pytest.raises(Exception, match="no policy attached"):
        dev.env_rollout(2)
    unchanged(s0)
    for widths, msg in (((20, 8, 26), "observation has 22 entries"), ((22, 8, 25), "table has 26 rows")):
        with pytest.raises(Exception, match=msg):
            dev.attach_policy(WeightPolicy(*pr.synthetic_policy(widths, 1)))
    with pytest.raises(Exception, match="no policy attached"):
        dev.env_rollout(2)
    dev.attach_policy(policy)
    with pytest.raises(Exception, match="needs a start table"):
        dev.env_rollout(2, on_end=1)
    for bad in (len(env.loop.track), -1):
        tab = np.zeros((2, B), dtype=int)
        tab[1, 1] = bad
        with pytest.raises(Exception, match="instance 1 at step 1 is outside the track"):
            dev.env_rollout(2, on_end=1, start_table=tab)
    with pytest.raises(Exception, match="on_end"):
        dev.env_rollout(2, on_end=2)
    unchanged(s0)
    # the policy goes with the environment
    dev.detach_env()
    with pytest.raises(Exception, match="no environment attached"):
        dev.env_rollout(2)
    with pytest.raises(Exception, match="no policy attached"):
        dev.policy_eval(np.zeros((1, 22)))
    # an SNMPC or R2 loop takes no environment (tests/test_gpu_rl_env.py::test_refusals), so no rollout either
    for controller in ("snmpc", "r2"):
        other = ClosedLoopBatch(TRACK, batch=2, N=N, Tp=TP, on_device=True, controller=controller)
        other.dev.attach_policy(policy)
        with pytest.raises(Exception, match="no environment attached"):
            other.dev.env_rollout(2)
