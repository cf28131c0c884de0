"""
The PPO update on the device (tum_sim_ppo_* / closed_loop.PPOTrainer / closed_loop.learn) against the references of
tests/ppo_reference.py: gradients and diagnostics within the gate of the issue, the forward pass bit for bit against policy_eval_ac,
Adam against its long-double statement, the chained update against the stepwise one bit for bit, the acting nets against a fresh
attach of the downloaded parameters, learn() against the host-driven sequence, and the refusals.
Shipped track, N = 38, n_mpc_steps 3, the 26-row table of tests/golden/rl_env.npz, the agent of wmpc_policy.npz + wmpc_value.npz.

Gradient gate (units of u max |g_longdouble|, u = 2^-53): the device may have at most 4 x the larger of the host statement's and
torch's error on the same tensor, floor 32 -- all are FP64 sums of the same terms in different orders. The loss parts, approx_kl and
grad_norm are held to the same gate relative to their own value. The TOTAL loss is the combination of the parts and its terms cancel:
at "odd", n = 2 (-0.0623 - 0.0192 + 0.0609 = -0.0206) the device's total is 78 u of its own value off while its parts are 19.6, 2.2
and 6.4 u of theirs off (host statement and torch: 8 u) -- the same absolute error, 1.8e-16. It is therefore held to the absolute
bound the parts' gates imply (ppo_reference.loss_bound), not to the relative gate. What the device needs of each gate on one
MI355X: profiles/ppo_bounds.txt (the lines this module prints with the prefix ppo_bounds).
"""
import ctypes
import os

import numpy as np
import pytest

import ppo_reference as ref

pytestmark = pytest.mark.gpu

TRACK, N, TP, M = "monteblanco", 38, 3.04, 3
SIGMAS, LIMS = (0.1, 0.5), ((0.0, 0.0), (0.4, 1.0))
GAMMA, LAM = 0.99, 0.95
RESTARTS = (0, 200, 640, 900)
COLLECT_KEYS = ("observations", "actions", "log_probs", "values", "rewards", "rewards_raw", "episode_starts", "terminated", "truncated",
                "step_length", "qp_failures", "advantages", "returns", "last_values", "last_dones")
ROWS = ("obs", "actions", "old_log_probs", "advantages", "returns")


@pytest.fixture(scope="module")
def table(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_env.npz"))["F"]


@pytest.fixture(scope="module")
def agent(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"), os.path.join(golden_dir, "wmpc_value.npz"))


@pytest.fixture(scope="module")
def dev():
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch(TRACK, batch=2, N=N, Tp=TP, on_device=True).dev


def _env(B, table, **kw):
    from tum_control_amd.closed_loop import WeightScheduleEnv
    kw = dict(dict(rew_sigmas=SIGMAS, rew_lims=LIMS, N=N, Tp=TP, idx_start=np.array([0, 350, 800])[np.arange(B) % 3], n_mpc_steps=M,
                   auto_reset=True, episode_length=2, restart_indices=RESTARTS, seed=9), **kw)
    return WeightScheduleEnv(TRACK, B, table, **kw)


def _trainer(dev, name, **kw):
    from tum_control_amd.closed_loop import PPOTrainer, WeightPolicy
    return PPOTrainer(dev, WeightPolicy(*ref.nets(name)), **dict(ref.SETTINGS, **kw))


def _rows(inp, idx=slice(None)):
    return [inp[k][idx] for k in ROWS]


def _same_lists(a, b):
    return all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def _same_state(a, b):
    return a["t"] == b["t"] and _same_lists(a["m"], b["m"]) and _same_lists(a["v"], b["v"])


# ------------------------------------------------------------------------------------------- 1. gradients and diagnostics
def _check_gate(dev, name, n):
    from tum_control_amd.closed_loop import WeightPolicy, ppo_loss_and_grads
    inp, ld, th = ref.references(name, n)
    assert ld["kink"] > 1e-9          # no row near the kink of min(): nothing is set aside, clip_fraction is exact
    host = ppo_loss_and_grads(WeightPolicy(*ref.nets(name)), *_rows(inp), **ref.SETTINGS)
    tr = _trainer(dev, name)
    before = tr.policy(), tr.state()
    got = tr.step(*_rows(inp), lr=1e-3, apply=False, want_grads=True)
    e_dev = ref.errors(got["grads"], ld["grads"])
    gate = np.maximum(4.0 * np.maximum(ref.errors(host["grads"], ld["grads"]), ref.errors(th["grads"], ld["grads"])), ref.FLOOR)
    for t, e, g in zip(ref.tensor_names(ld["grads"]), e_dev, gate):
        print(f"ppo_bounds {name} n={n} {t}: device {e:.2f} gate {g:.2f} ratio {e / g:.3f}")
    missed = [t for t, e, g in zip(ref.tensor_names(ld["grads"]), e_dev, gate) if not e <= g]
    gates = {}
    for k in ref.GATED:
        e = ref.scalar_error(got[k], ld[k])
        g = gates[k] = max(4.0 * max(ref.scalar_error(host[k], ld[k]), ref.scalar_error(th[k], ld[k])), ref.FLOOR)
        print(f"ppo_bounds {name} n={n} {k}: device {e:.2f} gate {g:.2f} ratio {e / g:.3f}  (value {float(ld[k]):+.3e})")
        if not e <= g:
            missed.append(k)
    # the total loss: the combination of the gated parts, whose terms cancel -- an absolute bound from the parts' gates (ppo_reference)
    e, g = float(abs(ref.LD(got["loss"]) - ld["loss"])), ref.loss_bound(ld, gates)
    print(f"ppo_bounds {name} n={n} loss: device |error| {e:.3e} bound {g:.3e} ratio {e / g:.3f}  (value {float(ld['loss']):+.3e}, {ref.scalar_error(got['loss'], ld['loss']):.2f} u of it)")
    if not e <= g:
        missed.append("loss")
    assert not missed, (name, n, missed)
    assert got["clip_fraction"] == ld["clip_fraction"] and got["n"] == n
    # apply=False leaves parameters, moments and the counter as they were
    after = tr.policy(), tr.state()
    assert _same_lists([before[0].weights, before[0].biases, before[0].value_weights, before[0].value_biases],
                       [after[0].weights, after[0].biases, after[0].value_weights, after[0].value_biases])
    assert _same_state(before[1], after[1]) and after[1]["t"] == 0


@pytest.mark.parametrize("name", ["odd", "tiny", "widest"])
def test_gradients_and_diagnostics_within_the_gate(name, dev):
    for n in (2, 15, 16, 17, 37, 200):
        _check_gate(dev, name, n)


def test_gradients_at_the_shipped_shape(dev):
    _check_gate(dev, *ref.GOLDEN_CASE)


def test_one_row_takes_the_advantage_as_it_is(dev):
    inp = ref.case("odd", 1)
    ld = ref.loss_and_grads_ld(*ref.nets("odd"), **inp, **ref.SETTINGS, normalize_advantage=False)
    got = _trainer(dev, "odd").step(*_rows(inp), lr=1e-3, apply=False, want_grads=True)
    assert np.isfinite(got["loss"]) and abs(ref.LD(got["loss"]) - ld["loss"]) <= ref.loss_bound(ld, dict.fromkeys(ref.GATED, ref.FLOOR))
    assert (ref.errors(got["grads"], ld["grads"]) <= ref.FLOOR).all()


# ------------------------------------------------------------------------------------------- 2. forward bits
@pytest.mark.parametrize("name", ["odd", "tiny", "widest"])
def test_forward_pass_is_policy_eval_acs(name, dev):
    """the values and the log-probabilities the tile kernel computes are policy_ac_kernel's on the same rows, bit for bit"""
    tr = _trainer(dev, name)
    inp = ref.case(name, 37)
    ac = dev.policy_eval_ac(inp["obs"], 7, 3)
    got = tr.step(inp["obs"], ac["actions"], ac["log_probs"], inp["advantages"], inp["returns"], lr=1e-3, apply=False, want_rows=True)
    assert np.array_equal(got["values"], ac["values"]) and np.array_equal(got["log_probs"], ac["log_probs"])
    # so the ratio of a first epoch is exactly 1
    assert got["approx_kl"] == 0.0 and got["clip_fraction"] == 0.0


# ------------------------------------------------------------------------------------------- 3. Adam, isolated
@pytest.mark.parametrize("max_norm,clipped", [(1e-3, True), (1e3, False)])
def test_adam_against_the_long_double_statement(max_norm, clipped, dev):
    tr = _trainer(dev, "odd", max_grad_norm=max_norm)
    inp = ref.case("odd", 37)
    entries = differ = 0
    for t, lr in ((1, 3e-4), (2, 1e-3), (3, 5e-5)):
        pol, st = tr.policy(), tr.state()
        assert st["t"] == t - 1
        params = ref.flat([pol.weights, pol.biases, pol.value_weights, pol.value_biases])
        got = tr.step(*_rows(inp), lr=lr, apply=True, want_grads=True)
        assert (got["grad_norm"] > max_norm) == clipped
        P, Mo, Vo, total = ref.adam_ld(params, ref.flat(got["grads"]), ref.flat(st["m"]), ref.flat(st["v"]), t, lr, max_norm)
        # (the squares, a chain of at most 8, a tree of 8 levels, the chain over the slices: under 20 roundings, halved by the root)
        assert abs(ref.LD(got["grad_norm"]) - total) <= 16 * ref.U * total
        new, st1 = tr.policy(), tr.state()
        assert st1["t"] == t
        if t > 1:
            assert all(np.abs(m).max() > 0 for m in ref.flat(st["m"]))          # (non-zero moments go into steps 2 and 3)
        for x, want, m1, v1, mw, vw in zip(ref.flat([new.weights, new.biases, new.value_weights, new.value_biases]), P,
                                           ref.flat(st1["m"]), ref.flat(st1["v"]), Mo, Vo):
            assert x.dtype == np.float32
            off = x != want.astype(np.float32)
            near = ref.near_float32_boundary(want)
            assert not (off & ~near).any()
            assert (np.abs(x[off].astype(ref.LD) - want[off]) <= np.abs(np.spacing(x[off]).astype(ref.LD))).all()          # one float32 ulp
            entries += x.size; differ += int(off.sum())
            assert np.abs(m1.astype(ref.LD) - mw).max() <= 8 * ref.U * np.abs(mw).max()
            assert np.abs(v1.astype(ref.LD) - vw).max() <= 8 * ref.U * np.abs(vw).max()
    print("entries", entries, "one ulp off at a rounding boundary", differ)
    assert differ <= entries // 1000


# ------------------------------------------------------------------------------------------- 4. chained equals stepwise
def test_chained_update_equals_stepwise_bit_for_bit(dev):
    from tum_control_amd.closed_loop import minibatch_slices
    Nr, bs, n_epochs, lr = 100, 48, 2, 7e-4
    inp = ref.case("odd", Nr)
    buf = dict(observations=inp["obs"], actions=inp["actions"], log_probs=inp["old_log_probs"], advantages=inp["advantages"], returns=inp["returns"])
    rng = np.random.RandomState(21)
    perm = np.stack([rng.permutation(Nr) for _ in range(n_epochs)])

    def chained():
        tr = _trainer(dev, "odd")
        return tr.update(buf, perm, n_epochs, bs, lr), tr.policy(), tr.state()
    s1, p1, st1 = chained()
    assert s1["n"].tolist() == [[48, 48, 4]] * 2 and st1["t"] == 6
    tr = _trainer(dev, "odd")
    for e in range(n_epochs):
        for k, sl in enumerate(minibatch_slices(Nr, bs)):
            got = tr.step(*_rows(inp, perm[e][sl]), lr=lr, apply=True)
            for key in dev.PPO_STATS:
                assert np.array_equal(got[key], s1[key][e, k]), (key, e, k)
    p2, st2 = tr.policy(), tr.state()
    nets = lambda p: [p.weights, p.biases, p.value_weights, p.value_biases]
    assert _same_lists(nets(p1), nets(p2)) and _same_state(st1, st2)
    assert not _same_lists(nets(p1), [list(x) for x in ref.nets("odd")])          # (and the update did move the parameters)
    # the same call from the same state gives the same bits
    s3, p3, st3 = chained()
    assert all(np.array_equal(s1[k], s3[k]) for k in s1) and _same_lists(nets(p1), nets(p3)) and _same_state(st1, st3)
    # perm = None draws RandomState(seed).permutation(N) per epoch
    sa = _trainer(dev, "odd").update(buf, None, n_epochs, bs, lr, seed=21)
    assert all(np.array_equal(s1[k], sa[k]) for k in s1)


# ------------------------------------------------------------------------------------------- 5. the acting nets follow
def test_resident_nets_are_the_downloaded_parameters(dev):
    tr = _trainer(dev, "widest")
    inp = ref.case("widest", 37)
    tr.step(*_rows(inp), lr=1e-2, apply=True)
    tr.step(*_rows(inp), lr=1e-2, apply=True)
    x = np.random.RandomState(2).rand(50, 128)
    ac, ev = dev.policy_eval_ac(x, 5, 1), dev.policy_eval(x)
    # the transposed matrices follow too: the gradients of the resident nets are those of the downloaded parameters attached afresh
    g1 = tr.step(*_rows(inp), lr=0.0, apply=False, want_grads=True)
    pol = tr.policy()
    old = ref.nets("widest")
    assert all(np.abs(w - o).max() > 1e-4 for w, o in zip(pol.weights + pol.value_weights, old[0] + old[2]))
    from tum_control_amd.closed_loop import PPOTrainer
    tr2 = PPOTrainer(dev, pol, **ref.SETTINGS)          # (attach_policy: a fresh upload and packing)
    ac2, ev2 = dev.policy_eval_ac(x, 5, 1), dev.policy_eval(x)
    for k in ac:
        assert np.array_equal(ac[k], ac2[k]), k
    for k in ev:
        assert np.array_equal(ev[k], ev2[k]), k
    g2 = tr2.step(*_rows(inp), lr=0.0, apply=False, want_grads=True)
    assert _same_lists(g1["grads"], g2["grads"]) and g1["loss"] == g2["loss"]


def _train_once(env, tr, seed=3):
    r = env.collect(tr, 2, GAMMA, LAM)
    tr.update(None, None, 2, 4, 1e-2, seed=seed)
    return r


def test_collect_with_the_trainer_is_collect_with_its_policy(table, agent):
    from tum_control_amd.closed_loop import PPOTrainer
    a, b = _env(3, table), _env(3, table)
    ta, tb = PPOTrainer(a, agent, **ref.SETTINGS), PPOTrainer(b, agent, **ref.SETTINGS)
    r0a, r0b = _train_once(a, ta), _train_once(b, tb)
    for k in COLLECT_KEYS:
        assert np.array_equal(r0a[k], r0b[k]), k
    pol = tb.policy()
    assert np.abs(pol.weights[0] - agent.weights[0]).max() > 1e-4
    ra = a.collect(ta, 2, GAMMA, LAM)
    rb = b.collect(pol, 2, GAMMA, LAM)          # (attaches the downloaded nets: the trainer of b is gone)
    for k in COLLECT_KEYS:
        assert np.array_equal(ra[k], rb[k]), k
    with pytest.raises(Exception, match="no trainer attached"):
        tb.step(np.zeros((1, 22)), np.zeros(1, dtype=int), np.zeros(1), np.zeros(1), np.zeros(1), lr=1e-3)


# ------------------------------------------------------------------------------------------- 6. learn end to end
def test_learn_equals_the_host_driven_sequence(table, agent):
    from tum_control_amd.closed_loop import PPOTrainer, learn, learning_rate_schedule, minibatch_slices
    B, E, bs, n_epochs, n_updates = 3, 4, 6, 2, 2
    sched = learning_rate_schedule(1e-2, 1e-3, 1.0)
    a, b = _env(B, table), _env(B, table)
    ta, tb = PPOTrainer(a, agent, **ref.SETTINGS), PPOTrainer(b, agent, **ref.SETTINGS)
    out = learn(a, ta, n_updates, E, bs, n_epochs, GAMMA, LAM, sched, seed=40)
    assert len(out) == n_updates and out[0]["n"].tolist() == [[6, 6]] * n_epochs
    for u in range(n_updates):
        r = b.collect(tb, E, GAMMA, LAM)
        rows = dict(obs=r["observations"].reshape(E * B, -1), actions=r["actions"].reshape(-1), old_log_probs=r["log_probs"].reshape(-1),
                    advantages=r["advantages"].reshape(-1), returns=r["returns"].reshape(-1))
        rng = np.random.RandomState(40 + u)
        lr = sched(1.0 - (u + 1) / n_updates)
        for e in range(n_epochs):
            p = rng.permutation(E * B)
            for k, sl in enumerate(minibatch_slices(E * B, bs)):
                got = tb.step(*_rows(rows, p[sl]), lr=lr, apply=True)
                for key in b.dev.PPO_STATS:
                    assert np.array_equal(got[key], out[u][key][e, k]), (u, key, e, k)
        if u == 0:
            assert (out[0]["approx_kl"][0, 0] == 0.0) and (out[0]["approx_kl"][1] != 0.0).all()          # the first minibatch sees ratio 1
    pa, pb = ta.policy(), tb.policy()
    nets = lambda p: [p.weights, p.biases, p.value_weights, p.value_biases]
    assert _same_lists(nets(pa), nets(pb)) and _same_state(ta.state(), tb.state()) and ta.state()["t"] == n_updates * n_epochs * 2
    assert np.array_equal(a._next_obs, b._next_obs) and a._t == b._t == n_updates * E


# ------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(dev, table, agent):
    from tum_control_amd.closed_loop import PPOTrainer, WeightPolicy
    W, b, V, c = ref.nets("odd")
    with pytest.raises(ValueError, match="no value net"):
        PPOTrainer(dev, WeightPolicy(W, b))
    dev.attach_policy(WeightPolicy(W, b))
    with pytest.raises(Exception, match="no value net attached"):
        dev.ppo_attach()
    inp = ref.case("odd", 8)
    dev.attach_policy(WeightPolicy(W, b, V, c))
    with pytest.raises(Exception, match="no trainer attached"):
        dev.ppo_step(*_rows(inp), lr=1e-3)
    with pytest.raises(Exception, match="no trainer attached"):
        dev.ppo_update(8, np.arange(8)[None], 4, 1e-3, buffer=_rows(inp))
    tr = _trainer(dev, "odd")
    perm = np.arange(8)[None].copy()
    perm[0, 3] = 8
    with pytest.raises(Exception, match="outside the buffer"):
        dev.ppo_update(8, perm, 4, 1e-3, buffer=_rows(inp))
    ip = ctypes.POINTER(ctypes.c_int)
    bad = np.ascontiguousarray(perm, dtype=np.int32)
    stats = np.zeros(2 * 8)
    from tum_control_amd.solver import _dp
    rows = dev._ppo_rows("t", 8, *_rows(inp))
    args = [_dp(rows[0]), rows[1].ctypes.data_as(ip)] + [_dp(x) for x in rows[2:]]
    assert dev._L.tum_sim_ppo_update(dev._s, 8, *args, bad.ctypes.data_as(ip), 1, 4, 1e-3, _dp(stats)) != 0          # the C interface itself
    good = np.arange(8, dtype=np.int32)
    assert dev._L.tum_sim_ppo_update(dev._s, 8, *args, good.ctypes.data_as(ip), 1, 0, 1e-3, _dp(stats)) != 0           # batch_size < 1
    with pytest.raises(Exception, match="batch_size < 1"):
        dev.ppo_update(8, good[None], 0, 1e-3, buffer=_rows(inp))
    with pytest.raises(Exception, match="no collection on the device"):
        dev.ppo_update(8, good[None], 4, 1e-3)
    acts = inp["actions"].copy()
    acts[2] = 26
    with pytest.raises(Exception, match="outside the policy's 26"):
        tr.step(inp["obs"], acts, *_rows(inp)[2:], lr=1e-3)
    assert tr.state()["t"] == 0
    # re-attaching the policy detaches the trainer
    dev.attach_policy(WeightPolicy(W, b, V, c))
    with pytest.raises(Exception, match="no trainer attached"):
        tr.step(*_rows(inp), lr=1e-3)
    # a collection of another size than the update asks for
    env = _env(3, table)
    te = PPOTrainer(env, agent, **ref.SETTINGS)
    env.collect(te, 2, GAMMA, LAM)
    with pytest.raises(Exception, match="has 6 rows, not 8"):
        env.dev.ppo_update(8, good[None], 4, 1e-3)
