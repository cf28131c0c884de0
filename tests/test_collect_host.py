"""
The host statements of collecting PPO training data (closed_loop: philox4x32 / policy_uniforms, WeightPolicy with a value net and its
values / log_prob / sample, gae) against tests/collect_reference.py: Philox in Python integers, the long-double forward pass with its
rounding bounds, and the literal GAE loop. No GPU.
"""
import io
import os
import zipfile

import numpy as np
import pytest

import collect_reference as cr
import policy_reference as pr

KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
SEED, T = 0x1234567890abcdef, 2 ** 32 + 5          # both words of the key and of the decision counter in use


@pytest.fixture(scope="module")
def agent(golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"), os.path.join(golden_dir, "wmpc_value.npz"))


def test_philox_known_answers():
    """Random123's two published vectors and the third of the issue, by the reference in integers and by closed_loop's numpy one"""
    from tum_control_amd.closed_loop import philox4x32
    for ctr, key, want in KNOWN:
        want = [int(w, 16) for w in want.split()]
        assert cr.philox4x32(ctr, key) == want
        assert [int(x) for x in philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))] == want
    # batched: one counter per row
    got = philox4x32(np.array([k[0] for k in KNOWN], dtype=np.uint64), np.array([0, 0], dtype=np.uint64))
    assert [int(x) for x in got[0]] == [int(w, 16) for w in KNOWN[0][2].split()]


def test_uniform_formula():
    from tum_control_amd.closed_loop import policy_uniforms, uniform_from_words
    assert uniform_from_words(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 == cr.uniform(0xffffffff, 0xffffffff)
    assert uniform_from_words(0, 0) == 0.0 and uniform_from_words(31, 63) == 0.0          # the dropped low bits
    assert uniform_from_words(32, 0) == 2.0 ** -27 and uniform_from_words(0, 64) == 2.0 ** -53
    rng = np.random.RandomState(0)
    x = rng.randint(0, 2 ** 32, size=(1000, 2), dtype=np.uint64)
    u = uniform_from_words(x[:, 0], x[:, 1])
    assert np.array_equal(u, [cr.uniform(a, b) for a, b in x]) and (u >= 0).all() and (u < 1).all()
    # the stream: (seed, b, t) alone decide a draw -- not the batch size, not where the batch starts
    u = policy_uniforms(SEED, T, 40, first_instance=7)
    assert np.array_equal(u, cr.uniforms(SEED, T, 40, first_instance=7))
    assert np.array_equal(policy_uniforms(SEED, T, 5, first_instance=17), u[10:15])
    assert not np.array_equal(policy_uniforms(SEED, T + 1, 40, first_instance=7), u)
    assert not np.array_equal(policy_uniforms(SEED + 2 ** 32, T, 40, first_instance=7), u)
    assert not np.array_equal(policy_uniforms(SEED, T + 2 ** 32, 40, first_instance=7), u)


def _archive(path, widths_pi, widths_vf, seed=3):
    """a stable_baselines3-shaped archive: a zip whose policy.pth is a plain state dict"""
    import torch
    W, b = pr.synthetic_policy(widths_pi, seed)
    sd = {}
    for i, (w, v) in enumerate(zip(W[:-1], b[:-1])):
        sd[f"mlp_extractor.policy_net.{2 * i}.weight"], sd[f"mlp_extractor.policy_net.{2 * i}.bias"] = torch.from_numpy(w), torch.from_numpy(v)
    sd["action_net.weight"], sd["action_net.bias"] = torch.from_numpy(W[-1]), torch.from_numpy(b[-1])
    V = c = None
    if widths_vf is not None:
        V, c = pr.synthetic_policy(widths_vf, seed + 1)
        for i, (w, v) in enumerate(zip(V[:-1], c[:-1])):
            sd[f"mlp_extractor.value_net.{2 * i}.weight"], sd[f"mlp_extractor.value_net.{2 * i}.bias"] = torch.from_numpy(w), torch.from_numpy(v)
        sd["value_net.weight"], sd["value_net.bias"] = torch.from_numpy(V[-1]), torch.from_numpy(c[-1])
    buf = io.BytesIO()
    torch.save(sd, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
    return W, b, V, c


def test_value_net_round_trips_and_refusals(tmp_path, agent, golden_dir):
    from tum_control_amd.closed_loop import WeightPolicy
    p = str(tmp_path / "with_value.zip")
    W, b, V, c = _archive(p, (6, 9, 5, 4), (6, 7, 1))          # pi and vf differ in depth and widths
    pol = WeightPolicy.from_sb3_zip(p)
    assert all(np.array_equal(x, y) for x, y in zip(pol.weights + pol.biases, W + b))
    assert all(np.array_equal(x, y) for x, y in zip(pol.value_weights + pol.value_biases, V + c))
    q = str(tmp_path / "without_value.zip")
    W, b, _, _ = _archive(q, (6, 9, 5, 4), None)
    bare = WeightPolicy.from_sb3_zip(q)
    assert bare.value_weights is None and bare.value_biases is None
    with pytest.raises(ValueError, match="no value net"):
        bare.values(np.zeros(6))
    # the npz format: V / c in the same file, or in a second one
    f = str(tmp_path / "both.npz")
    np.savez(f, **{f"W{i}": w for i, w in enumerate(pol.weights)}, **{f"b{i}": v for i, v in enumerate(pol.biases)},
             **{f"V{i}": w for i, w in enumerate(V)}, **{f"c{i}": v for i, v in enumerate(c)})
    both = WeightPolicy.from_npz(f)
    assert all(np.array_equal(x, y) for x, y in zip(both.value_weights + both.value_biases, V + c))
    assert WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz")).value_weights is None
    assert [w.shape for w in agent.value_weights] == [(128, 22), (256, 128), (128, 256), (1, 128)]
    # mismatched widths
    for vw, msg in (((7, 7, 1), "takes 7 inputs"), ((6, 7, 2), "one row")):
        Vb, cb = pr.synthetic_policy(vw, 1)
        with pytest.raises(ValueError, match=msg):
            WeightPolicy(W, b, Vb, cb)
    Vb, cb = pr.synthetic_policy((6, 7, 1), 1)
    with pytest.raises(ValueError, match="does not fit"):
        WeightPolicy(W, b, [Vb[0], Vb[1][:, :5]], cb)
    with pytest.raises(ValueError, match="value_weights AND value_biases"):
        WeightPolicy(W, b, Vb)
    # without a value net: today's object
    x = np.random.RandomState(0).rand(50, 6)
    assert np.array_equal(bare.logits(x), pol.logits(x)) and np.array_equal(bare.predict(x), pol.predict(x))
    old = WeightPolicy.from_npz(os.path.join(golden_dir, "wmpc_policy.npz"))
    x = np.load(os.path.join(golden_dir, "wmpc_policy.npz"))["obs"]
    assert np.array_equal(old.logits(x), agent.logits(x)) and np.array_equal(old.predict(x), agent.predict(x))


@pytest.fixture(scope="module")
def seeded():
    return [x[:1024] for x in pr.seeded_observations()]


def test_values_within_the_forward_bound(agent, seeded, golden_dir):
    """pr.forward works for a net whose last width is 1; the host mirror within its bound; the recorded float32 pass nearby"""
    for x in seeded:
        v, bound = cr.value(agent.value_weights, agent.value_biases, x)
        got = agent.values(x)
        err = np.abs(got.astype(pr.LD) - v).astype(np.float64)
        print("values err / bound", (err / bound).max(), "bound", bound.max())
        assert got.shape == (len(x),) and (err <= bound).all()
    assert np.ndim(agent.values(np.zeros(22))) == 0
    rec = np.load(os.path.join(golden_dir, "wmpc_value.npz"))["values_f32"]
    assert np.abs(agent.values(np.load(os.path.join(golden_dir, "wmpc_policy.npz"))["obs"]) - rec).max() < 1e-4


def test_log_prob_within_its_bound(agent, seeded):
    for k, x in enumerate(seeded):
        a = agent.sample(x, SEED, T + k)
        lp, bound = cr.log_prob(agent.weights, agent.biases, x, a)
        err = np.abs(agent.log_prob(x, a).astype(pr.LD) - lp).astype(np.float64)
        print("log_prob err / bound", (err / bound).max(), "bound", bound.max())
        assert (err <= bound).all()
        # every action of one row: log of the softmax
        lp, bound = cr.log_prob(agent.weights, agent.biases, np.repeat(x[:1], 26, axis=0), np.arange(26))
        got = agent.log_prob(np.repeat(x[:1], 26, axis=0), np.arange(26))
        assert (np.abs(got.astype(pr.LD) - lp).astype(np.float64) <= bound).all()
        assert abs(np.exp(got).sum() - 1.0) < 1e-12


def test_sample_equals_the_long_double_cdf(agent):
    """all 4096 seeded rows of both kinds: the action of the long-double CDF on every decided row, and no row is set aside"""
    for k, x in enumerate(pr.seeded_observations()):
        u = cr.uniforms(SEED, T + k, len(x))
        want, decided = cr.sample(agent.weights, agent.biases, x, u)
        got = agent.sample(x, SEED, T + k)
        print("rows set aside", int((~decided).sum()), "of", len(x), "distinct actions", len(np.unique(got)))
        assert (~decided).sum() <= len(x) // 1000
        assert (~decided).sum() == 0          # (checked for this seed: the host mirror sets no row aside)
        assert np.array_equal(got[decided], want[decided])
        assert len(np.unique(got)) > 3
    # first_instance shifts the stream
    x = pr.seeded_observations()[0][:64]
    assert np.array_equal(agent.sample(x[10:20], SEED, T, first_instance=10), agent.sample(x, SEED, T)[10:20])
    # u S < c_j never holds for the last action's own boundary only if u S == S: the fallback is A - 1
    from tum_control_amd.closed_loop import WeightPolicy
    one = WeightPolicy([np.zeros((2, 3), np.float32), np.zeros((1, 2), np.float32)], [np.zeros(2, np.float32), np.zeros(1, np.float32)])
    assert np.array_equal(one.sample(np.zeros((5, 3)), 1, 2), np.zeros(5, dtype=int))


def test_sample_frequencies(agent):
    """200 000 draws on the all-zeros observation over t: every action within 5 standard deviations of its probability"""
    from tum_control_amd.closed_loop import policy_uniforms
    n = 200000
    p = agent.probabilities(np.zeros(22))
    # one instance, t = 0 .. n - 1: the uniforms in blocks (policy_uniforms is vectorised over instances, so t goes through the key-less
    # counter words one value at a time in the reference; here the same draws come from the numpy Philox with t as an array)
    from tum_control_amd.closed_loop import philox4x32, uniform_from_words
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 1] = np.arange(n)
    x = philox4x32(ctr, np.array([SEED & 0xffffffff, SEED >> 32], dtype=np.uint64))
    u = uniform_from_words(x[:, 0], x[:, 1])
    for t in (0, 1, 77777, n - 1):
        assert u[t] == policy_uniforms(SEED, t, 1)[0] == cr.uniforms(SEED, t, 1)[0]
    c = np.cumsum(np.exp(agent.logits(np.zeros(22)) - agent.logits(np.zeros(22)).max()))
    below = (u * c[-1])[:, None] < c[None, :]
    a = np.where(below.any(axis=1), np.argmax(below, axis=1), 25)
    for t in (0, 5, 1000):
        assert a[t] == agent.sample(np.zeros((1, 22)), SEED, t)[0]
    freq = np.bincount(a, minlength=26) / n
    sd = np.sqrt(p * (1 - p) / n)
    print("largest deviation in standard deviations", (np.abs(freq - p) / sd).max())
    assert (np.abs(freq - p) <= 5.0 * sd).all()


def test_gae_equals_the_literal_loop():
    from tum_control_amd.closed_loop import gae
    rng = np.random.RandomState(4)
    for E, B, starts in ((1, 1, None), (1, 7, None), (5, 9, None), (6, 4, 1.0), (6, 4, 0.0), (12, 33, None)):
        r, v = rng.randn(E, B), rng.randn(E, B)
        es = (rng.rand(E, B) < 0.3).astype(float) if starts is None else np.full((E, B), starts)
        lv, ld = rng.randn(B), (rng.rand(B) < 0.5).astype(float)
        adv, ret = gae(r, v, es, lv, ld, 0.99, 0.95)
        a0, r0 = cr.gae_loop(r, v, es, lv, ld, 0.99, 0.95)
        assert np.array_equal(adv, a0) and np.array_equal(ret, r0), (E, B)
    # against the textbook form on one episode without ends
    r, v = rng.randn(4, 1), rng.randn(4, 1)
    adv, _ = gae(r, v, np.zeros((4, 1)), np.array([0.3]), np.zeros(1), 0.9, 0.8)
    nv = np.append(v[1:, 0], 0.3)
    delta = r[:, 0] + 0.9 * nv - v[:, 0]
    want = [sum((0.9 * 0.8) ** (k - t) * delta[k] for k in range(t, 4)) for t in range(4)]
    assert np.allclose(adv[:, 0], want, rtol=0, atol=1e-13)
