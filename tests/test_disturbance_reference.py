"""
The plain binary64 statement of the counter-based disturbance draw -- closed_loop.disturbance_from_uniforms, and
DisturbanceModel.draw_counter around it -- held to the exact restatement of tests/disturbance_reference.py, and the properties a draw
has by its definition (include/tum_nmpc.h, "Disturbance draws"). No GPU.

THE GATE of the two normal kinds, used here and by tests/test_gpu_disturbances.py: max(32, 4 x the plain statement's own largest error)
in the units of disturbance_reference, per kind, measured below on disturbance_reference.measurement_draws() (3000 draws of the
generator and the forced words). 32 is the project's floor for a chain of a few library calls; nothing in a gate comes from a device
result. Measured (profiles/disturbance_bounds.txt): 'gaussian' 2.4, 'uniform' 0.96 units: both gates are 32.
"""
import functools

import numpy as np
import pytest

import disturbance_reference as dr
from tum_control_amd import closed_loop as cl

FLOOR = 32.0
NORMAL_KINDS = ("gaussian", "uniform")
KINDS = ("uniform", "gaussian", "absolute", "box")


@functools.lru_cache(maxsize=None)
def plain_errors(kind):
    """largest error of the plain statement over the measurement draws, in units (a float), and the draw it was seen at"""
    W, MA, MB = dr.measurement_draws()
    uA, uB = dr.uniforms(MA, MB)
    worst, at = 0.0, None
    for w in np.unique(W, axis=0):
        m = np.flatnonzero((W == w).all(axis=1))
        got = cl.disturbance_from_uniforms(kind, w, uA[m], uB[m])
        for k, n in enumerate(m):
            e = dr.errors(got[k], dr.exact(kind, w, [int(v) for v in MA[n]], [int(v) for v in MB[n]])).max()
            if e > worst:
                worst, at = float(e), int(n)
    return worst, at


def gate_units(kind):
    return max(FLOOR, 4.0 * plain_errors(kind)[0])


@pytest.mark.parametrize("kind", NORMAL_KINDS)
def test_plain_statement_against_the_exact_restatement(kind):
    W, _, _ = dr.measurement_draws()
    assert len(W) >= 3000
    worst, at = plain_errors(kind)
    print(f"disturbance_bounds plain {kind}: largest error {worst:.4g} units at draw {at}, gate {gate_units(kind):.4g}")
    assert np.isfinite(worst)
    assert worst <= FLOOR, "the plain statement itself is further from the exact value than the floor of the gate: look at it"


@pytest.mark.parametrize("kind", ("absolute", "box"))
def test_exact_kinds_are_equal_to_the_bit(kind):
    W, MA, MB = dr.measurement_draws()
    uA, uB = dr.uniforms(MA, MB)
    for w in np.unique(W, axis=0):
        m = np.flatnonzero((W == w).all(axis=1))
        got = cl.disturbance_from_uniforms(kind, w, uA[m], uB[m])
        ref = np.array([dr.exact(kind, w, [int(v) for v in MA[n]], [int(v) for v in MB[n]])["value"] for n in m])
        assert dr.same_bits(got, ref)


def test_forced_words_are_in_the_measurement():
    _, MA, MB = dr.measurement_draws()
    for a in dr.FORCED_A:
        for b in dr.FORCED_B:
            assert ((MA == a) & (MB == b)).all(axis=1).any(), (a, b)
    W, _, _ = dr.measurement_draws()
    assert (W[dr.N_RANDOM:] == 0.0).any() and (W[:dr.N_RANDOM] > 0.0).all()
    # uA = 0 is R = 0: a zero normal; uA = 1 - 2^-53 the largest R there is
    z = cl.disturbance_from_uniforms("gaussian", np.ones(7), *dr.uniforms([[0] * 5, [dr.TOP] * 5], [[2 ** 51] * 5] * 2))
    assert (z[0] == 0.0).all() and np.abs(z[1]).max() == pytest.approx(np.sqrt(2 * 53 * np.log(2.0)), rel=1e-12)


def _model(kind_w="uniform", kind_e="gaussian", **kw):
    return cl.DisturbanceModel(dict(simulate_disturbances=True, simulate_state_estimation=True, disturbance_type_derivatives=kind_w,
                                    disturbance_type_state_estimation=kind_e, **kw))


KAT_WORDS = [0x7b6c831f, 0x0fa3fccc, 0xb9cd1ad6, 0x64b0aab8]


def test_philox_restatement_known_answer():
    """Random123's own known-answer vector of Philox4x32-10 (kat_vectors: counter and key all ones)"""
    assert dr.philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_counter_layout_known_answer():
    """one (seed, b, t, s, j) with its four words, written out: the counter is (b, t & 0xffffffff, t >> 32, 0x100 (1 + s) + j), the key
    (seed & 0xffffffff, seed >> 32)"""
    seed, b, t, s, j = 0x123456789abcdef, 5, (1 << 32) + 77, 1, 3
    words = cl.philox4x32(np.array([b, t & 0xffffffff, t >> 32, 0x100 * (1 + s) + j], dtype=np.uint64),
                          np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    assert [int(v) for v in words] == KAT_WORDS
    assert dr.block_words(seed, b, t, s, j) == KAT_WORDS
    # ... and draw_counter reads exactly that block: the box kind's channels 6 (uA) of block 3, stream 1
    m = _model("box", "box")
    _, e = m.draw_counter(1, batch=1, seed=seed, first_step=t, first_instance=b)
    w = np.array(m.bounds_state_estimation)[:, 1]
    uA = cl.uniform_from_words(KAT_WORDS[0], KAT_WORDS[1])
    assert e[0, 0, 6] == -w[6] + uA * (2.0 * w[6])
    # the stream tag of the derivative disturbance is 0x100, of the estimation error 0x200: never 0 (the policy's draws)
    assert dr.block_words(seed, b, t, 0, j) != KAT_WORDS


@pytest.mark.parametrize("kinds", (("uniform", "gaussian"), ("box", "absolute"), ("gaussian", "box")))
def test_draw_counter_is_the_statement_of_its_words(kinds):
    """draw_counter against the restatement's own Philox and mantissas, through disturbance_from_uniforms: bit for bit"""
    m = _model(*kinds)
    seed, t0, b0 = (1 << 40) + 12345, 2 ** 31 - 2, 2 ** 32 - 3
    w, e = m.draw_counter(4, batch=5, seed=seed, first_step=t0, first_instance=b0)
    for s, (got, kind, bounds) in enumerate(((w, kinds[0], m.bounds_derivatives), (e, kinds[1], m.bounds_state_estimation))):
        for i in range(4):
            for k in range(5):
                mA, mB = dr.mantissas(seed, (b0 + k) & 0xffffffff, t0 + i, s)
                ref = cl.disturbance_from_uniforms(kind, np.array(bounds)[:, 1], *dr.uniforms(mA, mB))
                assert dr.same_bits(got[i, k], ref), (s, i, k)


def test_a_row_does_not_depend_on_the_window_or_the_batch():
    m = _model()
    full = m.draw_counter(9, batch=7, seed=3, first_step=10, first_instance=2)
    for q in range(2):
        assert dr.same_bits(m.draw_counter(3, batch=7, seed=3, first_step=14, first_instance=2)[q], full[q][4:7])
        assert dr.same_bits(m.draw_counter(9, batch=2, seed=3, first_step=10, first_instance=5)[q], full[q][:, 3:5])
        assert dr.same_bits(m.draw_counter(1, batch=1, seed=3, first_step=18, first_instance=8)[q], full[q][8:, 6:])
    # a window drawn in several slabs of steps (more than 2^16 rows) is the window
    big = m.draw_counter(3, batch=(1 << 16) // 2 + 1, seed=3, first_step=10, first_instance=2)
    assert dr.same_bits(big[0][:, :7], full[0][:3]) and dr.same_bits(big[1][:, :7], full[1][:3])


def test_streams_and_seeds_differ():
    m = _model("gaussian", "gaussian", **{f"w_{n}": 1.0 for n in cl.STATE_NAMES}, **{f"w_{n}_dot": 1.0 for n in cl.STATE_NAMES})
    w, e = m.draw_counter(4, batch=3, seed=1)
    assert not np.any(w == e)
    w2, e2 = m.draw_counter(4, batch=3, seed=2)
    assert not np.any(w == w2) and not np.any(e == e2)
    # neither stream meets the policy's draws under the same seed (their counter ends in 0): the box kind with w = 1/2 is u - 1/2,
    # u of channel 0 the first uniform of block 0
    half = {f"w_{n}": 0.5 for n in cl.STATE_NAMES}
    half.update({f"w_{n}_dot": 0.5 for n in cl.STATE_NAMES})
    bw, be = _model("box", "box", **half).draw_counter(1, batch=6, seed=9, first_step=4)
    pol = cl.policy_uniforms(9, 4, 6) - 0.5
    assert not np.any(bw[0, :, 0] == pol) and not np.any(be[0, :, 0] == pol)
    # a stream that is switched off is None, the other one unchanged
    m.derivatives = False
    w3, e3 = m.draw_counter(4, batch=3, seed=1)
    assert w3 is None and dr.same_bits(e3, e)


def test_kinds_keep_their_sets():
    n, B = 64, 64
    for zero in (None, 2):
        over = {} if zero is None else {f"w_{cl.STATE_NAMES[zero]}_dot": 0.0}
        m = _model("uniform", "box", **over)
        w, e = m.draw_counter(n, batch=B, seed=11)
        bw, be = np.array(m.bounds_derivatives)[:, 1], np.array(m.bounds_state_estimation)[:, 1]
        pos = bw > 0
        assert (np.sum(w[..., pos] ** 2 / bw[pos], axis=-1) <= 1 + 1e-12).all()
        assert (w[..., ~pos] == 0.0).all()
        assert (np.sum(w[..., pos] ** 2 / bw[pos], axis=-1) > 0).all()
        assert (e >= -be).all() and (e < be).all()
    m = _model("absolute", "absolute")
    w, e = m.draw_counter(3, batch=2, seed=11)
    assert dr.same_bits(w, np.broadcast_to(np.array(m.bounds_derivatives)[:, 1], (3, 2, 7)))
    assert dr.same_bits(e, np.broadcast_to(np.array(m.bounds_state_estimation)[:, 1], (3, 2, 7)))


def test_gaussian_moments():
    """16 384 draws with the shipped magnitudes: mean and standard deviation of every channel within 5 standard errors (fixed seed: a
    deterministic check)"""
    m = _model("gaussian", "gaussian")
    n = 16384
    w, e = m.draw_counter(128, batch=128, seed=2024)
    for got, bounds in ((w, m.bounds_derivatives), (e, m.bounds_state_estimation)):
        sd = np.array(bounds)[:, 1]
        x = got.reshape(n, 7)
        assert (np.abs(x.mean(axis=0)) <= 5 * sd / np.sqrt(n)).all()
        assert (np.abs(x.std(axis=0, ddof=1) - sd) <= 5 * sd / np.sqrt(2 * n)).all()


def test_legacy_draw_is_untouched():
    """`draw` keeps numpy's Mersenne-Twister stream: the counter-based one is another set of numbers from the same distributions"""
    m = _model()
    w, e = m.draw(3, batch=2, seed=4)
    wc, ec = m.draw_counter(3, batch=2, seed=4)
    assert w.shape == wc.shape and e.shape == ec.shape and not np.any(w == wc)
    rng = np.random.RandomState(4)
    assert dr.same_bits(w[0, 0], cl.generate_disturbances(m.bounds_derivatives, "uniform", rng))


def test_closed_loop_batch_refuses_what_a_draw_mode_cannot_do():
    with pytest.raises(ValueError, match="draw must be"):
        cl.ClosedLoopBatch("monteblanco", draw="philox")
    with pytest.raises(ValueError, match="on_device=True"):
        cl.ClosedLoopBatch("monteblanco", disturbances=_model(), draw="device")
    with pytest.raises(ValueError, match="DisturbanceModel"):
        cl.ClosedLoopBatch("monteblanco", disturbances=(None, None), draw="counter")
