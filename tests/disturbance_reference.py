"""
The counter-based disturbance draw of the closed loop once more, exactly: the definition of include/tum_nmpc.h ("Disturbance draws")
restated from its text -- not from disturbance_kernels.hpp, not from closed_loop.py -- in Python integers (Philox4x32-10, the 53-bit
mantissas), in mpmath at 60 digits (the two normal kinds) and in exact rational arithmetic rounded to nearest (the box kind), and the
draws at which the tests compare it with the plain binary64 statement closed_loop.disturbance_from_uniforms / DisturbanceModel.draw_counter
(tests/test_disturbance_reference.py) and with disturbance_draw_kernel (tests/test_gpu_disturbances.py).

The inputs of a draw are integers: the mantissas mA[j], mB[j] of its five blocks, u = m 2^-53 exactly; and the bounds w, exact binary64.

  'gaussian'  w[i] z[i],  z[2j] = R_j cos(theta_j), z[2j+1] = R_j sin(theta_j), R_j = sqrt(-2 ln(1 - uA_j)), theta_j = 2 pi uB_j
  'uniform'   sqrt(w[i]) r z[i] / |z|, |z| over z[0..6], r = uA_4 ^ (1/7) (1/7 the rational, not its binary64 neighbour); |z| = 0: zeros
  'absolute'  w[i]
  box         -w[i] + u_i (2 w[i]) with the product and the sum each rounded to nearest once: an exact statement of two IEEE operations,
              here float(Fraction) twice. Equal to the bit or wrong.

THE UNIT, per channel, from exact quantities only, u = 2^-53:
  a normal    u s R (1 + theta), s the channel's scale (w[i] for 'gaussian'): the roundings of the logarithm, the root and the
              product (u R each), the rounding of theta = 2 pi uB carried through sin / cos (u theta R)
  'uniform'   with the output o_i and E_j = R_j (1 + theta_j) of channel j's block:
              u ( |o_i| (1 + |ln uA_4| / 7) + sqrt(w[i]) r / |z| (E_i + |z_i| / |z|^2 sum_j |z_j| E_j) )
              -- the output's own roundings and the rounded exponent 1/7 of the power, and the normals' units carried through
              z_i / |z| (the quotient rule). r = 0 (uA_4 = 0) or |z| = 0: the output is an exact zero, the unit 0.
  box, 'absolute': none.
An error is |got - exact| / unit; where the unit is 0 the exact value is a zero and anything else is an infinite error.
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 60
U53 = 2.0 ** -53
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xffffffff
BLOCKS = 5


def philox(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) in Python integers: counter (4 words), key (2 words) -> 4 words"""
    c, k = [int(v) & MASK for v in counter], [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def block_words(seed, b, t, s, j):
    """the four words of block j of stream s for instance b at global control step t"""
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    return philox([int(b) & MASK, t & MASK, t >> 32, 0x100 * (1 + int(s)) + int(j)], [seed & MASK, seed >> 32])


def mantissa(x0, x1):
    return ((x0 >> 5) << 26) + (x1 >> 6)


def mantissas(seed, b, t, s):
    """(mA, mB): five integers each in [0, 2^53) -- u = m 2^-53"""
    mA, mB = [], []
    for j in range(BLOCKS):
        x = block_words(seed, b, t, s, j)
        mA.append(mantissa(x[0], x[1])); mB.append(mantissa(x[2], x[3]))
    return mA, mB


def uniforms(mA, mB):
    """the binary64 uniforms of mantissas (an exact conversion), shape (..., 5) each"""
    return np.array(mA, dtype=np.uint64).astype(np.float64) * U53, np.array(mB, dtype=np.uint64).astype(np.float64) * U53


def exact(kind, w, mA, mB):
    """dict(value: 7 mpf (normal kinds) or 7 floats (box, 'absolute'), unit: 7 floats or None)"""
    w = [float(v) for v in w]
    if kind == "absolute":
        return dict(value=list(w), unit=None)
    if kind not in ("uniform", "gaussian"):
        out = []
        for i in range(7):
            m = (mA if i % 2 == 0 else mB)[i >> 1]
            prod = float(Fraction(m, 2 ** 53) * Fraction(2.0 * w[i]))          # (2 w is exact)
            out.append(float(Fraction(-w[i]) + Fraction(prod)))
        return dict(value=out, unit=None)
    with mp.workdps(DPS):
        two53 = mp.mpf(2) ** 53
        z, E = [], []
        for j in range(4):
            uA, uB = mp.mpf(mA[j]) / two53, mp.mpf(mB[j]) / two53
            R = mp.sqrt(-2 * mp.log(1 - uA))
            th = 2 * mp.pi * uB
            z += [R * mp.cos(th), R * mp.sin(th)]
            E += [R * (1 + th)] * 2
        z, E = z[:7], E[:7]
        if kind == "gaussian":
            return dict(value=[mp.mpf(w[i]) * z[i] for i in range(7)], unit=[float(U53 * w[i] * E[i]) for i in range(7)])
        nz = mp.sqrt(sum(v * v for v in z))
        u4 = mp.mpf(mA[4]) / two53
        if nz == 0 or u4 == 0:
            return dict(value=[mp.mpf(0)] * 7, unit=[0.0] * 7)
        r = mp.root(u4, 7)
        carried = sum(abs(z[j]) * E[j] for j in range(7))
        value, unit = [], []
        for i in range(7):
            sw = mp.sqrt(mp.mpf(w[i]))
            o = sw * r * z[i] / nz
            value.append(o)
            unit.append(float(U53 * (abs(o) * (1 + abs(mp.log(u4)) / 7) + sw * r / nz * (E[i] + abs(z[i]) / nz ** 2 * carried))))
        return dict(value=value, unit=unit)


def errors(got, ref):
    """|got - exact| in units, per channel (normal kinds); a zero unit: 0 where got is the exact zero, inf elsewhere"""
    out = np.zeros(7)
    with mp.workdps(DPS):
        for i in range(7):
            d = abs(mp.mpf(float(got[i])) - ref["value"][i])
            out[i] = float(d / ref["unit"][i]) if ref["unit"][i] > 0 else (0.0 if d == 0 else math.inf)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------- the draws of the measurement
TOP = 2 ** 53 - 1          # u = 1 - 2^-53
FORCED_A = (0, 1, TOP)                                          # uA = 0, 2^-53, 1 - 2^-53
FORCED_B = (0, 2 ** 51, 2 ** 52, 3 * 2 ** 51, TOP)              # uB = 0, 1/4, 1/2, 3/4, 1 - 2^-53
N_RANDOM = 3000


def shipped_bounds():
    """(derivative magnitudes, estimation-error magnitudes) of the shipped configuration"""
    from tum_control_amd.closed_loop import DisturbanceModel
    m = DisturbanceModel()
    return np.array(m.bounds_derivatives, dtype=float)[:, 1], np.array(m.bounds_state_estimation, dtype=float)[:, 1]


def measurement_draws():
    """(W (n, 7), MA (n, 5), MB (n, 5)) integer mantissas and bounds: N_RANDOM draws of the generator itself (seeds below and above
    2^32, instances and steps up to 2^31 and beyond 2^32, both streams, the two shipped magnitude sets alternating), then the forced
    words -- every (uA, uB) pair of FORCED_A x FORCED_B in EVERY block at once (the radius block included), each pair also in one
    block alone with the generator's words elsewhere, and each once more with a zero bound on one channel."""
    wd, we = shipped_bounds()
    rng = np.random.RandomState(20241)
    W, MA, MB = [], [], []
    for n in range(N_RANDOM):
        seed = int(rng.randint(0, 2 ** 31)) << (0 if n % 3 else 17)
        b, t = int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 2 ** 31)) << (0 if n % 5 else 9)
        mA, mB = mantissas(seed, b, t, n & 1)
        W.append(wd if n & 1 == 0 else we); MA.append(mA); MB.append(mB)
    k = 0
    for a in FORCED_A:
        for bb in FORCED_B:
            base_a, base_b = mantissas(7, k, 1000 + k, k & 1)
            one_a, one_b = list(base_a), list(base_b)
            one_a[k % BLOCKS] = a; one_b[k % BLOCKS] = bb
            for mA, mB in (([a] * BLOCKS, [bb] * BLOCKS), (one_a, one_b)):
                w0 = np.array(wd if k & 1 == 0 else we)
                wz = w0.copy(); wz[k % 7] = 0.0
                for w in (w0, wz):
                    W.append(w); MA.append(list(mA)); MB.append(list(mB))
            k += 1
    return np.array(W), np.array(MA, dtype=np.uint64), np.array(MB, dtype=np.uint64)
