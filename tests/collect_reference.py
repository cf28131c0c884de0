"""
Reference of what collecting PPO training data adds to the policy net (closed_loop.WeightPolicy.values / log_prob / sample on the host,
policy_ac_kernel on the device), sharing no arithmetic with either: Philox4x32-10 in plain Python integers, and the log-probability and
the sampled action from the long-double forward pass of tests/policy_reference.py. Not a test module; tests/test_collect_host.py and
tests/test_gpu_collect.py import it.

The uniform. u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 with x0, x1 the first two words of Philox4x32-10 on the counter
(b, t & 0xffffffff, t >> 32, 0) and the key (seed & 0xffffffff, seed >> 32): a 53-bit integer times a power of two, exact in a double.
Host and device must agree on it to the bit.

The log-probability. With z the logits, m any shift and S(m) = sum_j exp(z_j - m): log p_a = (z_a - m) - log S(m) EXACTLY, whatever m
is -- the shift cancels. The code under test computes, with m^ its own largest COMPUTED logit,
        lp^ = fl( fl(z^_a - m^) - log^( S^ ) ),     S^ = fl-sum of exp^( fl(z^_j - m^) ) in index order.
Take m = m^ as the (exact) shift of the reference identity. With B = max_j B_logit, u = 2^-53, eps = 2^-52, spread = max z - min z:
  * z^_a against z_a:                          at most B
  * the rounding of the subtraction z^_a - m^: u |z_a - m| <= u spread (first order)
  * S^ against S(m^): every exponent moves by at most B (m^ is a constant here, so ONE B, not two), its subtraction rounds (u spread),
    exp returns its argument's exponential within c_exp ulp, the sum of A positive terms rounds A - 1 times: relative
    theta <= B + u spread + c_exp eps + A eps, and |log S^ - log S| = |log(1 + theta)| <= theta (first order)
  * the three lines above add up to 2 B + 2 u spread + c_exp eps + A eps, which is below
    probability_bound(z, B_logit) = 2 B + 2 u spread + 2 c_exp eps + (A + 4) eps; the difference, c_exp eps + 4 eps, pays for the
    second-order remainders and for the long-double reference's own 2^-11 part
  * log returns the logarithm of ITS argument within C_LOG ulp:  C_LOG eps |log S|      (C_LOG = 3: the OpenCL bound for a double log,
    which the device library meets; glibc's is below 1)
  * the final subtraction rounds:  u |lp| <= eps |log p_a|
        |lp^ - log p_a| <= probability_bound(z, B_logit) + C_LOG eps |log S| + eps |log p_a|
No further term is needed: S is evaluated with the shift max z, S in [1, A], so log S >= 0 and is itself of order 1.

The sampled action. The rule is the smallest j with u S < c_j, c the prefix sums of exp(z - m). In exact arithmetic that is the smallest
j with u < F_j, F_j = c_j / S the CDF. Every computed c_j / S is a ratio of sums of the terms whose RELATIVE error probability_bound
covers (a prefix sum is a sum of numerators), and the product u S rounds once more (u); comparing u S with c_j is comparing u with
c_j / S up to A eps for the at most A - 1 additions of the prefix that the bound of a single probability does not count. So where
|u - F_j| > probability_bound + A eps for EVERY j, computed and exact decision are the same; the other rows are set aside.
"""
import numpy as np

import policy_reference as pr

C_LOG = 3.0
M32 = 0xffffffff


def philox4x32(counter, key):
    """Philox4x32-10 in Python integers: counter and key as sequences of 32-bit words -> list of 4 words"""
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def uniform(x0, x1):
    """the stated formula in integers; the division by 2^53 of an integer below 2^53 is exact"""
    return ((int(x0) >> 5) * 2 ** 26 + (int(x1) >> 6)) / 2 ** 53


def uniforms(seed, t, n, first_instance=0):
    seed, t = int(seed), int(t)
    out = np.empty(n)
    for i in range(n):
        x = philox4x32([(first_instance + i) & M32, t & M32, t >> 32, 0], [seed & M32, seed >> 32])
        out[i] = uniform(x[0], x[1])
    return out


def value(weights, biases, obs, c_tanh=1.0):
    """(values in long double (n,), bound (n,)) of a net whose last width is 1"""
    z, b = pr.forward(weights, biases, obs, c_tanh=c_tanh)
    assert z.shape[1] == 1
    return z[:, 0], b[:, 0]


def log_prob(weights, biases, obs, actions, c_tanh=1.0):
    """(log p_a in long double (n,), its bound (n,)) for the given actions"""
    z, b = pr.forward(weights, biases, obs, c_tanh=c_tanh)
    d = z - z.max(axis=-1, keepdims=True)
    S = np.exp(d).sum(axis=-1)
    a = np.asarray(actions, dtype=np.int64)
    lp = d[np.arange(len(d)), a] - np.log(S)
    bound = pr.probability_bound(z, b) + C_LOG * pr.EPS * np.abs(np.log(S)).astype(np.float64) + pr.EPS * np.abs(lp).astype(np.float64)
    return lp, bound


def sample(weights, biases, obs, u, c_tanh=1.0):
    """(actions (n,) of the long-double CDF, decided (n,) bool): decided where u is further from every CDF boundary than
    probability_bound + A eps"""
    z, b = pr.forward(weights, biases, obs, c_tanh=c_tanh)
    A = z.shape[1]
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    F = np.cumsum(e, axis=-1) / e.sum(axis=-1, keepdims=True)
    ul = np.asarray(u).astype(pr.LD)[:, None]
    below = ul < F
    act = np.where(below.any(axis=1), np.argmax(below, axis=1), A - 1)
    band = pr.probability_bound(z, b) + A * pr.EPS
    decided = (np.abs(ul - F[:, :A - 1]).astype(np.float64) > band[:, None]).all(axis=1) if A > 1 else np.ones(len(z), dtype=bool)
    return act, decided


def gae_loop(rewards, values, episode_starts, last_values, last_dones, gamma, lam):
    """the loop of the issue, element by element in Python floats (IEEE double, no contraction)"""
    E, B = rewards.shape
    adv, ret = np.zeros((E, B)), np.zeros((E, B))
    for b in range(B):
        last = 0.0
        for t in range(E - 1, -1, -1):
            nnt = 1.0 - float(last_dones[b] if t == E - 1 else episode_starts[t + 1, b])
            nv = float(last_values[b] if t == E - 1 else values[t + 1, b])
            delta = (float(rewards[t, b]) + (gamma * nv) * nnt) - float(values[t, b])
            last = delta + ((gamma * lam) * nnt) * last
            adv[t, b] = last
            ret[t, b] = adv[t, b] + float(values[t, b])
    return adv, ret
