"""
Reference of the policy net (closed_loop.WeightPolicy on the host, policy_kernel on the device) that shares no arithmetic with either:
the forward pass in numpy.longdouble (x87 extended, unit roundoff 2^-64), and beside it a FORWARD ROUNDING BOUND for an evaluation in
float64, propagated layer by layer. Not a test module; tests/test_policy_host.py and tests/test_gpu_policy.py import it.

The network: h_0 = float32(obs) (exact in both), z_l = W_l h_{l-1} + b_l, h_l = tanh(z_l) for the hidden layers, the logits are the
last z. The weights are float32 values, exact in float64 and in long double.

The bound, with u = 2^-53 the unit roundoff, eps = 2^-52 (one ulp of v is at most eps |v|) and gamma_n = n u / (1 - n u):
  * a dot product of K terms plus the bias, summed in ANY order, with or without fused multiply-adds (BLAS on the host, the 16 x 16 x 4
    matrix instruction on the device, which accumulates 4 terms at a time onto the running sum), on inputs that carry an error dh already:
        |dz| <= gamma_{K+1} (sum_k |w_k| (|h_k| + dh_k) + |b|)  +  sum_k |w_k| dh_k             (Higham, Accuracy and Stability, 3.1)
    K is the TRUE input width: the zero padding of the device adds exact zeros.
  * tanh is 1-Lipschitz, and the implementation returns tanh of ITS argument within c_tanh ulp:
        |dh| <= dz + c_tanh eps (|tanh z| + dz)
    c_tanh = 1 for numpy (glibc's tanh: < 1 ulp); for the device it is measured (tests/test_gpu_policy.py, profiles/policy_bounds.txt).
  * the long-double reference itself obeys the same recursion with 2^-64 in place of 2^-53: a 2^-11 part of the bound. The bound is
    multiplied by 1 + 2^-10 for it.
B_logit(x) is the bound of the last z.

Probabilities p_j = exp(z_j - m) / sum_i exp(z_i - m), m the largest logit (computed: the largest COMPUTED logit; the shift cancels
exactly in the exact quotient, so which m is used does not matter). RELATIVE bound of every p_j:
        2 max_j B_logit          the exponents of numerator and denominator terms each move by at most B_logit ... e^{2B} - 1, first order
      + 2 u spread               the subtraction z_j - m rounds: u |z_j - m| <= u spread in two exponents, spread = max z - min z
      + 2 c_exp eps              exp of numerator and of the sum's terms, c_exp = 3 ulp: the OpenCL bound for exp in double, which the
                                 device library meets; glibc's is below 1
      + (n_actions + 4) eps      the sum of n_actions positive terms (gamma_{n-1}), the division, and the second-order remainder
and the probabilities sum to 1 within (n_actions + 4) eps.
"""
import numpy as np

U = 2.0 ** -53
EPS = 2.0 ** -52
C_EXP = 3.0
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


def seeded_observations():
    """the two input sets of the issue: RandomState(0).rand(4096, 22) and 2 * RandomState(1).randn(4096, 22)"""
    return np.random.RandomState(0).rand(4096, 22), 2.0 * np.random.RandomState(1).randn(4096, 22)


def forward(weights, biases, obs, c_tanh=1.0):
    """(logits in long double (n, A), B_logit (n, A) float64) for observations (n, n_in)"""
    h = np.atleast_2d(np.asarray(obs, dtype=np.float64)).astype(np.float32).astype(LD)
    dh = np.zeros(h.shape, dtype=LD)
    for i, (w, b) in enumerate(zip(weights, biases)):
        w, b = np.asarray(w).astype(LD), np.asarray(b).astype(LD)
        K = w.shape[1]
        aw = np.abs(w)
        z = h @ w.T + b
        carried = dh @ aw.T
        dz = gamma(K + 1) * ((np.abs(h) + dh) @ aw.T + np.abs(b)) + carried
        if i + 1 < len(weights):
            h = np.tanh(z)
            dh = dz + c_tanh * EPS * (np.abs(h) + dz)
        else:
            return z, (dz * (1.0 + 2.0 ** -10)).astype(np.float64)


def probabilities(z):
    """softmax of long-double logits, in long double"""
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def probability_bound(z, b_logit):
    """(n,) relative bound of every probability of a row"""
    z = np.asarray(z, dtype=np.float64)
    n_act = z.shape[-1]
    spread = z.max(axis=-1) - z.min(axis=-1)
    return 2.0 * b_logit.max(axis=-1) + 2.0 * U * spread + 2.0 * C_EXP * EPS + (n_act + 4) * EPS


def top_gap(z):
    """(n,) gap between the two largest logits of a row"""
    s = np.sort(np.asarray(z, dtype=LD), axis=-1)
    if s.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    return (s[:, -1] - s[:, -2]).astype(np.float64)


def actions(z):
    return np.argmax(np.asarray(z, dtype=LD), axis=-1)


def synthetic_policy(widths, seed):
    """a seeded float32 network of the given widths (inputs, hidden..., actions): weights randn / sqrt(inputs of the layer), biases 0.1 randn"""
    rng = np.random.RandomState(seed)
    W = [(rng.randn(o, i) / np.sqrt(i)).astype(np.float32) for i, o in zip(widths[:-1], widths[1:])]
    b = [(0.1 * rng.randn(o)).astype(np.float32) for o in widths[1:]]
    return W, b
