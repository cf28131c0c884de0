"""
References of the PPO update (closed_loop.ppo_loss_and_grads / adam_step on the host, ppo_*_kernel on the device) that share no arithmetic
with either. Not a test module; tests/test_ppo_host.py and tests/test_gpu_ppo.py import it.

(a) loss_and_grads_ld: loss, diagnostics and every gradient of one minibatch in numpy.longdouble (unit roundoff 2^-64) with the
    analytic backward pass.
(b) loss_and_grads_torch: the same through torch's CPU autograd in float64 -- torch.distributions.Categorical, torch.min / clamp,
    mse_loss, .std() -- so neither the forward expressions nor the backward pass are the project's.
(c) adam_ld: clip + Adam in long double on given gradients and moments.

The gate of a gradient tensor (the issue's): err(g) = max |g - g_ld| / (u max |g_ld|), u = 2^-53. All of (a), (b), the host statement
and the device are sums of the same terms in different orders: the host statement may have at most 4 x torch's error on the same
tensor, the device at most 4 x the larger of the two host errors, both with a floor of 32 units. A dropped or doubled row is off by
about 1 / n of the gradient: nine orders of magnitude outside.
"""
import numpy as np

import policy_reference as pr

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 32.0
SETTINGS = dict(clip_range=0.2, ent_coef=0.006, vf_coef=0.5)
NETS = {"odd": ((22, 20, 36, 26), (22, 37, 1)), "tiny": ((3, 5, 2), (3, 200, 17, 1)), "widest": ((128, 256, 200, 64), (128, 256, 1)),
        "shipped": ((22, 128, 256, 128, 26), (22, 128, 256, 128, 1))}
SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "grad_norm")
# the scalars the issue puts under the RELATIVE gate |x - x_ld| / (u |x_ld|): the loss parts, approx_kl and grad_norm. The total loss is
# their combination policy_loss + ent_coef entropy_loss + vf_coef value_loss, whose terms cancel (at "odd", n = 2: -0.0623 - 0.0192 +
# 0.0609 = -0.0206), so its relative error is that of the parts times the cancellation: it is held by loss_bound() instead.
GATED = SCALARS[1:]


def nets(name):
    """(W, b, V, c) of the seeded nets of a case: policy net seed 11, value net seed 12"""
    pw, vw = NETS[name]
    return pr.synthetic_policy(pw, 11) + pr.synthetic_policy(vw, 12)


def _forward(W, b, h, dt):
    hs = [h]
    for i, (w, bb) in enumerate(zip(W, b)):
        z = hs[-1] @ w.astype(dt).T + bb.astype(dt)
        hs.append(np.tanh(z) if i + 1 < len(W) else z)
    return hs


def _backward(W, hs, dz, dt):
    gW, gb = [None] * len(W), [None] * len(W)
    for l in range(len(W) - 1, -1, -1):
        gW[l], gb[l] = dz.T @ hs[l], dz.sum(0)
        if l:
            dz = (dz @ W[l].astype(dt)) * (1 - hs[l] * hs[l])
    return gW, gb


def case(name, n):
    """the inputs of a case of n rows: obs, actions, adv, ret from RandomState(5), old_log_prob = the net's own + 0.3 randn drawn last"""
    W, b, V, c = nets(name)
    rng = np.random.RandomState(5)
    obs = rng.rand(n, W[0].shape[1])
    act = rng.randint(0, W[-1].shape[0], n)
    adv, ret = rng.randn(n), rng.randn(n)
    z = _forward(W, b, obs.astype(np.float32).astype(np.float64), np.float64)[-1]
    d = z - z.max(1, keepdims=True)
    olp = (d - np.log(np.exp(d).sum(1, keepdims=True)))[np.arange(n), act] + 0.3 * rng.randn(n)
    return dict(obs=obs, actions=act, old_log_probs=olp, advantages=adv, returns=ret)


def loss_and_grads_ld(W, b, V, c, obs, actions, old_log_probs, advantages, returns, clip_range=0.2, ent_coef=0.006, vf_coef=0.5,
                      normalize_advantage=True):
    """(a): dict of the scalars of SCALARS, clip_fraction, kink (the smallest |r - (1 +- c)|), log_probs, values and grads = (gW, gb,
    gVW, gVb), everything long double"""
    dt = LD
    n = len(obs)
    act = np.asarray(actions)
    h0 = np.asarray(obs, dtype=np.float64).astype(np.float32).astype(dt)
    adv, ret, olp = (np.asarray(x, dtype=np.float64).astype(dt) for x in (advantages, returns, old_log_probs))
    a = adv
    if normalize_advantage and n > 1:
        a = (adv - adv.mean()) / (np.sqrt(((adv - adv.mean()) ** 2).sum() / (n - 1)) + dt(1e-8))
    hp = _forward(W, b, h0, dt)
    z = hp[-1]
    d = z - z.max(1, keepdims=True)
    e = np.exp(d)
    S = e.sum(1, keepdims=True)
    p, logp = e / S, d - np.log(S)
    lp = logp[np.arange(n), act]
    lr = lp - olp
    r = np.exp(lr)
    lo, hi = dt(1) - dt(clip_range), dt(1) + dt(clip_range)
    s1, s2 = a * r, a * np.clip(r, lo, hi)
    H = -(p * logp).sum(1)
    hv = _forward(V, c, h0, dt)
    v = hv[-1][:, 0]
    pl, vl, el = -np.minimum(s1, s2).mean(), ((ret - v) ** 2).mean(), -H.mean()
    g_lp = np.where(s1 <= s2, -s1, dt(0)) / n
    onehot = np.zeros_like(p)
    onehot[np.arange(n), act] = 1
    dz = g_lp[:, None] * (onehot - p) + dt(ent_coef) / n * p * (logp + H[:, None])
    gW, gb = _backward(W, hp, dz, dt)
    gVW, gVb = _backward(V, hv, (dt(vf_coef) * 2 / n * (v - ret))[:, None], dt)
    norm = np.sqrt(sum((g * g).sum() for g in gW + gb + gVW + gVb))
    return dict(loss=pl + dt(ent_coef) * el + dt(vf_coef) * vl, policy_loss=pl, value_loss=vl, entropy_loss=el, approx_kl=((r - 1) - lr).mean(),
                grad_norm=norm, clip_fraction=float((np.abs(r - 1) > dt(clip_range)).mean()),
                kink=float(np.minimum(np.abs(r - lo), np.abs(r - hi)).min()), unclipped=float((s1 <= s2).mean()),
                log_probs=lp, values=v, grads=(gW, gb, gVW, gVb))


def loss_and_grads_torch(W, b, V, c, obs, actions, old_log_probs, advantages, returns, clip_range=0.2, ent_coef=0.006, vf_coef=0.5,
                         normalize_advantage=True):
    """(b): dict of the scalars of SCALARS and grads = (gW, gb, gVW, gVb), float64, torch CPU autograd"""
    import torch

    def leaf(x):
        return torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    Wt, bt, Vt, ct = [leaf(w) for w in W], [leaf(x) for x in b], [leaf(w) for w in V], [leaf(x) for x in c]
    h0 = torch.tensor(np.asarray(obs, dtype=np.float64).astype(np.float32).astype(np.float64))

    def f(Ws, bs):
        h = h0
        for i, (w, bb) in enumerate(zip(Ws, bs)):
            h = h @ w.T + bb
            if i + 1 < len(Ws):
                h = torch.tanh(h)
        return h
    a = torch.tensor(np.asarray(advantages, dtype=np.float64))
    if normalize_advantage and len(a) > 1:
        a = (a - a.mean()) / (a.std() + 1e-8)
    dist = torch.distributions.Categorical(logits=f(Wt, bt))
    lp = dist.log_prob(torch.tensor(np.asarray(actions, dtype=np.int64)))
    r = torch.exp(lp - torch.tensor(np.asarray(old_log_probs, dtype=np.float64)))
    pl = -torch.min(a * r, a * torch.clamp(r, 1 - clip_range, 1 + clip_range)).mean()
    vl = torch.nn.functional.mse_loss(torch.tensor(np.asarray(returns, dtype=np.float64)), f(Vt, ct)[:, 0])
    el = -dist.entropy().mean()
    loss = pl + ent_coef * el + vf_coef * vl
    loss.backward()

    def grads(xs):
        return [x.grad.numpy() for x in xs]
    with torch.no_grad():
        log_ratio = lp - torch.tensor(np.asarray(old_log_probs, dtype=np.float64))
        kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).item()
        norm = torch.norm(torch.stack([torch.norm(x.grad) for x in Wt + bt + Vt + ct])).item()          # (clip_grad_norm_'s total)
    return dict(loss=loss.item(), policy_loss=pl.item(), value_loss=vl.item(), entropy_loss=el.item(), approx_kl=kl, grad_norm=norm,
                grads=(grads(Wt), grads(bt), grads(Vt), grads(ct)))


_CACHE = {}
# the one case whose long-double reference is read from tests/golden (make_ppo_golden.py: about 20 s of long-double matrix products)
GOLDEN_CASE = ("shipped", 4096)


def _golden_ld(name, n):
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    pi, vf = (np.load(os.path.join(here, f"ppo_{name}_{n}_{tag}.npz")) for tag in ("pi", "vf"))

    def get(d, k):
        x = d[k + "_hi"].astype(LD) + d[k + "_lo"].astype(LD)
        return x if x.ndim else x[()]
    n_pi, n_vf = len(NETS[name][0]) - 1, len(NETS[name][1]) - 1
    out = {k: get(pi, k) for k in SCALARS + ("log_probs",)}
    out.update({k: float(get(pi, k)) for k in ("clip_fraction", "kink", "unclipped")})
    out["values"] = get(vf, "values")
    out["grads"] = ([get(pi, f"W{l}") for l in range(n_pi)], [get(pi, f"b{l}") for l in range(n_pi)],
                    [get(vf, f"W{l}") for l in range(n_vf)], [get(vf, f"b{l}") for l in range(n_vf)])
    return out


def references(name, n):
    """(inputs, long-double reference, torch reference) of a case, computed once per process and not to be changed"""
    if (name, n) not in _CACHE:
        inp = case(name, n)
        net = nets(name)
        ld = _golden_ld(name, n) if (name, n) == GOLDEN_CASE else loss_and_grads_ld(*net, **inp, **SETTINGS)
        _CACHE[name, n] = (inp, ld, loss_and_grads_torch(*net, **inp, **SETTINGS))
    return _CACHE[name, n]


def tensor_names(grads):
    return [f"{tag}{l}" for tag, g in zip(("pi.W", "pi.b", "vf.W", "vf.b"), grads) for l in range(len(g))]


def flat(grads):
    return [g for group in grads for g in group]


def errors(grads, ref_grads):
    """err(g) of every tensor, in units of u max |g_ld|, in the order of tensor_names"""
    out = []
    for g, r in zip(flat(grads), flat(ref_grads)):
        m = float(np.abs(r).max())
        out.append(float(np.abs(np.asarray(g).astype(LD) - r).max()) / (U * m))
    return np.array(out)


def scalar_error(x, ref):
    """|x - ref| / (u |ref|)"""
    return float(abs(LD(x) - ref) / (U * abs(ref)))


def loss_bound(ld, gates, ent_coef=0.006, vf_coef=0.5):
    """ABSOLUTE bound of the total loss computed in float64 from parts that each meet their relative gate (gates: units of u per name
    of GATED): the parts' errors weighted as the loss weights them, plus 3 roundings (two products, two sums, each at most u of a
    partial sum no larger than the sum of the terms' magnitudes)"""
    terms = [(1.0, "policy_loss"), (ent_coef, "entropy_loss"), (vf_coef, "value_loss")]
    mags = [abs(c * float(ld[k])) for c, k in terms]
    return U * (sum(m * gates[k] for m, (c, k) in zip(mags, terms)) + 3.0 * sum(mags))


def adam_ld(params, grads, m, v, t, lr, max_grad_norm, betas=(0.9, 0.999), eps=1e-5):
    """(c): lists of arrays -> (new params, m, v in long double, total norm)"""
    b1, b2 = LD(betas[0]), LD(betas[1])
    g = [np.asarray(x, dtype=np.float64).astype(LD) for x in grads]
    total = np.sqrt(sum((x * x).sum() for x in g))
    coef = min(LD(1), LD(max_grad_norm) / (total + LD(1e-6)))
    step, bc2 = LD(lr) / (1 - b1 ** t), np.sqrt(1 - b2 ** t)
    P, M, V = [], [], []
    for th, x, m0, v0 in zip(params, g, m, v):
        x = coef * x
        m1 = b1 * np.asarray(m0).astype(LD) + (1 - b1) * x
        v1 = b2 * np.asarray(v0).astype(LD) + (1 - b2) * x * x
        P.append(np.asarray(th).astype(LD) - step * m1 / (np.sqrt(v1) / bc2 + LD(eps)))
        M.append(m1); V.append(v1)
    return P, M, V, total


def near_float32_boundary(x, rel=2.0 ** -40):
    """where the long-double x lies within rel |x| of the midpoint of two neighbouring float32 values: there the rounding of a float64
    computation of x may go either way"""
    x = np.asarray(x, dtype=LD)
    f = x.astype(np.float32)
    lo = np.where(f.astype(LD) <= x, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = (lo.astype(LD) + hi.astype(LD)) / 2
    return np.abs(x - mid) <= rel * np.abs(x)
