"""
The plant of the closed loop and its state estimator once more, exactly: forward evaluation only, in mpmath at 60 digits, and the
points at which the tests compare it with the plain binary64 statement of tum_control_amd.closed_loop (tests/test_plant_reference.py)
and with plant_advance_kernel of csrc/loop_kernels.hpp (tests/test_gpu_plant_reference.py).

What is restated, from the formulas of the reference project (not from the kernel, not from closed_loop.py):
  xdot(x, a, sr)                   the 7-state single track / Pacejka plant, Vehicle_Simulator/sim_model_dynamic_stm_pacejka.py:137-196
                                   (banking terms zero): x = (px, py, yaw, vl, vt, r, delta), inputs acceleration and steering rate
  step(x, a, sr, Ts, n_elem, w)    VehicleSimulator.py:73-77: classic RK4, n_elem equal elements over Ts, inputs held; with w the
                                   right-hand side is xdot + w (simulator_step_disturbed)
  sim_step(x, a, sr, w, e)         Utils/SimulationMode_main_class.py:106-150, simMode 0: the TRUE next state is the undisturbed step;
                                   the state the estimator is fed is the disturbed step (the undisturbed one without w) plus e, with
                                   a appended as the eighth entry
  moving_average(samples, window)  StateEstimation, :152-156: the mean of the last min(window, k) of the k samples so far
Every parameter is the exact binary64 number config.default_config() holds; so are 3.6, 100, 0.5, 0.001, 0.98, Ts and the inputs.
The branch vl > 0.001 and the two clips at +-0.98 are decided on the exact quantities at every RK stage.

THE UNIT. Errors are counted in a unit per point and channel, computed here from exact quantities only, u = 2^-53:

  xdot_i   u S_i + C_i, where S_i is the sum of the absolute values of the terms xdot_i is a sum of,
               xdot_0: vl cos(yaw), vt sin(yaw)                 xdot_1: vl sin(yaw), vt cos(yaw)            xdot_2: r          xdot_6: sr
               xdot_3: a, fr Fz_r / m, Faero / m, Fy_f sin(delta) / m, Fx_f cos(delta) / m, vt r
               xdot_4: Fy_r / m, Fy_f cos(delta) / m, Fx_f sin(delta) / m, vl r
               xdot_5: lf Fy_f cos(delta) / Iz, lf Fx_f sin(delta) / Iz, lr Fy_r / Iz
           (any evaluation that rounds every operation once errs by a small multiple of u S_i when its operands are well conditioned),
           and C_i is the conditioning a sum of absolute values cannot see: an intermediate quantity that is itself a sum, whose
           rounding reaches xdot_i through a steep function. There are two per axle.
             The slip angle: alpha_f = delta - atan(q_f), q_f = (vt + lf r) / vl; alpha_r = atan(q_r), q_r = (lr r - vt) / vl. Its own
             rounding unit is ua_f = u (|delta| + |atan q_f| + (|vt| + |lf r|) / (|vl| (1 + q_f^2))) -- the difference of two angles, and the
             numerator of q, a sum of two terms, carried through atan' -- and ua_r = u (|atan q_r| + (|lr r| + |vt|) / (|vl| (1 + q_r^2))).
             The tyre force is steep in alpha (B C D = 2e5 .. 4e5 N / rad).
             The friction-circle argument: G = Fx / Fmax with Fx_r = m a - fr Fz_r, a sum, unit ug_r = u (|m a| + |fr Fz_r|) / Fmax_r
             (ug_f = u |Fx_f| / Fmax_f); cos(asin(G)) = sqrt(1 - G^2) has the slope G / sqrt(1 - G^2), 4.9 next to the clip. A clipped G
             is the constant 0.98: no term.
           C_i = sum over the axles of |d xdot_i / d alpha| ua + |d xdot_i / d G| ug, the derivatives by differences at the working
           precision (a step of 1e-25: truncation far below binary64), composed over the last, linear step (xdot is linear in Fy_f, Fy_r).
  state after a step
           sum over the elements of  u |x_i| + h max over the four stages of unit(xdot_i) (+ u h |w_i| with a disturbance),  |x_i| the larger of the
           element's two ends: the roundings of x + h / 6 (...) and what the stage evaluations contribute. The unit does NOT carry the
           amplification of a stage's error by the following stages (h times the Jacobian): the gates are built from the plain
           statement's measured error, which suffers it alike, and that stays below 4 units on every point at every step used here.
  fed state  unit of the (disturbed) step + u |fed_i| (one more sum)
  estimator  u (sum of |samples| in the window) / count

THE DEVICE TERM. The plain statement calls libm (one ulp); the kernel calls fast_atan, fast_sincos and fast_sqrt_pos, held by
tests/test_gpu_model_reference.py to 2.5 ulp, 3 ulp + |n| delta and 1 ulp. The `dev` entry of xdot(..., dev=True) is, per channel, the sum over the twelve
results of those primitives in one evaluation (three atan per axle, the sine of the magic formula per axle, sin / cos of yaw and of
delta; the root's contract is libm's: nothing) of |d xdot_i / d result| ((contract - 1) ulp(result) + |n| delta), derivatives by
differences as above. For a step: h times the largest over the stages, summed over the elements.

THE POINTS (points()): six classes, each once with px = py = 0 and a small yaw ("near": the position and yaw channels show errors
of the increment) and once with positions of order 1e3 and |yaw| of 20 .. 100 rad of both signs ("far": inside +-1e5, on which
test_fast_sincos holds fast_sincos). raceline; slip_f*_r*: every pair of ranges of fast_atan's argument B alpha on both axles; accel: a
from -13 to 13 m/s^2 with the rear G clipped low, unclipped on both sides of zero and next to either clip, clipped high; lowspeed: vl
exactly 0.001, exactly 0, negative (with a < 0: the point stays at rest; with a > 0: the later stages cross into the moving branch at a
huge slip angle) and slightly above 0.001 with |vt| of order 1 (a huge slip angle, where the model is not stiff: the force is
saturated and d alpha / d vt = vl / vt^2); steer: delta at either bound; straight: everything but vl zero.
No point is set aside anywhere. KINK_MARGIN as in model_reference.py: a COMPUTED vl (every stage but the first of the first element)
keeps a relative distance of KINK_MARGIN from 0.001, |G| from 0.98, at every stage of every point with every step the tests use; the
first evaluation compares the caller's own binary64 input with 0.001, which every statement decides alike.
"""
import functools
import math

import mpmath as mp
import numpy as np

DPS = 60
U53 = 2.0 ** -53
VL_THR = 0.001
CLIP = 0.98
KINK_MARGIN = 1e-9
TS, N_ELEM = 0.02, 4
D_STEP = "1e-25"
ATAN_SEAMS = (math.tan(math.pi / 8), math.tan(3 * math.pi / 8))
# contract of the device primitive minus libm's one ulp, in ulp of the result (tests/test_gpu_model_reference.py)
EXTRA_ULP = dict(atan=1.5, sincos=2.0)


def config_numbers():
    from tum_control_amd import config
    c = config.default_config()
    d = {k: float(c["veh"][k]) for k in ("lf", "lr", "m", "Iz", "ro", "S", "Cd", "delta_f_min", "delta_f_max")}
    d.update({k: float(c["tire"][k]) for k in ("Bf", "Cf", "Df", "Ef", "Br", "Cr", "Dr", "Er")})
    d.update({k: float(c["phys"][k]) for k in ("g", "fr0", "fr1", "fr4")})
    return d


def _params():
    """the parameters as exact numbers at the working precision (call inside workdps)"""
    P = {k: mp.mpf(v) for k, v in config_numbers().items()}
    P["Fz_f"] = P["m"] * P["lr"] * P["g"] / (P["lf"] + P["lr"])
    P["Fz_r"] = P["m"] * P["lf"] * P["g"] / (P["lf"] + P["lr"])
    P["Fmax_f"] = mp.sqrt(P["Fz_f"] ** 2 + (P["Cf"] * P["Fz_f"]) ** 2)
    P["Fmax_r"] = mp.sqrt(P["Fz_r"] ** 2 + (P["Cr"] * P["Fz_r"]) ** 2)
    P["ka"] = mp.mpf(0.5) * P["ro"] * P["S"] * P["Cd"]
    return P


def _mpv(v):
    return [t if isinstance(t, mp.mpf) else mp.mpf(float(t)) for t in v]


def _tyre(B, C, D, E, alpha, G, bump=None):
    """Fy = D sin(C atan(B alpha - E (B alpha - atan(B alpha)))) sqrt(1 - G^2); bump = (name, d) adds d to one primitive's result"""
    nm, d = bump if bump else (None, 0)
    xx = B * alpha
    at1 = mp.atan(xx) + (d if nm == "atan_x" else 0)
    inner = xx - E * (xx - at1)
    th = mp.atan(inner) + (d if nm == "atan_in" else 0)
    sn = mp.sin(C * th) + (d if nm == "sin" else 0)
    return D * sn * mp.sqrt(1 - G * G), dict(atan_x=at1, atan_in=th, sin=sn, xx=xx, inner=inner, arg=C * th)


def _assemble(P, x, a, sr, Fx_f, fr, Fy_f, Fy_r, sy, cy, sd, cd):
    """xdot from the forces and the four sines: the last, linear step; also the terms of every channel"""
    vl, vt, r = x[3], x[4], x[5]
    m, Iz, lf, lr = P["m"], P["Iz"], P["lf"], P["lr"]
    terms = [[vl * cy, -vt * sy], [vl * sy, vt * cy], [r],
             [a, -fr * P["Fz_r"] / m, -P["ka"] * vl * vl / m, -Fy_f * sd / m, Fx_f * cd / m, vt * r],
             [Fy_r / m, Fy_f * cd / m, Fx_f * sd / m, -vl * r],
             [lf * Fy_f * cd / Iz, lf * Fx_f * sd / Iz, -lr * Fy_r / Iz],
             [sr]]
    return [mp.fsum(t) for t in terms], [mp.fsum(abs(v) for v in t) for t in terms]


def _xdot(P, x, a, sr, first=True, detail=False, want_dev=True):
    """xdot (7 mpf) at x (7 mpf) and a record of the evaluation: the quantities the kink margin is checked on; with detail the unit and
    the device term of every channel. first: vl is the caller's own input (module docstring)."""
    yaw, vl, vt, r, de = x[2], x[3], x[4], x[5], x[6]
    v = mp.sqrt(vl * vl + vt * vt) * mp.mpf(3.6)
    w = v / 100
    fr = P["fr0"] + P["fr1"] * w + P["fr4"] * w ** 4
    Fx_f = -fr * P["Fz_f"]
    Fx_r = P["m"] * a - fr * P["Fz_r"]
    moving = bool(vl > mp.mpf(VL_THR))
    if moving:
        q_f, q_r = (vt + P["lf"] * r) / vl, (P["lr"] * r - vt) / vl
        at_f, at_r = mp.atan(q_f), mp.atan(q_r)
        al_f, al_r = de - at_f, at_r
    else:
        q_f = q_r = at_f = at_r = al_f = al_r = mp.mpf(0)
    c = mp.mpf(CLIP)
    g_f, g_r = Fx_f / P["Fmax_f"], Fx_r / P["Fmax_r"]
    clip_f, clip_r = (1 if g_f > c else (-1 if g_f < -c else 0)), (1 if g_r > c else (-1 if g_r < -c else 0))
    G_f, G_r = (clip_f * c if clip_f else g_f), (clip_r * c if clip_r else g_r)
    tf, tr = (P["Bf"], P["Cf"], P["Df"], P["Ef"]), (P["Br"], P["Cr"], P["Dr"], P["Er"])
    Fy_f, inf_f = _tyre(*tf, al_f, G_f)
    Fy_r, inf_r = _tyre(*tr, al_r, G_r)
    sy, cy, sd, cd = mp.sin(yaw), mp.cos(yaw), mp.sin(de), mp.cos(de)
    xd, S = _assemble(P, x, a, sr, Fx_f, fr, Fy_f, Fy_r, sy, cy, sd, cd)
    rec = dict(moving=moving, clip_f=clip_f, clip_r=clip_r, g_f=g_f, g_r=g_r, vl=vl, first=first,
               q_f=q_f, q_r=q_r, xx_f=inf_f["xx"], xx_r=inf_r["xx"], in_f=inf_f["inner"], in_r=inf_r["inner"])
    if not detail:
        return xd, rec
    d = mp.mpf(D_STEP)
    lin = lambda **kw: _assemble(P, x, a, sr, Fx_f, fr, **{**dict(Fy_f=Fy_f, Fy_r=Fy_r, sy=sy, cy=cy, sd=sd, cd=cd), **kw})[0]
    dof = lambda xs: [abs(p - q) / d for p, q in zip(xs, xd)]          # |d xdot_i / d (what was moved by d)|
    by_Fy = dict(f=[abs(p - q) for p, q in zip(lin(Fy_f=Fy_f + 1), xd)], r=[abs(p - q) for p, q in zip(lin(Fy_r=Fy_r + 1), xd)])   # (linear: exact)
    u = mp.mpf(U53)
    unit = [u * s for s in S]
    dev = [mp.mpf(0)] * 7
    pi_half_delta = SINCOS_DELTA[0]

    def extra(kind, result, arg=None):
        e = mp.mpf(EXTRA_ULP[kind]) * ulp_of(result)
        if kind == "sincos":
            e += abs(mp.nint(2 * arg / mp.pi)) * pi_half_delta
        return e
    for ax, tp, al, G, clip, Fy, inf, at, q in (("f", tf, al_f, G_f, clip_f, Fy_f, inf_f, at_f, q_f), ("r", tr, al_r, G_r, clip_r, Fy_r, inf_r, at_r, q_r)):
        coef = by_Fy[ax]
        dFy = lambda **kw: abs(_tyre(*tp, kw.get("alpha", al), kw.get("G", G), kw.get("bump"))[0] - Fy) / d
        if moving:
            lever = P["lf"] if ax == "f" else P["lr"]
            ua = u * ((abs(de) if ax == "f" else 0) + abs(at) + (abs(vt) + abs(lever * r)) / (abs(vl) * (1 + q * q)))
            s_al = dFy(alpha=al + d)
            unit = [t + cf * s_al * ua for t, cf in zip(unit, coef)]
            if want_dev:
                dev = [t + cf * s_al * extra("atan", at) for t, cf in zip(dev, coef)]
        if not clip:
            Fx = Fx_f if ax == "f" else Fx_r
            ug = u * ((abs(Fx) if ax == "f" else abs(P["m"] * a) + abs(fr * P["Fz_r"])) / P["Fmax_" + ax])
            s_G = dFy(G=G + d)
            unit = [t + cf * s_G * ug for t, cf in zip(unit, coef)]
        for nm, kind in (("atan_x", "atan"), ("atan_in", "atan"), ("sin", "sincos")) if want_dev else ():
            s = dFy(bump=(nm, d))
            e = extra(kind, inf[nm], inf["arg"])
            dev = [t + cf * s * e for t, cf in zip(dev, coef)]
    for nm, val, arg in (("sy", sy, yaw), ("cy", cy, yaw), ("sd", sd, de), ("cd", cd, de)) if want_dev else ():
        s = dof(lin(**{nm: val + d}))
        e = extra("sincos", val, arg)
        dev = [t + si * e for t, si in zip(dev, s)]
    rec["unit"], rec["dev"] = unit, dev
    return xd, rec


# |pi / 2 - hi - lo| of fast_sincos's two-constant reduction: set by the GPU tests from the header's own literals (set_sincos_delta);
# the CPU tests never use the device term
SINCOS_DELTA = [mp.mpf(0)]


def set_sincos_delta(hi, lo):
    with mp.workdps(DPS):
        SINCOS_DELTA[0] = abs(mp.pi / 2 - mp.mpf(hi) - mp.mpf(lo))
    _step_cached.cache_clear(); _xdot_cached.cache_clear()


def ulp_of(v):
    """one unit in the last place of binary64 at the magnitude of the exact value v"""
    a = abs(v)
    if a == 0:
        return mp.mpf(2) ** -1074
    e = a.man.bit_length() + a.exp - 1
    return mp.mpf(2) ** max(e - 52, -1074)


def _kinks(rec):
    """relative distances of the computed quantities of one evaluation from their kinks"""
    out = [abs(abs(rec["g_f"]) - CLIP) / CLIP, abs(abs(rec["g_r"]) - CLIP) / CLIP]
    if not rec["first"]:
        out.append(abs(rec["vl"] - mp.mpf(VL_THR)) / mp.mpf(VL_THR))
    return float(min(out))


def _tup(x):
    return tuple(float(v) for v in x)


@functools.lru_cache(maxsize=None)
def _xdot_cached(x, a, sr, dev):
    with mp.workdps(DPS):
        P = _params()
        xd, rec = _xdot(P, _mpv(x), mp.mpf(a), mp.mpf(sr), True, True, dev)
        return dict(value=xd, unit=[float(t) for t in rec["unit"]], dev=[float(t) for t in rec["dev"]], margin=_kinks(rec), rec=rec)


def xdot(x, a, sr, dev=False):
    """dict: value (7 mpf), unit (7 floats), dev (7 floats: the device term, zeros unless asked for), margin (float), rec (the evaluation's record)"""
    return _xdot_cached(_tup(x), float(a), float(sr), bool(dev))


@functools.lru_cache(maxsize=None)
def _step_cached(x, a, sr, Ts, n_elem, w, want_dev):
    with mp.workdps(DPS):
        P = _params()
        x, a, sr = _mpv(x), mp.mpf(a), mp.mpf(sr)
        wv = _mpv(w) if w is not None else [mp.mpf(0)] * 7
        h = mp.mpf(Ts) / n_elem
        u = mp.mpf(U53)
        unit, dev, margin, recs = [mp.mpf(0)] * 7, [mp.mpf(0)] * 7, 1.0, []
        for el in range(n_elem):
            ks, su, sdv, t = [], [mp.mpf(0)] * 7, [mp.mpf(0)] * 7, x
            for st, ci in enumerate((0, mp.mpf(0.5), mp.mpf(0.5), 1)):
                if st:
                    t = [p + ci * h * q for p, q in zip(x, ks[-1])]
                k, rec = _xdot(P, t, a, sr, first=(el == 0 and st == 0), detail=True, want_dev=want_dev)
                ks.append([p + q for p, q in zip(k, wv)])
                su = [max(p, q) for p, q in zip(su, rec["unit"])]
                sdv = [max(p, q) for p, q in zip(sdv, rec["dev"])]
                margin = min(margin, _kinks(rec))
                recs.append({kk: rec[kk] for kk in ("moving", "clip_f", "clip_r")})
            xn = [p + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4) for p, k1, k2, k3, k4 in zip(x, *ks)]
            unit = [t + u * max(abs(p), abs(q)) + h * (s + u * abs(ww)) for t, p, q, s, ww in zip(unit, x, xn, su, wv)]
            dev = [t + h * s for t, s in zip(dev, sdv)]
            x = xn
        return dict(value=x, unit=[float(t) for t in unit], dev=[float(t) for t in dev], margin=margin, stages=recs)


def step(x, a, sr, Ts=TS, n_elem=N_ELEM, w=None, dev=False):
    """dict: value (7 mpf: the state after Ts), unit, dev (7 floats each; dev zeros unless asked for), margin (smallest kink distance over
    the stages), stages"""
    return _step_cached(_tup(x), float(a), float(sr), float(Ts), int(n_elem), None if w is None else _tup(w), bool(dev))


def sim_step(x, a, sr, w=None, e=None, Ts=TS, n_elem=N_ELEM, dev=False):
    """(true, fed): the step dict of the undisturbed step, and a dict value (8 mpf), unit, dev (8 floats) of the state the estimator is fed"""
    true = step(x, a, sr, Ts, n_elem, None, dev)
    dist = true if w is None else step(x, a, sr, Ts, n_elem, w, dev)
    with mp.workdps(DPS):
        val, unit = list(dist["value"]), list(dist["unit"])
        if e is not None:
            val = [p + mp.mpf(float(q)) for p, q in zip(val, e)]
            unit = [t + U53 * float(abs(p)) for t, p in zip(unit, val)]
        val.append(mp.mpf(float(a)))
    return true, dict(value=val, unit=unit + [0.0], dev=list(dist["dev"]) + [0.0], margin=min(true["margin"], dist["margin"]))


def moving_average(samples, window):
    """(exact mean (mpf) of the last min(window, k) of the k binary64 samples, its unit u (sum of |samples|) / count)"""
    s = [float(v) for v in samples][-int(window):]
    with mp.workdps(DPS):
        return mp.fsum(mp.mpf(v) for v in s) / len(s), U53 * float(mp.fsum(abs(mp.mpf(v)) for v in s)) / len(s)


def errors(got, exact, unit):
    """|got - exact| / unit per entry (binary64 got, mpf exact); 0 where equal, inf where a unit of 0 is missed"""
    out = np.zeros(len(exact))
    with mp.workdps(DPS):
        for i, (g, e, t) in enumerate(zip(got, exact, unit)):
            g = float(g)
            err = abs(mp.mpf(g) - e) if math.isfinite(g) else mp.inf
            out[i] = 0.0 if err == 0 else (float(err / mp.mpf(t)) if t > 0 else math.inf)
    return out


def errors_mod_2pi(got, exact, unit, channel=2):
    """errors() with one channel compared modulo 2 pi (the logs keep the yaw wrapped)"""
    out = errors(got, exact, unit)
    with mp.workdps(DPS):
        d = mp.mpf(float(got[channel])) - exact[channel]
        d -= 2 * mp.pi * mp.nint(d / (2 * mp.pi))
        out[channel] = 0.0 if d == 0 else float(abs(d) / mp.mpf(unit[channel]))
    return out


# ---------------------------------------------------------------------------------------------- the points
CLASSES = ("raceline", "slip", "accel", "lowspeed", "steer", "straight")
# The larger step of the GPU tests, one element: Ts_MPC, the largest of the candidates 0.04, 0.05, 0.06, 0.08, 0.1 tried on the CPU. With it
# h |xdot_i| is 0.63 |vt| and 0.34 |r| in the median over the points (0.21 and 0.09 at the shipped 0.02 / 1: an error of xdot then shows in
# the velocity states at the level of their own ulp), and the plain statement's largest error stays at 1.5 units, as at every
# candidate: no amplification by the stages yet (profiles/plant_bounds.txt has the table; tests/test_plant_reference.py asserts both).
LARGE_TS = 0.08
STEPS = ((TS, N_ELEM), (TS, 1), (LARGE_TS, 1))


def slip_class(v):
    v = abs(float(v))
    return "small" if v <= ATAN_SEAMS[0] else ("mid" if v <= ATAN_SEAMS[1] else "big")


def _a_for_gr(g, vl, vt, c):
    """a that puts the rear G at g (binary64: only to aim; the generator checks the exact model)"""
    Fz_r = c["m"] * c["lf"] * c["g"] / (c["lf"] + c["lr"])
    w = math.hypot(vl, vt) * 3.6 / 100
    fr = c["fr0"] + c["fr1"] * w + c["fr4"] * w ** 4
    return (g * Fz_r * math.sqrt(1 + c["Cr"] ** 2) + fr * Fz_r) / c["m"]


def _x1(x, c):
    vl, vt, r, de = x[3], x[4], x[5], x[6]
    return c["Bf"] * (de - math.atan((vt + c["lf"] * r) / vl)), c["Br"] * math.atan((c["lr"] * r - vt) / vl)


@functools.lru_cache(maxsize=None)
def points(seed=90210):
    """dict of read-only arrays: X (P, 7), A (P,), SR (P,), W (P, 7), E (P, 7) and tuples label, cls, variant (P each). Deterministic."""
    rng = np.random.default_rng(seed)
    c = config_numbers()
    X, A, SR, L, C, V = [], [], [], [], [], []

    def pose(variant, k):
        if variant == "near":
            return [0.0, 0.0, rng.uniform(-0.3, 0.3)]
        return [rng.uniform(400, 2500) * rng.choice([-1, 1]), rng.uniform(400, 2500) * rng.choice([-1, 1]), rng.uniform(20, 100) * (1 if k % 2 == 0 else -1)]

    def race(variant, k):
        return pose(variant, k) + [rng.uniform(6, 60), rng.normal(0, 0.3), rng.normal(0, 0.1), rng.normal(0, 0.03)], rng.uniform(-3, 2.5), rng.normal(0, 0.1)

    def add(cls, label, variant, x, a, sr):
        X.append(np.array(x, dtype=np.float64)); A.append(float(a)); SR.append(float(sr)); L.append(label); C.append(cls); V.append(variant)

    for variant in ("near", "far"):
        for k in range(10):
            add("raceline", "raceline", variant, *race(variant, k))
        k = 0
        for cf in ("small", "mid", "big"):
            for cr in ("small", "mid", "big"):
                while True:
                    x, a, sr = race(variant, k)
                    x[3] = rng.uniform(5, 30); x[4] = rng.uniform(-0.6, 0.6) * x[3]; x[5] = rng.uniform(-1.5, 1.5); x[6] = rng.uniform(-0.6, 0.6)
                    if cf == cr == "small":
                        x[4] = rng.normal(0, 0.02); x[5] = rng.normal(0, 0.02); x[6] = rng.normal(0, 0.01)
                    f, r = _x1(x, c)
                    if slip_class(f) == cf and slip_class(r) == cr:
                        break
                add("slip", f"slip_f{cf}_r{cr}", variant, x, a, sr); k += 1
        for k, (lab, g) in enumerate((("gr_clip_low", -1.4), ("gr_clip_low", -1.05), ("gr_inside_low", -0.97), ("gr_inside_low", -0.9),
                                      ("gr_mid", -0.4), ("gr_mid", 0.3), ("gr_inside_high", 0.9), ("gr_inside_high", 0.97),
                                      ("gr_clip_high", 1.05), ("gr_clip_high", 1.4))):
            x, _, sr = race(variant, k)
            add("accel", lab, variant, x, _a_for_gr(g * rng.uniform(0.995, 1.0), x[3], x[4], c), sr)
        k = 0
        for lab, vl in (("vl_at_thr", 0.001), ("vl_zero", 0.0), ("vl_negative", -0.002), ("vl_above_thr", 0.0011)):
            for sgn in (1.0, -1.0):
                x, _, sr = race(variant, k)
                x[3] = vl; x[4] = sgn * rng.uniform(0.7, 1.4); x[5] = sgn * rng.uniform(0.05, 0.3); x[6] = rng.normal(0, 0.1)
                # at rest with a < 0 the point stays at rest; with a > 0 (and always above the threshold) the stages move at a huge slip angle
                a = rng.uniform(1.5, 3.0) if (sgn > 0 or lab == "vl_above_thr") else -rng.uniform(1.5, 3.0)
                add("lowspeed", lab, variant, x, a, sr); k += 1
        for k, (lab, de) in enumerate((("steer_max", c["delta_f_max"]), ("steer_min", c["delta_f_min"])) * 2):
            x, a, sr = race(variant, k)
            x[3] = rng.uniform(6, 25); x[6] = de
            add("steer", lab, variant, x, a, math.copysign(abs(sr), de) if k < 2 else -math.copysign(abs(sr), de))
        for k, vl in enumerate((12.0, 47.5)):
            p = pose(variant, k) if variant == "far" else [0.0, 0.0, 0.0]
            add("straight", "straight", variant, p + [vl, 0.0, 0.0, 0.0], 0.0, 0.0)
    P = len(L)
    sim = np.array([0.8, 0.8, 0.1, 1.1, 0.1, 0.05, 0.1])          # the shipped magnitudes of the derivative disturbance ...
    est = np.array([0.15, 0.15, 0.01, 0.8, 0.35, 0.05, 0.005])    # ... and of the state estimation error (Config/EDGAR/sim_main_params.yaml:44-80)
    out = dict(X=np.array(X), A=np.array(A), SR=np.array(SR), W=rng.uniform(-1, 1, (P, 7)) * sim, E=rng.normal(0, 1, (P, 7)) * est)
    for v in out.values():
        v.setflags(write=False)
    out.update(label=tuple(L), cls=tuple(C), variant=tuple(V))
    return out


def groups():
    """the (class, variant) group of every point: the granularity of the gates"""
    p = points()
    return [f"{c}/{v}" for c, v in zip(p["cls"], p["variant"])]
