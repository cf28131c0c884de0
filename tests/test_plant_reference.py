"""
The exact statement of the plant and the estimator (tests/plant_reference.py) against (1) the plant states the reference project
logged, (2) the plain binary64 statement tum_control_amd.closed_loop.plant_xdot / plant_step / MovingAverageEstimator on every point,
and the points themselves: classes, branches, kink margin, nothing set aside. The GPU half is tests/test_gpu_plant_reference.py; it
takes `plain_errors` and `gate_units` from here.

Errors are counted in the units of plant_reference (its docstring). Gates:
  LOG_GATE     the logs: max(32, the largest error measured) rounded up once. The logged states are CasADi's binary64 RK4 of the same
               formulas, so the comparison carries that integrator's own rounding: measured 1.56 units (lvms step 1800, yaw) -> 32.
  PLAIN_GATE   the plain statement: 16 units. Every operation rounds once and libm's functions are good to an ulp; the unit weighs each
               rounding of a term, of a slip angle and of a friction-circle argument with at most one unit, and the longest chain
               from an input to a channel (slip angle, three nested functions of the magic formula, friction circle, force balance)
               has a dozen of them. Measured: 3.0 (xdot), 1.5 (steps), 0.98 (fed state), 1.96 (estimator).
  device       gate_units: max(32, 4 x the plain statement's largest error in the point's class / variant group and channel), plus
               plant_reference's device term (absolute) -- the rule of the condensing, SNMPC, GP and PPO tests.
Run as a script it prints the plain statement's half of profiles/plant_bounds.txt.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import plant_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROBE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device", "plant_probe.hip")
LOG_GATE = 32.0          # measured: 1.56
PLAIN_GATE = 16.0
FLOOR = 32.0
WINDOW_SETS = dict(ones=(1,) * 8, shipped=(1, 1, 4, 2, 2, 3, 4, 2), mixed=(1, 2, 3, 4, 2, 3, 4, 1))
# the disturbance cases of sim_step: (w, e, control step index past the realisation's length)
CASES = dict(none=(False, False, False), w=(True, False, False), e=(False, True, False), we=(True, True, False), past=(True, True, True))


def _cfg():
    from tum_control_amd import config
    return config.default_config()


def case_inputs(case):
    """(W, E) (P, 7) arrays or None of a disturbance case, as the loop applies them"""
    p = pr.points()
    w, e, past = CASES[case]
    return (p["W"] if w and not past else None), (p["E"] if e and not past else None)


@functools.lru_cache(maxsize=None)
def plain_errors(kind, Ts=pr.TS, n_elem=pr.N_ELEM, case="none"):
    """(P, channels) errors of the plain binary64 statement in units, on all points: kind 'xdot', 'step' (with the derivative
    disturbance of the points when case has one), 'fed' (the state the estimator is fed: 8 channels)"""
    from tum_control_amd import closed_loop as cl
    p, cfg = pr.points(), _cfg()
    X, A, SR = p["X"], p["A"], p["SR"]
    n = len(A)
    if kind == "xdot":
        got = cl.plant_xdot(X.copy(), A, SR, cfg)
        ref = [pr.xdot(X[i], A[i], SR[i]) for i in range(n)]
    else:
        W, E = case_inputs(case)
        got = cl.plant_step(X.copy(), A, SR, cfg, Ts=Ts, n_elem=n_elem, w=W)
        if kind == "step":
            ref = [pr.step(X[i], A[i], SR[i], Ts, n_elem, None if W is None else W[i]) for i in range(n)]
        else:
            if E is not None:
                got = got + E
            got = np.concatenate([got, A[:, None]], axis=1)
            ref = [pr.sim_step(X[i], A[i], SR[i], None if W is None else W[i], None if E is None else E[i], Ts, n_elem)[1] for i in range(n)]
    out = np.array([pr.errors(got[i], ref[i]["value"], ref[i]["unit"]) for i in range(n)])
    out.setflags(write=False)
    return out


def estimator_sequences(steps=7):
    """(steps, P, 8) samples: the points' states drifting along their own disturbance direction, the input a as the eighth entry"""
    p = pr.points()
    k = np.arange(steps)[:, None, None]
    return np.concatenate([p["X"][None] + 0.02 * k * p["W"][None] + 0.003 * (k % 3) * p["E"][None], np.broadcast_to(p["A"][None, :, None] * (1 + 0.1 * k), (steps, len(p["A"]), 1))], axis=2)


@functools.lru_cache(maxsize=None)
def plain_estimator_errors(name):
    """(steps, P, 8) errors in units of MovingAverageEstimator with the windows WINDOW_SETS[name]"""
    from tum_control_amd import closed_loop as cl
    S = estimator_sequences()
    keep = cl.WINDOWS
    cl.WINDOWS = WINDOW_SETS[name]
    try:
        est = cl.MovingAverageEstimator(S.shape[1])
        got = np.array([est(S[k].copy()) for k in range(len(S))])
    finally:
        cl.WINDOWS = keep
    out = np.zeros(S.shape)
    for k in range(S.shape[0]):
        for b in range(S.shape[1]):
            ex = [pr.moving_average(S[:k + 1, b, i], WINDOW_SETS[name][i]) for i in range(8)]
            out[k, b] = pr.errors(got[k, b], [e[0] for e in ex], [e[1] for e in ex])
    return out


def gate_units(plain):
    """(P, channels) gates in units from the plain statement's errors (P, channels): max(32, 4 x the largest of the point's group)"""
    g = np.array(pr.groups())
    out = np.zeros(plain.shape)
    for name in set(g):
        m = g == name
        out[m] = np.maximum(FLOOR, 4.0 * plain[m].max(axis=0))
    return out


# ---------------------------------------------------------------------------------------------- the logs
def _logged_steps():
    """(x, a, sr, x_next, tag) of a subsample of the plant steps the reference project logged"""
    out = []
    g = np.load(os.path.join(GOLDEN, "log_file_lvms_3.npz"))
    C, S, Uu = g["CiLX"], g["MPC_SimX"], g["simU"]
    for k in range(0, len(Uu), 90):
        out.append((C[k], S[k + 1][7], Uu[k][1], C[k + 1], f"lvms step {k}"))
    g = np.load(os.path.join(GOLDEN, "closed_loop_monteblanco_150.npz"))
    C, S, Uu = g["CiLX"], g["MPC_SimX"], g["simU"]
    for b in range(0, C.shape[0], 2):
        for k in range(b % 7, Uu.shape[1], 37):
            out.append((C[b, k], S[b, k + 1][7], Uu[b, k][1], C[b, k + 1], f"monteblanco loop {b} step {k}"))
    return out


def test_reference_steps_reproduce_the_logged_plant_states():
    """step(CiLX[k], MPC_SimX[k + 1][7], simU[k][1], 0.02, 4) = CiLX[k + 1] within LOG_GATE units, yaw modulo 2 pi: the indexing and
    the formulas against CasADi's integrator"""
    worst, at = 0.0, None
    steps = _logged_steps()
    for x, a, sr, xn, tag in steps:
        r = pr.step(x, a, sr, 0.02, 4)
        e = pr.errors_mod_2pi(xn, r["value"], r["unit"])
        if e.max() > worst:
            worst, at = float(e.max()), (tag, int(e.argmax()))
    print(f"plant_bounds logs: {len(steps)} logged steps, largest error {worst:.3f} units at {at}; gate {LOG_GATE}")
    assert len(steps) > 100 and worst <= LOG_GATE, (worst, at)


# ---------------------------------------------------------------------------------------------- the points
def test_points_reach_every_class_and_branch_with_nothing_set_aside():
    p = pr.points()
    n = len(p["label"])
    assert 60 <= n <= 400
    for cls in pr.CLASSES:
        for variant in ("near", "far"):
            assert any(c == cls and v == variant for c, v in zip(p["cls"], p["variant"])), (cls, variant)
    near, far = [np.array([v == t for v in p["variant"]]) for t in ("near", "far")]
    assert (p["X"][near, :2] == 0).all() and (np.abs(p["X"][near, 2]) <= 0.3).all()
    assert (np.abs(p["X"][far, :2]) >= 100).all() and np.abs(p["X"][far, 2]).max() <= 100 and (p["X"][far, 2] > 15).any() and (p["X"][far, 2] < -15).any()
    seen = {k: set() for k in ("q_f", "q_r", "xx_f", "xx_r", "in_f", "in_r")}
    checked = 0
    for i in range(n):
        lab, x = p["label"][i], p["X"][i]
        rec = pr.xdot(x, p["A"][i], p["SR"][i])["rec"]
        if rec["moving"]:
            for k in seen:
                seen[k].add(pr.slip_class(rec[k]))
        if lab.startswith("slip_"):
            cf, cr = lab.split("_")[1][1:], lab.split("_")[2][1:]
            assert rec["moving"] and pr.slip_class(rec["xx_f"]) == cf and pr.slip_class(rec["xx_r"]) == cr, lab
        elif lab.startswith("gr_"):
            assert rec["clip_r"] == dict(gr_clip_low=-1, gr_clip_high=1).get(lab, 0), lab
            if "inside" in lab:
                assert 0.85 < abs(float(rec["g_r"])) < 0.98
        elif lab.startswith("vl_"):
            assert x[3] == dict(vl_at_thr=0.001, vl_zero=0.0, vl_negative=-0.002, vl_above_thr=0.0011)[lab]
            assert rec["moving"] == (lab == "vl_above_thr")
            stages = pr.step(x, p["A"][i], p["SR"][i])["stages"]
            assert any(s["moving"] for s in stages) == (lab == "vl_above_thr" or p["A"][i] > 0), lab
            if lab == "vl_above_thr":
                assert abs(float(rec["q_f"])) > 500
        elif lab.startswith("steer_"):
            c = pr.config_numbers()
            assert x[6] == (c["delta_f_max"] if lab == "steer_max" else c["delta_f_min"])
        elif lab == "straight":
            assert (x[4:] == 0).all() and p["A"][i] == 0 and p["SR"][i] == 0 and x[3] > 0
        checked += 1
    assert checked == n          # nothing set aside
    # fast_atan's three ranges at its three call sites per axle. The third argument, B al - E (B al - atan(B al)) with E = 0.97, stays below
    # 0.03 B |al| + 0.97 pi / 2 < 2.2 for every slip angle there is (|al| < pi / 2 + 0.62): it cannot reach the last range (> 2.414).
    assert all(seen[k] == {"small", "mid", "big"} for k in ("q_f", "q_r", "xx_f", "xx_r")) and all(seen[k] == {"small", "mid"} for k in ("in_f", "in_r")), seen
    labels = set(p["label"])
    assert {"gr_clip_low", "gr_inside_low", "gr_mid", "gr_inside_high", "gr_clip_high", "vl_at_thr", "vl_zero", "vl_negative", "vl_above_thr",
            "steer_max", "steer_min", "straight", "raceline"} <= labels
    for variant, sel in (("near", near), ("far", far)):
        assert len({p["label"][i] for i in np.flatnonzero(sel)}) == len(labels), variant


def test_kink_margin_at_every_stage_of_every_step_used():
    p = pr.points()
    worst, count = 1.0, 0
    for Ts, ne in pr.STEPS:
        for i in range(len(p["A"])):
            for w in ((None, p["W"][i]) if (Ts, ne) == (pr.TS, pr.N_ELEM) else (None,)):
                worst = min(worst, pr.step(p["X"][i], p["A"][i], p["SR"][i], Ts, ne, w)["margin"]); count += 1
    print(f"plant_bounds kink margin: smallest relative distance {worst:.3e} over {count} steps (margin {pr.KINK_MARGIN:g}); 0 points set aside")
    assert worst > pr.KINK_MARGIN and count == len(p["A"]) * (len(pr.STEPS) + 1)


# ---------------------------------------------------------------------------------------------- the plain binary64 statement
def _by_group(err):
    g = np.array(pr.groups())
    return {name: err[g == name].max(axis=0) for name in sorted(set(g))}


def test_plain_xdot_against_the_exact_statement():
    e = plain_errors("xdot")
    print("plant_bounds plain xdot largest error in units per channel", np.round(e.max(axis=0), 3))
    assert np.isfinite(e).all() and e.max() <= PLAIN_GATE, (e.max(), pr.points()["label"][int(e.max(axis=1).argmax())])


@pytest.mark.parametrize("Ts,n_elem", pr.STEPS)
def test_plain_step_against_the_exact_statement(Ts, n_elem):
    for case in (("none", "w") if (Ts, n_elem) == (pr.TS, pr.N_ELEM) else ("none",)):
        e = plain_errors("step", Ts, n_elem, case)
        print(f"plant_bounds plain step Ts={Ts} n_elem={n_elem} case={case} largest error in units per channel", np.round(e.max(axis=0), 3))
        assert np.isfinite(e).all() and e.max() <= PLAIN_GATE, (case, e.max(), pr.points()["label"][int(e.max(axis=1).argmax())])


@pytest.mark.parametrize("case", ["w", "e", "we"])
def test_plain_fed_state_against_the_exact_sim_step(case):
    e = plain_errors("fed", pr.TS, pr.N_ELEM, case)
    print(f"plant_bounds plain fed state case={case} largest error in units per channel", np.round(e.max(axis=0), 3))
    assert np.isfinite(e).all() and e.max() <= PLAIN_GATE and (e[:, 7] == 0).all()


def test_the_larger_step_is_large_and_well_conditioned():
    """pr.LARGE_TS: h |xdot| reaches the size of the lateral velocity states, and the plain statement shows no amplification"""
    p = pr.points()
    e = plain_errors("step", pr.LARGE_TS, 1)
    rel = []
    for i in range(len(p["A"])):
        v = pr.step(p["X"][i], p["A"][i], p["SR"][i], pr.LARGE_TS, 1)["value"]
        rel.append([abs(float(v[c]) - p["X"][i][c]) / abs(p["X"][i][c]) if p["X"][i][c] else np.nan for c in (4, 5)])
    med = np.nanmedian(np.array(rel), axis=0)
    print(f"plant_bounds larger step Ts={pr.LARGE_TS}: median |x_next - x| / |x| of vt, r = {med[0]:.3f}, {med[1]:.3f}; plain largest error {e.max():.3f} units")
    assert med[0] >= 0.5 and med[1] >= 0.25 and e.max() <= 4.0


@pytest.mark.parametrize("name", sorted(WINDOW_SETS))
def test_plain_estimator_against_the_exact_mean(name):
    """every window of 1 to 4, the fill phase included; a window of 1 returns the sample itself"""
    e = plain_estimator_errors(name)
    print(f"plant_bounds plain estimator windows={name} largest error in units per state", np.round(e.max(axis=(0, 1)), 3))
    assert {w for ws in WINDOW_SETS.values() for w in ws} == {1, 2, 3, 4}
    assert e.max() <= PLAIN_GATE
    if name == "ones":
        assert e.max() == 0.0


# ---------------------------------------------------------------------------------------------- the probe
def probe_command(out):
    import __graft_entry__ as ge
    return [ge.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", ge.CSRC, "-o", out, PROBE_SRC]


def test_plant_probe_compiles_for_gfx950(tmp_path):
    import __graft_entry__ as ge
    if not (os.path.exists(ge.HIPCC) or shutil.which(ge.HIPCC)):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path / "libplant_probe.so")
    r = subprocess.run(probe_command(out), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(out), r.stdout + r.stderr


def report_lines():
    lines = ["# CPU half: closed_loop.plant_xdot / plant_step / MovingAverageEstimator against the exact statement, largest error in units",
             "# per class / variant group: channels px py yaw vl vt r delta (a)"]
    rows = [("xdot", plain_errors("xdot"))]
    rows += [(f"step Ts={Ts} n_elem={ne}", plain_errors("step", Ts, ne)) for Ts, ne in pr.STEPS]
    rows += [(f"fed state case={c}", plain_errors("fed", pr.TS, pr.N_ELEM, c)) for c in ("w", "e", "we")]
    for name, e in rows:
        lines.append(f"plain {name}: largest {e.max():.3f}")
        for g, v in _by_group(e).items():
            lines.append(f"  plain {name} {g:15s} " + " ".join(f"{t:6.3f}" for t in v))
    for name in sorted(WINDOW_SETS):
        lines.append(f"plain estimator windows={name}: " + " ".join(f"{t:6.3f}" for t in plain_estimator_errors(name).max(axis=(0, 1))))
    return lines


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("\n".join(report_lines()))
