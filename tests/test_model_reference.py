"""
The exact model reference (tests/model_reference.py) held to itself, the oracle held to it, and the bounds both this file and
tests/test_gpu_model_reference.py apply at model level.

Bound of one entry of f, J, Phi, A, B, h, grad h at one point (`allowance`): ten times the largest of
  - the oracle's move between two builds of its source with FMA contraction off and on,
  - its move under a one-ulp change of every input, over four sign patterns. The inputs of the oracle's functions are the state,
    the control AND the twenty scalar parameters of the model it is handed: one ulp of Df or Dr is one ulp of a tyre force, of m one
    ulp of every acceleration. At low speed the small entries are differences of tyre forces thousands of times their size, whose
    rounding a change of x and u alone does not sample (it moves both forces together). An input that sits on a kink decided on an
    input -- vl > 0.001, a < 0, a knot of the gg table -- or one double beside it keeps its value where the change would cross
    the kink (the two sides are different functions), and the gg table keeps its knots,
  - one ulp of the entry,
computed on the oracle alone: the allowance of tests/test_aux_reference.py (rk4_spread), extended from A to the other quantities,
with the same factor ten. Structural entries (the identity rows of px, py, psi, delta, a and the zeros) get no allowance: they
must be equal. A point whose bound exceeds 1e-9 of max(1, |entry|) is too ill-conditioned to tell a right kernel from a wrong one;
the generated set has none (asserted).

`PYTHONPATH=. python tests/test_model_reference.py` prints the CPU half of profiles/model_reference_bounds.txt.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_reference as mr
from oracle import oracle as _orc
from test_aux_reference import _contract_builds

U53 = 2.0 ** -53
FACTOR = 10.0
ILL = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROBE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device", "model_probe.hip")
KEYS = ("f", "J", "Phi", "A", "B", "h", "gh")

# what is computed at all; everything else is 0 or 1 on every side
COMPUTED = dict(f=np.ones(8, bool), J=np.ones((3, 5), bool), Phi=np.ones(8, bool), A=np.zeros((8, 8), bool), B=np.zeros((8, 2), bool),
                h=np.ones(1, bool), gh=np.zeros(8, bool))
COMPUTED["A"][:6, 3:] = True; COMPUTED["A"][:2, 2] = True
COMPUTED["B"][:6] = True; COMPUTED["B"][6, 1] = True; COMPUTED["B"][7, 0] = True
COMPUTED["gh"][[3, 5, 7]] = True
_NIN = 10 + len(mr._PNAMES)          # x, u, the scalar parameters
_SIGNS = [np.ones(_NIN), -np.ones(_NIN), np.where(np.arange(_NIN) % 2 == 0, 1.0, -1.0), np.where(np.arange(_NIN) % 2 == 0, -1.0, 1.0)]


def _model_moved(signs):
    m = _orc.edgar_model()
    for k, sg in zip(mr._PNAMES, signs):
        setattr(m, k, float(np.nextafter(getattr(m, k), sg * np.inf)))
    return m


@functools.lru_cache(maxsize=None)
def _libs():
    dp = ctypes.POINTER(ctypes.c_double)
    out = []
    for L in (_orc.lib(),) + tuple(_contract_builds()):
        L.oracle_stm_f.argtypes = [ctypes.POINTER(_orc.StmModel), dp, dp, dp, dp, dp]
        L.oracle_rk4_sens.argtypes = [ctypes.POINTER(_orc.StmModel), dp, dp, ctypes.c_double, ctypes.c_int, dp, dp, dp]
        L.oracle_h.argtypes = [ctypes.POINTER(_orc.StmModel), dp, dp, dp]
        out.append(L)
    return tuple(out)


def oracle_eval(L, x, u, dt, nsub, model=None):
    """the oracle's f, J, Phi, A, B, h, grad h at one point, from the library L"""
    model = model or _orc.edgar_model()
    x = np.ascontiguousarray(x, dtype=np.float64); u = np.ascontiguousarray(u, dtype=np.float64)
    d = _orc._dp
    xd = np.zeros(8); Jx = np.zeros((8, 8)); Ju = np.zeros((8, 2)); xn = np.zeros(8); A = np.zeros((8, 8)); B = np.zeros((8, 2))
    h = np.zeros(1); gh = np.zeros(8)
    L.oracle_stm_f(ctypes.byref(model), d(x), d(u), d(xd), d(Jx), d(Ju))
    L.oracle_rk4_sens(ctypes.byref(model), d(x), d(u), float(dt), int(nsub), d(xn), d(A), d(B))
    L.oracle_h(ctypes.byref(model), d(x), d(h), d(gh))
    return dict(f=xd, J=Jx[3:6, 3:8].copy(), Phi=xn, A=A, B=B, h=h, gh=gh)


def _input_side(x):
    v = mr.ggv_table()[0]
    seg = 0
    while seg < len(v) - 2 and x[3] >= v[seg + 1]:
        seg += 1
    return (bool(x[3] > mr.VL_THR), seg), bool(x[7] < 0.0)


def allowance(x, u, dt=mr.DT, nsub=3):
    """(oracle values, bound) per quantity, entry by entry (see the header)"""
    main, off, fast = _libs()
    x = np.asarray(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    base = oracle_eval(main, x, u, dt, nsub)
    a, b = oracle_eval(off, x, u, dt, nsub), oracle_eval(fast, x, u, dt, nsub)
    spread = {k: np.abs(a[k] - b[k]) for k in KEYS}
    side = _input_side(x)
    for s in _SIGNS:
        xp = np.nextafter(x, s[:8] * np.inf); up = np.nextafter(u, s[8:10] * np.inf)
        sp = _input_side(xp)
        if sp[0] != side[0]:
            xp[3] = x[3]
        if sp[1] != side[1]:
            xp[7] = x[7]
        p = oracle_eval(main, xp, up, dt, nsub, _model_moved(s[10:]))
        for k in KEYS:
            spread[k] = np.maximum(spread[k], np.abs(p[k] - base[k]))
    bound = {}
    for k in KEYS:
        sprd = np.maximum(spread[k], 2.0 * U53 * np.abs(base[k]))
        bound[k] = np.where(COMPUTED[k], FACTOR * sprd, 0.0)
    return base, bound


def ratio(got, want, bound):
    """largest |got - want| / bound over the entries; an entry without allowance must be equal (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if np.all(np.isfinite(r)) else float("inf")


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(GOLDEN, "model_reference.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def fixture_point(g, p, nsub=3, tag=""):
    """the reference of point p in the layout of oracle_eval"""
    return dict(f=g["f"][p], J=g["J"][p], Phi=g[f"Phi{nsub}{tag}"][p], A=g[f"A{nsub}{tag}"][p], B=g[f"B{nsub}{tag}"][p],
                h=np.atleast_1d(g["h"][p]), gh=g["gh"][p])


@functools.lru_cache(maxsize=None)
def point_bounds(nsub=3, tag=""):
    """(oracle values, bound) of every model point; tag "_u0": with u = 0"""
    g = fixture()
    return [allowance(g["X"][p], g["U"][p] if tag == "" else np.zeros(2), mr.DT, nsub) for p in range(len(g["labels"]))]


@functools.lru_cache(maxsize=None)
def oracle_report():
    """per (nsub, tag): oracle / bound at every point and quantity, and the worst bound relative to the entry's scale"""
    g = fixture()
    P = len(g["labels"])
    rows = []
    for nsub in mr.NSUBS:
        for tag in ("", "_u0"):
            for p in range(P):
                base, bound = point_bounds(nsub, tag)[p]
                ref = fixture_point(g, p, nsub, tag)
                for k in (KEYS if tag == "" and nsub == mr.NSUBS[0] else ("Phi", "A", "B")):          # (f, J, h, grad h: once)
                    ill = float(np.max(bound[k] / np.maximum(1.0, np.abs(ref[k]))))
                    rows.append((nsub, tag, p, str(g["labels"][p]), k, ratio(base[k], ref[k], bound[k]), ill))
    return rows


# ---------------------------------------------------------------------------------------------- the reference against itself
def test_reference_is_converged():
    """half the difference step and 80 digits instead of 60: nothing moves by more than 1e-30 relative"""
    X, U, L = mr.model_points()
    picks = [L.index(l) for l in ("nominal", "vl_above_thr", "slip_fbig_rbig", "gr_clip_high", "gf_clip_low", "a_-tiny", "knot4", "yaw_1e4")]
    worst = 0.0
    for p in picks:
        for fun, args in ((mr.eval_f, (X[p], U[p])), (mr.eval_phi, (X[p], U[p], mr.DT, 3)), (mr.eval_phi, (X[p], U[p], mr.DT, 1)), (mr.eval_h, (X[p],))):
            a = fun(*args, raw=True)[:-1]
            b = fun(*args, dps=mr.H_DPS + 20 if fun is mr.eval_h else 80, rel="5e-21", raw=True)[:-1]
            for va, vb in zip(a, b):
                fa = np.array(va, dtype=object).reshape(-1); fb = np.array(vb, dtype=object).reshape(-1)
                for ea, eb in zip(fa, fb):
                    worst = max(worst, float(abs(ea - eb) / (1 + abs(eb))))
    assert worst <= 1e-30, worst


def test_phi_against_exported_expression():
    """Phi with one RK4 step at the stored points of snmpc_expr.npz (states and inputs as stored) against the exported CasADi expression,
    to that file's own 2e-5 (its constants are truncated)"""
    g = np.load(os.path.join(GOLDEN, "snmpc_expr.npz"))
    n, worst = 0, 0.0
    for j in range(g["X"].shape[0]):
        X, F = g["X"][j].reshape(11, 8), g["F"][j].reshape(11, 8)
        for i in ([0] if g["stop"][j] == 1.0 else range(1, 11)):
            x = np.where(np.isfinite(X[i]), X[i], 0.0)
            phi = mr.eval_phi(x, g["U"][j], float(g["Ts"]), 1, derivatives=False)[0]
            worst = max(worst, float(np.max(np.abs(phi - F[i]) / (1.0 + np.abs(F[i])))))
            n += 1
    assert n == 264 and worst < 2e-5, (n, worst)


def test_wrap_is_fmod():
    for y in mr.primitive_points("wrap_yaw"):
        w = mr.wrap(float(y))
        assert 0.0 <= w <= mr.TWO_PI and abs(w - float(mr.wrap_exact(y))) <= mr.ulp_of(w) / 2


# ---------------------------------------------------------------------------------------------- the inputs
def test_every_label_is_present_and_taken():
    X, U, L = mr.model_points()
    assert sorted(set(L)) == sorted(set(mr.REQUIRED_LABELS))
    assert 150 <= len(L) <= 250
    wrong = [(p, L[p]) for p in range(len(L)) if not mr.label_holds(L[p], X[p], U[p])]
    assert not wrong, wrong


def test_fixture_is_the_generated_set_and_cannot_drift():
    """the committed file holds exactly the generated points, and one point per label recomputed now equals it bit for bit"""
    X, U, L = mr.model_points()
    g = fixture()
    assert np.array_equal(g["X"], X) and np.array_equal(g["U"], U) and list(g["labels"]) == list(L) and float(g["dt"]) == mr.DT
    idx = [L.index(l) for l in sorted(set(L))]
    again = mr.reference_arrays(idx)
    for k, v in again.items():
        assert np.array_equal(v, g[k][idx]), k
        assert g[k].shape[0] == len(L) and np.isfinite(g[k]).all(), k


def test_no_point_is_ill_conditioned_and_none_is_dropped():
    rows = oracle_report()
    P = len(fixture()["labels"])
    for k in KEYS:                                                    # every point in every comparison: the share left out is 0
        assert len({r[2] for r in rows if r[4] == k}) == P and len([r for r in rows if r[4] == k]) == P * (4 if k in ("Phi", "A", "B") else 1)
    ill = [(r[:5], r[6]) for r in rows if not r[6] <= ILL]
    assert not ill, ill[:10]


def test_oracle_against_reference():
    """stm_f, rk4_sens and h_con of the oracle, values and every derivative entry, at every model point, nsub 3 and 1, u as generated and 0"""
    rows = oracle_report()
    bad = [r[:6] for r in rows if not r[5] <= 1.0]
    assert not bad, bad[:20]


# ---------------------------------------------------------------------------------------------- the probe builds without a GPU
def probe_command(out):
    import __graft_entry__ as ge
    return [ge.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", ge.CSRC, "-o", out, PROBE_SRC]


def test_probe_compiles_for_gfx950(tmp_path):
    import __graft_entry__ as ge
    if not (os.path.exists(ge.HIPCC) or shutil.which(ge.HIPCC)):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path / "libmodel_probe.so")
    r = subprocess.run(probe_command(out), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(out), r.stdout + r.stderr


def report_lines():
    rows = oracle_report()
    lines = ["# CPU half: the oracle (stm_f, rk4_sens, h_con) against the exact reference, largest error / bound"]
    for k in KEYS:
        lines.append(f"oracle {k:4s} {max(r[5] for r in rows if r[4] == k):.3f}   (largest bound / max(1, |entry|): {max(r[6] for r in rows if r[4] == k):.2e})")
    for nsub in mr.NSUBS:
        for tag in ("", "_u0"):
            lines.append(f"oracle nsub={nsub}{tag or '   '} {max(r[5] for r in rows if r[0] == nsub and r[1] == tag):.3f}")
    for lab in sorted({r[3] for r in rows}):
        lines.append(f"oracle label {lab:20s} {max(r[5] for r in rows if r[3] == lab):.3f}")
    return lines


if __name__ == "__main__":
    print("\n".join(report_lines()))
