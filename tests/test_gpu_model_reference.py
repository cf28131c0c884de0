"""
The vehicle model on the device held to the exact reference of tests/model_reference.py (fixture tests/golden/model_reference.npz):

(a) the device functions of csrc/nmpc_device.hpp themselves, through tests/device/model_probe.hip -- a test-only translation unit
    compiled once per module into pytest's temporary directory and loaded with ctypes (a missing compiler is a failure here);
(b) the shipped linearisation kernels through the C-ABI: lin_kernel<false> ("lin-lane-per-stage"), lin_cols_kernel<false>
    ("lin-eight-lanes"), lin_uniform_kernel + lin_fill_kernel (a cold start with lin_dedup 1), with nsub 3 and 1, at N = 8 and at
    N = 49 (seven tiles), and h through the row constants of get_device("qp_vec");
(c) the edge of the domain: exact standstill.

Layout of (b). The model points sit on the EVEN stages k of small batches; stage k + 1 holds the binary64 rounding of the
reference's Phi(x_k, u_k), so that the defect b_k = Phi_dev - X_{k+1} is an exact difference of two neighbouring doubles and
b_k + X_{k+1} gives the kernel's Phi back without a rounding of its own (with an arbitrary X_{k+1}, as
test_gpu_dynamics_against_exported_expression lays its points out, the difference would round at ulp(X_{k+1}), far above the
bound of a small entry). Unused stages hold the harmless state. The status of the solve is not asserted.
The cold start of the uniform path cannot choose X_{k+1}: there X_{k+1} = x0, b = fl(Phi - x0), and b + x0 rounds once more; the
bound of Phi grows by u (|b| + |Phi|) (1 + 2u) for exactly these two roundings.

The coupled-SNMPC capsule does not serve get_from_qp_in (CoupledSnmpcSolver.get_from_qp_in raises: "not available for the stacked
state"); its linearisation kernels -- snmpc_lin_kernel, snmpc_lin_cols_kernel, lin_kernel<true>, lin_cols_kernel<true> -- are driven in
the same layout by tests/test_gpu_snmpc_reference.py through CoupledSnmpcSolver.get_snmpc_linearisation, with h at |v| (h_con_vabs)
against model_reference.eval_h_vabs; what they inline -- rk4_sens, rk4_sens_col with one RK4 step -- is also held by the probe in (a).

h through qp_vec. The condensing kernel writes, for stage s >= 1, d[2 (s - 1) + 1] = h(x_s) + g3 w3 + g5 w5 + g7 w7 with
(g3, g5, g7) = grad h(x_s) and w = g_s, the constant part of dx_s (g_0 = x0 - X_0, g_{k+1} = A_k g_k + b_k). After a cold start
g_0 = 0 and g_1 = b_0, which get_from_qp_in hands out to the bit. The test compares d[1] with h_ref + grad h_ref . b_0 within
bound(h) + sum_i bound(g_i) |b_0i| + 4 u (|h| + sum_i |g_i b_0i|): three products and three sums.

Bounds: the primitives' in the docstrings below. Model level: the allowance of tests/test_model_reference.py (`allowance`, measured on
the oracle alone) plus one term the oracle cannot know (`dev_bound`). The oracle divides; the device multiplies by frcp, whose
contract is a relative error of eps_f = s^2 + 2u = 2.2e-15 -- ten ulp -- per call (test_frcp_and_the_raw_seeds). Where such an error
reaches an entry through the ARGUMENT of a smooth function it acts like a ten-ulp change of an input, which ten times the
one-ulp input move covers. Where the reciprocal is a FACTOR of the entry it is a relative error of the entry itself, and the
allowance's floor of ten ulp of the entry (2.2e-15 |entry|) is already spent by one call. The longest chain of reciprocal
factors in stm_core is five, in d Fyf / d vl = dFyf alf_vl cgf + ...: two in dFyf (1 / (1 + inner^2), 1 / (1 + x1^2)) and three in
alf_vl = qf ivl cf2 with qf = (vt + lf r) ivl (ivl twice, cf2 once); a value (f, Phi) has at most one (isp in the rolling resistance;
qf enters through atan, as an argument), h_con has none (it divides). So the device bound of an entry is
    allowance + n eps_f |entry|,   n = 5 for J, A, B, 1 for f, Phi, 0 for h, grad h,
structural entries still exact. (Measured before this term existed: everything inside the allowance alone except d psi / d vl of one
point with nsub = 1, an entry of -2.5e-5 with an error of 11.5 ulp against a floor of 10.) Not covered here: the
sensitivity-free RK4 of sqp_kernels.hpp (it has a restatement of its own). The plant of loop_kernels.hpp is held to its own exact
statement by tests/test_gpu_plant_reference.py (tests/plant_reference.py).

Every test prints its largest error / bound ("MRB ..." lines): the GPU half of profiles/model_reference_bounds.txt.
"""
import ctypes
import math
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import model_reference as mr
from oracle import oracle as _orc
from test_model_reference import U53, fixture, point_bounds, probe_command, ratio

pytestmark = pytest.mark.gpu

DT = mr.DT
_dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


S_RCP = 4.5e-8          # relative error of the raw rcp seed, rounded up from the 4.464e-8 test_frcp_and_the_raw_seeds measures
EPS_F = S_RCP * S_RCP + 2 * U53
FRCP_CHAIN = dict(f=1, Phi=1, J=5, A=5, B=5, h=0, gh=0)


def dev_bound(bd, key, ref, rows=slice(None)):
    """bound of a device entry: the oracle's allowance plus the reciprocal factors the oracle does not have (module docstring)"""
    ref = np.asarray(ref, dtype=np.float64)
    return bd[key][rows] + np.where(bd[key][rows] > 0.0, FRCP_CHAIN[key] * EPS_F * np.abs(ref), 0.0)


def _report(name, value):
    print(f"MRB {name} {value:.4g}")


class Probe:
    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        L.probe_set_model.argtypes = [_dp, ctypes.c_int, _dp, _dp, _dp]
        L.probe_primitive.argtypes = [ctypes.c_int, _dp, _dp, _dp, ctypes.c_int]
        L.probe_wrap_yaw.argtypes = [_dp, _dp, ctypes.c_int]
        L.probe_pacejka.argtypes = [ctypes.c_int, _dp, _dp, _dp, ctypes.c_int]
        L.probe_stm_core.argtypes = [_dp, _dp, _dp, ctypes.c_int]
        L.probe_stm_core_quad.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_int]
        L.probe_interp_lin.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_int]
        L.probe_h_con.argtypes = [_dp, _dp, ctypes.c_int]
        L.probe_rk4_sens.argtypes = [_dp, _dp, ctypes.c_double, ctypes.c_int, _dp, _dp, _dp, ctypes.c_int]
        L.probe_rk4_sens_col.argtypes = [_dp, _dp, ctypes.c_double, ctypes.c_int, _dp, _dp, ctypes.c_int]
        m = _orc.edgar_model()
        p = np.array([getattr(m, k) for k in mr._PNAMES], dtype=np.float64)
        v, ax, ay = (np.array(t, dtype=np.float64) for t in mr.ggv_table())
        self._ok(L.probe_set_model(_p(p), len(v), _p(v), _p(ax), _p(ay)), "set_model")

    @staticmethod
    def _ok(rc, what):
        assert rc == 0, f"model_probe {what}: HIP status {rc}"

    @staticmethod
    def _in(a, shape=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a if shape is None else a.reshape(shape)

    def primitive(self, which, x):
        x = self._in(x); o0 = np.zeros_like(x); o1 = np.zeros_like(x)
        self._ok(self.L.probe_primitive(which, _p(x), _p(o0), _p(o1), x.size), f"primitive {which}")
        return o0, o1

    def wrap_yaw(self, x):
        x = self._in(x); o = np.zeros_like(x)
        self._ok(self.L.probe_wrap_yaw(_p(x), _p(o), x.size), "wrap_yaw")
        return o

    def pacejka(self, front, al):
        al = self._in(al); a = np.zeros_like(al); b = np.zeros_like(al)
        self._ok(self.L.probe_pacejka(int(front), _p(al), _p(a), _p(b), al.size), "pacejka")
        return a, b

    def stm_core(self, v5):
        v5 = self._in(v5); n = v5.shape[0]; f = np.zeros((n, 3)); J = np.zeros((n, 3, 5))
        self._ok(self.L.probe_stm_core(_p(v5), _p(f), _p(J), n), "stm_core")
        return f, J

    def stm_core_quad(self, v6):
        v6 = self._in(v6); n = v6.shape[0]; f = np.zeros((n, 4, 3)); J = np.zeros((n, 4, 3, 5)); sc = np.zeros((n, 4, 2))
        self._ok(self.L.probe_stm_core_quad(_p(v6), _p(f), _p(J), _p(sc), n), "stm_core_quad")
        return f, J, sc

    def interp_lin(self, tab, x):
        tab, x = self._in(tab), self._in(x); y = np.zeros_like(x); dy = np.zeros_like(x)
        self._ok(self.L.probe_interp_lin(_p(tab), _p(x), _p(y), _p(dy), x.size), "interp_lin")
        return y, dy

    def h_con(self, v3):
        v3 = self._in(v3); n = v3.shape[0]; o = np.zeros((n, 4))
        self._ok(self.L.probe_h_con(_p(v3), _p(o), n), "h_con")
        return o

    def rk4_sens(self, x, u, dt, nsub):
        x, u = self._in(x), self._in(u); n = x.shape[0]; xn = np.zeros((n, 8)); Sp = np.zeros((n, 2)); S = np.zeros((n, 6, 7))
        self._ok(self.L.probe_rk4_sens(_p(x), _p(u), dt, nsub, _p(xn), _p(Sp), _p(S), n), "rk4_sens")
        return xn, Sp, S

    def rk4_sens_col(self, x, u, dt, nsub):
        x, u = self._in(x), self._in(u); n = x.shape[0]; xn = np.zeros((n, 8, 8)); Sc = np.zeros((n, 8, 6))
        self._ok(self.L.probe_rk4_sens_col(_p(x), _p(u), dt, nsub, _p(xn), _p(Sc), n), "rk4_sens_col")
        return xn, Sc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("model_probe") / "libmodel_probe.so")
    r = subprocess.run(probe_command(out), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(out), "the probe does not compile:\n" + r.stdout + r.stderr
    return Probe(out)


# ---------------------------------------------------------------------------------------------- (a) the primitives
def _errors(dev, exact_fun, x, dps=50):
    """|dev - exact| and ulp(exact), per point, exact in mpmath"""
    err = np.zeros(len(x)); ulp = np.zeros(len(x)); ex = []
    with mp.workdps(dps):
        for i, (xv, dv) in enumerate(zip(x, dev)):
            e = exact_fun(mp.mpf(float(xv)))
            ex.append(e)
            err[i] = float(abs(mp.mpf(float(dv)) - e)); ulp[i] = mr.ulp_of(e)
    return err, ulp, ex


def _header_sincos_constants():
    """the two literals of fast_sincos's Cody-Waite reduction, read from the header"""
    import __graft_entry__ as ge
    src = open(os.path.join(ge.CSRC, "nmpc_device.hpp")).read()
    body = src[src.index("void fast_sincos("):src.index("double fast_atan(")]
    hi = re.search(r"fma\(-n,\s*([0-9.eE+-]+),\s*x\)", body).group(1)
    lo = re.search(r"fma\(-n,\s*([0-9.eE+-]+),\s*r\)", body).group(1)
    return float(hi), float(lo)


def test_frcp_and_the_raw_seeds(probe):
    """frcp: relative error <= s^2 + 2u, s the largest relative error of the raw rcp seed over the same inputs (the step r (2 - x r)
    squares the seed's error, the two fma round once each); s and the rsq seed's error are measured here and printed."""
    x = mr.primitive_points("frcp")
    seed, _ = probe.primitive(4, x)
    got, _ = probe.primitive(3, x)
    rel = lambda dev: np.array([float(abs(mp.mpf(float(d)) * mp.mpf(float(v)) - 1)) for d, v in zip(dev, x)])
    with mp.workdps(50):
        s = float(rel(seed).max()); e = rel(got)
    xs = mr.primitive_points("fast_sqrt_pos")
    rs, _ = probe.primitive(5, xs)
    with mp.workdps(50):
        s_rsq = max(float(abs(mp.mpf(float(d)) * mp.sqrt(mp.mpf(float(v))) - 1)) for d, v in zip(rs, xs))
    bound = s * s + 2 * U53
    _report("seed_rcp_relative_error_s", s); _report("seed_rsq_relative_error", s_rsq)
    _report("frcp_relative_error", float(e.max())); _report("frcp error/bound", float(e.max()) / bound)
    assert np.isfinite(got).all() and e.max() <= bound, (e.max(), bound, s)


def test_fast_sqrt_pos(probe):
    """<= 1 ulp of the exact root (the header's own contract)"""
    x = mr.primitive_points("fast_sqrt_pos")
    got, _ = probe.primitive(2, x)
    err, ulp, _ = _errors(got, mp.sqrt, x)
    r = err / ulp
    _report("fast_sqrt_pos ulp", float(r.max())); _report("fast_sqrt_pos error/bound", float(r.max()) / 1.0)
    assert r.max() <= 1.0, (r.max(), x[np.argmax(r)])


def test_fast_atan(probe):
    """<= 2.5 ulp of the exact value (fdlibm polynomial 1 ulp on the reduced argument, the subtraction from hi rounds at ulp(hi) <=
    2 ulp(result): 1 ulp, inner rounding 1/2 ulp); <= 1.5 ulp in the first range (hi = 0); odd to the bit; atan(+-0) = +-0"""
    x = mr.primitive_points("fast_atan")
    got, _ = probe.primitive(1, x)
    neg, _ = probe.primitive(1, -x)
    assert np.array_equal(neg, -got) and np.array_equal(np.signbit(neg), ~np.signbit(got))
    z, _ = probe.primitive(1, np.array([0.0, -0.0]))
    assert z[0] == 0.0 and z[1] == 0.0 and not np.signbit(z[0]) and np.signbit(z[1])
    err, ulp, _ = _errors(got, mp.atan, x)
    r = err / ulp
    first = np.abs(x) <= mr.ATAN_SEAMS[0]
    _report("fast_atan ulp first range", float(r[first].max())); _report("fast_atan ulp", float(r.max()))
    _report("fast_atan error/bound", max(float(r[first].max()) / 1.5, float(r.max()) / 2.5))
    assert first.any() and (~first).any()
    assert r[first].max() <= 1.5, (r[first].max(), x[first][np.argmax(r[first])])
    assert r.max() <= 2.5, (r.max(), x[np.argmax(r)])


def test_fast_sincos(probe):
    """|error| <= 3 ulp(exact) + |n| delta, n = rint(2 x / pi), delta = |pi/2 - hi - lo| of the header's two literals (fdlibm kernel
    1 ulp; the two fma of the reduction round at 1/2 ulp(r) <= 1 ulp(result) each; |n| delta is the truncated constant, which
    dominates next to multiples of pi / 2); <= 2 ulp for |x| <= pi / 4 (n = 0)"""
    x = mr.primitive_points("fast_sincos")
    sn, cs = probe.primitive(0, x)
    hi, lo = _header_sincos_constants()
    with mp.workdps(60):
        delta = abs(mp.pi / 2 - mp.mpf(hi) - mp.mpf(lo))
        n = np.array([abs(int(mp.nint(2 * mp.mpf(float(v)) / mp.pi))) for v in x], dtype=np.float64)
        nd = n * float(delta)
    small = np.abs(x) <= math.pi / 4
    assert (n[small] == 0).all() and small.any() and n.max() >= 60000
    _report("fast_sincos delta", float(delta))
    worst = {}
    for name, dev, fun in (("sin", sn, mp.sin), ("cos", cs, mp.cos)):
        err, ulp, _ = _errors(dev, fun, x, dps=60)
        r = err / np.where(small, 2.0 * ulp, 3.0 * ulp + nd)
        _report(f"fast_sincos {name} ulp |x|<=pi/4", float((err / ulp)[small].max()))
        _report(f"fast_sincos {name} largest error in ulp of the result", float((err / ulp).max()))
        _report(f"fast_sincos {name} error/bound", float(r.max()))
        worst[name] = (float(r.max()), float(x[np.argmax(r)]))
    assert all(v[0] <= 1.0 for v in worst.values()), worst


def test_fast_sincos_is_odd_and_even_to_the_bit(probe):
    """sin(-x) = -sin(x) and cos(-x) = cos(x) bit for bit, the sign of a zero included, at every point of the set. (This test found
    fast_sincos(-0.0) returning sin = +0.0: a reduction from x makes +0.0 of any zero twice over -- r = fma(+0.0, hi, -0.0) and
    s = fma(r z, ps, r) each add a zero of the other sign. The function now forms n with an fma onto +0.0 and copies the sign of r onto s; for every
    other x the bits are unchanged.)"""
    x = mr.primitive_points("fast_sincos")
    sn, cs = probe.primitive(0, x)
    sn_, cs_ = probe.primitive(0, -x)
    bad_s = np.flatnonzero((sn_ != -sn) | (np.signbit(sn_) == np.signbit(sn)))
    bad_c = np.flatnonzero((cs_ != cs) | (np.signbit(cs_) != np.signbit(cs)))
    _report("fast_sincos pairs not odd to the bit", float(len(bad_s))); _report("fast_sincos pairs not even to the bit", float(len(bad_c)))
    print("MRB fast_sincos not odd at x =", [float(v) for v in x[bad_s][:8]], "sin(x), sin(-x) =", [(float(a), float(b)) for a, b in zip(sn[bad_s][:8], sn_[bad_s][:8])])
    assert len(bad_c) == 0 and len(bad_s) == 0, (x[bad_s][:8], x[bad_c][:8])


def test_interp_lin_and_wrap_yaw(probe):
    """bit-equal to the binary64 restatement of the same two lines (the reference's arithmetic here IS binary64; fmod is exact);
    interp_lin's value also within 2 ulp of the exact line"""
    pts = mr.primitive_points("interp_lin")
    y, dy = probe.interp_lin(pts[:, 0], pts[:, 1])
    v, ax, ay = mr.ggv_table()
    worst = 0.0
    for i, (t, xv) in enumerate(pts):
        ys = ax if t == 0.0 else ay
        wy, ws = mr.interp_f64(v, ys, xv)
        assert y[i] == wy and dy[i] == ws, (t, xv, y[i], wy, dy[i], ws)
        with mp.workdps(60):
            P = mr.params()
            e, _, _ = mr.interp(P["ggv_v"], P["ggv_ax" if t == 0.0 else "ggv_ay"], mp.mpf(float(xv)), mr.Tape())
            worst = max(worst, float(abs(mp.mpf(float(y[i])) - e)) / mr.ulp_of(e))
    _report("interp_lin ulp of the exact line", worst); _report("interp_lin error/bound", worst / 2.0)
    assert worst <= 2.0
    yaw = mr.primitive_points("wrap_yaw")
    w = probe.wrap_yaw(yaw)
    want = np.array([mr.wrap(float(t)) for t in yaw])
    _report("wrap_yaw mismatching bits", float(np.count_nonzero(w != want)))
    assert np.array_equal(w, want) and np.array_equal(np.signbit(w), np.signbit(want))


# ---------------------------------------------------------------------------------------------- (a) the model functions
def _pacejka_bound(B, C, D, E, al):
    """First-order forward bound of |Fy error|, |dFy error| of pacejka() in binary64 (floats; u = 2^-53), from the contracts the primitive
    tests hold: fast_atan 2.5 ulp (<= 5u relative), fast_sincos 3 ulp (<= 6u relative; |n| delta is below 1e-28 here), frcp s^2 + 2u.
    x1 = B al; at1 = atan(x1); inner = x1 - E (x1 - at1); th = atan(inner); Fy = D sin(C th);
    dFy = D cos(C th) C r1 g B with r1 = 1 / (1 + inner^2), g = 1 - E + E r2, r2 = 1 / (1 + x1^2).
    Every rounding is carried to the result through the exact partial derivative of what follows; the sum is doubled for the neglected
    second-order terms."""
    u = U53
    frcp_rel = EPS_F
    x1 = B * al
    at1 = math.atan(x1)
    e_x1 = u * abs(x1)
    e_at1 = 5 * u * abs(at1) + e_x1 / (1 + x1 * x1)
    inner = x1 - E * (x1 - at1)
    e_in = e_x1 + E * (e_x1 + e_at1) + u * (abs(x1 - at1) + E * abs(x1 - at1) + abs(inner))
    th = math.atan(inner)
    e_th = 5 * u * abs(th) + e_in / (1 + inner * inner)
    arg = C * th
    e_arg = C * e_th + u * abs(arg)
    sn, cs = math.sin(arg), math.cos(arg)
    e_sn = 6 * u * abs(sn) + abs(cs) * e_arg
    e_cs = 6 * u * abs(cs) + abs(sn) * e_arg
    e_Fy = D * e_sn + u * abs(D * sn)
    r1, r2 = 1 / (1 + inner * inner), 1 / (1 + x1 * x1)
    rel_r1 = frcp_rel + (2 * abs(inner) * e_in + 2 * u * (1 + inner * inner)) * r1
    rel_r2 = frcp_rel + (2 * abs(x1) * e_x1 + 2 * u * (1 + x1 * x1)) * r2
    g = 1 - E + E * r2
    rel_g = (E * r2 * rel_r2 + 3 * u * g) / g
    rest = D * C * r1 * g * B
    e_dFy = rest * e_cs + abs(rest * cs) * (rel_r1 + rel_g + 6 * u)
    return 2 * e_Fy, 2 * e_dFy


def test_pacejka(probe):
    """Fy and dFy / d alpha of both axles against D sin(C atan(B al - E (B al - atan(B al)))) in mpmath (derivative: central
    difference). The oracle exports no magic formula of its own and a spread measured on a restatement is useless next to the peak of
    the curve, where dFy passes through zero and a one-ulp change of an input is swallowed by the rounding of C th: the bound is the
    forward bound derived in _pacejka_bound. alpha: the slip angles of the model points and a grid of +-1.2 rad (it passes both
    peaks); Fy(0) = 0 exactly."""
    g = fixture()
    E_ = _orc.EDGAR
    X = g["X"]
    mv = X[:, 3] > mr.VL_THR
    with np.errstate(all="ignore"):
        alf = np.where(mv, X[:, 6] - np.arctan((X[:, 4] + E_["lf"] * X[:, 5]) / X[:, 3]), 0.0)
        alr = np.where(mv, np.arctan((E_["lr"] * X[:, 5] - X[:, 4]) / X[:, 3]), 0.0)
    grid = np.linspace(-1.2, 1.2, 401)
    worst = (0.0, None)
    for front, al in ((1, np.concatenate([alf, grid, [0.0]])), (0, np.concatenate([alr, grid, [0.0]]))):
        prm = [float(E_[k + ("f" if front else "r")]) for k in ("B", "C", "D", "E")]
        Fy, dFy = probe.pacejka(front, al)
        with mp.workdps(mr.DPS):
            B, C, D, E = (mp.mpf(t) for t in prm)
            fy = lambda a: D * mp.sin(C * mp.atan(B * a - E * (B * a - mp.atan(B * a))))
            for i, a in enumerate(al):
                am = mp.mpf(float(a)); e = mp.mpf("1e-20")
                want = float(fy(am)), float((fy(am + e) - fy(am - e)) / (2 * e))
                bound = _pacejka_bound(*prm, float(a))
                for name, got, w, bd in (("Fy", Fy[i], want[0], bound[0]), ("dFy", dFy[i], want[1], bound[1])):
                    r = ratio(got, w, bd)
                    if r > worst[0]:
                        worst = (r, (front, name, float(a), float(got), w, bd))
        assert Fy[-1] == 0.0
    _report("pacejka error/bound", worst[0])
    assert worst[0] <= 1.0, worst


def test_stm_core_and_stm_core_quad(probe):
    """f = (vl', vt', r') and the 3 x 5 hand-derived Jacobian at every model point, lane-local and dealt over a DPP quad (the four
    lanes of a quad end with the same f, J to the bit; the quad's sin / cos of psi to fast_sincos's bound)"""
    g = fixture()
    X, P = g["X"], len(g["labels"])
    bounds = point_bounds(3, "")
    f, J = probe.stm_core(X[:, 3:8])
    fq, Jq, sc = probe.stm_core_quad(np.concatenate([X[:, 3:8], X[:, 2:3]], axis=1))
    for lane in range(1, 4):
        assert np.array_equal(fq[:, lane], fq[:, 0]) and np.array_equal(Jq[:, lane], Jq[:, 0]) and np.array_equal(sc[:, lane], sc[:, 0])
    worst = {"stm_core": 0.0, "stm_core_quad": 0.0}
    per_label = {}
    for p in range(P):
        b = bounds[p][1]
        for name, ff, JJ in (("stm_core", f[p], J[p]), ("stm_core_quad", fq[p, 0], Jq[p, 0])):
            r = max(ratio(ff, g["f"][p][3:6], dev_bound(b, "f", g["f"][p][3:6], slice(3, 6))), ratio(JJ, g["J"][p], dev_bound(b, "J", g["J"][p])))
            worst[name] = max(worst[name], r)
            per_label[str(g["labels"][p])] = max(per_label.get(str(g["labels"][p]), 0.0), r)
    for k, v in worst.items():
        _report(f"{k} error/bound", v)
    for k in sorted(per_label):
        _report(f"label {k} stm_core error/bound", per_label[k])
    hi, lo = _header_sincos_constants()
    with mp.workdps(60):
        delta = float(abs(mp.pi / 2 - mp.mpf(hi) - mp.mpf(lo)))
        for p in range(P):
            psi = mp.mpf(float(X[p, 2])); n = abs(int(mp.nint(2 * psi / mp.pi)))
            for got, e in ((sc[p, 0, 0], mp.sin(psi)), (sc[p, 0, 1], mp.cos(psi))):
                assert float(abs(mp.mpf(float(got)) - e)) <= 3.0 * mr.ulp_of(e) + n * delta, (p, float(psi))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad and len(per_label) == len(set(g["labels"])), (bad, {k: v for k, v in per_label.items() if not v <= 1.0})


def test_h_con(probe):
    """h and (d/dvl, d/dr, d/da) at every model point: both branches of a, every knot and one double either side, both ends"""
    g = fixture()
    X, P = g["X"], len(g["labels"])
    bounds = point_bounds(3, "")
    o = probe.h_con(X[:, [3, 5, 7]])
    worst = 0.0
    for p in range(P):
        b = bounds[p][1]
        worst = max(worst, ratio(o[p, 0], g["h"][p], b["h"][0]), ratio(o[p, 1:], g["gh"][p][[3, 5, 7]], b["gh"][[3, 5, 7]]))
    _report("h_con error/bound", worst)
    assert worst <= 1.0, worst


def _worst_entry(p, q, got, want, bound):
    """(label, quantity, index, value, error, bound) of the entry with the largest error / bound: what a failure reports"""
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(bound)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    i = np.unravel_index(np.argmax(r), r.shape)
    return str(fixture()["labels"][p]), p, q, tuple(int(t) for t in i), float(want[i]), float(err[i]), float(bound[i])


def _assemble(Sp, S):
    """rows 0..5 of A (8 columns) and of B (2 columns) from the structured sensitivities"""
    A = np.zeros((6, 8)); B = np.zeros((6, 2))
    A[0, 0] = A[1, 1] = A[2, 2] = 1.0
    A[:2, 2] = Sp
    A[:, 3:8] = S[:, :5]
    B[:, 0] = S[:, 5]; B[:, 1] = S[:, 6]
    return A, B


@pytest.mark.parametrize("nsub", mr.NSUBS)
@pytest.mark.parametrize("tag", ["", "_u0"])
def test_rk4_sens_and_rk4_sens_col(probe, nsub, tag):
    """one shooting interval with forward sensitivities at every model point (u as generated / u = 0): Phi, and rows px..r of A and B
    assembled from (Sp, S); rk4_sens_col's eight lanes carry the same state to the bit and one column each"""
    g = fixture()
    X, P = g["X"], len(g["labels"])
    U = g["U"] if tag == "" else np.zeros_like(g["U"])
    bounds = point_bounds(nsub, tag)
    xn, Sp, S = probe.rk4_sens(X, U, DT, nsub)
    xc, Sc = probe.rk4_sens_col(X, U, DT, nsub)
    for lane in range(1, 8):
        assert np.array_equal(xc[:, lane], xc[:, 0])
    assert (Sc[:, 7, 2] == 1.0).all() and (Sc[:, 7, 3:] == 0.0).all()
    worst = {"rk4_sens": 0.0, "rk4_sens_col": 0.0}
    where = {}
    for p in range(P):
        b = bounds[p][1]
        cols = (xc[p, 0], Sc[p, 7, :2], Sc[p, :7].T)
        for name, (x1, sp, s) in (("rk4_sens", (xn[p], Sp[p], S[p])), ("rk4_sens_col", cols)):
            A, B = _assemble(sp, s)
            for q, got, want in (("Phi", x1, g[f"Phi{nsub}{tag}"][p]), ("A", A, g[f"A{nsub}{tag}"][p][:6]), ("B", B, g[f"B{nsub}{tag}"][p][:6])):
                bd = dev_bound(b, q, want, slice(None) if q == "Phi" else slice(0, 6))
                r = ratio(got, want, bd)
                if r > worst[name]:
                    worst[name] = r; where[name] = _worst_entry(p, q, got, want, bd)
    for k, v in worst.items():
        _report(f"{k} nsub={nsub}{tag} error/bound", v)
    assert all(v <= 1.0 for v in worst.values()), (worst, where)


# ---------------------------------------------------------------------------------------------- (b) the shipped kernels
def _staged(N, nsub):
    """the model points on the even stages (module docstring): Xi, Ui, where[p] = (b, k)"""
    g = fixture()
    P = len(g["labels"])
    per = N // 2
    B = (P + per - 1) // per
    Xi = np.tile(mr.HARMLESS, (B, N + 1, 1)); Ui = np.zeros((B, N, 2)); where = []
    for p in range(P):
        b, k = p // per, 2 * (p % per)
        Xi[b, k] = g["X"][p]; Ui[b, k] = g["U"][p]; Xi[b, k + 1] = g[f"Phi{nsub}"][p]
        where.append((b, k))
    return Xi, Ui, where


@pytest.mark.parametrize("N,nsub", [(8, 3), (8, 1), (49, 3)])
@pytest.mark.parametrize("kernel", ["lin-lane-per-stage", "lin-eight-lanes"])
def test_linearisation_kernels(kernel, N, nsub):
    """A_k, B_k, b_k + x_{k+1} of lin_kernel<false> / lin_cols_kernel<false> at every model point, all 8 x 8 + 8 x 2 + 8 entries"""
    from tum_control_amd.solver import BatchedOcpSolver
    g = fixture()
    Xi, Ui, where = _staged(N, nsub)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=nsub, batch=Xi.shape[0], store_qp_in=True)
    s.install_reference_ocp()
    s.set_kernel(kernel)
    s.set_x0(Xi[:, 0]); s.set_iterate(X=Xi, U=Ui)
    s.solve()
    bounds = point_bounds(nsub, "")
    rec = {k: (s.get_from_qp_in(k, "A"), s.get_from_qp_in(k, "B"), s.get_from_qp_in(k, "b").reshape(-1, 8)) for k in sorted({k for _, k in where})}
    worst, n, at = 0.0, 0, None
    for p, (b, k) in enumerate(where):
        A, B, bb = (t[b] for t in rec[k])
        bd = bounds[p][1]
        for q, got, want in (("Phi", bb + Xi[b, k + 1], g[f"Phi{nsub}"][p]), ("A", A, g[f"A{nsub}"][p]), ("B", B, g[f"B{nsub}"][p])):
            bnd = dev_bound(bd, q, want)
            r = ratio(got, want, bnd)
            if r > worst:
                worst, at = r, _worst_entry(p, q, got, want, bnd)
        n += 1
    _report(f"{kernel} N={N} nsub={nsub} error/bound", worst)
    assert n == len(g["labels"]) and worst <= 1.0, (worst, at)


def _qp_vec(s, width):
    """(batch, width) doubles of get_device("qp_vec"), through a buffer of the HIP runtime the library itself is linked to"""
    L = s._L
    L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    L.hipFree.argtypes = [ctypes.c_void_p]
    out = np.zeros((s.batch, width)); dev = ctypes.c_void_p()
    assert L.hipMalloc(ctypes.byref(dev), out.nbytes) == 0
    try:
        s.get_device("qp_vec", dev.value); s.synchronize()
        assert L.hipMemcpy(out.ctypes.data, dev, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    finally:
        L.hipFree(dev)
    return out


@pytest.mark.parametrize("nsub", mr.NSUBS)
def test_uniform_linearisation_and_h_row(nsub):
    """lin_uniform_kernel + lin_fill_kernel: a cold start whose x0 are the model points (u = 0), N = 40, lin_dedup 1; the records of the
    first and the last stage; and h of stage 1 through qp_vec (module docstring)"""
    from tum_control_amd.solver import BatchedOcpSolver
    g = fixture()
    P, N = len(g["labels"]), 40
    s = BatchedOcpSolver(N=N, dt=DT, nsub=nsub, batch=P, store_qp_in=True)
    s.install_reference_ocp()
    s.options_set("lin_dedup", 1)
    s.set_kernel("lin-lane-per-stage")          # (where the batch fits one round of the chip the library's own choice is the eight-lane kernel)
    s.set_x0(g["X"]); s.cold_start()
    s.solve()
    assert s.get_stats("lin_uniform") == 1
    bounds = point_bounds(nsub, "_u0")
    worst, at = 0.0, None
    for k in (0, N - 1):
        A, B, bb = s.get_from_qp_in(k, "A"), s.get_from_qp_in(k, "B"), s.get_from_qp_in(k, "b").reshape(-1, 8)
        for p in range(P):
            bd = bounds[p][1]
            phi = bb[p] + g["X"][p]
            extra = U53 * (np.abs(bb[p]) + np.abs(phi)) * (1.0 + 2.0 * U53)
            for q, got, want in (("Phi", phi, g[f"Phi{nsub}_u0"][p]), ("A", A[p], g[f"A{nsub}_u0"][p]), ("B", B[p], g[f"B{nsub}_u0"][p])):
                bnd = dev_bound(bd, q, want) + (extra if q == "Phi" else 0.0)
                r = ratio(got, want, bnd)
                if r > worst:
                    worst, at = r, _worst_entry(p, q, got, want, bnd)
    _report(f"lin_uniform N={N} nsub={nsub} error/bound", worst)
    d1 = _qp_vec(s, 160)[:, 80 + 1]
    b0 = s.get_from_qp_in(0, "b").reshape(-1, 8)
    hb = point_bounds(3, "")
    worst_h = 0.0
    for p in range(P):
        gh, bd = g["gh"][p][[3, 5, 7]], hb[p][1]
        w = b0[p][[3, 5, 7]]
        want = (mp.mpf(float(g["h"][p])) + sum(mp.mpf(float(a)) * mp.mpf(float(c)) for a, c in zip(gh, w)))
        bound = bd["h"][0] + float(np.sum(bd["gh"][[3, 5, 7]] * np.abs(w))) + 4 * U53 * (abs(g["h"][p]) + float(np.sum(np.abs(gh * w))))
        err = float(abs(mp.mpf(float(d1[p])) - want))
        worst_h = max(worst_h, 0.0 if err == 0.0 else err / bound)
    _report(f"h row of qp_vec nsub={nsub} error/bound", worst_h)
    assert worst <= 1.0 and worst_h <= 1.0, (worst, at, worst_h)


# ---------------------------------------------------------------------------------------------- (c) the edge of the domain
def test_standstill_fails_only_its_own_instance():
    """vl = vt = 0 is outside fast_sqrt_pos's stated domain (and the model's own expression has no finite derivative there): the
    instance comes back with status 4 (acados: QP failure), as an instance with a NaN input does, its inputs untouched; its
    neighbours return the bits of a batch without it. Nothing faults: the NaN is data."""
    from tum_control_amd.solver import BatchedOcpSolver
    from tum_control_amd.workloads import nominal_batch
    N, B = 40, 12
    x0, yref = nominal_batch(B, N=N, seed=4)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B)
    s.install_reference_ocp()
    s.set_x0(x0); s.set_yref_all(yref); s.cold_start(); assert s.solve() == 0
    Xg, Ug = s.get_iterate()
    still = x0.copy(); still[5, 3] = 0.0; still[5, 4] = 0.0
    s.set_x0(still); s.cold_start()
    X0, U0 = s.get_iterate()
    assert s.solve() == 4
    st = s.get_stats("status")
    assert st[5] == 4 and (np.delete(st, 5) == 0).all()
    X, U = s.get_iterate()
    keep = np.arange(B) != 5
    assert np.array_equal(X[keep], Xg[keep]) and np.array_equal(U[keep], Ug[keep])
    assert np.array_equal(U[5], U0[5])
