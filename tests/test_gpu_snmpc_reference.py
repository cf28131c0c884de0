"""The kernels of the coupled SNMPC OCP around the interior point method -- sample linearisation, prologue, lin_kernel<true> /
lin_cols_kernel<true>, cond_kernel<., true> / cond_wide_kernel, epilogue, freeze, expand_kernel<., true> -- against the dense
long-double statement of tests/snmpc_reference.py (-m gpu).

What a case does: the iterate is set on every copy of every stage, lbx_0 = ubx_0, yref and the reference weights; ONE solve on the
pipeline; then the linearisation is read through CoupledSnmpcSolver.get_snmpc_linearisation, H, q, C, d and the step dv through
get_condensed_qp, and the stacked iterate of EVERY stage (a stage beyond uph runs snmpc_freeze_kernel), the cost and the slacks.
The statement runs in long double and in binary64 ON THE DEVICE'S OWN LINEARISATION: never a comparison with another device variant
or with the oracle. The interior point kernel's answer dv is an input.

The gate (tests/test_gpu_bo.py::_gate): per case and array the largest error of the device against the long-double run, in units of
u x scale (cond_reference: SCALES), is at most max(32, 4 x the error of the binary64 run). The cap of
tests/test_snmpc_reference.py (that error <= 64, sd > 0 on every chance row but for one PCE term) is asserted here too, on the
device's linearisation. Exact: U+ == U + dv, the frozen sample copies equal stage uph, the padding of H is the identity, that of q
and the rows zero, a gg row has no column beyond its stage. Every case prints "SQB" lines: device, binary64 statement, gate -- the
GPU half of profiles/snmpc_bounds.txt.

Model level (the last tests): hs / ghs, hn / ghn and cv of the getter against model_reference.eval_h_vabs within
test_snmpc_reference.allowance_h_vabs; the sample records and the nominal records of the stages >= uph against
model_reference.eval_phi with one RK4 step, in the layout of tests/test_gpu_model_reference.py (b), within that file's dev_bound.
h_con_vabs divides where h_con divides (no frcp), and its one reciprocal 1 / |v| is IEEE: no term beyond the allowance.
cv = fl(v . fl(1 / fl(sqrt(fl(vl^2 + vt^2))))): relative errors 2u, halved by the root plus its rounding u, plus u, plus u -- 4 u |cv|.
"""
import hashlib

import numpy as np
import pytest

import model_reference as mr
import snmpc_reference as sr
import test_snmpc_reference as ts

pytestmark = pytest.mark.gpu

DT, LD, U53 = ts.DT, np.longdouble, sr.U53
_REF = {}


def _instances(B):
    return sorted({b for b in (0, 63, 64, B - 1) if 0 <= b < B})


def _solver(shape, B, kernels):
    from tum_control_amd.solver import CoupledSnmpcSolver
    ns, L, N, uph = shape
    s = CoupledSnmpcSolver(N=N, dt=DT, batch=B, Apce=ts.pce(ns, L), uph=uph, gamma=ts.GAMMA)
    for k in kernels or ():
        s.set_kernel(k)
    s.install_reference_ocp()
    return s


def _device_weights(s):
    """(N + 1, 6): what install_reference_ocp hands to cost_set, by its own expression"""
    mpc = s.cfg["mpc"]
    w = 0.01 * np.array([mpc["q_lon"] / mpc["s_lon"] ** 2, mpc["q_lat"] / mpc["s_lat"] ** 2, mpc["q_yaw"] / mpc["s_yaw"] ** 2, mpc["q_vel"] / mpc["s_vel"] ** 2,
                         mpc["r_jerk"] / mpc["s_jerk"] ** 2, mpc["r_steering_rate"] / mpc["s_steering_rate"] ** 2])
    return np.tile(w, (s.N + 1, 1))


def _penalties(s):
    mpc, N = s.cfg["mpc"], s.N
    z = np.full((N + 1, 3), float(mpc["L1_pen"])); Z = np.full((N + 1, 3), float(mpc["L2_pen"]))
    return (z, z, Z, Z)


def _b(a, B):
    a = np.asarray(a)
    return a[None] if B == 1 else a


def _stacked(s):
    """(B, N + 1, n_s + 1, 8): every copy of every stage"""
    return np.stack([_b(s.get(k, "x"), s.batch).reshape(s.batch, s.ns + 1, 8) for k in range(s.N + 1)], axis=1)


def _slacks(s, rows):
    N = s.N
    out = []
    for f in ("sl", "su"):
        v = np.zeros((len(rows), 3 * N))
        for k in range(N + 1):
            g = _b(s.get(k, f), s.batch)[rows]
            n = 0
            if k < N:
                v[:, k] = g[:, n]; n += 1
            if k >= 1:
                v[:, N + 2 * (k - 1)] = g[:, n]; v[:, N + 2 * (k - 1) + 1] = g[:, n + 1]
        out.append(v)
    return out


def _reference(lin, p, W):
    """both runs of the statement, once per set of inputs (the kernel choices of a shape share the linearisation kernels: same bits)"""
    h = hashlib.sha1()
    for a in [lin[k] for k in sorted(lin)] + [p[k] for k in sorted(p)] + [W]:
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    if key not in _REF:
        _REF[key] = ts.both_runs(lin, p, W)
    return _REF[key]


class _Worst:
    def __init__(self, label):
        self.label, self.dev, self.f64 = label, {}, {}

    def add(self, name, got, ld, f64, scale):
        self.dev[name] = max(self.dev.get(name, 0.0), sr.units(got, ld, scale))
        self.f64[name] = max(self.f64.get(name, 0.0), sr.units(f64, ld, scale))

    def gate(self, name):
        return max(32.0, 4.0 * self.f64[name])

    def check(self):
        for name in self.dev:
            print(f"SQB {self.label} {name}: device {self.dev[name]:.2f} fp64 {self.f64[name]:.2f} gate {self.gate(name):.2f} (u x scale)")
        for name in self.dev:
            assert self.f64[name] <= ts.CAP, (self.label, name, "the statement's own error breaks the cap", self.f64[name])
            assert self.dev[name] <= self.gate(name), (self.label, name, self.dev[name], self.gate(name))


def _solve_and_check(label, s, shape, idx, x0, Y):
    """one solve of `s` at the iterate it holds; the instances idx against the statement. Returns the new stacked iterate."""
    ns, L, N, uph = shape
    nv, B = 2 * N, s.batch
    X = _stacked(s)
    _, U = s.get_iterate()
    W, pen = _device_weights(s), _penalties(s)
    s.solve()
    stat = np.atleast_1d(s.get_stats("status"))
    Xp = _stacked(s)
    Xn, Up = s.get_iterate()
    costs = np.atleast_1d(s.get_cost())
    sl, su = _slacks(s, idx)
    assert np.array_equal(Xn, Xp[:, :, 0]), (label, "the nominal copy of get('x') and of get_iterate differ")
    w = _Worst(label)
    for j, b in enumerate(idx):
        assert stat[b] == 0, (label, b, "status", stat[b])
        lin = {k: v[0] for k, v in s.get_snmpc_linearisation(b, 1).items()}
        lin.pop("cv")          # (the statement forms cl, ct from X itself; cv is held at model level below)
        qp = s.get_condensed_qp(b, 1)
        nvp = qp["H"].shape[-1]
        assert nvp == 16 * (7 if N > 48 else 6 if N > 40 else 5) and qp["C"].shape[1:] == (2 * N, nvp) and qp["dv_valid"]
        H, q, C, d, dv = qp["H"][0], qp["q"][0], qp["C"][0], qp["d"][0], qp["dv"][0]
        p = dict(A=ts.pce(ns, L), x0=x0[b], X=X[b], U=U[b], Y=Y[b])
        ld, f64 = _reference(lin, p, W)
        # ---- 1. the QP within the gate
        w.add("H", H[:nv, :nv], ld["H"], f64["H"], ld["sH"])
        w.dev["H-H'"] = max(w.dev.get("H-H'", 0.0), sr.units(H[:nv, :nv], H[:nv, :nv].T, ld["sH"])); w.f64["H-H'"] = w.f64["H"]
        w.add("q", q[:nv], ld["q"], f64["q"], ld["sq"])
        w.add("C steering", C[0::2, :nv], ld["C"][0::2], f64["C"][0::2], ld["sC"][0::2])
        w.add("C gg", C[1::2, :nv], ld["C"][1::2], f64["C"][1::2], ld["sC"][1::2])
        w.add("d", d, ld["d"], f64["d"], ld["sd"])
        if uph > 1:
            assert (ld["sdmin"] == 0.0) if L == 1 else (ld["sdmin"] > 0.0), (label, b, "sd of a chance row", ld["sdmin"])
        # ---- 2. exact structure
        pad = np.eye(nvp)[nv:]
        assert np.array_equal(H[nv:], pad) and np.array_equal(H[:, nv:], pad.T), (label, b, "padding of H")
        assert not q[nv:].any() and not C[:, nv:].any(), (label, b, "padding of q / the rows")
        for st in range(1, N + 1):
            assert not C[2 * (st - 1) + 1, 2 * st:].any(), (label, b, st, "columns beyond the stage")
        # ---- 3. the expansion and the cost
        assert np.array_equal(Up[b].reshape(-1), U[b].reshape(-1) + dv[:nv]), (label, b, "U+ != U + dv")
        ex = sr.expand(ld["M"], X[b], U[b], x0[b], dv[:nv], dtype=LD)
        ex64 = sr.expand(f64["M"], X[b], U[b], x0[b], dv[:nv], dtype=np.float64)
        w.add("X+ nominal", Xp[b, :, 0], ex["X"][:, 0], ex64["X"][:, 0], ex["sX"][:, 0])
        w.add("X+ samples", Xp[b, :uph + 1, 1:], ex["X"][:uph + 1, 1:], ex64["X"][:uph + 1, 1:], ex["sX"][:uph + 1, 1:])
        for k in range(uph + 1, N + 1):
            assert np.array_equal(Xp[b, k, 1:], Xp[b, uph, 1:]), (label, b, k, "a frozen sample copy differs from stage uph")
        ca = (Xp[b, :, 0], Up[b], Y[b], W, DT, sl[j], su[j]) + pen
        c_ld, c_s = sr.cost(*ca, dtype=LD)
        c_64, _ = sr.cost(*ca, dtype=np.float64)
        w.add("cost", costs[b], c_ld, c_64, c_s)
    w.check()
    return Xp


def _run(shape, kernels, B=3, rti2=False):
    ns, L, N, uph = shape
    s = _solver(shape, B, kernels)
    idx = _instances(B)
    label = f"{shape} {'+'.join(kernels) if kernels else 'auto'} B={B}"
    for kind in ("cold", "excited"):
        ps = [ts.problem(shape, kind, b) for b in range(B)]
        x0 = np.stack([p["x0"] for p in ps]); Y = np.stack([p["Y"] for p in ps])
        X = np.stack([p["X"] for p in ps]); U = np.stack([p["U"] for p in ps])
        s.constraints_set(0, "lbx", x0.reshape(B, -1)); s.constraints_set(0, "ubx", x0.reshape(B, -1))
        s.set_yref_all(Y)
        if kind == "cold":
            s.cold_start()
            assert np.array_equal(_stacked(s), X) and not s.get_iterate()[1].any()
        else:
            for k in range(N + 1):
                s.set(k, "x", X[:, k].reshape(B, -1))
            s.set_iterate(U=U)
        Xp = _solve_and_check(f"{label} {kind}", s, shape, idx, x0, Y)
    if rti2:          # the real-time iteration after the excited one: x0 moved to the new stage-1 states of every copy
        x0 = Xp[:, 1].copy()
        s.constraints_set(0, "lbx", x0.reshape(B, -1)); s.constraints_set(0, "ubx", x0.reshape(B, -1))
        _solve_and_check(f"{label} rti2", s, shape, idx, x0, Y)


def _id(c):
    return "-".join(str(v) for v in c[0]) + ("" if not c[1] else "-" + "+".join(c[1]))


@pytest.mark.parametrize("case", ts.GPU_CASES, ids=_id)
def test_coupled_snmpc_kernels(case):
    shape, kernels = case
    _run(shape, kernels, rti2=shape in ts.RTI2_SHAPES)


@pytest.mark.parametrize("kernel", ["lin-lane-per-stage", "lin-eight-lanes"])
def test_batch_edge(kernel):
    """67 instances of (12, 5): items of several instances in one wavefront of the sample linearisation, shadow lanes behind the last,
    instances 63 | 64"""
    _run((10, 10, 12, 5), (kernel,), B=67)


def test_get_snmpc_linearisation_refusals():
    from tum_control_amd import solver as sv
    shape = (10, 10, 12, 5)
    n = sv.BatchedOcpSolver(N=5, dt=DT, nsub=1, batch=2)
    with pytest.raises(Exception, match="not an SNMPC capsule"):
        sv.CoupledSnmpcSolver.get_snmpc_linearisation(n)
    s = _solver(shape, 2, None)
    with pytest.raises(Exception, match="no solve has run on the pipeline"):
        s.get_snmpc_linearisation()
    ps = [ts.problem(shape, "cold", b) for b in range(2)]
    x0 = np.stack([p["x0"] for p in ps])
    s.constraints_set(0, "lbx", x0.reshape(2, -1)); s.constraints_set(0, "ubx", x0.reshape(2, -1))
    s.set_yref_all(np.stack([p["Y"] for p in ps])); s.cold_start()
    s.solve()
    lin = s.get_snmpc_linearisation()
    assert lin["As"].shape == (2, 5, 10, 8, 8) and lin["Bs"].shape == (2, 5, 10, 8, 2) and lin["An"].shape == (2, 7, 8, 8) and lin["cv"].shape == (2, 13, 2)
    assert s.get_snmpc_linearisation(1, 1)["hs"].shape == (1, 5, 10) and not lin["hs"][:, 0].any() and not lin["ghs"][:, 0].any()
    for b0, nb in ((-1, 1), (0, 3), (2, 1), (1, 2)):
        with pytest.raises(Exception, match="out of bounds"):
            s.get_snmpc_linearisation(b0, nb)
    with sv.dev_library():
        f = sv.CoupledSnmpcSolver(N=12, dt=DT, batch=2, Apce=ts.pce(10, 10), uph=5, gamma=ts.GAMMA, qp_warm_start=False)
    f.install_reference_ocp()
    f.constraints_set(0, "lbx", x0.reshape(2, -1)); f.constraints_set(0, "ubx", x0.reshape(2, -1))
    f.set_yref_all(np.stack([p["Y"] for p in ps])); f.cold_start()
    f.set_kernel("fused")
    f.solve()
    with pytest.raises(Exception, match="fused"):
        f.get_snmpc_linearisation()


# ---------------------------------------------------------------------------------------------- model level
def _report(name, value):
    print(f"SQB model {name} error/bound {value:.4g}")


@pytest.mark.parametrize("kernel", ["lin-lane-per-stage", "lin-eight-lanes"])
def test_h_vabs_of_the_linearisation_kernels(kernel):
    """hs / ghs (snmpc_lin_kernel | snmpc_lin_cols_kernel) and hn / ghn / cv (lin_kernel<true> | lin_cols_kernel<true>) at
    model_reference.h_vabs_points: the sample copies of the stages 1 .. 7 of every instance hold the points in turn, the nominal copy
    of stage k of instance b holds point 8 b + k - 1. The status of the solve is not asserted."""
    from test_model_reference import ratio
    Xh, Lh, rows = ts.h_vabs_reference()
    P = len(Lh)
    N, ns = 8, 10
    B = (P + N - 1) // N
    X = np.tile(mr.HARMLESS, (B, N + 1, ns + 1, 1))
    at_s = {}
    for b in range(B):
        for k in range(1, N):
            for i in range(ns):
                p = ((k - 1) * ns + i + 3 * b) % P
                X[b, k, i + 1] = Xh[p]; at_s[(b, k, i)] = p
        for k in range(1, N + 1):
            if 8 * b + k - 1 < P:
                X[b, k, 0] = Xh[8 * b + k - 1]
    s = _solver((ns, 10, N, N), B, (kernel,))
    s.constraints_set(0, "lbx", X[:, 0].reshape(B, -1)); s.constraints_set(0, "ubx", X[:, 0].reshape(B, -1))
    for k in range(N + 1):
        s.set(k, "x", X[:, k].reshape(B, -1))
    s.set_iterate(U=np.zeros((B, N, 2)))
    s.solve()
    lin = s.get_snmpc_linearisation()
    worst = dict(hs=0.0, hn=0.0, cv=0.0)
    seen = set()
    for (b, k, i), p in at_s.items():
        h, g, info, oh, og, bh, bg = rows[p]
        r = max(ratio(np.array([lin["hs"][b, k, i]]), np.array([h]), np.array([bh])), ratio(lin["ghs"][b, k, i], g, bg))
        worst["hs"] = max(worst["hs"], r); seen.add(p)
        assert r <= 1.0, (kernel, "hs", b, k, i, Lh[p], r)
    for b in range(B):
        for k in range(1, N + 1):
            p = 8 * b + k - 1
            if p >= P:
                continue
            h, g, info, oh, og, bh, bg = rows[p]
            r = max(ratio(np.array([lin["hn"][b, k]]), np.array([h]), np.array([bh])), ratio(lin["ghn"][b, k], g, bg))
            worst["hn"] = max(worst["hn"], r)
            assert r <= 1.0, (kernel, "hn", b, k, Lh[p], r)
            vl, vt = LD(Xh[p, 3]), LD(Xh[p, 4])
            va = np.sqrt(vl * vl + vt * vt)
            want = np.array([vl / va, vt / va] if va > 0 else [0, 0], dtype=LD)
            err = np.abs(lin["cv"][b, k].astype(LD) - want)
            rc = float(np.max(np.where(err == 0, LD(0), err / np.where(want == 0, LD(1e-300), 4 * LD(U53) * np.abs(want)))))
            worst["cv"] = max(worst["cv"], rc)
            assert rc <= 1.0, (kernel, "cv", b, k, Lh[p], rc)
    assert seen == set(range(P))
    for k, v in worst.items():
        _report(f"{kernel} {k}", v)


@pytest.mark.parametrize("kernel", ["lin-lane-per-stage", "lin-eight-lanes"])
def test_sample_records_against_the_exact_model(kernel):
    """As, Bs, bs + x_{k+1} of snmpc_lin_kernel / snmpc_lin_cols_kernel at every model point with u = 0 (the copies of a stage share
    one input), all 8 x 8 + 8 x 2 + 8 entries"""
    from test_gpu_model_reference import dev_bound, _worst_entry
    from test_model_reference import fixture, point_bounds, ratio
    g = fixture()
    ns, N = 10, 8
    P = len(g["labels"])
    per = (N // 2) * ns
    B = (P + per - 1) // per
    X = np.tile(mr.HARMLESS, (B, N + 1, ns + 1, 1)); where = []
    for p in range(P):
        b, r = p // per, p % per
        k, i = 2 * (r // ns), r % ns
        X[b, k, i + 1] = g["X"][p]; X[b, k + 1, i + 1] = g["Phi1_u0"][p]
        where.append((b, k, i))
    s = _solver((ns, 10, N, N), B, (kernel,))
    s.constraints_set(0, "lbx", X[:, 0].reshape(B, -1)); s.constraints_set(0, "ubx", X[:, 0].reshape(B, -1))
    for k in range(N + 1):
        s.set(k, "x", X[:, k].reshape(B, -1))
    s.set_iterate(U=np.zeros((B, N, 2)))
    s.solve()
    lin = s.get_snmpc_linearisation()
    bounds = point_bounds(1, "_u0")
    worst, at = 0.0, None
    for p, (b, k, i) in enumerate(where):
        bd = bounds[p][1]
        for q, got, want in (("Phi", lin["bs"][b, k, i] + X[b, k + 1, i + 1], g["Phi1_u0"][p]), ("A", lin["As"][b, k, i], g["A1_u0"][p]),
                             ("B", lin["Bs"][b, k, i], g["B1_u0"][p])):
            bnd = dev_bound(bd, q, want)
            r = ratio(got, want, bnd)
            if r > worst:
                worst, at = r, _worst_entry(p, q, got, want, bnd)
    _report(f"{kernel} sample records", worst)
    assert worst <= 1.0, (worst, at)


@pytest.mark.parametrize("kernel", ["lin-lane-per-stage", "lin-eight-lanes"])
def test_nominal_records_beyond_uph_against_the_exact_model(kernel):
    """An, Bn, bn + x_{k+1} of lin_kernel<true> / lin_cols_kernel<true> on the stages >= uph (uph = 0: every stage) at every model point"""
    from test_gpu_model_reference import dev_bound, _staged, _worst_entry
    from test_model_reference import fixture, point_bounds, ratio
    g = fixture()
    ns, N = 10, 8
    Xi, Ui, where = _staged(N, 1)
    B = Xi.shape[0]
    X = np.tile(mr.HARMLESS, (B, N + 1, ns + 1, 1)); X[:, :, 0] = Xi
    s = _solver((ns, 10, N, 0), B, (kernel,))
    s.constraints_set(0, "lbx", X[:, 0].reshape(B, -1)); s.constraints_set(0, "ubx", X[:, 0].reshape(B, -1))
    for k in range(N + 1):
        s.set(k, "x", X[:, k].reshape(B, -1))
    s.set_iterate(U=Ui)
    s.solve()
    lin = s.get_snmpc_linearisation()
    bounds = point_bounds(1, "")
    worst, at = 0.0, None
    for p, (b, k) in enumerate(where):
        bd = bounds[p][1]
        for q, got, want in (("Phi", lin["bn"][b, k] + Xi[b, k + 1], g["Phi1"][p]), ("A", lin["An"][b, k], g["A1"][p]), ("B", lin["Bn"][b, k], g["B1"][p])):
            bnd = dev_bound(bd, q, want)
            r = ratio(got, want, bnd)
            if r > worst:
                worst, at = r, _worst_entry(p, q, got, want, bnd)
    _report(f"{kernel} nominal records", worst)
    assert worst <= 1.0, (worst, at)
