"""
plant_advance_kernel (csrc/loop_kernels.hpp, K9) held to the exact statement of tests/plant_reference.py:

(a) plant_xdot itself through tests/device/plant_probe.hip -- a test-only translation unit compiled once per module into pytest's
    temporary directory and loaded with ctypes (a missing compiler is a failure here): four lanes per point, all four lanes' results;
(b) one control step through the shipped kernel over the C-ABI: a small nominal capsule (N = 4) solves once on a race-line state
    (tum_sim_advance refuses before the first solve; the status words are 0), then per case set_state, set_iterate with the test's
    X[1][7] = a and U[0][1] = sr, advance, and x_sim / x_mpc / pose read back. Batches 1, 15, 16, 17, 33 (sixteen vehicles per 64-lane
    block: the last quad of a block, the first of the next, padding quads), every instance another point; (Ts, n_elem) = (0.02, 4) as
    shipped, (0.02, 1) and (plant_reference.LARGE_TS, 1);
(c) the disturbed pass: w only, e only, both, and a control step past the realisation's length;
(d) the estimator: seven advances (the four-slot ring is reused) with windows all 1, the shipped ones and a set in which every role
    and both of its states see another window;
(e) the logged rows of one step.

The gate of an entry is gate_units x unit + device term: gate_units = max(32, 4 x the plain binary64 statement's largest error in the
point's class / variant group and channel) in the units of plant_reference, the device term what fast_atan / fast_sincos may err
beyond libm's ulp (plant_reference's docstring). Nothing in a gate comes from a device result. Every test prints what the device
needed of its gate, and the plain statement's share beside it ("plant_bounds ..." lines): profiles/plant_bounds.txt.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import plant_reference as pr
from test_gpu_model_reference import _header_sincos_constants
from test_plant_reference import WINDOW_SETS, case_inputs, gate_units, plain_errors, plain_estimator_errors, probe_command, FLOOR

pytestmark = pytest.mark.gpu

N = 4
BATCHES = (1, 15, 16, 17, 33)
_dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def _report(name, dev, plain):
    print(f"plant_bounds {name}: device needed {dev:.4g} of its gate, the plain statement {plain:.4g}")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def plant_model_constants():
    """the 21 doubles of PlantModel as vehicle_constants (csrc/tum_nmpc.hip) folds them from the description, in binary64, same operations"""
    c = pr.config_numbers()
    lf, lr, m, Iz, g = c["lf"], c["lr"], c["m"], c["Iz"], c["g"]
    Fz_f, Fz_r = m * lr * g / (lf + lr), m * lf * g / (lf + lr)
    inv = lambda Fz, C: 1.0 / math.sqrt(Fz * Fz + (C * Fz) * (C * Fz))
    return np.array([lf, lr, m, 1.0 / m, 1.0 / Iz, 0.5 * c["ro"] * c["S"] * c["Cd"], c["Bf"], c["Cf"], c["Df"], c["Ef"], c["Br"], c["Cr"], c["Dr"], c["Er"],
                     Fz_f, Fz_r, inv(Fz_f, c["Cf"]), inv(Fz_r, c["Cr"]), c["fr0"], c["fr1"], c["fr4"]], dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def _sincos_delta():
    pr.set_sincos_delta(*_header_sincos_constants())


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plant_probe") / "libplant_probe.so")
    r = subprocess.run(probe_command(out), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(out), "the probe does not compile:\n" + r.stdout + r.stderr
    L = ctypes.CDLL(out)
    L.probe_plant_xdot.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_int]
    return L


def shares(got, refs, gates):
    """largest |got - exact| / (gate_units x unit + device term) over the entries of rows; refs: reference dicts, gates (rows, channels)"""
    worst, at = 0.0, None
    for i, (g, r) in enumerate(zip(got, refs)):
        bound = gates[i] * np.array(r["unit"]) + np.array(r["dev"])
        e = pr.errors(g, r["value"], bound)
        if e.max() > worst:
            worst, at = float(e.max()), (i, int(e.argmax()))
    return worst, at


# ---------------------------------------------------------------------------------------------- (a) plant_xdot
def test_plant_xdot_through_the_probe(probe):
    """all four lanes of every quad end with the same seven numbers to the bit, each within its gate of the exact xdot; the last block
    is partly filled"""
    p = pr.points()
    X, A, SR = p["X"], p["A"], p["SR"]
    n = len(A)
    assert (4 * n) % 64 != 0 and 4 * n > 64
    au = np.ascontiguousarray(np.stack([A, SR], axis=1))
    out = np.zeros((n, 4, 7))
    rc = probe.probe_plant_xdot(_p(plant_model_constants()), _p(np.ascontiguousarray(X)), _p(au), _p(out), n)
    assert rc == 0, f"plant_probe: HIP status {rc}"
    for lane in range(1, 4):
        assert same_bits(out[:, lane], out[:, 0]), lane
    refs = [pr.xdot(X[i], A[i], SR[i], dev=True) for i in range(n)]
    plain = plain_errors("xdot")
    gates = gate_units(plain)
    worst, at = shares(out[:, 0], refs, gates)
    groups = np.array(pr.groups())
    for name in sorted(set(groups)):
        m = np.flatnonzero(groups == name)
        w, _ = shares(out[m, 0], [refs[i] for i in m], gates[m])
        _report(f"xdot {name}", w, float((plain[m] / gates[m]).max()))
    _report("xdot", worst, float((plain / gates).max()))
    assert worst <= 1.0, (worst, at, p["label"][at[0]])


# ---------------------------------------------------------------------------------------------- the shipped kernel over the C-ABI
class Rig:
    """one capsule per batch size, solved once; loops of any (Ts, n_elem, windows) on it"""

    def __init__(self, B):
        from tum_control_amd.planner import load_track
        from tum_control_amd.solver import BatchedOcpSolver
        from tum_control_amd.workloads import nominal_batch
        x0, yref = nominal_batch(B, N=N)
        s = self.s = BatchedOcpSolver(N=N, dt=0.08, nsub=3, batch=B)
        s.install_reference_ocp()
        s.set_x0(x0); s.set_yref_all(yref); s.cold_start()
        assert s.solve() == 0 and (np.atleast_1d(s.get_stats("status")) == 0).all()
        self.B, self.track = B, load_track("monteblanco")

    def loop(self, Ts=pr.TS, n_elem=pr.N_ELEM, windows=WINDOW_SETS["shipped"], log_capacity=0):
        from tum_control_amd.solver import DeviceClosedLoop
        return DeviceClosedLoop(self.s, self.track, 3.04, Ts=Ts, n_elem=n_elem, windows=windows, log_capacity=log_capacity)

    def iterate(self, x_mpc, a, sr):
        """an iterate whose X[1][7] = a and U[0][1] = sr and whose neighbouring entries are something else"""
        B = self.B
        X = np.tile(np.asarray(x_mpc)[:, None, :], (1, N + 1, 1)); U = np.zeros((B, N, 2))
        X[:, 0, 7] = a + 1.0; X[:, 1, 7] = a; X[:, 2, 7] = a - 1.0
        U[:, 0, 0] = 0.25 + 0.01 * np.arange(B); U[:, 0, 1] = sr; U[:, 1, 1] = sr + 0.5
        self.s.set_iterate(X=X, U=U)
        return X, U

    def start(self, loop, idx):
        p = pr.points()
        x_sim = p["X"][idx]
        x_mpc = np.concatenate([x_sim, 0.5 * p["A"][idx, None]], axis=1)
        loop.set_state(x_sim, x_mpc, cold_start=False)
        return x_sim, x_mpc

    def one_step(self, loop, idx):
        p = pr.points()
        x_sim, x_mpc = self.start(loop, idx)
        X, U = self.iterate(x_mpc, p["A"][idx], p["SR"][idx])
        loop.advance()
        return loop.get("x_sim"), loop.get("x_mpc"), loop.get("pose"), (x_sim, x_mpc, X, U)


_RIGS = {}


@pytest.fixture(scope="module")
def rigs():
    def get(B):
        if B not in _RIGS:
            _RIGS[B] = Rig(B)
        return _RIGS[B]
    yield get
    _RIGS.clear()


def batch_points(B, shift):
    """the points of a batch: consecutive (mod P) from where the smaller batches ended, so that the five batches together pass every
    point but four and the three steps start at different places"""
    P = len(pr.points()["A"])
    return (shift + sum(b for b in BATCHES if b < B) + np.arange(B)) % P


# ---------------------------------------------------------------------------------------------- (b) one control step
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("step", range(len(pr.STEPS)))
def test_one_control_step(rigs, B, step):
    """x_sim against the exact step; pose its first two entries and x_mpc (first sample of every window) the new state and a, to the bit"""
    Ts, ne = pr.STEPS[step]
    p = pr.points()
    idx = batch_points(B, 29 * step)
    assert len(set(idx.tolist())) == B
    rig = rigs(B)
    loop = rig.loop(Ts, ne)
    x_sim, x_mpc, pose, _ = rig.one_step(loop, idx)
    del loop
    refs = [pr.step(p["X"][i], p["A"][i], p["SR"][i], Ts, ne, dev=True) for i in idx]
    plain = plain_errors("step", Ts, ne)
    gates = gate_units(plain)[idx]
    worst, at = shares(x_sim, refs, gates)
    _report(f"step Ts={Ts} n_elem={ne} batch={B}", worst, float((plain[idx] / gates).max()))
    assert worst <= 1.0, (worst, at, p["label"][idx[at[0]]])
    assert same_bits(pose, x_sim[:, :2])
    assert same_bits(x_mpc[:, :7], x_sim) and same_bits(x_mpc[:, 7], p["A"][idx])


# ---------------------------------------------------------------------------------------------- (c) the disturbed pass
def test_disturbed_pass(rigs):
    """w, e, both: the true state is that of the undisturbed step to the bit; x_mpc (windows 1: the fed state) against the exact sim_step.
    A control step past the realisation's length runs undisturbed again."""
    B = 17
    p = pr.points()
    idx = batch_points(B, 0)
    rig = rigs(B)
    loop = rig.loop(windows=WINDOW_SETS["ones"])
    base, base_mpc, _, _ = rig.one_step(loop, idx)
    loop.advance()
    base2, base2_mpc = loop.get("x_sim"), loop.get("x_mpc")
    assert same_bits(base_mpc[:, :7], base) and same_bits(base2_mpc[:, :7], base2) and not same_bits(base, base2)
    for case in ("w", "e", "we"):
        W, E = case_inputs(case)
        loop.set_disturbances(None if W is None else W[None, idx], None if E is None else E[None, idx])
        x_sim, x_mpc, pose, _ = rig.one_step(loop, idx)
        assert same_bits(x_sim, base) and same_bits(pose, base[:, :2]), case
        assert not same_bits(x_mpc[:, :7], x_sim), case
        refs = [pr.sim_step(p["X"][i], p["A"][i], p["SR"][i], None if W is None else W[i], None if E is None else E[i], dev=True)[1] for i in idx]
        plain = plain_errors("fed", pr.TS, pr.N_ELEM, case)
        gates = gate_units(plain)[idx]
        worst, at = shares(x_mpc, refs, gates)
        _report(f"fed state case={case}", worst, float((plain[idx] / gates).max()))
        assert worst <= 1.0 and same_bits(x_mpc[:, 7], p["A"][idx]), (case, worst, at, p["label"][idx[at[0]]])
        # the realisation holds one control step: the second one is past it
        loop.advance()
        assert same_bits(loop.get("x_sim"), base2) and same_bits(loop.get("x_mpc"), base2_mpc), case
    loop.set_disturbances(None, None)
    x_sim, x_mpc, _, _ = rig.one_step(loop, idx)
    assert same_bits(x_sim, base) and same_bits(x_mpc, base_mpc)


# ---------------------------------------------------------------------------------------------- (d) the estimator
def _sequence(rig, loop, idx, steps, W, E):
    """`steps` advances with a new (a, sr) each; returns x_sim (steps, B, 7), x_mpc (steps, B, 8) and the a of every step"""
    p = pr.points()
    loop.set_disturbances(W, E)
    _, x_mpc0 = rig.start(loop, idx)
    xs, xm, av = [], [], []
    for k in range(steps):
        a = p["A"][idx] * (1.0 - 0.15 * k) + 0.05 * k
        rig.iterate(x_mpc0, a, p["SR"][idx] * (1.0 - 0.3 * k))
        loop.advance()
        xs.append(loop.get("x_sim")); xm.append(loop.get("x_mpc")); av.append(a)
    return np.array(xs), np.array(xm), np.array(av)


def test_estimator_windows_and_ring(rigs):
    """windows all 1: x_mpc is the fed sample itself (with neither w nor e the true state), bit for bit. The shipped windows and the
    mixed set: x_mpc of every step against the exact mean of those binary64 samples, fill phase and reused ring slots included; the
    eighth state is the a the test set."""
    B, steps = 17, 7
    p = pr.points()
    idx = batch_points(B, 40)
    rig = rigs(B)
    k = np.arange(steps)[:, None, None]
    W = p["W"][None, idx] * (1.0 - 0.2 * k); E = p["E"][None, idx] * (0.5 + 0.1 * k)
    loop = rig.loop(windows=WINDOW_SETS["ones"])
    xs0, xm0, a0 = _sequence(rig, loop, idx, steps, None, None)
    assert same_bits(xm0[:, :, :7], xs0) and same_bits(xm0[:, :, 7], a0)
    xs, S, av = _sequence(rig, loop, idx, steps, W, E)          # S: the fed samples
    del loop
    assert same_bits(xs, xs0) and same_bits(S[:, :, 7], av) and not same_bits(S[:, :, :7], xs)
    for name in ("shipped", "mixed"):
        win = WINDOW_SETS[name]
        loop = rig.loop(windows=win)
        xs1, xm, _ = _sequence(rig, loop, idx, steps, W, E)
        del loop
        assert same_bits(xs1, xs), name          # (the same samples went in)
        plain = plain_estimator_errors(name).max(axis=(0, 1))
        gate = np.maximum(FLOOR, 4.0 * plain)
        worst, at = 0.0, None
        for t in range(steps):
            for b in range(B):
                ex = [pr.moving_average(S[:t + 1, b, i], win[i]) for i in range(8)]
                e = pr.errors(xm[t, b], [v[0] for v in ex], [v[1] * g for v, g in zip(ex, gate)])
                if e.max() > worst:
                    worst, at = float(e.max()), (t, b, int(e.argmax()))
        _report(f"estimator windows={name}", worst, float((plain / gate).max()))
        assert worst <= 1.0, (name, worst, at)
        if win[7] == 1:
            assert same_bits(xm[:, :, 7], av)


# ---------------------------------------------------------------------------------------------- (e) the logs
def test_logged_rows_of_one_step(rigs):
    """CiLX, MPC_SimX, simU, simREF of a logged step are, to the bit, the words the test put in or read back"""
    B = 16
    idx = batch_points(B, 0)
    rig = rigs(B)
    loop = rig.loop(log_capacity=2)
    rig.start(loop, idx)
    loop.plan()
    ref0 = loop.get("ref0")
    x_new, _, _, (x_sim, x_mpc, X, U) = rig.one_step(loop, idx)          # (set_state again: the logs restart at row 0)
    lg = loop.logs()
    assert lg["CiLX"].shape == (2, B, 7) and lg["MPC_SimX"].shape == (2, B, 8) and lg["simU"].shape == (1, B, 2) and lg["simREF"].shape == (1, B, 4)
    assert same_bits(lg["CiLX"][0], x_sim) and same_bits(lg["CiLX"][1], x_new)
    assert same_bits(lg["MPC_SimX"][0], x_mpc) and same_bits(lg["MPC_SimX"][1], X[:, 1])
    assert same_bits(lg["simU"][0], U[:, 0]) and (lg["simSolverDebug"][0, :, 4] == 0).all()
    assert same_bits(lg["simREF"][0], ref0) and same_bits(loop.get("ref0"), ref0) and np.abs(ref0).min(axis=1).max() > 0
    print("plant_bounds logged rows: CiLX, MPC_SimX, simU, simREF bit-equal")
