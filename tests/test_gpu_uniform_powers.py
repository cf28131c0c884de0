"""
The record-free condensing of a stage-uniform iterate in its POWER form (options_set("uniform_powers", 1), the default):
cond_uniform_kernel computes the sequences P_m = A^m B and g_{s+1} = A g_s + defect once per instance, on three DPP rows of the
wavefront, and the stages read them from LDS tables -- against the COLUMN form (options_set("uniform_powers", 0),
cond_uniform_columns_kernel), in which every lane carries its column of G through every stage.

Every case is a pair of TWIN capsules that differ in "uniform_powers" only.

Bound: bit equality (np.array_equal) of everything a solve leaves behind -- X, U, cost, status, qp_iter, and with them qp_status,
the residuals of the QP, sl, su and lam of every stage. The power form builds every entry of a sequence by the column form's FMAs on
the column form's operands in its order (the rows A leaves alone are carried, not summed with zero coefficients), the gradient sums
and the matrix instructions take the same operands in the same order: there is no rounding to allow for. (A column that is not there
yet is a read of +0.0 where the column form may hold -0.0; sums that start from +0.0 do not see the difference.)
No accessor reaches q and d of the hand-over without leaving the record-free chain (the debug dump and store_qp_in both keep the
records); they are compared through what the interior point method makes of them.

Shapes: batch 1025 is the smallest that takes the record-free chain (one wavefront per OCP in the condensing, the expansion a kernel of
its own). Horizons 38, 40 | 41, 48 | 49, 56: a part-filled and a full last segment of the five-, six- and seven-tile builds; 24 and
32: no stage with a column beyond the first 64 (the second bank of the gradient and of the gg row is not issued before stage 33).

Inputs: what the per-stage code handles and a table could get wrong -- x0 random with yaws on both sides of +-pi and of 0, a
reference that differs at every stage and instance (inputs' reference included), the diagonal of W different at every stage and
instance (cost_set per stage) and W_e different again. cold_start() sets U = 0 and the API has no other way to a stage-uniform iterate
with U != 0 (set() invalidates it): the inputs' share of the linearisation is exercised through the states 6 and 7 of x0.

get_stats("records_skipped") counts the solve on both twins: both took the chain. A second solve on the now non-uniform iterate runs
cond_kernel on both; the switch must not leak into it.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.08
B0 = 1025


@functools.lru_cache(maxsize=None)
def _problem(N):
    """x0 (B, 8), yref (B, N + 1, 6), diagonals of W (B, N, 6) and W_e (B, 4): read-only, shared by the twins"""
    rng = np.random.default_rng(7000 + N)
    B = B0
    x0 = np.zeros((B, 8))
    x0[:, 0:2] = 50.0 * rng.standard_normal((B, 2))
    # yaws: a quarter each just below / above +pi, -pi and around 0 (wrap_yaw maps to [0, 2 pi)), the rest anywhere
    centre = np.array([np.pi, -np.pi, 0.0, 0.0])[np.arange(B) % 4]
    spread = np.where(np.arange(B) % 4 == 3, np.pi, 0.05)
    x0[:, 2] = centre + spread * rng.uniform(-1.0, 1.0, B)
    x0[:, 3] = rng.uniform(5.0, 40.0, B)
    x0[:, 4] = 0.3 * rng.standard_normal(B)
    x0[:, 5] = 0.1 * rng.standard_normal(B)
    x0[:, 6] = 0.02 * rng.standard_normal(B)
    x0[:, 7] = 1.0 * rng.standard_normal(B)
    # the reference: straight on at the current speed, wrapped as the solver wraps the yaw, plus noise of its own at every stage
    t = DT * np.arange(N + 1)[None, :]
    yaw_w = np.mod(x0[:, 2], 2.0 * np.pi)
    yref = np.zeros((B, N + 1, 6))
    yref[:, :, 0] = x0[:, 0:1] + x0[:, 3:4] * t * np.cos(x0[:, 2:3]) + 0.2 * rng.standard_normal((B, N + 1))
    yref[:, :, 1] = x0[:, 1:2] + x0[:, 3:4] * t * np.sin(x0[:, 2:3]) + 0.2 * rng.standard_normal((B, N + 1))
    yref[:, :, 2] = yaw_w[:, None] + 0.02 * rng.standard_normal((B, N + 1))
    yref[:, :, 3] = x0[:, 3:4] + 0.5 * rng.standard_normal((B, N + 1))
    yref[:, :, 4] = 0.1 * rng.standard_normal((B, N + 1))
    yref[:, :, 5] = 0.01 * rng.standard_normal((B, N + 1))
    wf = rng.uniform(0.5, 1.5, (B, N, 6))
    wef = rng.uniform(0.5, 1.5, (B, 4))
    for a in (x0, yref, wf, wef):
        a.setflags(write=False)
    return x0, yref, wf, wef


def _mk(N, powers):
    from tum_control_amd.solver import BatchedOcpSolver
    x0, yref, wf, wef = _problem(N)
    s = BatchedOcpSolver(N=N, dt=DT, nsub=3, batch=B0)
    s.install_reference_ocp()
    s.options_set("uniform_powers", powers)
    # the installed diagonal, scaled per stage and instance
    mpc = s.cfg["mpc"]
    q = np.array([mpc["q_lon"] / mpc["s_lon"] ** 2, mpc["q_lat"] / mpc["s_lat"] ** 2, mpc["q_yaw"] / mpc["s_yaw"] ** 2,
                  mpc["q_vel"] / mpc["s_vel"] ** 2, mpc["r_jerk"] / mpc["s_jerk"] ** 2, mpc["r_steering_rate"] / mpc["s_steering_rate"] ** 2])
    eye6, eye4 = np.eye(6)[None], np.eye(4)[None]
    for k in range(N):
        s.cost_set(k, "W", eye6 * (0.01 * q * wf[:, k])[:, None, :])
    s.cost_set(N, "W", eye4 * (0.01 * q[:4] * wef)[:, None, :])
    s.set_x0(x0); s.set_yref_all(yref)
    return s


def _snap(s):
    X, U = s.get_iterate()
    r = dict(X=X, U=U, cost=np.atleast_1d(s.get_cost()), status=s.get_stats("status"), qp_iter=s.get_stats("qp_iter"),
             qp_status=s.get_stats("qp_status"), res=np.atleast_2d(s.get_stats("res")))
    for f in ("sl", "su", "lam"):
        r[f] = np.concatenate([np.atleast_2d(s.get(k, f)).reshape(s.batch, -1) for k in range(s.N + 1)], axis=1)
    return r


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    differ = []
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])          # (a failed instance carries NaN on both sides)
        print(what, k, "max |difference|", float(np.nanmax(np.abs(x.astype(float) - y.astype(float)))) if x.size else 0.0)
        if not (x.shape == y.shape and np.array_equal(x, y, equal_nan=(x.dtype.kind == "f"))):
            differ.append(k)
    assert not differ, (what, differ)


@pytest.mark.parametrize("N", [24, 32, 38, 40, 41, 48, 49, 56])
def test_power_form_equals_column_form(N):
    p, c = _mk(N, 1), _mk(N, 0)
    for s in (p, c):
        s.cold_start()
        s.solve()
    # both twins took the record-free chain
    assert p.get_stats("records_skipped") == 1 and c.get_stats("records_skipped") == 1
    assert p.get_stats("lin_uniform") == 1 and c.get_stats("lin_uniform") == 1
    a, b = _snap(p), _snap(c)
    print(f"N={N}: instances solved", int((a["status"] == 0).sum()), "of", B0, "qp_iter", int(a["qp_iter"].min()), "..", int(a["qp_iter"].max()))
    assert (a["status"] == 0).sum() > B0 // 2          # (the comparison is of solves, not of failures)
    _assert_same(a, b, f"N={N}")
    # the second solve: the iterate is uniform no more, cond_kernel runs on both
    for s in (p, c):
        s.solve()
    assert p.get_stats("records_skipped") == 1 and c.get_stats("records_skipped") == 1
    assert p.get_stats("lin_uniform") == 1 and c.get_stats("lin_uniform") == 1
    _assert_same(_snap(p), _snap(c), f"N={N}, second solve")
    p.synchronize(); c.synchronize()


def test_uniform_powers_option_validation():
    from tum_control_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(N=8, dt=DT, nsub=3, batch=4)
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception, match="uniform_powers"):
            s.options_set("uniform_powers", bad)
    with pytest.raises(Exception, match="uniform_powers"):          # the "unknown field" message lists the field
        s.options_set("no_such_option", 1)
    s.options_set("uniform_powers", 0); s.options_set("uniform_powers", 1)
