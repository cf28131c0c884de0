"""
Segment scoring on the device (segment_score_kernel / segment_group_kernel, tum_sim_segments_attach, tum_sim_run_segments) against the host
statement of the same rules on the same run's logs (closed_loop.segment_scores_from_logs, held to the reference's own log file by
tests/test_segments_host.py). Shipped tracks, the 26 weight sets of tests/golden/closed_loop_monteblanco_150.npz, N = 38.

The floating-point gate, 1e-12 absolute + relative: kernel and host read bit-identical inputs (the logs store exactly the words the
kernel reads), so what differs is the device's sin / cos / sqrt, a few ulp, and the order of roundings over at most 105 terms of size
O(1 m), O(1 m/s): of the order 1e-15.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12
INT_FIELDS = ("steps", "state", "qp_failures")
FLOAT_FIELDS = ("max_lat_dev", "rms_vel_dev", "max_a_comb")
FLAG_FIELDS = ("crashed", "done", "timed_out")


def _params(golden_dir, B):
    P = np.load(os.path.join(golden_dir, "closed_loop_monteblanco_150.npz"))["params"]
    return P[np.arange(B) % len(P)]


def _loop(B, params, starts, log_capacity, controller="nominal"):
    from tum_control_amd.closed_loop import ClosedLoopBatch
    return ClosedLoopBatch("monteblanco", batch=B, params=params, N=38, Tp=3.04, idx_start=starts, on_device=True,
                           log_capacity=log_capacity, controller=controller)


def _series(cl, logs):
    """host series of a run: signed lat_dev, a_comb and the planner's index, (steps, B) each"""
    from tum_control_amd import closed_loop as clm
    from tum_control_amd.planner import closest_index
    S = logs["simREF"].shape[0]
    lat, _, ac = clm.segment_step_channels(logs["CiLX"][:S], logs["simREF"], logs["MPC_SimX"][1:S + 1, :, 7], cl.cfg)
    return lat, ac, closest_index(cl.track, logs["CiLX"][:S, :, :2])


def _between(values, lo, hi):
    """a threshold in (lo, hi): the middle of the widest gap between neighbouring values of the series in [lo, hi]"""
    v = np.unique(values[(values >= lo) & (values <= hi)])
    assert len(v) >= 2 and v[0] == lo and v[-1] == hi
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1])


def _outcomes(lat, ac, idx, end, thr_lat, thr_ac, n):
    """state words after n steps, from the first step of every event -- used only to CHOOSE thresholds; what is asserted comes from
    closed_loop.segment_scores_from_logs"""
    def first(mask):
        m = mask[:n]
        return np.where(m.any(axis=0), m.argmax(axis=0), n)
    t1, t2, t4 = first((idx == end[None, :]) & (end[None, :] >= 0)), first(lat > thr_lat), first(ac > thr_ac)
    t = np.minimum(t1, np.minimum(t2, t4))
    return np.where(t < n, 1 * (t1 == t) + 2 * (t2 == t) + 4 * (t4 == t), 0)


def _covers(st, acomb_too):
    return bool((st == 1).any() and (st & 2).any() and (st == 0).any() and ((st & 4).any() or not acomb_too))


def _cut(logs, n):
    return {k: v[:n + (1 if k in ("CiLX", "MPC_SimX") else 0)] for k, v in logs.items()}


def _assert_same_logs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _assert_scores(dev, host, rows=slice(None)):
    for k in INT_FIELDS + FLAG_FIELDS:
        assert np.array_equal(np.asarray(dev[k])[rows], np.asarray(host[k])[rows]), (k, dev[k], host[k])
    for k in FLOAT_FIELDS:
        d, h = dev[k][rows], host[k][rows]
        err = np.abs(d - h) / (1.0 + np.abs(h))
        print(k, "max err", err.max())
        assert (np.abs(d - h) <= TOL + TOL * np.abs(h)).all(), (k, err.max())


def _host(cl, logs, end, thr_lat, thr_ac, first_step=0):
    from tum_control_amd.closed_loop import segment_scores_from_logs
    return segment_scores_from_logs(logs, cl.track, end, thr_lat, thr_ac, cl.cfg, first_step=first_step)


# ------------------------------------------------------------------------------------------------ 1 + 3: scores and groups, B = 70
B1, N1A, N1B = 70, 75, 30
GROUPS1 = np.array([0, 1, 3, 10, 70])          # sizes 1, 2, 7, 60


@pytest.fixture(scope="module")
def scored(golden_dir):
    """One run with logs and nothing attached; end indices and thresholds chosen from its logs; a fresh identical loop with segments
    attached: 75 steps through run(75) (the captured step body, replayed three times), then 30 steps of plain launches."""
    B = B1
    params = _params(golden_dir, B)
    starts = np.array([0, 350, 800])[np.arange(B) % 3]
    ref = _loop(B, params, starts, N1A + N1B)
    ref.dev.run(N1A); ref.dev.run(N1B)
    logs0 = ref.dev.logs()
    lat, ac, idx = _series(ref, logs0)
    S = N1A + N1B
    assert lat.shape == (S, B)
    # ends: the planner's index at steps 10, 37, 60 and 0 (done in the very first step), and "never" for every fifth instance
    kind = np.arange(B) % 5
    end = np.where(kind == 0, idx[10], np.where(kind == 1, idx[37], np.where(kind == 2, idx[60], np.where(kind == 4, idx[0], -1))))
    # thresholds: each in the middle of a gap of the WHOLE series, between the maxima of two of the instances that never end, and
    # the first pair with which the run shows every outcome (_outcomes): a crash by lat_dev inside the replayed chunks, one by
    # a_comb, segments done and segments still active
    never = np.nonzero(kind == 3)[0]
    mlat, mac = np.sort(lat[:N1A, never].max(axis=0)), np.sort(ac[:, never].max(axis=0))
    pairs = [(_between(lat, mlat[i], mlat[i + 1]), _between(ac, mac[j], mac[j + 1]))
             for i in range(len(never) - 2, -1, -1) for j in range(len(never) - 2, -1, -1)]
    good = [p for p in pairs if _covers(_outcomes(lat, ac, idx, end, p[0], p[1], N1A), False) and _covers(_outcomes(lat, ac, idx, end, p[0], p[1], S), True)]
    assert good, "no pair of thresholds shows every outcome on this run"
    thr_lat, thr_ac = good[0]
    assert np.abs(lat - thr_lat).min() > 1e-9 and np.abs(ac - thr_ac).min() > 1e-9
    cl = _loop(B, params, starts, S)
    cl.dev.attach_segments(end, thr_lat, thr_ac, group_offsets=GROUPS1)
    cl.dev.run(N1A)
    graph_steps = cl.dev.graph_steps
    seg_a = cl.dev.segments()
    active_a = cl.dev.segments_active
    cl.dev.run(N1B)
    seg_b = cl.dev.segments()
    groups = cl.dev.segment_groups()
    logs1 = cl.dev.logs()
    host_a = _host(ref, _cut(logs0, N1A), end, thr_lat, thr_ac)
    host_b = _host(ref, logs0, end, thr_lat, thr_ac)
    return dict(logs0=logs0, logs1=logs1, seg_a=seg_a, seg_b=seg_b, host_a=host_a, host_b=host_b, groups=groups, end=end,
                graph_steps=graph_steps, active_a=active_a, thr=(thr_lat, thr_ac))


def test_attaching_changes_nothing_the_loop_computes(scored):
    assert scored["graph_steps"] == 25          # the 75 steps were three replays of the captured chunk
    _assert_same_logs(scored["logs0"], scored["logs1"])


def test_the_inputs_cover_every_outcome(scored):
    """so that the comparison cannot pass empty: done, both kinds of crash, still active, a bit set in the very first step"""
    st = scored["host_a"]["state"]
    print("states after 75 steps", np.bincount(st, minlength=8), "after 105", np.bincount(scored["host_b"]["state"], minlength=8))
    assert (st == 1).any() and (st & 2).any() and (st == 0).any()          # a crash inside the replayed chunks
    h = scored["host_b"]
    st = h["state"]
    assert (st == 1).any() and (st & 2).any() and (st & 4).any() and (st == 0).any()
    assert ((st != 0) & (h["steps"] == 1)).any()
    assert h["done"].any() and h["crashed"].any() and h["timed_out"].any()
    assert (scored["host_b"]["steps"] == N1A + N1B).any() and len(np.unique(scored["host_b"]["steps"])) >= 5


def test_scores_equal_host_scoring_of_the_logs(scored):
    _assert_scores(scored["seg_a"], scored["host_a"])          # after the replayed chunks
    _assert_scores(scored["seg_b"], scored["host_b"])          # after 30 more plain launches
    assert scored["active_a"] == np.count_nonzero(scored["host_a"]["state"] == 0)


def test_groups_equal_numpy_means(scored):
    g, seg = scored["groups"], scored["seg_b"]
    assert g.shape == (4, 4)
    for i in range(4):
        sl = slice(GROUPS1[i], GROUPS1[i + 1])
        want = np.array([np.mean(-seg["max_lat_dev"][sl]), np.mean(-seg["rms_vel_dev"][sl])])
        assert (np.abs(g[i, :2] - want) <= TOL + TOL * np.abs(want)).all(), (i, g[i], want)
        assert g[i, 2] == GROUPS1[i + 1] - GROUPS1[i]
        assert g[i, 3] == np.count_nonzero(seg["crashed"][sl] | seg["timed_out"][sl])
    assert g[:, 3].max() > 0 and (g[:, 3] < g[:, 2]).any()


# ------------------------------------------------------------------------------------------------ 2: early stop
def test_early_stop_does_not_change_results(golden_dir):
    B, S = 6, 150
    params = _params(golden_dir, B)
    starts = np.array([0, 350, 800])[np.arange(B) % 3]
    ref = _loop(B, params, starts, S)
    ref.dev.run(S)
    _, _, idx = _series(ref, ref.dev.logs())
    end = idx[55 + np.arange(B), np.arange(B)]          # every end is reached within about 60 steps
    full = _loop(B, params, starts, 0)
    full.dev.attach_segments(end, np.inf, np.inf)
    full.dev.run(S)
    want = full.dev.segments()
    assert (want["state"] == 1).all() and 50 < want["steps"].max() <= 61          # one chunk of 50 is not enough, two are
    cl = _loop(B, params, starts, 0)
    cl.dev.attach_segments(end, np.inf, np.inf)
    cl.dev.run_segments(S, check_every=50)
    assert cl.dev.steps == 100 and cl.dev.segments_active == 0          # stopped after the second chunk
    got = cl.dev.segments()
    for k in INT_FIELDS + FLOAT_FIELDS + FLAG_FIELDS:
        assert np.array_equal(got[k], want[k]), k
    # one end that is never reached: all 150 steps run, and that instance has timed out
    visited = np.unique(idx[:, 0])
    end2 = end.copy(); end2[0] = (visited.max() + 200) % len(ref.track)
    assert end2[0] not in visited
    cl2 = _loop(B, params, starts, 0)
    cl2.dev.attach_segments(end2, np.inf, np.inf)
    cl2.dev.run_segments(S, check_every=50)
    got2 = cl2.dev.segments()
    assert cl2.dev.steps == S and cl2.dev.segments_active == 1
    assert got2["timed_out"].tolist() == [True] + [False] * (B - 1) and got2["steps"][0] == S and not got2["done"][0]
    for k in INT_FIELDS + FLOAT_FIELDS:
        assert np.array_equal(got2[k][1:], want[k][1:]), k


# ------------------------------------------------------------------------------------------------ 3: evaluate_segments
def test_evaluate_segments_equals_the_host_path(golden_dir):
    """P = 3 candidates x 2 groups x 2 segments: objectives, NaN rows and feasibility as the path through the logs gives them"""
    from tum_control_amd import closed_loop as clm
    P, S, max_steps = 3, 4, 100
    params = _params(golden_dir, 26)[[0, 9, 17]]
    seg_starts = np.array([0, 350, 800, 1000])
    ref = _loop(P * S, np.repeat(params, S, axis=0), np.tile(seg_starts, P), max_steps)
    ref.dev.run(max_steps)
    logs = ref.dev.logs()
    lat, ac, idx = _series(ref, logs)
    ends = idx[[40, 45, 50, 55], np.arange(S)]          # of candidate 0; every candidate passes every waypoint (2 m apart, < 0.8 m per step)
    segment_groups = [[(seg_starts[0], ends[0]), (seg_starts[1], ends[1])], [(seg_starts[2], ends[2]), (seg_starts[3], ends[3])]]
    # lat_dev threshold: the candidate with the largest deviation inside its scored windows crashes, the others do not
    free = _host(ref, logs, np.tile(ends, P), np.inf, np.inf)
    assert free["done"].all()
    scored_lat = np.where(np.arange(max_steps)[:, None] < free["steps"][None, :], lat, -np.inf).max(axis=0).reshape(P, S).max(axis=1)
    o = np.argsort(scored_lat)
    thr_lat = _between(lat, scored_lat[o[-2]], scored_lat[o[-1]])
    assert np.abs(lat - thr_lat).min() > 1e-9
    host = _host(ref, logs, np.tile(ends, P), thr_lat, np.inf)
    want_obj, want_feas = clm.segment_objectives(host, P, [2, 2])
    assert want_feas.sum() == 2 and not want_feas[o[-1]]
    obj, feas, seg = clm.evaluate_segments("monteblanco", params, segment_groups, thr_lat, np.inf, max_steps, check_every=50)
    assert obj.shape == (P, 2, 2) and np.array_equal(feas, want_feas)
    assert np.isnan(obj[~feas]).all() and np.isfinite(obj[feas]).all()
    assert (np.abs(obj[feas] - want_obj[feas]) <= TOL + TOL * np.abs(want_obj[feas])).all()
    _assert_scores(seg, host)


# ------------------------------------------------------------------------------------------------ 4: other controllers
@pytest.mark.parametrize("controller", ["r2", "snmpc"])
def test_other_controllers(controller):
    B, S = 3, 30
    starts = np.array([100, 100, 420])
    ref = _loop(B, None, starts, S, controller=controller)
    ref.dev.run(S)
    logs0 = ref.dev.logs()
    lat, ac, idx = _series(ref, logs0)
    end = np.array([idx[20, 0], -1, idx[12, 2]])
    m = ac.max(axis=0)
    thr_ac = _between(ac, np.sort(ac[:, 1])[-2], m[1])          # instance 1 crashes by a_comb on the step of its maximum
    assert np.abs(ac - thr_ac).min() > 1e-9
    cl = _loop(B, None, starts, S, controller=controller)
    cl.dev.attach_segments(end, np.inf, thr_ac)
    cl.dev.run(S)
    _assert_same_logs(logs0, cl.dev.logs())
    host = _host(ref, logs0, end, np.inf, thr_ac)
    assert (host["state"][1] & 4) and host["steps"][1] == int(np.argmax(ac[:, 1])) + 1
    _assert_scores(cl.dev.segments(), host)


# ------------------------------------------------------------------------------------------------ 5: lifecycle
def test_lifecycle(golden_dir):
    B, S = 3, 60
    params = _params(golden_dir, B)
    starts = np.array([0, 350, 800])
    cl = _loop(B, params, starts, 2 * S)
    # nothing attached: every seg_* field is refused
    for f in ("seg_steps", "seg_state", "seg_max_lat_dev", "seg_rms_vel_dev", "seg_max_a_comb", "seg_qp_failures"):
        with pytest.raises(Exception, match="no segments attached"):
            cl.dev._seg_get(f, B)
    with pytest.raises(Exception, match="no segments attached"):
        cl.dev.segments_active
    with pytest.raises(Exception, match="no segments attached"):
        cl.dev._seg_get("seg_groups", 4 * B)
    with pytest.raises(Exception, match="no segments attached"):
        cl.dev.run_segments(10)
    # offsets that do not start at 0, do not end at batch, or go back
    for bad in ([1, 3], [0, 2], [0, 2, 1, 3], [0, 0, 3]):
        with pytest.raises(Exception, match="group_offsets"):
            cl.dev.attach_segments(np.full(B, -1), np.inf, np.inf, group_offsets=bad)
    with pytest.raises(Exception, match="no segments attached"):
        cl.dev._seg_get("seg_steps", B)
    # attaching after a chunk was captured still scores: the second half of the run against the host
    cl.dev.run(S)
    assert cl.dev.graph_steps == 25
    cl.dev.attach_segments(np.full(B, -1), np.inf, np.inf)
    assert cl.dev.graph_steps == 0          # the chunk is captured again, with the extra launch
    cl.dev.run(S)
    assert cl.dev.graph_steps == 25
    logs = cl.dev.logs()
    _, _, idx = _series(cl, logs)
    host = _host(cl, logs, -1, np.inf, np.inf, first_step=S)
    got = cl.dev.segments()
    assert (got["steps"] == S).all()
    _assert_scores(got, host)
    # set_state zeroes scores and state words: a new run is a new evaluation
    cl.dev.set_state(cl.x_sim, cl.x_mpc, cold_start=True)
    z = cl.dev.segments()
    for k in INT_FIELDS + FLOAT_FIELDS:
        assert (z[k] == 0).all(), k
    assert cl.dev.segments_active == B
    # detach, then run: bit for bit a loop that never had segments
    a = _loop(B, params, starts, 2 * S)
    a.dev.attach_segments(idx[10, np.arange(B)], np.inf, np.inf)
    a.dev.run(S)
    a.dev.detach_segments()
    assert a.dev.graph_steps == 0
    a.dev.run(S)
    b = _loop(B, params, starts, 2 * S)
    b.dev.run(S); b.dev.run(S)
    _assert_same_logs(a.dev.logs(), b.dev.logs())
    with pytest.raises(Exception, match="no segments attached"):
        a.dev.segments()
