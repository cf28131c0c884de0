"""
The host side of loops on several tracks (no GPU): closed_loop.train_segments against what the reference's get_train_segments returns
(tests/golden/train_segments.npz, written by tests/golden/make_train_segments_golden.py), the host planner over a track set against
the planner on each track, start states with per-instance tracks, the refusals a track set is checked with before it reaches the
device, and the restart draws of a WeightScheduleEnv on two tracks.
The shipped race lines have 1190 (monteblanco), 921 (lvms) and 1002 (modena) waypoints: an index taken against the wrong length shows.
"""
import os

import numpy as np
import pytest

from tum_control_amd import closed_loop as clm
from tum_control_amd.planner import TRACKS, load_track, planner_emulator, planner_emulator_tracks
from tum_control_amd.solver import track_set

ROWS = {"monteblanco": 1190, "lvms": 921, "modena": 1002}


@pytest.fixture(scope="module")
def tables():
    t = {n: load_track(n) for n in TRACKS}
    assert {n: len(v) for n, v in t.items()} == ROWS
    return t


# ------------------------------------------------------------------------------------------------------------------ segmentation
def test_train_segments_equal_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "train_segments.npz"))
    groups = clm.train_segments()
    assert len(groups) == 2 and [len(x) for x in groups] == [10, 10]
    flat = [s for grp in groups for s in grp]
    assert all(set(s) == {"start", "end", "type", "trajectory"} for s in flat)
    assert [g_ for g_, grp in enumerate(groups) for _ in grp] == g["group"].tolist()
    for k in ("start", "end", "type"):
        assert [int(s[k]) for s in flat] == g[k].tolist(), k
    assert [s["trajectory"] for s in flat] == g["trajectory"].tolist()
    # what the fixture must show: five Modena then five Monteblanco segments per group, these pairs, two of them wrapped
    pairs = lambda grp, name: [(s["start"], s["end"]) for s in grp if s["trajectory"] == name]
    assert [s["trajectory"] for s in groups[0]] == [s["trajectory"] for s in groups[1]] == ["modena"] * 5 + ["monteblanco"] * 5
    assert pairs(groups[0], "modena") == [(45, 236), (230, 453), (488, 591), (581, 748), (754, 896)]
    assert pairs(groups[0], "monteblanco") == [(189, 303), (321, 430), (642, 697), (717, 817), (862, 951)]
    assert pairs(groups[1], "modena") == [(216, 250), (433, 508), (571, 601), (728, 774), (876, 65)]
    assert pairs(groups[1], "monteblanco") == [(283, 341), (410, 662), (677, 737), (797, 882), (931, 209)]
    assert all(s["type"] == g_ for g_, grp in enumerate(groups) for s in grp)
    wrapped = [(s["trajectory"], s["start"], s["end"]) for s in flat if s["end"] < s["start"]]
    assert wrapped == [("modena", 876, 65), ("monteblanco", 931, 209)]
    assert all(0 <= s["start"] < ROWS[s["trajectory"]] and 0 <= s["end"] < ROWS[s["trajectory"]] for s in flat)
    assert g["n_rows"].tolist() == [ROWS[n] for n in g["trajectory"].tolist()]


def test_train_segments_arguments():
    one = clm.train_segments(tracks=("monteblanco",))
    both = clm.train_segments()
    assert one[0] == both[0][5:] and one[1] == both[1][5:]
    # a wider overlap moves every end outwards; thresholds that never switch give no segment
    wide = clm.train_segments(overlap=15, tracks=("modena",))
    assert [s["start"] + 5 for s in wide[0]] == [s["start"] for s in both[0][:5]]
    assert clm.train_segments(curv_threshold_lo=-1.0, curv_threshold_hi=1e9) == [[], []]


# ----------------------------------------------------------------------------------------------------------------------- planner
def seam_pose(g, name, track):
    """a pose whose 39-point window crosses the 2 pi seam of the yaw channel: the first one tests/golden/planner.npz holds for the track
    (it holds some for lvms alone), else a pose 0.3 m off the waypoint five in front of the track's first seam"""
    seam = np.nonzero((np.abs(np.diff(g[f"{name}_n39"][:, :, 2], axis=1)) > 3.0).any(axis=1))[0]
    if len(seam):
        return g[f"{name}_pose"][seam[0]]
    row = np.nonzero(np.abs(np.diff(track[:, 2])) > np.deg2rad(250))[0][0]
    return track[row - 5, :2] + 0.3


def test_host_planner_over_a_set_is_the_planner_per_track(tables, golden_dir):
    g = np.load(os.path.join(golden_dir, "planner.npz"))
    names = list(TRACKS)
    table, rows, _ = track_set([tables[n] for n in names], None, 3)
    assert rows.tolist() == [0, 1190, 1190 + 921, 1190 + 921 + 1002] and len(table) == rows[-1]
    poses, of = [], []
    for t, n in enumerate(names):
        tr = tables[n]
        for p in (tr[-1, :2], tr[-2, :2], tr[-3, :2], seam_pose(g, n, tr)):
            poses.append(p); of.append(t)
    poses.append(tables["monteblanco"][1100, :2]); of.append(0)
    order = np.random.RandomState(0).permutation(len(of))          # interleaved: track_of is neither sorted nor contiguous
    poses, of = np.array(poses)[order], np.array(of)[order]
    idx, ref = planner_emulator_tracks(table, rows, of, poses, 39, 3.04)
    wraps = seams = 0
    for p in range(len(of)):
        tr = tables[names[of[p]]]
        i0, r = planner_emulator(tr, poses[p], 39, 3.04)
        assert idx[p] == i0 and np.array_equal(ref[p], r), p
        assert 0 <= idx[p] < len(tr)
        wraps += int(i0 >= len(tr) - 3)
        seams += int((np.abs(np.diff(r[:, 2])) > 3.0).any())
        if i0 >= len(tr) - 2:          # the walk went on at waypoint 0 of the pose's OWN track
            assert np.hypot(*(r[-1, :2] - tr[0, :2])) < np.hypot(*(r[-1, :2] - tr[len(tr) // 2, :2]))
    # (every shipped line closes on itself: its last waypoint IS its first, so a pose there has index 0 and the two before it wrap)
    assert wraps == 6 and (idx == 0).sum() == 3 and seams >= 3 and (idx >= 1002).any()


# ------------------------------------------------------------------------------------------------------------------ start states
def test_start_states_with_per_instance_tracks(tables):
    names = ["monteblanco", "modena"]
    tabs = [tables[n] for n in names]
    of = np.array([0, 1, 1, 0, 1])
    idx = np.array([1100, 1001, 5, 5, 0])
    x = clm.start_states(tabs, idx, 5, of)
    for b in range(5):
        want = clm.start_states(tabs[of[b]], int(idx[b]), 1)[0]
        assert np.array_equal(x[b], want), b
    assert not np.array_equal(x[2], x[3])          # the same waypoint number on two tracks
    # one index for all; the single-track form is what it was
    assert np.array_equal(clm.start_states(tabs, 7, 5, of)[1], clm.start_states(tabs[1], 7, 1)[0])
    assert np.array_equal(clm.start_states(tabs[0], idx.clip(0, 1001), 5), clm.start_states(tabs, idx.clip(0, 1001), 5, np.zeros(5, dtype=int)))
    # 1100 is a waypoint of Monteblanco and of no other track
    with pytest.raises(IndexError, match="own track"):
        clm.start_states(tabs, np.array([1100, 1100, 0, 0, 0]), 5, of)
    with pytest.raises(ValueError):
        clm.start_states(tabs, idx, 5, of[:4])


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_track_set_refusals(tables):
    tabs = [tables["monteblanco"], tables["modena"]]
    table, rows, of = track_set(tabs, [1, 0, 0, 1], 4)
    assert rows.dtype == np.int32 and of.dtype == np.int32 and rows.tolist() == [0, 1190, 2192] and of.tolist() == [1, 0, 0, 1]
    assert np.array_equal(table[1190:], tabs[1])
    assert track_set(tabs, None, 5)[2].tolist() == [0, 1, 0, 1, 0]                     # i % T
    t2, r2, _ = track_set(table, None, 4, track_rows=np.array([0, 1190, 2192]))       # the concatenated form
    assert np.array_equal(t2, table) and r2.tolist() == rows.tolist()
    for bad in ([0, 2, 0, 0], [0, -1, 0, 0]):
        with pytest.raises(ValueError, match="outside 0..1"):
            track_set(tabs, bad, 4)
    with pytest.raises(ValueError, match="per instance"):
        track_set(tabs, [0, 1, 0], 4)
    with pytest.raises(ValueError, match="per instance"):
        track_set(tabs, [0.0, 1.0, 0.0, 1.0], 4)
    for bad in ([0, 1190, 1190, 2192], [0, 1500, 1190, 2192], [0, 1190, 1191, 2192]):          # empty, descending, one row
        with pytest.raises(ValueError, match="ascend"):
            track_set(table, None, 4, track_rows=np.array(bad))
    for bad in ([1, 1190, 2192], [0, 1190, 2000], [0]):
        with pytest.raises(ValueError, match="offsets"):
            track_set(table, None, 4, track_rows=np.array(bad))
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        track_set([tabs[0], tabs[1][:, :3]], None, 4)


def test_track_names_refusals():
    names, tabs, of = clm.resolve_tracks(("monteblanco", "modena"), 5)
    assert names == ["monteblanco", "modena"] and [len(t) for t in tabs] == [1190, 1002] and of.tolist() == [0, 1, 0, 1, 0]
    assert clm.resolve_tracks(["modena", "lvms", "monteblanco"], 4, [2, 2, 0, 1])[2].tolist() == [2, 2, 0, 1]
    assert clm.resolve_tracks("lvms", 3)[2].tolist() == [0, 0, 0]
    with pytest.raises(KeyError, match="unknown track 'monza'"):
        clm.resolve_tracks(("monteblanco", "monza"), 4)
    with pytest.raises(ValueError, match="outside 0..1"):
        clm.resolve_tracks(("monteblanco", "modena"), 3, [0, 1, 2])
    with pytest.raises(ValueError, match="per instance"):
        clm.resolve_tracks(("monteblanco", "modena"), 3, [0, 1])
    with pytest.raises(ValueError, match="sequence of track names"):
        clm.resolve_tracks("monteblanco", 3, [0, 0, 0])
    with pytest.raises(ValueError):
        clm.resolve_tracks((), 3)


# ---------------------------------------------------------------------------------------------------------------- restart draws
def test_restart_draws_on_two_tracks():
    one = (0, 200, 640, 900)
    tracks = np.arange(16) % 2
    # equal lists: the stream of today's single list, call by call (a reset of all, then resets of some, then a start table)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    lists = clm.restart_lists((one, one), 2)
    for who in (np.arange(16), np.array([3, 4, 9]), np.tile(np.arange(16), 7)):
        want = np.asarray(one)[b.randint(0, len(one), size=len(who))]
        assert np.array_equal(clm.draw_restarts(a, lists, tracks[who]), want)
    assert np.array_equal(a.randint(0, 2 ** 31, size=4), b.randint(0, 2 ** 31, size=4))          # both generators stand at the same place
    # one list for every track is the same thing
    same = clm.restart_lists(one, 2)
    assert len(same) == 2 and all(np.array_equal(x, one) for x in same)
    # lists of their own: each instance draws into the list of its own track, one randint per instance in instance order
    own = clm.restart_lists(((0, 200, 1100), (7, 950)), 2)
    rng, ref = np.random.RandomState(11), np.random.RandomState(11)
    who = np.array([0, 1, 2, 5, 8, 9, 15])
    got = clm.draw_restarts(rng, own, tracks[who])
    want = [own[t][ref.randint(0, len(own[t]))] for t in tracks[who]]
    assert got.tolist() == want
    big = clm.draw_restarts(rng, own, tracks[np.tile(np.arange(16), 40)])
    assert set(big[0::2].tolist()) == {0, 200, 1100} and set(big[1::2].tolist()) == {7, 950}
    # equal lengths, different entries: one call of that size, every instance still indexes its own list
    mixed = clm.restart_lists(((0, 1100), (7, 950)), 2)
    rng, ref = np.random.RandomState(3), np.random.RandomState(3)
    k = ref.randint(0, 2, size=16)
    assert clm.draw_restarts(rng, mixed, tracks).tolist() == [mixed[t][i] for t, i in zip(tracks, k)]
    with pytest.raises(ValueError, match="per track"):
        clm.restart_lists(((0, 1), (2, 3), (4, 5)), 2)
    with pytest.raises(ValueError, match="at least one"):
        clm.restart_lists(((0, 1), ()), 2)


def test_the_docstring_no_longer_asks_for_one_object_per_track():
    assert "One object per track" not in clm.WeightScheduleEnv.__doc__ and "i % T" in clm.WeightScheduleEnv.__doc__
