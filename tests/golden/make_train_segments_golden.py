#!/usr/bin/env python3
"""
tests/golden/make_train_segments_golden.py <reference tree> -- regenerates train_segments.npz in this directory.

Runs only where the reference tree exists (its root as the one argument, or in the environment variable TUM_REFERENCE; the fixture is
committed, the tests never need this script). It imports the reference's get_train_segments
(Learning_To_Adapt/SafeRL_WMPC/BO_WMPC/track_segmentation.py) -- and through it helpers.py's hysteresis -- with stubs for the
third-party packages helpers.py imports that are absent, as make_rl_env_golden.py does; none of the reference's own functions is
stubbed. It calls get_train_segments() with its defaults from the root of the reference tree (the function opens Trajectories/...
relative to the working directory) and writes DATA only, one entry per segment in the order group 0 then group 1, each group in the
reference's order:

  group       (S,) index of the segment group the reference returned the segment in (0 curves, 1 straights)
  start, end  (S,) waypoint indices as the reference computes them (a segment that wraps past the end of its track has end < start)
  type        (S,) the segment's own type field
  trajectory  (S,) the track name
  n_rows      (S,) waypoints of that track's race line (what makes a wrapped segment recognisable)
"""
import json
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


class _Stub(types.ModuleType):
    """an absent third-party module: any name imported from it is a placeholder nothing here calls"""
    __path__ = []

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return type(item, (), {})


def _import_with_stubs(module, names):
    """import `names` from a reference module; every third-party module that is absent here becomes a stub, one at a time"""
    for _ in range(64):
        try:
            m = __import__(module, fromlist=list(names))
            return [getattr(m, n) for n in names]
        except ModuleNotFoundError as e:
            if not e.name or e.name.split(".")[0] in ("Utils", "Learning_To_Adapt", "Model_Predictive_Controller", "Vehicle_Simulator"):
                raise
            sys.modules[e.name] = _Stub(e.name)
    raise ImportError(module)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TUM_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit(__doc__)
    sys.path.insert(0, ref)
    get_train_segments, = _import_with_stubs("Learning_To_Adapt.SafeRL_WMPC.BO_WMPC.track_segmentation", ["get_train_segments"])
    os.chdir(ref)
    groups = get_train_segments()
    rows = {}
    out = dict(group=[], start=[], end=[], type=[], trajectory=[], n_rows=[])
    for g, segs in enumerate(groups):
        for s in segs:
            name = str(s["trajectory"])
            if name not in rows:
                with open(os.path.join("Trajectories", f"reftraj_{name}_edgar.json")) as f:
                    rows[name] = len(json.load(f)["ref_v"])
            out["group"].append(g); out["start"].append(int(s["start"])); out["end"].append(int(s["end"]))
            out["type"].append(int(s["type"])); out["trajectory"].append(name); out["n_rows"].append(rows[name])
    arrays = {k: np.array(v) if k == "trajectory" else np.array(v, dtype=np.int64) for k, v in out.items()}
    np.savez(os.path.join(OUT, "train_segments.npz"), **arrays)
    print("train_segments.npz: groups of", [len(g) for g in groups], "segments; wrapped:",
          [(t, a, b) for t, a, b in zip(out["trajectory"], out["start"], out["end"]) if b < a])


if __name__ == "__main__":
    main()
