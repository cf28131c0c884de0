"""
Writes tests/golden/ppo_shipped_4096_{pi,vf}.npz: the long-double reference of tests/ppo_reference.py (loss_and_grads_ld) for the case at
the shipped shape -- nets (22, 128, 256, 128, 26) / (22, 128, 256, 128, 1), n = 4096 -- which takes numpy about 20 s of long-double
matrix products, too long for a test. Every long-double array x is stored as hi = float64(x) and lo = float32(x - hi): 2^-77 relative,
against a gate in units of 2^-53. The inputs are NOT stored: ppo_reference.case() regenerates them from their seeds, and
tests/test_ppo_host.py holds torch's float64 autograd and the host statement on those inputs against this file.
    python tests/golden/make_ppo_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ppo_reference as ref  # noqa: E402


def split(x):
    x = np.asarray(x, dtype=ref.LD)
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(ref.LD)).astype(np.float32)


if __name__ == "__main__":
    name, n = ref.GOLDEN_CASE
    ld = ref.loss_and_grads_ld(*ref.nets(name), **ref.case(name, n), **ref.SETTINGS)
    gW, gb, gVW, gVb = ld["grads"]
    scal = {k: ld[k] for k in ref.SCALARS + ("clip_fraction", "kink", "unclipped")}
    for tag, Ws, bs, extra in (("pi", gW, gb, dict(log_probs=ld["log_probs"], **scal)), ("vf", gVW, gVb, dict(values=ld["values"]))):
        out = {}
        for k, x in [(f"W{l}", w) for l, w in enumerate(Ws)] + [(f"b{l}", b) for l, b in enumerate(bs)] + list(extra.items()):
            out[k + "_hi"], out[k + "_lo"] = split(x)
        np.savez(os.path.join(HERE, f"ppo_{name}_{n}_{tag}.npz"), **out)
