#!/usr/bin/env python3
"""
tests/golden/make_wmpc_value_golden.py <reference tree> -- regenerates wmpc_value.npz in this directory.

Runs only where the reference tree exists (the fixture is committed, the tests never need this script). It reads the trained agent
Learning_To_Adapt/SafeRL_WMPC/_models/new_BO_F/best_model/best_model.zip as make_wmpc_policy_golden.py does -- zipfile and
torch.load(weights_only=True) through WeightPolicy.from_sb3_zip; stable_baselines3 itself is not needed -- and writes DATA only:

  V0..V3, c0..c3   the value net (mlp_extractor.value_net.{0,2,4}, value_net) as float32, V row-major (out, in) as torch stores it
  values_f32       torch's own float32 forward pass on float32 of the first 256 rows of numpy.random.RandomState(0).rand(4096, 22)
                   (the `obs` of wmpc_policy.npz), recorded
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)


def main(ref):
    from tum_control_amd.closed_loop import WeightPolicy
    pol = WeightPolicy.from_sb3_zip(os.path.join(ref, "Learning_To_Adapt/SafeRL_WMPC/_models/new_BO_F/best_model/best_model.zip"))
    assert pol.value_weights is not None, "the archive holds no value net"
    assert [w.shape for w in pol.value_weights] == [(128, 22), (256, 128), (128, 256), (1, 128)]
    assert all(w.dtype == np.float32 for w in pol.value_weights + pol.value_biases)
    obs = np.random.RandomState(0).rand(4096, 22)[:256]
    with torch.no_grad():
        h = torch.from_numpy(obs.astype(np.float32))
        for i, (w, b) in enumerate(zip(pol.value_weights, pol.value_biases)):
            h = torch.nn.functional.linear(h, torch.from_numpy(w), torch.from_numpy(b))
            if i + 1 < len(pol.value_weights):
                h = torch.tanh(h)
    out = {f"V{i}": w for i, w in enumerate(pol.value_weights)}
    out.update({f"c{i}": b for i, b in enumerate(pol.value_biases)})
    out["values_f32"] = h.numpy()[:, 0]
    np.savez(os.path.join(OUT, "wmpc_value.npz"), **out)
    print("wmpc_value.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    main(sys.argv[1])
