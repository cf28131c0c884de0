#!/usr/bin/env python3
"""
tests/golden/make_wmpc_policy_golden.py <reference tree> -- regenerates wmpc_policy.npz in this directory.

Runs only where the reference tree exists (the fixture is committed, the tests never need this script). It reads the trained agent
Learning_To_Adapt/SafeRL_WMPC/_models/new_BO_F/best_model/best_model.zip -- a stable_baselines3 archive whose policy.pth is a plain
state dict, read here with zipfile and torch.load(weights_only=True); stable_baselines3 itself is not needed -- and writes DATA only:

  W0..W3, b0..b3   the policy net (mlp_extractor.policy_net.{0,2,4}, action_net) as float32, W row-major (out, in) as torch stores it
  obs              the first 256 rows of numpy.random.RandomState(0).rand(4096, 22), float64
  logits_f32       torch's own float32 forward pass on float32(obs): Linear / Tanh / Linear / Tanh / Linear / Tanh / Linear, recorded
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
    assert [w.shape for w in pol.weights] == [(128, 22), (256, 128), (128, 256), (26, 128)]
    assert all(w.dtype == np.float32 for w in pol.weights + pol.biases)
    obs = np.random.RandomState(0).rand(4096, 22)[:256]
    with torch.no_grad():
        h = torch.from_numpy(obs.astype(np.float32))
        for i, (w, b) in enumerate(zip(pol.weights, pol.biases)):
            h = torch.nn.functional.linear(h, torch.from_numpy(w), torch.from_numpy(b))
            if i + 1 < len(pol.weights):
                h = torch.tanh(h)
    out = {f"W{i}": w for i, w in enumerate(pol.weights)}
    out.update({f"b{i}": b for i, b in enumerate(pol.biases)})
    out["obs"], out["logits_f32"] = obs, h.numpy()
    np.savez(os.path.join(OUT, "wmpc_policy.npz"), **out)
    print("wmpc_policy.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    main(sys.argv[1])
