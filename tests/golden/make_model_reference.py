#!/usr/bin/env python3
"""
tests/golden/make_model_reference.py -- regenerates model_reference.npz in this directory (about two minutes).

Needs nothing but this repository and mpmath: tests/model_reference.py holds the exact model and the seeded generator of the
inputs. The file carries, per model point, the inputs and their labels and the binary64 roundings of

  f (8), J (3, 5)                          right-hand side and d(vl', vt', r') / d(vl, vt, r, delta, a)
  Phi<n> (8), A<n> (8, 8), B<n> (8, 2)     one shooting interval of 0.08 s with n = 3 and n = 1 RK4 steps
  Phi<n>_u0, A<n>_u0, B<n>_u0              the same with u = 0 (what a cold-started batch linearises at)
  h, gh (8)                                the gg circle and its gradient

tests/test_model_reference.py recomputes one point per label and requires equality with the file.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import model_reference as mr  # noqa: E402


def main():
    X, U, L = mr.model_points()
    out = mr.reference_arrays()
    np.savez_compressed(os.path.join(HERE, "model_reference.npz"), X=X, U=U, labels=np.array(L), dt=np.float64(mr.DT), **out)
    print(f"{len(L)} points, {len(set(L))} labels, {os.path.getsize(os.path.join(HERE, 'model_reference.npz'))} bytes")


if __name__ == "__main__":
    main()
