"""plan_pipeline (csrc/pipe_plan.hpp), the decision which kernel of every pipeline stage a solve launches, on the CPU: a stand-alone
program enumerates its whole input space and checks that no plan reads stage records that were not written, the rules of the tile
counts, the coupled SNMPC OCP, a full W, the split iteration and the graph capture, and the kernels of the named cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tum-control_amd", "csrc")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_pipe_plan_invariants_over_the_whole_input_space(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pipe_plan_check")
    # the header is built by a plain host compiler: nothing of HIP on the include path
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "pipe_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the check does not build:\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failed" in r.stdout
