"""
What the compiler reports for the kernels of the record-free path of a stage-uniform iterate (cond_uniform_kernel,
expand_uniform_kernel: csrc/pipe_kernels.hpp), from libtumnmpc.so.resources as build() leaves it -- the table
tests/test_host_logic.py::test_shipped_kernels_resource_budget reads, looked up by demangled name.
Columns: VGPRs AGPRs SGPR-spill VGPR-spill scratch LDS waves/SIMD.
"""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def resources():
    import __graft_entry__ as g
    if not (os.path.exists(g.HIPCC) or shutil.which("hipcc")) and not os.path.exists(g.LIB + ".resources"):
        pytest.skip("no hipcc and no resource table of a previous build on this host")
    g.build()
    rows = {}
    for line in open(g.LIB + ".resources"):
        parts = line.split()
        rows[parts[0]] = [int(x) for x in parts[1:]]
    filt = shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    names = list(rows)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {d.strip(): rows[n] for n, d in zip(names, dem)}


def _kernel(rows, sub):
    hit = [v for n, v in rows.items() if sub in n]
    assert len(hit) == 1, (sub, [n for n in rows if sub in n])
    return hit[0]


def test_headline_condensing_without_records_keeps_two_wavefronts_per_simd(resources):
    """cond_uniform_kernel<5> (N <= 40): no SGPR or VGPR spill, no scratch, two wavefronts per SIMD -- what cond_kernel<5, false, true> holds"""
    vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ = _kernel(resources, "cond_uniform_kernel<5>")
    assert (sgpr_spill, vgpr_spill, scratch) == (0, 0, 0) and occ == 2, (vgpr, agpr, sgpr_spill, vgpr_spill, scratch, occ)


@pytest.mark.parametrize("name", ["expand_uniform_kernel<5>", "expand_uniform_kernel<6>", "expand_uniform_kernel<7>",
                                  "cond_uniform_kernel<6>", "cond_uniform_kernel<7>"])
def test_record_free_kernels_have_no_scratch_and_no_spills(resources, name):
    vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ = _kernel(resources, name)
    assert (sgpr_spill, vgpr_spill, scratch) == (0, 0, 0), (name, sgpr_spill, vgpr_spill, scratch)


def test_the_record_form_keeps_its_one_name(resources):
    """the budget test of tests/test_host_logic.py finds the headline's record form by this substring and wants one hit"""
    _kernel(resources, "cond_kernel<5, false, true>")
    _kernel(resources, "expand_kernel<5, false>")
