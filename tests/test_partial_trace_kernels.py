"""The budgets and the ISA lint of tests/test_kernel_resources.py applied to the kernels of the partial-trace engine
(csrc/hxv_partial_trace.hip, under the cluster and the subset density matrices; no GPU needed: hipcc cross-compiles).  The engine is the
only file of the two density matrices with device code: their front ends and the group enumerations are C++ sources."""
from pathlib import Path

import pytest

import isa_lint

SRC = "hxv_partial_trace.hip"
MAX_VGPR_SPILL = 8
MAX_SCRATCH_BYTES = 40
KERNELS = {"pt_pair_kernel": 1, "pt_tile_kernel": 2, "pt_reduce_kernel": 1}   # (the tile kernel with 2 x 2 and with 4 x 4 tiles)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(isa_lint.HIPCC).exists():
        pytest.skip("hipcc not available")
    assert (isa_lint.CSRC / SRC).exists(), SRC
    return isa_lint.compile_to_asm(isa_lint.CSRC / SRC, tmp_path_factory.mktemp("isa_pt") / (SRC + ".s"))


def test_partial_trace_kernel_budgets(asm):
    md = isa_lint.kernel_metadata(asm)
    assert all(sum(k in n for n in md) == c for k, c in KERNELS.items()) and len(md) == sum(KERNELS.values()), list(md)
    bad = [(isa_lint.demangle(n), d) for n, d in md.items()
           if d.get("vgpr_spill_count", 0) > MAX_VGPR_SPILL or d.get("private_segment_fixed_size", 0) > MAX_SCRATCH_BYTES]
    assert not bad, bad


def test_partial_trace_kernels_have_no_vector_instruction_under_exec_zero(asm):
    found, n = [], 0
    for name, body in isa_lint.kernel_bodies(asm):
        n += 1
        found += [(isa_lint.demangle(name), x) for x in isa_lint.exec0_findings(body)]
    assert n >= sum(KERNELS.values())
    assert not found, found
