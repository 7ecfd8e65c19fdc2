"""The budgets and the ISA lint of tests/test_kernel_resources.py applied to the cluster-density-matrix kernels (csrc/hxv_cluster_dm.hip;
no GPU needed: hipcc cross-compiles)."""
from pathlib import Path

import pytest

import isa_lint

SRC = "hxv_cluster_dm.hip"
MAX_VGPR_SPILL = 8
MAX_SCRATCH_BYTES = 40


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(isa_lint.HIPCC).exists():
        pytest.skip("hipcc not available")
    assert (isa_lint.CSRC / SRC).exists(), SRC
    return isa_lint.compile_to_asm(isa_lint.CSRC / SRC, tmp_path_factory.mktemp("isa_cdm") / (SRC + ".s"))


def test_cluster_dm_kernel_budgets(asm):
    md = isa_lint.kernel_metadata(asm)
    assert sum("cdm_accumulate_kernel" in n for n in md) == 2 and any("cdm_reduce_kernel" in n for n in md), list(md)
    bad = [(isa_lint.demangle(n), d) for n, d in md.items()
           if d.get("vgpr_spill_count", 0) > MAX_VGPR_SPILL or d.get("private_segment_fixed_size", 0) > MAX_SCRATCH_BYTES]
    assert not bad, bad


def test_cluster_dm_kernels_have_no_vector_instruction_under_exec_zero(asm):
    found, n = [], 0
    for name, body in isa_lint.kernel_bodies(asm):
        n += 1
        found += [(isa_lint.demangle(name), x) for x in isa_lint.exec0_findings(body)]
    assert n >= 3
    assert not found, found
