"""The budgets and the ISA lint of tests/test_cluster_dm_kernels.py applied to the density-operator kernels (csrc/hxv_density_ops.hip;
no GPU needed: hipcc cross-compiles)."""
from pathlib import Path

import pytest

import isa_lint

SRC = "hxv_density_ops.hip"
MAX_VGPR_SPILL = 8
MAX_SCRATCH_BYTES = 40
KERNELS = ("dop_sums_kernel", "dop_apply_kernel", "dop_reduce_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(isa_lint.HIPCC).exists():
        pytest.skip("hipcc not available")
    assert (isa_lint.CSRC / SRC).exists(), SRC
    return isa_lint.compile_to_asm(isa_lint.CSRC / SRC, tmp_path_factory.mktemp("isa_dop") / (SRC + ".s"))


def test_density_ops_kernel_budgets(asm):
    md = isa_lint.kernel_metadata(asm)
    assert all(sum(k in n for n in md) == 1 for k in KERNELS) and len(md) == len(KERNELS), list(md)
    bad = [(n, d) for n, d in md.items()
           if d.get("vgpr_spill_count", 0) > MAX_VGPR_SPILL or d.get("private_segment_fixed_size", 0) > MAX_SCRATCH_BYTES]
    assert not bad, bad


def test_density_ops_kernels_have_no_vector_instruction_under_exec_zero(asm):
    found, n = [], 0
    for name, body in isa_lint.kernel_bodies(asm):
        n += 1
        found += [(name, x) for x in isa_lint.exec0_findings(body)]
    assert n >= len(KERNELS)
    assert not found, found
