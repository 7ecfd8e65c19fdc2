"""The budgets and the ISA lint of tests/test_kernel_resources.py applied to the impurity-observables kernels (csrc/hxv_observables.hip;
no GPU needed: hipcc cross-compiles)."""
from pathlib import Path

import pytest

import isa_lint

SRC = "hxv_observables.hip"
MAX_VGPR_SPILL = 8
MAX_SCRATCH_BYTES = 40


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(isa_lint.HIPCC).exists():
        pytest.skip("hipcc not available")
    return isa_lint.compile_to_asm(isa_lint.CSRC / SRC, tmp_path_factory.mktemp("isa_obs") / (SRC + ".s"))


def test_observables_kernel_budgets(asm):
    md = isa_lint.kernel_metadata(asm)
    assert all(any(k in n for n in md) for k in ("obs_rows_kernel", "obs_rdw_kernel", "obs_reduce_kernel")), list(md)
    bad = [(isa_lint.demangle(n), d) for n, d in md.items()
           if d.get("vgpr_spill_count", 0) > MAX_VGPR_SPILL or d.get("private_segment_fixed_size", 0) > MAX_SCRATCH_BYTES]
    assert not bad, bad


def test_observables_kernels_have_no_vector_instruction_under_exec_zero(asm):
    found, n = [], 0
    for name, body in isa_lint.kernel_bodies(asm):
        n += 1
        found += [(isa_lint.demangle(name), x) for x in isa_lint.exec0_findings(body)]
    assert n >= 4
    assert not found, found
