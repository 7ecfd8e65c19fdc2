"""The host tables of hxv_observables_accumulate and hxv_apply_density_ops checked by a stand-alone program
(tests/host/density_tables_check.cpp over csrc/hxv_sector.cpp, csrc/hxv_observables_tables.cpp and csrc/hxv_density_ops_tables.cpp; no HIP
call, no device): plain, and under -fsanitize=address,undefined.  The program is run directly as a child, nothing is preloaded.  The
sanitizer run is skipped when a GPU is present."""
import subprocess

import pytest


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.rstrip().endswith("OK") and r.stdout.count("CASE ") == 20
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_density_tables_check(built):
    _run(built.build_density_tables_check())


def test_density_tables_check_under_address_and_undefined_sanitizers(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("host sanitizer builds run on the CPU box")
    _run(built.build_density_tables_check(sanitize="address,undefined"))
