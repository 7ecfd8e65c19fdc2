"""The partial-trace tables on the CPU (tests/host/partial_trace_check.cpp).

Every table the builder of csrc/hxv_partial_trace_host.hpp hands to the kernels of the cluster and the subset density matrices is read
through one bounds-checked accessor: the pairs partition the sector over the ranks of a split, the work list and the reduction's tables
cover it without overlap, the classes hold what the kernels assume, the sign bits equal their definitions, and the matrix replayed from
the tables equals the partial trace taken from the basis maps.  This file drives that program, plain and under the host sanitizers (ASan +
UBSan), always as a stand-alone program."""
import os
import subprocess

import pytest

from test_host_plan_check import write_model

# the full mask last; each in both sign conventions, {0,2} also with every class sent to the tile kernel (the hook HXV_RDM_PAIR_KERNEL=0)
MASKS = (0x1, 0x5, 0xd, 0xf)
SPECS = ["cluster"] + [f"{mask:x}:{fs}" for mask in MASKS for fs in (0, 1)] + ["5:0:0", "5:1:0"]
ROW_ORDER_OFF = {"HXV_ROW_ORDER": "0"}
ROW_ORDER_FORCED = {"HXV_ROW_ORDER_MIN_DIMUP": "16", "HXV_ROW_ORDER_BITS": "8"}


def _cases():
    """name -> (model, sector, rank counts, specs, environment)"""
    from hxv import models

    chain8 = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)      # the Ns = 8 chain of the GPU tests
    cases = {}
    for sector in ((4, 3), (0, 8), (8, 1), (4, 4)):
        ranks = "1" if sector == (0, 8) else "1,2,3"     # DimDw = 1: build_sector_from_model refuses to split it ("nranks > DimDw")
        cases["chain8_%d_%d" % sector] = (chain8, sector, ranks, SPECS, {})
        cases["chain8_%d_%d_row_order_off" % sector] = (chain8, sector, ranks, SPECS, ROW_ORDER_OFF)
    cases["chain12_6_6_row_order_forced"] = (models.hm_1dchain(eps_bath=[0.3, -0.2]), (6, 6), "1,3", SPECS, ROW_ORDER_FORCED)
    # Nimp 5: the one case with 4 x 4 tiles, two per thread
    cases["chain10_5_5_cluster"] = (models.hm_1dchain(Nlat=5, Nbath=1, eps_bath=[0.3], xmu=0.1), (5, 5), "1,2,3", ["cluster"], {})
    return cases


CASE_NAMES = ["chain8_%d_%d%s" % (s + (o,)) for s in ((4, 3), (0, 8), (8, 1), (4, 4)) for o in ("", "_row_order_off")] + [
    "chain12_6_6_row_order_forced", "chain10_5_5_cluster"]


def _run(exe, tmp_path, name, env=None):
    model, sector, ranks, specs, case_env = _cases()[name]
    path = write_model(tmp_path / (name + ".model"), model)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HXV_ROW_ORDER")}
    p = subprocess.run([str(exe), str(path), str(sector[0]), str(sector[1]), ranks] + specs, capture_output=True, text=True,
                       env=dict(clean, **case_env, **(env or {})))
    lines = [dict(f.split("=", 1) for f in line.split(" ")[1:]) for line in p.stdout.splitlines() if line.startswith("CASE ")]
    return p.returncode, lines, p.stderr, len(specs) * len(ranks.split(","))


def _assert_passed(name, rc, lines, err, want, label=""):
    assert rc == 0 and "FAIL" not in err and "OUT OF RANGE" not in err, (name, rc, err[-2000:])
    assert len(lines) == want, (name, len(lines), want)
    assert all(int(l["pairs"]) > 0 and int(l["words_read"]) > 0 for l in lines), name
    if name.endswith("row_order_off"):
        assert all(l["row_order"] == "0" for l in lines), name
    if name.endswith("row_order_forced"):
        assert all(l["row_order"] == "1" for l in lines), name
    print(name + label + ":", len(lines), "cases,", sum(int(l["pairs"]) for l in lines), "pairs,", sum(int(l["words_read"]) for l in lines), "table words read")


def test_checker_is_built_from_host_sources_only(built):
    """The checker's source list names C++ files only, the group enumerations among them, and neither they nor the builder's header hold device
    code or include the HIP runtime's header."""
    names = [s.name for s in built.PARTIAL_TRACE_CHECK_SOURCES]
    assert names and all(n.endswith(".cpp") for n in names) and "hxv_partial_trace_groups.cpp" in names, names
    header = built.CSRC / "hxv_partial_trace_host.hpp"
    assert "hip/hip_runtime" not in header.read_text()
    for f in (header, built.CSRC / "hxv_partial_trace_groups.cpp"):
        text = f.read_text()
        assert "__global__" not in text and "__device__" not in text, f.name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_partial_trace_tables(built, tmp_path, name):
    exe = built.build_partial_trace_check()
    _assert_passed(name, *_run(exe, tmp_path, name))


def test_partial_trace_tables_under_asan_and_ubsan(built, tmp_path):
    """Every case once with the sector builder, the enumerations, the table builder and the checker compiled with
    -fsanitize=address,undefined -fno-sanitize-recover=undefined: exit 0 and no sanitizer report on stderr."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_partial_trace_check("address,undefined")
    leaks = 1
    for name in CASE_NAMES:
        env = {"ASAN_OPTIONS": f"detect_leaks={leaks}", "UBSAN_OPTIONS": "print_stacktrace=1"}
        rc, lines, err, want = _run(exe, tmp_path, name, env)
        if leaks and "LeakSanitizer has encountered a fatal error" in err:   # (a sandbox that forbids its stop-the-world tracer: said, not hidden)
            print("LeakSanitizer cannot run here: leak checking off\n" + err[-500:])
            leaks = 0
            rc, lines, err, want = _run(exe, tmp_path, name, dict(env, ASAN_OPTIONS="detect_leaks=0"))
        assert not any(s in err for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY:")), (name, err[-3000:])
        _assert_passed(name, rc, lines, err, want, " [asan+ubsan]")
