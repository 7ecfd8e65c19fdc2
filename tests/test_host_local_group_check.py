"""The host logic of a rank group on the CPU (tests/host/local_group_check.cpp over csrc/hxv_local_group.hpp; DESIGN.md section 4, "what is
verified, and what is not").

Every collective of the thread-rank transport (csrc/hxv_transport.cpp) stands on the barrier of that header, the drivers' error agreement
and their all-reduced dot products on its agree() and sum(), and every hxv_comm_init / hxv_destroy of an RCCL rank goes through its
communicator-cache bookkeeping.  The stand-alone program (its own main, std::threads as ranks, 2, 3, 4 and 8 of them, no HIP, no handle)
has one mode each:
    barrier   2000 generations; a shared counter shows that nobody leaves generation g before all have entered it
    timeout   timeout_s = 0.2 and one rank missing: everybody returns non-zero in bounded time, every later call at once
    abort     a thread that is no rank calls abort() while n-1 ranks wait: all wake with non-zero
    agree     all zero / one rank non-zero (every rank) / two ranks non-zero (every ordered pair: rank order decides) / a broken group
    sum       1e16, 1, -1e16, 3 dealt over the ranks at four shifts, -0.0 from everybody, one rank two elements short, 500 rounds back to
              back: every rank's total has the bits of the left-to-right sum from 0.0 that the program computes itself
    cache     eight threads, 3000 rounds each of bind-or-insert, evict, clear and release over a dozen keys with a counting destroy callback:
              every entry destroyed exactly once, none while bound, inits + reuses = binds; and a single-threaded walk of 4000 steps
              against the same policy written down again
Each mode is run directly as a child, nothing preloaded: the plain build, and once under the host sanitizers (ASan + UBSan, TSan)."""
import os
import re
import subprocess

import pytest

MODES = ["barrier", "timeout", "abort", "agree", "sum", "cache"]
# checks a mode makes at the least (the agree patterns and the walk's steps are counted one by one)
FLOOR = {"barrier": 12, "timeout": 4 * 2 + 1, "abort": 4 * 2 + 1, "agree": 4000, "sum": 9, "cache": 4000}


def run_mode(exe, mode, env=None):
    """-> (exit status, summary dict of the last stdout line, stderr)"""
    p = subprocess.run([str(exe), mode], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=300)
    lines = p.stdout.strip().splitlines()
    m = re.fullmatch(r"LOCAL_GROUP_CHECK mode=(\w+) checks=(\d+) failures=(\d+) (OK|FAILED)", lines[-1]) if lines else None
    summary = dict(mode=m.group(1), checks=int(m.group(2)), failures=int(m.group(3)), verdict=m.group(4)) if m else None
    return p.returncode, summary, p.stderr


def _assert_passed(rc, summary, err, mode):
    assert rc == 0, (mode, rc, err[-3000:])
    assert summary is not None, (mode, "no summary line", err[-3000:])
    assert summary["mode"] == mode and summary["failures"] == 0 and summary["verdict"] == "OK", (mode, summary, err[-3000:])
    assert summary["checks"] >= FLOOR[mode] and "FAIL" not in err, (mode, summary, err[-3000:])


def _no_report(err):
    return not any(s in err for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "WARNING: ThreadSanitizer", "runtime error:", "SUMMARY:"))


def test_checker_includes_the_header_alone(built):
    """The program includes csrc/hxv_local_group.hpp and nothing else of the project, and the header nothing but the standard library: no
    HIP, no RCCL, no handle."""
    root = built.ROOT
    prog = (root / "tests" / "host" / "local_group_check.cpp").read_text()
    assert re.findall(r'#include "([^"]+)"', prog) == ["hxv_local_group.hpp"]
    header = (built.CSRC / "hxv_local_group.hpp").read_text()
    assert not re.findall(r'#include "([^"]+)"', header)
    for text in (prog, header):
        code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
        assert not re.search(r"\bhip[A-Z]\w*|\bnccl[A-Z]\w*|hxv_handle", code)


@pytest.mark.parametrize("mode", MODES)
def test_mode_passes(built, mode):
    """each mode of the plain build as its own process: exit status 0 and the summary line with no failure"""
    rc, summary, err = run_mode(built.build_local_group_check(), mode)
    _assert_passed(rc, summary, err, mode)
    print(mode, summary)


def test_every_mode_under_asan_and_ubsan(built):
    """every mode with the program compiled with -fsanitize=address,undefined -fno-sanitize-recover=undefined: exit 0, no failure, no
    sanitizer report (leaks included: the program owns every entry it makes).  A stand-alone program, run directly; not on a GPU machine."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_local_group_check("address,undefined")
    leaks = 1
    for mode in MODES:
        rc, summary, err = run_mode(exe, mode, {"ASAN_OPTIONS": f"detect_leaks={leaks}"})
        if leaks and "LeakSanitizer has encountered a fatal error" in err:
            print("LeakSanitizer cannot run here: leak checking off\n" + err[-500:])
            leaks = 0
            rc, summary, err = run_mode(exe, mode, {"ASAN_OPTIONS": "detect_leaks=0"})
        assert _no_report(err), (mode, rc, err[-3000:])
        _assert_passed(rc, summary, err, mode)


def test_every_mode_under_tsan(built):
    """every mode under -fsanitize=thread, which is what this build is for: the barrier's generations, the timeout that breaks the group,
    the abort from a foreign thread, the deposits of agree and sum between their two barriers, the cache's bookkeeping from eight
    threads.  Exit 0, no failure, no report."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_local_group_check("thread")
    for mode in MODES:
        rc, summary, err = run_mode(exe, mode)
        assert _no_report(err), (mode, rc, err[-3000:])
        _assert_passed(rc, summary, err, mode)
