"""The option tables behind hxv_set_option and hxv_get_option checked by a stand-alone program (tests/host/options_check.cpp over
csrc/hxv_options.cpp; no HIP call, no device): plain, and under -fsanitize=address,undefined.  The program is run directly as a child,
nothing is preloaded.  The sanitizer run is skipped when a GPU is present.

test_names_agree_with_the_header_and_the_gpu_test ties the four statements of the option names together: the engine's table (the program's
--names), the "Options" block of include/hxv.h, and the OPTIONS table of tests/test_gpu_options.py.  A name added to one of them alone
fails it."""
import re
import subprocess

import pytest

from test_gpu_options import OPTIONS, READBACKS_IN_BLOCK, ROOT, header_option_names


def _run(exe):
    args = [f"{name}={','.join(str(v) for v in values)}" for name, (group, _, values) in OPTIONS.items() if group != 3]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.rstrip().endswith("OK") and r.stdout.count("CASE ") == 4
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_options_check(built):
    _run(built.build_options_check())


def test_options_check_under_address_and_undefined_sanitizers(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("host sanitizer builds run on the CPU box")
    _run(built.build_options_check(sanitize="address,undefined"))


def header_readback_names():
    """The quoted names of the header's "hxv_get_option additionally reports" paragraph, "a|_b|_c" and "a_b|c|d" spelled out the way
    header_option_names spells them (the alternatives replace the first one's last _-separated piece)."""
    text = (ROOT / "include" / "hxv.h").read_text()
    para = text[text.index("hxv_get_option additionally reports"): text.index("int hxv_set_option(")]
    para = para[: para.index("Every option of groups 1 and 2 reads back")]   # (what follows quotes settable names)
    names = set()
    for tok in re.findall(r'"([^"\n]+)"', para):
        first, *rest = tok.split("|")
        names.add(first)
        names.update(first[: first.rindex("_")] + (s if s.startswith("_") else "_" + s) for s in rest)
    return names


def test_names_agree_with_the_header_and_the_gpu_test(built):
    r = subprocess.run([str(built.build_options_check()), "--names"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line.split() for line in r.stdout.splitlines()]
    settable = {f[1]: int(f[2]) for f in lines if f[0] == "set"}
    readonly = [f[1] for f in lines if f[0] == "get"]
    assert len(settable) + len(readonly) == len(lines) and len(set(readonly)) == len(readonly)
    assert settable == {name: group for name, (group, _, _) in OPTIONS.items()}
    assert set(settable) == header_option_names() - READBACKS_IN_BLOCK
    quoted = header_readback_names()
    assert {"tile_bits_up", "nblocks_up", "job_up_active", "pass_b_order_last", "open_us_host", "open_us_plan", "open_us_upload",
            "open_us_total", "pool_live_blocks"} <= quoted           # (the paragraph was found and its a|b|c forms were spelled out)
    # ("tile_bits_up" is quoted there too: settable, its row answers from the plan's block bits; no name is in both tables)
    assert quoted - set(settable) == quoted - {"tile_bits_up"}
    assert quoted - set(settable) <= set(readonly), sorted(quoted - set(settable) - set(readonly))
    assert READBACKS_IN_BLOCK <= set(readonly)
    assert not set(settable) & set(readonly)
