#!/usr/bin/env python3
"""Which paths of the partial-trace kernels do the sectors of the density-matrix GPU tests reach on a 256-CU device?  No GPU needed.

Runs the stand-alone table checker (tests/host/partial_trace_check, built by build_partial_trace_check()) on the sectors that
tests/test_gpu_cluster_dm.py and tests/test_gpu_reduced_dm.py open, and on sector (8,8) of the Ns = 16 lattice, which no test opens for a
density matrix, and prints its REACH lines as a table: items of the two tile kernels, classes whose batch loop takes a second trip, the most
pairs a <4,2> item / a four-wave item stages at once (1: b = 0 only, the waves 1 to 3 idle), dw groups an item spans, staging rounds.
The second half of the table is the same for the synthetic cases of tests/partial_trace_kernels_ref.py (their own ncu), from the tables of
the host-only builder library.                                                                usage: scripts/partial_trace_reach.py"""
import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "tests")]

FIELDS = ["t2_items", "t4_items", "tile_classes", "classes_second_trip", "max_batches", "t4_max_bc", "nrep4_max_bc", "max_groups", "max_rounds"]


def real_sectors():
    from hxv import models

    chain8 = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    chain12 = models.hm_1dchain(eps_bath=[0.3, -0.2])
    chain10 = models.hm_1dchain(Nlat=5, Nbath=1, eps_bath=[0.3], xmu=0.1)
    square16 = models.hm_2dsquare()
    both = ["cluster", "5:1", "5:1:0", "f:1"]
    out = [("Ns 8 (%d,%d)" % s, chain8, s, both) for s in ((4, 4), (4, 3), (3, 5), (5, 4), (8, 1))]
    out += [("Ns 12 (6,6)", chain12, (6, 6), both), ("Ns 12 (5,7)", chain12, (5, 7), both)]
    out += [("Ns 16 (8,2)", square16, (8, 2), ["cluster"]), ("Ns 10 Nimp 5 (5,5)", chain10, (5, 5), ["cluster"])]
    out += [("Ns 16 (8,8), opened by no test", square16, (8, 8), ["cluster"])]
    return out


def main():
    import __graft_entry__ as ge
    from test_host_plan_check import write_model
    import partial_trace_kernels_ref as R

    exe = ge.build_partial_trace_check()
    print("%-34s %-8s " % ("sector", "spec") + " ".join("%s" % f for f in FIELDS))
    with tempfile.TemporaryDirectory() as tmp:
        for label, model, (nup, ndw), specs in real_sectors():
            path = write_model(Path(tmp) / "m.model", model)
            p = subprocess.run([str(exe), str(path), str(nup), str(ndw), "1"] + specs, capture_output=True, text=True)
            if p.returncode:   # Ns 16 (8,8): the checker's replay holds 165 million amplitudes to 1e-13 and misses it by rounding alone
                assert "opened by no test" in label and "replay" in p.stderr, p.stderr[-2000:]
                print("# (%s: the checker's own replay ends with: %s)" % (label, p.stderr.strip().splitlines()[-1]))
            for line in p.stdout.splitlines():
                if line.startswith("REACH "):
                    f = dict(x.split("=", 1) for x in line.split(" ")[1:])
                    print("%-34s %-8s " % (label, f["spec"]) + " ".join("%*s" % (len(k), f[k]) for k in FIELDS))
    # the synthetic cases: the same figures from the tables of the host-only builder
    lib = R.bind(ctypes.CDLL(str(ge.build_partial_trace_build())))
    for case in R.TILE_CASES + R.SPLIT_CASES + R.CHAIN_CASES:
        T = R.Tables(lib, R.make_sector(case))
        r = dict.fromkeys(FIELDS, 0)
        second, tile = set(), set()
        for k in range(T.nitems[0], len(T.items)):
            it, c = T.items[k], T.cls[T.items[k]["cls"]]
            t4 = T.kernel_of(k) == 2
            r["t4_items" if t4 else "t2_items"] += 1
            tile.add(int(it["cls"]))
            ngu, batch = int(c["ngu"]), int(c["batch"])
            gd0, gd1 = int(it["p0"]) // ngu, (int(it["p1"]) - 1) // ngu
            r["max_groups"] = max(r["max_groups"], gd1 - gd0 + 1)
            for gd in range(gd0, gd1 + 1):
                lo = int(it["p0"]) - gd0 * ngu if gd == gd0 else 0
                hi = int(it["p1"]) - gd1 * ngu if gd == gd1 else ngu
                nb, bc = -(-(hi - lo) // batch), min(batch, hi - lo)
                r["max_batches"] = max(r["max_batches"], nb)
                if nb > 1:
                    second.add(int(it["cls"]))
                if t4:
                    r["t4_max_bc"] = max(r["t4_max_bc"], bc)
                if c["nrep"] > 1:
                    r["nrep4_max_bc"] = max(r["nrep4_max_bc"], bc)
                r["max_rounds"] = max(r["max_rounds"], -(-bc * int(c["du"]) // R.PT_THREADS))
        r["tile_classes"], r["classes_second_trip"] = len(tile), len(second)
        print("%-34s %-8s " % ("synthetic " + case.name, "ncu=%d" % case.ncu) + " ".join("%*s" % (len(k), r[k]) for k in FIELDS))


if __name__ == "__main__":
    main()
