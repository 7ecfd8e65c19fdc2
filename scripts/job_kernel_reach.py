#!/usr/bin/env python3
"""Which paths of the pass-A job kernel hxv_up_job do the suite's sectors reach, and which do the synthetic cases add?  No GPU needed.

Runs the stand-alone plan checker (tests/host/plan_check, built by build_plan_check()) with --job-reach on sectors and option sets under
which GPU tests run pass A as jobs -- the option tests' S1 / S2 with forced block bits under every job_stages / job_groups value, the
layout contract's job family, the row-ordered Ns = 14 sectors, the Ns = 12 and Ns = 14 Lanczos sectors and the C3 shape (plain with
job_up = 1 and fused) -- and prints, from the plan's numbers and the restated geometry (tests/job_kernel_ref.py: reach_of), the reach
columns of tests/test_job_kernel_ref_cpu.py: block sizes n and their 1 KiB pieces nch, ring depth nst (* = clamped by the LDS budget), tiles
per job against nst, chunks, scratch groups per job, the largest wait distance (saturates above 63) and the KIN instantiation.  The second
half is the same for the synthetic cases and for the full-block sector of tests/test_gpu_job_kernel.py.   usage: scripts/job_kernel_reach.py"""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "tests")]


def suite_sectors():
    """(label, model, sector, option sets, lz values): the plain product runs as jobs under job_up = 1 only, the fused one by default"""
    from hxv import models

    s1 = models.hm_1dchain(Nlat=2, Nbath=3)
    s2 = models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1)
    chain12 = models.hm_1dchain(eps_bath=[0.3, -0.2])
    chain14 = models.hm_1dchain(Nlat=2, Nbath=6, eps_bath=list(np.linspace(-0.6, 0.7, 6)), xmu=0.05)
    c3 = models.hm_2dsquare(Nbath=3)
    star14 = models.hm_1dchain(Nlat=1, Nbath=13, eps_bath=[(k - 6) / 10 for k in range(13)])
    stages = [{"job_stages": s} for s in (2, 3, 4, 8)]
    groups = [{"job_groups": g} for g in (1, 3)]
    out = [("options S1 70x70, 3 bits", s1, (4, 4), [dict(o, tile_bits_up=3, tile_bits_dw=3, job_up=1) for o in [{}] + stages + groups], (0, 1)),
           ("options S2 70x56, 6 bits", s2, (4, 3), [dict(o, tile_bits_up=6, tile_bits_dw=3, job_up=1) for o in [{}] + stages + groups], (0, 1)),
           ("layout Ns 12 (4,3), 8 KB tiles", None, (4, 3), [{"lds_budget_kb_up": 8, "lds_budget_kb_dw": 8, "job_up": 1}], (0,)),
           ("Ns 12 (6,6) Lanczos", chain12, (6, 6), [{}], (1,)),
           ("Ns 14 (7,1) row order", chain14, (7, 1), [{"job_up": 1}], (0, 1)),
           ("Ns 14 (6,1) row order", chain14, (6, 1), [{"job_up": 1}], (0, 1)),
           ("C3 Ns 16 (8,8)", c3, (8, 8), [{"job_up": 1}, {"job_up": 1, "wt_cols": 2}], (0, 1)),
           ("NEW star Ns 14 (7,2), 12 bits", star14, (7, 2), [dict(o, tile_bits_up=12, job_up=1) for o in
                                                             [{}, {"job_stages": 2, "wt_cols": 2}, {"job_stages": 8, "wt_cols": 2}]], (0, 1))]
    return out


COLS = ["n", "nch", "nst", "ntile", "<ring-1", ">2ring", "chunks", "groups/job", "mid", "odd", "dist", "sat", "KIN", "nouter", "kin"]


def row(label, r):
    if not r["fits"]:
        return "%-46s does not fit the LDS: not run as jobs at this width" % label

    def rng(x):
        return "%d" % x[0] if len(x) == 1 else "%d..%d" % (x[0], x[-1])

    return "%-46s n %-9s nch %-6s nst %d%s ntile %-6s <ring-1 %d >2ring %d chunks %d groups/job %-5s mid %d odd %d dist %3d sat %d KIN %d nouter %-5s kin %s" % (
        label, rng(r["n"]), rng(r["nch"]), r["nst"], "*" if r["clamped"] else " ", rng(r["ntile"]), r["ntile_lt_ring"], r["ntile_gt_2ring"], r["chunks"],
        rng(r["groups_per_job"]), r["first_mid_group"], r["first_odd_group"], r["dist_max"], r["saturates"], r["KIN"], rng(r["nouter"]), rng(r["kin"]))


def main():
    import __graft_entry__ as ge
    import job_kernel_ref as R
    from test_gpu_layout_contract import _chain
    from test_host_plan_check import write_model

    exe = ge.build_plan_check()
    kin24 = False
    with tempfile.TemporaryDirectory() as tmp:
        for label, model, (nup, ndw), sets, lzs in suite_sectors():
            model = model or _chain(12)
            path = write_model(Path(tmp) / "m.model", model)
            cmd = [str(exe), str(path), str(nup), str(ndw), "0", "1", "0", "--job-reach"]
            for k, o in enumerate(sets):
                cmd += (["/"] if k else []) + ["%s=%d" % kv for kv in o.items()]
            p = subprocess.run(cmd, capture_output=True, text=True)
            assert p.returncode in (0, 2), p.stderr[-2000:]
            for line in p.stdout.splitlines():
                if not line.startswith("JOBREACH "):
                    continue
                f = dict(x.split("=", 1) for x in line.split(" ")[1:])
                o = sets[int(f["set"])]
                opts = ",".join("%s=%d" % kv for kv in o.items() if kv[0] in ("job_stages", "job_groups", "wt_cols"))
                if f["usable"] != "1":
                    print("%-46s the plan does not run as jobs (job_up_usable)" % (label + " " + opts))
                    continue
                blocks = [b.split(":") for b in f["blocks"].split(";")]
                sizes, nouter = [int(b[0]) for b in blocks], [int(b[1]) for b in blocks]
                gkin = [[int(x) for x in b[2].split("/")] for b in blocks]
                for lz in lzs:
                    wc = int(f["wt_cols"])
                    r = R.reach_of(sizes, nouter, gkin, int(f["qdw"]), int(f["ncoef_up"]), int(f["k_in"]), int(f["k_in_real"]), int(f["job_groups"]),
                                   int(f["job_stages"]), wc, lz)
                    if not r["fits"] and wc > 2:    # use_job_up: scratch groups of 2 columns where the configured width leaves no room
                        wc = 2
                        r = R.reach_of(sizes, nouter, gkin, int(f["qdw"]), int(f["ncoef_up"]), int(f["k_in"]), int(f["k_in_real"]), int(f["job_groups"]),
                                       int(f["job_stages"]), wc, lz)
                    if r["fits"] and not label.startswith("NEW"):
                        kin24 |= r["KIN"] == 24
                    print(row("%s %s lz%d wc%d" % (label, opts, lz, wc), r))
    print("KIN = 24 instantiation reached by a sector above that is not new: %s" % ("yes" if kin24 else "no"))
    for k, c in enumerate(R.all_cases()):
        t = R.tables_of(k)
        gkin = [[int(x) & 0xFFFF for x in t.gmax[int(t.gstart[b]):int(t.gstart[b]) + (c.sizes[b] + 63) // 64]] for b in range(c.nblocks)]
        r = R.reach_of(c.sizes, [a + b for a, b in c.outer], gkin, c.qdw, c.ncoef, t.k_in, t.k_in_real, c.job_groups, c.job_stages, c.wc, c.lz, c.xm, c.wt)
        print(row("synthetic %s lz%d wc%d" % (c.name, c.lz, c.wc), r))


if __name__ == "__main__":
    main()
