"""Cost of hxv_apply_one_body (include/hxv.h) per call at C3, sector (8,8), next to a device-to-device copy of one vector and to the route
the engine offered before: two hxv_apply_ladder_axpy calls per term through an intermediate sector.

  python scripts/one_body_bench.py [--reps 10] [--warmup 3] [--out profiles/one_body_bench.json]

Cases: one up term c^+_0 c_1; one dw term; the 8-term current operator of the two x-bonds (0,1), (2,3) of the plaquette; the 16-term kinetic
operator of the 2x2 cluster (four bonds, both directions, both spins).  For each: (new) one hxv_apply_one_body call without and with the
mean subtracted, tables cached (the first call, which builds them, is reported apart); (a) a device-to-device copy of the vector's bytes;
(b) per term hxv_apply_ladder_axpy (c_j) into a vector of the intermediate sector, (7,8) for an up term and (8,7) for a dw term, then
hxv_apply_ladder_axpy (c^+_i) with `accumulate` back into the sector.  The cold open of each intermediate sector (sector cache cleared) is
reported apart, as is the memory of its vector.  The byte model beside the ratio to the copy: 16 B written + 16 B of the thread's own
element read + 16 B per reached term element, over the copy's 32 B.  HIP events around each synchronous call after warm-up; median, minimum
and maximum over --reps.  Prints one JSON line per case; --out appends them to a file as well."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd")]


def _times_ms(fn, warmup, reps):
    import numpy as np
    import torch

    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models, observables

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    L = hxv.load_library()
    m = models.hm_2dsquare(Nbath=3)                              # bench.py's C3
    nup = ndw = 8
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    psi = torch.empty(sec.localElems, dtype=torch.complex128, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    psi.view(torch.float64).normal_(generator=g)
    psi.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
    psi /= torch.linalg.vector_norm(psi)
    h = np.asarray(m.impHloc)[:, :, 0, 0, 0, 0]
    kinetic = [(s, i, j, complex(h[i, j])) for s in (0, 1) for i in range(4) for j in range(4) if i != j and h[i, j] != 0]
    current = [t for op in observables.one_body_terms("current", [(0, 1), (2, 3)]) for t in op]
    cases = [("one_up_term", [(0, 0, 1, 1.0)]), ("one_dw_term", [(1, 0, 1, 1.0)]), ("current_x_bonds_8", current), ("kinetic_16", kinetic)]
    assert len(current) == 8 and len(kinetic) == 16
    mu, md = sec.maps()
    n2 = C.c_double()
    out = torch.empty_like(psi)
    for name, terms in cases:
        t0 = time.perf_counter()
        _, first_mean, first_n2 = sec.apply_one_body(terms, psi, subtract_mean=False, out=out)
        first_ms = (time.perf_counter() - t0) * 1e3              # includes building and uploading the tables
        ms = _times_ms(lambda: sec.apply_one_body(terms, psi, subtract_mean=False, out=out), a.warmup, a.reps)
        new_host = sec.vector_to_host(out)
        ms_sub = _times_ms(lambda: sec.apply_one_body(terms, psi, subtract_mean=True, out=out), a.warmup, a.reps)
        # the reached share of the targets, term by term, from the basis maps: the byte model's third summand
        reached = 0.0
        for s, i, j, _ in terms:
            cfg = np.asarray(md if s else mu, dtype=np.int64)
            live = ((cfg >> i) & 1) == 1
            if i != j:
                live &= ((cfg >> j) & 1) == 0
            reached += float(live.mean())
        model_ratio = (32.0 + 16.0 * reached) / 32.0
        # (a) a copy of one vector's bytes
        cp = torch.empty_like(out)
        copy = _times_ms(lambda: cp.copy_(out), a.warmup, a.reps)
        del cp
        # (b) two ladder calls per term through the intermediate sector of the term's spin
        spins = sorted({t[0] for t in terms})
        hxv.sector_cache_clear()
        mids, open_ms = {}, {}
        for s in spins:
            t0 = time.perf_counter()
            mids[s] = hxv.HxvSector.from_model(m, nup - (s == 0), ndw - (s == 1))
            open_ms[s] = (time.perf_counter() - t0) * 1e3
        tmps = {s: torch.empty(mids[s].localElems, dtype=torch.complex128, device="cuda") for s in spins}
        out_b = torch.empty_like(out)

        def ladder_route():
            for k, (s, i, j, c) in enumerate(terms):
                c = complex(c)
                L.hxv_apply_ladder_axpy(sec._h, mids[s]._h, j, s, 0, 1.0, 0.0, 0, psi.data_ptr(), tmps[s].data_ptr(), None)
                rc = L.hxv_apply_ladder_axpy(mids[s]._h, sec._h, i, s, 1, c.real, c.imag, int(k > 0), tmps[s].data_ptr(), out_b.data_ptr(), C.byref(n2))
                assert rc == 0, L.hxv_last_error().decode()

        torch.cuda.synchronize()
        lad = _times_ms(ladder_route, a.warmup, a.reps)
        diff = float(np.abs(sec.vector_to_host(out_b) - new_host).max())
        emit(dict(model="C3", case=name, sector=[nup, ndw], nterms=len(terms), elems=sec.Dim, vector_bytes=16 * sec.localElems, row_order=sec.row_perm is not None,
                  warmup=a.warmup, reps=a.reps, one_body_ms=ms[0], one_body_min_ms=ms[1], one_body_max_ms=ms[2], one_body_first_call_ms=first_ms,
                  one_body_subtract_mean_ms=ms_sub[0], one_body_subtract_mean_min_ms=ms_sub[1], one_body_subtract_mean_max_ms=ms_sub[2],
                  d2d_copy_ms=copy[0], d2d_copy_min_ms=copy[1], d2d_copy_max_ms=copy[2], ratio_to_copy=ms[0] / copy[0],
                  reached_share_summed=reached, byte_model_ratio_to_copy=model_ratio, ratio_over_byte_model=ms[0] / copy[0] / model_ratio,
                  ladder_route_ms=lad[0], ladder_route_min_ms=lad[1], ladder_route_max_ms=lad[2], ladder_route_ms_per_term=lad[0] / len(terms),
                  one_body_ms_per_term=ms[0] / len(terms), speedup_over_ladder_route=lad[0] / ms[0],
                  intermediate_sectors=[[nup - (s == 0), ndw - (s == 1)] for s in spins], intermediate_open_cold_ms=[open_ms[s] for s in spins],
                  intermediate_vector_bytes=[16 * mids[s].localElems for s in spins], max_abs_diff_to_ladder_route=diff,
                  mean=[first_mean.real, first_mean.imag], norm2=first_n2))
        del tmps, out_b
        for s in spins:
            mids[s].close()
        torch.cuda.empty_cache()
    sec.close()


if __name__ == "__main__":
    main()
