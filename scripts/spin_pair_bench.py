"""Cost of hxv_apply_spin_pair (include/hxv.h) per call at C3, source sector (8,8), next to a device-to-device copy of the target vector and
to the route the engine offered before: two hxv_apply_ladder_axpy calls per term through an intermediate sector.

  python scripts/spin_pair_bench.py [--reps 10] [--warmup 3] [--out profiles/spin_pair_bench.json]

Cases: (8,8) -> (7,7) with 1 term, the 4-term on-site s-wave and the 8-term d-wave pair operator of the 2x2 cluster; (8,8) -> (7,9) with
S^- of one orbital.  For each: (new) one hxv_apply_spin_pair call, tables cached (the first call, which builds them, is reported apart);
(a) a device-to-device copy of the target vector's bytes; (b) per term hxv_apply_ladder_axpy into a vector of the intermediate sector,
(8,7) for the pair operators and (7,8) for S^-, then hxv_apply_ladder_axpy with `accumulate` into the target.  The cold open of that
intermediate sector (sector cache cleared) is reported apart, as is the memory of its vector.  HIP events around each synchronous call after
warm-up, median over --reps.  Prints one JSON line per case; --out appends them to a file as well."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd")]


def _median_ms(fn, warmup, reps):
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
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    L = hxv.load_library()
    m = models.hm_2dsquare(Nbath=3)                              # bench.py's C3
    src = hxv.HxvSector.from_model(m, 8, 8)
    psi = torch.empty(src.localElems, dtype=torch.complex128, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    psi.view(torch.float64).normal_(generator=g)
    psi.view(src.DimDw, src.pitch)[:, src.DimUp:] = 0
    psi /= torch.linalg.vector_norm(psi)
    d_wave = []
    for (i, j), sg in (((0, 1), 1.0), ((2, 3), 1.0), ((0, 2), -1.0), ((1, 3), -1.0)):
        d_wave += [(i, j, 0.5 * sg), (j, i, 0.5 * sg)]
    cases = [("one_term", (7, 7), (False, False), [(0, 0, 1.0)]),
             ("s_wave_4", (7, 7), (False, False), [(i, i, 0.5) for i in range(4)]),
             ("d_wave_8", (7, 7), (False, False), d_wave),
             ("s_minus_1", (7, 9), (False, True), [(0, 0, 1.0)])]
    n2 = C.c_double()
    for name, (tu, td), (cu, cd), terms in cases:
        dst = hxv.HxvSector.from_model(m, tu, td)
        out = torch.empty(dst.localElems, dtype=torch.complex128, device="cuda")
        t0 = time.perf_counter()
        _, first_n2 = src.apply_spin_pair(dst, terms, cu, cd, psi, out=out)
        first_ms = (time.perf_counter() - t0) * 1e3              # includes building and uploading the tables
        ms, ms_min = _median_ms(lambda: src.apply_spin_pair(dst, terms, cu, cd, psi, out=out), a.warmup, a.reps)
        new_host = dst.vector_to_host(out)
        # (a) a copy of the target vector's bytes
        cp = torch.empty_like(out)
        copy_ms, copy_min = _median_ms(lambda: cp.copy_(out), a.warmup, a.reps)
        del cp
        # (b) two ladder calls per term through the intermediate sector: the dw operator first for the pair operators ((8,8) -> (8,7) ->
        # (7,7)), the up operator first for S^- ((8,8) -> (7,8) -> (7,9))
        dw_first = (tu, td) == (7, 7)
        hxv.sector_cache_clear()
        t0 = time.perf_counter()
        mid = hxv.HxvSector.from_model(m, 8, 7) if dw_first else hxv.HxvSector.from_model(m, 7, 8)
        open_ms = (time.perf_counter() - t0) * 1e3
        tmp = torch.empty(mid.localElems, dtype=torch.complex128, device="cuda")
        out_b = torch.empty_like(out)

        def ladder_route():
            for k, (i, j, c) in enumerate(terms):
                c = complex(c)
                if dw_first:
                    L.hxv_apply_ladder_axpy(src._h, mid._h, j, 1, int(cd), 1.0, 0.0, 0, psi.data_ptr(), tmp.data_ptr(), None)
                    rc = L.hxv_apply_ladder_axpy(mid._h, dst._h, i, 0, int(cu), c.real, c.imag, int(k > 0), tmp.data_ptr(), out_b.data_ptr(), C.byref(n2))
                else:
                    L.hxv_apply_ladder_axpy(src._h, mid._h, i, 0, int(cu), 1.0, 0.0, 0, psi.data_ptr(), tmp.data_ptr(), None)
                    rc = L.hxv_apply_ladder_axpy(mid._h, dst._h, j, 1, int(cd), c.real, c.imag, int(k > 0), tmp.data_ptr(), out_b.data_ptr(), C.byref(n2))
                assert rc == 0, L.hxv_last_error().decode()

        torch.cuda.synchronize()
        lad_ms, lad_min = _median_ms(ladder_route, a.warmup, a.reps)
        diff = float(np.abs(dst.vector_to_host(out_b) - new_host).max())
        emit(dict(model="C3", case=name, source=[8, 8], target=[tu, td], nterms=len(terms), target_elems=dst.Dim, target_bytes=16 * dst.localElems,
                  row_order=[src.row_perm is not None, dst.row_perm is not None], spin_pair_ms=ms, spin_pair_min_ms=ms_min, spin_pair_first_call_ms=first_ms,
                  d2d_copy_ms=copy_ms, d2d_copy_min_ms=copy_min, ratio_to_copy=ms / copy_ms, ladder_route_ms=lad_ms, ladder_route_min_ms=lad_min,
                  ladder_route_ms_per_term=lad_ms / len(terms), spin_pair_ms_per_term=ms / len(terms), speedup_over_ladder_route=lad_ms / ms,
                  intermediate_sector=[8, 7] if dw_first else [7, 8], intermediate_open_cold_ms=open_ms, intermediate_vector_bytes=16 * mid.localElems,
                  max_abs_diff_to_ladder_route=diff, norm2=first_n2))
        del tmp, out_b, out
        mid.close()
        dst.close()
        torch.cuda.empty_cache()
    src.close()


if __name__ == "__main__":
    main()
