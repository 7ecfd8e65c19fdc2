"""Cost of the twin-sector map (include/hxv.h, hxv_twin_vector) at C3: (7,9) -> (9,7), Dim = 1.31e8, and (8,8) onto itself, Dim = 1.66e8.

  python scripts/twin_bench.py [--reps 20] [--warmup 3] [--sectors 7:9,8:8] [--no-host]

Three times from one process, per sector pair:
  twin_ms       hxv_twin_vector, mean of --reps calls after warm-up, wall clock around the synchronous call;
  copy_ms       a device-to-device copy of the same 2 x 16 B x Dim (read the vector once, write it once), wall clock around copy + synchronise:
                the yardstick, what pure data movement of this size costs without a transpose;
  host_route_ms what a caller has without the entry: vector_to_host, numpy transpose, vector_from_host (timed once, parts reported),
                whose result the device vector is compared with bit for bit.
Prints one JSON line per pair."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd")]


def _mean_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sectors", default="7:9,8:8")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models

    L = hxv.load_library()
    m = models.hm_2dsquare(Nbath=3)   # bench.py's C3
    for pair in a.sectors.split(","):
        nup, ndw = (int(x) for x in pair.split(":"))
        sa = hxv.HxvSector.from_model(m, nup, ndw)
        sb = sa if nup == ndw else hxv.HxvSector.from_model(m, ndw, nup)
        d = torch.empty(sa.localElems, dtype=torch.complex128, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        d.view(torch.float64).normal_(generator=g)
        d.view(sa.DimDw, sa.pitch)[:, sa.DimUp:] = 0
        out = torch.empty(sb.localElems, dtype=torch.complex128, device="cuda")
        ncopy = min(d.numel(), out.numel())   # (equal for a twin pair: pitch_A * DimDw_A against pitch_B * DimDw_B differ by padding only)
        torch.cuda.synchronize()

        def twin():
            rc = L.hxv_twin_vector(sa._h, sb._h, d.data_ptr(), out.data_ptr())
            assert rc == 0, L.hxv_last_error()

        def copy():
            out[:ncopy].copy_(d[:ncopy])
            torch.cuda.synchronize()

        twin_ms = _mean_ms(twin, a.warmup, a.reps)
        copy_ms = _mean_ms(copy, a.warmup, a.reps)
        twin()
        res = {"model": "C3", "from": [nup, ndw], "to": [ndw, nup], "Dim": sa.Dim, "row_order_from": sa.row_perm is not None,
               "row_order_to": sb.row_perm is not None, "bytes_moved": 32 * sa.Dim, "twin_ms": twin_ms, "copy_ms": copy_ms,
               "twin_over_copy": twin_ms / copy_ms, "twin_GBps": 32 * sa.Dim / twin_ms / 1e6, "copy_GBps": 32 * sa.Dim / copy_ms / 1e6}
        if not a.no_host:
            t0 = time.perf_counter()
            v = sa.vector_to_host(d)
            t1 = time.perf_counter()
            w = np.ascontiguousarray(v.reshape(sa.DimDw, sa.DimUp).T).ravel()
            t2 = time.perf_counter()
            ref = sb.vector_from_host(w)
            t3 = time.perf_counter()
            res.update({"host_to_host_ms": (t1 - t0) * 1e3, "host_transpose_ms": (t2 - t1) * 1e3, "host_from_host_ms": (t3 - t2) * 1e3,
                        "host_route_ms": (t3 - t0) * 1e3, "host_over_twin": (t3 - t0) * 1e3 / twin_ms,
                        "equals_host_route": bool(torch.equal(ref, out))})
            del v, w, ref
        print(json.dumps(res), flush=True)
        del d, out
        sa.close()
        if sb is not sa:
            sb.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
