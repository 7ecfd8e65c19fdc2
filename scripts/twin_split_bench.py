"""Cost of the twin-sector map on SPLIT sectors (include/hxv.h, hxv_twin_vector with two handles of the same rank) at C3: (7,9) -> (9,7),
Dim = 1.31e8, with P = 2, 4, 8 THREAD RANKS ON ONE GPU (hxv_comm_init_local).

  python scripts/twin_split_bench.py [--reps 20] [--warmup 3] [--ranks 2,4,8] [--sector 7:9] [--no-host] [--out profiles/twin_split_bench.json]

All ranks share the one GPU: the exchange share below is device-to-device copies inside that GPU and waits at two host barriers, NOT link
time, and P host threads launch into one device.  No multi-GPU number comes out of this script.

From one process, one JSON line per P:
  twin_ms, copy_ms     the unsplit hxv_twin_vector and a device-to-device copy of the same 2 x 16 B x Dim, as scripts/twin_bench.py takes them;
  split_ms             the split call, mean of --reps collective calls after warm-up, wall clock around the synchronous call, the MAXIMUM over ranks;
  pack_ms, exchange_ms, unpack_ms   the call's three phases on each rank's stream by HIP events (hxv_get_option "twin_last_*_us"), mean over
                       the calls, per rank; kernels_ms = pack + unpack, the maximum over ranks;
  three_copies_ms      3 x copy_ms: summed over ranks the split route reads and writes the vector three times (pack, exchange copies, unpack);
                       split_over_three_copies is the figure to hold against 1.5;
  host_route_ms        what a split caller has without the entry, timed once, the maximum over ranks: per rank vector_to_host, numpy transpose
                       and scatter into the host vector of the twin sector, vector_from_host of its slab there;
  equals_unsplit / equals_host_route   every rank's result against the unsplit call's columns / the host route's slab, bit for bit."""
import argparse
import json
import sys
import threading
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
    ap.add_argument("--ranks", default="2,4,8")
    ap.add_argument("--sector", default="7:9")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "twin_split_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models

    L = hxv.load_library()
    m = models.hm_2dsquare(Nbath=3)   # bench.py's C3
    nup, ndw = (int(x) for x in a.sector.split(":"))
    assert nup != ndw
    # ---- the unsplit call and the copy, as scripts/twin_bench.py ----
    sa = hxv.HxvSector.from_model(m, nup, ndw)
    sb = hxv.HxvSector.from_model(m, ndw, nup)
    d = torch.empty(sa.localElems, dtype=torch.complex128, device="cuda")
    d.view(torch.float64).normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    d.view(sa.DimDw, sa.pitch)[:, sa.DimUp:] = 0
    full = torch.empty(sb.localElems, dtype=torch.complex128, device="cuda")
    ncopy = min(d.numel(), full.numel())
    torch.cuda.synchronize()

    def twin():
        rc = L.hxv_twin_vector(sa._h, sb._h, d.data_ptr(), full.data_ptr())
        assert rc == 0, L.hxv_last_error()

    def copy():
        full[:ncopy].copy_(d[:ncopy])
        torch.cuda.synchronize()

    twin_ms = _mean_ms(twin, a.warmup, a.reps)
    copy_ms = _mean_ms(copy, a.warmup, a.reps)
    twin()
    v = sa.vector_to_host(d)                      # A's host vector: what every rank cuts its slab from
    dim, dimup_a, dimdw_a, pitch_b = sa.Dim, sa.DimUp, sa.DimDw, sb.pitch
    row_orders = [sa.row_perm is not None, sb.row_perm is not None]
    full_cols = full.view(sb.DimDw, pitch_b)
    del d
    sa.close()
    sb.close()
    lines = []
    for P in (int(x) for x in a.ranks.split(",")):
        w_host = None if a.no_host else np.empty(dim, dtype=np.complex128)   # the twin sector's host vector, filled by all ranks
        bar = threading.Barrier(P)

        def rank(r, group):
            fa = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=P)
            fb = hxv.HxvSector.from_model(m, ndw, nup, rank=r, nranks=P)
            try:
                group.join(fb)
                slab = fa.vector_from_host(v[fa.mpiIshift: fa.mpiIshift + fa.vecDim])
                out = torch.empty(fb.localElems, dtype=torch.complex128, device="cuda")
                torch.cuda.synchronize()
                phases = np.zeros(3)

                def call(timed=False):
                    rc = L.hxv_twin_vector(fa._h, fb._h, slab.data_ptr(), out.data_ptr())
                    assert rc == 0, L.hxv_last_error()
                    if timed:
                        phases[:] += [fb.get_option(k) for k in ("twin_last_pack_us", "twin_last_exchange_us", "twin_last_unpack_us")]

                for _ in range(a.warmup):
                    call()
                bar.wait()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call(True)
                split_ms = (time.perf_counter() - t0) * 1e3 / a.reps
                c0 = fb.mpiIshift // fb.DimUp
                res = {"split_ms": split_ms, "phases_ms": (phases / a.reps * 1e-3).tolist(),
                       "equals_unsplit": bool(torch.equal(out.view(fb.mpiQdw, fb.pitch), full_cols[c0: c0 + fb.mpiQdw]))}
                if not a.no_host:
                    a0 = fa.mpiIshift // fa.DimUp
                    bar.wait()
                    t0 = time.perf_counter()
                    h = fa.vector_to_host(slab)
                    t1 = time.perf_counter()
                    w_host.reshape(dimup_a, dimdw_a)[:, a0: a0 + fa.mpiQdw] = h.reshape(fa.mpiQdw, dimup_a).T
                    bar.wait()                     # (the all-to-all of a caller with MPI: here every rank writes into one host array)
                    t2 = time.perf_counter()
                    ref = fb.vector_from_host(w_host[fb.mpiIshift: fb.mpiIshift + fb.vecDim])
                    t3 = time.perf_counter()
                    res.update({"host_ms": [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3],
                                "equals_host_route": bool(torch.equal(ref, out))})
                    del ref, h
                return res
            finally:
                fa.close()
                fb.close()

        rs = hxv.run_ranks(P, rank)
        ph = np.array([r["phases_ms"] for r in rs])
        split_ms = max(r["split_ms"] for r in rs)
        line = {"model": "C3", "from": [nup, ndw], "to": [ndw, nup], "Dim": dim, "nranks": P,
                "transport": "thread ranks sharing ONE GPU: the exchange is device-to-device copies and barrier waits, not link time; no multi-GPU number",
                "row_order_from": row_orders[0], "row_order_to": row_orders[1], "reps": a.reps,
                "twin_ms": twin_ms, "copy_ms": copy_ms, "split_ms": split_ms, "split_ms_per_rank": [r["split_ms"] for r in rs],
                "pack_ms_per_rank": ph[:, 0].tolist(), "exchange_ms_per_rank": ph[:, 1].tolist(), "unpack_ms_per_rank": ph[:, 2].tolist(),
                "kernels_ms": float((ph[:, 0] + ph[:, 2]).max()), "three_copies_ms": 3 * copy_ms, "split_over_three_copies": split_ms / (3 * copy_ms),
                "within_1p5": bool(split_ms <= 1.5 * 3 * copy_ms), "equals_unsplit": all(r["equals_unsplit"] for r in rs)}
        if not a.no_host:
            hm = np.array([r["host_ms"] for r in rs]).max(axis=0)
            line.update({"host_to_host_ms": hm[0], "host_transpose_scatter_ms": hm[1], "host_from_host_ms": hm[2], "host_route_ms": hm[3],
                         "host_over_split": hm[3] / split_ms, "equals_host_route": all(r["equals_host_route"] for r in rs)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del w_host
        torch.cuda.empty_cache()
        hxv.pool_trim()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
