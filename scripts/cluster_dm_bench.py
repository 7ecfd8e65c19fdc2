"""Cost of the cluster reduced density matrix (include/hxv.h, hxv_cluster_dm_accumulate) per state at C3 and C4, sector (8,8), Dim = 1.66e8.

  python scripts/cluster_dm_bench.py [--reps 10] [--warmup 3] [--models C3,C4] [--no-host]

Device route: HIP events on the current stream around each call after warm-up (the call is synchronous: tables are cached with the sector
image after the first call, scratch comes from the engine's buffer cache), median over --reps.  Next to it, from the same run: the existing
observables record (hxv_observables_accumulate), one product (hxv_time_apply), and the route a caller has without this entry --
vector_to_host + the numpy matrix (tests/cluster_dm_ref.vectorised), timed once -- whose result the device matrix is compared with.
floor_ms is one read of the vector, 16 B x Dim at 6.29 TB/s; cmadds is the count of complex multiply-adds of the Hermitian triangle
(sum over bath pairs of n(n+1)/2).  Where the time goes per kernel: run this script under rocprofv3 --kernel-trace --stats.
Prints one JSON line per model."""
import argparse
import json
import sys
import time
from math import comb
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "tests")]

HBM_BYTES_PER_S = 6.29e12


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
    ap.add_argument("--models", default="C3,C4")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models

    for name in a.models.split(","):
        m = models.hm_2dsquare(Nbath=3) if name == "C3" else models.bhz_2d(Nbath=1)   # bench.py's C3 and C4
        sec = hxv.HxvSector.from_model(m, 8, 8)
        if hxv.load_library().hxv_cluster_dm_elems(sec._h) == 0:   # C4: Nimp 8, a dense matrix of 16^8 elements
            print(json.dumps({"model": name, "Nimp": m.Nlat * m.Norb, "Dim": sec.Dim, "unsupported": "Nimp > 5"}), flush=True)
            sec.close()
            continue
        d = torch.empty(sec.localElems, dtype=torch.complex128, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        d.view(torch.float64).normal_(generator=g)
        d.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
        d /= torch.linalg.vector_norm(d)
        N = m.Nlat * m.Norb
        rho = np.zeros((4 ** N, 4 ** N), dtype=np.complex128, order="F")
        t0 = time.perf_counter()
        sec.cluster_dm(d, out=rho)
        first_ms = (time.perf_counter() - t0) * 1e3   # includes building and uploading the group tables and the work list
        ms, ms_min = _median_ms(lambda: sec.cluster_dm(d, out=rho), a.warmup, a.reps)
        rec = np.zeros(hxv.load_library().hxv_obs_record_elems(sec._h))
        sec.observables_record(d, out=rec)
        obs_ms, _ = _median_ms(lambda: sec.observables_record(d, out=rec), a.warmup, a.reps)
        hv = torch.empty_like(d)
        sec.time_apply(d, hv, a.warmup)
        product_ms = sec.time_apply(d, hv, a.reps)
        del hv
        nb, n = m.Ns - N, 8
        cls = [(comb(N, n - k) , comb(nb, k)) for k in range(nb + 1) if 0 <= n - k <= N]   # (block side, bath configurations) per spin
        cmadds = sum(gu * gd * (du * dd) * (du * dd + 1) // 2 for du, gu in cls for dd, gd in cls)
        floor_ms = sec.Dim * 16 / HBM_BYTES_PER_S * 1e3
        res = {"model": name, "Nimp": N, "Dim": sec.Dim, "ms_per_state": ms, "ms_min": ms_min, "ms_first_call": first_ms,
               "observables_record_ms": obs_ms, "product_ms": product_ms, "products_per_state": ms / product_ms,
               "floor_ms": floor_ms, "ratio_to_floor": ms / floor_ms, "cmadds": cmadds, "largest_block": max(du for du, _ in cls) ** 2,
               "trace": float(np.trace(rho).real)}
        if not a.no_host:
            from cluster_dm_ref import vectorised

            mu, md = sec.maps()
            t0 = time.perf_counter()
            v = sec.vector_to_host(d)
            t1 = time.perf_counter()
            ref = vectorised(m, mu, md, v)
            t2 = time.perf_counter()
            res.update({"host_copy_ms": (t1 - t0) * 1e3, "host_numpy_matrix_ms": (t2 - t1) * 1e3, "host_route_ms": (t2 - t0) * 1e3,
                        "device_beats_host": bool(ms < (t2 - t0) * 1e3), "max_abs_diff_to_host": float(np.abs(rho - ref).max())})
            del v, ref
        print(json.dumps(res), flush=True)
        del d
        sec.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
