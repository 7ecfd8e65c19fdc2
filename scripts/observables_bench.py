"""Cost of the impurity-observables record (include/hxv.h, hxv_observables_accumulate) per state at C3 and C4, sector (8,8), Dim = 1.66e8.

  python scripts/observables_bench.py [--reps 10] [--warmup 3] [--models C3,C4] [--host]

Device route: HIP events on the current stream around each call after warm-up (the call is synchronous: tables are cached with the sector
image after the first call, scratch comes from the engine's buffer cache), median over --reps.  bytes_requested_est is an ESTIMATE from binomial pair counts
(W reads the vector once; two 16-B gathers per row pair for R_up and two columns per column pair for R_dw, over the is < js half).
Where the time goes per kernel: run this script under rocprofv3 --kernel-trace --stats.  With --host,
the route a caller has without this entry: vector_to_host + the numpy record (tests/observables_ref.record_numpy), timed once.
Prints one JSON line per model."""
import argparse
import json
import sys
import time
from math import comb
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="C3,C4")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hxv
    from hxv import models

    for name in a.models.split(","):
        m = models.hm_2dsquare(Nbath=3) if name == "C3" else models.bhz_2d(Nbath=1)   # bench.py's C3 and C4
        sec = hxv.HxvSector.from_model(m, 8, 8)
        d = torch.empty(sec.localElems, dtype=torch.complex128, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        d.view(torch.float64).normal_(generator=g)
        d.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
        d /= torch.linalg.vector_norm(d)
        rec = np.zeros(hxv.load_library().hxv_obs_record_elems(sec._h))
        t0 = time.perf_counter()
        sec.observables_record(d, out=rec)
        first_ms = (time.perf_counter() - t0) * 1e3   # includes building and uploading the pair tables
        for _ in range(a.warmup):
            sec.observables_record(d, out=rec)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sec.observables_record(d, out=rec)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        N = m.Nlat * m.Norb
        # pairs per up row / per column: sum over configurations of (occupied impurity) x (empty impurity) orbitals
        ns, n = m.Ns, 8
        pairs = sum(comb(N, k) * comb(ns - N, n - k) * k * (N - k) for k in range(N + 1)) / comb(ns, n)
        vec_bytes = sec.DimDw * sec.DimUp * 16
        res = {"model": name, "Nimp": N, "Dim": sec.Dim, "ms_per_state": float(np.median(ms)), "ms_min": float(np.min(ms)),
               "ms_first_call": first_ms, "pairs_per_row": pairs,
               # ESTIMATE, not measured: W reads the vector once; R_up makes two 16-B gathers per row pair and R_dw reads two columns per column
               # pair, for the is < js half of the pairs (the other half is the conjugate)
               "bytes_requested_est": int(vec_bytes * (1 + 2 * pairs)),
               "vector_bytes": vec_bytes}
        if a.host:
            from observables_ref import record_numpy

            mu, md = sec.maps()
            t0 = time.perf_counter()
            v = sec.vector_to_host(d)
            t1 = time.perf_counter()
            record_numpy(m, mu, md, v)
            t2 = time.perf_counter()
            res.update({"host_copy_ms": (t1 - t0) * 1e3, "host_numpy_record_ms": (t2 - t1) * 1e3})
            del v
        print(json.dumps(res), flush=True)
        del d
        sec.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
