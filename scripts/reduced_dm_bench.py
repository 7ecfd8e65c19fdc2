"""Cost of the reduced density matrix of an impurity-orbital subset (include/hxv.h, hxv_reduced_dm_accumulate) per state at C3 and C4,
sector (8,8), Dim = 1.66e8.

  python scripts/reduced_dm_bench.py [--reps 10] [--warmup 3] [--models C3,C4] [--no-host] [--out FILE]

Cases per model: one orbital, one site (two orbitals at C4; the same mask as one orbital at C3), two sites, four orbitals (the whole cluster at
C3, every second orbital at C4).  Device route: HIP events on the current stream around each call after warm-up (the call is synchronous; the
tables of a mask are cached with the sector image after the first call), median over --reps.  Masks whose classes all fit the one-thread-
per-pair kernel (one and two orbitals) are measured a second time in the same process with every class sent to the register-tile kernel
(the hook HXV_RDM_PAIR_KERNEL=0, read when the tables of a mask are looked up): the A/B of the two accumulate kernels.  Next to the cases,
from the same run: hxv_cluster_dm_accumulate on the same state (C3; C4 has none), a device-to-device copy of the vector (one read and one
write of it: the read alone is the floor of any of this), and the route a caller has without this entry -- vector_to_host once, then the
numpy matrix (tests/reduced_dm_ref.direct) per mask, timed once -- whose result the device matrix is compared with.
Prints one JSON line per case; --out appends them to a file as well."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "tests")]

HBM_BYTES_PER_S = 6.29e12
AB_HOOK = "HXV_RDM_PAIR_KERNEL"


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

    os.environ.pop(AB_HOOK, None)
    for name in a.models.split(","):
        m = models.hm_2dsquare(Nbath=3) if name == "C3" else models.bhz_2d(Nbath=1)   # bench.py's C3 and C4
        N = m.Nlat * m.Norb
        cases = [("one_orbital", (0,)), ("one_site", tuple(range(m.Norb))), ("two_sites", tuple(range(2 * m.Norb))),
                 ("four_orbitals", (0, 1, 2, 3) if N == 4 else (0, 2, 4, 6))]
        cases = [c for i, c in enumerate(cases) if c[1] not in [x[1] for x in cases[:i]]]
        sec = hxv.HxvSector.from_model(m, 8, 8)
        d = torch.empty(sec.localElems, dtype=torch.complex128, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        d.view(torch.float64).normal_(generator=g)
        d.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
        d /= torch.linalg.vector_norm(d)
        floor_ms = sec.Dim * 16 / HBM_BYTES_PER_S * 1e3
        dst = torch.empty_like(d)
        copy_ms, _ = _median_ms(lambda: dst.copy_(d), a.warmup, a.reps)
        del dst
        base = {"model": name, "Nimp": N, "Dim": sec.Dim, "row_order": sec.row_perm is not None, "d2d_copy_ms": copy_ms, "floor_ms": floor_ms}
        if hxv.load_library().hxv_cluster_dm_elems(sec._h) > 0:
            rho = np.zeros((4 ** N, 4 ** N), dtype=np.complex128, order="F")
            sec.cluster_dm(d, out=rho)
            ms, ms_min = _median_ms(lambda: sec.cluster_dm(d, out=rho), a.warmup, a.reps)
            emit(dict(base, case="cluster_dm_full", ms_per_state=ms, ms_min=ms_min))
        v = None
        if not a.no_host:
            mu, md = sec.maps()
            t0 = time.perf_counter()
            v = sec.vector_to_host(d)
            host_copy_ms = (time.perf_counter() - t0) * 1e3
        for case, mask in cases:
            for fs in (False, True):
                rho = np.zeros((4 ** len(mask),) * 2, dtype=np.complex128, order="F")
                t0 = time.perf_counter()
                sec.reduced_dm(d, mask, fermi_sign=fs, out=rho)
                first_ms = (time.perf_counter() - t0) * 1e3   # includes building and uploading the group tables and the work list
                ms, ms_min = _median_ms(lambda: sec.reduced_dm(d, mask, fermi_sign=fs, out=rho), a.warmup, a.reps)
                res = dict(base, case=case, mask=list(mask), fermi_sign=int(fs), ms_per_state=ms, ms_min=ms_min, ms_first_call=first_ms,
                           ratio_to_floor=ms / floor_ms, trace=float(np.trace(rho).real))
                if len(mask) <= 2 and not fs:   # the A/B of the two accumulate kernels: the same classes through the register-tile kernel
                    alt = np.zeros_like(rho)
                    os.environ[AB_HOOK] = "0"
                    try:
                        sec.reduced_dm(d, mask, fermi_sign=fs, out=alt)
                        ms_t, ms_t_min = _median_ms(lambda: sec.reduced_dm(d, mask, fermi_sign=fs, out=alt), a.warmup, a.reps)
                    finally:
                        os.environ.pop(AB_HOOK, None)
                    ms2, _ = _median_ms(lambda: sec.reduced_dm(d, mask, fermi_sign=fs, out=rho), 1, a.reps)   # the pair kernel again, after
                    res.update({"ab_pair_kernel_ms": ms, "ab_pair_kernel_again_ms": ms2, "ab_tile_kernel_ms": ms_t, "ab_tile_kernel_min_ms": ms_t_min,
                                "ab_max_abs_diff": float(np.abs(alt - rho).max())})
                if v is not None:
                    from reduced_dm_ref import direct

                    t1 = time.perf_counter()
                    ref = direct(m, mu, md, v, mask, 1.0, int(fs))
                    host_ms = (time.perf_counter() - t1) * 1e3
                    res.update({"host_copy_ms": host_copy_ms, "host_numpy_matrix_ms": host_ms, "host_route_ms": host_copy_ms + host_ms,
                                "max_abs_diff_to_host": float(np.abs(rho - ref).max())})
                    del ref
                emit(res)
        del d, v
        sec.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
