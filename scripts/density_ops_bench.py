"""Cost of the density-type operators (include/hxv.h, hxv_apply_density_ops) per call at C3 and C4, sector (8,8), Dim = 1.66e8, and of the
whole chi_spin stage of the 2x2 cluster.

  python scripts/density_ops_bench.py [--reps 10] [--warmup 3] [--models C3,C4] [--nlanc 200] [--no-stage] [--out FILE]

Cases: nops = 1, 4, 8 at C3 and nops = 8 at C4, generic coefficients, subtract_mean on.  HIP events on the current stream around each call
after warm-up (the call is synchronous; the occupation words are cached with the sector image after the first call), median over --reps.
A call moves 16 + (16 + 16 nops) bytes per basis state; next to each case, from the same process, a device-to-device copy that moves the
same number of bytes ((2 + nops) / 2 vectors read and written) gives the copy rate, and the project's target for a streaming pass is
time <= 1.25 x bytes moved / that rate: `ratio_to_copy` is time / (bytes moved / copy rate).  The stage (C3 only): observables.susceptibility
with kind "spin" on a random unit state, once with a real state (what an eigenstate of a real H is: the real-vector kernels) and once with a
complex one, i.e. one hxv_apply_density_ops call, four hxv_lanczos_tridiag_probes runs of --nlanc steps with
four probes each, the pole sums at 64 frequencies.  Prints one JSON line per case; --out appends them to a file as well."""
import argparse
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
    ap.add_argument("--models", default="C3,C4")
    ap.add_argument("--nlanc", type=int, default=200)
    ap.add_argument("--no-stage", action="store_true")
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

    for name in a.models.split(","):
        m = models.hm_2dsquare(Nbath=3) if name == "C3" else models.bhz_2d(Nbath=1)   # bench.py's C3 and C4
        nimp = m.Nlat * m.Norb
        sec = hxv.HxvSector.from_model(m, 8, 8)
        d = torch.empty(sec.localElems, dtype=torch.complex128, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        d.view(torch.float64).normal_(generator=g)
        d.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
        d /= torch.linalg.vector_norm(d)
        base = {"model": name, "Nimp": nimp, "Dim": sec.Dim, "row_order": sec.row_perm is not None}
        rng = np.random.default_rng(3)
        for nops in ((1, 4, 8) if name == "C3" else (8,)):
            cf = rng.standard_normal((nops, 2, nimp))
            outs = [torch.empty_like(d) for _ in range(nops)]
            t0 = time.perf_counter()
            sec.apply_density_ops(cf, d, out=outs)
            first_ms = (time.perf_counter() - t0) * 1e3       # includes building and uploading the occupation words
            ms, ms_min = _median_ms(lambda: sec.apply_density_ops(cf, d, out=outs), a.warmup, a.reps)
            del outs
            moved = sec.Dim * (16 + 16 + 16 * nops)
            n = sec.Dim * (2 + nops) // 2                     # a copy of n elements reads and writes the same number of bytes
            src, dst = torch.empty(n, dtype=torch.complex128, device="cuda"), torch.empty(n, dtype=torch.complex128, device="cuda")
            src.view(torch.float64).normal_(generator=g)
            copy_ms, copy_min = _median_ms(lambda: dst.copy_(src), a.warmup, a.reps)
            del src, dst
            rate = 32.0 * n / (copy_ms * 1e-3)
            emit(dict(base, case="apply_density_ops", nops=nops, ms_per_call=ms, ms_min=ms_min, ms_first_call=first_ms, bytes_moved=moved,
                      d2d_copy_same_bytes_ms=copy_ms, d2d_copy_min_ms=copy_min, copy_rate_TBs=rate / 1e12, call_rate_TBs=moved / (ms * 1e-3) / 1e12,
                      ratio_to_copy=ms / (moved / rate * 1e3), target_ratio=1.25))
            torch.cuda.empty_cache()
        if name == "C3" and not a.no_stage:
            z = 2j * np.pi * np.arange(64) / 50.0
            for real_state in (True, False):                  # an eigenstate of a real H is real: the runs take the real-vector kernels
                if real_state:
                    psi = torch.complex(d.real, torch.zeros_like(d.real))
                    psi /= torch.linalg.vector_norm(psi)
                else:
                    psi = d
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                chi, info = observables.susceptibility(sec, psi, 0.0, "spin", z, nlanc=a.nlanc)
                stage_ms = (time.perf_counter() - t0) * 1e3
                emit(dict(base, case="chi_spin_stage", real_state=real_state, runs=nimp, nlanc=a.nlanc, steps=[int(x) for x in info["nsteps"]],
                          stage_ms=stage_ms, ms_per_run_step=stage_ms / max(int(info["nsteps"].sum()), 1),
                          real_vectors=int(sec.get_option("lanczos_real_last"))))
                del psi
        del d
        sec.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
