"""Cost of the Chebyshev recurrence (include/hxv.h: hxv_chebyshev_moments, hxv_chebyshev_apply and their _real forms) per order at C3, sector
(8,8), next to the product alone and to device-to-device copies; and of hxv_vector_random next to a copy and to vector_from_host.
Section "real" of the output: the same measurements on the real-vector path of the same build (real product, real drivers with the complex
per-order time beside them, the real step kernel through tests/device/chebyshev_real_kernels_check.hip with (3 + M) * 8 B per state, its
time per byte of its own traffic over the copy's).

  python scripts/chebyshev_bench.py [--orders 10] [--reps 5] [--warmup 2] [--out profiles/chebyshev_bench.json]

Per order, from the drivers: (time of a run with `orders` products - time of a run with none) / orders, for moments with 0, 1, 4 and 8 probes
and for apply; that is one product, one fused step, the all-in-one reduction and the order's stream synchronisation.  The product alone:
apply_device_slab.  The step kernel alone: the engine's own kernel through the test-only launchers (tests/device/chebyshev_kernels_check.hip)
on the driver's grid, with M in {0, 1, 4, 8} probes, with and without the running sum.  Beside each: a device-to-device copy of
(3 + M) * 16 B per state, (4 + M) * 16 B with a running sum -- the vectors the step touches; the copy reads and writes that many bytes --
and the step's own traffic, (3 + M) reads + 1 write without and (4 + M) reads + 2 writes with the running sum.  The project's target for a
streaming pass is 1.25 x the copy of the same bytes.  HIP events (drivers, copies) and the host clock around the synchronous launchers
(kernels); median, minimum and maximum over --reps.  One JSON object in --out."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd")]


def _stats(ms):
    import numpy as np

    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def _event_ms(fn, warmup, reps):
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
    return ms


def _clock_ms(fn, warmup, reps):
    import torch

    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                   # (the launchers wait for the kernel)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "chebyshev_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    import hxv
    from hxv import chebyshev as ch, models

    m = models.hm_2dsquare(Nbath=3)                              # bench.py's C3
    nup = ndw = 8
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    n = sec.localElems

    def vector(seed):
        v = torch.empty(n, dtype=torch.complex128, device="cuda")
        v.view(torch.float64).normal_(generator=torch.Generator(device="cuda").manual_seed(seed))
        v.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = 0
        return v / torch.linalg.vector_norm(v)

    psi = vector(1)
    probes = [vector(10 + j) for j in range(8)]
    wa, wb = ch.spectral_window(sec)
    K = a.orders
    res = dict(model="C3", sector=[nup, ndw], elems=sec.Dim, local_elems=n, vector_bytes=16 * n, row_order=sec.row_perm is not None, window=[wa, wb],
               orders=K, warmup=a.warmup, reps=a.reps, target_ratio=1.25, drivers={}, step_kernel={})

    # ---- the product alone
    hv = torch.empty_like(psi)
    prod = _event_ms(lambda: sec.apply_device_slab(psi, hv), a.warmup, a.reps * 2)
    res["product"] = _stats(prod)
    p_ms = res["product"]["median_ms"]

    # ---- the drivers, per order
    coef = np.ones(K + 1, dtype=np.complex128) / (K + 1)
    out = torch.empty_like(psi)
    runs = [(f"moments_{M}_probes", M, (lambda M=M: sec.chebyshev_moments(psi, probes[:M], K + 1, wa, wb)), (lambda M=M: sec.chebyshev_moments(psi, probes[:M], 1, wa, wb)))
            for M in (0, 1, 4, 8)]
    runs.append(("apply", 0, lambda: sec.chebyshev_apply(psi, coef, wa, wb, out=out), lambda: sec.chebyshev_apply(psi, coef[:1], wa, wb, out=out)))
    for name, M, full, none in runs:
        t_full, t_none = _stats(_event_ms(full, a.warmup, a.reps)), _stats(_event_ms(none, a.warmup, a.reps))
        per = (t_full["median_ms"] - t_none["median_ms"]) / K
        res["drivers"][name] = dict(probes=M, run_ms=t_full, run_without_products_ms=t_none, per_order_ms=per, per_order_minus_product_ms=per - p_ms,
                                    per_order_over_product=per / p_ms)
        print(json.dumps({name: res["drivers"][name]}), flush=True)

    # ---- the step kernel alone, on the driver's grid, and the copies
    L = C.CDLL(str(ge.build_chebyshev_kernels_check()))
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.ckc_step.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(vp), dbl, dbl, dbl, dbl, vp, vp]
    L.ckc_grid_for.argtypes = [i64]
    grid = L.ckc_grid_for(n)                                     # the driver's own rule (grid_for of csrc/hxv_lanczos_kernels.hpp)
    res["grid"] = grid
    cur, prev = vector(2), vector(3)
    hv.copy_(vector(4))
    out.zero_()
    part = torch.zeros((grid + 1) * 19, dtype=torch.float64, device="cuda")
    sums = torch.zeros(20, dtype=torch.float64, device="cuda")
    plist = (C.c_void_p * 8)(*[p.data_ptr() for p in probes])
    big = 16 * n * 12
    src, dst = torch.zeros(big, dtype=torch.uint8, device="cuda"), torch.empty(big, dtype=torch.uint8, device="cuda")
    for with_sum in (False, True):
        for M in (0, 1, 4, 8):
            def step():
                # (small scalars: the vectors stay bounded over the repetitions)
                rc = L.ckc_step(grid, M, 0, n, hv.data_ptr(), cur.data_ptr(), prev.data_ptr(), out.data_ptr() if with_sum else None, plist if M else None,
                                0.5, 0.25, 0.125, 0.0625, part.data_ptr(), sums.data_ptr())
                assert rc == 0, rc
            k_ms = _stats(_clock_ms(step, a.warmup, a.reps))
            nvec = (4 if with_sum else 3) + M
            nb = 16 * n * nvec
            c_ms = _stats(_event_ms(lambda: dst[:nb].copy_(src[:nb]), a.warmup, a.reps))
            traffic = 16 * n * (nvec + (2 if with_sum else 1))
            key = f"M{M}_{'sum' if with_sum else 'nosum'}"
            res["step_kernel"][key] = dict(probes=M, running_sum=with_sum, kernel_ms=k_ms, copy_bytes=nb, copy_ms=c_ms, ratio_to_copy=k_ms["median_ms"] / c_ms["median_ms"],
                                           kernel_traffic_bytes=traffic, kernel_GBps=traffic / k_ms["median_ms"] / 1e6, copy_GBps=2 * nb / c_ms["median_ms"] / 1e6)
            print(json.dumps({key: res["step_kernel"][key]}), flush=True)

    # ---- the REAL-vector path of the same build: the product alone, the drivers per order, the step kernel alone, the random vector
    res["real"] = real = dict(available=bool(sec.real_vectors_available), drivers={}, step_kernel={})
    if real["available"]:
        def real_vector(seed):
            v = vector(seed)
            v.imag.zero_()
            return v / torch.linalg.vector_norm(v)

        rpsi = real_vector(1)
        rprobes = [real_vector(10 + j) for j in range(8)]
        nr = hxv.load_library().hxv_realvec_elems(sec._h)       # DimDw * pitch_real doubles
        rv, rhv = torch.zeros(nr, dtype=torch.float64, device="cuda"), torch.zeros(nr, dtype=torch.float64, device="cuda")
        rv.normal_(generator=torch.Generator(device="cuda").manual_seed(5))
        pr = nr // sec.DimDw
        rv.view(sec.DimDw, pr)[:, sec.DimUp:] = 0
        real["vector_bytes"] = 8 * nr
        real["product"] = _stats(_event_ms(lambda: sec.apply_device_real(rv, rhv), a.warmup, a.reps * 2))
        rp_ms = real["product"]["median_ms"]
        rcoef = np.ones(K + 1) / (K + 1)
        runs = [(f"moments_{M}_probes", M, (lambda M=M: sec.chebyshev_moments_real(rpsi, rprobes[:M], K + 1, wa, wb)),
                 (lambda M=M: sec.chebyshev_moments_real(rpsi, rprobes[:M], 1, wa, wb))) for M in (0, 1, 4, 8)]
        runs.append(("apply", 0, lambda: sec.chebyshev_apply_real(rpsi, rcoef, wa, wb, out=out), lambda: sec.chebyshev_apply_real(rpsi, rcoef[:1], wa, wb, out=out)))
        for name, M, full, none in runs:
            t_full, t_none = _stats(_event_ms(full, a.warmup, a.reps)), _stats(_event_ms(none, a.warmup, a.reps))
            per = (t_full["median_ms"] - t_none["median_ms"]) / K
            cper = res["drivers"][name]["per_order_ms"]
            real["drivers"][name] = dict(probes=M, run_ms=t_full, run_without_products_ms=t_none, per_order_ms=per, per_order_minus_product_ms=per - rp_ms,
                                         per_order_over_product=per / rp_ms, complex_per_order_ms=cper, complex_over_real=cper / per)
            print(json.dumps({"real " + name: real["drivers"][name]}), flush=True)
        # the real step kernel on the driver's grid for n2 = nr / 2 double2 elements; the buffers are the front halves of the complex ones
        LR = C.CDLL(str(ge.build_chebyshev_real_kernels_check()))
        LR.crk_step.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(vp), dbl, dbl, dbl, vp, vp]
        n2 = nr // 2
        rgrid = L.ckc_grid_for(n2)
        real["grid"] = rgrid
        for with_sum in (False, True):
            for M in (0, 1, 4, 8):
                def rstep():
                    rc = LR.crk_step(rgrid, M, 0, n2, hv.data_ptr(), cur.data_ptr(), prev.data_ptr(), out.data_ptr() if with_sum else None, plist if M else None,
                                     0.5, 0.25, 0.125, part.data_ptr(), sums.data_ptr())
                    assert rc == 0, rc
                k_ms = _stats(_clock_ms(rstep, a.warmup, a.reps))
                nvec = (4 if with_sum else 3) + M
                nb = 8 * nr * nvec
                c_ms = _stats(_event_ms(lambda: dst[:nb].copy_(src[:nb]), a.warmup, a.reps))
                traffic = 8 * nr * (nvec + (2 if with_sum else 1))
                key = f"M{M}_{'sum' if with_sum else 'nosum'}"
                kg, cg = traffic / k_ms["median_ms"] / 1e6, 2 * nb / c_ms["median_ms"] / 1e6
                real["step_kernel"][key] = dict(probes=M, running_sum=with_sum, kernel_ms=k_ms, copy_bytes=nb, copy_ms=c_ms, ratio_to_copy=k_ms["median_ms"] / c_ms["median_ms"],
                                                kernel_traffic_bytes=traffic, kernel_GBps=kg, copy_GBps=cg, time_per_byte_over_copy=cg / kg,
                                                complex_kernel_ms=res["step_kernel"][key]["kernel_ms"]["median_ms"])
                print(json.dumps({"real " + key: real["step_kernel"][key]}), flush=True)

    # ---- the seeded random vector: one streaming pass (16 B written per state) against a device-to-device copy of the vector (16 B read and
    #      16 B written per state) and against numpy-free vector_from_host of a host array that already exists
    rnd = torch.empty_like(psi)
    host = np.zeros(sec.vecDim, dtype=np.complex128)
    res["random_vector"] = dict(
        real_ms=_stats(_event_ms(lambda: sec.random_vector(1, False, out=rnd), a.warmup, a.reps)),
        complex_ms=_stats(_event_ms(lambda: sec.random_vector(1, True, out=rnd), a.warmup, a.reps)),
        copy_ms=_stats(_event_ms(lambda: rnd.copy_(psi), a.warmup, a.reps)),
        vector_from_host_ms=_stats(_clock_ms(lambda: sec.vector_from_host(host), 1, max(a.reps // 2, 2))), bytes_written=16 * n)
    print(json.dumps({"random_vector": res["random_vector"]}), flush=True)
    sec.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
