"""Cost of the probe overlaps (include/hxv.h, hxv_lanczos_tridiag_probes) at C3, sector (9,8) from the real ground state of (8,8), and at C4
(complex H), and of the whole 2x2 Green's-function stage both ways.

  python scripts/probes_bench.py [--workloads C3,C4] [--steps 10:60] [--probes 0,1,3,7] [--no-stage] [--nlanc 200]

Per workload, one process, wall clock around the synchronous calls; a per-step time is the difference of two runs of different length
(--steps a:b, the minimum of 4 repetitions each) divided by b - a, so that what a run pays once (real-vector check, probe conversion,
start-vector norm) drops out; "spread" is the largest (max - min) / min among the repetitions, the noise of each figure:
  tridiag_ms_step       hxv_lanczos_tridiag with lanczos_graph = 0 and = 1
  probes_ms_step        the probes driver with 0 / 1 / 3 / 7 probes
  copy_GBps             a device-to-device copy of one vector of the sector in the same process, read + written bytes over time
                        (the rate scripts/twin_bench.py reports)
  extra_ms_step         probes_ms_step[n] - probes_ms_step[0]
  stream_ms             (1 + n) x 8 B (real run) or 16 B (complex run) per state at copy_GBps: what reading the Lanczos vector and n probes once costs
  extra_over_stream     the ratio; the target is <= 1.25
--stage (default, C3 only): the Green's-function stage of the 2x2 cluster for spin up from one ground state -- scripts/harness.py's 56
channels, the 20 of ed_gf_symmetric, and 8 probe runs (4 orbitals x c^dagger / c, the 3 other orbitals as probes), each with nlanc steps.
Prints one JSON line per workload and one for the stage."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "scripts")]


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


REPS = 4


def _per_step(run, n_a, n_b):
    """-> (ms per step from the minima of REPS runs of each length, the largest relative spread of the repetitions: the noise of the figure)"""
    run(n_a)                                   # warm-up: lazy allocations of the handle
    t_a = [_timed(lambda: run(n_a)) for _ in range(REPS)]
    t_b = [_timed(lambda: run(n_b)) for _ in range(REPS)]
    spread = max((max(t) - min(t)) / min(t) for t in (t_a, t_b))
    return (min(t_b) - min(t_a)) / (n_b - n_a), spread


def workload(name, steps, probe_counts):
    import torch
    import hxv
    from hxv import models

    m, (nup, ndw) = {"C3": (models.hm_2dsquare(Nbath=3), (8, 8)), "C4": (models.bhz_2d(Nbath=1), (8, 8))}[name]
    nimp = m.Nlat * m.Norb
    gs = hxv.HxvSector.from_model(m, nup, ndw)
    e0, psi, nit = gs.lanczos_eigh(512, 1e-10, native=True)
    sec = hxv.HxvSector.from_model(m, nup + 1, ndw)
    vecs = [gs.apply_ladder(sec, i, 0, True, psi)[0] for i in range(min(nimp, 1 + max(probe_counts)))]
    while len(vecs) < 1 + max(probe_counts):   # (more probes than orbitals: copies in buffers of their own stream like any other vector)
        vecs.append(vecs[len(vecs) % nimp].clone())
    gs.close()
    del psi
    hxv.pool_trim()
    torch.cuda.empty_cache()
    n_a, n_b = steps
    res = {"workload": name, "sector": [nup + 1, ndw], "Dim": sec.Dim, "steps": [n_a, n_b], "tridiag_ms_step": {}, "probes_ms_step": {}, "spread": {},
           "extra_ms_step": {}, "stream_ms": {}, "extra_over_stream": {}}
    for g in (0, 1):
        sec.set_option("lanczos_graph", g)
        res["tridiag_ms_step"][f"graph{g}"], res["spread"][f"graph{g}"] = _per_step(lambda n: sec.lanczos_tridiag(vecs[0], n), n_a, n_b)
    real = bool(sec.get_option("lanczos_real_last"))
    res["real_vectors"] = real
    for npr in probe_counts:
        res["probes_ms_step"][str(npr)], res["spread"][f"probes{npr}"] = _per_step(lambda n: sec.lanczos_tridiag_probes(vecs[0], vecs[1:1 + npr], n), n_a, n_b)
        assert bool(sec.get_option("lanczos_real_last")) == real
    src, dst = vecs[0], torch.empty_like(vecs[0])

    def copy():
        dst.copy_(src)

    copy()
    copy_ms = min(_timed(copy) for _ in range(10))
    rate = 32 * src.numel() / copy_ms / 1e6                   # GB/s, read + written bytes
    res["copy_GBps"] = rate
    per_state = 8 if real else 16
    n_state = sec.Dim
    for npr in probe_counts:
        if npr == 0:
            continue
        extra = res["probes_ms_step"][str(npr)] - res["probes_ms_step"]["0"]
        stream = (1 + npr) * per_state * n_state / rate / 1e6
        res["extra_ms_step"][str(npr)], res["stream_ms"][str(npr)], res["extra_over_stream"][str(npr)] = extra, stream, extra / stream
    sec.close()
    del vecs, src, dst
    hxv.pool_trim()
    torch.cuda.empty_cache()
    return res


def stage(nlanc):
    """the 2x2 Green's-function stage at C3 for spin up, three ways, on the same ground-state sector (8,8)"""
    import torch
    import harness
    import hxv
    from hxv import greens, models

    m = models.hm_2dsquare(Nbath=3)
    out = {"stage": "C3 2x2, spin up", "nlanc": nlanc}
    for key, sym in (("channels56_s", False), ("channels20_symmetric_s", True)):
        recs, summ = harness.gf_solve(m, 8, 8, nlanc=nlanc, symmetric=sym, gs_method="lanczos")
        out[key] = summ["real_channels_s"] + summ["complex_channels_s"]
        out[key.replace("_s", "_count")] = summ["channels"]
        out[key.replace("_s", "_whole_solve_s")] = summ["gf_solve_s"]
        hxv.pool_trim()
        torch.cuda.empty_cache()
    gs = hxv.HxvSector.from_model(m, 8, 8)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-13, native=True)
    nimp = m.Nlat * m.Norb
    t_runs = 0.0
    t_all = time.perf_counter()
    for create in (True, False):
        sec = hxv.HxvSector.from_model(m, 9 if create else 7, 8)
        vecs, n2s = zip(*[gs.apply_ladder(sec, i, 0, create, psi) for i in range(nimp)])
        for i in range(nimp):
            probes = [vecs[j] for j in range(nimp) if j != i]
            t0 = time.perf_counter()
            a, b, ov, n = sec.lanczos_tridiag_probes(vecs[i], probes, min(sec.Dim, nlanc))
            torch.cuda.synchronize()
            t_runs += time.perf_counter() - t0
            greens.poles_weights(a[:n], b[:n], ov, n2s[i] ** 0.5)
        sec.close()
        del vecs
    gs.close()
    out["probe_runs8_s"] = t_runs
    out["probe_stage_whole_s"] = time.perf_counter() - t_all
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,C4")
    ap.add_argument("--steps", default="10:60")
    ap.add_argument("--probes", default="0,1,3,7")
    ap.add_argument("--nlanc", type=int, default=200)
    ap.add_argument("--no-stage", action="store_true")
    a = ap.parse_args()
    steps = tuple(int(x) for x in a.steps.split(":"))
    counts = [int(x) for x in a.probes.split(",")]
    assert counts[0] == 0, "the first probe count must be 0: the extra cost is measured against it"
    for w in [x for x in a.workloads.split(",") if x]:
        print(json.dumps(workload(w, steps, counts)), flush=True)
    if not a.no_stage:
        print(json.dumps(stage(a.nlanc)), flush=True)


if __name__ == "__main__":
    main()
