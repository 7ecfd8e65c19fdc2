"""Cost of the paired probe runs (include/hxv.h, hxv_lanczos_tridiag_pair_probes) at C3, sector (9,8), start vectors and probes c^dagger_j|gs>
from the real ground state of (8,8).

  python scripts/pair_probes_bench.py [--steps 10:60] [--probes 1,3,4,8] [--reps 4]

One process; every call is synchronous, and is timed between two HIP events recorded around it.  A per-step time is the difference of two
runs of different length (--steps a:b, the minimum of --reps repetitions each, after one warm-up run) divided by b - a, so that what a run
pays once (the check, the probes' conversion, the start vectors' norms) drops out; "spread" is the largest (max - min) / min among the
repetitions, the noise of each figure.  Per probe count M:
  pair_probes_ms_channel_step   (a) the new call: ms per step / 2
  probes_ms_step                (b) hxv_lanczos_tridiag_probes on its default real path, same M, same process
  pair_ms_channel_step          (c) hxv_lanczos_tridiag_pair without probes: ms per step / 2
  copy_GBps                     (d) a device-to-device copy of one vector of the sector, read + written bytes over time
  overlap_ms_step               2 * ((a) - (c)): the overlap pass of one paired step
  stream_ms                     (16 + 8 M) B per state at (d)
  overlap_over_stream           the ratio; the target is <= 1.25 (LABNOTES "Probe overlaps")
  a_below_b                     (a) < (b)
and per_solve: the steps' cost of the probe runs of a 2x2 solve, 4 paired runs against 8 single ones with 4 probes, per Lanczos step.
Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd"), str(ROOT / "scripts")]


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _per_step(run, n_a, n_b, reps):
    run(n_a)                                   # warm-up: lazy allocations of the handle
    t_a = [_timed(lambda: run(n_a)) for _ in range(reps)]
    t_b = [_timed(lambda: run(n_b)) for _ in range(reps)]
    spread = max((max(t) - min(t)) / min(t) for t in (t_a, t_b))
    return (min(t_b) - min(t_a)) / (n_b - n_a), spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="10:60")
    ap.add_argument("--probes", default="1,3,4,8")
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    n_a, n_b = (int(x) for x in a.steps.split(":"))
    counts = [int(x) for x in a.probes.split(",")]

    import torch
    import hxv
    from hxv import models

    m, (nup, ndw) = models.hm_2dsquare(Nbath=3), (8, 8)
    nimp = m.Nlat * m.Norb
    gs = hxv.HxvSector.from_model(m, nup, ndw)
    e0, psi, nit = gs.lanczos_eigh(512, 1e-10, native=True)
    sec = hxv.HxvSector.from_model(m, nup + 1, ndw)
    vecs = [gs.apply_ladder(sec, i, 0, True, psi)[0] for i in range(nimp)]
    gs.close()
    del psi
    hxv.pool_trim()
    torch.cuda.empty_cache()
    probes = list(vecs)
    while len(probes) < max(counts):           # (more probes than orbitals: copies in buffers of their own stream like any other vector)
        probes.append(vecs[len(probes) % nimp].clone())
    res = {"workload": "C3", "sector": [nup + 1, ndw], "Dim": sec.Dim, "steps": [n_a, n_b], "reps": a.reps, "spread": {},
           "pair_probes_ms_channel_step": {}, "probes_ms_step": {}, "overlap_ms_step": {}, "stream_ms": {}, "overlap_over_stream": {},
           "a_below_b": {}}
    t, res["spread"]["pair"] = _per_step(lambda n: sec.lanczos_tridiag_pair(vecs[0], vecs[1], n), n_a, n_b, a.reps)
    res["pair_ms_channel_step"] = t / 2
    assert sec.get_option("lanczos_real_last") == 2
    for M in counts:
        t, res["spread"][f"pair_probes{M}"] = _per_step(lambda n: sec.lanczos_tridiag_pair_probes(vecs[0], vecs[1], probes[:M], n), n_a, n_b, a.reps)
        assert sec.get_option("lanczos_real_last") == 2
        res["pair_probes_ms_channel_step"][str(M)] = t / 2
        res["probes_ms_step"][str(M)], res["spread"][f"probes{M}"] = _per_step(lambda n: sec.lanczos_tridiag_probes(vecs[0], probes[:M], n), n_a, n_b, a.reps)
        assert sec.get_option("lanczos_real_last") == 1
    src, dst = vecs[0], torch.empty_like(vecs[0])

    def copy():
        dst.copy_(src)

    copy()
    copy_ms = min(_timed(copy) for _ in range(10))
    rate = 32 * src.numel() / copy_ms / 1e6                   # GB/s, read + written bytes
    res["copy_GBps"] = rate
    for M in counts:
        k = str(M)
        ov = 2 * (res["pair_probes_ms_channel_step"][k] - res["pair_ms_channel_step"])
        stream = (16 + 8 * M) * sec.Dim / rate / 1e6
        res["overlap_ms_step"][k], res["stream_ms"][k], res["overlap_over_stream"][k] = ov, stream, ov / stream
        res["overlap_GBps"] = res.get("overlap_GBps", {})
        res["overlap_GBps"][k] = (16 + 8 * M) * sec.Dim / ov / 1e6
        res["a_below_b"][k] = res["pair_probes_ms_channel_step"][k] < res["probes_ms_step"][k]
    if "4" in res["probes_ms_step"]:
        res["per_solve"] = {"paired_runs4_ms_per_step": 4 * 2 * res["pair_probes_ms_channel_step"]["4"], "single_runs8_ms_per_step": 8 * res["probes_ms_step"]["4"]}
    sec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
