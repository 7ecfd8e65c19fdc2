"""bench.py's one-line JSON contract, checked on the line committed under profiles/ and, on a GPU, on the lines of a plain and a --full run."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_committed_bench_line_has_the_contract_fields():
    """The newest line under profiles/ is a --full line: the headline fields and the legs beside it."""
    files = sorted((ROOT / "profiles").glob("r*_bench_n1_v*.json"), key=lambda p: tuple(int(x) for x in re.search(r"r(\d+)_bench_n1_v(\d+)", p.name).groups()))
    line = json.loads(files[-1].read_text().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["unit"] == "GB/s" and line["n_gpus"] == 1 and line["higher_is_better"] is True and line["vs_baseline"] is None
    assert "workload" in line["config"] and "model" not in line["config"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or r["traffic"] > r["algorithmic_bytes"]
    c = line["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["unit"] == "GB/s" and "sample" in c
    # value = 32 B x Dim / step time
    dim = int(re.search(r"Dim=(\d+)", line["config"]["workload"]).group(1))
    assert abs(line["value"] - 32.0 * dim / (line["ms_per_step"] * 1e-3) / 1e9) < 0.5


def test_bench_defaults_follow_the_measurement_spec():
    src = (ROOT / "bench.py").read_text()
    assert '"--steps", type=int, default=100' in src and '"--warmup", type=int, default=20' in src      # >=20 warm-up, >=100 timed
    assert '"--gpus", type=int, default=1' in src


class _Layout:
    """The layout part of an open sector (pitch, device row order) with HxvSector's own pad / unpad: enough for bench.py's input and dump."""

    def __init__(self, DimUp, ncols, pitch, row_order):
        import numpy as np
        from hxv.engine import HxvSector

        self.pad, self.unpad, self._row_tables = (f.__get__(self) for f in (HxvSector.pad, HxvSector.unpad, HxvSector._row_tables))
        self.DimUp, self.pitch, self.localElems, self._row_dev = DimUp, pitch, ncols * pitch, {}
        self.row_perm = self.row_sign = None
        if row_order:
            rng = np.random.default_rng(3)
            self.row_perm, self.row_sign = rng.permutation(DimUp).astype(np.int32), rng.choice([-1, 1], DimUp).astype(np.int8)


def test_bench_input_and_dump_do_not_depend_on_the_device_layout(tmp_path, monkeypatch):
    """--dump-outputs compares two builds output for output: the input vector is the same in the reference's order whatever pitch and row
    order a build gives the sector (pad rows zero), and the dump is the caller's view of Hv (reference order; pad rows never read), whole
    or at the same seeded positions."""
    import numpy as np
    import torch
    import bench

    DimUp, q = 3000, 50
    a, b = _Layout(DimUp, q, DimUp, False), _Layout(DimUp, q, 3008, True)
    va, vb = bench.seeded_slab(a, 1234, "cpu"), bench.seeded_slab(b, 1234, "cpu")
    assert torch.equal(a.unpad(va), b.unpad(vb)) and torch.all(vb.view(q, b.pitch)[:, DimUp:] == 0)
    f = lambda x: x * (2 - 1j) + 0.5                 # (an operator that is elementwise in the reference's order)
    ha, hb = a.pad(f(a.unpad(va))), b.pad(f(b.unpad(vb)))
    hb.view(q, b.pitch)[:, DimUp:] = float("nan")
    ref = f(a.unpad(va)).numpy()
    for sample in (1 << 21, 4096):
        monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
        got = []
        for name, s, h in (("a", a, ha), ("b", b, hb)):
            bench.dump_outputs(s, h, str(tmp_path / f"{name}{sample}"), 0, 1)
            x = np.load(tmp_path / f"{name}{sample}" / "hv.npy")
            assert x.dtype == np.float64 and x.shape == (min(sample, q * DimUp), 2) and np.isfinite(x).all()
            got.append(x)
        assert np.array_equal(got[0], got[1])
        z = got[0][:, 0] + 1j * got[0][:, 1]
        assert np.all(np.isin(z, ref)) and (sample < q * DimUp or np.array_equal(z, ref))
    bench.dump_outputs(b, hb, str(tmp_path / "ranks"), 1, 2)      # several ranks share the budget, one file each
    assert np.load(tmp_path / "ranks" / "hv_rank1.npy").shape == (2048, 2)


@pytest.mark.gpu
def test_bench_dump_is_the_product_of_the_timed_steps(built, tmp_path):
    """`bench.py --steps K --dump-outputs DIR` at C2 (small enough to dump whole): K timed steps, and DIR/hv.npy = H v of the bench's
    seeded input in the reference's order, against the CPU oracle's product."""
    import numpy as np
    import torch
    import bench
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "C2", "--steps", "7", "--warmup", "1", "--no-cpu-baseline",
                        "--no-lanczos", "--no-other-workloads", "--no-gf-solve", "--no-apply-host", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    m = models.hm_1dchain()
    sec = hxv.HxvSector.from_model(m, 6, 6)
    v = sec.unpad(bench.seeded_slab(sec, 1234, torch.device("cuda", 0))).cpu().numpy()
    sec.close()
    ref = OracleSector(m, 6, 6).spMatVec_main(v)
    hv = np.load(tmp_path / "out" / "hv.npy")
    assert hv.dtype == np.float64 and hv.shape == (len(ref), 2)
    assert np.abs(hv[:, 0] + 1j * hv[:, 1] - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.gpu
def test_bench_plain_run_measures_the_headline_only_and_full_adds_the_legs(built):
    """A plain run sets up, warms up, times the steps and prints the headline line; roofline, CPU baseline, Lanczos, host-array and
    exchange-volume legs come with --full only (C2 has no solve-shaped or C4 / C5 leg), and both lines state the headline alike."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def run(*extra):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "C2", "--steps", "5", "--warmup", "2", *extra],
                           capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    plain, full = run(), run("--full")
    assert set(plain) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                          "dtype", "data", "config"}
    assert set(plain["config"]) == {"workload", "DimUp", "DimDw", "device_row_order", "parallelism", "matvecs_per_s"}
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "dtype", "data"):
        assert plain[k] == full[k], k
    dim = int(re.search(r"Dim=(\d+)", plain["config"]["workload"]).group(1))
    for line in (plain, full):      # (ms_per_step is rounded to 1e-4 ms: about 0.2 % of a C2 step)
        assert line["ms_per_step"] > 0 and abs(line["value"] / (32.0 * dim / (line["ms_per_step"] * 1e-3) / 1e9) - 1) < 5e-3
    assert full["roofline"]["kernel_ms"] > 0 and "lanczos" in full["roofline"] and full["cpu_baseline"]["cores"] >= 1
    for k in ("exchange_ingest_bytes_per_gpu_at_8_ranks", "apply_host", "lanczos_ms_per_iter", "lanczos_paired_real_ms_per_iter"):
        assert k in full["config"], k
    assert "failed" not in full["config"]["apply_host"]
