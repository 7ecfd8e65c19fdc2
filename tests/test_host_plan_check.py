"""The tile-plan tables on the CPU (tests/host/plan_check.cpp; DESIGN.md section 3, "plan checker").

Every table make_tile_plan hands to the kernels is read back the way the kernels read it -- per block, thread and slot, through one
bounds-checked accessor -- expanded into (row, source, coefficient) triplets and compared, exactly and as multisets per row, with the
one-spin CSR of the sector; the device row order and the invariants the kernels assume are checked beside it.  This file drives that
program: against the oracle's matrices (an independent implementation), over the named shapes of the option sweep with every plan option
value, over a seeded random sweep, and once under the host sanitizers (ASan + UBSan, TSan), always as a stand-alone program.

Each run prints, per shape, the triplets compared and the table words read (pytest -s shows them)."""
import math
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from random_models import random_model
from test_gpu_options import COMBINED, OPTIONS, PLAN_STATS, _shape_model

TOL = 2e-13          # the project's H x V tolerance (values against the oracle)
# nnz(H_up) of C3 (8,8): 14.93 stored elements per row of 12870 (tests/golden/survey_known_answers.json, "nnz_up")
C3_NNZ_UP = 192192
DOCUMENTED = ("block larger", "does not fit", "must be")
PLAN_OPTIONS = [n for n, (grp, _, _) in OPTIONS.items() if grp == 2]


# ---- driving the checker --------------------------------------------------------------------------------------------------------------
def write_model(path, model):
    """the fields of hxv_model in the array order of HxvSector._model_struct"""
    from hxv.engine import HxvSector

    m, (h, hb, vb) = HxvSector._model_struct(model)
    if model.Nbath == 0:
        hb, vb = hb[:0], vb[:0]
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", m.nlat, m.norb, m.nspin, m.nbath, m.hfmode, 0))
        f.write(struct.pack("<10d", *list(m.uloc), m.ust, m.jh, m.jx, m.jp, m.xmu))
        f.write(struct.pack("<3q", h.size, hb.size, vb.size))
        for a in (h, hb, vb):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return path


def run_checker(exe, model_path, sector, shard=(0, 1), exchange=0, panel=0, dump=None, sets=({},), env=None):
    """-> (exit status, {set index: ("PLAN", {name: int}) | ("REFUSED", message)}, stderr, seconds)"""
    cmd = [str(exe), str(model_path), str(sector[0]), str(sector[1]), str(shard[0]), str(shard[1]), str(exchange)]
    if panel:
        cmd += ["--panel", str(panel)]
    if dump:
        cmd += ["--dump", str(dump)]
    for k, opts in enumerate(sets):
        cmd += (["/"] if k else []) + [f"{n}={v}" for n, v in opts.items()]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    out = {}
    for line in p.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        fields = rest.split(" ")
        k = int(fields[0].split("=")[1])
        if kind == "PLAN":
            out[k] = ("PLAN", {a: int(b) for a, b in (f.split("=") for f in fields[2:])})
        else:
            out[k] = ("REFUSED", rest)
    return p.returncode, out, p.stderr, time.perf_counter() - t0


def _assert_passed(rc, out, err, nsets, what, may_refuse=True):
    assert rc in ((0, 2) if may_refuse else (0,)), (what, rc, err[-2000:])
    assert len(out) == nsets, (what, rc, err[-2000:])
    for k, (kind, val) in out.items():
        if kind == "REFUSED":
            assert may_refuse and any(d in val for d in DOCUMENTED), (what, k, val)
    assert "FAIL" not in err and "OUT OF RANGE" not in err, (what, err[-2000:])


@pytest.fixture(scope="session")
def checker(built):
    return built.build_plan_check()


def test_checker_is_built_from_host_sources_only(built):
    """The checker's source list names C++ files only, the plan builder among them, and the plan builder holds no device code: neither
    __global__ nor __device__ appears in hxv_tile_plan.cpp."""
    names = [s.name for s in built.PLAN_CHECK_SOURCES]
    assert names and all(n.endswith(".cpp") for n in names), names
    plan = [s for s in built.PLAN_CHECK_SOURCES if s.name == "hxv_tile_plan.cpp"]
    assert len(plan) == 1, names
    text = plan[0].read_text()
    assert "__global__" not in text and "__device__" not in text


# ---- the named shapes --------------------------------------------------------------------------------------------------------------------
def _full_size(key):
    from hxv import models

    return {"C3": (models.hm_2dsquare(Nbath=3), 16), "C4": (models.bhz_2d(Nbath=1, Ust=0.5, Jh=0.1), 16),
            "C4_kanamori": (models.bhz_2d(Nbath=1, Ust=0.5, Jh=0.1, Jx=0.1, Jp=0.1), 16), "C5": (models.hm_ring(6, 2), 18)}[key]


def _named_shapes():
    """name -> dict(model, sector, shard, exchange, panel, base options)"""
    shapes = {}
    for key in ("S1", "S2", "S3", "S4", "S1r", "S2r"):
        m, sector, bits = _shape_model(key)
        shapes[key] = dict(model=m, sector=sector, shard=(1, 3) if key.endswith("r") else (0, 1), base={"tile_bits_up": bits, "tile_bits_dw": bits})
    m, sector, bits = _shape_model("S2")
    shapes["S2_up6"] = dict(model=m, sector=sector, shard=(0, 1), base={"tile_bits_up": 6, "tile_bits_dw": bits})
    for key, sector in (("C3", (8, 8)), ("C3", (7, 9)), ("C4", (8, 8)), ("C4_kanamori", (8, 8)), ("C5", (9, 9))):
        shapes[f"{key}_{sector[0]}_{sector[1]}"] = dict(model=_full_size(key)[0], sector=sector, shard=(0, 1), base={})
    for ex in (0, 1, 2):
        shapes[f"C3_rank3of8_x{ex}"] = dict(model=_full_size("C3")[0], sector=(8, 8), shard=(3, 8), exchange=ex, base={})
    shapes["C3_panel16"] = dict(model=_full_size("C3")[0], sector=(8, 8), shard=(0, 1), panel=16, base={})
    return shapes


SHAPE_NAMES = ["S1", "S2", "S3", "S4", "S1r", "S2r", "S2_up6", "C3_8_8", "C3_7_9", "C4_8_8", "C4_kanamori_8_8", "C5_9_9", "C3_rank3of8_x0",
               "C3_rank3of8_x1", "C3_rank3of8_x2", "C3_panel16"]
_MODEL_FILES = {}


def _model_file(tmp_path_factory, name, model):
    if name not in _MODEL_FILES:
        _MODEL_FILES[name] = write_model(tmp_path_factory.mktemp("plan_models") / (name + ".model"), model)
    return _MODEL_FILES[name]


def _run_shape(exe, tmp_path_factory, name, sets, **kw):
    sh = _named_shapes()[name]
    path = _model_file(tmp_path_factory, name, sh["model"])
    sets = [dict(sh["base"], **s) for s in sets]
    return run_checker(exe, path, sh["sector"], sh["shard"], sh.get("exchange", 0), sh.get("panel", 0), sets=sets, **kw)


def _report(name, out, seconds):
    plans = [v for kind, v in out.values() if kind == "PLAN"]
    if plans:
        p = plans[0]
        print(f"{name}: {len(plans)} plans, {len(out) - len(plans)} refused, {seconds:.1f} s; default-option set: triplets up {p.get('triplets_up')} "
              f"dw {p.get('triplets_dw')}, table words read {p.get('words_read')}, blocks {p.get('nblocks_up')} x {p.get('nblocks_dw')}, "
              f"row order {p.get('row_order')}, job registers checked {p.get('job_checked')}")


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------------
ORACLE_CASES = {"chain": ("chain", None, 1), "C3_8_8": ("C3", (8, 8), 64), "C3_7_9": ("C3", (7, 9), 64), "C4_8_8": ("C4", (8, 8), 64),
                "C4_kanamori_8_8": ("C4_kanamori", (8, 8), 64), "C5_9_9": ("C5", (9, 9), 512)}   # model, sector (None: every sector), oracle ranks


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_sector_matrices_equal_the_oracle(checker, tmp_path_factory, tmp_path, case):
    """The CSR the exact table check compares with (--dump: both spins in the reference's order, and the basis maps) against
    OracleSector.csr / map_up / map_dw: rowptr, columns and maps exactly, values within 2e-13 * max|value|.  The oracle is opened with a
    large rank count, so it allocates no Dim-sized array; every sector of hm_1dchain(Nlat=2, Nbath=2), and the five full-size sectors."""
    from hxv import models
    from oracle.oracle import OracleSector

    name, sector, size = ORACLE_CASES[case]
    m = models.hm_1dchain(Nlat=2, Nbath=2) if name == "chain" else _full_size(name)[0]
    sectors = [sector] if sector else [(nup, ndw) for nup in range(m.Ns + 1) for ndw in range(m.Ns + 1)]
    for k, sector in enumerate(sectors):
        path = _model_file(tmp_path_factory, name, m)
        d = tmp_path / f"dump{k}"
        d.mkdir()
        rc, out, err, sec = run_checker(checker, path, sector, dump=d)
        _assert_passed(rc, out, err, 1, (case, sector), may_refuse=False)
        orc = OracleSector(m, *sector, 0, min(size, math.comb(m.Ns, sector[1])))
        nnz = {}
        for which in ("up", "dw"):
            rp, cols, vals = orc.csr(which)
            nnz[which] = int(rp[-1])
            assert np.array_equal(np.fromfile(d / f"{which}_rowptr.i64", dtype=np.int64), rp), (case, sector, which)
            assert np.array_equal(np.fromfile(d / f"{which}_cols.i32", dtype=np.int32) + 1, cols), (case, sector, which)   # (the oracle's are 1-based)
            got = np.fromfile(d / f"{which}_vals.c128", dtype=np.complex128)
            assert got.shape == vals.shape
            if vals.size:
                assert np.abs(got - vals).max() <= TOL * np.abs(vals).max(), (case, sector, which)
        assert np.array_equal(np.fromfile(d / "map_up.u32", dtype=np.uint32).astype(np.int64), np.asarray(orc.map_up(), dtype=np.int64))
        assert np.array_equal(np.fromfile(d / "map_dw.u32", dtype=np.uint32).astype(np.int64), np.asarray(orc.map_dw(), dtype=np.int64))
        orc.close()
        # every stored element of the oracle's matrices was met once in the tables
        assert (out[0][1]["triplets_up"], out[0][1]["triplets_dw"]) == (nnz["up"], nnz["dw"]), (case, sector)
        if case != "chain":
            _report(case, out, sec)
            if case == "C3_8_8":
                assert nnz["up"] == C3_NNZ_UP


# ---- 2. the named shapes x every plan option value --------------------------------------------------------------------------------------
def _option_sets():
    """the default set first, then each plan option at each value OPTIONS lists, one at a time, then COMBINED"""
    return [{}] + [{n: v} for n in PLAN_OPTIONS for v in OPTIONS[n][2]] + [dict(COMBINED)]


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_every_plan_option_value(checker, tmp_path_factory, name):
    """S1-S4, S1r, S2r of tests/test_gpu_options.py at their forced block bits (S2 also with 6 up bits, where pass A can run as jobs),
    the four full-size sectors, C3 as rank 3 of 8 in all three exchanges and a 16-row dw panel: each plan option of OPTIONS at each
    listed value, one at a time, and COMBINED (nothing is thinned: Ns = 18 takes the whole list too).  The default set must be accepted;
    another set may be refused with a documented message."""
    sets = _option_sets()
    rc, out, err, sec = _run_shape(checker, tmp_path_factory, name, sets)
    _assert_passed(rc, out, err, len(sets), name)
    assert out[0][0] == "PLAN" and out[0][1]["usable"] == 1, (name, out[0])
    if name == "S2_up6":
        assert out[0][1]["job_checked"] == 1, name      # (the job kernel's packed registers were expanded too)
    if name.startswith("C3") and "panel" not in name:
        assert out[0][1]["row_order"] == 1 and out[0][1]["job_checked"] == 1, (name, out[0])
    if name == "C3_8_8":
        assert out[0][1]["triplets_up"] == C3_NNZ_UP, out[0]
    _report(name, out, sec)


# ---- 2b. sectors with a one-spin dimension above 65535 (tests/wide_sectors.py; the GPU runs them in tests/test_gpu_wide_sectors.py) -----
def _wide_shapes():
    """name -> dict(sector = a name of wide_sectors.SECTORS or (model key, nup, ndw), shard, exchange, sets, and what the default-option plan
    must look like: at least `blocks` (up, dw) blocks, at least `outer` (up, dw) out-of-block partners, the row order on or off).  The P
    sectors take the option sets the GPU file runs on them; the plan checker has no sanitizer run of these shapes."""
    p_opts = [{o: v} for o, vals in (("cols_per_tile", (2, 8)), ("rows_per_tile", (2, 8)), ("block_order", (0, 1, 2)), ("job_up", (1,))) for v in vals]
    bits6 = [{"tile_bits_up": 6, "tile_bits_dw": 6}]
    shapes = {
        "ns20_10_1": dict(sector="ns20_10_1", sets=[{}] + bits6 + p_opts, blocks=(256, 1), outer=(14, 0), row_order=1),
        "ns20_1_10": dict(sector="ns20_1_10", sets=[{}] + bits6 + p_opts, blocks=(1, 512), outer=(0, 16), row_order=0),
        "ns22_11_0": dict(sector=("chain22", 11, 0), sets=[{}], blocks=(1024, 1), outer=(15, 0), row_order=1),
        "ns22_0_11": dict(sector=("chain22", 0, 11), sets=[{}], blocks=(1, 1024), outer=(0, 15), row_order=0),
        "ns22_2_1": dict(sector="ns22_2_1", sets=[{}], blocks=(1, 1), outer=(0, 0), row_order=0),
        "ns24_6_1": dict(sector="ns24_6_1", sets=[{}] + p_opts, blocks=(2510, 1), outer=(32, 0), row_order=0),
        "ns24_1_6": dict(sector="ns24_1_6", sets=[{}] + p_opts, blocks=(1, 4096), outer=(0, 34), row_order=0),
    }
    for ex in (0, 1, 2):
        shapes[f"ns20_1_10_rank1of2_x{ex}"] = dict(sector="ns20_1_10", shard=(1, 2), exchange=ex, sets=[{}], blocks=(1, 256), outer=(0, 14), row_order=0)
    return shapes


WIDE_NAMES = ["ns22_2_1", "ns20_10_1", "ns20_1_10", "ns22_11_0", "ns22_0_11", "ns24_6_1", "ns24_1_6", "ns20_1_10_rank1of2_x0", "ns20_1_10_rank1of2_x1",
              "ns20_1_10_rank1of2_x2"]


def _wide_model(spec):
    import wide_sectors as WS

    if isinstance(spec, str):
        key, nup, ndw = WS.SECTORS[spec]
    else:
        key, nup, ndw = spec
    return key, WS.model(key), (nup, ndw)


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_wide_sector_plans_and_matrices(checker, tmp_path_factory, tmp_path, name):
    """The six sectors of Ns = 20 to 24 whose one-spin dimension is 134 596 to 705 432, Ns 22 (0,11) and the small Ns 22 (2,1) (Ns > 20: the
    sector builder searches the sorted basis instead of a 2^Ns table), default options; 64-row blocks (15 444 of them) and the option sets of
    the GPU file on the sectors with both passes; (1,10) as rank 1 of 2 in the three exchanges.  Every plan passes the table check, none
    is refused, and on the unsplit shapes the matrices the check compares with are the oracle's, every stored element met once."""
    from oracle.oracle import OracleSector

    sh = _wide_shapes()[name]
    key, m, sector = _wide_model(sh["sector"])
    path = _model_file(tmp_path_factory, "wide_" + key, m)
    shard, unsplit = sh.get("shard", (0, 1)), "shard" not in sh
    d = tmp_path / "dump"
    d.mkdir()
    rc, out, err, sec = run_checker(checker, path, sector, shard, sh.get("exchange", 0), dump=d if unsplit else None, sets=sh["sets"])
    _assert_passed(rc, out, err, len(sh["sets"]), name, may_refuse=False)
    p = out[0][1]
    assert p["usable"] == 1 and p["row_order"] == sh["row_order"], (name, p)
    assert p["nblocks_up"] >= sh["blocks"][0] and p["nblocks_dw"] >= sh["blocks"][1], (name, p)
    assert p["max_outer_up"] >= sh["outer"][0] and p["max_outer_dw"] >= sh["outer"][1], (name, p)
    for k, s in enumerate(sh["sets"]):
        q = out[k][1]
        if s.get("tile_bits_up") == 6:
            assert max(q["nblocks_up"], q["nblocks_dw"]) == 15444 and max(q["max_outer_up"], q["max_outer_dw"]) >= 25, (name, q)
        if s.get("job_up") == 1:       # above 65535 up rows pass A never runs as jobs; 20 or 24 up rows in one block may
            assert q["job_up_active"] == (0 if math.comb(m.Ns, sector[0]) > 65535 else 1), (name, q)
    _report(name, out, sec)
    if not unsplit:
        return
    orc = OracleSector(m, *sector, 0, min(64, math.comb(m.Ns, sector[1])))
    nnz = {}
    for which in ("up", "dw"):
        rp, cols, vals = orc.csr(which)
        nnz[which] = int(rp[-1])
        assert np.array_equal(np.fromfile(d / f"{which}_rowptr.i64", dtype=np.int64), rp), (name, which)
        assert np.array_equal(np.fromfile(d / f"{which}_cols.i32", dtype=np.int32) + 1, cols), (name, which)
        got = np.fromfile(d / f"{which}_vals.c128", dtype=np.complex128)
        assert got.shape == vals.shape
        if vals.size:
            assert np.abs(got - vals).max() <= TOL * np.abs(vals).max(), (name, which)
    assert np.array_equal(np.fromfile(d / "map_up.u32", dtype=np.uint32).astype(np.int64), np.asarray(orc.map_up(), dtype=np.int64))
    assert np.array_equal(np.fromfile(d / "map_dw.u32", dtype=np.uint32).astype(np.int64), np.asarray(orc.map_dw(), dtype=np.int64))
    orc.close()
    for k in range(len(sh["sets"])):
        assert (out[k][1]["triplets_up"], out[k][1]["triplets_dw"]) == (nnz["up"], nnz["dw"]), (name, k)


def test_only_the_dimup_gate_keeps_the_job_kernel_off_the_star_sector(checker, tmp_path_factory):
    """wide_sectors.GATE: on the star model with 12 block bits and "job_max_blocks" = 256 every condition of job_up_usable but DimUp < 65536
    holds.  (6,1), 38 760 up rows: pass A is planned as jobs and the job kernel's packed registers expand to the sector's matrix.  (10,1),
    184 756 rows: the same block shapes, no jobs."""
    import wide_sectors as WS

    key, m, sector = _wide_model(WS.GATE_SECTOR)
    path = _model_file(tmp_path_factory, "wide_" + key, m)
    for sec, active in (((6, 1), 1), (sector, 0)):
        rc, out, err, _ = run_checker(checker, path, sec, sets=[dict(WS.GATE_OPTIONS)])
        _assert_passed(rc, out, err, 1, (key, sec), may_refuse=False)
        p = out[0][1]
        assert p["nblocks_up"] <= 256 and p["max_block_up"] <= 960 and p["max_outer_up"] <= 8 and p["k_in_up"] <= 24, (sec, p)
        assert (p["job_up_active"], p["job_checked"]) == (active, active), (sec, p)
        assert (math.comb(m.Ns, sec[0]) < 65536) == bool(active)


def test_a_spin_dimension_above_2_to_the_20_is_refused(checker, tmp_path):
    """Ns = 24, sector (12,0): C(24,12) = 2 704 156 states of one spin are more than the 20 bits of an ELL source index.  The sector builder
    says so before it builds any matrix."""
    from hxv import models

    path = write_model(tmp_path / "chain24.model", models.hm_1dchain(Nlat=4, Nbath=5))
    rc, out, err, sec = run_checker(checker, path, (12, 0))
    print(f"refused after {sec:.1f} s")
    assert rc == 1 and not out and "spin-sector dimension exceeds 2^20" in err, (rc, out, err[-500:])


# ---- 3. seeded random sweep ----------------------------------------------------------------------------------------------------------
FUZZ_SEED0 = 4000


def _fuzz_case(seed):
    rng = np.random.default_rng(FUZZ_SEED0 + seed)
    m = random_model(rng, max_ns=12, min_bath=1)
    Ns = m.Ns
    nup, ndw = (int(np.clip(Ns // 2 + rng.integers(-1, 2), 0, Ns)) for _ in range(2))
    size = int(rng.integers(1, min(4, math.comb(Ns, ndw)) + 1))
    rank = int(rng.integers(size))
    exchange = int(rng.integers(3))
    opts = {"lds_budget_kb": int(rng.choice([8, 16, 32])), "cols_per_tile": int(rng.choice([2, 4, 8])), "rows_per_tile": int(rng.choice([2, 4, 8])),
            "threads_up": int(rng.choice([256, 512, 1024])), "threads_dw": int(rng.choice([256, 512, 1024])), "sort_mode": int(rng.integers(3)),
            "wt_cols": int(rng.choice([2, 4, 8, 16])), "job_cols": int(rng.choice([1, 2])), "pair_rows": int(rng.choice([0, 1])),
            "job_groups": int(rng.choice([1, 3, 100])), "job_max_blocks": int(rng.choice([0, 32])), "block_order": int(rng.choice([-1, 0, 1, 2]))}
    return m, (nup, ndw), (rank, size), exchange, opts


def test_random_models_sectors_shards_and_plan_options(checker, tmp_path):
    """64 seeds of random_model(max_ns=12, min_bath=1): a sector near half filling, a rank split of 1-4 in a random exchange, the random
    option dictionary of tests/test_gpu_fuzz.py.  A refused plan counts as passed; at least 48 of the 64 draws must produce a plan."""
    planned, triplets = 0, 0
    for seed in range(64):
        m, sector, shard, exchange, opts = _fuzz_case(seed)
        path = write_model(tmp_path / f"fuzz{seed}.model", m)
        rc, out, err, _ = run_checker(checker, path, sector, shard, exchange, sets=[opts])
        _assert_passed(rc, out, err, 1, (seed, sector, shard, exchange, opts))
        if out[0][0] == "PLAN":
            planned += 1
            triplets += out[0][1].get("triplets_up", 0) + out[0][1].get("triplets_dw", 0)
    print(f"random sweep: {planned} of 64 draws produced a plan, {triplets} triplets compared")
    assert planned >= 48, planned


# ---- 4. host sanitizers (stand-alone programs; never on a GPU machine) ------------------------------------------------------------------
def _no_report(err):
    return not any(s in err for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "WARNING: ThreadSanitizer", "runtime error:", "SUMMARY:"))


def test_named_shapes_under_asan_and_ubsan(built, tmp_path_factory):
    """Every named shape once, default options (the S shapes at their forced block bits), with the builders and the checker compiled with
    -fsanitize=address,undefined -fno-sanitize-recover=undefined: exit 0 and no sanitizer report on stderr.  Leak checking is ON and works
    for root and for an unprivileged user (where a sandbox forbids LeakSanitizer's tracer the test says so and goes on without it); the
    program calls no HIP entry point and the runtime library it is linked with reports nothing at load time: no suppressions file."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_plan_check("address,undefined")
    leaks = 1
    for name in SHAPE_NAMES:
        env = {"ASAN_OPTIONS": f"detect_leaks={leaks}", "UBSAN_OPTIONS": "print_stacktrace=1"}
        rc, out, err, sec = _run_shape(exe, tmp_path_factory, name, [{}], env=env)
        if leaks and "LeakSanitizer has encountered a fatal error" in err:   # (a sandbox that forbids its stop-the-world tracer: said, not hidden)
            print("LeakSanitizer cannot run here: leak checking off\n" + err[-500:])
            leaks = 0
            rc, out, err, sec = _run_shape(exe, tmp_path_factory, name, [{}], env=dict(env, ASAN_OPTIONS="detect_leaks=0"))
        assert rc == 0 and _no_report(err), (name, rc, err[-3000:])
        assert out[0][0] == "PLAN", (name, out)
        _report(name + " [asan+ubsan]", out, sec)


def test_builder_threads_under_tsan(built, tmp_path_factory):
    """C3, C4 and one Ns = 12 shape (the random-model generator's seed 1, unsplit) under -fsanitize=thread: the sector builder runs up to
    three host threads, make_tile_plan two.  Exit 0 and no report."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_plan_check("thread")
    for name in ("C3_8_8", "C4_8_8"):
        rc, out, err, sec = _run_shape(exe, tmp_path_factory, name, [{}])
        assert rc == 0 and _no_report(err), (name, rc, err[-3000:])
        _report(name + " [tsan]", out, sec)
    from hxv import models

    path = _model_file(tmp_path_factory, "square_B2", models.hm_2dsquare(Nbath=2))   # Ns = 12
    rc, out, err, sec = run_checker(exe, path, (6, 6), sets=[{"lds_budget_kb": 8}])
    assert rc == 0 and _no_report(err) and out[0][0] == "PLAN", (rc, err[-3000:])
    _report("square_B2 (6,6), 8 KB budgets [tsan]", out, sec)


# ---- 5. the plan checked on the CPU is the plan the device runs ------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_plan_stats_match_host_checker(built, checker, tmp_path):
    """S1-S4 at their forced block bits, _chain(12) (4,3) with 8 KB budgets and _model(14) (7,1) of tests/test_gpu_layout_contract.py: every
    PLAN_STATS value hxv_get_option reports on the opened handle equals the plain (unsanitized) checker's line for the same sector and
    options, computed on this machine's CPU."""
    import hxv
    from test_gpu_layout_contract import _chain, _model

    cases = []
    for key in ("S1", "S2", "S3", "S4"):
        m, sector, bits = _shape_model(key)
        cases.append((key, m, sector, {"tile_bits_up": bits, "tile_bits_dw": bits}))
    cases.append(("chain12", _chain(12), (4, 3), {"lds_budget_kb_up": 8, "lds_budget_kb_dw": 8}))
    cases.append(("model14", _model(14), (7, 1), {}))
    for name, m, sector, opts in cases:
        path = write_model(tmp_path / (name + ".model"), m)
        rc, out, err, _ = run_checker(checker, path, sector, sets=[opts])
        _assert_passed(rc, out, err, 1, name, may_refuse=False)
        sec = hxv.HxvSector.from_model(m, *sector)
        for k, v in opts.items():
            sec.set_option(k, v)
        got = {n: sec.get_option(n) for n in PLAN_STATS}
        sec.close()
        assert got == {n: out[0][1][n] for n in PLAN_STATS}, name
