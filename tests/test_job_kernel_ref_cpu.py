"""The cases of tests/job_kernel_ref.py are safe to launch, reach the paths they are there for, have the engine's geometry, and the
comparison bites (no GPU, no kernel).

SAFE.  `walk` forms every index through a checked lookup into the buffers tests/test_gpu_job_kernel.py uploads and holds every LDS byte
offset against the launch's LDS size; it walks every case, every variant the GPU file launches, and must give the bits of the plain sum.
REACH.  From the geometry and the tables: block sizes, ring depths, chunk cuts, scratch layouts, instantiations, slot kinds.
GEOMETRY.  The restated geometry is the engine's job_up_geometry / job_up_fits, read through jkc_geometry (no device call).
BITE.  One named mistake at a time is switched on in the restatement; the bit-for-bit comparison must refuse it on at least one case."""
import ctypes as C

import numpy as np
import pytest

import job_kernel_ref as R

CASES = R.all_cases()
IDS = [c.name for c in CASES]
GEO = ["ngroups", "gpx", "chunks", "ns", "stage_bytes", "wt_bytes", "nst", "lds_bytes", "kin_rows", "nwg", "fits"]


# ---- SAFE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_walk_stays_inside_and_gives_the_plain_sum(k):
    c, t, val, exp = R.prepared(k, "exact")
    got = R.walk(c, t, val)                       # raises OutOfBounds at the first index outside a buffer
    assert R.differs(got, exp[:3]) == []
    g = R.case_geometry(c, t)
    hv = got[0]
    h0 = R.h0_buffer(c)
    H, H0 = hv[:-1].reshape(c.qdw, c.pitch), h0[:-1].reshape(c.qdw, c.pitch)
    assert np.array_equal(R.bits(hv[-1:]), R.bits(h0[-1:])), "the guard"
    assert np.array_equal(R.bits(H[:, c.dimup:]), R.bits(H0[:, c.dimup:])), "pad rows"
    assert not np.isnan(H[:, :c.dimup]).any()
    for p_, off in ((got[1], 0.0), (got[2], 100.0)):
        assert np.array_equal(p_[g["nwg"]:], R.partial0(g["nwg"] + 3)[g["nwg"]:] - off), "partials beyond the launch"
    if c.lz:
        assert not np.isnan(got[1][:g["nwg"]]).any() and (got[1][:g["nwg"]] != R.partial0(g["nwg"] + 3)[:g["nwg"]]).all()


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_launch_arguments_obey_the_launchers_rules(k):
    c, t = CASES[k], R.tables_of(k)
    g = R.case_geometry(c, t)
    assert c.pitch >= c.dimup and c.pitch % 8 == 0 and 1 <= c.dimup < 65536
    assert 0 <= c.dw0 and c.dw0 + c.qdw <= c.ndw and 0 <= c.slab0 and c.slab0 + c.qdw <= c.nslots
    assert c.max_block <= 64 * R.JOB_LOADER and t.k_in <= R.JOB_KIN and t.k_in % 4 == 0 and t.max_outer <= R.JOB_KO
    assert g["fits"] and g["lds_bytes"] <= R.LDS_BUDGET and c.wc in (0, 2, 4, 8, 16) and c.ncoef <= 255
    assert sorted(t.order.tolist()) == list(range(c.nblocks))
    assert (np.diff([c.sizes[b] for b in t.order]) <= 0).all(), "largest block first"
    # the input buffers hold NaN wherever pass A reads nothing
    val = R.values(c, t, "exact")
    V = val.v.reshape(c.nslots, c.pitch)
    assert np.isnan(V[:, c.dimup:]).all() and np.isnan(V[:c.slab0]).all() and np.isnan(V[c.slab0 + c.qdw:]).all()
    assert not np.isnan(V[c.slab0:c.slab0 + c.qdw, :c.dimup]).any()
    if c.wt and c.wc:
        W = val.wt.reshape(-1, c.dimup, c.wc).transpose(0, 2, 1).reshape(-1, c.dimup)
        assert np.isnan(W[c.qdw:]).all() and not np.isnan(W[:c.qdw]).any()


@pytest.mark.parametrize("name", R.VARIANT_CASES)
def test_variants_stay_inside_and_give_the_same_vector(name):
    k = IDS.index(name)
    c, t, val, exp = R.prepared(k, "exact")
    for kw in [dict(job_stages=s) for s in R.VARIANT_STAGES] + [dict(job_groups=g) for g in R.VARIANT_GROUPS]:
        if not R.case_geometry(c, t, **kw)["fits"]:
            continue
        got = R.walk(c, t, val, **kw)
        assert R.differs(got[:1], exp[:1]) == [], kw


@pytest.mark.parametrize("k", R.plain_cases_that_fit_the_epilogue(), ids=lambda k: IDS[k])
def test_plain_cases_also_walk_with_the_epilogue(k):
    """the GPU file runs the plain cases once more as LZ = 1 with s = 1, c = 0 and no xm (the ring stages are twice as large then)"""
    c, t, val, exp = R.prepared(k, "exact")
    one = R.values(c, t, "exact")
    one.scal[[R.I_S, R.I_C]] = [1.0, 0.0]
    got = R.walk(c, t, one, lz=1)
    assert R.differs(got[:1], exp[:1]) == []


@pytest.mark.parametrize("kind", ["exact", "exactc"])
def test_exact_kinds_have_headroom(kind):
    for k, c in enumerate(CASES):
        if kind not in c.real_kinds():
            continue
        c, t, val, _ = R.prepared(k, kind)
        el, pa = R.exact_headroom(c, t, val)
        assert el < 2.0 ** 53 / 1024 and pa < 2.0 ** 53 / 1024, (c.name, el, pa)
        for a in (val.v, val.wt, val.xm, val.scoef, val.a_up, val.a_dw, val.scal):
            if a is not None:
                z = np.ascontiguousarray(a).view(np.float64)
                assert not (np.signbit(z) & (z == 0.0)).any(), "no -0 among the inputs"


# ---- REACH -----------------------------------------------------------------------------------------------------------------------------------
def test_every_path_is_reached():
    seen = dict(n=set(), nst=set(), clamped=False, short=False, one=False, long=False, sat=False, unsat=False, unequal=False, idle=set(), wc=set(),
                span3=False, mid=False, odd=False, ragged=False, slab=False, wt=set(), KIN=set(), kin=set(), nouter=set(), slots=set())
    for k, c in enumerate(CASES):
        t = R.tables_of(k)
        st = {}
        R.walk(c, t, R.prepared(k, "exact")[2], stats=st)
        seen["n"] |= st["n"]
        seen["nst"].add(st["nst"])
        seen["clamped"] |= st["clamped"]
        seen["short"] |= any(x < st["nst"] - 1 for x in st["ntile"])
        seen["one"] |= 1 in st["ntile"]
        seen["long"] |= any(x > 2 * st["nst"] for x in st["ntile"])
        seen["sat"] |= any(d > 63 for d in st["dist"])
        seen["unsat"] |= any(0 < d < 63 for d in st["dist"])
        runs = {}
        for xcd, nt in st["run_lengths"]:
            runs.setdefault(xcd, set()).add(nt)
        seen["unequal"] |= st["chunks"] > 1 and any(len(v) > 1 for v in runs.values())
        if st["idle"]:
            seen["idle"].add(c.lz)
        seen["wc"].add(c.wc)
        seen["span3"] |= c.wt and any(x >= 3 for x in st["groups_per_job"])
        seen["mid"] |= c.wc > 1 and any(x != 0 for x in st["first_mod"])
        seen["odd"] |= 1 in st["first_odd"]
        seen["ragged"] |= c.wc > 1 and c.qdw % c.wc != 0
        seen["slab"] |= c.slab0 > 0 and c.dw0 > 0 and c.slab0 != c.dw0
        seen["wt"].add(c.wt)
        seen["KIN"].add(st["KIN"])
        seen["kin"] |= st["kin"]
        seen["nouter"] |= st["nouter"]
        seen["slots"] |= st["slots"]
    n = seen["n"]
    assert {1, 63, 64, 65, 960} <= n
    assert any(65 < x < 897 and x % 64 for x in n) and any(897 <= x < 960 for x in n)
    assert {2, 3, 4, 8} <= seen["nst"] and seen["clamped"]
    assert seen["short"] and seen["one"] and seen["long"] and seen["sat"] and seen["unsat"]
    assert seen["unequal"] and seen["idle"] == {0, 1, 2}
    assert {0, 2, 4, 8, 16} <= seen["wc"] and seen["span3"] and seen["mid"] and seen["odd"] and seen["ragged"]
    assert seen["slab"] and seen["wt"] == {True, False}
    assert seen["KIN"] == {20, 24}
    assert 0 in seen["kin"] and any(x and x % 4 == 0 for x in seen["kin"]) and any(x % 4 for x in seen["kin"])
    assert {0, 4, 8} <= seen["nouter"] and seen["nouter"] & {1, 2, 3}
    assert {(False, True), (True, False), (True, True)} <= seen["slots"]
    assert any(c.lz and not c.xm for c in CASES) and any(c.lz and c.xm for c in CASES) and {c.lz for c in CASES} == {0, 1, 2}
    assert {c.norb for c in CASES} == {1, 2}


def test_reach_from_the_plan_numbers_is_the_walks():
    """scripts/job_kernel_reach.py works from R.reach_of; it must say what the walk of the same launch sees"""
    for k, c in enumerate(CASES):
        t = R.tables_of(k)
        st = {}
        R.walk(c, t, R.prepared(k, "exact")[2], stats=st)
        gkin = [[int(x) & 0xFFFF for x in t.gmax[int(t.gstart[b]):int(t.gstart[b]) + (c.sizes[b] + 63) // 64]] for b in range(c.nblocks)]
        r = R.reach_of(c.sizes, [a + b for a, b in c.outer], gkin, c.qdw, c.ncoef, t.k_in, t.k_in_real, c.job_groups, c.job_stages, c.wc, c.lz, c.xm, c.wt)
        assert r["nst"] == st["nst"] and r["chunks"] == st["chunks"] and r["KIN"] == st["KIN"] and r["clamped"] == st["clamped"], c.name
        assert set(r["ntile"]) == st["ntile"] and r["dist_max"] == max(st["dist"]) and set(r["kin"]) == st["kin"], c.name
        assert set(r["groups_per_job"]) == st["groups_per_job"] and r["idle_wg"] == st["idle"] and set(r["nouter"]) == st["nouter"], c.name


# ---- GEOMETRY --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jkc(built):
    L = C.CDLL(str(built.build_job_kernel_check()))
    L.jkc_geometry.argtypes = [C.c_int] * 11 + [C.POINTER(C.c_int64)]
    return L


def engine_geometry(L, qdw, nblocks, max_block, ncoef, k_in, k_in_real, max_outer, job_groups, job_stages, wc, lz):
    out = (C.c_int64 * 11)()
    assert L.jkc_geometry(qdw, nblocks, max_block, ncoef, k_in, k_in_real, max_outer, job_groups, job_stages, wc, lz, out) == 0
    return dict(zip(GEO, list(out)))


def test_geometry_is_the_engines(jkc):
    for k, c in enumerate(CASES):
        t = R.tables_of(k)
        for lz in (0, 1, 2):
            for st in [c.job_stages] + R.VARIANT_STAGES:
                for jg in [c.job_groups] + R.VARIANT_GROUPS:
                    mine = R.geometry(c.qdw, c.max_block, c.nblocks, c.ncoef, t.k_in, t.k_in_real, jg, st, c.wc, lz)
                    eng = engine_geometry(jkc, c.qdw, c.nblocks, c.max_block, c.ncoef, t.k_in, t.k_in_real, t.max_outer, jg, st, c.wc, lz)
                    assert {n: int(mine[n]) for n in GEO} == eng, (c.name, lz, st, jg)


def test_geometry_sweep_and_the_c3_shape(jkc):
    for max_block in (1, 64, 65, 448, 897, 900, 924, 960):
        for wc in (0, 1, 2, 4, 8, 16):
            for lz in (0, 1):
                for st in (2, 3, 4, 8):
                    for qdw, jg in ((3432, 100), (200, 7), (9, 1)):
                        mine = R.geometry(qdw, max_block, 8, 3, 24, 22, jg, st, wc, lz)
                        eng = engine_geometry(jkc, qdw, 8, max_block, 3, 24, 22, 8, jg, st, wc, lz)
                        assert {n: int(mine[n]) for n in GEO} == eng, (max_block, wc, lz, st, qdw, jg)
    # C3: blocks of about 900 rows with the epilogue do not fit beside scratch groups of 4 columns, and fit beside groups of 2 with 3 stages
    assert not R.geometry(3432, 900, 8, 3, 24, 22, 100, 4, 4, 1)["fits"]
    g = R.geometry(3432, 900, 8, 3, 24, 22, 100, 4, 2, 1)
    assert g["fits"] and g["nst"] == 3


def test_geometry_entry_refuses_nonsense(jkc):
    out = (C.c_int64 * 11)()
    assert jkc.jkc_geometry(0, 8, 900, 3, 24, 22, 8, 100, 4, 4, 1, out) == 1
    assert jkc.jkc_geometry(10, 8, 900, 3, 24, 22, 8, 100, 4, 3, 1, out) == 1
    assert jkc.jkc_geometry(10, 8, 900, 3, 24, 22, 8, 100, 9, 4, 1, out) == 1
    assert jkc.jkc_geometry(10, 8, 900, 3, 24, 22, 8, 100, 4, 4, 1, None) == 1


# ---- BITE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bug", R.BUGS)
def test_the_comparison_refuses_every_mistake(bug):
    refused = []
    for k, c in enumerate(CASES):
        c, t, val, exp = R.prepared(k, "exact")
        try:
            if R.differs(R.walk(c, t, val, bug=bug), exp[:3]):
                refused.append((c.name, "bits"))
        except R.OutOfBounds:
            refused.append((c.name, "bounds"))
        if any(how == "bits" for _, how in refused):
            break
    assert any(how == "bits" for _, how in refused), (bug, refused)


def test_no_mistake_is_listed_twice_or_unknown():
    assert len(set(R.BUGS)) == len(R.BUGS) == 18
