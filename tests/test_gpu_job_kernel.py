"""The pass-A job kernel hxv_up_job alone, through the test-only launcher of tests/device/job_kernel_check.hip, on the synthetic tables, slabs,
ring depths, chunk cuts and scratch layouts of tests/job_kernel_ref.py.  tests/test_job_kernel_ref_cpu.py has shown every one of these
launches to stay inside its buffers and its LDS, to reach the paths the product's sectors do not, and the comparison made here to refuse
each of the listed mistakes.

Exact values (small integers times signed powers of two, every sum exact in float64 in any order) are compared bit for bit over the whole
of hv, partial and partial2: hv starts from a sentinel pattern with a guard element behind it, the partials from a pattern that is longer than
the launch has workgroups, and v, xm and the scratch hold NaN wherever the contract reads nothing.  Random values are held to the bound
derived in the restatement's docstring against a sum in extended precision.  Then the bit identities the code promises, the launcher's
refusals, and last the same thresholds on a real plan with full blocks through the C ABI against the oracle."""
import ctypes as C

import numpy as np
import pytest

import job_kernel_ref as R

pytestmark = pytest.mark.gpu

BAD = 1  # hipErrorInvalidValue
CASES = R.all_cases()
IDS = [c.name for c in CASES]


class JkcArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("start", "tstart", "gstart", "gmax", "ell_in", "bh_ptr", "bh", "rs_ptr", "rs_off", "rs_tab", "rs_base", "rs_neg",
                                           "order", "scoef", "a_up", "a_dw", "map_up", "map_dw", "v", "wt", "xm", "hv", "scal", "partial", "partial2")] +
                [(n, C.c_int32) for n in ("dimup", "dimdw", "pitch", "qdw", "dw0", "slab0", "vslots", "real_h", "nblocks", "max_block", "ncoef", "k_in",
                                          "k_in_real", "max_outer", "job_groups", "job_stages", "wc", "lz", "i_s", "i_c", "i_s2", "i_c2", "nscal", "npartial",
                                          "norb", "nlat")] +
                [("uloc", C.c_double * 5), ("ust", C.c_double), ("orbmask", C.c_uint32 * 5), ("sitemask", C.c_uint32 * 16)])


@pytest.fixture(scope="session")
def jkc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_job_kernel_check()))
    L.jkc_up_job.argtypes = [C.POINTER(JkcArgs)]
    return L


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


class Launch:
    """one launch of the case: the device buffers, the status, and what came back"""

    def __init__(self, L, c, t, val, lz=None, job_stages=None, job_groups=None, over=None, null=()):
        lz = c.lz if lz is None else lz
        g = R.case_geometry(c, t, job_stages, job_groups, lz)
        npart = g["nwg"] + 3
        self.h0, self.p0, self.p20 = R.h0_buffer(c), R.partial0(npart), R.partial0(npart) - 100.0
        tabs = {n: dev(getattr(t, n)) for n in ("start", "tstart", "gstart", "gmax", "ell_in", "bh_ptr", "bh", "rs_ptr", "rs_off", "rs_tab", "rs_base",
                                                "rs_neg", "order", "map_up", "map_dw")}
        self.inputs = dict(v=val.v, wt=val.wt, xm=val.xm if lz else None, scoef=val.scoef, a_up=val.a_up, a_dw=val.a_dw, scal=val.scal)
        self.d_in = {n: (None if a is None else dev(a)) for n, a in self.inputs.items()}
        self.d_hv, self.d_p, self.d_p2 = dev(self.h0), dev(self.p0), dev(self.p20)
        a = JkcArgs()
        for n, d in list(tabs.items()) + list(self.d_in.items()) + [("hv", self.d_hv), ("partial", self.d_p), ("partial2", self.d_p2)]:
            setattr(a, n, None if d is None or n in null else d.data_ptr())
        ints = dict(dimup=c.dimup, dimdw=c.ndw, pitch=c.pitch, qdw=c.qdw, dw0=c.dw0, slab0=c.slab0, vslots=c.nslots, real_h=val.real_h,
                    nblocks=c.nblocks, max_block=c.max_block, ncoef=c.ncoef, k_in=t.k_in, k_in_real=t.k_in_real, max_outer=t.max_outer,
                    job_groups=job_groups or c.job_groups, job_stages=job_stages or c.job_stages, wc=c.wc, lz=lz, i_s=R.I_S, i_c=R.I_C, i_s2=R.I_S2,
                    i_c2=R.I_C2, nscal=R.NSCAL, npartial=npart, norb=c.norb, nlat=val.nlat)
        ints.update(over or {})
        for n, x in ints.items():
            setattr(a, n, int(x))
        a.ust = val.ust
        for i in range(5):
            a.uloc[i], a.orbmask[i] = float(val.uloc[i]), int(val.orbmask[i])
        for i in range(16):
            a.sitemask[i] = int(val.sitemask[i])
        self.status = L.jkc_up_job(C.byref(a))
        self.got = (self.d_hv.cpu().numpy(), self.d_p.cpu().numpy(), self.d_p2.cpu().numpy())

    def untouched(self):
        return R.differs(self.got, (self.h0, self.p0, self.p20)) == []

    def inputs_kept(self):
        return all(a is None or np.array_equal(R.bits(self.d_in[n].cpu().numpy()), R.bits(a)) for n, a in self.inputs.items())


def within(got, exp):
    """largest |got - exact| / bound over hv and over each partial array, against the UNROUNDED long-double values (0/0 counts as 0: where
    the bound is 0 the value is the start pattern's)"""
    bound, bp, bp2, (xhv, xp, xp2) = exp[3:]
    out = []
    err = np.stack([np.abs(got[0][:-1].real - xhv[:-1, 0]), np.abs(got[0][:-1].imag - xhv[:-1, 1])], axis=1)
    for e, b in ((err, bound), (np.abs(got[1] - xp), bp), (np.abs(got[2] - xp2), bp2)):
        assert not np.isnan(e).any()
        assert (e[b == 0] == 0).all(), "an element without a term changed"
        out.append(float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
    return out


# ---- every case, every kind of values ----------------------------------------------------------------------------------------------------------
# (the paired epilogue exists for real H only: its cases run the two real kinds)
ALONE = [(k, kind) for k, c in enumerate(CASES) for kind in c.real_kinds()]


@pytest.mark.parametrize("k,kind", ALONE, ids=[f"{IDS[k]}-{kind}" for k, kind in ALONE])
def test_kernel_alone(jkc, k, kind):
    c, t, val, exp = R.prepared(k, kind)
    run = Launch(jkc, c, t, val)
    assert run.status == 0
    if kind.startswith("exact"):
        assert R.differs(run.got, exp[:3]) == [], (c.name, kind)
    else:
        assert np.array_equal(R.bits(run.got[0][-1:]), R.bits(exp[0][-1:])), "the guard"
        ratios = within(run.got, exp)
        print(f"RATIO {c.name} {kind} hv {ratios[0]:.3f} partial {ratios[1]:.3f} partial2 {ratios[2]:.3f}")
        assert max(ratios) <= 1.0, (c.name, kind, ratios)
    assert run.inputs_kept()


# ---- bit identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [i for i, c in enumerate(CASES) if c.lz == 2], ids=[c.name for c in CASES if c.lz == 2])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_paired_epilogue_is_two_single_ones(jkc, k, kind):
    """LZ = 2 on (x, y) gives, component by component, the bits of two LZ = 1 runs on (x, 0) and (y, 0): vector and partials"""
    c, t, val, _ = R.prepared(k, kind)
    pair = Launch(jkc, c, t, val)
    assert pair.status == 0
    for comp, (i_s, i_c), part in (("real", (R.I_S, R.I_C), pair.got[1]), ("imag", (R.I_S2, R.I_C2), pair.got[2])):
        one = R.values(c, t, kind)

        def only(a):
            """the chosen component in the real part, 0 in the imaginary one; NaN where the contract reads nothing stays NaN"""
            if a is None:
                return None
            x = getattr(a, comp)
            return R.cpx(x, np.where(np.isnan(x), np.nan, 0.0))

        one.v, one.wt, one.xm = only(val.v), only(val.wt), only(val.xm)
        single = Launch(jkc, c, t, one, lz=1, over=dict(i_s=i_s, i_c=i_c))
        assert single.status == 0
        rows = lambda h: h[:-1].reshape(c.qdw, c.pitch)[:, :c.dimup]
        a, b = getattr(rows(pair.got[0]), comp), rows(single.got[0]).real
        assert np.array_equal(R.bits(np.ascontiguousarray(a)), R.bits(np.ascontiguousarray(b))), (c.name, comp)
        assert (rows(single.got[0]).imag == 0).all()
        nwg = R.case_geometry(c, t)["nwg"]    # (behind them the two arrays keep their own start patterns)
        assert np.array_equal(R.bits(part[:nwg]), R.bits(single.got[1][:nwg])), (c.name, comp, "partials")


@pytest.mark.parametrize("k", R.plain_cases_that_fit_the_epilogue(), ids=lambda k: IDS[k])
@pytest.mark.parametrize("kind", ["exact", "random", "randomc"])
def test_unit_epilogue_stores_the_plain_product(jkc, k, kind):
    """LZ = 1 with s = 1, c = 0 and no xm stores the bits of LZ = 0"""
    c, t, val, _ = R.prepared(k, kind)
    plain = Launch(jkc, c, t, val)
    one = R.values(c, t, kind)
    one.scal[[R.I_S, R.I_C]] = [1.0, 0.0]
    unit = Launch(jkc, c, t, one, lz=1)
    assert plain.status == 0 and unit.status == 0
    assert R.differs(unit.got[:1], plain.got[:1]) == []


@pytest.mark.parametrize("name", R.VARIANT_CASES)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_ring_depth_and_chunk_cut_change_no_operation(jkc, name, kind):
    """the same case under job_stages 2 / 3 / 4 / 8 and under several job_groups: the same hv bits; the partials (other workgroups, other
    sums) are compared as exact sums"""
    k = IDS.index(name)
    c, t, val, exp = R.prepared(k, kind)
    base = Launch(jkc, c, t, val)
    assert base.status == 0
    n = 0
    for kw in [dict(job_stages=s) for s in R.VARIANT_STAGES] + [dict(job_groups=g) for g in R.VARIANT_GROUPS]:
        g = R.case_geometry(c, t, **kw)
        if not g["fits"]:
            continue
        run = Launch(jkc, c, t, val, **kw)
        assert run.status == 0, kw
        assert R.differs(run.got[:1], base.got[:1]) == [], (name, kw)
        if kind == "exact":
            want = R.expected(c, t, val, g=g)
            assert R.differs(run.got, want[:3]) == [], (name, kw)
        n += 1
    assert n >= 6


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [("dimup", 65536), ("max_block", 961), ("max_outer", 9), ("k_in", 28), ("job_stages", 1), ("job_stages", 9), ("wc", 3), ("wc", 32), ("wc", -2),
            ("wc", "too wide"), ("pitch", "dimup-1"), ("dw0", -1), ("dw0", "dimdw-qdw+1"), ("slab0", -1), ("slab0", "vslots-qdw+1"), ("qdw", 0),
            ("npartial", "nwg-1"), ("lz", 3), ("i_s", R.NSCAL), ("i_c", -1), ("norb", 0), ("norb", 6)]
NULLS = ["start", "tstart", "gstart", "gmax", "ell_in", "bh_ptr", "bh", "rs_ptr", "rs_off", "rs_tab", "rs_base", "rs_neg", "order", "scoef", "a_up", "a_dw",
         "map_up", "map_dw", "v", "hv", "scal", "partial"]


def _full():
    return IDS.index("full-960-lz1-clamped")


@pytest.mark.parametrize("arg,value", REFUSALS, ids=[f"{a}={v}" for a, v in REFUSALS])
def test_launcher_refuses(jkc, arg, value):
    c, t, val, _ = R.prepared(_full(), "exact")
    g = R.case_geometry(c, t)
    rel = {"dimup-1": c.dimup - 1, "dimdw-qdw+1": c.ndw - c.qdw + 1, "vslots-qdw+1": c.nslots - c.qdw + 1, "nwg-1": g["nwg"] - 1, "too wide": 4}
    if value == "too wide":
        assert not R.geometry(c.qdw, c.max_block, c.nblocks, c.ncoef, t.k_in, t.k_in_real, c.job_groups, c.job_stages, 4, c.lz)["fits"]
    run = Launch(jkc, c, t, val, over={arg: rel.get(value, value)})
    assert run.status == BAD and run.untouched()


@pytest.mark.parametrize("name", NULLS)
def test_launcher_refuses_null(jkc, name):
    c, t, val, _ = R.prepared(_full(), "exact")
    run = Launch(jkc, c, t, val, null=(name,))
    assert run.status == BAD and run.untouched()


def test_launcher_refuses_the_paired_epilogue_with_complex_h(jkc):
    k = IDS.index("edge-sizes-lz2")
    c, t, _, _ = R.prepared(k, "exact")
    val = R.values(c, t, "exactc")
    run = Launch(jkc, c, t, val)
    assert run.status == BAD and run.untouched()
    c, t, val, _ = R.prepared(k, "exact")
    run = Launch(jkc, c, t, val, null=("partial2",))
    assert run.status == BAD and run.untouched()


# ---- the same thresholds on a real plan with full blocks ---------------------------------------------------------------------------------------
# One site with 13 bath levels (Ns = 14), sector (7, 2), 12 block bits: four up blocks of C(12,7) = 792, C(12,6) = 924 (twice) and C(12,5) = 792
# rows -- all 15 compute waves live, the last one partly -- two out-of-block partners each, DimUp = 3432 in the device row order, 91 columns.
# tests/host/plan_check.cpp reads "job_up_active" = 1 for it under job_up = 1 with scratch groups of 2 and 4 columns.  With wt_cols = 8 two
# group buffers of 960 rows x 8 columns leave no room for two ring stages (job_up_fits): "job_up_active" reads 0 for the configured width and
# the product runs its jobs beside groups of 2 columns instead (use_job_up), as the fused product does at every width here.  The wt_cols = 8
# legs therefore run the job geometry of the wt_cols = 2 legs: they hold the fallback (and pass B writing the width pass A reads) to the
# oracle, not the kernel beside groups of 8 columns -- those, like groups of 16, are run by the synthetic cases only.
ORACLE_TOL = 1e-13
FULL_SECTOR = (7, 2)
FULL_BASE = {"tile_bits_up": 12, "job_up": 1}
FULL_GEOMETRIES = [{}, {"job_stages": 2, "wt_cols": 2}, {"job_stages": 8, "wt_cols": 2}, {"job_stages": 2, "wt_cols": 8}, {"job_stages": 8, "wt_cols": 8}]
_FULL = {}


def _full_case():
    """(model, oracle, v, H v) of the full-block sector, opened and computed once"""
    if not _FULL:
        from hxv import models
        from oracle.oracle import OracleSector

        m = models.hm_1dchain(Nlat=1, Nbath=13, eps_bath=[(k - 6) / 10 for k in range(13)])
        orc = OracleSector(m, *FULL_SECTOR)
        rng = np.random.default_rng(1492)
        v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
        ref = orc.spMatVec_main(v)
        _FULL.update(m=m, orc=orc, v=v, ref=ref)
    return _FULL["m"], _FULL["orc"], _FULL["v"], _FULL["ref"]


def _open_full(geometry, **kw):
    import hxv

    m = _full_case()[0]
    sec = hxv.HxvSector.from_model(m, *FULL_SECTOR, **kw)
    for o, x in dict(FULL_BASE, **geometry).items():
        sec.set_option(o, x)
    got = {n: sec.get_option(n) for n in ("nblocks_up", "max_block_up", "max_outer_up", "k_in_up", "tile_bits_up", "job_up_active")}
    assert got["tile_bits_up"] == 12 and got["nblocks_up"] == 4 and 897 <= got["max_block_up"] == 924 and got["max_outer_up"] <= 8 and got["k_in_up"] <= 24, got
    assert got["job_up_active"] == (0 if geometry.get("wt_cols") == 8 else 1), (geometry, got)
    return sec


@pytest.mark.parametrize("rank,nranks", [(0, 1), (1, 3)], ids=["unsplit", "rank1of3"])
def test_full_blocks_plain_product_meets_the_oracle(built, rank, nranks):
    """poisoned pad rows and unused slots in, sentinel pad rows out (the helpers of tests/test_gpu_layout_contract.py), the oracle's product at
    1e-13, the same bits under job_stages 2 and 8"""
    import torch
    from hxv import dw_split
    import test_gpu_layout_contract as LC

    m, orc, v, ref = _full_case()
    V, Rf = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
    q, c0 = dw_split(orc.DimDw, rank, nranks)
    scale = np.abs(ref).max()
    seen = {}
    for geo in FULL_GEOMETRIES:
        sec = _open_full(geo, rank=rank, nranks=nranks)
        try:
            lay = LC.lay_of(sec)
            assert lay.perm is not None and sec.DimUp == 3432 and sec.mpiQdw == q
            vin = LC.gathered(V, lay, nranks, "cuda")
            hv = LC.sentinel_like(sec.localElems, torch.complex128, "cuda")
            sec.apply_device(vin, hv)
            torch.cuda.synchronize()
            assert LC.pad_bits_off(hv, lay, LC.SENTINEL) == 0, (geo, "pad rows were written")
            got = LC.live(hv, lay)
            assert np.isfinite(got).all(), (geo, "a dead element was read")
            err = np.abs(got - Rf[c0:c0 + q]).max() / scale
            print(f"full blocks {geo} rank {rank}/{nranks}: {err:.2e}")
            assert err <= ORACLE_TOL, (geo, err)
            same = seen.setdefault(geo.get("wt_cols"), hv.cpu().numpy())
            assert np.array_equal(R.bits(same), R.bits(hv.cpu().numpy())), (geo, "bits differ between ring depths")
        finally:
            sec.close()


def test_full_blocks_fused_lanczos_meets_the_oracle(built):
    """twelve fused Lanczos steps against the oracle's recurrence at the 1e-11 of tests/test_gpu_wide_sectors.py; the same coefficients bit
    for bit under job_stages 2 and 8"""
    import torch

    m, orc, v, _ = _full_case()
    vn = v / np.linalg.norm(v)
    a0, b0 = orc.lanc_tridiag(vn, 12)
    seen = {}
    for geo in FULL_GEOMETRIES:
        sec = _open_full(geo)
        try:
            assert sec.get_option("lanczos_fused") == 1
            a, b, n = sec.lanczos_tridiag(sec.pad(torch.from_numpy(vn).cuda()), 12)
            assert n == len(a0) == 12
            ea, eb = np.abs(a - a0).max() / np.abs(a0).max(), np.abs(b[1:] - b0[1:]).max() / np.abs(b0).max()
            print(f"full blocks {geo} 12 fused Lanczos steps: alpha {ea:.2e}, beta {eb:.2e}")
            assert ea <= 1e-11 and eb <= 1e-11, (geo, ea, eb)
            same = seen.setdefault(geo.get("wt_cols"), (np.array(a), np.array(b)))
            assert np.array_equal(R.bits(same[0]), R.bits(np.array(a))) and np.array_equal(R.bits(same[1]), R.bits(np.array(b))), geo
        finally:
            sec.close()
