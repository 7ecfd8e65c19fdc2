"""The three kernels of the non-local block spH0nd, one by one: hxv_nonlocal_kernel (searches the sector maps), hxv_nonlocal_tab (one-spin
move tables, one workgroup per column and 1024 rows) and hxv_nonlocal_csr (stored rows), through the test-only launchers of
tests/device/nonlocal_kernels_check.hip.  The product reaches them on real sectors only, all of them with DimUp <= 924 before this file:
one row chunk per column, one trip of every grid-stride loop.  Here each runs alone on the synthetic tables, slabs, chunk counts and GRIDS
of tests/nonlocal_kernels_ref.py, which tests/test_nonlocal_kernels_ref_cpu.py has shown to stay inside their buffers, to reach the
second and third chunk and loop trip, and to be refused when the kernel makes any of the listed mistakes.

Exact values (small integers times signed powers of two) are compared bit for bit over the whole buffer; random values within the bound
derived in the restatement's docstring, (T + 2) * 2**-53 * (|h0| + sum|c||x|) per component for T terms ((2T + 2) for the complex
coefficients of the CSR form), against a sum in extended precision.  Throughout, hv starts from a sentinel pattern with a guard element
behind it -- pad rows, the guard and every element without a term must keep its bits, -0.0 included -- and v holds NaN wherever the
contract does not read.

Last, the same thresholds on a real model against the oracle: two orbitals on one site with six bath levels each (Ns = 14), sectors
(7, 1) and (7, 2) (DimUp = 3432: four row chunks, several pass-A blocks) and (2, 7) (the long dimension is the dw one)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import nonlocal_kernels_ref as R

pytestmark = pytest.mark.gpu

BAD = 1  # hipErrorInvalidValue
CASES = R.all_cases()
IDS = [f"{k}-{c.name}" for k, c in CASES]


@pytest.fixture(scope="session")
def nkc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_nonlocal_kernels_check()))
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    L.nkc_nonlocal_kernel.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f64, f64]
    L.nkc_nonlocal_tab.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f64, f64]
    L.nkc_nonlocal_csr.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]
    return L


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def call(L, kernel, c, coef, d_v, d_hv, **over):
    """the status of one launch of the case's kernel on these two device buffers; `over` replaces arguments by name"""
    if kernel == "tab":
        a = dict(rchunks=c.rchunks, v=d_v, hv=d_hv, nd_up=dev(c.nd_up), nd_dw=dev(c.nd_dw), dimup=c.dimup, dimdw=c.dimdw, pitch=c.pitch, qdw=c.qdw,
                 dw0=c.dw0, nlat=c.nlat, norb=c.norb, jx=coef[0], jp=coef[1])
        fn = L.nkc_nonlocal_tab
    elif kernel == "kernel":
        a = dict(gx=c.gx, v=d_v, hv=d_hv, map_up=dev(c.map_up), map_dw=dev(c.map_dw), vcol=dev(c.vcol), dimup=c.dimup, dimdw=c.dimdw, pitch=c.pitch,
                 qdw=c.qdw, dw0=c.dw0, nlat=c.nlat, norb=c.norb, jx=coef[0], jp=coef[1])
        fn = L.nkc_nonlocal_kernel
    else:
        # (an empty cols / vals array still needs an address: one element that no row names)
        cols, vals = (c.cols, coef) if c.cols.shape[0] else (np.ones(1, dtype=np.int32), np.full(1, R.NAN))
        a = dict(gx=c.gx, v=d_v, hv=d_hv, rowptr=dev(c.rowptr), cols=dev(cols), vals=dev(vals), vcol=dev(c.vcol), dimup=c.dimup, dimdw=c.dimdw,
                 pitch=c.pitch, qdw=c.qdw, dw0=c.dw0)
        fn = L.nkc_nonlocal_csr
    a.update(over)
    return fn(*[None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x) for x in a.values()])


@lru_cache(maxsize=None)
def prepared(k, kind):
    """(coefficients, terms, v, h0) of CASES[k] with one kind of values: computed once, never changed"""
    kernel, c = CASES[k]
    coef = R.coefficients(kernel, c, kind)
    terms = R.terms_of(kernel, c, coef)
    return coef, terms, R.inputs(c, terms, kind), R.h0_buffer(c.nhv)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_kernel_alone(nkc, k, kind):
    kernel, c = CASES[k]
    coef, terms, v, h0 = prepared(k, kind)
    d_v, d_hv = dev(v), dev(h0)
    assert call(nkc, kernel, c, coef, d_v, d_hv) == 0
    got = d_hv.cpu().numpy()
    assert R.check(terms, v, h0, got, kind) == [], (kernel, c.name, kind)
    assert np.array_equal(R.bits(d_v.cpu().numpy()), R.bits(v))


# ---- the launchers' refusals -----------------------------------------------------------------------------------------------------------------
def _first(kernel, name):
    return next(k for k, (kn, c) in enumerate(CASES) if kn == kernel and c.name == name)


# (argument, its bad value: a number, None for a NULL, or the name of an entry of `relative`, worked out from the case)
COMMON_BAD = [("dimup", 0), ("dimdw", 0), ("qdw", 0), ("pitch", "dimup-1"), ("pitch", "pitch+4"), ("dw0", -1), ("dw0", "dimdw-qdw+1"), ("v", None),
              ("hv", None)]


def relative(c):
    return {"dimup-1": c.dimup - 1, "pitch+4": c.pitch + 4, "dimdw-qdw+1": c.dimdw - c.qdw + 1}


REFUSALS = (
    [("tab", "up2049-q3-L2O2-Jxp", n, x) for n, x in COMMON_BAD + [("rchunks", 2), ("rchunks", 0), ("rchunks", 21846), ("nd_up", None), ("nd_dw", None),
                                                                    ("norb", 0), ("norb", 6), ("nlat", 0), ("nlat", 17)]] +
    [("kernel", "ns8-4+4-L2O2-Jxp-grid4", n, x) for n, x in COMMON_BAD + [("gx", 0), ("gx", 65536), ("map_up", None), ("map_dw", None), ("vcol", None),
                                                                        ("norb", 0), ("norb", 6), ("nlat", 0), ("nlat", 17)]] +
    [("csr", "up67-dw40-q30-grid4", n, x) for n, x in COMMON_BAD + [("gx", 0), ("gx", 65536), ("rowptr", None), ("cols", None), ("vals", None),
                                                                     ("vcol", None)]])


@pytest.mark.parametrize("kernel,name,arg,value", REFUSALS, ids=[f"{k}-{a}={v}" for k, _, a, v in REFUSALS])
def test_launcher_refuses(nkc, kernel, name, arg, value):
    k = _first(kernel, name)
    c = CASES[k][1]
    coef, _, v, h0 = prepared(k, "exact")
    if isinstance(value, str):
        value = relative(c)[value]
    d_hv = dev(h0)
    assert call(nkc, kernel, c, coef, dev(v), d_hv, **{arg: value}) == BAD
    assert np.array_equal(R.bits(d_hv.cpu().numpy()), R.bits(h0))


def test_launcher_refuses_more_orbitals_than_bits(nkc):
    k = _first("tab", "up63-q1-L2O2-Jxp")
    c = CASES[k][1]
    coef, _, v, h0 = prepared(k, "exact")
    d_hv = dev(h0)
    assert call(nkc, "tab", c, coef, dev(v), d_hv, nlat=7, norb=5) == BAD      # 35 orbitals
    assert np.array_equal(R.bits(d_hv.cpu().numpy()), R.bits(h0))


# ---- the same thresholds on a real model, against the oracle ---------------------------------------------------------------------------------------
HXV_TOL = 2e-13
NS14_SECTORS = [(7, 1), (7, 2), (2, 7)]      # DimUp x DimDw = 3432 x 14, 3432 x 91, 91 x 3432
# (rank 0 of 3 beside rank 1: in (7, 1) the one dw particle sits on an impurity orbital only in columns 0 and 1, so rank 1 has no spH0nd row)
NS14_SHARDS = [(0, 1), (1, 3), (0, 3)]


def _ns14():
    from hxv import models

    return models.bhz_2d(Nx=1, Ny=1, Nbath=6, Ust=1.0, Jh=0.3, Jx=0.3, Jp=0.25)     # two orbitals, six bath levels each: Ns = 14


@lru_cache(maxsize=None)
def _ns14_reference(nup, ndw):
    """(v, H v) of the whole sector from the oracle's serial product: computed once per sector"""
    from hxv import models
    from oracle.oracle import OracleSector

    orc = OracleSector(_ns14(), nup, ndw)
    v = models.deterministic_vector(orc.Dim)
    hv = orc.spMatVec_main(v)
    orc.close()
    v.setflags(write=False)
    hv.setflags(write=False)
    return v, hv


@pytest.mark.parametrize("shard", NS14_SHARDS, ids=["unsplit", "rank1of3", "rank0of3"])
@pytest.mark.parametrize("sector", NS14_SECTORS, ids=[f"{a}+{b}" for a, b in NS14_SECTORS])
def test_ns14_product_matches_the_oracle(built, sector, shard):
    """the product with the spH0nd block where DimUp (or DimDw) passes 1024, for both product kernels, with the block folded into pass A
    and as its own pass (hxv_nonlocal_tab with four row chunks per column), unsplit and for rank 1 of 3 on the gather layout"""
    import torch
    import hxv
    from oracle.oracle import OracleSector

    (nup, ndw), (rank, size) = sector, shard
    m = _ns14()
    v, full = _ns14_reference(nup, ndw)
    orc = OracleSector(m, nup, ndw, rank, size)
    ref = full[orc.mpiIshift:orc.mpiIshift + orc.vecDim]
    sec = hxv.HxvSector.from_model(m, nup, ndw, rank=rank, nranks=size)
    assert (sec.DimUp, sec.DimDw) == (orc.DimUp, orc.DimDw) and max(sec.DimUp, sec.DimDw) == 3432 and sec.Dim == v.shape[0]
    assert (sec.vecDim, sec.mpiQdw, sec.mpiIshift) == (orc.vecDim, orc.mpiQdw, orc.mpiIshift)
    if nup == 7:
        assert sec.DimUp > 1024
    dv = torch.from_numpy(sec.to_gather_layout(np.array(v), size)).cuda()
    for kernel in (0, 1):
        for fold in (0, 1):
            sec.set_option("kernel", kernel)
            sec.set_option("fold_nd", fold)
            got = sec.unpad(sec.apply_device(dv)).cpu().numpy()
            err = np.abs(got - ref).max()
            print(f"ns14 {sector} {shard} kernel={kernel} fold_nd={fold}: err {err:.3e} of {np.abs(ref).max():.3e}, nblocks_up {sec.get_option('nblocks_up')}")
            assert err <= HXV_TOL * np.abs(ref).max(), (sector, shard, kernel, fold)
            assert (sec.get_option("kernel"), sec.get_option("fold_nd")) == (kernel, fold)
            if fold == 1 and nup == 7:
                assert sec.get_option("nblocks_up") > 1
    sec.close()
    orc.close()


@pytest.mark.parametrize("shard", NS14_SHARDS, ids=["unsplit", "rank1of3", "rank0of3"])
@pytest.mark.parametrize("sector", NS14_SECTORS, ids=[f"{a}+{b}" for a, b in NS14_SECTORS])
def test_ns14_stored_rows_match_the_oracle(built, sector, shard):
    """the same sectors on a from_csr handle that takes the oracle's spH0nd rows through set_nonlocal_csr (hxv_nonlocal_csr)"""
    import torch
    import hxv
    from oracle.oracle import OracleSector

    (nup, ndw), (rank, size) = sector, shard
    v, full = _ns14_reference(nup, ndw)
    orc = OracleSector(_ns14(), nup, ndw, rank, size)
    ref = full[orc.mpiIshift:orc.mpiIshift + orc.vecDim]
    sec = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag(), rank=rank, nranks=size)
    rp, cols, vals = orc.csr("nd")
    assert rp.shape == (orc.vecDim + 1,) and max(sec.DimUp, sec.DimDw) == 3432
    assert cols.shape[0] > 0 or (sector, shard) == ((7, 1), (1, 3))
    sec.set_nonlocal_csr(rp, cols, vals)
    dv = torch.from_numpy(sec.to_gather_layout(np.array(v), size)).cuda()
    for kernel in (0, 1):
        for fold in (0, 1):
            sec.set_option("kernel", kernel)
            sec.set_option("fold_nd", fold)
            got = sec.unpad(sec.apply_device(dv)).cpu().numpy()
            err = np.abs(got - ref).max()
            print(f"ns14 stored rows {sector} {shard} kernel={kernel} fold_nd={fold}: err {err:.3e} of {np.abs(ref).max():.3e}")
            assert err <= HXV_TOL * np.abs(ref).max(), (sector, shard, kernel, fold)
    sec.close()
    orc.close()
