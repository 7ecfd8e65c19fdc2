"""Pass B's out-of-block phase with and without the dead-wave skip (csrc/hxv_tiled.hip).

A thread of pass B owns NP (row, column) pairs of the tile, NP sized for the plan's largest block.  In a smaller block the last pair
iterations of a wave can lie past the block altogether; the kernel then issues nothing for them (tile load, block hops, row slots, the add
into the tile) and runs out-of-block code compiled for the number of pairs the wave does own.  None of this changes a floating-point
operation or its order, and bit 4096 of the `debug` option switches it off (DevTiles::debug).  So for every plan below the product with the
shipped settings must equal, bit for bit, the product with the bit set, and one setting per case meets the CPU oracle.

Shapes: Ns = 12, sectors (6,6) and (5,7), blocks of 8 low orbitals / an 8 KB tile budget: many blocks of unequal size, every one
smaller than the workgroup (most waves are dead, some are partly live), four high orbitals (several row slots per block); blocks of 10 and
11 low orbitals (two to four pairs per thread, the last ones dead in some waves); 2 / 4 / 8 rows and 2 / 4 columns per tile, complex and
real vectors, real and complex H; a sector split over three thread ranks (gather slots that are not the identity, blocks without a local
column, blocks cut by the slab edge); poisoned pad rows."""
import os
from functools import lru_cache

import numpy as np
import pytest

import test_gpu_layout_contract as lc   # (its layout helpers; importing the module collects none of its tests here)

NO_SKIP = 4096                           # debug bit: pass B without the dead-wave skip
ORACLE_TOL = 1e-13                       # max|got - ref| <= ORACLE_TOL * max|ref|
PLANS = {"bits8": {"tile_bits_up": 8, "tile_bits_dw": 8}, "lds8": {"lds_budget_kb": 8}}
# Blocks of 8 low orbitals hold at most 70 columns: one pair per thread, a wave is live or dead.  Two, four and eight pairs per thread with
# only the LAST ones dead in some waves (the out-of-block code compiled for fewer live pairs) need blocks nearer the workgroup's size:
# 10 low orbitals give dw blocks of 210 / 252 / 210 columns, 11 give 462 / 462 (at 2, 4, 8 rows per tile: 1 - 4 pairs per thread).
# 256-thread workgroups on the blocks of 10: 2, 4 and EIGHT pairs per thread (two groups of four in the out-of-block phase, the second
# one partly dead).
BIG_PLANS = {"bits10": {"tile_bits_up": 10, "tile_bits_dw": 10}, "bits11": {"tile_bits_up": 10, "tile_bits_dw": 11},
             "bits10_t256": {"tile_bits_up": 10, "tile_bits_dw": 10, "threads_dw": 256}}
SECTORS = [(6, 6), (5, 7)]


@pytest.fixture(autouse=True)
def _experiments_gate():
    """the `debug` option is behind HXV_EXPERIMENTS=1"""
    old = os.environ.get("HXV_EXPERIMENTS")
    os.environ["HXV_EXPERIMENTS"] = "1"
    yield
    if old is None:
        os.environ.pop("HXV_EXPERIMENTS", None)
    else:
        os.environ["HXV_EXPERIMENTS"] = old


@lru_cache(maxsize=None)
def _model(kind):
    """Ns = 12, one orbital: the bath chain of hxv.models (real H) / an open chain with complex bonds and a few longer ones (complex H)"""
    from hxv import models
    from hxv.models import Model

    if kind == "real":
        return models.hm_1dchain(Nlat=4, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.05)
    Ns = 12
    rng = np.random.default_rng(1212)
    A = np.zeros((Ns, Ns), dtype=np.complex128)
    for i in range(Ns - 1):
        A[i, i + 1] = -(0.5 + rng.random()) * np.exp(1j * rng.uniform(0, 2 * np.pi))
    for i, j in ((0, 9), (2, 11), (3, 8), (1, 10), (5, 11)):   # bonds between the low and the high orbitals of either block split
        A[i, j] = rng.standard_normal() * 0.4 + 0.3j * rng.standard_normal()
    A = A + A.conj().T
    A[np.diag_indices(Ns)] = rng.standard_normal(Ns) * 0.3
    h = A.reshape(Ns, Ns, 1, 1, 1, 1)
    return Model(Ns, 1, 1, 0, h, np.zeros((Ns, Ns, 1, 1, 1, 1, 0)), np.zeros((Ns, 1, 1, 0)), Uloc=[1.7], xmu=0.1, hfmode=False, name="cchain12")


@lru_cache(maxsize=None)
def _case(kind, nup, ndw):
    """(oracle sector, complex input, H v, real input, H x): computed once, shared and never changed"""
    from oracle.oracle import OracleSector

    orc = OracleSector(_model(kind), nup, ndw)
    rng = np.random.default_rng(100 * nup + ndw)
    v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
    ref = orc.spMatVec_main(v)
    x = rng.standard_normal(orc.Dim)
    refx = orc.spMatVec_main(x.astype(np.complex128)) if kind == "real" else None
    return orc, v, ref, x, refx


def _relerr(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def _open(kind, nup, ndw, opts, **kw):
    import hxv

    sec = hxv.HxvSector.from_model(_model(kind), nup, ndw, **kw)
    for k, val in opts.items():
        sec.set_option(k, val)
    return sec


def _plan_facts(sec):
    return {k: sec.get_option(k) for k in ("nblocks_up", "nblocks_dw", "max_block_up", "max_block_dw", "max_outer_dw",
                                           "rows_per_tile", "cols_per_tile")}


@pytest.mark.gpu
@pytest.mark.parametrize("plan", sorted(PLANS) + sorted(BIG_PLANS))
@pytest.mark.parametrize("sector", SECTORS, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_complex_vectors_skip_gives_the_same_bits(built, kind, sector, plan):
    import torch

    nup, ndw = sector
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    dv = torch.tensor(v, device="cuda")
    checked, pairs, slots = 0, 0, 0
    for R in (2, 4, 8):
        for C in (2, 4):
            sec = _open(kind, nup, ndw, dict({**PLANS, **BIG_PLANS}[plan], rows_per_tile=R, cols_per_tile=C))
            facts = _plan_facts(sec)
            what = f"{kind} ({nup},{ndw}) {plan} {facts}"
            print(what)
            assert facts["nblocks_dw"] > 1 and facts["nblocks_up"] > 1, what
            if plan in PLANS:                             # smaller than the workgroup: waves without a live lane in every block
                assert facts["max_block_dw"] * R <= 1024 - 64, what
            pairs = max(pairs, -(-facts["max_block_dw"] * R // sec.get_option("threads_dw")))
            slots = max(slots, facts["max_outer_dw"])
            base = sec.apply_device(dv).clone()
            torch.cuda.synchronize()
            if (R, C) == (4, 4) or (R, C) == (8, 2):     # one or two settings per case meet the oracle
                err = _relerr(base.cpu().numpy(), ref)
                print(f"  oracle relerr {err:.2e}")
                assert err <= ORACLE_TOL, (what, err)
                checked += 1
            sec.set_option("debug", NO_SKIP)
            got = sec.apply_device(dv)
            torch.cuda.synchronize()
            assert torch.equal(got, base), f"{what}: debug {NO_SKIP} changes {int((got != base).sum())} elements"
            sec.close()
    assert checked >= 1
    assert plan in PLANS or pairs >= (8 if plan == "bits10_t256" else 2), f"{plan}: at most {pairs} pairs per thread"
    assert plan in BIG_PLANS or slots >= 3, f"at most {slots} out-of-block partners per block"


@pytest.mark.gpu
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("sector", SECTORS, ids=lambda s: "%d_%d" % s)
def test_real_vectors_skip_gives_the_same_bits(built, sector, plan):
    """REAL vectors (real H): pass B on row pairs (the complex kernel at half the rows) and on single rows"""
    import torch

    nup, ndw = sector
    orc, _, _, x, refx = _case("real", nup, ndw)
    assert np.abs(refx.imag).max() == 0.0
    dx = torch.tensor(x, device="cuda")
    for pairs in (1, 0):
        for R, C in ((2, 2), (4, 4), (8, 2), (4, 8)):
            sec = _open("real", nup, ndw, dict(PLANS[plan], rows_per_tile=R, cols_per_tile=C, real_dw_pairs=pairs))
            what = f"real vectors ({nup},{ndw}) {plan} pairs={pairs} {_plan_facts(sec)}"
            print(what)
            assert sec.real_vectors_available, what
            base = sec.apply_device_real(dx).clone()
            torch.cuda.synchronize()
            if (R, C) == (4, 4):
                err = _relerr(base.cpu().numpy(), refx.real)
                print(f"  oracle relerr {err:.2e}")
                assert err <= ORACLE_TOL, (what, err)
            sec.set_option("debug", NO_SKIP)
            assert sec.real_vectors_available, f"{what}: debug {NO_SKIP} blocks the real-vector mode"
            got = sec.apply_device_real(dx)
            torch.cuda.synchronize()
            assert torch.equal(got, base), f"{what}: debug {NO_SKIP} changes {int((got != base).sum())} elements"
            sec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_split_sector_on_three_thread_ranks(built, kind):
    """all-gather exchange, three thread ranks: the gather slots are not the identity, some blocks of a rank hold no local column (the
    early return), others are cut by the slab edge.  Pad rows carry NaN going in and a sentinel coming out."""
    import torch
    import hxv

    nup, ndw = 5, 7
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    V, Rf = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
    scale = np.abs(ref).max()
    P = 3

    def rank(r, group):
        sec = _open(kind, nup, ndw, {"tile_bits_up": 8, "tile_bits_dw": 8}, rank=r, nranks=P)
        assert sec.exchange_mode == "allgather"
        group.join(sec)
        lay = lc.lay_of(sec)
        c0 = sec.mpiIshift // sec.DimUp
        vl = lc.native(V[c0: c0 + sec.mpiQdw], lay).cuda()
        outs = []
        for bits in (0, NO_SKIP):
            sec.set_option("debug", bits)
            hv = lc.sentinel_like(sec.localElems, torch.complex128, "cuda")
            sec.apply_device_slab(vl, hv)
            torch.cuda.synchronize()
            outs.append((bits, hv))
        facts = _plan_facts(sec)
        sec.close()
        return c0, lay, outs, facts

    res = hxv.run_ranks(P, rank, transport="local")
    for r, (c0, lay, outs, facts) in enumerate(res):
        print(f"rank {r}: {facts}")
        assert facts["nblocks_dw"] > 1
        base = outs[0][1]
        lc.check_out(base, lay, Rf[c0: c0 + base.numel() // lay.pitch], scale, f"{kind} rank {r}/{P}")
        err = np.abs(lc.live(base, lay) - Rf[c0: c0 + base.numel() // lay.pitch]).max() / scale
        print(f"  oracle relerr {err:.2e}")
        assert err <= ORACLE_TOL, (r, err)
        for bits, hv in outs[1:]:
            assert torch.equal(lc._bits(hv), lc._bits(base)), f"{kind} rank {r}/{P}: debug {bits} changes the output (pad rows included)"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_pad_rows_and_unused_slots_stay_untouched(built, kind):
    """the default family of the layout contract on the many-block plan, shipped settings and the skip off: poisoned pad rows in
    the input (a read of one reaches a live row as NaN), a sentinel in every pad row of the output, bit-identical afterwards; unsplit and
    as rank 1 of 3 with a caller-gathered vector (the short ranks' unused column slot poisoned as well)"""
    import torch
    from hxv import dw_split

    for nup, ndw in ((6, 5),):                            # DimUp 924 -> pitch 928 (four pad rows per column), DimDw 792
        orc, v, ref, _, _ = _case(kind, nup, ndw)
        V, Rf = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
        scale = np.abs(ref).max()
        for P, r in ((1, 0), (3, 1)):
            for fam in ({"lds_budget_kb": 8}, {"lds_budget_kb": 8, "rows_per_tile": 8, "cols_per_tile": 2}, {"tile_bits_dw": 8, "rows_per_tile": 2}):
                sec = _open(kind, nup, ndw, fam, rank=r, nranks=P)
                lay = lc.lay_of(sec)
                q, c0 = dw_split(orc.DimDw, r, P)
                vin = lc.gathered(V, lay, P, "cuda")
                assert vin.numel() == sec.fullElems
                for bits in (0, NO_SKIP):
                    sec.set_option("debug", bits)
                    hv = lc.sentinel_like(sec.localElems, torch.complex128, "cuda")
                    sec.apply_device(vin, hv)
                    torch.cuda.synchronize()
                    lc.check_out(hv, lay, Rf[c0: c0 + q], scale, f"{kind} ({nup},{ndw}) rank {r}/{P} {fam} debug {bits}")
                sec.close()
