"""Pass B's two phase orders (csrc/hxv_tiled.hip, hxv_pass_dw's ORD): out-of-block sums in registers against sums added into the tile.

Where the plan allows it, pass B runs its out-of-block hops first, keeps their sums in registers through the in-block phase and finishes
every (row, column) pair in the thread that owns it: tile element + register sum, stored from the registers.  A thread's pairs are then the
ones of the blocked store -- columns counted from the block's aligned scratch group, so up to wc - 1 column positions in front of a block
are dead lanes -- and the plan must have room for them in its NP sweeps; eight pairs per thread, row-major scratch patches and blocks
without that room keep the earlier order.  Neither order changes a floating-point operation or its order, bit 8192 of the `debug` option
asks for the earlier one (DevTiles::debug), and the option "pass_b_order_last" reads back which one the last launch ran.  So for every plan
below the product with the shipped settings must equal, bit for bit, the product with the bit set, the read-back must name the order the
plan calls for, and one setting per case meets the CPU oracle.

Shapes: Ns = 12, sectors (6,6) and (5,7).
  * blocks of 8 low orbitals (16 blocks of 1 .. 70 columns): many unequal blocks, all smaller than the workgroup -- dead, partly live and
    live waves at one pair per thread.  Their starts are all EVEN (sums of binomials of 8), so blocks of 7 low orbitals (32 blocks of
    1 .. 35 columns) are run as well: their starts take every residue modulo 2, 4 and 8, which the test asserts from the basis itself.
  * blocks of 10 low orbitals (210 / 252 columns): with 256 threads at 2 and 4 rows, and 1024 threads at 4 and 8 rows, the workgroup's
    sweeps hold 256 columns -- 252 + 3 dead positions need the last sweep's last lanes at scratch groups of 4 columns, and do not fit at
    groups of 8 (the launcher must fall back); 256 threads at 8 rows are EIGHT pairs per thread (always the earlier order: the bit is a
    no-op).  Blocks of 11 low orbitals (462 columns): two pairs per thread at 4 rows, the last one dead in some waves; four at 8 rows, an
    instantiation that is not built with register sums (it would spill: the earlier order again).
  * 2 / 4 / 8 rows per tile, column-major and row-major patches, real and complex H, complex and real vectors, row pairs on and off.
  * a sector split over three thread ranks (gather slots that are not the identity, blocks cut by the slab edge so that the first or the
    last local column falls inside a block, blocks without a local column), pad rows poisoned going in and a sentinel coming out.
  * the row-panel product of the all-to-all exchange (natural-layout output: no dead positions), sentinel in its pad rows.
The blocked scratch itself is private to a handle: a store outside a block's own columns shows as a changed element of another block's
columns in the output (the comparison is bit for bit over the whole output, pad rows included)."""
import os
from functools import lru_cache
from math import comb

import numpy as np
import pytest

import test_gpu_layout_contract as lc   # (its layout helpers; importing the module collects none of its tests here)

OLD_ORDER = 8192                         # debug bit: pass B in the earlier phase order
ORACLE_TOL = 1e-13                       # max|got - ref| <= ORACLE_TOL * max|ref|
NS = 12
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
    rng = np.random.default_rng(1212)
    A = np.zeros((NS, NS), dtype=np.complex128)
    for i in range(NS - 1):
        A[i, i + 1] = -(0.5 + rng.random()) * np.exp(1j * rng.uniform(0, 2 * np.pi))
    for i, j in ((0, 9), (2, 11), (3, 8), (1, 10), (5, 11)):   # bonds between the low and the high orbitals of either block split
        A[i, j] = rng.standard_normal() * 0.4 + 0.3j * rng.standard_normal()
    A = A + A.conj().T
    A[np.diag_indices(NS)] = rng.standard_normal(NS) * 0.3
    h = A.reshape(NS, NS, 1, 1, 1, 1)
    return Model(NS, 1, 1, 0, h, np.zeros((NS, NS, 1, 1, 1, 1, 0)), np.zeros((NS, 1, 1, 0)), Uloc=[1.7], xmu=0.1, hfmode=False, name="cchain12")


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


def block_starts(ns, npart, lowbits):
    """starts of the prefix blocks of a spin's sorted basis (states that share their high ns - lowbits bits), from the basis itself"""
    st = [0]
    for hi in range(1 << (ns - lowbits)):
        k = npart - bin(hi).count("1")
        if 0 <= k <= lowbits:
            st.append(st[-1] + comb(lowbits, k))
    return st


def test_block_starts_of_the_basis():
    """the helper against an enumerated basis (CPU)"""
    for npart, low in ((6, 8), (7, 7), (5, 10)):
        states = [s for s in range(1 << NS) if bin(s).count("1") == npart]
        highs = [s >> low for s in states]
        st = [i for i in range(len(states)) if i == 0 or highs[i] != highs[i - 1]] + [len(states)]
        assert st == block_starts(NS, npart, low)


def _relerr(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def _open(kind, nup, ndw, opts, **kw):
    import hxv

    sec = hxv.HxvSector.from_model(_model(kind), nup, ndw, **kw)
    for k, val in opts.items():
        sec.set_option(k, val)
    return sec


def _facts(sec):
    return {k: sec.get_option(k) for k in ("nblocks_dw", "max_block_dw", "tile_bits_dw", "rows_per_tile", "cols_per_tile", "wt_cols",
                                           "threads_dw", "wt_colmajor")}


def _pairs_per_thread(max_block, rows, threads):
    """NP of the launcher: pairs per thread, rounded up to 1, 2, 4 or 8"""
    n = -(-max_block * rows // threads)
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8


def _regs_built(rows, npairs, real_h):
    """complex vectors: the instantiations built with the sums in registers (dw_regs_built of csrc/hxv_tiled.hip: the others would spill)"""
    if npairs > 4 or (rows == 8 and (npairs == 4 or (npairs == 2 and not real_h))) or (rows == 2 and npairs == 4 and not real_h):
        return False
    return True


def _expected_order(facts, real_h):
    """the order the plan calls for (complex vectors, blocked scratch of max(cols_per_tile, wt_cols) columns per group)"""
    rows = facts["rows_per_tile"]
    wc = max(min(4, facts["cols_per_tile"]), facts["wt_cols"])
    npairs = _pairs_per_thread(facts["max_block_dw"], rows, facts["threads_dw"])
    fits = (facts["max_block_dw"] + wc - 1) * rows <= npairs * facts["threads_dw"]
    return 1 if (_regs_built(rows, npairs, real_h) and fits and facts["wt_colmajor"]) else 0


def _both_orders(sec, apply, what, expect):
    """product with the shipped settings and with the bit set: the read-backs, and the same bits"""
    import torch

    assert sec.get_option("pass_b_order_last") == -1, what
    base = apply().clone()
    torch.cuda.synchronize()
    assert sec.get_option("pass_b_order_last") == expect, f"{what}: order {sec.get_option('pass_b_order_last')} ran, the plan calls for {expect}"
    sec.set_option("debug", OLD_ORDER)
    got = apply()
    torch.cuda.synchronize()
    assert sec.get_option("pass_b_order_last") == 0, what
    assert torch.equal(lc._bits(got), lc._bits(base)), f"{what}: debug {OLD_ORDER} changes {int((lc._bits(got) != lc._bits(base)).sum())} doubles"
    sec.set_option("debug", 0)
    return base


# (name, plan options, what the shape is there for)
SMALL = {"bits8": {"tile_bits_up": 8, "tile_bits_dw": 8}, "bits7": {"tile_bits_up": 8, "tile_bits_dw": 7}}
GROUPS = ((4, 4), (2, 2), (8, 4))        # (wt_cols, cols_per_tile): scratch groups of 4, 2 and 8 columns


@pytest.mark.gpu
@pytest.mark.parametrize("plan", sorted(SMALL))
@pytest.mark.parametrize("sector", SECTORS, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_block_starts_at_every_misalignment(built, kind, sector, plan):
    import torch

    nup, ndw = sector
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    dv = torch.tensor(v, device="cuda")
    checked = 0
    for wt_cols, C in GROUPS:
        for R in (2, 4, 8):
            for cm in (1, 0) if (wt_cols, R) == (4, 4) else (1,):
                sec = _open(kind, nup, ndw, dict(SMALL[plan], rows_per_tile=R, cols_per_tile=C, wt_cols=wt_cols, wt_colmajor=cm))
                facts = _facts(sec)
                what = f"{kind} ({nup},{ndw}) {plan} {facts}"
                print(what)
                st = block_starts(NS, ndw, facts["tile_bits_dw"])
                assert facts["nblocks_dw"] == len(st) - 1 and facts["max_block_dw"] == max(b - a for a, b in zip(st, st[1:])), what
                res = sorted({s % wt_cols for s in st[:-1]})
                print(f"  block starts modulo {wt_cols}: {res}")
                if plan == "bits7":
                    assert res == list(range(wt_cols)), what
                assert facts["max_block_dw"] * R <= 1024 - 64, what      # waves without a live lane in every block
                base = _both_orders(sec, lambda: sec.apply_device(dv), what, 1 if cm else 0)
                if R == 4:
                    err = _relerr(base.cpu().numpy(), ref)
                    print(f"  oracle relerr {err:.2e}")
                    assert err <= ORACLE_TOL, (what, err)
                    checked += 1
                sec.close()
    assert checked >= 3


# blocks near the workgroup's capacity: (plan options, rows per tile, pairs per thread)
BIG = (({"tile_bits_dw": 10, "threads_dw": 1024}, 4, 1), ({"tile_bits_dw": 10, "threads_dw": 1024}, 8, 2),
       ({"tile_bits_dw": 10, "threads_dw": 256}, 2, 2), ({"tile_bits_dw": 10, "threads_dw": 256}, 4, 4),
       ({"tile_bits_dw": 10, "threads_dw": 256}, 8, 8), ({"tile_bits_dw": 11, "threads_dw": 1024}, 8, 4),
       ({"tile_bits_dw": 11, "threads_dw": 1024}, 4, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("sector", SECTORS, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_last_lanes_of_the_last_sweep_and_the_fallback(built, kind, sector):
    import torch

    nup, ndw = sector
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    dv = torch.tensor(v, device="cuda")
    tight = fallback = eight = 0
    for opts, R, npairs in BIG:
        for wt_cols in (4, 8):
            sec = _open(kind, nup, ndw, dict(opts, tile_bits_up=10, rows_per_tile=R, wt_cols=wt_cols))
            facts = _facts(sec)
            what = f"{kind} ({nup},{ndw}) {facts}"
            T, mb = facts["threads_dw"], facts["max_block_dw"]
            assert _pairs_per_thread(mb, R, T) == npairs, what
            room = npairs * T // R - (mb + wt_cols - 1)          # column positions left in the last sweep
            expect = _expected_order(facts, kind == "real")
            print(what, f"pairs {npairs} room {room} order {expect}")
            assert expect == (1 if _regs_built(R, npairs, kind == "real") and room >= 0 else 0), what
            if expect and room < 64 // R:
                tight += 1                                       # the last sweep's last wave owns live columns
            if npairs <= 4 and room < 0:
                fallback += 1
            if npairs == 8:
                eight += 1
            base = _both_orders(sec, lambda: sec.apply_device(dv), what, expect)
            if wt_cols == 4:
                err = _relerr(base.cpu().numpy(), ref)
                print(f"  oracle relerr {err:.2e}")
                assert err <= ORACLE_TOL, (what, err)
            sec.close()
    assert tight >= 3 and fallback >= 4 and eight == 2, (tight, fallback, eight)


@pytest.mark.gpu
@pytest.mark.parametrize("sector", SECTORS, ids=lambda s: "%d_%d" % s)
def test_real_vectors(built, sector):
    """REAL vectors (real H): pass B on row pairs (the complex kernel at half the rows) and on single rows; scratch groups of
    2 * wt_cols real columns"""
    import torch

    nup, ndw = sector
    orc, _, _, x, refx = _case("real", nup, ndw)
    assert np.abs(refx.imag).max() == 0.0
    dx = torch.tensor(x, device="cuda")
    for pairs in (1, 0):
        for R, C, cm in ((2, 2, 1), (4, 4, 1), (8, 2, 1), (4, 8, 1), (4, 4, 0)):
            sec = _open("real", nup, ndw, dict(SMALL["bits7"], rows_per_tile=R, cols_per_tile=C, real_dw_pairs=pairs, wt_colmajor=cm))
            what = f"real vectors ({nup},{ndw}) pairs={pairs} {_facts(sec)}"
            print(what)
            assert sec.real_vectors_available, what
            # (blocks of at most 35 columns in sweeps of 128 and more: room for every group width; row pairs need column-major patches)
            base = _both_orders(sec, lambda: sec.apply_device_real(dx), what, 1 if (cm or pairs) else 0)
            if (R, C) == (4, 4):
                err = _relerr(base.cpu().numpy(), refx.real)
                print(f"  oracle relerr {err:.2e}")
                assert err <= ORACLE_TOL, (what, err)
            sec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_split_sector_on_three_thread_ranks(built, kind):
    """all-gather exchange, three thread ranks: the gather slots are not the identity, some blocks of a rank hold no local column (the
    early return), others are cut by the slab edge (the first / last local column lies inside a block, and the store's aligned mapping
    starts before the slab).  Pad rows carry NaN going in and a sentinel coming out."""
    import torch
    import hxv

    nup, ndw = 5, 7
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    V, Rf = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
    scale = np.abs(ref).max()
    P = 3

    def ranks_of(low):
        def rank(r, group):
            sec = _open(kind, nup, ndw, {"tile_bits_up": 8, "tile_bits_dw": low}, rank=r, nranks=P)
            assert sec.exchange_mode == "allgather"
            group.join(sec)
            lay = lc.lay_of(sec)
            c0 = sec.mpiIshift // sec.DimUp
            st = block_starts(NS, ndw, low)
            cut = [a for a, b in zip(st, st[1:]) if a < c0 < b or a < c0 + sec.mpiQdw < b]
            vl = lc.native(V[c0: c0 + sec.mpiQdw], lay).cuda()
            outs = []
            for bits in (0, OLD_ORDER):
                sec.set_option("debug", bits)
                hv = lc.sentinel_like(sec.localElems, torch.complex128, "cuda")
                sec.apply_device_slab(vl, hv)
                torch.cuda.synchronize()
                outs.append((sec.get_option("pass_b_order_last"), hv))
            sec.close()
            return c0, lay, outs, cut

        return rank

    ncut = 0
    for low in (7, 8):
        for r, (c0, lay, outs, cut) in enumerate(hxv.run_ranks(P, ranks_of(low), transport="local")):
            ncut += len(cut)
            (order, base), (order_old, hv) = outs
            what = f"{kind} rank {r}/{P} blocks of {low} low orbitals"
            assert (order, order_old) == (1, 0), (what, order, order_old)
            lc.check_out(base, lay, Rf[c0: c0 + base.numel() // lay.pitch], scale, what)
            err = np.abs(lc.live(base, lay) - Rf[c0: c0 + base.numel() // lay.pitch]).max() / scale
            print(f"{what}: oracle relerr {err:.2e}")
            assert err <= ORACLE_TOL, (what, err)
            assert torch.equal(lc._bits(hv), lc._bits(base)), f"{what}: debug {OLD_ORDER} changes the output (pad rows included)"
    assert ncut >= 1, "no block is cut by a slab edge"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_row_panel_product_of_the_all_to_all_exchange(built, kind):
    """hxv_apply_dw_panel: pass B alone with a natural-layout output (no scratch groups, no dead positions), odd and even row counts"""
    import scipy.sparse as sp
    import torch
    import hxv

    nup, ndw = 5, 7
    orc, v, _, _, _ = _case(kind, nup, ndw)
    du, dd = orc.DimUp, orc.DimDw
    V = v.reshape(dd, du)
    rp, cols, vals = orc.csr("dw")
    Y = sp.csr_matrix((vals, cols - 1, rp), shape=(dd, dd)) @ V        # (v H_dw^T) in the [column][row] layout
    yscale = np.abs(Y).max()
    for nr, u0, opts in ((37, 3, {"tile_bits_dw": 7}), (64, 100, {"tile_bits_dw": 10, "threads_dw": 256})):
        pan = hxv.HxvSector.dw_panel(_model(kind), nup, ndw, nr)
        for k, val in opts.items():
            pan.set_option(k, val)
        lay = lc.SimpleNamespace(dimup=nr, pitch=pan.pitch, perm=None, sign=None)
        x = lc.native(V[:, u0:u0 + nr], lay).cuda()
        outs = []
        for bits in (0, OLD_ORDER):
            pan.set_option("debug", bits)
            y = lc.sentinel_like(pan.localElems, torch.complex128, "cuda")
            pan.apply_dw_panel(x, y)
            torch.cuda.synchronize()
            outs.append((y, pan.get_option("pass_b_order_last")))
        what = f"dw panel {kind} ({nup},{ndw}) nrows={nr} {opts}"
        assert (outs[0][1], outs[1][1]) == (1, 0), (what, outs[0][1], outs[1][1])
        lc.check_out(outs[0][0], lay, Y[:, u0:u0 + nr], yscale, what)
        err = np.abs(lc.live(outs[0][0], lay) - Y[:, u0:u0 + nr]).max() / yscale
        print(f"{what}: oracle relerr {err:.2e}")
        assert err <= ORACLE_TOL, (what, err)
        assert torch.equal(lc._bits(outs[1][0]), lc._bits(outs[0][0])), f"{what}: debug {OLD_ORDER} changes the output (pad rows included)"
        pan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "cplx"])
def test_pad_rows_and_unused_slots_stay_untouched(built, kind):
    """the default family of the layout contract on many-block plans, both orders: poisoned pad rows in the input (a read of one reaches a
    live row as NaN), a sentinel in every pad row of the output, bit-identical afterwards; unsplit and as rank 1 of 3 with a
    caller-gathered vector (the short ranks' unused column slot poisoned as well)"""
    import torch
    from hxv import dw_split

    nup, ndw = 6, 5                                           # DimUp 924 -> pitch 928 (four pad rows per column), DimDw 792
    orc, v, ref, _, _ = _case(kind, nup, ndw)
    V, Rf = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
    scale = np.abs(ref).max()
    for P, r in ((1, 0), (3, 1)):
        for fam in ({"tile_bits_dw": 7}, {"tile_bits_dw": 7, "rows_per_tile": 8, "cols_per_tile": 2, "wt_cols": 8}, {"tile_bits_dw": 8, "rows_per_tile": 2}):
            sec = _open(kind, nup, ndw, fam, rank=r, nranks=P)
            lay = lc.lay_of(sec)
            q, c0 = dw_split(orc.DimDw, r, P)
            vin = lc.gathered(V, lay, P, "cuda")
            assert vin.numel() == sec.fullElems
            outs = []
            for bits in (0, OLD_ORDER):
                sec.set_option("debug", bits)
                hv = lc.sentinel_like(sec.localElems, torch.complex128, "cuda")
                sec.apply_device(vin, hv)
                torch.cuda.synchronize()
                what = f"{kind} ({nup},{ndw}) rank {r}/{P} {fam} debug {bits}"
                assert sec.get_option("pass_b_order_last") == (0 if bits else 1), what
                lc.check_out(hv, lay, Rf[c0: c0 + q], scale, what)
                outs.append(hv)
            assert torch.equal(lc._bits(outs[0]), lc._bits(outs[1])), f"{kind} rank {r}/{P} {fam}: the orders differ"
            sec.close()
