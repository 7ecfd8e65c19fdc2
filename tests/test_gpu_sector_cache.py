"""The sector-image cache on the device (csrc/hxv_cache.cpp): no stale hit, no state shared by handles.

A cache hit hands a new handle the host description, the default tile plan and every device table of an earlier open; a second open of a
sector that is still open shares them live.  If the key forgot one input, or one handle wrote into what its siblings share, the result
would be a correct product of the wrong Hamiltonian.  So: every product here is compared with the CPU oracle of the model that was
OPENED (OracleSector.spMatVec_main, 1e-13 relative to max|ref|, the project's H x V tolerance), after the cache was given every chance
to answer with the image of another model; and bit-identity (torch.equal / np.array_equal) wherever two handles must run the same tables.
The key itself, the LRU policy, the cap and the threads are checked on the CPU by tests/test_host_cache_check.py.

Shapes, the smallest at which the code can still go wrong:
  M1  hm_1dchain(Nlat=2, Nbath=3)                                          sector (4,4)  real H, 70 x 70 (S1 of test_gpu_options.py)
  M2  bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.4, Jh=0.1, Jx=0.25, Jp=-0.1)       sector (4,3)  complex H, Norb 2, a bath, spH0nd; Ns 8, 70 x 56
  M3  hm_2dsquare(Nbath=2, xmu=0.1)                                        sector (6,5)  opened with the row-order hooks of
      test_gpu_row_order.py (HXV_ROW_ORDER_MIN_DIMUP=16, HXV_ROW_ORDER_BITS=8): the image holds a non-identity row order
Every test starts and ends with sector_cache_clear() and reads sector_cache_stats() as differences."""
import copy
import os
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-13          # H x V against the oracle, relative to max|ref|
STALE = 1e-6         # a mutant that enters H moves the oracle's product by more than this (relative): a stale hit cannot pass TOL
ROOT = Path(__file__).resolve().parent.parent
# the plan read-backs of tests/test_gpu_options.py, restated
PLAN_STATS = ("tile_bits_up", "tile_bits_dw", "nblocks_up", "nblocks_dw", "n_in_up", "n_out_up", "n_in_dw", "n_out_dw", "k_in_up", "k_out_up", "k_in_dw",
              "k_out_dw", "max_block_up", "max_block_dw", "max_outer_up", "max_outer_dw", "table_classes_up", "table_classes_dw", "job_up_active")


# ---- models, mutants, references ----------------------------------------------------------------------------------------------------------
def _base(case):
    from hxv import models

    if case == "M1":
        return models.hm_1dchain(Nlat=2, Nbath=3), (4, 4)
    if case == "M2":
        return models.bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.4, Jh=0.1, Jx=0.25, Jp=-0.1), (4, 3)
    return models.hm_2dsquare(Nbath=2, xmu=0.1), (6, 5)


def mutants(case):
    """[(name, model, sector, enters H)]: deep copies of the base with ONE change each"""
    base, (nup, ndw) = _base(case)
    out = []

    def add(name, change, enters=True, sector=(nup, ndw)):
        m = copy.deepcopy(base)
        change(m)
        out.append((name, m, sector, enters))

    def attr(field, delta):
        return lambda m: setattr(m, field, getattr(m, field) + delta)

    def elem(field, index, delta):
        def change(m):
            getattr(m, field)[index] += delta
        return change

    def uloc(o):
        return elem("Uloc", o, 0.5)

    L, S, O, B = base.Nlat, base.Nspin, base.Norb, base.Nbath
    for o in range(2):
        add(f"Uloc[{o}]", uloc(o), enters=o < O)
    for field in ("Ust", "Jh", "Jx", "Jp"):
        add(field, attr(field, 0.3), enters=O > 1)
    add("xmu", attr("xmu", 0.3))
    add("hfmode", lambda m: setattr(m, "hfmode", not m.hfmode))
    first6, last6 = (0,) * 6, (L - 1, L - 1, S - 1, S - 1, O - 1, O - 1)
    add("impHloc first diagonal", elem("impHloc", first6, 0.3))
    add("impHloc last diagonal", elem("impHloc", last6, 0.3))

    def hop(delta):
        def change(m):
            m.impHloc[0, 1, 0, 0, 0, 0] += delta
            m.impHloc[1, 0, 0, 0, 0, 0] += np.conj(delta)
        return change

    add("impHloc hopping", hop(0.2))
    if case == "M2":
        add("impHloc hopping, imaginary part", hop(0.2j))
    add("Hbath first", elem("Hbath", first6 + (0,), 0.3))
    add("Hbath last", elem("Hbath", last6 + (B - 1,), 0.3))
    add("Vbath first", elem("Vbath", (0, 0, 0, 0), 0.2))
    add("Vbath last", elem("Vbath", (L - 1, S - 1, O - 1, B - 1), 0.2))
    if nup != ndw:
        add("sector (ndw,nup)", lambda m: None, sector=(ndw, nup))
    add("sector (nup-1,ndw)", lambda m: None, sector=(nup - 1, ndw))
    return out


_VEC, _REF = {}, {}


def _vec(dim):
    if dim not in _VEC:
        rng = np.random.default_rng(1000 + dim)
        _VEC[dim] = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    return _VEC[dim]


def _oracle(tag, model, sector):
    """the oracle's product of the test vector of that dimension, computed once per tag and never changed"""
    if tag not in _REF:
        from oracle.oracle import OracleSector

        orc = OracleSector(model, *sector)
        ref = orc.spMatVec_main(_vec(orc.Dim))
        ref.setflags(write=False)
        _REF[tag] = ref
        orc.close()
    return _REF[tag]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _delta(s1, s0):
    return {k: s1[k] - s0[k] for k in ("hits", "misses", "entries")}


def _product(sec, kernel=None):
    """(padded device result: the bits; contiguous numpy result in the reference's order) of the test vector on this handle"""
    import torch

    if kernel is not None:
        sec.set_option("kernel", kernel)       # (sets the handle's kernel choice only: no plan is built)
    dv = sec.pad(torch.from_numpy(_vec(sec.Dim)).cuda())
    hv = sec.apply_device(dv)
    torch.cuda.synchronize()
    return hv, sec.unpad(hv).cpu().numpy()


def _open_counted(model, sector, **kw):
    """-> (handle, open_cache_hit, change of the cache's counters over the open)"""
    import hxv

    s0 = hxv.sector_cache_stats()
    sec = hxv.HxvSector.from_model(model, *sector, **kw)
    return sec, sec.get_option("open_cache_hit"), _delta(hxv.sector_cache_stats(), s0)


def _three_paths(model, sector, ref, what, expect_hit, bits=3):
    """Open, count, and run the three product paths: the handle as opened (the image's own device tables) with the tile kernels and with
    the naive kernel, then a second handle with `bits` block bits for both spins (a plan built from the shared host description, several
    blocks).  Everything is evaluated first and asserted together, so a failure shows the hit flag AND the errors.  -> the three results' bits"""
    sec, hit, d = _open_counted(model, sector)
    try:
        errs, out = [], []
        for kern in (1, 0):
            hv, got = _product(sec, kern)
            errs.append(_rel(got, ref))
            out.append(hv)
        times = tuple(sec.get_option(n) for n in ("open_us_host", "open_us_plan", "open_us_upload"))
    finally:
        sec.close()
    sec2, hit2, d2 = _open_counted(model, sector)
    try:
        sec2.set_option("tile_bits_up", bits)
        sec2.set_option("tile_bits_dw", bits)
        nblocks = sec2.get_option("nblocks_up")
        hv, got = _product(sec2)
        errs.append(_rel(got, ref))
        out.append(hv)
    finally:
        sec2.close()
    print(f"{what}: hit {hit}, counters {d}, errors tiled {errs[0]:.2e} naive {errs[1]:.2e} {bits}-bit plan {errs[2]:.2e}")
    want = {"hits": 1, "misses": 0, "entries": 0} if expect_hit else {"hits": 0, "misses": 1, "entries": 1}
    assert (hit, d) == (int(expect_hit), want) and max(errs) <= TOL, (what, "open_cache_hit", hit, d, "errors", errs)
    if expect_hit:
        assert times == (0, 0, 0), (what, times)
    assert (hit2, d2) == (1, {"hits": 1, "misses": 0, "entries": 0}), (what, "second handle", hit2, d2)
    assert nblocks > 1, (what, nblocks)
    return out


@pytest.fixture
def clean_cache(built):
    import hxv

    hxv.sector_cache_clear()
    live = hxv.live_handles()
    yield hxv
    hxv.sector_cache_clear()
    assert hxv.live_handles() == live


# ---- a. no stale hit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["M1", "M2"])
def test_a_changed_model_is_never_served_a_cached_image(clean_cache, case):
    """The base is opened and left in the cache; then one mutant at a time (every field of the model that hxv_model carries, first and
    last array elements, the sector): each must MISS and give the product of its own Hamiltonian on all three paths, and the base,
    re-opened after it, must HIT, cost nothing and give the bits of its first open.  For every mutant that enters H the oracle's products
    of mutant and base differ by more than 1e-6 on the test vector (asserted), so a stale hit cannot pass the 1e-13 comparison; the
    mutants that do not enter H (Ust, Jh, Jx, Jp and Uloc[1] at Norb = 1) must miss and be right all the same."""
    hxv = clean_cache
    base, sector = _base(case)
    ref0 = _oracle((case, "base"), base, sector)
    bits0 = _three_paths(base, sector, ref0, f"{case} base", expect_hit=False)
    import torch

    for name, model, sec_m, enters in mutants(case):
        ref = _oracle((case, name), model, sec_m)
        if enters and ref.shape == ref0.shape:
            moved = _rel(ref, ref0)
            assert moved > STALE, (case, name, "the mutation moves the oracle's product by only", moved)
        _three_paths(model, sec_m, ref, f"{case} {name}", expect_hit=False)
        again = _three_paths(base, sector, ref0, f"{case} base after {name}", expect_hit=True)
        assert all(torch.equal(a, b) for a, b in zip(again, bits0)), (case, name, "the re-opened base gives other bits")
    assert hxv.sector_cache_stats()["entries"] == 1 + len(mutants(case))


def test_dmft_loop_new_baths_miss_the_old_bath_hits(clean_cache, monkeypatch):
    """M3 under the row-order hooks, baths A, B, A, C with each handle closed before the next open: miss, miss, hit, miss; every product
    (the image's own tables, both kernels, and an 8-bit plan) matches its own bath's oracle, the second A is bit-identical to the first,
    and all four images hold a non-identity row order."""
    import torch

    hxv = clean_cache
    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    monkeypatch.setenv("HXV_ROW_ORDER_BITS", "8")
    hxv.sector_cache_clear()
    a, sector = _base("M3")
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    b.Vbath *= 1.1                                    # a new hybridisation
    b.Hbath[0, 0, 0, 0, 0, 0, 0] += 0.05              # ... and one moved level
    c.Hbath[..., 1] *= 0.9                            # the second replica rescaled
    bits = {}
    for name, model, expect_hit in (("A", a, False), ("B", b, False), ("A", a, True), ("C", c, False)):
        ref = _oracle(("M3", name), model, sector)
        if name != "A":
            assert _rel(ref, _oracle(("M3", "A"), a, sector)) > STALE, name
        out = _three_paths(model, sector, ref, f"M3 bath {name}", expect_hit=expect_hit, bits=8)
        if name in bits:
            assert all(torch.equal(x, y) for x, y in zip(out, bits[name])), "the second A gives other bits than the first"
        bits[name] = out
        sec = hxv.HxvSector.from_model(model, *sector)       # (a hit by now: only to read the image's row order)
        perm = sec.row_perm
        sec.close()
        assert perm is not None and sorted(perm.tolist()) == list(range(len(perm))) and not np.array_equal(perm, np.arange(len(perm))), name


# ---- b. handles that share an image do not see each other -------------------------------------------------------------------------------------
def _readbacks(sec):
    return {n: sec.get_option(n) for n in PLAN_STATS}


@pytest.mark.parametrize("case", ["M1", "M2"])
def test_options_set_on_one_handle_do_not_reach_its_siblings(clean_cache, case):
    """A and B share one image (B opened while A is open: a hit).  Every plan option set on A builds A's own plan: A reads the value back
    and matches the oracle, while B's product bits, plan read-backs, kernel, fold_nd and real-vector availability stay what they were;
    closing A frees A's tables and leaves B's bits alone; C, opened afterwards as a hit, gets the default plan: B's read-backs, B's bits."""
    import torch

    hxv = clean_cache
    model, sector = _base(case)
    ref = _oracle((case, "base"), model, sector)
    A, hit_a, d_a = _open_counted(model, sector)
    B, hit_b, d_b = _open_counted(model, sector)
    C = None
    try:
        assert (hit_a, d_a) == (0, {"hits": 0, "misses": 1, "entries": 1}) and (hit_b, d_b) == (1, {"hits": 1, "misses": 0, "entries": 0})
        # both handles report the image's tables: their own scratch is the same size, the tables are shared
        table_bytes = A.stats()["device_bytes"]
        assert table_bytes > 0 and B.stats()["device_bytes"] == table_bytes
        assert hxv.sector_cache_stats()["bytes"] > 0
        bits_b, got = _product(B)
        assert _rel(got, ref) <= TOL
        state_b = (_readbacks(B), B.get_option("kernel"), B.get_option("fold_nd"), B.real_vectors_available)
        defaults = _readbacks(A)
        assert defaults == state_b[0]
        settings = [("tile_bits_up", 3), ("tile_bits_dw", 3), ("cols_per_tile", 2), ("rows_per_tile", 2), ("kernel", 0), ("kernel", 1)]
        if case == "M2":
            settings += [("fold_nd", 0), ("job_up", 0)]
        for name, value in settings:
            A.set_option(name, value)
            assert A.get_option(name) == value, (case, name, "A does not read its own setting back", A.get_option(name))
            _, got = _product(A)
            assert _rel(got, ref) <= TOL, (case, name, value, "A", _rel(got, ref))
            hv, _ = _product(B)
            assert torch.equal(hv, bits_b), (case, name, value, "B's product changed")
            assert (_readbacks(B), B.get_option("kernel"), B.get_option("fold_nd"), B.real_vectors_available) == state_b, (case, name, value)
        assert A.get_option("nblocks_up") > 1 and A.get_option("nblocks_dw") > 1          # (A did run a plan of its own, with several blocks)
        assert A.stats()["device_bytes"] > B.stats()["device_bytes"] >= table_bytes          # (A's plans are A's own allocations)
        A.close()
        hv, _ = _product(B)
        assert torch.equal(hv, bits_b), (case, "B's product changed when A was closed")
        C, hit_c, d_c = _open_counted(model, sector)
        assert (hit_c, d_c) == (1, {"hits": 1, "misses": 0, "entries": 0})
        assert _readbacks(C) == state_b[0], (case, "C did not get the default plan", _readbacks(C), state_b[0])
        assert (C.get_option("kernel"), C.get_option("fold_nd"), C.real_vectors_available) == state_b[1:]
        hv, got = _product(C)
        assert torch.equal(hv, bits_b) and _rel(got, ref) <= TOL
    finally:
        for s in (A, B, C):
            if s is not None:
                s.close()


def test_lazily_built_tables_of_the_image_serve_the_next_handle(clean_cache):
    """M1: A runs observables_accumulate and cluster_dm_accumulate on a normalised vector, which builds their tables inside the image,
    and is closed; B opens as a hit and returns bit-identical records.  Both equal the CPU restatements (tests/observables_ref.py
    record_numpy, tests/cluster_dm_ref.py vectorised) to 1e-13, the bound of tests/test_gpu_observables.py and test_gpu_cluster_dm.py."""
    import torch
    from cluster_dm_ref import vectorised
    from observables_ref import record_numpy

    model, sector = _base("M1")
    v = _vec(70 * 70) / np.linalg.norm(_vec(70 * 70))
    recs = []
    for expect_hit in (0, 1):
        sec, hit, _ = _open_counted(model, sector)
        try:
            assert hit == expect_hit and sec.Dim == v.size
            dv = sec.pad(torch.from_numpy(v).cuda()).contiguous()
            recs.append((sec.observables_record(dv, 0.7), sec.cluster_dm(dv, 0.7), sec.maps()))
        finally:
            sec.close()
    (rec_a, cdm_a, (mu, md)), (rec_b, cdm_b, _) = recs
    assert np.array_equal(rec_a, rec_b) and np.array_equal(cdm_a, cdm_b)
    assert np.abs(rec_a - record_numpy(model, mu, md, v, 0.7)).max() < 1e-13
    assert np.abs(cdm_a - vectorised(model, mu, md, v, 0.7)).max() < 1e-13


# ---- c. lifetimes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_closed", ["A", "B"])
def test_clear_under_an_open_handle(clean_cache, first_closed):
    """M1: sector_cache_clear() while A is open leaves A's product bits alone (A keeps its image alive); the next open, B, is a miss
    with an image of its own and gives the same bits; closing the two in either order brings live_handles() back, and the cache ends
    with B's image alone."""
    import torch

    hxv = clean_cache
    model, sector = _base("M1")
    ref = _oracle(("M1", "base"), model, sector)
    live0 = hxv.live_handles()
    A, hit_a, d_a = _open_counted(model, sector)
    B = None
    try:
        assert (hit_a, d_a["misses"], d_a["entries"]) == (0, 1, 1)
        bits_a, got = _product(A)
        assert _rel(got, ref) <= TOL
        hxv.sector_cache_clear()
        st = hxv.sector_cache_stats()
        assert (st["entries"], st["bytes"]) == (0, 0)
        hv, _ = _product(A)
        assert torch.equal(hv, bits_a), "clear changed the product of an open handle"
        B, hit_b, d_b = _open_counted(model, sector)
        assert (hit_b, d_b) == (0, {"hits": 0, "misses": 1, "entries": 1})
        assert hxv.live_handles() == live0 + 2
        hv_b, got = _product(B)
        assert _rel(got, ref) <= TOL and torch.equal(hv_b, bits_a)
        hv, _ = _product(A)
        assert torch.equal(hv, bits_a)
        first, second = (A, B) if first_closed == "A" else (B, A)
        first.close()
        assert hxv.live_handles() == live0 + 1
        hv, _ = _product(second)
        assert torch.equal(hv, bits_a), "closing one handle changed the other's product"
        second.close()
        assert hxv.live_handles() == live0
        st = hxv.sector_cache_stats()
        assert st["entries"] == 1 and st["bytes"] > 0        # B's image; A's died with A
        C, hit_c, _ = _open_counted(model, sector)
        hv, _ = _product(C)
        C.close()
        assert hit_c == 1 and torch.equal(hv, bits_a)
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


# ---- d. the split, the exchange and the device in the key -----------------------------------------------------------------------------------
def test_split_and_exchange_are_part_of_the_key(clean_cache):
    """M1 unsplit, as ranks 0..1 of 2 and as ranks 0..2 of 3 (thread ranks, transport local).  Under the all-gather every open misses and
    every rank's product through its exchange matches the oracle's rows of that rank; the same opens again all hit with the same bits;
    with the halo exchange the same (rank, nranks) pairs miss again and are right; back under the all-gather they hit again."""
    import torch

    hxv = clean_cache
    model, sector = _base("M1")
    ref = _oracle(("M1", "base"), model, sector)
    v = _vec(ref.size)

    def round_(exchange, expect_hit):
        hxv.set_exchange_default(exchange)
        out = {}
        s0 = hxv.sector_cache_stats()
        sec, hit, _ = _open_counted(model, sector)
        hv, got = _product(sec)
        sec.close()
        assert _rel(got, ref) <= TOL
        out[(0, 1)] = (hit, hv)
        for nranks in (2, 3):
            def rank(r, group):
                sec = hxv.HxvSector.from_model(model, *sector, rank=r, nranks=nranks)
                try:
                    hit = sec.get_option("open_cache_hit")
                    mode = sec.exchange_mode
                    group.join(sec)
                    lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
                    hv = sec.apply_device_slab(sec.pad(torch.from_numpy(v[lo:hi].copy()).cuda(), sec.mpiQdw))
                    torch.cuda.synchronize()
                    return hit, mode, float(np.abs(sec.unpad(hv).cpu().numpy() - ref[lo:hi]).max() / np.abs(ref).max()), hv
                finally:
                    sec.close()

            for r, (hit, mode, err, hv) in enumerate(hxv.run_ranks(nranks, rank, transport="local")):
                assert mode == exchange and err <= TOL, (exchange, r, nranks, mode, err)
                out[(r, nranks)] = (hit, hv)
        d = _delta(hxv.sector_cache_stats(), s0)
        split = [k for k in out if k[1] > 1]
        # the unsplit sector has no exchange: its key does not change with the default
        hits = {k: h for k, (h, _) in out.items()}
        want_split = 1 if expect_hit else 0
        assert all(hits[k] == want_split for k in split), (exchange, hits)
        return out, d

    try:
        first, d = round_("allgather", False)
        assert first[(0, 1)][0] == 0 and d == {"hits": 0, "misses": 6, "entries": 6}, d
        again, d = round_("allgather", True)
        assert again[(0, 1)][0] == 1 and d == {"hits": 6, "misses": 0, "entries": 0}, d
        assert all(torch.equal(again[k][1], first[k][1]) for k in first)
        halo, d = round_("halo", False)
        assert halo[(0, 1)][0] == 1 and d == {"hits": 1, "misses": 5, "entries": 5}, d
        back, d = round_("allgather", True)
        assert d == {"hits": 6, "misses": 0, "entries": 0}, d
        assert all(torch.equal(back[k][1], first[k][1]) for k in first)
    finally:
        hxv.set_exchange_default("allgather")


# ---- e. the same key from several threads at once ---------------------------------------------------------------------------------------------
def test_four_threads_open_the_same_sector_at_once(clean_cache):
    """Four threads open M1 behind a barrier, run one product each and close: all four match the oracle; between one and four of them
    built the image (the others hit), one entry stays, no handle is left.  Run once: the race check is the host program under TSan."""
    import torch

    hxv = clean_cache
    model, sector = _base("M1")
    ref = _oracle(("M1", "base"), model, sector)
    _vec(ref.size)
    live0 = hxv.live_handles()
    s0 = hxv.sector_cache_stats()
    barrier = threading.Barrier(4, timeout=60)
    res, errs = [None] * 4, []

    def work(i):
        try:
            barrier.wait()
            sec = hxv.HxvSector.from_model(model, *sector)
            try:
                hv, got = _product(sec)
                res[i] = (sec.get_option("open_cache_hit"), _rel(got, ref), hv)
            finally:
                sec.close()
        except BaseException as e:  # noqa: BLE001 (reported below)
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    d = _delta(hxv.sector_cache_stats(), s0)
    assert all(r[1] <= TOL for r in res), [r[1] for r in res]
    assert all(torch.equal(r[2], res[0][2]) for r in res)
    assert 1 <= d["misses"] <= 4 and d["hits"] == 4 - d["misses"] and d["entries"] == 1, d
    assert sum(r[0] for r in res) == d["hits"]
    assert hxv.live_handles() == live0


# ---- f. the cap and the off switch on the device --------------------------------------------------------------------------------------------
_CHILD_PRELUDE = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np, torch, hxv
from hxv import models
from oracle.oracle import OracleSector
TOL = 1e-13
model = models.hm_1dchain(Nlat=2, Nbath=3)
def check(sec, nup, ndw, refs={{}}):
    if (nup, ndw) not in refs:
        orc = OracleSector(model, nup, ndw)
        rng = np.random.default_rng(1000 + orc.Dim)
        v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
        refs[(nup, ndw)] = (v, orc.spMatVec_main(v))
        orc.close()
    v, ref = refs[(nup, ndw)]
    got = sec.unpad(sec.apply_device(sec.pad(torch.from_numpy(v).cuda()))).cpu().numpy()
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= TOL, ((nup, ndw), err)
"""

_CHILD_CAP = _CHILD_PRELUDE + """
Ns, cap = model.Ns, 1 << 20
kept, evictions, peak = {{}}, 0, 0
for sweep in range(2):
    for nup in range(Ns + 1):
        for ndw in range(Ns + 1):
            s0 = hxv.sector_cache_stats()
            sec = hxv.HxvSector.from_model(model, nup, ndw)
            s1 = hxv.sector_cache_stats()
            assert s1["bytes"] <= cap, s1
            peak = max(peak, s1["bytes"])
            if s1["misses"] > s0["misses"] and s1["entries"] <= s0["entries"] and s1["bytes"] != s0["bytes"]:
                evictions += 1                       # an image went in (the bytes moved) and the cache did not grow: at least one went out
            check(sec, nup, ndw)
            if sweep == 0 and (nup, ndw) in ((4, 4), (3, 4)):
                kept[(nup, ndw)] = sec               # two early handles stay open through both sweeps
            else:
                sec.close()
for (nup, ndw), sec in kept.items():
    check(sec, nup, ndw)                              # their images were evicted long ago; the handles keep them alive
    sec.close()
st = hxv.sector_cache_stats()
print("CAP", "evictions", evictions, "peak_bytes", peak, st)
assert evictions >= 3, evictions
assert st["hits"] + st["misses"] == 2 * (Ns + 1) ** 2 and st["bytes"] <= cap
assert hxv.live_handles() == 0
"""

_CHILD_OFF = _CHILD_PRELUDE + """
for k in range(3):
    sec = hxv.HxvSector.from_model(model, 4, 4)
    assert sec.get_option("open_cache_hit") == 0
    check(sec, 4, 4)
    sec.close()
st = hxv.sector_cache_stats()
print("OFF", st)
assert (st["hits"], st["misses"], st["entries"], st["bytes"]) == (0, 0, 0, 0), st
"""

# the cap child took 2.6 s on an MI355X box (162 opens, 81 oracle products, the imports), the off child 2.2 s: 5 x 2.6 = 13, rounded up to 10 s
CHILD_TIMEOUT_S = 20


def test_cap_and_off_switch_in_fresh_processes(built):
    """Two fresh child processes, one after the other (the cap and the switch are read once per process).
    HXV_SECTOR_CACHE_MB=1: all 81 sectors of M1's model (Ns = 8) opened twice over, one product each against the oracle, two early
    handles kept open through both sweeps and checked again at the end; after every open bytes <= 1 MiB, and at least three opens put
    an image in without the number of entries growing (evictions).
    HXV_SECTOR_CACHE=0: M1 opened three times, each product right, no hit, and hits, misses and entries stay 0.
    Ns = 8 is enough: the measured run evicted 88 times (peak 1 048 200 bytes, 40 entries at the end).
    Time limit of a child: 20 s = five times the measured 2.6 s of the cap child (the off child: 2.2 s), rounded up to 10 s."""
    code = {"cap": _CHILD_CAP, "off": _CHILD_OFF}
    envs = {"cap": {"HXV_SECTOR_CACHE_MB": "1"}, "off": {"HXV_SECTOR_CACHE": "0"}}
    for which in ("cap", "off"):
        env = {k: v for k, v in os.environ.items() if k not in ("HXV_SECTOR_CACHE", "HXV_SECTOR_CACHE_MB")}
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, "-c", code[which].format(root=str(ROOT), pkg=str(ROOT / "cdmft-lanc-ed_amd"))], env=dict(env, **envs[which]),
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        print(which, f"{time.perf_counter() - t0:.1f} s", p.stdout.strip()[-400:])
        assert p.returncode == 0, (which, p.returncode, p.stdout[-1000:], p.stderr[-3000:])     # (the second child starts only after this)
        assert ("CAP" if which == "cap" else "OFF") in p.stdout
