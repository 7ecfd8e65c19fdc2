"""How a workgroup of the tile kernels starts (csrc/hxv_tiled.hip; LABNOTES "how a workgroup starts"): pass A asks for its C tile elements, the
wave's list length and one coefficient word per thread as straight-line code under `p < n` and stores them as they arrive, and reads the
block's words in front of the barrier; pass B is covered because every product runs it.  No operation or operand changed, so
every case meets the CPU oracle at the bound of tests/test_gpu_parity.py, max|Hv - ref| <= 1e-13 max|ref|, on the shapes at which a load
phase can go wrong: blocks smaller than a wave, blocks that are no multiple of 64 rows, the largest block of a plan, idle threads (p >= n),
tiles cut by the slab's edge (local column counts 1, 2, 3 mod 4 and below the tile width), the real-vector pair path with an odd last pair,
three ranks, the all-to-all pieces, coefficient tables longer than a wave and longer than a workgroup, the Lanczos epilogues, the folded
spH0nd block, a stored diagonal, the device row order.

Dead elements are hostile: every pad row and unused column slot of an input holds a quiet NaN, every vector lies inside a buffer with one
LDS size (160 KB) of NaN on either side, and every output starts as a sentinel NaN that must survive bit for bit wherever nothing is to be
written -- an element read from outside the block reaches a live row as NaN, a store outside it changes a sentinel."""
import numpy as np
import pytest

from test_gpu_layout_contract import POISON, SENTINEL, _chain, gathered, lay_of, live, native, pad_bits_off

pytestmark = pytest.mark.gpu

TOL = 1e-13                 # tests/test_gpu_parity.py
MARGIN = 160 * 1024         # bytes of NaN in front of and behind every vector: the LDS of one CU


# ---- hostile buffers --------------------------------------------------------------------------------------------------------------------
def _embedded(n, dtype, fill, src=None):
    """(view, whole): n elements of `dtype` in the middle of a device buffer filled with the bit pattern `fill`; `src` is copied in"""
    import torch

    es = torch.empty(0, dtype=dtype).element_size()
    whole = torch.empty((2 * MARGIN + n * es) // 8, dtype=torch.int64, device="cuda")
    whole.fill_(fill)
    view = whole[MARGIN // 8: MARGIN // 8 + n * es // 8].view(dtype)
    assert view.numel() == n and view.data_ptr() % 256 == 0
    if src is not None:
        view.copy_(src)
    return view, whole


def _margins_off(whole, fill):
    w = MARGIN // 8
    return int((whole[:w] != fill).sum().item() + (whole[-w:] != fill).sum().item())


def _check(out, whole, lay, ref, scale, what):
    assert _margins_off(whole, SENTINEL) == 0, f"{what}: a store outside the output vector"
    assert pad_bits_off(out, lay, SENTINEL) == 0, f"{what}: pad rows were written"
    got = live(out, lay)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite live elements: a dead element was read"
    err = np.abs(got - ref).max() / scale
    assert err <= TOL, f"{what}: max|got - ref| / max|ref| = {err:.3e}"


_REFS = {}


def _reference(key, model, nup, ndw, seed=3):
    """(model, oracle dims, V, R, scale) of one sector, computed once per session: V = the input, R = the oracle's product, [DimDw, DimUp]"""
    from oracle.oracle import OracleSector

    k = (key, nup, ndw, seed)
    if k not in _REFS:
        m = model()
        orc = OracleSector(m, nup, ndw)
        rng = np.random.default_rng(seed)
        v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
        ref = orc.spMatVec_main(v)
        du, dd = orc.DimUp, orc.DimDw
        _REFS[k] = (m, du, dd, v.reshape(dd, du), ref.reshape(dd, du), max(np.abs(ref).max(), 1e-300))
        orc.close()
    return _REFS[k]


def _product(sec, V, R, scale, what, P=1):
    """hxv_apply_device on hostile buffers: this rank's slab of R"""
    import torch

    lay = lay_of(sec)
    vin, _ = _embedded(sec.fullElems, torch.complex128, POISON, gathered(V, lay, P))
    out, whole = _embedded(sec.localElems, torch.complex128, SENTINEL)
    sec.apply_device(vin, out)
    torch.cuda.synchronize()
    c0 = sec.mpiIshift // sec.DimUp
    _check(out, whole, lay, R[c0: c0 + sec.mpiQdw], scale, what)


def _set(sec, opts):
    for k, v in opts.items():
        sec.set_option(k, v)


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def _random_hopping(Ns, cplx, seed):
    """Ns sites, every pair bonded with an amplitude drawn at random: Ns(Ns-1)/2 distinct amplitudes when real, Ns(Ns-1) when complex (a bond
    and its reverse are conjugates), each with both signs in the tile kernels' coefficient table (2 * count + 1 words)"""
    from hxv.models import Model

    rng = np.random.default_rng(seed)
    A = rng.standard_normal((Ns, Ns)) * 0.4
    if cplx:
        A = A + 1j * rng.standard_normal((Ns, Ns)) * 0.4
    A = (A + A.conj().T) / 2
    A[np.diag_indices(Ns)] = rng.standard_normal(Ns) * 0.3
    h = A.reshape(Ns, Ns, 1, 1, 1, 1).astype(np.complex128)
    return Model(Ns, 1, 1, 0, h, np.zeros((Ns, Ns, 1, 1, 1, 1, 0)), np.zeros((Ns, 1, 1, 0)), Uloc=[1.7], xmu=0.1, hfmode=False,
                 name=f"allbonds{Ns}{'c' if cplx else 'r'}")


def _bhz12():
    from hxv import models

    return models.bhz_2d(Nx=2, Ny=1, Nbath=2, Ust=0.4, Jh=0.1)


def _kanamori8():
    from hxv import models

    return models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15)


def _square8():
    from hxv import models

    return models.hm_2dsquare(Nbath=1)


# ---- 1. block shapes ------------------------------------------------------------------------------------------------------------------------
# Ns = 12.  Real H, sector (4,3): DimUp 495, DimDw 220; complex H (BHZ), sector (6,5): DimUp 924.  Block bits 5: every block smaller than a
# wave (at most 10 rows); 8: blocks of up to C(8,4) = 70 rows, no multiple of 64, two waves with idle lanes; 10: up to C(10,4) = 210 / C(10,5) =
# 252 (four waves, the last partly idle); the default plan: one block of 495 / 924 rows in a workgroup of 512 / 1024 threads.  Workgroups of
# 1024 threads on small blocks: whole waves idle.
BLOCK_PLANS = [
    ({"tile_bits_up": 5, "tile_bits_dw": 5}, lambda mb: mb < 64),
    ({"tile_bits_up": 8, "tile_bits_dw": 8}, lambda mb: 64 < mb < 128 and mb % 64),
    ({"tile_bits_up": 10, "tile_bits_dw": 10}, lambda mb: mb > 128 and mb % 64),
    ({}, lambda mb: mb % 64),
    ({"tile_bits_up": 5, "tile_bits_dw": 5, "threads_up": 1024, "threads_dw": 1024}, lambda mb: mb < 64),
    ({"tile_bits_up": 8, "tile_bits_dw": 8, "threads_up": 256, "threads_dw": 256}, lambda mb: 64 < mb < 128),
]


@pytest.mark.parametrize("h", ["real", "complex"])
def test_block_shapes_and_idle_threads(built, h):
    import hxv

    if h == "real":
        m, du, dd, V, R, scale = _reference("chain12", lambda: _chain(12), 4, 3)
    else:
        m, du, dd, V, R, scale = _reference("bhz12", _bhz12, 6, 5)
    nup, ndw = (4, 3) if h == "real" else (6, 5)
    ran = 0
    for plan, shape_ok in BLOCK_PLANS:
        for tile in ({"cols_per_tile": 4, "rows_per_tile": 4}, {"cols_per_tile": 2, "rows_per_tile": 8}, {"cols_per_tile": 4, "rows_per_tile": 2}):
            sec = hxv.HxvSector.from_model(m, nup, ndw)
            assert sec.stats()["real_h"] == (1 if h == "real" else 0)
            _set(sec, dict(plan, **tile))
            sec.set_option("job_up", 0)                       # the tile kernels, not the job kernel
            what = f"{m.name} ({nup},{ndw}) {plan} {tile}"
            _product(sec, V, R, scale, what)
            assert sec.get_option("kernel") == 1, what
            mb = sec.get_option("max_block_up")        # (real: up to C(bits,4) rows of 495; complex: up to C(bits,6) or C(bits,5) of 924)
            assert shape_ok(mb) and mb <= sec.get_option("threads_up"), (what, mb)
            ran += 1
            sec.close()
    assert ran == 18


# ---- 2. tiles cut by the slab's edge, slab0 != 0 ------------------------------------------------------------------------------------------------
def test_local_column_counts_and_column_offsets(built):
    """caller-gathered slabs of P ranks (slab0 != 0 for every rank but the first): local column counts with remainder 1, 2 and 3 modulo the
    tile width 4, and fewer local columns than a tile is wide"""
    import hxv
    from hxv import dw_split

    seen, narrow = set(), 0
    for ndw, P in ((2, 3), (3, 3), (1, 3), (1, 5)):             # DimDw 28 -> 10, 9, 9; 56 -> 19, 19, 18; 8 -> 3, 3, 2; 8 -> 2, 2, 2, 1, 1
        m, du, dd, V, R, scale = _reference("square8", _square8, 4, ndw)
        for r in range(P):
            q, c0 = dw_split(dd, r, P)
            for tile in ({"cols_per_tile": 4, "rows_per_tile": 4}, {"cols_per_tile": 2, "rows_per_tile": 2}):
                sec = hxv.HxvSector.from_model(m, 4, ndw, rank=r, nranks=P)
                _set(sec, dict(tile, tile_bits_up=4, tile_bits_dw=3, job_up=0))
                assert sec.mpiQdw == q and sec.mpiIshift == c0 * du
                _product(sec, V, R, scale, f"square8 (4,{ndw}) rank {r}/{P} q={q} {tile}", P)
                sec.close()
            seen.add(q % 4)
            narrow += q < 4
    assert seen >= {1, 2, 3}, seen
    assert narrow >= 3


# ---- 3. real vectors: two columns per LDS element ----------------------------------------------------------------------------------------------
def test_real_vector_pairs_with_an_odd_last_pair(built):
    """DimDw = 55 (Ns = 11, sector (3,2)): the last tile of 2, 4 and 8 columns holds 1, 3 and 7 of them, its last LDS pair one column and
    its clamped copy"""
    import torch
    import hxv
    from oracle.oracle import OracleSector

    m = _chain(11)
    orc = OracleSector(m, 3, 2)
    du, dd = orc.DimUp, orc.DimDw
    assert (du, dd) == (165, 55)
    x = np.random.default_rng(8).standard_normal(orc.Dim)
    ref = orc.spMatVec_main(x.astype(np.complex128))
    assert np.abs(ref.imag).max() == 0.0
    ref = ref.real.reshape(dd, du)
    scale = np.abs(ref).max()
    orc.close()
    for fam in ({"cols_per_tile": 2}, {"cols_per_tile": 4}, {"cols_per_tile": 8, "rows_per_tile": 4, "real_dw_pairs": 0}, {"cols_per_tile": 8, "real_dw_pairs": 1},
                {"cols_per_tile": 4, "tile_bits_up": 6, "tile_bits_dw": 6}, {"cols_per_tile": 8, "tile_bits_up": 6, "tile_bits_dw": 6, "threads_up": 1024}):
        sec = hxv.HxvSector.from_model(m, 3, 2)
        _set(sec, dict(fam, job_up=0))
        lay = lay_of(sec, real=True)
        vin, _ = _embedded(dd * lay.pitch, torch.float64, POISON, native(x.reshape(dd, du), lay))
        out, whole = _embedded(dd * lay.pitch, torch.float64, SENTINEL)
        sec.apply_device_real(vin, out)
        torch.cuda.synchronize()
        _check(out, whole, lay, ref, scale, f"real chain11 (3,2) {fam}")
        sec.close()


# ---- 4. three thread ranks, every exchange ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["allgather", "alltoall", "halo"])
def test_three_thread_ranks(built, exchange):
    """hxv_apply_device_slab on three thread ranks; "alltoall" hands pass A its accumulators in pieces (one per rank of origin, natural layout)"""
    import torch
    import hxv

    m, du, dd, V, R, scale = _reference("chain11", lambda: _chain(11), 3, 2)
    P = 3
    hxv.set_exchange_default(exchange)

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, 3, 2, rank=r, nranks=P)
        assert sec.exchange_mode == exchange
        sec.set_option("job_up", 0)
        group.join(sec)
        lay = lay_of(sec)
        c0 = sec.mpiIshift // sec.DimUp
        vl, _ = _embedded(sec.localElems, torch.complex128, POISON, native(V[c0: c0 + sec.mpiQdw], lay))
        out, whole = _embedded(sec.localElems, torch.complex128, SENTINEL)
        sec.apply_device_slab(vl, out)
        torch.cuda.synchronize()
        sec.close()
        return c0, lay, out, whole

    try:
        res = hxv.run_ranks(P, rank, transport="local")
    finally:
        hxv.set_exchange_default("allgather")
    for r, (c0, lay, out, whole) in enumerate(res):
        _check(out, whole, lay, R[c0: c0 + out.numel() // lay.pitch], scale, f"{exchange} rank {r}/{P}")


# ---- 5. coefficient tables longer than a wave, and longer than a workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["real_ns10", "complex_ns12"])
def test_coefficient_copy_spans_waves(built, case):
    """every pair of sites bonded at random.  Ns = 10, real: 45 amplitudes, 91 table words (two waves).  Ns = 12, complex: 132 amplitudes, 265
    words -- more than the 256 threads of the smallest workgroup, so the copy takes a second word per thread -- and under the 255 amplitudes
    past which the tile kernels are not used.  Blocks of fewer rows than there are words: threads without a row copy them."""
    import hxv

    if case == "real_ns10":
        m, du, dd, V, R, scale = _reference(case, lambda: _random_hopping(10, False, 41), 3, 2)
        nup, ndw, words = 3, 2, 91
    else:
        m, du, dd, V, R, scale = _reference(case, lambda: _random_hopping(12, True, 42), 3, 2)
        nup, ndw, words = 3, 2, 265
    longer = 0
    for fam in ({"threads_up": 256, "threads_dw": 256, "tile_bits_up": 7, "tile_bits_dw": 7}, {"tile_bits_up": 5, "tile_bits_dw": 5},
                {"threads_up": 256, "threads_dw": 256, "tile_bits_up": 4, "tile_bits_dw": 4, "cols_per_tile": 2, "rows_per_tile": 2}, {}):
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        _set(sec, dict(fam, job_up=0))
        assert sec.stats()["real_h"] == (1 if case == "real_ns10" else 0)
        _product(sec, V, R, scale, f"{case} {fam}")
        assert sec.get_option("kernel") == 1, "the tile kernels were not used"
        # the plan's own count (csrc/hxv_sector.cpp build_ell: an amplitude and its conjugate count apart): 2 * amplitudes + 1 table words
        got = {2 * sec.get_option("ncoef_up") + 1, 2 * sec.get_option("ncoef_dw") + 1}
        assert got == {words} and 64 < words < 2 * 255 + 1, (case, fam, got)
        if "threads_up" in fam:
            assert sec.get_option("threads_up") == 256 and sec.get_option("threads_dw") == 256
            longer += words > 256
        sec.close()
    assert longer == (2 if case == "complex_ns12" else 0)     # the copy's loop for words beyond one per thread ran in both passes, twice


# ---- 6. Lanczos epilogues against the unfused step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["complex", "real", "pair"])
def test_lanczos_epilogues_match_the_unfused_step(built, mode):
    """pass A with the Lanczos epilogue (LZ 1: complex and real vectors; LZ 2: two real vectors in one complex one) against the same
    recurrence from plain products, and against the oracle's sp_lanc_tridiag"""
    import torch
    import hxv
    from oracle.oracle import OracleSector

    m = _chain(12)
    nup, ndw, nl = 4, 3, 14
    orc = OracleSector(m, nup, ndw)
    rng = np.random.default_rng(17)
    va = rng.standard_normal(orc.Dim)
    vb = rng.standard_normal(orc.Dim)
    if mode == "complex":
        va = va + 1j * rng.standard_normal(orc.Dim)
    va, vb = (va / np.linalg.norm(va)).astype(np.complex128), (vb / np.linalg.norm(vb)).astype(np.complex128)
    refs = [orc.lanc_tridiag(va, nl)] + ([orc.lanc_tridiag(vb, nl)] if mode == "pair" else [])
    orc.close()
    got = {}
    for fused in (1, 0):
        for plan in ({}, {"tile_bits_up": 8, "tile_bits_dw": 8}, {"tile_bits_up": 5, "tile_bits_dw": 5, "cols_per_tile": 2}):
            sec = hxv.HxvSector.from_model(m, nup, ndw)
            _set(sec, dict(plan, job_up=0, lanczos_fused=fused, real_vectors=1 if mode == "real" else 0))
            da, db = torch.from_numpy(va).cuda(), torch.from_numpy(vb).cuda()
            if mode == "pair" and fused:
                runs = sec.lanczos_tridiag_pair(da, db, nl)
            elif mode == "pair":                               # (the paired driver is the fused recurrence only: its unfused step is two runs)
                runs = [sec.lanczos_tridiag(da, nl), sec.lanczos_tridiag(db, nl)]
            else:
                runs = [sec.lanczos_tridiag(da, nl)]
                assert sec.get_option("lanczos_real_last") == (1 if mode == "real" else 0)
            for k, ((a, b, n), (a0, b0)) in enumerate(zip(runs, refs)):
                assert n == nl
                assert np.abs(a - a0).max() <= 1e-11 * np.abs(a0).max() and np.abs(b[1:] - b0[1:]).max() <= 1e-11 * np.abs(b0).max(), (mode, fused, plan, k)
                got[(fused, tuple(plan), k)] = (a, b)
            sec.close()
    for (fused, plan, k), (a, b) in got.items():
        if fused:
            a0, b0 = got[(0, plan, k)]
            assert np.abs(a - a0).max() <= 1e-12 * np.abs(a0).max() and np.abs(b - b0).max() <= 1e-12 * np.abs(b0).max(), (mode, plan, k)


# ---- 7. the folded spH0nd block, a stored diagonal, the device row order ---------------------------------------------------------------------
def test_kanamori_block_inside_pass_a(built):
    import hxv

    m, du, dd, V, R, scale = _reference("kanamori8", _kanamori8, 4, 3)
    for fam in ({"cols_per_tile": 4}, {"cols_per_tile": 2}, {"cols_per_tile": 4, "tile_bits_up": 4, "tile_bits_dw": 4}, {"cols_per_tile": 2, "tile_bits_up": 3, "tile_bits_dw": 5, "threads_up": 1024}):
        for r, P in ((0, 1), (1, 3)):
            sec = hxv.HxvSector.from_model(m, 4, 3, rank=r, nranks=P)
            _set(sec, dict(fam, fold_nd=1, job_up=0))
            _product(sec, V, R, scale, f"kanamori8 (4,3) {fam} rank {r}/{P}", P)
            sec.close()


def test_stored_diagonal(built):
    """hxv_create_from_csr: the diagonal is read per element behind the barrier, index-chunk tiles instead of prefix blocks"""
    import torch
    import hxv
    from oracle.oracle import OracleSector

    m, du, dd, V, R, scale = _reference("chain11", lambda: _chain(11), 3, 2)
    orc = OracleSector(m, 3, 2)
    for fam in ({}, {"lds_budget_kb": 8}, {"lds_budget_kb": 8, "cols_per_tile": 2, "rows_per_tile": 8}):
        sec = hxv.HxvSector.from_csr(du, dd, orc.csr("up"), orc.csr("dw"), orc.diag())
        _set(sec, dict(fam, job_up=0))
        _product(sec, V, R, scale, f"from_csr chain11 (3,2) {fam}")
        assert sec.get_option("kernel") == 1 and sec.get_option("job_up_active") == 0, "pass A's tile kernel was not used"
        sec.close()
    orc.close()


def test_device_row_order(built, monkeypatch):
    """one sector with the device row order switched on below its size threshold (tests/test_gpu_row_order.py): 8 block bits at Ns = 12"""
    import hxv
    from hxv import models

    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    monkeypatch.setenv("HXV_ROW_ORDER_BITS", "8")
    hxv.sector_cache_clear()
    try:
        m, du, dd, V, R, scale = _reference("star12", lambda: models.hm_2dsquare(Nbath=2, xmu=0.2), 5, 7)
        for fam in ({}, {"cols_per_tile": 2, "rows_per_tile": 8}):
            sec = hxv.HxvSector.from_model(m, 5, 7)
            _set(sec, dict(fam, tile_bits_up=8, job_up=0))
            assert sec.row_perm is not None and not np.array_equal(sec.row_perm, np.arange(sec.DimUp))
            _product(sec, V, R, scale, f"star12 (5,7) row order {fam}")
            sec.close()
    finally:
        hxv.sector_cache_clear()
