"""Twin-sector eigenstates on SPLIT sectors on the MI355X (include/hxv.h, hxv_twin_vector with two handles that are the same rank of the
same split): rank r turns its slab of A = (nup,ndw) into its slab of B = (ndw,nup) with one all-to-all between a pack and an unpack kernel
(csrc/hxv_twin.hip).  2 - 4 thread ranks on one GPU, every test on both transports (thread ranks, and the RCCL branches through
tests/rccl_double), as tests/test_gpu_ranks.py does.  Exact against numpy through the host copies and bit for bit against the unsplit call
on the smallest shapes at which each thing can break, with the device row order off and forced on (the hooks of tests/test_gpu_twin.py);
the layout contract; a complex model; the product's other exchange modes; the result is B's eigenstate on the split sector; every new
refusal with its status and message."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS = {6: (3, 4), 8: (4, 5), 10: (5, 6)}
MIN_DIMUP = 16
# (Ns, nup, ndw, nranks, from is to): DimUp_A x DimDw_A, what it exercises
CASES = [
    (4, 1, 2, 4, False),    # 4 x 6: one B column per rank, A columns 2,2,1,1, nranks = DimUp_A (order off only: no hook values for Ns = 4)
    (6, 1, 3, 2, False),    # 6 x 20: blocks smaller than a tile, not multiples of 8
    (6, 1, 3, 3, False),    # 6 x 20: uneven A split 7,7,6
    (6, 3, 3, 3, False),    # 20 x 20: the same sector both sides, two handles; uneven both ways
    (6, 3, 3, 3, True),     # ... and one handle
    (8, 4, 1, 3, False),    # 70 x 8: with the hooks only A has a row order; splits 3,3,2 against 24,23,23
    (8, 1, 4, 3, False),    # 8 x 70: only B has one
    (8, 3, 5, 4, False),    # 56 x 56: two different row orders
    (10, 4, 5, 4, False),   # 210 x 252: several tiles, ragged both ways, B split 53,53,52,52
]
EXACT = [(c, mode) for c in CASES for mode in (("off",) if c[0] == 4 else ("off", "bits0", "bits1"))]


@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    """-> the `transport` argument of hxv.run_ranks; a mismatch between two ranks' plans ends as a failed test, not as a five-minute wait"""
    monkeypatch.setenv("HXV_LOCAL_TIMEOUT_S", "30")
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.fixture
def order_mode(monkeypatch):
    """set(mode, ns): row orders off, or forced on for DimUp >= 16 at one of the two block-bit values of BITS[ns]"""
    import hxv

    def set_mode(mode, ns):
        for k in ("HXV_ROW_ORDER", "HXV_ROW_ORDER_MIN_DIMUP", "HXV_ROW_ORDER_BITS"):
            monkeypatch.delenv(k, raising=False)
        if mode == "off":
            monkeypatch.setenv("HXV_ROW_ORDER", "0")
        else:
            monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", str(MIN_DIMUP))
            monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(BITS[ns][int(mode[-1])]))
        hxv.sector_cache_clear()

    yield set_mode
    hxv.sector_cache_clear()


def _chain(ns):
    from hxv import models

    nb = ns // 2 - 1
    return models.hm_1dchain(Nlat=2, Nbath=nb, eps_bath=[0.3, -0.2, 0.1, -0.15][:nb], xmu=0.15)


def _bhz_complex():
    from hxv import models

    return models.bhz_2d(Nx=2, Ny=1, Nbath=1, lam=0.3, Ust=0.5, Jh=0.2)   # Ns = 8, complex, no spin symmetry


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _transposed(v, sec):
    return v.reshape(sec.DimDw, sec.DimUp).T.ravel()


def _bits(t):
    import torch

    return torch.view_as_real(t).contiguous().view(torch.int64).cpu()


def _nan(n):
    import torch

    return torch.full((n,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")


def _open_pair(m, nup, ndw, same=False, **kw):
    import hxv

    a = hxv.HxvSector.from_model(m, nup, ndw, **kw)
    b = a if same else hxv.HxvSector.from_model(m, ndw, nup, **kw)
    assert (b.DimUp, b.DimDw) == (a.DimDw, a.DimUp)
    return a, b


def _close(*secs):
    for s in {id(s): s for s in secs}.values():
        s.close()


def _unsplit_twin(m, nup, ndw, v):
    """-> (the unsplit call's device result as [DimDw_B][pitch_B] bits on the host, the device tensor, the two row orders)"""
    a, b = _open_pair(m, nup, ndw)
    try:
        full = a.twin_vector(b, a.vector_from_host(v))
        return _bits(full).view(b.DimDw, b.pitch, 2), full, (a.row_perm, b.row_perm), (a.DimUp, b.DimUp)
    finally:
        _close(a, b)


def _split_twin(m, nup, ndw, nranks, same, v, transport, dirty_pads=False, after=None):
    """every rank: slab of A from the host vector, the split twin into a fresh buffer and into a NaN-filled one of the caller's.
    -> per rank (first index and length of B's slab in B's host vector, first column, the slab through vector_to_host, bits of the two
    results, was the source unchanged, the rank's row orders, what `after(fa, fb, out)` returned)"""
    import hxv

    def rank(r, group):
        fa, fb = _open_pair(m, nup, ndw, same, rank=r, nranks=nranks)
        try:
            group.join(fb)
            slab = fa.vector_from_host(v[fa.mpiIshift: fa.mpiIshift + fa.vecDim])
            if dirty_pads:
                slab.view(fa.mpiQdw, fa.pitch)[:, fa.DimUp:] = complex(np.nan, np.nan)
            before = _bits(slab)
            out = fa.twin_vector(fb, slab)
            assert out.numel() == fb.localElems
            mine = _nan(fb.localElems)
            assert fa.twin_vector(fb, slab, out=mine) is mine
            extra = after(fa, fb, out) if after else None
            return (fb.mpiIshift, fb.vecDim, fb.mpiIshift // fb.DimUp, fb.vector_to_host(out), _bits(out).view(fb.mpiQdw, fb.pitch, 2),
                    _bits(mine).view(fb.mpiQdw, fb.pitch, 2), bool((_bits(slab) == before).all()), (fa.row_perm, fb.row_perm), extra)
        finally:
            _close(fa, fb)

    return hxv.run_ranks(nranks, rank, transport=transport)


@pytest.mark.parametrize("case,mode", EXACT, ids=lambda x: x if isinstance(x, str) else "-".join(str(int(y)) for y in x))
def test_split_twin_vector_is_the_exact_transpose_and_the_unsplit_calls_bits(built, transport, order_mode, case, mode):
    ns, nup, ndw, nranks, same = case
    order_mode(mode, ns)
    m = _chain(ns)
    v = _rand(_dim(ns, nup, ndw), 1000 * ns + 10 * nup + ndw)
    ref_bits, _, perms, dimups = _unsplit_twin(m, nup, ndw, v)
    for perm, dimup in zip(perms, dimups):
        # the chain takes a non-identity order wherever the hooks apply; off means off
        assert (perm is not None) == (mode != "off" and dimup >= MIN_DIMUP), (mode, dimup)
        if perm is not None:
            assert not np.array_equal(perm, np.arange(dimup))
    if (ns, nup, ndw) == (8, 3, 5) and mode != "off":
        assert not np.array_equal(perms[0], perms[1])
    want = v.reshape(-1, dimups[0]).T.ravel()                                   # B's host vector
    res = _split_twin(m, nup, ndw, nranks, same, v, transport)
    cols = 0
    for lo, n, c0, host, out_bits, mine_bits, unchanged, rperms, _ in res:
        q = out_bits.shape[0]
        assert np.array_equal(host, want[lo: lo + n])
        assert bool((out_bits == ref_bits[c0: c0 + q]).all())                   # bit for bit the unsplit call's columns
        assert bool((mine_bits == out_bits).all())                              # staging buffers reused, every element written
        assert unchanged
        for p, rp in zip(perms, rperms):                                        # every rank stores its rows in the unsplit sector's order
            assert (p is None) == (rp is None) and (p is None or np.array_equal(p, rp))
        cols += q
    assert cols == ref_bits.shape[0]


def _dim(ns, nup, ndw):
    from math import comb

    return comb(ns, nup) * comb(ns, ndw)


@pytest.mark.parametrize("mode", ["off", "bits0"])
@pytest.mark.parametrize("ns,nup,ndw,nranks", [(6, 1, 3, 3), (8, 4, 1, 3), (10, 4, 5, 4)])
def test_split_twin_vector_layout_contract(built, transport, order_mode, mode, ns, nup, ndw, nranks):
    """pad rows of d_psi are never read (NaN there does not spread), every element of d_out is written (NaN everywhere before), pad rows of
    d_out are zero, d_psi is unchanged bit for bit"""
    order_mode(mode, ns)
    m = _chain(ns)
    v = _rand(_dim(ns, nup, ndw), 5)
    a, b = _open_pair(m, nup, ndw)
    dimup_b, pitch_b, pitch_a, dimup_a = b.DimUp, b.pitch, a.pitch, a.DimUp
    _close(a, b)
    assert pitch_a > dimup_a or pitch_b > dimup_b
    want = v.reshape(-1, dimup_a).T.ravel()
    for lo, n, c0, host, out_bits, mine_bits, unchanged, _, _ in _split_twin(m, nup, ndw, nranks, False, v, transport, dirty_pads=True):
        o = mine_bits.numpy().view(np.float64)                                   # [qdw_B][pitch_B][re, im]
        assert o.shape[1] == pitch_b and np.isfinite(o).all()
        assert not o[:, dimup_b:].any()
        assert unchanged
        assert np.array_equal(host, want[lo: lo + n])
        assert bool((mine_bits == out_bits).all())


@pytest.mark.parametrize("mode", ["off", "bits0", "bits1"])
def test_split_twin_vector_is_exact_on_a_complex_model_without_spin_symmetry(built, transport, order_mode, mode):
    """the map is data movement: defined, and exact, where the result is no eigenstate; (2,3) <-> (3,2) of Ns = 8 on 3 ranks, both ways"""
    order_mode(mode, 8)
    m = _bhz_complex()
    for (nup, ndw), seed in (((2, 3), 77), ((3, 2), 78)):
        v = _rand(_dim(8, nup, ndw), seed)
        ref_bits, _, _, dimups = _unsplit_twin(m, nup, ndw, v)
        want = v.reshape(-1, dimups[0]).T.ravel()
        for lo, n, c0, host, out_bits, mine_bits, unchanged, _, _ in _split_twin(m, nup, ndw, 3, False, v, transport):
            assert np.array_equal(host, want[lo: lo + n])
            assert bool((out_bits == ref_bits[c0: c0 + out_bits.shape[0]]).all()) and bool((mine_bits == out_bits).all()) and unchanged


@pytest.mark.parametrize("exchange", ["halo", "alltoall"])
def test_split_twin_vector_does_not_depend_on_the_products_exchange(built, transport, monkeypatch, exchange):
    """(8,3,5) on 4 ranks with the product's other two exchanges: the same bits, and the handle's product still works on the result"""
    import torch
    import hxv

    ns, nup, ndw, nranks = 8, 3, 5, 4
    for k in ("HXV_ROW_ORDER", "HXV_ROW_ORDER_MIN_DIMUP", "HXV_ROW_ORDER_BITS"):
        monkeypatch.delenv(k, raising=False)
    m = _chain(ns)
    v = _rand(_dim(ns, nup, ndw), 41)
    a, b = _open_pair(m, nup, ndw)
    try:
        full = a.twin_vector(b, a.vector_from_host(v))
        ref_bits = _bits(full).view(b.DimDw, b.pitch, 2)
        h_ref = b.apply_device(full).cpu().numpy().reshape(b.DimDw, b.pitch)      # native form: padded in, padded out
    finally:
        _close(a, b)

    def after(fa, fb, out):
        assert fb.exchange_mode == exchange
        hv = fb.apply_device_slab(out)
        torch.cuda.synchronize()
        return hv.cpu().numpy().reshape(fb.mpiQdw, fb.pitch)

    hxv.set_exchange_default(exchange)
    try:
        res = _split_twin(m, nup, ndw, nranks, False, v, transport, after=after)
    finally:
        hxv.set_exchange_default("allgather")
    scale = np.abs(h_ref).max()
    for lo, n, c0, host, out_bits, mine_bits, unchanged, _, hv in res:
        q = out_bits.shape[0]
        assert bool((out_bits == ref_bits[c0: c0 + q]).all()) and bool((mine_bits == out_bits).all()) and unchanged
        assert np.abs(hv - h_ref[c0: c0 + q]).max() <= 1e-13 * scale             # the suite's product tolerance


def test_split_twin_of_a_ground_state_is_the_twin_sectors_eigenstate(built, transport):
    """Ns = 6, (2,3) -> (3,2) on 3 ranks: the split twin of A's ground state (computed unsplit, cut into slabs) is B's eigenstate on the split
    sector: <H_B> = E_A to 1e-12 and a residual no larger than twice the state's own in A + 1e-12 (the bounds of the unsplit test)."""
    import torch
    import hxv

    m = _chain(6)
    nup, ndw, nranks = 2, 3, 3
    a = hxv.HxvSector.from_model(m, nup, ndw)
    try:
        ev, vecs, nc, _ = a.eigh_lowest(1, tol=1e-14, native=True)
        assert nc == 1
        e_a, psi_a = float(ev[0]), vecs[0].contiguous()
        res_a = float(torch.linalg.norm(a.apply_device(psi_a) - e_a * psi_a))
        v = a.vector_to_host(psi_a)
    finally:
        a.close()

    def after(fa, fb, out):
        hv = fb.apply_device_slab(out)
        torch.cuda.synchronize()
        return fb.vector_to_host(hv)

    res = _split_twin(m, nup, ndw, nranks, False, v, transport, after=after)
    psi_b = np.concatenate([r[3] for r in res])
    h_psi_b = np.concatenate([r[8] for r in res])
    assert psi_b.size == v.size and [r[0] for r in res] == list(np.cumsum([0] + [r[1] for r in res[:-1]]))
    e_b = float(np.vdot(psi_b, h_psi_b).real)
    res_b = float(np.linalg.norm(h_psi_b - e_a * psi_b))
    print("E_A", e_a, "|<H_B> - E_A|", abs(e_b - e_a), "res_A", res_a, "res_B", res_b)
    assert abs(e_b - e_a) <= 1e-12
    assert res_b <= 2 * res_a + 1e-12


def test_split_twin_vector_refusals(built, monkeypatch):
    """decided from the arguments alone: each returns at once (one thread, no group running), names the entry and writes nothing"""
    import torch
    import hxv

    monkeypatch.setenv("HXV_ROW_ORDER", "0")
    hxv.sector_cache_clear()
    L = hxv.load_library()
    m = _chain(6)
    a02 = hxv.HxvSector.from_model(m, 1, 3, rank=0, nranks=2)
    b02 = hxv.HxvSector.from_model(m, 3, 1, rank=0, nranks=2)
    b12 = hxv.HxvSector.from_model(m, 3, 1, rank=1, nranks=2)
    b03 = hxv.HxvSector.from_model(m, 3, 1, rank=0, nranks=3)
    try:
        n = max(s.localElems for s in (a02, b02, b12, b03))
        x = torch.zeros(n, dtype=torch.complex128, device="cuda")
        y = torch.full((n,), complex(3.0, -4.0), dtype=torch.complex128, device="cuda")
        keep = y.clone()
        torch.cuda.synchronize()

        def refused(frm, to, status):
            rc = L.hxv_twin_vector(frm._h, to._h, x.data_ptr(), y.data_ptr())
            msg = L.hxv_last_error().decode()
            assert rc == status, (rc, status, msg)
            assert "hxv_twin_vector" in msg and len(msg) > len("hxv_twin_vector")
            torch.cuda.synchronize()
            assert torch.equal(y, keep)        # a refused call writes nothing

        STATE, UNSUPPORTED = 3, 4
        refused(a02, b03, UNSUPPORTED)         # 2 ranks with 3
        refused(a02, b02, STATE)               # split alike, `to` not bound to a communicator
        refused(a02, b12, UNSUPPORTED)         # rank 0 with rank 1
    finally:
        _close(a02, b02, b12, b03)
        hxv.sector_cache_clear()
