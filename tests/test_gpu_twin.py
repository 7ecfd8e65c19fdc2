"""Twin-sector eigenstates on the MI355X (include/hxv.h, hxv_twin_vector; HxvSector.twin_vector): the state of sector A = (nup,ndw) as a
vector of B = (ndw,nup), the transpose of the amplitude matrix, on the device.  Exact against numpy through the host copies on the smallest
shapes at which each thing can break, with the device row order off and forced on (the hooks of tests/test_gpu_row_order.py); the layout
contract (pad rows never read, every element written, pad rows zero); the result IS B's eigenstate for spin-symmetric models; another
kernel (the observables record) sees the spins swapped; every refusal with its status and message."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Ns -> two values of HXV_ROW_ORDER_BITS at which the chain below takes a non-identity row order (its two cluster sites tie to every replica)
BITS = {6: (3, 4), 8: (4, 5), 10: (5, 6)}
MIN_DIMUP = 16
MODES = ["off", "bits0", "bits1"]
# (Ns, nup, ndw): shape DimUp x DimDw, what it exercises
CASES = [
    (6, 0, 3),    # 1 x 20: a one-row column, pitch 8
    (6, 1, 3),    # 6 x 20: both sizes below a tile and not multiples of 8
    (6, 3, 3),    # 20 x 20: from == to; applying it twice returns the input
    (8, 1, 4),    # 8 x 70: with the hooks, only B has a row order
    (8, 4, 1),    # 70 x 8: only A has a row order
    (8, 3, 5),    # 56 x 56: both have different row orders
    (10, 3, 6),   # 120 x 210: several tiles with ragged edges both ways
    (10, 4, 5),   # 210 x 252: the same
]


def _chain(ns):
    from hxv import models

    nb = ns // 2 - 1
    return models.hm_1dchain(Nlat=2, Nbath=nb, eps_bath=[0.3, -0.2, 0.1, -0.15][:nb], xmu=0.15)


def _bhz_complex():
    from hxv import models

    return models.bhz_2d(Nx=2, Ny=1, Nbath=1, lam=0.3, Ust=0.5, Jh=0.2)   # Ns = 8, complex, no spin symmetry


def _jxjp():
    from hxv import models

    return models.bhz_2d(Nx=1, Ny=1, Nbath=2, Ust=1.0, Jh=0.3, Jx=0.3, Jp=0.3)   # Ns = 6, spin symmetric, with the spH0nd block


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


def _open_pair(m, nup, ndw):
    import hxv

    a = hxv.HxvSector.from_model(m, nup, ndw)
    b = a if nup == ndw else hxv.HxvSector.from_model(m, ndw, nup)
    assert (b.DimUp, b.DimDw) == (a.DimDw, a.DimUp)
    return a, b


def _close(*secs):
    for s in {id(s): s for s in secs}.values():
        s.close()


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _transposed(v, sec):
    return v.reshape(sec.DimDw, sec.DimUp).T.ravel()


def _bits(t):
    import torch

    return torch.view_as_real(t).contiguous().view(torch.int64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns,nup,ndw", CASES)
def test_twin_vector_is_the_exact_transpose(built, order_mode, mode, ns, nup, ndw):
    import torch

    order_mode(mode, ns)
    a, b = _open_pair(_chain(ns), nup, ndw)
    try:
        for s in (a, b):
            # the chain takes a non-identity order wherever the hooks apply; off means off
            assert (s.row_perm is not None) == (mode != "off" and s.DimUp >= MIN_DIMUP), (mode, s.DimUp)
            if s.row_perm is not None:
                assert not np.array_equal(s.row_perm, np.arange(s.DimUp))
        if (ns, nup, ndw) == (8, 3, 5) and mode != "off":
            assert not np.array_equal(a.row_perm, b.row_perm)
        v = _rand(a.Dim, 1000 * ns + 10 * nup + ndw)
        d = a.vector_from_host(v)
        out = a.twin_vector(b, d)
        assert out.numel() == b.localElems
        assert np.array_equal(b.vector_to_host(out), _transposed(v, a))
        if a is b:
            back = b.twin_vector(a, out)
            assert torch.equal(_bits(back), _bits(d))
        # a caller's own buffer, dirty: every element is written
        mine = torch.full((b.localElems,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        assert a.twin_vector(b, d, out=mine) is mine
        assert torch.equal(_bits(mine), _bits(out))
    finally:
        _close(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_twin_vector_is_exact_on_a_complex_model_without_spin_symmetry(built, order_mode, mode):
    """the map is data movement: defined, and exact, where the result is no eigenstate"""
    order_mode(mode, 8)
    a, b = _open_pair(_bhz_complex(), 2, 3)   # 28 x 56
    try:
        v = _rand(a.Dim, 77)
        assert np.array_equal(b.vector_to_host(a.twin_vector(b, a.vector_from_host(v))), _transposed(v, a))
        w = _rand(b.Dim, 78)
        assert np.array_equal(a.vector_to_host(b.twin_vector(a, b.vector_from_host(w))), _transposed(w, b))
    finally:
        _close(a, b)


@pytest.mark.parametrize("mode", ["off", "bits0"])
@pytest.mark.parametrize("ns,nup,ndw", [(6, 0, 3), (6, 1, 3), (6, 3, 3), (8, 4, 1), (10, 4, 5)])
def test_twin_vector_layout_contract(built, order_mode, mode, ns, nup, ndw):
    """pad rows of d_psi are never read (NaN there does not spread), every element of d_out is written (NaN everywhere before), pad rows of
    d_out are zero, d_psi is unchanged bit for bit"""
    import torch

    order_mode(mode, ns)
    a, b = _open_pair(_chain(ns), nup, ndw)
    try:
        assert a.pitch > a.DimUp or b.pitch > b.DimUp
        v = _rand(a.Dim, 5)
        d = a.vector_from_host(v)
        d.view(a.DimDw, a.pitch)[:, a.DimUp:] = complex(np.nan, np.nan)
        before = _bits(d).clone()
        out = torch.full((b.localElems,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        a.twin_vector(b, d, out=out)
        o = torch.view_as_real(out.view(b.DimDw, b.pitch))
        assert bool(torch.isfinite(o).all())
        assert int(torch.count_nonzero(o[:, b.DimUp:])) == 0
        assert torch.equal(_bits(d), before)
        assert np.array_equal(b.vector_to_host(out), _transposed(v, a))
    finally:
        _close(a, b)


@pytest.mark.parametrize("nup", range(6))
@pytest.mark.parametrize("name", ["chain", "jxjp"])
def test_twin_of_a_ground_state_is_the_twin_sectors_eigenstate(built, name, nup):
    """Spin-symmetric models, every pair nup < ndw with Dim > 1 (Ns = 6): psi_B = twin of A's ground state has A's energy as its expectation
    value of B's own product and a residual no larger than twice the state's own in A (+ 1e-12: the product's parity with the oracle);
    B's own lowest eigenvalue is A's to the project's eigenvalue tolerance."""
    import torch
    from math import comb

    m = _chain(6) if name == "chain" else _jxjp()
    assert m.Ns == 6
    pairs = [(nup, ndw) for ndw in range(nup + 1, 7) if comb(6, nup) * comb(6, ndw) > 1]
    assert pairs
    for nu, nd in pairs:
        a, b = _open_pair(m, nu, nd)
        try:
            ev, vecs, nc, _ = a.eigh_lowest(1, tol=1e-14, native=True)
            assert nc == 1
            e_a, psi_a = float(ev[0]), vecs[0].contiguous()
            res_a = float(torch.linalg.norm(a.apply_device(psi_a) - e_a * psi_a))
            psi_b = a.twin_vector(b, psi_a)
            hb = b.apply_device(psi_b)
            e_b = float(torch.vdot(psi_b, hb).real)
            res_b = float(torch.linalg.norm(hb - e_a * psi_b))
            evb, _, ncb, _ = b.eigh_lowest(1, tol=1e-14, want_vectors=False)
            print(name, (nu, nd), "E_A", e_a, "|<H_B> - E_A|", abs(e_b - e_a), "res_A", res_a, "res_B", res_b, "|E0_B - E_A|", abs(evb[0] - e_a))
            assert abs(e_b - e_a) <= 1e-12
            assert res_b <= 2 * res_a + 1e-12
            assert ncb == 1 and abs(evb[0] - e_a) <= 1e-10
        finally:
            _close(a, b)


def _swap_spins(rec, nimp):
    n = 4 ** nimp
    w = rec[:n].reshape(2 ** nimp, 2 ** nimp).T.ravel()   # W[a_up + 2^Nimp a_dw] <-> W[a_dw + 2^Nimp a_up]
    r = 2 * nimp * nimp
    return np.concatenate([w, rec[n + r: n + 2 * r], rec[n: n + r]])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["chain", "bhz"])
def test_observables_of_the_twin_have_the_spins_swapped(built, order_mode, name, mode):
    order_mode(mode, 8)
    m, (nup, ndw) = (_chain(8), (3, 5)) if name == "chain" else (_bhz_complex(), (2, 3))
    a, b = _open_pair(m, nup, ndw)
    try:
        if name == "chain":
            assert (a.row_perm is not None) == (mode != "off") and (b.row_perm is not None) == (mode != "off")
        v = _rand(a.Dim, 31)
        v /= np.linalg.norm(v)
        d = a.vector_from_host(v)
        rec_a = a.observables_record(d, weight=0.7)
        rec_b = b.observables_record(a.twin_vector(b, d), weight=0.7)
        assert rec_a.size == 4 ** m.Nimp + 4 * m.Nimp ** 2
        assert np.abs(rec_b - rec_a).max() > 1e-3                     # the sectors differ: the swap is not trivial
        assert np.abs(rec_b - _swap_spins(rec_a, m.Nimp)).max() <= 1e-12
    finally:
        _close(a, b)


def test_twin_vector_refusals(built, monkeypatch):
    import torch
    import hxv
    from oracle.oracle import OracleSector

    monkeypatch.setenv("HXV_ROW_ORDER", "0")
    hxv.sector_cache_clear()
    L = hxv.load_library()
    m = _chain(6)
    a, b, sym = hxv.HxvSector.from_model(m, 1, 3), hxv.HxvSector.from_model(m, 3, 1), hxv.HxvSector.from_model(m, 3, 3)
    other = hxv.HxvSector.from_model(m, 2, 3)
    half = hxv.HxvSector.from_model(m, 3, 1, rank=0, nranks=2)
    orc = OracleSector(m, 3, 1)
    fc = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag())
    try:
        n = max(s.localElems for s in (a, b, sym, other, half, fc))
        x = torch.zeros(n, dtype=torch.complex128, device="cuda")
        y = torch.full((n,), complex(3.0, -4.0), dtype=torch.complex128, device="cuda")
        keep = y.clone()
        torch.cuda.synchronize()

        def refused(frm, to, psi, out, status):
            rc = L.hxv_twin_vector(frm, to, psi, out)
            msg = L.hxv_last_error().decode()
            assert rc == status, (rc, status, msg)
            assert "hxv_twin_vector" in msg and len(msg) > len("hxv_twin_vector")
            torch.cuda.synchronize()
            assert torch.equal(y, keep)        # a refused call writes nothing

        px, py = x.data_ptr(), y.data_ptr()
        ARG, STATE, UNSUPPORTED = 1, 3, 4
        refused(a._h, other._h, px, py, ARG)       # (2,3) is not the twin of (1,3)
        refused(a._h, a._h, px, py, ARG)           # nor is (1,3) itself
        refused(sym._h, sym._h, py, py, ARG)       # d_out == d_psi
        refused(a._h, fc._h, px, py, STATE)        # a handle from stored matrices has no basis maps
        refused(fc._h, a._h, px, py, STATE)
        refused(a._h, half._h, px, py, UNSUPPORTED)  # a split sector
        refused(half._h, a._h, px, py, UNSUPPORTED)
        refused(None, b._h, px, py, ARG)
        refused(a._h, None, px, py, ARG)
        refused(a._h, b._h, None, py, ARG)
        refused(a._h, b._h, px, None, ARG)
        with pytest.raises(hxv.HxvError, match=r"status 1\).*twin"):
            a.twin_vector(other, x[: a.localElems].contiguous())
        assert L.hxv_twin_vector(a._h, b._h, px, py) == 0     # and the pair that is one goes through
    finally:
        _close(a, b, sym, other, half, fc)
        hxv.sector_cache_clear()
