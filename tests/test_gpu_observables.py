"""Impurity observables of device-resident states (include/hxv.h, hxv_observables_accumulate) on the MI355X: the device record against the
numpy record (tests/observables_ref.py) on every sector of small models, device row order on and off, split sectors, closed forms at the
headline size, end to end from the device eigensolver, determinism and errors."""
import numpy as np
import pytest

from observables_ref import literal, record_numpy

pytestmark = pytest.mark.gpu


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


def _record_matches(m, sectors, seed=0, tol=1e-13):
    import torch
    import hxv

    n = 0
    for k, (nup, ndw) in enumerate(sectors):
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        mu, md = sec.maps()
        v = _rand(sec.Dim, seed + k)
        d = sec.pad(torch.from_numpy(v).cuda())
        got = sec.observables_record(d, weight=0.7)
        ref = record_numpy(m, mu, md, v, 0.7)
        assert np.abs(got - ref).max() < tol, ((nup, ndw), np.abs(got - ref).max())
        n += sec.row_perm is not None
        sec.close()
    return n


def _all_sectors(m):
    return [(u, d) for u in range(m.Ns + 1) for d in range(m.Ns + 1)]


@pytest.mark.parametrize("row_order", ["default", "off", "forced"])
def test_record_on_every_sector_of_a_chain(built, row_order, monkeypatch):
    """Ns = 8 chain (Nimp 4): every sector, nup = 0, DimUp = 1 and DimDw = 1 ones included, in the default order (these sectors are below the
    row order's size threshold) and with the row order switched off.  "forced": the C2 chain (Ns = 12) with the device row order switched on
    for small sectors by the hooks tests/test_gpu_row_order.py uses, asserted on."""
    import hxv
    from hxv import models

    if row_order == "off":
        monkeypatch.setenv("HXV_ROW_ORDER", "0")
    elif row_order == "forced":
        monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
        monkeypatch.setenv("HXV_ROW_ORDER_BITS", "8")
    hxv.sector_cache_clear()
    try:
        if row_order == "forced":
            m = models.hm_1dchain(eps_bath=[0.3, -0.2])
            n = _record_matches(m, [(6, 6), (5, 7), (7, 2), (2, 0), (4, 12), (11, 6)], seed=50)
            assert n >= 4, n
        else:
            m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
            n = _record_matches(m, _all_sectors(m))
            if row_order == "off":
                assert n == 0
    finally:
        hxv.sector_cache_clear()


def test_record_in_the_default_device_row_order_at_dimup_12870(built):
    """The C3 geometry (Ns = 16, Nimp 4): DimUp = 12870 sectors take the device row order by default."""
    import hxv
    from hxv import models

    m = models.hm_2dsquare()
    sec = hxv.HxvSector.from_model(m, 8, 2)
    assert hxv.load_library().hxv_row_order(sec._h, None, None) == 1
    sec.close()
    assert _record_matches(m, [(8, 2), (2, 8)], seed=5) >= 1


OTHER_NIMP = {1: (lambda M: M.hm_1dchain(Nlat=1, Nbath=3), [(2, 2), (2, 0)]),
              3: (lambda M: M.hm_1dchain(Nlat=3, Nbath=1), [(3, 2), (3, 6)]),
              5: (lambda M: M.hm_1dchain(Nlat=5, Nbath=1), [(5, 4), (5, 0)]),
              8: (lambda M: M.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), [(4, 3), (4, 8)]),
              10: (lambda M: M.hm_1dchain(Nlat=10, Nbath=0), [(5, 4)])}


@pytest.mark.parametrize("row_order", ["off", "forced"])
@pytest.mark.parametrize("nimp", sorted(OTHER_NIMP))
def test_record_at_other_impurity_sizes(built, nimp, row_order, monkeypatch):
    """Nimp in {1, 3, 5, 8, 10}: fewer W bins than waves, pair counts that are no multiple of four, both lookup widths of o >> nimp, the whole
    LDS array of the dw pass; with each of the first four one sector with DimDw = 1.  In the reference's row order, and with the device row
    order forced by the hooks of tests/test_gpu_row_order.py: with Ns - 1 block bits the last impurity orbital and the last bath orbital but
    one are tied to the one high orbital, so the chains with a bath get a row order (asserted); the open 10-site chain has no orbital to move, and for the bath-less
    BHZ cluster the order is not asserted."""
    import hxv
    from hxv import models

    make, sectors = OTHER_NIMP[nimp]
    m = make(models)
    assert m.Nlat * m.Norb == nimp
    if row_order == "off":
        monkeypatch.setenv("HXV_ROW_ORDER", "0")
    else:
        monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "4")
        monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(m.Ns - 1))
    hxv.sector_cache_clear()
    try:
        n = _record_matches(m, sectors, seed=300 + nimp)
        if row_order == "off":
            assert n == 0
        elif nimp in (1, 3, 5):
            assert n == len(sectors), n
    finally:
        hxv.sector_cache_clear()


@pytest.mark.parametrize("kind", ["bhz", "jxjp"])
def test_record_complex_and_spin_exchange_models(built, kind):
    from hxv import models

    if kind == "bhz":
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=1.5, Ust=0.5, Jh=0.1)   # Nimp 4, Ns 8, complex impHloc
        _record_matches(m, _all_sectors(m), seed=100)
    else:
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15)
        _record_matches(m, [(4, 4), (3, 5), (0, 8), (8, 1)], seed=200)


@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.mark.parametrize("nranks,exchange", [(2, "allgather"), (3, "halo"), (4, "alltoall")])
def test_record_on_split_sectors(built, transport, nranks, exchange):
    """Every rank returns the global record, equal to the unsplit one, whatever exchange the products use."""
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    nup, ndw = 5, 4
    full = hxv.HxvSector.from_model(m, nup, ndw)
    v = _rand(full.Dim, 7)
    ref = full.observables_record(full.pad(torch.from_numpy(v).cuda()), weight=0.3)
    full.close()
    hxv.set_exchange_default(exchange)
    try:
        def rank(r, group):
            s = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
            group.join(s)
            slab = s.pad(torch.from_numpy(v[s.mpiIshift: s.mpiIshift + s.vecDim].copy()).cuda(), s.mpiQdw)
            out = s.observables_record(slab, weight=0.3)
            s.close()
            return out

        res = hxv.run_ranks(nranks, rank, transport=transport)
    finally:
        hxv.set_exchange_default("allgather")
    for got in res:
        assert np.abs(got - ref).max() < 1e-13


@pytest.mark.parametrize("name,levels_up,levels_dw", [("C3", (0, 1, 2, 3, 4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6, 7)), ("C3", (0, 1, 2, 3, 4, 5, 7, 10), (0, 2, 3, 4, 5, 6, 8, 13)),
                                                       ("C4", (0, 1, 2, 3, 4, 5, 6, 9), (1, 2, 3, 4, 5, 6, 7, 12))])
def test_closed_form_at_headline_size(built, name, levels_up, levels_dw):
    """U = 0: an exact Slater determinant (tests/onebody.py) at Dim = 1.66e8, the level sets of test_gpu_fullsize.py (ground state and excited
    determinants with different up and dw levels: a swap of the two spins in W or R shows).  R_s is the one-body projector on the occupied
    levels of spin s restricted to the impurity orbitals, <c^+_a c_b> = sum_k conj(Phi[a,k]) Phi[b,k]; docc = n_up n_dw orbital by orbital."""
    import torch
    import hxv
    from hxv import models, observables
    from onebody import one_body_matrix, slater_vector

    if name == "C3":
        m = models.hm_2dsquare(U=0.0)
    else:
        m = models.bhz_2d(Nx=2, Ny=2, Nbath=1, U=0.0)
    sec = hxv.HxvSector.from_model(m, 8, 8)
    mu, md = sec.maps()
    v, _ = slater_vector(m, mu, md, levels_up, levels_dw)
    # <v|v> summed pairwise: the normalisation inside slater_vector (a sequential sum of squares over 1.66e8 terms) leaves it 1 - O(1e-12)
    nrm2 = float(np.sum(v.real ** 2) + np.sum(v.imag ** 2))
    d = sec.vector_from_host(v)
    del v
    rec = sec.observables_record(d)
    del d
    torch.cuda.empty_cache()
    N = m.Nlat * m.Norb
    out = observables.derive(m, rec)
    for spin, lev in ((0, list(levels_up)), (1, list(levels_dw))):
        _, phi = np.linalg.eigh(one_body_matrix(m, spin if m.Nspin > 1 else 0))
        P = (np.conj(phi[:, lev]) @ phi[:, lev].T)[:N, :N]                     # P[a, b] = <c^+_a c_b>
        R = rec[4 ** N + 2 * N * N * spin: 4 ** N + 2 * N * N * (spin + 1)].view(np.complex128).reshape(N, N, order="F")
        assert np.abs(R - nrm2 * P).max() < 1e-12, (spin, np.abs(R - nrm2 * P).max())
        dn = np.real(np.diag(P)).reshape(m.Nlat, m.Norb)                        # is = iorb + ilat*Norb
        assert np.abs(out["dens_up" if spin == 0 else "dens_dw"] - nrm2 * dn).max() < 1e-12
    nu = out["dens_up"]
    nd = out["dens_dw"]
    assert np.abs(out["docc"] - nu * nd / nrm2).max() < 1e-12
    sec.close()


def test_end_to_end_from_the_device_eigensolver(built):
    """eigh_lowest on the device -> observables_record over the state list -> derive, against the oracle's eigenvectors through the literal
    loops.  Sectors with a non-degenerate lowest level (checked on the oracle's spectrum)."""
    import hxv
    from hxv import models, observables
    from oracle.oracle import OracleSector

    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.15)    # Ns = 6
    sectors = [(3, 3), (3, 2), (2, 3), (4, 3)]
    dev_states, ref_states = [], []
    for nup, ndw in sectors:
        o = OracleSector(m, nup, ndw)
        e, vv = np.linalg.eigh(o.dense())
        assert e[1] - e[0] > 1e-6
        ref_states.append((o.map_up(), o.map_dw(), vv[:, 0].copy(), e[0]))
        o.close()
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        ev, vecs, nc, _ = sec.eigh_lowest(1, tol=1e-13, native=True)
        assert nc >= 1 and abs(ev[0] - e[0]) < 1e-10
        dev_states.append((sec, ev[0], vecs[0].contiguous()))
    beta = 20.0
    got = observables.observables(m, dev_states, beta=beta)
    w = observables.thermal_weights([s[3] for s in ref_states], beta)
    ref = literal(m, [(mu, md, v, wi) for (mu, md, v, _), wi in zip(ref_states, w)])
    for k in ["dens", "dens_up", "dens_dw", "docc", "magz", "sz2", "n2", "s2tot", "Eknot", "Epot", "Ehartree", "single_particle_density_matrix"]:
        assert np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max() < 1e-9, k
    for s, _, _ in dev_states:
        s.close()


def test_determinism_accumulation_and_errors(built):
    import ctypes as C

    import torch
    import hxv
    from hxv import models

    m = models.hm_2dsquare(Nbath=1)   # Ns = 8, Nimp 4
    sec = hxv.HxvSector.from_model(m, 4, 4)
    a = sec.pad(torch.from_numpy(_rand(sec.Dim, 1)).cuda())
    b = sec.pad(torch.from_numpy(_rand(sec.Dim, 2)).cuda())
    r1 = sec.observables_record(a, 0.25)
    r2 = sec.observables_record(a, 0.25)
    assert np.array_equal(r1, r2)
    rb = sec.observables_record(b, 0.75)
    acc = sec.observables_record(a, 0.25)
    sec.observables_record(b, 0.75, out=acc, accumulate=True)
    assert np.array_equal(acc, r1 + rb)
    assert not np.any(sec.observables_record(a, 0.0))
    L = hxv.load_library()
    rec = np.zeros(L.hxv_obs_record_elems(sec._h))
    assert L.hxv_observables_accumulate(None, a.data_ptr(), 1.0, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert L.hxv_observables_accumulate(sec._h, None, 1.0, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert L.hxv_observables_accumulate(sec._h, a.data_ptr(), 1.0, 0, None) == 1
    # a handle built from stored matrices has no basis maps
    from oracle.oracle import OracleSector

    o = OracleSector(m, 4, 4)
    cs = hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag())
    o.close()
    assert L.hxv_obs_record_elems(cs._h) == 0
    d = torch.zeros(cs.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_observables_accumulate(cs._h, d.data_ptr(), 1.0, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 3
    cs.close()
    # Nimp = 11 > 10
    big = models.hm_1dchain(Nlat=11, Nbath=0)
    sb = hxv.HxvSector.from_model(big, 1, 1)
    db = torch.zeros(sb.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_observables_accumulate(sb._h, db.data_ptr(), 1.0, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 4
    sb.close()
    sec.close()
