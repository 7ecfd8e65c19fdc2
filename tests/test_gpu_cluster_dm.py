"""Cluster reduced density matrix of device-resident states (include/hxv.h, hxv_cluster_dm_accumulate) on the MI355X: the device matrix
against the numpy one (tests/cluster_dm_ref.py) on every sector of small models, device row order on and off, Nimp 1 to 5, split sectors,
the merged record's histogram, the closed form of a Slater determinant, end to end from the device eigensolver, determinism and errors."""
import numpy as np
import pytest

from cluster_dm_ref import entropy_and_purity, gaussian_entropy_and_purity, literal, vectorised

pytestmark = pytest.mark.gpu


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


def _matches(m, sectors, seed=0, tol=1e-13):
    """device matrix == vectorised() on a random normalised complex vector, weight 0.7; returns how many sectors took a device row order"""
    import torch
    import hxv

    n = 0
    for k, (nup, ndw) in enumerate(sectors):
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        mu, md = sec.maps()
        v = _rand(sec.Dim, seed + k)
        got = sec.cluster_dm(sec.pad(torch.from_numpy(v).cuda()), weight=0.7)
        ref = vectorised(m, mu, md, v, 0.7)
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        print((nup, ndw), "max error", err)
        assert err < tol, ((nup, ndw), err)
        n += sec.row_perm is not None
        sec.close()
    return n


def _all_sectors(m):
    return [(u, d) for u in range(m.Ns + 1) for d in range(m.Ns + 1)]


@pytest.mark.parametrize("row_order", ["default", "off", "forced"])
def test_matrix_on_every_sector_of_a_chain(built, row_order, monkeypatch):
    """Ns = 8 chain (Nimp 4): every sector, the DimUp = 1 and DimDw = 1 ones included, in the default order and with the row order switched
    off.  "forced": the Ns = 12 chain with the device row order switched on for small sectors by the hooks of tests/test_gpu_observables.py."""
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
            n = _matches(m, [(6, 6), (5, 7), (7, 2), (2, 0), (4, 12), (11, 6)], seed=50)
            assert n >= 4, n
        else:
            m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
            n = _matches(m, _all_sectors(m))
            if row_order == "off":
                assert n == 0
    finally:
        hxv.sector_cache_clear()


def test_matrix_in_the_default_device_row_order_at_dimup_12870(built):
    """The C3 geometry (Ns = 16, Nimp 4): DimUp = 12870 sectors take the device row order by default."""
    import hxv
    from hxv import models

    m = models.hm_2dsquare()
    sec = hxv.HxvSector.from_model(m, 8, 2)
    assert hxv.load_library().hxv_row_order(sec._h, None, None) == 1
    sec.close()
    assert _matches(m, [(8, 2), (2, 8)], seed=5) >= 1


@pytest.mark.parametrize("nlat,sector", [(1, (1, 1)), (2, (2, 2)), (5, (5, 5))])
def test_matrix_at_nimp_1_2_and_5(built, nlat, sector):
    """Chains with one bath level; Nimp 5, sector (5,5): the 100 x 100 blocks of the classes with two or three impurity particles per spin."""
    from hxv import models

    _matches(models.hm_1dchain(Nlat=nlat, Nbath=1, eps_bath=[0.3], xmu=0.1), [sector], seed=20 + nlat)


@pytest.mark.parametrize("kind", ["bhz", "jxjp"])
def test_matrix_complex_and_spin_exchange_models(built, kind):
    from hxv import models

    if kind == "bhz":
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=1.5, Ust=0.5, Jh=0.1)   # Nimp 4, Ns 8, complex impHloc
        _matches(m, _all_sectors(m), seed=100)
    else:
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15)
        _matches(m, [(4, 4), (3, 5), (0, 8), (8, 1)], seed=200)


@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.mark.parametrize("nranks,exchange", [(2, "allgather"), (3, "halo"), (4, "alltoall")])
def test_matrix_on_split_sectors(built, transport, nranks, exchange):
    """Sector (5,4) of the Ns = 8 chain: DimDw = 70, so bath runs straddle the uneven rank boundaries.  Every rank returns the global matrix,
    equal to the unsplit one, whatever exchange the products use."""
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    nup, ndw = 5, 4
    full = hxv.HxvSector.from_model(m, nup, ndw)
    v = _rand(full.Dim, 7)
    ref = full.cluster_dm(full.pad(torch.from_numpy(v).cuda()), weight=0.3)
    full.close()
    hxv.set_exchange_default(exchange)
    try:
        def rank(r, group):
            s = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
            group.join(s)
            slab = s.pad(torch.from_numpy(v[s.mpiIshift: s.mpiIshift + s.vecDim].copy()).cuda(), s.mpiQdw)
            out = s.cluster_dm(slab, weight=0.3)
            s.close()
            return out

        res = hxv.run_ranks(nranks, rank, transport=transport)
    finally:
        hxv.set_exchange_default("allgather")
    assert abs(np.trace(ref) - 0.3) < 1e-13
    for got in res:
        assert np.abs(got - ref).max() < 1e-13


def test_diagonal_is_the_device_records_histogram(built):
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    sec = hxv.HxvSector.from_model(m, 4, 3)
    d = sec.pad(torch.from_numpy(_rand(sec.Dim, 3)).cuda())
    rho = sec.cluster_dm(d, weight=0.7)
    rec = sec.observables_record(d, weight=0.7)
    sec.close()
    assert np.abs(np.diag(rho).real - rec[:4 ** 4]).max() < 1e-13 and not np.any(np.diag(rho).imag)


@pytest.mark.parametrize("kind", ["chain", "bhz"])
def test_closed_form_of_a_slater_determinant(built, kind):
    """U = 0 at Ns = 8 (tests/onebody.py): entropy and purity of the device matrix against the Gaussian closed form."""
    import hxv
    from hxv import models
    from onebody import slater_vector

    if kind == "chain":
        m, nup, ndw, lu, ld = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1, U=0.0), 4, 3, (0, 1, 2, 4), (0, 2, 3)
    else:
        m, nup, ndw, lu, ld = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=0.0), 4, 4, (0, 1, 2, 3), (0, 1, 3, 5)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    mu, md = sec.maps()
    v, _ = slater_vector(m, mu, md, lu, ld)
    rho = sec.cluster_dm(sec.vector_from_host(v))
    sec.close()
    S, pur = entropy_and_purity(rho)
    S0, pur0 = gaussian_entropy_and_purity(m, lu, ld)
    print("entropy error", S - S0, "purity error", pur - pur0)
    assert abs(S - S0) < 1e-12 and abs(pur - pur0) < 1e-12


def test_end_to_end_from_the_device_eigensolver(built):
    """eigh_lowest on the device -> observables.cluster_density_matrix with beta = 20, against the oracle's eigenvectors through the literal
    loops, on the four sectors of tests/test_gpu_observables.py (non-degenerate lowest level, checked on the oracle's spectrum)."""
    import hxv
    from hxv import models, observables
    from oracle.oracle import OracleSector

    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.15)    # Ns = 6
    dev_states, ref_states = [], []
    for nup, ndw in [(3, 3), (3, 2), (2, 3), (4, 3)]:
        o = OracleSector(m, nup, ndw)
        e, vv = np.linalg.eigh(o.dense())
        assert e[1] - e[0] > 1e-6
        ref_states.append((o.map_up(), o.map_dw(), vv[:, 0].copy(), e[0]))
        o.close()
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        ev, vecs, nc, _ = sec.eigh_lowest(1, tol=1e-13, native=True)
        assert nc >= 1 and abs(ev[0] - e[0]) < 1e-10
        dev_states.append((sec, ev[0], vecs[0].contiguous()))
    got = observables.cluster_density_matrix(m, dev_states, beta=20.0)
    w = observables.thermal_weights([s[3] for s in ref_states], 20.0)
    ref = literal(m, [(mu, md, v, wi) for (mu, md, v, _), wi in zip(ref_states, w)])
    assert got.shape == (16, 16) and abs(np.trace(got) - 1.0) < 1e-12
    assert np.abs(got - ref).max() < 1e-9
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
    r1 = sec.cluster_dm(a, 0.25)
    r2 = sec.cluster_dm(a, 0.25)
    assert np.array_equal(r1, r2)
    rb = sec.cluster_dm(b, 0.75)
    acc = sec.cluster_dm(a, 0.25)
    sec.cluster_dm(b, 0.75, out=acc, accumulate=True)
    assert np.array_equal(acc, r1 + rb)
    assert not np.any(sec.cluster_dm(a, 0.0))
    L = hxv.load_library()
    pd = C.POINTER(C.c_double)
    assert L.hxv_cluster_dm_elems(sec._h) == 2 * 16 ** 4
    out = np.zeros(2 * 16 ** 4)
    assert L.hxv_cluster_dm_accumulate(None, a.data_ptr(), 1.0, 0, out.ctypes.data_as(pd)) == 1
    assert L.hxv_cluster_dm_accumulate(sec._h, None, 1.0, 0, out.ctypes.data_as(pd)) == 1
    assert L.hxv_cluster_dm_accumulate(sec._h, a.data_ptr(), 1.0, 0, None) == 1
    # a handle built from stored matrices has no basis maps
    from oracle.oracle import OracleSector

    o = OracleSector(m, 4, 4)
    cs = hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag())
    o.close()
    assert L.hxv_cluster_dm_elems(cs._h) == 0
    d = torch.zeros(cs.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_cluster_dm_accumulate(cs._h, d.data_ptr(), 1.0, 0, out.ctypes.data_as(pd)) == 3
    cs.close()
    # a dw panel
    mp, keep = hxv.HxvSector._model_struct(m)
    ph = C.c_void_p()
    assert L.hxv_create_dw_panel(C.byref(mp), 4, 4, 16, 0, C.byref(ph)) == 0
    assert L.hxv_cluster_dm_elems(ph) == 0
    assert L.hxv_cluster_dm_accumulate(ph, a.data_ptr(), 1.0, 0, out.ctypes.data_as(pd)) == 3
    L.hxv_destroy(ph)
    del keep
    # a split sector without its communicator
    half = hxv.HxvSector.from_model(m, 4, 4, rank=0, nranks=2)
    dh = torch.zeros(half.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_cluster_dm_accumulate(half._h, dh.data_ptr(), 1.0, 0, out.ctypes.data_as(pd)) == 3
    half.close()
    # Nimp = 6 > 5
    big = models.hm_1dchain(Nlat=6, Nbath=0)
    sb = hxv.HxvSector.from_model(big, 1, 1)
    db = torch.zeros(sb.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_cluster_dm_elems(sb._h) == 0
    assert L.hxv_cluster_dm_accumulate(sb._h, db.data_ptr(), 1.0, 0, out.ctypes.data_as(pd)) == 4
    sb.close()
    sec.close()
