"""Reduced density matrix of an impurity-orbital subset of device-resident states (include/hxv.h, hxv_reduced_dm_accumulate) on the MI355X:
the device matrix against the numpy one (tests/reduced_dm_ref.py direct) in both sign conventions on every sector of small models, device
row order on and off, Nimp 6 (where the dense cluster matrix ends), complex and spin-exchange models, the full mask against the cluster
matrix, the diagonal against the merged record, split sectors, the closed form of a Slater determinant, end to end from the device
eigensolver, determinism, the table cache and errors."""
import numpy as np
import pytest

from cluster_dm_ref import entropy_and_purity, literal
from reduced_dm_ref import direct, gaussian_entropy_and_purity_subset, mask_int, masked_trace_literal

pytestmark = pytest.mark.gpu
TOL = 1e-13   # the cluster matrix's own tolerance (tests/test_gpu_cluster_dm.py)


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


def _matches(m, sectors, masks, seed=0):
    """device matrix == direct() on a random normalised complex vector, weight 0.7, every mask, both conventions; returns how many sectors
    took a device row order"""
    import torch
    import hxv

    n, worst = 0, 0.0
    for k, (nup, ndw) in enumerate(sectors):
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        mu, md = sec.maps()
        v = _rand(sec.Dim, seed + k)
        d = sec.pad(torch.from_numpy(v).cuda())
        for mask in masks:
            for fs in (0, 1):
                got = sec.reduced_dm(d, mask, weight=0.7, fermi_sign=bool(fs))
                ref = direct(m, mu, md, v, mask, 0.7, fs)
                assert got.shape == ref.shape
                err = np.abs(got - ref).max()
                worst = max(worst, err)
                assert err < TOL, ((nup, ndw), mask, fs, err)
                assert np.array_equal(got, got.conj().T) and not np.any(np.diag(got).imag)
        n += sec.row_perm is not None
        sec.close()
    print(len(sectors), "sectors,", len(masks), "masks: max error", worst)
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
    masks = [(0,), (3,), (0, 2), (1, 3), (0, 2, 3), (0, 1, 2, 3)]
    try:
        if row_order == "forced":
            m = models.hm_1dchain(eps_bath=[0.3, -0.2])
            n = _matches(m, [(6, 6), (5, 7), (7, 2), (2, 0), (4, 12)], masks, seed=50)
            assert n >= 3, n
        else:
            m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
            n = _matches(m, _all_sectors(m), masks)
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
    assert _matches(m, [(8, 2), (2, 8)], [(0, 3), (1,)], seed=5) >= 1


@pytest.mark.parametrize("nbath,sectors", [(0, [(3, 3)]), (1, [(6, 6), (5, 7)])])
def test_matrix_at_nimp_6(built, nbath, sectors):
    """Nimp 6: no dense cluster matrix (hxv_cluster_dm_elems is 0).  Nbath = 0: the environment is traced impurity orbitals only."""
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=6, Nbath=nbath)
    masks = [(0,), (2, 3), (0, 5), (1, 2, 4, 5)]
    sec = hxv.HxvSector.from_model(m, *sectors[0])
    L = hxv.load_library()
    assert L.hxv_cluster_dm_elems(sec._h) == 0
    for mask in masks:
        assert L.hxv_reduced_dm_elems(sec._h, mask_int(mask)) == 2 * 16 ** len(mask)
    sec.close()
    _matches(m, sectors, masks, seed=300 + nbath)


@pytest.mark.parametrize("kind", ["bhz", "jxjp"])
def test_matrix_complex_and_spin_exchange_models(built, kind):
    from hxv import models

    masks = [(0, 1), (0, 2)]   # one site; one orbital of each site
    if kind == "bhz":
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=1.5, Ust=0.5, Jh=0.1)   # Nimp 4, Ns 8, complex impHloc
        _matches(m, _all_sectors(m), masks, seed=100)
    else:
        m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15)
        _matches(m, [(4, 4), (3, 5), (0, 8), (8, 1)], masks, seed=200)


def test_full_mask_is_the_cluster_matrix_and_the_diagonal_is_the_records_histogram(built):
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    sec = hxv.HxvSector.from_model(m, 4, 3)
    d = sec.pad(torch.from_numpy(_rand(sec.Dim, 3)).cuda())
    cdm = sec.cluster_dm(d, weight=0.7)
    for fs in (False, True):   # no traced impurity orbital: no sign either way
        full = sec.reduced_dm(d, range(4), weight=0.7, fermi_sign=fs)
        print("full mask, fermi_sign", fs, "bit-identical to cluster_dm:", np.array_equal(full, cdm), "max difference", np.abs(full - cdm).max())
        assert np.abs(full - cdm).max() < TOL
    W = sec.observables_record(d, weight=0.7)[:4 ** 4].reshape(16, 16)   # [a_dw, a_up]
    for mask in [(0,), (1, 3), (0, 2, 3)]:
        nw = 1 << len(mask)
        pext = np.array([sum(((a >> b) & 1) << k for k, b in enumerate(mask)) for a in range(16)])
        marg = np.zeros((nw, nw))
        np.add.at(marg, (pext[:, None], pext[None, :]), W)
        for fs in (False, True):
            rho = sec.reduced_dm(d, mask, weight=0.7, fermi_sign=fs)
            assert np.abs(np.diag(rho).real - marg.reshape(-1)).max() < TOL and not np.any(np.diag(rho).imag)
    sec.close()


def test_pad_rows_are_never_read(built):
    """The layout contract of tests/test_gpu_layout_contract.py: DimUp = 70 in a pitch of 72, NaN in the pad rows changes no bit; both kernels
    (mask {0,2}: the pair kernel, {0,1,2,3}: the tile kernel), row order at its default."""
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    sec = hxv.HxvSector.from_model(m, 4, 3)
    assert sec.pitch > sec.DimUp
    d = sec.pad(torch.from_numpy(_rand(sec.Dim, 9)).cuda())
    bad = d.clone()
    bad.view(sec.DimDw, sec.pitch)[:, sec.DimUp:] = complex(float("nan"), float("nan"))
    for mask in [(0, 2), (0, 1, 2, 3)]:
        for fs in (False, True):
            assert np.array_equal(sec.reduced_dm(d, mask, 0.7, fermi_sign=fs), sec.reduced_dm(bad, mask, 0.7, fermi_sign=fs))
    sec.close()


@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.mark.parametrize("nranks,exchange", [(2, "allgather"), (3, "halo"), (4, "alltoall")])
def test_matrix_on_split_sectors(built, transport, nranks, exchange):
    """Sector (5,4) of the Ns = 8 chain, mask {0,2}: the dw groups are scattered columns that straddle the uneven rank boundaries.  Every rank
    returns the global matrix, equal to the unsplit one, whatever exchange the products use."""
    import torch
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1)
    nup, ndw, mask = 5, 4, (0, 2)
    full = hxv.HxvSector.from_model(m, nup, ndw)
    v = _rand(full.Dim, 7)
    dv = full.pad(torch.from_numpy(v).cuda())
    ref = [full.reduced_dm(dv, mask, weight=0.3, fermi_sign=bool(fs)) for fs in (0, 1)]
    mu, md = full.maps()
    full.close()
    for fs in (0, 1):
        assert np.abs(ref[fs] - direct(m, mu, md, v, mask, 0.3, fs)).max() < TOL
    hxv.set_exchange_default(exchange)
    try:
        def rank(r, group):
            s = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
            group.join(s)
            slab = s.pad(torch.from_numpy(v[s.mpiIshift: s.mpiIshift + s.vecDim].copy()).cuda(), s.mpiQdw)
            out = [s.reduced_dm(slab, mask, weight=0.3, fermi_sign=bool(fs)) for fs in (0, 1)]
            s.close()
            return out

        res = hxv.run_ranks(nranks, rank, transport=transport)
    finally:
        hxv.set_exchange_default("allgather")
    for got in res:
        for fs in (0, 1):
            assert np.abs(got[fs] - ref[fs]).max() < TOL


@pytest.mark.parametrize("kind", ["chain", "bhz"])
def test_closed_form_of_a_slater_determinant(built, kind):
    """U = 0 at Ns = 8 (tests/onebody.py), mask {0,2}: with the Fermi sign the device matrix has the entropy and purity of the Gaussian closed
    form; the reference's convention misses the entropy by more than 1e-2 (tests/test_reduced_dm_cpu.py: -4.2e-2 chain, +1.0e-1 BHZ)."""
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
    d = sec.vector_from_host(v)
    S1, pur1 = entropy_and_purity(sec.reduced_dm(d, (0, 2), fermi_sign=True))
    S0, pur0 = entropy_and_purity(sec.reduced_dm(d, (0, 2), fermi_sign=False))
    sec.close()
    Sg, purg = gaussian_entropy_and_purity_subset(m, lu, ld, (0, 2))
    print("fermi sign: entropy error", S1 - Sg, "purity error", pur1 - purg, "; reference sign: entropy gap", S0 - Sg)
    assert abs(S1 - Sg) < 1e-12 and abs(pur1 - purg) < 1e-12
    assert abs(S0 - Sg) > 1e-2


def test_end_to_end_from_the_device_eigensolver(built):
    """eigh_lowest on the device -> observables.reduced_density_matrix with beta = 20 and mask {0}, against the oracle's eigenvectors through
    the reference's masked trace of the literal cluster matrix, on the four sectors of tests/test_gpu_cluster_dm.py."""
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
    got = observables.reduced_density_matrix(m, dev_states, (0,), beta=20.0)
    mask2d = np.zeros((m.Nlat, m.Norb), dtype=bool)
    mask2d.reshape(-1)[0] = True
    assert np.array_equal(got, observables.reduced_density_matrix(m, dev_states, mask2d, beta=20.0))
    w = observables.thermal_weights([s[3] for s in ref_states], 20.0)
    ref, signs = masked_trace_literal(literal(m, [(mu, md, v, wi) for (mu, md, v, _), wi in zip(ref_states, w)]), 2, (0,))
    assert signs == {1.0}
    assert got.shape == (4, 4) and abs(np.trace(got) - 1.0) < 1e-12
    assert np.abs(got - ref).max() < 1e-9
    for s, _, _ in dev_states:
        s.close()


def test_determinism_accumulation_cache_and_errors(built):
    import ctypes as C

    import torch
    import hxv
    from hxv import models

    m = models.hm_2dsquare(Nbath=1)   # Ns = 8, Nimp 4
    hxv.sector_cache_clear()
    sec = hxv.HxvSector.from_model(m, 4, 4)
    va, vb = _rand(sec.Dim, 1), _rand(sec.Dim, 2)
    a = sec.pad(torch.from_numpy(va).cuda())
    b = sec.pad(torch.from_numpy(vb).cuda())
    A, B = (0, 2), (1, 2, 3)
    r1 = sec.reduced_dm(a, A, 0.25)
    assert np.array_equal(r1, sec.reduced_dm(a, A, 0.25))
    rb = sec.reduced_dm(b, A, 0.75)
    acc = sec.reduced_dm(a, A, 0.25)
    sec.reduced_dm(b, A, 0.75, out=acc, accumulate=True)
    assert np.array_equal(acc, r1 + rb)
    assert not np.any(sec.reduced_dm(a, A, 0.0))
    # mask A, then B, then A; the other convention of A in between; more masks than the image keeps tables for
    rB = sec.reduced_dm(a, B, 0.25)
    r1f = sec.reduced_dm(a, A, 0.25, fermi_sign=True)
    assert rB.shape == (64, 64) and not np.array_equal(r1f, r1)
    assert np.array_equal(r1, sec.reduced_dm(a, A, 0.25))
    others = [(0,), (1,), (2,), (3,), (0, 1), (1, 2), (2, 3), (0, 3), (1, 3), (0, 1, 2)]
    first = [sec.reduced_dm(a, o, 0.25) for o in others]
    assert np.array_equal(r1, sec.reduced_dm(a, A, 0.25)) and np.array_equal(rB, sec.reduced_dm(a, B, 0.25))
    assert np.array_equal(r1f, sec.reduced_dm(a, A, 0.25, fermi_sign=True))
    for o, f in zip(others, first):
        assert np.array_equal(f, sec.reduced_dm(a, o, 0.25))
    # a fresh image gives the same bits
    sec.close()
    hxv.sector_cache_clear()
    sec = hxv.HxvSector.from_model(m, 4, 4)
    assert np.array_equal(r1, sec.reduced_dm(a, A, 0.25)) and np.array_equal(rB, sec.reduced_dm(a, B, 0.25))
    # status codes
    L = hxv.load_library()
    pd = C.POINTER(C.c_double)
    out = np.zeros(2 * 16 ** 4)
    po = out.ctypes.data_as(pd)
    assert L.hxv_reduced_dm_elems(sec._h, 0b0101) == 2 * 16 ** 2 and L.hxv_reduced_dm_elems(sec._h, 0b1111) == 2 * 16 ** 4
    assert L.hxv_reduced_dm_elems(sec._h, 0) == 0 and L.hxv_reduced_dm_elems(sec._h, 0b10000) == 0
    assert L.hxv_reduced_dm_accumulate(None, a.data_ptr(), 1, 0, 1.0, 0, po) == 1
    assert L.hxv_reduced_dm_accumulate(sec._h, None, 1, 0, 1.0, 0, po) == 1
    assert L.hxv_reduced_dm_accumulate(sec._h, a.data_ptr(), 1, 0, 1.0, 0, None) == 1
    assert L.hxv_reduced_dm_accumulate(sec._h, a.data_ptr(), 0, 0, 1.0, 0, po) == 1          # empty mask
    assert L.hxv_reduced_dm_accumulate(sec._h, a.data_ptr(), 0b10001, 0, 1.0, 0, po) == 1    # bit 4 of Nimp = 4
    assert L.hxv_reduced_dm_accumulate(sec._h, a.data_ptr(), 1, 2, 1.0, 0, po) == 1          # fermi_sign
    assert L.hxv_reduced_dm_accumulate(sec._h, a.data_ptr(), 1, -1, 1.0, 0, po) == 1
    assert not np.any(out)
    with pytest.raises(hxv.HxvError):
        sec.reduced_dm(a, (0, 4))
    # a handle built from stored matrices has no basis maps
    from oracle.oracle import OracleSector

    o = OracleSector(m, 4, 4)
    cs = hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag())
    o.close()
    assert L.hxv_reduced_dm_elems(cs._h, 1) == 0
    d = torch.zeros(cs.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_reduced_dm_accumulate(cs._h, d.data_ptr(), 1, 0, 1.0, 0, po) == 3
    cs.close()
    # a dw panel
    mp, keep = hxv.HxvSector._model_struct(m)
    ph = C.c_void_p()
    assert L.hxv_create_dw_panel(C.byref(mp), 4, 4, 16, 0, C.byref(ph)) == 0
    assert L.hxv_reduced_dm_elems(ph, 1) == 0
    assert L.hxv_reduced_dm_accumulate(ph, a.data_ptr(), 1, 0, 1.0, 0, po) == 3
    L.hxv_destroy(ph)
    del keep
    # a split sector without its communicator
    half = hxv.HxvSector.from_model(m, 4, 4, rank=0, nranks=2)
    dh = torch.zeros(half.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_reduced_dm_accumulate(half._h, dh.data_ptr(), 1, 0, 1.0, 0, po) == 3
    half.close()
    # five orbitals (Nimp = 6)
    big = models.hm_1dchain(Nlat=6, Nbath=0)
    sb = hxv.HxvSector.from_model(big, 1, 1)
    db = torch.zeros(sb.localElems, dtype=torch.complex128, device="cuda")
    assert L.hxv_reduced_dm_elems(sb._h, 0b11111) == 0 and L.hxv_reduced_dm_elems(sb._h, 0b101101) == 2 * 16 ** 4
    assert L.hxv_reduced_dm_accumulate(sb._h, db.data_ptr(), 0b11111, 0, 1.0, 0, po) == 4
    assert L.hxv_reduced_dm_accumulate(sb._h, db.data_ptr(), 0b1000000, 0, 1.0, 0, po) == 1   # bit 6 of Nimp = 6
    sb.close()
    sec.close()
    hxv.sector_cache_clear()
