"""Paired probe runs on the MI355X (include/hxv.h: hxv_lanczos_tridiag_pair_probes; HxvSector.lanczos_tridiag_pair_probes;
hxv.observables.susceptibility(paired=True)): two real channels and their overlaps with a shared probe list on ONE product per step.

  - alanc / blanc / overlaps / nsteps of each component are hxv_lanczos_tridiag_probes' on that start vector through the complex-vector
    kernels (real_vectors = 0, lanczos_graph = 0, job_up 2 and 0), bit for bit; without probes the call is hxv_lanczos_tridiag_pair, bit for bit
  - G_ij(i w_n) of the Ns = 8 square cluster from 2 paired runs per spin and side against the dense Lehmann sum          1e-9 (the tolerance of
    test_gpu_probes.py::test_off_diagonal_green_function_from_one_run_per_orbital)
  - susceptibility(paired=True) against paired=False and the Lehmann sum         1e-9 * max(1, max|chi_ref|) (test_gpu_density_ops.py's)
  - split sectors, determinism and buffers, errors."""
import ctypes as C

import numpy as np
import pytest
from ladder_ref import apply_op as _apply_op

import chi_ref

pytestmark = pytest.mark.gpu

BETA, LMATS = 50.0, 64
WM = np.pi / BETA * (2 * np.arange(1, LMATS + 1) - 1)   # ED_GF_SHARED.f90:49


def _unit(x):
    return x / np.linalg.norm(x)


def _rand(rng, n):
    return rng.standard_normal(n).astype(np.complex128)


# ---- 1. bit for bit against two single runs ---------------------------------------------------------------------------------------------
def _pair_case(case):
    """sector and start vectors of test_gpu_lanczos.py::test_paired_tridiagonalisation_is_two_single_runs_bit_for_bit"""
    from hxv import models
    from oracle.oracle import OracleSector

    if case == "C2":
        m, (nup, ndw), nl = models.hm_1dchain(), (6, 6), 30
    elif case == "breakdown_in_one":
        m, (nup, ndw), nl = models.hm_1dchain(Nlat=2, Nbath=1), (2, 2), 40   # Dim 36 < nl: the Krylov spaces close
    else:
        m, (nup, ndw), nl = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (3, 3), 25
    rng = np.random.default_rng(7)
    dim = OracleSector(m, nup, ndw).Dim
    xa, xb = _unit(rng.standard_normal(dim)), _unit(rng.standard_normal(dim))
    if case == "unequal_norms":
        xa, xb = 3.0 * xa, 0.25 * xb
    if case == "breakdown_in_one":
        # vector a lives in a small invariant subspace: an eigenvector of H -> its recurrence stops after one step
        w, U = np.linalg.eigh(OracleSector(m, nup, ndw).dense())
        xa = _unit(np.real(U[:, 3] * np.exp(-1j * np.angle(U[np.abs(U[:, 3]).argmax(), 3]))))
    return m, (nup, ndw), nl, xa.astype(np.complex128), xb.astype(np.complex128), rng


@pytest.mark.parametrize("case,nprobes", [("chain8", 1), ("chain8", 3), ("unequal_norms", 1), ("unequal_norms", 3), ("breakdown_in_one", 1),
                                          ("breakdown_in_one", 3), ("C2", 8)])
def test_paired_probe_run_is_two_single_probe_runs_bit_for_bit(built, case, nprobes):
    import hxv

    m, (nup, ndw), nl, xa, xb, rng = _pair_case(case)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    assert sec.real_vectors_available
    if case == "C2":
        assert sec.localElems > 1024 * 256        # the grid-stride loop runs more than once, lz_probe_final adds several partials per thread
    da, db = sec.vector_from_host(xa), sec.vector_from_host(xb)
    probes = [da] + [sec.vector_from_host(_rand(rng, sec.Dim)) for _ in range(nprobes - 1)]     # real random probes; one is vin_a itself
    sec.set_option("lanczos_graph", 0)
    sec.set_option("real_vectors", 0)
    for job_up in (2, 0):
        sec.set_option("job_up", job_up)
        ra, rb = sec.lanczos_tridiag_pair_probes(da, db, probes, nl)
        assert sec.get_option("lanczos_real_last") == 2
        for name, got, vin in (("a", ra, da), ("b", rb, db)):
            a1, b1, ov1, n1 = sec.lanczos_tridiag_probes(vin, probes, nl)
            assert sec.get_option("lanczos_real_last") == 0
            a, b, ov, n = got
            assert n == n1, (case, job_up, name, n, n1)
            assert ov.shape == (n, nprobes) and ov.dtype == np.complex128
            assert np.array_equal(a[:n], a1[:n]) and np.array_equal(b[:n], b1[:n]), (case, job_up, name, np.abs(a - a1).max(), np.abs(b - b1).max())
            assert np.array_equal(ov[:n].real, ov1[:n].real), (case, job_up, name, np.abs(ov.real - ov1.real).max())
            assert not ov.imag.any() and not ov1.imag.any()
            assert np.abs(ov).max() > 0
        if case == "breakdown_in_one":
            assert ra[3] < 5 and rb[3] > ra[3]
            # the whole arrays of the C entry: component a's overlaps past its breakdown are zero, b went on alone (matched above in every step)
            full = _raw_call(sec, da, db, probes, nl)
            assert full[0][3] == ra[3] and not full[0][2][ra[3]:].any() and not full[0][0][ra[3]:].any()
            assert np.array_equal(full[1][2][: rb[3]], rb[2]) and not full[1][2][rb[3]:].any()
        else:
            assert ra[3] == rb[3] == nl
            assert abs(ra[2][0, 0] - np.linalg.norm(xa)) <= 1e-13 * np.linalg.norm(xa)       # vin_a as its own probe: its norm comes first
        # no probe: the paired tridiagonalisation itself
        (a0, b0, ov0, n0), (a0b, b0b, ov0b, n0b) = sec.lanczos_tridiag_pair_probes(da, db, [], nl)
        (aa, ba, na), (ab, bb, nb) = sec.lanczos_tridiag_pair(da, db, nl)
        assert (n0, n0b) == (na, nb) and ov0.shape == (na, 0)
        assert np.array_equal(a0, aa) and np.array_equal(b0, ba) and np.array_equal(a0b, ab) and np.array_equal(b0b, bb)
        assert np.array_equal(a0[:na], ra[0][:na]) and np.array_equal(b0b[:nb], rb[1][:nb])    # ... and the probes change nothing in it
    sec.close()


def _raw_call(sec, va, vb, probes, nlanc, threshold=1e-12):
    """the C entry itself, whole output arrays (entries past nsteps included) -> (alanc, blanc, overlaps[nlanc, nprobes], nsteps) of a and of b"""
    import torch
    import hxv

    torch.cuda.synchronize()
    npr = len(probes)
    pd = C.POINTER(C.c_double)
    arr = [np.full(nlanc, 7.0) for _ in range(4)]
    ovs = [np.full(2 * nlanc * max(npr, 1), 7.0) for _ in range(2)]
    na, nb = C.c_int32(-1), C.c_int32(-1)
    plist = (C.c_void_p * max(npr, 1))(*[p.data_ptr() for p in probes])
    p = lambda x: x.ctypes.data_as(pd)  # noqa: E731
    rc = hxv.load_library().hxv_lanczos_tridiag_pair_probes(sec._h, va.data_ptr(), vb.data_ptr(), npr, plist, nlanc, p(arr[0]), p(arr[1]), p(ovs[0]),
                                                            p(arr[2]), p(arr[3]), p(ovs[1]), threshold, C.byref(na), C.byref(nb))
    assert rc == 0, hxv.load_library().hxv_last_error()
    ova, ovb = (o[: 2 * nlanc * npr].view(np.complex128).reshape(nlanc, npr) for o in ovs)
    return (arr[0], arr[1], ova, na.value), (arr[2], arr[3], ovb, nb.value)


# ---- 2. Green's function ----------------------------------------------------------------------------------------------------------------
def _lehmann(w1, U1, vecs, e0, sign):
    """G[w, j, i] = sum_n <p_j|n><n|p_i> / (i w - sign (E_n - E0))"""
    A = U1.conj().T @ np.stack(vecs, axis=1)                   # <n|p_i>
    den = 1.0 / (1j * WM[:, None] - sign * (w1[None, :] - e0))  # [w, n]
    return np.einsum("wn,nj,ni->wji", den, A.conj(), A)


@pytest.fixture(scope="module")
def square_gs(built):
    """the Ns = 8 square cluster and its ground state of (4,4), found once on the device"""
    import hxv
    from hxv import models

    m = models.hm_2dsquare(Nbath=1)
    gs = hxv.HxvSector.from_model(m, 4, 4)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)          # stays on the device
    yield dict(m=m, gs=gs, e0=e0, psi=psi, psi_h=gs.vector_to_host(psi), maps=gs.maps())
    gs.close()


@pytest.mark.parametrize("spin,create", [(0, True), (0, False), (1, True), (1, False)])
def test_green_function_of_the_square_cluster_from_two_paired_runs(square_gs, spin, create):
    """Orbitals paired (0,1) and (2,3), all four c^dagger_j|gs> (c_j|gs>) as probes of both runs: 2 paired runs give the 4 x 4 block that 4 single
    probe runs give.  The Lehmann sum is taken with the device's own ground-state vector, so nothing depends on how far it has converged."""
    import hxv
    from hxv import greens
    from oracle.oracle import OracleSector

    m, gs, e0, psi = square_gs["m"], square_gs["gs"], square_gs["e0"], square_gs["psi"]
    nimp = m.Nlat * m.Norb
    assert nimp == 4
    d = 1 if create else -1
    nu, nd = (4 + d, 4) if spin == 0 else (4, 4 + d)
    sec = hxv.HxvSector.from_model(m, nu, nd)
    H = OracleSector(m, nu, nd).dense()
    assert not H.imag.any()
    w1, U1 = np.linalg.eigh(H.real)
    sign = 1.0 if create else -1.0
    nl = min(sec.Dim, 200)                                      # lanc_nGFiter, ED_GF_NORMAL.f90:204-207
    pcie_gs = (gs.stats()["h2d_bytes"], gs.stats()["d2h_bytes"])
    dev, n2s = zip(*[gs.apply_ladder(sec, i, spin, create, psi) for i in range(nimp)])
    pcie = (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"])
    G = np.zeros((LMATS, nimp, nimp), dtype=np.complex128)
    for i, i2 in ((0, 1), (2, 3)):
        runs = sec.lanczos_tridiag_pair_probes(dev[i], dev[i2], list(dev), nl)
        assert sec.get_option("lanczos_real_last") == 2
        for col, (a, b, ov, n) in zip((i, i2), runs):
            poles, wts = greens.poles_weights(a[:n], b[:n], ov, np.sqrt(n2s[col]))       # (hxv_gf_from_probes takes the array as it is)
            G[:, :, col] = greens.evaluate(poles, wts, 1j * WM, e0, sign)
    assert (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"]) == pcie                  # no Dim-sized PCIe traffic
    assert (gs.stats()["h2d_bytes"], gs.stats()["d2h_bytes"]) == pcie_gs
    ref_vecs = [_apply_op(square_gs["psi_h"], square_gs["maps"], sec.maps(), i, spin, create) for i in range(nimp)]
    Gref = _lehmann(w1, U1, ref_vecs, e0, sign)
    err = np.abs(G - Gref).max()
    print(f"square Ns=8 spin {spin} create {create}: max |G - Lehmann| = {err:.3e}, max |G| = {np.abs(Gref).max():.3e}, "
          f"max off-diagonal |G| = {max(np.abs(Gref[:, i, j]).max() for i in range(nimp) for j in range(nimp) if i != j):.3e}")
    assert err <= 1e-9, err
    sec.close()


# ---- 3. susceptibility ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_dense(built):
    """the Ns = 6 chain of test_gpu_density_ops.py's chi tests and the dense spectrum of its sector (3,3), computed once"""
    from hxv import models
    from oracle.oracle import OracleSector

    m, (nup, ndw) = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), (3, 3)
    orc = OracleSector(m, nup, ndw)
    w, U = np.linalg.eigh(orc.dense())
    return dict(m=m, sector=(nup, ndw), w=w, U=U, maps=(orc.map_up(), orc.map_dw()))


@pytest.mark.parametrize("kind", ["spin", "three_ops"])
def test_paired_susceptibility_matches_the_unpaired_one_and_the_lehmann_sum(chain_dense, kind):
    import hxv
    from hxv import observables

    m, (nup, ndw), w, U = chain_dense["m"], chain_dense["sector"], chain_dense["w"], chain_dense["U"]
    assert w[1] - w[0] > 1e-3                                    # non-degenerate ground state: no Curie term
    nimp = m.Nlat * m.Norb
    if kind == "spin":
        coef, arg = chi_ref.spin_charge_coef("spin", nimp), "spin"                         # nops = 2: one pair
    else:
        # S^z_0, n_1 and a mixed operator: three columns, the last one without a partner
        coef = np.array([[[0.5, 0.0], [-0.5, 0.0]], [[0.0, 1.0], [0.0, 1.0]], [[0.3, -0.7], [0.2, 0.4]]])
        arg = coef
    psi = U[:, 0]
    psi = np.real(psi * np.exp(-1j * np.angle(psi[np.abs(psi).argmax()]))).astype(np.complex128)
    psi /= np.linalg.norm(psi)
    vecs, _, _ = chi_ref.fluctuations(chi_ref.density_f(*chain_dense["maps"], coef), psi)
    ref = chi_ref.lehmann_chi(w, U, 0, list(vecs), 1j * chi_ref.NU)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(psi)
    pcie = (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"])
    chi1, info1 = observables.susceptibility(sec, dpsi, w[0], arg, 1j * chi_ref.NU)
    assert sec.get_option("lanczos_real_last") == 1
    chi2, info2 = observables.susceptibility(sec, dpsi, w[0], arg, 1j * chi_ref.NU, paired=True)
    assert sec.get_option("lanczos_real_last") == (2 if kind == "spin" else 1)            # (three columns: the last run is a single one)
    assert (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"]) == pcie
    scale = max(1.0, np.abs(ref).max())
    e_ref, e_pair = np.abs(chi2 - ref).max(), np.abs(chi2 - chi1).max()
    print(f"chain {kind}: max|chi| = {np.abs(ref).max():.3e}, |paired - Lehmann| = {e_ref:.3e}, |paired - unpaired| = {e_pair:.3e}, "
          f"steps {info2['nsteps'].tolist()} / {info1['nsteps'].tolist()}")
    assert chi2.shape == (chi_ref.NFREQ, coef.shape[0], coef.shape[0])
    assert e_ref <= 1e-9 * scale, (e_ref, scale)
    assert e_pair <= 1e-9 * scale, (e_pair, scale)
    assert info2["dropped_weight"] <= 1e-20
    assert np.array_equal(info2["norm2"], info1["norm2"]) and (info2["nsteps"] > 0).all()
    sec.close()


def test_paired_susceptibility_is_refused_for_complex_h_and_the_default_is_unpaired(built):
    import hxv
    from hxv import models, observables

    sec = hxv.HxvSector.from_model(models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), 4, 3)
    assert not sec.real_vectors_available
    e0, psi, _ = sec.lanczos_eigh(64, 1e-10, native=True)
    with pytest.raises(hxv.HxvError, match="paired"):
        observables.susceptibility(sec, psi, e0, "spin", 1j * chi_ref.NU[:2], nlanc=8, paired=True)
    sec.close()


# ---- 4. split sectors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


NL_SPLIT = 30


@pytest.fixture(scope="module")
def unsplit_pair(built):
    """The unsplit paired call the split ones are compared with, made once.  The Ns = 12 chain (C2), sector (6,3): DimDw = 220 columns (74 + 73
    + 73 on 3 ranks), Dim = 203 280.  Two recurrences that differ by one rounding (here: the order of the sums over the ranks) separate
    geometrically once Ritz values converge (the head of test_gpu_probes.py), so the sector has to be one where 30 steps stay clear of that: a
    numpy recurrence on the oracle's product, run twice from unit start vectors that differ by 1e-16 relative noise, keeps the overlaps with
    unit probes within 5e-17 over 30 steps on this sector (and within 1e-17 on (6,6)), but lets them drift to 5e-12 on the Ns = 8 square
    cluster's (4,4) (Dim 4900; 4e-17 after 12 steps, 5e-15 after 20)."""
    import hxv
    from hxv import models

    m, (nup, ndw) = models.hm_1dchain(), (6, 3)
    ser = hxv.HxvSector.from_model(m, nup, ndw)
    rng = np.random.default_rng(5)
    va, vb = _unit(_rand(rng, ser.Dim)), _unit(_rand(rng, ser.Dim))
    ps = [_unit(_rand(rng, ser.Dim)) for _ in range(3)]
    ra, rb = ser.lanczos_tridiag_pair_probes(ser.vector_from_host(va), ser.vector_from_host(vb), [ser.vector_from_host(p) for p in ps], NL_SPLIT)
    ser.close()
    return dict(m=m, sector=(nup, ndw), va=va, vb=vb, ps=ps, ra=ra, rb=rb)


@pytest.mark.parametrize("nranks,exchange", [(2, "allgather"), (3, "alltoall"), (3, "allgather"), (2, "alltoall")])
def test_split_sector_paired_overlaps_equal_the_unsplit_ones(unsplit_pair, transport, nranks, exchange):
    import torch
    import hxv

    u = unsplit_pair
    m, (nup, ndw), nl = u["m"], u["sector"], NL_SPLIT
    hxv.set_exchange_default(exchange)

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        da, db = sec.vector_from_host(u["va"][lo:hi].copy()), sec.vector_from_host(u["vb"][lo:hi].copy())
        dps = [sec.vector_from_host(p[lo:hi].copy()) for p in u["ps"]]
        c0 = sec.get_option("allreduce_count")
        (aa, ba, na), (ab, bb, nb) = sec.lanczos_tridiag_pair(da, db, nl)
        c1 = sec.get_option("allreduce_count")
        ra, rb = sec.lanczos_tridiag_pair_probes(da, db, dps, nl)
        c2 = sec.get_option("allreduce_count")
        r_none = sec.lanczos_tridiag_pair_probes(da, db, [], nl)
        c3 = sec.get_option("allreduce_count")
        refused = None
        if exchange == "allgather":
            # a start vector at hxv_slab_home is staged; a PROBE there is refused, by every rank together (nobody is left in a collective)
            home = sec.slab_home()
            home.copy_(da)
            rh, _ = sec.lanczos_tridiag_pair_probes(home, db, dps, nl)
            assert rh[3] == ra[3] and np.array_equal(rh[0], ra[0]) and np.array_equal(rh[2], ra[2])
            home = sec.slab_home()
            with pytest.raises(hxv.HxvError) as ei:
                sec.lanczos_tridiag_pair_probes(da, db, [dps[0], home if r == 0 else dps[1]], nl)      # only rank 0's own argument is bad
            refused = str(ei.value)
        torch.cuda.synchronize()
        cols = sec.mpiQdw
        sec.close()
        return dict(ra=ra, rb=rb, pair=((aa, ba, na), (ab, bb, nb)), extra=(c2 - c1) - (c1 - c0), none=(c3 - c2) - (c1 - c0), r_none=r_none,
                    cols=cols, refused=refused)

    try:
        res = hxv.run_ranks(nranks, rank, transport=transport)
    finally:
        hxv.set_exchange_default("allgather")
    if nranks == 3:
        assert len({o["cols"] for o in res}) > 1                                            # uneven column counts
    worst = max(np.abs(o[k][2] - u[k][2]).max() for o in res for k in ("ra", "rb"))
    print(f"{nranks} ranks {exchange}: max |overlaps - unsplit| = {worst:.3e}, max |alanc - unsplit| = {np.abs(res[0]['ra'][0] - u['ra'][0]).max():.3e}")
    for o in res:
        for k, (ap, bp, n_p) in zip(("ra", "rb"), o["pair"]):
            a, b, ov, n = o[k]
            assert n == n_p == nl and ov.shape == (nl, 3)
            assert np.array_equal(a, ap) and np.array_equal(b, bp)                          # bit-identical to hxv_lanczos_tridiag_pair on the same split
            assert np.array_equal(ov, res[0][k][2])                                         # identical on every rank
            assert not ov.imag.any()
            assert np.abs(ov - u[k][2]).max() <= 1e-12, np.abs(ov - u[k][2]).max()
        assert np.array_equal(o["r_none"][0][0], o["pair"][0][0]) and np.array_equal(o["r_none"][1][1], o["pair"][1][1])
        assert o["extra"] == nl, o["extra"]                                                 # exactly ONE more all-reduce per step ...
        assert o["none"] == 0                                                               # ... and none without probes
        if exchange == "allgather":
            assert "gather buffer" in o["refused"] or "peer rank" in o["refused"]


# ---- 5. determinism and buffers ---------------------------------------------------------------------------------------------------------
def test_determinism_buffers_and_traffic(built):
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=2, Nbath=3)
    live0 = hxv.live_handles()
    sec = hxv.HxvSector.from_model(m, 4, 4)
    rng = np.random.default_rng(2)
    da, db = sec.vector_from_host(_rand(rng, sec.Dim)), sec.vector_from_host(_rand(rng, sec.Dim))
    dps = [sec.vector_from_host(_rand(rng, sec.Dim)) for _ in range(5)]
    first = sec.lanczos_tridiag_pair_probes(da, db, dps, 30)       # (lazy allocations of the handle happen here)
    st0, pool0 = sec.stats(), hxv.pool_stats()
    again = sec.lanczos_tridiag_pair_probes(da, db, dps, 30)
    st1, pool1 = sec.stats(), hxv.pool_stats()
    for f, g in zip(first, again):
        for x, y in zip(f[:3], g[:3]):
            assert np.array_equal(x, y)                            # the same bits on every call
        assert f[3] == g[3] == 30
    assert (st1["h2d_bytes"], st1["d2h_bytes"]) == (st0["h2d_bytes"], st0["d2h_bytes"])     # no Dim-sized PCIe traffic
    # the five real probe buffers and the scratch came from the cache and went back to it
    assert pool1["hits"] >= pool0["hits"] + 6 and pool1["misses"] == pool0["misses"] and pool1["cached_bytes"] == pool0["cached_bytes"]
    assert st1["device_bytes"] == st0["device_bytes"]
    sec.close()
    assert hxv.live_handles() == live0


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def test_imaginary_probe_is_refused(built):
    import hxv
    from hxv import models

    sec = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), 3, 3)
    rng = np.random.default_rng(4)
    da, db, p0, p1 = (sec.vector_from_host(_rand(rng, sec.Dim)) for _ in range(4))
    bad = p1.clone()
    bad[1] += 1e-3j                                                # ONE element with an imaginary part
    with pytest.raises(hxv.HxvError, match="must be real"):
        sec.lanczos_tridiag_pair_probes(da, db, [p0, bad], 6)
    assert "HXV_ERR_ARG" in _error_name(hxv, sec, da, db, [p0, bad])
    with pytest.raises(hxv.HxvError, match="must be real"):
        sec.lanczos_tridiag_pair_probes(da, bad, [p0, p1], 6)      # ... or a start vector
    ra, rb = sec.lanczos_tridiag_pair_probes(da, db, [p0, p1], 6)  # the handle is as good as before
    assert ra[3] == rb[3] == 6
    sec.close()


def _error_name(hxv, sec, da, db, probes):
    pd = C.POINTER(C.c_double)
    z = [np.zeros(6) for _ in range(4)] + [np.zeros(2 * 6 * len(probes)) for _ in range(2)]
    na, nb = C.c_int32(), C.c_int32()
    plist = (C.c_void_p * len(probes))(*[p.data_ptr() for p in probes])
    p = lambda x: x.ctypes.data_as(pd)  # noqa: E731
    rc = hxv.load_library().hxv_lanczos_tridiag_pair_probes(sec._h, da.data_ptr(), db.data_ptr(), len(probes), plist, 6, p(z[0]), p(z[1]), p(z[4]),
                                                            p(z[2]), p(z[3]), p(z[5]), 1e-12, C.byref(na), C.byref(nb))
    return {1: "HXV_ERR_ARG"}.get(rc, str(rc))


def test_imaginary_probe_on_one_rank_is_refused_on_every_rank(built):
    """2 thread ranks, the bad probe on rank 1 only: the sum of Im^2 is all-reduced, so both ranks return HXV_ERR_ARG from the same place and
    nobody is left in a collective -- the good call that follows runs on both."""
    import torch
    import hxv
    from hxv import models

    m, (nup, ndw) = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (3, 3)
    rng = np.random.default_rng(6)
    va, vb, p0 = (_rand(rng, 400) for _ in range(3))

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=2)
        group.join(sec)
        assert sec.Dim == 400
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        da, db, dp = (sec.vector_from_host(x[lo:hi].copy()) for x in (va, vb, p0))
        bad = dp.clone()
        if r == 1:
            bad[0] += 0.5j
        L = hxv.load_library()
        pd = C.POINTER(C.c_double)
        z = [np.zeros(6) for _ in range(4)] + [np.zeros(12) for _ in range(2)]
        na, nb = C.c_int32(), C.c_int32()
        plist = (C.c_void_p * 1)(bad.data_ptr())
        p = lambda x: x.ctypes.data_as(pd)  # noqa: E731
        torch.cuda.synchronize()
        rc = L.hxv_lanczos_tridiag_pair_probes(sec._h, da.data_ptr(), db.data_ptr(), 1, plist, 6, p(z[0]), p(z[1]), p(z[4]), p(z[2]), p(z[3]), p(z[5]),
                                               1e-12, C.byref(na), C.byref(nb))
        good = sec.lanczos_tridiag_pair_probes(da, db, [dp], 6)
        torch.cuda.synchronize()
        sec.close()
        return rc, good

    res = hxv.run_ranks(2, rank, transport="local")
    assert [rc for rc, _ in res] == [1, 1]                         # HXV_ERR_ARG on both
    assert res[0][1][0][3] == res[1][1][0][3] == 6 and np.array_equal(res[0][1][0][2], res[1][1][0][2])


def test_complex_h_is_unsupported(built):
    import hxv
    from hxv import models

    sec = hxv.HxvSector.from_model(models.bhz_2d(Nbath=0), 4, 4)
    rng = np.random.default_rng(9)
    da, db, dp = (sec.vector_from_host(_rand(rng, sec.Dim)) for _ in range(3))
    L = hxv.load_library()
    pd = C.POINTER(C.c_double)
    z = [np.zeros(4) for _ in range(4)] + [np.zeros(8) for _ in range(2)]
    p = lambda x: x.ctypes.data_as(pd)  # noqa: E731
    na, nb = C.c_int32(), C.c_int32()
    plist = (C.c_void_p * 1)(dp.data_ptr())
    rc = L.hxv_lanczos_tridiag_pair_probes(sec._h, da.data_ptr(), db.data_ptr(), 1, plist, 4, p(z[0]), p(z[1]), p(z[4]), p(z[2]), p(z[3]), p(z[5]), 1e-12,
                                           C.byref(na), C.byref(nb))
    assert rc == 4, (rc, L.hxv_last_error())                       # HXV_ERR_UNSUPPORTED
    assert b"hxv_lanczos_tridiag_pair_probes" in L.hxv_last_error()
    with pytest.raises(hxv.HxvError):
        sec.lanczos_tridiag_pair_probes(da, db, [dp], 4)
    sec.close()


def test_argument_errors(built):
    import torch
    import hxv
    from hxv import models

    L = hxv.load_library()
    sec = hxv.HxvSector.from_model(models.plaquette_2x2_nobath(), 2, 2)
    rng = np.random.default_rng(1)
    dv, dw = sec.vector_from_host(_rand(rng, sec.Dim)), sec.vector_from_host(_rand(rng, sec.Dim))
    arr = [np.zeros(4) for _ in range(4)]
    ova, ovb = np.zeros(2 * 4 * 9), np.zeros(2 * 4 * 9)
    na, nb = C.c_int32(), C.c_int32()
    pd = C.POINTER(C.c_double)
    aa, ba, ab, bb = (x.ctypes.data_as(pd) for x in arr)
    poa, pob = ova.ctypes.data_as(pd), ovb.ctypes.data_as(pd)
    one = (C.c_void_p * 1)(dv.data_ptr())
    nine = (C.c_void_p * 9)(*([dv.data_ptr()] * 9))
    hole = (C.c_void_p * 2)(dv.data_ptr(), None)
    h, v, w = sec._h, dv.data_ptr(), dw.data_ptr()
    tail = (1e-12, C.byref(na), C.byref(nb))
    bad = {
        "NULL handle": (None, v, w, 1, one, 4, aa, ba, poa, ab, bb, pob) + tail,
        "bad argument": (h, None, w, 1, one, 4, aa, ba, poa, ab, bb, pob) + tail,
        "bad argument ": (h, v, None, 1, one, 4, aa, ba, poa, ab, bb, pob) + tail,
        "bad argument  ": (h, v, w, 1, one, 4, aa, None, poa, ab, bb, pob) + tail,
        "nlanc < 1": (h, v, w, 1, one, 0, aa, ba, poa, ab, bb, pob) + tail,
        "nprobes must be": (h, v, w, 9, nine, 4, aa, ba, poa, ab, bb, pob) + tail,
        "nprobes must be ": (h, v, w, -1, one, 4, aa, ba, poa, ab, bb, pob) + tail,
        "needs the probe list": (h, v, w, 1, None, 4, aa, ba, poa, ab, bb, pob) + tail,
        "needs the probe list ": (h, v, w, 1, one, 4, aa, ba, None, ab, bb, pob) + tail,
        "needs the probe list  ": (h, v, w, 1, one, 4, aa, ba, poa, ab, bb, None) + tail,
        "NULL entry": (h, v, w, 2, hole, 4, aa, ba, poa, ab, bb, pob) + tail,
    }
    for text, args in bad.items():
        assert L.hxv_lanczos_tridiag_pair_probes(*args) == 1, text     # HXV_ERR_ARG
        msg = L.hxv_last_error().decode()
        assert "hxv_lanczos_tridiag_pair_probes" in msg and text.strip() in msg, (text, msg)
    # no probe: allowed, list and overlaps may be NULL
    assert L.hxv_lanczos_tridiag_pair_probes(h, v, w, 0, None, 4, aa, ba, None, ab, bb, None, *tail) == 0 and na.value == 4 and nb.value == 4
    # the Python form takes native device vectors only: no dispatch on the length
    with pytest.raises(hxv.HxvError, match="padded layout"):
        sec.lanczos_tridiag_pair_probes(dv[:-1].contiguous(), dw, [], 4)
    with pytest.raises(hxv.HxvError, match="padded layout"):
        sec.lanczos_tridiag_pair_probes(dv, dw, [torch.zeros(sec.Dim + 3, dtype=torch.complex128, device="cuda")], 4)
    with pytest.raises(hxv.HxvError, match="zero or not finite"):
        sec.lanczos_tridiag_pair_probes(torch.zeros_like(dv), dw, [], 4)
    sec.close()
