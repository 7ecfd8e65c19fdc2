"""Density-type operators and the susceptibility stage on the MI355X (include/hxv.h: hxv_apply_density_ops; HxvSector.apply_density_ops,
hxv.greens.chi_evaluate, hxv.observables.susceptibility).

  - the vectors out_a = (f_a - m_a) psi against numpy on vector_to_host   |d| <= 1e-14 * max_a sum|coef_a| * max|psi|: one rounding of f - m
    plus the summation error of m, with a margin of about 50; mean within 1e-13 * sum|coef_a|, norm2 within 1e-13 * (sum|coef_a|)^2
  - pad rows: never read (NaN planted in psi's), written as exact zeros (over a sentinel)
  - the device row order and the reference's order give the same columns
  - closed forms: total charge on the bath-free plaquette, <S^z_i^2> of hxv_observables_derive
  - chi_spin, chi_charge against the dense Lehmann sum at nu_0 .. nu_63, beta = 50      1e-9 * max(1, max|chi_ref|): the project's tolerance
    for G, scaled because |chi| reaches 9 on the BHZ sector; psi is the DENSE ground state, uploaded, so that the new code is measured and
    not the convergence of an eigenvector
  - split sectors on both transports, determinism, buffers, argument errors.
"""
import ctypes as C

import numpy as np
import pytest

import chi_ref

pytestmark = pytest.mark.gpu


def _rand_unit(rng, n, real):
    v = (rng.standard_normal(n) + (0.0 if real else 1j * rng.standard_normal(n))).astype(np.complex128)
    return v / np.linalg.norm(v)


def _model(shape):
    from hxv import models

    return {"plaquette": (models.plaquette_2x2_nobath(), (2, 2)),                                # 36 elements: less than one block
            "pad_rows": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (4, 3)),       # DimUp = 15: a pad row in every column
            "blocks": (models.hm_1dchain(Nlat=2, Nbath=3), (4, 4)),                              # DimUp = 70, 5040 padded elements: 20 blocks
            "ns14": (models.hm_1dchain(Nlat=2, Nbath=6), (7, 7)),                                # DimUp = 3432: two row chunks per column
            "bhz": (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3))}[shape]                     # Nimp = 8: both 5-bit halves of the lookup


COMBOS = [(nops, sub) for nops in (1, 3, 8) for sub in (False, True)]


def _coefs(nimp):
    rng = np.random.default_rng(17)
    return {nops: rng.standard_normal((nops, 2, nimp)) for nops in (1, 3, 8)}


def _check_vectors(sec, psi_h, dpsi, coefs, tag, keep=None):
    """every (nops, subtract_mean) combination against numpy; -> the worst ratios to the three bounds"""
    mu, md = sec.maps()
    psimax = np.abs(psi_h).max()
    psi2 = psi_h.reshape(sec.DimDw, sec.DimUp)
    w2 = np.abs(psi2) ** 2
    wu, wd, wn = w2.sum(axis=0), w2.sum(axis=1), w2.sum()
    worst = np.zeros(3)
    for nops, sub in COMBOS:
        cf = coefs[nops]
        s1 = np.abs(cf).sum(axis=(1, 2))
        vecs, mean, n2 = sec.apply_density_ops(cf, dpsi, subtract_mean=sub)
        assert len(vecs) == nops and mean.shape == n2.shape == (nops,)
        nimp = cf.shape[2]
        bu = np.stack([(mu >> b) & 1 for b in range(nimp)]).astype(np.float64)
        bd = np.stack([(md >> b) & 1 for b in range(nimp)]).astype(np.float64)
        fu, fd = cf[:, 0, :] @ bu, cf[:, 1, :] @ bd
        for a in range(nops):
            m_ref = (fu[a] @ wu + fd[a] @ wd) / wn
            g = fu[a][None, :] + fd[a][:, None] - (m_ref if sub else 0.0)
            ref = g * psi2
            got = sec.vector_to_host(vecs[a]).reshape(sec.DimDw, sec.DimUp)
            dv, dm, dn = np.abs(got - ref).max(), abs(mean[a] - m_ref), abs(n2[a] - (np.abs(ref) ** 2).sum())
            worst = np.maximum(worst, [dv / (1e-14 * s1.max() * psimax), dm / (1e-13 * s1[a]), dn / (1e-13 * s1[a] ** 2)])
            if keep is not None and (nops, sub, a) == (1, True, 0):
                keep.append(got.copy())
    print(f"{tag}: worst error / bound: vectors {worst[0]:.3f}, mean {worst[1]:.3f}, norm2 {worst[2]:.3f}")
    return worst


# ---- 1. the vectors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("shape", ["plaquette", "pad_rows", "blocks", "bhz"])
def test_vectors_means_and_norms_match_numpy(built, shape, real):
    import hxv

    m, (nup, ndw) = _model(shape)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    psi_h = _rand_unit(np.random.default_rng(7), sec.Dim, real)
    dpsi = sec.vector_from_host(psi_h)
    raw = dpsi.view(sec.mpiQdw, sec.pitch)
    if sec.pitch > sec.DimUp:
        raw[:, sec.DimUp:] = complex(np.nan, np.nan)             # a pad row of psi is never read
    worst = _check_vectors(sec, psi_h, dpsi, _coefs(m.Nlat * m.Norb), f"{shape} real={real}")
    assert worst.max() <= 1.0, worst
    if real:
        vecs, _, _ = sec.apply_density_ops(_coefs(m.Nlat * m.Norb)[3], dpsi)
        assert all(not v.imag.any().item() for v in vecs)        # a real state stays real: the real-vector Lanczos path stays open
    sec.close()


def test_pad_rows_of_every_output_are_written_as_zero(built):
    import torch
    import hxv

    m, (nup, ndw) = _model("pad_rows")
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    assert sec.DimUp == 15 and sec.pitch == 16
    dpsi = sec.vector_from_host(_rand_unit(np.random.default_rng(7), sec.Dim, False))
    for nops, sub in COMBOS:
        outs = [torch.full((sec.localElems,), 7.0 + 7.0j, dtype=torch.complex128, device="cuda") for _ in range(nops)]
        vecs, _, _ = sec.apply_density_ops(_coefs(m.Nlat * m.Norb)[nops], dpsi, subtract_mean=sub, out=outs)
        for v, o in zip(vecs, outs):
            assert v is o
            raw = torch.view_as_real(v.view(sec.mpiQdw, sec.pitch))
            assert (raw[:, sec.DimUp:] == 0).all().item() and not (raw[:, :sec.DimUp] == 7.0).any().item()
    sec.close()


_NS14 = {}


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("order", ["1", "0"])
def test_device_row_order_and_host_order_match_numpy_and_each_other(built, monkeypatch, order, real):
    import hxv

    monkeypatch.setenv("HXV_ROW_ORDER", order)
    hxv.sector_cache_clear()
    m, (nup, ndw) = _model("ns14")
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    assert sec.DimUp == 3432
    assert (sec.row_perm is not None) == (order == "1")
    c = _NS14.setdefault(real, {})
    if "psi" not in c:
        c["psi"] = _rand_unit(np.random.default_rng(7), sec.Dim, real)
    keep = []
    worst = _check_vectors(sec, c["psi"], sec.vector_from_host(c["psi"]), _coefs(2), f"ns14 row order {order} real={real}", keep)
    sec.close()
    hxv.sector_cache_clear()
    assert worst.max() <= 1.0, worst
    if "first" in c:                                             # the other order ran before: the same columns within the vector bound
        d = np.abs(keep[0] - c.pop("first")).max()
        bound = 1e-14 * np.abs(_coefs(2)[1]).sum() * np.abs(c["psi"]).max()
        print(f"ns14 real={real}: device order against host order {d:.3e} (bound {bound:.3e})")
        assert d <= bound, (d, bound)
        c.pop("psi")
    else:
        c["first"] = keep[0]


# ---- 2. closed forms --------------------------------------------------------------------------------------------------------------------
def test_total_charge_of_the_bath_free_plaquette_has_no_fluctuation(built):
    import hxv

    m, (nup, ndw) = _model("plaquette")
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(_rand_unit(np.random.default_rng(3), sec.Dim, False))
    _, mean, n2 = sec.apply_density_ops(np.ones((1, 2, 4)), dpsi)
    assert abs(mean[0] - (nup + ndw)) <= 1e-13 and n2[0] <= 1e-28, (mean, n2)
    sec.close()


def test_spin_fluctuation_equals_the_observables_sz2(built):
    import hxv
    from hxv import observables

    m, (nup, ndw) = _model("blocks")
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(_rand_unit(np.random.default_rng(4), sec.Dim, False))
    sz2 = observables.derive(m, sec.observables_record(dpsi))["sz2"]
    _, mean, n2 = sec.apply_density_ops(observables.density_coefficients("spin", 2), dpsi)
    for i in range(2):
        assert abs(n2[i] + mean[i] ** 2 - sz2[i, i, 0, 0]) <= 1e-12, (i, n2[i], mean[i], sz2[i, i, 0, 0])
    sec.close()


# ---- 3. chi against the Lehmann sum -----------------------------------------------------------------------------------------------------
def _chi_model(name):
    from hxv import models

    return {"chain": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), (3, 3), True),
            "plaquette": (models.plaquette_2x2_nobath(U=4.0, t=1.0, hfmode=True), (2, 2), True),
            "bhz": (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3), False)}[name]


@pytest.fixture(scope="module", params=["chain", "plaquette", "bhz"])
def dense(request, built):
    """the dense spectrum of the sector, computed once for both kinds"""
    from oracle.oracle import OracleSector

    m, (nup, ndw), real = _chi_model(request.param)
    orc = OracleSector(m, nup, ndw)
    w, U = np.linalg.eigh(orc.dense())
    return dict(name=request.param, m=m, sector=(nup, ndw), real=real, w=w, U=U, maps=(orc.map_up(), orc.map_dw()))


@pytest.mark.parametrize("kind", ["spin", "charge"])
def test_susceptibility_matches_the_lehmann_sum(dense, kind):
    import hxv
    from hxv import observables

    m, (nup, ndw), w, U = dense["m"], dense["sector"], dense["w"], dense["U"]
    assert w[1] - w[0] > 1e-3                                    # non-degenerate ground state: no Curie term
    nimp = m.Nlat * m.Norb
    psi = U[:, 0]
    if dense["real"]:
        psi = np.real(psi * np.exp(-1j * np.angle(psi[np.abs(psi).argmax()]))).astype(np.complex128)
        psi /= np.linalg.norm(psi)
    f = chi_ref.density_f(*dense["maps"], chi_ref.spin_charge_coef(kind, nimp))
    vecs, mean_ref, n2_ref = chi_ref.fluctuations(f, psi)
    ref = chi_ref.lehmann_chi(w, U, 0, list(vecs), 1j * chi_ref.NU)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(psi)
    pcie = (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"])
    chi, info = observables.susceptibility(sec, dpsi, w[0], kind, 1j * chi_ref.NU)
    assert (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"]) == pcie           # nothing Dim-sized crossed PCIe
    err, scale = np.abs(chi - ref).max(), max(1.0, np.abs(ref).max())
    asym = np.abs(ref - ref.transpose(0, 2, 1)).max()
    print(f"{dense['name']} {kind}: max|chi| = {np.abs(ref).max():.3e}, |chi - Lehmann| = {err:.3e}, dropped weight {info['dropped_weight']:.3e}, "
          f"steps {info['nsteps'].tolist()}, max|chi_ab - chi_ba| = {asym:.3e}")
    assert chi.shape == (chi_ref.NFREQ, nimp, nimp)
    assert np.abs(info["mean"] - mean_ref).max() <= 1e-13 and np.abs(info["norm2"] - n2_ref).max() <= 1e-13
    assert err <= 1e-9 * scale, (err, scale)
    assert info["dropped_weight"] <= 1e-20
    if dense["real"]:
        assert sec.get_option("lanczos_real_last") == 1
    else:
        assert asym > 1e-6                                       # chi_ab != chi_ba on this sector: a wrong conjugation would show
    sec.close()


def test_whole_stage_from_the_device_ground_state_without_pcie_traffic(built):
    import hxv
    from hxv import observables
    from oracle.oracle import OracleSector

    m, (nup, ndw), _ = _chi_model("chain")
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    e0, psi, _ = sec.lanczos_eigh(512, 1e-14, native=True)
    st0 = sec.stats()
    chi, info = observables.susceptibility(sec, psi, e0, "spin", 1j * chi_ref.NU)
    chi_c, info_c = observables.susceptibility(sec, psi, e0, "charge", 1j * chi_ref.NU)
    st1 = sec.stats()
    assert (st1["h2d_bytes"], st1["d2h_bytes"]) == (st0["h2d_bytes"], st0["d2h_bytes"])
    orc = OracleSector(m, nup, ndw)
    w, U = np.linalg.eigh(orc.dense())
    assert abs(w[0] - e0) < 1e-10 and w[1] - w[0] > 1e-3
    for kind, got in (("spin", chi), ("charge", chi_c)):
        f = chi_ref.density_f(orc.map_up(), orc.map_dw(), chi_ref.spin_charge_coef(kind, 2))
        ref = chi_ref.lehmann_chi(w, U, 0, list(chi_ref.fluctuations(f, U[:, 0])[0]), 1j * chi_ref.NU)
        # the eigenvector is converged to 1e-7 in the residual: chi is second order in that error, far below the stage's 1e-9
        print(f"chain end to end {kind}: |chi - Lehmann| = {np.abs(got - ref).max():.3e}")
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert info["dropped_weight"] <= 1e-20 and info_c["dropped_weight"] <= 1e-20
    sec.close()


# ---- 4. split sectors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.mark.parametrize("name,nranks", [("chain", 2), ("chain", 3), ("bhz", 3)])
def test_split_sector_slabs_equal_the_unsplit_columns(built, transport, name, nranks):
    import torch
    import hxv

    m, (nup, ndw) = _model("pad_rows" if name == "chain" else "bhz")       # chain (4,3): DimDw = 20, uneven on 3 ranks
    real = name == "chain"
    ser = hxv.HxvSector.from_model(m, nup, ndw)
    psi = _rand_unit(np.random.default_rng(5), ser.Dim, real)
    cf = np.random.default_rng(6).standard_normal((3, 2, m.Nlat * m.Norb))
    vecs0, mean0, n20 = ser.apply_density_ops(cf, ser.vector_from_host(psi))
    host0 = [ser.vector_to_host(v) for v in vecs0]
    ser.close()
    s1 = np.abs(cf).sum(axis=(1, 2))
    bound = 1e-14 * s1.max() * np.abs(psi).max()

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        dpsi = sec.vector_from_host(psi[lo:hi].copy())
        c0 = sec.get_option("allreduce_count")
        vecs, mean, n2 = sec.apply_density_ops(cf, dpsi)
        c1 = sec.get_option("allreduce_count")
        d = max(np.abs(sec.vector_to_host(v) - h[lo:hi]).max() for v, h in zip(vecs, host0))
        # only rank 0's own argument is bad: every rank returns an error, nobody is left waiting
        outs = [torch.empty_like(dpsi) for _ in range(3)]
        refused = None
        with pytest.raises(hxv.HxvError) as ei:
            sec.apply_density_ops(cf, dpsi, out=[outs[0], None if r == 0 else outs[1], outs[2]])
        refused = str(ei.value)
        again = sec.apply_density_ops(cf, dpsi)                   # ... and the communicator is still usable
        torch.cuda.synchronize()
        sec.close()
        return dict(mean=mean, n2=n2, d=d, count=c1 - c0, refused=refused, again=(again[1], again[2]))

    res = hxv.run_ranks(nranks, rank, transport=transport)
    print(f"{name} {nranks} ranks: max |slab - unsplit| = {max(o['d'] for o in res):.3e} (bound {bound:.3e}), "
          f"max |mean - unsplit| = {max(np.abs(o['mean'] - mean0).max() for o in res):.3e}")
    for r, o in enumerate(res):
        assert np.array_equal(o["mean"], res[0]["mean"]) and np.array_equal(o["n2"], res[0]["n2"])      # identical on every rank
        assert np.abs(o["mean"] - mean0).max() <= 1e-13 and np.abs(o["n2"] - n20).max() <= 1e-13
        assert o["d"] <= bound, (o["d"], bound)
        assert o["count"] == 2, o["count"]                        # ONE all-reduce per pass
        assert ("NULL entry" in o["refused"]) if r == 0 else ("peer rank" in o["refused"] or "NULL entry" in o["refused"]), o["refused"]
        assert np.array_equal(o["again"][0], o["mean"]) and np.array_equal(o["again"][1], o["n2"])


def test_split_sector_without_its_communicator_is_refused(built):
    import torch
    import hxv

    m, (nup, ndw) = _model("pad_rows")
    sec = hxv.HxvSector.from_model(m, nup, ndw, rank=0, nranks=2)
    dpsi = torch.zeros(sec.localElems, dtype=torch.complex128, device="cuda")
    with pytest.raises(hxv.HxvError, match="status 3.*communicator"):
        sec.apply_density_ops(np.ones((1, 2, 2)), dpsi)
    sec.close()


# ---- 5. determinism, buffers, errors ----------------------------------------------------------------------------------------------------
def test_determinism_and_buffers(built):
    import torch
    import hxv

    m, (nup, ndw) = _model("blocks")
    live0 = hxv.live_handles()
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(_rand_unit(np.random.default_rng(2), sec.Dim, False))
    cf = _coefs(2)[8]
    first = sec.apply_density_ops(cf, dpsi)                       # (the occupation words are built here)
    st0, pool0 = sec.stats(), hxv.pool_stats()
    again = sec.apply_density_ops(cf, dpsi)
    st1, pool1 = sec.stats(), hxv.pool_stats()
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    assert all(torch.equal(x, y) for x, y in zip(first[0], again[0]))                  # the same bits on every call
    assert (st1["h2d_bytes"], st1["d2h_bytes"]) == (st0["h2d_bytes"], st0["d2h_bytes"])
    assert pool1["cached_bytes"] == pool0["cached_bytes"] and pool1["misses"] == pool0["misses"] and pool1["hits"] == pool0["hits"] + 1
    assert st1["device_bytes"] == st0["device_bytes"]
    sec.close()
    assert hxv.live_handles() == live0


def test_argument_errors_write_nothing(built):
    import torch
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    L = hxv.load_library()
    ARG, STATE, UNSUPPORTED = 1, 3, 4
    m = models.plaquette_2x2_nobath()
    sec = hxv.HxvSector.from_model(m, 2, 2)
    dpsi = sec.vector_from_host(_rand_unit(np.random.default_rng(1), sec.Dim, True))
    outs = [torch.full((sec.localElems,), 7.0 + 7.0j, dtype=torch.complex128, device="cuda") for _ in range(9)]
    pd = C.POINTER(C.c_double)
    cf, mean, n2 = np.ones(9 * 2 * 4), np.full(9, 7.0), np.full(9, 7.0)
    bad_cf, inf_cf = cf.copy(), cf.copy()
    bad_cf[5], inf_cf[2] = np.nan, np.inf
    ptr = lambda x: x.ctypes.data_as(pd)  # noqa: E731
    lst = lambda *ps: (C.c_void_p * len(ps))(*ps)  # noqa: E731
    o = [t.data_ptr() for t in outs]
    h, v = sec._h, dpsi.data_ptr()
    zero, nan = torch.zeros_like(dpsi), torch.full_like(dpsi, complex(np.nan, 0.0))
    bad = {
        "NULL handle": (None, 1, ptr(cf), 1, v, lst(o[0]), ptr(mean), ptr(n2)),
        "NULL argument": (h, 1, None, 1, v, lst(o[0]), ptr(mean), ptr(n2)),
        "NULL argument ": (h, 1, ptr(cf), 1, None, lst(o[0]), ptr(mean), ptr(n2)),
        "NULL argument  ": (h, 1, ptr(cf), 1, v, None, ptr(mean), ptr(n2)),
        "NULL argument   ": (h, 1, ptr(cf), 1, v, lst(o[0]), None, ptr(n2)),
        "NULL argument    ": (h, 1, ptr(cf), 1, v, lst(o[0]), ptr(mean), None),
        "nops must be": (h, 0, ptr(cf), 1, v, lst(o[0]), ptr(mean), ptr(n2)),
        "nops must be ": (h, 9, ptr(cf), 1, v, lst(*o), ptr(mean), ptr(n2)),
        "NULL entry": (h, 2, ptr(cf), 1, v, lst(o[0], None), ptr(mean), ptr(n2)),
        "named twice": (h, 3, ptr(cf), 1, v, lst(o[0], o[1], o[0]), ptr(mean), ptr(n2)),
        "is d_psi": (h, 2, ptr(cf), 1, v, lst(o[0], v), ptr(mean), ptr(n2)),
        "not finite": (h, 2, ptr(bad_cf), 1, v, lst(o[0], o[1]), ptr(mean), ptr(n2)),
        "not finite ": (h, 1, ptr(inf_cf), 0, v, lst(o[0]), ptr(mean), ptr(n2)),
        "zero or not finite": (h, 1, ptr(cf), 1, zero.data_ptr(), lst(o[0]), ptr(mean), ptr(n2)),
        "zero or not finite ": (h, 1, ptr(cf), 0, nan.data_ptr(), lst(o[0]), ptr(mean), ptr(n2)),
    }
    torch.cuda.synchronize()
    for text, args in bad.items():
        assert L.hxv_apply_density_ops(*args) == ARG, text
        msg = L.hxv_last_error().decode()
        assert "hxv_apply_density_ops" in msg and text.strip() in msg, (text, msg)
    # handles without basis maps: from CSR, a dw panel
    orc = OracleSector(m, 2, 2)
    csr = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag())
    panel = hxv.HxvSector.dw_panel(m, 2, 2, 4)
    for other in (csr, panel):
        assert L.hxv_apply_density_ops(other._h, 1, ptr(cf), 1, v, lst(o[0]), ptr(mean), ptr(n2)) == STATE
        assert "basis maps" in L.hxv_last_error().decode()
        other.close()
    # Nimp > 10
    big = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=11, Nbath=0), 1, 1)
    assert L.hxv_apply_density_ops(big._h, 1, ptr(np.ones(2 * 11)), 1, v, lst(o[0]), ptr(mean), ptr(n2)) == UNSUPPORTED
    assert "Nimp > 10" in L.hxv_last_error().decode()
    big.close()
    torch.cuda.synchronize()
    assert (mean == 7.0).all() and (n2 == 7.0).all()             # nothing was written: neither the scalars ...
    assert all(torch.equal(t, torch.full_like(t, 7.0 + 7.0j)) for t in outs)        # ... nor an output
    # the Python form takes native device vectors and a (nops, 2, Nimp) array
    with pytest.raises(hxv.HxvError, match="padded layout"):
        sec.apply_density_ops(np.ones((1, 2, 4)), dpsi[:-1].contiguous())
    with pytest.raises(hxv.HxvError, match="shape"):
        sec.apply_density_ops(np.ones((2, 4)), dpsi)
    with pytest.raises(hxv.HxvError, match="Nimp = 4"):
        sec.apply_density_ops(np.ones((1, 2, 3)), dpsi)          # fewer coefficients than the library would read
    sec.close()
