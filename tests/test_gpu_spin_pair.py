"""Operators that change both spin sectors on the MI355X (include/hxv.h: hxv_apply_spin_pair; HxvSector.apply_spin_pair,
hxv.observables.spin_pair_terms / spin_pair_susceptibility) against the numpy restatement of tests/spin_pair_ref.py.

  - the vectors, all four flag combinations, 1 / 4 / 32 terms with random complex coefficients over all orbitals (bath included; 32 terms
    repeat pairs), |d| <= 4 (nterms + 1) 2^-53 sum|coef| max|psi|: one rounding per product and per add, complex multiplication;
    norm2 within 1e-13 (sum|coef|)^2 <psi|psi>; a single term with coef = 1 bit for bit
  - a single term equals the two ladder calls through the intermediate sector, in either order, bit for bit
  - pad rows: never read (NaN planted in psi's), written as exact zeros (over a sentinel); a real state with real coefficients stays real
  - the device row order on neither, either or both sectors: the same host vectors bit for bit
  - hermiticity on the device, two identical calls
  - chi of S^- equals twice the longitudinal spin susceptibility on singlets; the pair susceptibility (local, s-wave, d-wave; complex BHZ)
    equals the dense Lehmann sum: 64 bosonic frequencies, beta = 50, 1e-9 * max(1, max|chi|), dense ground state uploaded, nlanc >= Dim
  - missing sectors, argument errors, split handles, buffers.
The s-wave / d-wave operators run on hm_2dsquare(Nbath=1) (Ns = 8), sector (1,1): the largest for which the dense spectrum of the
neighbour (2,2) is a matter of a second; three bath levels per site (Ns = 16) have no dense reference."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spin_pair_ref as R

pytestmark = pytest.mark.gpu

FLAGS = list(itertools.product((False, True), repeat=2))
EPS = 2.0 ** -53
SENT = complex(7.0, 7.0)


def _shape(name):
    from hxv import models

    return {"plaquette": lambda: (models.plaquette_2x2_nobath(), (2, 2)),                               # 36 -> 16 elements
            "pad_rows": lambda: (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (4, 3)),      # DimUp 15 -> 20 / 6, DimDw 20 -> 15
            "blocks": lambda: (models.hm_1dchain(Nlat=2, Nbath=3), (4, 4)),
            "bhz": lambda: (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3)),                           # orbitals up to 7
            "ns12": lambda: (models.hm_1dchain(Nlat=2, Nbath=5), (6, 6))}[name]()                       # 792 target rows: four row chunks


def _target(nup, ndw, cu, cd):
    return nup + (1 if cu else -1), ndw + (1 if cd else -1)


def _rand(rng, n, real=False):
    v = (rng.standard_normal(n) + (0.0 if real else 1j * rng.standard_normal(n))).astype(np.complex128)
    return v / np.linalg.norm(v)


def _terms(rng, ns, n, real=False):
    return [(int(rng.integers(ns)), int(rng.integers(ns)), complex(rng.standard_normal(), 0.0 if real else rng.standard_normal())) for _ in range(n)]


def _upload_with_nan_pads(sec, psi_h):
    d = sec.vector_from_host(psi_h)
    if sec.pitch > sec.DimUp:
        d.view(sec.mpiQdw, sec.pitch)[:, sec.DimUp:] = complex(np.nan, np.nan)
    return d


def _maps(sec):
    mu, md = sec.maps()
    return np.asarray(mu), np.asarray(md)


def _bits(t):
    """the 64-bit patterns of a device vector with -0 written as +0: an element no term reaches is +0 here, while the second of two ladder
    calls (sign * 0) and the row-order conversion to the host (basis sign * 0) may leave -0 -- the two ladder orders differ from EACH OTHER
    in that; every other pattern is compared as it is"""
    import torch

    return (torch.view_as_real(t) + 0.0).view(torch.int64)


def _host_bits(v):
    return (v.view(np.float64) + 0.0).view(np.uint64)


# ---- 1. the vectors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu,cd", FLAGS)
@pytest.mark.parametrize("shape", ["plaquette", "pad_rows", "blocks", "bhz", "ns12"])
def test_vectors_and_norms_match_the_restatement(built, shape, cu, cd):
    import torch
    import hxv

    m, (nup, ndw) = _shape(shape)
    a = hxv.HxvSector.from_model(m, nup, ndw)
    b = hxv.HxvSector.from_model(m, *_target(nup, ndw, cu, cd))
    rng = np.random.default_rng(31)
    psi_h = _rand(rng, a.Dim)
    dpsi = _upload_with_nan_pads(a, psi_h)                       # a pad row of psi is never read
    ma, mb = _maps(a), _maps(b)
    lists = [_terms(rng, m.Ns, n) for n in (1, 4, 32)]
    lists.append([(m.Ns - 1, m.Ns - 2, 0.7 - 0.2j), (0, 1, 1.5j), (m.Ns - 1, m.Ns - 2, -0.3 + 0.1j)])       # a repeated pair, bath orbitals
    lists.append([(int(rng.integers(m.Ns)), int(rng.integers(m.Ns)), 1.0)])                                  # single term, coef = 1
    worst = np.zeros(2)
    for terms in lists:
        out = torch.full((b.localElems,), SENT, dtype=torch.complex128, device="cuda")
        got_d, n2 = a.apply_spin_pair(b, terms, cu, cd, dpsi, out=out)
        assert got_d is out
        raw = got_d.view(b.mpiQdw, b.pitch)
        assert (torch.view_as_real(raw[:, b.DimUp:]) == 0).all().item()                 # pad rows: exact zeros over the sentinel
        assert not (raw[:, :b.DimUp] == SENT).any().item()
        got = b.vector_to_host(got_d)
        ref = R.apply(ma, mb, terms, cu, cd, psi_h)
        s1 = sum(abs(c) for _, _, c in terms)
        bound = 4 * (len(terms) + 1) * EPS * s1 * np.abs(psi_h).max()
        dv, dn = np.abs(got - ref).max(), abs(n2 - np.vdot(ref, ref).real)
        worst = np.maximum(worst, [dv / bound, dn / (1e-13 * s1 ** 2 * np.vdot(psi_h, psi_h).real)])
        if len(terms) == 1 and terms[0][2] == 1.0:
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))             # bit for bit
    print(f"{shape} flags {int(cu)}{int(cd)}: worst error / bound: vectors {worst[0]:.3f}, norm2 {worst[1]:.3f}")
    assert worst.max() <= 1.0, worst
    a.close()
    b.close()


# ---- 2. composition with the ladders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu,cd", FLAGS)
@pytest.mark.parametrize("shape", ["pad_rows", "bhz"])
def test_single_term_equals_two_ladder_calls_in_either_order(built, shape, cu, cd):
    import torch
    import hxv

    m, (nup, ndw) = _shape(shape)
    tu, td = _target(nup, ndw, cu, cd)
    a, b = hxv.HxvSector.from_model(m, nup, ndw), hxv.HxvSector.from_model(m, tu, td)
    via_dw, via_up = hxv.HxvSector.from_model(m, nup, td), hxv.HxvSector.from_model(m, tu, ndw)
    dpsi = _upload_with_nan_pads(a, _rand(np.random.default_rng(5), a.Dim))
    for ou, od in ((0, m.Ns - 1), (m.Ns - 2, 1), (2, 2)):
        one, _ = a.apply_spin_pair(b, [(ou, od, 1.0)], cu, cd, dpsi)
        mid, _ = a.apply_ladder(via_dw, od, 1, cd, dpsi)                                # dw first, then up ...
        two, _ = via_dw.apply_ladder(b, ou, 0, cu, mid)
        assert torch.equal(_bits(one), _bits(two)), (ou, od)
        mid, _ = a.apply_ladder(via_up, ou, 0, cu, torch.nan_to_num(dpsi))              # ... and up first, then dw
        two, _ = via_up.apply_ladder(b, od, 1, cd, mid)
        assert torch.equal(_bits(one), _bits(two)), (ou, od)
        assert one.abs().max().item() > 0
    for s in (a, b, via_dw, via_up):
        s.close()


# ---- 3. real states, repeated calls, hermiticity ----------------------------------------------------------------------------------------
def test_real_state_with_real_coefficients_stays_real_and_calls_repeat_bit_for_bit(built):
    import torch
    import hxv

    m, (nup, ndw) = _shape("blocks")
    rng = np.random.default_rng(8)
    a = hxv.HxvSector.from_model(m, nup, ndw)
    for cu, cd in FLAGS:
        b = hxv.HxvSector.from_model(m, *_target(nup, ndw, cu, cd))
        dpsi = _upload_with_nan_pads(a, _rand(rng, a.Dim, real=True))
        terms = _terms(rng, m.Ns, 8, real=True)
        one, n1 = a.apply_spin_pair(b, terms, cu, cd, dpsi)
        two, n2 = a.apply_spin_pair(b, terms, cu, cd, dpsi)
        assert not one.imag.any().item() and one.real.any().item()                      # the real-vector Lanczos path stays open
        assert torch.equal(_bits(one), _bits(two)) and n1 == n2                         # the same bits on every call
        b.close()
    a.close()


@pytest.mark.parametrize("cu,cd", FLAGS)
def test_hermiticity_on_the_device(built, cu, cd):
    import torch
    import hxv

    m, (nup, ndw) = _shape("bhz")
    rng = np.random.default_rng(12)
    a, b = hxv.HxvSector.from_model(m, nup, ndw), hxv.HxvSector.from_model(m, *_target(nup, ndw, cu, cd))
    psi, phi = a.vector_from_host(_rand(rng, a.Dim)), b.vector_from_host(_rand(rng, b.Dim))
    terms = _terms(rng, m.Ns, 6)
    o_psi, _ = a.apply_spin_pair(b, terms, cu, cd, psi)
    od_phi, _ = b.apply_spin_pair(a, R.dagger(terms), not cu, not cd, phi)
    lhs, rhs = torch.vdot(phi, o_psi).item(), np.conj(torch.vdot(psi, od_phi).item())
    print(f"flags {int(cu)}{int(cd)}: |<phi|O psi> - conj(<psi|O^+ phi>)| = {abs(lhs - rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-13 * sum(abs(c) for _, _, c in terms)
    a.close()
    b.close()


# ---- 4. device row order ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu,cd", [(False, False), (False, True)])
def test_row_order_on_either_side_gives_the_same_host_vectors(built, monkeypatch, cu, cd):
    import hxv

    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    monkeypatch.setenv("HXV_ROW_ORDER_BITS", "8")
    from hxv import models

    m, (nup, ndw) = models.hm_2dsquare(Nbath=2), (6, 6)          # Ns = 12, the cluster the row-order tests use: DimUp 924 -> 792
    rng = np.random.default_rng(21)
    psi_h, terms = None, _terms(rng, m.Ns, 6)
    results = []
    for oa, ob in itertools.product("01", repeat=2):
        hxv.sector_cache_clear()
        monkeypatch.setenv("HXV_ROW_ORDER", oa)
        a = hxv.HxvSector.from_model(m, nup, ndw)
        monkeypatch.setenv("HXV_ROW_ORDER", ob)
        b = hxv.HxvSector.from_model(m, *_target(nup, ndw, cu, cd))
        assert (a.row_perm is not None) == (oa == "1") and (b.row_perm is not None) == (ob == "1")
        if psi_h is None:
            psi_h = _rand(rng, a.Dim)
        out, n2 = a.apply_spin_pair(b, terms, cu, cd, _upload_with_nan_pads(a, psi_h))
        results.append((b.vector_to_host(out), n2))
        a.close()
        b.close()
    hxv.sector_cache_clear()
    ref = R.apply(R.sector_maps(m.Ns, nup, ndw), R.sector_maps(m.Ns, *_target(nup, ndw, cu, cd)), terms, cu, cd, psi_h)
    assert np.abs(results[0][0] - ref).max() <= 4 * 7 * EPS * sum(abs(c) for _, _, c in terms) * np.abs(psi_h).max()
    for v, n2 in results[1:]:
        assert np.array_equal(_host_bits(v), _host_bits(results[0][0]))                 # bit for bit, whichever side has an order
        assert abs(n2 - results[0][1]) <= 1e-13 * results[0][1]                         # (the norm's summation order follows the rows)


# ---- 5. susceptibilities ----------------------------------------------------------------------------------------------------------------
def _ground_state(name):
    m, (nup, ndw), real = R.chi_fixture(name)
    w, U, maps = R.dense_sector(m, nup, ndw)
    psi = R.real_gauge(U[:, 0]) if real else U[:, 0].astype(np.complex128)
    return m, (nup, ndw), real, w[0], psi, maps


def _lehmann(m, sector, e0, psi, maps, ops, cu, cd, z, drop=()):
    """the dense sum over both neighbours; -> (chi, the sector O^+ reaches or None, the sector O reaches or None)"""
    nup, ndw = sector
    sides, secs = [], []
    for lower in (False, True):
        fu, fd = (cu, cd) if lower else (not cu, not cd)
        tu, td = _target(nup, ndw, fu, fd)
        if not (0 <= tu <= m.Ns and 0 <= td <= m.Ns):
            sides.append(None)
            secs.append(None)
            continue
        wb, Ub, mb = R.dense_sector(m, tu, td)
        sides.append((wb, Ub, [R.apply(maps, mb, op if lower else R.dagger(op), fu, fd, psi) for op in ops]))
        secs.append((tu, td))
    return R.lehmann_chi(e0, sides[0], sides[1], z), secs[0], secs[1]


def _device_chi(m, sector, e0, psi, ops, cu, cd, z, s_raise, s_lower):
    import hxv
    from hxv import observables

    sec = hxv.HxvSector.from_model(m, *sector)
    up = hxv.HxvSector.from_model(m, *s_raise) if s_raise else None
    lo = hxv.HxvSector.from_model(m, *s_lower) if s_lower else None
    dpsi = sec.vector_from_host(psi)
    secs = [s for s in (sec, up, lo) if s is not None]
    pcie = [(s.stats()["h2d_bytes"], s.stats()["d2h_bytes"]) for s in secs]
    nl = max(s.Dim for s in secs)                                # nlanc >= Dim: the new code is measured, not a truncation
    chi, info = observables.spin_pair_susceptibility(sec, lo, up, dpsi, e0, ops, cu, cd, z, nlanc=nl)
    assert [(s.stats()["h2d_bytes"], s.stats()["d2h_bytes"]) for s in secs] == pcie   # nothing Dim-sized crossed PCIe
    for s in secs:
        s.close()
    return chi, info


@pytest.mark.parametrize("name", ["plaquette", "chain"])
def test_spin_flip_susceptibility_is_twice_the_longitudinal_one_on_a_singlet(built, name):
    import hxv
    from hxv import observables

    m, (nup, ndw), real, e0, psi, _ = _ground_state(name)
    nimp = m.Nlat * m.Norb
    z = 1j * R.NU
    ops = observables.spin_pair_terms("spin_flip", nimp)
    chi, info = _device_chi(m, (nup, ndw), e0, psi, ops, False, True, z, (nup + 1, ndw - 1), (nup - 1, ndw + 1))
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    zz, _ = observables.susceptibility(sec, sec.vector_from_host(psi), e0, "spin", z, nlanc=sec.Dim)
    sec.close()
    err, scale = np.abs(chi - 2.0 * zz).max(), max(1.0, np.abs(chi).max())
    print(f"{name}: max|chi_-+| = {np.abs(chi).max():.3e}, |chi_-+ - 2 chi_zz| = {err:.3e}, steps {info['nsteps_raise'].tolist()} {info['nsteps_lower'].tolist()}")
    assert chi.shape == (R.NFREQ, nimp, nimp) and np.abs(chi).max() > 1e-2
    assert err <= 1e-9 * scale, (err, scale)


def _plaquette_waves():
    """the on-site s-wave (4 terms) and the d-wave (8 terms: +x bonds, -y bonds, both orders of the bond) pair operators of the 2x2 cluster,
    sites 0 1 / 2 3 as hm_2dsquare numbers them"""
    s_wave = [(i, i, 0.5) for i in range(4)]
    d_wave = []
    for (i, j), sg in (((0, 1), 1.0), ((2, 3), 1.0), ((0, 2), -1.0), ((1, 3), -1.0)):
        d_wave += [(i, j, 0.5 * sg), (j, i, 0.5 * sg)]
    return [d_wave, s_wave]


@pytest.mark.parametrize("name,kind", [("plaquette", "local_pair"), ("chain", "local_pair"), ("square", "waves"), ("bhz", "local_pair")])
def test_pair_susceptibility_matches_the_lehmann_sum(built, name, kind):
    from hxv import observables

    m, sector, real, e0, psi, maps = _ground_state(name)
    ops = _plaquette_waves() if kind == "waves" else observables.spin_pair_terms(kind, m.Nlat * m.Norb)
    z = 1j * R.NU
    ref, s_raise, s_lower = _lehmann(m, sector, e0, psi, maps, ops, False, False, z)
    chi, info = _device_chi(m, sector, e0, psi, ops, False, False, z, s_raise, s_lower)
    err, scale = np.abs(chi - ref).max(), max(1.0, np.abs(ref).max())
    print(f"{name} {kind}: max|chi| = {np.abs(ref).max():.3e}, |chi - Lehmann| = {err:.3e}, norms {info['norm2_raise'].tolist()} {info['norm2_lower'].tolist()}")
    assert chi.shape == (R.NFREQ, len(ops), len(ops)) and np.abs(ref).max() > 1e-3
    assert err <= 1e-9 * scale, (err, scale)


@pytest.mark.parametrize("sector,kind,flags,missing", [((0, 2), "local_pair", (False, False), "lower"), ((2, 4), "spin_flip", (False, True), "lower"),
                                                       ((4, 3), "local_pair", (False, False), "raise")])
def test_missing_sector_gives_a_zero_sum_and_the_other_still_matches(built, sector, kind, flags, missing):
    from hxv import models, observables

    m = models.plaquette_2x2_nobath(U=4.0, t=1.0, hfmode=True, xmu=0.3)
    w, U, maps = R.dense_sector(m, *sector)
    psi, e0 = R.real_gauge(U[:, 0]), w[0]
    ops = observables.spin_pair_terms(kind, 4)
    z = 1j * R.NU + 0.1                                          # off the axis: these sectors are not ground states, e_n may vanish
    ref, s_raise, s_lower = _lehmann(m, sector, e0, psi, maps, ops, *flags, z)
    assert (s_lower if missing == "lower" else s_raise) is None and (s_raise if missing == "lower" else s_lower) is not None
    chi, info = _device_chi(m, sector, e0, psi, ops, *flags, z, s_raise, s_lower)
    assert not info["norm2_" + missing].any() and not info["nsteps_" + missing].any()
    err = np.abs(chi - ref).max()
    print(f"plaquette {sector} {kind}, no {missing} sector: |chi - Lehmann| = {err:.3e}, max|chi| = {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 1e-3 and err <= 1e-9 * max(1.0, np.abs(ref).max())


# ---- 6. errors, split handles, buffers --------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(built):
    import torch
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    L = hxv.load_library()
    ARG, STATE = 1, 3
    m = models.plaquette_2x2_nobath()
    a, b, wrong = hxv.HxvSector.from_model(m, 2, 2), hxv.HxvSector.from_model(m, 1, 1), hxv.HxvSector.from_model(m, 1, 2)
    other_ns = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2), 2, 2)
    dpsi = a.vector_from_host(_rand(np.random.default_rng(1), a.Dim))
    out = torch.full((64,), SENT, dtype=torch.complex128, device="cuda")
    ou, od = np.array([0, 3], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    cf = np.array([1.0, 0.0, 0.5, -0.5])
    n2 = C.c_double(7.0)
    pi, pd = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_double)))
    big = np.zeros(33, dtype=np.int32)
    bad_hi, bad_lo = np.array([0, 4], dtype=np.int32), np.array([-1, 0], dtype=np.int32)
    nan_cf, inf_cf = cf.copy(), cf.copy()
    nan_cf[3], inf_cf[0] = np.nan, np.inf
    h, t, v, o, r = a._h, b._h, dpsi.data_ptr(), out.data_ptr(), C.byref(n2)
    bad = {
        "NULL argument": (None, t, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r),
        "NULL argument ": (h, None, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r),
        "NULL argument  ": (h, t, 0, 0, 2, None, pi(od), pd(cf), v, o, r),
        "NULL argument   ": (h, t, 0, 0, 2, pi(ou), None, pd(cf), v, o, r),
        "NULL argument    ": (h, t, 0, 0, 2, pi(ou), pi(od), None, v, o, r),
        "NULL argument     ": (h, t, 0, 0, 2, pi(ou), pi(od), pd(cf), None, o, r),
        "NULL argument      ": (h, t, 0, 0, 2, pi(ou), pi(od), pd(cf), v, None, r),
        "number of terms": (h, t, 0, 0, 0, pi(ou), pi(od), pd(cf), v, o, r),
        "number of terms ": (h, t, 0, 0, 33, pi(big), pi(big), pd(np.ones(66)), v, o, r),
        "orbital outside": (h, t, 0, 0, 2, pi(bad_hi), pi(od), pd(cf), v, o, r),
        "orbital outside ": (h, t, 0, 0, 2, pi(ou), pi(bad_lo), pd(cf), v, o, r),
        "not finite": (h, t, 0, 0, 2, pi(ou), pi(od), pd(nan_cf), v, o, r),
        "not finite ": (h, t, 0, 0, 2, pi(ou), pi(od), pd(inf_cf), v, o, r),
        "d_out == d_psi": (h, t, 0, 0, 2, pi(ou), pi(od), pd(cf), v, v, r),
        "different Ns": (h, other_ns._h, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r),
        "not the sector": (h, wrong._h, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r),
        "not the sector ": (h, t, 1, 1, 2, pi(ou), pi(od), pd(cf), v, o, r),
        "not the sector  ": (h, t, 0, 1, 2, pi(ou), pi(od), pd(cf), v, o, r),
    }
    torch.cuda.synchronize()
    for text, args in bad.items():
        assert L.hxv_apply_spin_pair(*args) == ARG, text
        msg = L.hxv_last_error().decode()
        assert "hxv_apply_spin_pair" in msg and text.strip() in msg, (text, msg)
    orc = OracleSector(m, 2, 2)
    csr = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag())
    panel = hxv.HxvSector.dw_panel(m, 2, 2, 4)
    for other in (csr, panel):
        assert L.hxv_apply_spin_pair(other._h, t, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r) == STATE
        assert "basis maps" in L.hxv_last_error().decode()
        assert L.hxv_apply_spin_pair(h, other._h, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, r) == STATE
        other.close()
    torch.cuda.synchronize()
    assert n2.value == 7.0 and torch.equal(out, torch.full_like(out, SENT))             # nothing was written
    assert L.hxv_apply_spin_pair(h, t, 0, 0, 2, pi(ou), pi(od), pd(cf), v, o, None) == 0    # norm2 may be NULL
    with pytest.raises(hxv.HxvError, match="padded layout"):
        a.apply_spin_pair(b, [(0, 0, 1.0)], False, False, dpsi[:-1].contiguous())
    for s in (a, b, wrong, other_ns):
        s.close()


def test_split_handles_are_refused_on_every_rank_and_nobody_waits(built):
    import torch
    import hxv

    m, (nup, ndw) = _shape("pad_rows")

    def rank(r, group):
        a = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=2)
        b = hxv.HxvSector.from_model(m, nup - 1, ndw - 1, rank=r, nranks=2)
        group.join(b)                                            # `to` even has its communicator: the refusal comes first
        whole = hxv.HxvSector.from_model(m, nup - 1, ndw - 1)
        psi = torch.zeros(a.localElems, dtype=torch.complex128, device="cuda")
        out = torch.full((whole.localElems,), SENT, dtype=torch.complex128, device="cuda")
        msgs = []
        for src, dst in ((a, b), (a, whole)):
            with pytest.raises(hxv.HxvError) as ei:
                src.apply_spin_pair(dst, [(0, 0, 1.0)], False, False, psi, out=out[:dst.localElems])
            msgs.append(str(ei.value))
        torch.cuda.synchronize()
        untouched = torch.equal(out, torch.full_like(out, SENT))
        for s in (a, b, whole):
            s.close()
        return msgs, untouched

    for msgs, untouched in hxv.run_ranks(2, rank):
        assert all("status 4" in t and "split sectors" in t for t in msgs), msgs
        assert untouched


def test_handles_and_buffers_are_back_after_fifty_calls(built):
    import hxv

    m, (nup, ndw) = _shape("blocks")
    live0 = hxv.live_handles()
    a, b = hxv.HxvSector.from_model(m, nup, ndw), hxv.HxvSector.from_model(m, nup - 1, ndw + 1)
    dpsi = a.vector_from_host(_rand(np.random.default_rng(2), a.Dim))
    terms = _terms(np.random.default_rng(3), m.Ns, 5)
    first = a.apply_spin_pair(b, terms, False, True, dpsi)                             # (the tables are built here)
    st0, pool0 = (a.stats(), b.stats()), hxv.pool_stats()
    for _ in range(50):
        again = a.apply_spin_pair(b, terms, False, True, dpsi, out=first[0])
        assert again[1] == first[1]
    st1, pool1 = (a.stats(), b.stats()), hxv.pool_stats()
    assert pool1 == pool0
    assert [s["device_bytes"] for s in st1] == [s["device_bytes"] for s in st0]
    assert [(s["h2d_bytes"], s["d2h_bytes"]) for s in st1] == [(s["h2d_bytes"], s["d2h_bytes"]) for s in st0]
    a.close()
    b.close()
    assert hxv.live_handles() == live0
