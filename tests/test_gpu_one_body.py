"""One-body operators c^+_i c_j inside a sector on the MI355X (include/hxv.h: hxv_apply_one_body; HxvSector.apply_one_body,
hxv.observables.one_body_terms / one_body_susceptibility / one_body_density_matrix) against the numpy restatement of tests/one_body_ref.py.

  - the vectors, 1 / 4 / 32 terms with random complex coefficients over both spins and all orbitals (bath and diagonal ones included):
    |d| <= 4 (nterms + 1) 2^-53 sum|coef| max|psi| without the mean (one rounding per product and per add, complex multiplication),
    + 4 2^-53 |m| max|psi| with it; mean within 1e-13 sum|coef|, norm2 within 1e-13 (sum|coef|)^2 <psi|psi>; a single term with coef = 1
    bit for bit
  - a single term equals the two ladder calls through (nup - 1, ndw) / (nup, ndw - 1), bit for bit
  - identities: sum_i n_i,s has mean n_s and no fluctuation; the model's hopping terms reproduce H psi - D psi; sectors with no up particle
    or no up hole give zeros
  - pad rows: never read (NaN planted in psi's), written as exact zeros (over a sentinel); a real state with real coefficients stays real;
    two identical calls; hermiticity on the device; the device row order on and off: the same host vector bit for bit
  - chi of bond, current, hop and exciton operators equals the dense Lehmann sum over the sector's own spectrum without the ground state:
    64 bosonic frequencies, beta = 50, 1e-9 * max(1, max|chi|), dense ground state uploaded, nlanc >= Dim
  - the one-body density matrix; argument errors, split handles, buffers."""
import ctypes as C

import numpy as np
import pytest

import one_body_ref as R
import spin_pair_ref as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SENT = complex(7.0, 7.0)


def _shape(name):
    from hxv import models

    return {"plaquette": lambda: (models.plaquette_2x2_nobath(), (2, 2)),                               # 36 elements
            "pad_rows": lambda: (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (4, 3)),      # DimUp 15 -> pitch 16
            "blocks": lambda: (models.hm_1dchain(Nlat=2, Nbath=3), (4, 4)),
            "bhz": lambda: (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3)),                           # orbitals up to 7
            "ns12": lambda: (models.hm_1dchain(Nlat=2, Nbath=5), (6, 6))}[name]()                       # 924 rows: four row chunks


def _rand(rng, n, real=False):
    v = (rng.standard_normal(n) + (0.0 if real else 1j * rng.standard_normal(n))).astype(np.complex128)
    return v / np.linalg.norm(v)


def _terms(rng, ns, n, real=False):
    return [(int(rng.integers(2)), int(rng.integers(ns)), int(rng.integers(ns)), complex(rng.standard_normal(), 0.0 if real else rng.standard_normal()))
            for _ in range(n)]


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
    calls (sign * 0) and the row-order conversion to the host (basis sign * 0) may leave -0; every other pattern is compared as it is"""
    import torch

    return (torch.view_as_real(t) + 0.0).view(torch.int64)


def _host_bits(v):
    return (v.view(np.float64) + 0.0).view(np.uint64)


# ---- 1. the vectors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subtract", [False, True])
@pytest.mark.parametrize("shape", ["plaquette", "pad_rows", "blocks", "bhz", "ns12"])
def test_vectors_means_and_norms_match_the_restatement(built, shape, subtract):
    import torch
    import hxv

    m, (nup, ndw) = _shape(shape)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    rng = np.random.default_rng(31)
    psi_h = _rand(rng, sec.Dim)
    dpsi = _upload_with_nan_pads(sec, psi_h)                     # a pad row of psi is never read
    maps = _maps(sec)
    lists = [_terms(rng, m.Ns, n) for n in (1, 4, 32)]
    lists.append([(1, m.Ns - 1, m.Ns - 2, 0.7 - 0.2j), (0, 0, 1, 1.5j), (1, m.Ns - 1, m.Ns - 2, -0.3 + 0.1j), (0, 2, 2, 0.4)])  # a repeat, bath, diagonal
    lists.append([(int(rng.integers(2)), int(rng.integers(m.Ns)), int(rng.integers(m.Ns)), 1.0)])                            # single term, coef = 1
    worst = np.zeros(3)
    pp = np.vdot(psi_h, psi_h).real
    for terms in lists:
        out = torch.full((sec.localElems,), SENT, dtype=torch.complex128, device="cuda")
        got_d, mean, n2 = sec.apply_one_body(terms, dpsi, subtract_mean=subtract, out=out)
        assert got_d is out
        raw = got_d.view(sec.mpiQdw, sec.pitch)
        assert (torch.view_as_real(raw[:, sec.DimUp:]) == 0).all().item()               # pad rows: exact zeros over the sentinel
        assert not (raw[:, :sec.DimUp] == SENT).any().item()
        got = sec.vector_to_host(got_d)
        ref, rmean, rn2 = R.apply(maps, terms, psi_h, subtract)
        s1 = sum(abs(t[3]) for t in terms)
        bound = 4 * (len(terms) + 1) * EPS * s1 * np.abs(psi_h).max() + (4 * EPS * abs(rmean) * np.abs(psi_h).max() if subtract else 0.0)
        dv, dm, dn = np.abs(got - ref).max(), abs(mean - rmean), abs(n2 - rn2)
        worst = np.maximum(worst, [dv / bound, dm / (1e-13 * s1), dn / (1e-13 * s1 ** 2 * pp)])
        if len(terms) == 1 and terms[0][3] == 1.0 and not subtract:
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))             # bit for bit
    print(f"{shape} subtract {int(subtract)}: worst error / bound: vectors {worst[0]:.3f}, mean {worst[1]:.3f}, norm2 {worst[2]:.3f}")
    assert worst.max() <= 1.0, worst
    sec.close()


# ---- 2. composition with the ladders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 1])
@pytest.mark.parametrize("shape", ["pad_rows", "bhz"])
def test_single_term_equals_two_ladder_calls(built, shape, spin):
    import torch
    import hxv

    m, (nup, ndw) = _shape(shape)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    via = hxv.HxvSector.from_model(m, nup - (spin == 0), ndw - (spin == 1))
    dpsi = _upload_with_nan_pads(sec, _rand(np.random.default_rng(5), sec.Dim))
    for i, j in ((0, m.Ns - 1), (m.Ns - 2, 1), (2, 2), (1, 0)):
        one, _, _ = sec.apply_one_body([(spin, i, j, 1.0)], dpsi, subtract_mean=False)
        mid, _ = sec.apply_ladder(via, j, spin, False, dpsi)                            # c_j, then c^+_i
        two, _ = via.apply_ladder(sec, i, spin, True, mid)
        assert torch.equal(_bits(one), _bits(two)), (spin, i, j)
        assert one.abs().max().item() > 0
    sec.close()
    via.close()


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pad_rows", "bhz"])
def test_total_number_of_a_spin_has_its_mean_and_no_fluctuation(built, shape):
    import hxv

    m, (nup, ndw) = _shape(shape)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = _upload_with_nan_pads(sec, _rand(np.random.default_rng(6), sec.Dim))
    for spin, n in ((0, nup), (1, ndw)):
        out, mean, n2 = sec.apply_one_body([(spin, i, i, 1.0) for i in range(m.Ns)], dpsi, subtract_mean=True)
        print(f"{shape} spin {spin}: mean - n = {abs(mean - n):.3e}, norm2 of the fluctuation {n2:.3e}")
        assert abs(mean - n) <= 1e-13 and n2 <= 1e-26
    sec.close()


def test_hopping_terms_reproduce_the_off_diagonal_part_of_h(built):
    import torch
    import hxv
    from hxv import models

    m = models.plaquette_2x2_nobath()
    sec = hxv.HxvSector.from_model(m, 2, 2)
    assert sec.row_perm is None                                  # (device layout = the reference's rows with padded columns)
    psi_h = _rand(np.random.default_rng(9), sec.Dim)
    h = np.asarray(m.impHloc)[:, :, 0, 0, 0, 0]
    terms = [(s, i, j, h[i, j]) for s in (0, 1) for i in range(4) for j in range(4) if i != j and h[i, j] != 0]
    assert len(terms) == 16                                      # four bonds, both directions, both spins: the kinetic operator
    out, _, _ = sec.apply_one_body(terms, sec.vector_from_host(psi_h), subtract_mean=False)
    hpsi = sec.apply_device(torch.from_numpy(psi_h).cuda()).cpu().numpy()
    want = hpsi - sec.diag() * psi_h
    err = np.abs(sec.vector_to_host(out) - want).max()
    print(f"|sum t_ij c+_i c_j psi - (H psi - D psi)| = {err:.3e}")
    assert np.abs(want).max() > 0.1 and err <= 1e-13
    sec.close()


@pytest.mark.parametrize("nup", [0, 4])
def test_sectors_without_an_up_particle_or_an_up_hole_give_zeros(built, nup):
    import torch
    import hxv
    from hxv import models

    m = models.plaquette_2x2_nobath()
    sec = hxv.HxvSector.from_model(m, nup, 2)
    dpsi = _upload_with_nan_pads(sec, _rand(np.random.default_rng(3), sec.Dim))
    out = torch.full((sec.localElems,), SENT, dtype=torch.complex128, device="cuda")
    _, mean, n2 = sec.apply_one_body([(0, 0, 1, 1.0), (0, 3, 2, -0.5j), (0, 1, 0, 2.0)], dpsi, subtract_mean=False, out=out)
    assert (torch.view_as_real(out) == 0).all().item() and mean == 0 and n2 == 0.0     # all dead
    sec.close()


# ---- 4. real states, repeated calls, hermiticity, row order -----------------------------------------------------------------------------
def test_real_state_with_real_coefficients_stays_real_and_calls_repeat_bit_for_bit(built):
    import torch
    import hxv

    m, (nup, ndw) = _shape("blocks")
    rng = np.random.default_rng(8)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = _upload_with_nan_pads(sec, _rand(rng, sec.Dim, real=True))
    terms = _terms(rng, m.Ns, 8, real=True)
    for subtract in (False, True):
        one, m1, n1 = sec.apply_one_body(terms, dpsi, subtract_mean=subtract)
        two, m2, n2 = sec.apply_one_body(terms, dpsi, subtract_mean=subtract)
        assert not one.imag.any().item() and one.real.any().item() and m1.imag == 0     # the real-vector Lanczos path stays open
        assert torch.equal(_bits(one), _bits(two)) and n1 == n2 and m1 == m2            # the same bits on every call
    sec.close()


def test_hermiticity_on_the_device(built):
    import torch
    import hxv

    m, (nup, ndw) = _shape("bhz")
    rng = np.random.default_rng(12)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    psi, phi = sec.vector_from_host(_rand(rng, sec.Dim)), sec.vector_from_host(_rand(rng, sec.Dim))
    terms = _terms(rng, m.Ns, 6)
    o_psi, _, _ = sec.apply_one_body(terms, psi, subtract_mean=False)
    od_phi, _, _ = sec.apply_one_body(R.dagger(terms), phi, subtract_mean=False)
    lhs, rhs = torch.vdot(phi, o_psi).item(), np.conj(torch.vdot(psi, od_phi).item())
    print(f"|<phi|O psi> - conj(<psi|O^+ phi>)| = {abs(lhs - rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-13 * sum(abs(t[3]) for t in terms)
    sec.close()


def test_row_order_on_and_off_gives_the_same_host_vector(built, monkeypatch):
    import hxv
    from hxv import models

    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    monkeypatch.setenv("HXV_ROW_ORDER_BITS", "8")
    m, (nup, ndw) = models.hm_2dsquare(Nbath=2), (6, 6)          # Ns = 12, the cluster the row-order tests use
    rng = np.random.default_rng(21)
    terms = _terms(rng, m.Ns, 6)
    psi_h, results = None, []
    for order in "01":
        hxv.sector_cache_clear()
        monkeypatch.setenv("HXV_ROW_ORDER", order)
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        assert (sec.row_perm is not None) == (order == "1")
        if psi_h is None:
            psi_h = _rand(rng, sec.Dim)
        for subtract in (False, True):
            out, mean, n2 = sec.apply_one_body(terms, _upload_with_nan_pads(sec, psi_h), subtract_mean=subtract)
            results.append((sec.vector_to_host(out), mean, n2))
        sec.close()
    hxv.sector_cache_clear()
    ref, _, _ = R.apply(S.sector_maps(m.Ns, nup, ndw), terms, psi_h)
    assert np.abs(results[0][0] - ref).max() <= 4 * 7 * EPS * sum(abs(t[3]) for t in terms) * np.abs(psi_h).max()
    assert np.array_equal(_host_bits(results[2][0]), _host_bits(results[0][0]))         # bit for bit, with or without an order
    for off, on in ((results[0], results[2]), (results[1], results[3])):                # (the sums' order follows the rows)
        assert abs(on[1] - off[1]) <= 1e-13 * 6 and abs(on[2] - off[2]) <= 1e-13 * max(off[2], 1.0)
    assert np.abs(results[3][0] - results[1][0]).max() <= 4 * EPS * abs(results[1][1]) * np.abs(psi_h).max() + 1e-13 * 6 * np.abs(psi_h).max()


# ---- 5. susceptibilities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("plaquette", "hermitian"), ("plaquette", "hop"), ("chain", "hermitian"), ("bhz", "exciton"),
                                        ("square", "hermitian")])
def test_susceptibility_matches_the_lehmann_sum(built, name, which):
    import hxv
    from hxv import observables

    m, (nup, ndw), real = S.chi_fixture(name)
    w, U, maps = S.dense_sector(m, nup, ndw)
    psi = S.real_gauge(U[:, 0]) if real else U[:, 0].astype(np.complex128)
    Ug = U.copy()
    Ug[:, 0] = psi
    ops = R.chi_ops(name)[which]
    z = 1j * S.NU
    ref = R.lehmann_chi(w, Ug, maps, ops, z)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = sec.vector_from_host(psi)
    pcie = (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"])
    chi, info = observables.one_body_susceptibility(sec, dpsi, w[0], ops, z, nlanc=sec.Dim)     # nlanc >= Dim: the new code is measured, not a truncation
    assert (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"]) == pcie                         # nothing Dim-sized crossed PCIe
    sec.close()
    err, scale = np.abs(chi - ref).max(), max(1.0, np.abs(ref).max())
    print(f"{name} {which}: max|chi| = {np.abs(ref).max():.3e}, |chi - Lehmann| = {err:.3e}, steps {info['nsteps'].tolist()}, "
          f"dropped {info['dropped_weight']:.3e}, norms {info['norm2'].tolist()}")
    assert chi.shape == (S.NFREQ, len(ops), len(ops)) and np.abs(ref).max() > 1e-3
    assert err <= 1e-9 * scale, (err, scale)
    assert info["dropped_weight"] <= 1e-20
    assert info["nsteps"].all()                                  # every run ran: no start vector of these operators vanishes
    for a, op in enumerate(ops):                                 # the means and norms are those of the restatement
        for side, lst in enumerate((R.dagger(op), op)):
            _, rm, rn2 = R.apply(maps, lst, psi, True)
            assert abs(info["mean"][side, a] - rm) <= 1e-12 and abs(info["norm2"][side, a] - rn2) <= 1e-12 * max(1.0, rn2)


def test_named_operators_are_the_restatements_term_lists(built):
    from hxv import observables

    same = lambda a, b: sorted((s, i, j, complex(c)) for s, i, j, c in a) == sorted((s, i, j, complex(c)) for s, i, j, c in b)  # noqa: E731
    assert all(same(a, b) for a, b in zip(observables.one_body_terms("bond", [(0, 1), (0, 2)]), [R.bond(0, 1), R.bond(0, 2)]))
    assert same(observables.one_body_terms("current", [(0, 1)])[0], R.current(0, 1))
    assert same(observables.one_body_terms("hop", [(0, 1)])[0], R.hop(0, 1))
    assert same(observables.one_body_terms("exciton_singlet", [(0, 1)])[0], R.exciton(0, 1, False))
    assert same(observables.one_body_terms("exciton_triplet_z", [(2, 3)])[0], R.exciton(2, 3, True))
    assert observables.one_body_terms([[(0, 1, 2, 0.5)]]) == [[(0, 1, 2, 0.5 + 0j)]]
    import hxv

    with pytest.raises(hxv.HxvError):
        observables.one_body_terms("bonds", [(0, 1)])


# ---- 6. the one-body density matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pad_rows", "bhz", "ns12"])
def test_one_body_density_matrix(built, shape):
    import hxv
    from hxv import observables

    m, (nup, ndw) = _shape(shape)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    psi_h = _rand(np.random.default_rng(14), sec.Dim)
    dpsi = sec.vector_from_host(psi_h)
    rho = observables.one_body_density_matrix(sec, dpsi)
    assert rho.shape == (2, m.Ns, m.Ns)
    if shape == "ns12":
        # 288 tables, more than an image keeps (128): the second sweep finds none of its first tables and builds them again, to the same bits
        assert np.array_equal(observables.one_body_density_matrix(sec, dpsi).view(np.float64), rho.view(np.float64))
        maps = _maps(sec)
        for s, i, j in ((0, 0, 11), (1, 7, 2), (0, 5, 5)):
            assert abs(rho[s, i, j] - R.apply(maps, [(s, i, j, 1.0)], psi_h)[1]) <= 1e-13
    assert np.abs(rho - rho.conj().transpose(0, 2, 1)).max() <= 1e-13                   # Hermitian
    assert abs(np.trace(rho[0]) - nup) <= 1e-12 and abs(np.trace(rho[1]) - ndw) <= 1e-12
    obs = observables.observables(m, [(sec, 0.0, dpsi)])
    nimp, O = m.Nlat * m.Norb, m.Norb
    spdm = obs["single_particle_density_matrix"]
    for sp in range(m.Nspin):
        block = np.array([[spdm[i // O, j // O, sp, sp, i % O, j % O] for j in range(nimp)] for i in range(nimp)])
        assert np.abs(block).max() > 1e-3 and np.abs(rho[sp, :nimp, :nimp] - block).max() <= 1e-12
    for spin, key in ((0, "dens_up"), (1, "dens_dw")):
        assert np.abs(np.diag(rho[spin])[:nimp].real - obs[key].reshape(-1)).max() <= 1e-12      # (Nlat, Norb) in C order = site * Norb + orbital
    sec.close()


# ---- 7. errors, split handles, buffers --------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(built):
    import torch
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    L = hxv.load_library()
    ARG, STATE = 1, 3
    m = models.plaquette_2x2_nobath()
    a = hxv.HxvSector.from_model(m, 2, 2)
    dpsi = a.vector_from_host(_rand(np.random.default_rng(1), a.Dim))
    out = torch.full((a.localElems,), SENT, dtype=torch.complex128, device="cuda")
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    sp, oi, oj = i32(0, 1), i32(0, 3), i32(1, 2)
    cf = np.array([1.0, 0.0, 0.5, -0.5])
    mean, n2 = (C.c_double * 2)(7.0, 7.0), C.c_double(7.0)
    pi, pd = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_double)))
    big = np.zeros(33, dtype=np.int32)
    nan_cf, inf_cf = cf.copy(), cf.copy()
    nan_cf[3], inf_cf[0] = np.nan, np.inf
    h, v, o, r = a._h, dpsi.data_ptr(), out.data_ptr(), C.byref(n2)
    bad = {
        "NULL argument": (None, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, o, mean, r),
        "NULL argument ": (h, 2, None, pi(oi), pi(oj), pd(cf), 1, v, o, mean, r),
        "NULL argument  ": (h, 2, pi(sp), None, pi(oj), pd(cf), 1, v, o, mean, r),
        "NULL argument   ": (h, 2, pi(sp), pi(oi), None, pd(cf), 1, v, o, mean, r),
        "NULL argument    ": (h, 2, pi(sp), pi(oi), pi(oj), None, 1, v, o, mean, r),
        "NULL argument     ": (h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, None, o, mean, r),
        "NULL argument      ": (h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, None, mean, r),
        "number of terms": (h, 0, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, o, mean, r),
        "number of terms ": (h, 33, pi(big), pi(big), pi(big), pd(np.ones(66)), 1, v, o, mean, r),
        "spin": (h, 2, pi(i32(0, 2)), pi(oi), pi(oj), pd(cf), 1, v, o, mean, r),
        "spin ": (h, 2, pi(i32(-1, 0)), pi(oi), pi(oj), pd(cf), 1, v, o, mean, r),
        "orbital outside": (h, 2, pi(sp), pi(i32(0, 4)), pi(oj), pd(cf), 1, v, o, mean, r),
        "orbital outside ": (h, 2, pi(sp), pi(oi), pi(i32(-1, 0)), pd(cf), 1, v, o, mean, r),
        "not finite": (h, 2, pi(sp), pi(oi), pi(oj), pd(nan_cf), 1, v, o, mean, r),
        "not finite ": (h, 2, pi(sp), pi(oi), pi(oj), pd(inf_cf), 1, v, o, mean, r),
        "d_out == d_psi": (h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, v, mean, r),
    }
    torch.cuda.synchronize()
    for text, args in bad.items():
        assert L.hxv_apply_one_body(*args) == ARG, text
        msg = L.hxv_last_error().decode()
        assert "hxv_apply_one_body" in msg and text.strip() in msg, (text, msg)
    orc = OracleSector(m, 2, 2)
    csr = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag())
    panel = hxv.HxvSector.dw_panel(m, 2, 2, 4)
    for other in (csr, panel):
        assert L.hxv_apply_one_body(other._h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, o, mean, r) == STATE
        assert "hxv_apply_one_body" in L.hxv_last_error().decode() and "basis maps" in L.hxv_last_error().decode()
        other.close()
    torch.cuda.synchronize()
    assert list(mean) == [7.0, 7.0] and n2.value == 7.0 and torch.equal(out, torch.full_like(out, SENT))      # nothing was written
    # a state that is zero or not finite: known only from the gather pass, so the scalars are untouched but d_out is not (include/hxv.h)
    for bad_psi in (torch.zeros_like(dpsi), torch.full_like(dpsi, complex(np.inf, 0.0))):
        assert L.hxv_apply_one_body(h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, bad_psi.data_ptr(), o, mean, r) == ARG
        assert "hxv_apply_one_body" in L.hxv_last_error().decode() and "zero or not finite" in L.hxv_last_error().decode()
    assert list(mean) == [7.0, 7.0] and n2.value == 7.0
    assert L.hxv_apply_one_body(h, 2, pi(sp), pi(oi), pi(oj), pd(cf), 1, v, o, None, None) == 0               # mean and norm2 may be NULL
    with pytest.raises(hxv.HxvError, match="padded layout"):
        a.apply_one_body([(0, 0, 1, 1.0)], dpsi[:-1].contiguous())
    a.close()


def test_split_handles_are_refused_on_every_rank_and_nobody_waits(built):
    import torch
    import hxv

    m, (nup, ndw) = _shape("pad_rows")

    def rank(r, group):
        a = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=2)
        group.join(a)                                            # the handle even has its communicator: the refusal comes first
        psi = torch.zeros(a.localElems, dtype=torch.complex128, device="cuda")
        out = torch.full((a.localElems,), SENT, dtype=torch.complex128, device="cuda")
        with pytest.raises(hxv.HxvError) as ei:
            a.apply_one_body([(0, 0, 1, 1.0)], psi, out=out)
        torch.cuda.synchronize()
        untouched = torch.equal(out, torch.full_like(out, SENT))
        a.close()
        return str(ei.value), untouched

    for msg, untouched in hxv.run_ranks(2, rank):
        assert "status 4" in msg and "split sectors" in msg, msg
        assert untouched


def test_handles_and_buffers_are_back_after_fifty_calls(built):
    import hxv

    m, (nup, ndw) = _shape("blocks")
    live0 = hxv.live_handles()
    a = hxv.HxvSector.from_model(m, nup, ndw)
    dpsi = a.vector_from_host(_rand(np.random.default_rng(2), a.Dim))
    terms = _terms(np.random.default_rng(3), m.Ns, 5)
    first = a.apply_one_body(terms, dpsi)                                               # (the tables are built here)
    st0, pool0, blocks0 = a.stats(), hxv.pool_stats(), a.get_option("pool_live_blocks")
    for _ in range(50):
        again = a.apply_one_body(terms, dpsi, out=first[0])
        assert again[1] == first[1] and again[2] == first[2]
    st1, pool1 = a.stats(), hxv.pool_stats()
    assert pool1["cached_bytes"] == pool0["cached_bytes"] and pool1["misses"] == pool0["misses"]    # the scratch block goes out and comes back
    assert a.get_option("pool_live_blocks") == blocks0
    assert st1["device_bytes"] == st0["device_bytes"]
    assert (st1["h2d_bytes"], st1["d2h_bytes"]) == (st0["h2d_bytes"], st0["d2h_bytes"])
    a.close()
    assert hxv.live_handles() == live0
