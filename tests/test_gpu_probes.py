"""Probe overlaps on the MI355X (include/hxv.h: hxv_lanczos_tridiag_probes, hxv_gf_from_probes; HxvSector.lanczos_tridiag_probes, hxv.greens):
off-diagonal Green's functions G_ij from ONE Lanczos run per orbital instead of the reference's mixed channels (ED_GF_NORMAL.f90:315-903).

  - alanc / blanc / nsteps of the new driver are hxv_lanczos_tridiag's, bit for bit (host-stepped and graph-captured)
  - overlaps[k, j] = <p_j|q_k> against a numpy three-term recurrence on the oracle's dense matrix      1e-10 over the first 10 steps (the bound
    hxv.h states for two Lanczos runs over their first steps)
  - G_ij(i w_n) from the overlaps against the Lehmann sum of the dense sector                            1e-9 (the diagonal's tolerance in
    test_gpu_lanczos.py::test_impurity_green_function_vs_lehmann), 64 Matsubara frequencies at beta = 50, nlanc = min(Dim, 200)
  - against the reference's own route 1/2 (G_{i+j} - G_ii - G_jj) through hxv_lanczos_tridiag            1e-9
  - other handle kinds, the device row order, split sectors, determinism, lifetime, argument errors.

WHERE TWO RUNS ARE COMPARED STEP BY STEP the comparison covers the early steps: two Lanczos recurrences that differ by one rounding
(another summation order: split / unsplit, fused / plain, real / complex kernels) separate geometrically once Ritz values converge; 12 steps
keep an initial 1e-16 below the 1e-11 / 1e-12 the comparisons ask for on these sectors.  The Green's function itself does not have that
sensitivity and is compared from full-length runs."""
import ctypes as C

import numpy as np
import pytest
from ladder_ref import apply_op as _apply_op

pytestmark = pytest.mark.gpu

BETA, LMATS = 50.0, 64
WM = np.pi / BETA * (2 * np.arange(1, LMATS + 1) - 1)   # ED_GF_SHARED.f90:49


def _lanczos_numpy(H, v, probes, nsteps):
    """plain three-term recurrence, no re-orthogonalisation: alanc, blanc (blanc[0] = 0) and <p_j|q_k>"""
    q = v / np.linalg.norm(v)
    qm = np.zeros_like(q)
    a, b, ov = np.zeros(nsteps), np.zeros(nsteps), np.zeros((nsteps, len(probes)), dtype=complex)
    beta = 0.0
    for k in range(nsteps):
        ov[k] = [np.vdot(p, q) for p in probes]
        w = H @ q - beta * qm
        a[k] = np.vdot(q, w).real
        w = w - a[k] * q
        beta = np.linalg.norm(w)
        if k + 1 < nsteps:
            b[k + 1] = beta
        qm, q = q, w / beta
    return a, b, ov


def _rand(rng, n, real):
    v = rng.standard_normal(n) + (0.0 if real else 1j * rng.standard_normal(n))
    return v.astype(np.complex128)


def _raw_call(sec, vin, probes, nlanc, threshold=1e-12):
    """the C entry itself, whole output arrays (entries past nsteps included)"""
    import torch
    import hxv

    torch.cuda.synchronize()
    npr = len(probes)
    a, b, ov, n = np.full(nlanc, 7.0), np.full(nlanc, 7.0), np.full(2 * nlanc * max(npr, 1), 7.0), C.c_int32(-1)
    plist = (C.c_void_p * max(npr, 1))(*[p.data_ptr() for p in probes])
    pd = C.POINTER(C.c_double)
    rc = hxv.load_library().hxv_lanczos_tridiag_probes(sec._h, vin.data_ptr(), npr, plist, nlanc, a.ctypes.data_as(pd), b.ctypes.data_as(pd),
                                                       ov.ctypes.data_as(pd), threshold, C.byref(n))
    assert rc == 0, hxv.load_library().hxv_last_error()
    return a, b, ov[: 2 * nlanc * npr].view(np.complex128).reshape(nlanc, npr), n.value


# ---- 1. the same recurrence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chain_real", "bhz_complex", "breakdown"])
@pytest.mark.parametrize("nprobes", [0, 1, 8])
def test_alanc_blanc_are_the_tridiagonalisation_s_bit_for_bit(built, case, nprobes):
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    rng = np.random.default_rng(11)
    if case == "chain_real":
        m, (nup, ndw), nl, real = models.hm_1dchain(Nlat=2, Nbath=2), (4, 3), 40, True
    elif case == "bhz_complex":
        m, (nup, ndw), nl, real = models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3), 40, False
    else:
        m, (nup, ndw), nl, real = models.plaquette_2x2_nobath(), (2, 2), 60, True     # Dim = 36 < nlanc
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    v = _rand(rng, sec.Dim, real)
    if case == "breakdown":
        # the start vector lives in a small invariant subspace: an eigenvector of H -> the recurrence stops after one step
        w, U = np.linalg.eigh(OracleSector(m, nup, ndw).dense())
        v = np.real(U[:, 3] * np.exp(-1j * np.angle(U[np.abs(U[:, 3]).argmax(), 3]))).astype(np.complex128)
    v /= np.linalg.norm(v)
    dv = sec.vector_from_host(v)
    probes = [sec.vector_from_host(_rand(rng, sec.Dim, real)) for _ in range(nprobes)]
    ap, bp, ovp, n = _raw_call(sec, dv, probes, nl)
    assert sec.get_option("lanczos_real_last") == (1 if real else 0)
    for graph in (0, 1):
        sec.set_option("lanczos_graph", graph)
        a, b, n0 = sec.lanczos_tridiag(dv, nl)
        assert n == n0 and np.array_equal(ap, a) and np.array_equal(bp, b), (case, graph, n, n0)
    if case == "breakdown":
        assert n < 5
        assert not ovp[n:].any()                                   # steps that did not run: zero
    else:
        assert n == nl
    if nprobes:
        assert np.abs(ovp[:n]).max() > 0
        a2, b2, ov2, n2 = sec.lanczos_tridiag_probes(dv, probes, nl)
        assert ov2.shape == (n, nprobes) and n2 == n and np.array_equal(ov2, ovp[:n]) and np.array_equal(a2, ap)
    sec.close()


# ---- 2. the overlaps are what they say --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one_short_block", "pads_in_both_layouts", "several_blocks"])
@pytest.mark.parametrize("real", [True, False])
def test_overlaps_match_a_numpy_recurrence_on_the_dense_matrix(built, shape, real):
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    if shape == "one_short_block":
        m, (nup, ndw) = models.plaquette_2x2_nobath(), (2, 2)                         # 36 elements: less than one block of 256
    elif shape == "pads_in_both_layouts":
        m, (nup, ndw) = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (4, 3)   # DimUp = 15: pad rows in the complex and the real layout
    else:
        m, (nup, ndw) = models.hm_1dchain(Nlat=2, Nbath=3), (4, 4)                    # DimUp = 70, 5040 padded elements: 20 blocks
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    if shape == "pads_in_both_layouts":
        assert sec.DimUp % 8 != 0 and sec.DimUp % 16 != 0
    H = OracleSector(m, nup, ndw).dense()
    rng = np.random.default_rng(3)
    unit = lambda x: x / np.linalg.norm(x)  # noqa: E731
    # UNIT start vector and UNIT probes: an overlap's absolute error is proportional to its probe's norm, so the absolute 1e-10 is stated for
    # probes of norm 1 (the vectors this driver is for have norm <= 1: |c^dagger_j|gs>|^2 is an occupation)
    v, ps = unit(_rand(rng, sec.Dim, real)), [unit(_rand(rng, sec.Dim, real)) for _ in range(3)]
    dv, dps = sec.vector_from_host(v), [sec.vector_from_host(p) for p in ps]
    a, b, ov, n = sec.lanczos_tridiag_probes(dv, dps + [dv], 12)
    assert n == 12 and sec.get_option("lanczos_real_last") == (1 if real else 0)
    ar, br, ovr = _lanczos_numpy(H, v, ps + [v], 10)
    print(f"{shape} real={real}: max |d overlaps| = {np.abs(ov[:10] - ovr).max():.3e}, max |d alanc| = {np.abs(a[:10] - ar).max():.3e}, "
          f"max |d blanc| = {np.abs(b[:10] - br).max():.3e}")
    assert np.abs(ov[:10] - ovr).max() <= 1e-10, np.abs(ov[:10] - ovr).max()
    assert np.abs(a[:10] - ar).max() <= 1e-10 and np.abs(b[:10] - br).max() <= 1e-10
    # the start vector as its own probe: the first overlap is its norm
    assert abs(ov[0, 3] - 1.0) <= 1e-13
    if real:
        assert not ov.imag.any()
    # UNNORMALISED vectors scale as defined: vin -> c0 vin leaves the q_k alone (the driver normalises), probe -> c_j probe scales its column by
    # c_j; vin as its own probe gives c0 first.  Each column is compared within 1e-10 times ITS OWN factor c_j, which is known exactly.
    c0, cs = 123.0, [0.5, 7.0, 300.0]
    dv2 = sec.vector_from_host(c0 * v)
    a2, b2, ov2, _ = sec.lanczos_tridiag_probes(dv2, [sec.vector_from_host(c * p) for c, p in zip(cs, ps)] + [dv2], 12)
    for j, c in enumerate(cs):
        assert np.abs(ov2[:10, j] - c * ov[:10, j]).max() <= 1e-10 * c, (j, np.abs(ov2[:10, j] - c * ov[:10, j]).max())
    assert abs(ov2[0, 3] - c0) <= 1e-13 * c0
    assert np.abs(a2[:10] - a[:10]).max() <= 1e-10 and np.abs(b2[:10] - b[:10]).max() <= 1e-10
    sec.close()


# ---- 3. the point of it -----------------------------------------------------------------------------------------------------------------
def _lehmann(w1, U1, vecs, e0, sign):
    """G[w, j, i] = sum_n <p_j|n><n|p_i> / (i w - sign (E_n - E0))"""
    A = U1.conj().T @ np.stack(vecs, axis=1)                   # <n|p_i>
    den = 1.0 / (1j * WM[:, None] - sign * (w1[None, :] - e0))  # [w, n]
    return np.einsum("wn,nj,ni->wji", den, A.conj(), A)


def _continued_fraction(sec, dvec, n2, e0, sign, nl):
    a, b, n = sec.lanczos_tridiag(dvec, nl, threshold=1e-12)
    ev, Z = np.linalg.eigh(np.diag(a[:n]) + np.diag(b[1:n], 1) + np.diag(b[1:n], -1))
    return (n2 * Z[0, :] ** 2 / (1j * WM[:, None] - sign * (ev[None, :] - e0))).sum(axis=1)


@pytest.mark.parametrize("model_name", ["chain_B1", "plaquette"])
def test_off_diagonal_green_function_from_one_run_per_orbital(built, model_name):
    import hxv
    from hxv import greens, models
    from oracle.oracle import OracleSector

    if model_name == "chain_B1":
        m, N = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), 3
    else:
        m, N = models.plaquette_2x2_nobath(U=4.0, t=1.0, hfmode=True), 2
    nimp = m.Nlat * m.Norb
    gs = hxv.HxvSector.from_model(m, N, N)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)          # stays on the device
    w0, U0 = np.linalg.eigh(OracleSector(m, N, N).dense())
    assert abs(w0[0] - e0) < 1e-10 and w0[1] - w0[0] > 1e-6        # non-degenerate ground state
    psi_h = gs.vector_to_host(psi)
    psi_ref = U0[:, 0] * np.sign(np.vdot(U0[:, 0], psi_h).real)
    maps0 = gs.maps()
    pcie0 = (gs.stats()["h2d_bytes"], gs.stats()["d2h_bytes"])
    worst = worst_mix = 0.0
    for spin in (0, 1):
        for create in (True, False):
            d = 1 if create else -1
            nu, nd = (N + d, N) if spin == 0 else (N, N + d)
            sec = hxv.HxvSector.from_model(m, nu, nd)
            w1, U1 = np.linalg.eigh(OracleSector(m, nu, nd).dense())
            sign = 1.0 if create else -1.0
            nl = min(sec.Dim, 200)                                  # lanc_nGFiter, ED_GF_NORMAL.f90:204-207
            dev, n2s = zip(*[gs.apply_ladder(sec, i, spin, create, psi) for i in range(nimp)])
            ref_vecs = [_apply_op(psi_ref, maps0, sec.maps(), i, spin, create) for i in range(nimp)]
            Gref = _lehmann(w1, U1, ref_vecs, w0[0], sign)
            G = np.zeros_like(Gref)
            for i in range(nimp):
                a, b, ov, n = sec.lanczos_tridiag_probes(dev[i], list(dev), nl)       # ONE run: column i of G, every row j
                poles, wts = greens.poles_weights(a[:n], b[:n], ov, np.sqrt(n2s[i]))
                G[:, :, i] = greens.evaluate(poles, wts, 1j * WM, e0, sign)
                assert sec.get_option("lanczos_real_last") == 1
            worst = max(worst, np.abs(G - Gref).max())
            # the reference's route: 1/2 (G_{i+j} - G_ii - G_jj) from three continued fractions (ED_GF_NORMAL.f90:315-903, build_gf_normal)
            Gd = [_continued_fraction(sec, dev[i], n2s[i], e0, sign, nl) for i in range(nimp)]
            for i in range(nimp):
                for j in range(i + 1, nimp):
                    mix, n2 = gs.apply_ladder(sec, i, spin, create, psi)
                    mix, n2 = gs.apply_ladder(sec, j, spin, create, psi, coef=1.0, out=mix)
                    Gmix = 0.5 * (_continued_fraction(sec, mix, n2, e0, sign, nl) - Gd[i] - Gd[j])
                    worst_mix = max(worst_mix, np.abs(G[:, i, j] - Gmix).max(), np.abs(G[:, j, i] - Gmix).max())
            assert (sec.stats()["h2d_bytes"], sec.stats()["d2h_bytes"]) == (0, 0)     # everything stayed on the device
            sec.close()
    print(f"{model_name}: max |G - Lehmann| = {worst:.3e}, max |G - mixed-channel route| = {worst_mix:.3e}")
    assert pcie0[0] == gs.stats()["h2d_bytes"]
    assert worst <= 1e-9, worst
    assert worst_mix <= 1e-9, worst_mix
    gs.close()


# ---- 4. complex H: the conjugation convention -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin,create", [(0, True), (1, False)])
def test_complex_h_gij_differs_from_gji_and_matches_the_lehmann_amplitudes(built, spin, create):
    import hxv
    from hxv import greens
    from oracle.oracle import OracleSector

    from hxv import models

    m = models.bhz_2d(Nbath=0)
    gs = hxv.HxvSector.from_model(m, 4, 4)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)
    # the reference state of the Lehmann sum is the device's own eigenvector (an eigenstate of H to 1e-7 in the residual, 1e-14 in the
    # energy): nothing depends on which vector of a degenerate level the Lanczos run picked
    c = dict(psi_h=gs.vector_to_host(psi), maps=gs.maps())
    nimp = m.Nlat * m.Norb
    assert nimp == 8
    d = 1 if create else -1
    nu, nd = (4 + d, 4) if spin == 0 else (4, 4 + d)
    sec = hxv.HxvSector.from_model(m, nu, nd)
    w1, U1 = np.linalg.eigh(OracleSector(m, nu, nd).dense())
    sign = 1.0 if create else -1.0
    nl = min(sec.Dim, 200)
    dev, n2s = zip(*[gs.apply_ladder(sec, i, spin, create, psi) for i in range(nimp)])
    Gref = _lehmann(w1, U1, [_apply_op(c["psi_h"], c["maps"], sec.maps(), i, spin, create) for i in range(nimp)], e0, sign)
    G = np.zeros_like(Gref)
    for i in range(nimp):
        others = [j for j in range(nimp) if j != i]                                   # the 7 other orbitals as probes
        a, b, ov, n = sec.lanczos_tridiag_probes(dev[i], [dev[j] for j in others], nl)
        assert sec.get_option("lanczos_real_last") == 0
        poles, wts = greens.poles_weights(a[:n], b[:n], ov, np.sqrt(n2s[i]))
        G[:, others, i] = greens.evaluate(poles, wts, 1j * WM, e0, sign)
        G[:, i, i] = Gref[:, i, i]                                                    # (the diagonal is test_gpu_lanczos.py's business)
    err = np.abs(G - Gref).max()
    asym = np.abs(Gref - Gref.transpose(0, 2, 1)).max()
    print(f"bhz spin {spin} create {create}: max |G - Lehmann| = {err:.3e}, max |G_ij - G_ji| = {asym:.3e}")
    assert asym > 1e-3                                            # G_ij != G_ji here: a wrong conjugation would show
    assert err <= 1e-9, err
    sec.close()
    gs.close()


def test_imaginary_probe_on_a_real_model_takes_the_complex_path(built):
    import hxv
    from hxv import greens, models
    from oracle.oracle import OracleSector

    m, N = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), 3
    gs = hxv.HxvSector.from_model(m, N, N)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)
    psi_h = gs.vector_to_host(psi)
    sec = hxv.HxvSector.from_model(m, N + 1, N)
    w1, U1 = np.linalg.eigh(OracleSector(m, N + 1, N).dense())
    (v0, n20), (v1, _) = gs.apply_ladder(sec, 0, 0, True, psi), gs.apply_ladder(sec, 1, 0, True, psi)
    ref = [_apply_op(psi_h, gs.maps(), sec.maps(), i, 0, True) for i in (0, 1)]
    ref[1] = 1j * ref[1]
    a, b, ov, n = sec.lanczos_tridiag_probes(v0, [v0, 1j * v1], min(sec.Dim, 200))
    assert sec.get_option("lanczos_real_last") == 0               # one probe with an imaginary part: the complex kernels
    poles, wts = greens.poles_weights(a[:n], b[:n], ov, np.sqrt(n20))
    G = greens.evaluate(poles, wts, 1j * WM, e0, 1.0)
    Gref = _lehmann(w1, U1, ref, e0, 1.0)[:, :, 0]
    assert np.abs(G - Gref).max() <= 1e-9, np.abs(G - Gref).max()
    a, b, ov, n = sec.lanczos_tridiag_probes(v0, [v0, v1], 8)
    assert sec.get_option("lanczos_real_last") == 1
    sec.close()
    gs.close()


# ---- 5. other handle kinds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["from_csr", "kanamori_nd_csr", "kanamori_fold_nd_0", "lanczos_fused_0", "kernel_0"])
def test_other_handle_kinds_give_the_default_handle_s_overlaps(built, kind):
    import hxv
    from hxv import greens, models
    from oracle.oracle import OracleSector

    if kind.startswith("kanamori"):
        m, (nup, ndw), real = models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15), (4, 4), False      # spH0nd folded into pass A by default
    else:
        m, (nup, ndw), real = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (4, 3), True
    ref = hxv.HxvSector.from_model(m, nup, ndw)
    if kind in ("from_csr", "kanamori_nd_csr"):
        o = OracleSector(m, nup, ndw)
        sec = hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag(), nd=o.csr("nd") if kind == "kanamori_nd_csr" else None)
    else:
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        name, value = {"kanamori_fold_nd_0": ("fold_nd", 0), "lanczos_fused_0": ("lanczos_fused", 0), "kernel_0": ("kernel", 0)}[kind]
        sec.set_option(name, value)
    rng = np.random.default_rng(8)
    # unit start vector and unit probes: the absolute 1e-11 is stated for probes of norm 1 (an overlap's error scales with its probe's norm)
    v = _rand(rng, ref.Dim, real)
    v /= np.linalg.norm(v)
    ps = [p / np.linalg.norm(p) for p in (_rand(rng, ref.Dim, real) for _ in range(3))]
    nl = 12                                                        # (the early steps: see the head of this file)
    out = []
    for s in (ref, sec):
        a, b, ov, n = s.lanczos_tridiag_probes(s.vector_from_host(v), [s.vector_from_host(p) for p in ps], nl)
        assert n == nl
        poles, wts = greens.poles_weights(a, b, ov, np.linalg.norm(v))
        out.append((a, b, ov, greens.evaluate(poles, wts, 1j * WM, 0.0, 1.0)))
    (a0, b0, ov0, G0), (a1, b1, ov1, G1) = out
    print(f"{kind}: max |d overlaps| = {np.abs(ov1 - ov0).max():.3e}, max |d G| = {np.abs(G1 - G0).max():.3e}, max |d alanc| = {np.abs(a1 - a0).max():.3e}")
    assert np.abs(ov1 - ov0).max() <= 1e-11, np.abs(ov1 - ov0).max()
    assert np.abs(G1 - G0).max() <= 1e-11, np.abs(G1 - G0).max()
    assert np.abs(a1 - a0).max() <= 1e-11
    ref.close()
    sec.close()


# ---- 6. device row order ----------------------------------------------------------------------------------------------------------------
def test_device_row_order_gives_the_reference_order_s_overlaps(built, monkeypatch):
    """The same run on the same sector with and without the device row order: another summation order in every product and every dot, so the
    two recurrences differ by roundings that grow with the step; 30 steps, 1e-12 absolute.  An overlap's absolute error is proportional to its
    probe's norm, so the absolute bound is stated for UNIT probes and a unit start vector -- the norms of the vectors this driver is for
    (|c^dagger_j|gs>|^2 is an occupation, at most 1)."""
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=2, Nbath=6)                         # Ns = 14, sector (7,7): DimUp = 3432 >= 2048
    rng = np.random.default_rng(21)
    out = []
    for order in ("1", "0"):
        monkeypatch.setenv("HXV_ROW_ORDER", order)
        hxv.sector_cache_clear()
        sec = hxv.HxvSector.from_model(m, 7, 7)
        assert sec.DimUp == 3432
        assert (sec.row_perm is not None) == (order == "1")
        if not out:
            v, ps = _rand(rng, sec.Dim, True), [_rand(rng, sec.Dim, True) for _ in range(2)]
            v, ps = v / np.linalg.norm(v), [p / np.linalg.norm(p) for p in ps]
        a, b, ov, n = sec.lanczos_tridiag_probes(sec.vector_from_host(v), [sec.vector_from_host(p) for p in ps], 30)
        assert n == 30
        out.append((a, ov))
        sec.close()
    hxv.sector_cache_clear()
    (a1, ov1), (a0, ov0) = out
    print(f"row order on / off, 30 steps: max |d overlaps| = {np.abs(ov1 - ov0).max():.3e} (max |overlap| {np.abs(ov0).max():.3e}), "
          f"max |d alanc| = {np.abs(a1 - a0).max():.3e} (max |alanc| {np.abs(a0).max():.3e})")
    assert np.abs(ov0).max() > 1e-5                                # (unit random vectors of Dim 1.2e7: overlaps of 3e-4, far above the bound)
    assert np.abs(ov1 - ov0).max() <= 1e-12, np.abs(ov1 - ov0).max()
    assert np.abs(a1 - a0).max() <= 1e-12, np.abs(a1 - a0).max()


# ---- 7. split sectors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["local", "rccl_double"])
def transport(request, built, monkeypatch):
    if request.param == "local":
        return "local"
    monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))
    return "rccl"


@pytest.mark.parametrize("name,nranks,exchange", [("chain", 2, "allgather"), ("chain", 3, "alltoall"), ("bhz", 3, "allgather"), ("bhz", 2, "alltoall")])
def test_split_sector_overlaps_equal_the_unsplit_ones(built, transport, name, nranks, exchange):
    import torch
    import hxv
    from hxv import models

    if name == "chain":
        m, (nup, ndw), real = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (3, 3), True      # DimDw = 20: uneven for 3 ranks
    else:
        m, (nup, ndw), real = models.bhz_2d(Nbath=0), (4, 4), False
    ser = hxv.HxvSector.from_model(m, nup, ndw)
    rng = np.random.default_rng(5)
    # unit start vector and unit probes: the absolute 1e-12 is stated for probes of norm 1 (an overlap's error scales with its probe's norm)
    v = _rand(rng, ser.Dim, real)
    v /= np.linalg.norm(v)
    ps = [p / np.linalg.norm(p) for p in (_rand(rng, ser.Dim, real) for _ in range(3))]
    nl = 12                                                        # (the early steps: see the head of this file)
    a0, b0, ov0, n0 = ser.lanczos_tridiag_probes(ser.vector_from_host(v), [ser.vector_from_host(p) for p in ps], nl)
    ser.close()
    hxv.set_exchange_default(exchange)

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        dv = sec.vector_from_host(v[lo:hi].copy())
        dps = [sec.vector_from_host(p[lo:hi].copy()) for p in ps]
        c0 = sec.get_option("allreduce_count")
        at, bt, nt = sec.lanczos_tridiag(dv, nl)
        c1 = sec.get_option("allreduce_count")
        a, b, ov, n = sec.lanczos_tridiag_probes(dv, dps, nl)
        c2 = sec.get_option("allreduce_count")
        was_real = sec.get_option("lanczos_real_last")
        a_none, b_none, _, n_none = sec.lanczos_tridiag_probes(dv, [], nl)
        c3 = sec.get_option("allreduce_count")
        refused = None
        if exchange == "allgather":
            # a start vector at hxv_slab_home is staged; a PROBE there is refused, by every rank together (nobody is left in a collective)
            home = sec.slab_home()
            home.copy_(dv)
            ah, bh, ovh, nh = sec.lanczos_tridiag_probes(home, dps, nl)
            assert nh == n and np.array_equal(ah, a) and np.array_equal(ovh, ov)
            home = sec.slab_home()
            with pytest.raises(hxv.HxvError) as ei:
                sec.lanczos_tridiag_probes(dv, [dps[0], home if r == 0 else dps[1]], nl)      # only rank 0's own argument is bad
            refused = str(ei.value)
        torch.cuda.synchronize()
        sec.close()
        return dict(a=a, b=b, ov=ov, n=n, at=at, bt=bt, nt=nt, real=was_real, extra=(c2 - c1) - (c1 - c0), none=(c3 - c2) - (c1 - c0),
                    a_none=a_none, refused=refused)

    try:
        res = hxv.run_ranks(nranks, rank, transport=transport)
    finally:
        hxv.set_exchange_default("allgather")
    print(f"{name} {nranks} ranks {exchange}: max |overlaps - unsplit| = {max(np.abs(o['ov'] - ov0).max() for o in res):.3e}")
    for o in res:
        assert o["n"] == o["nt"] == n0 == nl
        assert np.array_equal(o["a"], o["at"]) and np.array_equal(o["b"], o["bt"])     # bit-identical to hxv_lanczos_tridiag on the same split
        assert np.array_equal(o["a_none"], o["at"])
        assert np.array_equal(o["ov"], res[0]["ov"])                                    # identical on every rank
        assert np.abs(o["ov"] - ov0).max() <= 1e-12, np.abs(o["ov"] - ov0).max()
        assert o["real"] == (1 if real else 0)
        assert o["extra"] == nl, o["extra"]                                             # exactly ONE more all-reduce per step ...
        assert o["none"] == 0                                                           # ... and none without probes
        if exchange == "allgather":
            assert "gather buffer" in o["refused"] or "peer rank" in o["refused"]


# ---- 8. determinism and lifetime --------------------------------------------------------------------------------------------------------
def test_determinism_buffers_and_traffic(built):
    import hxv
    from hxv import models

    m = models.hm_1dchain(Nlat=2, Nbath=3)
    live0 = hxv.live_handles()
    sec = hxv.HxvSector.from_model(m, 4, 4)
    rng = np.random.default_rng(2)
    dv = sec.vector_from_host(_rand(rng, sec.Dim, True))
    dps = [sec.vector_from_host(_rand(rng, sec.Dim, True)) for _ in range(5)]
    first = sec.lanczos_tridiag_probes(dv, dps, 30)                # (lazy allocations of the handle happen here)
    assert sec.get_option("lanczos_real_last") == 1
    st0, pool0 = sec.stats(), hxv.pool_stats()
    again = sec.lanczos_tridiag_probes(dv, dps, 30)
    st1, pool1 = sec.stats(), hxv.pool_stats()
    for x, y in zip(first[:3], again[:3]):
        assert np.array_equal(x, y)                                # the same bits on every call
    assert (st1["h2d_bytes"], st1["d2h_bytes"]) == (st0["h2d_bytes"], st0["d2h_bytes"])     # no Dim-sized PCIe traffic
    # the five real-mode probe buffers came from the cache and went back to it
    assert pool1["hits"] >= pool0["hits"] + 5 and pool1["misses"] == pool0["misses"] and pool1["cached_bytes"] == pool0["cached_bytes"]
    assert st1["device_bytes"] == st0["device_bytes"]
    sec.close()
    assert hxv.live_handles() == live0


# ---- 9. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(built):
    import torch
    import hxv
    from hxv import models

    L = hxv.load_library()
    sec = hxv.HxvSector.from_model(models.plaquette_2x2_nobath(), 2, 2)
    dv = sec.vector_from_host(_rand(np.random.default_rng(1), sec.Dim, True))
    a, b, ov, n = np.zeros(4), np.zeros(4), np.zeros(2 * 4 * 9), C.c_int32()
    pd = C.POINTER(C.c_double)
    pa, pb, po = a.ctypes.data_as(pd), b.ctypes.data_as(pd), ov.ctypes.data_as(pd)
    one = (C.c_void_p * 1)(dv.data_ptr())
    nine = (C.c_void_p * 9)(*([dv.data_ptr()] * 9))
    hole = (C.c_void_p * 2)(dv.data_ptr(), None)
    h, v = sec._h, dv.data_ptr()
    bad = {
        "NULL handle": (None, v, 1, one, 4, pa, pb, po, 1e-12, C.byref(n)),
        "bad argument": (h, None, 1, one, 4, pa, pb, po, 1e-12, C.byref(n)),
        "bad argument ": (h, v, 1, one, 4, None, pb, po, 1e-12, C.byref(n)),
        "bad argument  ": (h, v, 1, one, 4, pa, None, po, 1e-12, C.byref(n)),
        "bad argument   ": (h, v, 1, one, 4, pa, pb, po, 1e-12, None),
        "nlanc < 1": (h, v, 1, one, 0, pa, pb, po, 1e-12, C.byref(n)),
        "nprobes must be": (h, v, 9, nine, 4, pa, pb, po, 1e-12, C.byref(n)),
        "nprobes must be ": (h, v, -1, one, 4, pa, pb, po, 1e-12, C.byref(n)),
        "needs the probe list": (h, v, 1, None, 4, pa, pb, po, 1e-12, C.byref(n)),
        "needs the probe list ": (h, v, 1, one, 4, pa, pb, None, 1e-12, C.byref(n)),
        "NULL entry": (h, v, 2, hole, 4, pa, pb, po, 1e-12, C.byref(n)),
    }
    for text, args in bad.items():
        assert L.hxv_lanczos_tridiag_probes(*args) == 1, text     # HXV_ERR_ARG
        msg = L.hxv_last_error().decode()
        assert "hxv_lanczos_tridiag_probes" in msg and text.strip() in msg, (text, msg)
    assert L.hxv_lanczos_tridiag_probes(h, v, 0, None, 4, pa, pb, None, 1e-12, C.byref(n)) == 0 and n.value == 4    # no probe: allowed
    # the Python form takes native device vectors only: no dispatch on the length
    with pytest.raises(hxv.HxvError, match="padded layout"):
        sec.lanczos_tridiag_probes(dv[:-1].contiguous(), [], 4)
    with pytest.raises(hxv.HxvError, match="padded layout"):
        sec.lanczos_tridiag_probes(dv, [torch.zeros(sec.Dim + 3, dtype=torch.complex128, device="cuda")], 4)
    with pytest.raises(hxv.HxvError, match="zero or not finite"):
        sec.lanczos_tridiag_probes(torch.zeros_like(dv), [], 4)
    sec.close()
