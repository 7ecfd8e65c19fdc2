"""The REAL-vector Chebyshev drivers and the seeded random device state on the MI355X (include/hxv.h: hxv_chebyshev_moments_real,
hxv_chebyshev_apply_real, hxv_vector_random; HxvSector.chebyshev_moments_real / chebyshev_apply_real / random_vector;
hxv.chebyshev.thermal_state), on the sectors and with the reference machinery of tests/test_gpu_chebyshev.py, restated here.

H is the oracle's dense matrix of the sector, H = V diag(E) V^T.  Expected moments: sum_k <p|k><k|v> cos(n arccos x_k), x = (E - b)/a, in long
double; expected vectors: V f(E) V^T v.  v = Re c^dagger_0|gs>, p_j = Re c^dagger_j|gs> (spin up, j < 3), |gs> the ground state of the sector
with one up electron less; the window is the exact spectrum widened by 5 %.
TOLERANCES: that file's own rule.  Per sector the float64 numpy recurrence on the dense H is compared on the CPU with the closed form; the
device must meet the closed form within 10 x that deviation, with floors 1e-13 |p||v| for the moments, 1e-13 |v|^2 for the self-moments and
1e-13 |v| max|f| for f(H) v.  The sector with DimUp = 3432 (Dim 48048, device row order) has no dense matrix: there the expectation is the
float64 recurrence through the oracle's product and the floors alone apply (1e-13 |v| max|coef| for the vectors).  The complex entries run
on the same vectors at the same tolerance; whether their d_out has the real entry's bits is printed, not asserted.
SPLIT RUN: 3 thread ranks on the Ns = 6 chain (DimDw = 20: 7 + 7 + 6 columns) against the unsplit real run at the sector's tolerance.
Every measured deviation is printed."""
import ctypes as C

import numpy as np
import pytest

import chebyshev_real_ref as R

pytestmark = pytest.mark.gpu

NMOM = 24
TAU = 2.0                  # e^{-tau H}: tau = beta/2 at beta = 4
SEED = 11
LD = np.longdouble
ERR_ARG, ERR_UNSUPPORTED = 1, 4


def _model(name):
    from hxv import models

    return {
        "chain6_33": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), 3, 3),
        "square8_44": (models.hm_2dsquare(Nbath=1), 4, 4),
        "bhz_complex_22": (models.bhz_2d(Nbath=0), 2, 2),
        "jxjp_nd_22": (models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15), 2, 2),
        "pads_43": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), 4, 3),
        "thin_dw_71": (models.hm_1dchain(Nlat=2, Nbath=6), 7, 1),
    }[name]


def _open(name):
    import hxv

    m, nup, ndw = _model(name)
    return hxv.HxvSector.from_model(m, nup, ndw)


_cache = {}


def _numpy_recurrence(ref, v, norder, coef=None):
    """float64: moments[n, j], <t_n|t_n>, <t_n|t_{n-1}> and sum_n coef_n t_n, from the real vector v"""
    a, b, mv = ref["a"], ref["b"], ref["matvec"]
    P = np.array(ref["probes"])
    mom, tt, tc = np.zeros((norder, len(P))), np.zeros(norder), np.zeros(norder)
    t0, t1 = None, v.copy()
    out = np.zeros_like(v) if coef is not None else None
    for n in range(norder):
        if n == 1:
            t0, t1 = t1, (mv(t1) - b * t1) / a
        elif n > 1:
            t0, t1 = t1, 2.0 * (mv(t1) - b * t1) / a - t0
        mom[n], tt[n] = P @ t1, t1 @ t1
        tc[n] = t1 @ t0 if n else 0.0
        if coef is not None:
            out += coef[n] * t1
    return mom, tt, tc, out


def _self_from(tt, tc):
    """the doubling formulas of include/hxv.h on host sums"""
    n = len(tt)
    mu = np.zeros(2 * n - 1)
    mu[0] = tt[0]
    for k in range(1, n):
        mu[2 * k - 1] = tc[1] if k == 1 else 2.0 * tc[k] - tc[1]
        mu[2 * k] = 2.0 * tt[k] - tt[0]
    return mu


def _closed_moments(ref, p, norder):
    """sum_k <p|k><k|v> cos(n arccos x_k) in long double (real H: real eigenvectors)"""
    th = np.arccos((ref["E"].astype(LD) - LD(ref["b"])) / LD(ref["a"]))
    w = ((ref["V"].T @ ref["v"]) * (ref["V"].T @ p)).astype(LD)
    return np.asarray(np.cos(np.outer(np.arange(norder).astype(LD), th)) @ w, dtype=np.float64)


def _reference(name):
    """host side of a sector, built ONCE and left unchanged: real v and probes (reference layout), the product, the eigendecomposition, the
    window, the random vector of SEED, the coefficient series of e^{-tau H}, and everything the float64 recurrence and the closed forms give"""
    if name in _cache:
        return _cache[name]
    import hxv
    from hxv import chebyshev as ch
    from oracle.oracle import OracleSector

    m, nup, ndw = _model(name)
    gs = hxv.HxvSector.from_model(m, nup - 1, ndw)
    to = hxv.HxvSector.from_model(m, nup, ndw)
    _, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)
    vecs = [np.ascontiguousarray(to.vector_to_host(gs.apply_ladder(to, j, 0, True, psi)[0]).real) for j in range(3)]
    gs.close()
    orc = OracleSector(m, nup, ndw)
    ref = dict(v=vecs[0], probes=vecs, r=np.ascontiguousarray(R.random_vector(SEED, to.Dim).real))
    dense = name != "thin_dw_71"
    if dense:
        H = orc.dense()
        assert not H.imag.any()
        H = np.ascontiguousarray(H.real)
        E, V = np.linalg.eigh(H)
        ref.update(E=E, V=V, matvec=lambda x: H @ x, a=0.5 * (E[-1] - E[0]) * 1.05, b=0.5 * (E[-1] + E[0]))
    else:
        a, b = ch.spectral_window(to, nlanc=80, margin=0.05)
        ref.update(E=None, matvec=lambda x: orc.spMatVec_main(x.astype(np.complex128)).real, a=a, b=b)
    to.close()
    a, b = ref["a"], ref["b"]
    coef = ch.exp_coefficients(TAU, a, b).real.copy()
    nv, npmax, nr = np.linalg.norm(vecs[0]), max(np.linalg.norm(p) for p in vecs), np.linalg.norm(ref["r"])
    mom_np, tt_np, tc_np, out_np = _numpy_recurrence(ref, vecs[0], max(NMOM, len(coef)), np.concatenate([coef, np.zeros(max(NMOM - len(coef), 0))]))
    _, _, _, th_np = _numpy_recurrence(ref, ref["r"], len(coef), coef)
    mom_np, self_np = mom_np[:NMOM], _self_from(tt_np[:NMOM], tc_np[:NMOM])
    if dense:
        closed = np.stack([_closed_moments(ref, p, 2 * NMOM - 1) for p in vecs], axis=1)
        f = np.exp(-TAU * E)
        exact, exact_th = V @ (f * (V.T @ vecs[0])), V @ (f * (V.T @ ref["r"]))
        ref.update(dev=np.abs(mom_np - closed[:NMOM]).max(), dev_self=np.abs(self_np - closed[:, 0]).max(), dev_v=np.abs(out_np - exact).max(),
                   dev_th=np.abs(th_np - exact_th).max(), expect=closed[:NMOM], expect_self=closed[:, 0], exact=exact, exact_th=exact_th)
        ref.update(tol=max(10 * ref["dev"], 1e-13 * npmax * nv), tol_self=max(10 * ref["dev_self"], 1e-13 * nv * nv),
                   tol_v=max(10 * ref["dev_v"], 1e-13 * nv * f.max()), tol_th=max(10 * ref["dev_th"], 1e-13 * nr * f.max()))
    else:
        nan = float("nan")
        ref.update(dev=nan, dev_self=nan, dev_v=nan, dev_th=nan, expect=mom_np, expect_self=self_np, exact=out_np, exact_th=th_np,
                   tol=1e-13 * npmax * nv, tol_self=1e-13 * nv * nv, tol_v=1e-13 * nv * np.abs(coef).max(), tol_th=1e-13 * nr * np.abs(coef).max())
    ref.update(coef=coef)
    _cache[name] = ref
    return ref


def _cplx(x):
    return np.ascontiguousarray(x, dtype=np.complex128)


SECTORS = ["chain6_33", "pads_43", "square8_44", "thin_dw_71"]
SHAPES = {"chain6_33": (20, 12), "pads_43": (15, 1), "square8_44": (70, 10), "thin_dw_71": (3432, 8)}     # DimUp, real pad rows


@pytest.mark.parametrize("name", SECTORS)
def test_real_entries_against_dense_algebra(built, name):
    import torch
    from hxv import chebyshev as ch

    ref = _reference(name)
    a, b, coef = ref["a"], ref["b"], ref["coef"]
    sec = _open(name)
    assert sec.real_vectors_available
    assert (sec.DimUp, -sec.DimUp % 16) == SHAPES[name]
    if name == "thin_dw_71":
        assert sec.row_perm is not None
    dv, dps = sec.vector_from_host(_cplx(ref["v"])), [sec.vector_from_host(_cplx(p)) for p in ref["probes"]]
    keep, keeps = dv.clone(), [p.clone() for p in dps]
    sec.chebyshev_moments_real(dv, dps[:1], 2, a, b)        # (the handle takes its product scratch from the cache at its first product, and keeps it)
    live0 = sec.get_option("pool_live_blocks")

    # ---- moments with three probes and with none; self-moments; the complex entry on the same vectors
    mom, smom = sec.chebyshev_moments_real(dv, dps, NMOM, a, b)
    assert sec.get_option("pool_live_blocks") == live0
    mom0, smom0 = sec.chebyshev_moments_real(dv, [], NMOM, a, b)
    assert sec.get_option("pool_live_blocks") == live0
    assert mom.shape == (NMOM, 3) and mom.dtype == np.float64 and mom0.shape == (NMOM, 0) and smom.shape == (2 * NMOM - 1,) and smom.dtype == np.float64
    assert np.array_equal(smom, smom0)
    momc, smomc = sec.chebyshev_moments(dv, dps, NMOM, a, b)
    err, err_self = np.abs(mom - ref["expect"]).max(), np.abs(smom - ref["expect_self"]).max()
    errc, errc_self = np.abs(momc - ref["expect"]).max(), np.abs(smomc - ref["expect_self"]).max()
    print(f"{name}: Dim {sec.Dim}, window a = {a:.4f} b = {b:.4f}; CPU recurrence vs closed form {ref['dev']:.3e} (self {ref['dev_self']:.3e}); real "
          f"entry vs expectation {err:.3e} (tol {ref['tol']:.3e}), self-moments {err_self:.3e} (tol {ref['tol_self']:.3e}); complex entry {errc:.3e}, "
          f"{errc_self:.3e}; real moments bit-identical to the complex entry's real parts: {np.array_equal(mom, momc.real)}")
    assert err <= ref["tol"] and err_self <= ref["tol_self"] and errc <= ref["tol"] and errc_self <= ref["tol_self"]
    assert np.abs(smom[:NMOM] - mom[:, 0]).max() <= ref["tol_self"]        # v is its own first probe

    # ---- e^{-tau H} v
    out, n2 = sec.chebyshev_apply_real(dv, coef, a, b)
    assert sec.get_option("pool_live_blocks") == live0
    assert not torch.any(out.imag != 0.0)                                     # Im(out) == 0 exactly
    pads = out.cpu().numpy().reshape(-1, sec.pitch)[:, sec.DimUp:]
    assert R.same_bits(pads, np.zeros_like(pads))
    outc, n2c = sec.chebyshev_apply(dv, coef.astype(np.complex128), a, b)
    got, gotc = sec.vector_to_host(out), sec.vector_to_host(outc)
    errv, errvc = np.abs(got - ref["exact"]).max(), np.abs(gotc - ref["exact"]).max()
    print(f"{name} exp(-tau H): {len(coef)} coefficients; CPU recurrence vs V f(E) V^T v {ref['dev_v']:.3e}; real entry {errv:.3e}, complex entry "
          f"{errvc:.3e} (tol {ref['tol_v']:.3e}); out bit-identical to the complex entry's: {torch.equal(out, outc)}")
    assert errv <= ref["tol_v"] and errvc <= ref["tol_v"]
    assert abs(n2 - np.vdot(got, got).real) <= 1e-13 * max(n2, 1e-300) * 8 and abs(n2c - n2) <= 1e-13 * n2 * 8
    # complex coefficients without an imaginary part are taken, others are refused
    out2, _ = sec.chebyshev_apply_real(dv, coef.astype(np.complex128), a, b)
    assert torch.equal(out2, out)
    import hxv

    with pytest.raises(hxv.HxvError, match="real coefficients"):
        sec.chebyshev_apply_real(dv, coef + 1e-300j, a, b)

    # ---- the thermal typical state of one seed: random_vector + exp_coefficients(beta/2) + apply, all on the device
    th, n2t = ch.thermal_state(sec, 2 * TAU, a, b, SEED)
    assert sec.get_option("pool_live_blocks") == live0
    gott = sec.vector_to_host(th)
    errt = np.abs(gott - ref["exact_th"]).max()
    thc, _ = ch.thermal_state(sec, 2 * TAU, a, b, SEED, real=False)           # (a complex random state: another vector, only its norm is looked at)
    print(f"{name} thermal state, seed {SEED}: CPU recurrence vs closed form {ref['dev_th']:.3e}; device {errt:.3e} (tol {ref['tol_th']:.3e})")
    assert errt <= ref["tol_th"] and not torch.any(th.imag != 0.0) and torch.any(thc.imag != 0.0)
    assert abs(n2t - np.vdot(gott, gott).real) <= 1e-13 * n2t * 8
    assert torch.equal(dv, keep) and all(torch.equal(p, k) for p, k in zip(dps, keeps))      # d_vin and the probes keep their bits
    sec.close()


def test_refusals(built):
    import torch
    import hxv
    from hxv import chebyshev as ch

    L = hxv.load_library()
    pd = C.POINTER(C.c_double)
    # ---- no real vectors on these sectors: HXV_ERR_UNSUPPORTED with the blocker's text
    # (the Jx/Jp sector of the BHZ model has complex amplitudes too, and that blocker is named first)
    for name, why in (("bhz_complex_22", "complex amplitudes"), ("jxjp_nd_22", "complex amplitudes")):
        sec = _open(name)
        assert not sec.real_vectors_available
        d, out = sec.random_vector(3), torch.zeros(sec.localElems, dtype=torch.complex128, device="cuda")
        live0 = sec.get_option("pool_live_blocks")
        smom, cf = np.zeros(7), np.array([1.0, 0.5])
        torch.cuda.synchronize()
        assert L.hxv_chebyshev_moments_real(sec._h, d.data_ptr(), 0, None, 4, 10.0, 0.0, None, smom.ctypes.data_as(pd)) == ERR_UNSUPPORTED
        assert "real vectors unavailable" in L.hxv_last_error().decode() and why in L.hxv_last_error().decode()
        assert L.hxv_chebyshev_apply_real(sec._h, d.data_ptr(), 2, cf.ctypes.data_as(pd), 10.0, 0.0, out.data_ptr(), None) == ERR_UNSUPPORTED
        assert "real vectors unavailable" in L.hxv_last_error().decode() and why in L.hxv_last_error().decode()
        assert sec.get_option("pool_live_blocks") == live0 and not torch.any(out != 0)
        with pytest.raises(hxv.HxvError):
            ch.thermal_state(sec, 1.0, 10.0, 0.0, 1, real=True)
        sec.close()

    ref = _reference("chain6_33")
    a, b, coef = ref["a"], ref["b"], ref["coef"]
    sec = _open("chain6_33")
    dv, dps = sec.vector_from_host(_cplx(ref["v"])), [sec.vector_from_host(_cplx(p)) for p in ref["probes"]]
    mom_ok, smom_ok = sec.chebyshev_moments_real(dv, dps, 4, a, b)
    out_ok, _ = sec.chebyshev_apply_real(dv, coef, a, b)
    live0 = sec.get_option("pool_live_blocks")
    plist = (C.c_void_p * 3)(*[p.data_ptr() for p in dps])
    mom, smom = np.zeros(4 * 3), np.zeros(7)
    mp, sp, cp = mom.ctypes.data_as(pd), smom.ctypes.data_as(pd), coef.ctypes.data_as(pd)
    sentinel = torch.full_like(dv, complex(-7.25, 3.5))
    out = sentinel.clone()
    tiny_v, tiny_p = dv.clone(), dps[1].clone()
    tiny_v[sec.DimUp - 1] += 1e-300j                         # one imaginary element whose square is zero
    tiny_p[5] += 1e-300j
    tiny_list = (C.c_void_p * 3)(dps[0].data_ptr(), tiny_p.data_ptr(), dps[2].data_ptr())
    zero, wide = torch.zeros_like(dv), np.zeros(NMOM * 3)
    torch.cuda.synchronize()
    M = lambda *args: L.hxv_chebyshev_moments_real(*args)  # noqa: E731
    A = lambda *args: L.hxv_chebyshev_apply_real(*args)  # noqa: E731
    bad = {
        "imaginary start vector": (lambda: M(sec._h, tiny_v.data_ptr(), 3, plist, 4, a, b, mp, sp), "imaginary"),
        "imaginary probe": (lambda: M(sec._h, dv.data_ptr(), 3, tiny_list, 4, a, b, mp, sp), "imaginary"),
        "apply imaginary start vector": (lambda: A(sec._h, tiny_v.data_ptr(), len(coef), cp, a, b, out.data_ptr(), None), "imaginary"),
        "narrow window": (lambda: M(sec._h, dv.data_ptr(), 3, plist, NMOM, 0.5 * a, b, wide.ctypes.data_as(pd), None), "outside the window"),
        "apply narrow window": (lambda: A(sec._h, dv.data_ptr(), NMOM, np.ones(NMOM).ctypes.data_as(pd), 0.5 * a, b, out.data_ptr(), None), "outside the window"),
        "apply out == in": (lambda: A(sec._h, dv.data_ptr(), len(coef), cp, a, b, dv.data_ptr(), None), "must not be d_vin"),
        "apply coef nan": (lambda: A(sec._h, dv.data_ptr(), 2, np.array([1.0, float("nan")]).ctypes.data_as(pd), a, b, out.data_ptr(), None), "not finite"),
        "zero vector": (lambda: M(sec._h, zero.data_ptr(), 3, plist, 4, a, b, mp, sp), "zero or not finite"),
        "nprobes > 8": (lambda: M(sec._h, dv.data_ptr(), 9, plist, 4, a, b, mp, sp), "nprobes"),
        "a = 0": (lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, 0.0, b, mp, sp), "window"),
    }
    for what, (call, text) in bad.items():
        assert call() == ERR_ARG, what
        msg = L.hxv_last_error().decode()
        assert "hxv_chebyshev" in msg and "_real" in msg and text in msg, (what, msg)
        assert sec.get_option("pool_live_blocks") == live0, what
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), what                   # d_out is written only on success
    # option real_vectors = 0 does not gate the entries: the same bits
    sec.set_option("real_vectors", 0)
    mom2, smom2 = sec.chebyshev_moments_real(dv, dps, 4, a, b)
    out2, _ = sec.chebyshev_apply_real(dv, coef, a, b)
    assert np.array_equal(mom2, mom_ok) and np.array_equal(smom2, smom_ok) and torch.equal(out2, out_ok)
    assert sec.get_option("pool_live_blocks") == live0
    sec.close()


def test_split_sector_on_three_ranks(built):
    import torch
    import hxv

    name = "chain6_33"
    ref = _reference(name)
    m, nup, ndw = _model(name)
    a, b, coef, v, probes = ref["a"], ref["b"], ref["coef"], ref["v"], ref["probes"]
    ser = _open(name)
    dv = ser.vector_from_host(_cplx(v))
    mom0, smom0 = ser.chebyshev_moments_real(dv, [ser.vector_from_host(_cplx(p)) for p in probes], NMOM, a, b)
    out0 = ser.vector_to_host(ser.chebyshev_apply_real(dv, coef, a, b)[0])
    live_before = ser.get_option("pool_live_blocks")
    seeds = (0, 2**63 + 5)
    randoms = {(s, cv): R.random_vector(s, ser.Dim, cv) for s in seeds for cv in (False, True)}

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=3)
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        d = sec.vector_from_host(_cplx(v[lo:hi]))
        keep = d.clone()
        dps = [sec.vector_from_host(_cplx(p[lo:hi])) for p in probes]
        c0 = sec.get_option("allreduce_count")
        mom, smom = sec.chebyshev_moments_real(d, dps, NMOM, a, b)
        c1 = sec.get_option("allreduce_count")
        out, n2 = sec.chebyshev_apply_real(d, coef, a, b)
        imag_free = not bool(torch.any(out.imag != 0.0))
        # an imaginary element on ONE rank: every rank returns HXV_ERR_ARG, nobody is left waiting
        spoiled = d.clone()
        if r == 1:
            spoiled[2] += 1e-300j
        with pytest.raises(hxv.HxvError) as refused:
            sec.chebyshev_moments_real(spoiled, dps, NMOM, a, b)
        with pytest.raises(hxv.HxvError) as narrow:
            sec.chebyshev_apply_real(d, np.ones(NMOM), 0.5 * a, b)
        rnd = {k: np.array_equal(sec.vector_to_host(sec.random_vector(k[0], k[1])), w[lo:hi]) for k, w in randoms.items()}
        res = dict(mom=mom, smom=smom, out=sec.vector_to_host(out), n2=n2, sizes=sec.vecDim, same=torch.equal(d, keep), reduces=c1 - c0,
                   imag_free=imag_free, msgs=[str(refused.value), str(narrow.value)], rnd=rnd)
        torch.cuda.synchronize()
        sec.close()
        return res

    res = hxv.run_ranks(3, rank)
    del dv
    assert ser.get_option("pool_live_blocks") == live_before                    # normal and failing calls of three ranks: every block is back
    ser.close()
    assert sorted(o["sizes"] for o in res) == [6 * 20, 7 * 20, 7 * 20]           # 7 + 7 + 6 columns
    out = np.concatenate([o["out"] for o in res])
    nv = np.linalg.norm(v)
    print(f"3 ranks: max |moments - unsplit| = {max(np.abs(o['mom'] - mom0).max() for o in res):.3e} (tol {ref['tol']:.3e}), "
          f"max |out - unsplit| = {np.abs(out - out0).max():.3e}, out bit-identical to the unsplit run: {np.array_equal(out, out0)}")
    for o in res:
        assert np.array_equal(o["mom"], res[0]["mom"]) and np.array_equal(o["smom"], res[0]["smom"])      # identical on every rank
        assert np.abs(o["mom"] - mom0).max() <= ref["tol"] and np.abs(o["smom"] - smom0).max() <= ref["tol_self"]
        assert o["reduces"] == NMOM + 1, o["reduces"]                             # ONE all-reduce per order, and one for the sum of |Im|
        assert o["same"] and o["imag_free"] and o["n2"] == res[0]["n2"]
        assert "imaginary" in o["msgs"][0] and "outside the window" in o["msgs"][1], o["msgs"]
        assert all(o["rnd"].values()), o["rnd"]                                  # each rank's slab of the one global random vector
    assert np.abs(out - out0).max() <= max(ref["tol_v"], 1e-13 * nv)


@pytest.mark.parametrize("name", ["pads_43", "thin_dw_71"])
def test_random_vector_is_the_formula_on_the_reference_index(built, name):
    """vector_to_host of the device vector equals the numpy restatement of include/hxv.h's formula element for element (equal values: the
    signed rows of a device row order come back through a negation, which may turn the +0.0 of a real vector's imaginary part into -0.0),
    real and complex, two seeds; pads are zero and the imaginary part of a real-valued vector is +0.0 in the raw device buffer"""
    import torch

    sec = _open(name)
    if name == "thin_dw_71":
        assert sec.row_perm is not None
    for seed in (0, 2**63 + 5):
        for cv in (False, True):
            d = sec.random_vector(seed, cv)
            raw = d.cpu().numpy().reshape(-1, sec.pitch)
            assert R.same_bits(raw[:, sec.DimUp:], np.zeros_like(raw[:, sec.DimUp:]))
            if not cv:
                assert R.same_bits(raw.imag, np.zeros_like(raw.imag))
            got, want = sec.vector_to_host(d), R.random_vector(seed, sec.Dim, cv)
            assert np.array_equal(got, want), (seed, cv)
            if sec.row_perm is None:
                assert R.same_bits(got, want)
    # filling a given vector: every element is written
    d = torch.full((sec.localElems,), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    assert sec.random_vector(7, True, out=d) is d and np.array_equal(sec.vector_to_host(d), R.random_vector(7, sec.Dim, True))
    assert not torch.any(torch.isnan(d.real)) and not torch.any(torch.isnan(d.imag))
    sec.close()


def test_random_vector_on_a_csr_handle_is_the_model_handles(built):
    import hxv
    from oracle.oracle import OracleSector

    for name in ("chain6_33", "thin_dw_71"):
        m, nup, ndw = _model(name)
        o = OracleSector(m, nup, ndw)
        csr = hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag())
        mod = _open(name)
        for cv in (False, True):
            a, b = csr.vector_to_host(csr.random_vector(9, cv)), mod.vector_to_host(mod.random_vector(9, cv))
            assert np.array_equal(a, b) and np.array_equal(a, R.random_vector(9, mod.Dim, cv))
        csr.close()
        mod.close()
