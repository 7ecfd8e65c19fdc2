"""The Chebyshev drivers on the MI355X against dense algebra (include/hxv.h: hxv_chebyshev_moments, hxv_chebyshev_apply;
HxvSector.chebyshev_moments / chebyshev_apply; hxv/chebyshev.py).

H is the oracle's dense matrix of the sector, H = V diag(E) V^dagger.  Expected moments: sum_k <p|k><k|v> cos(n arccos x_k), x = (E - b)/a, in
long double; expected vectors: V f(E) V^dagger v.  v = c^dagger_0|gs>, p_j = c^dagger_j|gs> (spin up, j < 3), |gs> the ground state of the
sector with one up electron less, from the engine's own lanczos_eigh and apply_ladder.  The window is the exact spectrum widened by 5 %.

TOLERANCES are not constants.  Per sector the float64 numpy recurrence on the dense H is compared ON THE CPU with the closed form; the device
must meet the closed form within 10 x that deviation (it adds the same terms in another order), with a floor of 1e-13 |p||v| for the moments
and 1e-13 |v| max|f| for f(H)v.  Every measured deviation is printed.  The doubled self-moments 2<t|t> - mu_0, 2 Re<t'|t> - mu_1 are
measured on the CPU through the same doubling formulas, so the same rule holds for them unchanged: 10 x that deviation, floor 1e-13 |v|^2;
the identities between device numbers (self-moments against the moments of v as its own probe, <t_n|t_n> = (mu_2n + mu_0)/2) and the norm
of e^{-iHt}v against |v| are held to those same tolerances, with no further factor.
The sector with DimUp = 3432 (Ns = 14, (7,1), Dim 48048) has no dense matrix here: there the expectation is the same float64 recurrence
through the oracle's own product -- two float64 evaluations of the same terms -- and the tolerance is the rule's floor alone:
1e-13 |p||v| for the moments, 1e-13 |v|^2 for the self-moments, 1e-13 |v| max|coef| for the vectors.
SPLIT RUN (3 thread ranks, DimDw = 20: 7 + 7 + 6 columns): compared with the unsplit run at the sector's own tolerance; the sums are added
in another order.  The test prints whether d_out is bit-identical to the unsplit one and asserts only the tolerance: on this sector it IS
bit-identical (the step is elementwise and the split product gives the unsplit product's bits here), the moments differ by 5.6e-17.
Measured on an MI355X: CPU recurrence against the closed form 1e-15 .. 5.3e-15 for the moments (the device the same to two digits), see
LABNOTES "Chebyshev recurrence".  Wall time of the file there: 12 tests in 5 s, 2.3 s of it the dense eigendecomposition of the Ns = 8
sector (Dim 4900)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMOM = 24
TAU, TIME = 2.0, 3.0       # e^{-tau H} (tau = beta/2 at beta = 4) and e^{-i H t}
LD = np.longdouble


def _model(name):
    from hxv import models

    return {
        "chain6_33": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), 3, 3),
        "from_csr": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), 3, 3),
        "square8_44": (models.hm_2dsquare(Nbath=1), 4, 4),
        "bhz_complex_22": (models.bhz_2d(Nbath=0), 2, 2),
        "jxjp_nd_22": (models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15), 2, 2),
        "pads_43": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), 4, 3),
        "thin_dw_71": (models.hm_1dchain(Nlat=2, Nbath=6), 7, 1),
    }[name]


def _open(name):
    import hxv
    from oracle.oracle import OracleSector

    m, nup, ndw = _model(name)
    if name == "from_csr":
        o = OracleSector(m, nup, ndw)
        return hxv.HxvSector.from_csr(o.DimUp, o.DimDw, o.csr("up"), o.csr("dw"), o.diag())
    return hxv.HxvSector.from_model(m, nup, ndw)


_cache = {}


def _reference(name):
    """host side of a sector, built once: v, probes (reference layout), the product, the eigendecomposition and the window"""
    if name in _cache:
        return _cache[name]
    import hxv
    from oracle.oracle import OracleSector

    m, nup, ndw = _model(name)
    gs = hxv.HxvSector.from_model(m, nup - 1, ndw)
    to = hxv.HxvSector.from_model(m, nup, ndw)
    _, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)
    vecs = [to.vector_to_host(gs.apply_ladder(to, j, 0, True, psi)[0]) for j in range(3)]
    gs.close()
    orc = OracleSector(m, nup, ndw)
    ref = dict(v=vecs[0], probes=vecs)
    if name == "thin_dw_71":
        ref["matvec"] = orc.spMatVec_main
        a, b = hxv.chebyshev.spectral_window(to, nlanc=80, margin=0.05)
        ref.update(a=a, b=b, E=None)
    else:
        H = orc.dense()
        E, V = np.linalg.eigh(H.real if not H.imag.any() else H)
        ref.update(H=H, E=E, V=V.astype(np.complex128), matvec=lambda x: H @ x)
        ref.update(a=0.5 * (E[-1] - E[0]) * 1.05, b=0.5 * (E[-1] + E[0]))
    to.close()
    _cache[name] = ref
    return ref


def _numpy_recurrence(ref, norder, coef=None):
    """float64: moments[n, j], <t_n|t_n>, Re<t_n|t_{n-1}> and sum_n coef_n t_n"""
    a, b, v, mv = ref["a"], ref["b"], ref["v"], ref["matvec"]
    P = np.array(ref["probes"]).conj()
    mom, tt, tc = np.zeros((norder, len(P)), dtype=complex), np.zeros(norder), np.zeros(norder)
    t0, t1 = None, v.copy()
    out = np.zeros_like(v) if coef is not None else None
    for n in range(norder):
        if n == 1:
            t0, t1 = t1, (mv(t1) - b * t1) / a
        elif n > 1:
            t0, t1 = t1, 2.0 * (mv(t1) - b * t1) / a - t0
        mom[n], tt[n] = P @ t1, np.vdot(t1, t1).real
        tc[n] = np.vdot(t1, t0).real if n else 0.0
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
    """sum_k <p|k><k|v> cos(n arccos x_k) in long double"""
    x = ((ref["E"].astype(LD) - LD(ref["b"])) / LD(ref["a"]))
    th = np.arccos(x)
    w = (ref["V"].conj().T @ ref["v"]) * (ref["V"].conj().T @ p).conj()
    wr, wi = w.real.astype(LD), w.imag.astype(LD)
    c = np.cos(np.outer(np.arange(norder).astype(LD), th))
    return np.asarray(c @ wr, dtype=np.float64) + 1j * np.asarray(c @ wi, dtype=np.float64)


def _f_of_h(ref, f):
    return ref["V"] @ (f(ref["E"]) * (ref["V"].conj().T @ ref["v"]))


SECTORS = ["chain6_33", "square8_44", "bhz_complex_22", "jxjp_nd_22", "from_csr", "pads_43", "thin_dw_71"]


@pytest.mark.parametrize("name", SECTORS)
def test_moments_and_functions_of_h_against_dense_algebra(built, name):
    import torch
    from hxv import chebyshev as ch

    ref = _reference(name)
    a, b, v, probes = ref["a"], ref["b"], ref["v"], ref["probes"]
    sec = _open(name)
    if name == "pads_43":
        assert sec.DimUp % 8 != 0
    if name == "thin_dw_71":
        assert sec.DimUp >= 2048 and sec.row_perm is not None
    dv, dps = sec.vector_from_host(v), [sec.vector_from_host(p) for p in probes]
    keep = dv.clone()
    nv, npmax = np.linalg.norm(v), max(np.linalg.norm(p) for p in probes)
    dense = ref["E"] is not None

    # ---- what the CPU recurrence itself deviates by -> the tolerances
    mom_np, tt_np, tc_np, _ = _numpy_recurrence(ref, 2 * NMOM - 1 if dense else NMOM)
    if dense:
        closed = np.stack([_closed_moments(ref, p, 2 * NMOM - 1) for p in probes], axis=1)
        dev = np.abs(mom_np[:NMOM] - closed[:NMOM]).max()
        dev_self = np.abs(_self_from(tt_np[:NMOM], tc_np[:NMOM]) - closed[:, 0].real).max()
        tol, expect = max(10 * dev, 1e-13 * npmax * nv), closed[:NMOM]
        tol_self = max(10 * dev_self, 1e-13 * nv * nv)
        expect_self = closed[:, 0].real
    else:
        dev = dev_self = float("nan")
        tol, tol_self = 1e-13 * npmax * nv, 1e-13 * nv * nv
        expect, expect_self = mom_np, _self_from(tt_np, tc_np)

    # ---- moments with three probes and with none; self-moments
    mom, smom = sec.chebyshev_moments(dv, dps, NMOM, a, b)
    mom0, smom0 = sec.chebyshev_moments(dv, [], NMOM, a, b)
    assert mom.shape == (NMOM, 3) and mom0.shape == (NMOM, 0) and smom.shape == (2 * NMOM - 1,)
    assert np.array_equal(smom, smom0)                     # the self-overlaps do not depend on the probes
    err, err_self = np.abs(mom - expect).max(), np.abs(smom - expect_self).max()
    print(f"{name}: Dim {sec.Dim}, window a = {a:.4f} b = {b:.4f}; CPU recurrence vs closed form {dev:.3e} (self {dev_self:.3e}); "
          f"device vs expectation {err:.3e} (tol {tol:.3e}), self-moments {err_self:.3e} (tol {tol_self:.3e})")
    assert err <= tol and err_self <= tol_self
    # self-moments against the moments of the run with v as its own probe (p_0 = c^dagger_0|gs> = v)
    assert np.abs(smom[:NMOM] - mom[:, 0].real).max() <= tol_self and np.abs(mom[:, 0].imag).max() <= tol
    assert torch.equal(dv, keep)                           # d_vin bit-identical

    # ---- apply with the coefficients of a single T_n is the moments' own t_n
    for n in (0, 1, NMOM - 1):
        e = np.zeros(n + 1, dtype=complex)
        e[n] = 1.0
        tn, n2 = sec.chebyshev_apply(dv, e, a, b)
        ov = np.array([torch.vdot(p, tn).item() for p in dps])
        assert np.abs(ov - mom[n]).max() <= tol, (n, np.abs(ov - mom[n]).max())
        assert abs(n2 - 0.5 * (smom[2 * n] + smom[0])) <= tol_self, n     # <t_n|t_n> = (mu_2n + mu_0) / 2
    assert torch.equal(dv, keep)

    # ---- e^{-tau H} v and e^{-iHt} v
    for what, coef, f in (("exp(-tau H)", ch.exp_coefficients(TAU, a, b), lambda E: np.exp(-TAU * E)),
                          ("exp(-iHt)", ch.propagator_coefficients(TIME, a, b), lambda E: np.exp(-1j * TIME * E))):
        out, n2 = sec.chebyshev_apply(dv, coef, a, b)
        got = sec.vector_to_host(out)
        _, _, _, out_np = _numpy_recurrence(ref, len(coef), coef)
        if dense:
            exact = _f_of_h(ref, f)
            fmax = np.abs(f(ref["E"])).max()
            devv = np.abs(out_np - exact).max()
            tolv = max(10 * devv, 1e-13 * nv * fmax)
        else:
            exact, devv = out_np, float("nan")
            tolv = 1e-13 * nv * np.abs(coef).max()
        errv = np.abs(got - exact).max()
        print(f"{name} {what}: {len(coef)} coefficients; CPU recurrence vs V f(E) V^+ v {devv:.3e}; device {errv:.3e} (tol {tolv:.3e})")
        assert errv <= tolv
        assert abs(n2 - np.vdot(got, got).real) <= 1e-13 * max(n2, 1e-300) * 8
        if what == "exp(-iHt)":                               # norm conservation, to the same tolerance
            print(f"{name} {what}: | |out| - |v| | = {abs(np.sqrt(n2) - nv):.3e} (tol {tolv:.3e})")
            assert abs(np.sqrt(n2) - nv) <= tolv, abs(np.sqrt(n2) - nv)
    assert torch.equal(dv, keep)
    sec.close()


def test_kpm_spectral_function_is_the_jackson_smoothed_lehmann_sum(built):
    """Ns = 6 chain: the reconstruction from the device's 47 self-moments against sum_k |<k|v>|^2 K_N(w, E_k), K_N the Jackson kernel of
    the same order -- an identity in the moments, so the bound is the moments' tolerance carried through the series:
    |dA| <= sum_n eps_n g_n |d mu_n| / (pi a sqrt(1 - x^2))."""
    from hxv import chebyshev as ch

    ref = _reference("chain6_33")
    a, b = ref["a"], ref["b"]
    sec = _open("chain6_33")
    _, smom = sec.chebyshev_moments(sec.vector_from_host(ref["v"]), [], NMOM, a, b)
    sec.close()
    N = 2 * NMOM - 1
    mom_np, tt_np, tc_np, _ = _numpy_recurrence(ref, N)
    closed = _closed_moments(ref, ref["v"], N).real
    nv2 = np.vdot(ref["v"], ref["v"]).real
    tol_mu = max(10 * np.abs(_self_from(tt_np[:NMOM], tc_np[:NMOM]) - closed).max(), 1e-13 * nv2)     # the self-moments' tolerance of the rule above
    x = np.linspace(-0.99, 0.99, 397)
    omega = a * x + b
    A = ch.spectral_function(smom, a, b, omega)
    w = np.abs(ref["V"].conj().T @ ref["v"]) ** 2
    g = ch.jackson(N)
    eps = np.where(np.arange(N) == 0, 1.0, 2.0)
    xk = (ref["E"] - b) / a
    K = (np.cos(np.outer(np.arccos(x), np.arange(N))) * (g * eps)) @ np.cos(np.outer(np.arange(N), np.arccos(xk)))   # [omega, k]
    lehmann = (K @ w) / (np.pi * a * np.sqrt(1 - x * x))
    bound = np.sum(g * eps) * tol_mu / (np.pi * a * np.sqrt(1 - x * x))
    print(f"KPM vs Jackson-smoothed Lehmann: max |dA| = {np.abs(A - lehmann).max():.3e}, max A = {A.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(np.abs(A - lehmann) <= bound)
    assert A.min() > -bound.max() and abs(np.sum(0.5 * (A[1:] + A[:-1]) * np.diff(omega)) - nv2) < 0.02 * nv2     # positive, and the weight is there


def test_split_sector_on_three_ranks(built):
    import torch
    import hxv
    from hxv import chebyshev as ch

    name = "chain6_33"
    ref = _reference(name)
    m, nup, ndw = _model(name)
    a, b, v, probes = ref["a"], ref["b"], ref["v"], ref["probes"]
    ser = _open(name)
    dv = ser.vector_from_host(v)
    mom0, smom0 = ser.chebyshev_moments(dv, [ser.vector_from_host(p) for p in probes], NMOM, a, b)
    coef = ch.propagator_coefficients(TIME, a, b)
    out0 = ser.vector_to_host(ser.chebyshev_apply(dv, coef, a, b)[0])
    # (the count of blocks out of the device's buffer cache is per DEVICE and the ranks run side by side: it is read here, with the unsplit
    #  handle still open, before the ranks start and after the last of them has closed its sector)
    live_before = ser.get_option("pool_live_blocks")
    mom_np, tt_np, tc_np, _ = _numpy_recurrence(ref, NMOM)
    closed = np.stack([_closed_moments(ref, p, NMOM) for p in probes], axis=1)
    nv, npmax = np.linalg.norm(v), max(np.linalg.norm(p) for p in probes)
    tol = max(10 * np.abs(mom_np - closed).max(), 1e-13 * npmax * nv)
    tol_self = max(10 * np.abs(_self_from(tt_np, tc_np) - _closed_moments(ref, v, 2 * NMOM - 1).real).max(), 1e-13 * nv * nv)

    def rank(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=3)
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        d = sec.vector_from_host(v[lo:hi].copy())
        keep = d.clone()
        dps = [sec.vector_from_host(p[lo:hi].copy()) for p in probes]
        c0 = sec.get_option("allreduce_count")
        mom, smom = sec.chebyshev_moments(d, dps, NMOM, a, b)
        c1 = sec.get_option("allreduce_count")
        out, n2 = sec.chebyshev_apply(d, coef, a, b)
        # a start vector at hxv_slab_home is staged; a probe there is refused by every rank together
        home = sec.slab_home()
        home.copy_(d)
        momh, _ = sec.chebyshev_moments(home, dps, NMOM, a, b)
        home = sec.slab_home()
        with pytest.raises(hxv.HxvError) as refused:
            sec.chebyshev_moments(d, [dps[0], home if r == 0 else dps[1]], NMOM, a, b)      # only rank 0's own argument is bad
        with pytest.raises(hxv.HxvError) as refused_out:
            sec.chebyshev_apply(d, coef, a, b, out=home if r == 1 else out)                 # only rank 1's
        # a window half as wide as the spectrum: every rank returns the guard's error, nobody is left waiting
        with pytest.raises(hxv.HxvError) as narrow:
            sec.chebyshev_moments(d, dps, NMOM, 0.5 * a, b)
        with pytest.raises(hxv.HxvError) as narrow_apply:
            sec.chebyshev_apply(d, coef, 0.5 * a, b)
        same = torch.equal(d, keep)
        res = dict(mom=mom, smom=smom, momh=momh, out=sec.vector_to_host(out), n2=n2, lo=lo, hi=hi, sizes=sec.vecDim, same=same,
                   reduces=c1 - c0, msgs=[str(e.value) for e in (refused, refused_out, narrow, narrow_apply)])
        torch.cuda.synchronize()
        sec.close()
        return res

    res = hxv.run_ranks(3, rank)
    del dv
    assert ser.get_option("pool_live_blocks") == live_before                    # normal and failing calls of three ranks: every block is back
    ser.close()
    assert len({o["sizes"] for o in res}) > 1                                   # an uneven split
    out = np.concatenate([o["out"] for o in res])
    print(f"3 ranks: max |moments - unsplit| = {max(np.abs(o['mom'] - mom0).max() for o in res):.3e} (tol {tol:.3e}), "
          f"max |out - unsplit| = {np.abs(out - out0).max():.3e}, out bit-identical to the unsplit run: {np.array_equal(out, out0)}")
    for o in res:
        assert np.array_equal(o["mom"], res[0]["mom"]) and np.array_equal(o["smom"], res[0]["smom"])      # identical on every rank
        assert np.array_equal(o["momh"], o["mom"])
        assert np.abs(o["mom"] - mom0).max() <= tol and np.abs(o["smom"] - smom0).max() <= tol_self
        assert o["reduces"] == NMOM, o["reduces"]                                # ONE all-reduce per order
        assert o["same"]
        assert o["n2"] == res[0]["n2"]
        for msg in o["msgs"][:2]:
            assert "gather buffer" in msg or "peer rank" in msg, msg
        for msg in o["msgs"][2:]:
            assert "outside the window" in msg, msg
    assert np.abs(out - out0).max() <= max(tol, 1e-13 * nv)


def test_error_paths_and_buffers(built):
    import torch
    import hxv

    ref = _reference("chain6_33")
    a, b = ref["a"], ref["b"]
    sec = _open("chain6_33")
    L = hxv.load_library()
    dv = sec.vector_from_host(ref["v"])
    dps = [sec.vector_from_host(p) for p in ref["probes"]]
    keep = dv.clone()
    out = torch.empty_like(dv)
    pd = C.POINTER(C.c_double)
    mom, smom = np.zeros(2 * 4 * 3), np.zeros(7)
    coef = np.array([1.0, 0.0, 0.5, 0.0])
    plist = (C.c_void_p * 3)(*[p.data_ptr() for p in dps])
    holed = (C.c_void_p * 3)(dps[0].data_ptr(), None, dps[2].data_ptr())
    many = (C.c_void_p * 9)(*[dps[0].data_ptr()] * 9)
    M = lambda *args: L.hxv_chebyshev_moments(*args)  # noqa: E731
    A = lambda *args: L.hxv_chebyshev_apply(*args)  # noqa: E731
    mp, sp, cp = mom.ctypes.data_as(pd), smom.ctypes.data_as(pd), coef.ctypes.data_as(pd)
    sec.apply_device_slab(dv)                                       # (the handle takes its product scratch from the cache at its first product, and keeps it)
    torch.cuda.synchronize()
    live0 = sec.get_option("pool_live_blocks")
    assert M(sec._h, dv.data_ptr(), 3, plist, 4, a, b, mp, sp) == 0
    assert M(sec._h, dv.data_ptr(), 3, plist, 4, a, b, mp, None) == 0          # self_moments may be NULL
    assert A(sec._h, dv.data_ptr(), 2, cp, a, b, out.data_ptr(), None) == 0    # norm2 may be NULL
    assert sec.get_option("pool_live_blocks") == live0
    inf, nan = float("inf"), float("nan")
    bad_coef = np.array([1.0, 0.0, nan, 0.0]).ctypes.data_as(pd)
    zero, notfinite = torch.zeros_like(dv), dv.clone()
    notfinite[3] = complex(nan, 0.0)
    bad_plist = (C.c_void_p * 3)(dps[0].data_ptr(), notfinite.data_ptr(), dps[2].data_ptr())
    torch.cuda.synchronize()
    bad_calls = {
        "NULL d_vin": lambda: M(sec._h, None, 3, plist, 4, a, b, mp, sp),
        "nmom < 1": lambda: M(sec._h, dv.data_ptr(), 3, plist, 0, a, b, mp, sp),
        "a = 0": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, 0.0, b, mp, sp),
        "a < 0": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, -a, b, mp, sp),
        "a inf": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, inf, b, mp, sp),
        "a nan": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, nan, b, mp, sp),
        "b nan": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, a, nan, mp, sp),
        "b inf": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, a, inf, mp, sp),
        "nprobes < 0": lambda: M(sec._h, dv.data_ptr(), -1, plist, 4, a, b, mp, sp),
        "nprobes > 8": lambda: M(sec._h, dv.data_ptr(), 9, many, 4, a, b, mp, sp),
        "NULL list": lambda: M(sec._h, dv.data_ptr(), 3, None, 4, a, b, mp, sp),
        "NULL entry": lambda: M(sec._h, dv.data_ptr(), 3, holed, 4, a, b, mp, sp),
        "NULL moments": lambda: M(sec._h, dv.data_ptr(), 3, plist, 4, a, b, None, sp),
        "zero vector": lambda: M(sec._h, zero.data_ptr(), 3, plist, 4, a, b, mp, sp),
        "non-finite vector": lambda: M(sec._h, notfinite.data_ptr(), 3, plist, 4, a, b, mp, sp),
        "non-finite probe, nmom = 1": lambda: M(sec._h, dv.data_ptr(), 3, bad_plist, 1, a, b, mp, sp),
        "non-finite probe": lambda: M(sec._h, dv.data_ptr(), 3, bad_plist, 4, a, b, mp, sp),
        "narrow window": lambda: M(sec._h, dv.data_ptr(), 3, plist, 24, 0.5 * a, b, np.zeros(2 * 24 * 3).ctypes.data_as(pd), None),
        "apply NULL d_vin": lambda: A(sec._h, None, 2, cp, a, b, out.data_ptr(), None),
        "apply NULL d_out": lambda: A(sec._h, dv.data_ptr(), 2, cp, a, b, None, None),
        "apply NULL coef": lambda: A(sec._h, dv.data_ptr(), 2, None, a, b, out.data_ptr(), None),
        "apply ncoef < 1": lambda: A(sec._h, dv.data_ptr(), 0, cp, a, b, out.data_ptr(), None),
        "apply out == in": lambda: A(sec._h, dv.data_ptr(), 2, cp, a, b, dv.data_ptr(), None),
        "apply a = 0": lambda: A(sec._h, dv.data_ptr(), 2, cp, 0.0, b, out.data_ptr(), None),
        "apply b nan": lambda: A(sec._h, dv.data_ptr(), 2, cp, a, nan, out.data_ptr(), None),
        "apply coef nan": lambda: A(sec._h, dv.data_ptr(), 2, bad_coef, a, b, out.data_ptr(), None),
        "apply zero vector": lambda: A(sec._h, zero.data_ptr(), 2, cp, a, b, out.data_ptr(), None),
        "apply narrow window": lambda: A(sec._h, dv.data_ptr(), 24, np.ones(48).ctypes.data_as(pd), 0.5 * a, b, out.data_ptr(), None),
    }
    for what, call in bad_calls.items():
        assert call() == 1, what                                   # HXV_ERR_ARG
        msg = L.hxv_last_error().decode()
        assert "hxv_chebyshev" in msg, (what, msg)
        if "narrow" in what:
            assert "outside the window" in msg
        assert sec.get_option("pool_live_blocks") == live0, what
    torch.cuda.synchronize()
    assert torch.equal(dv, keep)
    with pytest.raises(hxv.HxvError):
        sec.chebyshev_moments(dv[:-1], [], 4, a, b)
    sec.close()


def test_spectral_window_holds_the_spectrum(built):
    import hxv

    ref = _reference("chain6_33")
    sec = _open("chain6_33")
    a, b = hxv.chebyshev.spectral_window(sec)
    E = ref["E"]
    width = E[-1] - E[0]
    assert b - a < E[0] and E[-1] < b + a
    assert 2 * a < 1.06 * width                                    # 2 % per side on Ritz values that lie inside the spectrum
    # the guard is quiet with it
    sec.chebyshev_moments(sec.vector_from_host(ref["v"]), [], 64, a, b)
    sec.close()
