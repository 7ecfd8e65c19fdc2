"""The bosonic pole sum without a GPU (hxv.greens.chi_evaluate): fed by a numpy recurrence on the oracle's dense matrix (chi_ref.py) and compared
with the dense Lehmann sum at 64 bosonic frequencies nu_n = 2 pi n / beta, beta = 50, nu_0 = 0 included.

  - chi_evaluate against the Lehmann sum                        1e-12 (the numpy route's own error is <= 5e-14 on these sectors; the margin
                                                                covers another tridiagonal QL)
  - the rounding ghosts of psi are there and are dropped        >= 1 Ritz value within the cutoff of E, dropped weight <= 1e-20
  - cutoff = 0 changes nothing at nu >= nu_1                     1e-12
"""
import numpy as np
import pytest

import chi_ref


def _case(name):
    from hxv import models

    if name == "chain":
        return models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), 3, 3
    return models.plaquette_2x2_nobath(U=4.0, t=1.0, hfmode=True), 2, 2


@pytest.fixture(scope="module", params=["chain", "plaquette"])
def stage(request, built):
    """the dense sector, its ground state, and per kind the fluctuation vectors, the Lehmann sum and the numpy recurrence of every column"""
    from oracle.oracle import OracleSector

    m, nup, ndw = _case(request.param)
    orc = OracleSector(m, nup, ndw)
    H = orc.dense()
    w, U = np.linalg.eigh(H)
    assert w[1] - w[0] > 1e-3                                    # non-degenerate ground state: no Curie term
    psi, nimp = U[:, 0], m.Nlat * m.Norb
    nl = min(200, H.shape[0])
    out = {}
    for kind in ("spin", "charge"):
        f = chi_ref.density_f(orc.map_up(), orc.map_dw(), chi_ref.spin_charge_coef(kind, nimp))
        vecs, mean, n2 = chi_ref.fluctuations(f, psi)
        runs = [chi_ref.lanczos(H, vecs[b], list(vecs), nl) if n2[b] >= 1e-24 else None for b in range(nimp)]
        out[kind] = dict(ref=chi_ref.lehmann_chi(w, U, 0, list(vecs), 1j * chi_ref.NU), runs=runs, n2=n2)
    return dict(name=request.param, e0=w[0], nimp=nimp, kinds=out)


@pytest.mark.parametrize("kind", ["spin", "charge"])
def test_chi_evaluate_matches_the_lehmann_sum_and_drops_the_ghosts(stage, kind):
    from hxv import greens

    k, e0, nimp = stage["kinds"][kind], stage["e0"], stage["nimp"]
    chi, chi0 = np.zeros_like(k["ref"]), np.zeros_like(k["ref"])
    dropped, ghosts, live = 0.0, 0, 0
    for b, run in enumerate(k["runs"]):
        if run is None:
            continue
        live += 1
        a, bl, ov = run
        poles, wts = greens.poles_weights(a, bl, ov, np.sqrt(k["n2"][b]))
        chi[:, :, b], d = greens.chi_evaluate(poles, wts, 1j * chi_ref.NU, e0)
        ghosts += int((np.abs(poles - e0) <= 1e-8).sum())
        dropped += d
        with np.errstate(all="ignore"):
            chi0[:, :, b], d0 = greens.chi_evaluate(poles, wts, 1j * chi_ref.NU, e0, cutoff=0.0)
        assert d0 <= d
    err, err0 = np.abs(chi - k["ref"]).max(), np.abs(chi0[1:] - k["ref"][1:]).max()
    print(f"{stage['name']} {kind}: max|chi| = {np.abs(k['ref']).max():.3e}, |chi - Lehmann| = {err:.3e}, cutoff 0 at nu >= nu_1: {err0:.3e}, "
          f"{ghosts} Ritz values within 1e-8 of E, dropped weight {dropped:.3e}")
    assert live > 0 and np.abs(k["ref"]).max() > 1e-3          # (there is a signal; the smallest is the plaquette charge, 0.05)
    assert err <= 1e-12, err
    assert ghosts >= 1 and dropped <= 1e-20, (ghosts, dropped)
    assert err0 <= 1e-12, err0


def test_chi_evaluate_is_the_formula(built):
    from hxv import greens

    poles = np.array([-1.0, -1.0 + 5e-9, 0.5, 2.0])
    w = np.array([[3e-25, 1e-25j], [1e-26, 0.0], [1.0 + 0.5j, 0.25], [0.3, -0.1j]])
    z = np.array([[0.0, 0.7j], [1.3j, 0.2 + 0.4j]])
    chi, dropped = greens.chi_evaluate(poles, w, z, -1.0)
    assert chi.shape == (2, 2, 2)
    ref = -sum(w[n] / (z[..., None] - (poles[n] + 1.0)) - w[n].conj() / (z[..., None] + (poles[n] + 1.0)) for n in (2, 3))
    assert np.abs(chi - ref).max() <= 1e-15
    assert abs(dropped - (3e-25 + 1e-25 + 1e-26)) <= 1e-37
    # the reference's Lehmann form for real weights at z = i nu:  sum_n W_n 2 e_n / (nu^2 + e_n^2)
    wr, nu = np.array([[0.4], [0.1]]), np.array([0.0, 0.3, 2.0])
    chi, _ = greens.chi_evaluate(np.array([0.5, 2.0]), wr, 1j * nu, 0.0)
    ref = sum(wr[n, 0] * 2 * e / (nu ** 2 + e ** 2) for n, e in enumerate((0.5, 2.0)))
    assert np.abs(chi[:, 0] - ref).max() <= 1e-15
    # a pole AT the cutoff is dropped, one just above is kept
    _, d = greens.chi_evaluate(np.array([1e-8, 2e-8]), np.array([[1.0], [2.0]]), np.array([1j]), 0.0)
    assert d == 1.0


def test_density_coefficients_and_the_symbol(built):
    import ctypes

    import hxv
    from hxv import observables

    assert "hxv_apply_density_ops" in hxv.EXPORTS and hasattr(ctypes.CDLL(str(hxv.LIB_PATH)), "hxv_apply_density_ops")
    assert np.array_equal(observables.density_coefficients("spin", 4), chi_ref.spin_charge_coef("spin", 4))
    assert np.array_equal(observables.density_coefficients("charge", 2), chi_ref.spin_charge_coef("charge", 2))
    with pytest.raises(hxv.HxvError):
        observables.density_coefficients("pair", 2)
    with pytest.raises(hxv.HxvError):
        observables.density_coefficients(np.zeros((2, 2, 3)), 4)
    # a NULL handle is refused before the device is touched
    assert hxv.load_library().hxv_apply_density_ops(None, 1, None, 1, None, None, None, None) == 1
