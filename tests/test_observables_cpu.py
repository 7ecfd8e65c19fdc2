"""hxv_observables_derive (host code of the library, no device) against the reference's loops restated literally (tests/observables_ref.py):
records built in numpy from oracle eigenvectors, reduced by the library, must give what the basis-state loops give."""
import numpy as np
import pytest

from observables_ref import literal, oracle_states, record_numpy

NAMES = ["dens", "dens_up", "dens_dw", "docc", "magz", "sz2", "n2", "s2tot", "Eknot", "Epot", "Ehartree", "Dust", "Dund",
         "single_particle_density_matrix"]


def _check(model, states, beta=None):
    from hxv import observables

    w = observables.thermal_weights([e for *_, e in states], beta)
    rec = sum(record_numpy(model, mu, md, v, wi) for (mu, md, v, _), wi in zip(states, w))
    got = observables.derive(model, rec)
    ref = literal(model, [(mu, md, v, wi) for (mu, md, v, _), wi in zip(states, w)])
    for k in NAMES:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.abs(g - r).max() < 1e-12, (k, np.abs(g - r).max())
    return got, ref


@pytest.mark.parametrize("hfmode", [True, False])
def test_chain_norb1(built, hfmode):
    from hxv import models

    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], hfmode=hfmode, xmu=0.1)
    got, _ = _check(m, oracle_states(m, [(3, 3)]))
    assert (got["Ehartree"] != 0.0) == hfmode


def test_two_orbitals_with_ust_and_jh(built):
    from hxv import models

    m = models.bhz_2d(Nx=1, Ny=1, Nbath=1, U=2.0, Ust=1.2, Jh=0.3)   # Nlat 1, Norb 2, Nspin 2, Ns 4
    got, _ = _check(m, oracle_states(m, [(2, 2), (2, 1)], nstates=2))
    assert got["Dust"] > 0 and got["Dund"] >= 0


def test_complex_bhz_two_sites(built):
    from hxv import models

    m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=1.5, Ust=0.5, Jh=0.1)   # Nlat 2, Norb 2, Nspin 2: Nimp 4, Ns 8, complex impHloc
    assert np.abs(m.impHloc.imag).max() > 0
    rng = np.random.default_rng(3)
    st = oracle_states(m, [(4, 4)])
    mu, md, v, e = st[0]
    x = rng.standard_normal(v.size) + 1j * rng.standard_normal(v.size)  # a complex state as well: R's imaginary parts are not zero
    st.append((mu, md, x / np.linalg.norm(x), e + 0.05))
    got, _ = _check(m, st, beta=10.0)
    assert np.abs(got["single_particle_density_matrix"].imag).max() > 1e-6


def test_plaquette_without_bath(built):
    from hxv import models

    m = models.plaquette_2x2_nobath(U=4.0, hfmode=True)   # Nimp = Ns = 4
    _check(m, oracle_states(m, [(2, 2)], nstates=3))


def test_finite_temperature_over_sectors(built):
    from hxv import models

    m = models.hm_1dchain(Nlat=2, Nbath=1, eps_bath=[0.2], hfmode=True)   # Ns = 4
    st = oracle_states(m, [(2, 2), (1, 2), (2, 1), (2, 3)], nstates=2)
    _check(m, st, beta=5.0)


def test_thermal_weights_follow_the_reference():
    from hxv import observables

    assert np.allclose(observables.thermal_weights([1.0, 2.0, 3.0]), 1 / 3)
    w = observables.thermal_weights([-1.0, -0.5], beta=2.0)
    assert np.allclose(w, np.exp([0.0, -1.0]) / (1 + np.exp(-1.0)))


def test_ehartree_constant_term_uses_uloc_of_the_orbital(built):
    """The one deliberate divergence (include/hxv.h): the reference's constant term 0.25*uloc(is), is = imp_state_index (ED_OBSERVABLES.f90:399),
    reads Uloc past Norb.  Chain of two sites, Norb = 1, Uloc = (2, 0, ...): the reference adds 0.25*(U(1) + U(2)) = 0.5 per unit weight, the
    engine 0.25*(U(1) + U(1)) = 1.0 -- a difference of exactly 0.5 for a normalised state list."""
    from hxv import models, observables

    m = models.hm_1dchain(Nlat=2, Nbath=1, eps_bath=[0.2], U=2.0, hfmode=True)
    st = oracle_states(m, [(2, 2)])
    rec = sum(record_numpy(m, mu, md, v, 1.0) for mu, md, v, _ in st)
    got = observables.derive(m, rec)
    ref = literal(m, [(mu, md, v, 1.0) for mu, md, v, _ in st])
    assert abs(got["Ehartree"] - ref["Ehartree"]) < 1e-12
    assert abs((got["Ehartree"] - ref["Ehartree_reference"]) - 0.5) < 1e-12


def test_record_sizes_and_errors(built):
    import ctypes as C

    import hxv
    from hxv import models, observables

    m = models.bhz_2d(Nx=2, Ny=1, Nbath=1)
    assert observables.record_elems(m) == 4 ** 4 + 4 * 16
    L = hxv.load_library()
    mm, keep = hxv.HxvSector._model_struct(m)
    assert L.hxv_obs_derived_elems(C.byref(mm)) == 5 * 4 + 2 * 16 + 2 + 5 + 2 * 4 * 4 * 4
    assert L.hxv_observables_derive(C.byref(mm), None, None) == 1                # HXV_ERR_ARG
    big = models.hm_1dchain(Nlat=11, Nbath=0)
    mb, keepb = hxv.HxvSector._model_struct(big)
    assert L.hxv_obs_derived_elems(C.byref(mb)) == 0                              # Nimp > 10
