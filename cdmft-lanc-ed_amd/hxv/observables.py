"""Impurity observables and local energy from device-resident eigenstates (include/hxv.h, hxv_observables_*).

The reference's lanc_observables / lanc_local_energy / single-particle density matrix (ED_OBSERVABLES.f90:94-452, 609-686) in two steps:
HxvSector.observables_record turns each state of the state list into a small raw record on the device, summed with the reference's
weights; derive() turns the summed record into the named quantities (host code of the library, shared with the Fortran glue).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import HxvSector, _chk, _p, load_library

# derive(): name, shape (Fortran order), dtype -- in the order of hxv_observables_derive's output
_FIELDS = ["dens", "dens_up", "dens_dw", "docc", "magz", "sz2", "n2", "s2tot", "Eknot", "Epot", "Ehartree", "Dust", "Dund",
           "single_particle_density_matrix"]


def _shapes(model):
    L, O, S = model.Nlat, model.Norb, model.Nspin
    return {"dens": (L, O), "dens_up": (L, O), "dens_dw": (L, O), "docc": (L, O), "magz": (L, O), "sz2": (L, L, O, O), "n2": (L, L, O, O),
            "s2tot": (L,), "Eknot": (), "Epot": (), "Ehartree": (), "Dust": (), "Dund": (), "single_particle_density_matrix": (L, L, S, S, O, O)}


def record_elems(model) -> int:
    """Length of a raw record: 4^Nimp + 4 Nimp^2 doubles."""
    n = model.Nlat * model.Norb
    return 4 ** n + 4 * n * n


def derive(model, record: np.ndarray) -> dict:
    """The reference's named quantities from a (summed, weighted) record, with its names and array shapes (Fortran order).
    Epot includes Ehartree (ED_OBSERVABLES.f90:434).  Ehartree's constant term uses uloc(iorb), not the reference's uloc(is) (hxv.h)."""
    L = load_library()
    rec = np.ascontiguousarray(record, dtype=np.float64)
    assert rec.size == record_elems(model), (rec.size, record_elems(model))
    m, keep = HxvSector._model_struct(model)
    n = L.hxv_obs_derived_elems(C.byref(m))
    if n <= 0:
        raise ValueError("derive: unsupported model (Nimp <= 10, Norb <= 5)")
    out = np.zeros(n)
    _chk(L.hxv_observables_derive(C.byref(m), _p(rec, C.c_double), _p(out, C.c_double)), "hxv_observables_derive")
    del keep
    res, k = {}, 0
    for name, shape in _shapes(model).items():
        size = int(np.prod(shape)) if shape else 1
        if name == "single_particle_density_matrix":
            res[name] = out[k:k + 2 * size].view(np.complex128).reshape(shape, order="F").copy()
            k += 2 * size
        elif shape == ():
            res[name] = float(out[k])
            k += 1
        else:
            res[name] = out[k:k + size].reshape(shape, order="F").copy()
            k += size
    assert k == n
    return res


def thermal_weights(energies, beta: float | None = None) -> np.ndarray:
    """peso of every state (ED_DIAG.f90:357-366 zeta_function, ED_OBSERVABLES.f90:134-135): zero temperature (beta None) 1/size each;
    finite temperature exp(-beta (Ei - Egs)) / Z."""
    e = np.asarray(energies, dtype=np.float64)
    if beta is None:
        return np.full(e.size, 1.0 / e.size)
    b = np.exp(-float(beta) * (e - e.min()))
    return b / b.sum()


def observables(model, states, beta: float | None = None) -> dict:
    """The whole state list at once: states = [(sector, energy, device vector), ...] (sector: an open HxvSector, the vector in its padded
    layout).  Records summed with thermal_weights, then derive()."""
    w = thermal_weights([e for _, e, _ in states], beta)
    rec = np.zeros(record_elems(model))
    for (sec, _, psi), wi in zip(states, w):
        sec.observables_record(psi, weight=wi, out=rec, accumulate=True)
    return derive(model, rec)


def cluster_density_matrix(model, states, beta: float | None = None) -> np.ndarray:
    """The reference's cluster_density_matrix (dm_flag; density_matrix_impurity, ED_OBSERVABLES.f90:465-582) of the whole state list:
    rho_imp = sum_i peso_i Tr_bath |psi_i><psi_i|, complex (4^Nimp, 4^Nimp), element [io, jo] with io = a_up + 2^Nimp a_dw.  states and
    beta as in observables(); every state's matrix is computed on the device (HxvSector.cluster_dm) and summed on the host."""
    w = thermal_weights([e for _, e, _ in states], beta)
    n = 4 ** (model.Nlat * model.Norb)
    rho = np.zeros((n, n), dtype=np.complex128, order="F")
    for (sec, _, psi), wi in zip(states, w):
        sec.cluster_dm(psi, weight=wi, out=rho, accumulate=True)
    return rho


def reduced_density_matrix(model, states, orbital_mask, beta: float | None = None, fermi_sign: bool = False) -> np.ndarray:
    """The reference's ed_get_reduced_density_matrix_single (ED_IO/get_reduced_dm.f90:68-212) of the whole state list without the dense
    cluster matrix, so for any Nimp: rho_S = sum_i peso_i Tr_env |psi_i><psi_i|, S the impurity orbitals of `orbital_mask` (bit indices or a
    bool array (Nlat, Norb)), complex (4^Nred, 4^Nred).  fermi_sign=False gives the reference's numbers (a plain partial trace), True the
    matrix with the Jordan-Wigner sign; states and beta as in cluster_density_matrix()."""
    w = thermal_weights([e for _, e, _ in states], beta)
    rho = None
    for (sec, _, psi), wi in zip(states, w):
        rho = sec.reduced_dm(psi, orbital_mask, weight=wi, fermi_sign=fermi_sign, out=rho, accumulate=rho is not None)
    return rho
