"""Impurity observables and local energy from device-resident eigenstates (include/hxv.h, hxv_observables_*).

The reference's lanc_observables / lanc_local_energy / single-particle density matrix (ED_OBSERVABLES.f90:94-452, 609-686) in two steps:
HxvSector.observables_record turns each state of the state list into a small raw record on the device, summed with the reference's
weights; derive() turns the summed record into the named quantities (host code of the library, shared with the Fortran glue).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import HxvError, HxvSector, _chk, _p, load_library

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


def density_coefficients(kind, nimp: int) -> np.ndarray:
    """coef (nops, 2, Nimp) of HxvSector.apply_density_ops: "spin" = S^z of every impurity orbital (cu = +1/2, cd = -1/2 on orbital a),
    "charge" = n of every impurity orbital (cu = cd = 1); an array is taken as it is."""
    if isinstance(kind, str):
        if kind not in ("spin", "charge"):
            raise HxvError('susceptibility: kind is "spin", "charge" or a coefficient array (nops, 2, Nimp)')
        cf = np.zeros((nimp, 2, nimp))
        for a in range(nimp):
            cf[a, 0, a], cf[a, 1, a] = (0.5, -0.5) if kind == "spin" else (1.0, 1.0)
        return cf
    cf = np.ascontiguousarray(kind, dtype=np.float64)
    if cf.ndim != 3 or cf.shape[1] != 2 or cf.shape[2] != nimp:
        raise HxvError(f"susceptibility: a coefficient array has the shape (nops, 2, Nimp = {nimp})")
    return cf


def susceptibility(sec, psi, e_state: float, kind, z, nlanc: int = 200, cutoff: float = 1e-8, paired: bool = False):
    """chi_ab(z) = <<dO_a; dO_b>> of ONE device-resident eigenstate psi (energy e_state) of the open sector `sec`: the impurity spin
    ("spin": O_a = S^z_a) or charge ("charge": O_a = n_a) susceptibility between the impurity orbitals, or between the operators of an
    explicit coefficient array (nops, 2, Nimp); the reference's buildChi_impurity stage (ED_GREENS_FUNCTIONS.f90:68-106).  One
    apply_density_ops call builds every dO_a|psi>; column b is one lanczos_tridiag_probes run from dO_b|psi> with all dO_a|psi> as probes
    (a column whose start vector has norm2 < 1e-24 is zero and is skipped), then greens.poles_weights and greens.chi_evaluate.  Nothing
    Dim-sized crosses PCIe.  A thermal average is the caller's sum over the state list, sum_m peso_m chi^(m) (thermal_weights).
    paired=True (real H only: sec.real_vectors_available, HxvError otherwise): the columns that are not skipped are taken two at a time
    through lanczos_tridiag_pair_probes, one product per step for both; a column left without a partner runs singly.
    -> (chi[len(z), nops, nops] complex128, info = {"mean", "norm2", "nsteps", "dropped_weight"})."""
    from . import greens

    if not sec.nimp():
        raise HxvError("susceptibility needs a sector built from a model with Nimp <= 10")
    if paired and not sec.real_vectors_available:
        raise HxvError("susceptibility: paired=True needs a real Hamiltonian (real_vectors_available)")
    cf = density_coefficients(kind, sec.nimp())
    nops = cf.shape[0]
    if nops > 8:
        raise HxvError("susceptibility: at most 8 operators per call (HXV_MAX_DENSITY_OPS, HXV_MAX_PROBES)")
    z = np.asarray(z, dtype=np.complex128).reshape(-1)
    vecs, mean, norm2 = sec.apply_density_ops(cf, psi, subtract_mean=True)
    chi = np.zeros((z.size, nops, nops), dtype=np.complex128)
    nsteps, dropped = np.zeros(nops, dtype=np.int64), 0.0
    nl = min(int(nlanc), sec.Dim)
    cols = [b for b in range(nops) if not norm2[b] < 1e-24]
    while cols:
        if paired and len(cols) > 1:
            pair, cols = cols[:2], cols[2:]
            runs = sec.lanczos_tridiag_pair_probes(vecs[pair[0]], vecs[pair[1]], vecs, nl)
        else:
            pair, cols = cols[:1], cols[1:]
            runs = (sec.lanczos_tridiag_probes(vecs[pair[0]], vecs, nl),)
        for b, (al, bl, ov, n) in zip(pair, runs):
            poles, wts = greens.poles_weights(al[:n], bl[:n], ov, np.sqrt(norm2[b]))
            chi[:, :, b], d = greens.chi_evaluate(poles, wts, z, e_state, cutoff)
            nsteps[b], dropped = n, dropped + d
    return chi, dict(mean=mean, norm2=norm2, nsteps=nsteps, dropped_weight=dropped)


def spin_pair_terms(kind, nimp: int):
    """The operators of HxvSector.apply_spin_pair as a list of term lists [(orb_up, orb_dw, coef), ...], one per operator: "local_pair" =
    c_{a,up} c_{a,dw} of every impurity orbital (flags create_up = create_dw = False), "spin_flip" = S^-_a = c^+_{a,dw} c_{a,up} (create_up =
    False, create_dw = True); an explicit list of term lists is taken as it is."""
    if isinstance(kind, str):
        if kind not in ("local_pair", "spin_flip"):
            raise HxvError('spin_pair_terms: kind is "local_pair", "spin_flip" or a list of term lists')
        return [[(a, a, 1.0)] for a in range(nimp)]
    return [[(int(i), int(j), complex(c)) for i, j, c in op] for op in kind]


def spin_pair_susceptibility(sec, sec_lower, sec_raise, psi, e_state: float, ops, create_up: bool, create_dw: bool, z, nlanc: int = 200):
    """chi_ab(z) = <<O_a; O_b^+>> of ONE device-resident eigenstate psi (energy e_state) of the open sector `sec` for operators that change
    both spin sectors, O_a = sum_t coef_t X_t Y_t with the flags (create_up, create_dw) (HxvSector.apply_spin_pair; ops as spin_pair_terms
    returns them, at most 8):

        chi_ab(z) = -[ sum_n <O_a^+ psi|n><n|O_b^+ psi> / (z - e_n)  -  sum_m <O_b psi|m><m|O_a psi> / (z + e_m) ],   e = E_level - e_state,

    n over `sec_raise`, the sector O^+ reaches (the flags inverted), m over `sec_lower`, the one O reaches; a sector that does not exist
    (nup or ndw outside [0, Ns]) is passed as None and its sum is zero.  O^+ is the same term list with conjugated coefficients and both
    flags inverted.  Column b of the first sum is one lanczos_tridiag_probes run in sec_raise from O_b^+ psi with all O_a^+ psi as probes,
    row a of the second one run in sec_lower from O_a psi with all O_b psi as probes; a start vector with norm2 < 1e-24 is skipped.  For
    Hermitian O this is chi_evaluate's formula.  Nothing Dim-sized crosses PCIe.
    -> (chi[len(z), nops, nops] complex128, info = {"norm2_raise", "norm2_lower", "nsteps_raise", "nsteps_lower"})."""
    from . import greens

    ops = [list(op) for op in ops]
    nops = len(ops)
    if nops < 1 or nops > 8:
        raise HxvError("spin_pair_susceptibility: 1 to 8 operators per call (HXV_MAX_PROBES)")
    z = np.asarray(z, dtype=np.complex128).reshape(-1)
    chi = np.zeros((z.size, nops, nops), dtype=np.complex128)
    info = dict(norm2_raise=np.zeros(nops), norm2_lower=np.zeros(nops), nsteps_raise=np.zeros(nops, dtype=np.int64),
                nsteps_lower=np.zeros(nops, dtype=np.int64))
    if sec_raise is not None:
        dag = [[(i, j, np.conj(complex(c))) for i, j, c in op] for op in ops]
        vecs = [sec.apply_spin_pair(sec_raise, op, not create_up, not create_dw, psi) for op in dag]
        nl = min(int(nlanc), sec_raise.Dim)
        for b in range(nops):
            info["norm2_raise"][b] = vecs[b][1]
            if vecs[b][1] < 1e-24:
                continue
            al, bl, ov, n = sec_raise.lanczos_tridiag_probes(vecs[b][0], [v for v, _ in vecs], nl)
            poles, wts = greens.poles_weights(al[:n], bl[:n], ov, np.sqrt(vecs[b][1]))
            chi[:, :, b] -= greens.evaluate(poles, wts, z, e_state, +1.0)   # wts[n, a] = <O_a^+ psi|n><n|O_b^+ psi>
            info["nsteps_raise"][b] = n
    if sec_lower is not None:
        vecs = [sec.apply_spin_pair(sec_lower, op, create_up, create_dw, psi) for op in ops]
        nl = min(int(nlanc), sec_lower.Dim)
        for a in range(nops):
            info["norm2_lower"][a] = vecs[a][1]
            if vecs[a][1] < 1e-24:
                continue
            al, bl, ov, n = sec_lower.lanczos_tridiag_probes(vecs[a][0], [v for v, _ in vecs], nl)
            poles, wts = greens.poles_weights(al[:n], bl[:n], ov, np.sqrt(vecs[a][1]))
            chi[:, a, :] += greens.evaluate(poles, wts, z, e_state, -1.0)   # wts[m, b] = <O_b psi|m><m|O_a psi>
            info["nsteps_lower"][a] = n
    return chi, info


def one_body_terms(kind, pairs=None):
    """The operators of HxvSector.apply_one_body as a list of term lists [(spin, i, j, coef), ...], one per entry of `pairs` (orbital pairs
    (i, j), 0-based in [0, Ns)): "hop" = sum_s c^+_is c_js, "bond" = sum_s (c^+_is c_js + h.c.), "current" = i sum_s (c^+_is c_js - h.c.),
    "exciton_singlet" = sum_s c^+_as c_bs and "exciton_triplet_z" = sum_s s c^+_as c_bs (s = +1 up, -1 dw) for pairs (a, b) of orbitals
    (the triplet xy component c^+_a,up c_b,dw is spin_pair_terms' kind); an explicit list of term lists is taken as it is."""
    if isinstance(kind, str):
        if kind not in ("hop", "bond", "current", "exciton_singlet", "exciton_triplet_z") or pairs is None:
            raise HxvError('one_body_terms: kind is "hop", "bond", "current", "exciton_singlet" or "exciton_triplet_z" with a list of orbital '
                           "pairs, or a list of term lists")
        ops = []
        for i, j in pairs:
            i, j = int(i), int(j)
            if kind == "bond":
                ops.append([(s, a, b, 1.0 + 0.0j) for s in (0, 1) for a, b in ((i, j), (j, i))])
            elif kind == "current":
                ops.append([(s, a, b, c) for s in (0, 1) for a, b, c in ((i, j, 1.0j), (j, i, -1.0j))])
            else:
                ops.append([(s, i, j, complex(-1.0 if (kind == "exciton_triplet_z" and s == 1) else 1.0)) for s in (0, 1)])
        return ops
    return [[(int(s), int(i), int(j), complex(c)) for s, i, j, c in op] for op in kind]


def _one_body_dagger(op):
    return [(s, j, i, np.conj(complex(c))) for s, i, j, c in op]


def _one_body_summed(op):
    """a term list as {(spin, i, j): summed coefficient} without the zeros: equal for two lists that are the same operator term by term"""
    acc = {}
    for s, i, j, c in op:
        acc[(s, i, j)] = acc.get((s, i, j), 0.0) + complex(c)
    return {k: v for k, v in acc.items() if v != 0.0}


def one_body_susceptibility(sec, psi, e_state: float, ops, z, nlanc: int = 200, cutoff: float = 1e-8):
    """chi_ab(z) = <<dO_a; dO_b^+>> of ONE device-resident eigenstate psi (energy e_state) of the open sector `sec` for one-body operators
    O_a = sum_t coef_t c^+_{i s} c_{j s} (HxvSector.apply_one_body; ops as one_body_terms returns them, 1 to 8), on the fluctuations
    dO = O - <O>: spin_pair_susceptibility's formula with both neighbouring sectors equal to `sec`,

        chi_ab(z) = -[ sum_n <dO_a^+ psi|n><n|dO_b^+ psi> / (z - e_n)  -  sum_m <dO_b psi|m><m|dO_a psi> / (z + e_m) ],   e = E_level - e_state.

    Column b of the first sum is one lanczos_tridiag_probes run from dO_b^+ psi with all dO_a^+ psi as probes, row a of the second one run
    from dO_a psi with all dO_b psi as probes; a start vector with norm2 < 1e-24 is skipped.  Poles with |e_n| <= cutoff are dropped and
    their weight reported, as in greens.chi_evaluate and for its reason: a run started from dO|psi> still finds psi itself to rounding.
    When every operator equals its own dagger as a term multiset the second set of runs is the first: one set runs and chi_evaluate sums
    both.  Nothing Dim-sized crosses PCIe.
    -> (chi[len(z), nops, nops] complex128, info = {"mean", "norm2", "nsteps", "dropped_weight"}; mean, norm2 and nsteps have the shape
    (2, nops): [0] the O^+ side, [1] the O side, equal for Hermitian operators)."""
    from . import greens

    ops = one_body_terms(ops)
    nops = len(ops)
    if nops < 1 or nops > 8:
        raise HxvError("one_body_susceptibility: 1 to 8 operators per call (HXV_MAX_PROBES)")
    z = np.asarray(z, dtype=np.complex128).reshape(-1)
    dag = [_one_body_dagger(op) for op in ops]
    hermitian = all(_one_body_summed(a) == _one_body_summed(b) for a, b in zip(ops, dag))
    chi = np.zeros((z.size, nops, nops), dtype=np.complex128)
    mean, norm2 = np.zeros((2, nops), dtype=np.complex128), np.zeros((2, nops))
    nsteps, dropped = np.zeros((2, nops), dtype=np.int64), 0.0
    nl = min(int(nlanc), sec.Dim)

    def pole_sum(poles, wts, sign):
        e = poles - float(e_state)
        keep = np.abs(e) > float(cutoff)
        return greens.evaluate(poles[keep], wts[keep], z, e_state, sign), float(np.abs(wts[~keep]).sum())

    for side, lists in enumerate((dag,) if hermitian else (dag, ops)):
        vecs = [sec.apply_one_body(op, psi, subtract_mean=True) for op in lists]
        mean[side], norm2[side] = [m for _, m, _ in vecs], [n2 for _, _, n2 in vecs]
        for k in range(nops):
            if vecs[k][2] < 1e-24:
                continue
            al, bl, ov, n = sec.lanczos_tridiag_probes(vecs[k][0], [v for v, _, _ in vecs], nl)
            poles, wts = greens.poles_weights(al[:n], bl[:n], ov, np.sqrt(vecs[k][2]))
            nsteps[side, k] = n
            if hermitian:
                chi[:, :, k], d = greens.chi_evaluate(poles, wts, z, e_state, cutoff)
            elif side == 0:
                part, d = pole_sum(poles, wts, +1.0)         # wts[n, a] = <dO_a^+ psi|n><n|dO_b^+ psi>, b = k
                chi[:, :, k] -= part
            else:
                part, d = pole_sum(poles, wts, -1.0)         # wts[m, b] = <dO_b psi|m><m|dO_a psi>, a = k
                chi[:, k, :] += part
            dropped += d
    if hermitian:
        mean[1], norm2[1], nsteps[1] = mean[0], norm2[0], nsteps[0]
    return chi, dict(mean=mean, norm2=norm2, nsteps=nsteps, dropped_weight=dropped)


def one_body_density_matrix(sec, psi) -> np.ndarray:
    """rho[s, i, j] = <psi|c^+_{i s} c_{j s}|psi> / <psi|psi> over ALL Ns orbitals of the sector, bath included (observables() covers the
    impurity block): complex (2, Ns, Ns) from the means of 2 Ns^2 single-term apply_one_body calls.  A convenience, not a hot path."""
    import math

    import torch

    # Ns from the basis maps: the n with C(n, particles) = dimension, for the spin that has particles (an empty sector of both spins has
    # no one-body density matrix to speak of)
    ns = 0
    for cfgs in sec.maps():
        npart = bin(int(cfgs[0])).count("1")
        if npart:
            ns = next(n for n in range(npart, 33) if math.comb(n, npart) == len(cfgs))
            break
    if not ns:
        raise HxvError("one_body_density_matrix: the sector holds no particle")
    rho =np.zeros((2, ns, ns), dtype=np.complex128)
    out = torch.empty_like(psi)
    for s in (0, 1):
        for i in range(ns):
            for j in range(ns):
                rho[s, i, j] = sec.apply_one_body([(s, i, j, 1.0)], psi, subtract_mean=False, out=out)[1]
    return rho
