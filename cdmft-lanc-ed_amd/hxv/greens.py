"""Green's functions from probe overlaps (include/hxv.h: hxv_lanczos_tridiag_probes, hxv_gf_from_probes).

One Lanczos run from v = c^dagger_i|gs> (or c_i|gs>) with the other orbitals' vectors p_j as probes gives every <p_j|(z - H)^-1|v>: the
off-diagonal impurity Green's functions without the reference's mixed channels (ED_GF_NORMAL.f90:315-903).  poles_weights is host code of
the library (its own tridiagonal QL); evaluate applies the reference's pole convention (add_to_lanczos_gf_normal, ED_GF_NORMAL.f90:915-975).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import _chk, _p, load_library


def poles_weights(alanc, blanc, overlaps, norm: float):
    """-> (poles[nsteps] ascending, weights[nsteps, nprobes] complex128) with <p_j|(z - H)^-1|v> ~ sum_n weights[n, j] / (z - poles[n]).
    alanc, blanc, overlaps: the first nsteps entries of what HxvSector.lanczos_tridiag_probes returned (nsteps = len(alanc));
    norm = |v| of the unnormalised start vector (sqrt of apply_ladder's norm2; 1.0 for a vector that was normalised before the run and
    whose norm is applied by the caller)."""
    a = np.ascontiguousarray(alanc, dtype=np.float64)
    b = np.ascontiguousarray(blanc, dtype=np.float64)
    n = int(a.size)
    ov = np.ascontiguousarray(overlaps, dtype=np.complex128).reshape(n, -1) if n else np.zeros((0, 0), dtype=np.complex128)
    assert b.size == n and ov.shape[0] == n
    npr = int(ov.shape[1])
    poles = np.zeros(max(n, 1))
    w = np.zeros((max(n, 1), npr), dtype=np.complex128)
    as_d = lambda x: C.cast(x.ctypes.data, C.POINTER(C.c_double))  # noqa: E731
    _chk(load_library().hxv_gf_from_probes(n, _p(a, C.c_double), _p(b, C.c_double), npr, as_d(ov) if npr else None, float(norm),
                                           _p(poles, C.c_double), as_d(w) if npr else None), "hxv_gf_from_probes")
    return poles[:n], w[:n]


def evaluate(poles, weights, z, e0: float, sign: float):
    """sum_n weights[n, ...] / (z - sign * (poles[n] - e0)) for every z: sign = +1 for a c^dagger channel, -1 for a c channel, e0 the
    ground-state energy (the reference's isign and Ei, ED_GF_NORMAL.f90:958-973).  -> array of shape z.shape + weights.shape[1:]."""
    poles = np.asarray(poles, dtype=np.float64)
    w = np.asarray(weights, dtype=np.complex128)
    z = np.asarray(z, dtype=np.complex128)
    den = 1.0 / (z[..., None] - sign * (poles - e0))          # z.shape + (n,)
    return np.tensordot(den, w, axes=([-1], [0]))


def chi_evaluate(poles, weights, z, e_state: float, cutoff: float = 1e-8):
    """The bosonic pole sum of a susceptibility column (include/hxv.h, hxv_apply_density_ops):

        chi[..., a](z) = - sum_n [ w_n[a] / (z - e_n) - conj(w_n[a]) / (z + e_n) ],   e_n = poles[n] - e_state,

    poles, weights from poles_weights() of the run started from dO_b|psi> with the probes dO_a|psi> and norm = |dO_b psi|; e_state the
    energy of psi.  At z = i nu and real symmetric weights this is the reference's Lehmann form sum_n W_n 2 e_n / (nu^2 + e_n^2).
    Poles with |e_n| <= cutoff are DROPPED: a run started from dO|psi> still finds psi itself (dO projects it out to rounding only), as
    Ritz values within 1e-8 of e_state with weights of 1e-25, and at z = 0 such a pole is tiny / tiny, or x / 0.  A degenerate level that
    carries real weight is the caller's Curie term, not this sum's.
    -> (chi of shape z.shape + weights.shape[1:], dropped_weight = the summed |weight| of the dropped poles: assert it is negligible)."""
    poles = np.asarray(poles, dtype=np.float64)
    w = np.asarray(weights, dtype=np.complex128)
    z = np.asarray(z, dtype=np.complex128)
    e = poles - float(e_state)
    keep = np.abs(e) > float(cutoff)
    dropped = float(np.abs(w[~keep]).sum())
    e, w = e[keep], w[keep]
    chi = -(np.tensordot(1.0 / (z[..., None] - e), w, axes=([-1], [0])) - np.tensordot(1.0 / (z[..., None] + e), w.conj(), axes=([-1], [0])))
    return chi, dropped
