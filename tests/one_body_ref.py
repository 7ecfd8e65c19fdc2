"""numpy restatement of hxv_apply_one_body (include/hxv.h) and of hxv.observables.one_body_susceptibility, from the basis maps alone.
Vectors are in the reference's layout, i = iup + idw * DimUp; a sector's maps are (map_up, map_dw), each the ascending bit strings of one
spin (orbital o <-> bit o).  A term is (spin, i, j, coef) = coef c^+_{i,spin} c_{j,spin}; the sign is the fermionic one,
(-1)^(occupied same-spin orbitals strictly between i and j).  The fixtures, the Fock matrices and the dense spectra are spin_pair_ref's."""
import numpy as np

import spin_pair_ref as S


def table(cfgs, i, j):
    """for every configuration of one spin: the index of its source under c^+_i c_j, or -1, and the sign (+1 / -1, 0 where dead)"""
    m = np.asarray(cfgs, dtype=np.int64)
    bi, bj = 1 << i, 1 << j
    live = (m & bi) != 0
    if i != j:
        live &= (m & bj) == 0
    src_cfg = m ^ bi ^ bj
    pos = np.minimum(np.searchsorted(m, src_cfg), m.size - 1)
    live &= m[pos] == src_cfg
    par = np.zeros(m.size, dtype=np.int64)
    for b in range(min(i, j) + 1, max(i, j)):
        par ^= (src_cfg >> b) & 1
    return np.where(live, pos, -1), np.where(live, 1 - 2 * par, 0)


def apply(maps, terms, psi, subtract_mean=False):
    """-> (out, mean, norm2) of hxv_apply_one_body: out = (sum_t coef_t c^+_i c_j - m) psi, the terms summed in order in the real arithmetic
    of the kernel (one rounding per product and per add; the first live term is stored, not added to zero), mean = <psi|O psi> / <psi|psi>,
    m = mean when subtract_mean, norm2 = <out|out> of what is returned"""
    mu, md = maps
    psi2 = np.asarray(psi, dtype=np.complex128).reshape(len(md), len(mu))
    out = np.zeros_like(psi2)
    touched = np.zeros(out.shape, dtype=bool)
    for spin, i, j, cf in terms:
        src, sg = table(md if spin else mu, i, j)
        live = np.nonzero(src >= 0)[0]
        if live.size == 0:
            continue
        cf = complex(cf)
        if spin:
            x, g, idx = psi2[src[live], :], sg[live][:, None].astype(np.float64), (live, slice(None))
        else:
            x, g, idx = psi2[:, src[live]], sg[live][None, :].astype(np.float64), (slice(None), live)
        r = g * (cf.real * x.real - cf.imag * x.imag) + 1j * (g * (cf.real * x.imag + cf.imag * x.real))
        out[idx] = np.where(touched[idx], out[idx] + r, r)
        touched[idx] = True
    out = out.reshape(-1)
    flat = psi2.reshape(-1)
    mean = np.vdot(flat, out) / np.vdot(flat, flat).real
    if subtract_mean:
        out = out - mean * flat
    return out, complex(mean), float(np.vdot(out, out).real)


def dagger(terms):
    """O^+ of a term list: i and j exchanged, conjugated coefficients"""
    return [(s, j, i, np.conj(complex(c))) for s, i, j, c in terms]


def fock_operator(ns, terms):
    """sum_t coef_t c^+_{i s} c_{j s} as a 4^ns x 4^ns matrix of true fermionic operators (up orbital o = mode o, dw orbital o = mode ns + o)"""
    n = 2 * ns
    op = np.zeros((2 ** n, 2 ** n), dtype=complex)
    for s, i, j, cf in terms:
        op += complex(cf) * (S.fock_c(n, s * ns + i).T @ S.fock_c(n, s * ns + j))
    return op


# ---- the operators of the susceptibility checks, by fixture of spin_pair_ref.chi_fixture (tests/test_one_body_ref_cpu.py asserts the
# ---- fixtures' properties on the CPU); built here, not with hxv.observables.one_body_terms, which the GPU test compares with them
def bond(i, j):
    return [(s, a, b, 1.0) for s in (0, 1) for a, b in ((i, j), (j, i))]


def current(i, j):
    return [(s, a, b, c) for s in (0, 1) for a, b, c in ((i, j, 1.0j), (j, i, -1.0j))]


def hop(i, j):
    return [(s, i, j, 1.0) for s in (0, 1)]


def exciton(a, b, triplet):
    return [(s, a, b, -1.0 if (triplet and s == 1) else 1.0) for s in (0, 1)]


def chi_ops(name):
    """the operator lists of one fixture: Hermitian sets run the one-set path, the single hop on the plaquette both run sets"""
    return {"plaquette": {"hermitian": [bond(0, 1), current(0, 1), bond(0, 2)], "hop": [hop(0, 1)]},
            "chain": {"hermitian": [bond(0, 1), current(0, 1)]},
            # (impurity orbital = site * Norb + orbital: the two orbitals of site 0 are 0 and 1, those of site 1 are 2 and 3)
            "bhz": {"exciton": [exciton(0, 1, False), exciton(0, 1, True), exciton(2, 3, False), exciton(2, 3, True)]},
            "square": {"hermitian": [bond(0, 1), bond(0, 4), current(0, 1)]}}[name]


def lehmann_chi(w, U, maps, ops, z):
    """the dense sum of spin_pair_ref.lehmann_chi with both neighbours equal to the state's own sector: the ground state (level 0) is the
    state, left out of the spectrum, and the vectors are the fluctuations (O - <O>) psi"""
    psi, e0 = U[:, 0], w[0]
    up = [apply(maps, dagger(op), psi, True)[0] for op in ops]
    lo = [apply(maps, op, psi, True)[0] for op in ops]
    return S.lehmann_chi(e0, (w[1:], U[:, 1:], up), (w[1:], U[:, 1:], lo), z)
