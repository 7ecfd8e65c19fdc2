"""Test infrastructure for the reduced density matrix of an impurity-orbital subset (include/hxv.h, hxv_reduced_dm_accumulate).

masked_trace_literal(): the reference's loop nest (ED_IO/get_reduced_dm.f90:127-157) restated index by index on a dense cluster density
matrix, with get_sign (:170-191) and split_state (:193-210) as written; it also returns the set of sign products (:148) of the pairs that
contribute, which is what shows that the reference's masked trace carries no sign at all.
direct(): the same matrix from the vector, for any Nimp, with or without the Jordan-Wigner sign of the subset.
Masks are iterables of 0-based impurity bit indices (bit b <-> the reference's index b + 1 = jorb + (ilat-1)*Norb).
Both return (4^Nred, 4^Nred) complex arrays, element [io, jo], io = a_up + 2^Nred a_dw, a = the subset's occupations in ascending bit order.
"""
import numpy as np

from cluster_dm_ref import nimp_of


def mask_bits(mask):
    return sorted(int(b) for b in mask)


def mask_int(mask):
    return sum(1 << b for b in mask_bits(mask))


def _bdecomp(i, n):
    return [(i >> k) & 1 for k in range(n)]


def _bjoin(bits):
    return sum(b << k for k, b in enumerate(bits))


def _get_sign(state, indices):
    """:170-191, indices 1-based"""
    filtered = list(state)
    for r in indices:
        filtered[r - 1] = 0
    n = 0
    for r in indices:
        n += sum(filtered[:r])
    return 1.0 if n % 2 == 0 else -1.0


def _split_state(state, red, tr):
    return _bjoin([state[r - 1] for r in red]), _bjoin([state[r - 1] for r in tr])


def masked_trace_literal(cdm, Nimp, mask):
    """-> (rdm, set of the sign products met on contributing pairs).  The per-configuration work of the four nested loops is tabulated
    once (it depends on one spin configuration alone); the loop over (i, j) and the cycle condition are the reference's."""
    bits = mask_bits(mask)
    Nred = len(bits)
    if Nred == Nimp:
        return np.array(cdm, dtype=np.complex128), {1.0}   # :102-105, the matrix poured as it is
    red = [b + 1 for b in bits]
    tr = [b + 1 for b in range(Nimp) if b not in bits]
    nw = 1 << Nimp
    sign, redst, trst = np.zeros(nw), np.zeros(nw, dtype=np.int64), np.zeros(nw, dtype=np.int64)
    for s in range(nw):
        st = _bdecomp(s, Nimp)
        sign[s] = _get_sign(st, red)
        redst[s], trst[s] = _split_state(st, red, tr)
    rdm = np.zeros((4 ** Nred, 4 ** Nred), dtype=np.complex128)
    signs = set()
    by_tr = {}
    for s in range(nw):
        by_tr.setdefault(int(trst[s]), []).append(s)
    for iUP in range(nw):
        for iDW in range(nw):
            i = iUP + iDW * nw
            io = redst[iUP] + redst[iDW] * 2 ** Nred
            for jUP in by_tr[int(trst[iUP])]:          # jTrUP /= iTrUP: cycle
                for jDW in by_tr[int(trst[iDW])]:      # jTrDW /= iTrDW: cycle
                    j = jUP + jDW * nw
                    jo = redst[jUP] + redst[jDW] * 2 ** Nred
                    sg = sign[iUP] * sign[iDW] * sign[jUP] * sign[jDW]
                    signs.add(float(sg))
                    rdm[io, jo] += cdm[i, j] * sg
    return rdm, signs


def _pext(m, bits):
    out = np.zeros_like(m)
    for k, b in enumerate(bits):
        out |= ((m >> b) & 1) << k
    return out


def _fermi(m, bits, S):
    """(-1)^n per configuration: n = for every occupied orbital r of the subset, the occupied orbitals outside it below r"""
    n = np.zeros_like(m)
    for r in bits:
        below = m & ~S & ((1 << r) - 1)
        cnt = np.zeros_like(m)
        for k in range(r):
            cnt += (below >> k) & 1
        n += ((m >> r) & 1) * cnt
    return 1.0 - 2.0 * (n & 1)


def _classes(m, bits, S):
    """one spin's configurations by environment particle number: [(index array [group, member], the members' subset occupations), ...];
    a group = the configurations that share m & ~S, its members in ascending order"""
    env = m & ~S
    npart = np.zeros_like(m)
    for k in range(32):
        npart += (env >> k) & 1
    out = []
    for k in np.unique(npart):
        idx = np.flatnonzero(npart == k)
        idx = idx[np.argsort(env[idx], kind="stable")]
        ngrp = np.unique(env[idx]).size
        idx = idx.reshape(ngrp, -1)
        a = _pext(m[idx], bits)
        assert np.all(env[idx] == env[idx[:, :1]]) and np.all(a == a[:1])
        out.append((idx, a[0]))
    return out


def direct(model, map_up, map_dw, psi, mask, peso=1.0, fermi_sign=0):
    bits = mask_bits(mask)
    assert bits and bits[-1] < nimp_of(model) and len(set(bits)) == len(bits)
    S = mask_int(bits)
    Nred = len(bits)
    mu, md = np.asarray(map_up, dtype=np.int64), np.asarray(map_dw, dtype=np.int64)
    P = np.asarray(psi, dtype=np.complex128).reshape(len(md), len(mu))   # [idw, iup]
    if fermi_sign:
        P = P * _fermi(md, bits, S)[:, None] * _fermi(mu, bits, S)[None, :]
    nw = 1 << Nred
    rho = np.zeros((nw * nw, nw * nw), dtype=np.complex128)
    cu, cd = _classes(mu, bits, S), _classes(md, bits, S)
    for rows, a_u in cu:                       # rows [up group, iu], a_u [iu]
        for cols, a_d in cd:                   # cols [dw group, id], a_d [id]
            X = P[cols.reshape(-1)][:, rows.reshape(-1)].reshape(cols.shape + rows.shape)     # [dw group, id, up group, iu]
            X = X.transpose(1, 3, 0, 2).reshape(a_d.size * a_u.size, -1)                      # [(id, iu), pair]
            orb = (a_u[None, :] + nw * a_d[:, None]).reshape(-1)
            rho[np.ix_(orb, orb)] += X @ X.conj().T
    return peso * rho


def gaussian_entropy_and_purity_subset(model, levels_up, levels_dw, mask):
    """cluster_dm_ref.gaussian_entropy_and_purity with each spin's one-body projector restricted to the subset's rows and columns."""
    from onebody import one_body_matrix

    bits = mask_bits(mask)
    S, pur = 0.0, 1.0
    for spin, lev in ((0, list(levels_up)), (model.Nspin - 1, list(levels_dw))):
        _, phi = np.linalg.eigh(one_body_matrix(model, spin))
        Psub = (np.conj(phi[:, lev]) @ phi[:, lev].T)[np.ix_(bits, bits)]
        for nu in np.linalg.eigvalsh(Psub):
            for x in (nu, 1.0 - nu):
                if x > 1e-300:
                    S -= x * np.log(x)
            pur *= nu * nu + (1.0 - nu) * (1.0 - nu)
    return S, pur
