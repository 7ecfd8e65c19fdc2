"""Test infrastructure for the cluster reduced density matrix (include/hxv.h, hxv_cluster_dm_accumulate).

literal(): the reference's loop nest (ED_OBSERVABLES.f90 density_matrix_impurity :465-582) restated basis state by basis state, on maps and
vectors in the reference's layout (i = iup + idw*DimUp): every pair of basis states that share both bath configurations contributes
psi_i conj(psi_j) peso to element (io, jo) -- no bath groups, no classes, no blocks, so the engine's reformulation is checked against the
loop body itself (:539-566).
vectorised(): the same matrix as rank-k updates X X^+, X the amplitudes of the bath pairs (b_up, b_dw) as columns; the columns of one dw
bath configuration and every up bath configuration of one particle number go into one product.
Both return a (4^Nimp, 4^Nimp) complex array, element [io, jo], io = a_up + 2^Nimp a_dw (0-based).
"""
import numpy as np


def nimp_of(model):
    return model.Nlat * model.Norb


def literal(model, states):
    """states: [(map_up, map_dw, psi, peso), ...]"""
    N = nimp_of(model)
    nw = 1 << N
    rho = np.zeros((nw * nw, nw * nw), dtype=np.complex128)
    for map_up, map_dw, psi, peso in states:
        du = len(map_up)
        by_bath_up, by_bath_dw = {}, {}
        for iup, m in enumerate(map_up):
            by_bath_up.setdefault(int(m) >> N, []).append((iup, int(m) & (nw - 1)))
        for idw, m in enumerate(map_dw):
            by_bath_dw.setdefault(int(m) >> N, []).append((idw, int(m) & (nw - 1)))
        for i in range(len(psi)):
            iup, idw = i % du, i // du
            mup, mdw = int(map_up[iup]), int(map_dw[idw])
            io = (mup & (nw - 1)) + nw * (mdw & (nw - 1))
            for jup, a_up in by_bath_up[mup >> N]:
                for jdw, a_dw in by_bath_dw[mdw >> N]:
                    jo = a_up + nw * a_dw
                    rho[io, jo] += psi[i] * np.conj(psi[jup + jdw * du]) * peso
    return rho


def _groups(mp, N):
    """{bath particle number: [index array of one bath configuration's run, ...]} and the impurity bits of every index"""
    mp = np.asarray(mp, dtype=np.int64)
    bath = mp >> N
    out = {}
    start = 0
    for k in range(1, len(mp) + 1):
        if k == len(mp) or bath[k] != bath[start]:
            out.setdefault(bin(int(bath[start])).count("1"), []).append(np.arange(start, k))
            start = k
    return out, mp & ((1 << N) - 1)


def vectorised(model, map_up, map_dw, psi, peso=1.0):
    N = nimp_of(model)
    nw = 1 << N
    P = np.asarray(psi, dtype=np.complex128).reshape(len(map_dw), len(map_up))  # [idw, iup]
    gup, aup = _groups(map_up, N)
    gdw, adw = _groups(map_dw, N)
    rho = np.zeros((nw * nw, nw * nw), dtype=np.complex128)
    for runs_up in gup.values():
        rows = np.stack(runs_up)                      # [up group, iu]
        a_u = aup[rows[0]]
        for runs_dw in gdw.values():
            a_d = adw[runs_dw[0]]
            orb = (a_u[None, :] + nw * a_d[:, None]).reshape(-1)          # component iu + dU*id -> io
            blk = np.zeros((orb.size, orb.size), dtype=np.complex128)
            for cols in runs_dw:
                X = P[cols][:, rows]                                       # [id, up group, iu]
                X = X.transpose(0, 2, 1).reshape(orb.size, rows.shape[0])  # [(id, iu), up group]
                blk += X @ X.conj().T
            rho[np.ix_(orb, orb)] += peso * blk
    return rho


def entropy_and_purity(rho):
    w = np.linalg.eigvalsh(rho)
    w = w[w > 1e-300]
    return float(-(w * np.log(w)).sum()), float(np.real(np.trace(rho @ rho)))


def gaussian_entropy_and_purity(model, levels_up, levels_dw):
    """The closed form for a U = 0 Slater determinant: nu = eigenvalues of the impurity block of each spin's one-body projector;
    S = sum_s sum_k [h(nu_k) + h(1 - nu_k)], h(x) = -x ln x;  Tr rho^2 = prod_s prod_k (nu_k^2 + (1 - nu_k)^2)."""
    from onebody import one_body_matrix

    N = nimp_of(model)
    S, pur = 0.0, 1.0
    for spin, lev in ((0, list(levels_up)), (model.Nspin - 1, list(levels_dw))):
        _, phi = np.linalg.eigh(one_body_matrix(model, spin))
        Pimp = (np.conj(phi[:, lev]) @ phi[:, lev].T)[:N, :N]
        for nu in np.linalg.eigvalsh(Pimp):
            for x in (nu, 1.0 - nu):
                if x > 1e-300:
                    S -= x * np.log(x)
            pur *= nu * nu + (1.0 - nu) * (1.0 - nu)
    return S, pur
