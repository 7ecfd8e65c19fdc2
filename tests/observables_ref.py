"""Test infrastructure for the impurity observables (include/hxv.h, hxv_observables_*).

literal(): the reference's three loops restated basis state by basis state (ED_OBSERVABLES.f90 lanc_observables :94-236, lanc_local_energy
:246-452, the single-particle density matrix of density_matrix_impurity :609-686), on maps and vectors in the reference's layout -- no
histogram, no pair tables, so the engine's reformulation is checked against the loops themselves.
record_numpy(): the raw record (W, R_up, R_dw) the device computes, in numpy, from the same inputs.
"""
import numpy as np


def _c(pos, m):
    """c_pos |m> (ED_SETUP.f90 c): (new state, sign)"""
    return m ^ (1 << pos), (-1) ** bin(m & ((1 << pos) - 1)).count("1")


def _cdg(pos, m):
    return m | (1 << pos), (-1) ** bin(m & ((1 << pos) - 1)).count("1")


def literal(model, states):
    """states: [(map_up, map_dw, psi (reference layout i = iup + idw*DimUp), peso), ...] -> dict with derive()'s names, plus
    'Ehartree_reference': Ehartree with the reference's own constant term 0.25*uloc(is) (:399) where that line is defined (every
    is <= 5, the length of Uloc), else None."""
    L, O, S = model.Nlat, model.Norb, model.Nspin
    N = L * O
    H, U, Ust, Jh = model.impHloc, model.Uloc, model.Ust, model.Jh
    dens, dup, ddw, docc, magz = (np.zeros((L, O)) for _ in range(5))
    sz2, n2 = np.zeros((L, L, O, O)), np.zeros((L, L, O, O))
    s2tot = np.zeros(L)
    eknot = epot = ehart = ehart_ref = dust = dund = 0.0
    spdm = np.zeros((L, L, S, S, O, O), dtype=np.complex128)
    ref_defined = N <= 5

    def idx(il, io):  # imp_state_index, 0-based
        return io + il * O

    for map_up, map_dw, psi, peso in states:
        du = len(map_up)
        pos_up = {int(x): i for i, x in enumerate(map_up)}
        pos_dw = {int(x): i for i, x in enumerate(map_dw)}
        for i in range(len(psi)):
            iup, idw = i % du, i // du
            mup, mdw = int(map_up[iup]), int(map_dw[idw])
            nud = [[(mup >> k) & 1 for k in range(N)], [(mdw >> k) & 1 for k in range(N)]]
            nu, nd = nud
            gw = peso * abs(psi[i]) ** 2
            # lanc_observables
            sz = np.array([[(nu[idx(il, io)] - nd[idx(il, io)]) / 2 for io in range(O)] for il in range(L)])
            nt = np.array([[nu[idx(il, io)] + nd[idx(il, io)] for io in range(O)] for il in range(L)], dtype=float)
            for il in range(L):
                for io in range(O):
                    s = idx(il, io)
                    dens[il, io] += nt[il, io] * gw
                    dup[il, io] += nu[s] * gw
                    ddw[il, io] += nd[s] * gw
                    docc[il, io] += nu[s] * nd[s] * gw
                    magz[il, io] += (nu[s] - nd[s]) * gw
                s2tot[il] += sz[il, :].sum() ** 2 * gw
            for il in range(L):
                for io in range(O):
                    sz2[il, il, io, io] += sz[il, io] * sz[il, io] * gw
                    n2[il, il, io, io] += nt[il, io] * nt[il, io] * gw
                    for jl in range(L):
                        for jo in range(io + 1, O):
                            sz2[il, jl, io, jo] += sz[il, io] * sz[jl, jo] * gw
                            sz2[il, jl, jo, io] += sz[il, jo] * sz[jl, io] * gw
                            n2[il, jl, io, jo] += nt[il, io] * nt[jl, jo] * gw
                            n2[il, jl, jo, io] += nt[il, jo] * nt[jl, io] * gw
            # lanc_local_energy
            for il in range(L):
                for io in range(O):
                    s = idx(il, io)
                    eknot += (H[il, il, 0, 0, io, io] * nu[s] * gw).real
                    eknot += (H[il, il, S - 1, S - 1, io, io] * nd[s] * gw).real
            for il in range(L):
                for jl in range(L):
                    for io in range(O):
                        for jo in range(O):
                            s, t = idx(il, io), idx(jl, jo)
                            if H[il, jl, 0, 0, io, jo] != 0 and nu[t] == 1 and nu[s] == 0:
                                k1, sg1 = _c(t, mup)
                                k2, sg2 = _cdg(s, k1)
                                j = pos_up[k2] + idw * du
                                eknot += (H[il, jl, 0, 0, io, jo] * sg1 * sg2 * psi[i] * np.conj(psi[j]) * peso).real
                            if H[il, jl, S - 1, S - 1, io, jo] != 0 and nd[t] == 1 and nd[s] == 0:
                                k1, sg1 = _c(t, mdw)
                                k2, sg2 = _cdg(s, k1)
                                j = iup + pos_dw[k2] * du
                                eknot += (H[il, jl, S - 1, S - 1, io, jo] * sg1 * sg2 * psi[i] * np.conj(psi[j]) * peso).real
            for il in range(L):
                for io in range(O):
                    s = idx(il, io)
                    epot += U[io] * nu[s] * nd[s] * gw
            if O > 1:
                for il in range(L):
                    for io in range(O):
                        for jo in range(io + 1, O):
                            s, t = idx(il, io), idx(il, jo)
                            epot += Ust * (nu[s] * nd[t] + nu[t] * nd[s]) * gw
                            dust += (nu[s] * nd[t] + nu[t] * nd[s]) * gw
                            epot += (Ust - Jh) * (nu[s] * nu[t] + nd[s] * nd[t]) * gw
                            dund += (nu[s] * nu[t] + nd[s] * nd[t]) * gw
            if model.hfmode:
                for il in range(L):
                    for io in range(O):
                        s = idx(il, io)
                        ehart += -0.5 * U[io] * (nu[s] + nd[s]) * gw + 0.25 * U[io] * gw
                        if ref_defined:
                            ehart_ref += -0.5 * U[io] * (nu[s] + nd[s]) * gw + 0.25 * U[s] * gw
                if O > 1:
                    for il in range(L):
                        for io in range(O):
                            for jo in range(io + 1, O):
                                s, t = idx(il, io), idx(il, jo)
                                for u in (Ust, Ust - Jh):
                                    x = -0.5 * u * (nu[s] + nd[s] + nu[t] + nd[t]) * gw + 0.25 * u * gw
                                    ehart += x
                                    ehart_ref += x
            # single-particle density matrix
            for il in range(L):
                for sp in range(S):
                    for io in range(O):
                        spdm[il, il, sp, sp, io, io] += peso * nud[sp][idx(il, io)] * np.conj(psi[i]) * psi[i]
            for sp in range(S):
                m_s = mup if sp == 0 else mdw
                for il in range(L):
                    for jl in range(L):
                        for io in range(O):
                            for jo in range(O):
                                s, t = idx(il, io), idx(jl, jo)
                                if nud[sp][t] == 1 and nud[sp][s] == 0:
                                    r, sg1 = _c(t, m_s)
                                    k, sg2 = _cdg(s, r)
                                    j = pos_up[k] + idw * du if sp == 0 else iup + pos_dw[k] * du
                                    spdm[il, jl, sp, sp, io, jo] += peso * sg1 * psi[i] * sg2 * np.conj(psi[j])
    return {"dens": dens, "dens_up": dup, "dens_dw": ddw, "docc": docc, "magz": magz, "sz2": sz2, "n2": n2, "s2tot": s2tot, "Eknot": eknot,
            "Epot": epot + ehart, "Ehartree": ehart, "Dust": dust, "Dund": dund, "single_particle_density_matrix": spdm,
            "Ehartree_reference": ehart_ref if (ref_defined and model.hfmode) else None}


def _pairs(conf, nimp):
    """every (is, js, target, sign) with c^+_is c_js |conf> != 0, is != js"""
    out = []
    for js in range(nimp):
        if not (conf >> js) & 1:
            continue
        r, s1 = _c(js, conf)
        for is_ in range(nimp):
            if is_ == js or (r >> is_) & 1:
                continue
            k, s2 = _cdg(is_, r)
            out.append((is_, js, k, s1 * s2))
    return out


def record_numpy(model, map_up, map_dw, psi, weight=1.0):
    """The raw record of hxv_observables_accumulate from a vector in the reference's layout (numpy, the histogram formulation)."""
    N = model.Nlat * model.Norb
    nw = 1 << N
    mu, md = np.asarray(map_up, dtype=np.int64), np.asarray(map_dw, dtype=np.int64)
    P = np.asarray(psi, dtype=np.complex128).reshape(len(md), len(mu))  # [idw, iup]
    A = np.abs(P) ** 2
    W = np.zeros((nw, nw))  # [a_dw, a_up]
    np.add.at(W, ((md & (nw - 1))[:, None], (mu & (nw - 1))[None, :]), A)
    R = np.zeros((2, N, N), dtype=np.complex128)
    pos_up = {int(x): i for i, x in enumerate(mu)}
    pos_dw = {int(x): i for i, x in enumerate(md)}
    for iup, conf in enumerate(mu):
        for is_, js, k, sg in _pairs(int(conf), N):
            R[0, is_, js] += sg * np.dot(P[:, iup], np.conj(P[:, pos_up[k]]))
    for idw, conf in enumerate(md):
        for is_, js, k, sg in _pairs(int(conf), N):
            R[1, is_, js] += sg * np.dot(P[idw, :], np.conj(P[pos_dw[k], :]))
    for s in range(N):
        R[0, s, s] = A[:, ((mu >> s) & 1) == 1].sum()
        R[1, s, s] = A[((md >> s) & 1) == 1, :].sum()
    return weight * np.concatenate([W.ravel(), R[0].ravel(order="F").view(np.float64), R[1].ravel(order="F").view(np.float64)])


def oracle_states(model, sectors, nstates=1):
    """(map_up, map_dw, psi, energy) of the lowest `nstates` eigenpairs of each sector, from the CPU oracle's dense matrix."""
    from oracle.oracle import OracleSector

    out = []
    for nup, ndw in sectors:
        o = OracleSector(model, nup, ndw)
        e, v = np.linalg.eigh(o.dense())
        for k in range(min(nstates, len(e))):
            out.append((o.map_up(), o.map_dw(), v[:, k].copy(), float(e[k])))
        o.close()
    return out
