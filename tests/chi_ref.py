"""numpy restatement of the susceptibility stage (include/hxv.h, hxv_apply_density_ops; hxv.greens.chi_evaluate): the density-type operator from
the basis maps, a plain three-term recurrence with probe overlaps, and the dense Lehmann sum.  Vectors are in the reference's layout,
i = iup + idw * DimUp."""
import numpy as np

BETA, NFREQ = 50.0, 64
NU = 2.0 * np.pi * np.arange(NFREQ) / BETA          # bosonic Matsubara frequencies, nu_0 = 0 included


def density_f(map_up, map_dw, coef):
    """f[a, i]: the diagonal of O_a = sum_is (cu_a[is] n_is,up + cd_a[is] n_is,dw); coef (nops, 2, Nimp), the impurity orbitals are the low bits"""
    coef = np.asarray(coef, dtype=np.float64)
    mu, md = np.asarray(map_up, dtype=np.int64), np.asarray(map_dw, dtype=np.int64)
    nimp = coef.shape[2]
    bits_u = np.stack([(mu >> b) & 1 for b in range(nimp)]).astype(np.float64)      # [Nimp, DimUp]
    bits_d = np.stack([(md >> b) & 1 for b in range(nimp)]).astype(np.float64)
    fu, fd = coef[:, 0, :] @ bits_u, coef[:, 1, :] @ bits_d                          # [nops, DimUp], [nops, DimDw]
    return (fu[:, None, :] + fd[:, :, None]).reshape(coef.shape[0], -1)              # idw slow, iup fast


def fluctuations(f, psi, subtract_mean=True):
    """-> ((f_a - m_a) psi [nops, Dim], mean[nops], norm2[nops])"""
    w = np.abs(psi) ** 2
    mean = (f * w).sum(axis=1) / w.sum()
    out = (f - (mean[:, None] if subtract_mean else 0.0)) * psi[None, :]
    return out, mean, (np.abs(out) ** 2).sum(axis=1)


def lanczos(H, v, probes, nsteps):
    """plain three-term recurrence, no re-orthogonalisation, no stop: alanc, blanc (blanc[0] = 0), overlaps[k, j] = <p_j|q_k>"""
    q = v / np.linalg.norm(v)
    qm = np.zeros_like(q)
    a, b, ov = np.zeros(nsteps), np.zeros(nsteps), np.zeros((nsteps, len(probes)), dtype=complex)
    beta = 0.0
    for k in range(nsteps):
        ov[k] = [np.vdot(p, q) for p in probes]
        w = H @ q - beta * qm
        a[k] = np.vdot(q, w).real
        w = w - a[k] * q
        beta = np.linalg.norm(w)
        if beta == 0.0:
            return a[:k + 1], b[:k + 1], ov[:k + 1]
        if k + 1 < nsteps:
            b[k + 1] = beta
        qm, q = q, w / beta
    return a, b, ov


def poles_weights(a, b, ov, norm):
    """numpy.linalg.eigh form of hxv_gf_from_probes: weights[n, j] = norm * Z_1n * sum_k o_kj Z_kn"""
    ev, Z = np.linalg.eigh(np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1))
    return ev, norm * Z[0, :, None] * (Z.T @ ov)


def lehmann_chi(w, U, istate, vecs, z):
    """chi[z, a, b] = - sum_{n != istate} [ W_n^{ab} / (z - e_n) - conj(W_n^{ab}) / (z + e_n) ],  W_n^{ab} = <p_a|n><n|p_b>,  e_n = E_n - E_istate,
    over the dense spectrum (w, U) of the sector; vecs[a] = dO_a|psi>"""
    A = U.conj().T @ np.stack(vecs, axis=1)                      # <n|p_a>
    keep = np.arange(w.size) != istate
    e, A = w[keep] - w[istate], A[keep]
    W = np.einsum("na,nb->nab", A.conj(), A)
    z = np.asarray(z, dtype=complex)
    return -(np.einsum("zn,nab->zab", 1.0 / (z[:, None] - e), W) - np.einsum("zn,nab->zab", 1.0 / (z[:, None] + e), W.conj()))


def spin_charge_coef(kind, nimp):
    cf = np.zeros((nimp, 2, nimp))
    for a in range(nimp):
        cf[a, 0, a], cf[a, 1, a] = (0.5, -0.5) if kind == "spin" else (1.0, 1.0)
    return cf
