"""numpy restatement of hxv_apply_spin_pair (include/hxv.h) and of hxv.observables.spin_pair_susceptibility, from the basis maps alone.
Vectors are in the reference's layout, i = iup + idw * DimUp; a sector's maps are (map_up, map_dw), each the ascending bit strings of one
spin (orbital o <-> bit o).  The sign convention is the engine's: every one-spin operator carries (-1)^(occupied orbitals of ITS spin below
the orbital) and nothing else."""
import numpy as np

BETA, NFREQ = 50.0, 64
NU = 2.0 * np.pi * np.arange(NFREQ) / BETA          # bosonic Matsubara frequencies, nu_0 = 0 included


def one_spin_table(map_from, map_to, orbital, create):
    """for every configuration of map_to: the index in map_from of its source under c (create False) / c^dagger (True) on `orbital`, or -1,
    and the sign (+1 / -1, 0 where dead)"""
    mf, mt = np.asarray(map_from, dtype=np.int64), np.asarray(map_to, dtype=np.int64)
    bit = 1 << orbital
    live = ((mt & bit) != 0) == bool(create)
    src_cfg = mt ^ bit
    pos = np.searchsorted(mf, src_cfg)
    pos_c = np.minimum(pos, mf.size - 1) if mf.size else np.zeros_like(pos)
    live &= (mf[pos_c] == src_cfg) if mf.size else False
    below = src_cfg & (bit - 1)
    par = np.zeros(mt.size, dtype=np.int64)
    for b in range(orbital):
        par ^= (below >> b) & 1
    return np.where(live, pos_c, -1), np.where(live, 1 - 2 * par, 0)


def apply(maps_a, maps_b, terms, create_up, create_dw, psi):
    """out = sum_t coef_t X_t Y_t psi from sector a into sector b; terms = [(orb_up, orb_dw, coef), ...], summed in order, in the real
    arithmetic of the kernel (one rounding per product and per add; the first live term is stored, not added to zero)"""
    (mua, mda), (mub, mdb) = maps_a, maps_b
    psi2 = np.asarray(psi, dtype=np.complex128).reshape(len(mda), len(mua))
    out = np.zeros((len(mdb), len(mub)), dtype=np.complex128)
    touched = np.zeros(out.shape, dtype=bool)
    for ou, od, cf in terms:
        su, gu = one_spin_table(mua, mub, ou, create_up)
        sd, gd = one_spin_table(mda, mdb, od, create_dw)
        lu, ld = np.nonzero(su >= 0)[0], np.nonzero(sd >= 0)[0]
        if lu.size == 0 or ld.size == 0:
            continue
        x = psi2[np.ix_(sd[ld], su[lu])]
        sg = (gd[ld][:, None] * gu[lu][None, :]).astype(np.float64)
        cf = complex(cf)
        r = sg * (cf.real * x.real - cf.imag * x.imag) + 1j * (sg * (cf.real * x.imag + cf.imag * x.real))
        idx = np.ix_(ld, lu)
        out[idx] = np.where(touched[idx], out[idx] + r, r)
        touched[idx] = True
    return out.reshape(-1)


def dagger(terms):
    """O^+ of a term list: conjugated coefficients (and both flags inverted, which is the caller's part)"""
    return [(i, j, np.conj(complex(c))) for i, j, c in terms]


def lehmann_chi(e_state, raise_side, lower_side, z):
    """chi[z, a, b] = -[ sum_n <O_a^+ psi|n><n|O_b^+ psi> / (z - e_n)  -  sum_m <O_b psi|m><m|O_a psi> / (z + e_m) ],  e = E_level - e_state.
    raise_side = (w, U, [O_a^+ psi]) over the dense spectrum of the sector O^+ reaches, lower_side the same with [O_a psi] for the sector O
    reaches; either may be None (the sector does not exist): its sum is zero."""
    z = np.asarray(z, dtype=complex)
    nops = len((raise_side or lower_side)[2])
    chi = np.zeros((z.size, nops, nops), dtype=complex)
    if raise_side is not None:
        w, U, vecs = raise_side
        A = U.conj().T @ np.stack(vecs, axis=1)                  # <n|O_a^+ psi>
        chi -= np.einsum("zn,na,nb->zab", 1.0 / (z[:, None] - (w - e_state)), A.conj(), A)
    if lower_side is not None:
        w, U, vecs = lower_side
        B = U.conj().T @ np.stack(vecs, axis=1)                  # <m|O_a psi>
        chi += np.einsum("zm,mb,ma->zab", 1.0 / (z[:, None] + (w - e_state)), B.conj(), B)
    return chi


# ---- explicit Fock-space matrices (Jordan-Wigner, Kronecker products) for small Ns: the check of the restatement itself -------------------
def fock_c(nmodes, k):
    """c_k on nmodes fermionic modes, basis index = sum_k n_k 2^k, sign (-1)^(occupied modes below k)"""
    a = np.array([[0.0, 1.0], [0.0, 0.0]])
    zs = np.diag([1.0, -1.0])
    op = np.ones((1, 1))
    for m in range(nmodes - 1, -1, -1):                          # mode 0 is the fastest index: it goes last into the Kronecker product
        op = np.kron(op, a if m == k else (zs if m < k else np.eye(2)))
    return op


def fock_index(maps, ns):
    """Fock index of every state of the sector in the reference's layout, modes: up orbital o = mode o, dw orbital o = mode ns + o"""
    mu, md = np.asarray(maps[0], dtype=np.int64), np.asarray(maps[1], dtype=np.int64)
    return (mu[None, :] + (md[:, None] << ns)).reshape(-1)


def fock_operator(ns, terms, create_up, create_dw):
    """sum_t coef_t X_t Y_t as a 4^ns x 4^ns matrix of true fermionic operators (X to the left of Y)"""
    n = 2 * ns
    op = np.zeros((2 ** n, 2 ** n), dtype=complex)
    for ou, od, cf in terms:
        x, y = fock_c(n, ou), fock_c(n, ns + od)
        op += complex(cf) * ((x.T if create_up else x) @ (y.T if create_dw else y))
    return op


def sector_maps(ns, nup, ndw):
    cfg = np.arange(2 ** ns)
    pop = np.array([bin(int(c)).count("1") for c in cfg])
    return cfg[pop == nup], cfg[pop == ndw]


# ---- the fixtures of the susceptibility checks (tests/test_spin_pair_ref_cpu.py asserts their properties on the CPU) ----------------------
def chi_fixture(name):
    """-> (model, (nup, ndw), real).  xmu is chosen (and recorded here) so that no level of a neighbouring sector lies within 1e-2 of the
    chosen sector's ground state: nu_0 = 0 is then a fair point of the Lehmann sums.  min|e_n| over the sectors each check uses:
    plaquette (2,2), xmu 0.3: 2.08 (pair), 0.296 (spin flip); chain (3,3), xmu 0.3: 0.328, 0.484; square (Ns = 8) (1,1), xmu -2.0: 0.192
    (pair); bhz (1,1), xmu -3.0: 0.661 (pair).  The square and BHZ clusters are used with the pair operators only, in a sector small
    enough for a dense spectrum of its neighbour (2,2), Dim 784."""
    from hxv import models

    return {"plaquette": lambda: (models.plaquette_2x2_nobath(U=4.0, t=1.0, hfmode=True, xmu=0.3), (2, 2), True),
            "chain": lambda: (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0, xmu=0.3), (3, 3), True),
            "square": lambda: (models.hm_2dsquare(Nbath=1, xmu=-2.0), (1, 1), True),
            "bhz": lambda: (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1, xmu=-3.0), (1, 1), False)}[name]()


def neighbours(ns, nup, ndw):
    """the four sectors an operator of this family reaches, None where nup or ndw leaves [0, Ns]: keys (dup, ddw)"""
    return {(du, dd): ((nup + du, ndw + dd) if 0 <= nup + du <= ns and 0 <= ndw + dd <= ns else None) for du in (-1, 1) for dd in (-1, 1)}


_DENSE = {}


def dense_sector(model, nup, ndw):
    """(w, U, (map_up, map_dw)) of a sector from the oracle's dense matrix, computed once per (model name, xmu, sector)"""
    from oracle.oracle import OracleSector

    key = (model.name, float(model.xmu), nup, ndw)
    if key not in _DENSE:
        orc = OracleSector(model, nup, ndw)
        w, U = np.linalg.eigh(orc.dense())
        _DENSE[key] = (w, U, (np.array(orc.map_up()), np.array(orc.map_dw())))
        orc.close()
    return _DENSE[key]


def real_gauge(psi):
    psi = np.real(psi * np.exp(-1j * np.angle(psi[np.abs(psi).argmax()]))).astype(np.complex128)
    return psi / np.linalg.norm(psi)
