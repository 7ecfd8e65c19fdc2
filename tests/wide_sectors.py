"""Sectors with a one-spin dimension above 65535, and their oracle answers, shared by tests/test_gpu_wide_sectors.py.

ED_DIAG walks every sector of a model, so an Ns = 20 solve opens (10,0), (10,1), (1,10), ...: skinny sectors, one spin dimension 184 756 and
the other 1 to 20.  The CPU oracle answers for them in seconds, and they are the cheapest inputs that put tables of that size in front of the
kernels.  Every sector here is a real sector of a real model; nothing is synthetic.

  "S" sectors  one spin has no particle (or, Ns 22 (2,1), is tiny): one pass only, Dim <= 184 756, an oracle product costs 0.1 s
  "P" sectors  both passes, Dim 2.7e6 to 3.7e6
  "G"          the one plan on the far side of the job kernel's DimUp < 65536 gate (see GATE below)

`oracle(name)` opens the OracleSector once per process and keeps it with ONE reference product of models.deterministic_vector(Dim); tests
leave both unchanged.  `record_numpy_fast` is tests/observables_ref.py's record_numpy without its Python loop over basis states
(tests/test_wide_sectors_ref_cpu.py holds the two equal on small sectors)."""
import time

import numpy as np

MODELS = {
    "chain20": lambda M: M.hm_1dchain(Nlat=4, Nbath=4),                                 # Ns 20, real H, one orbital
    "chain22": lambda M: M.hm_1dchain(Nlat=2, Nbath=10),                                # Ns 22: the host builds without the 2^Ns lookup table
    "bhz24": lambda M: M.bhz_2d(Nbath=2, Ust=0.5, Jh=0.1, Jx=0.1, Jp=0.1),              # Ns 24, complex H, spH0nd live where both spins have particles
    # Ns 20: every bath orbital hops to the one site only; distinct bath levels, or H moves a vector inside a six-dimensional Krylov space
    "star20": lambda M: M.hm_1dchain(Nlat=1, Nbath=19, eps_bath=[(k - 9) / 10 for k in range(19)]),
}
# name -> (model, nup, ndw)
SECTORS = {
    "ns20_10_0": ("chain20", 10, 0), "ns20_0_10": ("chain20", 0, 10), "ns24_6_0": ("bhz24", 6, 0), "ns22_2_1": ("chain22", 2, 1),
    "ns20_10_1": ("chain20", 10, 1), "ns20_1_10": ("chain20", 1, 10), "ns24_6_1": ("bhz24", 6, 1), "ns24_1_6": ("bhz24", 1, 6),
    "star20_10_1": ("star20", 10, 1),
    "ns20_1_9": ("chain20", 1, 9),       # source of the split dw ladder into (1,10); no oracle answer is needed for it
}
S_SECTORS = ["ns22_2_1", "ns20_10_0", "ns20_0_10", "ns24_6_0"]
P_SECTORS = ["ns20_10_1", "ns20_1_10", "ns24_6_1", "ns24_1_6"]
DRIVER_SECTORS = ["ns20_10_0", "ns20_0_10", "ns24_6_0"]
# GATE.  job_up_usable (csrc/hxv_tile_plan.cpp) lets pass A run as jobs only where the up blocks have at most 960 rows and 8 out-of-block
# partners AND DimUp < 65536 (hxv_up_job packs out-of-block rows into 16-bit-scaled fields).  A block's partner count is at least the number
# of high orbitals that hop to a low one, and 65536 / 960 > 64 blocks need 7 high orbitals or more: only a model whose high orbitals have ONE
# hop each gets there.  The star (one site, 19 bath orbitals) with 12 low bits does: 256 blocks of at most C(12,6) = 924 rows, 8 partners.
# With "job_max_blocks" raised to 256 the DimUp gate is then the only one that says no.
GATE_SECTOR = "star20_10_1"
GATE_OPTIONS = (("tile_bits_up", 12), ("job_max_blocks", 256), ("job_up", 1))
LADDER_SOURCES = ["ns20_1_9"]

_MODELS, _ORACLE, _EIG = {}, {}, {}
ORACLE_SECONDS = {}         # name -> (open, product): what the cache cost, for the lab notes


def model(key):
    if key not in _MODELS:
        from hxv import models

        _MODELS[key] = MODELS[key](models)
    return _MODELS[key]


def sector(name):
    """-> (model, nup, ndw)"""
    key, nup, ndw = SECTORS[name]
    return model(key), nup, ndw


def oracle(name):
    """-> (OracleSector, v = deterministic_vector(Dim), the oracle's H v), opened and computed once per process"""
    if name not in _ORACLE:
        from hxv import models
        from oracle.oracle import OracleSector

        m, nup, ndw = sector(name)
        t0 = time.perf_counter()
        orc = OracleSector(m, nup, ndw)
        t1 = time.perf_counter()
        v = models.deterministic_vector(orc.Dim)
        ref = orc.spMatVec_main(v)
        ORACLE_SECONDS[name] = (t1 - t0, time.perf_counter() - t1)
        print(f"oracle {name}: {orc.DimUp} x {orc.DimDw}, open {t1 - t0:.1f} s, vector and product {time.perf_counter() - t1:.1f} s")
        v.setflags(write=False)
        ref.setflags(write=False)
        _ORACLE[name] = (orc, v, ref)
    return _ORACLE[name]


def oracle_matrix(name):
    """the oracle's whole H of an S sector as a scipy CSR matrix: diagonal + the one-spin matrix of the spin that has particles (+ spH0nd)"""
    import scipy.sparse as sp

    orc, _, _ = oracle(name)
    assert orc.DimUp == 1 or orc.DimDw == 1, name
    which = "up" if orc.DimDw == 1 else "dw"
    rp, cols, vals = orc.csr(which)
    H = sp.diags(orc.diag()) + sp.csr_matrix((vals, cols - 1, rp), shape=(orc.Dim, orc.Dim))
    rp, cols, vals = orc.csr("nd")
    if rp[-1]:
        H = H + sp.csr_matrix((vals, cols - 1, rp), shape=(orc.Dim, orc.Dim))
    return H.tocsr()


def extremal_eigenvalues(name):
    """(E0, max|w|) of an S sector from scipy's ARPACK on oracle_matrix, once per process"""
    if name not in _EIG:
        import scipy.sparse.linalg as sla

        H = oracle_matrix(name)
        t0 = time.perf_counter()
        e0 = float(sla.eigsh(H, k=1, which="SA", tol=1e-12)[0][0])
        top = float(sla.eigsh(H, k=1, which="LA", tol=1e-8)[0][0])
        print(f"eigsh {name}: E0 {e0:.12f}, top {top:.6f}, {time.perf_counter() - t0:.1f} s")
        _EIG[name] = (e0, max(abs(e0), abs(top)))
    return _EIG[name]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _parity_below(x, pos):
    """popcount(x & ((1 << pos) - 1)) & 1 on an int64 array"""
    p = np.zeros(x.shape, dtype=np.int64)
    for b in range(pos):
        p ^= (x >> b) & 1
    return p


def record_numpy_fast(model, map_up, map_dw, psi, weight=1.0):
    """observables_ref.record_numpy with its loop over basis states turned into array operations per ordered orbital pair: the same W
    histogram, R_s[is, js] = sum over the states with js occupied and is empty of sign * <psi at the state | psi at its partner>"""
    N = model.Nlat * model.Norb
    nw = 1 << N
    mu, md = np.asarray(map_up, dtype=np.int64), np.asarray(map_dw, dtype=np.int64)
    P = np.asarray(psi, dtype=np.complex128).reshape(len(md), len(mu))  # [idw, iup]
    A = np.abs(P) ** 2
    W = np.zeros((nw, nw))  # [a_dw, a_up]
    np.add.at(W, ((md & (nw - 1))[:, None], (mu & (nw - 1))[None, :]), A)
    R = np.zeros((2, N, N), dtype=np.complex128)
    for spin, conf in ((0, mu), (1, md)):
        for js in range(N):
            for is_ in range(N):
                if is_ == js:
                    continue
                sel = np.flatnonzero((((conf >> js) & 1) == 1) & (((conf >> is_) & 1) == 0))
                if not sel.size:
                    continue
                r = conf[sel] ^ (1 << js)
                k = r | (1 << is_)
                pos = np.searchsorted(conf, k)
                assert np.array_equal(conf[pos], k)
                sg = np.where((_parity_below(conf[sel], js) ^ _parity_below(r, is_)) != 0, -1.0, 1.0)
                if spin == 0:
                    R[0, is_, js] = np.sum(sg * np.sum(P[:, sel] * np.conj(P[:, pos]), axis=0))
                else:
                    R[1, is_, js] = np.sum(sg * np.sum(P[sel, :] * np.conj(P[pos, :]), axis=1))
    for s in range(N):
        R[0, s, s] = A[:, ((mu >> s) & 1) == 1].sum()
        R[1, s, s] = A[((md >> s) & 1) == 1, :].sum()
    return weight * np.concatenate([W.ravel(), R[0].ravel(order="F").view(np.float64), R[1].ravel(order="F").view(np.float64)])


def ladder_numpy(psi, maps_from, maps_to, pos, spin, create):
    """ladder_ref.apply_op (ED_GF_NORMAL.f90:180-199) with its loop over source states turned into one signed gather; exact: every target
    element is +-one source element or +0.0"""
    mu_f, md_f = (np.asarray(x, dtype=np.int64) for x in maps_from)
    mu_t, md_t = (np.asarray(x, dtype=np.int64) for x in maps_to)
    P = np.asarray(psi, dtype=np.complex128).reshape(len(md_f), len(mu_f))      # [idw, iup]
    out = np.zeros((len(md_t), len(mu_t)), dtype=np.complex128)
    src, dst = (mu_f, mu_t) if spin == 0 else (md_f, md_t)
    bit = 1 << pos
    live = np.flatnonzero(((src & bit) != 0) != bool(create))
    t = np.searchsorted(dst, src[live] ^ bit)
    assert np.array_equal(dst[t], src[live] ^ bit)
    sg = np.where(_parity_below(src[live], pos) != 0, -1.0, 1.0)
    if spin == 0:
        out[:, t] = P[:, live] * sg[None, :]
    else:
        out[t, :] = P[live, :] * sg[:, None]
    return out.reshape(-1)
