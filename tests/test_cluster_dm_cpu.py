"""The cluster reduced density matrix without a device: the two restatements of tests/cluster_dm_ref.py against each other, against the merged
observables record (its W is the diagonal, its R_s a signed sum of off-diagonal elements) and against the closed form of a Slater
determinant; and the C-ABI's presence in the header and the library."""
import re
from pathlib import Path

import numpy as np
import pytest

from cluster_dm_ref import entropy_and_purity, gaussian_entropy_and_purity, literal, nimp_of, vectorised
from observables_ref import _pairs, record_numpy


def _maps(m, nup, ndw):
    from oracle.oracle import OracleSector

    o = OracleSector(m, nup, ndw)
    mu, md = o.map_up(), o.map_dw()
    o.close()
    return mu, md


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


def _cases():
    from hxv import models

    return [(models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1), 4, 3), (models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=0.0), 4, 4)]


@pytest.fixture(scope="module")
def matrices(built):
    """(model, maps, vector, vectorised matrix) of the two models, computed once"""
    out = []
    for k, (m, nup, ndw) in enumerate(_cases()):
        mu, md = _maps(m, nup, ndw)
        v = _rand(len(mu) * len(md), 11 + k)
        out.append((m, mu, md, v, vectorised(m, mu, md, v, 0.7)))
    return out


def test_literal_equals_vectorised(matrices):
    for m, mu, md, v, rho in matrices:
        ref = literal(m, [(mu, md, v, 0.7)])
        assert np.abs(rho - ref).max() < 1e-14
        assert np.abs(rho - rho.conj().T).max() < 1e-15 and abs(np.trace(rho) - 0.7) < 1e-14


def test_diagonal_is_the_records_histogram(matrices):
    for m, mu, md, v, rho in matrices:
        n = 4 ** nimp_of(m)
        rec = record_numpy(m, mu, md, v, 0.7)
        assert np.abs(np.diag(rho).real - rec[:n]).max() < 1e-14 and np.abs(np.diag(rho).imag).max() < 1e-15


def test_records_r_is_a_signed_sum_of_off_diagonal_elements(matrices):
    """R_s(is,js) = sum sgn * rho(io,jo), |jo> = c^+_is c_js |io> on spin s, the other spin's impurity bits traced: the new matrix carries the
    sign convention of the merged record (no sign between the spins)."""
    for m, mu, md, v, rho in matrices:
        N = nimp_of(m)
        nw = 1 << N
        rec = record_numpy(m, mu, md, v, 0.7)
        for spin in (0, 1):
            R = rec[nw * nw + 2 * N * N * spin: nw * nw + 2 * N * N * (spin + 1)].view(np.complex128).reshape(N, N, order="F")
            got = np.zeros((N, N), dtype=np.complex128)
            for a in range(nw):
                for is_, js, k, sg in _pairs(a, N):
                    for other in range(nw):
                        io, jo = (a + nw * other, k + nw * other) if spin == 0 else (other + nw * a, other + nw * k)
                        got[is_, js] += sg * rho[io, jo]
            off = ~np.eye(N, dtype=bool)
            assert np.abs(got[off] - R[off]).max() < 1e-14


@pytest.mark.parametrize("kind", ["chain", "bhz"])
def test_closed_form_of_a_slater_determinant(built, kind):
    from hxv import models
    from onebody import slater_vector

    if kind == "chain":
        m, nup, ndw, lu, ld = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1, U=0.0), 4, 3, (0, 1, 2, 4), (0, 2, 3)
    else:
        m, nup, ndw, lu, ld = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=0.0), 4, 4, (0, 1, 2, 3), (0, 1, 3, 5)
    mu, md = _maps(m, nup, ndw)
    v, _ = slater_vector(m, mu, md, lu, ld)
    S, pur = entropy_and_purity(vectorised(m, mu, md, v))
    S0, pur0 = gaussian_entropy_and_purity(m, lu, ld)
    assert abs(S - S0) < 1e-12 and abs(pur - pur0) < 1e-12, (S - S0, pur - pur0)


def test_the_c_abi_is_declared_and_exported(built):
    import ctypes as C

    import hxv

    hdr = (Path(__file__).resolve().parents[1] / "include" / "hxv.h").read_text()
    assert re.search(r"int64_t\s+hxv_cluster_dm_elems\s*\(\s*const hxv_handle\s*\*", hdr)
    assert re.search(r"int\s+hxv_cluster_dm_accumulate\s*\(\s*hxv_handle\s*\*", hdr)
    L = hxv.load_library()
    assert "hxv_cluster_dm_elems" in hxv.engine.EXPORTS and "hxv_cluster_dm_accumulate" in hxv.engine.EXPORTS
    assert L.hxv_cluster_dm_elems(None) == 0
    assert L.hxv_cluster_dm_accumulate(None, None, C.c_double(1.0), 0, None) == 1   # HXV_ERR_ARG before anything touches a device
