"""The reduced density matrix of an impurity-orbital subset without a device: the reference's masked trace restated literally
(tests/reduced_dm_ref.py) against the matrix computed from the vector, the reference's sign factor shown to be +1 on every contributing
pair, the closed form of a Slater determinant in both sign conventions, and the C-ABI's presence in the header and the library."""
import re
from pathlib import Path

import numpy as np
import pytest

from cluster_dm_ref import entropy_and_purity, literal, nimp_of, vectorised
from reduced_dm_ref import direct, gaussian_entropy_and_purity_subset, masked_trace_literal
from test_cluster_dm_cpu import _cases, _maps, _rand

MASKS = [(0,), (0, 1), (0, 2), (1, 3), (0, 2, 3), (0, 1, 2, 3)]
SLATER_MASKS = [(0,), (0, 1), (1, 2, 3), (0, 2), (1, 3), (0, 3), (0, 2, 3), (0, 1, 2, 3)]
# the reference's convention misses the closed form on these (entropy gaps of 2e-2 to 2.6e-1, printed by the test) ...
REFERENCE_SIGN_MISSES = [(0, 2), (0, 3)]
# ... and meets it on these: no traced impurity orbital lies between two reduced ones
REFERENCE_SIGN_MATCHES = [(0, 1), (1, 2, 3)]


@pytest.fixture(scope="module")
def dense(built):
    """(model, maps, vector, literal cluster matrix) of the two models of test_cluster_dm_cpu.py, weight 0.7, computed once"""
    out = []
    for k, (m, nup, ndw) in enumerate(_cases()):
        mu, md = _maps(m, nup, ndw)
        v = _rand(len(mu) * len(md), 11 + k)
        out.append((m, mu, md, v, literal(m, [(mu, md, v, 0.7)])))
    return out


def _slater(kind):
    from hxv import models
    from onebody import slater_vector

    if kind == "chain":
        m, nup, ndw, lu, ld = models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3], xmu=0.1, U=0.0), 4, 3, (0, 1, 2, 4), (0, 2, 3)
    else:
        m, nup, ndw, lu, ld = models.bhz_2d(Nx=2, Ny=1, Nbath=1, U=0.0), 4, 4, (0, 1, 2, 3), (0, 1, 3, 5)
    mu, md = _maps(m, nup, ndw)
    v, _ = slater_vector(m, mu, md, lu, ld)
    return m, mu, md, v, lu, ld


@pytest.mark.parametrize("mask", MASKS)
def test_the_references_masked_trace_is_the_plain_partial_trace(dense, mask):
    """masked_trace_literal(literal cdm) == direct(fermi_sign=0), and the reference's sign product is +1 on every pair that contributes."""
    for m, mu, md, v, cdm in dense:
        ref, signs = masked_trace_literal(cdm, nimp_of(m), mask)
        got = direct(m, mu, md, v, mask, 0.7, 0)
        assert got.shape == ref.shape == (4 ** len(mask),) * 2
        assert np.abs(got - ref).max() < 1e-14
        assert signs == {1.0}, signs


def test_hermitian_trace_and_the_full_mask(dense):
    for m, mu, md, v, _ in dense:
        for fs in (0, 1):
            for mask in MASKS:
                rho = direct(m, mu, md, v, mask, 0.7, fs)
                assert np.abs(rho - rho.conj().T).max() < 1e-15 and abs(np.trace(rho) - 0.7) < 1e-14
            full = direct(m, mu, md, v, range(nimp_of(m)), 0.7, fs)
            assert np.abs(full - vectorised(m, mu, md, v, 0.7)).max() < 1e-14


@pytest.mark.parametrize("kind", ["chain", "bhz"])
def test_closed_form_with_the_fermi_sign(built, kind):
    m, mu, md, v, lu, ld = _slater(kind)
    for mask in SLATER_MASKS:
        S, pur = entropy_and_purity(direct(m, mu, md, v, mask, 1.0, 1))
        S0, pur0 = gaussian_entropy_and_purity_subset(m, lu, ld, mask)
        print(kind, mask, "entropy error", S - S0, "purity error", pur - pur0)
        assert abs(S - S0) < 1e-12 and abs(pur - pur0) < 1e-12, (mask, S - S0, pur - pur0)


@pytest.mark.parametrize("kind", ["chain", "bhz"])
def test_closed_form_with_the_references_sign(built, kind):
    """The reference's numbers are physical for {0,1} and {1,2,3} and not for {0,2} and {0,3}."""
    m, mu, md, v, lu, ld = _slater(kind)
    for mask in REFERENCE_SIGN_MATCHES + REFERENCE_SIGN_MISSES:
        S, pur = entropy_and_purity(direct(m, mu, md, v, mask, 1.0, 0))
        S0, pur0 = gaussian_entropy_and_purity_subset(m, lu, ld, mask)
        print(kind, mask, "entropy gap", S - S0, "purity gap", pur - pur0)
        if mask in REFERENCE_SIGN_MATCHES:
            assert abs(S - S0) < 1e-12 and abs(pur - pur0) < 1e-12, (mask, S - S0)
        else:
            assert abs(S - S0) > 1e-2, (mask, S - S0)


def test_the_c_abi_is_declared_and_exported(built):
    import ctypes as C

    import hxv

    hdr = (Path(__file__).resolve().parents[1] / "include" / "hxv.h").read_text()
    assert re.search(r"int64_t\s+hxv_reduced_dm_elems\s*\(\s*const hxv_handle\s*\*\s*h\s*,\s*uint32_t", hdr)
    assert re.search(r"int\s+hxv_reduced_dm_accumulate\s*\(\s*hxv_handle\s*\*", hdr)
    L = hxv.load_library()
    assert "hxv_reduced_dm_elems" in hxv.engine.EXPORTS and "hxv_reduced_dm_accumulate" in hxv.engine.EXPORTS
    assert L.hxv_reduced_dm_elems(None, 1) == 0
    assert L.hxv_reduced_dm_accumulate(None, None, 1, 0, C.c_double(1.0), 0, None) == 1   # HXV_ERR_ARG before anything touches a device
