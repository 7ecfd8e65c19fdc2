"""The twin-sector map (include/hxv.h: hxv_twin_vector) without a GPU: the numpy restatement of the reference's definition
(tests/twin_ref.py) is the transpose of the amplitude matrix; H of sector (ndw,nup) is T H T^t of sector (nup,ndw) for spin-symmetric models
and is not for complex BHZ with a spin-orbit term; the kernel file keeps the register / scratch budgets and passes the ISA lint of
tests/test_kernel_resources.py; the built library exports the entry point."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import isa_lint
import twin_ref
from test_kernel_resources import MAX_SCRATCH_BYTES, MAX_VGPR_SPILL


def _models():
    from hxv import models

    return {
        "chain_eps": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.15), (2, 4)),
        "chain_nohf": (models.hm_1dchain(Nlat=2, Nbath=1, hfmode=False, xmu=0.3), (1, 3)),
        "bhz_site": (models.bhz_2d(Nx=1, Ny=1, Nbath=2), (1, 3)),
        "bhz_site_jxjp": (models.bhz_2d(Nx=1, Ny=1, Nbath=2, Ust=1.0, Jh=0.3, Jx=0.3, Jp=0.3), (2, 4)),
    }


def _ns(m):
    return m.Nlat * m.Norb * (1 + m.Nbath)


@pytest.mark.parametrize("ns,nup,ndw", [(6, 1, 3), (6, 2, 4), (6, 0, 3), (8, 3, 5)])
def test_the_reference_order_is_the_transpose_of_the_amplitude_matrix(ns, nup, ndw):
    from hxv import models
    from oracle.oracle import OracleSector

    m = models.hm_1dchain(Nlat=2, Nbath={6: 2, 8: 3}[ns], eps_bath=None)
    assert _ns(m) == ns
    a, b = OracleSector(m, nup, ndw), OracleSector(m, ndw, nup)
    assert np.array_equal(a.map_up(), b.map_dw()) and np.array_equal(a.map_dw(), b.map_up())
    order = twin_ref.twin_order(a.map_up(), a.map_dw(), ns)
    assert sorted(order.tolist()) == list(range(a.Dim))
    rng = np.random.default_rng(ns * 100 + nup * 10 + ndw)
    v = rng.standard_normal(a.Dim) + 1j * rng.standard_normal(a.Dim)
    assert np.array_equal(v[order], v.reshape(a.DimDw, a.DimUp).T.ravel())
    assert np.array_equal(twin_ref.twin_matrix(a.map_up(), a.map_dw(), ns) @ v, v[order])


@pytest.mark.parametrize("name", ["chain_eps", "chain_nohf", "bhz_site", "bhz_site_jxjp"])
def test_twin_sector_hamiltonian_is_the_transposed_one_for_spin_symmetric_models(name):
    from oracle.oracle import OracleSector

    m, (nup, ndw) = _models()[name]
    a, b = OracleSector(m, nup, ndw), OracleSector(m, ndw, nup)
    t = twin_ref.twin_matrix(a.map_up(), a.map_dw(), _ns(m))
    diff = np.abs(b.dense() - t @ a.dense() @ t.T).max()
    print(name, "max |H_B - T H_A T^t| =", diff)
    assert diff <= 1e-13


def test_twin_sector_hamiltonian_differs_without_spin_symmetry():
    """complex BHZ with lam != 0: the spin blocks differ, so the check above can fail"""
    from hxv import models
    from oracle.oracle import OracleSector

    m = models.bhz_2d(Nx=2, Ny=1, Nbath=1, lam=0.3, Ust=0.5, Jh=0.2)
    a, b = OracleSector(m, 2, 3), OracleSector(m, 3, 2)
    t = twin_ref.twin_matrix(a.map_up(), a.map_dw(), _ns(m))
    diff = np.abs(b.dense() - t @ a.dense() @ t.T).max()
    print("max |H_B - T H_A T^t| =", diff)
    assert diff > 0.1


@pytest.fixture(scope="module")
def twin_asm(tmp_path_factory):
    if not Path(isa_lint.HIPCC).exists():
        pytest.skip("hipcc not available")
    return isa_lint.compile_to_asm(isa_lint.CSRC / "hxv_twin.hip", tmp_path_factory.mktemp("isa") / "hxv_twin.hip.s")


def test_twin_kernel_budgets(twin_asm):
    md = isa_lint.kernel_metadata(twin_asm)
    assert md, "no kernel metadata found"
    for name, d in md.items():
        assert d.get("vgpr_spill_count", 0) <= MAX_VGPR_SPILL and d.get("private_segment_fixed_size", 0) <= MAX_SCRATCH_BYTES, (isa_lint.demangle(name), d)


def test_twin_kernel_has_no_vector_instruction_with_exec_zero(twin_asm):
    n, found = 0, []
    for name, body in isa_lint.kernel_bodies(twin_asm):
        n += 1
        found += [(isa_lint.demangle(name), x) for x in isa_lint.exec0_findings(body)]
    assert n > 0
    assert not found, found


def test_library_exports_the_twin_entry(built):
    import hxv

    assert "hxv_twin_vector" in hxv.EXPORTS
    assert hasattr(ctypes.CDLL(str(hxv.LIB_PATH)), "hxv_twin_vector")
