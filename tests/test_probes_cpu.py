"""Probe overlaps -> poles and weights without a GPU (include/hxv.h: hxv_gf_from_probes; hxv.greens): the library's host code against
numpy.linalg.eigh and a dense solve of (z - T) on synthetic tridiagonal matrices; argument errors; both new symbols exported."""
import ctypes

import numpy as np
import pytest


def _tridiag(a, b):
    return np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)


def _case(name):
    rng = np.random.default_rng({"n1": 1, "n2": 2, "n37": 37, "breakdown": 4, "complex": 5}[name])
    n = {"n1": 1, "n2": 2}.get(name, 37)
    a = rng.standard_normal(n)
    b = np.abs(rng.standard_normal(n)) + 0.1
    b[0] = 0.0                                   # blanc(1) is unused (ED_GF_NORMAL.f90:949-951)
    if name == "breakdown":
        b[11] = 0.0                              # a zero inside: T is two blocks
    npr = 3
    ov = rng.standard_normal((n, npr)).astype(np.complex128)
    if name in ("complex", "n2"):
        ov = ov + 1j * rng.standard_normal((n, npr))
    return a, b, ov, 1.7


@pytest.mark.parametrize("name", ["n1", "n2", "n37", "breakdown", "complex"])
def test_poles_and_weights_match_eigh_and_a_dense_solve(built, name):
    from hxv import greens

    a, b, ov, norm = _case(name)
    n = a.size
    poles, w = greens.poles_weights(a, b, ov, norm)
    T = _tridiag(a, b)
    assert poles.shape == (n,) and w.shape == ov.shape
    assert np.abs(poles - np.linalg.eigvalsh(T)).max() <= 1e-12
    # sum_n w[n, j] / (z - poles[n]) = norm * sum_k o_kj [(z - T)^-1]_{k,1} at 16 complex z (off the real axis: Matsubara-like and generic)
    rng = np.random.default_rng(99)
    zs = np.concatenate([1j * np.pi / 50.0 * (2 * np.arange(1, 9) - 1), rng.standard_normal(8) + 1j * (0.3 + np.abs(rng.standard_normal(8)))])
    assert zs.size == 16
    got = greens.evaluate(poles, w, zs, 0.0, 1.0)
    for iz, z in enumerate(zs):
        col = np.linalg.solve(z * np.eye(n) - T, np.eye(n)[:, 0])
        ref = norm * (ov * col[:, None]).sum(axis=0)
        assert np.abs(got[iz] - ref).max() <= 1e-12, (name, z, np.abs(got[iz] - ref).max())
    # the diagonal: a probe equal to the start vector has o = (norm, 0, 0, ...) and the reference's weights norm^2 Z_1n^2 (:958-973)
    o0 = np.zeros((n, 1), dtype=np.complex128)
    o0[0, 0] = norm
    _, w0 = greens.poles_weights(a, b, o0, norm)
    ev, Z = np.linalg.eigh(T)
    assert np.abs(np.sort(w0[:, 0].real) - np.sort(norm ** 2 * Z[0, :] ** 2)).max() <= 1e-12 and np.abs(w0.imag).max() == 0.0


def test_evaluate_applies_the_pole_convention(built):
    from hxv import greens

    poles, w = np.array([0.5, 2.0]), np.array([[1.0 + 0j], [0.25 + 0j]])
    z = np.array([0.3j, 1.1j])
    for sign in (1.0, -1.0):
        ref = sum(w[n, 0] / (z - sign * (poles[n] - 0.2)) for n in range(2))
        assert np.abs(greens.evaluate(poles, w, z, 0.2, sign)[:, 0] - ref).max() < 1e-15


def test_gf_from_probes_argument_errors(built):
    import hxv

    L = hxv.load_library()
    pd = ctypes.POINTER(ctypes.c_double)
    a, b, ov = np.zeros(3), np.zeros(3), np.zeros(6)
    poles, w = np.zeros(3), np.zeros(6)
    ptr = lambda x: x.ctypes.data_as(pd)  # noqa: E731
    null = ctypes.cast(None, pd)
    assert L.hxv_gf_from_probes(3, ptr(a), ptr(b), 1, ptr(ov), 1.0, ptr(poles), ptr(w)) == 0
    assert L.hxv_gf_from_probes(3, ptr(a), ptr(b), 0, null, 1.0, ptr(poles), null) == 0         # no probe: poles only
    for args in ((0, ptr(a), ptr(b), 1, ptr(ov), 1.0, ptr(poles), ptr(w)),
                 (3, null, ptr(b), 1, ptr(ov), 1.0, ptr(poles), ptr(w)),
                 (3, ptr(a), null, 1, ptr(ov), 1.0, ptr(poles), ptr(w)),
                 (3, ptr(a), ptr(b), 1, null, 1.0, ptr(poles), ptr(w)),
                 (3, ptr(a), ptr(b), 1, ptr(ov), 1.0, null, ptr(w)),
                 (3, ptr(a), ptr(b), 1, ptr(ov), 1.0, ptr(poles), null),
                 (3, ptr(a), ptr(b), -1, ptr(ov), 1.0, ptr(poles), ptr(w))):
        assert L.hxv_gf_from_probes(*args) == 1                                                 # HXV_ERR_ARG
        assert b"hxv_gf_from_probes" in L.hxv_last_error()
    with pytest.raises(hxv.HxvError):
        hxv.greens.poles_weights(np.zeros(0), np.zeros(0), np.zeros((0, 1)), 1.0)


def test_new_symbols_are_exported(built):
    import hxv

    lib = ctypes.CDLL(str(hxv.LIB_PATH))
    for name in ("hxv_lanczos_tridiag_probes", "hxv_gf_from_probes"):
        assert name in hxv.EXPORTS and hasattr(lib, name)
    # a NULL handle is refused before the device is touched
    assert hxv.load_library().hxv_lanczos_tridiag_probes(None, None, 0, None, 1, None, None, None, 1e-12, None) == 1
