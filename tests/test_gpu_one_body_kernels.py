"""The kernels of hxv_apply_one_body (csrc/hxv_one_body_kernels.hpp) alone on the MI355X, on synthetic tables
(tests/device/one_body_kernels_check.hip), with integer-valued data so that every product and every sum is exact and is compared with ==.

Shapes: DimUp 5 (pitch 8); DimUp 300 (pitch 304: two row chunks, the last partial); 600 columns of DimUp 1021 (pitch 1024): 2400 work items,
more than the grid cap of 2048, so the grid-stride loop runs.  Tables: all dead, the identity, a signed permutation, 32 terms on one table,
mixed up and dw terms with a dw term dead for some columns.  The output starts as a sentinel with a guard element behind it and its pad rows
must come back as zeros; psi holds NaN in its pad rows.  A second run per case plants NaN in every element of psi that no table names as a
source as well: the thread's OWN element is still read for <psi|psi> and <psi|out> (that read is part of the kernel), so that run checks the
vector and <out|out> alone, which no unnamed source may reach.  Then the mean-subtraction pass, and two launches bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = complex(7.5, -7.25)                                       # (no integer-valued result is the sentinel)
SHAPES = {"tiny": (5, 3), "two_chunks": (300, 4), "grid_stride": (1021, 600)}      # (DimUp, columns)


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_one_body_kernels_check()))
    pu8, pi32, pd, vp, i, d = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p, C.c_int, C.c_double
    L.obk_run.argtypes = [i, i, pu8, pu8, pd, pi32, i, pi32, i, i, i, i, vp, vp, pd]
    L.obk_shift.argtypes = [i, d, d, i, i, i, vp, vp, pd]
    L.obk_grid.argtypes = [i, i]
    return L


def _pitch(n):
    return (n + 7) // 8 * 8


def _pack(src, neg):
    """source (or -1) and sign bit -> table words"""
    out = np.full(src.shape, -1, dtype=np.int32)
    live = src >= 0
    out[live] = ((src[live].astype(np.int64) | (neg[live].astype(np.int64) << 31)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return out


def _signed_perm(rng, n, live_frac=1.0):
    src = rng.permutation(n)
    src[rng.random(n) >= live_frac] = -1
    return _pack(src, rng.integers(0, 2, n))


def _identity(n):
    return _pack(np.arange(n), np.zeros(n, dtype=np.int64))


def _dead(n):
    return np.full(n, -1, dtype=np.int32)


def _tables(kind, rng, dimup, dimdw):
    """-> (up tables, dw tables, t_spin, t_tab, integer coefficients)"""
    ci = lambda n: (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)  # noqa: E731
    if kind == "dead":
        return [_dead(dimup)], [_dead(dimdw)], [0, 1], [0, 0], ci(2) + 1
    if kind == "identity":
        return [_identity(dimup)], [_identity(dimdw)], [0, 1], [0, 0], np.array([2.0 - 1.0j, 1.0 + 3.0j])
    if kind == "permutation":
        return [_signed_perm(rng, dimup)], [_dead(dimdw)], [0], [0], np.array([1.0 + 0.0j])
    if kind == "32_on_one":
        return [_signed_perm(rng, dimup, 0.8)], [_dead(dimdw)], [0] * 32, [0] * 32, ci(32)
    if kind == "mixed":
        up = [_signed_perm(rng, dimup, 0.7), _signed_perm(rng, dimup, 0.5), _signed_perm(rng, dimup, 0.3)]
        dw = [_signed_perm(rng, dimdw, 0.5), _signed_perm(rng, dimdw, 0.9)]
        dw[0][0] = -1                                            # dead for column 0 at every size
        return up, dw, [1, 0, 0, 1, 0, 1, 0], [0, 2, 0, 1, 1, 0, 2], ci(7)
    raise KeyError(kind)


def _reference(up, dw, t_spin, t_tab, coef, psi2):
    out = np.zeros_like(psi2)
    touched = np.zeros(out.shape, dtype=bool)
    named = np.zeros(out.shape, dtype=bool)                      # the elements of psi some term names as a source
    for s, k, cf in zip(t_spin, t_tab, coef):
        e = (dw if s else up)[k].astype(np.int64)
        live = np.nonzero(e != -1)[0]
        if not live.size:
            continue
        src, g = e[live] & 0x7FFFFFFF, np.where((e[live] >> 31) & 1, -1.0, 1.0)
        if s:
            x, g, idx = psi2[src, :], g[:, None], (live, slice(None))
            named[src, :] = True
        else:
            x, g, idx = psi2[:, src], g[None, :], (slice(None), live)
            named[:, src] = True
        r = g * (cf.real * x.real - cf.imag * x.imag) + 1j * (g * (cf.real * x.imag + cf.imag * x.real))
        out[idx] = np.where(touched[idx], out[idx] + r, r)
        touched[idx] = True
    return out, named


def _launch(lib, up, dw, t_spin, t_tab, coef, psi2, grid=0):
    """-> (out [dimdw][dimup] as the kernel left it, the four sums, the padded device psi and out)"""
    import torch

    dimdw, dimup = psi2.shape
    pitch = _pitch(dimup)
    padded = np.full((dimdw, pitch), complex(np.nan, np.nan))    # a pad row of psi is never read
    padded[:, :dimup] = psi2
    dpsi = torch.from_numpy(padded.reshape(-1)).cuda()
    dout = torch.full((dimdw * pitch + 1,), SENT, dtype=torch.complex128, device="cuda")     # + the guard element
    torch.cuda.synchronize()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    ts, tt = np.ascontiguousarray(t_spin, dtype=np.uint8), np.ascontiguousarray(t_tab, dtype=np.uint8)
    cf = np.ascontiguousarray(coef, dtype=np.complex128)
    upc, dwc = np.ascontiguousarray(np.stack(up), dtype=np.int32), np.ascontiguousarray(np.stack(dw), dtype=np.int32)
    sums = np.full(4, -1.0)
    g = grid if grid else lib.obk_grid(pitch, dimdw)
    rc = lib.obk_run(g, len(cf), p(ts, C.c_uint8), p(tt, C.c_uint8), p(cf.view(np.float64), C.c_double), p(upc, C.c_int32), len(up), p(dwc, C.c_int32),
                     len(dw), dimup, pitch, dimdw, dpsi.data_ptr(), dout.data_ptr(), p(sums, C.c_double))
    assert rc == 0, rc
    got = dout.cpu().numpy()
    assert got[-1] == SENT                                       # the guard element behind the output
    got = got[:-1].reshape(dimdw, pitch)
    assert not (got == SENT).any()                               # every element was written ...
    assert (got[:, dimup:].view(np.float64) == 0).all()          # ... pad rows as zeros
    return got[:, :dimup], sums, dpsi, dout, g


def _int_state(rng, dimdw, dimup):
    return (rng.integers(-5, 6, (dimdw, dimup)) + 1j * rng.integers(-5, 6, (dimdw, dimup))).astype(np.complex128)


@pytest.mark.parametrize("kind", ["dead", "identity", "permutation", "32_on_one", "mixed"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_vector_and_all_four_sums_are_exact(lib, shape, kind):
    dimup, dimdw = SHAPES[shape]
    rng = np.random.default_rng(len(kind) * 1000 + dimup)
    up, dw, t_spin, t_tab, coef = _tables(kind, rng, dimup, dimdw)
    psi2 = _int_state(rng, dimdw, dimup)
    ref, named = _reference(up, dw, t_spin, t_tab, coef, psi2)
    got, sums, _, _, grid = _launch(lib, up, dw, t_spin, t_tab, coef, psi2)
    assert np.array_equal(got, ref)
    ov = np.vdot(psi2, ref)
    want = [np.vdot(psi2, psi2).real, ov.real, ov.imag, np.vdot(ref, ref).real]
    assert sums.tolist() == want, (sums, want)
    if shape == "grid_stride":
        assert grid == 2048 < dimdw * 4                          # more work items than workgroups
    if kind == "dead":
        assert not ref.any() and sums[3] == 0.0
    else:
        assert ref.any()
    if (kind == "32_on_one" and shape != "tiny") or (kind == "mixed" and shape == "grid_stride"):
        assert not named.all()                                   # (there is something to plant)
    # the same with NaN in every element no table names as a source: neither the vector nor <out|out> may see one
    planted = psi2.copy()
    planted[~named] = complex(np.nan, np.nan)
    got, sums, _, _, _ = _launch(lib, up, dw, t_spin, t_tab, coef, planted)
    assert np.array_equal(got, ref) and sums[3] == want[3]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mean_subtraction_pass_is_exact_and_sums_the_norm_afresh(lib, shape):
    dimup, dimdw = SHAPES[shape]
    pitch = _pitch(dimup)
    rng = np.random.default_rng(dimup)
    up, dw, t_spin, t_tab, coef = _tables("mixed", rng, dimup, dimdw)
    psi2 = _int_state(rng, dimdw, dimup)
    ref, _ = _reference(up, dw, t_spin, t_tab, coef, psi2)
    _, _, dpsi, dout, grid = _launch(lib, up, dw, t_spin, t_tab, coef, psi2)
    m = complex(2.0, -3.0)
    n2 = C.c_double(-1.0)
    assert lib.obk_shift(grid, m.real, m.imag, dimup, pitch, dimdw, dpsi.data_ptr(), dout.data_ptr(), C.byref(n2)) == 0
    got = dout.cpu().numpy()
    assert got[-1] == SENT
    got = got[:-1].reshape(dimdw, pitch)
    want = ref - m * psi2                                        # integers: exact
    assert np.array_equal(got[:, :dimup], want)
    assert (got[:, dimup:].view(np.float64) == 0).all()          # the pad rows stay zero: psi's NaN pads were not read
    assert n2.value == np.vdot(want, want).real


def test_two_launches_give_the_same_bits(lib):
    dimup, dimdw = SHAPES["two_chunks"]
    rng = np.random.default_rng(4)
    up, dw, t_spin, t_tab, _ = _tables("mixed", rng, dimup, dimdw)
    coef = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    psi2 = rng.standard_normal((dimdw, dimup)) + 1j * rng.standard_normal((dimdw, dimup))
    a = _launch(lib, up, dw, t_spin, t_tab, coef, psi2)
    b = _launch(lib, up, dw, t_spin, t_tab, coef, psi2)
    ref, _ = _reference(up, dw, t_spin, t_tab, coef, psi2)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert np.abs(a[0] - ref).max() <= 4 * 8 * 2.0 ** -53 * np.abs(coef).sum() * np.abs(psi2).max()
    real = _launch(lib, up, dw, t_spin, t_tab, coef.real.astype(np.complex128), psi2.real.astype(np.complex128))
    assert (real[0].imag == 0).all() and real[0].real.any() and real[1][2] == 0.0    # a real state with real coefficients stays real


def test_launcher_refuses_what_could_leave_the_buffers(lib):
    import torch

    x = torch.zeros(64, dtype=torch.complex128, device="cuda")
    zero = np.zeros(1, dtype=np.uint8)
    cf, sums = np.ones(2), np.zeros(4)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731

    def call(up, dw, spin=zero, dimup=4, pitch=8, dimdw=2, grid=1):
        return lib.obk_run(grid, 1, p(spin, C.c_uint8), p(zero, C.c_uint8), p(cf, C.c_double), p(up, C.c_int32), 1, p(dw, C.c_int32), 1, dimup, pitch,
                           dimdw, x.data_ptr(), x.data_ptr() + 16 * 32, p(sums, C.c_double))

    up, dw = np.arange(4, dtype=np.int32), np.arange(2, dtype=np.int32)
    assert call(up, dw) == 0
    assert call(np.array([0, 1, 2, 4], dtype=np.int32), dw) == 1          # a source row outside the vector
    assert call(up, np.array([0, 2], dtype=np.int32)) == 1                # a source column outside the vector
    assert call(up, dw, spin=np.array([2], dtype=np.uint8)) == 1
    assert call(up, dw, pitch=4 + 1) == 1 and call(up, dw, pitch=2) == 1 and call(up, dw, grid=0) == 1 and call(up, dw, grid=4096) == 1
    n2 = C.c_double()
    assert lib.obk_shift(1, 1.0, 0.0, 4, 8, 2, x.data_ptr(), x.data_ptr(), C.byref(n2)) == 1        # in place
