"""The kernels of hxv_apply_spin_pair (csrc/hxv_spin_pair_kernels.hpp) alone on the MI355X, on synthetic tables
(tests/device/spin_pair_kernels_check.hip): dead tables, a single live column, random signed permutations, DimUp = 1, 7, 8, 9 and one size
with several row chunks, grids smaller than the work.  The output starts as a sentinel with a guard element behind it, the source holds NaN
in its pad rows.  Single-term coef = +-1 cases are compared as 64-bit patterns; several terms within
4 (nterms + 1) 2^-53 sum|coef| max|psi| (one rounding per product and per add, complex multiplication); the norm within 1e-13 relative."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = complex(7.0, -7.0)


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_spin_pair_kernels_check()))
    pu8, pi32, pd, vp, i = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p, C.c_int
    L.spk_run.argtypes = [i, i, i, pu8, pu8, pu8, pd, pi32, i, pi32, i, i, i, i, i, i, i, vp, vp, pd]
    L.spk_grid.argtypes = [i, i]
    return L


def _pitch(n):
    return (n + 7) // 8 * 8


def _signed_perm_table(rng, n_to, n_from, live_frac=1.0):
    """a random injective map target -> source with random signs; the targets beyond the sources (or dropped by live_frac) are dead"""
    tab = np.full(n_to, -1, dtype=np.int64)
    k = min(n_to, n_from)
    tgt = rng.permutation(n_to)[:k]
    src = rng.permutation(n_from)[:k]
    keep = rng.random(k) < live_frac
    tab[tgt[keep]] = src[keep] | (rng.integers(0, 2, keep.sum()) << 31)
    return _pack(tab)


def _pack(tab):
    out = np.full(tab.shape, -1, dtype=np.int32)
    live = tab >= 0
    out[live] = (tab[live] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return out


def _reference(up, dw, uq_tab, t_uq, t_dw, coef, psi2, dimup_to, dimdw_to):
    out = np.zeros((dimdw_to, dimup_to), dtype=np.complex128)
    touched = np.zeros(out.shape, dtype=bool)
    for t in range(len(coef)):
        e, d = up[uq_tab[t_uq[t]]].astype(np.int64), dw[t_dw[t]].astype(np.int64)
        lu, ld = np.nonzero(e != -1)[0], np.nonzero(d != -1)[0]
        if not lu.size or not ld.size:
            continue
        x = psi2[np.ix_(d[ld] & 0x7FFFFFFF, e[lu] & 0x7FFFFFFF)]
        sg = np.where((((d[ld] >> 31) & 1)[:, None] ^ ((e[lu] >> 31) & 1)[None, :]) == 1, -1.0, 1.0)
        cf = coef[t]
        r = sg * (cf.real * x.real - cf.imag * x.imag) + 1j * (sg * (cf.real * x.imag + cf.imag * x.real))
        idx = np.ix_(ld, lu)
        out[idx] = np.where(touched[idx], out[idx] + r, r)
        touched[idx] = True
    return out


def _run(lib, up, dw, uq_tab, t_uq, t_dw, coef, dimup_from, dimdw_from, grid, seed, real=False):
    import torch

    n_up, dimup_to = up.shape
    n_dw, dimdw_to = dw.shape
    rng = np.random.default_rng(seed)
    pf, pt = _pitch(dimup_from), _pitch(dimup_to)
    psi2 = rng.standard_normal((dimdw_from, dimup_from)) + (0.0 if real else 1j * rng.standard_normal((dimdw_from, dimup_from)))
    padded = np.full((dimdw_from, pf), complex(np.nan, np.nan))
    padded[:, :dimup_from] = psi2
    dpsi = torch.from_numpy(padded.reshape(-1)).cuda()
    dout = torch.full((dimdw_to * pt + 1,), SENT, dtype=torch.complex128, device="cuda")     # + the guard element
    torch.cuda.synchronize()
    n2 = C.c_double(-1.0)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)  # noqa: E731
    a_uq, a_tu, a_td = u8(uq_tab), u8(t_uq), u8(t_dw)
    cf = np.ascontiguousarray(coef, dtype=np.complex128)
    upc, dwc = np.ascontiguousarray(up, dtype=np.int32), np.ascontiguousarray(dw, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    g = grid if grid else lib.spk_grid(pt, dimdw_to)
    rc = lib.spk_run(g, len(cf), len(a_uq), p(a_uq, C.c_uint8), p(a_tu, C.c_uint8), p(a_td, C.c_uint8), p(cf.view(np.float64), C.c_double),
                     p(upc, C.c_int32), n_up, p(dwc, C.c_int32), n_dw, dimup_to, pt, dimdw_to, dimup_from, pf, dimdw_from, dpsi.data_ptr(),
                     dout.data_ptr(), C.byref(n2))
    assert rc == 0, rc
    got = dout.cpu().numpy()
    assert got[-1] == SENT                                       # the guard element behind the output
    got = got[:-1].reshape(dimdw_to, pt)
    assert not (got == SENT).any()                               # every element was written ...
    assert (got[:, dimup_to:].view(np.float64) == 0).all()       # ... pad rows as zeros
    ref = _reference(upc, dwc, a_uq, a_tu, a_td, cf, psi2, dimup_to, dimdw_to)
    return got[:, :dimup_to], ref, n2.value, np.abs(psi2).max()


DIMS = [1, 7, 8, 9, 600]        # 600 rows: three row chunks of 256 per column


@pytest.mark.parametrize("dimup_to", DIMS)
@pytest.mark.parametrize("coef", [1.0, -1.0])
def test_single_term_signed_permutation_is_exact(lib, dimup_to, coef):
    rng = np.random.default_rng(dimup_to)
    dimup_from, dimdw_to, dimdw_from = dimup_to + 3, 5, 4
    up = np.stack([_signed_perm_table(rng, dimup_to, dimup_from)])
    dw = np.stack([_signed_perm_table(rng, dimdw_to, dimdw_from)])
    got, ref, n2, _ = _run(lib, up, dw, [0], [0], [0], [coef], dimup_from, dimdw_from, 0, 3)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))                 # 64-bit patterns
    assert (np.abs(ref) > 0).any() and (ref[dw[0] == -1] == 0).all()
    assert abs(n2 - (np.abs(ref) ** 2).sum()) <= 1e-13 * (np.abs(ref) ** 2).sum()


@pytest.mark.parametrize("dimup_to", [9, 600])
def test_dead_tables_give_zeros(lib, dimup_to):
    up = np.full((2, dimup_to), -1, dtype=np.int32)
    dw = np.full((1, 6), -1, dtype=np.int32)
    live_up = np.stack([np.arange(dimup_to, dtype=np.int32)] * 2)
    live_dw = np.arange(6, dtype=np.int32)[None, :]
    for u, d in ((up, dw), (live_up, dw), (up, live_dw)):
        got, ref, n2, _ = _run(lib, u, d, [0, 1], [0, 1], [0, 0], [1.0, 2.0 - 1.0j], dimup_to, 6, 0, 4)
        assert not ref.any() and (got.view(np.float64) == 0).all() and n2 == 0.0


@pytest.mark.parametrize("dimup_to", [7, 600])
def test_single_live_column(lib, dimup_to):
    rng = np.random.default_rng(8)
    dw = np.full((1, 9), -1, dtype=np.int32)
    dw[0, 4] = np.int32(2) | np.int32(-2 ** 31)                  # target column 4 <- source column 2, minus
    up = np.stack([_signed_perm_table(rng, dimup_to, dimup_to)])
    got, ref, n2, _ = _run(lib, up, dw, [0], [0], [0], [1.0], dimup_to, 3, 0, 5)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    assert ref[4].any() and not np.delete(ref, 4, axis=0).any()


@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("nterms,nuq", [(4, 2), (32, 5), (32, 32)])
def test_many_terms_shared_tables_and_small_grids(lib, grid, nterms, nuq):
    rng = np.random.default_rng(100 * nterms + nuq)
    dimup_to, dimup_from, dimdw_to, dimdw_from, n_up, n_dw = 523, 530, 11, 13, 40, 6
    up = np.stack([_signed_perm_table(rng, dimup_to, dimup_from, 0.7) for _ in range(n_up)])
    dw = np.stack([_signed_perm_table(rng, dimdw_to, dimdw_from, 0.6) for _ in range(n_dw)])
    uq_tab = rng.permutation(n_up)[:nuq]
    t_uq = np.concatenate([np.arange(nuq), rng.integers(0, nuq, nterms - nuq)])   # every distinct table is used
    rng.shuffle(t_uq)
    t_dw = rng.integers(0, n_dw, nterms)
    coef = rng.standard_normal(nterms) + 1j * rng.standard_normal(nterms)
    got, ref, n2, pmax = _run(lib, up, dw, uq_tab, t_uq, t_dw, coef, dimup_from, dimdw_from, grid, 6)
    bound = 4 * (nterms + 1) * 2.0 ** -53 * np.abs(coef).sum() * pmax
    d = np.abs(got - ref).max()
    print(f"terms {nterms}, tables {nuq}, grid {grid}: |d| = {d:.3e} (bound {bound:.3e})")
    assert d <= bound
    assert abs(n2 - (np.abs(ref) ** 2).sum()) <= 1e-13 * (np.abs(ref) ** 2).sum()


def test_real_input_and_real_coefficients_stay_real_and_runs_repeat_bit_for_bit(lib):
    rng = np.random.default_rng(9)
    up = np.stack([_signed_perm_table(rng, 300, 310, 0.8) for _ in range(3)])
    dw = np.stack([_signed_perm_table(rng, 7, 9, 0.8) for _ in range(3)])
    args = (up, dw, [0, 1, 2], [0, 1, 2, 1], [0, 1, 2, 2], [0.5, -1.5, 2.0, 0.25], 310, 9)
    a = _run(lib, *args, 0, 11, real=True)
    b = _run(lib, *args, 0, 11, real=True)
    assert (a[0].imag == 0).all() and a[0].real.any()
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[2] == b[2]


def test_launcher_refuses_what_could_leave_the_buffers(lib):
    import torch

    x = torch.zeros(64, dtype=torch.complex128, device="cuda")
    one = np.zeros(1, dtype=np.uint8)
    cf = np.ones(2)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    n2 = C.c_double()

    def call(up, dw, dimup_to=4, pitch_to=8, dimdw_to=2, dimup_from=4, pitch_from=8, dimdw_from=2, grid=1):
        return lib.spk_run(grid, 1, 1, p(one, C.c_uint8), p(one, C.c_uint8), p(one, C.c_uint8), p(cf, C.c_double), p(up, C.c_int32), 1, p(dw, C.c_int32), 1,
                           dimup_to, pitch_to, dimdw_to, dimup_from, pitch_from, dimdw_from, x.data_ptr(), x.data_ptr() + 16 * 32, C.byref(n2))

    up, dw = np.arange(4, dtype=np.int32), np.arange(2, dtype=np.int32)
    assert call(up, dw) == 0
    assert call(np.array([0, 1, 2, 4], dtype=np.int32), dw) == 1          # a source row outside the source
    assert call(up, np.array([0, 2], dtype=np.int32)) == 1                # a source column outside the source
    assert call(up, dw, pitch_to=4) == 1 and call(up, dw, pitch_from=9) == 1 and call(up, dw, grid=0) == 1 and call(up, dw, grid=4096) == 1
