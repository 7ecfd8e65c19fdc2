"""The two kernels of the paired probe runs, one by one (lz_probe_real_pc and lz_probe_dots_pair<M> of csrc/hxv_lanczos_kernels.hpp through
the test-only launchers of tests/device/pair_probe_kernels_check.hip).  The driver tests reach them at the driver's geometry only; here each
runs alone on grids of one to three blocks over sizes around the wave, the block and the loop round, and once in the driver's geometry
(RED_BLOCKS * 256 + 513 elements on RED_BLOCKS blocks).

  - integer-valued data: every product and every partial sum is an exact double whatever the order, so the sums must EQUAL numpy's
  - random data: component a (b) of the paired kernel against lz_probe_dots<M, false> on (Re x, 0) ((Im x, 0)) with the probes in the complex
    layout, bit for bit -- the identity the driver's bit-for-bit promise rests on -- and probe j of M against that probe alone, bit for bit
  - a NaN guard stands behind everything a kernel may read, rows of `partial` beyond the grid keep a sentinel
  - lz_probe_real_pc: Re copied bit for bit on the rows below dimup, exact zeros on the pad rows whatever the source holds there (NaN here),
    per-block sums of Im^2 over the rows below dimup only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
GRIDS = [1, 2, 3]
SENT = -12345.678
NAN = float("nan")


@pytest.fixture(scope="session")
def ppc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_pair_probe_kernels_check()))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.ppc_probe_real_pc.argtypes = [i32, i64, i32, i32, vp, vp, vp]
    L.ppc_probe_dots_pair.argtypes = [i32, i32, i64, vp, C.POINTER(vp), vp, vp]
    L.ppc_probe_dots_complex.argtypes = [i32, i32, i64, vp, C.POINTER(vp), vp, vp]
    return L


def _sizes(L):
    return [(n, g) for n in NS for g in GRIDS] + [(L.ppc_red_blocks() * 256 + 513, L.ppc_red_blocks())]


def _dev(a, guard):
    """device copy of a host array with one guard element behind it"""
    import torch

    return torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1), np.array([guard], dtype=a.dtype)])).cuda()


def _run(L, entry, grid, m, n, x, probes):
    """-> (out[2m], partial[grid + 1, 2m]); x complex[n], probes: m host arrays (real[n] for the paired kernel, complex[n] for the complex one)"""
    import torch

    dx = _dev(x, complex(NAN, NAN))
    dps = [_dev(p, NAN if p.dtype == np.float64 else complex(NAN, NAN)) for p in probes]
    part = torch.full(((grid + 1) * 2 * m,), SENT, dtype=torch.float64, device="cuda")
    out = torch.full((2 * m + 1,), SENT, dtype=torch.float64, device="cuda")
    plist = (C.c_void_p * m)(*[p.data_ptr() for p in dps])
    torch.cuda.synchronize()
    assert getattr(L, entry)(grid, m, n, dx.data_ptr(), plist, part.data_ptr(), out.data_ptr()) == 0
    out, part = out.cpu().numpy(), part.cpu().numpy().reshape(grid + 1, 2 * m)
    assert out[2 * m] == SENT and (part[grid] == SENT).all()      # nothing written past the 2m sums and the grid's rows
    return out[: 2 * m], part[:grid]


def test_integer_data_gives_the_exact_sums(ppc):
    rng = np.random.default_rng(1)
    for n, grid in _sizes(ppc):
        for m in ((8,) if grid > 3 else (1, 2, 3, 4, 5, 6, 7, 8) if n in (257, 1000) else (1, 8)):    # (every m: the dispatch of launch_probe_dots_pair)
            x = rng.integers(-8, 9, n) + 1j * rng.integers(-8, 9, n)
            ps = [rng.integers(-8, 9, n).astype(np.float64) for _ in range(m)]
            out, part = _run(ppc, "ppc_probe_dots_pair", grid, m, n, x.astype(np.complex128), ps)
            ref = np.array([[np.dot(p, x.real), np.dot(p, x.imag)] for p in ps]).reshape(-1)
            assert np.array_equal(out, ref), (n, grid, m)
            assert np.array_equal(part.sum(axis=0), ref), (n, grid, m)                 # (a_j, b_j) per block, in that order
            # block b owns the elements i with (i // 256) % grid == b
            own = (np.arange(n) // 256) % grid
            for b in range(grid if grid <= 3 else 0):
                refb = np.array([[np.dot(p[own == b], x.real[own == b]), np.dot(p[own == b], x.imag[own == b])] for p in ps]).reshape(-1)
                assert np.array_equal(part[b], refb), (n, grid, m, b)


def test_each_component_is_the_complex_kernel_s_sum_bit_for_bit(ppc):
    rng = np.random.default_rng(2)
    for n, grid in _sizes(ppc):
        for m in ((1, 3, 8) if grid <= 3 else (8,)):
            x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128)
            ps = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for _ in range(m)]
            out, _ = _run(ppc, "ppc_probe_dots_pair", grid, m, n, x, ps)
            again, _ = _run(ppc, "ppc_probe_dots_pair", grid, m, n, x, ps)
            assert np.array_equal(out.view(np.uint64), again.view(np.uint64))          # the same bits on every call
            cps = [p.astype(np.complex128) for p in ps]
            for c, comp in enumerate((x.real, x.imag)):
                ref, _ = _run(ppc, "ppc_probe_dots_complex", grid, m, n, comp.astype(np.complex128), cps)
                assert not ref[1::2].any()                                             # (real data: no imaginary part)
                assert np.array_equal(out[c::2].view(np.uint64), ref[0::2].view(np.uint64)), (n, grid, m, c)
            if n:
                assert np.isfinite(out).all() and np.abs(out).max() > 0
            # probe j of M against that probe alone
            for j in (0, m - 1):
                one, _ = _run(ppc, "ppc_probe_dots_pair", grid, 1, n, x, [ps[j]])
                assert np.array_equal(one.view(np.uint64), out[2 * j: 2 * j + 2].view(np.uint64)), (n, grid, m, j)


@pytest.mark.parametrize("dimup,pitch,ncol", [(1, 8, 1), (15, 16, 20), (6, 8, 6), (70, 72, 70), (64, 64, 9), (1000, 1000, 300)])
def test_probe_real_pc_copies_re_zeroes_the_pads_and_sums_im2(ppc, dimup, pitch, ncol):
    import torch

    rng = np.random.default_rng(3)
    n = pitch * ncol
    for grid in (1, 2, 3, min(ppc.ppc_red_blocks(), (n + 255) // 256)):
        src = (rng.standard_normal((ncol, pitch)) + 1j * rng.integers(-4, 5, (ncol, pitch))).astype(np.complex128)
        src[:, dimup:] = complex(NAN, NAN)                                             # pad rows: never read into the sums, written as zero
        dsrc = _dev(src, complex(NAN, NAN))
        dst = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda")
        part = torch.full((grid + 1,), SENT, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ppc.ppc_probe_real_pc(grid, n, dimup, pitch, dsrc.data_ptr(), dst.data_ptr(), part.data_ptr()) == 0
        dst, part = dst.cpu().numpy(), part.cpu().numpy()
        assert dst[n] == SENT and part[grid] == SENT
        got = dst[:n].reshape(ncol, pitch)
        assert np.array_equal(got[:, :dimup].view(np.uint64), src[:, :dimup].real.copy().view(np.uint64))
        assert not got[:, dimup:].any() and not np.signbit(got[:, dimup:]).any()
        im2 = np.where(np.arange(pitch)[None, :] < dimup, np.nan_to_num(src.imag) ** 2, 0.0).reshape(-1)
        own = (np.arange(n) // 256) % grid
        assert np.array_equal(part[:grid], np.array([im2[own == b].sum() for b in range(grid)])), (grid, part[:grid])   # integers: exact
    # refused before anything is launched
    assert ppc.ppc_probe_real_pc(0, n, dimup, pitch, None, None, None) != 0
    assert ppc.ppc_probe_real_pc(1, n, dimup, 0, None, None, None) != 0
    assert ppc.ppc_probe_dots_pair(1, 9, n, None, None, None, None) != 0
