"""The REAL-vector kernels of the Chebyshev recurrence, the conversion that opens a real run and the kernel of hxv_vector_random, one by one
(csrc/hxv_chebyshev_real_kernels.hpp through the test-only launchers of tests/device/chebyshev_real_kernels_check.hip; cases, layout, exact
expectations and bounds: tests/chebyshev_real_ref.py, which tests/test_chebyshev_real_ref_cpu.py shows to bite).

Each launch stands alone, with the grid as an argument: n in {1, 255, 256, 257} double2 elements and two, three and four trips of the
grid-stride loop with a ragged last one on grids of one, two and three workgroups; M in {0, 1, 3, 8} probes (and every other instantiation
once), with and without the running sum, the general and the first-step form, and step 0 with and without its output.  Every case twice:
small integers with power-of-two scalars, where every output vector, every block partial and every sum must be the exact result BIT FOR
BIT, and normal deviates against long double within the bounds derived in chebyshev_real_ref.py.  Whole buffers are compared: NaN where
nothing may be read, unchanged bits where nothing may be written, a sentinel behind the partials and the sums.  A second launch on the same
inputs must give the same bits.  And on the same memory the COMPLEX kernels (ci = 0) store the same t_next and their Re accumulators are the
real kernels' sums, bit for bit, partials included.
All cases of one kind and number format run in one test (some hundred launches of a few microseconds each)."""
import ctypes as C

import numpy as np
import pytest

import chebyshev_real_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def crk(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_chebyshev_real_kernels_check()))
    vp, i32, i64, dbl, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_uint64
    L.crk_constants.argtypes = [C.POINTER(C.c_int)]
    L.crk_constants.restype = None
    L.crk_init.argtypes = [i32, i32, i64, vp, vp, C.POINTER(vp), dbl, vp, vp]
    L.crk_step.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(vp), dbl, dbl, dbl, vp, vp]
    L.crk_complex_init.argtypes = [i32, i32, i64, vp, vp, C.POINTER(vp), dbl, dbl, vp, vp]
    L.crk_complex_step.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(vp), dbl, dbl, dbl, dbl, vp, vp]
    L.crk_to_real.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp]
    L.crk_random.argtypes = [i32, i64, vp, u64, i32, i32, i32, i32, vp, vp]
    L.crk_mix.argtypes = [u64]
    L.crk_mix.restype = u64
    return L


def test_constants_and_refusals(crk):
    c = (C.c_int * 4)()
    crk.crk_constants(c)
    assert tuple(c) == (R.RED_BLOCKS, R.MAX_PROBES, R.nsums(0), 3)
    one = (C.c_void_p * 1)(None)
    for grid, m, n, probes in ((0, 0, 8, None), (1025, 0, 8, None), (1, -1, 8, one), (1, 9, 8, one), (1, 0, -1, None), (1, 1, 8, None)):
        assert crk.crk_init(grid, m, n, None, None, probes, 0.0, None, None) == 1
        assert crk.crk_step(grid, m, 0, n, None, None, None, None, probes, 1.0, 0.0, 0.0, None, None) == 1


def launch(crk, case, complex_form=False):
    """-> (mem, partial, sums) after one launch on fresh device copies of the case's memory; complex_form: the complex kernels with ci = 0,
    with their own 2m + 3 sums"""
    import torch

    import chebyshev_ref as CR

    mem = torch.from_numpy(case["mem"]).cuda()
    p0, s0 = CR.fresh_outputs(case) if complex_form else R.fresh_outputs(case)
    partial, sums = torch.from_numpy(p0).cuda(), torch.from_numpy(s0).cuda()
    row = mem.shape[1] * mem.element_size()
    at = lambda s: mem.data_ptr() + s * row  # noqa: E731
    m = case["m"]
    probes = (C.c_void_p * max(m, 1))(*[at(R.PROBE0 + j) for j in range(m)])
    out = at(R.OUT) if case["with_sum"] else None
    pl = probes if m else None
    if case["kind"] == "init":
        if complex_form:
            rc = crk.crk_complex_init(case["grid"], m, case["n"], at(R.CUR), out, pl, case["cr"], 0.0, partial.data_ptr(), sums.data_ptr())
        else:
            rc = crk.crk_init(case["grid"], m, case["n"], at(R.CUR), out, pl, case["cr"], partial.data_ptr(), sums.data_ptr())
    else:
        args = (case["grid"], m, int(case["first"]), case["n"], at(R.HV), at(R.CUR), at(R.PREV), out, pl, case["ch"], case["cc"], case["cr"])
        if complex_form:
            rc = crk.crk_complex_step(*args, 0.0, partial.data_ptr(), sums.data_ptr())
        else:
            rc = crk.crk_step(*args, partial.data_ptr(), sums.data_ptr())
    assert rc == 0, rc
    return mem.cpu().numpy(), partial.cpu().numpy(), sums.cpu().numpy()


def run_all(crk, cases):
    count = 0
    for case in cases:
        got = launch(crk, case)
        what = (case["kind"], case["n"], case["grid"], case["m"], case["with_sum"], case["first"], case["integer"])
        assert R.check(case, got) == [], what
        again = launch(crk, case)
        assert all(R.same_bits(a, b) for a, b in zip(got, again)), what
        # the complex kernels on the same memory: the same stored vectors, and their Re accumulators are these sums
        cmem, cpartial, csums = launch(crk, case, complex_form=True)
        g, idx = case["grid"], R.re_accumulators(case["m"])
        if case["kind"] == "step":
            assert R.same_bits(got[0][R.PREV], cmem[R.PREV]), what
        if case["with_sum"]:  # (fma(cr, t, o) against fma(cr, t, fma(-0.0, t', o)): equal values; a zero may differ in sign only)
            assert np.array_equal(got[0][R.OUT, :case["n"]], cmem[R.OUT, :case["n"]]), what
        assert R.same_bits(got[1][:g], cpartial[:g][:, idx]), what
        assert R.same_bits(got[2][:-1], csums[:-1][idx]), what
        count += 1
    return count


@pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])
def test_step_kernel(crk, integer):
    assert run_all(crk, (R.make_step(1000 + k, n, g, m, s, f, integer) for k, (n, g, m, s, f) in enumerate(R.step_cases()))) > 300


@pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])
def test_initial_kernel(crk, integer):
    assert run_all(crk, (R.make_init(5000 + k, n, g, m, o, integer) for k, (n, g, m, o) in enumerate(R.init_cases()))) > 150


def test_pad_rows_come_out_as_plus_zero(crk):
    """zero inputs (a pad row) give +0.0 in t_next and in the running sum, whatever the signs of b and of the coefficient"""
    for first in (False, True):
        case = R.make_step(3, 257, 2, 1, True, first, True)
        case["mem"][:, 100:140] = 0.0
        for cc, cr in ((1.0, -1.0), (-2.0, 1.0), (0.0, -1.0)):
            case.update(cc=cc, cr=cr)
            mem, _, _ = launch(crk, case)
            for s in (R.PREV, R.OUT):
                assert R.same_bits(mem[s, 100:140], np.zeros(40, dtype=np.complex128)), (first, cc, s)


@pytest.mark.parametrize("dimup,dimdw,grid", [(20, 5, 1), (15, 40, 2), (70, 9, 3), (1, 1, 1)])
def test_conversion_to_real_and_its_imaginary_sum(crk, dimup, dimdw, grid):
    """ch_to_real: dst = Re src with pads zero, NaN pads of src never read, the gap behind dst untouched; the partials add up to sum |Im| --
    exactly zero for a real vector, and not zero for ONE imaginary element of 1e-300, whose square is zero"""
    import torch

    pc, pr = (dimup + 7) // 8 * 8, (dimup + 15) // 16 * 16
    rng = np.random.default_rng(dimup)
    src = np.full((dimdw, pc), complex(np.nan, np.nan))
    src[:, :dimup] = rng.integers(-4, 5, (dimdw, dimup))
    for tiny in (None, (dimdw - 1, dimup - 1), (0, 0)):
        s = src.copy()
        if tiny:
            s[tiny] += 1e-300j
        d_src = torch.from_numpy(s).cuda()
        d_dst = torch.full((dimdw * pr + 4,), R.SENT, dtype=torch.float64, device="cuda")
        d_par = torch.full((grid + 1,), R.SENT, dtype=torch.float64, device="cuda")
        assert crk.crk_to_real(grid, dimup, dimdw, pc, pr, d_src.data_ptr(), d_dst.data_ptr(), d_par.data_ptr()) == 0
        dst, par = d_dst.cpu().numpy(), d_par.cpu().numpy()
        want = np.zeros((dimdw, pr))
        want[:, :dimup] = s[:, :dimup].real
        assert R.same_bits(dst[:dimdw * pr].reshape(dimdw, pr), want) and np.all(dst[dimdw * pr:] == R.SENT) and par[grid] == R.SENT
        assert par[:grid].sum() == (1e-300 if tiny else 0.0) and (1e-300 * 1e-300 == 0.0)


def test_random_kernel_is_the_formula(crk):
    """vec_random against the numpy restatement, bit for bit: real and complex, a column offset (a rank's slab), a row permutation with signs
    (a device row order), pads zero, nothing behind n written; several trips on one to three workgroups"""
    import torch

    assert crk.crk_mix(12345) == int(R.mix(np.uint64(12345))[0])
    dimup, pitch, ncols, col0 = 21, 24, 130, 7
    n = ncols * pitch
    rng = np.random.default_rng(1)
    iperm = rng.permutation(dimup).astype(np.int32)
    sign = rng.integers(0, 2, dimup).astype(np.uint8)
    ref_idx = (np.arange(ncols)[:, None] + col0) * dimup
    for seed in (0, 2**64 - 3):
        for cv in (0, 1):
            for grid, perm in ((1, False), (2, True), (3, True)):
                q = torch.full((n + 8,), complex(R.SENT, R.SENT), dtype=torch.complex128, device="cuda")
                d_ip, d_sg = torch.from_numpy(iperm).cuda(), torch.from_numpy(sign).cuda()
                rc = crk.crk_random(grid, n, q.data_ptr(), seed, cv, dimup, pitch, col0, d_ip.data_ptr() if perm else None,
                                    d_sg.data_ptr() if perm else None)
                assert rc == 0
                got = q.cpu().numpy()
                assert np.all(got[n:] == complex(R.SENT, R.SENT))
                got = got[:n].reshape(ncols, pitch)
                assert R.same_bits(got[:, dimup:], np.zeros((ncols, pitch - dimup), dtype=np.complex128))
                rows = iperm if perm else np.arange(dimup)
                sg = np.where(sign != 0, -1.0, 1.0) if perm else np.ones(dimup)
                idx = (ref_idx + rows[None, :]).astype(np.uint64)
                want = np.zeros((ncols, dimup), dtype=np.complex128)
                want.real = sg * R.uniform(seed, idx.ravel(), 0).reshape(ncols, dimup)
                if cv:
                    want.imag = sg * R.uniform(seed, idx.ravel(), 1).reshape(ncols, dimup)
                assert R.same_bits(got[:, :dimup], want), (seed, cv, grid)
