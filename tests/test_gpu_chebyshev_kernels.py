"""The two kernels of the Chebyshev recurrence, one by one (csrc/hxv_chebyshev_kernels.hpp through the test-only launchers of
tests/device/chebyshev_kernels_check.hip; cases, layout, exact expectations and bounds: tests/chebyshev_ref.py, which
tests/test_chebyshev_ref_cpu.py shows to bite).

The driver tests reach these kernels at a driver's geometry and through a whole recurrence.  Here each launch stands alone, with the grid as
an argument: n in {1, 255, 256, 257} and two, three and four trips of the grid-stride loop with a ragged last one on grids of one, two and
three workgroups; M in {0, 1, 3, 8} probes (and every other instantiation once), with and without the running sum, the general and the
first-step form, and step 0 with and without its output.  Every case twice: small integers with power-of-two scalars, where every output
vector, every block partial and every sum must be the exact result BIT FOR BIT, and normal deviates against long double within the bounds
derived in chebyshev_ref.py.  Whole buffers are compared: NaN where nothing may be read, unchanged bits where nothing may be written, a
sentinel behind the partials and the sums.  A second launch on the same inputs must give the same bits.
All cases of one kind and number format run in one test (about 400 launches of a few microseconds each): well under a second apiece."""
import ctypes as C

import numpy as np
import pytest

import chebyshev_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def ckc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_chebyshev_kernels_check()))
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.ckc_constants.argtypes = [C.POINTER(C.c_int)]
    L.ckc_constants.restype = None
    L.ckc_grid_for.argtypes = [i64]
    L.ckc_init.argtypes =[i32, i32, i64, vp, vp, C.POINTER(vp), dbl, dbl, vp, vp]
    L.ckc_step.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, C.POINTER(vp), dbl, dbl, dbl, dbl, vp, vp]
    return L


def test_constants(ckc):
    c = (C.c_int * 3)()
    ckc.ckc_constants(c)
    assert tuple(c) == (R.RED_BLOCKS, R.MAX_PROBES, R.nsums(0))
    for n in (0, 1, 256, 257, 1024 * 256 + 1, 1 << 40):           # the driver's grid: never empty, at most RED_BLOCKS
        assert ckc.ckc_grid_for(n) == max(1, min((n + 255) // 256, R.RED_BLOCKS)), n


def test_launchers_refuse_what_no_launch_can_take(ckc):
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched, so none is passed"""
    one = (C.c_void_p * 1)(None)
    for grid, m, n, probes in ((0, 0, 8, None), (1025, 0, 8, None), (1, -1, 8, one), (1, 9, 8, one), (1, 0, -1, None), (1, 1, 8, None)):
        assert ckc.ckc_init(grid, m, n, None, None, probes, 0.0, 0.0, None, None) == 1
        assert ckc.ckc_step(grid, m, 0, n, None, None, None, None, probes, 1.0, 0.0, 0.0, 0.0, None, None) == 1


def launch(ckc, case):
    """-> (mem, partial, sums) after one launch on fresh device copies of the case's memory"""
    import torch

    mem = torch.from_numpy(case["mem"]).cuda()
    p0, s0 = R.fresh_outputs(case)
    partial, sums = torch.from_numpy(p0).cuda(), torch.from_numpy(s0).cuda()
    row = mem.shape[1] * mem.element_size()
    at = lambda s: mem.data_ptr() + s * row  # noqa: E731
    m = case["m"]
    probes = (C.c_void_p * max(m, 1))(*[at(R.PROBE0 + j) for j in range(m)])
    out = at(R.OUT) if case["with_sum"] else None
    if case["kind"] == "init":
        rc = ckc.ckc_init(case["grid"], m, case["n"], at(R.CUR), out, probes if m else None, case["cr"], case["ci"], partial.data_ptr(), sums.data_ptr())
    else:
        rc = ckc.ckc_step(case["grid"], m, int(case["first"]), case["n"], at(R.HV), at(R.CUR), at(R.PREV), out, probes if m else None, case["ch"],
                          case["cc"], case["cr"], case["ci"], partial.data_ptr(), sums.data_ptr())
    assert rc == 0, rc
    return mem.cpu().numpy(), partial.cpu().numpy(), sums.cpu().numpy()


def run_all(ckc, cases):
    for case in cases:
        got = launch(ckc, case)
        what = (case["kind"], case["n"], case["grid"], case["m"], case["with_sum"], case["first"], case["integer"])
        assert R.check(case, got) == [], what
        again = launch(ckc, case)
        assert all(R.same_bits(a, b) for a, b in zip(got, again)), what


@pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])
def test_step_kernel(ckc, integer):
    run_all(ckc, (R.make_step(1000 + k, n, g, m, s, f, integer) for k, (n, g, m, s, f) in enumerate(R.step_cases())))


@pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])
def test_initial_kernel(ckc, integer):
    run_all(ckc, (R.make_init(5000 + k, n, g, m, o, integer) for k, (n, g, m, o) in enumerate(R.init_cases())))


def test_pad_rows_come_out_as_plus_zero(ckc):
    """zero inputs (a pad row) give +0.0 in t_next and in the running sum, whatever the signs of b and of the coefficient"""
    for first in (False, True):
        case = R.make_step(3, 257, 2, 1, True, first, True)
        case["mem"][:, 100:140] = 0.0
        for cc, cr, ci in ((1.0, -1.0, 1.0), (-2.0, 1.0, -1.0), (0.0, -1.0, -1.0)):
            case.update(cc=cc, cr=cr, ci=ci)
            mem, _, _ = launch(ckc, case)
            for s in (R.PREV, R.OUT):
                assert R.same_bits(mem[s, 100:140], np.zeros(40, dtype=np.complex128)), (first, cc, s)
