"""The three kernels of hxv_apply_density_ops, one by one (csrc/hxv_density_ops_kernels.hpp through the test-only launchers of
tests/device/density_ops_kernels_check.hip; cases, synthetic tables, expectations and bounds: tests/density_ops_kernels_ref.py, which
tests/test_density_kernels_ref_cpu.py compares with explicit Jordan-Wigner operators and shows to bite).

The driver tests reach these kernels at Nimp 2, 4 and 8 with at most two row chunks and a grid of one workgroup per item.  Here each launch
stands alone, with the grid and the chunking as arguments: one, two and several items per workgroup (the stride item += gridDim), more
workgroups than items, one chunk of two inner trips with a ragged second one, three chunks, a chunk half in the pad rows and one wholly
beyond the pitch; Nimp in {1, 5, 6, 10} (both sides of the boundary of the two lookup halves), 1, 3 and 8 operators, zero and nonzero means;
the reduction over 1 to 600 workgroups with and without the norm's slot.  Every case twice: small integers, where every output vector, every
partial and every sum must be the exact value BIT FOR BIT, and normal deviates against long double within the bounds derived in the ref
module.  Whole buffers are compared: NaN pad rows in psi, +0.0 pad rows in every output, +0.0 in the slots of operators that are not there
and in the partials of idle workgroups, a guard column, row and entry behind the buffers.  A second launch on fresh copies must give the
same bits.  All cases of one kernel and number format run in one test."""
import ctypes as C

import numpy as np
import pytest

import density_ops_kernels_ref as R

pytestmark = pytest.mark.gpu
FORMATS = pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])


@pytest.fixture(scope="module")
def dkc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_density_ops_kernels_check()))
    vp, i32 = C.c_void_p, C.c_int
    L.dkc_constants.argtypes = [C.POINTER(C.c_int)]
    L.dkc_constants.restype = None
    L.dkc_sums.argtypes = [i32] * 8 + [vp] * 5
    L.dkc_apply.argtypes = [i32] * 8 + [vp] * 4 + [C.POINTER(vp), C.POINTER(C.c_double), vp]
    L.dkc_reduce.argtypes = [i32, i32, i32, vp, vp]
    return L


def test_constants(dkc):
    c = (C.c_int * 7)()
    dkc.dkc_constants(c)
    assert tuple(c) == (R.DOP_THREADS, R.DOP_MAX, R.DOP_NSUM, R.DOP_MAX_NIMP, R.DOP_UNROLL, R.DOP_CHUNK, R.DOP_WG_PER_CU)


def test_launchers_refuse_what_no_launch_can_take(dkc):
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched, so none is passed"""
    good = dict(grid=1, dimup=5, pitch=8, qdw=1, nimp=3, nops=2, nchunk=1, rows=8)
    wrong = [dict(grid=0), dict(grid=-3), dict(nimp=0), dict(nimp=11), dict(nops=0), dict(nops=9), dict(dimup=-1), dict(dimup=0), dict(pitch=4),
             dict(pitch=12), dict(qdw=-1), dict(nchunk=0), dict(rows=0), dict(rows=-8), dict(rows=12), {}]  # ({}: nothing wrong but the NULL pointers)
    for w in wrong:
        a = [dict(good, **w)[k] for k in ("grid", "dimup", "pitch", "qdw", "nimp", "nops", "nchunk", "rows")]
        assert dkc.dkc_sums(*a, None, None, None, None, None) == 1, w
        assert dkc.dkc_apply(*a, None, None, None, None, None, None, None) == 1, w
    for grid, nblocks, norm_at in ((0, 4, -1), (10, 4, -1), (1, -1, -1), (1, 4, -2), (1, 4, 9), (1, 4, -1)):
        assert dkc.dkc_reduce(grid, nblocks, norm_at, None, None) == 1


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def launch(dkc, case):
    """-> the buffers of R.evaluate()'s shape after one launch on fresh device copies"""
    if case["kind"] == "reduce":
        partial, sums = _dev(case["partial"]), _dev(case["sums0"])
        rc = dkc.dkc_reduce(case["grid"], case["nblocks"], case["norm_at"], partial.data_ptr(), sums.data_ptr())
        assert rc == 0, rc
        return (sums.cpu().numpy(),)
    shape = [case[k] for k in ("grid", "dimup", "pitch", "qdw", "nimp", "nops", "nchunk", "rows")]
    psi, occ_up, occ_dw, coef, partial = (_dev(case[k]) for k in ("psi", "occ_up", "occ_dw", "coef", "partial0"))
    if case["kind"] == "sums":
        rc = dkc.dkc_sums(*shape, psi.data_ptr(), occ_up.data_ptr(), occ_dw.data_ptr(), coef.data_ptr(), partial.data_ptr())
        assert rc == 0, rc
        return (partial.cpu().numpy(),)
    outs = _dev(case["outs0"])
    nops = case["nops"]
    step = outs[0].numel() * outs.element_size()
    ptrs = (C.c_void_p * nops)(*[outs.data_ptr() + a * step for a in range(nops)])
    m = (C.c_double * nops)(*case["m"])
    rc = dkc.dkc_apply(*shape, psi.data_ptr(), occ_up.data_ptr(), occ_dw.data_ptr(), coef.data_ptr(), ptrs, m, partial.data_ptr())
    assert rc == 0, rc
    return outs.cpu().numpy(), partial.cpu().numpy()


def run_all(dkc, name, cases):
    ratios = []
    for case in cases:
        what = (name, {k: v for k, v in case.items() if np.isscalar(v)})
        got = launch(dkc, case)
        assert R.check(case, got, ratios) == [], what
        assert all(R.same_bits(a, b) for a, b in zip(got, launch(dkc, case))), what
    if ratios:
        print(f"largest error / bound, {name}: {max(ratios):.3f}")


@FORMATS
def test_sums_kernel(dkc, integer):
    run_all(dkc, "dop_sums_kernel", (R.make_pass(700 + k, "sums", *c, integer) for k, c in enumerate(R.pass_cases())))


@FORMATS
def test_apply_kernel(dkc, integer):
    run_all(dkc, "dop_apply_kernel", (R.make_pass(700 + k, "apply", *c, integer) for k, c in enumerate(R.pass_cases())))


@FORMATS
def test_reduce_kernel(dkc, integer):
    run_all(dkc, "dop_reduce_kernel", (R.make_reduce(900 + k, *c, integer) for k, c in enumerate(R.reduce_cases())))
