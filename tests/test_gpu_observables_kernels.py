"""The four kernels of hxv_observables_accumulate, one by one (csrc/hxv_observables_kernels.hpp through the test-only launchers of
tests/device/observables_kernels_check.hip; cases, synthetic tables, expectations and bounds: tests/observables_kernels_ref.py, which
tests/test_density_kernels_ref_cpu.py compares with explicit Jordan-Wigner operators and shows to bite).

The driver tests reach these kernels at Nimp = 4 (and once at 2) with a sector's own tables.  Here each launch stands alone, with the grid
as an argument: Nimp in {1, 3, 5, 10} -- fewer groups than waves, a pair count that is no multiple of four, the whole LDS array of the dw
pass, o >> nimp at every size -- groups of 0, 1, 63, 64, 65 and 130 entries side by side, DimUp in {1, 5, 300} for the row passes and
{1, 255, 256, 257, 600} for the dw pass, 0 to 600 columns in the reduction, a gathered copy with unused slots, surplus workgroups.  Every
case twice: small integers, where every output must be the exact sum BIT FOR BIT, and normal deviates against long double within the bounds
derived in the ref module.  Whole buffers are compared: NaN wherever no table points, unchanged bits wherever the kernel owns nothing, a
guard behind every buffer.  A second launch on fresh copies must give the same bits.  All cases of one kernel and number format run in one
test."""
import ctypes as C

import numpy as np
import pytest

import observables_kernels_ref as R

pytestmark = pytest.mark.gpu
FORMATS = pytest.mark.parametrize("integer", [True, False], ids=["integers-bit-for-bit", "normal-deviates"])


@pytest.fixture(scope="module")
def okc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_observables_kernels_check()))
    vp, i32 = C.c_void_p, C.c_int
    L.okc_constants.argtypes = [C.POINTER(C.c_int)]
    L.okc_constants.restype = None
    L.okc_rows.argtypes = [i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.okc_rdw.argtypes = [i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.okc_reduce.argtypes = [i32, i32, vp, i32, vp, vp, vp]
    return L


def test_constants(okc):
    c = (C.c_int * 3)()
    okc.okc_constants(c)
    assert tuple(c) == (R.OBS_THREADS, R.OBS_WAVES, R.OBS_MAX_NIMP)


def test_launchers_refuse_what_no_launch_can_take(okc):
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched, so none is passed"""
    for grid, nimp, pitch, dimup, qdw in ((0, 3, 8, 5, 1), (-1, 3, 8, 5, 1), (1, 0, 8, 5, 1), (1, 11, 8, 5, 1), (1, 3, 8, 5, -1), (1, 3, 0, 0, 1),
                                          (1, 3, 8, 5, 1)):  # (the last: nothing wrong but the NULL pointers)
        for pairs in (0, 1):
            assert okc.okc_rows(pairs, grid, nimp, None, pitch, qdw, None, None, None, None, None) == 1
        assert okc.okc_rdw(grid, nimp, None, None, pitch, dimup, qdw, None, None, None, None, None) == 1
        assert okc.okc_reduce(grid, nimp, None, qdw, None, None, None) == 1
    assert okc.okc_rdw(1, 3, None, None, 8, -1, 1, None, None, None, None, None) == 1
    assert okc.okc_rdw(1, 3, None, None, 8, 9, 1, None, None, None, None, None) == 1  # rows beyond the pitch
    assert okc.okc_reduce(64 + 18 + 1, 3, None, 0, None, None, None) == 1              # a workgroup beyond the record


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).cuda()  # (an empty table still needs an address)


def launch(okc, case):
    """-> the whole output buffer after one launch on fresh device copies"""
    out = _dev(case["out0"])
    nimp, qdw, grid = case["nimp"], case["qdw"], case["grid"]
    if case["kind"] == "rows":
        psi, t = _dev(case["psi"]), [_dev(case[k]) for k in ("seg_ptr", "ent_a", "ent_b", "ent_s")]
        rc = okc.okc_rows(int(case["pairs"]), grid, nimp, psi.data_ptr(), case["pitch"], qdw, *[x.data_ptr() for x in t], out.data_ptr())
    elif case["kind"] == "rdw":
        psi, t = _dev(case["psi"]), [_dev(case[k]) for k in ("dwp_ptr", "dwp_slot", "dwp_p", "dwp_s")]
        full = psi if case["full"] is None else _dev(case["full"])
        rc = okc.okc_rdw(grid, nimp, psi.data_ptr(), full.data_ptr(), case["pitch"], case["dimup"], qdw, *[x.data_ptr() for x in t], out.data_ptr())
    else:
        col, t = (_dev(case["colout"]) if qdw else None), [_dev(case[k]) for k in ("dwbin_ptr", "dwbin_cols")]
        rc = okc.okc_reduce(grid, nimp, col.data_ptr() if qdw else None, qdw, *[x.data_ptr() for x in t], out.data_ptr())
    assert rc == 0, rc
    return out.cpu().numpy()


def run_all(okc, name, cases):
    ratios = []
    for case in cases:
        what = (name, {k: v for k, v in case.items() if np.isscalar(v)})
        got = launch(okc, case)
        assert R.check(case, got, ratios) == [], what
        assert R.same_bits(got, launch(okc, case)), what
    if ratios:
        print(f"largest error / bound, {name}: {max(ratios):.3f}")


@FORMATS
@pytest.mark.parametrize("pairs", [False, True], ids=["W-bins", "R_up-pairs"])
def test_rows_kernel(okc, pairs, integer):
    run_all(okc, "obs_rows_kernel<%s>" % str(pairs).lower(), (R.make_rows(100 + k, *c, pairs, integer) for k, c in enumerate(R.rows_cases())))


@FORMATS
def test_rdw_kernel(okc, integer):
    run_all(okc, "obs_rdw_kernel", (R.make_rdw(300 + k, *c, integer) for k, c in enumerate(R.rdw_cases())))


@FORMATS
def test_reduce_kernel(okc, integer):
    run_all(okc, "obs_reduce_kernel", (R.make_reduce(500 + k, *c, integer) for k, c in enumerate(R.reduce_cases())))


def test_reduce_without_columns_is_all_plus_zero(okc):
    for nimp in (1, 3, 5, 10):
        case = R.make_reduce(1, nimp, 0, True, True)
        got = launch(okc, case)
        assert R.same_bits(got[:-1], np.zeros(len(got) - 1)) and R.same_bits(got[-1:], np.array([R.SENT])), nimp
