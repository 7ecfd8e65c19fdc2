"""The streaming kernels of hxv_eigh_lowest, one by one, against exact sums (csrc/hxv_eigh_kernels.hpp through the test-only launchers of
tests/device/eigh_kernels_check.hip; references and bounds: tests/eigh_kernels_ref.py, whose helpers tests/test_eigh_kernels_ref_cpu.py
shows to bite).

The solver corrects a wrong projection or a lost partial sum with a few more products, so none of this shows in its eigenvalues.  Here
every kernel runs alone, with stride != n, with grids of one to three blocks over sizes around the wave, the block and the loop round,
and once in the driver's own geometry.  Every case:
  - stride = n rounded up to 8, plus 8; the gap [n, stride) of every slot and every slot a kernel must not touch hold NaN: a kernel that
    reads them shows NaN in its output, and after the call they must be bitwise what they were;
  - one NaN guard slot (vector, coefficient, index, partial row) stands behind everything a kernel may read;
  - rows of `partial` beyond the grid, and outputs of tr_colsum beyond nval, keep a sentinel;
  - the call is made twice on fresh copies of the inputs and gives identical bits;
  - sums are finished by tr_colsum, as in the driver, and compared with the long-double sum within gamma(D + 2) sum|t_i| (chain_depth);
    elementwise outputs within their per-component bounds.  For the two fused kernels the reference dot is taken with the vector the
    device wrote.
Wall time of the file on an MI355X: 1173 cases in 5.5 s once the libraries are built (the driver-geometry cases take 0.1 - 0.4 s each,
every other case under 50 ms)."""
import ctypes as C

import numpy as np
import pytest

import eigh_kernels_ref as R

pytestmark = pytest.mark.gpu

NS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
GRIDS = [1, 2, 3]
SIZES = [(n, g) for n in NS for g in GRIDS]
SENT = -1.2345678e300
NAN = float("nan")
CNAN = complex(NAN, NAN)


# ---- the library --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def ekc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_eigh_kernels_check()))
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.ekc_constants.argtypes = [C.POINTER(C.c_int)]
    L.ekc_constants.restype = None
    L.ekc_mdot.argtypes = [i32, i64, vp, i64, i32, vp, vp]
    L.ekc_colsum.argtypes = [i32, vp, i32, i32, i32, vp, i32]
    L.ekc_maxpy.argtypes = [i32, i64, vp, i64, i32, vp, vp, vp, vp]
    L.ekc_scale_nrm.argtypes = [i32, i64, vp, dbl, vp]
    L.ekc_rotate.argtypes = [i32, i64, vp, i64, i32, i32, vp]
    L.ekc_rotate_dots.argtypes = [i32, i64, vp, i64, i32, i32, vp, vp, C.POINTER(C.c_int)]
    L.ekc_axpy_mdot.argtypes = [i32, i64, vp, i64, i32, vp, dbl, vp, vp]
    c = (C.c_int * 4)()
    L.ekc_constants(c)
    L.JB, L.TR_BLOCKS, L.MAXCV, L.FUSE_NJ = (int(x) for x in c)
    return L


def test_constants(ekc):
    """what the shapes below assume (a change of a constant must come with new dispatch and capacity cases)"""
    assert (ekc.JB, ekc.TR_BLOCKS, ekc.MAXCV, ekc.FUSE_NJ) == (8, 4096, 64, 16)


# ---- memory -------------------------------------------------------------------------------------------------------------------------------
def stride_of(n):
    return (n + 7) // 8 * 8 + 8


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def slots(rng, nslots, n, filled):
    """complex [nslots, stride]: NaN everywhere but [:n] of the slots in `filled`"""
    h = np.full((nslots, stride_of(n)), CNAN)
    for s in filled:
        h[s, :n] = R.random_complex(rng, n)
    return h


def reals(rng, count, guard=1):
    """`count` random reals and `guard` NaN behind them"""
    return np.concatenate([R.random_reals(rng, count), np.full(guard, NAN)])


def sentinel(*shape):
    return np.full(shape, SENT)


def twice(run, what):
    """run() -> dict of host arrays; both runs start from fresh copies of the inputs and must agree bit for bit"""
    a, b = run(), run()
    for key in a:
        assert same_bits(a[key], b[key]), (what, key, "two runs differ")
    return a


def ok(rc, what):
    assert rc == 0, (what, "HIP status", rc)


def finish_sum(ekc, d_partial, grid, ldp, nval, zero_odd=0):
    """tr_colsum as the driver runs it (one block) into a sentinel-backed output -> host array [nval + 2]"""
    out = dev(sentinel(nval + 2))
    ok(ekc.ekc_colsum(1, ptr(d_partial), grid, ldp, nval, ptr(out), zero_odd), "tr_colsum")
    return host(out)


def check_partial_rows(part, grid, what):
    assert same_bits(part[grid:], sentinel(*part[grid:].shape)), (what, "partial rows beyond the grid were written")


def check_gaps(after, before, n, what):
    assert same_bits(after[..., n:], before[..., n:]), (what, "the gap [n, stride) changed")


DRIVER = (4096 * 256 + 513, 4096)       # TR_BLOCKS * 256 + 513 elements on TR_BLOCKS blocks (test_constants pins TR_BLOCKS)


def with_sizes(name, values, driver_value):
    """every value at every small (n, grid), and `driver_value` once in the driver's geometry"""
    out = [pytest.param(v, n, g, id=f"{name}{v}-n{n}-grid{g}") for v in values for n, g in SIZES]
    return out + [pytest.param(driver_value, *DRIVER, id=f"{name}{driver_value}-driver-geometry")]


# ---- tr_mdot ------------------------------------------------------------------------------------------------------------------------------
def run_mdot(ekc, V, w, n, nb, grid):
    dV, dw, dp = dev(V), dev(w), dev(sentinel(grid + 2, 2 * ekc.JB))
    ok(ekc.ekc_mdot(grid, n, ptr(dV), V.shape[1], nb, ptr(dw), ptr(dp)), "tr_mdot")
    out = finish_sum(ekc, dp, grid, 2 * ekc.JB, 2 * nb)
    return dict(V=host(dV), w=host(dw), partial=host(dp), out=out)


@pytest.mark.parametrize("nb,n,grid", with_sizes("nb", range(1, 9), 2))
def test_tr_mdot(ekc, nb, n, grid):
    what = ("tr_mdot", f"nb={nb}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([11, nb, n, grid])
    V, w = slots(rng, nb + 1, n, range(nb)), slots(rng, 1, n, [0])
    r = twice(lambda: run_mdot(ekc, V, w, n, nb, grid), what)
    assert same_bits(r["V"], V) and same_bits(r["w"], w), (what, "an input changed")
    check_partial_rows(r["partial"], grid, what)
    assert np.all(np.isfinite(r["partial"][:grid, :2 * nb])), (what, "partial not finite")
    assert same_bits(r["out"][2 * nb:], sentinel(2)), (what, "tr_colsum wrote beyond nval")
    ref, ab = R.dots(V[:nb, :n], w[0, :n])
    R.check_sum(r["out"][:2 * nb].reshape(nb, 2), ref, ab, R.chain_depth(n, grid, grid), what)


@pytest.mark.parametrize("nb,n,grid", with_sizes("nb", [1], 1))
def test_tr_mdot_on_real_vectors(ekc, nb, n, grid):
    """REAL-vector mode: two real arrays of 2n doubles viewed as n double2; the real part is their dot product, and through
    tr_colsum(zero_odd = 1) the odd output is exactly 0.0"""
    what = ("tr_mdot real view", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([12, n, grid])
    st = stride_of(n)
    a, b = np.full((2, 2 * st), NAN), np.full((1, 2 * st), NAN)
    a[0, :2 * n], b[0, :2 * n] = R.random_reals(rng, 2 * n), R.random_reals(rng, 2 * n)

    def run():
        dV, dw, dp = dev(a), dev(b), dev(sentinel(grid + 2, 2 * ekc.JB))
        ok(ekc.ekc_mdot(grid, n, ptr(dV), st, 1, ptr(dw), ptr(dp)), what)
        return dict(V=host(dV), w=host(dw), partial=host(dp), out=finish_sum(ekc, dp, grid, 2 * ekc.JB, 2, 1))

    r = twice(run, what)
    assert same_bits(r["V"], a) and same_bits(r["w"], b), (what, "an input changed")
    check_partial_rows(r["partial"], grid, what)
    x, y = R.ld(a[0, :2 * n]), R.ld(b[0, :2 * n])
    R.check_sum(r["out"][:1], np.sum(x * y).reshape(1), np.sum(np.abs(x * y)).reshape(1), R.chain_depth(n, grid, grid), what)
    assert same_bits(r["out"][1:], np.array([0.0, SENT, SENT])), (what, "odd output not +0.0, or the sentinel went", r["out"][1:])


# ---- tr_colsum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_odd", [0, 1])
@pytest.mark.parametrize("ldp,nval", [(1, 1), (16, 16), (16, 13), (32, 32), (32, 29), (33, 33), (33, 30)])
@pytest.mark.parametrize("nblocks", [1, 2, 255, 256, 257, 4096])
def test_tr_colsum(ekc, nblocks, ldp, nval, zero_odd):
    what = ("tr_colsum", f"nblocks={nblocks}", f"ld={ldp}", f"nval={nval}", f"zero_odd={zero_odd}")
    rng = np.random.default_rng([13, nblocks, ldp, nval, zero_odd])
    p = np.full((nblocks + 1, ldp), NAN)          # (a NaN row behind the last block, NaN in the columns beyond nval)
    p[:nblocks, :nval] = R.random_reals(rng, (nblocks, nval))
    if zero_odd:
        p[:, 1::2] = NAN                          # (the odd columns must not be read)

    def run():
        dp, out = dev(p), dev(sentinel(nval + 2))
        ok(ekc.ekc_colsum(1, ptr(dp), nblocks, ldp, nval, ptr(out), zero_odd), what)
        return dict(partial=host(dp), out=host(out))

    r = twice(run, what)
    assert same_bits(r["partial"], p), (what, "the input changed")
    assert same_bits(r["out"][nval:], sentinel(2)), (what, "wrote beyond nval")
    ref, ab = R.colsum(p[:nblocks], nval, zero_odd)
    R.check_sum(r["out"][:nval], ref, ab, R.chain_depth(None, 1, nblocks), what)
    if zero_odd:
        odd = r["out"][1:nval:2]
        assert same_bits(odd, np.zeros(odd.shape)), (what, "odd outputs are not +0.0", odd)


# ---- tr_maxpy -----------------------------------------------------------------------------------------------------------------------------
def selection(rng, nj):
    """-> (number of slots, idx): nj distinct slots, slot 0 and the last slot among them, neither ascending nor descending where nj allows"""
    if nj <= 1:
        return 1, list(range(nj))
    nslots = nj + 2
    while True:
        idx = [0, nslots - 1] + [int(s) for s in rng.choice(np.arange(1, nslots - 1), size=nj - 2, replace=False)]
        idx = [idx[i] for i in rng.permutation(nj)]
        if nj == 2:
            return nslots, [nslots - 1, 0]
        if idx != sorted(idx) and idx != sorted(idx, reverse=True):
            return nslots, idx


@pytest.mark.parametrize("nj,n,grid", with_sizes("nj", [0, 1, 2, 3, 4, 5, 8, 65], 2))
def test_tr_maxpy(ekc, nj, n, grid):
    what = ("tr_maxpy", f"nj={nj}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([14, nj, n, grid])
    if (n, grid) == DRIVER:
        nslots, idx = 2, [1, 0]                                         # (two basis vectors in all)
    else:
        nslots, idx = selection(rng, nj)
    assert nj <= ekc.MAXCV + 1 and len(idx) == nj and (nj == 0 or (0 in idx and nslots - 1 in idx))
    V, w = slots(rng, nslots, n, idx), slots(rng, 1, n, [0])           # (slots not selected are NaN throughout)
    coef = reals(rng, 2 * nj, guard=2)                                  # complex coefficients, imaginary parts non-zero
    unused = [s for s in range(nslots) if s not in idx]
    didx = np.array(idx + [unused[0] if unused else 0], dtype=np.int32)  # (the guard entry names a NaN slot where there is one)

    def run():
        dV, dw, di, dc, dp = dev(V), dev(w), dev(didx), dev(coef), dev(sentinel(grid + 2))
        ok(ekc.ekc_maxpy(grid, n, ptr(dV), V.shape[1], nj, ptr(di), ptr(dc), ptr(dw), ptr(dp)), what)
        return dict(V=host(dV), w=host(dw), idx=host(di), coef=host(dc), partial=host(dp), out=finish_sum(ekc, dp, grid, 1, 1))

    r = twice(run, what)
    assert same_bits(r["V"], V) and same_bits(r["idx"], didx) and same_bits(r["coef"], coef), (what, "an input changed")
    check_gaps(r["w"], w, n, what)
    check_partial_rows(r["partial"], grid, what)
    ref, bound = R.maxpy(V[:, :n], idx, coef, w[0, :n])
    R.check_elementwise(r["w"][0, :n], ref, bound, what)
    nrm, ab = R.norm2(r["w"][0, :n])                                    # (of the vector the device wrote)
    R.check_sum(r["out"][:1], nrm.reshape(1), ab.reshape(1), R.chain_depth(n, grid, grid), what + ("norm",))
    assert same_bits(r["out"][1:], sentinel(2)), (what, "tr_colsum wrote beyond nval")


# ---- tr_scale_nrm -------------------------------------------------------------------------------------------------------------------------
SCALE_MODES = {"r1-norm": (1.0, True), "scale-norm": (1.0 / 3.7, True), "scale-only": (-271.25, False)}


@pytest.mark.parametrize("mode,n,grid", with_sizes("", list(SCALE_MODES), "scale-norm"))
def test_tr_scale_nrm(ekc, mode, n, grid):
    r_, with_partial = SCALE_MODES[mode]
    what = ("tr_scale_nrm", f"r={r_}", f"partial={with_partial}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([15, n, grid, int(with_partial)])
    x = slots(rng, 1, n, [0])

    def run():
        dx, dp = dev(x), dev(sentinel(grid + 2))
        ok(ekc.ekc_scale_nrm(grid, n, ptr(dx), r_, ptr(dp) if with_partial else None), what)
        return dict(x=host(dx), partial=host(dp), out=finish_sum(ekc, dp, grid, 1, 1) if with_partial else sentinel(3))

    r = twice(run, what)
    if r_ == 1.0:
        assert same_bits(r["x"], x), (what, "r = 1 must leave x as it is")
    else:
        check_gaps(r["x"], x, n, what)
        ref, bound = R.scale(x[0, :n], r_)
        R.check_elementwise(r["x"][0, :n], ref, bound, what)
    if with_partial:
        check_partial_rows(r["partial"], grid, what)
        nrm, ab = R.norm2(x[0, :n])                                     # (the kernel sums the squares of what it READ)
        R.check_sum(r["out"][:1], nrm.reshape(1), ab.reshape(1), R.chain_depth(n, grid, grid), what + ("norm",))
        assert same_bits(r["out"][1:], sentinel(2)), (what, "tr_colsum wrote beyond nval")
    else:
        assert same_bits(r["partial"], sentinel(grid + 2)), (what, "partial written though none was passed")


# ---- tr_rotate ----------------------------------------------------------------------------------------------------------------------------
ROTATE_MK = [(2, 1), (4, 4), (8, 1), (8, 7), (9, 3), (16, 15), (17, 16), (32, 31), (33, 1), (33, 17), (64, 1), (64, 16), (64, 63), (64, 64)]


def rotate_cases():
    out = []
    for m, k in ROTATE_MK:
        for n in (NS if m <= 9 else [1, 257]):
            out += [pytest.param(m, k, n, g, id=f"m{m}-k{k}-n{n}-grid{g}") for g in GRIDS]
    return out + [pytest.param(2, 1, *DRIVER, id="m2-k1-driver-geometry")]


@pytest.mark.parametrize("m,k,n,grid", rotate_cases())
def test_tr_rotate(ekc, m, k, n, grid):
    what = ("tr_rotate", f"m={m}", f"k={k}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([16, m, k, n, grid])
    V = slots(rng, m + 1, n, range(m))                                  # (slot m: NaN guard)
    S = reals(rng, m * k, guard=2)

    def run():
        dV, dS = dev(V), dev(S)
        ok(ekc.ekc_rotate(grid, n, ptr(dV), V.shape[1], m, k, ptr(dS)), what)
        return dict(V=host(dV), S=host(dS))

    r = twice(run, what)
    assert same_bits(r["S"], S), (what, "S changed")
    assert same_bits(r["V"][k:], V[k:]), (what, "a slot from k on changed")
    check_gaps(r["V"], V, n, what)
    ref, bound = R.rotate(V[:m, :n], S[:m * k].reshape(k, m).T, k)
    R.check_elementwise(r["V"][:k, :n], ref, bound, what)


# ---- tr_rotate_dots -----------------------------------------------------------------------------------------------------------------------
ROTATE_DOTS_MK = [(2, 1), (8, 7), (9, 8), (16, 15), (17, 16), (32, 16), (33, 16), (64, 1), (64, 16)]


def rotate_dots_cases():
    out = [pytest.param(m, k, n, g, id=f"m{m}-k{k}-n{n}-grid{g}") for m, k in ROTATE_DOTS_MK for n, g in SIZES]
    return out + [pytest.param(2, 1, *DRIVER, id="m2-k1-driver-geometry")]


def run_rotate_dots(ekc, V, S, n, m, k, grid, what):
    dV, dS, dp = dev(V), dev(S), dev(sentinel(grid + 2, 2 * ekc.FUSE_NJ))
    launched = C.c_int(-1)
    ok(ekc.ekc_rotate_dots(grid, n, ptr(dV), V.shape[1], m, k, ptr(dS), ptr(dp), C.byref(launched)), what)
    out = finish_sum(ekc, dp, grid, 2 * ekc.FUSE_NJ, 2 * k) if launched.value == 1 else sentinel(2 * k + 2)
    return dict(V=host(dV), S=host(dS), partial=host(dp), out=out, launched=np.array([launched.value]))


@pytest.mark.parametrize("m,k,n,grid", rotate_dots_cases())
def test_tr_rotate_dots(ekc, m, k, n, grid):
    what = ("tr_rotate_dots", f"m={m}", f"k={k}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([17, m, k, n, grid])
    V = slots(rng, m + 2, n, range(m + 1))                              # (slot m: the residual vector; slot m + 1: NaN guard)
    S = reals(rng, m * k, guard=2)
    r = twice(lambda: run_rotate_dots(ekc, V, S, n, m, k, grid, what), what)
    assert r["launched"][0] == 1, (what, "launch_rotate_dots refused")
    assert same_bits(r["S"], S), (what, "S changed")
    check_gaps(r["V"], V, n, what)
    assert same_bits(r["V"][k, :n], V[m, :n]), (what, "slot k is not the old slot m")
    assert same_bits(r["V"][k + 1:], V[k + 1:]), (what, "a slot behind k changed")
    ref, bound = R.rotate(V[:m, :n], S[:m * k].reshape(k, m).T, k)
    R.check_elementwise(r["V"][:k, :n], ref, bound, what)
    check_partial_rows(r["partial"], grid, what)
    dref, ab = R.dots(r["V"][:k, :n], V[m, :n])                         # (with the y_j the device wrote)
    R.check_sum(r["out"][:2 * k].reshape(k, 2), dref, ab, R.chain_depth(n, grid, grid), what + ("dots",))
    assert same_bits(r["out"][2 * k:], sentinel(2)), (what, "tr_colsum wrote beyond nval")


def test_tr_rotate_dots_refuses_more_than_fuse_nj(ekc):
    """k = 17 = FUSE_NJ + 1: the launcher returns false and nothing at all is written"""
    m, k, n, grid = 32, 17, 257, 2
    what = ("tr_rotate_dots", f"m={m}", f"k={k}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([18])
    V, S = slots(rng, m + 2, n, range(m + 1)), reals(rng, m * k, guard=2)
    r = twice(lambda: run_rotate_dots(ekc, V, S, n, m, k, grid, what), what)
    assert r["launched"][0] == 0, what
    assert same_bits(r["V"], V) and same_bits(r["S"], S) and same_bits(r["partial"], sentinel(grid + 2, 2 * ekc.FUSE_NJ)), (what, "something was written")


# ---- tr_axpy_mdot -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,n,grid", with_sizes("nv", [1, 2, 7, 16], 2))
def test_tr_axpy_mdot(ekc, nv, n, grid):
    what = ("tr_axpy_mdot", f"nv={nv}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([19, nv, n, grid])
    a = -0.37
    V, w = slots(rng, nv + 1, n, range(nv)), slots(rng, 1, n, [0])
    coef = np.full(ekc.FUSE_NJ + 1, NAN)                                # (NaN behind the nv coefficients the kernel may read)
    coef[:nv] = R.random_reals(rng, nv)
    coef[nv - 1] = 0.0                                                  # the measured-only vectors: the newest one, and one inside
    if nv >= 7:
        coef[2] = 0.0

    def run():
        dV, dw, dc, dp = dev(V), dev(w), dev(coef), dev(sentinel(grid + 2, 2 * ekc.FUSE_NJ))
        ok(ekc.ekc_axpy_mdot(grid, n, ptr(dV), V.shape[1], nv, ptr(dc), a, ptr(dw), ptr(dp)), what)
        return dict(V=host(dV), w=host(dw), coef=host(dc), partial=host(dp), out=finish_sum(ekc, dp, grid, 2 * ekc.FUSE_NJ, 2 * nv))

    r = twice(run, what)
    assert same_bits(r["V"], V) and same_bits(r["coef"], coef), (what, "an input changed")
    check_gaps(r["w"], w, n, what)
    ref, bound = R.axpy(V[:nv, :n], coef[:nv], a, w[0, :n])
    R.check_elementwise(r["w"][0, :n], ref, bound, what)
    check_partial_rows(r["partial"], grid, what)
    assert np.all(np.isfinite(r["partial"][:grid])), (what, "partial not finite")       # (all 2 NJ accumulators: the unused ones are zero)
    dref, ab = R.dots(V[:nv, :n], r["w"][0, :n])                        # (with the vector the device wrote)
    R.check_sum(r["out"][:2 * nv].reshape(nv, 2), dref, ab, R.chain_depth(n, grid, grid), what + ("dots",))
    assert same_bits(r["out"][2 * nv:], sentinel(2)), (what, "tr_colsum wrote beyond nval")
