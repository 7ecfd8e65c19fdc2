"""The kernels of the single-vector Lanczos recurrence, one by one (csrc/hxv_lanczos_kernels.hpp through the test-only launchers of
tests/device/lanczos_kernels_check.hip; references, bounds and exact restatements: tests/lanczos_kernels_ref.py, which
tests/test_lanczos_kernels_ref_cpu.py shows to bite).

Every driver test reaches these kernels at a driver's geometry and compares recurrence coefficients to 1e-10, or two drivers that share the
kernels with each other.  Here every kernel runs alone, with stride != n, on grids of one to three blocks over sizes around the wave, the
block and the loop round, and once in the driver's own geometry (RED_BLOCKS * 256 + 513 elements on RED_BLOCKS blocks).  Every case:
  - stride = n rounded up to 8, plus 8; the gap [n, stride) of every slot and every buffer a kernel must not read hold NaN: a kernel that
    reads them shows NaN in its output, and after the call they must be bitwise what they were;
  - one NaN guard stands behind everything a kernel may read;
  - rows of `partial` beyond the grid keep a sentinel, and so does every slot of `scal` but the one written;
  - the call is made twice on fresh copies of the inputs and gives identical bits; the output is finite.
Bounds (derived in lanczos_kernels_ref.py from the kernel text): a sum finished by lz_final / lz_probe_final is within gamma(D + 2) sum|t_i|
of the long-double sum, D = 2 ceil(n / (256 grid)) + 8 + ceil(np / 256) + 8 (thread loop, eight-level LDS tree, finishing kernel); where a
kernel updates w and then sums it, the updated w has its own elementwise bound and the sum is referenced with the w the device wrote;
fma(-a, y, x) within u |x - a y|, x - b p and z + c x within gamma(2) of the magnitudes, x / s within gamma(2) |x / s|.  Bit for bit: the
start vectors against their uint64 restatement, the layout conversions, the paired kernel against two single runs, probe j of M against that
probe alone, and lz_next / lz_mul / lz_sqrt against IEEE double on the host and against LzScale compiled from the same header.  The
lz_next chain is 50 successive random betas with magnitudes from 1e-150 to 1e150 (the project records no such sequence; 50 steps, the
first 40 of them recorded, is this file's choice).
Wall time of the file on an MI355X: 1119 cases in 3.6 s once the libraries are built (the driver-geometry cases take 0.03 - 0.43 s each, every
other case under 50 ms but the very first, which loads the library)."""
import ctypes as C

import numpy as np
import pytest

import lanczos_kernels_ref as R

pytestmark = pytest.mark.gpu

NS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
GRIDS = [1, 2, 3]
SIZES = [(n, g) for n in NS for g in GRIDS]
DRIVER = (R.RED_BLOCKS * 256 + 513, R.RED_BLOCKS)       # (test_constants pins RED_BLOCKS)
ALL_SIZES = [pytest.param(n, g, id=f"n{n}-grid{g}") for n, g in SIZES] + [pytest.param(*DRIVER, id="driver-geometry")]
SENT = R.SENT
NAN = float("nan")
CNAN = complex(NAN, NAN)
NSCAL = 16
OUT_SLOT = 5
same_bits = R.same_bits


# ---- the library --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def lkc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_lanczos_kernels_check()))
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double
    L.lkc_constants.argtypes = [C.POINTER(C.c_int)]
    L.lkc_constants.restype = None
    L.lkc_grid_for.argtypes = [i64]
    L.lkc_sub_dot.argtypes = [i32, i64, vp, vp, vp, vp, i32, vp]
    L.lkc_sub_nrm.argtypes = [i32, i64, vp, vp, vp, i32, vp]
    L.lkc_sub_nrm_pair.argtypes = [i32, i64, vp, vp, vp, i32, i32, vp, vp]
    L.lkc_pack_pair.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp]
    L.lkc_nrm.argtypes = [i32, i64, vp, vp]
    L.lkc_final.argtypes = [i32, vp, i32, vp, i32, i32]
    L.lkc_probe_dots.argtypes = [i32, i32, i32, i64, vp, C.POINTER(vp), vp, vp]
    L.lkc_probe_final.argtypes = [i32, vp, i32, i32, vp]
    L.lkc_scale.argtypes = [i32, i64, vp, vp, vp, i32]
    L.lkc_axpy.argtypes = [i32, i64, vp, vp, dbl]
    L.lkc_init.argtypes = [i32, i64, vp, u64, i32, i32, i32, vp, vp]
    L.lkc_init_real.argtypes = [i32, i64, vp, u64, i32, i32, i32, vp, vp]
    L.lkc_to_real.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp]
    L.lkc_to_complex.argtypes = [i32, i32, i32, i32, i32, vp, vp]
    L.lkc_mul.argtypes = [i32, vp, i32, i32, i32]
    L.lkc_sqrt.argtypes = [i32, vp, i32]
    L.lkc_next.argtypes = [i32, vp, vp, vp, i32]
    L.lkc_host_scale_next.argtypes = [C.POINTER(dbl), dbl, C.POINTER(dbl)]
    L.lkc_host_scale_next.restype = None
    c = (C.c_int * 7)()
    L.lkc_constants(c)
    L.constants = tuple(int(x) for x in c)
    return L


def test_constants(lkc):
    """what the shapes here and the restatements of lanczos_kernels_ref.py assume: RED_BLOCKS, HXV_MAX_PROBES and the scalar slots"""
    assert lkc.constants == (1024, 8, R.LZ_ALPHA, R.LZ_BETA, R.LZ_S, R.LZ_C, R.LZ_STEP)
    assert (R.RED_BLOCKS, R.MAX_PROBES) == lkc.constants[:2]


def test_grid_for(lkc):
    """min(ceil(n / 256), RED_BLOCKS), and never an empty grid"""
    for n in (0, 1, 255, 256, 257, 1000, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1, 1 << 40):
        assert lkc.lkc_grid_for(n) == max(1, min((n + 255) // 256, 1024)), n


def test_launchers_refuse_what_the_tables_do_not_hold(lkc):
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched, so none is passed"""
    assert lkc.lkc_nrm(0, 8, None, None) == 1 and lkc.lkc_nrm(1025, 8, None, None) == 1 and lkc.lkc_nrm(1, -1, None, None) == 1
    one = (C.c_void_p * 1)(None)
    for m in (0, 9, -1):
        assert lkc.lkc_probe_dots(1, 0, m, 8, None, one, None, None) == 1, m
    assert lkc.lkc_probe_dots(1, 0, 1, 8, None, None, None, None) == 1
    assert lkc.lkc_final(1, None, -1, None, 0, 0) == 1 and lkc.lkc_sub_nrm(1, 8, None, None, None, -1, None) == 1
    assert lkc.lkc_init(1, 8, None, 0, 9, 8, 0, None, None) == 1 and lkc.lkc_to_real(1, 9, 1, 8, 16, None, None, None) == 1
    assert lkc.lkc_next(2, None, None, None, 4) == 1 and lkc.lkc_mul(0, None, 0, 0, 0) == 1 and lkc.lkc_sqrt(1, None, -1) == 1


# ---- memory -------------------------------------------------------------------------------------------------------------------------------
def stride_of(n):
    return (n + 7) // 8 * 8 + 8


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t, offset_bytes=0):
    return None if t is None else t.data_ptr() + offset_bytes


def slot_ptr(t, s):
    """device address of slot s of a [nslots, stride] tensor"""
    return t.data_ptr() + s * t.shape[1] * t.element_size()


def slots(rng, nslots, n, filled, real_view=False):
    """complex [nslots, stride]: NaN everywhere but [:n] of the slots in `filled`.  real_view: the data are 2n reals viewed as n double2"""
    h = np.full((nslots, stride_of(n)), CNAN)
    for s in filled:
        h[s, :n] = R.random_reals(rng, 2 * n).view(np.complex128) if real_view else R.random_complex(rng, n)
    return h


def as_checked(v, real_view):
    """what the reference sees: the complex vector, or -- real_view -- the 2n reals it is a view of (as (re, 0) pairs: the same sums)"""
    return np.ascontiguousarray(v).view(np.float64) if real_view else v


def sentinel(*shape):
    return np.full(shape, SENT)


def scalars(**at):
    """NSCAL doubles, NaN (a read guard) but for the given slots, e.g. scalars(s2=0.5)"""
    s = np.full(NSCAL, NAN)
    for k, v in at.items():
        s[int(k[1:])] = v
    return s


def twice(run, what):
    """run() -> dict of host arrays; both runs start from fresh copies of the inputs and must agree bit for bit"""
    a, b = run(), run()
    for key in a:
        assert same_bits(a[key], b[key]), (what, key, "two runs differ")
    return a


def ok(rc, what):
    assert rc == 0, (what, "HIP status", rc)


def finish(lkc, d_partial, np_, op, what):
    """lz_final as the driver runs it (one block) into slot OUT_SLOT of a sentinel-filled scal -> the value"""
    sc = dev(sentinel(NSCAL))
    ok(lkc.lkc_final(1, ptr(d_partial), np_, ptr(sc), OUT_SLOT, op), what + ("lz_final",))
    sc = host(sc)
    assert same_bits(np.delete(sc, OUT_SLOT), sentinel(NSCAL - 1)), (what, "lz_final wrote another slot of scal")
    assert np.isfinite(sc[OUT_SLOT]), (what, "not finite", sc[OUT_SLOT])
    return sc[OUT_SLOT:OUT_SLOT + 1].copy()


def check_partial(part, grid, what):
    assert same_bits(part[grid:], sentinel(*part[grid:].shape)), (what, "partial rows beyond the grid were written")
    assert np.all(np.isfinite(part[:grid])), (what, "partial not finite")


def check_gaps(after, before, n, what):
    assert same_bits(after[..., n:], before[..., n:]), (what, "the gap [n, stride) changed")


# ---- lz_nrm -------------------------------------------------------------------------------------------------------------------------------
def run_nrm(lkc, x, n, grid, op, what):
    dx, dp = dev(x), dev(sentinel(grid + 2))
    ok(lkc.lkc_nrm(grid, n, ptr(dx), ptr(dp)), what)
    return dict(x=host(dx), partial=host(dp), out=finish(lkc, dp, grid, op, what))


@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_nrm(lkc, n, grid, op, view):
    what = ("lz_nrm", f"n={n}", f"grid={grid}", f"op={op}", view)
    rng = np.random.default_rng([21, n, grid, op])
    x = slots(rng, 1, n, [0], view == "real")
    r = twice(lambda: run_nrm(lkc, x, n, grid, op, what), what)
    assert same_bits(r["x"], x), (what, "the input changed")
    check_partial(r["partial"], grid, what)
    R.check_norm(r["out"][0], as_checked(x[0, :n], view == "real"), n, grid, op, what)


# ---- lz_sub_dot ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("mode", ["first", "ib"])
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_sub_dot(lkc, n, grid, mode, view):
    """w -= b qm, partial sums of Re <q|w>.  first: ib = -1, qm is a NaN buffer that must not be read and w is not written"""
    what = ("lz_sub_dot", f"n={n}", f"grid={grid}", mode, view)
    rng = np.random.default_rng([22, n, grid, mode == "ib"])
    V = slots(rng, 4, n, [0, 2] if mode == "first" else [0, 1, 2], view == "real")      # w, qm, q, NaN guard
    ib, b = (-1, None) if mode == "first" else (2, -0.8125 * 1.37)
    sc = scalars() if b is None else scalars(s2=b)

    def run():
        dV, ds, dp = dev(V), dev(sc), dev(sentinel(grid + 2))
        ok(lkc.lkc_sub_dot(grid, n, slot_ptr(dV, 0), slot_ptr(dV, 1), slot_ptr(dV, 2), ptr(ds), ib, ptr(dp)), what)
        return dict(V=host(dV), scal=host(ds), partial=host(dp), out=finish(lkc, dp, grid, 0, what))

    r = twice(run, what)
    assert same_bits(r["V"][1:], V[1:]) and same_bits(r["scal"], sc), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    check_partial(r["partial"], grid, what)
    R.check_sub_dot(r["V"][0, :n], r["out"][0], V[0, :n], V[1, :n], V[2, :n], b, n, grid, what)


# ---- lz_sub_nrm ---------------------------------------------------------------------------------------------------------------------------
def run_sub_nrm(lkc, V, sc, ia, n, grid, op, what):
    dV, ds, dp = dev(V), dev(sc), dev(sentinel(grid + 2))
    ok(lkc.lkc_sub_nrm(grid, n, slot_ptr(dV, 0), slot_ptr(dV, 1), ptr(ds), ia, ptr(dp)), what)
    return dict(V=host(dV), scal=host(ds), partial=host(dp), out=finish(lkc, dp, grid, op, what))


@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_sub_nrm(lkc, n, grid, view):
    what = ("lz_sub_nrm", f"n={n}", f"grid={grid}", view)
    rng = np.random.default_rng([23, n, grid])
    V = slots(rng, 3, n, [0, 1], view == "real")                                        # w, q, NaN guard
    a = 0.7310585786300049
    sc = scalars(s4=a)
    r = twice(lambda: run_sub_nrm(lkc, V, sc, 4, n, grid, 1, what), what)
    assert same_bits(r["V"][1:], V[1:]) and same_bits(r["scal"], sc), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    check_partial(r["partial"], grid, what)
    R.check_sub_nrm(r["V"][0, :n], r["out"][0], V[0, :n], V[1, :n], a, n, grid, 1, what)


# ---- lz_final -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("np_", [0, 1, 255, 256, 257, 1024, 9216])
def test_lz_final(lkc, np_, op):
    """9216 = (1 + 8) * RED_BLOCKS: the real-vector check of a start vector and eight probes in one reduction"""
    what = ("lz_final", f"np={np_}", f"op={op}")
    rng = np.random.default_rng([24, np_, op])
    p = np.concatenate([np.abs(R.random_reals(rng, np_)) if op else R.random_reals(rng, np_), [NAN]])

    def run():
        dp = dev(p)
        return dict(out=finish(lkc, dp, np_, op, what), partial=host(dp))

    r = twice(run, what)
    assert same_bits(r["partial"], p), (what, "the input changed")
    R.check_final(r["out"][0], p[:np_], op, what)


# ---- lz_sub_nrm_pair ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_sub_nrm_pair(lkc, n, grid):
    """per component against the reference; and bit for bit "paired = two single runs": w.re and partial_a are those of lz_sub_nrm on
    (w.re, 0), (q.re, 0) with a at the same n and grid, w.im and partial_b those of (w.im, 0), (q.im, 0) with b"""
    what = ("lz_sub_nrm_pair", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([25, n, grid])
    V = slots(rng, 3, n, [0, 1])
    a, b = 0.7310585786300049, -1.6180339887498949
    sc = scalars(s4=a, s12=b)

    def run():
        dV, ds, dpa, dpb = dev(V), dev(sc), dev(sentinel(grid + 2)), dev(sentinel(grid + 2))
        ok(lkc.lkc_sub_nrm_pair(grid, n, slot_ptr(dV, 0), slot_ptr(dV, 1), ptr(ds), 4, 12, ptr(dpa), ptr(dpb)), what)
        return dict(V=host(dV), scal=host(ds), pa=host(dpa), pb=host(dpb), oa=finish(lkc, dpa, grid, 1, what), ob=finish(lkc, dpb, grid, 1, what))

    r = twice(run, what)
    assert same_bits(r["V"][1:], V[1:]) and same_bits(r["scal"], sc), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    check_partial(r["pa"], grid, what)
    check_partial(r["pb"], grid, what)
    w = r["V"][0, :n]
    R.check_sub_nrm(w, None, V[0, :n], V[1, :n], a, n, grid, 1, what, b)
    R.check_norm(r["oa"][0], w.real, n, grid, 1, what + ("norm a",))
    R.check_norm(r["ob"][0], w.imag, n, grid, 1, what + ("norm b",))
    for name, part, coef, key, okey in (("re", np.real, a, "pa", "oa"), ("im", np.imag, b, "pb", "ob")):
        S = np.full(V.shape, CNAN)
        S[:2, :n] = part(V[:2, :n])                                                     # (x, 0)
        s = run_sub_nrm(lkc, S, scalars(s4=coef), 4, n, grid, 1, what + ("single", name))
        assert same_bits(s["V"][0, :n].real, part(w)), (what, name, "w differs from the single run")
        assert same_bits(s["V"][0, :n].imag, np.zeros(n)), (what, name, "the single run's zero component")
        assert same_bits(s["partial"], r[key]) and same_bits(s["out"], r[okey]), (what, name, "partial sums differ from the single run")


# ---- lz_pack_pair -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inputs", ["complex", "real"])
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_pack_pair(lkc, n, grid, inputs):
    what = ("lz_pack_pair", f"n={n}", f"grid={grid}", inputs)
    rng = np.random.default_rng([26, n, grid])
    V = slots(rng, 4, n, [0, 1])                                                        # a, b, q (NaN: written), NaN guard
    if inputs == "real":
        V[:2, :n] = V[:2, :n].real

    def run():
        dV, dpi, dpa, dpb = dev(V), dev(sentinel(grid + 2)), dev(sentinel(grid + 2)), dev(sentinel(grid + 2))
        ok(lkc.lkc_pack_pair(grid, n, slot_ptr(dV, 0), slot_ptr(dV, 1), slot_ptr(dV, 2), ptr(dpi), ptr(dpa), ptr(dpb)), what)
        return dict(V=host(dV), pi=host(dpi), pa=host(dpa), pb=host(dpb), oi=finish(lkc, dpi, grid, 0, what),
                    oa=finish(lkc, dpa, grid, 1, what), ob=finish(lkc, dpb, grid, 1, what))

    r = twice(run, what)
    assert same_bits(r["V"][[0, 1, 3]], V[[0, 1, 3]]), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    for key in ("pi", "pa", "pb"):
        check_partial(r[key], grid, what)
    R.check_bits(r["V"][2, :n], V[0, :n].real + 1j * V[1, :n].real, what + ("q = (Re a, Re b)",))
    im = np.concatenate([V[0, :n].imag, V[1, :n].imag])
    if inputs == "real":
        R.check_bits(r["oi"], np.zeros(1), what + ("p_im of real inputs",))
    else:
        # (a visit adds Im(a_i)^2 + Im(b_i)^2: the sum of two products, then the accumulation -- the two roundings per visit of chain_depth)
        ref, ab = R.sumsq(im)
        R.check_scalar_sum(r["oi"][0], ref, ab, R.chain_depth(n, grid, grid), what + ("p_im",))
    for name, src, key, okey in (("a", 0, "pa", "oa"), ("b", 1, "pb", "ob")):
        S = np.full((1, V.shape[1]), CNAN)
        S[0, :n] = V[src, :n].real
        s = run_nrm(lkc, S, n, grid, 1, what + ("lz_nrm", name))
        assert same_bits(s["partial"], r[key]) and same_bits(s["out"], r[okey]), (what, name, "not the bits of lz_nrm on (Re, 0)")
        R.check_norm(r[okey][0], V[src, :n].real, n, grid, 1, what + ("norm", name))


# ---- lz_probe_dots, lz_probe_final --------------------------------------------------------------------------------------------------------
def run_probes(lkc, V, js, x_slot, n, grid, real, what):
    """the probes in slots `js` of V against slot x_slot, through launch_probe_dots"""
    m = len(js)
    dV, dp, do = dev(V), dev(sentinel(grid + 2, 2 * m)), dev(sentinel(2 * m + 2))
    plist = (C.c_void_p * m)(*[slot_ptr(dV, j) for j in js])
    ok(lkc.lkc_probe_dots(grid, real, m, n, slot_ptr(dV, x_slot), plist, ptr(dp), ptr(do)), what)
    return dict(V=host(dV), partial=host(dp), out=host(do))


def probe_cases():
    out = [pytest.param(m, real, n, g, id=f"M{m}-{'real' if real else 'complex'}-n{n}-grid{g}") for m in range(1, 9) for real in (0, 1) for n, g in SIZES]
    return out + [pytest.param(8, 0, *DRIVER, id="M8-complex-driver-geometry"), pytest.param(3, 1, *DRIVER, id="M3-real-driver-geometry")]


@pytest.mark.parametrize("m,real,n,grid", probe_cases())
def test_lz_probe_dots(lkc, m, real, n, grid):
    """every instance of the switch on M, with pairwise different probes: Re and Im <p_j|x> within their own bounds, slot by slot; REAL: the
    imaginary slots are +0.0; probe j of the M-probe call has the bits of that probe alone through the M = 1 instance"""
    what = ("lz_probe_dots", f"M={m}", f"real={real}", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([27, m, real, n, grid])
    V = slots(rng, m + 2, n, range(m + 1), bool(real))                                  # probes 0..m-1, x in slot m, NaN guard
    r = twice(lambda: run_probes(lkc, V, list(range(m)), m, n, grid, real, what), what)
    assert same_bits(r["V"], V), (what, "an input changed")
    check_partial(r["partial"], grid, what)
    R.check_probe_output(r["out"], as_checked(V[:m, :n], bool(real)), as_checked(V[m, :n], bool(real)), n, grid, bool(real), what)
    out = r["out"][:2 * m]
    if m > 1:
        for j in range(m):
            s = run_probes(lkc, V, [j], m, n, grid, real, what + ("alone", j))
            assert same_bits(s["out"][:2], out[2 * j:2 * j + 2]), (what, f"probe {j} differs from the same probe alone", s["out"][:2], out[2 * j:2 * j + 2])
            assert same_bits(s["partial"][:grid].ravel(), r["partial"][:grid, 2 * j:2 * j + 2].ravel()), (what, f"probe {j}: block partials differ")


@pytest.mark.parametrize("nc", [2, 5, 16])
@pytest.mark.parametrize("np_", [0, 1, 255, 256, 257, 1024])
def test_lz_probe_final(lkc, np_, nc):
    what = ("lz_probe_final", f"np={np_}", f"nc={nc}")
    rng = np.random.default_rng([28, np_, nc])
    p = np.full((np_ + 1, nc), NAN)
    p[:np_] = R.random_reals(rng, (np_, nc))

    def run():
        dp, do = dev(p), dev(sentinel(nc + 2))
        ok(lkc.lkc_probe_final(1, ptr(dp), np_, nc, ptr(do)), what)
        return dict(partial=host(dp), out=host(do))

    r = twice(run, what)
    assert same_bits(r["partial"], p), (what, "the input changed")
    assert same_bits(r["out"][nc:], sentinel(2)), (what, "wrote beyond nc")
    R.check_probe_final(r["out"][:nc], p[:np_], what)


# ---- lz_scale, lz_axpy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_scale(lkc, n, grid, in_place):
    what = ("lz_scale", f"n={n}", f"grid={grid}", f"in_place={in_place}")
    rng = np.random.default_rng([29, n, grid])
    V = slots(rng, 3, n, [0])                                                           # w, q (NaN: written), NaN guard
    s = 3.7320508075688772
    sc = scalars(s1=s)
    qs = 0 if in_place else 1

    def run():
        dV, ds = dev(V), dev(sc)
        ok(lkc.lkc_scale(grid, n, slot_ptr(dV, qs), slot_ptr(dV, 0), ptr(ds), 1), what)
        return dict(V=host(dV), scal=host(ds))

    r = twice(run, what)
    assert same_bits(r["scal"], sc) and same_bits(np.delete(r["V"], qs, axis=0), np.delete(V, qs, axis=0)), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    R.check_scale(r["V"][qs, :n], V[0, :n], s, what)


@pytest.mark.parametrize("n,grid", ALL_SIZES)
def test_lz_axpy(lkc, n, grid):
    what = ("lz_axpy", f"n={n}", f"grid={grid}")
    rng = np.random.default_rng([30, n, grid])
    V = slots(rng, 3, n, [0, 1])                                                        # y, q, NaN guard
    c = -0.4142135623730951

    def run():
        dV = dev(V)
        ok(lkc.lkc_axpy(grid, n, slot_ptr(dV, 0), slot_ptr(dV, 1), c), what)
        return dict(V=host(dV))

    r = twice(run, what)
    assert same_bits(r["V"][1:], V[1:]), (what, "an input changed")
    check_gaps(r["V"], V, n, what)
    R.check_axpy(r["V"][0, :n], V[0, :n], c, V[1, :n], what)


# ---- lz_init, lz_init_real ----------------------------------------------------------------------------------------------------------------
DIMUPS = [1, 7, 8, 9, 70]
QDWS = [0, 1, 3]
SEEDS = [0, 1, 2 ** 63 + 12345]


def up8(x):
    return (x + 7) // 8 * 8


def up16(x):
    return (x + 15) // 16 * 16


def run_init(lkc, real, grid, seed, dimup, pitch, qdw, col0, iperm, sign, what):
    """-> the [qdw, pitch] vector; the buffer starts as NaN and keeps 8 NaN behind the vector"""
    n = pitch * qdw
    buf = np.full(n + 8, NAN if real else CNAN)
    dq = dev(buf)
    di = None if iperm is None else dev(np.concatenate([iperm, [2 ** 31 - 1]]).astype(np.int32))      # (a guard entry no row may use)
    dg = None if sign is None else dev(np.concatenate([sign, [1]]).astype(np.uint8))
    fn = lkc.lkc_init_real if real else lkc.lkc_init
    ok(fn(grid, n, ptr(dq), seed, dimup, pitch, col0, ptr(di), ptr(dg)), what)
    q = host(dq)
    assert same_bits(q[n:], buf[n:]), (what, "wrote behind the vector")
    return q[:n].reshape(qdw, pitch)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("order", ["identity", "permuted"])
@pytest.mark.parametrize("col0", [0, 5])
@pytest.mark.parametrize("qdw", QDWS)
@pytest.mark.parametrize("dimup", DIMUPS)
def test_lz_init(lkc, dimup, qdw, col0, order, seed):
    """both start vectors, bit for bit against the uint64 restatement; pad rows exactly zero; the real vector is the real part of the
    complex one.  Two blocks for at most 240 elements: the second one is partly or wholly beyond n"""
    what = ("lz_init", f"dimup={dimup}", f"qdw={qdw}", f"col0={col0}", order, f"seed={seed}")
    rng = np.random.default_rng([31, dimup, qdw, col0])
    iperm = sign = None
    if order == "permuted":
        iperm, sign = rng.permutation(dimup).astype(np.int32), rng.integers(0, 2, dimup).astype(np.uint8)
    pc, pr = up8(dimup), up16(dimup)
    zc = twice(lambda: dict(q=run_init(lkc, 0, 2, seed, dimup, pc, qdw, col0, iperm, sign, what)), what)["q"]
    zr = twice(lambda: dict(q=run_init(lkc, 1, 2, seed, dimup, pr, qdw, col0, iperm, sign, what + ("real",))), what)["q"]
    R.check_bits(zc, R.init(seed, dimup, pc, qdw, col0, iperm, sign), what)
    R.check_bits(zr, R.init_real(seed, dimup, pr, qdw, col0, iperm, sign), what + ("real",))
    assert same_bits(zc[:, dimup:], np.zeros((qdw, pc - dimup), dtype=np.complex128)), (what, "complex pad rows")
    assert same_bits(zr[:, dimup:], np.zeros((qdw, pr - dimup))), (what, "real pad rows")
    assert same_bits(zr[:, :dimup], np.ascontiguousarray(zc[:, :dimup].real)), (what, "the real vector is not the real part")
    assert np.all(np.abs(zc.real) <= 0.5) and np.all(np.abs(zc.imag) <= 0.5)


@pytest.mark.parametrize("real", [0, 1])
@pytest.mark.parametrize("dimup", [7, 70])
def test_lz_init_slabs_concatenate(lkc, dimup, real):
    """a split sector starts from the unsplit vector: the slabs of col0 = 0, 2, 5 (2, 3 and 1 columns) side by side are the vector of six columns"""
    what = ("lz_init slabs", f"dimup={dimup}", f"real={real}")
    rng = np.random.default_rng([32, dimup])
    iperm, sign = rng.permutation(dimup).astype(np.int32), rng.integers(0, 2, dimup).astype(np.uint8)
    pitch, seed = (up16 if real else up8)(dimup), 0x5EED5EED
    whole = run_init(lkc, real, 3, seed, dimup, pitch, 6, 0, iperm, sign, what)
    parts = [run_init(lkc, real, 1, seed, dimup, pitch, q, c0, iperm, sign, what) for c0, q in ((0, 2), (2, 3), (5, 1))]
    assert same_bits(np.concatenate(parts, axis=0), whole), what


# ---- lz_to_real, lz_to_complex ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdw", QDWS)
@pytest.mark.parametrize("dimup", DIMUPS)
def test_lz_to_real_and_back(lkc, dimup, qdw):
    """the data rows are copied exactly and the pads are zero; dst == nullptr only reduces, partial == nullptr only converts;
    lz_to_complex(lz_to_real(x)) has the bits of Re x.  The pad rows of the source hold NaN: they must not be read"""
    what = ("lz_to_real", f"dimup={dimup}", f"qdw={qdw}")
    rng = np.random.default_rng([33, dimup, qdw])
    pc, pr, grid = up8(dimup), up16(dimup), 2
    src = np.full((qdw + 1, pc), CNAN)                                                  # (one NaN column behind)
    src[:qdw, :dimup] = R.random_complex(rng, (qdw, dimup))
    dst0 = np.full(qdw * pr + 8, NAN)

    def run(with_dst, with_partial):
        ds, dd, dp = dev(src), dev(dst0), dev(sentinel(grid + 2))
        ok(lkc.lkc_to_real(grid, dimup, qdw, pc, pr, ptr(ds), ptr(dd) if with_dst else None, ptr(dp) if with_partial else None), what)
        out = finish(lkc, dp, grid, 0, what) if with_partial else sentinel(1)
        return dict(src=host(ds), dst=host(dd), partial=host(dp), out=out)

    expect, (ref, ab) = R.to_real(src[:qdw], dimup, pr)
    depth = R.chain_depth(qdw * pr, grid, grid)
    for with_dst, with_partial in ((1, 1), (0, 1), (1, 0)):
        w = what + (f"dst={with_dst}", f"partial={with_partial}")
        r = twice(lambda: run(with_dst, with_partial), w)
        assert same_bits(r["src"], src), (w, "the input changed")
        if with_dst:
            R.check_bits(r["dst"][:qdw * pr].reshape(qdw, pr), expect, w)
            assert same_bits(r["dst"][qdw * pr:], dst0[qdw * pr:]), (w, "wrote behind the vector")
        else:
            assert same_bits(r["dst"], dst0), (w, "dst written though none was passed")
        if with_partial:
            check_partial(r["partial"], grid, w)
            R.check_scalar_sum(r["out"][0], ref, ab, depth, w + ("sum Im^2",))
        else:
            assert same_bits(r["partial"], sentinel(grid + 2)), (w, "partial written though none was passed")

    # back: real [qdw, pr] with NaN pads (not to be read) -> complex [qdw, pc]
    real = np.full((qdw + 1, pr), NAN)
    real[:qdw, :dimup] = expect[:, :dimup]
    back0 = np.full(qdw * pc + 8, CNAN)

    def run_back():
        ds, dd = dev(real), dev(back0)
        ok(lkc.lkc_to_complex(grid, dimup, qdw, pc, pr, ptr(ds), ptr(dd)), what + ("lz_to_complex",))
        return dict(src=host(ds), dst=host(dd))

    r = twice(run_back, what + ("lz_to_complex",))
    assert same_bits(r["src"], real) and same_bits(r["dst"][qdw * pc:], back0[qdw * pc:]), (what, "lz_to_complex: input changed or wrote behind")
    back = r["dst"][:qdw * pc].reshape(qdw, pc)
    R.check_bits(back, R.to_complex(real[:qdw], dimup, pc), what + ("lz_to_complex",))
    assert same_bits(np.ascontiguousarray(back[:, :dimup].real), np.ascontiguousarray(src[:qdw, :dimup].real)), (what, "round trip")
    assert same_bits(back[:, dimup:], np.zeros((qdw, pc - dimup), dtype=np.complex128)) and not np.any(back.imag), (what, "pads or imaginary parts")


# ---- the scalar chain ---------------------------------------------------------------------------------------------------------------------
def test_lz_mul_and_lz_sqrt(lkc):
    """IEEE double product and square root: the bits of the host's; every other slot untouched"""
    rng = np.random.default_rng(34)
    for _ in range(20):
        sc = sentinel(NSCAL)
        a, b = R.random_reals(rng, 2) * 10.0 ** rng.uniform(-100, 100, 2)
        sc[0], sc[2] = a, b
        d = dev(sc)
        ok(lkc.lkc_mul(1, ptr(d), 4, 0, 2), "lz_mul")
        got = host(d)
        expect = sc.copy()
        expect[4] = a * b
        R.check_bits(got, expect, ("lz_mul", a, b))
        sc[7] = abs(a)
        d = dev(sc)
        ok(lkc.lkc_sqrt(1, ptr(d), 7), "lz_sqrt")
        expect = sc.copy()
        expect[7] = np.sqrt(abs(a))
        R.check_bits(host(d), expect, ("lz_sqrt", a))


def test_lz_next_chain(lkc):
    """50 successive lz_next steps on random betas of magnitude 1e-150 .. 1e150 (this file's choice: the project records no such sequence),
    nmax = 40: LZ_S and LZ_C have the bits of the host's LzScale::next() + c() (compiled from the same header) and of plain IEEE double;
    alpha_out[k] and beta_out[k + 1] are written for k < nmax only, sentinels behind; LZ_STEP counts up; nothing else changes"""
    rng = np.random.default_rng(35)
    steps, nmax = 50, 40
    betas = 10.0 ** rng.uniform(-150, 150, steps + 1)
    alphas = R.random_reals(rng, steps)
    sc = sentinel(NSCAL)
    sc[R.LZ_S], sc[R.LZ_C], sc[R.LZ_STEP] = 1.0 / betas[0], 0.0, 1.0
    a_ref, b_ref = sentinel(nmax + 2), sentinel(nmax + 2)
    d_a, d_b = dev(a_ref), dev(b_ref)
    state = (C.c_double * 2)(sc[R.LZ_S], betas[0])
    for k in range(steps):
        sc[R.LZ_ALPHA], sc[R.LZ_BETA] = alphas[k], betas[k + 1]
        d = dev(sc)
        ok(lkc.lkc_next(1, ptr(d), ptr(d_a), ptr(d_b), nmax), ("lz_next", k))
        R.next_step(sc, a_ref, b_ref, nmax)
        got = host(d)
        R.check_bits(got, sc, ("lz_next", k, "scal against IEEE double"))
        c = C.c_double(0.0)
        lkc.lkc_host_scale_next(state, betas[k + 1], C.byref(c))
        assert same_bits(got[[R.LZ_S, R.LZ_C]], np.array([state[0], c.value])), ("lz_next", k, "LzScale on the host", got, state[0], c.value)
        assert got[R.LZ_STEP] == k + 2 and np.all(np.isfinite(got[[R.LZ_S, R.LZ_C]]))
        R.check_bits(host(d_a), a_ref, ("lz_next", k, "alpha_out"))
        R.check_bits(host(d_b), b_ref, ("lz_next", k, "beta_out"))
    assert same_bits(a_ref[nmax:], sentinel(2)) and same_bits(b_ref[nmax:], sentinel(2)) and b_ref[0] == SENT and a_ref[0] == SENT
    assert same_bits(a_ref[1:nmax], alphas[:nmax - 1]) and same_bits(b_ref[2:nmax], betas[1:nmax - 1])


# ---- tridiag_ql's contract: no caller passes n = 0 ------------------------------------------------------------------------------------------
def test_every_caller_refuses_nlanc_below_one(built):
    """tridiag_ql writes e[n - 1]: n = 0 is outside its contract (tests/test_host_lanczos_check.py never calls it so).  Every entry that
    reaches it refuses nlanc / nitermax / nsteps < 1 with HXV_ERR_ARG before anything runs"""
    import torch

    import hxv
    from hxv import models

    L = hxv.load_library()
    sec = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), 3, 3)
    v = models.deterministic_vector(sec.Dim).astype(np.complex128)
    dv = torch.zeros(sec.pitch * sec.DimDw, dtype=torch.complex128, device="cuda")
    a, b = np.zeros(4), np.zeros(4)
    pd = C.POINTER(C.c_double)
    pa, pb = a.ctypes.data_as(pd), b.ctypes.data_as(pd)
    n1, n2, e = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    err_arg = 1
    for nl in (0, -1):
        assert L.hxv_lanczos_tridiag(sec._h, dv.data_ptr(), nl, pa, pb, 0.0, C.byref(n1)) == err_arg
        assert L.hxv_lanczos_tridiag_probes(sec._h, dv.data_ptr(), 0, None, nl, pa, pb, None, 0.0, C.byref(n1)) == err_arg
        assert L.hxv_lanczos_tridiag_pair(sec._h, dv.data_ptr(), dv.data_ptr(), nl, pa, pb, pa, pb, 0.0, C.byref(n1), C.byref(n2)) == err_arg
        assert L.hxv_lanczos_eigh(sec._h, nl, 1e-12, C.byref(e), None, C.byref(n1)) == err_arg
        assert L.hxv_lanczos_tridiag_host(sec._h, v.ctypes.data, nl, pa, pb, 0.0, C.byref(n1)) == err_arg
        assert L.hxv_lanczos_tridiag_pair_host(sec._h, v.ctypes.data, v.ctypes.data, nl, pa, pb, pa, pb, 0.0, C.byref(n1), C.byref(n2)) == err_arg
        assert L.hxv_lanczos_eigh_host(sec._h, nl, 1e-12, C.byref(e), None, C.byref(n1)) == err_arg
        assert L.hxv_gf_from_probes(nl, pa, pb, 0, None, 1.0, pa, None) == err_arg
