"""The checks of tests/lanczos_kernels_ref.py bite, and their bounds hold (no GPU, no kernel).

For every kernel of csrc/hxv_lanczos_kernels.hpp there is a numpy restatement in double precision IN THE KERNEL'S ORDER (the emu_* functions
of lanczos_kernels_ref.py, or a plain Python loop here): thread-strided accumulation, the eight-level tree of block_sum, lz_final's second
stage, fused multiply-adds where the kernel has them.  It is fed to the SAME check functions tests/test_gpu_lanczos_kernels.py feeds the
device's output to, and must pass at every (n, grid) of that file, the driver's geometry included -- which also shows, for every input
generator, that reference and bound agree with a correct computation.  Then one named mistake at a time is switched on (a lost last
element, a lost or doubled partial sum, the gap read as data, a probe in the wrong slot, the conjugate overlap, a forgotten or doubled
square root, a pad row not zeroed, iperm used as perm, sign / col0 ignored, re and im from one hash, c = s_new / s_old, ...) and the same
check must refuse it.

Bounds, in one paragraph: a term of a sum passes D = 2 ceil(n / (256 grid)) + 8 (+ ceil(np / 256) + 8 through the finishing kernel)
additions and the tolerance is gamma(D + 2) sum|t_i|; elementwise u |x - a y| for the fused update (plus the reference's own 2**-63),
gamma(2) of the magnitudes for the two-rounding updates; everything else is compared bit for bit.
Wall time: 1029 cases in 6 s."""
import math
from fractions import Fraction

import numpy as np
import pytest

import lanczos_kernels_ref as R

NS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
GRIDS = [1, 2, 3]
DRIVER = (R.RED_BLOCKS * 256 + 513, R.RED_BLOCKS)
SHAPES = [pytest.param(n, g, id=f"n{n}-grid{g}") for n in NS for g in GRIDS] + [pytest.param(*DRIVER, id="driver-geometry")]
MUT_SHAPES = [(257, 1), (257, 2), (1000, 3), (65, 1)]          # where the mistakes are switched on (every one has n > 0 and a ragged round)
NAN = float("nan")
SENT = R.SENT


def refuses(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def vec(rng, n, real_view=False):
    return R.random_reals(rng, 2 * n).view(np.complex128) if real_view else R.random_complex(rng, n)


def checked(v, real_view):
    return np.ascontiguousarray(v).view(np.float64) if real_view else v


def reduce_(terms, n, grid, op=0, mutant=None, final_mutant=None):
    return R.emu_final(R.emu_partials(terms, n, grid, mutant), op, final_mutant)


# ---- the tools themselves -------------------------------------------------------------------------------------------------------------------
def test_tools():
    assert np.finfo(np.longdouble).nmant >= 63
    assert R.chain_depth(1000, 2) == 2 * 2 + 8 and R.chain_depth(1000, 2, 2) == 2 * 2 + 8 + 1 + 8 and R.chain_depth(None, 1, 257) == 2 + 8
    assert R.chain_depth(0, 3) == 8 and R.chain_depth(*DRIVER, DRIVER[1]) == 4 + 8 + 4 + 8 and R.chain_depth(None, 1, 9216) == 36 + 8
    # fma64 is a correctly rounded fused multiply-add on data with heavy cancellation
    rng = np.random.default_rng(1)
    a, b = R.random_reals(rng, 3000), R.random_reals(rng, 3000)
    c = -(a * b) * (1.0 + rng.choice([0.0, 1e-15, 1e-12, 1e-3, 1.0], 3000))
    got = R.fma64(a, b, c)
    for i in range(3000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert got[i] == float(exact), (i, a[i], b[i], c[i])     # (float(Fraction) rounds to nearest even)
    # the tree adds in block_sum's order (t with t + 128, then t with t + 64, ...): 1 in thread 0 and half an ulp in threads 64 and 128 are
    # lost one after the other; any order that adds the two halves first would give 1 + 2**-52
    x = np.zeros(256)
    x[0], x[64], x[128] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert R._tree(x) == 1.0 and (x[64] + x[128]) + x[0] == 1.0 + 2.0 ** -52
    assert R._tree(np.ones(256)) == 256.0
    # uniform: range, and the first value of splitmix64 from state 0 (0xE220A8397B1DCDAF, Vigna's reference sequence)
    u0 = R.uniform(np.array([0], dtype=np.uint64))[0]
    assert u0 == (0xE220A8397B1DCDAF >> 11) / 2.0 ** 53 - 0.5
    u = R.uniform(np.arange(100000, dtype=np.uint64))
    assert u.min() >= -0.5 and u.max() < 0.5 and abs(u.mean()) < 0.01 and len(np.unique(u)) == 100000


# ---- lz_nrm, lz_final -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("n,grid", SHAPES)
def test_nrm_accepts_the_kernel_order(n, grid, op, view):
    rng = np.random.default_rng([21, n, grid, op])
    x = vec(rng, n, view == "real")
    R.check_norm(reduce_(R.emu_nrm_terms(x), n, grid, op), checked(x, view == "real"), n, grid, op, ("lz_nrm",))


@pytest.mark.parametrize("n,grid", MUT_SHAPES)
def test_nrm_refuses_mistakes(n, grid):
    rng = np.random.default_rng([21, n, grid])
    x = vec(rng, n)
    t = R.emu_nrm_terms(x)
    for op in (0, 1):
        R.check_norm(reduce_(t, n, grid, op), x, n, grid, op, ("lz_nrm",))
        refuses(R.check_norm, reduce_(t, n, grid, op, "drop_last"), x, n, grid, op, ("last element lost",))
        refuses(R.check_norm, reduce_(t, n, grid, op, "drop_block"), x, n, grid, op, ("one block's partial lost",))
        refuses(R.check_norm, reduce_(t, n, grid, op, None, "twice"), x, n, grid, op, ("a partial added twice",))
    gap = np.concatenate([x, np.full(8, complex(NAN, NAN))])
    refuses(R.check_norm, reduce_(R.emu_nrm_terms(gap), n + 8, grid, 0), x, n, grid, 0, ("the gap read as data",))
    refuses(R.check_norm, reduce_(t, n, grid, 1, None, "no_sqrt"), x, n, grid, 1, ("sqrt forgotten",))
    refuses(R.check_norm, reduce_(t, n, grid, 1, None, "sqrt_twice"), x, n, grid, 1, ("sqrt applied twice",))
    refuses(R.check_norm, reduce_(t, n, grid, 1), x, n, grid, 0, ("sqrt applied where op = 0",))


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("np_", [0, 1, 255, 256, 257, 1024, 9216])
def test_final(np_, op):
    rng = np.random.default_rng([24, np_, op])
    p = np.abs(R.random_reals(rng, np_)) if op else R.random_reals(rng, np_)
    R.check_final(R.emu_final(p, op), p, op, ("lz_final",))
    if np_ == 0:
        return
    refuses(R.check_final, R.emu_final(p, op, "drop_last"), p, op, ("last partial lost",))
    refuses(R.check_final, R.emu_final(p, op, "twice"), p, op, ("a partial added twice",))
    if np_ % 256:
        refuses(R.check_final, R.emu_final(p[:np_ - np_ % 256], op), p, op, ("the ragged last round lost",))
    if op:
        refuses(R.check_final, R.emu_final(p, 1, "no_sqrt"), p, 1, ("sqrt forgotten",))
        refuses(R.check_final, R.emu_final(p, 1, "sqrt_twice"), p, 1, ("sqrt applied twice",))
    refuses(R.check_final, NAN, p, op, ("NaN",))


@pytest.mark.parametrize("nc", [2, 5, 16])
@pytest.mark.parametrize("np_", [0, 1, 255, 256, 257, 1024])
def test_probe_final(np_, nc):
    rng = np.random.default_rng([28, np_, nc])
    p = R.random_reals(rng, (np_, nc))
    good = np.array([R.emu_final(p[:, c]) for c in range(nc)])
    R.check_probe_final(good, p, ("lz_probe_final",))
    if np_:
        refuses(R.check_probe_final, np.roll(good, 1), p, ("columns shifted",))
        refuses(R.check_probe_final, np.array([R.emu_final(p[:, c], 0, "drop_last") for c in range(nc)]), p, ("last row lost",))
        if np_ > 1:
            refuses(R.check_probe_final, np.array([R.emu_final(p.ravel()[c * np_:(c + 1) * np_]) for c in range(nc)]), p, ("partial read transposed",))


# ---- lz_sub_dot -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("mode", ["first", "ib"])
@pytest.mark.parametrize("n,grid", SHAPES)
def test_sub_dot_accepts_the_kernel_order(n, grid, mode, view):
    rng = np.random.default_rng([22, n, grid, mode == "ib"])
    w, qm, q = (vec(rng, n, view == "real") for _ in range(3))
    b = None if mode == "first" else -0.8125 * 1.37
    wa, t = R.emu_sub_dot(w, b, qm, q)
    R.check_sub_dot(wa, reduce_(t, n, grid), w, qm, q, b, n, grid, ("lz_sub_dot",))


@pytest.mark.parametrize("n,grid", MUT_SHAPES)
def test_sub_dot_refuses_mistakes(n, grid):
    rng = np.random.default_rng([22, n, grid])
    w, qm, q = (vec(rng, n) for _ in range(3))
    b = 1.1131
    wa, t = R.emu_sub_dot(w, b, qm, q)
    args = (w, qm, q, b, n, grid)
    R.check_sub_dot(wa, reduce_(t, n, grid), *args, ("lz_sub_dot",))
    refuses(R.check_sub_dot, wa, reduce_(t, n, grid, 0, "drop_last"), *args, ("last element lost",))
    refuses(R.check_sub_dot, wa, reduce_(t, n, grid, 0, "drop_block"), *args, ("a block lost",))
    refuses(R.check_sub_dot, wa, reduce_(t, n, grid, 0, None, "twice"), *args, ("a partial twice",))
    stale = wa.copy()
    stale[n - 1] = w[n - 1]
    refuses(R.check_sub_dot, stale, reduce_(t, n, grid), *args, ("last element of w not written",))
    w0, t0 = R.emu_sub_dot(w, None, qm, q)
    refuses(R.check_sub_dot, w0, reduce_(t0, n, grid), *args, ("b ignored",))
    refuses(R.check_sub_dot, wa, reduce_(t0, n, grid), *args, ("the dot taken with the old w",))
    wp, tp = R.emu_sub_dot(w, -b, qm, q)
    refuses(R.check_sub_dot, wp, reduce_(tp, n, grid), *args, ("w += b qm",))
    # ib = -1: qm is a NaN buffer; a kernel that reads it, or writes w, is refused
    nanq = np.full(n, complex(NAN, NAN))
    first = (w, nanq, q, None, n, grid)
    R.check_sub_dot(w0, reduce_(t0, n, grid), *first, ("ib = -1",))
    wn, tn = R.emu_sub_dot(w, 0.0, nanq, q)
    refuses(R.check_sub_dot, wn, reduce_(tn, n, grid), *first, ("qm read with ib = -1",))
    refuses(R.check_sub_dot, wa, reduce_(t0, n, grid), *first, ("w written with ib = -1",))
    _, tc = R.emu_sub_dot(w, None, qm, np.conj(q) * 1j)
    refuses(R.check_sub_dot, w0, reduce_(tc, n, grid), *first, ("the imaginary part of the overlap",))


# ---- lz_sub_nrm, lz_sub_nrm_pair --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["complex", "real"])
@pytest.mark.parametrize("n,grid", SHAPES)
def test_sub_nrm_accepts_the_kernel_order(n, grid, view):
    rng = np.random.default_rng([23, n, grid])
    w, q = vec(rng, n, view == "real"), vec(rng, n, view == "real")
    a = 0.7310585786300049
    wa = R.emu_sub_nrm(w, a, q)
    R.check_sub_nrm(wa, reduce_(R.emu_nrm_terms(wa), n, grid, 1), w, q, a, n, grid, 1, ("lz_sub_nrm",))
    # the paired kernel: two coefficients, two sums
    b = -1.6180339887498949
    wp = R.emu_sub_nrm(w, a, q, b)
    R.check_sub_nrm(wp, None, w, q, a, n, grid, 1, ("lz_sub_nrm_pair",), b)
    R.check_norm(reduce_(wp.real * wp.real, n, grid, 1), wp.real, n, grid, 1, ("pair, norm a",))
    R.check_norm(reduce_(wp.imag * wp.imag, n, grid, 1), wp.imag, n, grid, 1, ("pair, norm b",))


@pytest.mark.parametrize("n,grid", MUT_SHAPES)
def test_sub_nrm_refuses_mistakes(n, grid):
    rng = np.random.default_rng([23, n, grid])
    w, q = vec(rng, n), vec(rng, n)
    a, b = 0.7310585786300049, -1.6180339887498949
    wa = R.emu_sub_nrm(w, a, q)
    nrm = reduce_(R.emu_nrm_terms(wa), n, grid, 1)
    args = (w, q, a, n, grid, 1)
    R.check_sub_nrm(wa, nrm, *args, ("lz_sub_nrm",))
    # the sharp bound: an update that is one ulp off somewhere is already outside
    ulp = wa.copy()
    ulp[7] = np.nextafter(np.nextafter(ulp[7].real, np.inf), np.inf) + 1j * ulp[7].imag
    refuses(R.check_sub_nrm, ulp, None, *args, ("one component two ulps off",))
    refuses(R.check_sub_nrm, R.emu_sub_nrm(w, -a, q), None, *args, ("w += a q",))
    stale = wa.copy()
    stale[n - 1] = w[n - 1]
    refuses(R.check_sub_nrm, stale, None, *args, ("last element not written",))
    refuses(R.check_sub_nrm, wa, reduce_(R.emu_nrm_terms(w), n, grid, 1), *args, ("the norm of the old w",))
    refuses(R.check_sub_nrm, wa, reduce_(R.emu_nrm_terms(wa), n, grid, 1, "drop_last"), *args, ("last element lost",))
    refuses(R.check_sub_nrm, wa, reduce_(R.emu_nrm_terms(wa), n, grid, 1, None, "no_sqrt"), *args, ("sqrt forgotten",))
    wp = R.emu_sub_nrm(w, a, q, b)
    R.check_sub_nrm(wp, None, *args, ("pair",), b)
    refuses(R.check_sub_nrm, R.emu_sub_nrm(w, b, q, a), None, *args, ("pair, coefficients exchanged",), b)
    refuses(R.check_sub_nrm, wa, None, *args, ("pair, a used for both",), b)
    refuses(R.check_norm, reduce_(wp.imag * wp.imag, n, grid, 1), wp.real, n, grid, 1, ("pair, the two sums exchanged",))
    refuses(R.check_norm, reduce_(R.emu_nrm_terms(wp), n, grid, 1), wp.real, n, grid, 1, ("pair, one sum over both components",))


# ---- lz_pack_pair -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grid", SHAPES)
def test_pack_pair(n, grid):
    rng = np.random.default_rng([26, n, grid])
    a, b = vec(rng, n), vec(rng, n)
    q = a.real + 1j * b.real
    R.check_bits(q, a.real + 1j * b.real, ("q",))
    im = np.concatenate([a.imag, b.imag])
    ref, ab = R.sumsq(im)
    t = a.imag * a.imag + b.imag * b.imag
    d = R.chain_depth(n, grid, grid)
    R.check_scalar_sum(reduce_(t, n, grid), ref, ab, d, ("p_im",))
    R.check_norm(reduce_(a.real * a.real, n, grid, 1), a.real, n, grid, 1, ("p_a",))
    if n:
        refuses(R.check_bits, a.real + 1j * a.imag, q, ("q = a",))
        refuses(R.check_scalar_sum, reduce_(a.imag * a.imag, n, grid), ref, ab, d, ("Im b left out",))
        refuses(R.check_norm, reduce_(b.real * b.real, n, grid, 1), a.real, n, grid, 1, ("p_a and p_b exchanged",))
        refuses(R.check_bits, np.array([5e-324]), np.zeros(1), ("p_im of real inputs not exactly zero",))


# ---- lz_probe_dots ----------------------------------------------------------------------------------------------------------------------------
def emu_probes(P, x, n, grid, real, mutant=None):
    """-> out[2 M + 2], the last two a sentinel, as the GPU test lays it out"""
    m = P.shape[0]
    out = np.full(2 * m + 2, SENT)
    for j in range(m):
        re, im = R.emu_probe_terms(P[j], x, "conj" if mutant == "conj" else None)
        out[2 * j] = reduce_(re, n, grid)
        out[2 * j + 1] = 0.0 if (real and mutant != "real_im") else reduce_(im, n, grid)
    if mutant == "slot":            # probe M - 1 is reported in slot M
        out[2 * m:2 * m + 2] = out[2 * m - 2:2 * m]
        out[2 * m - 2:2 * m] = SENT
    if mutant == "swap" and m > 1:
        out[:4] = out[[2, 3, 0, 1]]
    return out


def probe_shapes():
    out = [pytest.param(m, real, n, g, id=f"M{m}-{'real' if real else 'complex'}-n{n}-grid{g}") for m in range(1, 9) for real in (0, 1) for n in NS for g in GRIDS]
    return out + [pytest.param(8, 0, *DRIVER, id="M8-complex-driver-geometry"), pytest.param(3, 1, *DRIVER, id="M3-real-driver-geometry")]


@pytest.mark.parametrize("m,real,n,grid", probe_shapes())
def test_probes_accept_the_kernel_order(m, real, n, grid):
    rng = np.random.default_rng([27, m, real, n, grid])
    P, x = np.array([vec(rng, n, bool(real)) for _ in range(m)]).reshape(m, n), vec(rng, n, bool(real))
    R.check_probe_output(emu_probes(P, x, n, grid, real), checked(P, bool(real)), checked(x, bool(real)), n, grid, bool(real), ("lz_probe_dots",))


@pytest.mark.parametrize("m", range(1, 9))
@pytest.mark.parametrize("n,grid", MUT_SHAPES[:2])
def test_probes_refuse_mistakes(m, n, grid):
    rng = np.random.default_rng([27, m, n, grid])
    for real in (False, True):
        P, x = np.array([vec(rng, n, real) for _ in range(m)]), vec(rng, n, real)
        args = (checked(P, real), checked(x, real), n, grid, real)
        R.check_probe_output(emu_probes(P, x, n, grid, real), *args, ("lz_probe_dots",))
        refuses(R.check_probe_output, emu_probes(P, x, n, grid, real, "slot"), *args, ("probe M - 1 in slot M",))
        if m > 1:
            refuses(R.check_probe_output, emu_probes(P, x, n, grid, real, "swap"), *args, ("probes 0 and 1 exchanged",))
        refuses(R.check_probe_output, emu_probes(P, x, n - 1, grid, real), *args, ("last element lost",))
        if real:
            refuses(R.check_probe_output, emu_probes(P, x, n, grid, real, "real_im"), *args, ("REAL: an imaginary slot not zero",))
        else:
            refuses(R.check_probe_output, emu_probes(P, x, n, grid, real, "conj"), *args, ("Im <x|p> instead of Im <p|x>",))
            refuses(R.check_probe_output, emu_probes(P, x, n, grid, True), *args, ("complex run through the REAL instance",))
        gap = np.concatenate([x, np.full(8, complex(NAN, NAN))])
        Pg = np.concatenate([P, np.ones((m, 8))], axis=1)
        refuses(R.check_probe_output, emu_probes(Pg, gap, n + 8, grid, real), *args, ("the gap read as data",))


# ---- lz_scale, lz_axpy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grid", SHAPES)
def test_scale_and_axpy(n, grid):
    rng = np.random.default_rng([29, n, grid])
    w, y = vec(rng, n), vec(rng, n)
    s, c = 3.7320508075688772, -0.4142135623730951
    r = 1.0 / s
    R.check_scale(w.real * r + 1j * (w.imag * r), w, s, ("lz_scale",))
    R.check_axpy((y.real + c * w.real) + 1j * (y.imag + c * w.imag), y, c, w, ("lz_axpy",))
    R.check_axpy(R.fma64(c, w.real, y.real) + 1j * R.fma64(c, w.imag, y.imag), y, c, w, ("lz_axpy, contracted",))
    if n:
        good = w.real * r + 1j * (w.imag * r)
        stale = good.copy()
        stale[n - 1] = w[n - 1]
        refuses(R.check_scale, stale, w, s, ("last element not scaled",))
        refuses(R.check_scale, w * s, w, s, ("multiplied by s",))
        off = good.copy()
        off[0] = off[0].real * (1 + 2.0 ** -50) + 1j * off[0].imag
        refuses(R.check_scale, off, w, s, ("four ulps off",))
        refuses(R.check_axpy, y - c * w, y, c, w, ("y - c q",))
        refuses(R.check_axpy, y + c * np.conj(w), y, c, w, ("imaginary part with the wrong sign",))
        good = y + c * w
        good[n - 1] = y[n - 1]
        refuses(R.check_axpy, good, y, c, w, ("last element not written",))


# ---- lz_init, lz_init_real --------------------------------------------------------------------------------------------------------------------
MASK = (1 << 64) - 1


def py_uniform(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return float(x >> 11) * (1.0 / 9007199254740992.0) - 0.5


def py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, mutant=None):
    """the kernel's loop over i, in Python integers"""
    out = np.full(qdw * pitch, NAN if real else complex(NAN, NAN))
    if mutant == "iperm_as_perm" and iperm is not None:
        iperm = np.argsort(iperm)
    for i in range(qdw * pitch):
        lcol, row = divmod(i, pitch)
        col = lcol + (0 if mutant == "no_col0" else col0)
        if row >= dimup:
            if mutant != "pad":
                out[i] = 0.0
            continue
        rrow = int(iperm[row]) if iperm is not None else row
        neg = sign is not None and sign[row] and mutant != "no_sign"
        z = (((col * dimup + rrow) & MASK) * 2 + seed) & MASK
        re, im = py_uniform(z), py_uniform(z if mutant == "same_hash" else (z + 1) & MASK)
        if real:
            out[i] = -re if neg else re
        else:
            sg = -1.0 if neg else 1.0
            out[i] = complex(sg * re, sg * im)
    return out.reshape(qdw, pitch)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 12345])
@pytest.mark.parametrize("order", ["identity", "permuted"])
@pytest.mark.parametrize("col0", [0, 5])
@pytest.mark.parametrize("qdw", [0, 1, 3])
@pytest.mark.parametrize("dimup", [1, 7, 8, 9, 70])
def test_init(dimup, qdw, col0, order, seed):
    rng = np.random.default_rng([31, dimup, qdw, col0])
    iperm = sign = None
    if order == "permuted":
        iperm, sign = rng.permutation(dimup).astype(np.int32), rng.integers(0, 2, dimup).astype(np.uint8)
        if dimup > 1:
            sign[:2] = [1, 0]
    for real, pitch, ref in ((0, (dimup + 7) // 8 * 8, R.init), (1, (dimup + 15) // 16 * 16, R.init_real)):
        expect = ref(seed, dimup, pitch, qdw, col0, iperm, sign)
        R.check_bits(py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign), expect, ("lz_init", real))
        if qdw == 0:
            continue
        if pitch > dimup:
            refuses(R.check_bits, py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, "pad"), expect, ("a pad row not zeroed",))
        if col0:
            refuses(R.check_bits, py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, "no_col0"), expect, ("col0 ignored",))
        if order == "permuted" and dimup > 1:
            refuses(R.check_bits, py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, "no_sign"), expect, ("sign ignored",))
        if order == "permuted" and dimup > 2 and not np.array_equal(np.argsort(iperm), iperm):
            refuses(R.check_bits, py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, "iperm_as_perm"), expect, ("iperm applied as perm",))
        if not real:
            refuses(R.check_bits, py_init(real, seed, dimup, pitch, qdw, col0, iperm, sign, "same_hash"), expect, ("re and im from the same hash",))
            refuses(R.check_bits, py_init(real, seed ^ 1, dimup, pitch, qdw, col0, iperm, sign), expect, ("another seed",))
    zc = R.init(seed, dimup, (dimup + 7) // 8 * 8, qdw, col0, iperm, sign)
    zr = R.init_real(seed, dimup, (dimup + 15) // 16 * 16, qdw, col0, iperm, sign)
    assert R.same_bits(zr[:, :dimup], np.ascontiguousarray(zc[:, :dimup].real))


def test_init_slabs_concatenate():
    rng = np.random.default_rng(32)
    iperm, sign = rng.permutation(70).astype(np.int32), rng.integers(0, 2, 70).astype(np.uint8)
    whole = R.init(7, 70, 72, 6, 0, iperm, sign)
    parts = [R.init(7, 70, 72, q, c0, iperm, sign) for c0, q in ((0, 2), (2, 3), (5, 1))]
    assert R.same_bits(np.concatenate(parts, axis=0), whole)


# ---- lz_to_real, lz_to_complex ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdw", [0, 1, 3])
@pytest.mark.parametrize("dimup", [1, 7, 8, 9, 70])
def test_to_real_and_back(dimup, qdw):
    rng = np.random.default_rng([33, dimup, qdw])
    pc, pr, grid = (dimup + 7) // 8 * 8, (dimup + 15) // 16 * 16, 2
    src = np.full((qdw, pc), complex(NAN, NAN))
    src[:, :dimup] = R.random_complex(rng, (qdw, dimup))

    flat = np.concatenate([src.ravel(), np.full(qdw * pr, complex(NAN, NAN))])     # (what a wrong pitch reads behind the source: NaN)

    def kernel(mutant=None):
        dst, t = np.full(qdw * pr, NAN), np.zeros(qdw * pr)
        for i in range(qdw * pr):
            col, row = divmod(i, pr)
            x = 0.0
            if row < (pc if mutant == "pad" else dimup):
                z = flat[col * (pr if mutant == "pitch" else pc) + row] if row < pc else complex(NAN, NAN)
                x, t[i] = z.real, z.imag * z.imag
            dst[i] = x
        return dst.reshape(qdw, pr), t

    expect, (ref, ab) = R.to_real(src, dimup, pr)
    dst, t = kernel()
    R.check_bits(dst, expect, ("lz_to_real",))
    d = R.chain_depth(qdw * pr, grid, grid)
    R.check_scalar_sum(reduce_(t, qdw * pr, grid), ref, ab, d, ("sum Im^2",))
    back = R.to_complex(expect, dimup, pc)
    assert R.same_bits(np.ascontiguousarray(back[:, :dimup].real), np.ascontiguousarray(src[:, :dimup].real)) and not np.any(back.imag)
    if qdw:
        if pc > dimup:
            refuses(R.check_bits, kernel("pad")[0], expect, ("a pad row copied",))
        if qdw > 1 and pr != pc:
            refuses(R.check_bits, kernel("pitch")[0], expect, ("the source read with the destination's pitch",))
        refuses(R.check_scalar_sum, reduce_(t, qdw * pr, grid, 0, "drop_block"), ref, ab, d, ("a block lost",)) if qdw * pr > 256 else None
        refuses(R.check_scalar_sum, reduce_(np.abs(src[:, :dimup].imag).ravel(), qdw * dimup, grid), ref, ab, d, ("|Im| instead of Im^2",))
        wrong = back.copy()
        wrong[0, 0] = complex(back[0, 0].real, src[0, 0].imag)
        refuses(R.check_bits, wrong, R.to_complex(expect, dimup, pc), ("an imaginary part kept",))


# ---- the scalar chain -------------------------------------------------------------------------------------------------------------------------
def test_mul_and_sqrt():
    """lz_mul and lz_sqrt are compared bit for bit with IEEE double: a product formed in single precision, or through a reciprocal, a
    forgotten or doubled square root, and a neighbouring slot written are all refused"""
    rng = np.random.default_rng(34)
    a, b = (float(x) for x in R.random_reals(rng, 2))
    sc = np.full(16, SENT)
    sc[0], sc[2], sc[7] = a, b, abs(a)
    good = sc.copy()
    good[4], good[7] = a * b, math.sqrt(abs(a))
    R.check_bits(good, good.copy(), ("lz_mul, lz_sqrt",))
    for what, slot, value in (("single precision", 4, float(np.float32(a) * np.float32(b))), ("a / (1 / b)", 4, a / (1.0 / b)),
                              ("sqrt forgotten", 7, abs(a)), ("sqrt twice", 7, math.sqrt(math.sqrt(abs(a)))), ("slot 5 written", 5, a * b)):
        bad = good.copy()
        bad[slot] = value
        assert value != good[slot]
        refuses(R.check_bits, bad, good, (what,))


def test_next_chain():
    """the restatement of lz_next follows beta_{k+1} / beta_k to two roundings, and a chain with c = s_new / s_old -- the reciprocal -- or with
    the counter, the record or the limit wrong is refused bit for bit"""
    rng = np.random.default_rng(35)
    steps, nmax = 50, 40
    betas = 10.0 ** rng.uniform(-150, 150, steps + 1)
    alphas = R.random_reals(rng, steps)

    def chain(mutant=None):
        sc = np.full(16, SENT)
        sc[R.LZ_S], sc[R.LZ_C], sc[R.LZ_STEP] = 1.0 / betas[0], 0.0, 1.0
        a, b = np.full(nmax + 2, SENT), np.full(nmax + 2, SENT)
        hist = []
        for k in range(steps):
            sc[R.LZ_ALPHA], sc[R.LZ_BETA] = alphas[k], betas[k + 1]
            if mutant is None:
                R.next_step(sc, a, b, nmax)
            else:
                kk = int(sc[R.LZ_STEP])
                lim = nmax + 1 if mutant == "limit" else nmax
                if kk < lim:
                    a[kk] = sc[R.LZ_ALPHA]
                    if kk + 1 < lim or mutant == "beta_limit":
                        b[kk + (0 if mutant == "beta_slot" else 1)] = sc[R.LZ_BETA]
                s_old, s_new = sc[R.LZ_S], 1.0 / sc[R.LZ_BETA]
                sc[R.LZ_C] = s_new / s_old if mutant == "c" else (s_old / s_new if mutant == "c_div" else 1.0 / (s_new * (1.0 / s_old)))
                sc[R.LZ_S] = s_new
                sc[R.LZ_STEP] = float(kk + (0 if mutant == "step" else 1))
            hist.append(sc.copy())
        return np.array(hist), a, b

    good = chain()
    for k in range(steps):
        c, want = R.ld(good[0][k, R.LZ_C]), R.ld(betas[k + 1]) / R.ld(betas[k])
        assert abs(c - want) <= R.gamma(5) * abs(want), k        # (1 / beta_k, its reciprocal, 1 / beta_{k+1}, the product, the division)
        assert good[0][k, R.LZ_STEP] == k + 2
    assert R.same_bits(good[1][nmax:], np.full(2, SENT)) and R.same_bits(good[2][nmax:], np.full(2, SENT))
    for mutant in ("c", "c_div", "step", "limit", "beta_limit", "beta_slot"):
        bad = chain(mutant)
        assert not all(R.same_bits(x, y) for x, y in zip(good, bad)), mutant
    # LzScale by its definition: s = 1 / beta, c = beta_k / beta_{k-1}
    s, bp, c = R.scale_next(0.25, 123.0, 8.0)
    assert (s, bp, c) == (0.125, 4.0, 2.0)
