"""References, forward error bounds and exact restatements for the kernels of the Lanczos recurrence (csrc/hxv_lanczos_kernels.hpp) and for
LzScale (csrc/hxv_lanczos_host.hpp).  CPU only.

Everything is numpy in np.longdouble; gamma, ld, check_sum and check_elementwise are those of tests/eigh_kernels_ref.py (u = 2**-53,
gamma(k) = k u / (1 - k u), U_REF = 2**-63 for the reference's own rounding).  The bounds are functions of the INPUTS alone, derived from
the order of operations the kernel text shows; the derivation stands next to each.  Nothing here has seen a kernel's output.

Sums (chain_depth): a term passes at most D additions, and the tolerance is gamma(D + 2) sum|t_i| (one more rounding for the product inside
the term, one to spare).  Elementwise outputs: see sub_fma, sub_mul, scale_div, axpy.  Exact restatements, compared bit for bit: the start
vectors (uniform, init, init_real: integer hashing in uint64 with wrap-around, then floating-point operations that are all exact), the
layout conversions (copies), and the scalar chain (IEEE double division, product and square root, correctly rounded on both sides).

The second half (emu_*) restates the kernels in double precision IN THE KERNEL'S ORDER, with named mistakes that can be switched on:
tests/test_lanczos_kernels_ref_cpu.py feeds both to the check_* functions below, the same ones tests/test_gpu_lanczos_kernels.py feeds
the device's output to, and requires that the right one passes and every wrong one is refused."""
import math

import numpy as np

from eigh_kernels_ref import LD, U, U_REF, check_elementwise, check_sum, dots, gamma, ld, random_complex, random_reals, split  # noqa: F401

RED_BLOCKS = 1024        # (test_constants of the GPU file pins the header's values to these)
MAX_PROBES = 8
LZ_ALPHA, LZ_BETA, LZ_S, LZ_C, LZ_STEP = 0, 1, 2, 3, 6
SENT = -1.2345678e300   # what the tests fill every output with that must not be written


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_bits(got, expect, what):
    got, expect = np.ascontiguousarray(got), np.ascontiguousarray(expect)
    assert got.shape == expect.shape and got.dtype == expect.dtype, (what, got.shape, expect.shape, got.dtype, expect.dtype)
    if got.tobytes() != expect.tobytes():
        g, e = got.reshape(-1), expect.reshape(-1)
        bad = np.flatnonzero(np.any(g.view(np.uint8).reshape(g.size, -1) != e.view(np.uint8).reshape(e.size, -1), axis=1))
        raise AssertionError((what, "bits differ", [(int(i), g[i], e[i]) for i in bad[:4]]))


# ---- sums ---------------------------------------------------------------------------------------------------------------------------------
def chain_depth(n, grid, final_np=None):
    """D: the longest chain of floating-point additions one term of a sum can pass through.

    In the thread: the grid-stride loop visits at most ceil(n / (256 grid)) elements; every visit is one accumulation and one rounding
    inside the term (the sum or the fused multiply-add of the element's two products).                          2 ceil(n / (256 grid))
    In the block: block_sum is a tree of eight LDS levels (128, 64, ..., 1); these kernels have no wave shuffle.              + 8
    lz_final / lz_probe_final, where the sum is finished by one (final_np = its np): a thread adds at most ceil(np / 256) partial sums
    into an accumulator that starts at zero, then the same eight-level tree.                               + ceil(np / 256) + 8
    n = None: the finishing kernel alone."""
    d = 0
    if n is not None:
        d += 2 * math.ceil(n / (256 * grid)) + 8
    if final_np is not None:
        d += math.ceil(final_np / 256) + 8
    return d


def sumsq(x):
    """sum of re^2 + im^2 (complex x) or of x^2 (real x) -> (ref, abs_sum), equal: every term is a square"""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        xr, xi = split(x)
        s = np.sum(xr * xr + xi * xi)
    else:
        s = np.sum(ld(x) ** 2)
    return LD(s), LD(s)


def redot(q, w):
    """Re <q|w> = sum q.re w.re + q.im w.im -> (ref, abs_sum)"""
    qr, qi = split(q)
    wr, wi = split(w)
    a, b = qr * wr, qi * wi
    return LD(np.sum(a + b)), LD(np.sum(np.abs(a) + np.abs(b)))


def check_scalar_sum(got, ref, ab, depth, what):
    check_sum(np.array([got]), np.array([ref], dtype=LD), np.array([ab], dtype=LD), depth, what)


def check_sqrt_sum(got, ref, ab, depth, what):
    """got = sqrt(s') where s' is the device's sum of NON-NEGATIVE terms (ab == ref = s).  With g = gamma(depth + 2), |s' - s| <= g s, so
    |sqrt(s') - sqrt(s)| = |s' - s| / (sqrt(s') + sqrt(s)) <= g sqrt(s) / (1 + sqrt(1 - g)); the square root itself is correctly rounded:
    + u sqrt(s') <= u (1 + g) sqrt(s); + U_REF sqrt(s) for the reference's own square root."""
    assert ab == ref, (what, "check_sqrt_sum is for sums of squares")
    assert np.isfinite(got), (what, "not finite")
    g, r = gamma(depth + 2), np.sqrt(LD(ref))
    tol = g * r / (LD(1) + np.sqrt(LD(1) - g)) + (U * (LD(1) + g) + U_REF) * r
    err = abs(LD(got) - r)
    assert err <= tol, (what, f"depth {depth}", float(err), float(tol))


def check_norm(got, x, n, grid, op, what):
    """lz_nrm (or the norm half of lz_sub_nrm / lz_pack_pair) on `grid` blocks, finished by lz_final(np = grid, op)"""
    ref, ab = sumsq(x)
    d = chain_depth(n, grid, grid)
    (check_sqrt_sum if op else check_scalar_sum)(got, ref, ab, d, what)


def check_redot(got, q, w, n, grid, what):
    ref, ab = redot(q, w)
    check_scalar_sum(got, ref, ab, chain_depth(n, grid, grid), what)


def check_final(got, partial, op, what):
    """lz_final alone over partial[0..np)"""
    p = ld(partial)
    ref, ab = LD(np.sum(p)), LD(np.sum(np.abs(p)))
    d = chain_depth(None, 1, len(p))
    (check_sqrt_sum if op else check_scalar_sum)(got, ref, ab, d, what)


def check_probe_final(got, partial, what):
    """lz_probe_final alone: got[c] = sum over the rows of partial[np, nc]"""
    p = ld(partial)
    check_sum(got, np.sum(p, axis=0), np.sum(np.abs(p), axis=0), chain_depth(None, 1, p.shape[0]), what)


def check_probes(got, P, x, n, grid, real, what):
    """got[2m] = (Re, Im) <p_j|x>, j < m, from lz_probe_dots<m, real> on `grid` blocks and lz_probe_final.  Re and Im each have their own
    bound (the magnitudes of the two real products that enter each).  real: x and the probes are real arrays viewed as double2, Re is their
    dot product, and every Im slot is +0.0 exactly (the kernel writes the constant)."""
    P = np.atleast_2d(P)
    m = P.shape[0]
    got = np.asarray(got).reshape(m, 2)
    ref, ab = dots(P, x)
    d = chain_depth(n, grid, grid)
    if real:
        check_sum(got[:, 0], ref[:, 0], ab[:, 0], d, what + ("re",))
        check_bits(got[:, 1], np.zeros(m), what + ("imaginary slots of a real run",))
    else:
        check_sum(got, ref, ab, d, what)


def check_probe_output(out, P, x, n, grid, real, what):
    """out[2 M + 2] as lz_probe_final leaves it in a sentinel-filled array: the 2 M overlaps (check_probes), the sentinel behind them"""
    m = np.atleast_2d(P).shape[0]
    out = np.asarray(out)
    assert out.shape == (2 * m + 2,), (what, out.shape)
    assert same_bits(out[2 * m:], np.full(2, SENT)), (what, "lz_probe_final wrote beyond 2 M", out[2 * m:])
    check_probes(out[:2 * m], P, x, n, grid, real, what)


# ---- elementwise outputs ------------------------------------------------------------------------------------------------------------------
def sub_fma(x, a, y, b=None):
    """fma(-a, y, x) per component (a for the real parts, b -- default a -- for the imaginary parts) -> ((re, im), (bound_re, bound_im)).
    One rounding of the exact x - a y: u |x - a y|, sharp.  The reference rounds the product and the difference to 64 bits, each within
    2**-64 of its magnitude: U_REF (|x| + |a y|) covers both, cancellation included."""
    xr, xi = split(x)
    yr, yi = split(y)
    a = LD(a)
    b = a if b is None else LD(b)
    pr, pi = a * yr, b * yi
    rr, ri = xr - pr, xi - pi
    return (rr, ri), (U * np.abs(rr) + U_REF * (np.abs(xr) + np.abs(pr)), U * np.abs(ri) + U_REF * (np.abs(xi) + np.abs(pi)))


def sub_mul(x, b, p):
    """x - b p per component, product and difference each rounded (or contracted to one rounding): gamma(2) (|x| + |b p|)"""
    xr, xi = split(x)
    pr, pi = split(p)
    b = LD(b)
    tr, ti = b * pr, b * pi
    g = gamma(2)
    return (xr - tr, xi - ti), (g * (np.abs(xr) + np.abs(tr)), g * (np.abs(xi) + np.abs(ti)))


def scale_div(x, s):
    """lz_scale: r = 1 / s rounded, then x r rounded: gamma(2) |x / s|, plus U_REF |x / s| for the reference's division"""
    xr, xi = split(x)
    s = LD(s)
    rr, ri = xr / s, xi / s
    g = gamma(2) + U_REF
    return (rr, ri), (g * np.abs(rr), g * np.abs(ri))


def axpy(z, c, x):
    """lz_axpy: z + c x per component: gamma(2) (|z| + |c x|)"""
    zr, zi = split(z)
    xr, xi = split(x)
    c = LD(c)
    tr, ti = c * xr, c * xi
    g = gamma(2)
    return (zr + tr, zi + ti), (g * (np.abs(zr) + np.abs(tr)), g * (np.abs(zi) + np.abs(ti)))


# ---- exact restatements -------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def uniform(z):
    """lz_uniform: splitmix64 of z (uint64, wrap-around) -> (-0.5, 0.5).  The top 53 bits convert to double exactly, the scaling by 2**-53
    is exact, and so is the subtraction of 0.5 (both operands are multiples of 2**-53 below 1)."""
    x = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5


def _init_keys(seed, dimup, pitch, qdw, col0, iperm):
    """-> (z [qdw, dimup] uint64: the hash argument of the real part of every data row)"""
    rrow = np.arange(dimup, dtype=np.int64) if iperm is None else np.asarray(iperm, dtype=np.int64)
    col = np.arange(qdw, dtype=np.int64)[:, None] + col0
    idx = (col * dimup + rrow[None, :]).astype(np.uint64)
    with np.errstate(over="ignore"):
        return idx * np.uint64(2) + np.uint64(seed & M64)


def init(seed, dimup, pitch, qdw, col0=0, iperm=None, sign=None):
    """lz_init: complex [qdw, pitch]; device row `row` of global column col0 + c holds sgn(row) (uniform(z), uniform(z + 1)) with
    z = 2 (col dimup + iperm[row]) + seed; rows dimup..pitch are zero.  Multiplying by +-1 is exact."""
    out = np.zeros((qdw, pitch), dtype=np.complex128)
    if dimup == 0 or qdw == 0:
        return out
    z = _init_keys(seed, dimup, pitch, qdw, col0, iperm)
    sgn = np.where(np.asarray(sign[:dimup]) != 0, -1.0, 1.0)[None, :] if sign is not None else 1.0
    with np.errstate(over="ignore"):
        re, im = uniform(z.ravel()).reshape(z.shape), uniform((z + np.uint64(1)).ravel()).reshape(z.shape)
    out[:, :dimup] = sgn * re + 1j * (sgn * im)
    return out


def init_real(seed, dimup, pitch, qdw, col0=0, iperm=None, sign=None):
    """lz_init_real: real [qdw, pitch], the real part of init's vector"""
    out = np.zeros((qdw, pitch))
    if dimup == 0 or qdw == 0:
        return out
    z = _init_keys(seed, dimup, pitch, qdw, col0, iperm)
    r = uniform(z.ravel()).reshape(z.shape)
    out[:, :dimup] = np.where(np.asarray(sign[:dimup]) != 0, -r, r) if sign is not None else r
    return out


def to_real(src, dimup, pr):
    """lz_to_real of complex src [qdw, pc] -> (real [qdw, pr] with zero pads, (sum Im^2, abs_sum) over the data rows)"""
    src = np.asarray(src)
    out = np.zeros((src.shape[0], pr))
    out[:, :dimup] = src[:, :dimup].real
    im = ld(src[:, :dimup].imag)
    s = LD(np.sum(im * im))
    return out, (s, s)


def to_complex(src, dimup, pc):
    """lz_to_complex of real src [qdw, pr] -> complex [qdw, pc], zero pads, zero imaginary parts"""
    src = np.asarray(src)
    out = np.zeros((src.shape[0], pc), dtype=np.complex128)
    out[:, :dimup] = src[:, :dimup]
    return out


def scale_next(s_cur, beta_prev, beta):
    """LzScale::next(beta) then c() in IEEE double (Python floats): -> (s_cur, beta_prev, c)"""
    s_cur, beta = float(s_cur), float(beta)
    beta_prev = 1.0 / s_cur
    s_cur = 1.0 / beta
    return s_cur, beta_prev, 1.0 / (s_cur * beta_prev)


def next_step(scal, alpha_out, beta_out, nmax):
    """lz_next on host copies (in place), through scale_next: the device must give these bits"""
    k = int(scal[LZ_STEP])
    if k < nmax:
        alpha_out[k] = scal[LZ_ALPHA]
        if k + 1 < nmax:
            beta_out[k + 1] = scal[LZ_BETA]
    s, _, c = scale_next(scal[LZ_S], 0.0, scal[LZ_BETA])
    scal[LZ_S], scal[LZ_C], scal[LZ_STEP] = s, c, float(k + 1)


# ---- composite checks of the updating kernels -----------------------------------------------------------------------------------------------
def check_sub_dot(w_after, out, w, qm, q, b, n, grid, what):
    """lz_sub_dot + lz_final(op 0).  b = None: ib = -1, w must be untouched.  The dot is referenced with the w the device wrote."""
    if b is None:
        check_bits(w_after, w, what + ("w must not change with ib = -1",))
    else:
        ref, bound = sub_mul(w, b, qm)
        check_elementwise(w_after, ref, bound, what + ("w",))
    check_redot(out, q, w_after, n, grid, what + ("dot",))


def check_sub_nrm(w_after, out, w, q, a, n, grid, op, what, b=None):
    """lz_sub_nrm + lz_final(op); b: the paired kernel's second coefficient (the two norms are checked by the caller per component)"""
    ref, bound = sub_fma(w, a, q, b)
    check_elementwise(w_after, ref, bound, what + ("w",))
    if out is not None:
        check_norm(out, w_after, n, grid, op, what + ("norm",))


def check_scale(q_after, w, s, what):
    ref, bound = scale_div(w, s)
    check_elementwise(q_after, ref, bound, what)


def check_axpy(y_after, y, c, q, what):
    ref, bound = axpy(y, c, q)
    check_elementwise(y_after, ref, bound, what)


# ---- the kernels restated in double, in their own order, with switchable mistakes ------------------------------------------------------------
def _two_prod(a, b):
    """a b = p + e exactly (Veltkamp / Dekker), for magnitudes far from over- and underflow"""
    p = a * b
    c = 134217729.0
    ah = a * c - (a * c - a)
    bh = b * c - (b * c - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """round(a b + c) with one rounding, from error-free transformations: a b = p + e, c + p = s + t exactly, then s + (t + e).  The inner
    sum is rounded, so the result can miss the correctly rounded one only when the exact value lies within u**2 |s| of a rounding
    boundary (about 2**-52 per element); the seeds of the CPU test are fixed."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p, e = _two_prod(a, b)
    s = c + p
    bb = s - c
    t = (c - (s - bb)) + (p - bb)
    return s + (t + e)


def emu_partials(term, n, grid, mutant=None):
    """partial[grid] of a streaming reduction whose thread adds term[i] (already rounded as the kernel rounds it) for
    i = block 256 + t, + 256 grid, ...; then block_sum's tree.
    mutants: "drop_last" (the loop stops at n - 1), "drop_block" (the last block's partial is zero)."""
    term = np.asarray(term, dtype=np.float64)[:n]
    if mutant == "drop_last" and n > 0:
        term = term[:n - 1]
    rounds = max(1, math.ceil(len(term) / (256 * grid)))
    padded = np.zeros(rounds * grid * 256)
    padded[:len(term)] = term
    padded = padded.reshape(rounds, grid, 256)
    acc = np.zeros((grid, 256))
    for k in range(rounds):
        acc = acc + padded[k]
    part = _tree(acc)
    if mutant == "drop_block":
        part[grid - 1] = 0.0
    return part


def _tree(acc):
    red = np.array(acc, dtype=np.float64)
    s = 128
    while s > 0:
        red[..., :s] = red[..., :s] + red[..., s:2 * s]
        s >>= 1
    return red[..., 0].copy()


def emu_final(partial, op=0, mutant=None):
    """lz_final over partial[0..np): thread t adds partial[t], partial[t + 256], ...; tree; op 1: sqrt.
    mutants: "twice" (the last partial is added again), "drop_last", "no_sqrt", "sqrt_twice"."""
    p = np.asarray(partial, dtype=np.float64)
    if mutant == "twice" and len(p):
        p = np.concatenate([p, p[-1:]])
    if mutant == "drop_last":
        p = p[:-1]
    rounds = max(1, math.ceil(len(p) / 256))
    padded = np.zeros(rounds * 256)
    padded[:len(p)] = p
    acc = np.zeros(256)
    for k in range(rounds):
        acc = acc + padded[k * 256:(k + 1) * 256]
    s = float(_tree(acc))
    if mutant == "no_sqrt":
        return s
    if op:
        s = math.sqrt(s)
        if mutant == "sqrt_twice":
            s = math.sqrt(s)
    return s


def _parts(z):
    z = np.asarray(z)
    return (z.real.astype(np.float64), z.imag.astype(np.float64)) if np.iscomplexobj(z) else (z.astype(np.float64), np.zeros(z.shape))


def emu_nrm_terms(x):
    """lz_nrm's term: t = re re rounded, then fma(im, im, t)"""
    xr, xi = _parts(x)
    return fma64(xi, xi, xr * xr)


def emu_sub_nrm(w, a, q, b=None):
    """lz_sub_nrm / lz_sub_nrm_pair's update -> w after"""
    wr, wi = _parts(w)
    qr, qi = _parts(q)
    return fma64(-a, qr, wr) + 1j * fma64(-(a if b is None else b), qi, wi)


def emu_sub_dot(w, b, qm, q):
    """lz_sub_dot -> (w after, terms); b = None: ib = -1"""
    wr, wi = _parts(w)
    if b is not None:
        pr, pi = _parts(qm)
        wr, wi = wr - b * pr, wi - b * pi
    qr, qi = _parts(q)
    return wr + 1j * wi, qr * wr + qi * wi


def emu_probe_terms(p, x, mutant=None):
    """lz_probe_dots' terms of one probe -> (re terms, im terms).  mutant "conj": the imaginary part of <x|p> instead of <p|x>."""
    pr, pi = _parts(p)
    xr, xi = _parts(x)
    re = fma64(pi, xi, pr * xr)
    im = fma64(-pi, xr, pr * xi)
    return re, (-im if mutant == "conj" else im)
