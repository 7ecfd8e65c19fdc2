"""References and forward error bounds for the streaming kernels of hxv_eigh_lowest (csrc/hxv_eigh_kernels.hpp).

Everything here is numpy in np.longdouble (x87 extended precision, 64-bit significand): a plain transcription of what each kernel is meant
to compute, and next to it the textbook forward bound (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3) for the order of
operations the kernel uses.  The bounds are functions of the INPUTS alone; nothing here has seen a kernel's output.  They hold whether or
not the compiler contracts a*b + c to an FMA (an FMA drops a rounding, it never adds one).

Notation: u = 2**-53, gamma(k) = k u / (1 - k u).  Vectors are complex arrays [slot, n]; "per component" means that the real and the
imaginary part of an output are bounded separately, each with the magnitudes of the real numbers that enter it.

The reference's own error: products of two doubles are rounded to 64 bits (2**-64 relative), sums go through numpy's pairwise summation
(about log2(n) + 16 additions deep), so a reference sum is off by less than 2**-58 sum|t_i| at the largest size used -- 2**-9 of the
smallest tolerance below (gamma(13)).  Only tr_scale_nrm's elementwise bound, u |r x|, is sharp (a correctly rounded product reaches it),
and there the reference's rounding is added to the tolerance explicitly (scale_bound)."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must be the x87 80-bit format (x86-64)"

U = LD(2.0) ** -53
U_REF = LD(2.0) ** -63     # one rounding of the reference (half an ulp of a 64-bit significand), doubled for a difference taken in it


def gamma(k):
    k = LD(k)
    return k * U / (LD(1) - k * U)


def ld(a):
    return np.asarray(a).astype(LD)


# ---- sums ---------------------------------------------------------------------------------------------------------------------------------
def chain_depth(n, grid, colsum_blocks=None):
    """D: the longest chain of floating-point additions that one term of a kernel's sum can pass through.

    In the thread: the grid-stride loop visits at most ceil(n / (256 grid)) elements, and every visit puts the running sum through two
    additions (acc += p + q: the sum of the element's two products, then the accumulation).           2 ceil(n / (256 grid))
    In the wave: wave_sum is six shuffle-and-add steps (32, 16, 8, 4, 2, 1).                                                     + 6
    In the block: the four waves' sums are added left to right.                                                                  + 3
    tr_colsum, where the sum is finished by it (colsum_blocks = its `nblocks`): a thread adds at most ceil(nblocks / 256) partial sums
    into an accumulator that starts at zero, then the block's 256 accumulators go through an eight-level tree.
                                                                                                       + ceil(nblocks / 256) + 8
    tr_colsum alone: only the last line.  The bound on a sum is then gamma(D + 2) sum|t_i|: D additions, one rounding for the product
    itself and one to spare for the order in which a compiler may associate p + q + acc."""
    d = 0
    if n is not None:
        d += 2 * math.ceil(n / (256 * grid)) + 6 + 3
    if colsum_blocks is not None:
        d += math.ceil(colsum_blocks / 256) + 8
    return d


def sum_bound(abs_sum, depth):
    return gamma(depth + 2) * abs_sum


def check_sum(got, ref, abs_sum, depth, what):
    """|got - ref| <= gamma(depth + 2) * sum|t_i| for every entry; got must be finite"""
    got, ref, abs_sum = ld(got), ld(ref), ld(abs_sum)
    assert got.shape == ref.shape == abs_sum.shape, (what, got.shape, ref.shape, abs_sum.shape)
    assert np.all(np.isfinite(got)), (what, "not finite")
    err, tol = np.abs(got - ref), sum_bound(abs_sum, depth)
    bad = np.flatnonzero(~(err <= tol).ravel())
    assert bad.size == 0, (what, f"depth {depth}", [(int(i), float(err.ravel()[i]), float(tol.ravel()[i])) for i in bad[:4]])


def check_elementwise(got, ref, bound, what):
    """per component: |Re(got - ref)| <= Re(bound), |Im(got - ref)| <= Im(bound); bound carries the two real bounds as (re, im)"""
    gr, gi = split(got)
    (rr, ri), (br, bi) = ref, bound
    assert gr.shape == rr.shape == br.shape, (what, gr.shape, rr.shape, br.shape)
    assert np.all(np.isfinite(gr)) and np.all(np.isfinite(gi)), (what, "not finite")
    for name, g, r, b in (("re", gr, rr, br), ("im", gi, ri, bi)):
        err = np.abs(g - r)
        bad = np.flatnonzero(~(err <= b).ravel())
        assert bad.size == 0, (what, name, [(int(i), float(err.ravel()[i]), float(b.ravel()[i])) for i in bad[:4]])


def split(z):
    """complex128 array -> (real, imag) in long double"""
    z = np.asarray(z)
    return z.real.astype(LD), z.imag.astype(LD)


def dots(V, w):
    """sum_i conj(V_j[i]) w[i] for every row j of V: -> (ref[j, 2], abs_sum[j, 2]), [:, 0] the real part, [:, 1] the imaginary part;
    abs_sum = the sum of the magnitudes of the real products that make up each"""
    V = np.atleast_2d(np.asarray(V))
    vr, vi = split(V)
    xr, xi = split(w)
    ref = np.zeros((V.shape[0], 2), dtype=LD)
    ab = np.zeros((V.shape[0], 2), dtype=LD)
    for j in range(V.shape[0]):
        a, b, c, d = vr[j] * xr, vi[j] * xi, vr[j] * xi, vi[j] * xr
        ref[j, 0], ref[j, 1] = np.sum(a + b), np.sum(c - d)
        ab[j, 0], ab[j, 1] = np.sum(np.abs(a) + np.abs(b)), np.sum(np.abs(c) + np.abs(d))
    return ref, ab


def norm2(w):
    """sum |w_i|^2 -> (ref, abs_sum) (equal: every term is a square)"""
    xr, xi = split(w)
    s = np.sum(xr * xr + xi * xi)
    return s, s


def colsum(partial, nval, zero_odd):
    """tr_colsum of partial[nblocks, ld]: -> (ref[nval], abs_sum[nval]); with zero_odd the odd outputs are exactly 0 whatever the column holds"""
    p = ld(partial)
    ref = np.zeros(nval, dtype=LD)
    ab = np.zeros(nval, dtype=LD)
    for t in range(nval):
        if zero_odd and (t & 1):
            continue
        ref[t], ab[t] = np.sum(p[:, t]), np.sum(np.abs(p[:, t]))
    return ref, ab


# ---- elementwise outputs ------------------------------------------------------------------------------------------------------------------
def maxpy(V, idx, coef, w):
    """w - sum_j c_j V_idx[j], c_j = coef[2j] + i coef[2j+1] -> ((re, im), (bound_re, bound_im)).
    Per component gamma(2 nj + 2) (|w| + sum_j (|cr_j| + |ci_j|) (|Re V_j| + |Im V_j|)): a term passes two additions per vector (the
    difference of its two products, the update of x), one product rounding, one to spare."""
    xr, xi = split(w)
    br, bi = np.abs(xr), np.abs(xi)
    nj = len(idx)
    for j, s in enumerate(idx):
        yr, yi = split(V[s])
        cr, ci = LD(coef[2 * j]), LD(coef[2 * j + 1])
        xr = xr - (cr * yr - ci * yi)
        xi = xi - (cr * yi + ci * yr)
        t = (abs(cr) + abs(ci)) * (np.abs(yr) + np.abs(yi))
        br, bi = br + t, bi + t
    g = gamma(2 * nj + 2)
    return (xr, xi), (g * br, g * bi)


def scale(x, r):
    """r x -> ((re, im), (bound_re, bound_im)); bound u |r x| plus the reference's own rounding of the product and of the difference"""
    xr, xi = split(x)
    r = LD(r)
    pr, pi = r * xr, r * xi
    return (pr, pi), ((U + U_REF) * np.abs(pr), (U + U_REF) * np.abs(pi))


def rotate(X, S, k):
    """y_j = sum_l S[l, j] x_l for j < k (S real [m, >=k], X complex [m, n]) -> ((re, im)[k, n], (bound_re, bound_im)[k, n]).
    Per component gamma(m + 1) sum_l |S_lj| |x_l|: m additions (the accumulator starts at zero) and the product."""
    X = np.asarray(X)
    m, n = X.shape
    S = ld(S)
    xr, xi = split(X)
    ar, ai = np.abs(xr), np.abs(xi)
    yr, yi = np.zeros((k, n), dtype=LD), np.zeros((k, n), dtype=LD)
    br, bi = np.zeros((k, n), dtype=LD), np.zeros((k, n), dtype=LD)
    for j in range(k):
        for l in range(m):
            s = S[l, j]
            yr[j] += s * xr[l]
            yi[j] += s * xi[l]
            br[j] += abs(s) * ar[l]
            bi[j] += abs(s) * ai[l]
    g = gamma(m + 1)
    return (yr, yi), (g * br, g * bi)


def axpy(V, coef, a, w):
    """a w - sum_j coef[j] V_j (coef real) -> ((re, im), (bound_re, bound_im)); per component gamma(nv + 2) (|a| |w| + sum_j |c_j| |V_j|):
    nv subtractions, the scaling by a, the product."""
    xr, xi = split(w)
    a = LD(a)
    xr, xi = a * xr, a * xi
    br, bi = np.abs(xr), np.abs(xi)
    nv = len(coef)
    for j in range(nv):
        yr, yi = split(V[j])
        c = LD(coef[j])
        xr, xi = xr - c * yr, xi - c * yi
        br, bi = br + abs(c) * np.abs(yr), bi + abs(c) * np.abs(yi)
    g = gamma(nv + 2)
    return (xr, xi), (g * br, g * bi)


def to_complex(ref):
    """(re, im) in long double -> complex128, each part rounded once"""
    return ref[0].astype(np.float64) + 1j * ref[1].astype(np.float64)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def random_reals(rng, shape):
    """mixed sign, magnitude log-uniform in 1e-3 .. 1e3"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def random_complex(rng, shape):
    """independent real and imaginary parts"""
    return random_reals(rng, shape) + 1j * random_reals(rng, shape)
