"""References for the REAL-vector kernels of the Chebyshev recurrence and for hxv_vector_random (csrc/hxv_chebyshev_real_kernels.hpp): a numpy
emulation of ch_init_real / ch_step_real on the kernels' own memory layout, the exact / long-double expectations, the check that compares a
result -- the device's (tests/test_gpu_chebyshev_real_kernels.py) or the emulation's (tests/test_chebyshev_real_ref_cpu.py, which also shows
that the check refuses named mistakes) -- with them, and the restatement of the random vector's formula in numpy uint64.

MEMORY OF A CASE: that of tests/chebyshev_ref.py, whose cases, layout and helpers are reused unchanged -- one complex128 array [4 + M, stride]
with the slots HV, CUR, PREV, OUT and the M probes.  A complex128 element is the kernels' double2: TWO CONSECUTIVE REAL elements (x = .real,
y = .imag), n counts double2 elements.  NaN in the gap behind n and in every slot the kernel must not read, a sentinel behind the partials
(one row more than the grid) and the sums (one entry more than M + 2).

WHAT THE KERNELS COMPUTE (per real component; the text of ch_step_real):
    t    = fma(-cc, cur, fma(ch, hv, -prev))        prev = 0 in the FIRST form   -- the complex kernel's own order
    out  = fma(cr, t, out)                          with a running sum; step 0: fma(c0, v, +0.0)
    sums = sum_i fma(p.y, t.y, p.x*t.x) (j < M),  the same with (t, t),  the same with (t, cur);   step 0: <p_j|v>, <v|v>, 0
M + 2 sums, each the Re accumulator of the complex kernels on the same memory.

INTEGER CASES are exact by the argument of chebyshev_ref.py (the same value ranges, the same sizes): every output vector, every partial and
every sum must equal the emulation's BIT FOR BIT.

NORMAL-DEVIATE CASES, u = 2^-53, gamma_k = k u / (1 - k u):
  * t: as in chebyshev_ref.py,  |t_dev - t| <= gamma_2 (|ch hv| + |prev| + |cc cur|).
  * out: ONE fused multiply-add on the t the device wrote, one rounding of an exact value:  |out_dev - (out_old + cr t)| <= gamma_1 (|out_old| + |cr t|).
  * a sum: as in chebyshev_ref.py, the terms have the same shape fl(fl(a b) + c d) and the additions the same longest path
    D = ceil(n / (256 grid)) + ceil(grid / 256) + 16:  |sum_dev - sum| <= gamma_{D + 2} sum_i (|a_i b_i| + |c_i d_i|), the reference sum
    taken in long double over the t the device wrote."""
import numpy as np

import chebyshev_ref as C

SENT, HV, CUR, PREV, OUT, PROBE0 = C.SENT, C.HV, C.CUR, C.PREV, C.OUT, C.PROBE0
RED_BLOCKS, MAX_PROBES, GRIDS, MS = C.RED_BLOCKS, C.MAX_PROBES, C.GRIDS, C.MS
same_bits, gamma, trips, step_cases, init_cases = C.same_bits, C.gamma, C.trips, C.step_cases, C.init_cases
MISTAKES = ("one_component", "tail_dropped", "first_reads_prev", "cr_one_component", "im_term")


def nsums(m):
    return m + 2


def make_step(seed, n, g, m, with_sum, first, integer):
    """chebyshev_ref's case (same memory, same scalars); the real kernels have no ci"""
    return dict(C.make_step(seed, n, g, m, with_sum, first, integer), ci=0.0)


def make_init(seed, n, g, m, with_out, integer):
    return dict(C.make_init(seed, n, g, m, with_out, integer), ci=0.0)


def fresh_outputs(case):
    """(partial [grid + 1, m+2], sums [m+2 + 1]) as the launch finds them"""
    return np.full((case["grid"] + 1, nsums(case["m"])), SENT), np.full(nsums(case["m"]) + 1, SENT)


def _dot_terms(a, b, mistake=None):
    """per double2 element: a.x b.x + a.y b.y"""
    if mistake == "one_component":
        return a.real * b.real
    if mistake == "im_term":
        return a.real * b.imag - a.imag * b.real
    return a.real * b.real + a.imag * b.imag


def emulate(case, mistake=None):
    """-> (mem, partial, sums) after the launch, computed on the kernel's own layout.  mistake: one of MISTAKES, for the CPU test that shows
    the check to bite: a sum taken over one component only, the ragged last trip dropped, FIRST reading prev, cr applied to one component
    only, an Im-style term (a.x b.y - a.y b.x) in the probe sums."""
    assert mistake in (None,) + MISTAKES
    n, g, m = case["n"], case["grid"], case["m"]
    mem = case["mem"].copy()
    partial, sums = fresh_outputs(case)
    live = n - n % (256 * g) if mistake == "tail_dropped" and n >= 256 * g else n
    sl = slice(0, live)
    cur = mem[CUR, sl]
    probes = [mem[PROBE0 + j, sl] for j in range(m)]
    cr = np.longdouble(case["cr"])

    def axpy(o, t):  # o + cr t per component, in long double and rounded once: the kernel's one fused multiply-add
        (ox, oy), (tx, ty) = C._ld(o), C._ld(t)
        return C._cplx(ox + cr * tx + 0.0, oy + (ty if mistake == "cr_one_component" else cr * ty) + 0.0)

    T = np.zeros((live, nsums(m)))
    if case["kind"] == "init":
        t = cur
        if case["with_sum"]:
            mem[OUT, sl] = axpy(np.zeros(live, dtype=np.complex128), t)
    else:
        reads_prev = not case["first"] or mistake == "first_reads_prev"
        prev = mem[PREV, sl] if reads_prev else np.zeros(live, dtype=np.complex128)
        (hx, hy), (cx, cy), (px, py) = C._ld(mem[HV, sl]), C._ld(cur), C._ld(prev)
        ch, cc = np.longdouble(case["ch"]), np.longdouble(case["cc"])
        t = C._cplx(ch * hx - px - cc * cx + 0.0, ch * hy - py - cc * cy + 0.0)
        if case["with_sum"]:
            mem[OUT, sl] = axpy(mem[OUT, sl], t)
        mem[PREV, sl] = t
        T[:, m + 1] = _dot_terms(t, cur, "one_component" if mistake == "one_component" else None)
    for j in range(m):
        T[:, j] = _dot_terms(probes[j], t, mistake)
    T[:, m] = _dot_terms(t, t, "one_component" if mistake == "one_component" else None)
    blk = (np.arange(live) // 256) % g
    for b in range(g):
        partial[b] = T[blk == b].sum(axis=0) + 0.0
    sums[:-1] = partial[:g].sum(axis=0)
    return mem, partial, sums


def check(case, got):
    """got = (mem, partial, sums) after the launch.  -> list of complaints, empty when the result is what the kernel text promises."""
    bad = []
    n, g, m = case["n"], case["grid"], case["m"]
    mem0 = case["mem"]
    mem, partial, sums = got
    step = case["kind"] == "step"
    written = ([PREV] if step else []) + ([OUT] if case["with_sum"] else [])
    if partial.shape != (g + 1, nsums(m)) or sums.shape != (nsums(m) + 1,):
        return ["partial / sums do not have the real kernels' shape (m + 2 sums)"]
    for s in range(mem.shape[0]):
        if s not in written and not same_bits(mem[s], mem0[s]):
            bad.append(f"slot {s} must not be written")
        if not same_bits(mem[s, n:], mem0[s, n:]):
            bad.append(f"slot {s}: the gap behind n changed")
    if not same_bits(partial[g:], np.full_like(partial[g:], SENT)) or not same_bits(sums[-1:], np.array([SENT])):
        bad.append("a partial row beyond the grid or the entry behind the sums was written")
    for s in written:
        if not np.all(np.isfinite(mem[s, :n].view(np.float64))):
            bad.append(f"slot {s}: not finite -- something that must not be read was read, or an element was not written")
    if not np.all(np.isfinite(partial[:g])) or not np.all(np.isfinite(sums[:-1])):
        bad.append("a sum is not finite")
    if bad:
        return bad
    if case["integer"]:
        emem, epartial, esums = emulate(case)
        for s in written:
            if not same_bits(mem[s], emem[s]):
                bad.append(f"slot {s}: not the exact result bit for bit")
        if not same_bits(partial, epartial):
            bad.append("partial: not the exact sums bit for bit")
        if not same_bits(sums, esums):
            bad.append("sums: not the exact sums bit for bit")
        return bad
    cur = mem0[CUR, :n]
    cr = np.longdouble(case["cr"])
    if step:
        hx, hy = C._ld(mem0[HV, :n])
        cx, cy = C._ld(cur)
        px, py = C._ld(np.zeros(n, dtype=np.complex128) if case["first"] else mem0[PREV, :n])
        ch, cc = np.longdouble(case["ch"]), np.longdouble(case["cc"])
        t_dev = mem[PREV, :n]
        for name, dv, h, c_, p in (("x", t_dev.real, hx, cx, px), ("y", t_dev.imag, hy, cy, py)):
            ref = ch * h - p - cc * c_
            bound = gamma(2) * (np.abs(ch * h) + np.abs(p) + np.abs(cc * c_))
            if np.any(np.abs(dv - ref) > bound):
                bad.append(f"t_next.{name}: beyond gamma_2 of the magnitudes (max excess {float(np.max(np.abs(dv - ref) - bound)):.3e})")
    else:
        t_dev = cur
    tx, ty = C._ld(t_dev)
    if case["with_sum"]:
        ox, oy = C._ld(mem0[OUT, :n]) if step else C._ld(np.zeros(n, dtype=np.complex128))
        o_dev = mem[OUT, :n]
        for name, dv, o, t in (("x", o_dev.real, ox, tx), ("y", o_dev.imag, oy, ty)):
            if np.any(np.abs(dv - (o + cr * t)) > gamma(1) * (np.abs(o) + np.abs(cr * t))):
                bad.append(f"out.{name}: beyond gamma_1 of the magnitudes")
    D = trips(n, g) + -(-g // 256) + 16
    refs, mags = [], []
    for j in range(m):
        qx, qy = C._ld(mem0[PROBE0 + j, :n])
        refs.append(np.sum(qx * tx + qy * ty))
        mags.append(np.sum(np.abs(qx * tx) + np.abs(qy * ty)))
    refs.append(np.sum(tx * tx + ty * ty))
    mags.append(refs[-1])
    if step:
        cx, cy = C._ld(cur)
        refs.append(np.sum(tx * cx + ty * cy))
        mags.append(np.sum(np.abs(tx * cx) + np.abs(ty * cy)))
    else:
        refs.append(np.longdouble(0))
        mags.append(np.longdouble(0))
    for k, (r, mg) in enumerate(zip(refs, mags)):
        if abs(np.longdouble(sums[k]) - r) > gamma(D + 2) * mg:
            bad.append(f"sum {k}: {sums[k]!r} against {float(r)!r}, bound {float(gamma(D + 2) * mg):.3e}")
    tot = partial[:g].astype(np.longdouble).sum(axis=0)
    if np.any(np.abs(sums[:-1] - tot) > gamma(-(-g // 256) + 8) * np.abs(partial[:g]).astype(np.longdouble).sum(axis=0)):
        bad.append("sums are not the block partials added up")
    return bad


def re_accumulators(m, step=True):
    """indices, among the complex kernels' 2m + 3 sums, of the m + 2 the real kernels produce: Re<p_j|t>, <t|t>, Re<t|cur>"""
    return [2 * j for j in range(m)] + [2 * m, 2 * m + 1]


# ---- hxv_vector_random (include/hxv.h) restated in numpy uint64 ------------------------------------------------------------------------
_GOLD, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(x):
    """the splitmix64 finaliser on a uint64 array (wrap-around arithmetic)"""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64)).copy()
    x += _GOLD
    x = (x ^ (x >> np.uint64(30))) * _M1
    x = (x ^ (x >> np.uint64(27))) * _M2
    return x ^ (x >> np.uint64(31))


def uniform(seed, index, c):
    """u(I, c) = (double)(mix(mix(seed) ^ (2 I + c)) >> 11) * 2^-53 - 0.5"""
    key = mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))[0]
    z = mix(key ^ (np.asarray(index, dtype=np.uint64) * np.uint64(2) + np.uint64(c)))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def random_vector(seed, dim, complex_valued=False, first=0):
    """elements first .. first + dim - 1 of the vector of `seed` in the reference's layout (I = col * DimUp + row), complex128"""
    idx = np.arange(first, first + dim, dtype=np.uint64)
    v = np.zeros(dim, dtype=np.complex128)
    v.real = uniform(seed, idx, 0)
    if complex_valued:
        v.imag = uniform(seed, idx, 1)
    return v


def lanczos_start_real(seed, dim):
    """the real part of the engine's Lanczos start vector (lz_init: the hash of 2 I + seed, no key): what hxv_vector_random must NOT be"""
    z = mix(np.arange(dim, dtype=np.uint64) * np.uint64(2) + np.uint64(seed))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def overlap(a, b):
    return float(abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b)))
