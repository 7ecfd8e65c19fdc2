"""References for the two kernels of the Chebyshev recurrence (csrc/hxv_chebyshev_kernels.hpp): the cases, a numpy emulation of each kernel
on the kernel's own memory layout, the exact / long-double expectations and the check that compares a result -- the device's
(tests/test_gpu_chebyshev_kernels.py) or the emulation's (tests/test_chebyshev_ref_cpu.py, which also shows that the check refuses named
mistakes) -- with them.

MEMORY OF A CASE.  One complex array [4 + M, stride], stride = n rounded up to 8, plus 8: slots HV, CUR, PREV (read and overwritten with
t_next; the FIRST form only writes it), OUT (the running sum; step 0 only writes it), then the M probes.  The gap [n, stride) of every slot
holds NaN and must be bitwise unchanged afterwards; a slot the kernel must not read holds NaN in [0, n) as well, so a read shows in the
output; a slot the kernel must not write must be bitwise unchanged.  `partial` has one row more than the grid and `sums` one entry more than
2M + 3, both prefilled with SENT: the extra row and entry must keep it.

WHAT THE KERNEL COMPUTES (per element i < n; the text of ch_step):
    t    = fma(-cc, cur, fma(ch, hv, -prev))        per component; prev = 0 in the FIRST form
    out  = (fma(cr, t.x, fma(-ci, t.y, out.x)), fma(cr, t.y, fma(ci, t.x, out.y)))        with a running sum
    sums = sum conj(p_j) t (re, im; j < M),  sum |t|^2,  sum conj(t) cur (re, im)
and step 0 (ch_init): out = (c0r + i c0i) v in the same two-fma form from +0.0, sums = <p_j|v>, <v|v>, 0, 0.

INTEGER CASES.  hv, cur, prev, out and the probes are integers in [-4, 4] and ch, cc, cr, ci are +-2^k with |k| <= 2 (ch > 0), so |t| <= 36
in multiples of 1/4, every term of a sum is a multiple of 1/16 below 2^12 and a sum over the at most 2309 elements of a case stays below
2^24: every product, every sum and every partial sum is exactly representable, whatever the order, so
every output vector, every partial and every sum must equal the emulation's BIT FOR BIT (signed zeros included: the pads' +0.0 is part of
the contract, and the emulation's zeros are checked to be +0.0 where the kernel's are).

NORMAL-DEVIATE CASES: bounds, with u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1).
  * t: two fused multiply-adds, each one rounding of an exact a*b + c:  fl(fl(ch hv - prev) - cc cur).  With d = ch hv - prev,
    |fl(d) - d| <= u |d| and the second rounding adds u |fl(d) - cc cur|, so  |t_dev - t| <= gamma_2 (|ch hv| + |prev| + |cc cur|).
  * out: the same shape on the t the device wrote:  |out_dev - out| <= gamma_2 (|out_old| + |cr t.x| + |ci t.y|)  (and x <-> y).
  * a sum: every term is one rounded product fed to one fma, fl(fl(a b) + c d): relative error of the term against |a b| + |c d| at most
    gamma_2.  A thread adds its ceil(n / (256 grid)) terms in order, the LDS tree adds 8 levels, lz_probe_final adds ceil(grid / 256) block
    partials per thread and 8 levels more: D = ceil(n / (256 grid)) + ceil(grid / 256) + 16 additions on the longest path, so
        |sum_dev - sum| <= gamma_{D + 2} sum_i (|a_i b_i| + |c_i d_i|),
    the reference sum taken in long double over the t THE DEVICE WROTE (its own bound is the first item), as the Lanczos kernel references do."""
import numpy as np

RED_BLOCKS = 1024
MAX_PROBES = 8
SENT = -7.25e77
NAN = float("nan")
CNAN = complex(NAN, NAN)
U = 2.0 ** -53
HV, CUR, PREV, OUT, PROBE0 = 0, 1, 2, 3, 4
MISTAKES = ("wrong_buffer", "b_sign", "conj_side", "sum_late", "tail_dropped")


def gamma(k):
    return k * U / (1.0 - k * U)


def nsums(m):
    return 2 * m + 3


def stride_of(n):
    return (n + 7) // 8 * 8 + 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
GRIDS = (1, 2, 3)
MS = (0, 1, 3, 8)


def sizes(g):
    """around the block, then two, three and four trips of the grid-stride loop with a ragged last one"""
    return (1, 255, 256, 257, 256 * g + 5, 2 * 256 * g + 5, 3 * 256 * g + 5)


def step_cases():
    """(n, grid, m, with_sum, first): the cross of the sizes, the grids, M in MS, the running sum and the first-step form; then every other
    instantiation M = 2, 4 .. 7 once per form at a two-block ragged size"""
    out = [(n, g, m, s, f) for g in GRIDS for n in sizes(g) for m in MS for s in (False, True) for f in (False, True)]
    out += [(257, 2, m, s, f) for m in (2, 4, 5, 6, 7) for s in (False, True) for f in (False, True)]
    return out


def init_cases():
    """(n, grid, m, with_out)"""
    out = [(n, g, m, o) for g in GRIDS for n in sizes(g) for m in MS for o in (False, True)]
    out += [(257, 2, m, o) for m in (2, 4, 5, 6, 7) for o in (False, True)]
    return out


def trips(n, g):
    return -(-n // (256 * g))


def _values(rng, n, integer):
    if integer:
        return (rng.integers(-4, 5, n) + 1j * rng.integers(-4, 5, n)).astype(np.complex128)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _scalar(rng, integer):
    if integer:
        return float(rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-2, 3)))
    return float(rng.standard_normal())


def make_step(seed, n, g, m, with_sum, first, integer):
    """-> case dict: mem [4 + m, stride] as the kernel finds it, the scalars, and what identifies the launch"""
    rng = np.random.default_rng(seed)
    mem = np.full((4 + m, stride_of(n)), CNAN)
    for s in [HV, CUR] + ([] if first else [PREV]) + ([OUT] if with_sum else []) + [PROBE0 + j for j in range(m)]:
        mem[s, :n] = _values(rng, n, integer)
    ch = abs(_scalar(rng, integer)) + (0.0 if integer else 0.1)
    return dict(kind="step", n=n, grid=g, m=m, with_sum=with_sum, first=first, integer=integer, mem=mem, ch=ch, cc=_scalar(rng, integer),
                cr=_scalar(rng, integer), ci=_scalar(rng, integer))


def make_init(seed, n, g, m, with_out, integer):
    """step 0: the start vector is in slot CUR; HV and PREV are not touched at all"""
    rng = np.random.default_rng(seed)
    mem = np.full((4 + m, stride_of(n)), CNAN)
    for s in [CUR] + [PROBE0 + j for j in range(m)]:
        mem[s, :n] = _values(rng, n, integer)
    return dict(kind="init", n=n, grid=g, m=m, with_sum=with_out, first=False, integer=integer, mem=mem, ch=0.0, cc=0.0,
                cr=_scalar(rng, integer), ci=_scalar(rng, integer))


def fresh_outputs(case):
    """(partial [grid + 1, 2m+3], sums [2m+3 + 1]) as the launch finds them"""
    return np.full((case["grid"] + 1, nsums(case["m"])), SENT), np.full(nsums(case["m"]) + 1, SENT)


# ---- the emulation ----------------------------------------------------------------------------------------------------------------------
def _block_of(n, g):
    return (np.arange(n) // 256) % g


def _terms(case, t, cur, probes, conj_side=False):
    """[n, 2m+3] the terms of the sums, in double like the kernel's"""
    m, n = case["m"], case["n"]
    T = np.zeros((n, nsums(m)))
    for j in range(m):
        p = probes[j]
        T[:, 2 * j] = p.real * t.real + p.imag * t.imag
        T[:, 2 * j + 1] = (p.real * t.imag - p.imag * t.real) * (-1.0 if conj_side else 1.0)
    T[:, 2 * m] = t.real * t.real + t.imag * t.imag
    if case["kind"] == "step":
        T[:, 2 * m + 1] = t.real * cur.real + t.imag * cur.imag
        T[:, 2 * m + 2] = (t.real * cur.imag - t.imag * cur.real) * (-1.0 if conj_side else 1.0)
    return T


def _cplx(x, y):
    z = np.empty(len(x), dtype=np.complex128)
    z.real, z.imag = x, y  # (rounded to double here)
    return z


def emulate(case, mistake=None):
    """-> (mem, partial, sums) after the launch, computed in double on the kernel's own layout.  mistake: one of MISTAKES, for the CPU test
    that shows the check to bite."""
    assert mistake in (None,) + MISTAKES
    n, g, m = case["n"], case["grid"], case["m"]
    mem = case["mem"].copy()
    partial, sums = fresh_outputs(case)
    live = n - n % (256 * g) if mistake == "tail_dropped" and n >= 256 * g else n  # elements the loop reaches
    sl = slice(0, live)
    cur = mem[CUR, sl]
    probes = [mem[PROBE0 + j, sl] for j in range(m)]
    cr, ci = np.longdouble(case["cr"]), np.longdouble(case["ci"])

    def axpy(o, t):  # o + (cr + i ci) t, each component in long double and rounded once (the kernel's two fused multiply-adds round twice)
        (ox, oy), (tx, ty) = _ld(o), _ld(t)
        return _cplx(ox + cr * tx - ci * ty + 0.0, oy + cr * ty + ci * tx + 0.0)

    if case["kind"] == "init":
        t = cur
        if case["with_sum"]:
            mem[OUT, sl] = axpy(np.zeros(live, dtype=np.complex128), t)
    else:
        cc = np.longdouble(-case["cc"] if mistake == "b_sign" else case["cc"])
        prev = np.zeros(live, dtype=np.complex128) if case["first"] else mem[PREV, sl]
        (hx, hy), (cx, cy), (px, py) = _ld(mem[HV, sl]), _ld(cur), _ld(prev)
        ch = np.longdouble(case["ch"])
        t = _cplx(ch * hx - px - cc * cx + 0.0, ch * hy - py - cc * cy + 0.0)
        if case["with_sum"]:
            mem[OUT, sl] = axpy(mem[OUT, sl], cur if mistake == "sum_late" else t)
    T = _terms(dict(case, n=live), t, cur, probes, conj_side=mistake == "conj_side")
    if case["kind"] == "step":
        mem[CUR if mistake == "wrong_buffer" else PREV, sl] = t
    blk = _block_of(live, g)
    for b in range(g):
        partial[b] = T[blk == b].sum(axis=0) + 0.0
    sums[:-1] = partial[:g].sum(axis=0)
    return mem, partial, sums


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def _ld(z):
    return np.asarray(z.real, dtype=np.longdouble), np.asarray(z.imag, dtype=np.longdouble)


def check(case, got):
    """got = (mem, partial, sums) after the launch.  -> list of complaints, empty when the result is what the kernel text promises."""
    bad = []
    n, g, m = case["n"], case["grid"], case["m"]
    mem0 = case["mem"]
    mem, partial, sums = got
    step = case["kind"] == "step"
    written = ([PREV] if step else []) + ([OUT] if case["with_sum"] else [])
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
    # normal deviates: long double, with the bounds of the docstring
    cur = mem0[CUR, :n]
    cr, ci = np.longdouble(case["cr"]), np.longdouble(case["ci"])
    if step:
        hx, hy = _ld(mem0[HV, :n])
        cx, cy = _ld(cur)
        px, py = _ld(np.zeros(n, dtype=np.complex128) if case["first"] else mem0[PREV, :n])
        ch, cc = np.longdouble(case["ch"]), np.longdouble(case["cc"])
        t_dev = mem[PREV, :n]
        for name, dv, h, c_, p in (("re", t_dev.real, hx, cx, px), ("im", t_dev.imag, hy, cy, py)):
            ref = ch * h - p - cc * c_
            bound = gamma(2) * (np.abs(ch * h) + np.abs(p) + np.abs(cc * c_))
            if np.any(np.abs(dv - ref) > bound):
                bad.append(f"t_next.{name}: beyond gamma_2 of the magnitudes (max excess {float(np.max(np.abs(dv - ref) - bound)):.3e})")
    else:
        t_dev = cur
    tx, ty = _ld(t_dev)
    if case["with_sum"]:
        ox, oy = _ld(mem0[OUT, :n]) if step else _ld(np.zeros(n, dtype=np.complex128))
        o_dev = mem[OUT, :n]
        for name, dv, ref, bound in (("re", o_dev.real, ox + cr * tx - ci * ty, np.abs(ox) + np.abs(cr * tx) + np.abs(ci * ty)),
                                     ("im", o_dev.imag, oy + cr * ty + ci * tx, np.abs(oy) + np.abs(cr * ty) + np.abs(ci * tx))):
            if np.any(np.abs(dv - ref) > gamma(2) * bound):
                bad.append(f"out.{name}: beyond gamma_2 of the magnitudes")
    # the sums over the t the device wrote
    D = trips(n, g) + -(-g // 256) + 16
    refs, mags = [], []
    for j in range(m):
        qx, qy = _ld(mem0[PROBE0 + j, :n])
        refs += [np.sum(qx * tx + qy * ty), np.sum(qx * ty - qy * tx)]
        mags += [np.sum(np.abs(qx * tx) + np.abs(qy * ty)), np.sum(np.abs(qx * ty) + np.abs(qy * tx))]
    refs.append(np.sum(tx * tx + ty * ty))
    mags.append(refs[-1])
    if step:
        cx, cy = _ld(cur)
        refs += [np.sum(tx * cx + ty * cy), np.sum(tx * cy - ty * cx)]
        mags += [np.sum(np.abs(tx * cx) + np.abs(ty * cy)), np.sum(np.abs(tx * cy) + np.abs(ty * cx))]
    else:
        refs += [np.longdouble(0), np.longdouble(0)]
        mags += [np.longdouble(0), np.longdouble(0)]
    for k, (r, mg) in enumerate(zip(refs, mags)):
        if abs(np.longdouble(sums[k]) - r) > gamma(D + 2) * mg:
            bad.append(f"sum {k}: {sums[k]!r} against {float(r)!r}, bound {float(gamma(D + 2) * mg):.3e}")
    # the final kernel adds the block partials: their sum is the sum, within the final kernel's own additions
    tot = partial[:g].astype(np.longdouble).sum(axis=0)
    if np.any(np.abs(sums[:-1] - tot) > gamma(-(-g // 256) + 8) * np.abs(partial[:g]).astype(np.longdouble).sum(axis=0)):
        bad.append("sums are not the block partials added up")
    return bad
