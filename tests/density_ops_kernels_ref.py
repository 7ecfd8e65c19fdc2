"""References for the three kernels of hxv_apply_density_ops (csrc/hxv_density_ops_kernels.hpp): the cases with their synthetic tables, a
plain numpy evaluation of what each kernel must leave in memory (long double sums), and check(case, got), which compares WHOLE buffers with
it.  tests/test_gpu_density_ops_kernels.py runs the cases on the device; tests/test_density_kernels_ref_cpu.py compares the evaluation with
explicit Jordan-Wigner operators and shows that check() refuses the outputs of named wrong kernels.

WHAT THE KERNELS COMPUTE.  f_a(r, c) = fu_a(occ_up[r]) + fd_a(occ_dw[c]),  fs_a(o) = sum over the set bits is of o of coef[a][s][is], the low
five bits and the bits above summed apart and then added.  A work item = (column c, chunk k of `rows` rows), item i = c nchunk + k on workgroup
i mod grid.  Pass 1: partial[b][a] = sum over b's items of f_a |psi|^2 (a < nops; +0.0 for nops <= a < DOP_MAX), partial[b][DOP_MAX] = the
same of |psi|^2.  Pass 2: out_a = (f_a - m_a) psi on the rows below dimup, +0.0 on the pad rows [dimup, pitch) of every column;
partial[b][a] = sum of |out_a|^2, +0.0 for a >= nops (slot DOP_MAX included).  A workgroup without an item writes nine +0.0.  The reduction:
sums[v] = sum over the blocks of partial[.][v], or of partial[.][DOP_MAX] for v = norm_at.

MEMORY OF A CASE.  psi has one column more than qdw, every output vector too, partial one row more than the grid, sums one entry more than
DOP_NSUM: whatever lies beyond what the launch owns holds NaN (inputs) or SENT (outputs) and must come back with the same bits.  The pad
rows of psi hold NaN; occ_up is zero there as the builder leaves it.  The columns of `partial` that a reduction does not read hold NaN.

NUMBER FORMATS.  Integers: psi re, im in [-6, 6], coefficients in [-3, 3], means in [-5, 5] without 0 (or all 0): |f - m| <= 65, a term
below 2^19, a sum over the at most 12291 elements of a case below 2^33: everything is exact in double in any order, with or without
contraction, zero sums are +0.0: BIT FOR BIT.  Normal deviates, u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, lemma
3.1; a sum evaluated along any tree of height h errs by at most gamma_h times the sum of the magnitudes):
  f_a      a half's table entry adds at most min(nimp, 5) coefficients, the first to +0.0: h5 = min(nimp, 5) - 1 roundings; + 1 where the
           halves are added (nimp > 5); + 1 for fu + fd:  df = h5 + [nimp > 5] + 1, against  mf = the sum of the |coef| added.
           Pass 2 subtracts m from fd first: dg = df + 1, mg = mf + |m|.
  out_a    one more rounding for the product:  |out - (f - m) psi| <= gamma_{dg + 1} mg |psi|  per component.
  sums     |psi|^2 = x^2 + y^2: two roundings on a way, contracted or not.  A thread adds its elements of an item in ceil(len / 256) steps
           (len = the item's rows below dimup; the lanes beyond them add exact zeros), item after item: T_b = the sum of that over the
           workgroup's items; then 6 butterfly steps and the 4 waves in order (3 adds).
             pass 1:  D = T_b + 9 + df + 2 + 1  (f, |psi|^2, their product; contraction saves one), against sum mf |psi|^2;
                      the norm  D = T_b + 9 + 2.
             pass 2:  over the out THE DEVICE WROTE (its own bound is the item above):  D = T_b + 9 + 2.
  reduce   a thread adds ceil(nblocks / 256) partials, 6 steps, 3 adds:  D = ceil(nblocks / 256) + 9.
(a first addition to +0.0 is exact, so each D counts one more than needed: a margin below a factor 2)."""
import numpy as np

DOP_THREADS = 256
DOP_MAX = 8
DOP_NSUM = 9
DOP_MAX_NIMP = 10
DOP_UNROLL = 4
DOP_CHUNK = 2048
DOP_WG_PER_CU = 8
SENT = -7.25e77
CSENT = complex(SENT, SENT)
NAN = float("nan")
CNAN = complex(NAN, NAN)
U = 2.0 ** -53
LD = np.longdouble
FAULTS = ("hi", "chunk", "item1", "pad", "trip")


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * U / (1.0 - k * U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def chunking(pitch):
    """the builder's formula (csrc/hxv_density_ops_tables.cpp; pinned by tests/host/density_tables_check.cpp) -> (nchunk, rows)"""
    nchunk = max(1, -(-pitch // DOP_CHUNK))
    return nchunk, (-(-pitch // nchunk) + 7) // 8 * 8


def grid_for(nitems, ncu):
    return max(1, min(nitems, DOP_WG_PER_CU * ncu))


def _values(rng, shape, integer):
    if integer:
        return (rng.integers(-6, 7, shape) + 1j * rng.integers(-6, 7, shape)).astype(np.complex128)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _ld(z):
    return np.asarray(z.real, dtype=LD), np.asarray(z.imag, dtype=LD)


def f_tables(coef, nimp, occ, spin, fault=None):
    """coef [nops, 2, nimp], occ [n] -> (f [nops, n], magnitude [nops, n]) in long double"""
    nops = coef.shape[0]
    f, mf = np.zeros((nops, len(occ)), dtype=LD), np.zeros((nops, len(occ)), dtype=LD)
    for i in range(min(nimp, 5) if fault == "hi" else nimp):
        bit = ((np.asarray(occ, dtype=np.int64) >> i) & 1).astype(LD)
        f += coef[:, spin, i].astype(LD)[:, None] * bit[None, :]
        mf += np.abs(coef[:, spin, i]).astype(LD)[:, None] * bit[None, :]
    return f, mf


def depth_f(nimp):
    return min(nimp, 5) - 1 + (1 if nimp > 5 else 0) + 1


def _geometry(case, fault=None):
    """-> (item [qdw, pitch]: the work item an element belongs to, covered [qdw, pitch]: some work item reaches it, T [grid]: per-thread
    steps of each workgroup)"""
    qdw, pitch, dimup, nchunk, rows, grid = (case[k] for k in ("qdw", "pitch", "dimup", "nchunk", "rows", "grid"))
    r = np.arange(pitch)
    chunk = r // rows
    covered = np.broadcast_to(chunk < (nchunk - 1 if (fault == "chunk" and nchunk > 1) else nchunk), (qdw, pitch)).copy()
    item = np.arange(qdw)[:, None] * nchunk + chunk[None, :]
    if fault == "trip":  # the last, ragged trip of 1024 rows of an item is not made
        r0 = chunk * rows
        ln = np.minimum(r0 + rows, pitch) - r0
        covered &= np.broadcast_to((ln % 1024 == 0) | (r - r0 < ln // 1024 * 1024), (qdw, pitch))
    T = np.zeros(grid, dtype=np.int64)
    for it in range(qdw * nchunk):
        r0 = (it % nchunk) * rows
        T[it % grid] += -(-max(0, min(r0 + rows, dimup) - r0) // 256)
    return item, covered, T


def _block_sums(case, item, term, fault=None):
    """term [qdw, pitch] (zero where nothing is added) -> [grid] sums by workgroup"""
    grid, nitems = case["grid"], case["qdw"] * case["nchunk"]
    per_item = np.zeros(max(nitems, 1), dtype=LD)
    np.add.at(per_item, item.reshape(-1), term.reshape(-1))
    out = np.zeros(grid, dtype=LD)
    for b in range(grid):
        its = np.arange(b, nitems, 1 if fault == "item1" else grid)
        out[b] = per_item[its].sum() if len(its) else LD(0)
    return out


def sums_expect(case, fault=None):
    """-> (partial, mag, D): [grid, DOP_NSUM] in long double"""
    qdw, pitch, dimup, nimp, nops, grid = (case[k] for k in ("qdw", "pitch", "dimup", "nimp", "nops", "grid"))
    item, covered, T = _geometry(case, fault)
    item = np.minimum(item, max(qdw * case["nchunk"] - 1, 0))  # (rows beyond the last chunk: not covered, any item will do)
    live = covered & (np.arange(pitch) < dimup)[None, :]
    xr, xi = _ld(np.where(live, case["psi"][:qdw], 0.0))
    w = xr * xr + xi * xi
    fu, mu = f_tables(case["coef"], nimp, case["occ_up"], 0, fault)
    fd, md = f_tables(case["coef"], nimp, case["occ_dw"][:qdw], 1, fault)
    partial, mag, D = np.zeros((grid, DOP_NSUM), dtype=LD), np.zeros((grid, DOP_NSUM), dtype=LD), np.zeros((grid, DOP_NSUM), dtype=np.int64)
    for a in range(nops):
        partial[:, a] = _block_sums(case, item, (fu[a][None, :] + fd[a][:, None]) * w, fault)
        mag[:, a] = _block_sums(case, item, (mu[a][None, :] + md[a][:, None]) * w, fault)
        D[:, a] = T + 9 + depth_f(nimp) + 3
    partial[:, DOP_MAX] = mag[:, DOP_MAX] = _block_sums(case, item, w, fault)
    D[:, DOP_MAX] = T + 9 + 2
    return partial, mag, D


def apply_expect(case, fault=None):
    """-> (written [qdw, pitch], re, im, mag [nops, qdw, pitch] in long double): out_a and the magnitude its error is measured against
    (mg |psi| per component is mag * |component|: returned as mg alone)"""
    qdw, pitch, dimup, nimp, nops = (case[k] for k in ("qdw", "pitch", "dimup", "nimp", "nops"))
    _, covered, _ = _geometry(case, fault)
    below = (np.arange(pitch) < dimup)[None, :]
    written = covered & (below | (fault != "pad"))
    xr, xi = _ld(np.where(covered & below, case["psi"][:qdw], 0.0))
    fu, mu = f_tables(case["coef"], nimp, case["occ_up"], 0, fault)
    fd, md = f_tables(case["coef"], nimp, case["occ_dw"][:qdw], 1, fault)
    m = case["m"].astype(LD)
    g = fu[:, None, :] + fd[:, :, None] - m[:, None, None]
    mg = mu[:, None, :] + md[:, :, None] + np.abs(m)[:, None, None]
    zero = LD(0)  # (a pad row is written as +0.0, not as (f - m) times a zero)
    return written, np.where(below[None], g * xr[None], zero), np.where(below[None], g * xi[None], zero), mg


def _norm_partials(case, outs, fault=None):
    """[grid, DOP_NSUM] sums of |out_a|^2 by workgroup over the vectors `outs` [nops, qdw + 1, pitch] (where written), and T"""
    item, covered, T = _geometry(case, fault)
    item = np.minimum(item, max(case["qdw"] * case["nchunk"] - 1, 0))
    part = np.zeros((case["grid"], DOP_NSUM), dtype=LD)
    for a in range(case["nops"]):
        yr, yi = _ld(np.where(covered, outs[a, :case["qdw"]], 0.0))
        part[:, a] = _block_sums(case, item, yr * yr + yi * yi, fault)
    return part, T


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
SHAPES = ((5, 8) + chunking(8), (2041, 2048) + chunking(2048), (4097, 4104) + chunking(4104), (13, 16, 3, 8))
NIMP_NOPS = [(n, k) for n in (1, 5, 6, 10) for k in (1, 3, 8)]


def pass_cases():
    """(dimup, pitch, nchunk, rows, qdw, grid, nimp, nops, zero_mean): the shapes, column counts and grids crossed, the (nimp, nops) pairs
    dealt over them in turn (each three times or more), then every (nimp, nops) pair on the synthetic shape with two workgroups"""
    out, k = [], 0
    for shape in SHAPES:
        for qdw in (1, 3):
            nitems = qdw * shape[2]
            for grid in (1, 2, nitems, nitems + 5):
                out.append(shape + (qdw, grid) + NIMP_NOPS[(5 * k) % 12] + (k % 3 == 0,))
                k += 1
    out += [SHAPES[3] + (3, 2) + nn + (i % 2 == 1,) for i, nn in enumerate(NIMP_NOPS)]
    return out


def make_pass(seed, kind, dimup, pitch, nchunk, rows, qdw, grid, nimp, nops, zero_mean, integer):
    assert kind in ("sums", "apply")
    rng = np.random.default_rng(seed)
    psi = np.full((qdw + 1, pitch), CNAN)
    psi[:qdw, :dimup] = _values(rng, (qdw, dimup), integer)
    occ_up = np.zeros(pitch, dtype=np.uint32)
    occ_up[:dimup] = rng.integers(0, 1 << nimp, dimup)
    occ_dw = rng.integers(0, 1 << nimp, qdw + 1).astype(np.uint32)
    if integer:
        coef = rng.integers(-3, 4, (nops, 2, nimp)).astype(np.float64)
        m = (rng.integers(1, 6, nops) * rng.choice([-1, 1], nops)).astype(np.float64)
    else:
        coef, m = rng.standard_normal((nops, 2, nimp)), rng.standard_normal(nops)
    if zero_mean or kind == "sums":
        m = np.zeros(nops)
    return dict(kind=kind, dimup=dimup, pitch=pitch, nchunk=nchunk, rows=rows, qdw=qdw, grid=grid, nimp=nimp, nops=nops, integer=integer, psi=psi,
                occ_up=occ_up, occ_dw=occ_dw, coef=coef, m=m, partial0=np.full((grid + 1, DOP_NSUM), SENT),
                outs0=np.full((nops, qdw + 1, pitch), CSENT) if kind == "apply" else None)


def reduce_cases():
    """(nblocks, nops, norm_at, grid)"""
    return [(nb, nops, na, nops + x) for nb in (1, 255, 256, 257, 600) for nops in (1, 3, 8) for na in (-1, nops) for x in (0, 1)]


def make_reduce(seed, nblocks, nops, norm_at, grid, integer):
    rng = np.random.default_rng(seed)
    partial = np.full((nblocks + 1, DOP_NSUM), NAN)
    read = sorted({DOP_MAX if v == norm_at else v for v in range(grid)})
    partial[:nblocks, read] = rng.integers(-900, 901, (nblocks, len(read))) if integer else rng.standard_normal((nblocks, len(read)))
    return dict(kind="reduce", nblocks=nblocks, nops=nops, norm_at=norm_at, grid=grid, integer=integer, partial=partial,
                sums0=np.full(DOP_NSUM + 1, SENT))


def reduce_expect(case, fault=None):
    nb = case["nblocks"]
    live = nb // 256 * 256 if (fault == "trip" and nb % 256) else nb
    src = [DOP_MAX if v == case["norm_at"] else v for v in range(case["grid"])]
    p = case["partial"][:live][:, src].astype(LD)
    return p.sum(axis=0) + LD(0), np.abs(p).sum(axis=0), -(-nb // 256) + 9


# ---- the evaluation as buffers, and the check -------------------------------------------------------------------------------------------
def evaluate(case, fault=None):
    """the buffers a kernel with the named fault (None: the kernel of the header) leaves, rounded to double from the long double values:
    (partial,) for pass 1, (outs, partial) for pass 2, (sums,) for the reduction"""
    if case["kind"] == "reduce":
        sums = case["sums0"].copy()
        sums[:case["grid"]] = reduce_expect(case, fault)[0].astype(np.float64)
        return (sums,)
    partial = case["partial0"].copy()
    if case["kind"] == "sums":
        partial[:case["grid"]] = sums_expect(case, fault)[0].astype(np.float64)
        return (partial,)
    written, re, im, _ = apply_expect(case, fault)
    outs = case["outs0"].copy()
    for a in range(case["nops"]):
        o = outs[a, :case["qdw"]]
        o.real[written], o.imag[written] = re[a][written].astype(np.float64), im[a][written].astype(np.float64)
    partial[:case["grid"]] = _norm_partials(case, outs, fault)[0].astype(np.float64)
    return outs, partial


def _cmp(bad, name, integer, dev, ref, bound, ratios):
    if not np.all(np.isfinite(dev)):
        bad.append(f"{name}: not finite -- something that must not be read was read, or an owned element was not written")
    elif integer:
        if not same_bits(dev, np.asarray(ref).astype(np.float64)):
            bad.append(f"{name}: not the exact values bit for bit")
    else:
        err = np.abs(np.asarray(dev).astype(LD) - ref)
        if np.any(err > bound):
            k = np.unravel_index(int(np.argmax(err - bound)), err.shape)
            bad.append(f"{name}: {float(np.asarray(dev)[k])!r} against {float(np.asarray(ref)[k])!r}, bound {float(np.asarray(bound)[k]):.3e}")
        elif ratios is not None and np.any(bound > 0):
            ratios.append(float(np.max(err[bound > 0] / bound[bound > 0])))


def _zero_slots(case, partial):
    """the slots of the operators that are not there, and every slot of a workgroup without an item, are +0.0 and nothing else"""
    g, nops, nitems = case["grid"], case["nops"], case["qdw"] * case["nchunk"]
    bad = []
    if not same_bits(partial[:g, nops:DOP_MAX], np.zeros((g, DOP_MAX - nops))):
        bad.append("a partial slot of an operator beyond nops is not +0.0")
    if not same_bits(partial[nitems:g], np.zeros((max(g - nitems, 0), DOP_NSUM))):
        bad.append("a workgroup without an item did not write zeros")
    return bad


def check(case, got, ratios=None):
    """got: the buffers of evaluate()'s shape after the launch -> list of complaints, empty when they are what the kernel text promises.
    ratios: a list that receives the largest error / bound of a normal-deviate case (to be recorded, not asserted)"""
    bad = []
    integer = case["integer"]
    if case["kind"] == "reduce":
        (sums,) = got
        g = case["grid"]
        if not same_bits(sums[g:], case["sums0"][g:]):
            bad.append("an entry behind the sums was written")
        ref, mag, D = reduce_expect(case)
        _cmp(bad, "sums", integer, sums[:g], ref, gamma(D) * mag, ratios)
        return bad
    partial = got[-1]
    g = case["grid"]
    if not same_bits(partial[g:], case["partial0"][g:]):
        bad.append("the partial row behind the grid was written")
    if case["kind"] == "sums":
        ref, mag, D = sums_expect(case)
        _cmp(bad, "partial", integer, partial[:g], ref, gamma(D) * mag, ratios)
        return bad + _zero_slots(case, partial)
    outs = got[0]
    qdw, nops = case["qdw"], case["nops"]
    if not same_bits(outs[:, qdw], case["outs0"][:, qdw]):
        bad.append("the column behind the slab was written")
    written, re, im, mg = apply_expect(case)
    if not np.all(written):
        if not same_bits(outs[:, :qdw][:, ~written], case["outs0"][:, :qdw][:, ~written]):
            bad.append("an element no work item owns was written")
    o = np.ascontiguousarray(outs[:, :qdw][:, written])
    if not np.all(np.isfinite(o.view(np.float64))):
        return bad + ["out: not finite -- a pad row of psi was read, or an owned element was not written"]
    xr, xi = _ld(np.where(written & (np.arange(case["pitch"]) < case["dimup"])[None, :], case["psi"][:qdw], 0.0))
    k = gamma(depth_f(case["nimp"]) + 2)
    _cmp(bad, "out.re", integer, np.ascontiguousarray(o.real), re[:, written], k * (mg * np.abs(xr)[None])[:, written], ratios)
    _cmp(bad, "out.im", integer, np.ascontiguousarray(o.imag), im[:, written], k * (mg * np.abs(xi)[None])[:, written], ratios)
    pad = outs[:, :qdw, case["dimup"]:][:, written[:, case["dimup"]:]]
    if not same_bits(pad, np.zeros_like(pad)):
        bad.append("a pad row of an output is not +0.0")
    ref, T = _norm_partials(case, outs)  # over the vectors the device wrote
    D = np.repeat((T + 9 + 2)[:, None], DOP_NSUM, axis=1)
    _cmp(bad, "partial", integer, partial[:g], ref, gamma(D) * ref, ratios)
    if not same_bits(partial[:g, DOP_MAX], np.zeros(g)):
        bad.append("pass 2 left something in the norm's slot")
    return bad + _zero_slots(case, partial)
