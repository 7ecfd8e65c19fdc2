"""References for the four kernels of hxv_observables_accumulate (csrc/hxv_observables_kernels.hpp): the cases with their synthetic tables,
a plain numpy evaluation of what each kernel must leave in memory (long double sums over the tables), and check(case, got), which compares
WHOLE buffers with it.  tests/test_gpu_observables_kernels.py runs the cases on the device; tests/test_density_kernels_ref_cpu.py compares
the evaluation with explicit Jordan-Wigner operators and shows that check() refuses the outputs of named wrong kernels.

MEMORY OF A CASE.  psi (and a separate gathered copy `full`) has two columns more than qdw, colout two columns more than qdw and one guard
element, rec one guard element: whatever lies beyond what the launch owns holds NaN (inputs) or SENT (outputs) and must come back with the
same bits -- a launch with grid = qdw + 2 has two workgroups with nothing to do.  Pad rows [dimup, pitch) and every element of an input that
no table names hold NaN, so a read that the tables do not ask for shows in the output; the table entries themselves are always in range and
respect the builders' contract (a column names a pair at most once).  An output element the kernel does not own keeps SENT.

NUMBER FORMATS.  Integers: re, im in [-6, 6] (|z| <= 9), signs +-1; a term is an integer below 2^8, a sum over at most 4096 of them (or 600
column values below 2^15) stays far below 2^53: every product and sum is exact in double in any order, with or without contraction, and a
zero sum is +0.0 (round to nearest gives -0.0 only from two negative zeros, and every accumulator starts as +0.0; obs_rdw_kernel multiplies its
sum by the sign afterwards, so a zero sum under a minus sign is -0.0 there, in the evaluation as on the device): the device's buffers must
equal the evaluation's BIT FOR BIT.  Normal deviates: against the long double sums, with u = 2^-53 and gamma_k = k u / (1 - k u) (Higham,
Accuracy and Stability, lemma 3.1),
        |device - sum| <= gamma_D * sum_i (|a_i b_i| + |c_i d_i|),         D = (additions on a term's longest way) + (roundings inside a term).
  A term  s (a b + c d), s = +-1:  the two products and their sum are rounded (3 roundings, 2 on any one way) without contraction; with it
  fma(a, b, fl(c d)) rounds twice and the multiplication by s joins the accumulating fma: 2 roundings inside a term either way.
  obs_rows_kernel   a lane adds its ceil(n / 64) entries of a group of n in order, then 6 butterfly steps:      D = ceil(n / 64) + 6 + 2
  obs_rdw_kernel    a thread adds ceil(dimup / 256) rows, 6 butterfly steps, the 4 waves in order (3 adds); the sign is exact:
                                                                                                             D = ceil(dimup / 256) + 9 + 2
  obs_reduce_kernel a thread adds ceil(m / 256) of the m column values (the bin's, or all qdw), 6 steps, 3 adds; a term is a stored value:
                                                                                                             D = ceil(m / 256) + 9
(a first addition to +0.0 is exact, so each D counts one more than needed: a margin below a factor 2).  In the driver a record element
passes through a column kernel's chain and then the reduction's: here each kernel's output is compared on given inputs, one chain each."""
import numpy as np

OBS_THREADS = 256
OBS_WAVES = 4
OBS_MAX_NIMP = 10
SENT = -7.25e77
CSENT = complex(SENT, SENT)
NAN = float("nan")
CNAN = complex(NAN, NAN)
U = 2.0 ** -53
LD = np.longdouble
GROUP_SIZES = (130, 0, 65, 1, 64, 63)
FAULTS = ("conj", "sign", "transpose", "boundary", "trip", "adw")


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * U / (1.0 - k * U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _values(rng, shape, integer):
    if integer:
        return (rng.integers(-6, 7, shape) + 1j * rng.integers(-6, 7, shape)).astype(np.complex128)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _ld(z):
    return np.asarray(z.real, dtype=LD), np.asarray(z.imag, dtype=LD)


def _cplx(x, y):
    z = np.empty(np.shape(x), dtype=np.complex128)
    z.real, z.imag = x, y  # (rounded to double here)
    return z


def _tp(p, nimp):
    """the pair index with is and js exchanged"""
    return (p // nimp) + nimp * (p % nimp)


# ---- what the kernels compute, from the tables ---------------------------------------------------------------------------------------------
def rows_values(psi, nimp, qdw, seg_ptr, ea, eb, es, pairs, fault=None):
    """-> (re, im, mag_re, mag_im, D): [qdw, nw] (W bins, im = 0) or [qdw, np] (pair groups) in long double; mag = sum of the magnitudes of
    the products a sum is made of, D as in the module's docstring"""
    nw, npair = 1 << nimp, nimp * nimp
    g0, ng = (nw, npair) if pairs else (0, nw)
    sizes = np.diff(seg_ptr)[g0:g0 + ng]
    e_lo = seg_ptr[g0:g0 + ng].astype(np.int64)
    gid = np.repeat(np.arange(ng), sizes)
    e = np.repeat(e_lo, sizes) + (np.arange(sizes.sum()) - np.repeat(np.cumsum(sizes) - sizes, sizes))
    k_in = e - np.repeat(e_lo, sizes)
    n_of = np.repeat(sizes, sizes)
    if fault == "boundary":
        keep = k_in < n_of - 1
        gid, e = gid[keep], e[keep]
    elif fault == "trip":
        keep = (n_of % 64 == 0) | (k_in < n_of // 64 * 64)
        gid, e = gid[keep], e[keep]
    re, im, mre, mim = (np.zeros((qdw, ng), dtype=LD) for _ in range(4))
    if len(e):
        xr, xi = _ld(psi[:qdw][:, ea[e]])
        yr, yi = _ld(psi[:qdw][:, eb[e]])
        s = np.ones(len(e), dtype=LD) if (fault == "sign" or not pairs) else es[e].astype(LD)
        for c in range(qdw):
            np.add.at(re[c], gid, s * (xr[c] * yr[c] + xi[c] * yi[c]))
            np.add.at(mre[c], gid, np.abs(xr[c] * yr[c]) + np.abs(xi[c] * yi[c]))
            if pairs:
                np.add.at(im[c], gid, s * (xi[c] * yr[c] - xr[c] * yi[c]))
                np.add.at(mim[c], gid, np.abs(xi[c] * yr[c]) + np.abs(xr[c] * yi[c]))
    if pairs and fault == "conj":
        im = -im
    if pairs and fault == "transpose":
        t = [_tp(p, nimp) for p in range(npair)]
        re, im, mre, mim = re[:, t], im[:, t], mre[:, t], mim[:, t]
        sizes = sizes[t]
    return re, im, mre, mim, -(-sizes // 64) + 6 + 2


def rdw_values(psi, full, nimp, dimup, qdw, dwp_ptr, dwp_slot, dwp_p, dwp_s, fault=None):
    """-> (re, im, mag_re, mag_im, D): [qdw, np]; a pair the column does not name: zero"""
    npair = nimp * nimp
    re, im, mre, mim = (np.zeros((qdw, npair), dtype=LD) for _ in range(4))
    live = dimup // 256 * 256 if (fault == "trip" and dimup % 256) else dimup
    for c in range(qdw):
        xr, xi = _ld(psi[c, :live])
        for k in range(dwp_ptr[c], dwp_ptr[c + 1] - (1 if fault == "boundary" else 0)):
            yr, yi = _ld(full[dwp_slot[k], :live])
            s = LD(1 if fault == "sign" else dwp_s[k])
            p = _tp(dwp_p[k], nimp) if fault == "transpose" else dwp_p[k]
            re[c, p] = s * (np.sum(xr * yr + xi * yi) + LD(0))  # (the kernel's accumulator starts as +0.0; the sign multiplies the sum: -0.0 is possible)
            im[c, p] = s * (np.sum(xi * yr - xr * yi) + LD(0)) * (-1 if fault == "conj" else 1)
            mre[c, p] = np.sum(np.abs(xr * yr) + np.abs(xi * yi))
            mim[c, p] = np.sum(np.abs(xi * yr) + np.abs(xr * yi))
    return re, im, mre, mim, -(-dimup // 256) + 9 + 2


def reduce_values(colout, nimp, qdw, dwbin_ptr, dwbin_cols, fault=None):
    """colout [qdw, gtot] complex -> (rec, mag, D): [nw^2 + 4 np] in long double"""
    nw, npair = 1 << nimp, nimp * nimp
    nww = nw * nw
    rec, mag, D = np.zeros(nww + 4 * npair, dtype=LD), np.zeros(nww + 4 * npair, dtype=LD), np.zeros(nww + 4 * npair, dtype=np.int64)
    sizes = np.diff(dwbin_ptr).astype(np.int64)
    k_in = np.arange(len(dwbin_cols)) - np.repeat(dwbin_ptr[:-1].astype(np.int64), sizes)
    n_of = np.repeat(sizes, sizes)
    keep = np.ones(len(dwbin_cols), dtype=bool)
    if fault == "boundary":
        keep = k_in < n_of - 1
    elif fault == "trip":
        keep = (n_of % 256 == 0) | (k_in < n_of // 256 * 256)
    bin_of = np.repeat(np.arange(nw), sizes)[keep]
    cols = np.asarray(dwbin_cols)[keep]
    W, Wm = np.zeros((nw, nw), dtype=LD), np.zeros((nw, nw), dtype=LD)  # [a_dw, a_up]
    if len(cols):
        v = np.asarray(colout[cols, :nw].real, dtype=LD)
        np.add.at(W, bin_of, v)
        np.add.at(Wm, bin_of, np.abs(v))
    Dw = np.repeat(-(-sizes // 256) + 9, nw)
    if fault == "adw":  # a_dw = o >> (nimp - 1): twice the bin, past the last one for the upper half (nothing there)
        o = np.arange(nww)
        a_up, a_dw = o & (nw - 1), o >> (nimp - 1)
        ok = a_dw < nw
        rec[:nww][ok], mag[:nww][ok] = W[a_dw[ok], a_up[ok]], Wm[a_dw[ok], a_up[ok]]
    else:
        rec[:nww], mag[:nww] = W.reshape(-1), Wm.reshape(-1)
    D[:nww] = Dw
    live = qdw // 256 * 256 if (fault == "trip" and qdw % 256) else qdw
    r = colout[:live, nw:nw + 2 * npair]
    rr, ri = _ld(r)
    rec[nww::2], rec[nww + 1::2] = rr.sum(axis=0), ri.sum(axis=0)
    mag[nww::2], mag[nww + 1::2] = np.abs(rr).sum(axis=0), np.abs(ri).sum(axis=0)
    D[nww:] = -(-qdw // 256) + 9
    return rec, mag, D


# ---- tables the builder's way (csrc/hxv_observables_tables.cpp; the reference's row order, one rank) and the whole record ----------------
def _hop(m, i, j):
    """c^+_i c_j |m>, i < j -> (image, sign) or None"""
    if not (m >> j) & 1 or (m >> i) & 1:
        return None
    between = bin(m & ((1 << j) - 1) & ~((1 << (i + 1)) - 1)).count("1")
    return (m ^ (1 << j)) | (1 << i), -1 if between & 1 else 1


def build_tables(map_up, map_dw, nimp):
    nw, npair = 1 << nimp, nimp * nimp
    mu, md = [int(x) for x in map_up], [int(x) for x in map_dw]
    iu, idw = {m: k for k, m in enumerate(mu)}, {m: k for k, m in enumerate(md)}
    seg, ea, eb, es = [], [], [], []
    for g in range(nw):
        seg.append(len(ea))
        rows = [r for r, m in enumerate(mu) if m & (nw - 1) == g]
        ea += rows
        eb += rows
        es += [1] * len(rows)
    for p in range(npair):
        i, j = p % nimp, p // nimp
        seg.append(len(ea))
        if i >= j:
            continue
        for r, m in enumerate(mu):
            h = _hop(m, i, j)
            if h:
                ea.append(r), eb.append(iu[h[0]]), es.append(h[1])
    seg.append(len(ea))
    dptr, dslot, dp, ds = [0], [], [], []
    for m in md:
        for p in range(npair):
            i, j = p % nimp, p // nimp
            h = _hop(m, i, j) if i < j else None
            if h:
                dslot.append(idw[h[0]]), dp.append(p), ds.append(h[1])
        dptr.append(len(dslot))
    bins = [[c for c, m in enumerate(md) if m & (nw - 1) == g] for g in range(nw)]
    bptr = np.concatenate([[0], np.cumsum([len(b) for b in bins])])
    i32, i8 = (lambda x: np.asarray(x, dtype=np.int32)), (lambda x: np.asarray(x, dtype=np.int8))
    return dict(nimp=nimp, seg_ptr=i32(seg), ent_a=i32(ea), ent_b=i32(eb), ent_s=i8(es), dwp_ptr=i32(dptr), dwp_slot=i32(dslot), dwp_p=i32(dp),
                dwp_s=i8(ds), dwbin_ptr=i32(bptr), dwbin_cols=i32([c for b in bins for c in b]))


def record(t, psi):
    """psi [dimdw, dimup] -> the raw record [nw^2 + 4 np] the four kernels leave (long double), through the same evaluation check() uses"""
    nimp, (qdw, dimup) = t["nimp"], psi.shape
    nw, npair = 1 << nimp, nimp * nimp
    col = np.zeros((qdw, nw + 2 * npair), dtype=np.clongdouble)
    w = rows_values(psi, nimp, qdw, t["seg_ptr"], t["ent_a"], t["ent_b"], t["ent_s"], False)
    r = rows_values(psi, nimp, qdw, t["seg_ptr"], t["ent_a"], t["ent_b"], t["ent_s"], True)
    d = rdw_values(psi, psi, nimp, dimup, qdw, t["dwp_ptr"], t["dwp_slot"], t["dwp_p"], t["dwp_s"])
    col[:, :nw] = w[0]
    col[:, nw:nw + npair] = r[0] + 1j * r[1]
    col[:, nw + npair:] = d[0] + 1j * d[1]
    return reduce_values(col, nimp, qdw, t["dwbin_ptr"], t["dwbin_cols"])[0]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def rows_cases():
    """(nimp, dimup, qdw, grid)"""
    return [(n, d, q, q + x) for n in (1, 3, 5, 10) for d in (1, 5, 300) for q in (1, 3) for x in (0, 2)]


def make_rows(seed, nimp, dimup, qdw, grid, pairs, integer):
    rng = np.random.default_rng(seed)
    nw, npair = 1 << nimp, nimp * nimp
    ng = nw + npair
    sizes = np.array([GROUP_SIZES[(seed + g) % 6] for g in range(ng)])
    sizes[nw:] = [GROUP_SIZES[(seed + 3 + p) % 6] for p in range(npair)]  # (the pair groups start elsewhere in the cycle than the W bins)
    seg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    nent = int(seg_ptr[-1])
    ea = rng.integers(0, dimup, nent).astype(np.int32)
    eb = rng.integers(0, dimup, nent).astype(np.int32)  # a != b wherever dimup > 1
    es = rng.choice(np.array([-1, 1], dtype=np.int8), nent)
    eb[:seg_ptr[nw]] = ea[:seg_ptr[nw]]
    es[:seg_ptr[nw]] = 1
    pitch = (dimup + 7) // 8 * 8
    psi = np.full((qdw + 2, pitch), CNAN)
    lo, hi = (seg_ptr[nw], nent) if pairs else (0, seg_ptr[nw])
    named = np.unique(np.concatenate([ea[lo:hi], eb[lo:hi]]))
    psi[:qdw, named] = _values(rng, (qdw, len(named)), integer)
    return dict(kind="rows", pairs=pairs, nimp=nimp, dimup=dimup, pitch=pitch, qdw=qdw, grid=grid, integer=integer, psi=psi, seg_ptr=seg_ptr,
                ent_a=ea, ent_b=eb, ent_s=es, out0=np.full((qdw + 2) * (nw + 2 * npair) + 1, CSENT))


def rdw_cases():
    """(nimp, dimup, separate, grid surplus)"""
    return [(n, d, s, 2 * ((k + s) % 2)) for n in (1, 3, 10) for k, d in enumerate((1, 255, 256, 257, 600)) for s in (0, 1)]


def make_rdw(seed, nimp, dimup, separate, surplus, integer):
    """three columns: no pair, one pair, all np pairs in a shuffled order.  separate: `full` is a gathered copy of 2 ranks x cmax = 4 slots
    (this rank's slab at slots 4 .. 6, slot 7 unused) instead of psi itself"""
    rng = np.random.default_rng(seed)
    nw, npair, qdw = 1 << nimp, nimp * nimp, 3
    nslot = 8 if separate else qdw
    dwp_ptr = np.array([0, 0, 1, 1 + npair], dtype=np.int32)
    dwp_p = np.concatenate([[rng.integers(0, npair)], rng.permutation(npair)]).astype(np.int32)
    dwp_slot = rng.integers(0, nslot - (1 if separate else 0), 1 + npair).astype(np.int32)
    dwp_s = rng.choice(np.array([-1, 1], dtype=np.int8), 1 + npair)
    pitch = (dimup + 7) // 8 * 8
    psi = np.full((qdw + 2, pitch), CNAN)
    psi[1:qdw, :dimup] = _values(rng, (qdw - 1, dimup), integer)  # (column 0 has no pair: it is read only as somebody's partner)
    if separate:
        full = np.full((nslot, pitch), CNAN)
        used = np.unique(dwp_slot)
        full[used, :dimup] = _values(rng, (len(used), dimup), integer)
        for c in range(1, qdw):
            if 4 + c in used:
                full[4 + c] = psi[c]  # (a gathered copy holds the slab itself)
    else:
        if 0 in dwp_slot:
            psi[0, :dimup] = _values(rng, dimup, integer)
        full = None
    return dict(kind="rdw", nimp=nimp, dimup=dimup, pitch=pitch, qdw=qdw, grid=qdw + surplus, integer=integer, psi=psi, full=full, dwp_ptr=dwp_ptr,
                dwp_slot=dwp_slot, dwp_p=dwp_p, dwp_s=dwp_s, out0=np.full((qdw + 2) * (nw + 2 * npair) + 1, CSENT))


def reduce_cases():
    """(nimp, qdw, one_bin)"""
    return [(n, q, b) for n in (1, 3, 5, 10) for q in (0, 1, 255, 256, 257, 600) for b in (False, True)]


def make_reduce(seed, nimp, qdw, one_bin, integer):
    """one_bin: one dw bin holds every column and the others are empty; else bin 0 is empty and the columns are spread over the others.
    dwbin_cols is a shuffled permutation either way."""
    rng = np.random.default_rng(seed)
    nw, npair = 1 << nimp, nimp * nimp
    bins = np.full(qdw, int(rng.integers(0, nw))) if one_bin else rng.integers(1, nw, qdw)
    order = np.lexsort((rng.permutation(qdw), bins))
    dwbin_ptr = np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=nw))]).astype(np.int32)
    colout = _values(rng, (qdw, nw + 2 * npair), integer)
    colout.imag[:, :nw] = NAN  # (a W slot's imaginary part is nobody's input)
    return dict(kind="reduce", nimp=nimp, qdw=qdw, grid=nw * nw + 2 * npair, integer=integer, colout=colout, dwbin_ptr=dwbin_ptr,
                dwbin_cols=order.astype(np.int32), out0=np.full(nw * nw + 4 * npair + 1, SENT))


# ---- the evaluation as buffers, and the check -------------------------------------------------------------------------------------------
def _expect(case, fault=None):
    """-> (written, re, im, mag_re, mag_im, D) over the case's WHOLE output buffer (complex for the column kernels, real for the record; im
    parts None there): written = the elements the kernel owns"""
    nimp, qdw = case["nimp"], case["qdw"]
    nw, npair = 1 << nimp, nimp * nimp
    gtot = nw + 2 * npair
    n = len(case["out0"])
    if case["kind"] == "reduce":
        rec, mag, D = reduce_values(case["colout"], nimp, qdw, case["dwbin_ptr"], case["dwbin_cols"], fault)
        written = np.ones(n, dtype=bool)
        written[-1] = False
        pad = lambda a, dt: np.concatenate([a, np.zeros(1, dtype=dt)])  # noqa: E731
        return written, pad(rec, LD), None, pad(mag, LD), None, pad(D, np.int64)
    if case["kind"] == "rows":
        v = rows_values(case["psi"], nimp, qdw, case["seg_ptr"], case["ent_a"], case["ent_b"], case["ent_s"], case["pairs"], fault)
        s0, ns = (nw, npair) if case["pairs"] else (0, nw)
    else:
        full = case["psi"] if case["full"] is None else case["full"]
        v = rdw_values(case["psi"], full, nimp, case["dimup"], qdw, case["dwp_ptr"], case["dwp_slot"], case["dwp_p"], case["dwp_s"], fault)
        s0, ns = nw + npair, npair
    written = np.zeros(n, dtype=bool)
    out = [np.zeros(n, dtype=LD) for _ in range(4)] + [np.zeros(n, dtype=np.int64)]
    for c in range(qdw):
        sl = slice(c * gtot + s0, c * gtot + s0 + ns)
        written[sl] = True
        for k in range(4):
            out[k][sl] = v[k][c]
        out[4][sl] = v[4]
    return (written,) + tuple(out)


def evaluate(case, fault=None):
    """the output buffer a kernel with the named fault (None: the kernel of the header) leaves, rounded to double from the long double sums"""
    written, re, im, _, _, _ = _expect(case, fault)
    got = case["out0"].copy()
    if im is None:
        got[written] = re[written].astype(np.float64)
    else:
        got[written] = _cplx(re[written].astype(np.float64), im[written].astype(np.float64))
    return got


def check(case, got, ratios=None):
    """got: the whole output buffer after the launch -> list of complaints, empty when it is what the kernel text promises.  ratios: a list
    that receives the largest error / bound of a normal-deviate case (to be recorded, not asserted)"""
    bad = []
    out0 = case["out0"]
    if got.shape != out0.shape or got.dtype != out0.dtype:
        return [f"buffer of shape {got.shape} {got.dtype}"]
    written, re, im, mre, mim, D = _expect(case)
    if not same_bits(got[~written], out0[~written]):
        bad.append("an element the kernel does not own was written")
    g = got[written]
    parts = [("re", g.real, re[written], mre[written])] + ([] if im is None else [("im", g.imag, im[written], mim[written])])
    for name, dev, ref, mag in parts:
        if not np.all(np.isfinite(dev)):
            bad.append(f"{name}: not finite -- something no table names was read, or an owned element was not written")
        elif case["integer"]:
            if not same_bits(np.ascontiguousarray(dev), ref.astype(np.float64)):
                bad.append(f"{name}: not the exact sums bit for bit")
        else:
            err, bound = np.abs(dev.astype(LD) - ref), gamma(D[written]) * mag
            if np.any(err > bound):
                k = int(np.argmax(err - bound))
                bad.append(f"{name}: {dev[k]!r} against {float(ref[k])!r}, bound {float(bound[k]):.3e}")
            elif ratios is not None and np.any(bound > 0):
                ratios.append(float(np.max(err[bound > 0] / bound[bound > 0])))
    return bad
