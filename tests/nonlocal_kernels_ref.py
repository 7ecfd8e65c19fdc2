"""What the three kernels of the non-local block spH0nd promise (csrc/hxv_nonlocal_kernels.hpp: hxv_nonlocal_kernel, hxv_nonlocal_tab,
hxv_nonlocal_csr), restated in numpy, and the cases they are run on one by one (tests/test_gpu_nonlocal_kernels.py on the device,
tests/test_nonlocal_kernels_ref_cpu.py without one).

All three compute, for every local element (row i of local column cl, global column c = dw0 + cl),

    hv[cl*pitch + i] += sum_k coef_k * v[slot_k*pitch + row_k]

and leave hv alone (not even "+= 0") where the sum has no term.  They differ in where the terms come from.

WHAT A TABLE WORD MEANS (read from the kernels and from the builder `moves` in build_sector_from_model, hxv_sector.cpp)

  hxv_nonlocal_tab reads the one-spin move tables nd_up [Q][DimUp] and nd_dw [Q][DimDw], Q = nlat*norb*norb, entry number
  (il*norb + x)*norb + y for "site il, orbital x -> orbital y", x != y (the entries with x == y exist and are never read).  The word of
  state s in entry (il, x, y) describes c^+_y c_x |s>:
    - ND_INVALID = 0xFFFFFFFF when the move does not apply (x empty or y occupied);
    - otherwise bit 31 is the fermionic sign (1 = minus) and bits 0..30 are the index of the target.  For the up table the index is a ROW
      of a column.  For the dw table it is already a COLUMN SLOT of the gathered vector v (the builder stores vcol[target]), so this kernel
      never reads vcol and the slots may lie anywhere in v.
  For the orbital pair (io, jo), io != jo, of site il the kernel calls q the entry (il, io, jo) and r the entry (il, jo, io).  Spin
  exchange is [c^+_jo c_io]_dw [c^+_io c_jo]_up: dw word from entry q, up word from entry r, coefficient Jx.  Pair hopping is
  [c^+_io c_jo]_dw [c^+_io c_jo]_up: dw word from entry r, up word from entry r, coefficient Jp.  A term exists when both words are valid
  and its coupling is not zero; its sign is the XOR of the two sign bits, its source v[slot(dw word)*pitch + index(up word)].

  hxv_nonlocal_kernel has no tables: it reads the sorted configurations map_up [DimUp], map_dw [DimDw] (orbital o of site il is bit
  il*norb + o), applies the same two operators to the bit strings, finds the targets by binary search and reads
  v[vcol[target column]*pitch + target row]: vcol [DimDw] maps a global dw column to its column slot of v.

  hxv_nonlocal_csr reads stored rows: rowptr [nloc + 1] over the LOCAL elements t = cl*DimUp + i, cols 1-based (Fortran) GLOBAL state
  numbers j + 1 with j = jdw*DimUp + jup (the split is by DimUp, never by the pitch), complex vals; the source is
  v[vcol[jdw]*pitch + jup].  A row with no stored entry is not written.

  Pad rows (DimUp <= row < pitch) of v are never read and those of hv never written.

THE RESTATEMENTS (`*_terms`) list, per local element, the terms (coefficient, index into v) in the kernel's order, from the case's tables
alone.  Every lookup goes through `look`, which refuses an index outside its array, and every index into v through `Reads.at`, which also
records it: the recorded set is what the contract reads, `inputs` puts NaN everywhere else in v.  `expected` turns terms and v into the
whole hv buffer; `check` compares a buffer a kernel (or `*_emulate`) produced with it.

VALUES.  hv starts from a sentinel pattern (every third element (-0.0, -0.0), the others SENT), one guard element behind it included.
Elements the contract does not write -- pad rows, the guard, elements without a term -- keep those bits, compared as 64-bit patterns: a
"+= 0.0" turns a -0.0 into +0.0 and shows.
  exact:  v holds small nonzero integers, Jx, Jp and the parts of the CSR values are signed powers of two: every product and every partial
          sum is exact in double in any order, fused or not, so acc is exact and hv = fl(h0 + acc) is ONE correctly rounded addition (per
          component), the same in numpy and on the device.  The whole buffer is compared by bits.
  random: v and the coefficients are normal deviates.  The reference is h0 + the sum in numpy.longdouble (64-bit significand, checked at
          use).  THE BOUND, derived before any device run, u = 2**-53, per component, T = the number of terms of THAT element:
          real coefficients (kernel, tab): acc = 0; acc = fl(acc + fl(c*x)) (or one fma) T times; h = fl(h0 + acc).  The first addition
          is to zero and exact, so a term passes through at most 1 product, T - 1 additions and the final addition: T + 1 roundings,
          h0 through one.  |h - exact| <= gamma_{T+1} * sum|c||x| + u*|h0|, gamma_n = n*u/(1 - n*u), and gamma_{T+1} <= (T + 3/2)*u for
          T <= 2**40, so     |h - exact| <= (T + 2) * u * (|h0| + sum|c||x|)     with u/2 * sum|c||x| to spare; the reference's own
          error, (T + 2) * 2**-64 * (...), fits into that spare 2**9 times over.
          complex coefficients (csr, cfma): per component 2T fmas, then the final addition: 2T + 1 roundings at most, so
              |h.re - exact| <= (2T + 2) * u * (|h0.re| + sum(|c.re||x.re| + |c.im||x.im|)),
              |h.im - exact| <= (2T + 2) * u * (|h0.im| + sum(|c.re||x.im| + |c.im||x.re|)).
          h0 is part of the sum because the kernels ADD to hv: the last rounding is relative to h0 + acc.

THE EMULATIONS (`*_emulate`) walk the kernels' thread and block arithmetic (blockIdx, threadIdx, chunk, clamp, grid stride) in numpy on a
GRID, accumulate in double as the kernels do and go through the same refusing lookups.  `bug=` switches ONE named mistake on (MISTAKES);
the CPU test requires the clean emulation to pass `check` on every case and every mistake to be refused by some case."""
from dataclasses import dataclass
from itertools import combinations

import numpy as np

ND_INVALID = 0xFFFFFFFF
IDX = 0x7FFFFFFF
U = 2.0 ** -53
SENT = complex(-1.2345678, 0.87654321)
NAN = complex(float("nan"), float("nan"))
CHUNK = 1024          # rows per workgroup of hxv_nonlocal_tab
BLOCK = 256           # threads per workgroup of the two grid-stride kernels
KINDS = ("exact", "random")

# name -> (the kernels it can be made in, what it is)
MISTAKES = {
    "no_chunk_offset": (("tab",), "the chunk offset dropped from the row: i = threadIdx.x"),
    "cl_mod": (("tab",), "cl computed with % rchunks instead of / rchunks"),
    "clamped_writes": (("tab",), "a clamped thread (i >= dimup) writes"),
    "out_dimup": (("tab", "kernel", "csr"), "the output indexed with dimup instead of pitch"),
    "no_dw0": (("tab", "kernel"), "dw0 left out of the column lookup"),
    # (in the dw lookups: exchanged in all three lookups they only visit the orbital pairs in another order, which is no mistake)
    "q_r_swapped": (("tab",), "the q and r entries exchanged between the two dw words"),
    "jx_jp_swapped": (("tab", "kernel"), "Jx and Jp exchanged"),
    "sign_one_word": (("tab",), "the sign taken from the up word instead of the xor of the two"),
    "sign_in_index": (("tab",), "the sign bit left in the index"),
    "vcol_ignored": (("kernel", "csr"), "vcol ignored: the dw column used as the column slot"),
    "csr_zero_based": (("csr",), "the CSR column used 0-based"),
    "stride_blockdim": (("kernel", "csr"), "the grid stride taken as blockDim.x only"),
    "one_trip": (("kernel", "csr"), "the loop ended after its first trip"),
    "write_without_any": (("tab", "kernel", "csr"), "hv written when `any` is false (an empty row in the CSR form)"),
    "pad_row_read": (("csr",), "a pad row of v read: the CSR column split by the pitch instead of dimup"),
}


def roundup8(n):
    return (n + 7) & ~7


def bits(a):
    """the array as 64-bit patterns: -0.0 and +0.0 differ, NaN equals itself"""
    return np.ascontiguousarray(a).view(np.int64)


def look(a, idx, what, ok=None):
    """a[idx], refusing an index outside a; with `ok`, only the indices where ok holds are looked up (the others give a[0])"""
    idx = np.asarray(idx, dtype=np.int64)
    if ok is not None:
        idx = np.where(ok, idx, 0)
    if idx.size and (idx.min() < 0 or idx.max() >= a.shape[0]):
        raise IndexError(f"{what}: index {int(idx.min())}..{int(idx.max())} outside [0, {a.shape[0]})")
    return a[idx]


class Reads:
    """the indices into v a restatement asks for: refused outside [0, n), recorded otherwise"""

    def __init__(self, n):
        self.n = n
        self.mask = np.zeros(n, dtype=bool)

    def at(self, idx, ok, what):
        idx = np.where(ok, np.asarray(idx, dtype=np.int64), 0)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise IndexError(f"{what}: index {int(idx.min())}..{int(idx.max())} outside v[0, {self.n})")
        self.mask[idx[ok]] = True
        return idx


@dataclass
class Terms:
    """per local element e (hv index out[e]) and term slot k, in the kernel's order: valid[k, e], coef[k, e] (complex), vidx[k, e]; read:
    mask over v of the elements some term reads"""
    out: np.ndarray
    valid: np.ndarray
    coef: np.ndarray
    vidx: np.ndarray
    read: np.ndarray
    complex_coef: bool

    @property
    def written(self):
        return self.valid.any(axis=0)


def _terms(out, rows, reads, complex_coef):
    n = out.shape[0]
    if rows:
        valid, coef, vidx = (np.stack([r[k] for r in rows]) for k in range(3))
    else:
        valid, coef, vidx = np.zeros((0, n), dtype=bool), np.zeros((0, n), dtype=np.complex128), np.zeros((0, n), dtype=np.int64)
    return Terms(out, valid, coef.astype(np.complex128), vidx, reads.mask, complex_coef)


def h0_buffer(n):
    """what hv holds before a launch: n elements and the guard; every third element (-0.0, -0.0), the others SENT"""
    h = np.full(n + 1, SENT, dtype=np.complex128)
    h.real[::3] = -0.0
    h.imag[::3] = -0.0
    return h


def values(rng, n, kind):
    if kind == "exact":     # small NONZERO integers
        vals = np.array([v for v in range(-9, 10) if v], dtype=np.float64)
        return (rng.choice(vals, n) + 1j * rng.choice(vals, n)).astype(np.complex128)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128)


def pow2(rng, n=None):
    """signed powers of two between 1/4 and 4"""
    return rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-2, 3, n)


def inputs(case, terms, kind):
    """v: values of this kind where the contract reads, NaN everywhere else (pad rows, unused slots, unreached elements)"""
    rng = np.random.default_rng(case.seed + 31)
    v = values(rng, case.nv, kind)
    v[~terms.read] = NAN
    return v


def couplings(case, kind):
    """(jx, jp) of a tab or kernel case: which of the two are on is the case's, their values the kind's"""
    rng = np.random.default_rng(case.seed + 5)
    jx, jp = (pow2(rng), pow2(rng)) if kind == "exact" else rng.standard_normal(2)
    if kind == "exact" and abs(jx) == abs(jp):
        jp *= 2.0                       # (never the same magnitude: exchanging them must show)
    return (float(jx) if "x" in case.terms_on else 0.0), (float(jp) if "p" in case.terms_on else 0.0)


def expected(terms, v, h0, kind):
    """(want, bound): the whole hv buffer the contract promises, and for kind "random" the bound per component of every element (complex:
    .real bounds the real part, .imag the imaginary one; None for "exact", where `want` holds bit for bit)"""
    x = np.where(terms.valid, v[terms.vidx], 0.0)
    c = np.where(terms.valid, terms.coef, 0.0)
    wr = terms.written
    o = terms.out[wr]
    want = h0.copy()
    if kind == "exact":
        re = (c.real * x.real - c.imag * x.imag).sum(axis=0)      # every product and partial sum exact
        im = (c.real * x.imag + c.imag * x.real).sum(axis=0)
        want.real[o] = h0.real[o] + re[wr]
        want.imag[o] = h0.imag[o] + im[wr]
        return want, None
    L = np.longdouble
    assert np.finfo(L).nmant >= 63, "numpy.longdouble has no extended precision on this platform"
    cr, ci, xr, xi = c.real.astype(L), c.imag.astype(L), x.real.astype(L), x.imag.astype(L)
    re = h0.real[terms.out].astype(L) + (cr * xr - ci * xi).sum(axis=0)
    im = h0.imag[terms.out].astype(L) + (cr * xi + ci * xr).sum(axis=0)
    sre = np.abs(h0.real[terms.out]).astype(L) + (np.abs(cr * xr) + np.abs(ci * xi)).sum(axis=0)
    sim = np.abs(h0.imag[terms.out]).astype(L) + (np.abs(cr * xi) + np.abs(ci * xr)).sum(axis=0)
    t = terms.valid.sum(axis=0)
    roundings = (2 * t + 2 if terms.complex_coef else t + 2).astype(L)
    want = want.astype(np.clongdouble)
    bound = np.zeros(h0.shape[0], dtype=np.clongdouble)
    want.real[o], want.imag[o] = re[wr], im[wr]
    bound.real[o], bound.imag[o] = (roundings * L(U) * sre)[wr], (roundings * L(U) * sim)[wr]
    return want, bound


def check(terms, v, h0, got, kind):
    """the failures of buffer `got` against the contract, as strings; none: accepted"""
    if got.shape != h0.shape or got.dtype != np.complex128:
        return [f"shape or type: {got.shape} {got.dtype}"]
    want, bound = expected(terms, v, h0, kind)
    fails = []
    touched = np.zeros(h0.shape[0], dtype=bool)
    touched[terms.out[terms.written]] = True
    keep = np.flatnonzero(~touched & (bits(got).reshape(-1, 2) != bits(h0).reshape(-1, 2)).any(axis=1))
    if keep.size:
        k = int(keep[0])
        where = "the guard" if k == h0.shape[0] - 1 else f"element {k}"
        fails.append(f"{keep.size} elements the contract does not write changed, the first: {where}, {got[k]!r} for {h0[k]!r}")
    if kind == "exact":
        bad = np.flatnonzero(touched & (bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2)).any(axis=1))
    else:
        g = got.astype(np.clongdouble)
        inside = (np.abs(g.real - want.real) <= bound.real) & (np.abs(g.imag - want.imag) <= bound.imag)     # (a NaN is not inside)
        bad = np.flatnonzero(touched & ~inside)
    if bad.size:
        k = int(bad[0])
        fails.append(f"{bad.size} written elements wrong, the first: element {k}, {got[k]!r} for {complex(want[k])!r}" +
                     ("" if bound is None else f" (bound {complex(bound[k])!r})"))
    return fails


def _local(case):
    """(cl, i, out) of every local element t = cl*dimup + i"""
    cl = np.repeat(np.arange(case.qdw, dtype=np.int64), case.dimup)
    i = np.tile(np.arange(case.dimup, dtype=np.int64), case.qdw)
    return cl, i, cl * case.pitch + i


def _pairs(nlat, norb):
    return [(il, io, jo) for il in range(nlat) for io in range(norb) for jo in range(norb) if io != jo]


def _add(hv, o, acc, what):
    """hv[o] += acc, one thread after the other, refusing an element outside the buffer (the guard is inside it)"""
    o = np.asarray(o, dtype=np.int64)
    if o.size and (o.min() < 0 or o.max() >= hv.shape[0]):
        raise IndexError(f"{what}: write at {int(o.min())}..{int(o.max())} outside hv[0, {hv.shape[0]}) (guard included)")
    np.add.at(hv.real, o, acc.real)
    np.add.at(hv.imag, o, acc.imag)


# ---- hxv_nonlocal_tab ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Tab:
    name: str
    seed: int
    dimup: int
    dimdw: int
    pitch: int
    qdw: int
    dw0: int
    nlat: int
    norb: int
    terms_on: str            # "x", "p" or "xp"
    nslots: int              # column slots of v; the last one is named only by the never-read x == y entries
    rchunks: int
    nd_up: np.ndarray        # [Q*dimup] uint32
    nd_dw: np.ndarray        # [Q*dimdw] uint32
    dead_col: int            # local column all of whose dw moves are invalid, or -1

    @property
    def nv(self):
        return self.nslots * self.pitch

    @property
    def nhv(self):
        return self.qdw * self.pitch


def _tab_case(name, seed, dimup, qdw, nlat, norb, terms_on, wide_pitch=False, extra_chunk=False, dead_col=None):
    rng = np.random.default_rng(seed)
    dw0 = 2
    dimdw = dw0 + qdw + 2
    nslots = dimdw + 3
    Q = nlat * norb * norb
    if dead_col is None:
        dead_col = 1 if qdw > 1 else -1
    sign = lambda n: rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    nd_up = np.empty((Q, dimup), dtype=np.uint32)
    nd_dw = np.empty((Q, dimdw), dtype=np.uint32)
    dead_rows = rng.random(dimup) < 0.1                  # rows without any valid up move
    for q in range(Q):
        x, y = (q // norb) % norb, q % norb
        if x == y:      # never read: a valid-looking word that names the slot (and a row) nothing else names
            nd_up[q] = rng.permutation(dimup).astype(np.uint32)
            nd_dw[q] = np.uint32(nslots - 1)
            continue
        nd_up[q] = rng.permutation(dimup).astype(np.uint32) | sign(dimup)
        nd_up[q][(rng.random(dimup) < 0.25) | dead_rows] = ND_INVALID
        nd_dw[q] = rng.permutation(nslots - 1)[:dimdw].astype(np.uint32) | sign(dimdw)
        nd_dw[q][rng.random(dimdw) < 0.3] = ND_INVALID
        if dead_col >= 0:
            nd_dw[q][dw0 + dead_col] = ND_INVALID
    rchunks = -(-dimup // CHUNK) + (1 if extra_chunk else 0)
    pitch = roundup8(dimup) + (16 if wide_pitch else 0)
    return Tab(name, seed, dimup, dimdw, pitch, qdw, dw0, nlat, norb, terms_on, nslots, rchunks, nd_up.reshape(-1), nd_dw.reshape(-1), dead_col)


TAB_DIMUPS = (1, 63, 1023, 1024, 1025, 2048, 2049, 3000)


def tab_cases():
    out, n = [], 0
    for dimup in TAB_DIMUPS:
        for qdw in (1, 3):
            for nlat, norb in ((1, 2), (2, 2), (1, 3)):
                for on in ("x", "p", "xp"):
                    out.append(_tab_case(f"up{dimup}-q{qdw}-L{nlat}O{norb}-J{on}", 3000 + n, dimup, qdw, nlat, norb, on, wide_pitch=n % 4 == 1))
                    n += 1
    out.append(_tab_case("up1500-q1-the-only-column-dead", 3900, 1500, 1, 1, 2, "xp", dead_col=0))
    out.append(_tab_case("up1030-q2-one-chunk-more-than-needed", 3901, 1030, 2, 2, 2, "xp", wide_pitch=True, extra_chunk=True))
    return out


def tab_terms(c, jx, jp):
    cl, i, out = _local(c)
    col = cl + c.dw0
    reads, rows = Reads(c.nv), []
    for il, io, jo in _pairs(c.nlat, c.norb):
        q, r = (il * c.norb + io) * c.norb + jo, (il * c.norb + jo) * c.norb + io
        u = look(c.nd_up, r * c.dimup + i, "nd_up").astype(np.int64)
        for coupling, entry in ((jx, q), (jp, r)):
            if coupling == 0.0:
                continue
            d = look(c.nd_dw, entry * c.dimdw + col, "nd_dw").astype(np.int64)
            ok = (u != ND_INVALID) & (d != ND_INVALID)
            vidx = reads.at((d & IDX) * c.pitch + (u & IDX), ok, "v")
            if (((u & IDX) >= c.dimup) & ok).any():
                raise IndexError("nd_up names a pad row")
            rows.append((ok, np.where(((u ^ d) >> 31) & 1, -coupling, coupling), vidx))
    return _terms(out, rows, reads, False)


def tab_emulate(c, jx, jp, v, h0, bug=None):
    G = c.qdw * c.rchunks
    b = np.repeat(np.arange(G, dtype=np.int64), CHUNK)
    tid = np.tile(np.arange(CHUNK, dtype=np.int64), G)
    cl = b % c.rchunks if bug == "cl_mod" else b // c.rchunks
    i = tid if bug == "no_chunk_offset" else (b - cl * c.rchunks) * CHUNK + tid
    row_ok = i < c.dimup
    ir = np.minimum(i, c.dimup - 1)
    col = cl + (0 if bug == "no_dw0" else c.dw0)
    if bug == "jx_jp_swapped":
        jx, jp = jp, jx
    acc = np.zeros(b.shape[0], dtype=np.complex128)
    any_ = np.zeros(b.shape[0], dtype=bool)
    invalid = np.full(b.shape[0], ND_INVALID, dtype=np.int64)
    for il, io, jo in _pairs(c.nlat, c.norb):
        q, r = (il * c.norb + io) * c.norb + jo, (il * c.norb + jo) * c.norb + io
        qd, rd = (r, q) if bug == "q_r_swapped" else (q, r)
        dse = look(c.nd_dw, qd * c.dimdw + col, "nd_dw").astype(np.int64) if jx != 0.0 else invalid
        dph = look(c.nd_dw, rd * c.dimdw + col, "nd_dw").astype(np.int64) if jp != 0.0 else invalid
        live = ~((dse == ND_INVALID) & (dph == ND_INVALID))
        u = look(c.nd_up, r * c.dimup + ir, "nd_up", live).astype(np.int64)
        live &= u != ND_INVALID
        jup = u if bug == "sign_in_index" else u & IDX
        for d, coupling in ((dse, jx), (dph, jp)):
            ok = live & (d != ND_INVALID)
            slot = d if bug == "sign_in_index" else d & IDX
            x = look(v, slot * c.pitch + jup, "v", ok)
            sg = ((u if bug == "sign_one_word" else u ^ d) >> 31) & 1
            cf = np.where(sg, -coupling, coupling)
            acc.real += np.where(ok, cf * x.real, 0.0)
            acc.imag += np.where(ok, cf * x.imag, 0.0)
            any_ |= ok
    wr = any_ & row_ok
    if bug == "clamped_writes":
        wr = any_
    if bug == "write_without_any":
        wr = row_ok
    o = cl * (c.dimup if bug == "out_dimup" else c.pitch) + i
    hv = h0.copy()
    _add(hv, o[wr], acc[wr], "hv")
    return hv


# ---- the two grid-stride kernels ---------------------------------------------------------------------------------------------------------------
def trips(gx, nloc):
    """(number of trips the busiest thread takes, elements of the last trip, threads of the grid)"""
    per = gx * BLOCK
    n = -(-nloc // per)
    return n, nloc - (n - 1) * per, per


def _stride_loop(gx, nloc, bug):
    t0 = np.arange(gx * BLOCK, dtype=np.int64)
    stride = BLOCK if bug == "stride_blockdim" else gx * BLOCK
    trip = 0
    while True:
        t = t0 + trip * stride
        t = t[t < nloc]
        if t.size == 0:
            return
        yield t
        trip += 1
        if bug == "one_trip":
            return


def popc(x):
    return np.bitwise_count(np.asarray(x, dtype=np.uint64)).astype(np.int64)


def sector_map(ns, n):
    """the sorted configurations of n particles in ns orbitals"""
    return np.array(sorted(sum(1 << b for b in occ) for occ in combinations(range(ns), n)), dtype=np.uint32)


def slots(rng, dimdw, nslots):
    """a vcol that is not the identity: the dw columns scattered injectively over nslots column slots"""
    return rng.permutation(nslots)[:dimdw].astype(np.uint32)


# ---- hxv_nonlocal_kernel ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Search:
    name: str
    seed: int
    ns: int
    nup: int
    ndw: int
    nlat: int
    norb: int
    terms_on: str
    qdw: int
    dw0: int
    pitch: int
    nslots: int
    gx: int
    map_up: np.ndarray
    map_dw: np.ndarray
    vcol: np.ndarray

    @property
    def dimup(self):
        return self.map_up.shape[0]

    @property
    def dimdw(self):
        return self.map_dw.shape[0]

    @property
    def nv(self):
        return self.nslots * self.pitch

    @property
    def nhv(self):
        return self.qdw * self.pitch


def _search_case(name, seed, ns, nup, ndw, nlat, norb, on, qdw, dw0, gx, wide_pitch=False):
    rng = np.random.default_rng(seed)
    mu, md = sector_map(ns, nup), sector_map(ns, ndw)
    nslots = md.shape[0] + 3
    return Search(name, seed, ns, nup, ndw, nlat, norb, on, qdw, dw0, roundup8(mu.shape[0]) + (8 if wide_pitch else 0), nslots, gx, mu, md,
                  slots(rng, md.shape[0], nslots))


GRIDS = (8, 4, 3)      # on about 2000 local elements: one trip, two, three, each with a ragged last one


def search_cases():
    out = []
    for k, gx in enumerate(GRIDS):          # Ns = 8, 70 x 70, 29 local columns from column 20: 2030 local elements
        for j, on in enumerate(("x", "p", "xp")):
            out.append(_search_case(f"ns8-4+4-L2O2-J{on}-grid{gx}", 4000 + 10 * k + j, 8, 4, 4, 2, 2, on, 29, 20, gx, wide_pitch=j == 1))
    out.append(_search_case("ns8-3+5-L1O3-Jxp-grid3", 4100, 8, 3, 5, 1, 3, "xp", 36, 11, 3))             # 56 x 56, 2016 local elements
    out.append(_search_case("ns8-5+2-L2O3-Jxp-grid4", 4101, 8, 5, 2, 2, 3, "xp", 25, 3, 4, True))        # 56 x 28, 1400
    out.append(_search_case("ns6-3+3-L3O2-Jxp-grid1", 4102, 6, 3, 3, 3, 2, "xp", 13, 5, 1))              # 20 x 20, 260: two trips of one block
    out.append(_search_case("ns6-2+4-L1O3-Jx-grid1", 4103, 6, 2, 4, 1, 3, "x", 15, 0, 1))                # 15 x 15, whole: one ragged trip
    out.append(_search_case("ns5-2+3-L1O2-Jxp-grid2", 4104, 5, 2, 3, 1, 2, "xp", 4, 6, 2))               # 10 x 10, the last 4 columns
    out.append(_search_case("ns4-2+2-L2O2-Jxp-grid1", 4105, 4, 2, 2, 2, 2, "xp", 3, 2, 1))               # 6 x 6
    out.append(_search_case("ns4-1+3-L1O2-Jp-grid1", 4106, 4, 1, 3, 1, 2, "p", 2, 1, 1))                 # 4 x 4
    out.append(_search_case("ns4-0+2-L1O2-Jxp-grid1", 4107, 4, 0, 2, 1, 2, "xp", 3, 2, 1))               # 1 x 6: no up move exists, nothing is written
    return out


def _hop(m, a, b):
    """c^+_b c_a |m> for an array of configurations: (applies, target, sign bit); the sign of c / c^+ is the parity of the occupied
    orbitals below (ED_SETUP.f90:807-833)"""
    m = np.asarray(m, dtype=np.int64)
    ok = (((m >> a) & 1) == 1) & (((m >> b) & 1) == 0)
    m1 = m & ~(1 << a)
    sg = (popc(m & ((1 << a) - 1)) + popc(m1 & ((1 << b) - 1))) & 1
    return ok, m1 | (1 << b), sg


def _index_in(sorted_map, target, ok, what):
    """position of each target in the map, refusing one that is not there"""
    pos = np.searchsorted(sorted_map, np.where(ok, target, sorted_map[0]))
    if (ok & ((pos >= sorted_map.shape[0]) | (look(sorted_map, np.minimum(pos, sorted_map.shape[0] - 1), what) != target))).any():
        raise IndexError(f"{what}: a target configuration is not in the map")
    return pos


def search_terms(c, jx, jp):
    cl, i, out = _local(c)
    mu, md = look(c.map_up, i, "map_up"), look(c.map_dw, cl + c.dw0, "map_dw")
    reads, rows = Reads(c.nv), []
    for il, io, jo in _pairs(c.nlat, c.norb):
        a, b = il * c.norb + io, il * c.norb + jo                  # spin exchange: dw a -> b, up b -> a; pair hopping: both b -> a
        up_ok, up_to, up_sg = _hop(mu, b, a)
        for coupling, (dw_ok, dw_to, dw_sg) in ((jx, _hop(md, a, b)), (jp, _hop(md, b, a))):
            if coupling == 0.0:
                continue
            ok = up_ok & dw_ok
            jup, jdw = _index_in(c.map_up, up_to, ok, "map_up"), _index_in(c.map_dw, dw_to, ok, "map_dw")
            vidx = reads.at(look(c.vcol, jdw, "vcol", ok).astype(np.int64) * c.pitch + jup, ok, "v")
            rows.append((ok, np.where(up_sg ^ dw_sg, -coupling, coupling), vidx))
    return _terms(out, rows, reads, False)


def _par_below(m, pos):
    return popc(m & ((1 << pos) - 1)) & 1


def _rank_in_map(sorted_map, dim, value):
    """the kernel's binary search: the lower bound, never past dim - 1"""
    return np.minimum(np.searchsorted(sorted_map[:dim], value), dim - 1)


def search_emulate(c, jx, jp, v, h0, bug=None):
    if bug == "jx_jp_swapped":
        jx, jp = jp, jx
    hv = h0.copy()
    map_up, map_dw = c.map_up.astype(np.int64), c.map_dw.astype(np.int64)
    for t in _stride_loop(c.gx, c.qdw * c.dimup, bug):
        cl = t // c.dimup
        i = t - cl * c.dimup
        mu, md = look(map_up, i, "map_up"), look(map_dw, cl + (0 if bug == "no_dw0" else c.dw0), "map_dw")
        acc = np.zeros(t.shape[0], dtype=np.complex128)
        any_ = np.zeros(t.shape[0], dtype=bool)
        for il, io, jo in _pairs(c.nlat, c.norb):
            is_, js = io + il * c.norb, jo + il * c.norb
            nu_i, nu_j, nd_i, nd_j = ((mu >> is_) & 1) == 1, ((mu >> js) & 1) == 1, ((md >> is_) & 1) == 1, ((md >> js) & 1) == 1
            for coupling, ok, frm, to in ((jx, nu_j & nd_i & ~nd_j & ~nu_i, is_, js), (jp, nu_j & nd_j & ~nd_i & ~nu_i, js, is_)):
                if coupling == 0.0:
                    continue
                k1 = md & ~(1 << frm)
                k2 = k1 | (1 << to)
                k3 = mu & ~(1 << js)
                k4 = k3 | (1 << is_)
                sg = _par_below(md, frm) ^ _par_below(k1, to) ^ _par_below(mu, js) ^ _par_below(k3, is_)
                jdw, jup = _rank_in_map(map_dw, c.dimdw, k2), _rank_in_map(map_up, c.dimup, k4)
                slot = jdw if bug == "vcol_ignored" else look(c.vcol, jdw, "vcol", ok).astype(np.int64)
                x = look(v, slot * c.pitch + jup, "v", ok)
                cf = np.where(sg == 1, -coupling, coupling)
                acc.real += np.where(ok, cf * x.real, 0.0)
                acc.imag += np.where(ok, cf * x.imag, 0.0)
                any_ |= ok
        wr = np.ones_like(any_) if bug == "write_without_any" else any_
        o = cl * (c.dimup if bug == "out_dimup" else c.pitch) + i
        _add(hv, o[wr], acc[wr], "hv")
    return hv


# ---- hxv_nonlocal_csr ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Csr:
    name: str
    seed: int
    dimup: int
    dimdw: int
    pitch: int
    qdw: int
    dw0: int
    nslots: int
    gx: int
    vcol: np.ndarray
    rowptr: np.ndarray       # [qdw*dimup + 1] int64
    cols: np.ndarray         # int32, 1-based global
    vals: np.ndarray         # complex128; the EXACT kind's values (signed powers of two in both parts); "random" draws its own

    @property
    def nv(self):
        return self.nslots * self.pitch

    @property
    def nhv(self):
        return self.qdw * self.pitch


def _csr_case(name, seed, dimup, dimdw, qdw, dw0, gx, wide_pitch=False):
    rng = np.random.default_rng(seed)
    nloc = qdw * dimup
    count = rng.integers(0, 5, nloc)                      # 0 to 4 stored entries per row
    count[rng.integers(0, nloc)] = 0
    count[0] = 4 if dimup * dimdw >= 4 else dimup * dimdw
    count = np.minimum(count, dimup * dimdw)
    rowptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    cols = np.concatenate([rng.permutation(dimup * dimdw)[:k] for k in count] + [np.zeros(0, dtype=np.int64)]).astype(np.int32) + 1
    nnz = int(rowptr[-1])
    vals = np.empty(nnz, dtype=np.complex128)
    vals.real, vals.imag = pow2(rng, nnz), pow2(rng, nnz)
    nslots = dimdw + 3
    return Csr(name, seed, dimup, dimdw, roundup8(dimup) + (16 if wide_pitch else 0), qdw, dw0, nslots, gx, slots(rng, dimdw, nslots), rowptr, cols,
               vals)


def csr_cases():
    out = []
    for k, gx in enumerate(GRIDS):          # 67 x 40, 30 local columns from column 5: 2010 local rows
        out.append(_csr_case(f"up67-dw40-q30-grid{gx}", 5000 + k, 67, 40, 30, 5, gx, wide_pitch=k == 1))
    out.append(_csr_case("up1-dw9-q4-grid1", 5100, 1, 9, 4, 3, 1))
    out.append(_csr_case("up300-dw3-q1-grid1", 5101, 300, 3, 1, 2, 1, wide_pitch=True))           # two trips of one block
    out.append(_csr_case("up8-dw8-q8-grid2", 5102, 8, 8, 8, 0, 2))                                # the whole sector, grid past the end
    return out


def csr_values(c, kind):
    if kind == "exact":
        return c.vals
    rng = np.random.default_rng(c.seed + 9)
    return (rng.standard_normal(c.vals.shape[0]) + 1j * rng.standard_normal(c.vals.shape[0])).astype(np.complex128)


def csr_terms(c, vals):
    cl, i, out = _local(c)
    t = cl * c.dimup + i
    k0, k1 = look(c.rowptr, t, "rowptr"), look(c.rowptr, t + 1, "rowptr")
    reads, rows = Reads(c.nv), []
    for kk in range(int((k1 - k0).max()) if t.size else 0):
        ok = k0 + kk < k1
        j = look(c.cols, k0 + kk, "cols", ok).astype(np.int64) - 1
        jdw = j // c.dimup
        jup = j - jdw * c.dimup
        vidx = reads.at(look(c.vcol, jdw, "vcol", ok).astype(np.int64) * c.pitch + jup, ok, "v")
        rows.append((ok, look(vals, k0 + kk, "vals", ok), vidx))
    return _terms(out, rows, reads, True)


def csr_emulate(c, vals, v, h0, bug=None):
    hv = h0.copy()
    split = c.pitch if bug == "pad_row_read" else c.dimup
    for t in _stride_loop(c.gx, c.qdw * c.dimup, bug):
        k0, k1 = look(c.rowptr, t, "rowptr"), look(c.rowptr, t + 1, "rowptr")
        acc = np.zeros(t.shape[0], dtype=np.complex128)
        for kk in range(int((k1 - k0).max())):
            ok = k0 + kk < k1
            j = look(c.cols, k0 + kk, "cols", ok).astype(np.int64) - (0 if bug == "csr_zero_based" else 1)
            jdw = j // split
            jup = j - jdw * split
            slot = np.where(ok, jdw, 0) if bug == "vcol_ignored" else look(c.vcol, jdw, "vcol", ok).astype(np.int64)
            x = look(v, slot * c.pitch + jup, "v", ok)
            cf = look(vals, k0 + kk, "vals", ok)
            acc.real += np.where(ok, cf.real * x.real, 0.0)          # cfma, one component after the other
            acc.real += np.where(ok, -cf.imag * x.imag, 0.0)
            acc.imag += np.where(ok, cf.real * x.imag, 0.0)
            acc.imag += np.where(ok, cf.imag * x.real, 0.0)
        wr = np.ones(t.shape[0], dtype=bool) if bug == "write_without_any" else k0 != k1
        cl = t // c.dimup
        o = cl * (c.dimup if bug == "out_dimup" else c.pitch) + (t - cl * c.dimup)
        _add(hv, o[wr], acc[wr], "hv")
    return hv


# ---- one interface over the three ------------------------------------------------------------------------------------------------------------
def all_cases():
    return [("tab", c) for c in tab_cases()] + [("kernel", c) for c in search_cases()] + [("csr", c) for c in csr_cases()]


def coefficients(kernel, c, kind):
    """what the kind puts beside the case's tables: (jx, jp), or the CSR values"""
    return csr_values(c, kind) if kernel == "csr" else couplings(c, kind)


def terms_of(kernel, c, coef):
    if kernel == "csr":
        return csr_terms(c, coef)
    return (tab_terms if kernel == "tab" else search_terms)(c, *coef)


def emulate(kernel, c, coef, v, h0, bug=None):
    if kernel == "csr":
        return csr_emulate(c, coef, v, h0, bug)
    return (tab_emulate if kernel == "tab" else search_emulate)(c, *coef, v, h0, bug)
