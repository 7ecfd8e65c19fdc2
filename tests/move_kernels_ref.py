"""What the kernels that only MOVE amplitudes between layouts promise, restated in numpy, and the cases they are run on one by one
(tests/test_gpu_move_kernels.py on the device, tests/test_move_kernels_ref_cpu.py without one).

One function per kernel states the contract of its head comment element by element: which element of which buffer ends up where, times
which sign.  None walks the kernel's thread loops.  Every index goes through `take` / `put`, which refuse an index outside the array, so
running a case's restatement is also the proof that its tables stay inside the buffers `*_inputs` allocates -- the very buffers the GPU
file uploads.  What the LAUNCH adds to that (which elements a grid covers, how many trips its loops take) is computed by `*_trips` from
the case and the kernel's geometry alone.

Buffers a kernel writes start as SENT everywhere (one guard element behind them included); a restatement returns the whole buffer, so one
comparison of bits says that every promised element holds its value and that nothing else was touched.  Buffers a kernel reads hold NaN
wherever the contract says "never read".

`bug=` switches ONE named mistake on (the list is MISTAKES); the CPU test requires every one of them to change some case's bits."""
from dataclasses import dataclass, field
from itertools import combinations

import numpy as np

SENT = complex(-12345.678, 8765.4321)
NAN = complex(float("nan"), float("nan"))
TW, TW_THREADS = 32, 256


def roundup8(n):
    return (n + 7) & ~7


def bits(a):
    """the array as 64-bit patterns: -0.0 and +0.0 differ, NaN equals itself"""
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _idx(a, idx, what):
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= a.shape[0]):
        raise IndexError(f"{what}: index {int(idx.min())}..{int(idx.max())} outside [0, {a.shape[0]})")
    return idx


def take(a, idx, what):
    return a[_idx(a, idx, what)]


def put(a, idx, val, what):
    a[_idx(a, idx, what)] = val


def neg(x, s):
    """x where s is 0, (-re, -im) where it is not: what the kernels do with a basis sign"""
    return np.where(np.asarray(s) != 0, -x, x)


def cplx(re, im):
    """the complex array of these parts, their bits kept (re + 1j * im would turn a -0.0 into +0.0)"""
    out = np.empty(np.broadcast(re, im).shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def data(rng, n, integer=False):
    if integer:     # small NONZERO integers: every product and sum is exact whether or not the compiler fuses them, and no product is a signed zero
        vals = np.array([v for v in range(-9, 10) if v], dtype=np.float64)
        return (rng.choice(vals, n) + 1j * rng.choice(vals, n)).astype(np.complex128)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128)


def fresh(n):
    """a buffer the kernel writes: n elements and the guard, all SENT"""
    return np.full(n + 1, SENT, dtype=np.complex128)


def with_guard(a, guard=NAN):
    return np.concatenate([a, np.array([guard], dtype=a.dtype)])


@dataclass
class RowOrder:
    """perm: reference row -> device row; iperm: device row -> reference row; sign: by device row (1 = minus)"""
    perm: np.ndarray
    iperm: np.ndarray
    sign: np.ndarray


def row_order(rng, n):
    iperm = rng.permutation(n).astype(np.int32)
    perm = np.empty(n, dtype=np.int32)
    perm[iperm] = np.arange(n, dtype=np.int32)
    return RowOrder(perm, iperm, rng.integers(0, 2, n).astype(np.uint8))


def _ip(order, n, bug=None):
    if order is None:
        return np.arange(n, dtype=np.int64)
    return (order.perm if bug == "perm_for_iperm" else order.iperm).astype(np.int64)


def _sg(order, n, dropped=False):
    if order is None or dropped:
        return np.zeros(n, dtype=np.uint8)
    return order.sign


# ---- twin_transpose_kernel -------------------------------------------------------------------------------------------------------------------
@dataclass
class Transpose:
    name: str
    dimup_a: int
    dimup_b: int
    pitch_a: int
    pitch_b: int
    oa: object
    ob: object
    gx: int
    gy: int


def transpose_cases():
    dims = [1, 7, 8, 31, 32, 33, 65, 100]
    pairs = [(d, d) for d in dims] + [(1, 100), (100, 1), (7, 33), (33, 8), (31, 65), (65, 32), (32, 100), (8, 31), (100, 7)]
    out = []
    for n, (da, db) in enumerate(pairs):
        for which in ("none", "a", "b", "both"):
            rng = np.random.default_rng(1000 + 10 * n + len(which))
            oa = row_order(rng, da) if which in ("a", "both") else None
            ob = row_order(rng, db) if which in ("b", "both") else None
            pa, pb = roundup8(da), roundup8(db)
            out.append(Transpose(f"{da}x{db}-{which}", da, db, pa, pb, oa, ob, -(-da // TW), -(-pb // TW)))
    rng = np.random.default_rng(1999)
    out.append(Transpose("33x65-both-wide-pitches", 33, 65, 48, 88, row_order(rng, 33), row_order(rng, 65), 2, 3))
    out.append(Transpose("31x9-both-grid-past-the-end", 31, 9, 32, 16, row_order(rng, 31), row_order(rng, 9), 3, 2))
    return out


def transpose_inputs(c, seed=0):
    rng = np.random.default_rng(seed + 7)
    a = data(rng, c.dimup_b * c.pitch_a).reshape(c.dimup_b, c.pitch_a)
    a[:, c.dimup_a:] = NAN                      # pad rows of d_a are never read
    return with_guard(a.reshape(-1))


def transpose_ref(c, d_a, bug=None):
    """d_b[kB*pitch_b + rB] = sB[rB] * sA[rA] * d_a[kA*pitch_a + rA], kB = iperm_A[rA], kA = iperm_B[rB]; pad rows of every column +0.0"""
    out = fresh(c.dimup_a * c.pitch_b)
    ra, rb = np.arange(c.dimup_a)[:, None], np.arange(c.dimup_b)[None, :]
    kb, ka = _ip(c.oa, c.dimup_a, bug)[:, None], _ip(c.ob, c.dimup_b, bug)[None, :]
    s = _sg(c.oa, c.dimup_a, bug == "sign_a_dropped")[:, None] ^ _sg(c.ob, c.dimup_b, bug == "sign_b_dropped")[None, :]
    put(out[:-1], kb * c.pitch_b + rb, neg(take(d_a[:-1], ka * c.pitch_a + ra, "d_a"), s), "d_b")
    if bug != "transpose_pad_unwritten":
        pad = np.arange(c.dimup_a)[:, None] * c.pitch_b + np.arange(c.dimup_b, c.pitch_b)[None, :]
        put(out[:-1], pad, complex(-0.0, -0.0) if bug == "transpose_pad_negzero" else 0.0, "d_b pad rows")
    return out


def transpose_trips(c):
    """no loop: the grid must cover A's rows along x and B's rows UP TO THE PITCH along y"""
    return {"covers": c.gx * TW >= c.dimup_a and c.gy * TW >= c.pitch_b}


# ---- twin_pack_kernel ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Pack:
    name: str
    dimup_a: int
    qa: int
    pitch_a: int
    stride: int
    own_lo: int
    own_hi: int
    oa: object
    gx: int
    gy: int


def pack_cases():
    out = []
    n = 0
    for da in (1, 31, 33, 70):
        owns = {"empty-low": (0, 0), "whole": (0, da), "middle": (da // 3, max(da // 3, 2 * da // 3)), "to-tile-edge": (0, min(da, TW)),
                "from-tile-edge": (min(da, TW), da)}
        for qa in (1, 31, 32, 33, 70):
            full = -(-qa // TW)
            for gy in sorted({1, min(2, full), full}):
                kind = list(owns)[n % len(owns)]
                rng = np.random.default_rng(2000 + n)
                oa = None if n % 7 == 3 else row_order(rng, da)
                stride = roundup8(qa) + (16 if n % 5 == 2 else 0)
                out.append(Pack(f"{da}x{qa}-own-{kind}-gy{gy}", da, qa, roundup8(da) + (8 if n % 4 == 1 else 0), stride, *owns[kind], oa,
                                -(-da // TW), gy))
                n += 1
    return out


def pack_inputs(c, seed=0):
    rng = np.random.default_rng(seed + 11)
    a = data(rng, c.qa * c.pitch_a).reshape(c.qa, c.pitch_a)
    a[:, c.dimup_a:] = NAN                      # pad rows of d_a are never read
    return with_guard(a.reshape(-1))


def pack_ref(c, d_a, bug=None):
    """the element of reference row iup = iperm_A[rA] and local column col, times sA[rA], goes to own[(iup - own_lo)*stride + col] when
    own_lo <= iup < own_hi and to send[iup*stride + col] otherwise; stride pads and the own block's rows of send are not written"""
    send, own = fresh(c.dimup_a * c.stride), fresh((c.own_hi - c.own_lo) * c.stride + (c.stride if bug == "pack_own_hi_inclusive" else 0))
    ra, col = np.arange(c.dimup_a)[:, None], np.arange(c.qa)[None, :]
    iup = _ip(c.oa, c.dimup_a, bug)[:, None]
    val = neg(take(d_a[:-1], col * c.pitch_a + ra, "d_a"), _sg(c.oa, c.dimup_a, bug == "sign_a_dropped")[:, None])
    mine = (iup >= c.own_lo) & ((iup <= c.own_hi) if bug == "pack_own_hi_inclusive" else (iup < c.own_hi))
    mine = np.broadcast_to(mine, val.shape)
    put(own[:-1], ((iup - c.own_lo) * c.stride + col)[mine], val[mine], "own")
    to_send = np.ones_like(mine) if bug == "pack_own_also_sent" else ~mine
    put(send[:-1], (iup * c.stride + col)[to_send], val[to_send], "send")
    if bug == "pack_pad_written" and c.stride > c.qa:
        put(send[:-1], np.arange(c.dimup_a) * c.stride + c.qa, 0.0, "send")
    if bug == "pack_own_hi_inclusive":      # (the extra row the mistake writes lies behind the real buffer: shown as a changed guard)
        extra = own[(c.own_hi - c.own_lo) * c.stride:-1]
        own = own[:(c.own_hi - c.own_lo) * c.stride + 1].copy()
        if not same_bits(extra, np.full_like(extra, SENT)):
            own[-1] = 0.0
    return send, own


def pack_trips(c):
    """x: no loop, the grid must cover A's rows; y: blocks loop over the tiles of local columns"""
    tiles = -(-c.qa // TW)
    return {"covers": c.gx * TW >= c.dimup_a, "c0_trips": -(-tiles // c.gy), "ragged": c.qa % TW != 0}


# ---- twin_unpack_kernel ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Unpack:
    name: str
    nranks: int
    first: np.ndarray          # [P+1] first column of A per rank (A's columns = B's reference rows)
    off: np.ndarray            # [P+1] element offset of each rank's block in recv (the last: the end)
    stride: np.ndarray         # [P]
    dimup_b: int
    pitch_b: int
    qb: int
    ob: object
    gx: int
    gy: int

    def tab(self):
        return np.concatenate([self.first, self.off, self.stride]).astype(np.int64)


def uneven_split(rng, n, p):
    """[p+1] firsts of p ranks over n columns, unevenly, single-column ranks where n allows; ranks without a column only when n < p"""
    if n <= p:
        q = np.zeros(p, dtype=np.int64)
        q[p - n:] = 1                            # (the empty ranks in front: firsts repeat at the low end)
    else:
        q = np.ones(p, dtype=np.int64)
        extra = n - p
        heavy = rng.permutation(p)[: max(1, p // 2)]
        share = rng.multinomial(extra, np.ones(len(heavy)) / len(heavy))
        q[heavy] += share
    return np.concatenate([[0], np.cumsum(q)]).astype(np.int64)


def unpack_cases():
    out = []
    n = 0
    for db in (1, 9, 255, 256, 257, 300):
        for p in (2, 3, 4, 8):
            qb = (1, 5)[n % 2] if db != 300 else 5
            for gy in sorted({1, min(2, qb), qb}):
                rng = np.random.default_rng(3000 + n)
                first = uneven_split(rng, db, p)
                q = np.diff(first)
                stride = np.array([roundup8(max(int(x), 1)) + 8 * (r % 3) for r, x in enumerate(q)], dtype=np.int64)
                off = np.concatenate([[0], np.cumsum(qb * stride + 8)]).astype(np.int64)        # (8 elements nobody reads between blocks)
                ob = None if n % 6 == 4 else row_order(rng, db)
                pb = roundup8(db) + (8 if n % 5 == 1 else 0)
                out.append(Unpack(f"{db}-P{p}-qb{qb}-gy{gy}", p, first, off, stride, db, pb, qb, ob, -(-pb // TW_THREADS), gy))
                n += 1
    return out


def unpack_inputs(c, seed=0):
    rng = np.random.default_rng(seed + 13)
    recv = np.full(int(c.off[-1]), NAN, dtype=np.complex128)
    for o in range(c.nranks):
        q = int(c.first[o + 1] - c.first[o])
        blk = np.full((c.qb, int(c.stride[o])), NAN, dtype=np.complex128)      # stride pads are never read
        blk[:, :q] = data(rng, c.qb * q).reshape(c.qb, q)
        recv[int(c.off[o]):int(c.off[o]) + blk.size] = blk.reshape(-1)
    return with_guard(recv)


def owner_of(first, idw, bug=None):
    """the rank o with first[o] <= idw < first[o+1]"""
    o = np.zeros_like(idw)
    for p in range(1, len(first) - 1):
        o += (idw > first[p]) if bug == "unpack_owner_gt" else (idw >= first[p])
    return o


def unpack_ref(c, recv, bug=None):
    """d_b[kB*pitch_b + rB] = sB[rB] * recv[off[o] + kB*S(o) + idw - first[o]], idw = iperm_B[rB], o the owner of column idw of A;
    rows DimUp_B <= rB < pitch_b are +0.0"""
    out = fresh(c.qb * c.pitch_b)
    rb, kb = np.arange(c.dimup_b)[None, :], np.arange(c.qb)[:, None]
    idw = _ip(c.ob, c.dimup_b, bug)[None, :]
    o = owner_of(c.first, idw, bug)
    st = take(c.stride, np.zeros_like(o) if bug == "unpack_wrong_block_stride" else o, "stride")
    src = take(c.off, o, "off") + kb * st + idw - take(c.first, o, "first")
    put(out[:-1], kb * c.pitch_b + rb, neg(take(recv[:-1], src, "recv"), _sg(c.ob, c.dimup_b, bug == "sign_b_dropped")[None, :]), "d_b")
    if c.pitch_b > c.dimup_b:
        pad = kb * c.pitch_b + np.arange(c.dimup_b, c.pitch_b)[None, :]
        put(out[:-1], pad, take(recv[:-1], int(c.off[0]) + kb * int(c.stride[0]), "recv") if bug == "unpack_pad_copied" else 0.0, "d_b pad rows")
    return out


def unpack_trips(c):
    """x: one thread per device row of B up to the pitch, no loop; y: blocks loop over the local columns"""
    return {"covers": c.gx * TW_THREADS >= c.pitch_b, "kb_trips": -(-c.qb // c.gy), "ragged": c.qb % c.gy != 0,
            "past_pitch": c.gx * TW_THREADS > c.pitch_b}


# ---- ladder_kernel ---------------------------------------------------------------------------------------------------------------------------
def basis(ns, k):
    """all states of k particles on ns orbitals, ascending: the reference's sector map"""
    return np.array(sorted(sum(1 << b for b in s) for s in combinations(range(ns), k)), dtype=np.uint32)


@dataclass
class Ladder:
    name: str
    ns: int
    orbital: int
    spin: int
    create: int
    map_from: np.ndarray       # sorted reference map of the source sector
    map_to: np.ndarray         # spin 0: by device row of the target; spin 1: the local target columns
    dimup_to: int
    dimdw_to: int
    pitch_from: int
    pitch_to: int
    ofrom: object              # spin 0 only: the source sector's row order, or None
    sign_to: object            # spin 0 only: the target's basis signs by device row, or None
    gx: int
    psi_cols: int = field(default=0)

    @property
    def dim_from(self):
        return len(self.map_from)

    @property
    def n(self):
        return self.dimup_to * self.dimdw_to


def ladder_cases():
    out = []
    n = 0
    for ns, k in ((4, 2), (6, 3), (9, 4)):
        for create in (1, 0):
            mf, mt = basis(ns, k - 1 if create else k + 1), basis(ns, k)
            for orbital in (0, ns // 2, ns - 1):
                for spin in (0, 1):
                    for variant in (0, 1):
                        rng = np.random.default_rng(4000 + n)
                        if spin == 0:
                            dimup_to, dimdw_to = len(mt), (len(mt) if (ns, variant) == (4, 0) else 7)
                            pf, pt = roundup8(len(mf)) + 8 * variant, roundup8(dimup_to) + 16
                            if variant:
                                ofrom, oto = row_order(rng, len(mf)), row_order(rng, dimup_to)
                                map_to, sign_to = mt[oto.iperm], oto.sign
                            else:
                                ofrom, map_to, sign_to = None, mt, None
                            psi_cols = dimdw_to
                        else:
                            dimup_to = (5, 11, 19)[n % 3]
                            lo = 1 + variant if len(mt) > 3 else 0                  # the target is a slab: map_to is offset ...
                            map_to = mt[lo:len(mt) - 1 - variant]                   # ... and has fewer columns than DimDw
                            dimdw_to, ofrom, sign_to = len(map_to), None, None
                            pf, pt = roundup8(dimup_to) + 8, roundup8(dimup_to)
                            psi_cols = len(mf)
                        full = -(-dimup_to * dimdw_to // 256)
                        gx = (1, 2, 3, full)[n % 4]
                        out.append(Ladder(f"ns{ns}k{k}-{'cdg' if create else 'c'}{orbital}-spin{spin}-v{variant}-gx{gx}", ns, orbital, spin, create, mf,
                                          map_to, dimup_to, dimdw_to, pf, pt, ofrom, sign_to, gx, psi_cols))
                        n += 1
    return out


LADDER_MODES = {"copy": (1.0 + 0.0j, 0, False), "integer": (2.0 - 3.0j, 1, True), "integer-fresh": (-1.0 + 2.0j, 0, True)}


def ladder_inputs(c, integer, seed=0):
    rng = np.random.default_rng(seed + 17)
    rows = c.dim_from if c.spin == 0 else c.dimup_to
    psi = data(rng, c.psi_cols * c.pitch_from, integer).reshape(c.psi_cols, c.pitch_from)
    psi[:, rows:] = NAN                                                             # pad rows of the source are never read
    out0 = fresh(c.dimdw_to * c.pitch_to)
    o = out0[:-1].reshape(c.dimdw_to, c.pitch_to)
    o[:, :c.dimup_to] = data(rng, c.n, integer).reshape(c.dimdw_to, c.dimup_to)     # what `accumulate` adds to; pad rows keep SENT
    return with_guard(psi.reshape(-1)), out0


def popcount(x):
    return np.array([bin(int(v)).count("1") for v in np.asarray(x).ravel()], dtype=np.int64).reshape(np.shape(x))


def ladder_terms(c, bug=None):
    """for every target element (column col, row i): is it reached, with which sign (0 / 1 = minus), from which element of psi"""
    col, i = np.arange(c.dimdw_to)[:, None], np.arange(c.dimup_to)[None, :]
    swapped = bug == "ladder_roles_swapped"
    which = (i if c.spin == 0 else col) if not swapped else (col if c.spin == 0 else i)
    which = np.broadcast_to(which, (c.dimdw_to, c.dimup_to))
    m_to = take(c.map_to, which, "map_to").astype(np.int64)
    bit = 1 << c.orbital
    want = (c.create != 0) != (bug == "ladder_create_inverted")
    reached = ((m_to & bit) != 0) == want
    m_from = m_to ^ bit
    j = np.searchsorted(c.map_from, m_from.astype(np.uint32))
    if bug != "ladder_create_inverted":
        assert (take(c.map_from, j[reached], "map_from") == m_from[reached]).all(), "the source state is not in the source map"
    j = np.minimum(j, c.dim_from - 1)                       # (a state that is not there: where the kernel's search ends)
    below = bit - 1 if bug != "ladder_parity_counts_orbital" else 2 * bit - 1
    sg = popcount((m_to if bug == "ladder_parity_of_target" else m_from) & below) & 1
    if c.spin == 0:
        if c.ofrom is not None:
            j = take(c.ofrom.perm, j, "perm_from").astype(np.int64)
            sg = sg ^ take(c.ofrom.sign, j, "sign_from")
        if c.sign_to is not None:
            sg = sg ^ take(c.sign_to, np.broadcast_to(i, sg.shape), "sign_to")
    src = (col * c.pitch_from + j) if (c.spin == 0) != swapped else (j * c.pitch_from + i)
    return reached, sg, src


def ladder_ref(c, psi, out0, coef, accumulate, bug=None):
    """out[col*pitch_to + i] = (accumulate ? out : +0.0) + coef * sign * psi[source], or without the second term where the orbital of the
    target state is not in the state the operator leaves; rows >= dimup_to of out are not touched.  Products and sums in float64, each
    rounded: exact (and the device's bits) when coef is 1 or all numbers are small integers."""
    reached, sg, src = ladder_terms(c, bug)
    if bug == "ladder_coef_conjugated":
        coef = np.conj(coef)
    if bug == "ladder_accumulate_ignored":
        accumulate = 0
    x = take(psi[:-1], np.where(reached, src, 0), "psi")
    s = np.where(sg != 0, -1.0, 1.0)
    re = np.where(reached, s * (coef.real * x.real - coef.imag * x.imag), 0.0)
    im = np.where(reached, s * (coef.real * x.imag + coef.imag * x.real), 0.0)
    out = out0.copy()
    dst = np.arange(c.dimdw_to)[:, None] * c.pitch_to + np.arange(c.dimup_to)[None, :]
    if accumulate:
        o = take(out0[:-1], dst, "out")
        re, im = re + o.real, im + o.imag
    put(out[:-1], dst, cplx(re, im), "out")
    return out


def ladder_ref_long(c, psi, out0, coef, accumulate):
    """the same in long double, with what the error bound of the GPU test needs: (re, im, mag_re, mag_im) over [dimdw_to, dimup_to],
    mag_re = |c.x||x.x| + |c.y||x.y|, mag_im = |c.x||x.y| + |c.y||x.x| (zero where the target is not reached)"""
    L = np.longdouble
    reached, sg, src = ladder_terms(c)
    x = take(psi[:-1], np.where(reached, src, 0), "psi")
    s = np.where(sg != 0, L(-1), L(1))
    cx, cy, xx, xy = L(coef.real), L(coef.imag), x.real.astype(L), x.imag.astype(L)
    re = np.where(reached, s * (cx * xx - cy * xy), L(0))
    im = np.where(reached, s * (cx * xy + cy * xx), L(0))
    mre = np.where(reached, abs(cx) * abs(xx) + abs(cy) * abs(xy), L(0))
    mim = np.where(reached, abs(cx) * abs(xy) + abs(cy) * abs(xx), L(0))
    if accumulate:
        dst = np.arange(c.dimdw_to)[:, None] * c.pitch_to + np.arange(c.dimup_to)[None, :]
        o = take(out0[:-1], dst, "out")
        re, im = re + o.real.astype(L), im + o.imag.astype(L)
    return re, im, mre, mim


def stride_trips(n, gx, block=256):
    """a grid-stride loop of gx blocks over n elements: rounds of the busiest thread, and whether the last round is ragged"""
    per = gx * block
    return {"rounds": -(-n // per), "ragged": n % per != 0}


def ladder_trips(c):
    return stride_trips(c.n, c.gx)


# ---- ladder_cols_kernel ----------------------------------------------------------------------------------------------------------------------
@dataclass
class LadderCols:
    name: str
    dimup: int
    pitch_from: int
    pitch_to: int
    slot: np.ndarray
    sign: np.ndarray
    nlocal: int
    nrecv: int
    accumulate: int
    coef: complex
    integer: bool
    gx: int

    @property
    def ncols(self):
        return len(self.slot)


def ladder_cols_cases():
    out = []
    slot = np.array([2, -2, 0, 0, -3, 1, -1], dtype=np.int32)       # local 2, received 1, (unreached), local 0, received 2, (unreached), received 0
    sign = np.array([1, -1, 0, -1, 1, 0, 1], dtype=np.int32)
    n = 0
    for dimup in (1, 255, 256, 257, 600):
        for accumulate in (0, 1):
            for integer in (False, True):
                coef = (2.0 - 3.0j) if integer else (1.0 + 0.0j)
                out.append(LadderCols(f"{dimup}-acc{accumulate}-{'int' if integer else 'copy'}", dimup, roundup8(dimup) + 8, roundup8(dimup) + (16 if n % 2 else 0),
                                      slot, sign, 3, 3, accumulate, coef, integer, 7 if n % 3 else 9))
                n += 1
    return out


def ladder_cols_inputs(c, seed=0):
    rng = np.random.default_rng(seed + 19)

    def cols(k):
        a = data(rng, k * c.pitch_from, c.integer).reshape(k, c.pitch_from)
        a[:, c.dimup:] = NAN                                                        # pad rows of both sources are never read
        return with_guard(a.reshape(-1))

    out0 = fresh(c.ncols * c.pitch_to)
    o = out0[:-1].reshape(c.ncols, c.pitch_to)
    o[:, :c.dimup] = data(rng, c.ncols * c.dimup, c.integer).reshape(c.ncols, c.dimup)
    return cols(c.nlocal), cols(c.nrecv), out0


def ladder_cols_ref(c, psi_local, recv, out0, bug=None):
    """out[col][i] = (accumulate ? out[col][i] : +0.0) + coef * sign[col] * src_col[i] for i < dimup; src_col = column slot[col] of psi_local
    (slot >= 0) or column -1-slot[col] of recv (slot < 0), nothing where sign[col] == 0; pad rows are not touched"""
    out = out0.copy()
    rows = np.arange(c.pitch_to if bug == "ladder_cols_pad_written" else c.dimup)
    for col in range(c.ncols):
        sg, sl = int(c.sign[col]), int(c.slot[col])
        dst = col * c.pitch_to + rows
        re = im = np.zeros(len(rows))
        if sg != 0:
            if sl >= 0:
                x = take(psi_local[:-1], sl * c.pitch_from + np.minimum(rows, c.dimup - 1), "psi_local")
            else:
                k = -1 - sl if bug != "ladder_cols_recv_off_by_one" else min(-sl, c.nrecv - 1)     # (clipped to stay in the buffer)
                x = take(recv[:-1], k * c.pitch_from + np.minimum(rows, c.dimup - 1), "recv")
            re = sg * (c.coef.real * x.real - c.coef.imag * x.imag)
            im = sg * (c.coef.real * x.imag + c.coef.imag * x.real)
        elif bug == "ladder_cols_unreached_unwritten":
            continue
        if c.accumulate:
            o = take(out0[:-1], dst, "out")
            re, im = re + o.real, im + o.imag
        put(out[:-1], dst, cplx(re, im), "out")
    return out


def ladder_cols_trips(c):
    """one workgroup per column (blocks past ncols return); its 256 threads loop over the rows"""
    local = ((c.sign != 0) & (c.slot >= 0)).any()
    received = ((c.sign != 0) & (c.slot < 0)).any()
    return {"covers": c.gx >= c.ncols, "rounds": -(-c.dimup // 256), "ragged": c.dimup % 256 != 0, "local": bool(local), "received": bool(received),
            "unreached": bool((c.sign == 0).any())}


# ---- pack_columns_kernel ---------------------------------------------------------------------------------------------------------------------
@dataclass
class PackColumns:
    name: str
    pitch: int
    nsrc: int
    cols: np.ndarray


def pack_columns_cases():
    return [PackColumns(f"pitch{p}", p, 5, np.array([3, 0, 3, 4, 1], dtype=np.int32)) for p in (8, 256, 264, 1000)]


def pack_columns_inputs(c, seed=0):
    return with_guard(data(np.random.default_rng(seed + 23), c.nsrc * c.pitch))      # whole columns travel, pad rows included


def pack_columns_ref(c, src, bug=None):
    """out[b*pitch + i] = in[cols[b]*pitch + i] for every listed column b and all i < pitch"""
    out = fresh(len(c.cols) * c.pitch)
    b, i = np.arange(len(c.cols))[:, None], np.arange(c.pitch)[None, :]
    put(out[:-1], b * c.pitch + i, take(src[:-1], take(c.cols, b, "cols").astype(np.int64) * c.pitch + i, "in"), "out")
    return out


def pack_columns_trips(c):
    return {"rounds": -(-c.pitch // 256), "ragged": c.pitch % 256 != 0}


# ---- add_pieces_kernel -----------------------------------------------------------------------------------------------------------------------
@dataclass
class AddPieces:
    name: str
    real: bool
    dimup: int
    pitch: int
    ncols: int
    row0: np.ndarray
    row1: np.ndarray
    stride: np.ndarray
    gx: int
    gy: int = field(default=0)          # blocks along y; they loop over the columns.  0: one per column

    def __post_init__(self):
        self.gy = self.gy or self.ncols

    @property
    def nwtr(self):
        return len(self.row0)


def add_pieces_cases():
    out = []
    n = 0
    for dimup in (1, 257, 700):
        full = -(-dimup // 256)
        for nwtr in (1, 2, 4, 8):
            for real in (False, True):
                rng = np.random.default_rng(5000 + n)
                live = nwtr - 1 if nwtr > 2 else nwtr                   # one EMPTY range, in the middle of the list, where there are more than two
                if dimup >= live:
                    cuts = np.sort(rng.choice(np.arange(1, dimup), live - 1, replace=False)) if live > 1 else np.zeros(0, dtype=np.int64)
                    edges = np.concatenate([[0], cuts, [dimup]]).astype(np.int64)
                else:                                                   # (fewer rows than ranges: the rest are empty too)
                    edges = np.concatenate([[0], np.full(live, dimup)]).astype(np.int64)
                if live < nwtr:
                    edges = np.insert(edges, nwtr // 2, edges[nwtr // 2])
                row0, row1 = edges[:-1].astype(np.int32), edges[1:].astype(np.int32)
                ln = (row1 - row0).astype(np.int64)
                stride = ln + 1 + (np.arange(nwtr)[::-1] if n % 2 else np.arange(nwtr))      # every range its own stride, a pad behind every column
                gx = sorted({1, min(2, full), full})[n % len({1, min(2, full), full})]
                out.append(AddPieces(f"{dimup}-nwtr{nwtr}-{'real' if real else 'complex'}-gx{gx}", real, dimup, roundup8(dimup) + (8 if n % 3 == 0 else 0), 3,
                                     row0, row1, stride, gx))
                n += 1
    # fewer blocks along y than columns: the column loop's second and third trips, ragged
    for real in (False, True):
        for ncols, gy in ((5, 2), (7, 1)):
            out.append(AddPieces(f"257-nwtr2-{'real' if real else 'complex'}-cols{ncols}-gy{gy}", real, 257, 264, ncols, np.array([0, 100], dtype=np.int32),
                                 np.array([100, 257], dtype=np.int32), np.array([101, 160], dtype=np.int64), 2, gy))
    # more one-row columns than a grid holds along y (65535): what a rank of a skinny sector keeps (DimUp small, DimDw above 2 * 65535)
    out.append(AddPieces("1-nwtr1-complex-cols70001-gy65535", False, 1, 8, 70001, np.array([0], dtype=np.int32), np.array([1], dtype=np.int32),
                         np.array([2], dtype=np.int64), 1, 65535))
    return out


def add_pieces_inputs(c, seed=0):
    """-> hv [ncols*pitch + guard] (pad rows SENT), pieces: one buffer [ncols*stride + guard] per range (stride pads NaN); float64 when real"""
    rng = np.random.default_rng(seed + 29)
    dt = np.float64 if c.real else np.complex128
    sent, nan = (SENT.real, float("nan")) if c.real else (SENT, NAN)

    def rnd(k):
        return rng.standard_normal(k) if c.real else data(rng, k)

    hv = np.full(c.ncols * c.pitch + 1, sent, dtype=dt)
    hv[:-1].reshape(c.ncols, c.pitch)[:, :c.dimup] = rnd(c.ncols * c.dimup).reshape(c.ncols, c.dimup)
    pieces = []
    for k in range(c.nwtr):
        ln, st = int(c.row1[k] - c.row0[k]), int(c.stride[k])
        p = np.full((c.ncols, st), nan, dtype=dt)
        p[:, :ln] = rnd(c.ncols * ln).reshape(c.ncols, ln)
        pieces.append(np.concatenate([p.reshape(-1), np.array([nan], dtype=dt)]))
    return hv, pieces


def add_pieces_ref(c, hv0, pieces, bug=None):
    """hv[col*pitch + row] += piece_k[col*stride_k + row - row0_k] for every row < dimup, k the range with row0_k <= row < row1_k; one IEEE
    add per component; pad rows are not touched"""
    hv = hv0.copy()
    ncols = min(c.ncols, c.gy) if bug == "add_pieces_no_column_loop" else c.ncols     # (the mistake: one column per block of the grid, no loop)
    for row in range(c.dimup):
        if bug == "add_pieces_range_gt":
            k = 0
            while k + 1 < c.nwtr and row > c.row1[k]:
                k += 1
        else:
            k = [q for q in range(c.nwtr) if c.row0[q] <= row < c.row1[q]]
            assert len(k) == 1, "the ranges do not tile the rows"
            k = k[0]
        st = int(c.stride[0 if bug == "add_pieces_stride0_for_all" else k])
        col = np.arange(ncols)
        dst = col * c.pitch + row
        put(hv[:-1], dst, take(hv0[:-1], dst, "hv") + take(pieces[k][:-1], col * st + row - int(c.row0[k]), "piece"), "hv")
    return hv


def add_pieces_trips(c):
    t = stride_trips(c.dimup, c.gx)
    t["empty_in_the_middle"] = any(c.row0[k] == c.row1[k] for k in range(1, c.nwtr - 1))
    t["col_trips"], t["col_ragged"] = -(-c.ncols // c.gy), c.ncols % c.gy != 0
    return t


# ---- rows_ref_to_dev, rows_dev_to_ref --------------------------------------------------------------------------------------------------------
@dataclass
class Rows:
    name: str
    dimup: int
    pitch: int
    ncols: int
    order: RowOrder
    gx: int


def rows_cases():
    out = []
    n = 0
    for dimup in (1, 7, 8, 9, 255, 257):
        for ncols in (1, 3):
            for gx in (1, 2, 3):
                rng = np.random.default_rng(6000 + n)
                out.append(Rows(f"{dimup}x{ncols}-gx{gx}", dimup, roundup8(dimup) + (8 if n % 4 == 2 else 0), ncols, row_order(rng, dimup), gx))
                n += 1
    return out


def rows_inputs(c, seed=0):
    """-> ref [ncols*dimup + guard] contiguous, dev [ncols*pitch + guard] with NaN pad rows"""
    rng = np.random.default_rng(seed + 31)
    dev = data(rng, c.ncols * c.pitch).reshape(c.ncols, c.pitch)
    dev[:, c.dimup:] = NAN                                                          # pad rows are never read on the way out
    return with_guard(data(rng, c.ncols * c.dimup)), with_guard(dev.reshape(-1))


def rows_ref_to_dev_ref(c, ref, bug=None):
    """dst[col*pitch + d] = sign[d] * src[col*dimup + iperm[d]] for d < dimup, +0.0 for dimup <= d < pitch"""
    out = fresh(c.ncols * c.pitch)
    col, d = np.arange(c.ncols)[:, None], np.arange(c.dimup)[None, :]
    r = _ip(c.order, c.dimup, bug)[None, :]
    s = take(c.order.sign, r if bug == "rows_sign_by_reference_row" else d, "sign")
    put(out[:-1], col * c.pitch + d, neg(take(ref[:-1], col * c.dimup + r, "src"), s), "dst")
    if c.pitch > c.dimup:
        put(out[:-1], col * c.pitch + np.arange(c.dimup, c.pitch)[None, :], 0.0, "dst pad rows")
    return out


def rows_dev_to_ref_ref(c, dev, bug=None):
    """dst[col*dimup + i] = sign[perm[i]] * src[col*pitch + perm[i]] for i < dimup"""
    out = fresh(c.ncols * c.dimup)
    col, i = np.arange(c.ncols)[:, None], np.arange(c.dimup)[None, :]
    d = (c.order.iperm if bug == "perm_for_iperm" else c.order.perm).astype(np.int64)[None, :]
    s = take(c.order.sign, i if bug == "rows_sign_by_reference_row" else d, "sign")
    put(out[:-1], col * c.dimup + i, neg(take(dev[:-1], col * c.pitch + d, "src"), s), "dst")
    return out


def rows_trips(c, to_dev):
    return stride_trips((c.pitch if to_dev else c.dimup) * c.ncols, c.gx)


# ---- the chain without a communicator --------------------------------------------------------------------------------------------------------
def dw_split(dim, p):
    """[p+1] firsts of the reference's split of `dim` columns over p ranks (ED_HAMILTONIAN.f90:93-105)"""
    q, rem = divmod(dim, p)
    return np.array([r * q + min(r, rem) for r in range(p)] + [dim], dtype=np.int64)


CHAIN_SHAPES = [(37, 45, 2), (37, 45, 3), (37, 45, 8), (64, 9, 2), (64, 9, 3), (64, 9, 8)]      # DimUp_A, DimDw_A, P


# every named mistake, with the restatement it is a variant of
MISTAKES = {
    "sign_a_dropped": "transpose", "sign_b_dropped": "transpose", "perm_for_iperm": "transpose", "transpose_pad_unwritten": "transpose",
    "transpose_pad_negzero": "transpose",
    "pack_own_hi_inclusive": "pack", "pack_pad_written": "pack", "pack_own_also_sent": "pack",
    "unpack_owner_gt": "unpack", "unpack_wrong_block_stride": "unpack", "unpack_pad_copied": "unpack",
    "ladder_parity_counts_orbital": "ladder", "ladder_create_inverted": "ladder", "ladder_accumulate_ignored": "ladder",
    "ladder_coef_conjugated": "ladder", "ladder_roles_swapped": "ladder",
    "ladder_cols_pad_written": "ladder_cols", "ladder_cols_unreached_unwritten": "ladder_cols", "ladder_cols_recv_off_by_one": "ladder_cols",
    "add_pieces_range_gt": "add_pieces", "add_pieces_stride0_for_all": "add_pieces", "add_pieces_no_column_loop": "add_pieces",
    "rows_sign_by_reference_row": "rows",
}
# "parity taken of the target instead of the source" is no mistake: the two states differ in the operator's own orbital only, and par_below
# counts strictly below it.  The CPU test shows that the variant gives the same bits on every case, so that nobody looks for a check of it.
IDENTITIES = {"ladder_parity_of_target": "ladder"}
