"""A restatement of the pass-A job kernel hxv_up_job (csrc/hxv_job_kernels.hpp) in numpy, and the cases it is run on alone.

A case starts from TRIPLETS (row, source row, signed-coefficient index) per block and a signed-coefficient table.  From them
`build_tables` makes the kernel's tables exactly as DevTiles documents them (start, tstart, gstart / gmax, ell_in with EMPTY words, bh_ptr /
bh, rs_ptr / rs_off / rs_tab / rs_base / rs_neg with shared tables, order, scoef whose last entry is 0), `geometry` restates
job_up_geometry / job_up_fits of csrc/hxv_tile_plan.cpp, and `walk` restates what every workgroup of the launch does with the tables:
chunk cut, loader (ring stage of every tile, group buffer of every scratch group, the counted wait), clamps, re-packed table words, kin per
wave, the four slots that are always gathered, diagonal, one-tile-late store, epilogue and per-workgroup partials.  Every index `walk`
forms goes through a checked lookup into the very buffers the GPU file uploads, every LDS byte offset is held against the launch's LDS
size: a case that walks is safe to launch.  `walk(..., bug=NAME)` makes one named mistake (BUGS).

The EXPECTED result does not come from the tables but from the triplets and a plain sum in np.longdouble (`expected`):

    hv[c][r] = s*((a_up[r] + a_dw[dw0+c] + cross)*v[slab0+c][r] + wt(c,r) + sum coef*v[slab0+c][src]) - c_m*xm[c][r]

Values.  "exact*": every input is a small integer times a signed power of two, chosen so that every sum -- the partials included -- is a
multiple of a quantum q with sum|terms|/q < 2**53: exact in float64 in ANY order, fused or not (`exact_headroom`, asserted by the CPU test);
the device must give these bits.  A zero sum is +0 (the accumulator starts from +0 or from a scratch value, no input is -0), and the two
epilogue steps are applied to it in the kernel's order, so that the sign of a zero result is the kernel's as well.

"random*": normal values.  BOUND, derived here before any device run.  u = 2**-53, gamma(k) = k*u/(1 - k*u).  Per component of an
element the kernel makes: the diagonal d (at most KD = 8 roundings: the sums au + adw + cross, the products and sums of diag_cross), one
fused multiply-add per real product -- 1 for the diagonal, 1 per hop with real H, 2 per hop with complex H (Re: c.x*x.x - c.y*x.y, Im:
c.x*x.y + c.y*x.x) -- starting from the scratch value, one multiplication by s, one fused multiply-add with xm.  With T hops and F = T
(real H) or 2T (complex H) products the standard bound for a sum of F + 1 products accumulated in any order, scaled and updated, is

    |hv - exact| <= gamma(F + 3 + KD) * ( |s| * ( D|x| + |wt| + sum_hops A ) + |c_m||xm| ),       D = |a_up| + |a_dw| + sum|U|n + |Ust||n|

component by component, with A = |c||x| for real H and, for complex H, A_re = |c.x||x.x| + |c.y||x.y|, A_im = |c.x||x.y| + |c.y||x.x|
(the complex-product factor).  The slots the kernel always gathers with a zero coefficient add exact zeros.  A workgroup's partial sum is
sum_t s*(x.x*w.x + x.y*w.y) over its rows and tiles: each term has 3 roundings (two products, one of them fused, and the fused
multiply-add by s), a thread chains ntile of them, the wave reduction adds 6 levels and the sum over the waves 15 more, so

    |partial - exact| <= sum |s||x| * (bound of w)  +  gamma(ntile + 3 + 6 + 15) * sum |s| (|x.x||w.x| + |x.y||w.y|)

(the paired epilogue: each component alone, its own s).  The longdouble reference's own error is 2**-11 of these and is ignored."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

SHIFT = 20                     # TILE_COEF_SHIFT
OFFM = (1 << SHIFT) - 1
JOB_WAVES, JOB_LOADER, JOB_MAX_STAGES, JOB_KIN, JOB_KO = 16, 15, 8, 24, 8
HOP_CHUNK = 8
LDS_BUDGET = 160 * 1024
KD = 8
U = 2.0 ** -53
NAN = complex(np.nan, np.nan)
SENT = complex(-1234.5, 4321.25)   # hv before the launch; the guard behind it
KINDS = ["exact", "exactc", "random", "randomc"]
I_S, I_C, I_S2, I_C2, NSCAL = 1, 3, 0, 4, 6   # places of s, c, s2, c2 in the scalar array

BUGS = ["stage_prev", "group_not_alternated", "chunk_round", "xm_slab0", "v_no_slab0", "diag_no_dw0", "tstart_ignored", "rs_neg_ignored",
        "rs_base_ignored", "bh_no_row", "kin_round_down", "drop_last_store", "store_current_column", "idle_partial_unwritten", "lz2_swapped",
        "cm_with_xm_null", "pad_lanes_sum", "wc0_blocked"]


class OutOfBounds(Exception):
    pass


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    sizes: list                 # rows of each block
    kin: list                   # per block: longest in-block list, or a list of one bound per 64-row group
    outer: list                 # per block: (row slots, block hops)
    qdw: int
    dw0: int = 0
    dimdw: int = 0              # 0: dw0 + qdw
    slab0: int = 0
    vslots: int = 0             # 0: slab0 + qdw
    pad: int = 0                # pitch = dimup rounded up to 8, plus 8 * pad
    wc: int = 4
    lz: int = 0
    xm: bool = True             # with lz: a previous Lanczos vector
    wt: bool = True
    job_groups: int = 100
    job_stages: int = 4
    norb: int = 1
    ncoef: int = 3
    share: dict = field(default_factory=dict)   # block -> earlier block of the same size whose in-block tables (and row-slot tables) it shares
    seed: int = 1

    @property
    def dimup(self):
        return int(sum(self.sizes))

    @property
    def pitch(self):
        return (self.dimup + 7) // 8 * 8 + 8 * self.pad

    @property
    def ndw(self):
        return self.dimdw or self.dw0 + self.qdw

    @property
    def nslots(self):
        return self.vslots or self.slab0 + self.qdw

    @property
    def nblocks(self):
        return len(self.sizes)

    @property
    def max_block(self):
        return max(self.sizes)

    def real_kinds(self):
        return [k for k in KINDS if not (self.lz == 2 and k.endswith("c"))]


def all_cases():
    C = Case
    return [
        # the small block sizes, unequal chunk cuts, idle workgroups, shared tables, every slot kind
        C("edge-sizes-lz1", [65, 64, 63, 1, 64, 65, 1], [9, 4, [0], 1, 4, 9, 0], [(2, 0), (0, 1), (1, 0), (0, 1), (0, 1), (2, 0), (0, 0)], qdw=37, dw0=5,
          dimdw=50, slab0=40, vslots=80, pad=1, wc=4, lz=1, job_groups=2, job_stages=4, share={5: 0, 4: 1}),
        C("edge-sizes-lz0-nowt", [65, 64, 63, 1, 64, 65, 1], [9, 4, [0], 1, 4, 9, 0], [(2, 0), (0, 1), (1, 0), (0, 1), (0, 1), (2, 0), (0, 0)], qdw=37,
          dw0=3, dimdw=41, slab0=2, vslots=40, wc=4, lz=0, wt=False, job_groups=2, job_stages=3, share={5: 0, 4: 1}),
        C("edge-sizes-lz2", [65, 64, 63, 1, 64, 65, 1], [9, 4, [0], 1, 4, 9, 0], [(2, 0), (0, 1), (1, 0), (0, 1), (0, 1), (2, 0), (0, 0)], qdw=37, dw0=5,
          dimdw=50, slab0=40, vslots=80, wc=2, lz=2, job_groups=2, job_stages=2, share={5: 0, 4: 1}),
        # few columns: XCDs without a group, one tile per job, jobs shorter than the ring
        C("q3-idle-lz0", [200, 130], [[7, 12, 3, 0], [5, 0, 2]], [(3, 0), (4, 0)], qdw=3, dw0=1, dimdw=9, slab0=4, vslots=9, wc=2, lz=0, job_stages=8),
        C("q3-idle-lz1-noxm", [200, 130], [[7, 12, 3, 0], [5, 0, 2]], [(3, 0), (4, 0)], qdw=3, dw0=1, dimdw=9, slab0=4, vslots=9, wc=0, lz=1, xm=False,
          job_stages=8, pad=2),
        C("q3-idle-lz2", [200, 130], [[7, 12, 3, 0], [5, 0, 2]], [(3, 0), (4, 0)], qdw=3, dw0=1, dimdw=9, slab0=4, vslots=9, wc=16, lz=2, job_stages=4),
        C("q17-short-jobs", [200, 200, 70], [16, 16, 6], [(4, 4), (4, 4), (0, 0)], qdw=17, dw0=2, dimdw=21, slab0=17, vslots=51, wc=8, lz=1,
          job_stages=8, share={1: 0}),
        # mid-size blocks, long jobs, every scratch layout, jobs that start mid-group and on an odd group
        C("mid-wc2-long", [330, 200, 330], [13, 8, 13], [(1, 1), (3, 0), (1, 1)], qdw=150, dw0=7, dimdw=160, slab0=150, vslots=300, wc=2, lz=1,
          job_groups=7, job_stages=3, share={2: 0}),
        C("mid-wc4-natural-rows", [330, 200, 330], [13, 8, 13], [(1, 1), (3, 0), (1, 1)], qdw=75, dw0=0, dimdw=80, slab0=5, vslots=85, wc=4, lz=0,
          job_groups=3, job_stages=2, share={2: 0}),
        C("mid-wc8-odd", [330, 200], [13, 8], [(2, 0), (3, 0)], qdw=99, dw0=1, dimdw=100, slab0=1, vslots=101, wc=8, lz=2, job_groups=5, job_stages=4),
        C("mid-wc16", [130, 100], [13, 8], [(2, 0), (3, 0)], qdw=99, dw0=1, dimdw=100, slab0=1, vslots=101, wc=16, lz=1, xm=False, job_groups=100,
          job_stages=8),
        C("mid-wc0-natural", [330, 200], [13, 8], [(2, 0), (3, 0)], qdw=99, dw0=1, dimdw=100, slab0=1, vslots=101, wc=0, lz=1, job_groups=4, job_stages=4,
          pad=3),
        C("mid-norb2-kin24", [200, 200, 100], [23, 23, 21], [(5, 3), (5, 3), (1, 0)], qdw=41, dw0=9, dimdw=64, slab0=3, vslots=50, wc=4, lz=1, norb=2,
          job_groups=2, share={1: 0}, ncoef=5),
        C("mid-norb2-kin24-lz0", [200, 200, 100], [23, 23, 21], [(5, 3), (5, 3), (1, 0)], qdw=41, dw0=9, dimdw=64, slab0=3, vslots=50, wc=2, lz=0, norb=2,
          job_groups=3, share={1: 0}, ncoef=5),
        # full blocks: all 15 compute waves, a partly live last wave, the saturated wait, the ring clamped by the LDS budget
        C("full-960-lz0-st8", [960, 924, 960], [20, 17, 20], [(4, 4), (6, 0), (4, 4)], qdw=70, dw0=11, dimdw=90, slab0=70, vslots=140, wc=0, lz=0,
          job_groups=100, job_stages=8, share={2: 0}, pad=1),
        C("full-960-lz1-clamped", [960, 897, 960], [24, 17, 24], [(4, 4), (6, 0), (4, 4)], qdw=40, dw0=11, dimdw=60, slab0=40, vslots=80, wc=2, lz=1,
          job_groups=100, job_stages=8, share={2: 0}),
        C("full-960-lz2-st2", [960, 897], [12, 17], [(8, 0), (6, 0)], qdw=30, dw0=0, dimdw=30, slab0=0, vslots=30, wc=2, lz=2, job_groups=2, job_stages=2),
    ]


# ---- tables from triplets ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Tables:
    start: np.ndarray
    tstart: np.ndarray
    gstart: np.ndarray
    gmax: np.ndarray
    ell_in: np.ndarray
    bh_ptr: np.ndarray
    bh: np.ndarray
    rs_ptr: np.ndarray
    rs_off: np.ndarray
    rs_tab: np.ndarray
    rs_base: np.ndarray
    rs_neg: np.ndarray
    order: np.ndarray
    k_in: int
    k_in_real: int
    max_outer: int
    map_up: np.ndarray
    map_dw: np.ndarray
    trip: np.ndarray            # [ntrip][3] (row, source row, signed-coefficient index): what the tables MEAN


def build_tables(c: Case) -> Tables:
    """The triplets of the case (a seeded draw) and the tables that say the same.  In-block: row p of block b has cnt[p] hops to rows of
    its own block, in slots 0 .. cnt-1 of ell_in (word = index << 20 | source offset in the block; every other slot EMPTY = (2*ncoef) << 20).
    A block in `share` has its in-block triplets copied from the earlier block: its words live at the earlier block's rows only (tstart), its
    own rows of ell_in and its own groups of gmax hold DECOY words that a kernel ignoring tstart would add.  Out-of-block: block hops (the
    same-sized partner block, identity on the rows, one signed coefficient) and row slots (one word per row: index << 20 | source row,
    absolute with rs_base 0, or -- a table two blocks share -- relative to the partner block's start given as rs_base, the second user with
    rs_neg = 1 and the opposite sign in its triplets)."""
    rng = np.random.default_rng(1000 + c.seed)
    nb, nsc = c.nblocks, 2 * c.ncoef + 1
    EMPTY = np.uint32((nsc - 1) << SHIFT)
    start = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.uint32)
    dimup = c.dimup
    trip = []
    # in-block lists
    lists = {}
    for b in range(nb):
        n = c.sizes[b]
        if b in c.share:
            a = c.share[b]
            assert a < b and c.sizes[a] == n and a not in c.share
            lists[b] = lists[a]
            continue
        ng = (n + 63) // 64
        bound = c.kin[b] if isinstance(c.kin[b], list) else [c.kin[b]] * ng
        bound = (bound + [bound[-1]] * ng)[:ng]
        cnt = np.zeros(n, dtype=np.int64)
        for g in range(ng):
            lo, hi = g * 64, min(n, g * 64 + 64)
            cnt[lo:hi] = rng.integers(0, bound[g] + 1, hi - lo)
            cnt[rng.integers(lo, hi)] = bound[g]
        lists[b] = [(rng.integers(0, n, cnt[p]), rng.integers(0, nsc - 1, cnt[p])) for p in range(n)]
    k_in_real = max(len(l[0]) for b in range(nb) for l in lists[b])
    k_in = max(HOP_CHUNK, (k_in_real + HOP_CHUNK - 1) // HOP_CHUNK * HOP_CHUNK)
    ell = np.full((k_in, dimup), EMPTY, dtype=np.uint32)
    tstart = start[:-1].copy()
    gstart = np.zeros(nb + 1, dtype=np.uint32)
    gmax = []
    for b in range(nb):
        n, r0 = c.sizes[b], int(start[b])
        gstart[b] = len(gmax)
        for p in range(n):
            src, sc = lists[b][p]
            for k in range(len(src)):
                trip.append((r0 + p, r0 + int(src[k]), int(sc[k])))
        if b in c.share:
            ell[:, r0:r0 + n] = np.uint32(0 << SHIFT)          # decoy: +coefficient 0 times the block's first row, in every slot
            gmax += [k_in | (5 << 16)] * ((n + 63) // 64)      # decoy bounds (the high half is pass B's: never read here)
            tstart[b] = start[c.share[b]]
            continue
        for p in range(n):
            src, sc = lists[b][p]
            ell[:len(src), r0 + p] = (sc.astype(np.uint32) << SHIFT) | src.astype(np.uint32)
        for g in range(0, n, 64):
            gmax.append(max(len(lists[b][p][0]) for p in range(g, min(n, g + 64))) | (3 << 16))
    for b in c.share:
        gstart[b] = gstart[c.share[b]]
    gstart[nb] = len(gmax)
    # out-of-block
    bh_ptr, bh, rs_ptr, rs_off, rs_base, rs_neg, rs_tab = [0], [], [0], [], [], [], []
    owner_tabs = {}   # (block, slot) -> (offset, source block)
    for b in range(nb):
        n, r0 = c.sizes[b], int(start[b])
        nrs, nbh = c.outer[b]
        for i in range(nrs):
            a = c.share.get(b)
            sb = (b + 1 + i) % nb
            if a is not None and (a, i) in owner_tabs:   # a block of the owner's partner's size, another one where there is one
                so = owner_tabs[(a, i)][1]
                sb = ([x for x in range(nb) if c.sizes[x] == c.sizes[so] and x != so] + [so])[0]
            if a is not None and (a, i) in owner_tabs:
                off, neg = owner_tabs[(a, i)][0], i & 1 ^ 1      # the earlier block's table, every other slot with the opposite sign
                words = np.array(rs_tab[off:off + n], dtype=np.uint32)
                base = int(start[sb])
            else:
                relative = b in c.share.values() and sb != 0      # an owner's table is relative to its partner block (base > 0)
                ns_b = c.sizes[sb]
                has = rng.random(n) < 0.8
                src = rng.integers(0, ns_b, n)
                sc = rng.integers(0, nsc - 1, n)
                base = int(start[sb]) if relative else 0
                words = np.where(has, (sc.astype(np.uint32) << SHIFT) | (src + (0 if relative else int(start[sb]))).astype(np.uint32), EMPTY).astype(np.uint32)
                off, neg = len(rs_tab), 0
                rs_tab += [int(w) for w in words]
                owner_tabs[(b, i)] = (off, sb)
            rs_off.append(off)
            rs_base.append(base)
            rs_neg.append(neg)
            for p in range(n):
                w = int(words[p])
                if w != int(EMPTY):
                    trip.append((r0 + p, (w & OFFM) + base, (w >> SHIFT) ^ neg))
        rs_ptr.append(len(rs_off))
        same = [x for x in range(nb) if x != b and c.sizes[x] == n]
        for i in range(nbh):
            sb = same[i % len(same)]
            sc = int(rng.integers(0, nsc - 1))
            bh += [int(start[sb]), sc]
            for p in range(n):
                trip.append((r0 + p, int(start[sb]) + p, sc))
        bh_ptr.append(len(bh) // 2)
    u32 = lambda x: np.array(x if len(x) else [0], dtype=np.uint32)  # (an empty table still needs an address)
    order = np.array(sorted(range(nb), key=lambda b: -c.sizes[b]), dtype=np.uint32)
    nbits = 2 * c.norb
    return Tables(start, tstart, gstart, u32(gmax), ell.reshape(-1), np.array(bh_ptr, dtype=np.uint32), u32(bh), np.array(rs_ptr, dtype=np.uint32),
                  u32(rs_off), u32(rs_tab), u32(rs_base), u32(rs_neg), order, k_in, k_in_real,
                  max(nrs + nbh for nrs, nbh in c.outer), rng.integers(0, 1 << nbits, dimup).astype(np.uint32),
                  rng.integers(0, 1 << nbits, c.ndw).astype(np.uint32), np.array(trip, dtype=np.int64).reshape(-1, 3))


# ---- geometry (job_up_geometry, job_up_fits) -----------------------------------------------------------------------------------------------
def geometry(qdw, max_block, nblocks, ncoef, k_in, k_in_real, job_groups, job_stages, wc, lz):
    g = {}
    g["ngroups"] = qdw                                   # one column per tile
    g["gpx"] = (qdw + 7) // 8
    g["chunks"] = max(1, (g["gpx"] + job_groups // 2) // job_groups)
    g["ns"] = (max_block + 63) // 64 * 64
    g["stage_bytes"] = (2 if lz else 1) * g["ns"] * 16
    g["wt_bytes"] = g["ns"] * max(wc, 1) * 16
    g["tab"] = ((2 * ncoef + 1) * 16 + 255) // 256 * 256 + 256
    room = LDS_BUDGET - g["tab"] - 2 * g["wt_bytes"]
    g["nst"] = min(job_stages, JOB_MAX_STAGES, -(-room // g["stage_bytes"]) if room < 0 else room // g["stage_bytes"])  # (C++ division truncates)
    g["lds_bytes"] = g["nst"] * g["stage_bytes"] + 2 * g["wt_bytes"] + g["tab"]
    g["kin_rows"] = min(k_in, (k_in_real + 3) // 4 * 4)
    g["nwg"] = 8 * g["chunks"] * nblocks
    g["fits"] = g["nst"] >= 2
    return g


def case_geometry(c: Case, t: Tables, job_stages=None, job_groups=None, lz=None):
    return geometry(c.qdw, c.max_block, c.nblocks, c.ncoef, t.k_in, t.k_in_real, job_groups or c.job_groups, job_stages or c.job_stages, c.wc,
                    c.lz if lz is None else lz)


# ---- values -----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Values:
    scoef: np.ndarray       # [2*ncoef+1] complex, last 0
    a_up: np.ndarray
    a_dw: np.ndarray
    uloc: np.ndarray        # [5]
    ust: float
    orbmask: np.ndarray     # [5]
    sitemask: np.ndarray    # [16]
    nlat: int
    v: np.ndarray           # [nslots*pitch] complex, NaN where pass A reads nothing
    wt: np.ndarray | None   # blocked [groups][dimup][wc] or natural [qdw][pitch]
    xm: np.ndarray | None   # [qdw*pitch]
    scal: np.ndarray        # [NSCAL]
    real_h: int


def _dyadic(rng, size, top, frac):
    """integers in [-top, top] times 2**-frac"""
    return rng.integers(-top, top + 1, size).astype(np.float64) * 2.0 ** -frac


def values(c: Case, t: Tables, kind: str, lz=None, xm_on=None) -> Values:
    """exact: v multiples of 1/4 up to 4, scratch multiples of 1/16, coefficients, diagonal terms and scalars multiples of 1/2."""
    rng = np.random.default_rng(77 + c.seed + 13 * KINDS.index(kind))
    exact, cplx = kind.startswith("exact"), kind.endswith("c")
    lz = c.lz if lz is None else lz
    dimup, pitch = c.dimup, c.pitch

    def draw(size, top, frac, nonzero=False):
        if exact:
            x = _dyadic(rng, size, top, frac)
            if nonzero:
                x = np.where(x == 0.0, 2.0 ** -frac, x)
            return x + 0.0
        return rng.standard_normal(size)

    def cdraw(size, top, frac):
        return cpx(draw(size, top, frac), draw(size, top, frac))

    coef = draw(c.ncoef, 6, 1, nonzero=True) + (1j * draw(c.ncoef, 6, 1, nonzero=True) if cplx else 0.0)
    scoef = np.zeros(2 * c.ncoef + 1, dtype=np.complex128)
    scoef[0:-1:2], scoef[1:-1:2] = coef, -coef
    scoef = scoef + 0.0
    uloc, orbmask, sitemask = np.zeros(5), np.zeros(5, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    uloc[:c.norb] = draw(c.norb, 6, 1, nonzero=True)
    nlat = 1 if c.norb == 1 else 2
    if c.norb == 1:
        orbmask[0] = 0b11
    else:                     # two sites of two orbitals: orbital o of site l is bit l*2 + o
        orbmask[:2] = [0b0101, 0b1010]
        sitemask[:2] = [0b0011, 0b1100]
    ust = float(draw(1, 6, 1, nonzero=True)[0]) if c.norb > 1 else 0.0
    v = np.full((c.nslots, pitch), NAN, dtype=np.complex128)
    v[c.slab0:c.slab0 + c.qdw, :dimup] = cdraw((c.qdw, dimup), 16, 2)
    wt = None
    if c.wt:
        if c.wc:
            ng = (c.qdw + c.wc - 1) // c.wc
            wt = np.full((ng * c.wc, dimup), NAN, dtype=np.complex128)     # [column][row] first
            wt[:c.qdw] = cdraw((c.qdw, dimup), 64, 4)
            wt = np.ascontiguousarray(wt.reshape(ng, c.wc, dimup).transpose(0, 2, 1))  # wt[group][row][wc]
        else:
            wt = np.full((c.qdw, pitch), NAN, dtype=np.complex128)
            wt[:, :dimup] = cdraw((c.qdw, dimup), 64, 4)
        wt = wt.reshape(-1)
    xm = None
    if lz and (c.xm if xm_on is None else xm_on):
        xm = np.full((c.qdw, pitch), NAN, dtype=np.complex128)
        xm[:, :dimup] = cdraw((c.qdw, dimup), 16, 2)
        xm = xm.reshape(-1)
    scal = np.full(NSCAL, np.nan)
    scal[[I_S, I_C, I_S2, I_C2]] = draw(4, 6, 1, nonzero=True)
    return Values(scoef, draw(dimup, 8, 1), draw(c.ndw, 8, 1), uloc, ust, orbmask, sitemask, nlat, v.reshape(-1), wt, xm, scal, 0 if cplx else 1)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popc(x):
    x = np.asarray(x, dtype=np.uint32)
    return _POP8[x & 255] + _POP8[(x >> 8) & 255] + _POP8[(x >> 16) & 255] + _POP8[x >> 24]


def cpx(re, im):
    """re + i*im without an arithmetic operation (keeps the sign of a zero)"""
    re, im = np.broadcast_arrays(np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64))
    out = np.empty(re.shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def cross_terms(c: Case, val: Values, mu, md, dt=np.float64):
    """the products U_o * n and Ust * n of diag_cross for configurations mu (array) and md (scalar), as a list of arrays of type dt"""
    both = mu & np.uint32(md)
    out = [dt(val.uloc[o]) * popc(both & val.orbmask[o]).astype(dt) for o in range(c.norb)]
    if c.norb > 1 and val.ust != 0.0:
        acc = sum(popc(mu & val.sitemask[l]) * popc(np.uint32(md) & val.sitemask[l]) - popc(both & val.sitemask[l]) for l in range(val.nlat))
        out.append(dt(val.ust) * acc.astype(dt))
    return out


# ---- the expected result: triplets and a plain sum ------------------------------------------------------------------------------------------
LD, CLD = np.longdouble, np.clongdouble


def h0_buffer(c: Case):
    h = np.empty(c.qdw * c.pitch + 1, dtype=np.complex128)
    h[:] = SENT * (1 + (np.arange(h.shape[0]) % 7))
    return h


def partial0(n):
    return -7.5 - np.arange(n, dtype=np.float64)


def jobs_of(c: Case, t: Tables, g, bug=None):
    """(workgroup, block, first column, end column) of every workgroup; idle ones have end <= first"""
    out = []
    for b in range(g["nwg"]):
        xcd, j = b & 7, b >> 3
        chunk = j // c.nblocks
        kb = int(take(t.order, j - chunk * c.nblocks, "order"))
        if bug == "chunk_round":
            cut = lambda q: -(-(q * g["gpx"]) // g["chunks"])
        else:
            cut = lambda q: (q * g["gpx"]) // g["chunks"]
        g0 = xcd * g["gpx"] + cut(chunk)
        g1 = min(xcd * g["gpx"] + cut(chunk + 1), g["ngroups"])
        out.append((b, kb, g0, g1 if chunk < g["chunks"] else g0))
    return out


def expected(c: Case, t: Tables, val: Values, lz=None, g=None):
    """(hv, partial, partial2, bound_hv, bound_p, bound_p2, exact): the result in extended precision from the triplets, rounded to float64
    with the epilogue's two steps applied in the kernel's order (so that an exact kind gives the kernel's bits), and the BOUNDS of the
    docstring.  hv keeps h0_buffer wherever the kernel stores nothing; partials keep partial0 beyond the launch's workgroups.  `exact` holds
    the same three buffers UNROUNDED, as np.longdouble (hv as [qdw*pitch+1][2] real and imaginary parts): what the random kinds are held
    against, so that no rounding of the reference stands between the device and the bound."""
    lz = c.lz if lz is None else lz
    g = g or case_geometry(c, t, lz=lz)
    dimup, pitch, qdw = c.dimup, c.pitch, c.qdw
    X = val.v.reshape(c.nslots, pitch)[c.slab0:c.slab0 + qdw, :dimup].astype(CLD)
    # one explicit zero triplet per row, so that every row has a segment
    rows = np.concatenate([t.trip[:, 0], np.arange(dimup)])
    srcs = np.concatenate([t.trip[:, 1], np.arange(dimup)])
    cf = np.concatenate([val.scoef[t.trip[:, 2]], np.zeros(dimup)]).astype(CLD)
    o = np.argsort(rows, kind="stable")
    rows, srcs, cf = rows[o], srcs[o], cf[o]
    seg = np.searchsorted(rows, np.arange(dimup))
    nhop = np.diff(np.concatenate([seg, [len(rows)]])) - 1
    if c.wt:
        W = (val.wt.reshape(-1, dimup, c.wc).transpose(0, 2, 1).reshape(-1, dimup)[:qdw] if c.wc else val.wt.reshape(qdw, pitch)[:, :dimup]).astype(CLD)
    S = np.empty((qdw, dimup), dtype=CLD)
    A = np.empty((qdw, dimup, 2), dtype=LD)     # sums of absolute terms, per component
    cre, cim = np.abs(cf.real), np.abs(cf.imag)
    for col in range(qdw):
        x = X[col]
        terms = cross_terms(c, val, t.map_up, t.map_dw[c.dw0 + col], LD)
        d = val.a_up.astype(LD) + LD(val.a_dw[c.dw0 + col]) + sum(terms)
        dabs = np.abs(val.a_up) + abs(val.a_dw[c.dw0 + col]) + sum(np.abs(x_) for x_ in terms)
        xs = x[srcs]
        S[col] = d * x + np.add.reduceat(cf * xs, seg)
        A[col, :, 0] = dabs * np.abs(x.real) + np.add.reduceat(cre * np.abs(xs.real) + cim * np.abs(xs.imag), seg)
        A[col, :, 1] = dabs * np.abs(x.imag) + np.add.reduceat(cre * np.abs(xs.imag) + cim * np.abs(xs.real), seg)
        if c.wt:
            S[col] += W[col]
            A[col, :, 0] += np.abs(W[col].real)
            A[col, :, 1] += np.abs(W[col].imag)
    F = (nhop if val.real_h else 2 * nhop)[None, :]
    s1, c1, s2, c2 = (val.scal[i] for i in (I_S, I_C, I_S2, I_C2))
    if lz == 0:
        sre = sim = 1.0
        cre_, cim_ = 0.0, 0.0
    else:
        sre, sim = (s1, s1) if lz == 1 else (s1, s2)
        cre_, cim_ = ((c1, c1) if lz == 1 else (c1, c2)) if val.xm is not None else (0.0, 0.0)
    XM = val.xm.reshape(qdw, pitch)[:, :dimup] if val.xm is not None else np.zeros((qdw, dimup), dtype=np.complex128)
    wre_x = S.real * LD(sre) - LD(cre_) * XM.real.astype(LD)
    wim_x = S.imag * LD(sim) - LD(cim_) * XM.imag.astype(LD)
    gam = gamma(F + 3 + KD)
    bre = gam * (abs(sre) * A[:, :, 0] + abs(cre_) * np.abs(XM.real))
    bim = gam * (abs(sim) * A[:, :, 1] + abs(cim_) * np.abs(XM.imag))
    # float64 result: the sum rounded once (+0 for a zero), then the epilogue's two steps in float64 (exact for the exact kinds)
    S64r, S64i = S.real.astype(np.float64) + 0.0, S.imag.astype(np.float64) + 0.0
    if lz == 0:
        wr, wi = S64r, S64i
    else:
        wr, wi = S64r * sre, S64i * sim
        if val.xm is not None:
            wr, wi = wr + (-cre_) * XM.real, wi + (-cim_) * XM.imag
    hv = h0_buffer(c)
    H = hv[:-1].reshape(qdw, pitch)
    H[:, :dimup] = cpx(wr, wi)
    bound = np.zeros((qdw, pitch, 2))
    bound[:, :dimup, 0], bound[:, :dimup, 1] = bre, bim
    npart = g["nwg"] + 3
    part, part2 = partial0(npart), partial0(npart) - 100.0
    bp, bp2 = np.zeros(npart), np.zeros(npart)
    xhv = np.stack([hv.real.astype(LD), hv.imag.astype(LD)], axis=1)
    xH = xhv[:-1].reshape(qdw, pitch, 2)
    xH[:, :dimup, 0], xH[:, :dimup, 1] = wre_x, wim_x
    xpart, xpart2 = part.astype(LD), part2.astype(LD)
    if lz:
        xr, xi = X.real, X.imag
        tre, tim = LD(sre) * xr * wre_x, LD(sim) * xi * wim_x
        ere, eim = abs(sre) * np.abs(xr) * bre, abs(sim) * np.abs(xi) * bim
        for b, kb, g0, g1 in jobs_of(c, t, g):
            r0, r1 = int(t.start[kb]), int(t.start[kb + 1])
            if g1 <= g0:
                part[b] = xpart[b] = 0.0
                if lz == 2:
                    part2[b] = xpart2[b] = 0.0
                continue
            gd = gamma(g1 - g0 + 3 + 6 + 15)
            sl = (slice(g0, g1), slice(r0, r1))
            if lz == 1:
                xpart[b] = tre[sl].sum() + tim[sl].sum()
                part[b] = float(xpart[b])
                bp[b] = float(ere[sl].sum() + eim[sl].sum() + gd * (np.abs(tre[sl]).sum() + np.abs(tim[sl]).sum()))
            else:
                xpart[b], xpart2[b] = tre[sl].sum(), tim[sl].sum()
                part[b], part2[b] = float(xpart[b]), float(xpart2[b])
                bp[b] = float(ere[sl].sum() + gd * np.abs(tre[sl]).sum())
                bp2[b] = float(eim[sl].sum() + gd * np.abs(tim[sl]).sum())
    return hv, part, part2, bound.reshape(-1, 2), bp, bp2, (xhv, xpart, xpart2)


def exact_headroom(c: Case, t: Tables, val: Values, lz=None):
    """largest sum|terms| / quantum over the elements (quantum 2**-5) and over the partials (2**-8) of an exact kind: below 2**53 every sum of
    the kernel is exact in float64 in any order"""
    lz = c.lz if lz is None else lz
    _, p, p2, bound, bp, bp2 = expected(c, t, val, lz)[:6]
    # the bounds are gamma(k) * sum|terms| with k >= 11: sum|terms| <= bound / (11 u)
    el = bound.max() / (11 * U) / 2.0 ** -5
    pa = max(bp.max(), bp2.max()) / (11 * U) / 2.0 ** -8 if lz else 0.0
    return el, pa


# ---- the restatement of a launch ----------------------------------------------------------------------------------------------------------
def take(arr, idx, what):
    """arr[idx] after the check that a kernel does not make"""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= arr.shape[0]):
        raise OutOfBounds(f"{what}: index {int(idx.min())}..{int(idx.max())} outside [0,{arr.shape[0]})")
    return arr[idx]


def walk(c: Case, t: Tables, val: Values, bug=None, lz=None, job_stages=None, job_groups=None, stats=None):
    """(hv, partial, partial2) as the kernel leaves them, from the TABLES, every workgroup in turn.  Raises OutOfBounds at the first index
    outside a buffer or LDS offset outside the launch's LDS.  `stats`: a dict that collects what the launch reaches."""
    lz = c.lz if lz is None else lz
    g = case_geometry(c, t, job_stages, job_groups, lz)
    if not g["fits"] or g["lds_bytes"] > LDS_BUDGET:
        raise OutOfBounds("the launch does not fit")
    st = stats if stats is not None else {}
    for k in ("n", "ntile", "dist", "kin", "nouter", "slots", "first_mod", "first_odd", "groups_per_job", "nch"):
        st.setdefault(k, set())
    st.update(nst=g["nst"], chunks=g["chunks"], idle=0, KIN=20 if g["kin_rows"] <= 20 else JOB_KIN, run_lengths=set(), clamped=g["nst"] < (job_stages or c.job_stages))
    dimup, pitch, qdw, nst, ns = c.dimup, c.pitch, c.qdw, g["nst"], g["ns"]
    nscoef = 2 * c.ncoef + 1
    LCB = 3 if val.real_h else 4
    EMPTY = (nscoef - 1) << SHIFT
    book = (nscoef * 16 + 255) // 256 * 256
    ring0 = book + 256
    wtb = ring0 + nst * g["stage_bytes"]
    lds_bytes = g["lds_bytes"]
    wcw = max(c.wc, 1)
    lw = wcw.bit_length() - 1
    KIN = st["KIN"]

    def lds_ok(off_hi, what):
        if off_hi > lds_bytes:
            raise OutOfBounds(f"LDS {what}: byte {off_hi} beyond {lds_bytes}")

    lds_ok(book + 4 * JOB_MAX_STAGES + 8, "bookkeeping words")
    if lz:
        lds_ok(ring0 + 8 * (JOB_WAVES + JOB_LOADER), "wave sums")
    hv = h0_buffer(c)
    hvd = hv[:-1]
    npart = g["nwg"] + 3
    part, part2 = partial0(npart), partial0(npart) - 100.0
    xm_on = lz and val.xm is not None
    sc = val.scal[I_S] if lz else 1.0
    cm = val.scal[I_C] if (lz and (xm_on or bug == "cm_with_xm_null")) else 0.0
    sc2 = val.scal[I_S2] if lz == 2 else 1.0
    cm2 = val.scal[I_C2] if (lz == 2 and (xm_on or bug == "cm_with_xm_null")) else 0.0
    coef_lds = val.scoef if not val.real_h else val.scoef.real.astype(np.complex128)

    for b, kb, g0, g1 in jobs_of(c, t, g, bug):
        ntile = g1 - g0
        if ntile <= 0:
            st["idle"] += 1
            if lz and bug != "idle_partial_unwritten":
                take(part, b, "partial")
                part[b] = 0.0
                if lz == 2:
                    part2[b] = 0.0
            continue
        r0 = int(take(t.start, kb, "start"))
        n = int(take(t.start, kb + 1, "start")) - r0
        nch = (n + 63) >> 6
        st["n"].add(n); st["ntile"].add(ntile); st["nch"].add(nch); st["run_lengths"].add((b & 7, ntile))
        nlive = nch * 64                         # rows of the live compute waves
        p = np.arange(nlive)
        row_ok = p < n
        pr = np.minimum(p, n - 1)
        wave = p >> 6
        # ---- tables into registers
        tb0 = r0 if bug == "tstart_ignored" else int(take(t.tstart, kb, "tstart"))
        tin = np.full((KIN, nlive), 0, dtype=np.uint32)
        for k in range(KIN):
            e = np.full(nlive, EMPTY, dtype=np.uint32)
            if k < g["kin_rows"]:
                e = np.where(row_ok, take(t.ell_in, k * dimup + tb0 + pr, "ell_in"), e).astype(np.uint32)
            tin[k] = ((e >> SHIFT) << (16 + LCB)) | ((e & OFFM) << 4)
            if (((e.astype(np.int64) & OFFM) << 4) > 0xFFFF).any():
                raise OutOfBounds("in-block offset does not fit 16 bits")
        rs0, rs1 = int(take(t.rs_ptr, kb, "rs_ptr")), int(take(t.rs_ptr, kb + 1, "rs_ptr"))
        bh0, bh1 = int(take(t.bh_ptr, kb, "bh_ptr")), int(take(t.bh_ptr, kb + 1, "bh_ptr"))
        nrs, nbh = rs1 - rs0, bh1 - bh0
        nouter = nrs + nbh
        st["nouter"].add(nouter); st["slots"].add((nrs > 0, nbh > 0))
        if nouter > JOB_KO:
            raise OutOfBounds("more out-of-block slots than registers")
        tou = np.zeros((JOB_KO, nlive), dtype=np.uint32)
        for i in range(JOB_KO):
            e = np.full(nlive, EMPTY, dtype=np.int64)
            if i < nrs:
                e = take(t.rs_tab, int(take(t.rs_off, rs0 + i, "rs_off")) + pr, "rs_tab").astype(np.int64)
                neg = 0 if bug == "rs_neg_ignored" else int(take(t.rs_neg, rs0 + i, "rs_neg"))
                base = 0 if bug == "rs_base_ignored" else int(take(t.rs_base, rs0 + i, "rs_base"))
                e = np.where(e != EMPTY, ((e ^ (neg << SHIFT)) & ~OFFM) | ((e & OFFM) + base), e)
            elif i < nouter:
                h = bh0 + i - nrs
                e = (int(take(t.bh, 2 * h + 1, "bh")) << SHIFT) | (int(take(t.bh, 2 * h, "bh")) + (0 if bug == "bh_no_row" else pr))
                e = np.broadcast_to(np.asarray(e, dtype=np.int64), (nlive,))
            e = np.where(row_ok, e, EMPTY)
            if ((e & OFFM) >= 65536).any():
                raise OutOfBounds("out-of-block row does not fit the packed word")
            tou[i] = (((e >> SHIFT) << 23) | ((e & OFFM) << 4)).astype(np.uint32)
        kin_w = take(t.gmax, int(take(t.gstart, kb, "gstart")) + np.arange(nch), "gmax").astype(np.int64) & 0xFFFF
        for x in kin_w:
            st["kin"].add(int(x))
        if bug == "kin_round_down":
            kin_w = kin_w & ~3
        kin = kin_w[wave]
        au = take(val.a_up, r0 + pr, "a_up")
        mu = take(t.map_up, r0 + pr, "map_up")
        # ---- the loader's schedule: what each ring stage and group buffer holds when compute tile k reads it
        ring = [None] * nst        # tile index
        wbuf = [None, None]        # scratch group
        vdone, wdone = [0] * nst, [0, 0]
        ops = 0
        st_issue = 0
        tile_ops = nch * (2 if xm_on else 1)
        wpieces = (n * wcw + 63) >> 6
        lds_ok(wtb + 2 * g["wt_bytes"], "group buffers")
        if wpieces * 1024 > g["wt_bytes"] or nch * 64 > ns:
            raise OutOfBounds("a DMA piece beyond its buffer")
        if xm_on and 2 * ns * 16 > g["stage_bytes"]:
            raise OutOfBounds("the xm tile beyond its stage")

        def issue_v(k):
            nonlocal ops, st_issue
            ring[st_issue] = k
            ops += tile_ops
            vdone[st_issue] = ops
            st_issue = (st_issue + 1) % nst

        def issue_w(G):
            nonlocal ops
            bi = 0 if bug == "group_not_alternated" else G & 1
            wbuf[bi] = G
            if c.wt:
                ops += wpieces
            wdone[bi] = ops

        clast = min(g1, qdw) - 1
        Gfirst, Glast = g0 >> lw, clast >> lw
        st["first_mod"].add(g0 & (wcw - 1)); st["first_odd"].add(Gfirst & 1); st["groups_per_job"].add(Glast - Gfirst + 1)
        issue_w(Gfirst)
        issued = 0
        while issued < min(nst - 1, ntile):
            issue_v(issued)
            issued += 1
        if Gfirst < Glast:
            issue_w(Gfirst + 1)
        Gprev = Gfirst
        asum = np.zeros(nlive)
        asum2 = np.zeros(nlive)
        pend = None
        for k in range(ntile):
            col = g0 + k
            Gk = col >> lw
            need = max(vdone[k % nst], wdone[0 if bug == "group_not_alternated" else Gk & 1])
            dist = ops - need
            st["dist"].add(dist)
            if dist < 0:
                raise OutOfBounds("the wait names operations not yet issued")
            # A(k): afterwards the loader refills what tile k-1 used -- BEFORE compute k in this walk: a buffer it must not touch shows
            if issued < ntile:
                issue_v(issued)
                issued += 1
            if Gk != Gprev:
                if Gk < Glast:
                    issue_w(Gk + 1)
                Gprev = Gk
            stage = (k - 1) % nst if bug == "stage_prev" else k % nst
            held = ring[stage]
            lds_ok(ring0 + stage * g["stage_bytes"] + g["stage_bytes"], "ring stage")
            # the tile in that stage: rows 0 .. nch*64-1 (the last piece repeats row n-1), column slab0 + c of v and c of xm
            if held is None:
                xt = np.full(nlive, NAN)
                xmt = np.full(nlive, NAN)
            else:
                ch = min(g0 + held, qdw - 1)
                vcol = ch if bug == "v_no_slab0" else c.slab0 + ch
                xt = take(val.v, vcol * pitch + r0 + pr, "v tile")
                if xm_on and bug == "xm_slab0":    # (what lies behind xm's last column is not the test's: NaN stands for it)
                    xi = (c.slab0 + ch) * pitch + r0 + pr
                    xmt = np.where(xi < val.xm.shape[0], val.xm[np.minimum(xi, val.xm.shape[0] - 1)], NAN)
                else:
                    xmt = take(val.xm, ch * pitch + r0 + pr, "xm tile") if xm_on else np.full(nlive, NAN)
            cc = min(col, qdw - 1)
            # scratch value
            if c.wt:
                bi = 0 if bug == "group_not_alternated" else (cc >> lw) & 1
                G = wbuf[bi]
                off = p * wcw + (cc & (wcw - 1))
                lds_ok(wtb + bi * g["wt_bytes"] + int(off.max()) * 16 + 16, "scratch read")
                if G is None:
                    acc = np.full(nlive, NAN)
                else:
                    blocked = c.wc or bug == "wc0_blocked"
                    base = (G * dimup + r0) * wcw if blocked else G * pitch + r0
                    loaded = off < wpieces * 64
                    acc = np.where(loaded, take(val.wt, base + np.minimum(off, n * wcw - 1), "scratch group"), NAN)
            else:
                acc = np.zeros(nlive, dtype=np.complex128)
            cg = (0 if bug == "diag_no_dw0" else c.dw0) + cc
            md, adw = take(t.map_dw, cg, "map_dw"), take(val.a_dw, cg, "a_dw")
            d = au + adw
            for x_ in cross_terms(c, val, mu, md):
                d = d + x_
            acc = acc + d * xt
            # in-block hops: groups of four slots while k4 < kin of the wave
            for q in range(KIN):
                on = (q // 4 * 4) < kin
                if not on.any():
                    continue
                e = tin[q].astype(np.int64)
                ca = e >> 16
                if ((ca >> LCB) >= nscoef).any() or (ca + (1 << LCB) > book).any():
                    raise OutOfBounds("coefficient address")
                src = (e & 0xFFFF) >> 4
                if (src[on] >= ns).any():
                    raise OutOfBounds("LDS in-block source beyond the tile column")
                if (src[on] >= n).any():
                    raise OutOfBounds("in-block source beyond the block")
                acc = acc + np.where(on, coef_lds[ca >> LCB] * xt[np.minimum(src, nlive - 1)], 0.0)
            # out-of-block: slots 0..3 always, further ones while i < nouter
            for i in range(JOB_KO):
                if not (i < 4 or i < nouter):
                    continue
                w_ = tou[i].astype(np.int64)
                srow = (w_ & 0x7FFFFF) >> 4
                if (srow >= dimup).any():
                    raise OutOfBounds("gather beyond the column's rows")
                ci = w_ >> 23
                if (ci >= nscoef).any():
                    raise OutOfBounds("coefficient index")
                acc = acc + coef_lds[ci] * take(val.v, (c.slab0 + col) * pitch + srow, "gather")
            # epilogue
            w = acc
            if lz == 2:
                w = cpx(w.real * sc, w.imag * sc2)
                if xm_on or bug == "cm_with_xm_null":
                    w = cpx(w.real + (-cm) * xmt.real, w.imag + (-cm2) * xmt.imag)
                live = np.ones(nlive, dtype=bool) if bug == "pad_lanes_sum" else row_ok
                asum = asum + np.where(live, sc * (xt.real * w.real), 0.0)
                asum2 = asum2 + np.where(live, sc2 * (xt.imag * w.imag), 0.0)
            elif lz == 1:
                w = cpx(w.real * sc, w.imag * sc)
                if xm_on or bug == "cm_with_xm_null":
                    w = cpx(w.real + (-cm) * xmt.real, w.imag + (-cm) * xmt.imag)
                live = np.ones(nlive, dtype=bool) if bug == "pad_lanes_sum" else row_ok
                asum = asum + np.where(live, sc * (xt.real * w.real + xt.imag * w.imag), 0.0)
            # the previous tile's result is stored now, this one's a tile later
            if pend is not None:
                pc, pw = pend
                if bug == "store_current_column":
                    pc = col
                idx = pc * pitch + r0 + p[row_ok]
                take(hvd, idx, "hv store")
                hvd[idx] = pw[row_ok]
            pend = (col, w)
        if pend is not None and bug != "drop_last_store":
            pc, pw = pend
            idx = pc * pitch + r0 + p[row_ok]
            take(hvd, idx, "hv store")
            hvd[idx] = pw[row_ok]
        if lz:
            take(part, b, "partial")
            a1, a2 = (asum2, asum) if bug == "lz2_swapped" else (asum, asum2)
            part[b] = a1.sum() + 0.0
            if lz == 2:
                part2[b] = a2.sum() + 0.0
    return hv, part, part2


def differs(got, want):
    """bit-for-bit comparison of (hv, partial, partial2) triples: the names of the buffers that differ"""
    return [n for n, a, b in zip(("hv", "partial", "partial2"), got, want) if not np.array_equal(bits(a), bits(b))]


# ---- what the two test files share --------------------------------------------------------------------------------------------------------
# cases whose launch is repeated under other ring depths and chunk cuts (same hv bits: neither changes an operation)
VARIANT_CASES = ["edge-sizes-lz1", "mid-wc2-long", "mid-wc8-odd", "full-960-lz1-clamped"]
VARIANT_STAGES = [2, 3, 4, 8]
VARIANT_GROUPS = [1, 2, 3, 5, 100]


@lru_cache(maxsize=None)
def tables_of(k):
    return build_tables(all_cases()[k])


@lru_cache(maxsize=None)
def prepared(k, kind):
    """(case, tables, values, expected) of case k with one kind of values: computed once, never changed"""
    c = all_cases()[k]
    t = tables_of(k)
    val = values(c, t, kind)
    return c, t, val, expected(c, t, val)


def plain_cases_that_fit_the_epilogue():
    """indices of the LZ = 0 cases that can run once more as LZ = 1 (s = 1, c = 0, no xm): the ring stages are twice as large then"""
    return [k for k, c in enumerate(all_cases()) if c.lz == 0 and case_geometry(c, tables_of(k), lz=1)["fits"]]


# ---- reach of a launch from the plan's numbers alone (scripts/job_kernel_reach.py; held against walk's own statistics on the CPU) ---------
def loader_distances(n, g0, g1, qdw, nst, wcw, has_wt, xm_on):
    """the arguments `ops - need` of the loader's counted wait, tile by tile, for a block of n rows and the columns [g0, g1)"""
    nch, wpieces = (n + 63) >> 6, (n * wcw + 63) >> 6
    lw = wcw.bit_length() - 1
    ntile = g1 - g0
    vdone, wdone, ops, st_issue, out = [0] * nst, [0, 0], 0, 0, []

    def issue_w(G):
        nonlocal ops
        ops += wpieces if has_wt else 0
        wdone[G & 1] = ops

    def issue_v():
        nonlocal ops, st_issue
        ops += nch * (2 if xm_on else 1)
        vdone[st_issue] = ops
        st_issue = (st_issue + 1) % nst

    Gfirst, Glast = g0 >> lw, (min(g1, qdw) - 1) >> lw
    issue_w(Gfirst)
    issued = min(nst - 1, ntile)
    for _ in range(issued):
        issue_v()
    if Gfirst < Glast:
        issue_w(Gfirst + 1)
    Gprev = Gfirst
    for k in range(ntile):
        Gk = (g0 + k) >> lw
        out.append(ops - max(vdone[k % nst], wdone[Gk & 1]))
        if issued < ntile:
            issue_v()
            issued += 1
        if Gk != Gprev:
            if Gk < Glast:
                issue_w(Gk + 1)
            Gprev = Gk
    return out


def reach_of(sizes, nouter, gkin, qdw, ncoef, k_in, k_in_real, job_groups, job_stages, wc, lz, xm_on=True, has_wt=True):
    """the reach columns of one launch: sizes / nouter / gkin (in-block bound per 64-row group) per block"""
    g = geometry(qdw, max(sizes), len(sizes), ncoef, k_in, k_in_real, job_groups, job_stages, wc, lz)
    wcw = max(wc, 1)
    lw = wcw.bit_length() - 1
    r = dict(fits=g["fits"], nst=g["nst"], clamped=g["nst"] < job_stages, chunks=g["chunks"], KIN=20 if g["kin_rows"] <= 20 else JOB_KIN,
             n=sorted(set(sizes)), nch=sorted({(n + 63) >> 6 for n in sizes}), nouter=sorted(set(nouter)), kin=sorted({k for ks in gkin for k in ks}))
    if not g["fits"]:
        return r
    ntiles, dists, groups, idle, mid, odd = set(), set(), set(), 0, False, False
    for xcd in range(8):
        for chunk in range(g["chunks"]):
            g0 = xcd * g["gpx"] + (chunk * g["gpx"]) // g["chunks"]
            g1 = min(xcd * g["gpx"] + ((chunk + 1) * g["gpx"]) // g["chunks"], qdw)
            if g1 <= g0:
                idle += len(sizes)
                continue
            ntiles.add(g1 - g0)
            groups.add(((g1 - 1) >> lw) - (g0 >> lw) + 1)
            mid |= (g0 & (wcw - 1)) != 0
            odd |= ((g0 >> lw) & 1) == 1
            for n in set(sizes):
                dists |= set(loader_distances(n, g0, g1, qdw, g["nst"], wcw, has_wt, bool(lz) and xm_on))
    r.update(ntile=sorted(ntiles), ntile_lt_ring=min(ntiles) < g["nst"] - 1, ntile_gt_2ring=max(ntiles) > 2 * g["nst"], dist_max=max(dists),
             saturates=max(dists) > 63, groups_per_job=sorted(groups), idle_wg=idle, first_mid_group=mid, first_odd_group=odd)
    return r
