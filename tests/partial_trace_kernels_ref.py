"""References, bounds, exact restatements, the synthetic sectors and the case list for the kernels of the partial-trace engine
(csrc/hxv_partial_trace_kernels.hpp), shared by tests/test_gpu_partial_trace_kernels.py (the device) and
tests/test_partial_trace_kernels_ref_cpu.py (which shows that the checks bite and that the cases reach the paths they are there for).

Everything here is written from the table DEFINITIONS of csrc/hxv_partial_trace_host.hpp, not from the kernels' loops:
  pair p of a class       local dw group gd = p // ngu, up group g = p % ngu
  its component k         iu = k % du, id = k // du; row word rows[rows_off + g*du + iu], column word cols[cols_off + gd*dd + id];
                          x_k = s * src[slot * pitch + row], s = -1 where the two words' bits 31 differ
  an item's block         element (i, j), i <= j < n, = sum over its pairs [p0, p1) of x_i conj(x_j); tile (ti, tj) = tiles[tile_off + tile]
                          holds element (ti*t + a, tj*t + q) at out_off + tile*t*t + a*t + q
  nrep == 4               four such blocks in a row, wave w's holds the pairs b = w (mod 4) of each batch; a batch is `batch` consecutive
                          up groups of one dw group, counted from the item's first pair in that group
  reduce                  out[e] = sum over k < el_cnt[e] of partial[el_src[e] + k*el_stride[e]], in that order
  scatter                 class block element (i, j) -> rho[io, jo] and its conjugate to rho[jo, io], io = au[i % du] + (ad[i // du] << nsub)

Two input families.  EXACT: real and imaginary parts are integers in [-8, 8]; a product is below 2**7, an element sums at most
4 * (pairs of the case) of them, far below 2**53, so every partial sum in ANY order, fused or not, is an exact double and the device block
must equal the integer reference bit for bit (the integers are int64 here, which is exact for the same reason; MAX_EXACT_PAIRS is asserted).
ROUNDING: complex normals normalised over the named positions, against the same sum in long double.

The bound of the rounding family, from the kernel text.  An element's real (imaginary) part is a dot product of 2P products, P the pairs the
accumulator saw: `acc += a*b + c*d` rounds each product once (not at all where the compiler fuses it), their sum once, and the accumulation
once per pair -- the first of them onto zero, which is exact -- so a product passes at most 1 + 1 + (P - 1) <= 2P roundings for P >= 1.  The
sign factor f = +-1 is exact.  R further additions follow: the pair kernel's butterfly (6) and its four waves (v = 0 + red[0] + ... : 4),
the host's sum of the four wave blocks (4), the reduce kernel's el_cnt additions.  Hence |device - exact| <= gamma(2P + R) sum|products|.
c = 2 is added to the index: one unit for the long-double reference's own error, gamma_64bit(2P + R) sum|products| <= u sum|products| while
2P + R <= 2**11 (asserted), one for rounding that reference to double when the difference is taken.  The bound was derived before the first
device run and has not been touched since."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

PT_THREADS, PT_XS, PT_PAIR_N, PT_LOADS, PT_PAIR_COST, PT_WG_PER_CU = 256, 2048, 4, 4, 36, 4   # (the GPU test pins them to the library's)
U = 2.0 ** -53
SENT = complex(-1234.5, 6789.25)
NAN = float("nan")
CNAN = complex(NAN, NAN)
MASK = np.uint32(0x7FFFFFFF)
MAX_EXACT_PAIRS = 1 << 30          # 4 * 2**30 products below 2**7 stay below 2**53
PAIR_R = 6 + 4                     # pt_pair_kernel: xor butterfly over 64 lanes, then the four waves

CLS_DT = np.dtype([(f, "<i4") for f in ("du", "dd", "n", "t", "nt", "ntiles", "batch", "stride", "ngu", "rows_off", "cols_off", "tile_off", "nrep")])
ITEM_DT = np.dtype([("cls", "<i4"), ("p0", "<i4"), ("p1", "<i4"), ("pad", "<i4"), ("out_off", "<i8")])


def gamma(k):
    assert k * U < 0.01
    return k * U / (1.0 - k * U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- synthetic sectors ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """A sector that no Hamiltonian needs to have: ngu[k] (ngd[k]) up (dw) groups whose traced part holds k particles, each of
    C(nsub, nup - k) (C(nsub, ndw - k)) rows (columns); the rows and columns of the groups are a random permutation of the sector's."""
    name: str
    nsub: int
    nup: int
    ndw: int
    ngu: tuple
    ngd: tuple
    small_n: int = PT_PAIR_N
    ncu: int = 1
    nranks: int = 1
    rank: int = 0
    signs: str = "mixed"           # "mixed": random bits 31; "none"; "all": every word has it, which must change nothing
    cols: str = "random"           # "by_k": the groups' columns in list order, so that the last rank owns no dw group of the first k

    def du(self, k):
        return math.comb(self.nsub, self.nup - k) if 0 <= self.nup - k <= self.nsub else 0

    def dd(self, k):
        return math.comb(self.nsub, self.ndw - k) if 0 <= self.ndw - k <= self.nsub else 0


def dw_split(dimdw, rank, nranks):
    """(qdw, dw0): the columns of `rank` (the reference's split: the first dimdw % nranks ranks own one more)"""
    q, rem = divmod(dimdw, nranks)
    return q + (1 if rank < rem else 0), rank * q + min(rank, rem)


@dataclass
class Sector:
    case: Case
    words: np.ndarray      # int32[9]: nsub, nup, ndw, dimup, dimdw, nranks, cmax, qdw, dw0
    up: list               # [k] uint32 words, [ngu[k]][du(k)]
    dw: list
    pitch: int
    nslots: int            # column slots of src: dimdw, or nranks * cmax on a split sector
    dimup: int
    dimdw: int


def make_sector(case):
    assert len(case.ngu) == len(case.ngd)
    seed = [int.from_bytes(case.name.encode(), "little") % (1 << 63), case.nsub]
    perm_rng, sign_rng = np.random.default_rng(seed + [1]), np.random.default_rng(seed + [2])
    nk = len(case.ngu)
    assert all(case.du(k) > 0 or case.ngu[k] == 0 for k in range(nk)) and all(case.dd(k) > 0 or case.ngd[k] == 0 for k in range(nk))
    dimup = sum(case.ngu[k] * case.du(k) for k in range(nk))
    dimdw = sum(case.ngd[k] * case.dd(k) for k in range(nk))
    assert dimup > 0 and dimdw >= case.nranks

    def words(perm, counts, signs):
        out, pos = [], 0
        for cnt in counts:
            w = perm[pos:pos + cnt].astype(np.uint32)
            bits = sign_rng.integers(0, 2, cnt).astype(np.uint32)          # (drawn in every mode: the same permutation and amplitudes)
            if signs == "all":
                bits[:] = 1
            elif signs == "none":
                bits[:] = 0
            out.append(w | (bits << np.uint32(31)))
            pos += cnt
        return out

    rows = perm_rng.permutation(dimup)
    colp = perm_rng.permutation(dimdw)
    if case.cols == "by_k":
        colp = np.arange(dimdw)
    up = words(rows, [case.ngu[k] * case.du(k) for k in range(nk)], case.signs)
    dw = words(colp, [case.ngd[k] * case.dd(k) for k in range(nk)], case.signs)
    cmax = -(-dimdw // case.nranks)
    qdw, dw0 = dw_split(dimdw, case.rank, case.nranks)
    w = np.array([case.nsub, case.nup, case.ndw, dimup, dimdw, case.nranks, cmax, qdw, dw0], dtype=np.int32)
    return Sector(case, w, up, dw, (dimup + 7) // 8 * 8 + 8, dimdw if case.nranks == 1 else case.nranks * cmax, dimup, dimdw)


# ---- tables (the ptb_* entries of tests/host/partial_trace_build.hpp, in either library) ---------------------------------------------------
class BuildError(Exception):
    pass


def bind(lib):
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    lib.ptb_build.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, C.c_char_p, i32]
    lib.ptb_build.restype = vp
    lib.ptb_free.argtypes = [vp]
    lib.ptb_free.restype = None
    lib.ptb_sizes.argtypes = [vp, i64p]
    lib.ptb_copy.argtypes = [vp] * 11
    lib.ptb_class_configs.argtypes = [vp, i32, vp, vp]
    return lib


class Tables:
    """the host tables of pt_build for a Sector, as numpy arrays; .handle is the library's (freed with the object)"""

    def __init__(self, lib, sec, small_n=None, ncu=None):
        case = sec.case
        self.lib, self.sec = lib, sec
        up = np.ascontiguousarray(np.concatenate(sec.up), dtype=np.uint32)
        dw = np.ascontiguousarray(np.concatenate(sec.dw), dtype=np.uint32)
        ul = np.array([len(x) for x in sec.up], dtype=np.int64)
        dl = np.array([len(x) for x in sec.dw], dtype=np.int64)
        err = C.create_string_buffer(256)
        self.handle = lib.ptb_build(sec.words.ctypes.data, len(sec.up), up.ctypes.data, ul.ctypes.data, dw.ctypes.data, dl.ctypes.data,
                                    case.small_n if small_n is None else small_n, case.ncu if ncu is None else ncu, err, 256)
        if not self.handle:
            raise BuildError(err.value.decode())
        sz = (C.c_int64 * 11)()
        assert lib.ptb_sizes(self.handle, sz) == 0
        ncls, nitems, nrows, ncols, ntiles, self.out_elems, self.partial_elems = (int(x) for x in sz[:7])
        self.nitems = tuple(int(x) for x in sz[7:10])
        assert int(sz[10]) == CLS_DT.itemsize | (ITEM_DT.itemsize << 32), "PtClass / PtItem are not laid out as CLS_DT / ITEM_DT say"
        self.cls, self.items = np.zeros(ncls, CLS_DT), np.zeros(nitems, ITEM_DT)
        self.rows, self.cols, self.tiles = (np.zeros(n, np.uint32) for n in (nrows, ncols, ntiles))
        self.el_src, self.el_cnt, self.el_stride = np.zeros(self.out_elems, np.int64), np.zeros(self.out_elems, np.int32), np.zeros(self.out_elems, np.int32)
        self.cls_out_off, self.cls_ngd = np.zeros(ncls, np.int64), np.zeros(ncls, np.int32)
        assert lib.ptb_copy(self.handle, *(a.ctypes.data for a in (self.cls, self.items, self.rows, self.cols, self.tiles, self.el_src, self.el_cnt,
                                                                   self.el_stride, self.cls_out_off, self.cls_ngd))) == 0
        assert sum(self.nitems) == nitems

    def configs(self, ci):
        c = self.cls[ci]
        au, ad = np.zeros(c["du"], np.uint32), np.zeros(c["dd"], np.uint32)
        assert self.lib.ptb_class_configs(self.handle, ci, au.ctypes.data, ad.ctypes.data) == 0
        return au, ad

    def kernel_of(self, item):
        """0 pair kernel, 1 tile kernel <2,1>, 2 tile kernel <4,2>: the work list holds them in that order"""
        return 0 if item < self.nitems[0] else 1 if item < self.nitems[0] + self.nitems[1] else 2

    def block_elems(self, ci):
        c = self.cls[ci]
        return int(c["ntiles"]) * int(c["t"]) ** 2

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.ptb_free(self.handle)
            self.handle = None


def check_table_bounds(T):
    """Every index the kernels form from these tables stays inside the buffers the tests allocate (src of nslots * pitch elements, partial of
    partial_elems, out of out_elems, the LDS area of PT_XS).  Asserted before anything runs on a device."""
    sec = T.sec
    assert int((T.rows & MASK).max()) < sec.dimup <= sec.pitch
    assert len(T.cols) == 0 or int((T.cols & MASK).max()) < sec.nslots
    for c, ngd in zip(T.cls, T.cls_ngd):
        assert c["n"] == c["du"] * c["dd"] and c["t"] in (2, 4) and c["nrep"] in (1, 4) and 1 <= c["batch"]
        assert c["rows_off"] + c["ngu"] * c["du"] <= len(T.rows) and c["cols_off"] + int(ngd) * c["dd"] <= len(T.cols)
        assert c["tile_off"] + c["ntiles"] <= len(T.tiles) and c["ntiles"] <= (1 if c["t"] == 2 else 2) * PT_THREADS
        assert (c["dd"] - 1) * c["stride"] + c["batch"] * c["du"] <= PT_XS and c["stride"] >= c["batch"] * c["du"]
        tl = T.tiles[c["tile_off"]:c["tile_off"] + c["ntiles"]]
        assert int((tl & 0xFFFF).max()) < c["nt"] and int((tl >> 16).max()) < c["nt"]
    spans = []
    for k, it in enumerate(T.items):
        c = T.cls[it["cls"]]
        assert 0 <= it["p0"] < it["p1"] <= int(c["ngu"]) * int(T.cls_ngd[it["cls"]])
        kern = T.kernel_of(k)
        assert kern == 0 or (kern == 1) == (c["t"] == 2)
        if kern == 0:
            assert c["n"] <= PT_PAIR_N and c["t"] == 2 and c["nrep"] == 1 and c["ntiles"] * 4 <= PT_THREADS
        spans.append((int(it["out_off"]), int(it["out_off"]) + T.block_elems(it["cls"]) * int(c["nrep"])))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or (spans[0][0] >= 0 and spans[-1][1] <= T.partial_elems))
    if T.out_elems:
        last = T.el_src + np.maximum(T.el_cnt.astype(np.int64) - 1, 0) * T.el_stride
        assert T.el_src.min() >= 0 and T.el_cnt.min() >= 0 and (last[T.el_cnt > 0] < T.partial_elems).all()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def named_positions(T):
    """the positions of src that a table word names: (column slot of this rank's dw groups) x (row of an up group)"""
    sl = np.unique(T.cols & MASK).astype(np.int64)
    rw = np.unique(T.rows & MASK).astype(np.int64)
    return (sl[:, None] * T.sec.pitch + rw[None, :]).ravel()


def make_src(T, family, seed=0):
    """src[nslots * pitch + pitch]: NaN in the pad rows, in every slot no dw group of this rank names and in the guard behind the buffer"""
    rng = np.random.default_rng([seed, 77, len(T.rows), len(T.cols)])
    sec = T.sec
    src = np.full(sec.nslots * sec.pitch + sec.pitch, CNAN)
    pos = named_positions(T)
    if family == "exact":
        v = rng.integers(-8, 9, len(pos)) + 1j * rng.integers(-8, 9, len(pos))
    else:
        v = rng.standard_normal(len(pos)) + 1j * rng.standard_normal(len(pos))
        v /= np.linalg.norm(v) if len(pos) else 1.0
    src[pos] = v
    return src


# ---- the exact and the long-double reference -----------------------------------------------------------------------------------------------
def pair_vectors(T, ci, pairs, src):
    """x[p, k]: the signed amplitudes of the given pairs of class ci, k = iu + du*id"""
    c = T.cls[ci]
    du, dd, n, ngu = int(c["du"]), int(c["dd"]), int(c["n"]), int(c["ngu"])
    p = np.asarray(pairs, dtype=np.int64)
    gd, g = p // ngu, p % ngu
    k = np.arange(n)
    r = T.rows[int(c["rows_off"]) + g[:, None] * du + (k % du)[None, :]]
    cc = T.cols[int(c["cols_off"]) + gd[:, None] * dd + (k // du)[None, :]]
    s = 1.0 - 2.0 * ((r ^ cc) >> np.uint32(31)).astype(np.float64)
    return s * src[(cc & MASK).astype(np.int64) * T.sec.pitch + (r & MASK).astype(np.int64)]


def block_exact(x):
    """sum_p x_i conj(x_j) of integer-valued x[p, n] in integers: (re, im), each [n, n]"""
    assert len(x) < MAX_EXACT_PAIRS
    xr, xi = np.rint(x.real).astype(np.int64), np.rint(x.imag).astype(np.int64)
    assert (xr == x.real).all() and (xi == x.imag).all() and max(np.abs(xr).max(initial=0), np.abs(xi).max(initial=0)) <= 8
    return xr.T @ xr + xi.T @ xi, xi.T @ xr - xr.T @ xi


def block_longdouble(x):
    """the same in long double, and the sums of the products' magnitudes: (re, im, mag_re, mag_im)"""
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    ar, ai = np.abs(xr), np.abs(xi)
    return xr.T @ xr + xi.T @ xi, xi.T @ xr - xr.T @ xi, ar.T @ ar + ai.T @ ai, ai.T @ ar + ar.T @ ai


def block_layout(T, ci):
    """(offset in a block, i, j, live) of every element of a class block, in storage order"""
    c = T.cls[ci]
    t, n = int(c["t"]), int(c["n"])
    tl = T.tiles[int(c["tile_off"]):int(c["tile_off"]) + int(c["ntiles"])].astype(np.int64)
    a, q = np.meshgrid(np.arange(t), np.arange(t), indexing="ij")
    i = ((tl & 0xFFFF) * t)[:, None, None] + a[None]
    j = ((tl >> 16) * t)[:, None, None] + q[None]
    off = np.arange(len(tl) * t * t)
    i, j = i.ravel(), j.ravel()
    return off, i, j, (i <= j) & (j < n)


def wave_of_pairs(T, item):
    """which of the four wave blocks of an nrep == 4 item each of its pairs goes to: its position in its batch, modulo 4"""
    it = T.items[item]
    c = T.cls[it["cls"]]
    ngu, batch = int(c["ngu"]), int(c["batch"])
    p = np.arange(int(it["p0"]), int(it["p1"]))
    gd, g = p // ngu, p % ngu
    lo = np.where(gd == int(it["p0"]) // ngu, int(it["p0"]) % ngu, 0)
    return ((g - lo) % batch) % 4


def check_block(tag, dev, x, family, P, R, layout, dead_zero=False):
    """dev: one stored block (complex); x[p, n]: the pairs it must hold the sum of.  Exact family: bit for bit.  Rounding family: within
    gamma(2P + R + 2) sum|products| of the long-double sum, P the most pairs one accumulator saw, R the additions on top."""
    off, i, j, live = layout
    i, j, got = i[live], j[live], dev[off[live]]
    if len(x) == 0:
        x = np.zeros((1, int(layout[1].max()) + 1), complex)
    if family == "exact":
        re, im = block_exact(x)
        want = re[i, j].astype(np.float64) + 1j * im[i, j].astype(np.float64)
        bad = np.flatnonzero(got.view(np.int64).reshape(-1, 2) != want.view(np.int64).reshape(-1, 2))[:4] // 2
        assert same_bits(got, want), (tag, "exact family: (i, j, device, reference)", [(int(i[b]), int(j[b]), got[b], want[b]) for b in bad])
    else:
        assert 2 * P + R + 2 <= 1 << 11
        re, im, mre, mim = block_longdouble(x)
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), (tag, "not finite")
        g = np.longdouble(gamma(2 * max(P, 1) + R + 2))
        er, ei = np.abs(got.real.astype(np.longdouble) - re[i, j]), np.abs(got.imag.astype(np.longdouble) - im[i, j])
        br, bi = g * mre[i, j], g * mim[i, j]
        tiny = np.longdouble(1e-300)
        ratio = max(float((er / np.maximum(br, tiny)).max(initial=0)), float((ei / np.maximum(bi, tiny)).max(initial=0)))
        assert (er <= br).all() and (ei <= bi).all(), (tag, "rounding family: error / bound =", ratio)
    if dead_zero:
        d = dev[off[~live]]
        assert (d.real == 0).all() and (d.imag == 0).all(), (tag, "dead elements of the pair kernel are not zero")


def check_item(T, item, partial, src, family):
    """the block(s) of one work item in `partial` (the whole buffer, complex) against the reference"""
    it = T.items[item]
    ci = int(it["cls"])
    kern = T.kernel_of(item)
    layout = block_layout(T, ci)
    sz, o = T.block_elems(ci), int(it["out_off"])
    x = pair_vectors(T, ci, np.arange(int(it["p0"]), int(it["p1"])), src)
    assert np.isfinite(x.real).all() and np.isfinite(x.imag).all(), "the reference itself read a position no table names"
    tag = (T.sec.case.name, "item", item, "kernel", kern)
    if kern == 0:             # one thread's accumulator saw ceil(pairs / PT_THREADS) pairs
        check_block(tag, partial[o:o + sz], x, family, -(-len(x) // PT_THREADS), PAIR_R, layout, True)
    elif int(T.cls[ci]["nrep"]) == 1:
        check_block(tag, partial[o:o + sz], x, family, len(x), 0, layout)
    else:
        w = wave_of_pairs(T, item)
        tot = np.zeros(sz, complex)
        for k in range(4):
            check_block(tag + ("wave", k), partial[o + k * sz:o + (k + 1) * sz], x[w == k], family, int((w == k).sum()), 0, layout)
            tot = tot + partial[o + k * sz:o + (k + 1) * sz]
        check_block(tag + ("sum of the waves",), tot, x, family, int(np.bincount(w, minlength=4).max()), 4, layout)


def item_spans(T, items):
    """[out_off, out_off + ntiles*t*t*nrep) of the given items"""
    return [(int(T.items[k]["out_off"]), int(T.items[k]["out_off"]) + T.block_elems(int(T.items[k]["cls"])) * int(T.cls[T.items[k]["cls"]]["nrep"]))
            for k in items]


def check_untouched(tag, buf, spans, sentinel=SENT):
    """everything of buf outside the spans has the sentinel's bits"""
    keep = np.ones(len(buf), bool)
    for a, b in spans:
        keep[a:b] = False
    assert same_bits(buf[keep], np.full(int(keep.sum()), sentinel)), (tag, "written outside the items' blocks", np.flatnonzero(keep & (buf != sentinel))[:8])


def check_partials(T, items, partial, src, family):
    for k in items:
        check_item(T, k, partial, src, family)
    check_untouched((T.sec.case.name, "partial"), partial, item_spans(T, items))


# ---- bit-for-bit restatements (only additions occur) ---------------------------------------------------------------------------------------
def reduce_restated(partial, el_src, el_cnt, el_stride):
    """pt_reduce_kernel: the partials of an element added in list order onto +0"""
    acc = np.zeros(len(el_src), complex)
    for k in range(int(el_cnt.max(initial=0))):
        m = el_cnt > k
        acc[m] = acc[m] + partial[el_src[m] + k * el_stride[m].astype(np.int64)]
    return acc


def pair_last_stage_restated(wave_sums):
    """the last stage of pt_pair_kernel: v = 0, then the waves' sums 0, 1, 2, 3 in that order"""
    v = 0.0
    for w in wave_sums:
        v = v + w
    return v


def scatter_restated(T, raw, weight, accumulate, rho):
    """The host scatter on rho[4^nsub, 4^nsub] (complex; element (io, jo) at rho[jo, io], as the engine stores 2*(io + nn*jo)): weight * v
    rounded, then added; the lower triangle by conjugation; the diagonal's imaginary part zero."""
    nsub = int(T.sec.words[0])
    if not accumulate:
        rho[:] = 0
    for ci in range(len(T.cls)):
        c = T.cls[ci]
        au, ad = T.configs(ci)
        off, i, j, live = block_layout(T, ci)
        o = int(T.cls_out_off[ci])
        du = int(c["du"])
        for e in np.flatnonzero(live):
            v = raw[o + off[e]]
            ii, jj = int(i[e]), int(j[e])
            re = np.float64(weight) * np.float64(v.real)
            im = np.float64(0.0) if ii == jj else np.float64(weight) * np.float64(v.imag)
            io = int(au[ii % du]) + (int(ad[ii // du]) << nsub)
            jo = int(au[jj % du]) + (int(ad[jj // du]) << nsub)
            rho[jo, io] = complex(rho[jo, io].real + re, rho[jo, io].imag + im)
            if ii != jj:
                rho[io, jo] = complex(rho[io, jo].real + re, rho[io, jo].imag - im)
    return rho


def dense_partial_trace(sec, src):
    """rho of the kept orbitals straight from the amplitudes and the groups' MEANING, no table involved: member m of a group of k traced
    particles carries the m-th kept configuration (ascending) with n_spin - k particles; rho[jo, io] = sum over (up group, dw group) of
    psi(a_u, a_d) conj(psi(b_u, b_d)), io = a_u + (a_d << nsub), jo likewise for b.  Exact family: int64 parts -> (re, im)."""
    case = sec.case
    nsub, nn = case.nsub, 1 << case.nsub

    def members(groups, n_spin, d_of):
        env, conf, word = [], [], []
        e = 0
        for k, w in enumerate(groups):
            d = d_of(k)
            if d == 0 or len(w) == 0:
                continue
            confs = [a for a in range(nn) if bin(a).count("1") == n_spin - k]
            for g in range(len(w) // d):
                for m in range(d):
                    env.append(e)
                    conf.append(confs[m])
                    word.append(w[g * d + m])
                e += 1
        return np.array(env), np.array(conf), np.array(word, dtype=np.uint32), e

    eu, cu, wu, neu = members(sec.up, case.nup, case.du)
    ed, cd, wd, ned = members(sec.dw, case.ndw, case.dd)
    assert case.nranks == 1
    s = 1 - 2 * ((wu[:, None] ^ wd[None, :]) >> np.uint32(31)).astype(np.int64)
    amp = src[(wd & MASK).astype(np.int64)[None, :] * sec.pitch + (wu & MASK).astype(np.int64)[:, None]]
    pr = np.zeros((neu, ned, nn * nn), np.int64)
    pi = np.zeros((neu, ned, nn * nn), np.int64)
    orb = cu[:, None] + (cd[None, :] << nsub)
    E, D = np.broadcast_to(eu[:, None], orb.shape), np.broadcast_to(ed[None, :], orb.shape)
    pr[E, D, orb] = np.rint(amp.real).astype(np.int64) * s
    pi[E, D, orb] = np.rint(amp.imag).astype(np.int64) * s
    pr, pi = pr.reshape(-1, nn * nn), pi.reshape(-1, nn * nn)
    # [io, jo] = sum psi_io conj(psi_jo); stored at [jo, io]
    re = pr.T @ pr + pi.T @ pi
    im = pi.T @ pr - pr.T @ pi
    return re.T, im.T


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _pair_cases():
    shapes = {"1x1": (1, 0, 0), "2x1": (2, 1, 0), "1x2": (2, 0, 1), "3x1": (3, 1, 0), "1x3": (3, 0, 1), "4x1": (4, 1, 0), "1x4": (4, 0, 1), "2x2": (2, 1, 1)}
    sizes = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (4, 257), 600: (48, 50)}   # 257, 600: four items of that many
    out = []
    for name, (nsub, nup, ndw) in shapes.items():
        for npairs, (gu, gd) in sizes.items():
            if name in ("1x1", "2x2", "3x1") or npairs in (257, 600):
                out.append(Case(f"pair-{name}-{npairs}", nsub, nup, ndw, (gu,), (gd,)))
    return out


PAIR_CASES = _pair_cases()
TILE_CASES = [
    # <2,1>
    Case("t2-3x3-nrep4-long", 3, 1, 1, (500,), (13,)),                 # batch 225: three batches a group, staging in three rounds
    Case("t2-5x5", 5, 1, 1, (170,), (7,)),                             # n odd, 91 tiles, dd = 5
    Case("t2-1x15-nrep4", 6, 0, 2, (300,), (5,)),                      # du = 1
    Case("t2-6x6-171tiles", 6, 1, 1, (120,), (9,)),                    # waves partly idle, padded stride, dd = 6
    Case("t2-3x3-bc1", 3, 1, 1, (1,), (6,)),
    Case("t2-3x3-bc2", 3, 1, 1, (2,), (6,)),
    Case("t2-3x3-bc3", 3, 1, 1, (3,), (6,)),
    Case("t2-3x3-bc5", 3, 1, 1, (5,), (6,)),
    Case("t2-3x3-bc8", 3, 1, 1, (8,), (6,)),
    Case("t2-4x4-nrep4-ncu2", 4, 1, 1, (37,), (11,), ncu=2),
    Case("t2-small0-n1-n3", 3, 1, 1, (7, 29), (5, 23), small_n=0),     # HXV_RDM_PAIR_KERNEL=0: 3 x 1, 1 x 3 and 1 x 1 in the tile kernel
    Case("t2-small0-n1-n3-ncu4", 3, 1, 1, (7, 29), (5, 23), small_n=0, ncu=4),
    # <4,2>
    Case("t4-10x10", 5, 2, 2, (47,), (7,)),                            # n = 100: 69 threads own a second tile
    Case("t4-5x10", 5, 1, 2, (90,), (5,)),                             # n = 50: no second tile
    Case("t4-7x7", 7, 1, 1, (90,), (5,)),                              # n = 49, n % 4 == 1
    Case("t4-20x6", 6, 3, 1, (40,), (6,)),                             # n = 120
    Case("t4-10x10-ncu3", 5, 2, 2, (23,), (9,), ncu=3),
    Case("t4-10x5", 5, 2, 1, (60,), (6,)),
]
SIGN_CASES = [
    (Case("signs-large", 5, 1, 2, (45, 50), (4, 30), signs="none"), Case("signs-large", 5, 1, 2, (45, 50), (4, 30), signs="all")),
    (Case("signs-small", 3, 1, 1, (40, 300), (6, 23), signs="none"), Case("signs-small", 3, 1, 1, (40, 300), (6, 23), signs="all")),
]
SPLIT_CASES = [Case(f"split-rank{r}", 3, 1, 1, (40, 300), (6, 23), nranks=3, rank=r) for r in range(3)] + [
    Case("split-starved-rank2", 3, 1, 1, (40, 300), (6, 23), nranks=3, rank=2, cols="by_k"),
    Case("split-t4-rank1", 5, 2, 2, (30,), (8,), nranks=3, rank=1)]
CHAIN_CASES = [Case(f"chain-ncu{n}", 4, 2, 2, (3, 5, 4), (2, 4, 3), ncu=n) for n in (1, 256)]
REFUSED_CASE = Case("refused-15x15", 6, 2, 2, (2,), (2,))
KERNEL_CASES = PAIR_CASES + TILE_CASES + SPLIT_CASES + [a for a, _ in SIGN_CASES] + CHAIN_CASES
REDUCE_NEL = [1, 255, 256, 257, 1000]
REDUCE_CNT = [0, 1, 2, 37]


def reduce_tables(nel, seed):
    """Hand-made tables for pt_reduce_kernel: element e has cnt = REDUCE_CNT[e % 4] partials a stride of nel + 3 apart (larger than the
    block of nel elements, NaN between); partial holds NaN wherever no (e, k) points.  -> partial, el_src, el_cnt, el_stride"""
    rng = np.random.default_rng([seed, nel])
    cnt = np.array([REDUCE_CNT[(e + seed) % len(REDUCE_CNT)] for e in range(nel)], dtype=np.int32)
    stride = np.full(nel, nel + 3, dtype=np.int32)
    src = (7 + np.arange(nel)).astype(np.int64)
    partial = np.full(7 + (nel + 3) * max(REDUCE_CNT) + 5, CNAN)
    for e in range(nel):
        idx = src[e] + np.arange(cnt[e]) * int(stride[e])
        partial[idx] = rng.standard_normal(cnt[e]) + 1j * rng.standard_normal(cnt[e])
    return partial, src, cnt, stride
