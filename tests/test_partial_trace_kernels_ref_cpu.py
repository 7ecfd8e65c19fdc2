"""The cases of tests/partial_trace_kernels_ref.py reach the paths they are there for, and its checks bite (no GPU, no kernel).

REACH.  pt_build (through the host-only library of tests/host/partial_trace_build.cpp; the HIP launcher library is not loaded here) cuts the
tables of the very case list tests/test_gpu_partial_trace_kernels.py runs, and `reach` computes from items / cls what an item makes its
kernel do: batches per dw group and whether the last is partial, dw groups spanned, staging rounds, padded stride, live second tiles, idle
waves, the bc values of the four-wave classes, pairs per pair-kernel item, ...  Every path the GPU file is there for must be reached by at
least one case: a later change of pt_build's policy cannot silently empty a family.

BITE.  A numpy emulation of each kernel that reads the tables THE WAY THE KERNEL DOES (thread and wave ownership, the LDS image, batches,
lo / hi, clamped loads) is fed to the same check functions the device's output is fed to and must pass in both input families; then one
named mistake at a time is switched on and the same checks must refuse it, in each family it affects.  The emulation also records every
position of src it loads: a load outside the positions the item's own groups name is refused (on the device such a load shows as NaN in the
result where it is used, and is harmless only where it is discarded)."""
import ctypes as C

import numpy as np
import pytest

import partial_trace_kernels_ref as R

FAMILIES = ["exact", "rounding"]


@pytest.fixture(scope="session")
def ptb(built):
    return R.bind(C.CDLL(str(built.build_partial_trace_build())))


def tables(ptb, case):
    T = R.Tables(ptb, R.make_sector(case))
    R.check_table_bounds(T)
    return T


def refuses(fn, *a, **k):
    with pytest.raises((AssertionError, IndexError)):
        fn(*a, **k)


# ---- the emulations ------------------------------------------------------------------------------------------------------------------------
class Loads:
    """every position of src an emulated kernel loads, and what the item's groups allow"""

    def __init__(self):
        self.pos = []

    def __call__(self, src, pos):
        self.pos.append(np.atleast_1d(np.asarray(pos, dtype=np.int64)).ravel())
        return src[pos]

    def check(self, T, item):
        it = T.items[item]
        c = T.cls[it["cls"]]
        ngu, du, dd = int(c["ngu"]), int(c["du"]), int(c["dd"])
        gd0, gd1 = int(it["p0"]) // ngu, (int(it["p1"]) - 1) // ngu
        sl = (T.cols[c["cols_off"] + gd0 * dd:c["cols_off"] + (gd1 + 1) * dd] & R.MASK).astype(np.int64)
        rw = (T.rows[c["rows_off"]:c["rows_off"] + ngu * du] & R.MASK).astype(np.int64)
        allowed = (sl[:, None] * T.sec.pitch + rw[None, :]).ravel()
        got = np.unique(np.concatenate(self.pos)) if self.pos else np.zeros(0, np.int64)
        assert np.isin(got, allowed).all(), (T.sec.case.name, item, "a load outside the item's groups")


def emu_pair(T, item, src, partial, mut=None, loads=None):
    loads = loads or Loads()
    it = T.items[item]
    c = T.cls[it["cls"]]
    N, n, du, dd, ngu = R.PT_PAIR_N, int(c["n"]), int(c["du"]), int(c["dd"]), int(c["ngu"])
    crow, ccol = T.rows[c["rows_off"]:], T.cols[c["cols_off"]:]
    p0, p1 = int(it["p0"]), int(it["p1"])
    tid = np.arange(R.PT_THREADS)
    acc = np.zeros((R.PT_THREADS, N, N), complex)
    for base in range(p0, p1, R.PT_THREADS):
        p = base + tid
        act = p < (p1 - 1 if mut == "guard_off_by_one" else p1)
        p = p[act]
        gd = p // ngu
        g = p - gd * ngu
        x = np.zeros((len(p), N), complex)
        for k in range(N):
            kk = min(k, n - 1)
            a, b = (kk // du, kk % du) if mut == "divmod_exchanged" else (kk % du, kk // du)
            r, cc = crow[g * du + a], ccol[gd * dd + b]
            sg = (r >> 31) if mut == "sign_row_only" else ((r ^ cc) >> 31)
            f = np.where(sg == 1, -1.0, 1.0) if k < n else 0.0
            x[:, k] = f * loads(src, (cc & R.MASK).astype(np.int64) * T.sec.pitch + (r & R.MASK).astype(np.int64))
        upd = (np.conj(x)[:, :, None] * x[:, None, :]) if mut == "conj_wrong_factor" else (x[:, :, None] * np.conj(x)[:, None, :])
        acc[tid[act]] += upd
    red = np.zeros((4, N, N), complex)
    for w in range(4):
        v = acc[64 * w:64 * w + 64].copy()
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ m]
        red[w] = v[0]
    for t in range(min(int(c["ntiles"]) * 4, R.PT_THREADS)):
        pk = int(T.tiles[c["tile_off"] + (t >> 2)])
        i, j = (pk & 0xFFFF) * 2 + ((t >> 1) & 1), (pk >> 16) * 2 + (t & 1)
        v = 0j
        if i <= j < N:
            for w in range(4):
                v = v + red[w][i, j]
        partial[int(it["out_off"]) + t] = v
    return loads


def emu_tile(T, item, src, partial, mut=None, loads=None):
    loads = loads or Loads()
    it = T.items[item]
    c = T.cls[it["cls"]]
    Tt, NT = (2, 1) if T.kernel_of(item) == 1 else (4, 2)
    assert Tt == c["t"]
    n, du, dd, ngu, batch, stride, nrep, ntiles = (int(c[f]) for f in ("n", "du", "dd", "ngu", "batch", "stride", "nrep", "ntiles"))
    crow, ccol = T.rows[c["rows_off"]:], T.cols[c["cols_off"]:]
    # tiles by owner: thread (tid & 63 of every wave, or tid) + t * PT_THREADS
    owned = ntiles if mut != "second_tile_never" else min(ntiles, R.PT_THREADS)
    tl = T.tiles[c["tile_off"]:c["tile_off"] + ntiles].astype(np.int64)
    a = np.arange(Tt)
    i = np.minimum((tl & 0xFFFF)[:, None] * Tt + a[None, :], n - 1)
    j = np.minimum((tl >> 16)[:, None] * Tt + a[None, :], n - 1)
    st_off = batch * du if mut == "stride_unpadded" else stride
    offi, offj = (i // du) * st_off + i % du, (j // du) * st_off + j % du
    nw = nrep if nrep > 1 else 1
    acc = np.zeros((nw, ntiles, Tt, Tt), complex)
    xs = np.full(R.PT_XS, R.CNAN)
    p0, p1 = int(it["p0"]), int(it["p1"])
    gd0, gd1 = p0 // ngu, (p1 - 1) // ngu
    for gd in range(gd0, gd1 + 1):
        if mut == "middle_group_skipped" and gd0 < gd < gd1:
            continue
        first, last = (gd == gd1, gd == gd0) if mut == "lo_hi_exchanged" else (gd == gd0, gd == gd1)
        lo = p0 - gd0 * ngu if first else 0
        hi = p1 - gd1 * ngu if last else ngu
        for g0 in range(lo, hi, batch):
            bc = min(batch, hi - g0)
            if mut == "partial_batch_skipped" and bc < batch and g0 > lo:
                continue
            nk = bc * du
            k = np.arange(nk)
            r = crow[g0 * du + k]
            row = (r & R.MASK).astype(np.int64)
            for id0 in range(0, dd, R.PT_LOADS):
                for u in range(R.PT_LOADS):
                    cc = ccol[gd * dd + min(id0 + u, dd if mut == "clamp_dd" else dd - 1)]
                    x = loads(src, int(cc & R.MASK) * T.sec.pitch + row)
                    if id0 + u < dd:
                        f = np.where(((r ^ cc) >> 31) == 1, -1.0, 1.0)
                        xs[(id0 + u) * stride + k] = f * x
            for w in range(nw):
                step = 1 if mut == "waves_stride_one" else nw
                for b in range(w, bc, step):
                    o = 0 if mut == "o_dropped" else b * du
                    xi, xj = xs[offi[:owned] + o], xs[offj[:owned] + o]
                    acc[w, :owned] += xi[:, :, None] * np.conj(xj)[:, None, :]
    sz = ntiles * Tt * Tt
    written = ntiles if mut not in ("second_tile_index_off",) else min(ntiles, R.PT_THREADS)
    for w in range(nw):
        o = int(it["out_off"]) + (0 if mut == "wave_offset_missing" else w * sz)
        partial[o:o + written * Tt * Tt] = acc[w, :written].reshape(-1)
    return loads


def emu_reduce(partial, el_src, el_cnt, el_stride, mut=None):
    out = np.zeros(len(el_src), complex)
    for e in range(len(el_src)):
        n = int(el_cnt[e]) - (1 if mut == "one_early" and el_cnt[e] > 0 else 0)
        st = int(el_cnt[e]) if mut == "cnt_as_stride" else int(el_stride[e])
        acc = 0j
        for k in range(n):
            acc = acc + partial[(int(el_src[e]) + k * st) % len(partial)]      # (a mistaken stride may leave the buffer: wrapped)
        out[e] = acc
    return out


def emu_scatter(T, raw, weight, accumulate, rho, mut=None):
    nsub = int(T.sec.words[0])
    if not accumulate:
        rho[:] = 0
    ld = np.longdouble
    for ci in range(len(T.cls)):
        c = T.cls[ci]
        au, ad = T.configs(ci)
        t, du, n = int(c["t"]), int(c["du"]), int(c["n"])
        for tile in range(int(c["ntiles"])):
            pk = int(T.tiles[c["tile_off"] + tile])
            for a in range(t):
                for q in range(t):
                    i, j = (pk & 0xFFFF) * t + a, (pk >> 16) * t + q
                    if i > j or j >= n:
                        continue
                    v = raw[int(T.cls_out_off[ci]) + tile * t * t + a * t + q]
                    io, jo = int(au[i % du]) + (int(ad[i // du]) << nsub), int(au[j % du]) + (int(ad[j // du]) << nsub)

                    def add(old, x, sign):      # old + sign * weight * x: the product rounded first, or (the mistake) fused
                        if mut == "unrounded_product":
                            return float(ld(old) + ld(sign) * ld(weight) * ld(x))
                        return old + sign * (np.float64(weight) * np.float64(x))

                    s_up, s_lo = (-1.0, 1.0) if mut == "conj_upper" else (1.0, -1.0)
                    re = add(rho[jo, io].real, v.real, 1.0)
                    im = rho[jo, io].imag + 0.0 if i == j else add(rho[jo, io].imag, v.imag, s_up)
                    rho[jo, io] = complex(re, im)
                    if i != j:
                        rho[io, jo] = complex(add(rho[io, jo].real, v.real, 1.0), add(rho[io, jo].imag, v.imag, s_lo))
    return rho


def emulate(T, src, mut=None, items=None):
    """the partial buffer (sentinel-filled, with a guard) after the emulated kernels ran on the given items"""
    partial = np.full(T.partial_elems + 64, R.SENT)
    for k in (range(len(T.items)) if items is None else items):
        loads = (emu_pair if T.kernel_of(k) == 0 else emu_tile)(T, k, src, partial, mut)
        loads.check(T, k)
    return partial


# ---- reach ---------------------------------------------------------------------------------------------------------------------------------
def reach(T):
    """the paths the items of these tables make their kernels take, as a set of names"""
    out = set()
    for k, it in enumerate(T.items):
        c = T.cls[it["cls"]]
        kern = T.kernel_of(k)
        n, du, dd, ngu, batch, stride, nrep, ntiles = (int(c[f]) for f in ("n", "du", "dd", "ngu", "batch", "stride", "nrep", "ntiles"))
        p0, p1 = int(it["p0"]), int(it["p1"])
        gd0, gd1 = p0 // ngu, (p1 - 1) // ngu
        spans = gd1 - gd0 + 1
        if kern == 0:
            out |= {f"pair:{du}x{dd}", f"pair:pairs={p1 - p0}"}
            if spans > 1:
                out.add("pair:spans-dw-groups")
            if T.sec.case.nranks > 1:
                out.add("pair:split")
            continue
        K = "t2" if kern == 1 else "t4"
        out.add(f"{K}:n={n}")
        if n % 2 == 1:
            out.add(f"{K}:n-odd")
        if T.sec.case.nranks > 1:
            out.add(f"{K}:split")
        if T.sec.case.small_n == 0 and n <= R.PT_PAIR_N:
            out.add(f"{K}:small_n=0:n={n}")
        if spans >= 3 and p0 % ngu != 0 and p1 % ngu != 0:
            out.add(f"{K}:three-groups-mid-to-mid")
        if stride > batch * du:
            out.add(f"{K}:padded-stride")
        if dd % R.PT_LOADS and dd > R.PT_LOADS:
            out.add(f"{K}:dd-ragged")
        if kern == 2:
            out.add("t4:second-tiles" if ntiles > R.PT_THREADS else "t4:no-second-tile")
        if nrep == 1 and ntiles < R.PT_THREADS and ntiles % 64:
            out.add(f"{K}:nrep1-idle-lanes")
        if nrep == 1 and 192 >= ntiles:
            out.add(f"{K}:nrep1-idle-wave")
        for gd in range(gd0, gd1 + 1):
            lo = p0 - gd0 * ngu if gd == gd0 else 0
            hi = p1 - gd1 * ngu if gd == gd1 else ngu
            nb = -(-(hi - lo) // batch)
            if nb >= 3 and (hi - lo) % batch:
                out.add(f"{K}:three-batches-last-partial")
            for g0 in range(lo, hi, batch):
                bc = min(batch, hi - g0)
                if bc > 1:
                    out.add(f"{K}:several-pairs-staged")
                if bc * du > R.PT_THREADS:
                    out.add(f"{K}:staging-rounds")
                if nrep == 4:
                    out.add(f"{K}:nrep4:bc={bc}" if bc in (1, 2, 3, 5) else f"{K}:nrep4:bc%4={bc % 4}")
    if (T.cls_ngd == 0).any() and T.sec.case.nranks > 1:
        out.add("split:class-without-dw-group")
    return out


WANTED = (
    [f"{K}:{p}" for K in ("t2", "t4") for p in ("three-batches-last-partial", "three-groups-mid-to-mid", "staging-rounds", "padded-stride",
                                                "dd-ragged", "several-pairs-staged")]
    + ["t2:n=9", "t2:n=15", "t2:n=25", "t2:n-odd", "t2:small_n=0:n=1", "t2:small_n=0:n=3", "t2:nrep4:bc=1", "t2:nrep4:bc=2", "t2:nrep4:bc=3",
       "t2:nrep4:bc=5", "t2:nrep4:bc%4=0", "t2:nrep1-idle-lanes", "t2:n=36", "t2:split"]
    + ["t4:n=100", "t4:n=50", "t4:n=49", "t4:n=120", "t4:second-tiles", "t4:no-second-tile", "t4:split"]
    + [f"pair:{s}" for s in ("1x1", "2x1", "1x2", "3x1", "1x3", "4x1", "1x4", "2x2")]
    + [f"pair:pairs={p}" for p in (1, 63, 64, 65, 255, 256, 257, 600)] + ["pair:spans-dw-groups", "pair:split", "split:class-without-dw-group"])


@pytest.fixture(scope="session")
def reached(ptb):
    per_case = {c.name: reach(tables(ptb, c)) for c in R.KERNEL_CASES}
    return per_case, set().union(*per_case.values())


def test_every_path_is_reached(reached):
    per_case, every = reached
    missing = [w for w in WANTED if w not in every]
    assert not missing, missing
    # 257 pairs in ONE item (a second trip of the pair loop with one live thread), across dw groups of four pairs
    assert {"pair:pairs=257", "pair:spans-dw-groups"} <= per_case["pair-2x2-257"] and "pair:pairs=256" in per_case["pair-2x2-256"]
    # the paths of one kernel come together in single cases, not spread one by one
    assert {"t4:three-batches-last-partial", "t4:three-groups-mid-to-mid", "t4:padded-stride", "t4:second-tiles"} <= per_case["t4-10x10"]
    assert {"t4:staging-rounds", "t4:three-batches-last-partial"} <= per_case["t4-20x6"] and "t4:staging-rounds" in per_case["t4-7x7"]
    assert {"t2:three-batches-last-partial", "t2:three-groups-mid-to-mid", "t2:staging-rounds"} <= per_case["t2-3x3-nrep4-long"]
    assert {"t2:padded-stride", "t2:nrep1-idle-lanes", "t2:three-batches-last-partial"} <= per_case["t2-6x6-171tiles"]


def test_sign_cases_hold_all_four_combinations_in_one_block(ptb):
    """mixed signs: some pair of every tile case has rows with and without the bit and columns with and without it; the sign cases differ in
    nothing but the bits"""
    for case in R.TILE_CASES:
        T = tables(ptb, case)
        c = T.cls[int(np.argmax(T.cls["n"]))]
        if c["du"] < 2 or c["dd"] < 2:
            continue
        rb = (T.rows[c["rows_off"]:c["rows_off"] + c["ngu"] * c["du"]] >> 31).reshape(-1, c["du"])
        cb = (T.cols[c["cols_off"]:c["cols_off"] + int(T.cls_ngd[np.argmax(T.cls["n"])]) * c["dd"]] >> 31).reshape(-1, c["dd"])
        mixed = lambda m: ((m.min(axis=1) == 0) & (m.max(axis=1) == 1)).any()          # noqa: E731
        assert mixed(rb) and mixed(cb), case.name
    for none, every in R.SIGN_CASES:
        a, b = tables(ptb, none), tables(ptb, every)
        assert R.same_bits(a.rows & R.MASK, b.rows & R.MASK) and R.same_bits(a.cols & R.MASK, b.cols & R.MASK)
        assert (a.rows >> 31).max() == 0 and (a.cols >> 31).max() == 0 and (b.rows >> 31).min() == 1 and (b.cols >> 31).min() == 1


def test_builder_refuses_a_class_beyond_the_register_tiles(ptb):
    with pytest.raises(R.BuildError, match="synthetic sector: a class block exceeds the register tiles"):
        R.Tables(ptb, R.make_sector(R.REFUSED_CASE))


# ---- the checks accept the kernels' order ... ------------------------------------------------------------------------------------------------
ACCEPT = [c for c in R.KERNEL_CASES if c.name in (
    "pair-1x1-257", "pair-2x1-257", "pair-1x2-257", "pair-3x1-65", "pair-1x3-257", "pair-4x1-257", "pair-1x4-257", "pair-2x2-600", "pair-2x2-63",
    "t2-3x3-nrep4-long", "t2-5x5", "t2-1x15-nrep4", "t2-6x6-171tiles", "t2-3x3-bc3", "t2-3x3-bc5", "t2-small0-n1-n3", "t4-10x10", "t4-5x10",
    "t4-7x7", "t4-20x6", "split-rank1", "split-starved-rank2", "split-t4-rank1", "chain-ncu1", "chain-ncu256")]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ACCEPT, ids=lambda c: c.name)
def test_checks_accept_the_emulation(ptb, case, family):
    T = tables(ptb, case)
    src = R.make_src(T, family)
    partial = emulate(T, src)
    R.check_partials(T, range(len(T.items)), partial, src, family)
    out = emu_reduce(partial, T.el_src, T.el_cnt, T.el_stride)
    assert R.same_bits(out, R.reduce_restated(partial, T.el_src, T.el_cnt, T.el_stride))


# ---- ... and refuse the named mistakes -----------------------------------------------------------------------------------------------------
TILE_MISTAKES = {
    # mistake: the cases it is switched on in (each reaches the path the mistake is on)
    "stride_unpadded": ["t2-6x6-171tiles", "t4-10x10"],
    "o_dropped": ["t2-5x5", "t4-5x10"],
    "partial_batch_skipped": ["t2-3x3-nrep4-long", "t4-10x10"],
    "lo_hi_exchanged": ["t2-6x6-171tiles", "t4-10x10"],
    "middle_group_skipped": ["t2-3x3-nrep4-long", "t4-10x10"],
    "wave_offset_missing": ["t2-3x3-bc5", "t2-1x15-nrep4"],
    "waves_stride_one": ["t2-3x3-bc5", "t2-1x15-nrep4"],
    "second_tile_never": ["t4-10x10", "t4-20x6"],
    "second_tile_index_off": ["t4-10x10", "t4-20x6"],
    "clamp_dd": ["t2-5x5", "t4-5x10"],
}
PAIR_MISTAKES = {
    "sign_row_only": ["pair-2x2-63", "pair-1x3-257"],
    "conj_wrong_factor": ["pair-2x2-63", "pair-3x1-65"],
    "divmod_exchanged": ["pair-2x2-63", "pair-1x3-257", "pair-3x1-65"],
    "guard_off_by_one": ["pair-2x2-63", "pair-1x1-257", "pair-2x2-600"],
}


def by_name(name):
    return next(c for c in R.KERNEL_CASES if c.name == name)


def refused_in(T, family, mut):
    src = R.make_src(T, family)

    def run():
        R.check_partials(T, range(len(T.items)), emulate(T, src, mut), src, family)

    refuses(run)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mut,name", [(m, n) for d in (TILE_MISTAKES, PAIR_MISTAKES) for m, ns in d.items() for n in ns])
def test_checks_refuse_a_kernel_mistake(ptb, mut, name, family):
    refused_in(tables(ptb, by_name(name)), family, mut)


@pytest.mark.parametrize("family", FAMILIES)
def test_checks_refuse_tile_sign_and_conjugate_mistakes(ptb, family):
    """the same two mistakes in the tile kernel's text, made on the emulation's output: conj(block) and a block without the column signs"""
    T = tables(ptb, by_name("t2-5x5"))
    src = R.make_src(T, family)
    good = emulate(T, src)
    R.check_partials(T, range(len(T.items)), good, src, family)
    refuses(R.check_partials, T, range(len(T.items)), np.where(good == R.SENT, good, np.conj(good)), src, family)
    flipped = T.cols.copy()
    T.cols &= R.MASK                              # (the emulation reads no column sign; the reference reads them again below)
    bad = emulate(T, src)
    T.cols[:] = flipped
    refuses(R.check_partials, T, range(len(T.items)), bad, src, family)


def test_checks_refuse_a_write_outside_the_blocks(ptb):
    T = tables(ptb, by_name("t2-3x3-bc3"))
    src = R.make_src(T, "exact")
    p = emulate(T, src)
    p[T.partial_elems] = 0
    refuses(R.check_partials, T, range(len(T.items)), p, src, "exact")
    p = emulate(T, src, items=range(1, len(T.items)))
    refuses(R.check_partials, T, range(len(T.items)), p, src, "exact")          # an item that never ran leaves the sentinel


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("nel", R.REDUCE_NEL)
def test_reduce_restatement_and_its_mistakes(nel, seed):
    partial, src, cnt, stride = R.reduce_tables(nel, seed)
    want = R.reduce_restated(partial, src, cnt, stride)
    assert R.same_bits(emu_reduce(partial, src, cnt, stride), want) and np.isfinite(want.real).all() and (want[cnt == 0] == 0).all()
    assert set(cnt) == set(R.REDUCE_CNT) or nel == 1
    for mut in ("one_early", "cnt_as_stride"):
        if (cnt > (1 if mut == "cnt_as_stride" else 0)).any():
            assert not R.same_bits(emu_reduce(partial, src, cnt, stride, mut), want), mut
    # list order matters in the last bit somewhere at cnt = 37
    if nel >= 255:
        rev = np.array([sum(partial[src[e] + k * stride[e]] for k in reversed(range(cnt[e]))) if cnt[e] else 0j for e in range(nel)])
        assert not R.same_bits(rev, want)


def test_pair_last_stage_restatement():
    assert R.pair_last_stage_restated([1.0, 2.0 ** -53, 2.0 ** -53, 0.0]) == 1.0
    assert R.pair_last_stage_restated([2.0 ** -53, 2.0 ** -53, 1.0, 0.0]) == 1.0 + 2.0 ** -52


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_and_scatter(ptb, case):
    """the emulated chain against the dense partial trace (exact family, bit for bit after a power-of-two weight); scatter's restatement
    accepts the emulation of the host routine's loops and refuses its two mistakes"""
    T = tables(ptb, case)
    nn = 1 << (2 * case.nsub)
    src = R.make_src(T, "exact", 5)
    raw = R.reduce_restated(emulate(T, src), T.el_src, T.el_cnt, T.el_stride)
    rho = emu_scatter(T, raw, 0.25, False, np.full((nn, nn), R.SENT))
    re, im = R.dense_partial_trace(T.sec, src)
    assert R.same_bits(rho, 0.25 * re.astype(np.float64) + 1j * (0.25 * im.astype(np.float64)))
    assert R.same_bits(rho, R.scatter_restated(T, raw, 0.25, False, np.full((nn, nn), R.SENT)))
    src2 = R.make_src(T, "rounding", 6)
    raw2 = R.reduce_restated(emulate(T, src2), T.el_src, T.el_cnt, T.el_stride)
    first = R.scatter_restated(T, raw2, 0.3, False, np.full((nn, nn), R.SENT))      # (of the second's magnitude: a fused product shows)
    second = R.scatter_restated(T, raw2, 0.7, False, np.full((nn, nn), R.SENT))
    both = R.scatter_restated(T, raw2, 0.7, True, first.copy())
    assert R.same_bits(both + 0.0, first + second)
    assert R.same_bits(emu_scatter(T, raw2, 0.7, True, first.copy()), both)
    assert not R.same_bits(emu_scatter(T, raw2, 0.7, True, first.copy(), "unrounded_product"), both)
    assert not R.same_bits(emu_scatter(T, raw2, 0.7, False, first.copy(), "conj_upper"), second)
    # a dropped class shows in the dense comparison
    raw_bad = raw.copy()
    raw_bad[int(T.cls_out_off[len(T.cls) - 1])] += 1
    assert not R.same_bits(R.scatter_restated(T, raw_bad, 0.25, False, np.full((nn, nn), R.SENT)), rho)
