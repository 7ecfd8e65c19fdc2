"""The kernels of the partial-trace engine, one by one (csrc/hxv_partial_trace_kernels.hpp through the test-only launchers of
tests/device/partial_trace_kernels_check.hip; references, bounds, restatements and the case list: tests/partial_trace_kernels_ref.py, which
tests/test_partial_trace_kernels_ref_cpu.py shows to bite and to reach the paths named below).

The density-matrix tests reach these kernels only through the tables pt_build cuts for their sectors on a 256-CU device, where a work item
holds one pair or a few.  Here pt_build runs on SYNTHETIC sectors (any number of groups of any class shape) with ncu of 1 to 4, so that an
item has several batches with a partial last one, spans dw groups, stages in several rounds, uses a padded LDS stride, owns a second tile,
shares a batch among four waves -- and each kernel is launched alone on its slice of the work list.  Every case, in two input families
(EXACT: integer parts in [-8, 8], the device block equals the integer sum bit for bit; ROUNDING: normalised normals against long double,
within gamma(2P + R + 2) sum|products|, derived in the reference file before the first run and not touched since):
  - src holds NaN in the pad rows, in every column slot no dw group of the rank names and in a guard behind the buffer;
  - partial and out start as a sentinel; every element scatter would read is as referenced, everything outside the items' blocks (a guard
    behind the buffer included) keeps the sentinel's bits, the pair kernel's dead elements are zero;
  - the kernels run twice on fresh buffers and give identical bits;
  - pt_reduce_kernel then runs on the device's partials: bit for bit the list-order sum, and as referenced for the class as a whole.
Further: all-signs-set against no-sign-set (same bits), rank r of 3 on the gathered layout with a rank that owns no dw group of a class,
pt_reduce_kernel on hand-made tables (cnt = 0, stride larger than the block), the wave order of the pair kernel's last stage, the whole
chain with the host scatter against the dense partial trace taken straight from the amplitudes, the launchers' and the builder's refusals.
Wall time of the file on an MI355X: 153 cases in 2.5 s once the libraries are built (no case above 0.25 s)."""
import ctypes as C

import numpy as np
import pytest

import partial_trace_kernels_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FAMILIES = ["exact", "rounding"]
BAD = 1                                      # hipErrorInvalidValue


@pytest.fixture(scope="session")
def ptc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = R.bind(C.CDLL(str(built.build_partial_trace_kernels_check())))
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.ptc_constants.argtypes = [C.POINTER(C.c_int)]
    L.ptc_constants.restype = None
    L.ptc_upload.argtypes = [vp]
    for f in (L.ptc_pair, L.ptc_tile_2_1, L.ptc_tile_4_2):
        f.argtypes = [vp, i32, i32, vp, i32, vp]
    L.ptc_reduce.argtypes = [vp, vp, vp]
    L.ptc_reduce_tables.argtypes = [vp, vp, vp, vp, i64, vp]
    L.ptc_scatter.argtypes = [vp, vp, dbl, i32, vp]
    return L


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    import torch

    return torch.full((n,), R.SENT, dtype=torch.complex128, device="cuda")


def tables(ptc, case):
    sec = R.make_sector(case)
    T = R.Tables(ptc, sec)
    R.check_table_bounds(T)                  # before anything is launched on them
    assert ptc.ptc_upload(T.handle) == 0
    return T


def run_kernels(ptc, T, src):
    """each accumulating kernel alone on its part of the work list, onto one sentinel-filled partial buffer -> (host copy, device buffer)"""
    assert len(src) == (T.sec.nslots + 1) * T.sec.pitch
    s, p = dev(src), sentinel(T.partial_elems + GUARD)
    for k, f in enumerate((ptc.ptc_pair, ptc.ptc_tile_2_1, ptc.ptc_tile_4_2)):
        if T.nitems[k]:
            assert f(T.handle, 0, T.nitems[k], s.data_ptr(), T.sec.pitch, p.data_ptr()) == 0, (T.sec.case.name, k)
    return p.cpu().numpy(), p


def run_reduce(ptc, T, partial_d):
    o = sentinel(T.out_elems + GUARD)
    assert ptc.ptc_reduce(T.handle, partial_d.data_ptr(), o.data_ptr()) == 0
    return o.cpu().numpy()


def class_chain(T, ci):
    """(P, R) of a class's reduced block: the most pairs one accumulator of one of its items saw; the additions on top, the reduce's included"""
    P, pair = 0, False
    for k in np.flatnonzero(T.items["cls"] == ci):
        npairs = int(T.items[k]["p1"] - T.items[k]["p0"])
        if T.kernel_of(k) == 0:
            P, pair = max(P, -(-npairs // R.PT_THREADS)), True
        elif T.cls[ci]["nrep"] == 1:
            P = max(P, npairs)
        else:
            P = max(P, int(np.bincount(R.wave_of_pairs(T, k), minlength=4).max()))
    cnt = int(T.el_cnt[T.cls_out_off[ci]])
    return P, (R.PAIR_R if pair else 0) + cnt


def check_case(ptc, T, family, seed=0):
    src = R.make_src(T, family, seed)
    p, p_d = run_kernels(ptc, T, src)
    again, _ = run_kernels(ptc, T, src)
    assert R.same_bits(p, again), (T.sec.case.name, "two runs differ")
    R.check_partials(T, range(len(T.items)), p, src, family)
    out = run_reduce(ptc, T, p_d)
    assert R.same_bits(out[T.out_elems:], np.full(GUARD, R.SENT)), "pt_reduce_kernel wrote behind out"
    assert R.same_bits(out[:T.out_elems], R.reduce_restated(p, T.el_src, T.el_cnt, T.el_stride)), (T.sec.case.name, "reduce is not the list-order sum")
    for ci in range(len(T.cls)):
        o, sz = int(T.cls_out_off[ci]), T.block_elems(ci)
        npairs = int(T.cls[ci]["ngu"]) * int(T.cls_ngd[ci])
        x = R.pair_vectors(T, ci, np.arange(npairs), src)
        P, Radd = class_chain(T, ci)
        R.check_block((T.sec.case.name, "class", ci, "reduced"), out[o:o + sz], x, family, P, Radd, R.block_layout(T, ci))
        if npairs == 0:
            assert (T.el_cnt[o:o + sz] == 0).all() and R.same_bits(out[o:o + sz], np.zeros(sz, complex))
    return p, out, src


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_constants(ptc):
    """what the shapes of the case list and the reference assume"""
    c = (C.c_int * 6)()
    ptc.ptc_constants(c)
    assert tuple(c) == (256, 2048, 4, 4, 36, 4)
    assert tuple(c) == (R.PT_THREADS, R.PT_XS, R.PT_PAIR_N, R.PT_LOADS, R.PT_PAIR_COST, R.PT_WG_PER_CU)


def test_launchers_refuse_before_launching(ptc):
    """hipErrorInvalidValue: an empty or overlong slice, a null pointer, a handle whose tables were never uploaded, no handle at all"""
    case = R.CHAIN_CASES[0]
    host_only = R.Tables(ptc, R.make_sector(case))
    T = tables(ptc, case)
    assert T.nitems[0] > 0 and T.nitems[1] > 0 and T.nitems[2] == 0
    buf = sentinel(T.partial_elems + GUARD)
    src = dev(R.make_src(T, "exact"))
    s, p, pitch = src.data_ptr(), buf.data_ptr(), T.sec.pitch
    for f, n in ((ptc.ptc_pair, T.nitems[0]), (ptc.ptc_tile_2_1, T.nitems[1])):
        assert f(T.handle, 0, 0, s, pitch, p) == BAD and f(T.handle, 0, n + 1, s, pitch, p) == BAD and f(T.handle, 1, n, s, pitch, p) == BAD
        assert f(T.handle, -1, 1, s, pitch, p) == BAD and f(T.handle, 0, 1, None, pitch, p) == BAD and f(T.handle, 0, 1, s, pitch, None) == BAD
        assert f(T.handle, 0, 1, s, 0, p) == BAD and f(None, 0, 1, s, pitch, p) == BAD and f(host_only.handle, 0, 1, s, pitch, p) == BAD
    assert ptc.ptc_tile_4_2(T.handle, 0, 1, s, pitch, p) == BAD                       # the sector has no 4 x 4 tile class
    assert ptc.ptc_reduce(host_only.handle, p, p) == BAD and ptc.ptc_reduce(T.handle, None, p) == BAD and ptc.ptc_reduce(T.handle, p, None) == BAD
    assert ptc.ptc_reduce_tables(p, None, p, p, 1, p) == BAD and ptc.ptc_reduce_tables(p, p, p, p, 0, p) == BAD
    assert ptc.ptc_upload(T.handle) == BAD and ptc.ptc_upload(None) == BAD            # uploaded once
    assert ptc.ptc_scatter(None, p, 1.0, 0, p) == BAD
    assert R.same_bits(buf.cpu().numpy(), np.full(T.partial_elems + GUARD, R.SENT)), "a refused call wrote"


def test_builder_refuses_a_class_beyond_the_register_tiles(ptc):
    with pytest.raises(R.BuildError, match="synthetic sector: a class block exceeds the register tiles"):
        R.Tables(ptc, R.make_sector(R.REFUSED_CASE))


# ---- the kernels on pt_build's tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=lambda c: c.name)
def test_kernels(ptc, case, family):
    check_case(ptc, tables(ptc, case), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pair", R.SIGN_CASES, ids=lambda p: p[0].name)
def test_every_sign_set_is_no_sign_set(ptc, pair, family):
    none, every = (tables(ptc, c) for c in pair)
    assert (none.rows >> 31).max() == 0 and (every.rows >> 31).min() == 1 and (every.cols >> 31).min() == 1
    a, oa, _ = check_case(ptc, none, family)
    b, ob, _ = check_case(ptc, every, family)
    assert R.same_bits(a, b) and R.same_bits(oa, ob)


def test_split_rank_without_a_dw_group_of_a_class(ptc):
    """the starved rank's tables have a class with no local dw group: no item, cnt == 0, and the reduce writes 0 (asserted in check_case)"""
    T = tables(ptc, next(c for c in R.SPLIT_CASES if c.cols == "by_k"))
    assert (T.cls_ngd == 0).any() and (T.cls_ngd > 0).any()
    check_case(ptc, T, "exact")


def test_pair_kernel_adds_its_waves_in_order(ptc):
    """wave sums 1, 2**-53, 2**-53, 0 in a 1 x 1 class: v = 0 + 1 + 2**-53 + 2**-53 + 0 in that order is 1; any order that meets the two
    halves first gives 1 + 2**-52"""
    T = tables(ptc, next(c for c in R.PAIR_CASES if c.name == "pair-1x1-256"))
    assert len(T.items) == 1 and T.items[0]["p1"] - T.items[0]["p0"] == 256
    src = R.make_src(T, "exact")
    src[R.named_positions(T)] = 0
    c = T.cls[0]
    for p, v in ((0, 1.0), (64, 2.0 ** -27 * (1 + 1j)), (128, 2.0 ** -27 * (1 + 1j))):
        gd, g = divmod(p, int(c["ngu"]))
        src[int(T.cols[c["cols_off"] + gd] & R.MASK) * T.sec.pitch + int(T.rows[c["rows_off"] + g] & R.MASK)] = v
    part, _ = run_kernels(ptc, T, src)
    want = R.pair_last_stage_restated([1.0, 2.0 ** -53, 2.0 ** -53, 0.0])
    assert want == 1.0 and (2.0 ** -53 + 2.0 ** -53) + 1.0 != 1.0
    assert R.same_bits(part[int(T.items[0]["out_off"])], np.complex128(want))


# ---- pt_reduce_kernel on hand-made tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("nel", R.REDUCE_NEL)
def test_reduce_on_hand_made_tables(ptc, nel, seed):
    """cnt of 0, 1, 2 and 37 (every one of them at nel = 1 over the four seeds), a stride larger than the block with NaN between"""
    partial, src, cnt, stride = R.reduce_tables(nel, seed)
    assert (src + np.maximum(cnt - 1, 0).astype(np.int64) * stride).max() < len(partial) and (stride > nel).all()
    out = sentinel(nel + GUARD)
    p, s, n, st = dev(partial), dev(src), dev(cnt), dev(stride)
    for _ in range(2):
        assert ptc.ptc_reduce_tables(p.data_ptr(), s.data_ptr(), n.data_ptr(), st.data_ptr(), nel, out.data_ptr()) == 0
        got = out.cpu().numpy()
        assert R.same_bits(got[:nel], R.reduce_restated(partial, src, cnt, stride))
        assert R.same_bits(got[nel:], np.full(GUARD, R.SENT))
    assert np.isfinite(got[:nel].real).all() and (got[:nel][cnt == 0] == 0).all()


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_against_the_dense_partial_trace(ptc, case):
    """pair, tile, reduce, scatter on pt_build's tables of one nsub = 4 sector against rho taken straight from the amplitudes: the exact
    family bit for bit after a power-of-two weight; scatter bit for bit against its restatement, accumulated = sum of the single ones"""
    T = tables(ptc, case)
    nn = 1 << (2 * case.nsub)
    _, out, src = check_case(ptc, T, "exact", seed=5)
    raw = np.ascontiguousarray(out[:T.out_elems])
    rho = np.full((nn, nn), R.SENT)
    assert ptc.ptc_scatter(T.handle, raw.ctypes.data, 0.25, 0, rho.ctypes.data) == 0
    re, im = R.dense_partial_trace(T.sec, src)
    assert R.same_bits(rho, 0.25 * re.astype(np.float64) + 1j * (0.25 * im.astype(np.float64)))
    assert abs(np.trace(rho).real * 4 - (np.abs(src[R.named_positions(T)]) ** 2).sum()) == 0
    # rounding family: the restatement, and accumulation
    _, out2, _ = check_case(ptc, T, "rounding", seed=6)
    raw2 = np.ascontiguousarray(out2[:T.out_elems])
    w1, w2 = 0.3, 0.7
    single = []
    for w, r in ((w1, raw), (w2, raw2)):
        m = np.full((nn, nn), R.SENT)
        assert ptc.ptc_scatter(T.handle, r.ctypes.data, w, 0, m.ctypes.data) == 0
        assert R.same_bits(m, R.scatter_restated(T, r, w, False, np.full((nn, nn), R.SENT)))
        assert (np.diagonal(m).imag == 0).all() and R.same_bits(m, m.conj().T + 0.0)
        single.append(m)
    acc = single[0].copy()
    assert ptc.ptc_scatter(T.handle, raw2.ctypes.data, w2, 1, acc.ctypes.data) == 0
    assert R.same_bits(acc + 0.0, single[0] + single[1])
    assert R.same_bits(acc, R.scatter_restated(T, raw2, w2, True, single[0].copy()))
