"""The kernels that only MOVE amplitudes between layouts, one by one: the twin map (twin_transpose_kernel, twin_pack_kernel,
twin_unpack_kernel), the ladder operators (ladder_kernel, ladder_cols_kernel), the column packer and the piecewise add of the slab exchanges
(pack_columns_kernel, add_pieces_kernel<double>, <double2>) and the two row-order kernels (rows_ref_to_dev, rows_dev_to_ref), through the
test-only launchers of tests/device/move_kernels_check.hip.  The drivers reach them on real sectors and thread ranks only; here each runs
alone on the synthetic dimensions, row orders, splits, tables and GRIDS of tests/move_kernels_ref.py, which
tests/test_move_kernels_ref_cpu.py has shown to stay inside their buffers, to reach the second and third loop trips, and to be refused
when the kernel makes any of the listed mistakes.

These kernels move, multiply by +-1 and add at most once: the right answer is known bit for bit.  A buffer a kernel writes starts as a
sentinel with one guard element behind it and is compared WHOLE, as 64-bit patterns (so -0.0 is not +0.0), with the restatement's buffer:
every promised element holds its bits, everything else -- pad rows the contract leaves alone, stride pads, the own block's rows of `send`,
the guard -- still holds the sentinel.  A buffer a kernel reads holds NaN wherever the contract says "never read".

The one comparison that is not by bits is ladder_kernel with a random complex coef: test_ladder_random_coef_within_the_rounding_bound."""
import ctypes as C

import numpy as np
import pytest

import move_kernels_ref as R

pytestmark = pytest.mark.gpu

BAD = 1  # hipErrorInvalidValue


def ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="session")
def mkc(built):
    import torch  # noqa: F401  (first: one HIP runtime per process, see hxv/engine.py)

    L = C.CDLL(str(built.build_move_kernels_check()))
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    L.mkc_twin_transpose.argtypes = [i32, i32, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp]
    L.mkc_twin_pack.argtypes = [i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32]
    L.mkc_twin_unpack.argtypes = [i32, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp]
    L.mkc_ladder.argtypes = [i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, f64, f64, i32, vp, vp, vp]
    L.mkc_ladder_cols.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, f64, f64, i32]
    L.mkc_pack_columns.argtypes = [i32, vp, vp, vp, i32]
    L.mkc_add_pieces.argtypes = [i32, i32, i32, i32, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(vp), i32, i32]
    L.mkc_rows_ref_to_dev.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32]
    L.mkc_rows_dev_to_ref.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32]
    assert L.mkc_tw() == R.TW and L.mkc_tw_threads() == R.TW_THREADS
    return L


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def host(t):
    return t.cpu().numpy()


def order_dev(o, inverse=True):
    """(iperm or perm, sign) of a row order on the device, or (None, None)"""
    if o is None:
        return None, None
    return dev(o.iperm if inverse else o.perm), dev(o.sign)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.flatnonzero((R.bits(got).reshape(len(got), -1) != R.bits(want).reshape(len(want), -1)).any(axis=1))
    assert bad.size == 0, (what, f"{bad.size} of {len(got)} elements differ, the first at {int(bad[0])}: {got[bad[0]]!r} for {want[bad[0]]!r}")


# ---- twin_transpose_kernel -------------------------------------------------------------------------------------------------------------------
def run_transpose(L, c, d_a):
    ipa, sa = order_dev(c.oa)
    ipb, sb = order_dev(c.ob)
    out = dev(R.fresh(c.dimup_a * c.pitch_b))
    assert L.mkc_twin_transpose(c.gx, c.gy, ptr(d_a), c.dimup_a, c.pitch_a, ptr(ipa), ptr(sa), ptr(out), c.dimup_b, c.pitch_b, ptr(ipb), ptr(sb)) == 0
    return out


@pytest.mark.parametrize("c", R.transpose_cases(), ids=ids(R.transpose_cases()))
def test_twin_transpose(mkc, c):
    a = R.transpose_inputs(c)
    out = run_transpose(mkc, c, dev(a))
    same(host(out), R.transpose_ref(c, a), c.name)
    # and back: B -> A with the roles exchanged returns the input's bits on the rows of A (its pad rows, NaN in the input, come back +0.0)
    back = R.Transpose(c.name + "-back", c.dimup_b, c.dimup_a, c.pitch_b, c.pitch_a, c.ob, c.oa, -(-c.dimup_b // R.TW), -(-c.pitch_a // R.TW))
    again = host(run_transpose(mkc, back, out))
    want = a.copy()
    want[:-1].reshape(c.dimup_b, c.pitch_a)[:, c.dimup_a:] = 0.0
    want[-1] = R.SENT
    same(again, want, c.name + " and back")


# ---- twin_pack_kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.pack_cases(), ids=ids(R.pack_cases()))
def test_twin_pack(mkc, c):
    a = R.pack_inputs(c)
    want_send, want_own = R.pack_ref(c, a)
    d_a, send, own = dev(a), dev(R.fresh(c.dimup_a * c.stride)), dev(R.fresh((c.own_hi - c.own_lo) * c.stride))
    ipa, sa = order_dev(c.oa)
    assert mkc.mkc_twin_pack(c.gx, c.gy, ptr(d_a), c.dimup_a, c.pitch_a, c.qa, ptr(ipa), ptr(sa), ptr(send), ptr(own), c.stride, c.own_lo, c.own_hi) == 0
    same(host(send), want_send, c.name + " send")
    same(host(own), want_own, c.name + " own")


# ---- twin_unpack_kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.unpack_cases(), ids=ids(R.unpack_cases()))
def test_twin_unpack(mkc, c):
    recv = R.unpack_inputs(c)
    d_recv, tab, out = dev(recv), dev(c.tab()), dev(R.fresh(c.qb * c.pitch_b))
    ipb, sb = order_dev(c.ob)
    assert mkc.mkc_twin_unpack(c.gx, c.gy, ptr(d_recv), ptr(tab), c.nranks, ptr(out), c.dimup_b, c.pitch_b, c.qb, ptr(ipb), ptr(sb)) == 0
    same(host(out), R.unpack_ref(c, recv), c.name)


# ---- pack, the exchange on the host, unpack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("da,dw,p", R.CHAIN_SHAPES, ids=[f"{a}x{w}-P{p}" for a, w, p in R.CHAIN_SHAPES])
def test_twin_chain_without_a_communicator(mkc, built, da, dw, p):
    """the split map of hxv_twin.hip on p synthetic ranks: counts from hxv_twin_split_plan, every rank packs, the blocks move the way
    comm_sendrecv_cols moves them (rank r's send[send_ptr[q] .. send_ptr[q+1]) becomes rank q's recv[recv_ptr[r] .. recv_ptr[r+1]); the own
    block is not moved, the packer put it in place), every rank unpacks; the slabs together are the transpose, and twin_transpose_kernel's bits"""
    import torch

    H = C.CDLL(str(built.build_engine()))
    H.hxv_twin_split_plan.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int64)] * 2
    rng = np.random.default_rng(da * 1000 + dw * 10 + p)
    whole = R.Transpose(f"{da}x{dw}", da, dw, R.roundup8(da), R.roundup8(dw), R.row_order(rng, da), R.row_order(rng, dw), -(-da // R.TW), -(-R.roundup8(dw) // R.TW))
    a = R.transpose_inputs(whole, seed=p)
    want = R.transpose_ref(whole, a)
    d_whole = host(run_transpose(mkc, whole, dev(a)))
    same(d_whole, want, "the unsplit map")
    fa, fb = R.dw_split(dw, p), R.dw_split(da, p)
    ipa, sa = order_dev(whole.oa)
    ipb, sb = order_dev(whole.ob)
    sc, rc, send, recv = [], [], [], []
    for r in range(p):
        s, q = (C.c_int64 * p)(), (C.c_int64 * p)()
        assert H.hxv_twin_split_plan(da, dw, r, p, s, q) == 0
        sc.append(np.array(s[:], dtype=np.int64)), rc.append(np.array(q[:], dtype=np.int64))
    sp = [np.concatenate([[0], np.cumsum(x)]) for x in sc]
    rp = [np.concatenate([[0], np.cumsum(x)]) for x in rc]
    for r in range(p):
        qa, qb = int(fa[r + 1] - fa[r]), int(fb[r + 1] - fb[r])
        stride = int(sc[r][r]) // qb
        assert stride == R.roundup8(qa) and sp[r][p] == da * stride and sp[r][r] == fb[r] * stride and rc[r][r] == sc[r][r]
        slab = dev(R.with_guard(a[:-1].reshape(dw, whole.pitch_a)[fa[r]:fa[r + 1]].reshape(-1)))
        send.append(dev(R.fresh(int(sp[r][p]))))
        recv.append(torch.full((int(rp[r][p]) + 1,), complex("nan"), dtype=torch.complex128, device="cuda"))
        own = recv[r].data_ptr() + 16 * int(rp[r][r])
        assert mkc.mkc_twin_pack(-(-da // R.TW), min(-(-qa // R.TW), 65535), ptr(slab), da, whole.pitch_a, qa, ptr(ipa), ptr(sa), ptr(send[r]), own, stride,
                                 int(fb[r]), int(fb[r + 1])) == 0
        mine = host(send[r])[int(sp[r][r]):int(sp[r][r + 1])]
        same(mine, np.full_like(mine, R.SENT), "the own block's rows of send are not written")
    for r in range(p):
        for q in range(p):
            if q != r:
                assert sc[r][q] == rc[q][r]
                recv[q][int(rp[q][r]):int(rp[q][r + 1])] = send[r][int(sp[r][q]):int(sp[r][q + 1])]
    for q in range(p):
        qb = int(fb[q + 1] - fb[q])
        tab = dev(np.concatenate([fa, rp[q], rc[q] // qb]).astype(np.int64))
        out = dev(R.fresh(qb * whole.pitch_b))
        assert mkc.mkc_twin_unpack(-(-whole.pitch_b // R.TW_THREADS), min(qb, 65535), ptr(recv[q]), ptr(tab), p, ptr(out), dw, whole.pitch_b, qb, ptr(ipb),
                                   ptr(sb)) == 0
        lo, hi = int(fb[q]) * whole.pitch_b, int(fb[q + 1]) * whole.pitch_b
        same(host(out)[:-1], want[lo:hi], f"rank {q}: the numpy transpose")
        same(host(out)[:-1], d_whole[lo:hi], f"rank {q}: twin_transpose_kernel")
        assert R.same_bits(host(out)[-1:], np.array([R.SENT]))


# ---- ladder_kernel ---------------------------------------------------------------------------------------------------------------------------
def run_ladder(L, c, psi, out0, coef, accumulate):
    mf, mt, d_psi, out = dev(c.map_from), dev(c.map_to), dev(psi), dev(out0)
    pf, sf = order_dev(c.ofrom, inverse=False)
    st = None if c.sign_to is None else dev(c.sign_to)
    assert L.mkc_ladder(c.gx, ptr(mf), c.dim_from, ptr(mt), c.pitch_from, c.dimup_to, c.pitch_to, c.dimdw_to, c.orbital, c.spin, c.create, ptr(d_psi), ptr(out),
                        coef.real, coef.imag, accumulate, ptr(pf), ptr(sf), ptr(st)) == 0
    return host(out)


@pytest.mark.parametrize("c", R.ladder_cases(), ids=ids(R.ladder_cases()))
def test_ladder_bit_for_bit(mkc, c):
    """coef = 1 on random data (a signed copy), and small integers with an integer complex coef, with and without `accumulate` (every
    product and sum exact, fused or not)"""
    for mode, (coef, accumulate, integer) in R.LADDER_MODES.items():
        psi, out0 = R.ladder_inputs(c, integer)
        same(run_ladder(mkc, c, psi, out0, coef, accumulate), R.ladder_ref(c, psi, out0, coef, accumulate), f"{c.name} {mode}")


U = 2.0 ** -53
GAMMA3 = 3 * U / (1 - 3 * U)


@pytest.mark.parametrize("c", R.ladder_cases(), ids=ids(R.ladder_cases()))
def test_ladder_random_coef_within_the_rounding_bound(mkc, c):
    """Random data and a random complex coef: not bit for bit, the compiler may fuse the two products of a component.

    The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  Real part of a reached element (the imaginary part alike, with x.x and x.y exchanged):
    p = a - b, a = c.x x.x, b = c.y x.y.  The device forms fl(fl(a) - fl(b)), or one of the fused fl(a - fl(b)), fl(fl(a) - b).  Either way
    each of a and b passes through at most two roundings of relative size <= u: p^ = a (1 + t1) - b (1 + t2) with |t1|, |t2| <= gamma_2, so
    |p^ - p| <= gamma_2 (|a| + |b|).  The sign +-1 is exact.  With `accumulate` one more rounding, r^ = (p^ + o)(1 + d), |d| <= u, so against
    the exact R = p + o
        |r^ - R| <= |p^ - p| + u |p^ + o| <= gamma_2 (1 + u) (|a| + |b|) + u |R| <= gamma_3 (|a| + |b|) + u |R|,
    and without it R = p and the last term is spare.  An element that is not reached is +0.0 + o: exact.  The reference is the same
    expression in long double (u_L = 2^-64): its own error, at most 3 u_L (|a| + |b| + |o|), disappears in the u (|a| + |b|) by which gamma_3
    exceeds gamma_2 (1 + u).  Pad rows and the guard are compared by bits."""
    rng = np.random.default_rng(77)
    for accumulate in (0, 1):
        coef = complex(rng.standard_normal(), rng.standard_normal())
        psi, out0 = R.ladder_inputs(c, False, seed=accumulate + 1)
        got = run_ladder(mkc, c, psi, out0, coef, accumulate)
        re, im, mre, mim = R.ladder_ref_long(c, psi, out0, coef, accumulate)
        g = got[:-1].reshape(c.dimdw_to, c.pitch_to)
        for comp, ref, mag in ((g[:, :c.dimup_to].real, re, mre), (g[:, :c.dimup_to].imag, im, mim)):
            err = np.abs(comp.astype(np.longdouble) - ref)
            bound = np.longdouble(GAMMA3) * mag + np.longdouble(U) * np.abs(ref)
            worst = int(np.argmax(err - bound))
            print(f"{c.name} acc{accumulate}: max err {float(err.max()):.3e}, err - bound at its worst {float((err - bound).ravel()[worst]):.3e}")
            assert (err <= bound).all(), (c.name, accumulate, float(err.ravel()[worst]), float(bound.ravel()[worst]))
        want_pad = out0[:-1].reshape(c.dimdw_to, c.pitch_to)[:, c.dimup_to:]
        assert R.same_bits(np.ascontiguousarray(g[:, c.dimup_to:]), np.ascontiguousarray(want_pad)) and R.same_bits(got[-1:], out0[-1:]), c.name


# ---- ladder_cols_kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ladder_cols_cases(), ids=ids(R.ladder_cols_cases()))
def test_ladder_cols(mkc, c):
    pl, rv, out0 = R.ladder_cols_inputs(c)
    d_pl, d_rv, out, slot, sign = dev(pl), dev(rv), dev(out0), dev(c.slot), dev(c.sign)
    assert mkc.mkc_ladder_cols(c.gx, c.dimup, c.ncols, c.pitch_from, c.pitch_to, ptr(slot), ptr(sign), ptr(d_pl), ptr(d_rv), ptr(out), c.coef.real,
                               c.coef.imag, c.accumulate) == 0
    same(host(out), R.ladder_cols_ref(c, pl, rv, out0), c.name)


# ---- pack_columns_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.pack_columns_cases(), ids=ids(R.pack_columns_cases()))
def test_pack_columns(mkc, c):
    a = R.pack_columns_inputs(c)
    d_a, out, cols = dev(a), dev(R.fresh(len(c.cols) * c.pitch)), dev(c.cols)
    assert mkc.mkc_pack_columns(len(c.cols), ptr(d_a), ptr(out), ptr(cols), c.pitch) == 0
    same(host(out), R.pack_columns_ref(c, a), c.name)


# ---- add_pieces_kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.add_pieces_cases(), ids=ids(R.add_pieces_cases()))
def test_add_pieces(mkc, c):
    hv0, pieces = R.add_pieces_inputs(c)
    hv, d_pieces = dev(hv0), [dev(p) for p in pieces]
    row0, row1 = (C.c_int32 * c.nwtr)(*map(int, c.row0)), (C.c_int32 * c.nwtr)(*map(int, c.row1))
    stride, base = (C.c_int64 * c.nwtr)(*map(int, c.stride)), (C.c_void_p * c.nwtr)(*[p.data_ptr() for p in d_pieces])
    assert mkc.mkc_add_pieces(c.gx, c.gy, c.ncols, int(c.real), ptr(hv), c.nwtr, row0, row1, stride, base, c.dimup, c.pitch) == 0
    same(host(hv), R.add_pieces_ref(c, hv0, pieces), c.name)


# ---- rows_ref_to_dev, rows_dev_to_ref --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.rows_cases(), ids=ids(R.rows_cases()))
def test_rows_each_way_and_round_trip(mkc, c):
    ref, devv = R.rows_inputs(c)
    iperm, perm, sign = dev(c.order.iperm), dev(c.order.perm), dev(c.order.sign)
    d_ref, to_dev = dev(ref), dev(R.fresh(c.ncols * c.pitch))
    assert mkc.mkc_rows_ref_to_dev(c.gx, ptr(d_ref), ptr(to_dev), ptr(iperm), ptr(sign), c.dimup, c.pitch, c.ncols) == 0
    same(host(to_dev), R.rows_ref_to_dev_ref(c, ref), c.name + " in")
    d_dev, to_ref = dev(devv), dev(R.fresh(c.ncols * c.dimup))
    assert mkc.mkc_rows_dev_to_ref(c.gx, ptr(d_dev), ptr(to_ref), ptr(perm), ptr(sign), c.dimup, c.pitch, c.ncols) == 0
    same(host(to_ref), R.rows_dev_to_ref_ref(c, devv), c.name + " out")
    again = dev(R.fresh(c.ncols * c.dimup))
    assert mkc.mkc_rows_dev_to_ref(c.gx, ptr(to_dev), ptr(again), ptr(perm), ptr(sign), c.dimup, c.pitch, c.ncols) == 0
    want = ref.copy()
    want[-1] = R.SENT
    same(host(again), want, c.name + " in and out again")


# ---- the launchers refuse what could reach outside the buffers ---------------------------------------------------------------------------------
def test_the_launchers_refuse_bad_arguments(mkc):
    import torch

    x = torch.zeros(4096, dtype=torch.complex128, device="cuda")
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, q = x.data_ptr(), t.data_ptr()
    L = mkc
    for gx, gy, da, pa, db, pb, a in ((0, 1, 8, 8, 8, 8, p), (1, 0, 8, 8, 8, 8, p), (1, 1, 0, 8, 8, 8, p), (1, 1, 9, 8, 8, 8, p), (1, 1, 8, 12, 8, 8, p),
                                      (1, 1, 8, 8, 8, 4, p), (1, 1, 8, 8, 8, 8, None), (65536, 1, 8, 8, 8, 8, p)):
        assert L.mkc_twin_transpose(gx, gy, a, da, pa, None, None, p, db, pb, None, None) == BAD
    for gy, qa, stride, lo, hi, own in ((0, 4, 8, 0, 0, p), (1, 0, 8, 0, 0, p), (1, 9, 8, 0, 0, p), (1, 4, 12, 0, 0, p), (1, 4, 8, 2, 1, p), (1, 4, 8, 0, 9, p),
                                        (1, 4, 8, -1, 2, p), (1, 4, 8, 0, 2, None)):
        assert L.mkc_twin_pack(1, gy, p, 8, 8, qa, None, None, p, own, stride, lo, hi) == BAD
    for gx, tab, nr, db, pb, qb in ((0, q, 2, 8, 8, 1), (1, None, 2, 8, 8, 1), (1, q, 0, 8, 8, 1), (1, q, 2, 9, 8, 1), (1, q, 2, 8, 8, 0)):
        assert L.mkc_twin_unpack(gx, 1, p, tab, nr, p, db, pb, qb, None, None) == BAD
    for gx, dimf, pf, dut, pt, ddt, orb, spin, mf in ((0, 4, 8, 6, 8, 2, 0, 0, q), (1, 0, 8, 6, 8, 2, 0, 0, q), (1, 9, 8, 6, 8, 2, 0, 0, q), (1, 4, 8, 6, 4, 2, 0, 0, q),
                                                      (1, 4, 8, 6, 8, 0, 0, 0, q), (1, 4, 8, 6, 8, 2, 32, 0, q), (1, 4, 8, 6, 8, 2, 0, 2, q), (1, 4, 8, 6, 8, 2, 0, 0, None),
                                                      (1, 4, 8, 9, 16, 2, 0, 1, q)):
        assert L.mkc_ladder(gx, mf, dimf, q, pf, dut, pt, ddt, orb, spin, 1, p, p, 1.0, 0.0, 0, None, None, None) == BAD
    for gx, du, nc, pf, pt, slot in ((0, 8, 2, 8, 8, q), (1, 0, 2, 8, 8, q), (1, 8, 0, 8, 8, q), (1, 9, 2, 8, 16, q), (1, 8, 2, 8, 12, q), (1, 8, 2, 8, 8, None)):
        assert L.mkc_ladder_cols(gx, du, nc, pf, pt, slot, q, p, p, p, 1.0, 0.0, 0) == BAD
    for nc, cols, pitch in ((0, q, 8), (1, None, 8), (1, q, 0), (1, q, 12), (65536, q, 8)):
        assert L.mkc_pack_columns(nc, p, p, cols, pitch) == BAD
    r0, r1, s1, b1 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(8), (C.c_int64 * 1)(8), (C.c_void_p * 1)(p)
    nul = (C.c_void_p * 1)(None)
    for gx, nc, nw, du, pt, bb in ((0, 1, 1, 8, 8, b1), (1, 0, 1, 8, 8, b1), (1, 1, 0, 8, 8, b1), (1, 1, 1, 9, 8, b1), (1, 1, 1, 8, 12, b1), (1, 1, 1, 8, 8, nul)):
        assert L.mkc_add_pieces(gx, max(nc, 1), nc, 0, p, nw, r0, r1, s1, bb, du, pt) == BAD
    for gy in (0, 65536):       # (the blocks along y loop over the columns: their number is a grid extent of its own)
        assert L.mkc_add_pieces(1, gy, 1, 0, p, 1, r0, r1, s1, b1, 8, 8) == BAD
    for fn in (L.mkc_rows_ref_to_dev, L.mkc_rows_dev_to_ref):
        for gx, du, pt, nc, tb in ((0, 8, 8, 1, q), (1, 0, 8, 1, q), (1, 9, 8, 1, q), (1, 8, 12, 1, q), (1, 8, 8, 0, q), (1, 8, 8, 1, None)):
            assert fn(gx, p, p, tb, tb, du, pt, nc) == BAD
    torch.cuda.synchronize()
    assert (x == 0).all() and (t == 0).all()
