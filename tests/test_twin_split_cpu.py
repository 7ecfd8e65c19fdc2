"""The twin-sector map on split sectors (include/hxv.h: hxv_twin_vector across ranks, hxv_twin_split_plan) without a GPU: the library exports
the plan; rank p's send count towards q is rank q's receive count from p and both are qdw_B(q) * roundup8(qdw_A(p)) with the reference's
split rule (ED_HAMILTONIAN.f90:93-105) written out here; pack, exchange and unpack restated in numpy with those counts, random row orders
and signs on both sides, assemble to the reference's definition (tests/twin_ref.py).  That pins the layout the two kernels of
csrc/hxv_twin.hip implement; tests/test_twin_cpu.py applies the register / scratch budgets and the ISA lint to every kernel of that file."""
import ctypes
from itertools import combinations
from math import comb

import numpy as np
import pytest

import twin_ref

ARG = 1
# (Ns, nup, ndw, nranks): the shapes of tests/test_gpu_twin_split.py
SHAPES = [(4, 1, 2, 4), (6, 1, 3, 2), (6, 1, 3, 3), (6, 3, 3, 3), (8, 4, 1, 3), (8, 1, 4, 3), (8, 3, 5, 4), (10, 4, 5, 4)]


def _split(dim, r, p):
    """the reference's split of an axis of `dim` columns over p ranks: (columns of rank r, its first column)"""
    q, rem = divmod(dim, p)
    return q + (1 if r < rem else 0), r * q + min(r, rem)


def _up8(n):
    return (n + 7) // 8 * 8


def _sector_map(ns, n):
    """Fock numbers of the configurations of n particles on ns orbitals, ascending: the sector map of one spin"""
    return np.array(sorted(sum(1 << b for b in c) for c in combinations(range(ns), n)), dtype=np.int64)


def test_library_exports_the_split_plan(built):
    import hxv

    assert "hxv_twin_split_plan" in hxv.EXPORTS
    assert hasattr(ctypes.CDLL(str(hxv.LIB_PATH)), "hxv_twin_split_plan")
    assert callable(hxv.twin_split_plan)


@pytest.mark.parametrize("dimup,dimdw,nranks", [(comb(ns, nu), comb(ns, nd), p) for ns, nu, nd, p in SHAPES] + [(1430, 11440, 8)])
def test_split_plan_is_consistent_between_every_pair_of_ranks(built, dimup, dimdw, nranks):
    import hxv

    plans = [hxv.twin_split_plan(dimup, dimdw, r, nranks) for r in range(nranks)]
    for p in range(nranks):
        for q in range(nranks):
            want = _split(dimup, q, nranks)[0] * _up8(_split(dimdw, p, nranks)[0])
            assert plans[p][0][q] == plans[q][1][p] == want, (p, q, plans[p][0][q], plans[q][1][p], want)
    # what the packer's addressing rests on: a rank's send blocks, in rank order, tile a [dimup][stride] matrix
    for p in range(nranks):
        assert plans[p][0].sum() == dimup * _up8(_split(dimdw, p, nranks)[0])


def test_split_plan_refuses_bad_arguments(built):
    import hxv

    L = hxv.load_library()
    sc = (ctypes.c_int64 * 8)(*([-7] * 8))
    rc = (ctypes.c_int64 * 8)(*([-7] * 8))
    for args in [(6, 20, 0, 7), (20, 6, 0, 7), (6, 20, 2, 2), (6, 20, -1, 2), (6, 20, 0, 0), (0, 20, 0, 1), (6, 0, 0, 1)]:
        assert L.hxv_twin_split_plan(*args, sc, rc) == ARG, args
        assert "hxv_twin_split_plan" in L.hxv_last_error().decode()
    assert L.hxv_twin_split_plan(6, 20, 0, 2, None, rc) == ARG
    assert L.hxv_twin_split_plan(6, 20, 0, 2, sc, None) == ARG
    assert list(sc) == [-7] * 8 and list(rc) == [-7] * 8          # a refused call writes nothing
    assert L.hxv_twin_split_plan(6, 20, 0, 6, sc, rc) == 0        # nranks == min(dimup, dimdw) is the last one allowed
    with pytest.raises(hxv.HxvError, match=r"status 1\).*hxv_twin_split_plan"):
        hxv.twin_split_plan(6, 20, 0, 7)


def _device_slab(v, dimup, dw0, qdw, perm, sign):
    """this rank's slab in the device layout: [qdw][pitch], d[c, perm[iup]] = sign[iup] * v[iup + (dw0+c)*DimUp], pad rows NaN"""
    pitch = _up8(dimup)
    d = np.full((qdw, pitch), complex(np.nan, np.nan))
    d[:, perm] = sign[None, :] * v.reshape(-1, dimup)[dw0: dw0 + qdw, :]
    return d


@pytest.mark.parametrize("ns,nup,ndw,nranks", SHAPES)
def test_pack_exchange_unpack_in_numpy_is_the_reference_twin(built, ns, nup, ndw, nranks):
    import hxv

    P = nranks
    mu, md = _sector_map(ns, nup), _sector_map(ns, ndw)
    du, dd = mu.size, md.size                                   # A: DimUp x DimDw; B: dd x du
    rng = np.random.default_rng(1000 * ns + 100 * nup + 10 * ndw + P)
    v = rng.standard_normal(du * dd) + 1j * rng.standard_normal(du * dd)
    want = twin_ref.twin_vector(v, mu, md, ns)                  # the reference's definition: B's vector, index idw_A + iup_A*DimDw_A
    perm_a, sign_a = rng.permutation(du), rng.choice([-1.0, 1.0], du)   # reference row -> device row, sign by reference row (hxv_row_order)
    perm_b, sign_b = rng.permutation(dd), rng.choice([-1.0, 1.0], dd)
    iperm_a, iperm_b = np.argsort(perm_a), np.argsort(perm_b)
    fa = [_split(dd, p, P)[1] for p in range(P)] + [dd]         # first column of A per rank
    fb = [_split(du, p, P)[1] for p in range(P)] + [du]         # first column of B = reference up-row of A per rank
    plans = [hxv.twin_split_plan(du, dd, r, P) for r in range(P)]
    nan = complex(np.nan, np.nan)
    send, recv, sptr, rptr = [], [], [], []
    # pack: rank r cuts its slab by the receivers' row ranges; its own block goes straight into its receive buffer
    for r in range(P):
        sc, rc = plans[r]
        sptr.append(np.concatenate([[0], np.cumsum(sc)]))
        rptr.append(np.concatenate([[0], np.cumsum(rc)]))
        send.append(np.full(sptr[r][-1], nan))
        recv.append(np.full(rptr[r][-1], nan))
    for r in range(P):
        qa = fa[r + 1] - fa[r]
        stride = _up8(qa)
        slab = _device_slab(v, du, fa[r], qa, perm_a, sign_a)
        for ra in range(du):                                    # device rows of A; pad rows are never touched
            iup = iperm_a[ra]
            q = next(p for p in range(P) if fb[p] <= iup < fb[p + 1])
            row = sign_a[iup] * slab[:, ra]
            assert sptr[r][q] == fb[q] * stride                 # the blocks follow each other by reference row
            if q == r:
                o = rptr[r][r] + (iup - fb[r]) * stride
                recv[r][o: o + qa] = row
            else:
                o = sptr[r][q] + (iup - fb[q]) * stride
                send[r][o: o + qa] = row
    # exchange: the counts of the plan, nothing else
    for r in range(P):
        for q in range(P):
            if q != r:
                n = plans[r][0][q]
                assert n == plans[q][1][r]
                recv[q][rptr[q][r]: rptr[q][r] + n] = send[r][sptr[r][q]: sptr[r][q] + n]
    # unpack: every element of B's slab, pad rows zero, and back to the host layout
    got = np.empty_like(want)
    for r in range(P):
        qb = fb[r + 1] - fb[r]
        pitch_b = _up8(dd)
        out = np.full((qb, pitch_b), nan)
        for rb in range(pitch_b):
            if rb >= dd:
                out[:, rb] = 0.0
                continue
            idw = iperm_b[rb]
            o = next(p for p in range(P) if fa[p] <= idw < fa[p + 1])
            stride = _up8(fa[o + 1] - fa[o])
            out[:, rb] = sign_b[idw] * recv[r][rptr[r][o] + np.arange(qb) * stride + idw - fa[o]]
        assert np.isfinite(out.view(np.float64)).all()          # the stride pads and the unused own block of the send buffer are never read
        assert not out[:, dd:].any()
        host = sign_b[None, :] * out[:, perm_b]                 # hxv_vector_to_host: v[k*DimUp + i] = sign[i] * d[k, perm[i]]
        got[fb[r] * dd: fb[r + 1] * dd] = host.ravel()
    assert np.array_equal(got, want)
    assert np.array_equal(want, v.reshape(dd, du).T.ravel())
