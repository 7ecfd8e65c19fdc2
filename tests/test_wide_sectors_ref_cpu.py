"""The two array restatements of tests/wide_sectors.py equal the loops they stand for (no GPU): record_numpy_fast against
observables_ref.record_numpy and ladder_numpy against ladder_ref.apply_op, on small sectors of a one-orbital and of a two-orbital model."""
import numpy as np
import pytest

import wide_sectors as WS
from ladder_ref import apply_op
from observables_ref import record_numpy


def _models():
    from hxv import models

    return [(models.hm_1dchain(Nlat=4, Nbath=1, eps_bath=[0.3]), [(4, 3), (0, 5), (5, 1), (8, 8)]),
            (models.bhz_2d(Nx=2, Ny=1, Nbath=1, Ust=0.5, Jh=0.1), [(3, 4), (1, 6), (6, 0)])]


def _maps(ns, n):
    from move_kernels_ref import basis

    return basis(ns, n)


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


def test_record_numpy_fast_is_record_numpy():
    for m, sectors in _models():
        for k, (nup, ndw) in enumerate(sectors):
            mu, md = _maps(m.Ns, nup), _maps(m.Ns, ndw)
            v = _rand(len(mu) * len(md), 10 + k)
            want = record_numpy(m, mu, md, v, 0.7)
            got = WS.record_numpy_fast(m, mu, md, v, 0.7)
            assert got.shape == want.shape and np.abs(got - want).max() <= 4e-16 * max(1.0, np.abs(want).max()), (m.name, nup, ndw)


@pytest.mark.parametrize("spin,create", [(0, True), (0, False), (1, True), (1, False)])
def test_ladder_numpy_is_apply_op(spin, create):
    ns, nup, ndw = 8, 3, 4
    d = 1 if create else -1
    tup, tdw = (nup + d, ndw) if spin == 0 else (nup, ndw + d)
    maps_from, maps_to = (_maps(ns, nup), _maps(ns, ndw)), (_maps(ns, tup), _maps(ns, tdw))
    v = _rand(len(maps_from[0]) * len(maps_from[1]), 5)
    for pos in (0, 3, 7):
        assert np.array_equal(WS.ladder_numpy(v, maps_from, maps_to, pos, spin, create), apply_op(v, maps_from, maps_to, pos, spin, create)), pos


def test_the_sector_lists_name_what_the_gpu_file_expects():
    from math import comb

    assert set(WS.S_SECTORS + WS.P_SECTORS + [WS.GATE_SECTOR] + WS.LADDER_SOURCES) == set(WS.SECTORS)
    for name in WS.SECTORS:
        m, nup, ndw = WS.sector(name)
        assert m.Ns in (20, 22, 24) and m.Ns <= 24
        du, dd = comb(m.Ns, nup), comb(m.Ns, ndw)
        assert max(du, dd) <= 1 << 20
        assert (max(du, dd) > 65535) == (name != "ns22_2_1"), name
        if name in WS.S_SECTORS:
            assert du * dd <= 184756
    m, nup, ndw = WS.sector(WS.GATE_SECTOR)
    # 12 low bits, 8 high orbitals: blocks of at most C(12,6) = 924 <= 960 rows, one hop per high orbital
    assert comb(12, 6) <= 960 and m.Ns - 12 == 8 and comb(m.Ns, nup) >= 65536
