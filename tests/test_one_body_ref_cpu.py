"""The numpy restatement of hxv_apply_one_body and of the one-body susceptibility (tests/one_body_ref.py) against explicit Jordan-Wigner
Fock matrices, and the properties of the fixtures the GPU checks rest on (tests/test_gpu_one_body.py).  No GPU."""
import numpy as np
import pytest

import one_body_ref as R
import spin_pair_ref as S

NS = 4
SECTORS = [(2, 2), (3, 1), (1, 2)]


@pytest.mark.parametrize("nup,ndw", SECTORS)
def test_every_single_term_equals_its_jordan_wigner_matrix_exactly(nup, ndw):
    """integer-valued states: every product and sum is exact, the difference is 0"""
    maps = S.sector_maps(NS, nup, ndw)
    idx = S.fock_index(maps, NS)
    rng = np.random.default_rng(7)
    psi = (rng.integers(-9, 10, idx.size) + 1j * rng.integers(-9, 10, idx.size)).astype(np.complex128)
    for spin in (0, 1):
        for i in range(NS):
            for j in range(NS):
                op = R.fock_operator(NS, [(spin, i, j, 1.0)])
                block = op[np.ix_(idx, idx)]
                assert np.abs(np.delete(op[:, idx], idx, axis=0)).max() == 0        # nothing leaves the sector
                out, mean, n2 = R.apply(maps, [(spin, i, j, 1.0)], psi)
                ref = block @ psi
                assert np.array_equal(out, ref), (spin, i, j)
                assert mean == np.vdot(psi, ref) / np.vdot(psi, psi).real and n2 == np.vdot(ref, ref).real
                if i == j:                                                          # the occupation: diagonal, 0 or 1
                    assert np.array_equal(block, np.diag(np.diag(block))) and set(np.diag(block).real) <= {0.0, 1.0}


@pytest.mark.parametrize("nup,ndw", SECTORS)
def test_term_lists_sum_in_order_and_the_mean_is_subtracted(nup, ndw):
    maps = S.sector_maps(NS, nup, ndw)
    idx = S.fock_index(maps, NS)
    rng = np.random.default_rng(11)
    psi = rng.standard_normal(idx.size) + 1j * rng.standard_normal(idx.size)
    terms = [(int(rng.integers(2)), int(rng.integers(NS)), int(rng.integers(NS)), complex(rng.standard_normal(), rng.standard_normal())) for _ in range(12)]
    block = R.fock_operator(NS, terms)[np.ix_(idx, idx)]
    s1 = sum(abs(t[3]) for t in terms)
    out, mean, n2 = R.apply(maps, terms, psi)
    assert np.abs(out - block @ psi).max() <= 1e-14 * s1 * np.abs(psi).max() * len(terms)
    assert abs(mean - np.vdot(psi, block @ psi) / np.vdot(psi, psi).real) <= 1e-14 * s1
    fl, mean2, n2f = R.apply(maps, terms, psi, subtract_mean=True)
    assert mean2 == mean and abs(np.vdot(psi, fl)) <= 1e-13 * s1 * np.vdot(psi, psi).real
    assert abs(n2f - (n2 - abs(mean) ** 2 * np.vdot(psi, psi).real)) <= 1e-12 * s1 ** 2 * np.vdot(psi, psi).real
    # O^+ of the restatement is the adjoint matrix
    dag = R.fock_operator(NS, R.dagger(terms))[np.ix_(idx, idx)]
    assert np.abs(dag - block.conj().T).max() <= 1e-15 * s1


def test_the_listed_operators_are_what_their_names_say():
    maps = S.sector_maps(NS, 2, 2)
    idx = S.fock_index(maps, NS)
    blk = lambda terms: R.fock_operator(NS, terms)[np.ix_(idx, idx)]  # noqa: E731
    for op in (R.bond(0, 2), R.current(0, 2), R.bond(1, 3)):
        assert np.array_equal(blk(op), blk(op).conj().T) and np.abs(blk(op)).max() > 0
    h = blk(R.hop(0, 1))
    assert not np.array_equal(h, h.conj().T)
    assert np.array_equal(blk(R.bond(0, 1)), h + h.conj().T) and np.array_equal(blk(R.current(0, 1)), 1j * (h - h.conj().T))
    up, dw = blk([(0, 0, 1, 1.0)]), blk([(1, 0, 1, 1.0)])
    assert np.array_equal(blk(R.exciton(0, 1, False)), up + dw) and np.array_equal(blk(R.exciton(0, 1, True)), up - dw)


# in-sector gap and max|chi| of the listed operators, computed on the CPU from spin_pair_ref.chi_fixture
FIXTURES = {"plaquette": (0.296, 1.58), "chain": (0.484, 1.03), "bhz": (0.298, 0.223), "square": (0.290, 1.54)}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_have_an_in_sector_gap_and_a_susceptibility_to_measure(name):
    m, (nup, ndw), real = S.chi_fixture(name)
    w, U, maps = S.dense_sector(m, nup, ndw)
    gap = w[1] - w[0]
    z = 1j * S.NU
    biggest = max(np.abs(R.lehmann_chi(w, U, maps, ops, z)).max() for ops in R.chi_ops(name).values())
    print(f"{name} ({nup},{ndw}): in-sector gap {gap:.3f}, max|chi| {biggest:.3f}")
    assert gap > 1e-2                                            # no in-sector level within 1e-2 of the ground state: nu_0 = 0 is a fair point
    assert biggest > 1e-3
    want_gap, want_chi = FIXTURES[name]
    assert abs(gap - want_gap) <= 2e-3 and abs(biggest - want_chi) <= 6e-3 * max(1.0, want_chi)     # (the recorded figures, three digits)
    for ops in R.chi_ops(name).values():                         # every listed operator moves the state
        psi = U[:, 0]
        assert all(R.apply(maps, op, psi, True)[2] > 1e-6 for op in ops)
