"""The numpy restatement of hxv_apply_spin_pair and of the pair / spin-flip susceptibility (tests/spin_pair_ref.py) against explicit
Fock-space matrices, and the properties of the fixtures the GPU checks use (tests/test_gpu_spin_pair.py).  No GPU."""
import itertools

import numpy as np
import pytest

import spin_pair_ref as R

FLAGS = list(itertools.product((False, True), repeat=2))


def _terms(rng, ns, n):
    return [(int(rng.integers(ns)), int(rng.integers(ns)), complex(rng.standard_normal(), rng.standard_normal())) for _ in range(n)]


@pytest.mark.parametrize("ns", [2, 3, 4])
def test_restatement_equals_the_jordan_wigner_matrices_up_to_one_sign_per_sector_pair(ns):
    rng = np.random.default_rng(ns)
    for cu, cd in FLAGS:
        terms = _terms(rng, ns, 5)
        op = R.fock_operator(ns, terms, cu, cd)
        for nup, ndw in itertools.product(range(ns + 1), repeat=2):
            tu, td = nup + (1 if cu else -1), ndw + (1 if cd else -1)
            if not (0 <= tu <= ns and 0 <= td <= ns):
                continue
            ma, mb = R.sector_maps(ns, nup, ndw), R.sector_maps(ns, tu, td)
            ia, ib = R.fock_index(ma, ns), R.fock_index(mb, ns)
            block = op[np.ix_(ib, ia)]
            mine = np.stack([R.apply(ma, mb, terms, cu, cd, e) for e in np.eye(ia.size)], axis=1)
            # one constant sign for the whole pair of sectors: the dw operator passes the nup up particles of the source
            sign = (-1.0) ** nup
            assert np.abs(block).max() > 0 or np.abs(mine).max() == 0
            assert np.allclose(mine, sign * block, atol=1e-14), (ns, cu, cd, nup, ndw)
            # nothing of the operator leaves the target sector
            rest = np.delete(op[:, ia], ib, axis=0)
            assert np.abs(rest).max() == 0


@pytest.mark.parametrize("ns", [3, 4])
def test_hermiticity_relation_holds_for_random_vectors(ns):
    rng = np.random.default_rng(10 + ns)
    for cu, cd in FLAGS:
        terms = _terms(rng, ns, 4)
        nup, ndw = (1 if not cu else ns - 2), (2 if not cd else 1)
        tu, td = nup + (1 if cu else -1), ndw + (1 if cd else -1)
        ma, mb = R.sector_maps(ns, nup, ndw), R.sector_maps(ns, tu, td)
        psi = rng.standard_normal(len(ma[0]) * len(ma[1])) + 1j * rng.standard_normal(len(ma[0]) * len(ma[1]))
        phi = rng.standard_normal(len(mb[0]) * len(mb[1])) + 1j * rng.standard_normal(len(mb[0]) * len(mb[1]))
        lhs = np.vdot(phi, R.apply(ma, mb, terms, cu, cd, psi))
        rhs = np.conj(np.vdot(psi, R.apply(mb, ma, R.dagger(terms), not cu, not cd, phi)))
        assert abs(lhs - rhs) <= 1e-13 * sum(abs(c) for _, _, c in terms) * np.linalg.norm(psi) * np.linalg.norm(phi)


def test_chi_formula_equals_a_dense_lehmann_sum_with_fock_matrices():
    """a random Hermitian number-conserving H on ns = 3: chi from the restatement's sector-wise sums equals the textbook
    -[<psi|O (z - (H - E))^-1 O^+|psi> - <psi|O^+ (z + (H - E))^-1 O|psi>] with 64 x 64 matrices"""
    ns, rng = 3, np.random.default_rng(5)
    n = 2 * ns
    c = [R.fock_c(n, k) for k in range(n)]
    H = np.zeros((2 ** n, 2 ** n), dtype=complex)
    for s in (0, 1):
        t = rng.standard_normal((ns, ns)) + 1j * rng.standard_normal((ns, ns))
        t = t + t.conj().T
        for i in range(ns):
            for j in range(ns):
                H += t[i, j] * c[s * ns + i].T @ c[s * ns + j]
    for i in range(ns):
        H += 1.7 * (c[i].T @ c[i]) @ (c[ns + i].T @ c[ns + i])
    nup, ndw = 2, 1
    maps = R.sector_maps(ns, nup, ndw)
    idx = R.fock_index(maps, ns)
    w, U = np.linalg.eigh(H[np.ix_(idx, idx)])
    psi, e0 = U[:, 0], w[0]
    z = 1j * R.NU[:8] + 0.05
    for cu, cd in FLAGS:
        ops = [_terms(rng, ns, 3), _terms(rng, ns, 2)]
        sides = []
        for lower in (False, True):
            fu, fd = (cu, cd) if lower else (not cu, not cd)
            tu, td = nup + (1 if fu else -1), ndw + (1 if fd else -1)
            if not (0 <= tu <= ns and 0 <= td <= ns):
                sides.append(None)
                continue
            mb = R.sector_maps(ns, tu, td)
            ib = R.fock_index(mb, ns)
            wb, Ub = np.linalg.eigh(H[np.ix_(ib, ib)])
            sides.append((wb, Ub, [R.apply(maps, mb, op if lower else R.dagger(op), fu, fd, psi) for op in ops]))
        chi = R.lehmann_chi(e0, sides[0], sides[1], z)
        full = np.zeros(2 ** n, dtype=complex)
        full[idx] = psi
        O = [R.fock_operator(ns, op, cu, cd) for op in ops]
        eye = np.eye(2 ** n)
        for k, zz in enumerate(z):
            g1, g2 = np.linalg.inv(zz * eye - (H - e0 * eye)), np.linalg.inv(zz * eye + (H - e0 * eye))
            for a in range(2):
                for b in range(2):
                    ref = -(full.conj() @ O[a] @ g1 @ O[b].conj().T @ full - full.conj() @ O[b].conj().T @ g2 @ O[a] @ full)
                    assert abs(chi[k, a, b] - ref) <= 1e-11 * max(1.0, abs(ref)), (cu, cd, k, a, b)


@pytest.mark.parametrize("name", ["plaquette", "chain"])
def test_spin_symmetric_fixtures_have_a_singlet_ground_state(name):
    m, (nup, ndw), real = R.chi_fixture(name)
    w, _, _ = R.dense_sector(m, nup, ndw)
    w_flip, _, _ = R.dense_sector(m, nup + 1, ndw - 1)
    assert real and nup == ndw
    assert w[1] - w[0] > 1e-6                                    # non-degenerate in its own sector ...
    assert w_flip[0] - w[0] >= 1e-6                              # ... and no partner at S^z = 1: a singlet


@pytest.mark.parametrize("name,kinds", [("plaquette", "pair flip"), ("chain", "pair flip"), ("square", "pair"), ("bhz", "pair")])
def test_fixture_levels_stay_away_from_zero(name, kinds):
    m, (nup, ndw), _ = R.chi_fixture(name)
    w, _, _ = R.dense_sector(m, nup, ndw)
    nb = R.neighbours(m.Ns, nup, ndw)
    for (du, dd), s in nb.items():
        if s is None or ("pair" if du == dd else "flip") not in kinds:
            continue
        e = R.dense_sector(m, *s)[0] - w[0]
        print(f"{name} {s}: min|e_n| = {np.abs(e).min():.3e}")
        assert np.abs(e).min() >= 1e-2, (name, s)
