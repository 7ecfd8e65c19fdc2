"""The two host routines of hxv_eigh_lowest on the CPU (tests/host/eigh_small_check.cpp over csrc/hxv_eigh_host.hpp): jacobi_eigh, which
diagonalises the projected matrix of every restart, and keep_count, which decides how much of the basis a restart keeps.  The program is
stand-alone (its own main, no HIP); it is built plainly and with -fsanitize=address,undefined and run directly.

jacobi_eigh, over the matrix set of matrices(): `done` is set, w ascends, and with u = 2**-53 (residuals evaluated in long double)
    ||Z^T Z - I||_F <= c n u,      ||A Z - Z diag(w)||_F <= c n u ||A||_F,      max|w - eigvalsh(A)| <= c n u ||A||_F.
c is not chosen here: it is 8 times the worst value LAPACK (numpy.linalg.eigh) itself reaches for the same three quantities, in the
same units, over the same matrices, and not below 8 (cyclic Jacobi and QL / divide-and-conquer are both backward stable; a constant
factor between them is expected).  Measured with numpy.linalg.eigh on these matrices (test_lapack_yardstick prints them again):
    orthogonality 2.68 n u (tiny_offdiagonal6),   residual 0.831 n u ||A||_F (tiny_offdiagonal6),   eigenvalues 0.177 n u ||A||_F (arrow20_repeated)
    -> worst 2.68, c = 8 * 2.68 = 21.4  (C_BOUND).
jacobi_eigh itself reaches 18.9 (arrow64_separated) / 2.43 (arrow64_separated) / 1.30 (graded12) in these units.

keep_count, for all 2 <= m <= 64, 1 <= neigen < m, 0 <= nconv <= neigen, pct in {5, 20, 80}: 1 <= k <= m - 1, k >= min(neigen, m - 1),
k non-decreasing in pct and in nconv."""
import subprocess

import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
C_BOUND = 21.4


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------------
def arrow(n, k, theta, seed):
    """what the driver forms at a restart: the k kept Ritz values on the diagonal, the arrow (row and column k), a tridiagonal tail"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    A[np.arange(k), np.arange(k)] = theta
    A[k, :k] = A[:k, k] = rng.uniform(-1.0, 1.0, k) * 10.0 ** rng.uniform(-8, 0, k)     # beta_m s_mi: from converged to not at all
    for j in range(k, n):
        A[j, j] = rng.uniform(-2.0, 2.0)
        if j + 1 < n:
            A[j, j + 1] = A[j + 1, j] = rng.uniform(0.1, 1.5)
    return A


def matrices():
    out = {"n1": np.array([[3.5]]), "zero5": np.zeros((5, 5)), "diagonal6": np.diag([3.0, -1.0, 2.0, 2.0, 0.0, -7.5]),
           "equal_diagonal_2x2": np.array([[1.0, 0.5], [0.5, 1.0]])}
    for n, k in ((20, 8), (64, 24)):
        out[f"arrow{n}_separated"] = arrow(n, k, -3.0 + 0.25 * np.arange(k), 1)
        out[f"arrow{n}_clustered"] = arrow(n, k, -3.0 + 1e-14 * np.arange(k), 2)
        out[f"arrow{n}_repeated"] = arrow(n, k, -3.0 + 0.5 * (np.arange(k) // 2), 3)
    rng = np.random.default_rng(4)
    d = np.logspace(-12, 0, 12)
    B = rng.uniform(-1.0, 1.0, (12, 12))
    out["graded12"] = (B + B.T) * np.sqrt(np.outer(d, d))                  # |a_ij| ~ sqrt(d_i d_j): from 1e-12 to 1
    out["tiny_offdiagonal6"] = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) + 1e-305 * (np.ones((6, 6)) - np.eye(6))
    out["wilkinson21"] = np.diag(np.abs(np.arange(21) - 10.0)) + np.diag(np.ones(20), 1) + np.diag(np.ones(20), -1)
    for name, A in out.items():
        assert np.array_equal(A, A.T), name
    return out


def quality(A, w, Z, w_ref):
    """-> (orthogonality / (n u), residual / (n u ||A||_F), eigenvalue error / (n u ||A||_F)); a zero matrix must give exact zeros there"""
    n = A.shape[0]
    Al, wl, Zl = A.astype(LD), w.astype(LD), Z.astype(LD)
    orth = float(np.sqrt(np.sum((Zl.T.dot(Zl) - np.eye(n, dtype=LD)) ** 2)))
    res = float(np.sqrt(np.sum((Al.dot(Zl) - Zl * wl[None, :]) ** 2)))
    ev = float(np.max(np.abs(wl - w_ref.astype(LD))))
    nrm = float(np.sqrt(np.sum(Al ** 2)))
    if nrm == 0.0:
        assert res == 0.0 and ev == 0.0
        return orth / (n * U), 0.0, 0.0
    return orth / (n * U), res / (n * U * nrm), ev / (n * U * nrm)


# ---- driving the program --------------------------------------------------------------------------------------------------------------------
def write_matrices(path, mats):
    with open(path, "w") as f:
        for A in mats:
            f.write(f"{A.shape[0]}\n" + " ".join(float(x).hex() for x in A.T.ravel()) + "\n")      # column-major
    return path


def run_eigh(exe, path, env=None):
    """-> (exit status, [(done, w, Z)], stderr)"""
    p = subprocess.run([str(exe), "eigh", str(path)], capture_output=True, text=True, env=env)
    out = []
    for line in p.stdout.splitlines():
        head, ws, zs = line.split("|")
        done, n = (int(t.split("=")[1]) for t in head.split())
        w = np.array([float.fromhex(t) for t in ws.split()])
        Z = np.array([float.fromhex(t) for t in zs.split()]).reshape(n, n).T                    # column-major
        assert w.shape == (n,)
        out.append((done, w, Z))
    return p.returncode, out, p.stderr


def _no_report(err):
    return not any(s in err for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY:"))


def check_eigh(exe, tmp_path):
    mats = matrices()
    rc, out, err = run_eigh(exe, write_matrices(tmp_path / "matrices.txt", mats.values()))
    assert rc == 0 and _no_report(err), (rc, err[-3000:])
    assert len(out) == len(mats)
    worst = [0.0, 0.0, 0.0]
    for (name, A), (done, w, Z) in zip(mats.items(), out):
        assert done == 1, (name, "jacobi_eigh did not converge")
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(Z)), name
        assert np.all(np.diff(w) >= 0), (name, "w does not ascend", w)
        q = quality(A, w, Z, np.linalg.eigvalsh(A))
        print(f"jacobi_eigh {name}: orthogonality {q[0]:.3g} n u, residual {q[1]:.3g} n u |A|, eigenvalues {q[2]:.3g} n u |A|")
        worst = [max(a, b) for a, b in zip(worst, q)]
        for what, v in zip(("orthogonality", "residual", "eigenvalues"), q):
            assert v <= C_BOUND, (name, what, v, "in units of n u (|A|_F)")
    print(f"jacobi_eigh worst: {worst[0]:.3g} / {worst[1]:.3g} / {worst[2]:.3g}  (bound {C_BOUND})")


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
def test_lapack_yardstick():
    """C_BOUND is 8 times what numpy.linalg.eigh reaches on the same matrices in the same units, and not below 8 (header comment).  LAPACK's
    rounding errors depend on the BLAS kernels of the CPU it runs on, so the constant is compared with the live figure to a factor of two."""
    worst, where = [0.0, 0.0, 0.0], ["", "", ""]
    for name, A in matrices().items():
        w, Z = np.linalg.eigh(A)
        q = quality(A, w, Z, np.linalg.eigvalsh(A))
        for i in range(3):
            if q[i] > worst[i]:
                worst[i], where[i] = q[i], name
    print("LAPACK: orthogonality %.3g n u (%s), residual %.3g n u |A| (%s), eigenvalues %.3g n u |A| (%s)" %
          (worst[0], where[0], worst[1], where[1], worst[2], where[2]))
    live = max(8.0, 8.0 * max(worst))
    assert 0.5 * live <= C_BOUND <= 2.0 * live, (C_BOUND, live, worst)


def test_jacobi_eigh_plain_build(built, tmp_path):
    check_eigh(built.build_eigh_small_check(), tmp_path)


def test_jacobi_eigh_under_asan_and_ubsan(built, tmp_path):
    """the same matrices and checks with the program compiled with -fsanitize=address,undefined -fno-sanitize-recover=undefined: exit 0 and
    no sanitizer report; then keep_count's whole table.  A stand-alone program, run directly; not on a GPU machine."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_eigh_small_check("address,undefined")
    check_eigh(exe, tmp_path)
    p = subprocess.run([str(exe), "keep", "5", "20", "80"], capture_output=True, text=True)
    assert p.returncode == 0 and _no_report(p.stderr), (p.returncode, p.stderr[-3000:])
    assert p.stdout == subprocess.run([str(built.build_eigh_small_check()), "keep", "5", "20", "80"], capture_output=True, text=True).stdout


def test_jacobi_eigh_refuses_a_wrong_answer(built, tmp_path):
    """the three bounds bite: one eigenvector rotated by 1e-13, or one eigenvalue moved by 1e-13 |A|, is outside them"""
    A = matrices()["arrow20_separated"]
    rc, out, err = run_eigh(built.build_eigh_small_check(), write_matrices(tmp_path / "one.txt", [A]))
    assert rc == 0, err
    _, w, Z = out[0]
    ref = np.linalg.eigvalsh(A)
    assert max(quality(A, w, Z, ref)) <= C_BOUND
    Zt = Z.copy()
    Zt[:, 3] += 1e-13 * Z[:, 4]
    assert quality(A, w, Zt, ref)[0] > C_BOUND
    wt = w.copy()
    wt[5] += 1e-13 * np.linalg.norm(A)
    q = quality(A, wt, Z, ref)
    assert q[1] > C_BOUND and q[2] > C_BOUND


def test_keep_count(built):
    p = subprocess.run([str(built.build_eigh_small_check()), "keep", "5", "20", "80"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    k = {}
    for line in p.stdout.splitlines():
        m, neigen, nconv, pct, kk = (int(t) for t in line.split())
        k[m, neigen, nconv, pct] = kk
    expect = [(m, ne, nc, pct) for pct in (5, 20, 80) for m in range(2, 65) for ne in range(1, m) for nc in range(ne + 1)]
    assert sorted(k) == sorted(expect)
    for (m, ne, nc, pct), kk in k.items():
        assert 1 <= kk <= m - 1, (m, ne, nc, pct, kk)
        assert kk >= min(ne, m - 1), (m, ne, nc, pct, kk)
        if nc > 0:
            assert kk >= k[m, ne, nc - 1, pct], ("not monotone in nconv", m, ne, nc, pct)
        for lo, hi in ((5, 20), (20, 80)):
            if pct == hi:
                assert kk >= k[m, ne, nc, lo], ("not monotone in pct", m, ne, nc, pct)
