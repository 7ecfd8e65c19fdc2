"""The host routines of the Lanczos drivers on the CPU (tests/host/lanczos_host_check.cpp over csrc/hxv_lanczos_host.hpp): tridiag_ql, which
every driver's eigenvalues, Ritz vectors and Green's-function weights go through, LzScale, the host's copy of the fused recurrence's scale
factors, start_norm, and lowest_ritz, the lowest Ritz pair hxv_lanczos_eigh takes from tridiag_ql.  The program is stand-alone (its own main, no HIP); it is built plainly and with -fsanitize=address,undefined
and run directly, nothing is preloaded.

tridiag_ql, over the matrix set of matrices(): the convergence flag is set, and with u = 2**-53 and tol = 8 n u max(|d|, |e|) -- the
backward-error shape of the QL iteration (about n rotations per eigenvalue, each a few roundings of entries no larger than the matrix), not
fitted to this code --
    max|T z - lambda z| <= tol,      max|lambda - LAPACK| <= tol  (scipy.linalg.eigvalsh_tridiagonal by bisection, both sorted; see lapack()),
    max|Z^T Z - I| <= 8 n u min(1, max(|d|, |e|))  (orthogonality has no scale; no matrix of the set has a scale between 0 and 1, and the
    zero matrix must leave Z the identity exactly),
residual and orthogonality evaluated by the program in long double.  Without eigenvectors (z == nullptr) the eigenvalues have the bits of
those with.  A NaN entry returns false in bounded time.  n = 0 is outside tridiag_ql's contract (it writes e[n - 1]) and is never passed;
tests/test_gpu_lanczos_kernels.py asserts that every caller refuses nlanc < 1.
LzScale: begin, next and c() against their definitions in long double, one rounding per operation.  start_norm: snaps exactly the doubles
with |nrm - 1| <= 1e-14 (the difference is exact there; 1e-14 is the double nearest to it).
lowest_ritz: eigenvalue, index and vector have the bits of the sequence it stands for (identity, tridiag_ql, std::min_element), written out in
the program: n = 1, 2, 7, a degenerate lowest pair (the first of the equal eigenvalues is taken), n = 50; a NaN returns false.
Wall time: 6 tests in 3 s; 5 s when the sanitized program has to be built first."""
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from scipy.linalg import eigvalsh_tridiagonal

LD = np.longdouble
U = 2.0 ** -53


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------------
def matrices():
    """name -> (d[n], e[n]) with e[0] unused and e[i] coupling i - 1 and i, as the drivers pass them"""
    rng = np.random.default_rng(20241019)

    def tri(d, off):
        return np.asarray(d, dtype=np.float64), np.concatenate([[0.0], np.asarray(off, dtype=np.float64)])

    out = {"n1": tri([3.5], []), "n2": tri([1.0, -2.0], [1.5]), "n2_equal_diagonal": tri([1.0, 1.0], [4.0]),
           "zero6": tri(np.zeros(6), np.zeros(5)), "zero_diagonal9": tri(np.zeros(9), 1.0 + rng.random(8)),
           "split_in_the_middle10": tri(rng.normal(size=10) * 2, np.where(np.arange(9) == 4, 0.0, 1.0 + rng.random(9))),
           "wilkinson21": tri(np.abs(np.arange(21) - 10.0), np.ones(20))}
    g = np.logspace(-15, 15, 31)
    out["graded_up31"] = tri(g, np.sqrt(g[:-1] * g[1:]))
    out["graded_down31"] = tri(g[::-1], np.sqrt(g[:-1] * g[1:])[::-1])
    out["huge12"] = tri(1e150 * rng.normal(size=12), 1e150 * rng.normal(size=11))
    out["tiny_offdiagonal8"] = tri(np.arange(1.0, 9.0), np.full(7, 1e-300))
    out["constant_diagonal40"] = tri(np.full(40, 1.0), np.full(39, 1e-9))
    for n in (3, 10, 50, 150, 300):
        out[f"random{n}"] = tri(2.0 * rng.normal(size=n), 2.0 * rng.normal(size=n - 1))
    n = 60
    out["lanczos_decaying60"] = tri(rng.uniform(-2.0, 2.0, n), np.logspace(0, -14, n - 1) * rng.uniform(0.5, 1.5, n - 1))
    for name, (d, e) in out.items():
        s = scale(d, e)
        assert d.shape == e.shape and (s == 0.0 or s >= 1.0), name
    return out


def scale(d, e):
    return max(float(np.max(np.abs(d))), float(np.max(np.abs(e[1:]))) if len(e) > 1 else 0.0)


# ---- driving the program --------------------------------------------------------------------------------------------------------------------
def write_matrices(path, mats):
    with open(path, "w") as f:
        for d, e in mats:
            f.write(f"{len(d)}\n" + " ".join(float(x).hex() for x in d) + "\n" + " ".join(float(x).hex() for x in e) + "\n")
    return path


def run_ql(exe, path):
    """-> (exit status, [dict(conv, conv_noz, same, n, res, orth, lam)], stderr)"""
    p = subprocess.run([str(exe), "ql", str(path)], capture_output=True, text=True, timeout=120)
    out = []
    for line in p.stdout.splitlines():
        head, lam = line.split("|")
        r = {k: v for k, v in (t.split("=") for t in head.split())}
        r = {k: (float.fromhex(v) if k in ("res", "orth") else int(v)) for k, v in r.items()}
        r["lam"] = np.array([float.fromhex(t) for t in lam.split()])
        assert r["lam"].shape == (r["n"],)
        out.append(r)
    return p.returncode, out, p.stderr


def _no_report(err):
    return not any(s in err for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY:"))


def bounds(d, e):
    """-> (tol for residual and eigenvalues, tol for orthogonality)"""
    n, s = len(d), scale(d, e)
    return 8 * n * U * s, 8 * n * U * min(1.0, s)


def quality_ok(d, e, r, lam_ref):
    tol, tol_orth = bounds(d, e)
    ev = float(np.max(np.abs(np.sort(r["lam"]).astype(LD) - lam_ref.astype(LD))))
    return r["res"] <= tol and r["orth"] <= tol_orth and ev <= tol, (r["res"], r["orth"], ev, tol, tol_orth)


def lapack(d, e):
    """LAPACK's eigenvalues, ascending, by bisection (dstebz).  The function's default driver (dstemr, MRRR) is itself up to 0.94 of `tol` off on
    these matrices (1.1e-14 on random3, n = 3, measured against bisection in exact rationals, where tridiag_ql is 2.2e-16 off), which would
    leave the comparison no room; bisection is within 0.13 of tol of every other driver on the whole set."""
    return eigvalsh_tridiagonal(d, e[1:], lapack_driver="stebz") if len(d) > 1 else d.copy()


def check_ql(exe, tmp_path):
    mats = matrices()
    rc, out, err = run_ql(exe, write_matrices(tmp_path / "matrices.txt", mats.values()))
    assert rc == 0 and _no_report(err), (rc, err[-3000:])
    assert len(out) == len(mats)
    worst = [0.0, 0.0, 0.0]
    for (name, (d, e)), r in zip(mats.items(), out):
        assert r["n"] == len(d) and r["conv"] == 1 and r["conv_noz"] == 1, (name, "tridiag_ql did not converge")
        assert r["same"] == 1, (name, "the eigenvalues without eigenvectors differ from those with")
        assert np.all(np.isfinite(r["lam"])) and np.isfinite(r["res"]) and np.isfinite(r["orth"]), name
        good, (res, orth, ev, tol, tol_orth) = quality_ok(d, e, r, lapack(d, e))
        print(f"tridiag_ql {name}: residual {res:.3g}, eigenvalues {ev:.3g} (bound {tol:.3g}); orthogonality {orth:.3g} (bound {tol_orth:.3g})")
        if tol > 0:
            worst = [max(a, b) for a, b in zip(worst, (res / tol, ev / tol, orth / tol_orth))]
        assert good, (name, "residual, orthogonality, eigenvalue error", res, orth, ev, "bounds", tol, tol_orth)
    print(f"tridiag_ql worst, as fractions of the bounds: residual {worst[0]:.3g}, eigenvalues {worst[1]:.3g}, orthogonality {worst[2]:.3g}")


def check_nan(exe, tmp_path):
    """a NaN on the diagonal, off it, in the first and in the last place: false, promptly, and nothing for the sanitizers to report"""
    base = matrices()["random50"]
    mats = []
    for where, i in (("d", 0), ("d", 25), ("d", 49), ("e", 1), ("e", 30), ("e", 49)):
        d, e = base[0].copy(), base[1].copy()
        (d if where == "d" else e)[i] = np.nan
        mats.append((d, e))
    mats.append((np.array([np.nan]), np.array([0.0])))           # n = 1: nothing to iterate, the NaN is returned as it is
    rc, out, err = run_ql(exe, write_matrices(tmp_path / "nan.txt", mats))
    assert rc == 0 and _no_report(err), (rc, err[-3000:])
    assert [r["conv"] for r in out] == [0] * 6 + [1] and [r["conv_noz"] for r in out] == [0] * 6 + [1], [(r["conv"], r["conv_noz"]) for r in out]


def check_scale_and_norm(exe, tmp_path):
    rng = np.random.default_rng(7)
    lines = [10.0 ** rng.uniform(-150, 150, 40) for _ in range(4)] + [np.array([1.0, 1.0, 2.0, 0.5])]
    path = tmp_path / "scale.txt"
    path.write_text("".join(" ".join(float(x).hex() for x in ln) + "\n" for ln in lines))
    p = subprocess.run([str(exe), "scale", str(path)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and _no_report(p.stderr), (p.returncode, p.stderr[-3000:])
    one = LD(1)
    rounding = LD(U) * (1 + LD(2.0) ** -10)           # one rounding to double, and the long-double division's own 2**-64
    for ln, got in zip(lines, p.stdout.splitlines()):
        v = np.array([float.fromhex(t) for t in got.split()]).reshape(len(ln), 3)
        s_prev = None
        for k, x in enumerate(ln):
            s, bp, c = v[k]
            assert abs(LD(s) - one / LD(x)) <= rounding * abs(one / LD(x)), ("s_cur = 1 / beta", k)
            if k == 0:
                assert bp == x, "begin: beta_prev = nrm"
            else:
                assert abs(LD(bp) - one / LD(s_prev)) <= rounding * abs(one / LD(s_prev)), ("beta_prev = 1 / s_cur", k)
            prod = np.float64(s) * np.float64(bp)                                     # (an IEEE product: one rounding, checked next)
            assert abs(LD(prod) - LD(s) * LD(bp)) <= rounding * abs(LD(s) * LD(bp))
            assert abs(LD(c) - one / LD(prod)) <= rounding * abs(one / LD(prod)), ("c = 1 / (s_cur beta_prev)", k)
            if k:
                want = LD(x) / LD(ln[k - 1])
                # (five roundings: 1 / beta_{k-1}, its reciprocal, 1 / beta_k, the product, the division; gamma(5) = 5 u (1 + 5 u))
                assert abs(LD(c) - want) <= 5 * LD(U) * (1 + LD(2.0) ** -40) * abs(want), ("c is beta_k / beta_{k-1} to five roundings", k)
            s_prev = s
    # start_norm: every double within 60 ulps of the two edges 1 - 1e-14 and 1 + 1e-14, and some that are far
    xs = [0.0, 1.0, -1.0, 2.0, 0.5, 1e-300, 1e300, float("inf"), 1.0 + 1e-13, 1.0 - 1e-13]
    for edge in (1.0 - 1e-14, 1.0 + 1e-14):
        x = edge
        for _ in range(60):
            x = float(np.nextafter(x, 0.0))
        for _ in range(121):
            xs.append(x)
            x = float(np.nextafter(x, 2.0))
    p = subprocess.run([str(exe), "norm"] + [float(x).hex() for x in xs], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and _no_report(p.stderr), (p.returncode, p.stderr[-3000:])
    got = [float.fromhex(t) for t in p.stdout.split()]
    assert len(got) == len(xs)
    snapped = 0
    for x, y in zip(xs, got):
        inside = np.isfinite(x) and abs(Fraction(x) - 1) <= Fraction(1e-14)
        assert y == (1.0 if inside else x), (x.hex(), y.hex(), inside)
        snapped += bool(inside) and x != 1.0
    assert snapped > 100          # (both edges were really crossed: 45 doubles above 1 and 90 below it snap)
    p = subprocess.run([str(exe), "norm", "nan"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and np.isnan(float.fromhex(p.stdout.split()[0]))


def check_lowest_ritz(exe, tmp_path):
    mats = matrices()
    rng = np.random.default_rng(3)
    d7 = 2.0 * rng.normal(size=7)
    cases = [mats["n1"], mats["n2"], (d7, np.concatenate([[0.0], 0.5 + rng.random(6)])),
             # a degenerate lowest pair: two uncoupled copies of one 3 x 3 block (the first of the equal eigenvalues is taken) ...
             (np.array([1.0, -2.0, 0.5, 1.0, -2.0, 0.5]), np.array([0.0, 1.5, 0.75, 0.0, 1.5, 0.75])),
             # ... and a diagonal matrix with its lowest entry twice
             (np.array([3.0, -1.0, 2.0, -1.0, 5.0]), np.zeros(5)), mats["zero6"], mats["random50"]]
    rc, out, err = _run_ritz(exe, write_matrices(tmp_path / "ritz.txt", cases))
    assert rc == 0 and _no_report(err), (rc, err[-3000:])
    assert len(out) == len(cases)
    for (d, e), r in zip(cases, out):
        assert r["n"] == len(d) and r["ok"] == 1 and r["ok_ref"] == 1 and r["same"] == 1 and r["same_noy"] == 1, r
        assert 0 <= r["j"] < len(d)
    assert out[0]["e"] == 3.5 and out[0]["j"] == 0
    assert out[4]["e"] == -1.0 and out[4]["j"] == 1                     # the first of the two equal lowest entries
    assert abs(out[3]["e"] - lapack(*cases[3])[0]) <= bounds(*cases[3])[0]
    # a NaN: false from the helper as from the written-out sequence, and nothing for the sanitizers to report
    d, e = mats["random50"][0].copy(), mats["random50"][1].copy()
    d[25] = np.nan
    rc, out, err = _run_ritz(exe, write_matrices(tmp_path / "ritz_nan.txt", [(d, e), (np.array([1.0, np.nan]), np.array([0.0, 1.0]))]))
    assert rc == 0 and _no_report(err), (rc, err[-3000:])
    assert [(r["ok"], r["ok_ref"]) for r in out] == [(0, 0), (0, 0)], out


def _run_ritz(exe, path):
    p = subprocess.run([str(exe), "ritz", str(path)], capture_output=True, text=True, timeout=120)
    out = []
    for line in p.stdout.splitlines():
        r = {k: v for k, v in (t.split("=") for t in line.split())}
        out.append({k: (float.fromhex(v) if k == "e" else int(v)) for k, v in r.items()})
    return p.returncode, out, p.stderr


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
def test_tridiag_ql_plain_build(built, tmp_path):
    check_ql(built.build_lanczos_host_check(), tmp_path)


def test_tridiag_ql_nan_plain_build(built, tmp_path):
    check_nan(built.build_lanczos_host_check(), tmp_path)


def test_lzscale_and_start_norm_plain_build(built, tmp_path):
    check_scale_and_norm(built.build_lanczos_host_check(), tmp_path)


def test_lowest_ritz_plain_build(built, tmp_path):
    check_lowest_ritz(built.build_lanczos_host_check(), tmp_path)


def test_host_routines_under_asan_and_ubsan(built, tmp_path):
    """the same four checks with the program compiled with -fsanitize=address,undefined -fno-sanitize-recover=undefined: exit 0 and no
    sanitizer report.  A stand-alone program, run directly; not on a GPU machine."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = built.build_lanczos_host_check("address,undefined")
    check_ql(exe, tmp_path)
    check_nan(exe, tmp_path)
    check_scale_and_norm(exe, tmp_path)
    check_lowest_ritz(exe, tmp_path)


def test_bounds_refuse_a_wrong_answer(built, tmp_path):
    """the bounds bite: an eigenvalue moved by 1e-12 of the scale, a residual or an orthogonality defect of that size, a lost eigenvalue"""
    d, e = matrices()["random50"]
    rc, out, err = run_ql(built.build_lanczos_host_check(), write_matrices(tmp_path / "one.txt", [(d, e)]))
    assert rc == 0, err
    r, ref = out[0], lapack(d, e)
    assert quality_ok(d, e, r, ref)[0]
    s = scale(d, e)
    for key, val in (("res", 1e-12 * s), ("orth", 1e-12)):
        assert not quality_ok(d, e, dict(r, **{key: val}), ref)[0], key
    lam = r["lam"].copy()
    lam[7] += 1e-12 * s
    assert not quality_ok(d, e, dict(r, lam=lam), ref)[0]
    lam = r["lam"].copy()
    lam[3] = lam[4]
    assert not quality_ok(d, e, dict(r, lam=lam), ref)[0]
