"""The references of the observables and density-operator kernel tests shown to bite, without a GPU (tests/observables_kernels_ref.py,
tests/density_ops_kernels_ref.py; the device runs are tests/test_gpu_observables_kernels.py and tests/test_gpu_density_ops_kernels.py).

1. The refs' evaluation -- the numpy sums over the tables that check(case, got) compares a device buffer with -- against explicit
   Jordan-Wigner operators: c_k as spin_pair_ref.fock_c defines it (sign = parity of the occupied modes below k; up orbital o = mode o, dw
   orbital o = mode Ns + o, the sector's states at spin_pair_ref.fock_index).  A dense matrix of Ns = 6 has 2^24 entries, so the operator
   acts on a vector by index arithmetic here, and that form is compared with the dense matrices on 8 modes (Ns = 4) first.  Tables built the builder's way for Ns 4 .. 6 and Nimp 1, 3 and Ns must reproduce W, R_up, R_dw,
   (f_a - m_a) psi, the sums behind the means and the norms EXACTLY on integer states.
2. The evaluation passes its own check on the cases the GPU tests run, in both number formats.
3. For every planted fault, the buffers a kernel with that fault would leave are refused on at least one case of every kernel it can sit
   in, in BOTH number formats: the exact comparison and the derived bounds are tight enough to see it."""
import numpy as np
import pytest

import density_ops_kernels_ref as DR
import observables_kernels_ref as OR
import spin_pair_ref as SP


def jw_apply(nmodes, k, create, vec):
    """c_k (create False) or c_k^dagger on a vector over the 2^nmodes Fock states, index = sum_k n_k 2^k"""
    n = np.arange(1 << nmodes)
    occ = (n >> k) & 1
    src = n[occ == (0 if create else 1)]  # states the operator does not kill
    sign = 1 - 2 * (np.array([bin(int(x) & ((1 << k) - 1)).count("1") for x in src]) & 1)
    out = np.zeros_like(vec)
    out[src ^ (1 << k)] = sign * vec[src]
    return out


def test_index_form_is_the_matrix_form():
    rng = np.random.default_rng(5)
    v = rng.integers(-4, 5, 256) + 1j * rng.integers(-4, 5, 256)
    for k in range(8):
        c = SP.fock_c(8, k)
        assert np.array_equal(jw_apply(8, k, False, v), c @ v) and np.array_equal(jw_apply(8, k, True, v), c.T @ v)


SECTORS = [(4, 2, 2), (4, 1, 3), (5, 2, 3), (6, 3, 2)]


def _state(ns, nup, ndw, seed):
    mu, md = SP.sector_maps(ns, nup, ndw)
    rng = np.random.default_rng(seed)
    psi = (rng.integers(-6, 7, (len(md), len(mu))) + 1j * rng.integers(-6, 7, (len(md), len(mu)))).astype(np.complex128)
    full = np.zeros(1 << (2 * ns), dtype=np.complex128)
    full[SP.fock_index((mu, md), ns)] = psi.reshape(-1)
    return mu, md, psi, full


@pytest.mark.parametrize("ns,nup,ndw", SECTORS)
def test_observables_evaluation_against_jordan_wigner_operators(ns, nup, ndw):
    mu, md, psi, full = _state(ns, nup, ndw, 11 * ns + nup)
    n = np.arange(1 << (2 * ns))
    for nimp in sorted({1, 3, ns}):
        nw, npair = 1 << nimp, nimp * nimp
        rec = OR.record(OR.build_tables(mu, md, nimp), psi)
        # the occupation of a mode: the diagonal of c^+ c
        occ = [np.real(jw_apply(2 * ns, k, True, jw_apply(2 * ns, k, False, np.ones(len(n), dtype=np.complex128)))).astype(np.int64) for k in range(2 * ns)]
        a_up = sum(occ[i] << i for i in range(nimp))
        a_dw = sum(occ[ns + i] << i for i in range(nimp))
        W = np.bincount(a_up + nw * a_dw, weights=full.real ** 2 + full.imag ** 2, minlength=nw * nw)
        want = np.zeros(nw * nw + 4 * npair)
        want[:nw * nw] = W
        for spin in (0, 1):
            for js in range(nimp):
                for i in range(js):  # the device computes is < js; the rest of R stays zero for the host
                    r = np.vdot(full, jw_apply(2 * ns, spin * ns + i, True, jw_apply(2 * ns, spin * ns + js, False, full)))
                    q = nw * nw + 2 * npair * spin + 2 * (i + nimp * js)
                    want[q], want[q + 1] = r.real, r.imag
        assert np.array_equal(rec.astype(np.float64), want), (ns, nimp)


def _dop_case(mu, md, psi, nimp, nops, seed, kind, m=None):
    rng = np.random.default_rng(seed)
    qdw, dimup = psi.shape
    pitch = (dimup + 7) // 8 * 8
    nchunk, rows = DR.chunking(pitch)
    p = np.full((qdw + 1, pitch), DR.CNAN)
    p[:qdw, :dimup] = psi
    occ_up = np.zeros(pitch, dtype=np.uint32)
    occ_up[:dimup] = mu & ((1 << nimp) - 1)
    occ_dw = np.concatenate([md & ((1 << nimp) - 1), [0]]).astype(np.uint32)
    coef = rng.integers(-3, 4, (nops, 2, nimp)).astype(np.float64)
    return dict(kind=kind, dimup=dimup, pitch=pitch, nchunk=nchunk, rows=rows, qdw=qdw, grid=2, nimp=nimp, nops=nops, integer=True, psi=p,
                occ_up=occ_up, occ_dw=occ_dw, coef=coef, m=np.zeros(nops) if m is None else m, partial0=np.full((3, DR.DOP_NSUM), DR.SENT),
                outs0=np.full((nops, qdw + 1, pitch), DR.CSENT) if kind == "apply" else None)


@pytest.mark.parametrize("ns,nup,ndw", SECTORS)
def test_density_ops_evaluation_against_jordan_wigner_operators(ns, nup, ndw):
    mu, md, psi, full = _state(ns, nup, ndw, 7 * ns + ndw)
    idx = SP.fock_index((mu, md), ns)
    for nimp in sorted({1, 3, ns}):
        nops = 3
        case = _dop_case(mu, md, psi, nimp, nops, ns + nimp, "sums")
        (partial,) = DR.evaluate(case)
        m = np.array([2.0, -3.0, 1.0])
        acase = dict(_dop_case(mu, md, psi, nimp, nops, ns + nimp, "apply", m))
        outs, apart = DR.evaluate(acase)
        for a in range(nops):
            # O_a = sum_is cu n_is,up + cd n_is,dw as Jordan-Wigner operators on the full vector
            Opsi = np.zeros_like(full)
            for spin in (0, 1):
                for i in range(nimp):
                    Opsi += case["coef"][a, spin, i] * jw_apply(2 * ns, spin * ns + i, True, jw_apply(2 * ns, spin * ns + i, False, full))
            assert partial[:2, a].sum() == np.vdot(full, Opsi).real and np.vdot(full, Opsi).imag == 0.0, (ns, nimp, a)
            want = (Opsi - m[a] * full)[idx].reshape(psi.shape)
            assert np.array_equal(outs[a, :-1, :psi.shape[1]], want), (ns, nimp, a)
            assert np.all(outs[a, :-1, psi.shape[1]:] == 0.0)
            assert apart[:2, a].sum() == np.vdot(want, want).real, (ns, nimp, a)
        assert partial[:2, DR.DOP_MAX].sum() == np.vdot(full, full).real
        assert DR.check(case, (partial,)) == [] and DR.check(acase, (outs, apart)) == []


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------------------
def obs_cases(integer, small=True):
    """(kernel name, case) as tests/test_gpu_observables_kernels.py makes them; small: one Nimp = 10 case per kernel (the others cost the CPU
    seconds and add no new path to the evaluation)"""
    out, seen = [], set()
    for k, c in enumerate(OR.rows_cases()):
        for pairs in (False, True):
            if small and c[0] == 10 and ("rows", pairs) in seen:
                continue
            if c[0] == 10:
                seen.add(("rows", pairs))
            out.append(("rows_pairs" if pairs else "rows_w", OR.make_rows(100 + k, *c, pairs, integer)))
    out += [("rdw", OR.make_rdw(300 + k, *c, integer)) for k, c in enumerate(OR.rdw_cases())]
    for k, c in enumerate(OR.reduce_cases()):
        if small and c[0] == 10 and c[1:] != (257, False):
            continue
        out.append(("reduce", OR.make_reduce(500 + k, *c, integer)))
    return out


def dop_cases(integer):
    out = [(kind, DR.make_pass(700 + k, kind, *c, integer)) for kind in ("sums", "apply") for k, c in enumerate(DR.pass_cases())]
    return out + [("reduce", DR.make_reduce(900 + k, *c, integer)) for k, c in enumerate(DR.reduce_cases())]


@pytest.fixture(scope="module", params=[True, False], ids=["integers", "normal-deviates"])
def cases(request):
    return request.param, obs_cases(request.param), dop_cases(request.param)


def test_the_evaluation_passes_its_own_check(cases):
    _, obs, dop = cases
    for name, case in obs:
        assert OR.check(case, OR.evaluate(case)) == [], (name, case["nimp"], case["qdw"])
    for name, case in dop:
        assert DR.check(case, DR.evaluate(case)) == [], (name, {k: v for k, v in case.items() if np.isscalar(v)})


# fault -> the kernels it can sit in
OBS_FAULTS = {"conj": ("rows_pairs", "rdw"), "sign": ("rows_pairs", "rdw"), "transpose": ("rows_pairs", "rdw"),
              "boundary": ("rows_w", "rows_pairs", "rdw", "reduce"), "trip": ("rows_w", "rows_pairs", "rdw", "reduce"), "adw": ("reduce",)}
DOP_FAULTS = {"hi": ("sums", "apply"), "chunk": ("sums", "apply"), "item1": ("sums", "apply"), "pad": ("apply",), "trip": ("sums", "apply", "reduce")}


def test_every_planted_fault_is_refused(cases):
    """conjugate swapped, a sign dropped, is/js transposed, a group boundary off by one, the last lane trip dropped, a_dw = o >> (nimp-1);
    the high 5-bit half ignored, the last chunk skipped, item += 1 instead of += grid, pad rows left unwritten"""
    integer, obs, dop = cases
    assert set(OBS_FAULTS) == set(OR.FAULTS) and set(DOP_FAULTS) == set(DR.FAULTS)
    for R, lst, faults in ((OR, obs, OBS_FAULTS), (DR, dop, DOP_FAULTS)):
        for fault, kernels in faults.items():
            for kern in kernels:
                caught = sum(bool(R.check(case, R.evaluate(case, fault))) for name, case in lst if name == kern)
                assert caught > 0, (fault, kern, "integers" if integer else "normal deviates")
