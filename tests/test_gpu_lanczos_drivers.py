"""The host side of the Lanczos and Chebyshev drivers (csrc/hxv_lanczos.hip, csrc/hxv_chebyshev.hip) at the places a change of their loops, of
their runner or of their argument checks would show first.  Everything here is bits or literals: no tolerance.

  - short and boundary lengths: hxv_lanczos_tridiag with lanczos_graph 1 and 0 gives the same alanc / blanc / nsteps for nlanc in
    1, 2, 3, 7, 8, 9, 10, 11 -- both sides of the threshold of the device-only run (nlanc >= 8) and every remainder of its three-step
    rotation -- with real_vectors 1 and 0.  (tests/test_gpu_lanczos.py::test_graph_captured_tridiagonalisation_equals_the_stepwise_one
    compares the two at nlanc 25 .. 40 only.)
  - hxv_lanczos_tridiag_pair and hxv_lanczos_tridiag_pair_probes (1 and 3 probes) against the two single runs (real_vectors = 0) for nlanc in
    1, 2, 3, and at Dim 36 with one component an eigenvector and nlanc = 40: the WHOLE output arrays of the C entries, the zeros past each
    breakdown and both nsteps included.  (tests/test_gpu_pair_probes.py and tests/test_gpu_lanczos.py compare the steps both runs made, at
    nlanc 25 .. 40.)
  - refusals, word for word: return code and hxv_last_error() of the four probe-taking entries and of the four Chebyshev entries against
    literals taken from the source, and after each refusal a good call on the same handle gives the bits it gave before.
Sectors: hm_1dchain(Nlat=2, Nbath=2) (3,3), Dim 400, and hm_1dchain(Nlat=2, Nbath=1) (2,2), Dim 36, where Krylov spaces close."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
FILL = 7.0          # what the output arrays hold before a call: an entry the driver does not write shows


def _p(x):
    return x.ctypes.data_as(PD)


def _unit(x):
    return x / np.linalg.norm(x)


def _plist(probes):
    return (C.c_void_p * max(len(probes), 1))(*[p.data_ptr() for p in probes])


def _single(L, sec, vin, probes, nl):
    """hxv_lanczos_tridiag_probes itself -> whole alanc[nl], blanc[nl], overlaps[2 nl nprobes], nsteps"""
    import torch

    torch.cuda.synchronize()
    a, b, ov, n = np.full(nl, FILL), np.full(nl, FILL), np.full(2 * nl * max(len(probes), 1), FILL), C.c_int32(-1)
    rc = L.hxv_lanczos_tridiag_probes(sec._h, vin.data_ptr(), len(probes), _plist(probes), nl, _p(a), _p(b), _p(ov), 1e-12, C.byref(n))
    assert rc == 0, L.hxv_last_error()
    return a, b, ov[: 2 * nl * len(probes)], n.value


def _pair(L, sec, va, vb, probes, nl, entry="probes"):
    """hxv_lanczos_tridiag_pair_probes (or, entry = "pair", hxv_lanczos_tridiag_pair) itself -> the same four of a and of b"""
    import torch

    torch.cuda.synchronize()
    arr = [np.full(nl, FILL) for _ in range(4)]
    ovs = [np.full(2 * nl * max(len(probes), 1), FILL) for _ in range(2)]
    na, nb = C.c_int32(-1), C.c_int32(-1)
    if entry == "pair":
        assert not probes
        rc = L.hxv_lanczos_tridiag_pair(sec._h, va.data_ptr(), vb.data_ptr(), nl, _p(arr[0]), _p(arr[1]), _p(arr[2]), _p(arr[3]), 1e-12,
                                        C.byref(na), C.byref(nb))
    else:
        rc = L.hxv_lanczos_tridiag_pair_probes(sec._h, va.data_ptr(), vb.data_ptr(), len(probes), _plist(probes), nl, _p(arr[0]), _p(arr[1]),
                                               _p(ovs[0]), _p(arr[2]), _p(arr[3]), _p(ovs[1]), 1e-12, C.byref(na), C.byref(nb))
    assert rc == 0, L.hxv_last_error()
    k = 2 * nl * len(probes)
    return (arr[0], arr[1], ovs[0][:k], na.value), (arr[2], arr[3], ovs[1][:k], nb.value)


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


# ---- 1. short and boundary lengths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real_vectors", [1, 0])
def test_device_only_run_equals_the_host_stepped_one_at_short_lengths(built, real_vectors):
    import hxv
    from hxv import models

    sec = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2), 3, 3)
    assert sec.Dim == 400 and sec.real_vectors_available
    dv = sec.vector_from_host(_unit(np.random.default_rng(11).standard_normal(sec.Dim)).astype(np.complex128))
    sec.set_option("real_vectors", real_vectors)
    for nl in (1, 2, 3, 7, 8, 9, 10, 11):
        got = []
        for graph in (1, 0):
            sec.set_option("lanczos_graph", graph)
            got.append(sec.lanczos_tridiag(dv, nl))
            assert sec.get_option("lanczos_real_last") == real_vectors
        (a1, b1, n1), (a0, b0, n0) = got
        assert n1 == n0 == nl, (nl, n1, n0)
        assert np.array_equal(a1, a0) and np.array_equal(b1, b0), (nl, np.abs(a1 - a0).max(), np.abs(b1 - b0).max())
        assert b1[0] == 0.0 and np.all(np.isfinite(a1)) and (nl == 1 or b1[1:].min() > 0.0)
    sec.close()


# ---- 2. the paired drivers against two single runs, whole arrays --------------------------------------------------------------------------
@pytest.mark.parametrize("nprobes", [0, 1, 3])
def test_paired_run_is_two_single_runs_in_the_whole_arrays_at_short_lengths(built, nprobes):
    import hxv
    from hxv import models

    L = hxv.load_library()
    sec = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2), 3, 3)
    assert sec.Dim == 400
    rng = np.random.default_rng(12)
    da, db = (sec.vector_from_host((s * _unit(rng.standard_normal(sec.Dim))).astype(np.complex128)) for s in (3.0, 0.25))   # unequal norms
    probes = [sec.vector_from_host(rng.standard_normal(sec.Dim).astype(np.complex128)) for _ in range(nprobes)]
    sec.set_option("real_vectors", 0)
    sec.set_option("lanczos_graph", 0)
    for nl in (1, 2, 3):
        ra, rb = _pair(L, sec, da, db, probes, nl)
        assert sec.get_option("lanczos_real_last") == 2
        for got, vin in ((ra, da), (rb, db)):
            one = _single(L, sec, vin, probes, nl)
            assert sec.get_option("lanczos_real_last") == 0
            assert got[3] == one[3] == nl
            assert _same(got, one), (nl, nprobes)
            assert not np.any(got[0] == FILL) and not np.any(got[2] == FILL)      # every entry was written
        if nprobes == 0:
            assert _same(_pair(L, sec, da, db, [], nl, entry="pair")[0], ra) and _same(_pair(L, sec, da, db, [], nl, entry="pair")[1], rb)
    sec.close()


@pytest.mark.parametrize("nprobes", [0, 1, 3])
def test_paired_run_with_a_breakdown_in_one_component_in_the_whole_arrays(built, nprobes):
    """Dim 36, nlanc = 40: component a is an eigenvector and stops after its first step, b goes on alone until its Krylov space closes"""
    import hxv
    from hxv import models
    from oracle.oracle import OracleSector

    L = hxv.load_library()
    m, nl = models.hm_1dchain(Nlat=2, Nbath=1), 40
    sec = hxv.HxvSector.from_model(m, 2, 2)
    assert sec.Dim == 36
    rng = np.random.default_rng(13)
    w, U = np.linalg.eigh(OracleSector(m, 2, 2).dense())
    xa = _unit(np.real(U[:, 3] * np.exp(-1j * np.angle(U[np.abs(U[:, 3]).argmax(), 3]))))
    da, db = sec.vector_from_host(xa.astype(np.complex128)), sec.vector_from_host(_unit(rng.standard_normal(36)).astype(np.complex128))
    probes = [sec.vector_from_host(rng.standard_normal(36).astype(np.complex128)) for _ in range(nprobes)]
    sec.set_option("real_vectors", 0)
    sec.set_option("lanczos_graph", 0)
    ra, rb = _pair(L, sec, da, db, probes, nl)
    assert sec.get_option("lanczos_real_last") == 2
    assert ra[3] < 5 and ra[3] < rb[3], (ra[3], rb[3])
    for got, vin in ((ra, da), (rb, db)):
        one = _single(L, sec, vin, probes, nl)
        assert _same(got, one), (nprobes, got[3], one[3])
        n = got[3]
        assert not got[0][n:].any() and not got[1][n + 1:].any() and not got[2][2 * n * nprobes:].any()     # zeros past the breakdown
    if nprobes == 0:
        pa, pb = _pair(L, sec, da, db, [], nl, entry="pair")
        assert _same(pa, ra) and _same(pb, rb)
    sec.close()


# ---- 3. refusals, word for word -----------------------------------------------------------------------------------------------------------
NL, A, B = 6, 30.0, 0.0        # steps / orders of the good calls; a window that holds the spectrum of the Dim-400 sector with room to spare


@pytest.fixture(scope="module")
def chain400(built):
    import hxv
    from hxv import models

    sec = hxv.HxvSector.from_model(models.hm_1dchain(Nlat=2, Nbath=2), 3, 3)
    assert sec.Dim == 400
    rng = np.random.default_rng(14)
    v, w, p0, p1 = (sec.vector_from_host(rng.standard_normal(400).astype(np.complex128)) for _ in range(4))       # real: every entry takes them
    yield dict(sec=sec, L=hxv.load_library(), v=v, w=w, p=[p0, p1])
    sec.close()


def _refused(L, rc, text):
    assert rc == 1, (rc, text, L.hxv_last_error())          # HXV_ERR_ARG
    assert L.hxv_last_error().decode() == text, (L.hxv_last_error().decode(), text)


def _probe_entry_calls(c, who):
    """-> call(nprobes, list, out): the entry `who` with everything else good; good() -> the bytes of a good call's outputs"""
    import torch

    sec, L, v, w, p = c["sec"], c["L"], c["v"], c["w"], c["p"]
    h = sec._h
    arr = [np.zeros(NL) for _ in range(4)]
    out = [np.zeros(2 * NL * 2) for _ in range(2)]
    smom = np.zeros(2 * NL - 1)
    na, nb = C.c_int32(), C.c_int32()

    def call(npr, plist, o, o2="same"):
        torch.cuda.synchronize()
        o2 = o if o2 == "same" else o2
        if who == "hxv_lanczos_tridiag_probes":
            return L.hxv_lanczos_tridiag_probes(h, v.data_ptr(), npr, plist, NL, _p(arr[0]), _p(arr[1]), o and _p(out[0]), 1e-12, C.byref(na))
        if who == "hxv_lanczos_tridiag_pair_probes":
            return L.hxv_lanczos_tridiag_pair_probes(h, v.data_ptr(), w.data_ptr(), npr, plist, NL, _p(arr[0]), _p(arr[1]), o and _p(out[0]), _p(arr[2]),
                                                     _p(arr[3]), o2 and _p(out[1]), 1e-12, C.byref(na), C.byref(nb))
        f = L.hxv_chebyshev_moments if who == "hxv_chebyshev_moments" else L.hxv_chebyshev_moments_real
        return f(h, v.data_ptr(), npr, plist, NL, A, B, o and _p(out[0]), _p(smom))

    def good():
        for x in arr + out + [smom]:
            x[:] = FILL
        assert call(2, _plist(p), True) == 0, L.hxv_last_error()
        return b"".join(x.tobytes() for x in arr + out + [smom]) + bytes([na.value, nb.value])

    return call, good


@pytest.mark.parametrize("who,needs", [
    ("hxv_lanczos_tridiag_probes", "nprobes > 0 needs the probe list and the overlaps array"),
    ("hxv_lanczos_tridiag_pair_probes", "nprobes > 0 needs the probe list and both overlaps arrays"),
    ("hxv_chebyshev_moments", "nprobes > 0 needs the probe list and the moments array"),
    ("hxv_chebyshev_moments_real", "nprobes > 0 needs the probe list and the moments array")])
def test_probe_list_refusals_word_for_word(chain400, who, needs):
    c = chain400
    L, p = c["L"], c["p"]
    call, good = _probe_entry_calls(c, who)
    before = good()
    one = _plist(p[:1])
    nine = (C.c_void_p * 9)(*([p[0].data_ptr()] * 9))
    hole = (C.c_void_p * 2)(p[0].data_ptr(), None)
    cases = [((-1, one, True), who + ": nprobes must be 0 .. HXV_MAX_PROBES (8)"),
             ((9, nine, True), who + ": nprobes must be 0 .. HXV_MAX_PROBES (8)"),
             ((1, None, True), who + ": " + needs),
             ((2, hole, True), who + ": NULL entry in the probe list"),
             ((1, one, None), who + ": " + needs)]
    if who == "hxv_lanczos_tridiag_pair_probes":
        cases.append(((1, one, True, None), who + ": " + needs))          # (the second overlaps array alone)
    for args, text in cases:
        _refused(L, call(*args), text)
        assert good() == before, text
    if "lanczos" in who:
        assert before[-2] == NL                                             # (the good call made its NL steps)


@pytest.mark.parametrize("who", ["hxv_chebyshev_moments", "hxv_chebyshev_moments_real", "hxv_chebyshev_apply", "hxv_chebyshev_apply_real"])
def test_chebyshev_window_coefficient_and_output_refusals_word_for_word(chain400, who):
    import torch

    c = chain400
    sec, L, v, p = c["sec"], c["L"], c["v"], c["p"]
    real = who.endswith("_real")
    if "moments" in who:
        _, good = _probe_entry_calls(c, who)
        f = L.hxv_chebyshev_moments_real if real else L.hxv_chebyshev_moments
        mom, smom = np.zeros(2 * NL * 2), np.zeros(2 * NL - 1)
        before = good()
        for a in (0.0, -1.0, float("nan"), float("inf")):
            torch.cuda.synchronize()
            _refused(L, f(sec._h, v.data_ptr(), 2, _plist(p), NL, a, B, _p(mom), _p(smom)), who + ": the window needs a > 0 and finite a, b")
            assert good() == before, a
        return
    f = L.hxv_chebyshev_apply_real if real else L.hxv_chebyshev_apply
    ncoef = 5
    coef = np.linspace(1.0, 0.2, ncoef if real else 2 * ncoef)
    out = torch.zeros_like(v)
    n2 = C.c_double()

    def call(cf=coef, a=A, dst=out):
        torch.cuda.synchronize()
        return f(sec._h, v.data_ptr(), ncoef, _p(cf), a, B, dst.data_ptr(), C.byref(n2))

    def good():
        out.zero_()
        assert call() == 0, L.hxv_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes() + np.float64(n2.value).tobytes()

    before = good()
    assert n2.value > 0.0
    bad = coef.copy()
    bad[-1] = np.inf
    nan = coef.copy()
    nan[0] = np.nan
    for kw, text in ((dict(a=0.0), ": the window needs a > 0 and finite a, b"), (dict(cf=bad), ": a coefficient is not finite"),
                     (dict(cf=nan), ": a coefficient is not finite"), (dict(dst=v), ": d_out must not be d_vin")):
        _refused(L, call(**kw), who + text)
        assert good() == before, text
