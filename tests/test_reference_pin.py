"""The oracle and the engine's host tables against the REFERENCE'S OWN loop nests, executed (oracle/ref_pin.f90: our scope, the
reference's eight include fragments of ED_HAMILTONIAN/sparse and ED_HAMILTONIAN/direct compiled in unmodified).

  streams   every sp_insert_element call of H_local, H_non_local, H_up, H_dw, in call order, stored the way ED_SPARSE_MATRIX.f90:267-273
            stores them (row lists in insertion order, a repeated (i,j) summed where it first stands) == OracleSector.csr / diag():
            rowptr, columns and order identical, values equal to the last bit.  Nothing is excluded.
  direct    Hv of directMatVec_main's body == OracleSector.spMatVec_main on the same vector, 1e-13 relative to max|ref| (the project's
            H x V tolerance).  KNOWN QUIRK of the reference, asserted rather than waved off: direct/HxV_local.f90:83 bounds its ilat bath
            loop by size(bath_diag,3) = Norb where sparse/H_local.f90:85 has size(bath_diag,1) = Nlat.  With Nlat < Norb and a bath it
            indexes past bath_diag: never run (the driver refuses).  With Nlat > Norb it drops the bath energies of the sites ilat > Norb:
            the comparison is made after adding exactly those terms, computed here (reference_cases.dropped_bath_diagonal) -- they are
            identically zero for every named model of the list, non-zero for the dedicated model `chain_eps` (asserted) and for the
            random draws with Nlat > Norb and a bath.
  engine    the host builder's one-spin CSR and diagonal (tests/host/plan_check --dump: what HxvSector.csr / diag() hand back, without a
            device) against the streams: rowptr and columns exactly, values within 2e-13 max|value| (tests/test_host_plan_check.py's
            criterion against the oracle), diagonal within 1e-12 (tests/test_gpu_row_order.py's).

These tests skip only where neither the reference tree nor a built oracle/_ref/ref_pin exists."""
import numpy as np
import pytest

import reference_cases as rc
from oracle import reference_pin as rp

TOL = 1e-13
pytestmark = pytest.mark.skipif(not rp.available(), reason="neither the reference tree nor a built oracle/_ref/ref_pin")

CASES = rc.flat_cases()
_RUNS = {}


def _run(cid):
    """(reference run, oracle sector, vin), computed once per case"""
    if cid not in _RUNS:
        from hxv import models
        from oracle.oracle import OracleSector

        m, nup, ndw = {c[0]: c[1:] for c in CASES}[cid]
        orc = OracleSector(m, nup, ndw)
        v = models.deterministic_vector(orc.Dim)
        _RUNS[cid] = (rp.run(m, nup, ndw, v), orc, v)
    return _RUNS[cid]


def test_case_list_covers_what_it_must():
    shapes, nspins, sectors, direct_excluded, dropped = set(), set(), set(), 0, 0
    rnd = rc.random_cases()
    assert len(rnd) >= 12
    for _, m, secs in rnd:
        shapes.add((m.Nlat, m.Norb))
        nspins.add(m.Nspin)
        for nup, ndw in secs:
            sectors.add("empty" if (nup, ndw) == (0, 0) else "full" if (nup, ndw) == (m.Ns, m.Ns) else "one" if nup + ndw == 1 else "other")
        direct_excluded += not rp.direct_runs(m)
        dropped += m.Nbath > 0 and m.Nlat > m.Norb
    assert rc.SHAPES_WANTED <= shapes and nspins == {1, 2} and {"empty", "full", "one"} <= sectors
    print(f"{len(CASES)} cases; random draws: {len(rnd)}, direct excluded on {direct_excluded}, dropped bath terms on {dropped}")


def test_stream_storage_rule():
    """row lists in insertion order; a repeated (i,j) summed where it FIRST stands, in call order"""
    i = [2, 1, 2, 2, 1, 2]
    j = [3, 1, 1, 3, 2, 3]
    v = [1e16, 5.0, 7.0, 1.0, 9.0, -1e16]
    rp_, cols, vals = rp.stream_to_csr(i, j, v, 3)
    assert rp_.tolist() == [0, 2, 4, 4] and cols.tolist() == [1, 2, 3, 1]
    assert vals.tolist() == [5.0, 9.0, (1e16 + 1.0) - 1e16, 7.0]      # (summed in call order: 0, not 1)


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_streams_equal_the_oracle_bit_for_bit(cid):
    ref, orc, _ = _run(cid)
    assert (ref.DimUp, ref.DimDw) == (orc.DimUp, orc.DimDw)
    assert np.array_equal(ref.map_up, orc.map_up()) and np.array_equal(ref.map_dw, orc.map_dw())
    for which in ("up", "dw", "nd"):
        rp_, cols, vals = ref.csr(which)
        rpo, colso, valso = orc.csr(which)
        assert np.array_equal(rp_, rpo), (cid, which, "row lengths")
        assert np.array_equal(cols, colso), (cid, which, "columns / insertion order")
        bad = np.flatnonzero(vals != valso)
        assert bad.size == 0, (cid, which, "values", bad[:5], vals[bad[:5]], valso[bad[:5]])
    d, do = ref.diag(), orc.diag()
    bad = np.flatnonzero(d != do)
    assert bad.size == 0, (cid, "spH0d", bad[:5], d[bad[:5]], do[bad[:5]])
    m = ref.model
    if m.Norb > 1 and (m.Jx != 0 or m.Jp != 0) and min(ref.nup, ref.ndw) > 0 and max(ref.nup, ref.ndw) < m.Ns:
        assert ref.csr("nd")[1].size > 0, (cid, "H_non_local never inserted an element")


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_direct_product_equals_the_oracle(cid):
    ref, orc, v = _run(cid)
    m = ref.model
    if not rp.direct_runs(m):
        assert ref.hv is None
        with pytest.raises(ValueError, match="past bath_diag"):
            rp.run(m, ref.nup, ref.ndw, v, direct=True)
        # the stream product stands in for it in the recorded results: it must be the oracle's product too
        want = orc.spMatVec_main(v)
        assert np.abs(ref.stream_product(v) - want).max() <= TOL * max(np.abs(want).max(), 1e-300)
        return
    want = orc.spMatVec_main(v)
    scale = max(np.abs(want).max(), 1e-300)
    dropped = rc.dropped_bath_diagonal(m, ref.map_up, ref.map_dw) * v
    err = np.abs(ref.hv + dropped - want).max() / scale
    print(f"{cid}: Dim {ref.Dim}, direct vs oracle {err:.2e}, dropped bath terms {np.abs(dropped).max() / scale:.2e} of max|ref|")
    assert err <= TOL, cid
    if cid.startswith(rc.quirk_case()[0]):
        # the quirk is real: without the dropped terms the two differ, by exactly those terms
        assert np.abs(dropped).max() > 1e-3 * scale
        assert np.abs(ref.hv - want).max() > 1e-3 * scale
        assert np.abs((want - ref.hv) - dropped).max() <= TOL * scale
    elif not (m.Nbath > 0 and m.Nlat > m.Norb):
        assert not dropped.any()
    if cid.split("-")[0] in [c[0] for c in rc.named_cases()]:
        assert not dropped.any(), "a named model of the list must run the plain direct check"


@pytest.fixture(scope="module")
def checker(built):
    return built.build_plan_check()


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_engine_host_tables_equal_the_streams(checker, tmp_path, cid):
    import subprocess

    from test_host_plan_check import write_model

    ref, _, _ = _run(cid)
    path = write_model(tmp_path / "m.model", ref.model)
    d = tmp_path / "dump"
    d.mkdir()
    # (a plan refused for a tiny sector -- exit status 2 -- is not this test's business: the dump is written before the plans are made)
    p = subprocess.run([str(checker), str(path), str(ref.nup), str(ref.ndw), "0", "1", "0", "--dump", str(d), "--dump-diag"], capture_output=True, text=True)
    assert p.returncode in (0, 2), (cid, p.returncode, p.stderr[-2000:])
    assert "FAIL" not in p.stderr and "OUT OF RANGE" not in p.stderr, (cid, p.stderr[-2000:])
    for which in ("up", "dw"):
        rp_, cols, vals = ref.csr(which)
        assert np.array_equal(np.fromfile(d / f"{which}_rowptr.i64", dtype=np.int64), rp_), (cid, which)
        assert np.array_equal(np.fromfile(d / f"{which}_cols.i32", dtype=np.int32) + 1, cols), (cid, which)
        got = np.fromfile(d / f"{which}_vals.c128", dtype=np.complex128)
        assert got.shape == vals.shape
        if vals.size:
            assert np.abs(got - vals).max() <= 2e-13 * np.abs(vals).max(), (cid, which)
    assert np.array_equal(np.fromfile(d / "map_up.u32", dtype=np.uint32).astype(np.int64), ref.map_up.astype(np.int64))
    assert np.array_equal(np.fromfile(d / "map_dw.u32", dtype=np.uint32).astype(np.int64), ref.map_dw.astype(np.int64))
    diag = ref.diag()
    assert np.abs(diag.imag).max(initial=0.0) == 0.0
    got = np.fromfile(d / "diag.f64", dtype=np.float64)
    assert got.shape == diag.shape and np.abs(got - diag.real).max(initial=0.0) < 1e-12, cid


# ---- the recorded results (tests/golden/reference_hxv.npz, read by tests/test_gpu_reference_parity.py without the binary) ----------------
def test_golden_fixture_is_what_the_binary_writes_today():
    """scripts/make_golden_reference.py run again: every stored array byte for byte (the settings the reference program read, Hv as it wrote
    it); the energies, which numpy computes from the reference's streams, to 1e-12 and for the sectors up to Dim 1300 only (the two larger
    ones cost LAPACK half a minute).  And every stored Hv is the oracle's product too, at the H x V tolerance."""
    import sys
    from pathlib import Path

    from hxv import models
    from oracle.oracle import OracleSector

    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root / "scripts"))
    import make_golden_reference as gen

    assert gen.OUT.stat().st_size < 256 * 1024
    stored = np.load(gen.OUT)
    fresh = gen.build_arrays(energy_max_dim=1300)
    assert sorted(stored.files) == sorted(fresh)
    for name in stored.files:
        if name == "e0":
            continue
        a, b = stored[name], np.asarray(fresh[name])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    e_old, e_new = stored["e0"], fresh["e0"]
    assert np.isfinite(e_old).sum() >= 9
    both = np.isfinite(e_new)
    assert both.sum() >= 7 and not np.isfinite(e_new[np.isnan(e_old)]).any()
    assert np.abs(e_old[both] - e_new[both]).max() <= 1e-12
    cases = rc.golden_cases()
    assert [c[0] for c in cases] == [str(s) for s in stored["ids"]]
    for k, (cid, m, nup, ndw) in enumerate(cases):
        orc = OracleSector(m, nup, ndw)
        assert orc.Dim <= 4900
        want = orc.spMatVec_main(models.deterministic_vector(orc.Dim))
        assert np.abs(stored[f"hv_{k}"] - want).max() <= TOL * np.abs(want).max(), cid
        orc.close()
