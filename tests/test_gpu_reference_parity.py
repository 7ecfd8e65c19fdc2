"""The HIP paths against Hv AS THE REFERENCE'S OWN LOOP NESTS PRODUCED IT (tests/golden/reference_hxv.npz, written by
scripts/make_golden_reference.py from oracle/ref_pin.f90: the reference's ED_HAMILTONIAN/direct fragments executed; the product of its
sparse fragments' element streams where the direct ones may not run or drop bath terms -- DESIGN.md section 1).  Reads ONLY the fixture:
neither the binary, nor the reference tree, nor the C oracle.  Tolerance 1e-13 relative to max|ref| (the project's H x V tolerance), on
models.deterministic_vector(Dim) as the generator used it: both kernels, host arrays, real vectors where H is real, pass A as jobs where
the plan allows it, 2 and 3 thread ranks over the three exchanges, the device row order forced on; and the ground-state energy of every
stored model (numpy.linalg.eigvalsh of the reference streams' dense matrix) against eigh_lowest at 1e-10."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-13
GOLD = np.load(Path(__file__).resolve().parent / "golden" / "reference_hxv.npz")
IDS = [str(s) for s in GOLD["ids"]]
_CASES = {}
_JOB_BITS = (None, 6, 5, 4, 3)      # up block bits tried, in this order, until pass A runs as jobs (None: the plan's own)


def _case(cid):
    """(model, nup, ndw, v, reference Hv), rebuilt from the stored settings"""
    if cid not in _CASES:
        from hxv import models

        k = IDS.index(cid)
        L, O, S, B, hf, nup, ndw = (int(x) for x in GOLD["ints"][k])
        r = GOLD["reals"][k]
        m = models.Model(L, O, S, B, GOLD[f"imphloc_{k}"], GOLD[f"hbath_{k}"], GOLD[f"vbath_{k}"], Uloc=r[:5].copy(), Ust=float(r[5]), Jh=float(r[6]),
                         Jx=float(r[7]), Jp=float(r[8]), xmu=float(r[9]), hfmode=bool(hf), name=cid)
        ref = GOLD[f"hv_{k}"]
        _CASES[cid] = (m, nup, ndw, models.deterministic_vector(ref.size), ref)
    return _CASES[cid]


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_fixture_is_what_the_generator_promises():
    assert len(IDS) >= 10 and set(np.unique(GOLD["source"]).tolist()) == {0, 1}
    assert (Path(__file__).resolve().parent / "golden" / "reference_hxv.npz").stat().st_size < 256 * 1024
    for cid in IDS:
        m, nup, ndw, v, ref = _case(cid)
        assert ref.dtype == np.complex128 and 9 <= ref.size <= 4900 and np.isfinite(ref.view(np.float64)).all()


@pytest.mark.parametrize("cid", IDS)
def test_products_match_the_reference(built, cid):
    import torch
    import hxv

    m, nup, ndw, v, ref = _case(cid)
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    assert sec.Dim == ref.size
    dv = sec.pad(torch.from_numpy(v).cuda())
    for kern in (1, 0):
        sec.set_option("kernel", kern)
        hv = sec.unpad(sec.apply_device(dv))
        torch.cuda.synchronize()
        assert _rel(hv.cpu().numpy(), ref) <= TOL, (cid, "kernel", kern)
    sec.set_option("kernel", 1)
    assert _rel(sec.apply_host(v), ref) <= TOL, (cid, "host")
    if sec.real_vectors_available:            # H real: H Re(v) = Re(H v), H Im(v) = Im(H v)
        scale = np.abs(ref).max()
        for part, want in ((v.real, ref.real), (v.imag, ref.imag)):
            hr = sec.unpad_real(sec.apply_device_real(sec.pad_real(torch.from_numpy(np.ascontiguousarray(part)).cuda())))
            torch.cuda.synchronize()
            assert np.abs(hr.cpu().numpy() - want).max() <= TOL * scale, (cid, "real vectors")
    sec.close()
    # pass A as jobs, at the first block size at which the plan takes them
    for bits in _JOB_BITS:
        if bits is not None and bits >= m.Ns:
            continue
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        if bits is not None:
            sec.set_option("tile_bits_up", bits)
        sec.set_option("job_up", 1)
        active = sec.get_option("job_up_active") == 1
        if active:
            for cols in (1, 2):
                sec.set_option("job_cols", cols)
                hv = sec.unpad(sec.apply_device(sec.pad(torch.from_numpy(v).cuda())))
                torch.cuda.synchronize()
                assert _rel(hv.cpu().numpy(), ref) <= TOL, (cid, "jobs", bits, cols)
        sec.close()
        if active:
            break


@pytest.mark.parametrize("exchange", ["allgather", "halo", "alltoall"])
@pytest.mark.parametrize("cid", IDS)
def test_split_sectors_match_the_reference(built, cid, exchange):
    import torch
    import hxv

    m, nup, ndw, v, ref = _case(cid)
    scale = np.abs(ref).max()
    hxv.set_exchange_default(exchange)
    try:
        for nranks in (2, 3):
            def rank(r, group):
                sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
                group.join(sec)
                lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
                got_host = sec.apply_host(v[lo:hi])
                dv = sec.pad(torch.from_numpy(v[lo:hi].copy()).cuda(), sec.mpiQdw)
                got_dev = sec.unpad(sec.apply_device_slab(dv)).cpu().numpy()
                sec.close()
                return lo, hi, got_host, got_dev

            res = hxv.run_ranks(nranks, rank)
            assert sorted(lo for lo, *_ in res)[0] == 0 and sum(hi - lo for lo, hi, *_ in res) == ref.size
            for lo, hi, gh, gd in res:
                assert np.abs(gh - ref[lo:hi]).max() <= TOL * scale, (cid, exchange, nranks, "host")
                assert np.abs(gd - ref[lo:hi]).max() <= TOL * scale, (cid, exchange, nranks, "device")
    finally:
        hxv.set_exchange_default("allgather")


@pytest.mark.parametrize("cid", IDS)
def test_forced_device_row_order_matches_the_reference(built, monkeypatch, cid):
    import torch
    import hxv

    m, nup, ndw, v, ref = _case(cid)
    bits = max(2, m.Ns - 3)
    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(bits))
    hxv.sector_cache_clear()
    try:
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        sec.set_option("tile_bits_up", bits)
        dv = sec.pad(torch.from_numpy(v).cuda())
        for kern in (1, 0):
            sec.set_option("kernel", kern)
            hv = sec.unpad(sec.apply_device(dv))
            torch.cuda.synchronize()
            assert _rel(hv.cpu().numpy(), ref) <= TOL, (cid, "row order", kern)
        assert _rel(sec.apply_host(v), ref) <= TOL, (cid, "row order, host")
        sec.close()
    finally:
        hxv.sector_cache_clear()


@pytest.mark.parametrize("cid", [c for c, e in zip(IDS, GOLD["e0"]) if not np.isnan(e)])
def test_ground_state_energy_matches_the_reference_matrix(built, cid):
    import hxv

    m, nup, ndw, _, _ = _case(cid)
    want = float(GOLD["e0"][IDS.index(cid)])
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    ev, _, nconv, _ = sec.eigh_lowest(1, min(20, sec.Dim - 1), want_vectors=False)
    sec.close()
    assert nconv == 1 and abs(ev[0] - want) <= 1e-10, (cid, ev[0], want)


def test_every_conditional_path_is_reached_by_some_stored_case(built, monkeypatch):
    """The paths the tests above take only where a handle offers them are offered by at least one stored case each: real vectors, pass A as
    jobs, the two-transposes exchange, a non-identity device row order.  (Asked of the handles again, so that the test stands alone.)"""
    import hxv

    seen = {"real": 0, "jobs": 0, "alltoall": 0, "row_order": 0}
    for cid in IDS:
        m, nup, ndw, _, _ = _case(cid)
        sec = hxv.HxvSector.from_model(m, nup, ndw)
        seen["real"] += bool(sec.real_vectors_available)
        sec.close()
        for bits in _JOB_BITS:
            if bits is not None and bits >= m.Ns:
                continue
            sec = hxv.HxvSector.from_model(m, nup, ndw)
            if bits is not None:
                sec.set_option("tile_bits_up", bits)
            sec.set_option("job_up", 1)
            active = sec.get_option("job_up_active") == 1
            sec.close()
            if active:
                seen["jobs"] += 1
                break
        hxv.set_exchange_default("alltoall")
        try:
            sec = hxv.HxvSector.from_model(m, nup, ndw, rank=1, nranks=3)
            seen["alltoall"] += sec.exchange_mode == "alltoall"
            sec.close()
        finally:
            hxv.set_exchange_default("allgather")
    monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
    hxv.sector_cache_clear()
    try:
        for cid in IDS:
            m, nup, ndw, _, _ = _case(cid)
            monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(max(2, m.Ns - 3)))
            sec = hxv.HxvSector.from_model(m, nup, ndw)
            seen["row_order"] += sec.row_perm is not None and not np.array_equal(sec.row_perm, np.arange(sec.DimUp))
            sec.close()
    finally:
        hxv.sector_cache_clear()
    print(seen)
    assert all(seen.values()), seen
