"""Sectors with a one-spin dimension above 65535 against the oracle (tests/wide_sectors.py names them and caches the oracle's answers).

The engine accepts Ns <= 24 and one-spin dimensions up to 2^20; the rest of the suite stops at 48 620.  A solve does not: it walks every
sector, the skinny ones of Ns = 20 to 24 included (184 756 x 1 ... 20).  Above 65535 the job kernel of pass A is gated off, grids with a y
extent need a loop, and every kernel that gives a column a workgroup of its own sees more columns than ever before.  Here: the product on
every such sector (both kernels, host arrays, real vectors, plan options, 15 444 blocks), split over thread ranks with each exchange, the
kernels that move vectors (row order, twin map, ladder, random state), the Lanczos drivers and the observables.

Tolerances are the project's own: 1e-13 * max|ref| for a product (tests/test_gpu_parity.py), 1e-11 for tridiagonal coefficients, 1e-9 and
1e-7 for an eigenpair (tests/test_gpu_fuzz.py), 1e-13 for an observables record (tests/test_gpu_observables.py); data movement is exact.
Every test prints the error it found (pytest -s)."""
import numpy as np
import pytest

import chebyshev_real_ref as CR
import wide_sectors as WS

pytestmark = pytest.mark.gpu

TOL = 1e-13
DOCUMENTED = ("block larger", "does not fit", "must be")


def _open(name, **kw):
    import hxv

    m, nup, ndw = WS.sector(name)
    return hxv.HxvSector.from_model(m, nup, ndw, **kw)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the cached vectors are read-only)


def _bits(t):
    import torch

    return torch.view_as_real(t).contiguous().view(torch.int64).cpu()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _preconditions(sec, name):
    """what makes these sectors the far side of the suite: asserted, so that a later change of defaults cannot empty the tests"""
    if name != "ns22_2_1":
        assert max(sec.DimUp, sec.DimDw) > 65535, name
        assert sec.get_option("nblocks_up") >= 256 or sec.get_option("nblocks_dw") >= 512, (name, sec.get_option("nblocks_up"), sec.get_option("nblocks_dw"))
    if name in ("ns20_10_1", "ns20_10_0"):
        assert sec.row_perm is not None and not np.array_equal(sec.row_perm, np.arange(sec.DimUp)), name


def _product(sec, dv, ref, what):
    import torch

    hv = sec.unpad(sec.apply_device(dv))
    torch.cuda.synchronize()
    err = WS.rel(hv.cpu().numpy(), ref)
    print(f"{what}: max|got - ref| / max|ref| = {err:.2e}")
    assert err <= TOL, (what, err)


# ---- a. the product ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WS.S_SECTORS + WS.P_SECTORS)
def test_product_matches_the_oracle(built, name):
    """both kernels, host arrays, and on the real-H sectors the real-vector product of Re v and Im v"""
    import torch

    orc, v, ref = WS.oracle(name)
    sec = _open(name)
    try:
        assert (sec.DimUp, sec.DimDw, sec.Dim) == (orc.DimUp, orc.DimDw, orc.Dim)
        _preconditions(sec, name)
        if name in ("ns24_6_1", "ns24_1_6"):      # Jx, Jp with particles of both spins: the spH0nd block is live
            assert orc.csr("nd")[0][-1] > 0, name
        dv = sec.pad(_dev(v))
        for kern in (1, 0):
            sec.set_option("kernel", kern)
            _product(sec, dv, ref, f"{name} kernel {kern}")
        sec.set_option("kernel", 1)
        err = WS.rel(sec.apply_host(v), ref)
        print(f"{name} host arrays: {err:.2e}")
        assert err <= TOL, (name, "host", err)
        if name.startswith("ns20"):
            assert sec.real_vectors_available, name
        if sec.real_vectors_available:            # H real: H Re(v) = Re(H v), H Im(v) = Im(H v)
            scale = np.abs(ref).max()
            for part, want in ((v.real, ref.real), (v.imag, ref.imag)):
                hr = sec.unpad_real(sec.apply_device_real(sec.pad_real(_dev(np.ascontiguousarray(part)))))
                torch.cuda.synchronize()
                err = np.abs(hr.cpu().numpy() - want).max() / scale
                print(f"{name} real vectors: {err:.2e}")
                assert err <= TOL, (name, "real vectors", err)
    finally:
        sec.close()


PLAN_CASES = [(n, o, val) for n in WS.P_SECTORS
              for o, vals in (("cols_per_tile", (2, 8)), ("rows_per_tile", (2, 8)), ("block_order", (0, 1, 2)), ("job_up", (1,))) for val in vals]
PLAN_CASES += [(n, "fold_nd", val) for n in ("ns24_6_1", "ns24_1_6") for val in (0, 1)]
PLAN_CASES += [(n, "tile_bits", 6) for n in ("ns20_10_1", "ns20_1_10")]
EXPECTED_REFUSALS = ()


@pytest.mark.parametrize("name,option,value", PLAN_CASES, ids=[f"{n}-{o}{v}" for n, o, v in PLAN_CASES])
def test_product_with_a_plan_option_matches_the_oracle(built, name, option, value):
    """one option at a time on a fresh handle.  A set the plan builder refuses must be refused with a documented message, and must be one
    of EXPECTED_REFUSALS: the host plan checker accepts every set of this list on the CPU (tests/test_host_plan_check.py runs them), so the
    list is empty and no case ends at the refusal."""
    import hxv

    orc, v, ref = WS.oracle(name)
    sec = _open(name)
    try:
        _preconditions(sec, name)
        try:
            for o in (("tile_bits_up", "tile_bits_dw") if option == "tile_bits" else (option,)):
                sec.set_option(o, value)
        except hxv.HxvError as e:
            assert any(d in str(e) for d in DOCUMENTED), str(e)
            assert (name, option, value) in EXPECTED_REFUSALS, str(e)
            return
        if option == "job_up":          # more than 65535 up rows: pass A must not run as jobs, the product falls back to hxv_pass_up
            assert sec.get_option("job_up") == 1
            if sec.DimUp > 65535:
                assert sec.get_option("job_up_active") == 0
            else:                       # (20 or 24 up rows in one block: the job kernel is allowed, and is what runs)
                assert sec.get_option("job_up_active") == 1
        if option == "fold_nd":
            assert sec.get_option("fold_nd") == value
        if option == "tile_bits":       # 64-row prefix blocks: 15 444 of them on the wide spin, 25 to 27 out-of-block partners each
            nb = max(sec.get_option("nblocks_up"), sec.get_option("nblocks_dw"))
            ko = max(sec.get_option("max_outer_up"), sec.get_option("max_outer_dw"))
            print(f"{name}: {sec.get_option('nblocks_up')} x {sec.get_option('nblocks_dw')} blocks, at most {ko} out-of-block partners")
            assert nb >= 15000 and ko >= 25, (nb, ko)
        _product(sec, sec.pad(_dev(v)), ref, f"{name} {option} = {value}")
    finally:
        sec.close()


def test_a_tile_that_does_not_fit_the_lds_is_refused(built):
    """14 block bits on the 184 756-row spin: C(14,7) rows of 16 bytes are more than the 160 KB of LDS; the handle keeps its plan"""
    import hxv

    orc, v, ref = WS.oracle("ns20_10_1")
    sec = _open("ns20_10_1")
    try:
        before = {n: sec.get_option(n) for n in ("tile_bits_up", "nblocks_up", "max_block_up")}
        with pytest.raises(hxv.HxvError, match="does not fit"):
            sec.set_option("tile_bits_up", 14)
        assert {n: sec.get_option(n) for n in before} == before
        _product(sec, sec.pad(_dev(v)), ref, "ns20_10_1 after the refusal")
    finally:
        sec.close()


def test_the_job_kernel_stays_off_above_65535_rows_when_every_other_gate_is_open(built):
    """The star (one site, 19 bath orbitals) with 12 block bits is the one plan on which ONLY the DimUp < 65536 gate of job_up_usable says no
    (tests/wide_sectors.py, GATE): 256 blocks of at most 924 rows, 8 out-of-block partners, at most 24 in-block hops, "job_max_blocks"
    raised to 256.  The control: sector (6,1) of the same model with the same options, 38 760 rows, does plan pass A as jobs (read back
    only: nothing is launched there).  On (10,1) the plain and the fused product must fall back to the one-tile-per-workgroup kernel and
    match the oracle; with the gate taken out the job kernel's 16-bit-scaled row fields overflow."""
    import hxv
    import torch

    name = WS.GATE_SECTOR
    orc, v, ref = WS.oracle(name)
    m, nup, ndw = WS.sector(name)
    ctl = hxv.HxvSector.from_model(m, 6, 1)
    sec = _open(name)
    try:
        for s in (ctl, sec):
            for o, val in WS.GATE_OPTIONS:
                s.set_option(o, val)
            got = {n: s.get_option(n) for n in ("nblocks_up", "max_block_up", "max_outer_up", "k_in_up", "job_max_blocks", "job_cols", "sort_mode")}
            assert got["nblocks_up"] <= got["job_max_blocks"] == 256 and got["max_block_up"] <= 960 and got["max_outer_up"] <= 8 and got["k_in_up"] <= 24, got
            assert got["job_cols"] == 1 and got["sort_mode"] == 0, got
        assert ctl.DimUp < 65536 and ctl.get_option("job_up_active") == 1
        assert sec.DimUp == 184756 and sec.get_option("job_up_active") == 0
        _product(sec, sec.pad(_dev(v)), ref, f"{name}, job_up = 1 past every other gate")
        vn = v / np.linalg.norm(v)
        a, b, n = sec.lanczos_tridiag(sec.pad(_dev(vn)), 12)
        a0, b0 = orc.lanc_tridiag(vn, 12)
        assert n == len(a0) == 12
        ea, eb = np.abs(a - a0).max() / np.abs(a0).max(), np.abs(b[1:] - b0[1:]).max() / np.abs(b0).max()
        print(f"{name} fused Lanczos product, 12 steps: alpha {ea:.2e}, beta {eb:.2e}")
        assert ea <= 1e-11 and eb <= 1e-11
        torch.cuda.synchronize()
    finally:
        ctl.close()
        sec.close()


# ---- b. split sectors on thread ranks -----------------------------------------------------------------------------------------------------------
SPLITS = [("ns20_1_10", 2), ("ns20_1_10", 3), ("ns24_1_6", 2)]
EXCHANGES = [("allgather", 0), ("halo", 0), ("alltoall", 0), ("alltoall", 1)]


@pytest.mark.parametrize("exchange,overlap", EXCHANGES, ids=[e + ("-overlap" if o else "") for e, o in EXCHANGES])
@pytest.mark.parametrize("name,nranks", SPLITS, ids=[f"{n}-P{p}" for n, p in SPLITS])
def test_split_sectors_match_the_oracle(built, monkeypatch, name, nranks, exchange, overlap):
    """every rank's slab of the product through host arrays and through apply_device_slab.  (1,10) on 2 ranks keeps 92 378 columns per
    rank: with the all-to-all exchange and "exchange_overlap" the dw part is added by add_pieces_kernel, whose grid would need that many
    blocks along y -- it loops over the columns instead.  The BHZ sector carries spH0nd, which keeps the all-gather layout whatever is asked."""
    import hxv

    monkeypatch.setenv("HXV_LOCAL_TIMEOUT_S", "120")     # (a rank that fails must end the test, not leave its peers waiting)
    orc, v, ref = WS.oracle(name)
    m, nup, ndw = WS.sector(name)
    scale = np.abs(ref).max()
    hxv.set_exchange_default(exchange)
    try:
        def rank(r, group):
            sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
            try:
                sec.set_option("exchange_overlap", overlap)
                group.join(sec)
                lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
                got_host = sec.apply_host(v[lo:hi])
                dv = sec.pad(_dev(v[lo:hi]), sec.mpiQdw)
                got_dev = sec.unpad(sec.apply_device_slab(dv)).cpu().numpy()
                return lo, hi, got_host, got_dev, sec.exchange_mode, sec.mpiQdw, sec.get_option("exchange_overlap")
            finally:
                sec.close()

        res = hxv.run_ranks(nranks, rank)
    finally:
        hxv.set_exchange_default("allgather")
    assert sorted(lo for lo, *_ in res)[0] == 0 and sum(hi - lo for lo, hi, *_ in res) == ref.size
    for lo, hi, gh, gd, mode, q, ov in res:
        assert mode == (exchange if name.startswith("ns20") else {"alltoall": "allgather"}.get(exchange, exchange)), (name, mode)
        assert ov == overlap
        if nranks == 2:
            assert q > 65535, q
        eh, ed = np.abs(gh - ref[lo:hi]).max() / scale, np.abs(gd - ref[lo:hi]).max() / scale
        print(f"{name} P{nranks} {exchange} overlap {overlap}: {q} columns, host {eh:.2e}, device {ed:.2e}")
        assert eh <= TOL, (name, nranks, exchange, overlap, "host", eh)
        assert ed <= TOL, (name, nranks, exchange, overlap, "device", ed)


# ---- c. vectors moved at these sizes ---------------------------------------------------------------------------------------------------------------
def test_host_vectors_round_trip_through_the_device_row_order(built):
    """vector_from_host / vector_to_host on 184 756 rows in the device row order (rows_ref_to_dev, rows_dev_to_ref): the device vector is
    the torch restatement's bit for bit, pad rows +0.0, and the way back returns the input's bits"""
    orc, v, _ = WS.oracle("ns20_10_1")
    sec = _open("ns20_10_1")
    try:
        _preconditions(sec, "ns20_10_1")
        d = sec.vector_from_host(v)
        assert bool((_bits(d) == _bits(sec.pad(_dev(v)))).all())
        assert _same_bits(sec.vector_to_host(d), v)
    finally:
        sec.close()


def test_twin_vector_is_the_transpose_unsplit_and_on_two_ranks(built, monkeypatch):
    """(10,1) -> (1,10) and back.  Unsplit: the numpy transpose, bit for bit.  On 2 ranks the target rank keeps 92 378 columns, more than
    the 65535 blocks twin_unpack_kernel's grid has along y: its loop takes a second trip.  The split result carries the unsplit call's bits."""
    import hxv

    monkeypatch.setenv("HXV_LOCAL_TIMEOUT_S", "120")
    _, v, _ = WS.oracle("ns20_10_1")
    a, b = _open("ns20_10_1"), _open("ns20_1_10")
    try:
        assert (b.DimUp, b.DimDw) == (a.DimDw, a.DimUp) and a.row_perm is not None
        want = v.reshape(a.DimDw, a.DimUp).T.ravel()                               # B's host vector
        full = a.twin_vector(b, a.vector_from_host(v))
        assert _same_bits(b.vector_to_host(full), want)
        back = b.twin_vector(a, full)
        assert _same_bits(a.vector_to_host(back), v)
        bits_b = _bits(full).view(b.DimDw, b.pitch, 2)
        bits_a = _bits(back).view(a.DimDw, a.pitch, 2)
    finally:
        a.close()
        b.close()

    for frm, to, src, ref_bits in (("ns20_10_1", "ns20_1_10", v, bits_b), ("ns20_1_10", "ns20_10_1", want, bits_a)):
        def rank(r, group):
            fa, fb = _open(frm, rank=r, nranks=2), _open(to, rank=r, nranks=2)
            try:
                group.join(fb)
                slab = fa.vector_from_host(src[fa.mpiIshift: fa.mpiIshift + fa.vecDim])
                out = fa.twin_vector(fb, slab)
                return fb.mpiIshift // fb.DimUp, fb.mpiQdw, _bits(out).view(fb.mpiQdw, fb.pitch, 2)
            finally:
                fa.close()
                fb.close()

        res = hxv.run_ranks(2, rank)
        assert sum(q for _, q, _ in res) == ref_bits.shape[0]
        for c0, q, out_bits in res:
            if to == "ns20_1_10":
                assert q == 92378
            assert bool((out_bits == ref_bits[c0: c0 + q]).all()), (frm, to, c0)


def test_dw_ladder_unsplit_and_on_two_ranks(built, monkeypatch):
    """c^dagger on a dw orbital.  (10,0) -> (10,1), unsplit, 184 756 rows in the device row order.  A sector with one dw state cannot be split
    (refused, asserted), so the split form -- one column exchange, then ladder_cols_kernel with one workgroup per target column -- runs
    (1,9) -> (1,10) on 2 ranks, 92 378 target columns each, after the unsplit call on the same pair.  Every target element is +- one source
    element or zero: equal to the numpy restatement, norms to rounding."""
    import hxv

    monkeypatch.setenv("HXV_LOCAL_TIMEOUT_S", "120")
    m, _, _ = WS.sector("ns20_10_0")
    with pytest.raises(hxv.HxvError, match="nranks > DimDw"):
        hxv.HxvSector.from_model(m, 10, 0, rank=0, nranks=2)
    rng = np.random.default_rng(31)
    for frm, to, orbitals in (("ns20_10_0", "ns20_10_1", (0, 7, 19)), ("ns20_1_9", "ns20_1_10", (3, 12))):
        s0, s1 = _open(frm), _open(to)
        try:
            psi = rng.standard_normal(s0.Dim) + 1j * rng.standard_normal(s0.Dim)
            dpsi = s0.vector_from_host(psi)
            maps = (s0.maps(), s1.maps())
            wants = {}
            for orb in orbitals:
                out, n2 = s0.apply_ladder(s1, orb, 1, True, dpsi)
                want = WS.ladder_numpy(psi, maps[0], maps[1], orb, 1, True)
                assert np.array_equal(s1.vector_to_host(out), want), (frm, orb)
                ref2 = float(np.sum(np.abs(want) ** 2))
                assert ref2 > 0 and abs(n2 - ref2) <= 1e-12 * ref2, (frm, orb, n2, ref2)
                wants[orb] = (want, ref2)
        finally:
            s0.close()
            s1.close()
        if frm == "ns20_10_0":
            continue

        def rank(r, group):
            fa, fb = _open(frm, rank=r, nranks=2), _open(to, rank=r, nranks=2)
            try:
                group.join(fb)
                slab = fa.vector_from_host(psi[fa.mpiIshift: fa.mpiIshift + fa.vecDim])
                out = []
                for orb in orbitals:
                    o, n2 = fa.apply_ladder(fb, orb, 1, True, slab)
                    out.append((fb.vector_to_host(o), n2))
                return fb.mpiIshift, fb.vecDim, fb.mpiQdw, out
            finally:
                fa.close()
                fb.close()

        for lo, n, q, out in hxv.run_ranks(2, rank):
            assert q == 92378
            for orb, (got, n2) in zip(orbitals, out):
                want, ref2 = wants[orb]
                assert np.array_equal(got, want[lo: lo + n]), (orb, lo)
                assert abs(n2 - ref2) <= 1e-12 * ref2          # the GLOBAL norm, on every rank


@pytest.mark.parametrize("name", ["ns20_10_1", "ns20_1_10"])
def test_seeded_random_state_does_not_depend_on_the_row_order(built, name):
    """hxv_vector_random against the formula of include/hxv.h in numpy uint64 (tests/chebyshev_real_ref.py): the same numbers in the
    reference's layout with the device row order on (10,1) and without one (1,10); exact"""
    sec = _open(name)
    try:
        assert (sec.row_perm is not None) == (name == "ns20_10_1")
        for seed, cplx in ((7, False), (2 ** 40 + 3, True)):
            got = sec.vector_to_host(sec.random_vector(seed, cplx))
            assert np.array_equal(got, CR.random_vector(seed, sec.Dim, cplx)), (name, seed)
    finally:
        sec.close()


# ---- d. the drivers on the S sectors ------------------------------------------------------------------------------------------------------------
def _fused_product_runs_on_pass_up(sec):
    """the drivers' fused product is on by default and asks for the job kernel (job_up = 2); above 65535 up rows the plan cannot give it
    one, so the Lanczos epilogue rides on hxv_pass_up.  ((0,10) has ONE up row: nothing to assert there.)"""
    assert sec.get_option("lanczos_fused") == 1 and sec.get_option("job_up") == 2
    if sec.DimUp > 65535:
        sec.set_option("job_up", 1)
        assert sec.get_option("job_up_active") == 0
        sec.set_option("job_up", 2)


@pytest.mark.parametrize("name", WS.DRIVER_SECTORS)
def test_lanczos_tridiag_matches_the_oracle(built, name):
    orc, v, _ = WS.oracle(name)
    sec = _open(name)
    try:
        _preconditions(sec, name)
        _fused_product_runs_on_pass_up(sec)
        vn = v / np.linalg.norm(v)
        a, b, n = sec.lanczos_tridiag(sec.pad(_dev(vn)), 12)
        a0, b0 = orc.lanc_tridiag(vn, 12)
        assert n == len(a0) == 12
        ea, eb = np.abs(a - a0).max() / np.abs(a0).max(), np.abs(b[1:] - b0[1:]).max() / np.abs(b0).max()
        print(f"{name} 12 Lanczos steps: alpha {ea:.2e}, beta {eb:.2e}")
        assert ea <= 1e-11 and eb <= 1e-11
    finally:
        sec.close()


@pytest.mark.parametrize("name", WS.DRIVER_SECTORS)
def test_lowest_eigenpair_matches_arpack_on_the_oracles_matrix(built, name):
    orc, _, _ = WS.oracle(name)
    e0, wmax = WS.extremal_eigenvalues(name)
    sec = _open(name)
    try:
        _fused_product_runs_on_pass_up(sec)
        ev, X, nconv, nmv = sec.eigh_lowest(1, 16)
        x = X[0].cpu().numpy()
        res = np.linalg.norm(orc.spMatVec_main(x) - ev[0] * x)
        el = sec.lanczos_eigh(600, 1e-13, want_vector=False)[0]
        print(f"{name}: E0 {e0:.12f}, eigh_lowest off by {abs(ev[0] - e0):.2e} after {nmv} products, residual {res:.2e}, lanczos_eigh off by {abs(el - e0):.2e}")
        assert nconv == 1 and abs(ev[0] - e0) <= 1e-9 * max(1.0, abs(e0))
        assert abs(np.linalg.norm(x) - 1.0) <= 1e-12 and res <= 1e-7 * wmax
        assert abs(el - e0) <= 1e-9 * max(1.0, abs(e0))
    finally:
        sec.close()


# ---- e. observables, one workgroup per column ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,state", [("ns20_0_10", "ground"), ("ns20_1_10", "random")])
def test_observables_on_184756_columns(built, name, state):
    """the device record against the numpy record of the same state (read back through vector_to_host) at the 1e-13 of
    tests/test_gpu_observables.py, and observables() = accumulate + derive against derive of the numpy record at that file's 1e-12"""
    import torch
    from hxv import observables

    m, _, _ = WS.sector(name)
    sec = _open(name)
    try:
        _preconditions(sec, name)
        assert sec.mpiQdw == 184756
        if state == "ground":
            ev, vecs, nc, _ = sec.eigh_lowest(1, 16, native=True)
            assert nc == 1
            psi, e = vecs[0].contiguous(), float(ev[0])
        else:
            psi, e = sec.random_vector(11, True), 0.0
            psi /= torch.linalg.norm(psi)
        v = sec.vector_to_host(psi)
        assert abs(np.linalg.norm(v) - 1.0) <= 1e-12
        mu, md = sec.maps()
        got = sec.observables_record(psi, weight=0.7)
        ref = WS.record_numpy_fast(m, mu, md, v, 0.7)
        print(f"{name} {state}: record off by {np.abs(got - ref).max():.2e}")
        assert np.abs(got - ref).max() < 1e-13
        out = observables.observables(m, [(sec, e, psi)])
        want = observables.derive(m, ref / 0.7)
        for k in want:
            assert np.abs(np.asarray(out[k]) - np.asarray(want[k])).max() < 1e-12, k
    finally:
        sec.close()
