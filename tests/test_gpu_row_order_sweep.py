"""Seeded random sweep with the DEVICE ROW ORDER forced (include/hxv.h; plan_row_order / build_row_order_matrix / finish_row_order in
hxv_sector.cpp): the fuzz's random models (tests/random_models.py) at Ns up to 12, with the test hooks that switch the order on below its size
threshold (HXV_ROW_ORDER_MIN_DIMUP=16, HXV_ROW_ORDER_BITS drawn from [2, Ns-1]) -- so that complex H, the spH0nd block (Jx / Jp: folded
into pass A and as its own pass) and split sectors meet the order, which the hand-picked cases of tests/test_gpu_row_order.py reach only
partly.  Every path against the CPU oracle / the host restatements, in the reference's order: the product (tile options, both kernels,
thread ranks over the three exchanges), host arrays, real vectors, the drivers, the ladder operators and the observables record.  How many
seeds actually took a non-identity order, on complex H / with spH0nd / split, is asserted, not hoped for."""
import numpy as np
import pytest

from ladder_ref import apply_op
from observables_ref import record_numpy
from random_models import random_model

pytestmark = pytest.mark.gpu
NSEEDS = 32
EXCHANGES = ("allgather", "halo", "alltoall")
DIM_MAX = 250_000


def _comb(n, k):
    from math import comb

    return comb(n, k) if 0 <= k <= n else 0


def _draw(seed):
    """Everything a seed decides (host only): model, sector, block bits, the handle's tile bits, ranks, exchange, tile options, ladders."""
    rng = np.random.default_rng(9100 + seed)
    m = random_model(rng, max_ns=12, min_bath=2, p_exchange=0.7)
    while m.Ns < 8:                                     # (below 8 orbitals no spin has the 16 rows the hook asks for at useful fillings)
        m = random_model(rng, max_ns=12, min_bath=2, p_exchange=0.7)
    Ns = m.Ns
    nup = int(np.clip(Ns // 2 + rng.integers(-1, 2), 0, Ns))
    if rng.random() < 0.3:                              # small enough for the dense eigensolver: the drivers
        ndw = max([k for k in range(Ns // 2 + 1) if _comb(Ns, nup) * _comb(Ns, k) <= 3000], default=0)
    else:
        ndw = int(np.clip(Ns // 2 + rng.integers(-2, 3), 0, Ns))
        while _comb(Ns, nup) * _comb(Ns, ndw) > DIM_MAX:
            ndw = min(ndw, Ns - ndw) - 1
    # block bits in [2, Ns-1], mostly above the impurity: a cut inside the impurity orbitals leaves them sorted (no order) more often
    bits = int(rng.integers(max(2, m.Nlat * m.Norb + 1), Ns)) if rng.random() < 0.8 else int(rng.integers(2, Ns))
    tile_bits = bits if rng.random() < 0.75 else int(rng.choice([b for b in range(2, Ns) if b != bits]))
    nranks = int(rng.integers(1, min(3, _comb(Ns, ndw)) + 1))
    exchange = EXCHANGES[int(rng.integers(3))]
    opts = {"lds_budget_kb": int(rng.choice([8, 16, 32])), "cols_per_tile": int(rng.choice([2, 4, 8])), "rows_per_tile": int(rng.choice([2, 4, 8])),
            "threads_up": int(rng.choice([256, 512, 1024])), "threads_dw": int(rng.choice([256, 512, 1024])), "sort_mode": int(rng.integers(3)),
            "wt_cols": int(rng.choice([2, 4, 8, 16])), "job_cols": int(rng.choice([1, 2])), "pair_rows": int(rng.choice([0, 1])),
            "job_groups": int(rng.choice([1, 3, 100])), "job_max_blocks": int(rng.choice([0, 32])), "block_order": int(rng.choice([-1, 0, 1, 2]))}
    ladders = []
    for spin, n in ((0, nup), (1, ndw)):                # one operator per spin into a neighbour sector every rank can hold a column of
        create = bool(rng.integers(2))
        if not (0 <= n + (1 if create else -1) <= Ns) or (spin == 1 and _comb(Ns, n + (1 if create else -1)) < nranks):
            create = not create
        ladders.append((int(rng.integers(Ns)), spin, create))
    return dict(model=m, nup=nup, ndw=ndw, bits=bits, tile_bits=tile_bits, nranks=nranks, exchange=exchange, opts=opts, ladders=ladders,
                vseed=int(rng.integers(1 << 30)))


def _target(c, spin, create):
    d = 1 if create else -1
    return (c["nup"] + d, c["ndw"]) if spin == 0 else (c["nup"], c["ndw"] + d)


@pytest.fixture
def forced(monkeypatch):
    """returns a function that forces the row order for a seed's block bits (the same hooks as tests/test_gpu_row_order.py)"""
    import hxv

    def force(bits):
        monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", "16")
        monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(bits))
        hxv.sector_cache_clear()

    yield force
    hxv.sector_cache_clear()


def _set(sec, opts):
    """set options; False if the plan refuses the combination -- loudly, with the fuzz's messages, never silently wrong"""
    import hxv

    try:
        for k, v in opts.items():
            sec.set_option(k, v)
        return True
    except hxv.HxvError as e:
        assert "block larger" in str(e) or "does not fit" in str(e) or "must be" in str(e) or "needs the whole gathered vector" in str(e), str(e)
        return False


def _order_taken(sec):
    return sec.row_perm is not None and not np.array_equal(sec.row_perm, np.arange(sec.DimUp))


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_random_models_in_device_row_order_match_the_oracle(built, forced, monkeypatch, seed):
    import torch
    import hxv
    from oracle.oracle import OracleSector

    c = _draw(seed)
    m, nup, ndw, P = c["model"], c["nup"], c["ndw"], c["nranks"]
    nd = m.Norb > 1 and (m.Jx != 0.0 or m.Jp != 0.0)
    forced(c["bits"])
    what = (seed, m.Nlat, m.Norb, m.Nspin, m.Nbath, nup, ndw, c["bits"], c["tile_bits"], P, c["exchange"])
    orc = OracleSector(m, nup, ndw)
    rng = np.random.default_rng(c["vseed"])
    v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
    v /= np.linalg.norm(v)
    ref = orc.spMatVec_main(v)
    scale = max(np.abs(ref).max(), 1e-300)
    tol = 2e-13 * scale
    maps = (orc.map_up(), orc.map_dw())
    lad_ref = []
    for o, spin, cr in c["ladders"]:
        ot = OracleSector(m, *_target(c, spin, cr))
        lad_ref.append(apply_op(v, maps, (ot.map_up(), ot.map_dw()), o, spin, cr))
        ot.close()
    rec_ref = record_numpy(m, *maps, v, 0.6)

    # ---- the product on every rank's handle (the all-gather layout, no communicator): the fuzz's option draws, both kernels, spH0nd both ways
    families = [{}, c["opts"], {"kernel": 0}] + ([{"kernel": 1, "fold_nd": 0}, {"kernel": 0, "fold_nd": 0}, {"kernel": 1, "fold_nd": 1}] if nd else [])
    for rank in range(P):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=rank, nranks=P)
        if not _set(sec, {"tile_bits_up": c["tile_bits"]}):
            sec.close()
            continue
        if sec.row_perm is not None:
            assert sorted(sec.row_perm.tolist()) == list(range(sec.DimUp)) and set(np.unique(sec.row_sign).tolist()) <= {-1, 1}
        dv = torch.from_numpy(sec.to_gather_layout(v, P)).cuda()
        want = ref[sec.mpiIshift: sec.mpiIshift + sec.vecDim]
        for o in families:
            if not _set(sec, o):
                continue
            got = sec.unpad(sec.apply_device(dv)).cpu().numpy()
            assert np.abs(got - want).max() <= tol, (what, rank, o)
        sec.close()

    # ---- unsplit: host arrays, real vectors, the Lanczos recurrence, the drivers, ladders and the observables record
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    sec.set_option("tile_bits_up", c["tile_bits"])
    assert np.abs(sec.apply_host(v) - ref).max() <= tol, what
    if sec.real_vectors_available:
        xr = np.ascontiguousarray(v.real)
        want_r = orc.spMatVec_main(xr.astype(np.complex128))
        assert np.abs(sec.apply_device_real(torch.from_numpy(xr).cuda()).cpu().numpy() - want_r.real).max() <= tol, what
    a_o, b_o = orc.lanc_tridiag(v, 12)
    for fused in (1, 0):
        sec.set_option("lanczos_fused", fused)
        a, b, _ = sec.lanczos_tridiag(sec.pad(torch.from_numpy(v).cuda()), 12)
        k = min(8, len(a_o))
        assert np.abs(a[:k] - a_o[:k]).max() < 1e-10 and np.abs(b[:k] - b_o[:k]).max() < 1e-10, (what, fused)
    sec.set_option("lanczos_fused", 1)
    if 12 <= orc.Dim <= 3000:
        w = np.linalg.eigvalsh(orc.dense())
        e0, x, _ = sec.lanczos_eigh(600, 1e-13)
        x = x.cpu().numpy()
        assert abs(e0 - w[0]) <= 1e-9 * max(1.0, abs(w[0])), (what, e0, w[0])
        assert np.linalg.norm(orc.spMatVec_main(x) - e0 * x) <= 1e-6 * max(1.0, np.abs(w).max()), what
        ev, X, nconv, _ = sec.eigh_lowest(1, 16)
        assert abs(ev[0] - w[0]) <= 1e-9 * max(1.0, abs(w[0])), what
        x = X[0].cpu().numpy()
        assert np.linalg.norm(orc.spMatVec_main(x) - ev[0] * x) <= 1e-6 * max(1.0, np.abs(w).max()), what
    dpsi = sec.pad(torch.from_numpy(v).cuda())
    for (o, spin, cr), lr in zip(c["ladders"], lad_ref):
        tgt = hxv.HxvSector.from_model(m, *_target(c, spin, cr))
        out, _ = sec.apply_ladder(tgt, o, spin, cr, dpsi, out=torch.zeros(tgt.localElems, dtype=torch.complex128, device="cuda"))
        assert np.array_equal(tgt.unpad(out).cpu().numpy(), lr), (what, o, spin, cr)     # coefficient 1: the same numbers, bit for bit
        tgt.close()
    assert np.abs(sec.observables_record(dpsi, 0.6) - rec_ref).max() < 1e-13, what
    sec.close()

    # ---- thread ranks (the RCCL branches) through the drawn exchange: slab products, both ladders (the dw one is a column exchange) and the record
    if P > 1:
        monkeypatch.setenv("HXV_RCCL_LIB", str(built.build_rccl_double()))   # (RCCL branches: a rank's communicator serves its three sectors)
        hxv.set_exchange_default(c["exchange"])
        try:
            def rank(r, group):
                s = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=P)
                tg = [hxv.HxvSector.from_model(m, *_target(c, spin, cr), rank=r, nranks=P) for _, spin, cr in c["ladders"]]
                for x in [s] + tg:
                    x.set_option("tile_bits_up", c["tile_bits"])
                    group.join(x)
                lo, hi = s.mpiIshift, s.mpiIshift + s.vecDim
                slab = s.pad(torch.from_numpy(v[lo:hi].copy()).cuda(), s.mpiQdw)
                prods = []
                for o in ({"kernel": 1}, {"kernel": 0}) + (({"kernel": 1, "fold_nd": 0}, {"kernel": 1, "fold_nd": 1}) if nd else ()):
                    for k, val in o.items():
                        s.set_option(k, val)
                    prods.append((o, s.unpad(s.apply_device_slab(slab)).cpu().numpy()))
                lads = []
                for (o, spin, cr), t in zip(c["ladders"], tg):
                    out, _ = s.apply_ladder(t, o, spin, cr, slab, out=torch.zeros(t.localElems, dtype=torch.complex128, device="cuda"))
                    lads.append((t.mpiIshift, t.vecDim, t.unpad(out).cpu().numpy()))
                rec = s.observables_record(slab, 0.6)
                taken = _order_taken(s)
                for x in [s] + tg:
                    x.close()
                return lo, hi, prods, lads, rec, taken

            res = hxv.run_ranks(P, rank, transport="rccl")
        finally:
            hxv.set_exchange_default("allgather")
        for r, (lo, hi, prods, lads, rec, taken) in enumerate(res):
            for o, hv in prods:
                assert np.abs(hv - ref[lo:hi]).max() <= tol, (what, r, o)
            for (tlo, tn, got), lr in zip(lads, lad_ref):
                assert np.array_equal(got, lr[tlo: tlo + tn]), (what, r)
            assert np.abs(rec - rec_ref).max() < 1e-13, (what, r)


def test_the_sweep_reaches_the_row_order_where_it_claims_to(built, forced):
    """Coverage floors of the sweep above, from the sectors its seeds open: a non-identity order on most seeds, and on complex H_up, with the
    spH0nd block and on split sectors often enough that a wrong sign or amplitude on any of those paths fails some seed."""
    import hxv
    from oracle.oracle import OracleSector

    n = dict(order=0, complex=0, nd=0, split=0)
    for seed in range(NSEEDS):
        c = _draw(seed)
        m = c["model"]
        forced(c["bits"])
        sec = hxv.HxvSector.from_model(m, c["nup"], c["ndw"], rank=0, nranks=c["nranks"])
        taken = _order_taken(sec)
        sec.close()
        if not taken:
            continue
        n["order"] += 1
        orc = OracleSector(m, c["nup"], c["ndw"])
        n["complex"] += bool(np.any(np.imag(orc.csr("up")[2]) != 0))
        n["nd"] += m.Norb > 1 and (m.Jx != 0.0 or m.Jp != 0.0)
        n["split"] += c["nranks"] > 1
    assert n["order"] >= 3 * NSEEDS // 4 and n["complex"] >= 8 and n["nd"] >= 8 and n["split"] >= 5, n
