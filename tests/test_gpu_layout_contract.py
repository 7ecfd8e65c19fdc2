"""The device vector layout contract (include/hxv.h, DEVICE VECTOR LAYOUT and the all-gather layout of hxv_apply_device): every column holds
DimUp live rows padded to the pitch, the products never read a pad row and never write one, the Lanczos entries get and return zero pad rows,
and the unused column slot of a short rank in the all-gather layout is dead storage.

Every other test builds its inputs with zero pads and reads its outputs through unpad(), so it sees neither a pad row that is read (the
value is zero) nor one that is written (nobody looks).  Here the inputs carry a quiet NaN in every dead element -- 0 * NaN = NaN, so any
read that feeds arithmetic reaches a live row -- and every output buffer starts as one sentinel NaN bit pattern, compared BITWISE in the
pad rows afterwards (a write of anything, zero included, shows).  Live rows go back to the reference's order and meet the CPU oracle.
The vectors are built natively (pitch, device row order) and handed over in the native layout only.

The helpers at the top work on any torch tensor; test_layout_helpers_on_a_fake_layout checks them on the CPU."""
from types import SimpleNamespace

import numpy as np
import pytest
from ladder_ref import apply_op

POISON = 0x7FF8_0000_0000_0BAD      # quiet NaN in dead input elements
SENTINEL = 0x7FF8_DEAD_0000_BEEF    # quiet NaN every output buffer starts as
TOL = 2e-13                          # max|got - ref| <= TOL * max|ref|, the suite's product bound


# ---- layout helpers ----------------------------------------------------------------------------------------------------------------
def lay_of(sec, real=False):
    """(DimUp, pitch, perm, sign) of a sector's device vectors: the complex pitch or the real one, the device row order or None."""
    import hxv

    pitch = hxv.load_library().hxv_pitch_real(sec._h) if real else sec.pitch
    return SimpleNamespace(dimup=sec.DimUp, pitch=pitch, perm=sec.row_perm, sign=sec.row_sign)


def _bits(t):
    """int64 view of the doubles of a float64 / complex128 tensor (shares its storage)"""
    import torch

    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int64)


def native(cols, lay, nslots=None, dtype=None, device="cpu"):
    """[ncols, DimUp] numpy array in the reference's order -> device-layout tensor of nslots (>= ncols) columns: live rows in the device
    row order with their basis signs, every pad row and every column slot past ncols POISON."""
    import torch

    cols = np.asarray(cols)
    nslots = cols.shape[0] if nslots is None else nslots
    dtype = dtype or (torch.complex128 if np.iscomplexobj(cols) else torch.float64)
    out = torch.empty(nslots, lay.pitch, dtype=dtype)
    _bits(out).fill_(POISON)
    x = torch.from_numpy(np.ascontiguousarray(cols)).to(dtype)
    if lay.perm is not None:
        out[: cols.shape[0], torch.from_numpy(lay.perm.astype(np.int64))] = x * torch.from_numpy(lay.sign.astype(np.float64)).to(dtype)
    else:
        out[: cols.shape[0], : lay.dimup] = x
    return out.reshape(-1).to(device)


def gathered(V, lay, nranks, device="cpu"):
    """[DimDw, DimUp] reference-order vector -> the all-gather layout of hxv_apply_device: nranks slabs of cmax column slots, the unused
    slot of a rank that owns one column less POISON like every pad row."""
    import torch
    from hxv import dw_split

    cmax = -(-V.shape[0] // nranks)
    parts = []
    for r in range(nranks):
        q, c0 = dw_split(V.shape[0], r, nranks)
        parts.append(native(V[c0: c0 + q], lay, cmax))
    return torch.cat(parts).to(device)


def sentinel_like(n, dtype, device):
    import torch

    out = torch.empty(n, dtype=dtype, device=device)
    _bits(out).fill_(SENTINEL)
    return out


def pad_bits_off(t, lay, bits):
    """number of doubles in the pad rows of t whose bit pattern is not `bits`"""
    b = _bits(t.view(-1, lay.pitch)[:, lay.dimup:])
    return int((b != bits).sum().item())


def live(t, lay):
    """device-layout tensor -> [ncols, DimUp] numpy array in the reference's order"""
    x = t.view(-1, lay.pitch).cpu().numpy()
    if lay.perm is not None:
        return x[:, lay.perm] * lay.sign
    return x[:, : lay.dimup]


def check_out(t, lay, ref, scale, what, pad=SENTINEL):
    """output t: pad rows still `pad` bit for bit, live rows finite and within TOL * scale of ref ([ncols, DimUp], reference order)"""
    off = pad_bits_off(t, lay, pad)
    assert off == 0, f"{what}: {off} pad doubles were written"
    got = live(t, lay)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite live rows ({int((~np.isfinite(got)).sum())}): a dead element was read"
    if ref.size:
        err = np.abs(got - ref).max()
        assert err <= TOL * scale, f"{what}: max|got - ref| = {err:.3e} > {TOL:.0e} * {scale:.3e}"


# ---- the CPU self-check of the helpers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_order", [False, True])
@pytest.mark.parametrize("real", [False, True])
def test_layout_helpers_on_a_fake_layout(row_order, real):
    """poison marks every dead element and no live one, the sentinel check sees one changed pad double, live rows come back as they went in"""
    import torch
    from hxv import dw_split

    rng = np.random.default_rng(11)
    dimup, dimdw, nranks = 13, 7, 3                      # pitch 16 (real) / 16 (complex, roundup8); slabs of 3, 2, 2 columns
    lay = SimpleNamespace(dimup=dimup, pitch=16, perm=None, sign=None)
    if row_order:
        lay.perm, lay.sign = rng.permutation(dimup).astype(np.int32), rng.choice([-1, 1], dimup).astype(np.int8)
    V = rng.standard_normal((dimdw, dimup))
    if not real:
        V = V + 1j * rng.standard_normal((dimdw, dimup))
    g = gathered(V, lay, nranks)
    cmax = 3
    assert g.numel() == nranks * cmax * lay.pitch
    dead = np.zeros((nranks * cmax, lay.pitch), dtype=bool)
    dead[:, dimup:] = True
    for r in range(nranks):
        q, c0 = dw_split(dimdw, r, nranks)
        dead[r * cmax + q: (r + 1) * cmax] = True
        assert np.array_equal(live(g.view(nranks, -1)[r][: q * lay.pitch], lay), V[c0: c0 + q])
    b = _bits(g).view(nranks * cmax, lay.pitch, *(() if real else (2,))).numpy()
    is_poison = (b == POISON) if real else (b == POISON).all(-1)
    assert np.array_equal(is_poison, dead)
    assert not ((b == POISON) if real else (b == POISON).any(-1))[~dead].any()
    assert pad_bits_off(g, lay, POISON) == 0 and pad_bits_off(g, lay, SENTINEL) > 0
    # an output: sentinel everywhere, live rows written
    dtype = torch.float64 if real else torch.complex128
    out = sentinel_like(dimdw * lay.pitch, dtype, "cpu")
    o2 = out.view(dimdw, lay.pitch)
    if row_order:
        o2[:, torch.from_numpy(lay.perm.astype(np.int64))] = torch.from_numpy(V * lay.sign)
    else:
        o2[:, :dimup] = torch.from_numpy(V)
    check_out(out, lay, V, np.abs(V).max(), "fake")
    for k, val in ((0, 0.0), (5, float("nan"))):          # one pad double changed: a plain zero, another NaN payload
        bad = out.clone()
        _bits(bad.view(dimdw, lay.pitch)[k:k + 1, dimup + 1:dimup + 2]).view(-1)[-1] = torch.tensor(val, dtype=torch.float64).view(torch.int64)
        assert pad_bits_off(bad, lay, SENTINEL) == 1
        with pytest.raises(AssertionError, match="pad doubles were written"):
            check_out(bad, lay, V, np.abs(V).max(), "fake")
    bad = out.clone()                                      # a live element off by more than the bound / a NaN in a live row
    bad.view(dimdw, lay.pitch)[2, int(lay.perm[4]) if row_order else 4] += 1e-9
    with pytest.raises(AssertionError, match="max\\|got - ref\\|"):
        check_out(bad, lay, V, np.abs(V).max(), "fake")
    bad.view(dimdw, lay.pitch)[2, int(lay.perm[4]) if row_order else 4] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        check_out(bad, lay, V, np.abs(V).max(), "fake")


# ---- models and sectors ---------------------------------------------------------------------------------------------------------------
def _chain(Ns, seed=None, bath=0):
    """Ns sites, one orbital, real H: an open chain with random bonds, a few random longer bonds and random levels (no spatial symmetry, so
    the ground states below are not degenerate).  bath > 0: hm_1dchain with that many replicas instead (Ns = Nlat * (bath + 1))."""
    from hxv import models
    from hxv.models import Model

    if bath:
        return models.hm_1dchain(Nlat=Ns // (bath + 1), Nbath=bath, eps_bath=list(np.linspace(-0.6, 0.7, bath)), xmu=0.05)
    rng = np.random.default_rng(500 + Ns if seed is None else seed)
    A = np.zeros((Ns, Ns))
    for i in range(Ns - 1):
        A[i, i + 1] = A[i + 1, i] = -(0.5 + rng.random())
    for _ in range(Ns // 3):
        i, j = rng.choice(Ns, 2, replace=False)
        A[i, j] = A[j, i] = rng.standard_normal() * 0.4
    A[np.diag_indices(Ns)] = rng.standard_normal(Ns) * 0.3
    h = A.reshape(Ns, Ns, 1, 1, 1, 1).astype(np.complex128)
    return Model(Ns, 1, 1, 0, h, np.zeros((Ns, Ns, 1, 1, 1, 1, 0)), np.zeros((Ns, 1, 1, 0)), Uloc=[1.0 + rng.random()], xmu=0.1,
                 hfmode=bool(Ns % 2), name=f"chain{Ns}")


# (Ns, nup, ndw) -> DimUp covers every residue mod 16 (every complex pad 0..7, every real pad 0..15), DimDw odd and even
RESIDUE_SECTORS = [(16, 1, 1), (3, 0, 1), (2, 1, 1), (3, 1, 2), (4, 1, 2), (5, 1, 2), (4, 2, 3), (7, 1, 2), (8, 3, 1), (9, 1, 4), (5, 2, 3),
                   (11, 1, 2), (8, 2, 3), (13, 1, 1), (9, 4, 1), (6, 2, 3), (7, 3, 3), (11, 3, 2)]
# one sector per complex pad (DimUp mod 8 = 0..7) for the Lanczos drivers: dense reference
DRIVER_SECTORS = [(8, 3, 1), (9, 1, 2), (5, 2, 2), (7, 3, 2), (6, 3, 2), (7, 2, 3), (8, 4, 1), (6, 2, 3)]
# device row order (DimUp >= 2048): DimUp % 8 == 0 and odd DimUp
ROW_ORDER_SECTORS = [(14, 7, 1), (14, 6, 1)]


def _model(Ns):
    return {14: _chain(14, bath=6), 16: _chain(16, bath=3)}[Ns] if Ns in (14, 16) else _chain(Ns)


def _open(m, nup, ndw, opts=None, **kw):
    import hxv

    sec = hxv.HxvSector.from_model(m, nup, ndw, **kw)
    for k, v in (opts or {}).items():
        sec.set_option(k, v)
    return sec


def _try_opts(sec, opts):
    """set options; False if the plan refuses the combination (loudly, with its message)"""
    import hxv

    try:
        for k, v in opts.items():
            sec.set_option(k, v)
        return True
    except hxv.HxvError as e:
        assert "block larger" in str(e) or "does not fit" in str(e) or "must be" in str(e), str(e)
        return False


def _product_case(m, nup, ndw, seed):
    from oracle.oracle import OracleSector

    orc = OracleSector(m, nup, ndw)
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
    ref = orc.spMatVec_main(v)
    return orc, v, ref, max(np.abs(ref).max(), 1e-300)


def _run_product(sec, vin):
    """hxv_apply_device into a sentinel-filled output"""
    import torch

    hv = sentinel_like(sec.localElems, torch.complex128, "cuda")
    sec.apply_device(vin, hv)
    torch.cuda.synchronize()
    return hv


COMPLEX_FAMILIES = ([{}] + [{"cols_per_tile": c, "rows_per_tile": r} for c in (2, 4) for r in (2, 4, 8)] + [{"job_up": 1}, {"kernel": 0}])


# ---- 1. hxv_apply_device, complex vectors, unsplit ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_complex_product_never_reads_or_writes_pad_rows(built):
    """tile kernels (2 / 4 columns x 2 / 4 / 8 rows per tile), the job kernel, the one-thread-per-element kernel; every DimUp residue mod 16,
    a multi-block plan at Ns = 12, the two row-ordered sectors, complex H (BHZ), the spH0nd block folded and as its own pass."""
    import hxv
    from hxv import models

    cases = [(_model(Ns), nup, ndw, None) for Ns, nup, ndw in RESIDUE_SECTORS]
    cases += [(_chain(12), 4, 3, {"lds_budget_kb_up": 8, "lds_budget_kb_dw": 8})]
    cases += [(_model(Ns), nup, ndw, "row_order") for Ns, nup, ndw in ROW_ORDER_SECTORS]
    cases += [(models.bhz_2d(Nbath=0), 4, 3, None), (models.bhz_2d(Nbath=0), 1, 2, None)]
    kana = models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15)
    cases += [(kana, 2, 3, "nd"), (kana, 3, 2, "nd"), (kana, 4, 5, "nd")]
    residues, ran = set(), 0
    for m, nup, ndw, kind in cases:
        orc, v, ref, scale = _product_case(m, nup, ndw, nup * 31 + ndw)
        base = kind if isinstance(kind, dict) else {}
        families = [dict(base, **f) for f in COMPLEX_FAMILIES]
        if kind == "nd":
            families += [{"fold_nd": 0}, {"fold_nd": 0, "kernel": 0}]
        for fam in families:
            sec = _open(m, nup, ndw)
            what = f"{m.name} ({nup},{ndw}) DimUp={sec.DimUp} DimDw={sec.DimDw} pitch={sec.pitch} {fam}"
            assert sec.pitch == -(-sec.DimUp // 8) * 8, what
            assert (sec.row_perm is not None) == (kind == "row_order"), what
            if not _try_opts(sec, fam):
                sec.close()
                continue
            if isinstance(kind, dict):
                assert sec.get_option("nblocks_up") > 1, what
            lay = lay_of(sec)
            vin = gathered(v.reshape(orc.DimDw, orc.DimUp), lay, 1, "cuda")
            hv = _run_product(sec, vin)
            if fam.get("job_up") == 1:
                assert sec.get_option("job_up_active") == 1, what
            check_out(hv, lay, ref.reshape(orc.DimDw, orc.DimUp), scale, what)
            residues.add(sec.DimUp % 16)
            ran += 1
            sec.close()
    assert residues == set(range(16)) and ran >= 200, (residues, ran)


@pytest.mark.gpu
def test_stored_matrix_sectors_never_read_or_write_pad_rows(built):
    """hxv_create_from_csr (a stored diagonal) on an odd DimUp, and with the spH0nd block given as stored rows (hxv_set_nonlocal_csr)"""
    import hxv
    from hxv import models

    for m, nup, ndw, with_nd in ((_chain(11), 3, 2, False), (_chain(7), 2, 3, False),
                                 (models.bhz_2d(Nbath=0, Ust=0.7, Jh=0.2, Jx=0.2, Jp=0.15), 2, 3, True)):
        orc, v, ref, scale = _product_case(m, nup, ndw, 7 + nup)
        for fam in ({}, {"cols_per_tile": 2, "rows_per_tile": 8}, {"kernel": 0}):
            sec = hxv.HxvSector.from_csr(orc.DimUp, orc.DimDw, orc.csr("up"), orc.csr("dw"), orc.diag(), nd=orc.csr("nd") if with_nd else None)
            what = f"from_csr {m.name} ({nup},{ndw}) nd={with_nd} {fam}"
            assert sec.row_perm is None and _try_opts(sec, fam), what
            lay = lay_of(sec)
            hv = _run_product(sec, gathered(v.reshape(orc.DimDw, orc.DimUp), lay, 1, "cuda"))
            check_out(hv, lay, ref.reshape(orc.DimDw, orc.DimUp), scale, what)
            sec.close()


# ---- 2. hxv_apply_device on split sectors, caller-gathered -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_split_product_ignores_the_unused_slot_of_short_ranks(built):
    """the all-gather layout of P = 2, 3 ranks with an uneven DimDw: the short ranks' unused slot and every pad row POISON"""
    from hxv import dw_split

    cases = [(_model(7), 1, 2), (_model(11), 1, 2), (_model(9), 4, 1), (_chain(12), 4, 3), (_model(14), 6, 1)]
    uneven = 0
    for m, nup, ndw in cases:
        orc, v, ref, scale = _product_case(m, nup, ndw, 3 * nup + ndw)
        V, R = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
        for P in (2, 3):
            uneven += orc.DimDw % P != 0
            for r in range(P):
                for fam in ({}, {"kernel": 0}):
                    sec = _open(m, nup, ndw, fam, rank=r, nranks=P)
                    lay = lay_of(sec)
                    q, c0 = dw_split(orc.DimDw, r, P)
                    assert (sec.mpiQdw, sec.mpiIshift) == (q, c0 * orc.DimUp)
                    vin = gathered(V, lay, P, "cuda")
                    assert vin.numel() == sec.fullElems
                    what = f"{m.name} ({nup},{ndw}) DimUp={sec.DimUp} DimDw={sec.DimDw} rank {r}/{P} {fam}"
                    hv = _run_product(sec, vin)
                    check_out(hv, lay, R[c0: c0 + q], scale, what)
                    sec.close()
    assert uneven >= 6, uneven


# ---- 3. hxv_apply_device_real ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_real_product_never_reads_or_writes_pad_rows(built):
    """REAL vectors (pitch roundup16): pass B on row pairs and on single rows, odd and even DimUp, every real pad 0..15"""
    import torch

    cases = [(_model(Ns), nup, ndw) for Ns, nup, ndw in RESIDUE_SECTORS] + [(_chain(12), 4, 3)] + [(_model(Ns), nup, ndw) for Ns, nup, ndw in ROW_ORDER_SECTORS]
    residues, ran = set(), 0
    for m, nup, ndw in cases:
        orc, v, _, _ = _product_case(m, nup, ndw, nup + 5 * ndw)
        x = v.real.copy()
        ref = orc.spMatVec_main(x.astype(np.complex128))
        assert np.abs(ref.imag).max() == 0.0
        ref = ref.real.reshape(orc.DimDw, orc.DimUp)
        scale = max(np.abs(ref).max(), 1e-300)
        for fam in ({"real_dw_pairs": 1}, {"real_dw_pairs": 0}, {"real_dw_pairs": 1, "rows_per_tile": 8}, {"real_dw_pairs": 1, "rows_per_tile": 2},
                    {"real_dw_pairs": 0, "cols_per_tile": 8, "rows_per_tile": 4}):
            sec = _open(m, nup, ndw)
            what = f"real {m.name} ({nup},{ndw}) DimUp={sec.DimUp} DimDw={sec.DimDw} {fam}"
            assert sec.real_vectors_available, what
            if not _try_opts(sec, fam):
                sec.close()
                continue
            lay = lay_of(sec, real=True)
            assert lay.pitch == -(-sec.DimUp // 16) * 16, what
            vin = native(x.reshape(orc.DimDw, orc.DimUp), lay).cuda()
            hv = sentinel_like(sec.DimDw * lay.pitch, torch.float64, "cuda")
            sec.apply_device_real(vin, hv)
            torch.cuda.synchronize()
            check_out(hv, lay, ref, scale, what)
            residues.add(sec.DimUp % 16)
            ran += 1
            sec.close()
    assert residues == set(range(16)) and ran >= 80, (residues, ran)


# ---- 4. the two halves of exchange mode 2 ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_panel_halves_never_read_or_write_pad_rows(built):
    """hxv_apply_dw_panel on row panels of odd and even nrows (pitch roundup8(nrows)) and hxv_apply_up_add on the slabs of two ranks"""
    import scipy.sparse as sp
    import torch
    import hxv
    from hxv import dw_split

    for m, nup, ndw in ((_model(11), 3, 2), (_model(7), 3, 3)):
        orc, v, ref, scale = _product_case(m, nup, ndw, 99)
        du, dd = orc.DimUp, orc.DimDw
        V = v.reshape(dd, du)
        rp, cols, vals = orc.csr("dw")
        Y = sp.csr_matrix((vals, cols - 1, rp), shape=(dd, dd)) @ V        # (v H_dw^T) in the [column][row] layout
        yscale = np.abs(Y).max()
        for P in (2, 3):
            for r in range(P):
                nr, u0 = dw_split(du, r, P)
                pan = hxv.HxvSector.dw_panel(m, nup, ndw, nr)
                lay = SimpleNamespace(dimup=nr, pitch=pan.pitch, perm=None, sign=None)
                assert pan.pitch == -(-nr // 8) * 8 and pan.localElems == dd * pan.pitch
                x = native(V[:, u0:u0 + nr], lay).cuda()
                y = sentinel_like(pan.localElems, torch.complex128, "cuda")
                pan.apply_dw_panel(x, y)
                torch.cuda.synchronize()
                check_out(y, lay, Y[:, u0:u0 + nr], yscale, f"dw panel {m.name} ({nup},{ndw}) nrows={nr} ({r}/{P})")
                pan.close()
        assert du % 2 == 1
        for P in (2, 3):
            for r in range(P):
                sec = _open(m, nup, ndw, rank=r, nranks=P)
                lay = lay_of(sec)
                q, c0 = dw_split(dd, r, P)
                hv = sentinel_like(sec.localElems, torch.complex128, "cuda")
                sec.apply_up_add(native(V[c0:c0 + q], lay).cuda(), native(Y[c0:c0 + q], lay).cuda(), hv)
                torch.cuda.synchronize()
                check_out(hv, lay, ref.reshape(dd, du)[c0:c0 + q], scale, f"up_add {m.name} ({nup},{ndw}) rank {r}/{P}")
                sec.close()


# ---- 5. hxv_apply_device_slab through the three exchanges --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slab_product_through_every_exchange(built):
    """thread ranks (local transport), 2 and 3 of them, all-gather / halo / two transposes: POISON pad rows in v_local, sentinels in hv_local"""
    import torch
    import hxv

    m, nup, ndw = _model(11), 3, 2                        # DimUp 165 (odd; row panels of 83 / 82 and 55 / 55 / 55 rows), DimDw 55
    orc, v, ref, scale = _product_case(m, nup, ndw, 5)
    V, R = v.reshape(orc.DimDw, orc.DimUp), ref.reshape(orc.DimDw, orc.DimUp)
    for P in (2, 3):
        for exchange in ("allgather", "halo", "alltoall"):
            hxv.set_exchange_default(exchange)

            def rank(r, group):
                sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=P)
                assert sec.exchange_mode == exchange
                group.join(sec)
                lay = lay_of(sec)
                c0 = sec.mpiIshift // sec.DimUp
                vl = native(V[c0: c0 + sec.mpiQdw], lay).cuda()
                outs = []
                for _ in range(2):                        # (twice: the second product reuses the exchange's buffers)
                    hv = sentinel_like(sec.localElems, torch.complex128, "cuda")
                    sec.apply_device_slab(vl, hv)
                    torch.cuda.synchronize()
                    outs.append(hv)
                sec.close()
                return c0, lay, outs

            try:
                res = hxv.run_ranks(P, rank, transport="local")
            finally:
                hxv.set_exchange_default("allgather")
            for r, (c0, lay, outs) in enumerate(res):
                for k, hv in enumerate(outs):
                    check_out(hv, lay, R[c0: c0 + hv.numel() // lay.pitch], scale, f"slab {exchange} rank {r}/{P} product {k}")


# ---- 6. ladder operators --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ladder_operators_write_zero_pad_rows_and_keep_them_when_accumulating(built):
    """c / c^dagger of both spins between sectors whose pitches (or row orders) differ: a fresh output comes back with +0.0 pad rows whatever
    the buffer held; an accumulated one keeps its (zero) pad rows; live rows equal the host restatement bit for bit"""
    import ctypes as C
    import torch
    import hxv

    L = hxv.load_library()
    m7, m14 = _model(7), _model(14)
    pairs = [(m7, (2, 3), 0, True), (m7, (2, 3), 0, False), (m7, (2, 3), 1, True), (m7, (2, 3), 1, False),
             (m14, (7, 1), 0, False), (m14, (6, 1), 0, True), (m14, (6, 1), 1, True), (m14, (6, 2), 1, False)]
    for m, (nup, ndw), spin, create in pairs:
        d = 1 if create else -1
        to_n = (nup + d, ndw) if spin == 0 else (nup, ndw + d)
        s0, s1 = _open(m, nup, ndw), _open(m, *to_n)
        l0, l1 = lay_of(s0), lay_of(s1)
        assert l0.pitch != l1.pitch or spin == 1                      # (a dw operator keeps DimUp)
        rng = np.random.default_rng(nup + 10 * ndw + spin)
        psi = rng.standard_normal(s0.Dim) + 1j * rng.standard_normal(s0.Dim)
        P0 = psi.reshape(s0.DimDw, s0.DimUp)
        dpsi = native(P0, l0).cuda()
        _bits(dpsi.view(-1, l0.pitch)[:, l0.dimup:]).zero_()          # a Lanczos-class input: zero pad rows
        orbs = [0, m.Ns // 2, m.Ns - 1]
        refs = [apply_op(psi, s0.maps(), s1.maps(), o, spin, create).reshape(s1.DimDw, s1.DimUp) for o in orbs]
        what = f"{m.name} ({nup},{ndw})->{to_n} spin {spin} create {create}"
        out = sentinel_like(s1.localElems, torch.complex128, "cuda")
        n2 = C.c_double()
        torch.cuda.synchronize()
        assert L.hxv_apply_ladder_axpy(s0._h, s1._h, orbs[0], spin, int(create), 1.0, 0.0, 0, dpsi.data_ptr(), out.data_ptr(), C.byref(n2)) == 0, \
            L.hxv_last_error()
        torch.cuda.synchronize()
        assert pad_bits_off(out, l1, 0) == 0, f"{what}: fresh output's pad rows are not +0.0"
        assert np.array_equal(live(out, l1), refs[0]), what
        assert abs(n2.value - np.vdot(refs[0], refs[0]).real) <= 1e-12 * max(1.0, n2.value), what
        acc = refs[0]
        for o, ref in zip(orbs[1:], refs[1:]):             # the mixed channels: the next terms added with coefficient 1 (exact)
            _, n2a = s0.apply_ladder(s1, o, spin, create, dpsi, out=out)
            torch.cuda.synchronize()
            acc = acc + ref
            assert pad_bits_off(out, l1, 0) == 0, f"{what}: accumulate changed pad rows (orbital {o})"
            assert np.array_equal(live(out, l1), acc), f"{what} accumulate orbital {o}"
            assert abs(n2a - np.vdot(acc, acc).real) <= 1e-12 * max(1.0, n2a), what
        s0.close()
        s1.close()


# ---- 7. the Lanczos drivers and the library's own vectors --------------------------------------------------------------------------------
def _phase_err(x, ref):
    """|| x - e^{i phi} ref || with the phase that aligns them"""
    ov = np.vdot(ref, x)
    return np.linalg.norm(x - ov / abs(ov) * ref)


@pytest.mark.gpu
def test_lanczos_drivers_return_zero_pad_rows(built):
    """hxv_lanczos_eigh and hxv_eigh_lowest with real_vectors 0 / 1 and lanczos_fused 0 / 1 on one sector per complex pad 0..7 and on the
    odd-DimUp row-ordered sector: the eigenvector buffer starts as sentinels and comes back with +0.0 pad rows and the oracle's eigenvector"""
    import ctypes as C
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    import torch
    import hxv
    from oracle.oracle import OracleSector

    L = hxv.load_library()
    pads = set()
    for Ns, nup, ndw in DRIVER_SECTORS + ROW_ORDER_SECTORS[1:]:
        m = _model(Ns)
        orc = OracleSector(m, nup, ndw)
        dense = orc.Dim <= 3000
        if dense:
            w, U = np.linalg.eigh(orc.dense())
            e_ref, x_ref = w[0], U[:, 0]
            assert w[1] - w[0] > 1e-3, (Ns, nup, ndw, w[:2])         # (a unique ground state to compare with)
        else:
            du, dd = orc.DimUp, orc.DimDw
            mats = [sp.csr_matrix((vals, cols - 1, rp), shape=(n, n)) for (rp, cols, vals), n in ((orc.csr("up"), du), (orc.csr("dw"), dd))]
            H = sp.diags(orc.diag()) + sp.kron(mats[1], sp.identity(du)) + sp.kron(sp.identity(dd), mats[0])
            e_ref = sla.eigsh(H.tocsr(), k=1, which="SA", tol=1e-12)[0][0]
        for real_vectors in (0, 1):
            for fused in (0, 1):
                sec = _open(m, nup, ndw, {"real_vectors": real_vectors, "lanczos_fused": fused})
                lay = lay_of(sec)
                assert (sec.row_perm is not None) == (not dense)
                what = f"{m.name} ({nup},{ndw}) DimUp={sec.DimUp} real_vectors={real_vectors} fused={fused}"
                outs = []
                vec = sentinel_like(sec.localElems, torch.complex128, "cuda")
                e, n = C.c_double(), C.c_int32()
                torch.cuda.synchronize()
                assert L.hxv_lanczos_eigh(sec._h, 600, 1e-13, C.byref(e), vec.data_ptr(), C.byref(n)) == 0, L.hxv_last_error()
                assert sec.get_option("lanczos_real_last") == real_vectors, what
                outs.append(("lanczos_eigh", e.value, vec))
                ev = np.zeros(1)
                vecs = sentinel_like(sec.localElems, torch.complex128, "cuda")
                nc, nmv = C.c_int32(), C.c_int32()
                torch.cuda.synchronize()
                assert L.hxv_eigh_lowest(sec._h, 1, 16, 512, 0.0, ev.ctypes.data_as(C.POINTER(C.c_double)), vecs.data_ptr(), C.byref(nc), C.byref(nmv)) == 0, \
                    L.hxv_last_error()
                assert nc.value == 1, what
                outs.append(("eigh_lowest", ev[0], vecs))
                torch.cuda.synchronize()
                for name, e0, x in outs:
                    assert pad_bits_off(x, lay, 0) == 0, f"{what} {name}: pad rows of the eigenvector are not +0.0"
                    xr = live(x, lay).reshape(-1)
                    assert np.isfinite(xr).all() and abs(np.linalg.norm(xr) - 1.0) < 1e-12, f"{what} {name}"
                    assert abs(e0 - e_ref) <= 1e-10 * max(1.0, abs(e_ref)), f"{what} {name}: E0 {e0!r} vs {e_ref!r}"
                    if dense:
                        assert _phase_err(xr, x_ref) <= 1e-9, f"{what} {name}: {_phase_err(xr, x_ref):.2e}"
                    else:
                        res = np.linalg.norm(orc.spMatVec_main(xr) - e0 * xr)
                        assert res <= 1e-8 * max(1.0, abs(e0)), f"{what} {name}: residual {res:.2e}"
                pads.add(sec.pitch - sec.DimUp)
                sec.close()
    assert pads == set(range(8)), pads


@pytest.mark.gpu
def test_library_owned_vectors_have_zero_pad_rows(built):
    """hxv_vector_alloc hands out zeroed vectors even when the cache hands back a dirtied buffer; hxv_vector_from_host writes zero pad rows
    into a buffer that held sentinels"""
    import ctypes as C
    import torch
    import hxv

    L = hxv.load_library()
    for Ns, nup, ndw in ((7, 3, 2), (6, 2, 3), ROW_ORDER_SECTORS[1]):
        sec = _open(_model(Ns), nup, ndw)
        lay = lay_of(sec)
        n = int(sec.localElems)

        def view(p):
            class _V:
                pass

            o = _V()
            o.__cuda_array_interface__ = {"shape": (n,), "typestr": "<c16", "data": (int(p), False), "version": 2, "strides": None}
            return torch.as_tensor(o, device="cuda")

        for _ in range(2):                                 # the second allocation may reuse the first, dirtied buffer
            d = C.c_void_p()
            assert L.hxv_vector_alloc(sec._h, C.byref(d)) == 0 and d.value
            t = view(d.value)
            torch.cuda.synchronize()
            assert int((_bits(t) != 0).sum().item()) == 0, f"hxv_vector_alloc on ({nup},{ndw}): not zeroed"
            _bits(t).fill_(SENTINEL)
            torch.cuda.synchronize()
            assert L.hxv_vector_free(sec._h, d) == 0
        v = np.random.default_rng(1).standard_normal(sec.Dim) + 1j
        t = sentinel_like(n, torch.complex128, "cuda")
        torch.cuda.synchronize()
        assert L.hxv_vector_from_host(sec._h, v.ctypes.data, t.data_ptr()) == 0, L.hxv_last_error()
        torch.cuda.synchronize()
        assert pad_bits_off(t, lay, 0) == 0, f"hxv_vector_from_host on ({nup},{ndw}): pad rows not +0.0"
        assert np.array_equal(live(t, lay).reshape(-1), v)
        sec.close()
