"""Every documented engine option value against the oracle (include/hxv.h, "Options").

The default paths are pinned elsewhere; this file pins the branches BETWEEN the defaults: each option of groups 1 and 2 is set to
each value the header permits, one at a time on a freshly opened handle, read back, and the product compared with the CPU oracle
(max error <= 2e-13 * max|ref|, the project's H x V tolerance).  The bit-identities the header promises are asserted with torch.equal
on the padded device result, refused values must leave the handle exactly as it was, and both restart paths of hxv_eigh_lowest are
chosen on purpose and recognised by the engine's own counters.

Shapes: the smallest at which the branches still differ.  A single-block plan skips the out-of-block and block-hop code, so every
product test forces small prefix blocks (tile_bits) and asserts that both spins have several blocks and out-of-block entries.
  S1  real H, one orbital     hm_1dchain(Nlat=2, Nbath=3)                       sector (4,4)  70 x 70
  S2  complex H, Norb = 2     bhz_2d(Nbath=0, Ust=0.3, Jh=0.1)                  sector (4,3)  70 x 56
  S3  spH0nd inside pass A    bhz_2d(Nbath=0, Ust=0.4, Jh=0.1, Jx=0.25, Jp=-0.1) sector (4,3)  (pass A never runs as jobs here)
  S4  odd DimUp               hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6])   sector (2,3)  15 x 20
  S1r, S2r  rank 1 of 3 of S1 / S2 on the gather layout: a partly local dw block, a column count no multiple of the scratch group
Block bits: 3 for the 70-row spins, 2 for S4.  ONE DEPARTURE: with 3 (and 4, 5) block bits every up block of the BHZ sectors has 10 to 14
out-of-block partners, more than the 8 the job kernel keeps in registers, so pass A never runs as jobs there; the job options
(job_up, job_stages, job_groups, job_cols, job_max_blocks) take S2 / S2r with 6 block bits for the up spin (4 blocks, 8 partners at most),
where "job_up_active" reads 1 -- asserted, like the multi-block preconditions."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 2e-13
ROOT = Path(__file__).resolve().parent.parent

# ---- the option table, restated from include/hxv.h: name -> (group, default, permitted values that are tried) ------------------------
OPTIONS = {
    # 1. behaviour
    "kernel": (1, 1, (0, 1)),
    "real_vectors": (1, 1, (0, 1)),
    "lanczos_fused": (1, 1, (0, 1)),
    "lanczos_graph": (1, 1, (0, 1)),
    "lanczos_inplace": (1, 1, (0, 1)),
    "eigh_degenerate": (1, 0, (0, 1)),
    "eigh_measure_all": (1, 0, (0, 1)),
    "eigh_keep_pct": (1, 20, (5, 20, 80)),
    "eigh_fuse_restart": (1, 1, (0, 1)),
    "fold_nd": (1, 1, (0, 1)),
    "exchange_overlap": (1, 0, (0, 1)),
    # 2. tile shape and scheduling
    "cols_per_tile": (2, 4, (2, 4, 8)),
    "rows_per_tile": (2, 0, (0, 2, 4, 8)),
    "lds_budget_kb": (2, 64, (8, 64, 144)),
    "lds_budget_kb_up": (2, 64, (8, 64, 144)),
    "lds_budget_kb_dw": (2, 64, (8, 64, 144)),
    "threads_up": (2, 1024, (256, 512, 1024)),
    "threads_dw": (2, 1024, (256, 512, 1024)),
    "sort_mode": (2, 0, (0, 1, 2)),
    "sort_mode_dw": (2, 1, (0, 1)),
    "wt_cols": (2, 4, (2, 4, 8, 16)),
    "tile_bits_up": (2, -1, (2, 3)),        # (-1 = automatic: one block at these sizes, which is what this file must not test)
    "tile_bits_dw": (2, -1, (2, 3)),
    "lds_min_kb_up": (2, 0, (0, 16, 160)),
    "lds_min_kb_dw": (2, 0, (0, 16, 160)),
    "spread_banks": (2, 1, (0, 1)),
    "job_up": (2, 2, (0, 1, 2)),
    "job_groups": (2, 100, (1, 3, 100)),
    "job_cols": (2, 1, (1, 2)),
    "job_stages": (2, 4, (2, 3, 4, 8)),
    "job_max_blocks": (2, 32, (0, 32)),
    "wt_colmajor": (2, 1, (0, 1)),
    "real_dw_pairs": (2, 1, (0, 1)),
    "pair_rows": (2, -1, (-1, 0, 1)),
    "block_order": (2, -1, (-1, 0, 1, 2)),
    # 3. timing experiments: only their gate is checked
    "passes": (3, 3, ()),
    "debug": (3, 0, ()),
    "job_debug": (3, 0, ()),
}
# read-backs that the option block of the header names inside an option's description: not options
READBACKS_IN_BLOCK = {"slab_copies", "job_up_active"}
# the values no test set before this file, together (second pass of section 1)
COMBINED = (("wt_colmajor", 0), ("sort_mode_dw", 0), ("spread_banks", 0), ("real_dw_pairs", 0), ("cols_per_tile", 2), ("rows_per_tile", 2))
JOB_OPTIONS = ("job_up", "job_stages", "job_groups", "job_cols", "job_max_blocks")
PLAN_STATS = ("tile_bits_up", "tile_bits_dw", "nblocks_up", "nblocks_dw", "n_in_up", "n_out_up", "n_in_dw", "n_out_dw", "k_in_up", "k_out_up", "k_in_dw",
              "k_out_dw", "max_block_up", "max_block_dw", "max_outer_up", "max_outer_dw", "table_classes_up", "table_classes_dw", "job_up_active")


def header_option_names():
    """The quoted names of the "Options" comment block of include/hxv.h (CPU only), "a[_x|_y]" and "a_x|_y" spelled out."""
    text = (ROOT / "include" / "hxv.h").read_text()
    block = text[text.index("/* Options (name, value)"): text.index("hxv_get_option additionally reports")]
    names = set()
    for tok in re.findall(r'"([^"\n]+)"', block):
        m = re.fullmatch(r"(\w+)\[([\w|]+)\]", tok)
        if m:
            names.add(m.group(1))
            names.update(m.group(1) + s for s in m.group(2).split("|"))
        elif "|" in tok:
            first, *rest = tok.split("|")
            names.add(first)
            names.update(first[: first.rindex("_")] + s for s in rest)
        else:
            names.add(tok)
    return names


def _readback(sec, name, value):
    """what hxv_get_option must answer after set_option(name, value) (include/hxv.h, last paragraph of the option block)"""
    if name == "lds_budget_kb":
        return (sec.get_option("lds_budget_kb_up"), sec.get_option("lds_budget_kb_dw")) == (value, value)
    if name == "rows_per_tile" and value == 0:
        return sec.get_option(name) == 4     # (0 = 4 for sectors whose row panels fit the L2: every sector of this file)
    return sec.get_option(name) == value


# ---- shapes and their references, computed once ---------------------------------------------------------------------------------------
def _shape_model(key):
    from hxv import models

    return {
        "S1": (models.hm_1dchain(Nlat=2, Nbath=3), (4, 4), 3),
        "S2": (models.bhz_2d(Nbath=0, Ust=0.3, Jh=0.1), (4, 3), 3),
        "S3": (models.bhz_2d(Nbath=0, Ust=0.4, Jh=0.1, Jx=0.25, Jp=-0.1), (4, 3), 3),
        "S4": (models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]), (2, 3), 2),
    }[key[:2]]


SHAPES = ("S1", "S2", "S3", "S4", "S1r", "S2r")
_REF = {}


def _ref(key):
    """model, sector, (rank, nranks), block bits, the seeded complex vector and the oracle's products of it and of its real part"""
    if key[:2] not in _REF:
        from oracle.oracle import OracleSector

        m, (nup, ndw), bits = _shape_model(key)
        orc = OracleSector(m, nup, ndw)
        rng = np.random.default_rng(20 + SHAPES.index(key[:2]))
        v = rng.standard_normal(orc.Dim) + 1j * rng.standard_normal(orc.Dim)
        full = orc.spMatVec_main(v)
        real = orc.spMatVec_main(v.real.astype(np.complex128))
        dims = (orc.DimUp, orc.DimDw)
        orc.close()
        _REF[key[:2]] = dict(model=m, sector=(nup, ndw), bits=bits, v=v, full=full, real=real, dims=dims)
    r = dict(_REF[key[:2]])
    r["shard"] = (1, 3) if key.endswith("r") else (0, 1)
    return r


def _open(key, job=False):
    """a fresh handle of shape `key` with its block bits forced (job: the up bits at which pass A can run as jobs, see the module docstring)"""
    import hxv

    r = _ref(key)
    rank, nranks = r["shard"]
    sec = hxv.HxvSector.from_model(r["model"], *r["sector"], rank=rank, nranks=nranks)
    assert (sec.DimUp, sec.DimDw) == r["dims"]
    sec.set_option("tile_bits_up", 6 if (job and key[:2] == "S2") else r["bits"])
    sec.set_option("tile_bits_dw", r["bits"])
    return sec


def _assert_multiblock(sec, what):
    got = {n: sec.get_option(n) for n in ("nblocks_up", "nblocks_dw", "n_out_up", "n_out_dw")}
    assert got["nblocks_up"] > 1 and got["nblocks_dw"] > 1 and got["n_out_up"] > 0 and got["n_out_dw"] > 0, (what, got)


def _device_inputs(sec, key):
    import torch

    r = _ref(key)
    if "dv" not in _REF[key[:2]]:
        _REF[key[:2]]["dv"] = {}
    cache = _REF[key[:2]]["dv"]
    if r["shard"] not in cache:   # (the layouts depend on the sector's pitch and split only: shared by every handle of the shape)
        dv = torch.from_numpy(sec.to_gather_layout(r["v"], r["shard"][1])).cuda()
        real_h = key[:2] in ("S1", "S4")   # (the hm_1dchain models; BHZ has complex amplitudes)
        dr = sec.pad_real(torch.from_numpy(np.ascontiguousarray(r["v"].real)).cuda()) if (real_h and r["shard"][1] == 1) else None
        cache[r["shard"]] = (dv, dr)
    return cache[r["shard"]]


def _products(sec, key):
    """(padded complex result, padded real result or None) of the shape's vector on this handle"""
    import torch

    dv, dr = _device_inputs(sec, key)
    assert dv.numel() == sec.fullElems
    hv = sec.apply_device(dv)
    hr = None
    if dr is not None and sec.real_vectors_available:
        hr = sec.apply_device_real(dr)
    torch.cuda.synchronize()
    return hv, hr


def _check_against_oracle(sec, key, what):
    r = _ref(key)
    hv, hr = _products(sec, key)
    ref = r["full"][sec.mpiIshift: sec.mpiIshift + sec.vecDim]
    got = sec.unpad(hv).cpu().numpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= TOL, (what, "complex", err)
    if key in ("S1", "S4") and sec.get_option("kernel") == 1:
        assert hr is not None, (what, "real H, unsplit, tiled kernels: the real-vector product must be available")
    if hr is not None:
        refr = r["real"].real
        assert np.abs(r["real"].imag).max() == 0.0
        errr = np.abs(sec.unpad_real(hr).cpu().numpy() - refr).max() / np.abs(refr).max()
        assert errr <= TOL, (what, "real", errr)
    return hv, hr


# ---- 1. every value of every group-1 and group-2 option ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, (grp, _, _) in OPTIONS.items() if grp in (1, 2)])
def test_every_permitted_value_matches_the_oracle(built, name):
    """One option at a time on a freshly opened handle: set, read back, multi-block precondition, complex product (and the real-vector
    product where it is available) against the oracle.  The job options run with job_up = 1 and require that pass A then DOES run as
    jobs on S1, S2 and S4 (6 up block bits on S2, module docstring) -- except for the two values that switch the jobs off by design."""
    job = name in JOB_OPTIONS
    for value in OPTIONS[name][2]:
        for key in SHAPES:
            sec = _open(key, job=job)
            if job and name != "job_up":
                sec.set_option("job_up", 1)
            sec.set_option(name, value)
            what = (name, value, key)
            assert _readback(sec, name, value), (what, sec.get_option(name))
            _assert_multiblock(sec, what)
            if job and key[:2] != "S3":
                on = 1
                if (name, value) in (("job_cols", 2), ("job_max_blocks", 0)) or (name == "job_up" and value != 1):
                    on = 0
                assert sec.get_option("job_up_active") == on, what
            _check_against_oracle(sec, key, what)
            sec.close()


@pytest.mark.parametrize("key", SHAPES)
def test_previously_untested_values_together(built, key):
    """wt_colmajor 0, sort_mode_dw 0, spread_banks 0, real_dw_pairs 0, cols_per_tile 2 and rows_per_tile 2 on one handle."""
    sec = _open(key)
    for name, value in COMBINED:
        sec.set_option(name, value)
    for name, value in COMBINED:
        assert sec.get_option(name) == value, (key, name)
    _assert_multiblock(sec, key)
    _check_against_oracle(sec, key, ("combined", key))
    sec.close()


@pytest.mark.parametrize("key", ["S1", "S2"])
@pytest.mark.parametrize("stages", [2, 3, 4, 8])
def test_job_ring_depth_with_the_lanczos_epilogue(built, key, stages):
    """The fused Lanczos epilogue streams a third vector (the previous Lanczos vector) through the job kernel's tile ring: 24 steps of
    hxv_lanczos_tridiag with lanczos_fused = 1 against the unfused recurrence on the same handle, 1e-10 relative on alanc and blanc (the
    bound of test_fused_epilogue_matches_plain_recurrence_for_every_kernel_family), for every ring depth."""
    import torch

    r = _ref(key)
    sec = _open(key, job=True)
    sec.set_option("job_up", 1)
    sec.set_option("job_stages", stages)
    assert sec.get_option("job_stages") == stages and sec.get_option("job_up_active") == 1
    _assert_multiblock(sec, (key, stages))
    sec.set_option("real_vectors", 0)
    start = torch.from_numpy(r["v"] / np.linalg.norm(r["v"])).cuda()
    sec.set_option("lanczos_fused", 0)
    a0, b0, n0 = sec.lanczos_tridiag(start, 24)
    sec.set_option("lanczos_fused", 1)
    assert sec.get_option("lanczos_fused") == 1
    a1, b1, n1 = sec.lanczos_tridiag(start, 24)
    assert n0 == n1 == 24
    assert np.abs(a1 - a0).max() <= 1e-10 * np.abs(a0).max(), (key, stages)
    assert np.abs(b1 - b0).max() <= 1e-10 * np.abs(b0).max(), (key, stages)
    sec.close()


# ---- 2. the bit-identities the header promises ----------------------------------------------------------------------------------------
def _padded_products(key, options):
    sec = _open(key)
    for name, value in options:
        sec.set_option(name, value)
        assert sec.get_option(name) == value
    _assert_multiblock(sec, (key, options))
    hv, hr = _products(sec, key)
    hv, hr = hv.clone(), (hr.clone() if hr is not None else None)
    sec.close()
    return hv, hr


@pytest.mark.parametrize("key", ["S1", "S2", "S3", "S4"])
def test_wt_colmajor_is_bit_identical(built, key):
    """Row-major against column-major patches of the blocked dw-hop scratch: the complex product on S1, S2 and S3; the real-vector
    product on S1 and S4 with real_dw_pairs = 0 (with row pairs the scratch is column-major whatever the option says)."""
    import torch

    if key != "S4":
        a, _ = _padded_products(key, (("wt_colmajor", 0),))
        b, _ = _padded_products(key, (("wt_colmajor", 1),))
        assert torch.equal(a, b), key
    if key in ("S1", "S4"):
        _, a = _padded_products(key, (("real_dw_pairs", 0), ("wt_colmajor", 0)))
        _, b = _padded_products(key, (("real_dw_pairs", 0), ("wt_colmajor", 1)))
        assert a is not None and b is not None and torch.equal(a, b), key


@pytest.mark.parametrize("rows", [2, 4, 8])
@pytest.mark.parametrize("key", ["S1", "S4"])
def test_real_dw_pairs_is_bit_identical(built, key, rows):
    """Pass B of the real-vector product on pairs of rows (the complex kernel) against the double kernel, every tile height."""
    import torch

    _, a = _padded_products(key, (("rows_per_tile", rows), ("real_dw_pairs", 0)))
    _, b = _padded_products(key, (("rows_per_tile", rows), ("real_dw_pairs", 1)))
    assert a is not None and b is not None and torch.equal(a, b), (key, rows)


@pytest.mark.parametrize("options", [(), COMBINED], ids=["default", "combined"])
@pytest.mark.parametrize("key", ["S1", "S2", "S3", "S4"])
def test_product_is_reproducible(built, key, options):
    """The same call twice on one handle, and on two handles of the same sector: the same bits, pad rows included."""
    import torch

    sec = _open(key)
    for name, value in options:
        sec.set_option(name, value)
    _assert_multiblock(sec, (key, options))
    a, ar = _products(sec, key)
    a, ar = a.clone(), (ar.clone() if ar is not None else None)
    b, br = _products(sec, key)
    assert torch.equal(a, b), key
    assert (ar is None) == (br is None) and (ar is None or torch.equal(ar, br)), key
    sec.close()
    c, cr = _padded_products(key, options)
    assert torch.equal(a, c), key
    assert (ar is None) == (cr is None) and (ar is None or torch.equal(ar, cr)), key


# ---- 3. refusals leave the handle as it was --------------------------------------------------------------------------------------------
def _state(sec):
    return {n: sec.get_option(n) for n in list(OPTIONS) + list(PLAN_STATS) if n != "lds_budget_kb"}


REFUSALS = [("job_stages", 1, r"job_stages must be in \[2,8\]"), ("job_stages", 9, r"job_stages must be in \[2,8\]"),
            ("eigh_keep_pct", 4, r"eigh_keep_pct must be in \[5,80\]"), ("eigh_keep_pct", 81, r"eigh_keep_pct must be in \[5,80\]"),
            ("lds_min_kb_up", 161, r"lds_min_kb must be in \[0,160\]"), ("cols_per_tile", 3, "cols_per_tile must be 2, 4 or 8"),
            ("wt_cols", 5, "wt_cols must be 2, 4, 8 or 16"), ("threads_up", 128, "threads must be 256, 512 or 1024"),
            ("block_order", 3, "block_order must be -1, 0, 1 or 2"), ("pair_rows", 2, "pair_rows must be -1, 0 or 1"),
            ("no_such_option", 1, "unknown option no_such_option")]


@pytest.mark.parametrize("name,value,message", REFUSALS, ids=[f"{n}={v}" for n, v, _ in REFUSALS])
def test_refused_value_leaves_the_handle_as_it_was(built, name, value, message):
    """hxv_set_option assigns the new plan only after make_tile_plan accepted it: after a refusal every getter answers what it answered
    before and the product has the same bits.  On a handle that already carries non-default options, so that "as it was" is not "default"."""
    import torch
    import hxv

    for key in ("S1", "S2"):
        sec = _open(key)
        for n, v in COMBINED + (("wt_cols", 8), ("job_stages", 3), ("eigh_keep_pct", 35), ("lds_min_kb_up", 16), ("threads_up", 512),
                                ("block_order", 0), ("pair_rows", 1)):
            sec.set_option(n, v)
        before = _state(sec)
        hv, hr = _products(sec, key)
        hv, hr = hv.clone(), (hr.clone() if hr is not None else None)
        with pytest.raises(hxv.HxvError, match=message):
            sec.set_option(name, value)
        assert _state(sec) == before, (key, name, value)
        _assert_multiblock(sec, (key, name, value))
        hv2, hr2 = _products(sec, key)
        assert torch.equal(hv, hv2), (key, name, value)
        assert (hr is None) == (hr2 is None) and (hr is None or torch.equal(hr, hr2)), (key, name, value)
        sec.close()


def test_header_and_engine_name_the_same_options(built):
    """The option block of include/hxv.h against this file's table (a name added to the header needs a row here), and every name accepted
    by hxv_set_option with its default.  Group 3 beyond its gate is not this file's business (tests/test_gpu_comm.py holds the gate)."""
    import torch
    import hxv

    assert header_option_names() == set(OPTIONS) | READBACKS_IN_BLOCK
    key = "S2"
    sec = _open(key)
    hv0, _ = _products(sec, key)
    hv0 = hv0.clone()
    bits = (sec.get_option("tile_bits_up"), sec.get_option("tile_bits_dw"))
    old = os.environ.pop("HXV_EXPERIMENTS", None)
    try:
        for name, (group, default, _) in OPTIONS.items():
            if name.startswith("tile_bits"):
                continue                       # (their default, automatic, is set last: it changes the plan)
            sec.set_option(name, default)
            if group != 3:
                assert _readback(sec, name, default), name
        for name in READBACKS_IN_BLOCK:
            with pytest.raises(hxv.HxvError, match="unknown option"):
                sec.set_option(name, 0)
        before = _state(sec)
        for name, value in (("passes", 2), ("debug", 32), ("job_debug", 1)):   # a gated refusal changes nothing either
            with pytest.raises(hxv.HxvError, match="HXV_EXPERIMENTS"):
                sec.set_option(name, value)
        assert _state(sec) == before
    finally:
        if old is not None:
            os.environ["HXV_EXPERIMENTS"] = old
    assert (sec.get_option("tile_bits_up"), sec.get_option("tile_bits_dw")) == bits
    hv1, _ = _products(sec, key)
    assert torch.equal(hv0, hv1)               # defaults over defaults, and the refusals: the same product
    for name in ("tile_bits_up", "tile_bits_dw"):
        sec.set_option(name, OPTIONS[name][1])
    _check_against_oracle(sec, key, "defaults")
    sec.close()


# ---- 4. both restart paths of hxv_eigh_lowest, chosen on purpose -----------------------------------------------------------------------
_SPEC = {}


def _spectrum(key):
    """(model, sector, H as a sparse matrix, lowest 8 eigenvalues of the oracle's dense H by numpy.linalg.eigvalsh), once per session"""
    if key not in _SPEC:
        import scipy.sparse as sp
        from hxv import models
        from oracle.oracle import OracleSector

        if key == "LOCK":
            m, sector = models.bhz_2d(Nbath=0), (4, 4)
        else:
            m, sector, _ = _shape_model(key)
        Hd = OracleSector(m, *sector).dense()
        if np.abs(Hd.imag).max() == 0.0:
            Hd = np.ascontiguousarray(Hd.real)
        ev = np.linalg.eigvalsh(Hd)[:8].copy()
        _SPEC[key] = (m, sector, sp.csr_matrix(Hd), ev)
    return _SPEC[key]


def _eigh_problem(mode):
    """mode -> (model, sector, H, reference eigenvalues, real_vectors)"""
    if mode in ("S1_real", "S1_complex"):
        return _spectrum("S1") + (1 if mode == "S1_real" else 0,)
    if mode == "S2":
        return _spectrum("S2") + (0,)
    from test_gpu_lanczos import _c2e_matrix   # C2 with bath levels, Dim = 853 776, ARPACK reference (shared with that file's tests)

    m, H, ref = _c2e_matrix()
    return m, (6, 6), H, ref, (1 if mode == "C2_real" else 0)


def _solve(sec, H, ref, neigen, ncv, what):
    """one hxv_eigh_lowest(maxrestart 512, tol 0) with the bounds of test_eigh_lowest_large_krylov_basis; -> (eigenvalues, counters)"""
    ev, X, nconv, _ = sec.eigh_lowest(neigen, ncv, 512, 0.0)
    cnt = {n: sec.get_option("eigh_last_" + n) for n in ("restarts", "fused_restarts", "fused_first_steps", "check_products")}
    Xh = X.cpu().numpy().T
    assert nconv == neigen, (what, nconv)
    assert np.abs(ev - ref[:neigen]).max() < 1e-10, (what, ev, ref[:neigen])
    assert np.linalg.norm(H @ Xh - Xh * ev, axis=0).max() < 1e-8, what
    assert np.abs(Xh.conj().T @ Xh - np.eye(neigen)).max() < 1e-9, what
    assert cnt["restarts"] >= 2, (what, cnt)      # (else the restart code under test never ran)
    assert 0 <= cnt["fused_restarts"] <= cnt["restarts"], (what, cnt)
    return ev, cnt


def _eigh_sector(mode):
    import hxv

    m, sector, H, ref, real_vectors = _eigh_problem(mode)
    sec = hxv.HxvSector.from_model(m, *sector)
    sec.set_option("real_vectors", real_vectors)
    sec.set_option("eigh_degenerate", 1)           # (the dense spectrum holds every copy of a degenerate level)
    return sec, H, ref, real_vectors


@pytest.mark.parametrize("neigen,ncv", [(3, 12), (4, 24)])
@pytest.mark.parametrize("mode", ["S1_real", "S1_complex", "S2"])
def test_eigh_fused_and_separate_restart_passes(built, mode, neigen, ncv):
    """eigh_fuse_restart 1 against 0 at the default eigh_keep_pct, where few enough Ritz vectors are kept for the fused kernels: with the
    option on the counters must show tr_rotate_dots and tr_axpy_mdot at work, with it off neither; same eigenvalues to 1e-10."""
    sec, H, ref, real_vectors = _eigh_sector(mode)
    out = {}
    for fuse in (1, 0):
        sec.set_option("eigh_fuse_restart", fuse)
        assert sec.get_option("eigh_fuse_restart") == fuse
        ev, cnt = _solve(sec, H, ref, neigen, ncv, (mode, neigen, ncv, fuse))
        assert sec.get_option("lanczos_real_last") == real_vectors
        if fuse:
            assert cnt["fused_restarts"] > 0 and cnt["fused_first_steps"] > 0, (mode, cnt)
        else:
            assert cnt["fused_restarts"] == 0 and cnt["fused_first_steps"] == 0, (mode, cnt)
        out[fuse] = ev
    assert np.abs(out[1] - out[0]).max() < 1e-10
    sec.close()


@pytest.mark.parametrize("pct", [5, 20, 80])
@pytest.mark.parametrize("mode", ["S1_real", "S1_complex", "S2"])
def test_eigh_keep_pct_selects_the_restart_path(built, mode, pct):
    """(neigen, ncv) = (4, 40): at 80 per cent more Ritz vectors are kept than the fused kernels handle, so although eigh_fuse_restart is 1
    the rotation, the copy and the multi-dot run as separate passes and a cycle's first step takes the tr_maxpy arrow path; at 5 and 20
    the fused kernels run.  Which path ran is read from the engine's counters, not recomputed here.  (The product count is not bounded:
    it legitimately changes by large factors with this option.)"""
    sec, H, ref, real_vectors = _eigh_sector(mode)
    sec.set_option("eigh_keep_pct", pct)
    assert sec.get_option("eigh_keep_pct") == pct and sec.get_option("eigh_fuse_restart") == 1
    _, cnt = _solve(sec, H, ref, 4, 40, (mode, pct))
    assert sec.get_option("lanczos_real_last") == real_vectors
    if pct == 80:
        assert cnt["fused_restarts"] == 0 and cnt["fused_first_steps"] == 0, (mode, pct, cnt)
    else:
        assert cnt["fused_restarts"] > 0 and cnt["fused_first_steps"] > 0, (mode, pct, cnt)
    sec.close()


@pytest.mark.parametrize("mode,ncv", [(mode, ncv) for mode in ("S1_real", "S1_complex", "S2") for ncv in (8, 9, 16, 17, 32, 33)] +
                         [("C2_real", 64), ("C2_complex", 64)])
def test_eigh_basis_sizes_at_the_edges_of_the_rotation_kernels(built, mode, ncv):
    """tr_rotate and tr_rotate_dots are instantiated for bases of up to 8, 16, 32 and 64 (MAXCV) vectors: both sides of every edge, with
    neigen = 2, once through the fused and once through the separate passes.  ncv = 64 converges within one or two restarts on the
    3920- and 4900-state sectors (the numpy restatement of the algorithm predicts 1 to 2), so that size runs on C2 (hm_1dchain with bath
    levels, sector (6,6), Dim = 853 776, ARPACK reference; its H is real) with real and with complex vectors instead."""
    sec, H, ref, real_vectors = _eigh_sector(mode)
    out = {}
    for fuse in (1, 0):
        sec.set_option("eigh_fuse_restart", fuse)
        ev, cnt = _solve(sec, H, ref, 2, ncv, (mode, ncv, fuse))
        assert sec.get_option("lanczos_real_last") == real_vectors
        if fuse:
            assert cnt["fused_restarts"] > 0, (mode, ncv, cnt)
        else:
            assert cnt["fused_restarts"] == 0 and cnt["fused_first_steps"] == 0, (mode, ncv, cnt)
        out[fuse] = ev
    assert np.abs(out[1] - out[0]).max() < 1e-10
    sec.close()


def test_eigh_locking_rounds_through_the_separate_passes(built):
    """BHZ 2x2 sector (4,4) has a doubly degenerate second level (test_eigh_lowest_recovers_degenerate_levels: E = -5.80307083,
    -5.69466351 x 2, -5.61135083): with eigh_fuse_restart = 0 and eigh_keep_pct = 80 the locking round must still find the second copy."""
    import hxv

    m, sector, H, ref = _spectrum("LOCK")
    assert abs(ref[1] - ref[2]) < 1e-10 and np.allclose(ref[:4], [-5.80307083, -5.69466351, -5.69466351, -5.61135083], atol=5e-9)
    sec = hxv.HxvSector.from_model(m, *sector)
    sec.set_option("eigh_degenerate", 1)
    sec.set_option("eigh_fuse_restart", 0)
    sec.set_option("eigh_keep_pct", 80)
    ev, cnt = _solve(sec, H, ref, 3, 20, "locking")
    assert cnt["fused_restarts"] == 0 and cnt["fused_first_steps"] == 0, cnt
    assert cnt["check_products"] > 0, cnt           # the locking rounds ran
    assert abs(ev[1] - ev[2]) < 1e-10               # both copies
    sec.close()
