"""The cases of tests/nonlocal_kernels_ref.py, checked without a device before tests/test_gpu_nonlocal_kernels.py runs them on one.

IN BOUNDS: every table word of every case points inside its buffer (asserted on the words themselves, and again by the restatements, whose
every lookup refuses an index outside its array).

REACH, asserted from the tables and the geometry alone (test_reach_*):
  hxv_nonlocal_tab     written rows in the second and in the third chunk of a column; a ragged last chunk after full ones, with clamped
                       threads and written rows in it; a chunk more than needed (all of its threads clamped); all four combinations of the
                       two sign bits among the terms; Jx alone, Jp alone, both; a local column all of whose dw moves are invalid beside
                       columns that are written; an invalid up move under a valid dw move; elements without any term, some of them on a
                       (-0.0, -0.0) sentinel; a pitch above DimUp with more than one column; dw0 > 0 and DimDw > qdw
  hxv_nonlocal_kernel  one, two and three grid-stride trips, each with a ragged last trip, on a partial slab (dw0 > 0) with a vcol that is
                       not the identity; elements without a term on a (-0.0, -0.0) sentinel; both terms alone and together; both spins on
                       genuine bases of 4 to 8 orbitals
  hxv_nonlocal_csr     the same trips; rows of 0, 1, 2, 3 and 4 entries; an empty row on a (-0.0, -0.0) sentinel; columns in other dw
                       columns than the row's, outside the local slab, through a vcol that is not the identity

MUTATIONS: the numpy emulation of each kernel is accepted by the checks on every case and both kinds of values; with each of these
mistakes made in it, one at a time, some case refuses it (the check fails, or a lookup leaves its array):
  no_chunk_offset    tab              the chunk offset dropped from the row: i = threadIdx.x
  cl_mod             tab              cl computed with % rchunks instead of / rchunks
  clamped_writes     tab              a clamped thread (i >= dimup) writes
  out_dimup          tab kernel csr   the output indexed with dimup instead of pitch
  no_dw0             tab kernel       dw0 left out of the column lookup
  q_r_swapped        tab              the q and r entries exchanged (between the two dw words: exchanged in all three lookups they only
                                      visit the orbital pairs in another order, which the first version of this test showed to be no mistake)
  jx_jp_swapped      tab kernel       Jx and Jp exchanged
  sign_one_word      tab              the sign taken from one word instead of the xor
  sign_in_index      tab              the sign bit left in the index
  vcol_ignored       kernel csr       vcol ignored
  csr_zero_based     csr              the CSR column used 0-based
  stride_blockdim    kernel csr       the grid stride taken as blockDim.x only
  one_trip           kernel csr       the loop ended after its first trip
  write_without_any  tab kernel csr   hv written when `any` is false
  pad_row_read       csr              a pad row of v read (the column split by the pitch)"""
from functools import lru_cache

import numpy as np
import pytest

import nonlocal_kernels_ref as R

CASES = R.all_cases()
BY_NAME = {(k, c.name): c for k, c in CASES}
IDS = [f"{k}-{c.name}" for k, c in CASES]


@lru_cache(maxsize=None)
def prepared(kernel, name, kind):
    """(case, coefficients, terms, v, h0) of one case with one kind of values"""
    c = BY_NAME[(kernel, name)]
    coef = R.coefficients(kernel, c, kind)
    terms = R.terms_of(kernel, c, coef)
    return c, coef, terms, R.inputs(c, terms, kind), R.h0_buffer(c.nhv)


def of(kernel):
    return [c for k, c in CASES if k == kernel]


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


# ---- in bounds -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", of("tab"), ids=[c.name for c in of("tab")])
def test_tab_words_in_bounds(c):
    Q = c.nlat * c.norb * c.norb
    assert c.nd_up.shape == (Q * c.dimup,) and c.nd_dw.shape == (Q * c.dimdw,) and c.nd_up.dtype == c.nd_dw.dtype == np.uint32
    up, dw = c.nd_up[c.nd_up != R.ND_INVALID], c.nd_dw[c.nd_dw != R.ND_INVALID]
    assert ((up & R.IDX) < c.dimup).all() and ((dw & R.IDX) < c.nslots).all()
    assert c.dimup >= 1 and c.pitch >= c.dimup and c.pitch % 8 == 0 and 0 < c.dw0 and c.dw0 + c.qdw < c.dimdw
    assert c.rchunks * R.CHUNK >= c.dimup and 1 <= c.qdw * c.rchunks <= 65535


@pytest.mark.parametrize("c", of("kernel"), ids=[c.name for c in of("kernel")])
def test_search_tables_in_bounds(c):
    for m, n in ((c.map_up, c.nup), (c.map_dw, c.ndw)):
        assert (np.diff(m.astype(np.int64)) > 0).all() and (R.popc(m) == n).all() and int(m.max()) < 1 << c.ns
    assert c.nlat * c.norb <= c.ns <= 8 and c.pitch >= c.dimup and c.pitch % 8 == 0 and 0 <= c.dw0 and c.dw0 + c.qdw <= c.dimdw
    assert c.vcol.shape == (c.dimdw,) and int(c.vcol.max()) < c.nslots and len(set(c.vcol.tolist())) == c.dimdw
    assert not np.array_equal(c.vcol, np.arange(c.dimdw)) or c.dimdw == 1


@pytest.mark.parametrize("c", of("csr"), ids=[c.name for c in of("csr")])
def test_csr_tables_in_bounds(c):
    assert c.rowptr.shape == (c.qdw * c.dimup + 1,) and c.rowptr[0] == 0 and (np.diff(c.rowptr) >= 0).all()
    assert c.rowptr[-1] == c.cols.shape[0] == c.vals.shape[0]
    assert int(c.cols.min()) >= 1 and int(c.cols.max()) <= c.dimup * c.dimdw
    assert c.vcol.shape == (c.dimdw,) and int(c.vcol.max()) < c.nslots and len(set(c.vcol.tolist())) == c.dimdw
    assert c.pitch >= c.dimup and c.pitch % 8 == 0 and 0 <= c.dw0 and c.dw0 + c.qdw <= c.dimdw


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kernel,c", CASES, ids=IDS)
def test_restatement_stays_inside_and_never_reads_a_pad_row(kernel, c, kind):
    _, _, terms, v, h0 = prepared(kernel, c.name, kind)
    assert terms.read.shape == (c.nv,) and v.shape == (c.nv,) and h0.shape == (c.nhv + 1,)
    assert not terms.read.reshape(c.nslots, c.pitch)[:, c.dimup:].any()
    assert np.isnan(v.real[~terms.read]).all() and not np.isnan(v.real[terms.read]).any()
    out = terms.out
    assert len(set(out.tolist())) == out.shape[0] and ((out % c.pitch) < c.dimup).all() and int(out.max()) < c.nhv


# ---- reach -----------------------------------------------------------------------------------------------------------------------------------
def _tab_terms(c, kind="exact"):
    return prepared("tab", c.name, kind)[2]


def _written_rows(c, terms):
    w = np.zeros(c.nhv, dtype=bool)
    w[terms.out[terms.written]] = True
    return w.reshape(c.qdw, c.pitch)


def test_reach_tab_chunks():
    second = third = ragged = spare = False
    for c in of("tab"):
        w = _written_rows(c, _tab_terms(c))
        needed = -(-c.dimup // R.CHUNK)
        second |= c.rchunks >= 2 and w[:, R.CHUNK:2 * R.CHUNK].any()
        third |= c.rchunks >= 3 and w[:, 2 * R.CHUNK:3 * R.CHUNK].any()
        ragged |= needed >= 2 and c.dimup % R.CHUNK != 0 and w[:, (needed - 1) * R.CHUNK:c.dimup].any()
        spare |= c.rchunks > needed
    assert second and third and ragged and spare
    assert {-(-c.dimup // R.CHUNK) for c in of("tab")} == {1, 2, 3}
    assert set(R.TAB_DIMUPS) <= {c.dimup for c in of("tab")} and {c.qdw for c in of("tab")} == {1, 2, 3}
    assert {(c.nlat, c.norb) for c in of("tab")} >= {(1, 2), (2, 2), (1, 3)}


def test_reach_tab_signs_terms_and_invalid_moves():
    signs, on = set(), set()
    dead_col = dead_up = unwritten_negzero = wide = False
    for c in of("tab"):
        jx, jp = R.couplings(c, "exact")
        on.add((jx != 0.0, jp != 0.0))
        terms = _tab_terms(c)
        w = _written_rows(c, terms)
        h0 = R.h0_buffer(c.nhv)[:-1].reshape(c.qdw, c.pitch)
        col = np.arange(c.qdw) + c.dw0
        for il, io, jo in R._pairs(c.nlat, c.norb):
            q, r = (il * c.norb + io) * c.norb + jo, (il * c.norb + jo) * c.norb + io
            u = c.nd_up[r * c.dimup:(r + 1) * c.dimup].astype(np.int64)
            for coupling, e in ((jx, q), (jp, r)):
                if coupling == 0.0:
                    continue
                d = c.nd_dw[e * c.dimdw + col].astype(np.int64)
                ok = (u[None, :] != R.ND_INVALID) & (d[:, None] != R.ND_INVALID)
                for su in (0, 1):
                    for sd in (0, 1):
                        if (ok & ((u[None, :] >> 31) == su) & ((d[:, None] >> 31) == sd)).any():
                            signs.add((su, sd))
                dead_up |= bool(((u[None, :] == R.ND_INVALID) & (d[:, None] != R.ND_INVALID)).any())
        if c.dead_col >= 0 and c.qdw > 1:
            dead_col |= not w[c.dead_col].any() and w.any()
        live_cols = w.any(axis=1)
        unwritten_negzero |= bool((~w & (h0.real == 0) & np.signbit(h0.real))[live_cols, :c.dimup].any())
        wide |= c.pitch > c.dimup and c.qdw > 1 and w[1:].any()
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert on == {(True, False), (False, True), (True, True)}
    assert dead_col and dead_up and unwritten_negzero and wide
    assert any(c.qdw == 1 and c.dead_col == 0 and not _tab_terms(c).written.any() for c in of("tab"))


@pytest.mark.parametrize("kernel", ["kernel", "csr"])
def test_reach_grid_stride_trips(kernel):
    seen = set()
    for c in of(kernel):
        n, last, per = R.trips(c.gx, c.qdw * c.dimup)
        terms = prepared(kernel, c.name, "exact")[2]
        t_written = np.flatnonzero(terms.written)
        if last < per and t_written.size and int(t_written.max()) >= (n - 1) * per:      # a ragged last trip that writes something
            seen.add(n)
    assert {1, 2, 3} <= seen
    big = [c for c in of(kernel) if c.gx in R.GRIDS and c.qdw * c.dimup >= 2000]
    assert {c.gx for c in big} == set(R.GRIDS) and all(c.dw0 > 0 and c.dw0 + c.qdw <= c.dimdw for c in big)


def _negzero_at(c, idx):
    h = R.h0_buffer(c.nhv)[idx]
    return (h.real == 0) & np.signbit(h.real) & (h.imag == 0) & np.signbit(h.imag)


def test_reach_search():
    on, ns = set(), set()
    unwritten_negzero = False
    for c in of("kernel"):
        terms = prepared("kernel", c.name, "exact")[2]
        on.add(c.terms_on)
        ns.add(c.ns)
        unwritten_negzero |= bool(terms.written.any() and _negzero_at(c, terms.out[~terms.written]).any())
        if c.gx in R.GRIDS and c.qdw * c.dimup >= 2000:     # some source column lies outside the local slab
            used = set(np.unique(terms.vidx[terms.valid] // c.pitch).tolist())
            assert not used <= set(c.vcol[c.dw0:c.dw0 + c.qdw].tolist()), c.name
    assert on == {"x", "p", "xp"} and ns == {4, 5, 6, 8} and unwritten_negzero
    assert any(not prepared("kernel", c.name, "exact")[2].written.any() for c in of("kernel"))


def test_reach_csr():
    lengths = set()
    empty_negzero = outside = False
    for c in of("csr"):
        terms = prepared("csr", c.name, "exact")[2]
        lengths |= set(np.diff(c.rowptr).tolist())
        empty_negzero |= bool(_negzero_at(c, terms.out[~terms.written]).any())
        jdw = (c.cols.astype(np.int64) - 1) // c.dimup
        outside |= bool(((jdw < c.dw0) | (jdw >= c.dw0 + c.qdw)).any())
        assert np.iscomplexobj(c.vals) and (c.vals.real != 0).all() and (c.vals.imag != 0).all()
    assert lengths == {0, 1, 2, 3, 4} and empty_negzero and outside


# ---- the emulations, clean and with one mistake each ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kernel,c", CASES, ids=IDS)
def test_emulation_is_accepted(kernel, c, kind):
    _, coef, terms, v, h0 = prepared(kernel, c.name, kind)
    got = R.emulate(kernel, c, coef, v, h0)
    assert R.check(terms, v, h0, got, kind) == []
    assert R.bits(h0[-1:]).tolist() == R.bits(got[-1:]).tolist()


def refused(kernel, c, kind, bug):
    _, coef, terms, v, h0 = prepared(kernel, c.name, kind)
    try:
        got = R.emulate(kernel, c, coef, v, h0, bug)
    except IndexError:
        return "left its array"
    return "failed the check" if R.check(terms, v, h0, got, kind) else None


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("bug,kernel", [(b, k) for b, (ks, _) in R.MISTAKES.items() for k in ks])
def test_every_mistake_is_refused(bug, kernel, kind):
    caught = {}
    for c in of(kernel):
        how = refused(kernel, c, kind, bug)
        if how:
            caught[c.name] = how
        if how == "failed the check":
            break
    assert caught, f"{bug} ({R.MISTAKES[bug][1]}) in {kernel}: no case notices"
    if bug != "sign_in_index":      # (that one can only leave the array: bit 31 times the pitch is past any buffer)
        assert "failed the check" in caught.values(), f"{bug} in {kernel}: noticed only by leaving an array"


def test_the_listed_mistakes_are_the_ones_in_the_docstring():
    for bug, (kernels, _) in R.MISTAKES.items():
        line = next(ln for ln in __doc__.splitlines() if ln.strip().startswith(bug + " "))
        assert line.split()[1:1 + len(kernels)] == list(kernels), bug
    assert len(R.MISTAKES) == 15
