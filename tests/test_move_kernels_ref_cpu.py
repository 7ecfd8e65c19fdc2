"""The cases of tests/move_kernels_ref.py are safe to launch, reach the paths they are there for, and its checks bite (no GPU, no kernel).

SAFE.  Every restatement forms its indices through bounds-checked lookups into the buffers `*_inputs` allocates, the very buffers
tests/test_gpu_move_kernels.py uploads: running every case here shows that no table of any case points outside them.  What a launch adds
-- the launcher's own rules (a pitch is a multiple of 8 and not below its dimension, ...) and the grids that index without a guard -- is
asserted from the case beside it.

REACH.  Computed from the case lists: the second and third loop trips, the owners, the slot kinds and the range edges that no sector offers.

BITE.  One named mistake at a time is switched on in the restatement; the comparison of bits the GPU file makes must refuse it on at least
one case."""
import numpy as np
import pytest

import move_kernels_ref as R


def pitch_ok(pitch, dim):
    return dim >= 1 and pitch >= dim and pitch % 8 == 0


# ---- what each family runs: (case, inputs, reference(bug) -> tuple of buffers) -----------------------------------------------------------------
def runs(kind):
    if kind == "transpose":
        for c in R.transpose_cases():
            a = R.transpose_inputs(c)
            yield c, lambda bug=None, c=c, a=a: (R.transpose_ref(c, a, bug),)
    elif kind == "pack":
        for c in R.pack_cases():
            a = R.pack_inputs(c)
            yield c, lambda bug=None, c=c, a=a: R.pack_ref(c, a, bug)
    elif kind == "unpack":
        for c in R.unpack_cases():
            a = R.unpack_inputs(c)
            yield c, lambda bug=None, c=c, a=a: (R.unpack_ref(c, a, bug),)
    elif kind == "ladder":
        for c in R.ladder_cases():
            for mode, (coef, acc, integer) in R.LADDER_MODES.items():
                psi, out0 = R.ladder_inputs(c, integer)
                yield c, lambda bug=None, c=c, psi=psi, out0=out0, coef=coef, acc=acc: (R.ladder_ref(c, psi, out0, coef, acc, bug),)
    elif kind == "ladder_cols":
        for c in R.ladder_cols_cases():
            pl, rv, out0 = R.ladder_cols_inputs(c)
            yield c, lambda bug=None, c=c, pl=pl, rv=rv, out0=out0: (R.ladder_cols_ref(c, pl, rv, out0, bug),)
    elif kind == "pack_columns":
        for c in R.pack_columns_cases():
            a = R.pack_columns_inputs(c)
            yield c, lambda bug=None, c=c, a=a: (R.pack_columns_ref(c, a, bug),)
    elif kind == "add_pieces":
        for c in R.add_pieces_cases():
            hv, pieces = R.add_pieces_inputs(c)
            yield c, lambda bug=None, c=c, hv=hv, pieces=pieces: (R.add_pieces_ref(c, hv, pieces, bug),)
    elif kind == "rows":
        for c in R.rows_cases():
            ref, dev = R.rows_inputs(c)
            yield c, lambda bug=None, c=c, ref=ref, dev=dev: (R.rows_ref_to_dev_ref(c, ref, bug), R.rows_dev_to_ref_ref(c, dev, bug))
    else:
        raise KeyError(kind)


KINDS = ["transpose", "pack", "unpack", "ladder", "ladder_cols", "pack_columns", "add_pieces", "rows"]


# ---- SAFE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_case_stays_inside_its_buffers(kind):
    n = 0
    for c, ref in runs(kind):
        outs = ref()                    # raises IndexError at the first index outside a buffer
        for o in outs:
            assert R.same_bits(o[-1:], np.array([R.SENT.real if o.dtype == np.float64 else R.SENT], dtype=o.dtype)), (c.name, "the guard")
        n += 1
    assert n > 0


def test_launch_arguments_obey_the_launchers_rules():
    for c in R.transpose_cases():
        assert pitch_ok(c.pitch_a, c.dimup_a) and pitch_ok(c.pitch_b, c.dimup_b) and R.transpose_trips(c)["covers"], c.name
        assert 1 <= c.gx <= 65535 and 1 <= c.gy <= 65535
    for c in R.pack_cases():
        assert pitch_ok(c.pitch_a, c.dimup_a) and pitch_ok(c.stride, c.qa) and 0 <= c.own_lo <= c.own_hi <= c.dimup_a, c.name
        assert R.pack_trips(c)["covers"] and 1 <= c.gy <= 65535, c.name
    for c in R.unpack_cases():
        assert pitch_ok(c.pitch_b, c.dimup_b) and c.qb >= 1 and R.unpack_trips(c)["covers"] and 1 <= c.gy <= 65535, c.name
        q = np.diff(c.first)
        assert c.first[0] == 0 and c.first[-1] == c.dimup_b and (q >= 0).all() and (c.stride >= q).all(), c.name
        assert len(c.tab()) == 3 * c.nranks + 2
        ends = c.off[:-1] + c.qb * c.stride
        assert (ends <= c.off[1:]).all(), (c.name, "blocks overlap")
    for c in R.ladder_cases():
        assert pitch_ok(c.pitch_to, c.dimup_to) and pitch_ok(c.pitch_from, c.dim_from if c.spin == 0 else c.dimup_to), c.name
        assert (np.diff(c.map_from.astype(np.int64)) > 0).all() and 0 <= c.orbital < c.ns and c.pitch_from != c.pitch_to, c.name
        assert len(c.map_to) == (c.dimup_to if c.spin == 0 else c.dimdw_to) and c.psi_cols == (c.dimdw_to if c.spin == 0 else c.dim_from), c.name
        if c.ofrom is not None:
            assert sorted(c.ofrom.perm) == list(range(c.dim_from)) and len(c.ofrom.sign) == c.dim_from and len(c.sign_to) == c.dimup_to
    for c in R.ladder_cols_cases():
        assert pitch_ok(c.pitch_from, c.dimup) and pitch_ok(c.pitch_to, c.dimup) and c.pitch_from != c.pitch_to and R.ladder_cols_trips(c)["covers"], c.name
        live = c.sign != 0
        assert ((c.slot[live] < c.nlocal) & (-1 - c.slot[live] < c.nrecv)).all() and set(c.sign) == {-1, 0, 1}, c.name
    for c in R.pack_columns_cases():
        assert pitch_ok(c.pitch, 1) and ((0 <= c.cols) & (c.cols < c.nsrc)).all() and len(set(c.cols)) < len(c.cols), c.name
        assert list(c.cols) != sorted(c.cols)
    for c in R.add_pieces_cases():
        assert pitch_ok(c.pitch, c.dimup) and c.ncols >= 1 and c.nwtr >= 1 and 1 <= c.gx <= 65535 and 1 <= c.gy <= 65535, c.name
        # the ranges tile [0, dimup) in order; every buffer has room for its stride
        assert c.row0[0] == 0 and c.row1[-1] == c.dimup and (c.row0[1:] == c.row1[:-1]).all() and (c.stride > c.row1 - c.row0).all(), c.name
    for c in R.rows_cases():
        assert pitch_ok(c.pitch, c.dimup) and sorted(c.order.iperm) == list(range(c.dimup)), c.name
        assert (c.order.perm[c.order.iperm] == np.arange(c.dimup)).all()


# ---- REACH -----------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_no_sector_offers():
    pk = [R.pack_trips(c) for c in R.pack_cases()]
    assert any(t["c0_trips"] >= 3 for t in pk) and any(t["c0_trips"] >= 2 and t["ragged"] for t in pk)
    kinds = {c.name.split("-own-")[1].rsplit("-gy", 1)[0] for c in R.pack_cases()}
    assert kinds == {"empty-low", "whole", "middle", "to-tile-edge", "from-tile-edge"}
    assert any(c.stride > R.roundup8(c.qa) for c in R.pack_cases()) and any(c.oa is None for c in R.pack_cases())

    up = R.unpack_cases()
    assert any(R.unpack_trips(c)["kb_trips"] >= 3 and R.unpack_trips(c)["ragged"] for c in up)
    assert any(R.unpack_trips(c)["past_pitch"] and c.gx >= 2 for c in up)
    for p in (2, 3, 4, 8):
        owners, at_first, at_last, single = set(), False, False, False
        for c in (c for c in up if c.nranks == p):
            idw = R._ip(c.ob, c.dimup_b)
            o = R.owner_of(c.first, idw)
            owners |= set(int(x) for x in o)
            q = np.diff(c.first)
            at_first |= bool(np.isin(idw, c.first[:-1][q > 0]).any())
            at_last |= bool(np.isin(idw, (c.first[1:] - 1)[q > 0]).any())
            single |= bool((q == 1).any())
            assert len(set(int(s) for s in c.stride)) > 1, c.name
        assert owners == set(range(p)) and at_first and at_last and single, p

    tr = R.transpose_cases()
    assert any(c.pitch_b > R.roundup8(c.dimup_b) for c in tr) and any(c.gx * R.TW >= c.dimup_a + R.TW for c in tr)
    assert {(c.oa is None, c.ob is None) for c in tr} == {(True, True), (True, False), (False, True), (False, False)}

    def three_ragged(trips):
        return any(t["rounds"] >= 3 and t["ragged"] for t in trips)

    ld = R.ladder_cases()
    assert three_ragged([R.ladder_trips(c) for c in ld if c.n > 768 and c.gx == 1])
    assert {c.gx for c in ld if c.n > 768} >= {1, 2, 3}
    assert {(c.spin, c.create) for c in ld} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.spin == 0 and c.ofrom is not None and c.sign_to is not None for c in ld) and any(c.spin == 0 and c.ofrom is None for c in ld)
    assert all(c.dimdw_to < len(R.basis(c.ns, bin(int(c.map_to[0])).count("1"))) for c in ld if c.spin == 1 and c.ns > 4)
    assert three_ragged([R.ladder_cols_trips(c) for c in R.ladder_cols_cases()])
    assert all(t["local"] and t["received"] and t["unreached"] for t in (R.ladder_cols_trips(c) for c in R.ladder_cols_cases()))
    assert three_ragged([R.pack_columns_trips(c) for c in R.pack_columns_cases()])
    for real in (False, True):
        ap = [c for c in R.add_pieces_cases() if c.real == real]
        assert three_ragged([R.add_pieces_trips(c) for c in ap])
        assert any(R.add_pieces_trips(c)["empty_in_the_middle"] for c in ap) and {c.nwtr for c in ap} == {1, 2, 4, 8}
        assert any(R.add_pieces_trips(c)["col_trips"] >= 3 and R.add_pieces_trips(c)["col_ragged"] for c in ap)     # the column loop
        for c in ap:        # a row at every row0 and at every row1 - 1 of the ranges that hold rows
            live = c.row1 > c.row0
            assert ((c.row0[live] >= 0) & (c.row1[live] - 1 < c.dimup)).all()
    # more columns than a grid holds along y, at the largest y extent: the column loop's second trip is the only way to the columns past it
    wide = [c for c in R.add_pieces_cases() if c.ncols > 65535]
    assert wide and all(c.gy == 65535 and c.dimup == 1 and R.add_pieces_trips(c)["col_trips"] == 2 and R.add_pieces_trips(c)["col_ragged"] for c in wide)
    for to_dev in (True, False):
        assert three_ragged([R.rows_trips(c, to_dev) for c in R.rows_cases()])


# ---- BITE ------------------------------------------------------------------------------------------------------------------------------------
def verdicts(kind, bug):
    """per case: 'same' / 'differs' / 'outside' (the mistake forms an index outside a buffer: on the device a fault, not a comparison)"""
    out = []
    for c, ref in runs(kind):
        good = ref()
        try:
            bad = ref(bug)
        except IndexError:
            out.append("outside")
            continue
        out.append("same" if all(R.same_bits(g, b) for g, b in zip(good, bad)) else "differs")
    return out


@pytest.mark.parametrize("bug", sorted(R.MISTAKES))
def test_the_comparison_refuses_the_mistake(bug):
    v = verdicts(R.MISTAKES[bug], bug)
    assert "differs" in v, (bug, {k: v.count(k) for k in set(v)})


@pytest.mark.parametrize("bug,kind", [("sign_a_dropped", "pack"), ("perm_for_iperm", "pack"), ("sign_b_dropped", "unpack"), ("perm_for_iperm", "unpack"),
                                      ("perm_for_iperm", "rows")])
def test_the_row_order_mistakes_are_refused_in_the_other_kernels_too(bug, kind):
    assert "differs" in verdicts(kind, bug)


@pytest.mark.parametrize("bug", sorted(R.IDENTITIES))
def test_what_is_no_mistake_changes_no_bits(bug):
    assert set(verdicts(R.IDENTITIES[bug], bug)) == {"same"}


def test_the_chain_shapes_are_not_binomial_and_split_unevenly():
    for da, dw, p in R.CHAIN_SHAPES:
        assert p <= min(da, dw)
        fa, fb = R.dw_split(dw, p), R.dw_split(da, p)
        assert fa[-1] == dw and fb[-1] == da and (np.diff(fa) >= 1).all() and (np.diff(fb) >= 1).all()
    assert any(len(set(np.diff(R.dw_split(dw, p)))) > 1 for da, dw, p in R.CHAIN_SHAPES)
