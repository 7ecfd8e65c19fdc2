"""The references of tests/chebyshev_ref.py without a GPU: the cases of tests/test_gpu_chebyshev_kernels.py reach every loop trip and every
template instantiation of csrc/hxv_chebyshev_kernels.hpp, the numpy emulation of the kernels passes the check the device results go
through, and the check refuses each named mistake."""
import numpy as np
import pytest

import chebyshev_ref as R


def test_cases_reach_every_trip_and_every_instantiation():
    steps, inits = R.step_cases(), R.init_cases()
    assert {(m, s, f) for _, _, m, s, f in steps} == {(m, s, f) for m in range(R.MAX_PROBES + 1) for s in (False, True) for f in (False, True)}
    assert {m for _, _, m, _ in inits} == set(range(R.MAX_PROBES + 1)) and {o for _, _, _, o in inits} == {False, True}
    for cases in (steps, [(n, g, m, o, False) for n, g, m, o in inits]):
        for g in R.GRIDS:
            mine = [(n, m, s, f) for n, gg, m, s, f in cases if gg == g and m in R.MS]
            for m in R.MS:
                for s in (False, True):
                    for f in {c[3] for c in mine}:
                        ns = {n for n, mm, ss, ff in mine if (mm, ss, ff) == (m, s, f)}
                        assert {1, 255, 256, 257} <= ns
                        # one, two, three and four trips, the last one ragged
                        assert {(R.trips(n, g), n % (256 * g) != 0) for n in ns} >= {(1, True), (2, True), (3, True), (4, True)}
    assert max(n for n, *_ in steps) == 2309  # (the integer cases' exactness argument is made for this size)


def _some_cases(integer):
    seed = 0
    for n, g, m, s, f in R.step_cases():
        seed += 1
        if m in (0, 3, 8) or n == 257:
            yield R.make_step(seed, n, g, m, s, f, integer)
    for n, g, m, o in R.init_cases():
        seed += 1
        if m in (0, 3) or n == 257:
            yield R.make_init(seed, n, g, m, o, integer)


@pytest.mark.parametrize("integer", [True, False], ids=["integers", "normal"])
def test_emulation_is_accepted(integer):
    count = 0
    for case in _some_cases(integer):
        assert R.check(case, R.emulate(case)) == [], (case["kind"], case["n"], case["grid"], case["m"], case["with_sum"], case["first"])
        count += 1
    assert count > 300


@pytest.mark.parametrize("integer", [True, False], ids=["integers", "normal"])
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_named_mistakes_are_refused(mistake, integer):
    """the wrong buffer overwritten, b with the wrong sign, the conjugate on the wrong side of an overlap, the running sum one order late, the
    ragged tail dropped: each on a general step with a running sum and three probes, on two blocks with a ragged third trip"""
    case = R.make_step(77, 2 * 256 * 2 + 5, 2, 3, True, False, integer)
    assert case["cc"] != 0.0 and case["ci"] != 0.0
    assert R.check(case, R.emulate(case)) == []
    assert R.check(case, R.emulate(case, mistake)) != [], mistake


def test_the_first_step_does_not_read_its_destination_and_step_zero_does_not_read_out():
    """what the NaN prefill shows: a read of the first form's destination, or of step 0's out, is refused"""
    case = R.make_step(5, 257, 2, 1, False, True, False)
    mem, partial, sums = R.emulate(case)
    mem[R.PREV, :257] += case["mem"][R.PREV, :257]  # as if t_prev had been read
    assert R.check(case, (mem, partial, sums)) != []
    case = R.make_init(6, 257, 2, 1, True, False)
    mem, partial, sums = R.emulate(case)
    mem[R.OUT, :257] += case["mem"][R.OUT, :257]
    assert R.check(case, (mem, partial, sums)) != []


def test_a_write_behind_n_or_beyond_the_grid_is_refused():
    case = R.make_step(9, 255, 1, 0, True, False, True)
    mem, partial, sums = R.emulate(case)
    assert R.check(case, (mem, partial, sums)) == []
    for where in ("gap", "row", "entry"):
        m2, p2, s2 = mem.copy(), partial.copy(), sums.copy()
        if where == "gap":
            m2[R.PREV, 255] = 0.0
        elif where == "row":
            p2[1, 0] = 0.0
        else:
            s2[-1] = 0.0
        assert R.check(case, (m2, p2, s2)) != [], where


def test_pad_zeros_come_out_as_plus_zero():
    """zero inputs give +0.0 in the emulation whatever the signs of the scalars, so the bit-for-bit comparison holds the device to it"""
    case = R.make_step(3, 8, 1, 1, True, False, True)
    case["mem"][:, :8] = 0.0
    for cc, cr, ci in ((1.0, -1.0, 1.0), (-2.0, 1.0, -1.0)):
        case.update(cc=cc, cr=cr, ci=ci)
        mem, _, _ = R.emulate(case)
        for s in (R.PREV, R.OUT):
            assert R.same_bits(mem[s, :8], np.zeros(8, dtype=np.complex128))
