"""The references of tests/chebyshev_real_ref.py without a GPU: the numpy emulation of the real-vector Chebyshev kernels passes the check the
device results go through (tests/test_gpu_chebyshev_real_kernels.py), the check refuses each named mistake, and the formula of
hxv_vector_random (include/hxv.h), restated in numpy uint64, gives independent vectors for different seeds -- which the index formula of the
engine's Lanczos start vector does not."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import chebyshev_real_ref as R


def test_cases_reach_every_instantiation_and_the_sums_are_m_plus_two():
    steps, inits = R.step_cases(), R.init_cases()
    assert {(m, s, f) for _, _, m, s, f in steps} == {(m, s, f) for m in range(R.MAX_PROBES + 1) for s in (False, True) for f in (False, True)}
    assert {m for _, _, m, _ in inits} == set(range(R.MAX_PROBES + 1))
    assert [R.nsums(m) for m in (0, 1, 8)] == [2, 3, 10]
    assert R.re_accumulators(2) == [0, 2, 4, 5]


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
    """a sum over one component only, the ragged tail dropped, the first form reading its destination, the coefficient of the running sum on
    one component only, an Im-style term in a probe sum: each on a step with a running sum and three probes, on two blocks with a ragged
    third trip (the first-step form for the mistake that belongs to it)"""
    case = R.make_step(77, 2 * 256 * 2 + 5, 2, 3, True, mistake == "first_reads_prev", integer)
    assert case["cr"] != 1.0 and case["cc"] != 0.0
    assert R.check(case, R.emulate(case)) == []
    assert R.check(case, R.emulate(case, mistake)) != [], mistake


def test_a_result_with_the_complex_kernels_shape_is_refused():
    case = R.make_step(4, 257, 2, 1, False, False, True)
    mem, _, _ = R.emulate(case)
    import chebyshev_ref as C

    p, s = C.fresh_outputs(case)
    assert R.check(case, (mem, p, s)) != []


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
    case = R.make_step(3, 8, 1, 1, True, False, True)
    case["mem"][:, :8] = 0.0
    for cc, cr in ((1.0, -1.0), (-2.0, 1.0)):
        case.update(cc=cc, cr=cr)
        mem, _, _ = R.emulate(case)
        for s in (R.PREV, R.OUT):
            assert R.same_bits(mem[s, :8], np.zeros(8, dtype=np.complex128))


# ---- hxv_vector_random ------------------------------------------------------------------------------------------------------------------
SIZES = (300, 400, 48048)
OFFSETS = (1, 2, 3, 1000)


def test_mix_is_splitmix64():
    """the first outputs of splitmix64 from state 0 (Vigna's reference generator: state += golden, output = finaliser(state)) are
    mix(0), mix(golden), mix(2 golden): published values"""
    g = 0x9E3779B97F4A7C15
    got = [int(R.mix(np.uint64((k * g) & 0xFFFFFFFFFFFFFFFF))[0]) for k in range(3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_random_vector_values_and_layout():
    v = R.random_vector(5, 1000)
    assert v.dtype == np.complex128 and np.all(v.imag == 0.0) and not np.any(np.signbit(v.imag))
    assert v.real.min() >= -0.5 and v.real.max() < 0.5 and abs(v.real.mean()) < 5 * np.sqrt(1 / 12 / 1000)
    assert abs(np.vdot(v, v).real / 1000 - 1 / 12) < 0.01
    z = R.random_vector(5, 1000, complex_valued=True)
    assert np.array_equal(z.real, v.real) and R.overlap(z.real, z.imag) < 5 / np.sqrt(1000)
    assert np.array_equal(R.random_vector(5, 100, first=700), v[700:800])            # a slab is a window of the global vector


def test_different_seeds_give_independent_vectors():
    """the condition of the typical-state methods: for seeds 0..39 the normalised overlap with the vectors of seed + 1, + 2, + 3, + 1000 and with
    the one-element shift of seed + 2 stays below 5/sqrt(n), real and complex"""
    worst = 0.0
    for n in SIZES:
        cache = {}

        def vec(s, cv):
            if (s, cv) not in cache:
                cache[(s, cv)] = R.random_vector(s, n, cv)
            return cache[(s, cv)]

        for cv in (False, True):
            for s in range(40):
                a = vec(s, cv)
                for d in OFFSETS:
                    o = R.overlap(a, vec(s + d, cv))
                    worst = max(worst, o * np.sqrt(n))
                    assert o <= 5 / np.sqrt(n), (n, s, d, cv, o)
                o = R.overlap(a[1:], vec(s + 2, cv)[:-1])
                worst = max(worst, o * np.sqrt(n))
                assert o <= 5 / np.sqrt(n), (n, s, "shift", cv, o)
    print(f"largest normalised overlap: {worst:.2f}/sqrt(n)")


def test_the_lanczos_start_vector_fails_that_condition():
    """what the key is for: with the index formula 2 I + seed of lz_init, seed + 2 is seed shifted by one element"""
    a, b = R.lanczos_start_real(0, 400), R.lanczos_start_real(2, 400)
    assert np.array_equal(a[1:], b[:-1]) and R.overlap(a[1:], b[:-1]) > 5 / np.sqrt(400)


def test_the_library_exports_and_lists_the_new_entries():
    import hxv

    lib = ctypes.CDLL(str(hxv.LIB_PATH))
    hdr = (Path(__file__).resolve().parents[1] / "include" / "hxv.h").read_text()
    for name in ("hxv_chebyshev_moments_real", "hxv_chebyshev_apply_real", "hxv_vector_random"):
        assert name in hxv.EXPORTS and hasattr(lib, name) and f"int {name}(" in hdr
    for name in ("chebyshev_moments_real", "chebyshev_apply_real", "random_vector"):
        assert hasattr(hxv.HxvSector, name)
    from hxv import chebyshev as ch

    assert callable(ch.thermal_state)
    L = hxv.load_library()
    assert L.hxv_chebyshev_moments_real(None, None, 0, None, 1, 1.0, 0.0, None, None) == 1 and b"hxv_chebyshev_moments_real" in L.hxv_last_error()
    assert L.hxv_chebyshev_apply_real(None, None, 1, None, 1.0, 0.0, None, None) == 1 and b"hxv_chebyshev_apply_real" in L.hxv_last_error()
    assert L.hxv_vector_random(None, 0, 0, None) == 1 and b"hxv_vector_random" in L.hxv_last_error()
