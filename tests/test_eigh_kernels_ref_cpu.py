"""The comparison helpers of tests/eigh_kernels_ref.py bite (no GPU, no kernel).

Each helper that tests/test_gpu_eigh_kernels.py uses is given (a) its own reference, rounded to double, as the "result" and must accept it;
(b) the reference of the same operation with ONE element left out (the lost tail of a grid-stride loop, an unwritten component) and
(c) with TWO basis slots exchanged (a confused stride or index table), and must refuse both.  So the tolerances, which are computed from
the inputs alone, are tight enough to see the smallest mistakes the GPU tests are there for."""
import numpy as np
import pytest

import eigh_kernels_ref as R

N, GRID = 257, 1      # two loop rounds with a ragged second one: the deepest chain (the widest bound) among the small GPU shapes


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20240607)
    return dict(V=R.random_complex(rng, (8, N)), w=R.random_complex(rng, N), S=R.random_reals(rng, (8, 8)), coef=R.random_reals(rng, 16),
                part=R.random_reals(rng, (257, 16)))


def _refuses(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63
    assert float(R.gamma(1)) == pytest.approx(2.0 ** -53, rel=1e-12)
    assert R.chain_depth(1000, 2) == 2 * 2 + 9 and R.chain_depth(1000, 2, 2) == 2 * 2 + 9 + 1 + 8 and R.chain_depth(None, 1, 257) == 2 + 8
    assert R.chain_depth(0, 3) == 9


def test_check_sum_on_dots(data):
    V, w = data["V"], data["w"]
    ref, ab = R.dots(V, w)
    d = R.chain_depth(N, GRID, GRID)
    R.check_sum(ref.astype(np.float64), ref, ab, d, "dots")
    dropped, _ = R.dots(V[:, :-1], w[:-1])
    _refuses(R.check_sum, dropped.astype(np.float64), ref, ab, d, "dots, last element lost")
    one, _ = R.dots(np.delete(V, 100, axis=1), np.delete(w, 100))
    _refuses(R.check_sum, one.astype(np.float64), ref, ab, d, "dots, element 100 lost")
    swapped, _ = R.dots(V[[0, 1, 5, 3, 4, 2, 6, 7]], w)
    _refuses(R.check_sum, swapped.astype(np.float64), ref, ab, d, "dots, slots 2 and 5 exchanged")
    nan = ref.astype(np.float64)
    nan[3, 1] = np.nan
    _refuses(R.check_sum, nan, ref, ab, d, "dots, one NaN")


def test_check_sum_on_norm(data):
    w = data["w"]
    ref, ab = R.norm2(w)
    d = R.chain_depth(N, GRID, GRID)
    R.check_sum(np.float64(ref), ref, ab, d, "norm")
    for i in (0, 100, N - 1):
        lost, _ = R.norm2(np.delete(w, i))
        _refuses(R.check_sum, np.float64(lost), ref, ab, d, f"norm, element {i} lost")


def test_check_sum_on_colsum(data):
    p = data["part"]
    for zero_odd in (0, 1):
        ref, ab = R.colsum(p, 16, zero_odd)
        d = R.chain_depth(None, 1, p.shape[0])
        R.check_sum(ref.astype(np.float64), ref, ab, d, "colsum")
        if zero_odd:
            assert np.all(ref[1::2] == 0) and np.all(ab[1::2] == 0)
        lost, _ = R.colsum(p[:-1], 16, zero_odd)
        _refuses(R.check_sum, lost.astype(np.float64), ref, ab, d, "colsum, last block lost")
        q = p.copy()
        q[:, [2, 4]] = q[:, [4, 2]]
        swapped, _ = R.colsum(q, 16, zero_odd)
        _refuses(R.check_sum, swapped.astype(np.float64), ref, ab, d, "colsum, columns 2 and 4 exchanged")
    # with zero_odd the tolerance of an odd output is zero: anything but 0.0 is refused
    ref, ab = R.colsum(p, 16, 1)
    got = ref.astype(np.float64)
    got[3] = 5e-324
    _refuses(R.check_sum, got, ref, ab, R.chain_depth(None, 1, p.shape[0]), "colsum, odd output not zero")


def test_check_elementwise_on_maxpy(data):
    V, w, coef = data["V"], data["w"], data["coef"]
    idx = [7, 0, 3, 5]
    ref, bound = R.maxpy(V, idx, coef[:8], w)
    R.check_elementwise(R.to_complex(ref), ref, bound, "maxpy")
    lost, _ = R.maxpy(V, idx[:3], coef[:6], w)
    _refuses(R.check_elementwise, R.to_complex(lost), ref, bound, "maxpy, last vector lost")
    one = R.to_complex(ref)
    one[100] = w[100]
    _refuses(R.check_elementwise, one, ref, bound, "maxpy, element 100 not written")
    swapped, _ = R.maxpy(V, [7, 3, 0, 5], coef[:8], w)
    _refuses(R.check_elementwise, R.to_complex(swapped), ref, bound, "maxpy, two index entries exchanged")
    conj, _ = R.maxpy(V, idx, coef[:8] * np.tile([1.0, -1.0], 4), w)
    _refuses(R.check_elementwise, R.to_complex(conj), ref, bound, "maxpy, coefficients conjugated")


def test_check_elementwise_on_scale(data):
    w = data["w"]
    r = 1.0 / 3.7
    ref, bound = R.scale(w, r)
    R.check_elementwise(R.to_complex(ref), ref, bound, "scale")
    R.check_elementwise(w * r, ref, bound, "scale, correctly rounded products")
    one = w * r
    one[N - 1] = w[N - 1]
    _refuses(R.check_elementwise, one, ref, bound, "scale, last element not scaled")
    ulp = w * r
    ulp[5] = np.nextafter(ulp[5].real, np.inf) + 1j * ulp[5].imag
    ulp[5] = np.nextafter(ulp[5].real, np.inf) + 1j * ulp[5].imag
    _refuses(R.check_elementwise, ulp, ref, bound, "scale, one component two ulps off")


def test_check_elementwise_on_rotate(data):
    V, S = data["V"], data["S"]
    ref, bound = R.rotate(V, S, 5)
    R.check_elementwise(R.to_complex(ref), ref, bound, "rotate")
    lost, _ = R.rotate(V[:7], S[:7], 5)
    _refuses(R.check_elementwise, R.to_complex(lost), ref, bound, "rotate, last basis vector lost")
    swapped, _ = R.rotate(V[[0, 6, 2, 3, 4, 5, 1, 7]], S, 5)
    _refuses(R.check_elementwise, R.to_complex(swapped), ref, bound, "rotate, slots 1 and 6 exchanged")
    tr, _ = R.rotate(V, S.T, 5)
    _refuses(R.check_elementwise, R.to_complex(tr), ref, bound, "rotate, S transposed")


def test_check_elementwise_on_axpy(data):
    V, w, coef = data["V"], data["w"], data["coef"][:8].copy()
    coef[[2, 7]] = 0.0
    ref, bound = R.axpy(V, coef, 0.37, w)
    R.check_elementwise(R.to_complex(ref), ref, bound, "axpy")
    lost, _ = R.axpy(V[:6], coef[:6], 0.37, w)      # (vector 7 has a zero coefficient: dropping it alone changes nothing)
    _refuses(R.check_elementwise, R.to_complex(lost), ref, bound, "axpy, vector 6 lost")
    R.check_elementwise(R.to_complex(R.axpy(V[:7], coef[:7], 0.37, w)[0]), ref, bound, "axpy, a measured-only vector left out")
    swapped, _ = R.axpy(V[[0, 4, 2, 3, 1, 5, 6, 7]], coef, 0.37, w)
    _refuses(R.check_elementwise, R.to_complex(swapped), ref, bound, "axpy, slots 1 and 4 exchanged")
    noa, _ = R.axpy(V, coef, 1.0, w)
    _refuses(R.check_elementwise, R.to_complex(noa), ref, bound, "axpy, a ignored")
