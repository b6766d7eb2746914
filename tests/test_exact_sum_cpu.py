"""csrc/exact_sum.h on the host: the one rule for the scale of an exact sum against its spec
(oracle.gen_ps_oracle.fixed_point_shift), the one conversion and the one mean against their NumPy expressions, all
exactly.  tests/test_exact_sum_gpu.py holds the device's build of the same functions against this one."""
import numpy as np
import pytest

import exact_sum_cases as X
from oracle import gen_ps_oracle as O


@pytest.fixture(scope="module")
def host():
    return X.evaluate(None)


def test_the_shift_equals_the_oracles_for_every_magnitude_and_count(host):
    a, n = X.shift_inputs()
    assert len(a) == len(X.SHIFT_ABSMAX) * len(X.SHIFT_N) + 3
    want = np.array([O.fixed_point_shift(float(x), int(m)) for x, m in zip(a, n)], np.int32)
    np.testing.assert_array_equal(host[0], want)
    assert [int(v) for v in host[0][-3:]] == [k[2] for k in X.SHIFT_KNOWN] == [50, 210, -976]
    zero = ~(a > 0) | ~np.isfinite(a)  # +-0, inf, NaN
    assert zero.sum() == 4 * len(X.SHIFT_N) and not host[0][zero].any() and host[0][~zero].all()
    assert host[0].min() >= -1000 and host[0].max() == 1000  # the double subnormal meets the clamp


def test_the_rule_keeps_n_terms_within_2_to_the_61(host):
    """x 2^k < 2^(61 - ceil log2 n) before rounding, so the rounded term reaches that power of two at most and n of
    them 2^61: two bits below the int64 range (the callers' lists hold up to 4 N entries)."""
    a, n = X.shift_inputs()
    for x, m, k in zip(a, n, host[0]):
        if x > 0 and np.isfinite(x) and abs(int(k)) < 1000:
            assert int(np.rint(np.ldexp(x, int(k)))) * int(m) <= 1 << 61, (x, m, k)


def test_to_fixed_rounds_to_nearest_even(host):
    x, k = X.fixed_inputs()
    want = np.rint(np.ldexp(x, k)).astype(np.int64)
    np.testing.assert_array_equal(host[1], want)
    assert np.abs(want).max() == (1 << 61) - (1 << 8)  # the largest double below 1 at k = 61
    ties = np.ldexp(np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5]), -10)
    got = {float(t): int(host[1][np.nonzero((x == t) & (k == 10))[0][0]]) for t in ties}
    assert list(got.values()) == [0, 2, 2, 4, 0, -2, -2]


def test_fixed_mean_is_one_float64_division(host):
    s, k, c = X.mean_inputs()
    want = np.ldexp(s.astype(np.float64), -k) / c
    np.testing.assert_array_equal(host[2], want)
    assert np.isfinite(want).all() and (want != 0).sum() == (s != 0).sum()
