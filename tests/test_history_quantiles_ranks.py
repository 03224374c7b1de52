"""The Python side of the ring quantiles without a device: ranks to exact rationals over one denominator
(HipExec.quantile_ranks) and the raw [s, period, 1 + 2Q, w] blocks to the result dict (HipExec._quantile_dict)."""
from fractions import Fraction

import numpy as np
import pytest

from elodin_amd import _lib as L
from elodin_amd.exec import HipExec


def test_floats_are_read_through_their_decimal_repr():
    assert HipExec.quantile_ranks([0.99]) == ([99], 100)              # not 0x1.fae147ae147aep-1
    assert HipExec.quantile_ranks([0.01, 0.25, 0.5, 0.75, 0.99]) == ([1, 25, 50, 75, 99], 100)
    assert HipExec.quantile_ranks([0.0, 1.0, 0.5]) == ([0, 2, 1], 2)
    assert HipExec.quantile_ranks(0.5) == ([1], 2)
    assert HipExec.quantile_ranks([np.float64(0.1), 1e-3]) == ([100, 1], 1000)


def test_fractions_pairs_and_floats_share_one_denominator():
    num, den = HipExec.quantile_ranks([Fraction(1, 3), (1, 4), 0.5, (2, 6), 0, 1])
    assert den == 12 and num == [4, 3, 6, 4, 0, 12]                   # duplicates and any order stay as given
    assert HipExec.quantile_ranks([(k, 299) for k in range(16)]) == (list(range(16)), 299)
    assert HipExec.quantile_ranks([(0, 1), (1, 1)]) == ([0, 1], 1)
    assert HipExec.quantile_ranks([Fraction(1, 2 ** 32 - 1)]) == ([1], 2 ** 32 - 1)


@pytest.mark.parametrize("q", [
    [1.5], [-0.25], [(3, 2)], [Fraction(-1, 7)], [float("nan")], [float("inf")], [(1, 0)],      # outside [0, 1] or no number
    [], [k / 32 for k in range(17)],                                                            # none, more than 16
    [(1, 2 ** 32)], [Fraction(1, 2 ** 32 + 1)], [(1, 65537), (1, 65539)],                       # denominators beyond 32 bits
])
def test_refused_ranks(q):
    with pytest.raises(ValueError):
        HipExec.quantile_ranks(q)
    assert L.QUANTILE_MAX_RANKS == 16 and L.QUANTILE_ASYNC == 1


def test_result_dict_shapes_and_the_linear_formula():
    s, period, w = 2, 3, 7
    num, den = [1, 1, 3], 4
    rng = np.random.default_rng(5)
    raw = np.empty((s, period, 1 + 2 * 3, w))
    raw[:, :, 0] = rng.integers(1, 50, (s, period, w))
    raw[:, :, 1::2] = rng.normal(size=(s, period, 3, w))
    raw[:, :, 2::2] = raw[:, :, 1::2] + rng.uniform(0, 1, (s, period, 3, w))
    raw[0, 1, 0, 2], raw[0, 1, 1:, 2] = 0, np.nan                      # an element without a finite row
    d = HipExec._quantile_dict(["x"], [raw], num, den)["x"]
    assert sorted(d) == ["count", "linear", "lower", "upper"]
    assert d["count"].dtype == np.int64 and d["count"].shape == (s, period, w)
    for k in ("lower", "upper", "linear"):
        assert d[k].dtype == np.float64 and d[k].shape == (s, period, 3, w), k
    assert np.array_equal(d["lower"], raw[:, :, 1::2], equal_nan=True) and np.array_equal(d["upper"], raw[:, :, 2::2], equal_nan=True)
    for j in range(s):
        for g in range(period):
            for i in range(3):
                for c in range(w):
                    m = int(d["count"][j, g, c])
                    if m == 0:
                        assert np.isnan(d["linear"][j, g, i, c])
                        continue
                    frac = float(num[i] * (m - 1) % den) / float(den)
                    lo, hi = d["lower"][j, g, i, c], d["upper"][j, g, i, c]
                    assert d["linear"][j, g, i, c] == lo + (hi - lo) * frac
    some = d["count"][:, :, None, :].repeat(3, axis=2) > 0
    assert np.all(d["linear"][some] >= d["lower"][some]) and np.all(d["linear"][some] <= d["upper"][some])
