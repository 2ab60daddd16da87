"""languagedetection.topk.rank -- the order behind SCORE's top-k output, checked
on the CPU: entry 0 is breeze's first-maximum argmax (ldoracle.argmax_first),
the result a permutation prefix, and the NaN / signed-zero / tie rules as
include/ldgpu.h states them."""
import math
import random

import pytest

import ldoracle as O
from languagedetection import topk

NAN, INF = float("nan"), float("inf")
POOL = [NAN, INF, -INF, 0.0, -0.0, 1.5, 1.5, -2.0, 3.25, -1e300, 5e-324, -5e-324]


def _vectors(n, seed):
    rnd = random.Random(seed)
    for _ in range(n):
        L = rnd.randint(1, 12)
        yield [rnd.choice(POOL) for _ in range(L)]


def test_first_entry_is_the_breeze_argmax():
    for v in _vectors(20000, 1):
        assert topk.rank(v, 1)[0] == O.argmax_first(v), v
        assert topk.rank(v, len(v))[0] == O.argmax_first(v), v


def test_rank_is_a_permutation_prefix_in_order():
    for v in _vectors(5000, 2):
        full = topk.rank(v, len(v))
        assert sorted(full) == list(range(len(v)))
        for k in range(1, len(v) + 1):
            assert topk.rank(v, k) == full[:k]
        # consecutive entries respect the rule: never a greater value later,
        # equal values by ascending index
        for a, b in zip(full, full[1:]):
            x, y = v[a], v[b]
            if x == x and y == y:
                assert x > y or (x == y and a < b), (v, full)


def test_all_zero_vector_gives_the_first_k_indices():
    for L in (1, 2, 5, 300):
        for k in {1, min(L, 2), min(L, 16)}:
            assert topk.rank([0.0] * L, k) == list(range(k))
    assert topk.rank([0.0, -0.0, 0.0, -0.0], 4) == [0, 1, 2, 3]  # -0.0 equals +0.0
    assert topk.rank([-0.0, 0.0, 1.0], 3) == [2, 0, 1]


def test_nan_first_at_index_0_and_last_elsewhere():
    assert topk.rank([NAN, INF, 1.0], 3) == [0, 1, 2]
    assert topk.rank([1.0, NAN, -INF, NAN, 2.0], 5) == [4, 0, 2, 1, 3]
    assert topk.rank([NAN, NAN, -INF], 3) == [0, 2, 1]
    assert topk.rank([-INF, NAN], 2) == [0, 1]
    assert topk.rank([NAN], 1) == [0]


def test_ties_keep_ascending_index():
    assert topk.rank([2.0, 3.0, 3.0, 2.0, 3.0], 5) == [1, 2, 4, 0, 3]
    assert topk.rank([INF, INF, -INF, -INF], 4) == [0, 1, 2, 3]


def test_k_outside_the_vector_is_rejected():
    for k in (0, -1, 4):
        with pytest.raises(ValueError):
            topk.rank([1.0, 2.0, 3.0], k)
    assert math.isnan(NAN) and topk.MAX_TOPK == 16
