"""languagedetection.segments -- the smoothing rule behind ldgpu_score_segments,
checked on the CPU: optimality against brute force on exactly representable
inputs, the rule's edge properties, and the independence of documents."""
import itertools

import numpy as np
import pytest

from languagedetection import segments

NAN, INF = float("nan"), float("inf")


def literal(scores, penalty):
    """The rule written out once more with Python floats and lists only."""
    s = [[float(v) for v in row] for row in scores]
    n, L = len(s), len(s[0])

    def first_max(v):
        m, a = v[0], 0
        for l in range(1, L):
            if v[l] > m:
                m, a = v[l], l
        return m, a

    dp = list(s[0])
    sw = [[False] * L for _ in range(n)]
    arg = [0] * n
    m, arg[0] = first_max(dp)
    for j in range(1, n):
        t = m - penalty
        new = []
        for l in range(L):
            sw[j][l] = t > dp[l]
            new.append(s[j][l] + (t if sw[j][l] else dp[l]))
        dp = new
        m, arg[j] = first_max(dp)
    y = [0] * n
    y[n - 1] = arg[n - 1]
    for j in range(n - 1, 0, -1):
        y[j - 1] = arg[j - 1] if sw[j][y[j]] else y[j]
    return y


def test_smooth_reaches_the_best_path_value():
    """Small-integer scores and penalties: every fp64 operation is exact, so
    the returned path's value equals the maximum over all L^n sequences."""
    rng = np.random.default_rng(5)
    cases = 0
    for n, L in itertools.product(range(1, 7), range(1, 5)):
        for penalty in (0, 1, 3, 7):
            for _ in range(4):
                s = rng.integers(-4, 5, size=(n, L)).astype(np.float64)
                y = segments.smooth(s, penalty)
                assert y.dtype == np.int32 and y.shape == (n,)
                assert y.tolist() == literal(s, float(penalty))
                assert segments.path_value(s, y, penalty) == segments.best_path_value(s, penalty), (n, L, penalty, s)
                cases += 1
    assert cases == 6 * 4 * 4 * 4


def test_brute_force_is_what_it_says():
    s = np.array([[3.0, 0.0], [0.0, 5.0]])
    assert segments.best_path_value(s, 2) == 6.0      # 0 -> 1: 3 + 5 - 2
    assert segments.best_path_value(s, 10) == 5.0     # stay at 1
    assert segments.path_value(s, [0, 1], 2) == 6.0 and segments.path_value(s, [1, 1], 2) == 5.0
    assert segments.smooth(s, 2).tolist() == [0, 1] and segments.smooth(s, 10).tolist() == [1, 1]
    with pytest.raises(ValueError):
        segments.best_path_value(np.zeros((30, 4)), 1)


def test_one_span_documents_keep_the_first_maximum():
    rng = np.random.default_rng(6)
    for L in (1, 2, 7):
        for _ in range(20):
            row = rng.integers(-2, 3, size=(1, L)).astype(np.float64)
            for penalty in (0.0, 1.5, INF):
                assert segments.smooth(row, penalty).tolist() == [int(np.argmax(row[0]))]
    assert segments.smooth(np.zeros((1, 5)), 1.0).tolist() == [0]       # an empty span: no hit
    assert segments.smooth(np.zeros((0, 5)), 1.0).shape == (0,)


def test_infinite_penalty_gives_one_label_per_document():
    rng = np.random.default_rng(7)
    for _ in range(20):
        s = rng.normal(size=(int(rng.integers(2, 40)), 5))
        y = segments.smooth(s, INF)
        assert len(set(y.tolist())) == 1
        # ... the first maximum of the left-folded column sums (dp never switches)
        dp = s[0].copy()
        for j in range(1, len(s)):
            dp = s[j] + dp
        assert y[0] == int(np.argmax(dp))
    soff = [0, 3, 4, 9]
    y = segments.smooth_corpus(rng.normal(size=(9, 4)), soff, INF)
    assert all(len(set(y[a:b].tolist())) == 1 for a, b in zip(soff, soff[1:]))


def test_a_tie_stays():
    # t = m - penalty equals dp[1] exactly: language 1 does not switch
    s = np.array([[3.0, 1.0], [0.0, 4.0]])
    assert segments.smooth(s, 2.0).tolist() == [1, 1]     # 1 + 4 = 5 by staying (a switch would give 5 too)
    assert segments.smooth(s, 1.5).tolist() == [0, 1]     # 3 - 1.5 > 1: switches
    # penalty 0: t = m equals dp[a]: the maximum itself never "switches"
    s = np.array([[2.0, 2.0], [1.0, 1.0], [0.0, 0.0]])
    assert segments.smooth(s, 0.0).tolist() == [0, 0, 0]


def test_nan_rows():
    # a NaN at index 0 is the first maximum; t = NaN: nothing switches, and
    # dp[0] stays NaN for good: every later first maximum is 0 too
    s = np.array([[NAN, 5.0, 1.0], [0.0, 0.0, 9.0]])
    assert segments.first_max(s[0])[1] == 0 and np.isnan(segments.first_max(s[0])[0])
    assert segments.smooth(s, 1.0).tolist() == literal(s, 1.0) == [0, 0]
    s3 = np.array([[NAN, 5.0, 1.0], [0.0, 0.0, 9.0], [0.0, 0.0, 0.0]])
    assert segments.smooth(s3, 1.0).tolist() == literal(s3, 1.0) == [0, 0, 0]
    # a NaN elsewhere never wins and never switches (t > NaN is false)
    s = np.array([[1.0, NAN, 0.0], [0.0, 0.0, 7.0]])
    assert segments.first_max(s[0]) == (1.0, 0)
    assert segments.smooth(s, 0.5).tolist() == literal(s, 0.5) == [0, 2]
    s = np.array([[-INF, NAN], [0.0, 0.0]])
    assert segments.first_max(s[0])[1] == 0
    assert segments.smooth(s, 0.0).tolist() == literal(s, 0.0)
    # inf - inf: t is NaN, the span stays
    s = np.array([[INF, 0.0], [0.0, 1.0]])
    assert segments.smooth(s, INF).tolist() == literal(s, INF) == [0, 0]


def test_signed_zero_tie():
    for row in ([-0.0, 0.0], [0.0, -0.0]):
        m, a = segments.first_max(np.array(row))
        assert a == 0 and np.signbit(m) == np.signbit(row[0])
    s = np.array([[-0.0, 0.0, -1.0], [0.0, -0.0, -1.0]])
    assert segments.smooth(s, 0.0).tolist() == literal(s, 0.0) == [0, 0]


def test_penalty_is_checked():
    for bad in (-1.0, -0.0001, NAN, -INF):
        with pytest.raises(ValueError, match="penalty"):
            segments.smooth(np.zeros((2, 2)), bad)
        with pytest.raises(ValueError, match="penalty"):
            segments.smooth_corpus(np.zeros((2, 2)), [0, 2], bad)
    assert segments.smooth(np.zeros((2, 2)), -0.0).tolist() == [0, 0]


def test_documents_are_independent():
    rng = np.random.default_rng(8)
    counts = [1, 5, 1, 64, 2, 17, 1]
    docs = [rng.integers(-3, 4, size=(n, 6)).astype(np.float64) for n in counts]
    soff = np.concatenate([[0], np.cumsum(counts)])
    for penalty in (0.0, 2.0, INF):
        y = segments.smooth_corpus(np.concatenate(docs), soff, penalty)
        each = [segments.smooth(d, penalty) for d in docs]
        assert np.array_equal(y, np.concatenate(each))
        perm = rng.permutation(len(docs))
        soff_p = np.concatenate([[0], np.cumsum([counts[i] for i in perm])])
        y_p = segments.smooth_corpus(np.concatenate([docs[i] for i in perm]), soff_p, penalty)
        assert np.array_equal(y_p, np.concatenate([each[i] for i in perm]))
        assert len({tuple(e.tolist()) for e in each}) > 1
