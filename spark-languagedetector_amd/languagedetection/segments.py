"""The smoothing rule behind SCORE's segment output, restated in plain numpy
fp64 loops: the checker of ldgpu_score_segments (include/ldgpu.h), importable
without a GPU, as topk.py and spans.py are for their rules.

A document's spans 0 .. n-1 (languagedetection.spans) have the score rows
s_j[0 .. L).  With penalty an fp64 >= 0 (+inf allowed):

    first_max(v):  m = v[0], a = 0;  for l = 1 .. L-1: if v[l] > m: m = v[l]; a = l

    dp_0[l]    = s_0[l]
    (m_j, a_j) = first_max(dp_j)
    for j >= 1, with t = m_{j-1} - penalty (one fp64 subtraction):
        switch_j[l] = (t > dp_{j-1}[l])          a tie stays; any comparison with a NaN stays
        dp_j[l]     = s_j[l] + (t if switch_j[l] else dp_{j-1}[l])      one fp64 addition

    y_{n-1} = a_{n-1};   y_{j-1} = a_{j-1} if switch_j[y_j] else y_j     for j = n-1 .. 1

y_j is span j's smoothed label.  All comparisons are plain IEEE `>`, and no
multiply appears.  first_max is breeze's first maximum, the rule ldgpu_score
labels by: a document of one span keeps its span label, an empty document's
single empty span gets 0; with penalty = inf no span ever switches.

For finite scores the path maximises  sum_j s_j[y_j] - penalty * #(j: y_j !=
y_{j-1})  over all label sequences (best_path_value is the brute force).
"""
from __future__ import annotations

import itertools
from typing import Sequence, Tuple

import numpy as np


def check_penalty(penalty: float) -> float:
    p = float(penalty)
    if not p >= 0.0:
        raise ValueError(f"segment penalty = {p}: it must be >= 0 (+inf allowed)")
    return p


def first_max(v: np.ndarray) -> Tuple[np.float64, int]:
    if not np.isnan(v).any():  # (the same scan: argmax returns the first of the maxima, -0.0 == +0.0)
        a = int(np.argmax(v))
        return v[a], a
    m, a = v[0], 0
    for l in range(1, len(v)):
        if v[l] > m:
            m, a = v[l], l
    return m, a


def trace(scores: np.ndarray, penalty: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(switch bool[n, L], a int64[n], y int32[n]) of one document's score rows
    fp64[n, L]: the rule's intermediate values and the smoothed labels."""
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] < 1:
        raise ValueError("scores must be [n, L] with L >= 1")
    pen = np.float64(check_penalty(penalty))
    n, L = s.shape
    y = np.zeros(n, dtype=np.int32)
    switch = np.zeros((n, L), dtype=bool)
    arg = np.zeros(n, dtype=np.int64)
    if n == 0:
        return switch, arg, y
    dp = s[0].copy()
    m, arg[0] = first_max(dp)
    with np.errstate(invalid="ignore"):  # inf - inf, inf + -inf: NaN, as the rule says
        for j in range(1, n):
            t = m - pen
            switch[j] = t > dp                          # elementwise over l
            dp = s[j] + np.where(switch[j], t, dp)
            m, arg[j] = first_max(dp)
    y[n - 1] = arg[n - 1]
    for j in range(n - 1, 0, -1):
        y[j - 1] = arg[j - 1] if switch[j, y[j]] else y[j]
    return switch, arg, y


def smooth(scores: np.ndarray, penalty: float) -> np.ndarray:
    """int32[n]: the smoothed labels of one document's score rows fp64[n, L]."""
    return trace(scores, penalty)[2]


def smooth_corpus(scores: np.ndarray, span_offsets: Sequence[int], penalty: float) -> np.ndarray:
    """int32[n_spans]: smooth() of every document's rows
    scores[span_offsets[d]:span_offsets[d + 1]]; documents are independent."""
    s = np.asarray(scores, dtype=np.float64)
    soff = np.asarray(span_offsets, dtype=np.int64)
    check_penalty(penalty)
    out = np.zeros(int(soff[-1]) if len(soff) else 0, dtype=np.int32)
    for d in range(len(soff) - 1):
        a, b = int(soff[d]), int(soff[d + 1])
        out[a:b] = smooth(s[a:b], penalty)
    return out


def path_value(scores: np.ndarray, labels: Sequence[int], penalty: float) -> float:
    """sum_j s_j[y_j] - penalty * (number of label changes)."""
    s = np.asarray(scores, dtype=np.float64)
    y = [int(v) for v in labels]
    changes = sum(1 for j in range(1, len(y)) if y[j] != y[j - 1])
    return float(sum(s[j, y[j]] for j in range(len(y))) - (penalty * changes if changes else 0.0))


def best_path_value(scores: np.ndarray, penalty: float) -> float:
    """The maximum of path_value over all L^n label sequences (tiny inputs)."""
    s = np.asarray(scores, dtype=np.float64)
    n, L = s.shape
    if L ** n > 1 << 20:
        raise ValueError("best_path_value is a brute force: L^n must stay small")
    return max(path_value(s, y, penalty) for y in itertools.product(range(L), repeat=n))
