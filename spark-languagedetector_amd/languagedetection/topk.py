"""The order of a document's scores behind SCORE's top-k output, restated in
plain Python: the checker of ldgpu_score_topk (include/ldgpu.h), importable
without a GPU, as preprocessing.py is for the device preprocessors.

Language i comes before language j if s[i] > s[j], or if the two compare
equal and i < j, where

  * -0.0 equals +0.0;
  * a NaN at index 0 comes first;
  * a NaN at any other index comes after every non-NaN value (-inf
    included), NaNs among themselves by ascending index.

Entry 0 of the order is breeze's argmax (LanguageDetectorModel.scala:154: the
first element, then strictly-greater updates), i.e. the label SCORE gives.
"""
from __future__ import annotations

from typing import List, Sequence

MAX_TOPK = 16  # LDGPU_MAX_TOPK


def _key(s: Sequence[float], i: int):
    """Sort key of language i: smaller = earlier in the order."""
    v = s[i]
    if v != v:
        return (0, 0.0, 0) if i == 0 else (2, 0.0, i)
    return (1, -v, i)  # (-(-0.0) == -(+0.0): equal, then the index decides)


def rank(scores_row: Sequence[float], k: int) -> List[int]:
    """The first k languages of the order of `scores_row`."""
    s = [float(x) for x in scores_row]
    if not 1 <= k <= len(s):
        raise ValueError(f"k = {k} outside [1, {len(s)}]")
    return sorted(range(len(s)), key=lambda i: _key(s, i))[:k]
