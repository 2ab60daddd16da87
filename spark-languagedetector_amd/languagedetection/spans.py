"""The span rule behind SCORE's per-span output, restated in plain Python: the
checker of ldgpu_score_spans (include/ldgpu.h), importable without a GPU, as
topk.py is for the top-k order.

A document of `length` bytes is cut into overlapping spans of `width` bytes
every `stride` bytes (1 <= stride <= width):

  * one span if length <= width, otherwise 1 + ceil((length - width) / stride);
  * span j is bytes [j * stride, min(j * stride + width, length)) of the
    document; an empty document has one empty span;
  * spans are numbered document by document: span_offsets[d] is the index of
    document d's first span, span_offsets[n_docs] the number of spans.

Every span is scored as a document of its own.  runs() turns a document's span
labels into (start, end, label) runs: span j owns the units [j * stride,
(j + 1) * stride), the last span up to the document's end; consecutive spans of
one label merge; empty runs are dropped.  In the SCORE encoding one byte is one
UTF-16 unit, so the bounds index the Java or Python string.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

MAX_WIDTH = (1 << 28) - 1  # the document limit of the staged kernels


def check(width: int, stride: int) -> None:
    if width < 1:
        raise ValueError(f"span width = {width} < 1")
    if not 1 <= stride <= width:
        raise ValueError(f"span stride = {stride} outside [1, width = {width}]")
    if width > MAX_WIDTH:
        raise NotImplementedError(f"span width = {width}: the device path's limit is {MAX_WIDTH}")


def span_count(length: int, width: int, stride: int) -> int:
    return 1 if length <= width else 1 + -(-(length - width) // stride)


def span_bounds(length: int, width: int, stride: int) -> List[Tuple[int, int]]:
    """[(start, end)] of a document's spans, relative to the document."""
    check(width, stride)
    return [(j * stride, min(j * stride + width, length)) for j in range(span_count(length, width, stride))]


def span_offsets(offsets: Sequence[int], width: int, stride: int) -> np.ndarray:
    """int64[n_docs + 1]: the index of every document's first span."""
    check(width, stride)
    off = np.asarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("offsets must hold n_docs + 1 entries")
    lens = np.diff(off)
    if off[0] < 0 or (lens < 0).any():
        raise ValueError("offsets decrease")
    counts = np.where(lens <= width, 1, 1 + -(-(lens - width) // stride))
    out = np.zeros(len(off), dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def materialise(data: np.ndarray, offsets: Sequence[int], width: int, stride: int) -> Tuple[np.ndarray, np.ndarray]:
    """(span_data, span_byte_offsets): every span as a document of its own, in
    span order, packed like encoding.pack (padded to a multiple of 4, + 4)."""
    soff = span_offsets(offsets, width, stride)
    off = np.asarray(offsets, dtype=np.int64)
    n_docs, n_spans = len(off) - 1, int(soff[-1])
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(soff))
    j = np.arange(n_spans, dtype=np.int64) - soff[doc]
    start = off[doc] + j * stride
    end = np.minimum(start + width, off[doc + 1]) if n_spans else start
    lens = end - start
    boff = np.zeros(n_spans + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    total = int(boff[-1])
    # source index of every output byte: its span's start plus its position in the span
    idx = np.repeat(start - boff[:-1], lens) + np.arange(total, dtype=np.int64)
    out = np.zeros(((total + 3) & ~3) + 4, dtype=np.uint8)
    out[:total] = np.asarray(data, dtype=np.uint8)[idx]
    return out, boff


def runs(length: int, labels: Sequence[int], width: int, stride: int) -> List[Tuple[int, int, int]]:
    """[(start, end, label)] of a document of `length` units from its span
    labels (len(labels) == span_count(length, width, stride))."""
    check(width, stride)
    n = span_count(length, width, stride)
    if len(labels) != n:
        raise ValueError(f"{len(labels)} labels for a document of {n} spans")
    out: List[Tuple[int, int, int]] = []
    for j in range(n):
        a, b, lab = j * stride, (length if j == n - 1 else (j + 1) * stride), int(labels[j])
        if b <= a:
            continue
        if out and out[-1][2] == lab:
            out[-1] = (out[-1][0], b, lab)
        else:
            out.append((a, b, lab))
    return out
