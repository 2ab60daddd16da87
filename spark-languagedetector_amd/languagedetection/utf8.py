"""The UTF-8 rule behind SCORE's UTF-8 entry points, restated in numpy: the
checker of ldgpu_utf8_decode / ldgpu_score_utf8 (include/ldgpu.h UTF-8),
importable without a GPU, as topk.py is for the top-k order.

FIT counts a text's UTF-8 bytes, SCORE scans the low byte of every UTF-16 code
unit (encoding.py).  A caller that stores UTF-8 hands it over as it is; the
device decodes it by this rule.

A document is well-formed iff its bytes are a concatenation of the sequences
of Unicode Table 3-7 (``_TABLE`` below).  Everything else is ill-formed: C0,
C1 and F5..FF anywhere, a continuation byte without a lead, an overlong form,
an encoded surrogate (ED A0..BF), a value beyond U+10FFFF, a sequence cut off
by the end of its document (a sequence never borrows bytes from the next
document).  That set is what CPython's ``bytes.decode("utf-8")`` accepts --
the codec is what this module is tested against, so nothing here calls it.

A code point below 0x10000 gives one UTF-16 unit, a larger one a surrogate
pair; an ill-formed document is not decoded (host flag 1, empty output).

Spans of UTF-8 documents (ldgpu_span_offsets_utf, ldgpu_score_spans_utf,
ldgpu_score_segments_utf, ldgpu_score_topk_utf and their _device forms;
``span_geometry`` and ``byte_runs`` below are their checker).  The rule:

  - `width` and `stride` count UTF-16 units (= SCORE bytes), exactly as in
    ldgpu_score_spans.
  - A document's spans are those of ldgpu_span_offsets applied to its unit
    count u: one span if u <= width, otherwise 1 + ceil((u - width) / stride).
  - Well-formedness is ldgpu_utf8_decode's rule (Unicode Table 3-7).  An
    ill-formed document counts as u = 0: it has one empty span.
  - units[d] is u for a well-formed document and -1 for an ill-formed one.
  - start[i], for span j of document d, is an int64 byte index relative to
    the document's first byte: the index of the lead byte of the character
    that unit j * stride belongs to.  If unit j * stride is the low surrogate
    of a 4-byte character (the boundary splits the pair), it is that
    character's lead byte.  A character's bytes therefore always belong to
    one run, the one starting at or before its first unit.  At stride == 1
    both units of a pair give the same start.  Span 0 of every document has
    start 0; this includes an empty document's single span and an ill-formed
    document's single span.  Starts are non-decreasing within a document.
    Every start is < len for a non-empty well-formed document.
  - Labels and score rows of a well-formed document's spans are bit for bit
    those of ldgpu_score_spans, ldgpu_score_segments or ldgpu_score_topk on
    its SCORE encoding, on every model layout.
  - For an ill-formed document: its single span gets label -1 and the empty
    document's score row; the top-k form gives -1 in all k label entries and
    0.0 in the scores; the segment form gives -1.
  - ``byte_runs`` turns span labels into runs in bytes.  Span j owns bytes
    [start[j], start[j+1]), the last span up to the document's byte length.
    Consecutive spans of one label merge.  Empty runs are dropped.  This is
    the byte twin of ``spans.runs``.

The byte runs carry the labels of ``spans.runs`` in the same order, except
where a unit run holds no whole character.  That happens where a span boundary
splits a surrogate pair: the character's bytes go, whole, to the span that
starts at its low surrogate.  A span that is nothing but such a pair's high
surrogate (stride 1) then owns no byte: its start equals the next span's, its
byte run is empty and is dropped, while ``spans.runs`` keeps a run of one unit.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from ._lib import UTF8_STEP_BYTES

# bytes of a document that one wave of the device decoder takes per step
# (LDGPU_UTF8_STEP_BYTES; tests place sequences across this boundary)
STEP_BYTES = UTF8_STEP_BYTES

# Unicode Table 3-7: (first lead, last lead, sequence length, second byte's range)
_TABLE = ((0x00, 0x7F, 1, None),
          (0xC2, 0xDF, 2, (0x80, 0xBF)),
          (0xE0, 0xE0, 3, (0xA0, 0xBF)),
          (0xE1, 0xEC, 3, (0x80, 0xBF)),
          (0xED, 0xED, 3, (0x80, 0x9F)),
          (0xEE, 0xEF, 3, (0x80, 0xBF)),
          (0xF0, 0xF0, 4, (0x90, 0xBF)),
          (0xF1, 0xF3, 4, (0x80, 0xBF)),
          (0xF4, 0xF4, 4, (0x80, 0x8F)))


def _lead_tables():
    """Per byte value: the sequence length it announces as a lead (0: a
    continuation byte, -1: a byte no well-formed text holds) and the range of
    its second byte."""
    n = np.full(256, -1, dtype=np.int64)
    lo = np.zeros(256, dtype=np.int64)
    hi = np.zeros(256, dtype=np.int64)
    n[0x80:0xC0] = 0
    for first, last, length, second in _TABLE:
        n[first:last + 1] = length
        if second:
            lo[first:last + 1], hi[first:last + 1] = second
    return n, lo, hi


_LEN, _LO, _HI = _lead_tables()


def pack_utf8(docs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """Byte strings packed as (data uint8, offsets int64[n + 1]); data is padded
    to a multiple of 4 bytes (+4), as encoding.pack does."""
    from .encoding import pack
    return pack([bytes(d) for d in docs])


def span_geometry(data, offsets, width: int, stride: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(span_offsets int64[n + 1], units int64[n], starts int64[n_spans]) of
    the documents data[offsets[d]:offsets[d + 1]] by the rule above: what
    ldgpu_span_offsets_utf and the `starts` of ldgpu_score_spans_utf give."""
    from .spans import check
    check(width, stride)
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_docs = len(offsets) - 1
    if n_docs <= 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    _, unit_off, host = decode(data, offsets, low_bytes=True)
    u = np.diff(unit_off)
    units = np.where(host != 0, -1, u)
    counts = np.where(u <= width, 1, 1 + -(-(u - width) // stride))
    span_offsets = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(counts, out=span_offsets[1:])
    starts = np.zeros(int(span_offsets[-1]), dtype=np.int64)
    # the leads of the well-formed documents: byte position, document, first unit
    b0, b1 = int(offsets[0]), int(offsets[-1])
    c = data[b0:b1].astype(np.int64)
    pos = np.arange(len(c), dtype=np.int64) + b0
    doc = np.searchsorted(offsets, pos, side="right") - 1
    lead = (_LEN[c] >= 1) & (host[doc] == 0) if len(c) else np.zeros(0, dtype=bool)
    pos, doc, two = pos[lead], doc[lead], _LEN[c[lead]] == 4
    n_units = np.where(two, 2, 1)
    rank = np.cumsum(n_units) - n_units - unit_off[doc]      # the lead's first unit within its document
    for t, has in ((0, np.ones(len(pos), dtype=bool)), (1, two)):
        r = rank + t
        at = has & (r % stride == 0) & (r // stride < counts[doc])
        starts[span_offsets[doc[at]] + r[at] // stride] = pos[at] - offsets[doc[at]]
    return span_offsets, units, starts


def byte_runs(starts_d, n_bytes_d: int, labels_d) -> list:
    """[(start, end, label)] in bytes of one document of `n_bytes_d` bytes from
    its spans' starts and labels: span j owns [starts_d[j], starts_d[j + 1]),
    the last span up to n_bytes_d; consecutive spans of one label merge, empty
    runs are dropped (the byte twin of spans.runs)."""
    if len(starts_d) != len(labels_d):
        raise ValueError(f"{len(labels_d)} labels for {len(starts_d)} span starts")
    n = len(starts_d)
    out = []
    for j in range(n):
        a, b, lab = int(starts_d[j]), (int(n_bytes_d) if j == n - 1 else int(starts_d[j + 1])), int(labels_d[j])
        if b <= a:
            continue
        if out and out[-1][2] == lab:
            out[-1] = (out[-1][0], b, lab)
        else:
            out.append((a, b, lab))
    return out


def decode(data, offsets, low_bytes: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(out, out_offsets int64[n + 1], host uint8[n]) of the documents
    data[offsets[d]:offsets[d + 1]]: `out` holds the UTF-16 units (uint16) of
    every well-formed document -- with low_bytes their low bytes (uint8), the
    SCORE encoding -- and host[d] = 1 marks an ill-formed one, whose output is
    empty.

    Every lead byte checks its own followers (inside its document); a follower
    is a continuation byte and hence no lead, so a document is well-formed iff
    every lead passes and the lengths of its leads sum to its length."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_docs = len(offsets) - 1
    out_dtype = np.uint8 if low_bytes else np.uint16
    if n_docs <= 0:
        return np.zeros(0, dtype=out_dtype), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint8)
    b0, b1 = int(offsets[0]), int(offsets[-1])
    c = data[b0:b1].astype(np.int64)
    total = len(c)
    pos = np.arange(total, dtype=np.int64) + b0
    doc = np.searchsorted(offsets, pos, side="right") - 1     # (empty documents own no byte)
    end = offsets[doc + 1] if total else pos
    # the three bytes after each byte (0 beyond the buffer: never a continuation)
    pad = np.concatenate([c, np.zeros(3, dtype=np.int64)])
    c1, c2, c3 = pad[1:total + 1], pad[2:total + 2], pad[3:total + 3]
    n = _LEN[c]
    cont2, cont3 = (c2 & 0xC0) == 0x80, (c3 & 0xC0) == 0x80
    ok = (n >= 0) & (pos + n <= end)
    ok &= (n < 2) | ((c1 >= _LO[c]) & (c1 <= _HI[c]))
    ok &= (n < 3) | cont2
    ok &= (n < 4) | cont3
    claimed = np.bincount(doc, weights=np.where(ok, n, 0), minlength=n_docs).astype(np.int64) if total else \
        np.zeros(n_docs, dtype=np.int64)
    bad = np.bincount(doc, weights=~ok, minlength=n_docs) > 0 if total else np.zeros(n_docs, dtype=bool)
    host = bad | (claimed != np.diff(offsets))
    # code points of the leads of well-formed documents
    lead = (n >= 1) & ~host[doc] if total else np.zeros(0, dtype=bool)
    cl, n_l = c[lead], n[lead]
    x1, x2, x3 = c1[lead] & 0x3F, c2[lead] & 0x3F, c3[lead] & 0x3F
    cp = np.where(n_l == 1, cl,
                  np.where(n_l == 2, ((cl & 0x1F) << 6) | x1,
                           np.where(n_l == 3, ((cl & 0x0F) << 12) | (x1 << 6) | x2,
                                    ((cl & 0x07) << 18) | (x1 << 12) | (x2 << 6) | x3)))
    two = cp >= 0x10000
    v = cp - 0x10000
    n_units = np.where(two, 2, 1)
    first = np.zeros(len(cp) + 1, dtype=np.int64)
    np.cumsum(n_units, out=first[1:])
    units = np.zeros(int(first[-1]), dtype=np.int64)
    units[first[:-1]] = np.where(two, 0xD800 + (v >> 10), cp)
    units[first[:-1][two] + 1] = 0xDC00 + (v[two] & 0x3FF)
    per_doc = np.bincount(doc[lead], weights=n_units, minlength=n_docs).astype(np.int64) if total else \
        np.zeros(n_docs, dtype=np.int64)
    out_offsets = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(per_doc, out=out_offsets[1:])
    out = (units & 0xFF).astype(np.uint8) if low_bytes else units.astype(np.uint16)
    return out, out_offsets, host.astype(np.uint8)
