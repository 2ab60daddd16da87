"""languagedetection.utf8.span_geometry / byte_runs -- the span rule of
include/ldgpu.h "UTF-8: top-k, spans, segments" stated in numpy, the checker
that needs no GPU -- against a brute-force walk over Python str: per character,
text.encode("utf-8") gives its bytes and text.encode("utf-16-le") its units."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from languagedetection import _lib, spans, utf8

GEOMETRIES = [(1, 1), (2, 1), (3, 2), (5, 3), (7, 7), (64, 32), (300, 257)]
ILL = [b"\xe2\x82", b"\xc0\x80", b"ab\xff", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"x" * 300 + b"\xf0\x9f\x98"]
NAMES = ["ldgpu_span_offsets_utf", "ldgpu_span_offsets_utf_device", "ldgpu_score_topk_utf",
         "ldgpu_score_topk_utf_device", "ldgpu_score_spans_utf", "ldgpu_score_spans_utf_device",
         "ldgpu_score_segments_utf", "ldgpu_score_segments_utf_device"]


def texts():
    rng = np.random.default_rng(3)
    alphabet = ["a", "z", "é", "ß", "€", "語", "😀", "𐍈", " "]
    out = ["", "a", "é", "€", "😀", "😀" * 5, "a😀", "😀a", "ab😀cd😀", "😀" * 200, "€" * 90 + "😀" * 90]
    for n in (2, 3, 7, 31, 64, 65, 129, 300, 601):
        out.append("".join(alphabet[i] for i in rng.integers(0, len(alphabet), n)))
    return out


def brute(text, width, stride):
    """(units, [start of every span]) by walking the characters."""
    lead_of_unit, at = [], 0
    for ch in text:
        lead_of_unit += [at] * (len(ch.encode("utf-16-le")) // 2)
        at += len(ch.encode("utf-8"))
    u = len(lead_of_unit)
    n = spans.span_count(u, width, stride)
    return u, [lead_of_unit[j * stride] if u else 0 for j in range(n)]


@pytest.mark.parametrize("width,stride", GEOMETRIES)
def test_span_geometry_matches_a_walk_over_str(width, stride):
    docs, want_units, want_starts, want_counts = [], [], [], []
    for i, t in enumerate(texts()):
        docs.append(t.encode("utf-8"))
        u, st = brute(t, width, stride)
        want_units.append(u)
        want_starts += st
        want_counts.append(len(st))
        ill = ILL[i % len(ILL)]                 # every entry of the ill-formed list, interleaved
        docs.append(ill)
        want_units.append(-1)
        want_starts.append(0)
        want_counts.append(1)
    docs = [b""] + docs + [b""]
    want_units, want_counts, want_starts = [0] + want_units + [0], [1] + want_counts + [1], [0] + want_starts + [0]
    assert len(docs) >= 2 * len(ILL)
    data, off = utf8.pack_utf8(docs)
    soff, units, starts = utf8.span_geometry(data, off, width, stride)
    assert units.tolist() == want_units
    assert np.diff(soff).tolist() == want_counts and soff[0] == 0
    assert starts.tolist() == want_starts
    for d, doc in enumerate(docs):
        s = starts[soff[d]:soff[d + 1]]
        assert s[0] == 0 and (np.diff(s) >= 0).all()
        assert units[d] <= 0 or s[-1] < len(doc)


def test_a_boundary_inside_a_pair_gives_the_lead():
    text = "😀" * 6            # 12 units, 24 bytes
    doc = text.encode("utf-8")
    # odd strides split every second pair; stride 1 gives both halves the same start
    _, units, starts = utf8.span_geometry(doc, [0, len(doc)], 1, 1)
    assert units.tolist() == [12] and starts.tolist() == [4 * (j // 2) for j in range(12)]
    _, _, starts = utf8.span_geometry(doc, [0, len(doc)], 3, 3)
    assert starts.tolist() == [0, 4, 12, 16]          # units 0, 3 (low of pair 1), 6, 9 (low of pair 4)
    _, _, starts = utf8.span_geometry(doc, [0, len(doc)], 5, 3)
    assert starts.tolist() == [0, 4, 12, 16]          # 1 + ceil(7 / 3) = 4 spans
    # offsets[0] > 0 and no documents
    data = np.frombuffer(b"\xf0zz" + doc, dtype=np.uint8)
    soff, units, starts = utf8.span_geometry(data, [3, 3 + len(doc)], 4, 2)
    assert soff.tolist() == [0, 5] and units.tolist() == [12] and starts.tolist() == [0, 4, 8, 12, 16]
    soff, units, starts = utf8.span_geometry(data, [3], 4, 2)
    assert soff.tolist() == [0] and len(units) == 0 and len(starts) == 0
    with pytest.raises(ValueError):
        utf8.span_geometry(doc, [0, len(doc)], 2, 3)


@pytest.mark.parametrize("width,stride", GEOMETRIES)
def test_byte_runs_slice_the_document_into_whole_characters(width, stride):
    rng = np.random.default_rng(width * 1000 + stride)
    for t in texts():
        doc = t.encode("utf-8")
        soff, units, starts = utf8.span_geometry(doc, [0, len(doc)], width, stride)
        n = int(soff[1])
        for labels in (rng.integers(0, 3, n), np.arange(n), np.zeros(n, dtype=np.int64)):
            r = utf8.byte_runs(starts, len(doc), labels)
            assert b"".join(doc[a:b] for a, b, _ in r) == doc
            assert "".join(doc[a:b].decode("utf-8") for a, b, _ in r) == t
            assert all(a < b for a, b, _ in r) and all(r[i][1] == r[i + 1][0] for i in range(len(r) - 1))
            assert all(r[i][2] != r[i + 1][2] for i in range(len(r) - 1))
            # the unit twin: the same labels in the same order, once the unit
            # runs that hold no whole character are out -- a character's bytes
            # go to the span of its last unit (its low surrogate, if it has one)
            u16 = np.frombuffer(t.encode("utf-16-le"), dtype="<u2")
            high = (u16 >= 0xD800) & (u16 <= 0xDBFF)
            lasts = np.flatnonzero(~high)

            def whole(a, b):
                return bool(((lasts >= a) & (lasts < b)).any())

            unit_labels = [lab for a, b, lab in spans.runs(int(units[0]), labels, width, stride) if whole(a, b)]
            merged = [lab for i, lab in enumerate(unit_labels) if i == 0 or unit_labels[i - 1] != lab]
            assert [lab for _, _, lab in r] == merged


def test_a_unit_run_without_a_whole_character_has_no_byte_run():
    """Stride 1, every span its own label: the span that is a pair's high
    surrogate alone starts at the same byte as the next span (the pair's low
    surrogate, whose start is the lead), so it owns no byte and is dropped;
    spans.runs keeps it as a run of one unit."""
    t = "a😀b"
    doc = t.encode("utf-8")
    soff, units, starts = utf8.span_geometry(doc, [0, len(doc)], 1, 1)
    assert units.tolist() == [4] and starts.tolist() == [0, 1, 1, 5]
    labels = [0, 1, 2, 3]
    assert spans.runs(4, labels, 1, 1) == [(0, 1, 0), (1, 2, 1), (2, 3, 2), (3, 4, 3)]
    assert utf8.byte_runs(starts, len(doc), labels) == [(0, 1, 0), (1, 5, 2), (5, 6, 3)]
    assert doc[1:5].decode("utf-8") == "😀"
    # an empty document and an ill-formed one: one span at 0, no run
    assert utf8.byte_runs([0], 0, [-1]) == []
    with pytest.raises(ValueError):
        utf8.byte_runs([0, 1], 2, [0])


def test_the_eight_entry_points():
    src = open(os.path.join(ROOT, "include", "ldgpu.h")).read()
    declared = set(re.findall(r"\b(ldgpu_[a-z_]+)\s*\(", src))
    assert set(NAMES) <= declared
    assert set(NAMES) <= set(_lib.exported_symbols())
    assert not any("utf8" in s for s in NAMES)
    assert not set(NAMES) & set(_lib.utf8_symbols())
    for variant in ("product", "diag"):
        lib = _lib.load(variant=variant)
        for s in NAMES:
            assert getattr(lib, s).argtypes is not None and len(getattr(lib, s).argtypes) >= 7
