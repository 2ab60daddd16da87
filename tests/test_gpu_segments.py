"""SCORE's smoothed span labels (ldgpu_score_segments /
ldgpu_score_segments_device) against languagedetection.segments.smooth_corpus
applied to the C oracle's score rows of languagedetection.spans.materialise:
labels exactly equal, through the host and the device form."""
import ctypes
import functools
import math
import threading

import numpy as np
import pytest

from languagedetection import LanguageDetectorModel, _lib, encoding, segments, spans
from languagedetection.runtime import DeviceModel, PinnedArray
from test_gpu_spans import KINDS, kind_model, kind_table, oracle
from test_gpu_topk import make_table

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
GEOMETRY = [(4, 2), (5, 1), (64, 32)]
GRAMS = (1, 2, 3)
# (L, key lengths, form): "count" (a partial switch word), "dense" and "L300"
# (language blocks; dp in LDS) are the span tests' tables; L64 fills one switch
# word exactly, L130 takes three words per span with a partial last one
OWN = {"L64": (64, (1, 2, 3), "count"), "L130": (130, (1, 2, 3), "count")}
TABLES = ["count", "dense", "L300", "L64", "L130"]
# two finite penalties per geometry, chosen on the CPU from the oracle's score
# rows of seg_corpus: a span's score is a sum of log(1 + 1/k) per hit window
# (normal values in the dense table), so the scale grows with the width.  At
# the first every table has 10 % of its spans relabelled or more, at the second
# every table still has a document with two switches left (both asserted)
FINITE = {(4, 2): (0.7, 3.0), (5, 1): (0.7, 3.0), (64, 32): (6.0, 25.0)}


def seg_L(kind):
    return OWN[kind][0] if kind in OWN else KINDS[kind][0]


def seg_grams(kind):
    return GRAMS if kind in OWN else KINDS[kind][1]


@functools.lru_cache(maxsize=None)
def seg_table(kind):
    if kind not in OWN:
        return kind_table(kind)
    L, key_lens, form = OWN[kind]
    return make_table(np.random.default_rng(1300 + L), L, 400, list(key_lens), form)


@functools.lru_cache(maxsize=None)
def seg_model(kind, variant="product"):
    if kind not in OWN:
        return kind_model(kind, variant)
    return DeviceModel(seg_table(kind), seg_L(kind), list(GRAMS), variant=variant)


@functools.lru_cache(maxsize=None)
def keys_by_language(kind):
    """{language: the keys whose row is maximal (and positive) there}, for the
    languages with five such keys or more."""
    by = {}
    for key, row in seg_table(kind).items():
        top = max(row)
        if top > 0:
            for l, v in enumerate(row):
                if v == top:
                    by.setdefault(l, []).append(key)
    return {l: ks for l, ks in sorted(by.items()) if len(ks) >= 5}


def stretch_doc(rng, n_bytes, kind, stride):
    """n_bytes of stretches (4 .. 24 strides each) drawn from the keys of one
    language after the other, one key in seven from any language."""
    by = keys_by_language(kind)
    langs = list(by)[:12]
    every = [k for ks in by.values() for k in ks]
    out, lang = bytearray(), -1
    while len(out) < n_bytes:
        lang = int(rng.choice([l for l in langs if l != lang]))
        end = len(out) + int(rng.integers(4, 25)) * stride
        while len(out) < end:
            pool = every if rng.random() < 1 / 7 else by[lang]
            out += pool[int(rng.integers(0, len(pool)))]
    return bytes(out[:n_bytes])


def doc_bytes(n_spans, width, stride):
    """The length of a document of n_spans >= 2 spans (the shortest one)."""
    return width + (n_spans - 2) * stride + 1


def corpus_of(kind, width, stride, counts, seed):
    """Documents by span count: 0 an empty document, -1 one of width - 1
    bytes, 1 one of 1 .. width bytes, n >= 2 one of n spans."""
    rng = np.random.default_rng(seed)
    docs = []
    for n in counts:
        nb = 0 if n == 0 else width - 1 if n == -1 else int(rng.integers(1, width + 1)) if n == 1 else \
            doc_bytes(n, width, stride)
        docs.append(stretch_doc(rng, nb, kind, stride) if nb else b"")
    data, off = encoding.pack(docs)
    soff = spans.span_offsets(off, width, stride)
    assert np.diff(soff).tolist() == [max(abs(n), 1) for n in counts]
    return data, off, soff


# empty, shorter than width, 2 spans, short ones in a row, the backtrace's
# block edges, one long document
COUNTS = [0, -1, 2, 1, 1, 1, 1, 63, 64, 0, 65, 128, 1, 129, 1500, 1, 0]


@functools.lru_cache(maxsize=None)
def seg_corpus(kind, width, stride):
    data, off, soff = corpus_of(kind, width, stride, COUNTS, 40 + GEOMETRY.index((width, stride)))
    raw, rows, _, _ = oracle(seg_table(kind), seg_L(kind), seg_grams(kind), data, off, width, stride)
    for a in (data, off, soff, raw, rows):
        a.setflags(write=False)
    return data, off, soff, raw, rows


def path_switches(y, soff):
    """Per document the number of label changes along its spans."""
    return [int(np.count_nonzero(np.diff(y[a:b]))) for a, b in zip(soff[:-1], soff[1:])]


def device_segments(m, data, off, width, stride, penalty, extra=0):
    """ldgpu_span_offsets_device + ldgpu_score_segments_device on torch tensors
    and a non-default stream; the byte tensor holds exactly off[-1] bytes.
    -> the labels of `extra` spans more than there are, and the eight sentinel
    entries after them."""
    import torch
    dev = torch.device("cuda", 0)
    n, n_bytes = len(off) - 1, int(off[-1])
    d_bytes = torch.from_numpy(np.array(data[:n_bytes], dtype=np.uint8)).to(dev) if n_bytes else \
        torch.zeros(4, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
    d_soff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    n_spans = int(spans.span_offsets(off, width, stride)[-1]) + extra
    d_lab = torch.full((n_spans + 8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    m.span_offsets_device(d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), stream.cuda_stream)
    m.score_segments_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, width, stride, penalty,
                            d_soff.data_ptr(), n_spans, d_lab.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    out = d_lab.cpu().numpy()
    assert (out[n_spans:] == -7).all(), "a write past n_spans"
    return out[:n_spans]


def assert_labels(got, want, what=""):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10].tolist())


# ------------------------------------------------------ tables x geometry
@pytest.mark.parametrize("width,stride", GEOMETRY, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", TABLES)
def test_labels_equal_the_checker(kind, width, stride):
    data, off, soff, raw, rows = seg_corpus(kind, width, stride)
    m = seg_model(kind)
    if kind == "L300":
        assert "lang_blocks" in m.info()["layout"]
    assert len(np.unique(raw)) >= 4
    for penalty in (0.0, INF) + FINITE[(width, stride)]:
        want = segments.smooth_corpus(rows, soff, penalty)
        sw = path_switches(want, soff)
        # one-span documents keep their span label
        one = np.nonzero(np.diff(soff) == 1)[0]
        assert np.array_equal(want[soff[one]], raw[soff[one]])
        if penalty == INF:
            assert not any(sw)
        elif penalty > 0:
            # the checker's own output first: the penalty does something, and
            # still leaves switches to find
            changed = np.count_nonzero(want != raw) / len(raw)
            print(f"{kind} {(width, stride)} penalty {penalty}: {changed:.1%} of {len(raw)} spans relabelled, "
                  f"{sum(sw)} switches left, {sum(s >= 2 for s in sw)} documents with >= 2")
            assert changed >= 0.05 and max(sw) >= 2
        labels, got_soff = m.score_segments(data, off, width, stride, penalty)
        assert np.array_equal(got_soff, soff)
        assert_labels(labels, want, f"host, penalty {penalty}")
        assert_labels(device_segments(m, data, off, width, stride, penalty), want, f"device, penalty {penalty}")


# ------------------------------------------------------------ chunk cuts
# (looked up on the CPU like FINITE, for the chunk corpora: documents of a few
# spans need a smaller penalty to keep two switches)
CHUNK_FINITE = (1.0, 6.0)


def chunk_counts(c):
    """Span counts around chunks of c spans: a document that ends exactly on a
    chunk boundary, one over three chunks and more, then (c > 1) documents that
    start and end inside chunks -- a chunk one document enters and another
    leaves -- empty and one-span documents between them, and two documents of
    a fixed size (labels change there at every chunk size)."""
    return [c, 3 * c + 2, 2 * c, c + 1, 0, 1, 2 * c + 3, 1, 2, 0, 40, 25]


def chunk_facts(soff, c):
    """(a document boundary on a chunk boundary, the most chunks a document
    touches, a chunk that one document enters and a different one leaves)."""
    n = int(soff[-1])
    on_boundary = any(0 < g < n and g % c == 0 for g in soff.tolist())
    most = max(int((b - 1) // c - a // c + 1) for a, b in zip(soff[:-1], soff[1:]))
    two_rows = False
    for g0 in range(0, n, c):
        g1 = min(g0 + c, n)
        d_in = int(np.searchsorted(soff, g0, side="right")) - 1
        d_out = int(np.searchsorted(soff, g1 - 1, side="right")) - 1
        two_rows |= soff[d_in] < g0 and soff[d_out + 1] > g1 and d_in != d_out
    return on_boundary, most, bool(two_rows)


@pytest.mark.parametrize("kind", ["count", "L130", "L300"])
@pytest.mark.parametrize("chunk", [1, 5, 64])
def test_chunks_carry_dp_between_them(chunk, kind, monkeypatch):
    width, stride = 64, 32
    data, off, soff = corpus_of(kind, width, stride, chunk_counts(chunk), 70 + chunk)
    on_boundary, most, two_rows = chunk_facts(soff, chunk)
    assert on_boundary and most >= 3 and (two_rows or chunk == 1)
    L, grams = seg_L(kind), seg_grams(kind)
    raw, rows, _, _ = oracle(seg_table(kind), L, grams, data, off, width, stride)
    first = [g for g in range(chunk, int(soff[-1]), chunk) if g not in set(soff.tolist())]
    assert len(first) >= 3
    for penalty in (0.0,) + CHUNK_FINITE:
        want = segments.smooth_corpus(rows, soff, penalty)
        sw = path_switches(want, soff)
        stays = int(soff[-1]) - (len(soff) - 1) - sum(sw)
        changed = np.count_nonzero(want != raw) / len(raw)
        assert stays >= 1 and sum(sw) >= 1
        assert penalty == 0.0 or (changed >= 0.05 and max(sw) >= 2), (penalty, changed, sw)
        # at a chunk's first span inside a document -- where t comes from the
        # carried row -- some languages switch and some stay
        for g in first:
            d = int(np.searchsorted(soff, g, side="right")) - 1
            bits = segments.trace(rows[soff[d]:soff[d + 1]], penalty)[0][g - soff[d]]
            assert penalty == 0.0 or (bits.any() and not bits.all()), (penalty, g)
        ref = seg_model(kind).score_segments(data, off, width, stride, penalty)[0]
        assert_labels(ref, want, "product, unchunked")
        monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", str(chunk))
        diag = seg_model(kind, "diag")
        assert_labels(diag.score_segments(data, off, width, stride, penalty)[0], want, f"host, penalty {penalty}")
        assert_labels(device_segments(diag, data, off, width, stride, penalty), want, f"device, penalty {penalty}")
        monkeypatch.delenv("LDGPU_SPAN_CHUNK_SPANS")


# ------------------------------------------------------- non-finite rows
def test_non_finite_rows():
    """+inf, -inf and NaN entries at language 0 and elsewhere, hit in
    consecutive spans: dp rows and t go non-finite and stay defined."""
    L = 6
    row = lambda pairs: [pairs.get(l, 0.0) for l in range(L)]
    table = {b"a": row({0: 1.0, 3: 0.5}), b"b": row({1: 2.0}), b"c": row({2: 1.5, 5: 1.0}), b"d": row({4: 3.0}),
             b"n": row({0: NAN, 1: 1.0}), b"m": row({3: NAN, 2: 1.0}), b"p": row({0: INF}), b"q": row({4: INF, 1: 1.0}),
             b"r": row({0: -INF, 5: 2.0}), b"s": row({2: -INF}), b"z": row({l: -1.0 for l in range(L)})}
    rng = np.random.default_rng(3)
    plain, odd = [b"a", b"b", b"c", b"d", b"z", b" "], [b"n", b"m", b"p", b"q", b"r", b"s"]
    docs = [b"pr", b"rp", b"nnnn", b"abmmcd", b"qqss", b"prprpr", b"aabbqqqqccdd", b"cdssssab", b"", b"n"]
    for _ in range(60):
        n = int(rng.integers(2, 40))
        docs.append(b"".join((odd if rng.random() < 0.12 else plain)[int(rng.integers(0, 6))] for _ in range(n)))
    data, off = encoding.pack(docs)
    m = DeviceModel(table, L, [1])
    for width, stride in ((2, 1), (4, 2)):
        raw, rows, _, _ = oracle(table, L, [1], data, off, width, stride)
        soff = spans.span_offsets(off, width, stride)
        # consecutive spans with a non-finite row, of every kind
        bad = ~np.isfinite(rows).all(axis=1)
        assert np.count_nonzero(bad[1:] & bad[:-1]) >= 20
        assert np.isnan(rows[:, 0]).any() and np.isnan(rows[:, 1:]).any()
        assert np.isposinf(rows[:, 0]).any() and np.isposinf(rows[:, 1:]).any()
        assert np.isneginf(rows[:, 0]).any() and np.isneginf(rows[:, 1:]).any()
        seen = set()
        for penalty in (0.0, 0.75, 2.5, INF):
            want = segments.smooth_corpus(rows, soff, penalty)
            seen.add(tuple(want.tolist()))
            assert_labels(m.score_segments(data, off, width, stride, penalty)[0], want, f"host {penalty}")
            assert_labels(device_segments(m, data, off, width, stride, penalty), want, f"device {penalty}")
        assert len(seen) >= 3


# ---------------------------------------------------------- device form
def test_n_spans_over_estimate_and_no_documents():
    kind, width, stride = "count", 5, 1
    data, off, soff, raw, rows = seg_corpus(kind, width, stride)
    m = seg_model(kind)
    penalty = FINITE[(width, stride)][0]
    want = segments.smooth_corpus(rows, soff, penalty)
    # (device_segments checks the sentinels behind n_spans)
    for extra in (3, 200):
        got = device_segments(m, data, off, width, stride, penalty, extra=extra)
        assert_labels(got[:-extra], want)
        assert not got[-extra:].any()
    assert device_segments(m, data[:0], off[:1], width, stride, penalty).shape == (0,)
    assert device_segments(m, data[:0], off[:1], width, stride, penalty, extra=5).tolist() == [0] * 5
    labels, got_soff = m.score_segments(data[:0], off[:1], width, stride, penalty)
    assert labels.shape == (0,) and got_soff.tolist() == [0]


# -------------------------------------------------------- host pipeline
def pipeline_corpus(kind, seed, n_docs=30):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 40, size=n_docs).tolist()
    counts[3], counts[10] = 0, 150
    return corpus_of(kind, 64, 32, counts, seed)


def test_host_pipeline_pinned_pageable_and_threads(monkeypatch):
    monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", "64")
    kind, width, stride = "count", 64, 32
    penalty = FINITE[(width, stride)][0]
    L, grams = seg_L(kind), seg_grams(kind)
    m = seg_model(kind, "diag")

    def expect(data, off, soff):
        return segments.smooth_corpus(oracle(seg_table(kind), L, grams, data, off, width, stride)[1], soff, penalty)

    data, off, soff = pipeline_corpus(kind, 82)
    want = expect(data, off, soff)
    n = len(want)
    assert n >= 5 * 64
    assert_labels(m.score_segments(data, off, width, stride, penalty)[0], want, "pageable")
    pin = PinnedArray(len(data) + 16, np.uint8)
    pin.array[:len(data)] = data
    pl = PinnedArray(n, np.int32)
    pl.array[:] = -1
    got = m.score_segments(pin.array[:len(data)], off, width, stride, penalty, out_labels=pl.array)[0]
    assert got is pl.array
    assert_labels(pl.array, want, "pinned")
    for p in (pin, pl):
        p.close()

    # two threads on one context (ctypes drops the GIL)
    batches = [pipeline_corpus(kind, 90 + i, 20 + 10 * i) for i in range(2)]
    wants = [expect(*b) for b in batches]
    errors = []

    def run(i):
        try:
            for _ in range(3):
                assert_labels(m.score_segments(batches[i][0], batches[i][1], width, stride, penalty)[0], wants[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_failed_call_leaves_pipeline_clean(monkeypatch):
    """Chunks of whole documents within 5 spans, a failure injected at chunk
    2: the call drains, and the next call on the pooled pipeline is right --
    into a pageable array, then (after another failed call) a pinned one."""
    kind, width, stride = "count", 64, 32
    penalty = FINITE[(width, stride)][1]
    data, off, soff = corpus_of(kind, width, stride, [2, 3, 1, 4, 7, 2, 2, 0, 12, 1, 3], 85)
    rows = oracle(seg_table(kind), seg_L(kind), seg_grams(kind), data, off, width, stride)[1]
    want = segments.smooth_corpus(rows, soff, penalty)
    m = seg_model(kind, "diag")
    monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", "5")
    pl = PinnedArray(len(want), np.int32)
    for out in ({}, {"out_labels": pl.array}):
        monkeypatch.setenv("LDGPU_FAIL_CHUNK", "2")
        with pytest.raises(_lib.LdgpuError, match="injected failure"):
            m.score_segments(data, off, width, stride, penalty)
        monkeypatch.delenv("LDGPU_FAIL_CHUNK")
        pl.array[:] = -1
        assert_labels(m.score_segments(data, off, width, stride, penalty, **out)[0], want,
                      "pinned" if out else "pageable")
    pl.close()


# ----------------------------------------------------------------- errors
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_invalid_arguments_leave_the_outputs_untouched():
    import torch
    m = seg_model("count")
    lib = m.lib
    data, off, soff, _, _ = seg_corpus("count", 5, 1)
    data = np.ascontiguousarray(data)
    n = len(off) - 1
    labels = np.full(int(soff[-1]) + 64, -7, dtype=np.int32)

    def host(width, stride, penalty=1.0, offsets=off, n_docs=n, lab=labels, byt=data, model=m.h):
        return lib.ldgpu_score_segments(model, _ptr(byt), _ptr(np.ascontiguousarray(offsets, dtype=np.int64)), n_docs,
                                        width, stride, penalty, _ptr(lab))

    E, U = _lib.LDGPU_EINVAL, _lib.LDGPU_EUNSUPPORTED
    assert host(5, 1, penalty=-1.0) == E and b"penalty" in lib.ldgpu_last_error()
    assert host(5, 1, penalty=NAN) == E and host(5, 1, penalty=-INF) == E
    assert host(0, 1) == E and host(-1, 1) == E and host(4, 0) == E and host(4, 5) == E
    assert host(1 << 28, 1) == U and b"width" in lib.ldgpu_last_error()
    bad = np.array(off)
    bad[3] = bad[4] + 1
    assert host(4, 2, offsets=bad) == E and b"decrease" in lib.ldgpu_last_error()
    assert host(4, 2, n_docs=-1) == E and host(4, 2, lab=None) == E and host(4, 2, byt=None) == E
    assert host(4, 2, model=None) == E
    assert host(4, 2, n_docs=0, lab=None, byt=None) == _lib.LDGPU_OK
    assert (labels == -7).all()
    with pytest.raises(ValueError, match="penalty"):
        m.score_segments(data, off, 5, 1, -0.5)
    with pytest.raises(ValueError):
        m.score_segments(data, off, 4, 5, 1.0)
    with pytest.raises(NotImplementedError):
        m.score_segments(data, off, 1 << 28, 1, 1.0)

    dev = torch.device("cuda", 0)
    d_bytes = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.array(off)).to(dev)
    d_soff = torch.from_numpy(spans.span_offsets(off, 4, 2)).to(dev)
    d_lab = torch.full((len(labels),), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def device(width, stride, penalty=1.0, p_bytes=d_bytes.data_ptr(), n_docs=n, n_spans=100, p_lab=d_lab.data_ptr(),
               p_off=d_off.data_ptr(), p_soff=d_soff.data_ptr(), model=m.h):
        return lib.ldgpu_score_segments_device(model, ctypes.c_void_p(p_bytes), int(off[-1]),
                                               ctypes.c_void_p(p_off) if p_off else None, n_docs, width, stride,
                                               penalty, ctypes.c_void_p(p_soff) if p_soff else None, n_spans,
                                               ctypes.c_void_p(p_lab) if p_lab else None, ctypes.c_void_p(st))

    assert device(4, 2, penalty=-1.0) == E and b"penalty" in lib.ldgpu_last_error()
    assert device(4, 2, penalty=NAN) == E
    assert device(0, 1) == E and device(4, 0) == E and device(4, 5) == E and device(1 << 28, 1) == U
    assert device(4, 2, n_docs=-1) == E and device(4, 2, n_spans=-1) == E
    assert device(4, 2, p_lab=0) == E and device(4, 2, p_off=0) == E and device(4, 2, p_soff=0) == E
    assert device(4, 2, model=None) == E
    assert device(4, 2, p_bytes=d_bytes.data_ptr() + 1) == E and b"aligned" in lib.ldgpu_last_error()
    torch.cuda.synchronize()
    assert (d_lab.cpu().numpy() == -7).all()
    assert device(4, 2, n_spans=0) == _lib.LDGPU_OK
    assert device(4, 2, n_docs=0, n_spans=0, p_lab=0, p_off=0, p_soff=0) == _lib.LDGPU_OK


def test_wrong_length_row_raises_as_in_the_span_call():
    m = DeviceModel({b"ab": [1.0], b"xy": [0.0, 1.0]}, 2, [2])
    data, off = encoding.pack([b"xyxy", b"zzabzz"])
    assert m.score_segments(data, off, 3, 3, 0.5)[0].tolist() == [1, 1, 0, 0]
    with pytest.raises(ValueError, match="requirement failed"):
        m.score_segments(data, off, 4, 2, 0.5)
    with pytest.raises(ValueError, match="requirement failed"):
        device_segments(m, data, off, 4, 2, 0.5)
    # the error word is cleared: the next calls succeed
    assert m.score_segments(data, off, 3, 3, 0.5)[0].tolist() == [1, 1, 0, 0]
    assert device_segments(m, data, off, 3, 3, 0.5).tolist() == [1, 1, 0, 0]


# ------------------------------------------------------------- Python API
def test_predict_segments_on_a_two_language_text():
    import pandas as pd
    langs = ["xx", "yy"]
    one, two = math.log(2.0), math.log(1.5)
    # "a" grams speak for xx, "b" grams for yy, "c" weakly for both
    grams = {"a": [one, 0.0], "aa": [one, 0.0], "b": [0.0, one], "bb": [0.0, one], "c": [two, two], "ab": [two, two]}
    model = LanguageDetectorModel(gramProbabilities=grams, gramLengths=[1, 2], languages=langs)
    table = {encoding.gram_key(k): v for k, v in grams.items()}
    rng = np.random.default_rng(12)
    noisy = lambda main, other, n: "".join(other if rng.random() < 0.2 else main for _ in range(n))
    texts = [noisy("a", "b", 120) + noisy("b", "a", 120), "ccc", "", noisy("b", "c", 50)]
    width, stride, penalty = 4, 2, 2.5
    found = model.predict_segments(texts, width, stride, penalty)
    rough = model.predict_spans(texts, width, stride)
    for d, text in enumerate(texts):
        data, off = encoding.pack_score([text])
        rows = oracle(table, 2, [1, 2], data, off, width, stride)[1]
        want = segments.smooth(rows, penalty)
        assert found[d] == [(a, b, langs[l]) for a, b, l in spans.runs(len(text), want, width, stride)], d
    assert 2 <= len(found[0]) < len(rough[0]) and found[0][0][2] == "xx" and found[0][-1][2] == "yy"
    assert found[0][0][0] == 0 and found[0][-1][1] == len(texts[0])
    df = pd.DataFrame({"fulltext": texts})
    out = model.transformSegments(df, width, stride, penalty)
    assert list(out.columns) == ["fulltext", "langSegments"] and list(out["langSegments"]) == found
    assert list(model.transformSegments(df, width, stride, penalty, outputCol="runs").columns) == ["fulltext", "runs"]
    with pytest.raises(ValueError, match="Column langSegments already exists"):
        model.transformSegments(out, width, stride, penalty)
    with pytest.raises(ValueError, match="does not exist"):
        model.transformSegments(pd.DataFrame({"text": texts}), width, stride, penalty)
    with pytest.raises(ValueError, match="penalty"):
        model.predict_segments(texts, width, stride, -1.0)
