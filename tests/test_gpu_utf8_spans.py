"""Top-k, spans and segments of UTF-8 documents (ldgpu_span_offsets_utf,
ldgpu_score_topk_utf, ldgpu_score_spans_utf, ldgpu_score_segments_utf and their
_device forms): the span offsets, unit counts and byte starts against the numpy
checker languagedetection.utf8.span_geometry, the labels and fp64 score bits
against the non-UTF twins on encoding.pack_score of the decoded texts."""
import ctypes
import functools

import numpy as np
import pytest

import bytecorpus as B
import utf8corpus
from languagedetection import LanguageDetectorModel, _lib, encoding, utf8
from languagedetection.runtime import DeviceModel, PinnedArray

pytestmark = pytest.mark.gpu

S = utf8.STEP_BYTES
SEED = 11
SEQS = [b"a"] + utf8corpus.VALID_SEQS     # sequence lengths 1-4
GRIN = utf8corpus.VALID_SEQS[2]
ILL = [b"\xe2\x82", b"\xc0\x80", b"ab\xff", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"x" * 300 + b"\xf0\x9f\x98"]
GEOMETRIES = [(1, 1), (2, 1), (3, 2), (5, 3), (7, 7), (64, 32), (300, 257), (1000, 999)]
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def filler(n, k=0):
    return bytes(97 + (i + k) % 26 for i in range(n))


def pack_behind(docs, lead=b""):
    """`docs` packed behind `lead`: offsets[0] = len(lead)."""
    data, off = utf8.pack_utf8([lead] + list(docs))
    return data, off[1:]


# ----------------------------------------------------------------- geometry
@functools.lru_cache(maxsize=None)
def tiny_model(variant="product"):
    table = {b"ab": [0.5, 0.0], b"x": [0.0, 0.25], b"\xe9": [0.0, 1.0], b"\x00": [0.75, 0.0]}
    return DeviceModel(table, 2, [1, 2], variant=variant)


def boundary_docs():
    """A sequence of every length at every byte position around the decoder's
    step and twice the step, whole and cut after each of its bytes."""
    docs = []
    for around in (S, 2 * S):
        for p in range(around - 4, around + 2):
            for k, seq in enumerate(SEQS):
                docs.append(filler(p, k) + seq + filler(7, p))
                docs += [filler(p, k) + seq[:cut] for cut in range(1, len(seq) + 1)]
    return docs


def at_base(docs, base):
    """Every document of `docs` starting at `base` mod 4, behind padding
    documents of stray continuation bytes."""
    out, at = [], 0
    for d in docs:
        pad = b"\x80" * ((base - at) % 4)
        out += [pad, d]
        at += len(pad) + len(d)
    return out


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """[(documents, the bytes in front of offsets[0])]."""
    cases = [(utf8corpus.small_sequences(), b"")]
    cases += [(at_base(boundary_docs(), base), b"") for base in range(4)]
    # 4-byte characters only, one more than three quarters of a step's bytes hold, behind 0..3 bytes
    assert (3 * S) % 4 == 0
    cases += [([GRIN * (3 * S // 4 + 1), (GRIN * S)[:3 * S + 1], GRIN * (3 * S // 4)], b"q" * k) for k in range(4)]
    # offsets[0] > 0, a stray lead before it that would claim the first document's bytes
    cases += [([b"\x9f\x98\x80abc", b"abc", GRIN[1:], GRIN * 40 + b"z"], lead)
              for lead in (b"\xf0", b"zz\xe2", b"\xc3\xa9\xf0\x9f\x98")]
    # empty documents at both ends, and around an ill-formed one
    good = "Grüße, κόσμε €😀".encode("utf-8")
    cases.append(([b"", good, b"", b"\xc3(", b"", good * 30, b""], b""))
    return cases


def check_geometry(m, docs, lead, width, stride):
    data, off = pack_behind(docs, lead)
    want_soff, want_units, want_starts = utf8.span_geometry(data, off, width, stride)
    soff, units = m.span_offsets_utf8(data, off, width, stride)
    assert np.array_equal(soff, want_soff) and np.array_equal(units, want_units)
    labels, _, starts, _ = m.score_spans_utf8(data, off, width, stride, span_offsets=soff)
    assert np.array_equal(starts, want_starts)
    bad = np.flatnonzero(want_units < 0)
    assert (labels[want_soff[bad]] == -1).all() and (labels >= 0).sum() == len(labels) - len(bad)


@pytest.mark.parametrize("width,stride", GEOMETRIES)
def test_geometry(width, stride):
    m = tiny_model()
    for docs, lead in geometry_cases():
        check_geometry(m, docs, lead, width, stride)
    # no documents
    for offs in ([0], [5]):
        soff, units = m.span_offsets_utf8(np.zeros(8, np.uint8), np.array(offs, dtype=np.int64), width, stride)
        assert soff.tolist() == [0] and len(units) == 0
        labels, _, starts, _ = m.score_spans_utf8(np.zeros(8, np.uint8), np.array(offs, dtype=np.int64), width, stride)
        assert len(labels) == 0 and len(starts) == 0


# ------------------------------------------------------------------- parity
# (name: L, gram lengths, key lengths, table form, check of DeviceModel.info())
TABLES = {
    # an order-free table: hit counts per language
    "count": (20, (1, 2, 3), (1, 2, 3), "uniform",
              lambda i: i["mode"] == 2 and "lds_bloom" in i["layout"] and "classes" not in i["layout"]),
    # an ordered table: dense fp64 rows added in window order
    "dense": (9, (1, 2, 3), (1, 2, 3), "dense",
              lambda i: i["mode"] == 1 and not {"trie", "classes", "general_keys"} & set(i["layout"])),
}
PARITY_GEOMETRY = [(64, 32), (5, 3)]


@functools.lru_cache(maxsize=None)
def model(kind, variant="product"):
    L, grams, key_lens, form, ok = TABLES[kind]
    m = DeviceModel(B.byte_table(SEED, L, list(key_lens), 300, form), L, list(grams), variant=variant)
    assert ok(m.info()), (kind, m.info())
    return m


@functools.lru_cache(maxsize=None)
def corpus(kind, n_docs=300):
    """(texts, their UTF-8 documents with ill-formed ones interleaved, the
    index of every text's document, the ill-formed documents' indices)."""
    L = TABLES[kind][0]
    _, texts = B.texts(SEED, L, n_docs, 0, 180)
    docs, where, bad = [], [], []
    for i, t in enumerate(texts):
        if i % 9 == 0 or i == n_docs - 1:
            bad.append(len(docs))
            docs.append(ILL[len(bad) % len(ILL)])
        where.append(len(docs))
        docs.append(t.encode("utf-8"))
    bad.append(len(docs))
    docs.append(ILL[0])
    assert max(len(d) for d in docs) <= 700 and sum(not t.isascii() for t in texts) > 0.8 * n_docs
    return texts, docs, np.array(where), np.array(bad)


@functools.lru_cache(maxsize=None)
def empty_row(kind):
    row = model(kind).score(*encoding.pack([b""]), want_scores=True)[1][0]
    row.setflags(write=False)
    return row


def spliced(kind, soff_units, per_span, fill):
    """The twin's per-span array over the texts laid out over the documents of
    corpus(kind): the ill-formed documents' single spans hold `fill`."""
    _, docs, where, bad = corpus(kind)
    counts = np.ones(len(docs), dtype=np.int64)
    counts[where] = np.diff(soff_units)
    soff = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum(counts, out=soff[1:])
    out = np.empty((int(soff[-1]),) + per_span.shape[1:], dtype=per_span.dtype)
    out[soff[bad]] = fill
    keep = np.ones(len(out), dtype=bool)
    keep[soff[bad]] = False
    out[keep] = per_span
    return soff, out


@functools.lru_cache(maxsize=None)
def span_reference(kind, width, stride):
    """(span_offsets, labels, scores) the UTF form must give on corpus(kind)."""
    texts = corpus(kind)[0]
    labels, scores, soff_units = model(kind).score_spans(*encoding.pack_score(texts), width, stride, want_scores=True)
    soff, lab = spliced(kind, soff_units, labels, -1)
    _, sc = spliced(kind, soff_units, scores, empty_row(kind))
    for a in (soff, lab, sc):
        a.setflags(write=False)
    return soff, lab, sc


@pytest.mark.parametrize("width,stride", PARITY_GEOMETRY)
@pytest.mark.parametrize("kind", ["count", "dense"])
def test_spans_parity(kind, width, stride):
    m = model(kind)
    _, docs, _, bad = corpus(kind)
    data, off = utf8.pack_utf8(docs)
    want_soff, want_l, want_s = span_reference(kind, width, stride)
    soff, units = m.span_offsets_utf8(data, off, width, stride)
    assert np.array_equal(soff, want_soff) and np.flatnonzero(units < 0).tolist() == bad.tolist()
    labels, scores, starts, _ = m.score_spans_utf8(data, off, width, stride, want_scores=True, span_offsets=soff)
    assert np.array_equal(labels, want_l) and np.array_equal(bits(scores), bits(want_s))
    assert np.array_equal(starts, utf8.span_geometry(data, off, width, stride)[2])
    # labels only, and without starts
    labels, scores, starts, _ = m.score_spans_utf8(data, off, width, stride, want_starts=False)
    assert np.array_equal(labels, want_l) and scores is None and starts is None


@pytest.mark.parametrize("penalty", [0.0, 6.0, INF])
@pytest.mark.parametrize("kind", ["count", "dense"])
def test_segments_parity(kind, penalty):
    width, stride = 64, 32
    m = model(kind)
    texts, docs, _, _ = corpus(kind)
    data, off = utf8.pack_utf8(docs)
    twin, soff_units = m.score_segments(*encoding.pack_score(texts), width, stride, penalty)
    want_soff, want_l = spliced(kind, soff_units, twin, -1)
    labels, starts, soff = m.score_segments_utf8(data, off, width, stride, penalty)
    assert np.array_equal(soff, want_soff) and np.array_equal(labels, want_l)
    assert np.array_equal(starts, utf8.span_geometry(data, off, width, stride)[2])


@pytest.mark.parametrize("kind", ["count", "dense"])
def test_topk_parity(kind):
    m = model(kind)
    L = TABLES[kind][0]
    texts, docs, where, bad = corpus(kind)
    data, off = utf8.pack_utf8(docs)
    for k in sorted({1, min(L, 3), min(L, 16)}):
        twin_l, twin_s = m.score_topk(*encoding.pack_score(texts), k)
        labels, scores = m.score_topk_utf8(data, off, k)
        assert np.array_equal(labels[where], twin_l) and np.array_equal(bits(scores[where]), bits(twin_s))
        assert (labels[bad] == -1).all() and np.array_equal(bits(scores[bad]), bits(np.zeros((len(bad), k))))
        assert np.array_equal(m.score_topk_utf8(data, off, k, want_scores=False)[0], labels)


# --------------------------------------------------------------- chunk cuts
@pytest.mark.parametrize("kind", ["count", "dense"])
def test_chunk_cuts(kind, monkeypatch):
    """The diagnostics library with chunks of a few documents and a few spans:
    outputs of the host and the device forms identical to the uncut host
    call; one document has more spans than the budget."""
    import torch
    width, stride = 3, 2
    _, docs, _, _ = corpus(kind)
    docs = docs[:24]
    data, off = utf8.pack_utf8(docs)
    m, md = model(kind), model(kind, "diag")
    soff, units = m.span_offsets_utf8(data, off, width, stride)
    assert np.diff(soff).max() > 64
    want = m.score_spans_utf8(data, off, width, stride, want_scores=True, span_offsets=soff)
    want_seg = m.score_segments_utf8(data, off, width, stride, 2.0, span_offsets=soff)
    want_top = m.score_topk_utf8(data, off, 3)
    for budget in (1, 5, 64):
        monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", str(budget))
        got = md.score_spans_utf8(data, off, width, stride, want_scores=True, span_offsets=soff)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        assert np.array_equal(got[2], want[2])
        got = md.score_segments_utf8(data, off, width, stride, 2.0, span_offsets=soff)
        assert np.array_equal(got[0], want_seg[0]) and np.array_equal(got[1], want_seg[1])
    monkeypatch.delenv("LDGPU_SPAN_CHUNK_SPANS")
    for chunk in (1, 3):
        monkeypatch.setenv("LDGPU_SCORE_CHUNK_DOCS", str(chunk))
        got = md.score_topk_utf8(data, off, 3)
        assert np.array_equal(got[0], want_top[0]) and np.array_equal(bits(got[1]), bits(want_top[1]))
    monkeypatch.delenv("LDGPU_SCORE_CHUNK_DOCS")
    # the device forms under the same cuts
    dev = torch.device("cuda", 0)
    L, n, ns = TABLES[kind][0], len(docs), int(soff[-1])
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        d_data, d_off, d_soff = (torch.from_numpy(np.array(a)).to(dev) for a in (data, off, soff))
        for budget in (1, 5, 64):
            monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", str(budget))
            d_lab = torch.full((ns,), -7, dtype=torch.int32, device=dev)
            d_sc = torch.full((ns, L), -7.0, dtype=torch.float64, device=dev)
            d_sta = torch.full((ns,), -7, dtype=torch.int64, device=dev)
            md.score_spans_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride,
                                       d_soff.data_ptr(), ns, d_lab.data_ptr(), d_sc.data_ptr(), d_sta.data_ptr(),
                                       stream=st)
            d_seg = torch.full((ns,), -7, dtype=torch.int32, device=dev)
            d_seg_sta = torch.full((ns,), -7, dtype=torch.int64, device=dev)
            md.score_segments_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride, 2.0,
                                          d_soff.data_ptr(), ns, d_seg.data_ptr(), d_seg_sta.data_ptr(), stream=st)
            stream.synchronize()
            assert np.array_equal(d_lab.cpu().numpy(), want[0]) and np.array_equal(d_sta.cpu().numpy(), want[2])
            assert np.array_equal(bits(d_sc.cpu().numpy()), bits(want[1]))
            assert np.array_equal(d_seg.cpu().numpy(), want_seg[0])
            assert np.array_equal(d_seg_sta.cpu().numpy(), want_seg[1])
        monkeypatch.delenv("LDGPU_SPAN_CHUNK_SPANS")
        for chunk in (1, 3):
            monkeypatch.setenv("LDGPU_TOPK_CHUNK_DOCS", str(chunk))
            d_top = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
            d_top_s = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
            md.score_topk_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, 3, d_top.data_ptr(),
                                      d_top_s.data_ptr(), stream=st)
            stream.synchronize()
            assert np.array_equal(d_top.cpu().numpy(), want_top[0])
            assert np.array_equal(bits(d_top_s.cpu().numpy()), bits(want_top[1]))
        monkeypatch.delenv("LDGPU_TOPK_CHUNK_DOCS")


# ------------------------------------------------------------- device forms
def pinned(a):
    p = PinnedArray(a.shape, a.dtype)
    p.array[...] = a
    return p


@pytest.mark.parametrize("kind", ["count", "dense"])
def test_device_forms(kind):
    import torch
    width, stride, extra = 64, 32, 7
    m = model(kind)
    L = TABLES[kind][0]
    _, docs, _, bad = corpus(kind)
    data, off = utf8.pack_utf8(docs)
    n = len(docs)
    want_soff, want_l, want_s = span_reference(kind, width, stride)
    want_starts = utf8.span_geometry(data, off, width, stride)[2]
    want_units = utf8.span_geometry(data, off, width, stride)[1]
    want_seg = m.score_segments_utf8(data, off, width, stride, 6.0)[0]
    want_top = m.score_topk_utf8(data, off, 3)
    ns = int(want_soff[-1])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        d_data, d_off = torch.from_numpy(np.array(data)).to(dev), torch.from_numpy(np.array(off)).to(dev)
        d_soff = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        d_units = torch.full((n,), -7, dtype=torch.int64, device=dev)
        d_soff2 = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        m.span_offsets_utf8_device(d_data.data_ptr(), d_off.data_ptr(), n, width, stride, d_soff.data_ptr(),
                                   d_units.data_ptr(), stream=st)
        m.span_offsets_utf8_device(d_data.data_ptr(), d_off.data_ptr(), n, width, stride, d_soff2.data_ptr(), stream=st)
        d_lab = torch.full((ns + extra,), -7, dtype=torch.int32, device=dev)
        d_sc = torch.full((ns + extra, L), -7.0, dtype=torch.float64, device=dev)
        d_sta = torch.full((ns + extra,), -7, dtype=torch.int64, device=dev)
        m.score_spans_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride, d_soff.data_ptr(),
                                  ns + extra, d_lab.data_ptr(), d_sc.data_ptr(), d_sta.data_ptr(), stream=st)
        # d_scores NULL and d_starts NULL
        d_lab2 = torch.full((ns,), -7, dtype=torch.int32, device=dev)
        m.score_spans_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride, d_soff.data_ptr(),
                                  ns, d_lab2.data_ptr(), stream=st)
        d_seg = torch.full((ns + extra,), -7, dtype=torch.int32, device=dev)
        d_seg_sta = torch.full((ns + extra,), -7, dtype=torch.int64, device=dev)
        m.score_segments_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride, 6.0,
                                     d_soff.data_ptr(), ns + extra, d_seg.data_ptr(), d_seg_sta.data_ptr(), stream=st)
        d_seg2 = torch.full((ns,), -7, dtype=torch.int32, device=dev)
        m.score_segments_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, width, stride, 6.0,
                                     d_soff.data_ptr(), ns, d_seg2.data_ptr(), stream=st)
        d_top = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
        d_top_s = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
        d_top2 = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
        m.score_topk_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, 3, d_top.data_ptr(),
                                 d_top_s.data_ptr(), stream=st)
        m.score_topk_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, 3, d_top2.data_ptr(), stream=st)
    stream.synchronize()
    assert np.array_equal(d_soff.cpu().numpy(), want_soff) and np.array_equal(d_soff2.cpu().numpy(), want_soff)
    assert np.array_equal(d_units.cpu().numpy(), want_units)
    lab, sta = d_lab.cpu().numpy(), d_sta.cpu().numpy()
    assert np.array_equal(lab[:ns], want_l) and np.array_equal(bits(d_sc.cpu().numpy()[:ns]), bits(want_s))
    assert np.array_equal(sta[:ns], want_starts)
    assert (lab[ns:] == 0).all() and (sta[ns:] == 0).all()          # the over-estimate's tail
    assert np.array_equal(d_lab2.cpu().numpy(), want_l)
    seg, seg_sta = d_seg.cpu().numpy(), d_seg_sta.cpu().numpy()
    assert np.array_equal(seg[:ns], want_seg) and np.array_equal(seg_sta[:ns], want_starts)
    assert (seg[ns:] == 0).all() and (seg_sta[ns:] == 0).all()
    assert np.array_equal(d_seg2.cpu().numpy(), want_seg)
    assert np.array_equal(d_top.cpu().numpy(), want_top[0]) and np.array_equal(d_top2.cpu().numpy(), want_top[0])
    assert np.array_equal(bits(d_top_s.cpu().numpy()), bits(want_top[1]))
    # the host forms over page-locked buffers: copied from / to directly
    pd, po = pinned(data), pinned(off)
    pl, ps, pt = PinnedArray(ns, np.int32), PinnedArray((ns, L), np.float64), PinnedArray(ns, np.int64)
    pl.array[:], ps.array[:], pt.array[:] = -7, -7.0, -7
    got = m.score_spans_utf8(pd.array, po.array, width, stride, want_scores=True, span_offsets=want_soff,
                             out_labels=pl.array, out_scores=ps.array, out_starts=pt.array)
    assert got[0] is pl.array and got[2] is pt.array
    assert np.array_equal(pl.array, want_l) and np.array_equal(bits(ps.array), bits(want_s))
    assert np.array_equal(pt.array, want_starts)
    pl.array[:], pt.array[:] = -7, -7
    m.score_segments_utf8(pd.array, po.array, width, stride, 6.0, span_offsets=want_soff, out_labels=pl.array,
                          out_starts=pt.array)
    assert np.array_equal(pl.array, want_seg) and np.array_equal(pt.array, want_starts)
    for p in (pd, po, pl, ps, pt):
        p.close()


# ------------------------------------------------------------------- errors
def test_argument_checks():
    import torch
    lib = _lib.load()
    ctx = _lib.context(0)
    m = model("count")
    L = TABLES["count"][0]
    E, U, OK = _lib.LDGPU_EINVAL, _lib.LDGPU_EUNSUPPORTED, _lib.LDGPU_OK
    c = ctypes.c_void_p

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    data, off = utf8.pack_utf8([b"abcdefg", b"\xc3\xa9", b"", b"\xff"])
    soff, units = np.zeros(5, np.int64), np.zeros(4, np.int64)

    def so(ctx=ctx, data=data, off=off, n=4, w=4, s=2, soff=soff, units=units):
        return lib.ldgpu_span_offsets_utf(ctx, ptr(data), ptr(off), n, w, s, ptr(soff), ptr(units))

    assert so() == OK and soff.tolist() == [0, 3, 4, 5, 6] and units.tolist() == [7, 1, 0, -1]
    assert so(units=None) == OK
    assert so(w=0) == E and so(s=0) == E and so(s=5) == E and b"stride" in lib.ldgpu_last_error()
    assert so(w=1 << 28, s=1) == U
    assert so(ctx=None) == E and so(soff=None) == E and so(data=None) == E and so(off=None) == E and so(n=-1) == E
    assert so(off=np.array([0, 3, 2, 4, 4], dtype=np.int64)) == E and b"decrease" in lib.ldgpu_last_error()
    assert so(n=0, data=None) == OK and soff[0] == 0
    assert so() == OK and soff.tolist() == [0, 3, 4, 5, 6]
    ns = 6
    lab, sta, sc = np.zeros(ns, np.int32), np.zeros(ns, np.int64), np.zeros((ns, L))

    def sp(model=m.h, data=data, off=off, n=4, w=4, s=2, soff=soff, lab=lab, sc=None, sta=sta):
        return lib.ldgpu_score_spans_utf(model, ptr(data), ptr(off), n, w, s, ptr(soff), ptr(lab), ptr(sc), ptr(sta))

    def sg(model=m.h, data=data, off=off, n=4, w=4, s=2, pen=1.0, soff=soff, lab=lab, sta=sta):
        return lib.ldgpu_score_segments_utf(model, ptr(data), ptr(off), n, w, s, pen, ptr(soff), ptr(lab), ptr(sta))

    for f in (sp, sg):
        assert f() == OK and sta.tolist() == [0, 2, 4, 0, 0, 0] and lab[5] == -1 and (lab[:5] >= 0).all()
        assert f(w=0) == E and f(s=0) == E and f(s=5) == E and f(w=1 << 28, s=1) == U
        assert f(model=None) == E and f(lab=None) == E and f(data=None) == E and f(off=None) == E and f(n=-1) == E
        assert f(soff=None) == E and b"span_offsets" in lib.ldgpu_last_error()
        assert f(soff=np.array([0, 3, 2, 5, 6], dtype=np.int64)) == E and b"span_offsets" in lib.ldgpu_last_error()
        assert f(soff=np.array([1, 3, 4, 5, 6], dtype=np.int64)) == E
        assert f(soff=np.array([0, 3, 3, 5, 6], dtype=np.int64)) == E        # a document without a span
        assert f(n=0, lab=None, data=None, soff=None) == OK
        assert f(sta=None) == OK
        assert f() == OK                                                      # a later good call succeeds
    assert sp(sc=sc) == OK
    assert sg(pen=float("nan")) == E and sg(pen=-1.0) == E and b"penalty" in lib.ldgpu_last_error()
    assert sg(pen=INF) == OK

    top, top_s = np.zeros((4, 16), np.int32), np.zeros((4, 16))

    def tk(model=m.h, data=data, off=off, n=4, k=2, top=top, top_s=top_s):
        return lib.ldgpu_score_topk_utf(model, ptr(data), ptr(off), n, k, ptr(top), ptr(top_s))

    assert tk() == OK and top.reshape(-1)[6:8].tolist() == [-1, -1]
    assert tk(k=0) == E and tk(k=17) == E and tk(k=-1) == E and b"k =" in lib.ldgpu_last_error()
    assert tk(k=min(L, 16)) == OK
    assert tk(model=None) == E and tk(top=None) == E and tk(data=None) == E and tk(off=None) == E and tk(n=-1) == E
    assert tk(off=np.array([0, 2, 2 + (1 << 28), 3 + (1 << 28), 3 + (1 << 28)], dtype=np.int64)) == U
    assert tk(top_s=None) == OK and tk(n=0, top=None, data=None) == OK

    dev = torch.device("cuda", 0)
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    d[:len(data)] = torch.from_numpy(np.array(data))
    d_off, d_soff = torch.from_numpy(off).to(dev), torch.from_numpy(soff).to(dev)
    d_lab = torch.zeros(64, dtype=torch.int32, device=dev)
    d_sta = torch.zeros(16, dtype=torch.int64, device=dev)
    d_o = torch.zeros(8, dtype=torch.int64, device=dev)

    def dso(ctx=ctx, p=d.data_ptr(), off=d_off.data_ptr(), n=4, w=4, s=2, soff=d_o.data_ptr()):
        return lib.ldgpu_span_offsets_utf_device(ctx, c(p), c(off), n, w, s, c(soff), None, None)

    assert dso() == OK
    assert dso(ctx=None) == E and dso(n=-1) == E and dso(off=0) == E and dso(soff=0) == E and dso(s=9) == E
    assert dso(p=d.data_ptr() + 1) == E and b"aligned" in lib.ldgpu_last_error()
    assert dso(n=2 ** 31 - 1) == U

    def dsp(model=m.h, p=d.data_ptr(), nb=16, off=d_off.data_ptr(), n=4, w=4, s=2, soff=d_soff.data_ptr(), ns=6,
            lab=d_lab.data_ptr(), sta=d_sta.data_ptr()):
        return lib.ldgpu_score_spans_utf_device(model, c(p), nb, c(off), n, w, s, c(soff), ns, c(lab), None, c(sta), None)

    def dsg(model=m.h, p=d.data_ptr(), nb=16, off=d_off.data_ptr(), n=4, w=4, s=2, pen=1.0, soff=d_soff.data_ptr(),
            ns=6, lab=d_lab.data_ptr(), sta=d_sta.data_ptr()):
        return lib.ldgpu_score_segments_utf_device(model, c(p), nb, c(off), n, w, s, pen, c(soff), ns, c(lab), c(sta),
                                                   None)

    for f in (dsp, dsg):
        assert f() == OK
        assert f(model=None) == E and f(n=-1) == E and f(nb=-1) == E and f(ns=-1) == E and f(w=0) == E and f(s=5) == E
        assert f(off=0) == E and f(soff=0) == E and f(lab=0) == E and f(p=0) == E
        assert f(p=d.data_ptr() + 2) == E and b"aligned" in lib.ldgpu_last_error()
        assert f(n=2 ** 31 - 1) == U
        assert f(ns=0, off=0, soff=0, lab=0) == OK and f(sta=0) == OK and f() == OK
    assert dsg(pen=-0.5) == E and dsg(pen=float("nan")) == E

    def dtk(model=m.h, p=d.data_ptr(), nb=16, off=d_off.data_ptr(), n=4, k=2, top=d_lab.data_ptr()):
        return lib.ldgpu_score_topk_utf_device(model, c(p), nb, c(off), n, k, c(top), None, None)

    assert dtk() == OK
    assert dtk(model=None) == E and dtk(n=-1) == E and dtk(nb=-1) == E and dtk(k=0) == E and dtk(k=17) == E
    assert dtk(off=0) == E and dtk(top=0) == E and dtk(p=0) == E and dtk(p=d.data_ptr() + 3) == E
    assert dtk(n=2 ** 31 - 1) == U and dtk(n=0, off=0, top=0) == OK and dtk() == OK
    torch.cuda.synchronize()
    assert d_sta.cpu().numpy()[:6].tolist() == [0, 2, 4, 0, 0, 0] and d_lab.cpu().numpy()[:8].tolist()[6:8] == [-1, -1]


# ---------------------------------------------------------------------- API
def test_python_api():
    import pandas as pd
    kind = "count"
    L, grams, key_lens, form, _ = TABLES[kind]
    texts = list(corpus(kind)[0][:120])
    docs = [t.encode("utf-8") for t in texts]
    lm = LanguageDetectorModel(B.byte_table(SEED, L, list(key_lens), 300, form), list(grams),
                               [f"l{i}" for i in range(L)], device=0)
    width, stride = 16, 8
    assert lm.predict_spans_utf8(docs, width, stride, coords="units") == lm.predict_spans(texts, width, stride)
    assert lm.predict_segments_utf8(docs, width, stride, 2.0, coords="units") == \
        lm.predict_segments(texts, width, stride, 2.0)
    assert lm.predict_spans_utf8(utf8.pack_utf8(docs), width, stride, coords="units") == \
        lm.predict_spans(texts, width, stride)
    for runs in (lm.predict_spans_utf8(docs, width, stride), lm.predict_segments_utf8(docs, width, stride, 2.0)):
        for doc, text, r in zip(docs, texts, runs):
            assert "".join(doc[a:b].decode("utf-8") for a, b, _ in r) == text
            assert b"".join(doc[a:b] for a, b, _ in r) == doc and all(lang.startswith("l") for _, _, lang in r)
    bad = [0, 17, 119]
    docs2 = list(docs)
    for i, ill in zip(bad, ILL):
        docs2[i] = docs2[i][:40] + ill + b"\xff"
    for call in (lambda **kw: lm.predict_spans_utf8(docs2, width, stride, **kw),
                 lambda **kw: lm.predict_segments_utf8(docs2, width, stride, 2.0, **kw)):
        with pytest.raises(UnicodeDecodeError) as e:
            call()
        assert e.value.object == docs2[0]
        got = call(errors="skip")
        assert [i for i, r in enumerate(got) if r is None] == bad
        with pytest.raises(ValueError):
            call(errors="replace")
        with pytest.raises(ValueError):
            call(coords="chars")
    got = lm.predict_spans_utf8(docs2, width, stride, errors="skip")
    want = lm.predict_spans_utf8(docs, width, stride)
    assert all(g == w for i, (g, w) in enumerate(zip(got, want)) if i not in bad)
    # top-k
    want_l, want_s = lm.predict_topk([d.decode("utf-8", "replace") for d in docs2], 3)
    got_l, got_s = lm.predict_topk_utf8(docs2, 3)
    assert got_l == want_l and np.array_equal(bits(got_s), bits(want_s))
    with pytest.raises(UnicodeDecodeError):
        lm.predict_topk_utf8(docs2, 3, errors="strict")
    got_l, got_s = lm.predict_topk_utf8(docs, 3, errors="strict")
    want_l, want_s = lm.predict_topk(texts, 3)
    assert got_l == want_l and np.array_equal(bits(got_s), bits(want_s))
    # the three transforms
    df = pd.DataFrame({"fulltext": docs, "id": range(len(docs))})
    out = lm.transformTopKUtf8(df, 3)
    assert list(out.columns) == ["fulltext", "id", "lang_candidates", "lang_scores"]
    assert list(out["lang_candidates"]) == want_l
    out_s = lm.transformSpansUtf8(df, width, stride)
    assert list(out_s.columns) == ["fulltext", "id", "langSpans"] and list(out_s["langSpans"]) == want
    out_g = lm.transformSegmentsUtf8(df, width, stride, 2.0, coords="units")
    assert list(out_g["langSegments"]) == lm.predict_segments(texts, width, stride, 2.0)
    strings = pd.DataFrame({"fulltext": ["text"]})
    for call, frame in ((lambda f: lm.transformTopKUtf8(f, 3), out), (lambda f: lm.transformSpansUtf8(f, width, stride), out_s),
                        (lambda f: lm.transformSegmentsUtf8(f, width, stride, 2.0), out_g)):
        with pytest.raises(ValueError, match="already exists"):
            call(frame)
        with pytest.raises(ValueError, match="BinaryType"):
            call(strings)
