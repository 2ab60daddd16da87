"""SCORE's per-span output (ldgpu_score_spans / ldgpu_score_spans_device)
against the C oracle applied to languagedetection.spans.materialise: every
span scored as a document of its own, labels exact, scores bit for bit."""
import ctypes
import functools
import json
import math
import os
import threading

import numpy as np
import pytest

import geometry as G
import ldoracle as O
import ldoracle_c as OC
from conftest import GOLDEN
from languagedetection import LanguageDetectorModel, _lib, encoding, spans, synth
from languagedetection.runtime import DeviceModel, PinnedArray
from test_gpu_topk import ALPHABET, make_table

pytestmark = pytest.mark.gpu

AB = np.frombuffer(b"ab ", dtype=np.uint8)


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle(table, L, grams, data, off, width, stride):
    """(labels, scores, span data, span byte offsets) of the materialised spans."""
    sd, so = spans.materialise(data, off, width, stride)
    ol, os_ = OC.Table(table, L).score(list(grams), sd, so, want_scores=True, nthreads=8)
    return ol, os_, sd, so


def device_spans(m, data, off, width, stride, want_scores=True, extra=0):
    """ldgpu_span_offsets_device + ldgpu_score_spans_device on torch tensors and
    a non-default stream.  The byte tensor holds exactly off[-1] bytes: a read
    past n_bytes leaves the allocation's used part.  -> (labels, scores, span
    offsets), with `extra` spans more than there are."""
    import torch
    dev = torch.device("cuda", 0)
    n, n_bytes = len(off) - 1, int(off[-1])
    d_bytes = torch.from_numpy(np.array(data[:n_bytes], dtype=np.uint8)).to(dev) if n_bytes else \
        torch.zeros(4, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
    d_soff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    n_spans = int(spans.span_offsets(off, width, stride)[-1]) + extra
    d_lab = torch.full((n_spans,), -7, dtype=torch.int32, device=dev)
    d_sc = torch.full((n_spans, m.L), -1.0, dtype=torch.float64, device=dev) if want_scores else None
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    m.span_offsets_device(d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), stream.cuda_stream)
    m.score_spans_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), n_spans,
                         d_lab.data_ptr(), d_sc.data_ptr() if want_scores else 0, stream.cuda_stream)
    stream.synchronize()
    return d_lab.cpu().numpy(), d_sc.cpu().numpy() if want_scores else None, d_soff.cpu().numpy()


def assert_spans(got, ol, os_, what=""):
    labels, scores = got[0], got[1]
    assert labels.dtype == np.int32 and labels.shape == ol.shape, what
    assert np.array_equal(labels, ol), (what, np.nonzero(labels != ol)[0][:10].tolist())
    if scores is not None:
        assert scores.shape == os_.shape and np.array_equal(bits(scores), bits(os_)), what


# ------------------------------------------------------------------ golden
@pytest.mark.parametrize("width,stride", [(3, 1), (4, 2)])
def test_reference_score_kat(width, stride):
    kat = load("reference_kats.json")["score_kat"]
    table = {encoding.gram_key(k): v for k, v in kat["table"].items()}
    data, off = encoding.pack_score(kat["docs"])
    ol, os_, _, _ = oracle(table, 2, kat["gram_lengths"], data, off, width, stride)
    assert set(ol.tolist()) == {0, 1}
    m = DeviceModel(table, 2, kat["gram_lengths"])
    labels, scores, soff = m.score_spans(data, off, width, stride, want_scores=True)
    assert np.array_equal(soff, spans.span_offsets(off, width, stride))
    assert_spans((labels, scores), ol, os_)
    assert_spans(m.score_spans(data, off, width, stride), ol, os_)
    assert_spans(device_spans(m, data, off, width, stride), ol, os_)
    # the span that is exactly a key carries its language, its neighbours none
    assert labels[soff[2]] == 1 and labels[soff[0]] == 0 and scores[soff[2]].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("case", load("score_cases.json"), ids=lambda c: c["name"])
def test_golden_cases(case):
    table = {bytes.fromhex(k): [float.fromhex(v) for v in row] for k, row in case["table"]}
    L = len(case["languages"])
    data, off = encoding.pack([bytes.fromhex(h) for h in case["docs_hex"]])
    ol, os_, _, _ = oracle(table, L, case["gram_lengths"], data, off, 5, 2)
    m = DeviceModel(table, L, case["gram_lengths"])
    assert_spans(m.score_spans(data, off, 5, 2, want_scores=True), ol, os_)
    assert_spans(m.score_spans(data, off, 5, 2), ol, os_)
    assert_spans(device_spans(m, data, off, 5, 2), ol, os_)


# --------------------------------------------------------- geometry sweep
SWEEP = [(1, 1), (3, 1), (4, 4), (5, 2), (64, 32), (128, 64), (128, 128), (256, 128), (257, 100), (300, 7), (700, 256)]
# (name, L, grams, key lengths, form, values, alphabet, check of DeviceModel.info())
KINDS = {
    "count": (20, (1, 2, 3), (1, 2, 3), "count", None, ALPHABET, lambda i: i["mode"] == 2),
    "class2": (20, (1, 2, 3), (1, 2, 3), "mask", (math.log(2.0), math.log(1.5)), ALPHABET,
               lambda i: "classes" in i["layout"]),
    "ordered": (20, (1, 2, 3), (1, 2, 3), "mask", None, ALPHABET,
                lambda i: i["mode"] == 0 and "classes" not in i["layout"]),
    "dense": (9, (1, 3, 2), (1, 2, 3), "dense", None, ALPHABET, lambda i: i["mode"] == 1),
    "wide": (12, (8, 12), (5, 8, 9, 12), "mask", None, AB, lambda i: "wide_keys" in i["layout"]),
    "general": (12, (2, 20), (1, 2, 17, 20), "dense", None, AB, lambda i: "general_keys" in i["layout"]),
    "L300": (300, (1, 2, 3, 4), (1, 2, 3, 4), "count", None, ALPHABET, lambda i: "lang_blocks" in i["layout"]),
}


@functools.lru_cache(maxsize=None)
def kind_table(kind):
    L, grams, key_lens, form, values, alphabet, _ = KINDS[kind]
    rng = np.random.default_rng(sorted(KINDS).index(kind) + 700)
    return make_table(rng, L, 500 if alphabet is AB else 300, list(key_lens), form, alphabet=alphabet,
                      values=list(values) if values else None)


@functools.lru_cache(maxsize=None)
def kind_model(kind, variant="product"):
    L, grams, _, _, _, _, ok = KINDS[kind]
    m = DeviceModel(kind_table(kind), L, list(grams), variant=variant)
    assert ok(m.info()), (kind, m.info())
    return m


@functools.lru_cache(maxsize=None)
def sweep_corpus(width, stride, ab=False):
    """(data of exactly off[-1] bytes, off): the lengths around width and
    width + stride, random ones up to 1,500, empty documents between them and
    at both ends; the last non-empty document ends at the buffer's last byte,
    and the byte count is no multiple of 4."""
    k = SWEEP.index((width, stride))
    rng = np.random.default_rng(9000 + k)
    w, s = width, stride
    fixed = [0, 1, 2, w - 1, w, w + 1, w + s - 1, w + s, w + s + 1, 2 * w + 1]
    lens = []
    for x in fixed + rng.integers(1, 1501, size=14).tolist():
        lens += [int(x)] + ([0] if len(lens) % 3 == 0 else [])
    lens = [0, 0] + lens
    lens.append(5 + (1 + k % 3 - (sum(lens) + 5)) % 4)   # total % 4 = 1, 2 or 3
    lens += [0]
    assert sum(lens) % 4 == 1 + k % 3
    alphabet = AB if ab else ALPHABET
    data, off = encoding.pack([bytes(rng.choice(alphabet, size=n)) for n in lens])
    data = np.array(data[:int(off[-1])])
    for a in (data, off):
        a.setflags(write=False)
    return data, off


def residue_pairs(off, width, stride):
    """{(source start mod 4, packed destination start mod 4)} over the non-empty spans."""
    _, so = spans.materialise(np.zeros(int(off[-1]), np.uint8), off, width, stride)
    soff = spans.span_offsets(off, width, stride)
    out = set()
    for d in range(len(off) - 1):
        for j, (a, e) in enumerate(spans.span_bounds(int(off[d + 1] - off[d]), width, stride)):
            if e > a:
                out.add((int(off[d] + a) % 4, int(so[soff[d] + j]) % 4))
    return out


def test_sweep_reaches_every_pair_of_residues():
    reached = {ws: residue_pairs(sweep_corpus(*ws)[1], *ws) for ws in SWEEP}
    full = {(a, b) for a in range(4) for b in range(4)}
    assert set().union(*reached.values()) == full
    # an odd width or stride (beyond a few bytes) reaches all 16 on its own
    for ws in ((5, 2), (257, 100), (300, 7)):
        assert reached[ws] == full, (ws, sorted(full - reached[ws]))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("width,stride", SWEEP, ids=lambda v: str(v))
def test_geometry_sweep(width, stride, kind):
    L, grams, key_lens, _, _, alphabet, _ = KINDS[kind]
    data, off = sweep_corpus(width, stride, alphabet is AB)
    assert len(data) == off[-1] and len(data) % 4 in (1, 2, 3) and off[-2] == off[-1] and off[-3] < off[-2]
    ol, os_, _, so = oracle(kind_table(kind), L, grams, data, off, width, stride)
    assert len(np.unique(ol)) >= 2 or width < min(key_lens)   # (a span shorter than every key has no hit)
    m = kind_model(kind)
    # labels only (class mode on a table of two values), then with scores
    assert_spans(m.score_spans(data, off, width, stride), ol, os_, "host labels")
    assert_spans(m.score_spans(data, off, width, stride, want_scores=True), ol, os_, "host scores")
    got = device_spans(m, data, off, width, stride, want_scores=False)
    assert_spans(got, ol, os_, "device labels")
    assert np.array_equal(got[2], spans.span_offsets(off, width, stride))
    assert_spans(device_spans(m, data, off, width, stride), ol, os_, "device scores")


# --------------------------------------------------------------- chunking
def chunk_corpus(seed, n_docs=40):
    rng = np.random.default_rng(seed)
    lens = rng.integers(200, 1200, size=n_docs)
    lens[[0, 7, 8, n_docs - 1]] = 0
    lens[[3, 4]] = [63, 65]
    data, off = encoding.pack([bytes(rng.choice(ALPHABET, size=int(x))) for x in lens])
    return data, off


@pytest.mark.parametrize("chunk", [1, 5, 64])
def test_chunks_cut_inside_documents(chunk, monkeypatch):
    data, off = chunk_corpus(81, 12 if chunk == 1 else 40)
    width, stride = 64, 32
    soff = spans.span_offsets(off, width, stride)
    # chunk boundaries fall inside documents
    inside = [g for g in range(chunk, int(soff[-1]), chunk) if g not in set(soff.tolist())]
    assert len(inside) >= 3 and int(soff[-1]) >= 3 * chunk
    for kind in ("count", "ordered"):
        L, grams = KINDS[kind][0], KINDS[kind][1]
        ol, os_, _, _ = oracle(kind_table(kind), L, grams, data, off, width, stride)
        ref = kind_model(kind).score_spans(data, off, width, stride, want_scores=True)
        assert_spans(ref, ol, os_)
        monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", str(chunk))
        diag = kind_model(kind, "diag")
        for want in (False, True):
            assert_spans(device_spans(diag, data, off, width, stride, want_scores=want), ol, os_, "device")
            assert_spans(diag.score_spans(data, off, width, stride, want_scores=want), ol, os_, "host")
        monkeypatch.delenv("LDGPU_SPAN_CHUNK_SPANS")


@pytest.mark.parametrize("want_scores", [False, True])
def test_failed_call_leaves_pipeline_clean(want_scores, monkeypatch):
    """The host call in chunks of 5 spans, a failure injected at chunk 2
    (diagnostics library): chunks 0 and 1 are in flight when the call fails.
    It drains, and the next call on the pooled pipeline gives the oracle's
    labels and score bits -- into pageable arrays, and (after another failed
    call) into pinned arrays pre-filled with -1."""
    kind, width, stride = "ordered", 64, 32
    L, grams = KINDS[kind][0], KINDS[kind][1]
    data, off = chunk_corpus(81, 40)
    ol, os_, _, _ = oracle(kind_table(kind), L, grams, data, off, width, stride)
    n = len(ol)
    assert n >= 4 * 5
    m = kind_model(kind, "diag")
    monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", "5")
    pl, ps = PinnedArray(n, np.int32), PinnedArray((n, L), np.float64)
    for out in ({}, {"out_labels": pl.array, "out_scores": ps.array if want_scores else None}):
        monkeypatch.setenv("LDGPU_FAIL_CHUNK", "2")
        with pytest.raises(_lib.LdgpuError, match="injected failure"):
            m.score_spans(data, off, width, stride, want_scores=want_scores)
        monkeypatch.delenv("LDGPU_FAIL_CHUNK")
        pl.array[:] = -1
        ps.array[:] = -1.0
        got = m.score_spans(data, off, width, stride, want_scores=want_scores, **out)
        assert (got[1] is None) == (not want_scores)
        assert not out or (got[0] is pl.array and (got[1] is ps.array or not want_scores))
        assert_spans(got, ol, os_, "pinned" if out else "pageable")
    pl.close()
    ps.close()


def test_host_pipeline_pinned_pageable_and_threads(monkeypatch):
    monkeypatch.setenv("LDGPU_SPAN_CHUNK_SPANS", "64")
    kind, width, stride = "ordered", 64, 32
    L, grams = KINDS[kind][0], KINDS[kind][1]
    m = kind_model(kind, "diag")
    data, off = chunk_corpus(82)
    ol, os_, _, _ = oracle(kind_table(kind), L, grams, data, off, width, stride)
    n = len(ol)
    assert n >= 3 * 64
    assert_spans(m.score_spans(data, off, width, stride, want_scores=True), ol, os_, "pageable")
    pin = PinnedArray(len(data) + 16, np.uint8)
    pin.array[:len(data)] = data
    pl, ps = PinnedArray(n, np.int32), PinnedArray((n, L), np.float64)
    pl.array[:] = -1
    m.score_spans(pin.array[:len(data)], off, width, stride, want_scores=True, out_labels=pl.array,
                  out_scores=ps.array)
    assert_spans((pl.array, ps.array), ol, os_, "pinned")
    pl.array[:] = -1
    m.score_spans(pin.array[:len(data)], off, width, stride, out_labels=pl.array)
    assert_spans((pl.array, None), ol, os_, "pinned labels")
    for p in (pin, pl, ps):
        p.close()

    # 4 threads on one context (ctypes drops the GIL)
    batches = [chunk_corpus(90 + i, 30 + 10 * i) for i in range(4)]
    expect = [oracle(kind_table(kind), L, grams, d, o, width, stride)[:2] for d, o in batches]
    errors = []

    def run(i):
        try:
            for _ in range(3):
                assert_spans(m.score_spans(*batches[i], width, stride, want_scores=True), *expect[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ------------------------------------------------- several spans per wave
@pytest.mark.parametrize("width,stride", [(64, 32), (256, 128)])
def test_several_spans_per_wave(width, stride, monkeypatch):
    """One workgroup (12 waves) over a few thousand spans: the spans of a wave
    are staged in groups of several and, at 64 bytes, counted in packs."""
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    # the geometry tests' count table: its 1- and 2-byte keys name one language
    # each, so the model has the direct tables and packs short documents
    f = G.FORM_BY_NAME["count"]
    L, grams, table = f.L, list(f.grams), G.form_table(f, "short")
    rng = np.random.default_rng(width)
    lens = rng.integers(2000, 3000, size=60 if width == 64 else 200)
    data, off = encoding.pack([bytes(rng.choice(G.ALPHABET, size=int(x))) for x in lens])
    ol, os_, _, so = oracle(table, L, grams, data, off, width, stride)
    assert len(ol) >= 3000 and len(np.unique(ol)) > 2
    s = G.survey(so, max(grams), G.SCORE_WAVES)
    assert s.docs_per_wave >= 250 and s.staged_multi > 0 and max(s.group_sizes) >= 4
    if width == 64:
        assert s.pack_sizes >= {2, 3, 4}
    m = DeviceModel(table, L, grams, variant="diag")
    info = m.info()
    assert info["mode"] == 2 and "packs" in info["layout"] and "direct" in info["layout"]
    assert_spans(m.score_spans(data, off, width, stride), ol, os_, "host labels")
    assert_spans(m.score_spans(data, off, width, stride, want_scores=True), ol, os_, "host scores")
    assert_spans(device_spans(m, data, off, width, stride, want_scores=False), ol, os_, "device labels")
    assert_spans(device_spans(m, data, off, width, stride), ol, os_, "device scores")


# -------------------------------------------------- mixed-language documents
@functools.lru_cache(maxsize=None)
def mixed_setup():
    """8 synthetic languages, a table fitted by the oracle on 40 documents of
    256 bytes per language (grams 1, 2, 3; the 300 best per language)."""
    ls = synth.make_languages(8, seed=7)
    tdata, toff, tlang = synth.generate(ls, 320, 256, 256, seed=11, doc_lang=np.repeat(np.arange(8), 40))
    rows = list(zip([ls.names[i] for i in tlang], synth.texts(tdata, toff)))
    table = O.fit(rows, ls.names, [1, 2, 3], 300)
    return ls, table


def mixed_docs(ls, width, n_docs=200):
    """n_docs documents of two different languages, 3 width bytes each:
    (texts, [(language a, language b, length of a's part)])."""
    rng = np.random.default_rng(width)
    a = rng.integers(0, 8, size=n_docs)
    b = (a + rng.integers(1, 8, size=n_docs)) % 8
    da, oa, _ = synth.generate(ls, n_docs, 3 * width, 3 * width, seed=100 + width, doc_lang=a)
    db, ob, _ = synth.generate(ls, n_docs, 3 * width, 3 * width, seed=200 + width, doc_lang=b)
    ta, tb = synth.texts(da, oa), synth.texts(db, ob)
    return [x + y for x, y in zip(ta, tb)], [(int(a[i]), int(b[i]), 3 * width) for i in range(n_docs)]


@pytest.mark.parametrize("width,stride", [(128, 64), (64, 32)])
def test_mixed_language_documents(width, stride):
    ls, table = mixed_setup()
    assert len(table) == 2400 and {v for row in table.values() for v in row} == {0.0, math.log(2.0)}
    grams = [1, 2, 3]
    texts, parts = mixed_docs(ls, width)
    data, off = encoding.pack_score(texts)
    ol, _, _, _ = oracle(table, 8, grams, data, off, width, stride)
    soff = spans.span_offsets(off, width, stride)
    # conditions on the oracle alone: the feature does what it is for
    pure = right = two_runs = 0
    for d, (la, lb, cut) in enumerate(parts):
        lab = ol[soff[d]:soff[d + 1]]
        for j, (s, e) in enumerate(spans.span_bounds(len(texts[d]), width, stride)):
            if e <= cut or s >= cut:
                pure += 1
                right += int(lab[j] == (la if e <= cut else lb))
        two_runs += len(spans.runs(len(texts[d]), lab, width, stride)) == 2
    print(f"({width}, {stride}): pure spans right {right}/{pure}, documents with two runs {two_runs}/{len(parts)}")
    assert right >= 0.99 * pure and two_runs >= 0.95 * len(parts)
    # the GPU labels every span as the oracle does
    model = LanguageDetectorModel(gramProbabilities=table, gramLengths=grams, languages=ls.names)
    labels, _, got_soff = model.device_model().score_spans(data, off, width, stride)
    assert np.array_equal(got_soff, soff) and np.array_equal(labels, ol)
    found = model.predict_spans(texts, width, stride)
    for d in range(len(texts)):
        want = [(a, b, ls.names[l]) for a, b, l in spans.runs(len(texts[d]), ol[soff[d]:soff[d + 1]], width, stride)]
        assert found[d] == want, d


# --------------------------------------------------------------- device API
def test_device_api_on_a_side_stream():
    kind, width, stride = "ordered", 5, 2
    L, grams = KINDS[kind][0], KINDS[kind][1]
    data, off = sweep_corpus(width, stride)
    m = kind_model(kind)
    hl, hs, hsoff = m.score_spans(data, off, width, stride, want_scores=True)
    assert np.array_equal(hsoff, spans.span_offsets(off, width, stride))
    dl, ds, dsoff = device_spans(m, data, off, width, stride)
    assert np.array_equal(dsoff, hsoff) and np.array_equal(dl, hl) and np.array_equal(bits(ds), bits(hs))
    # three spans more than there are: three empty spans, label 0 and zero scores
    dl, ds, _ = device_spans(m, data, off, width, stride, extra=3)
    assert np.array_equal(dl[:-3], hl) and dl[-3:].tolist() == [0, 0, 0]
    assert np.array_equal(bits(ds[:-3]), bits(hs)) and not bits(ds[-3:]).any()
    dl, _, _ = device_spans(m, data, off, width, stride, want_scores=False, extra=3)
    assert np.array_equal(dl[:-3], hl) and dl[-3:].tolist() == [0, 0, 0]
    # no document: one offset, no span
    dl, ds, dsoff = device_spans(m, data[:0], off[:1], width, stride)
    assert dl.shape == (0,) and dsoff.tolist() == [0]
    hl0, _, hsoff0 = m.score_spans(data[:0], off[:1], width, stride)
    assert hl0.shape == (0,) and hsoff0.tolist() == [0]


# ----------------------------------------------------------------- errors
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_invalid_arguments_leave_the_outputs_untouched():
    import torch
    m = kind_model("ordered")
    lib = m.lib
    data, off = sweep_corpus(5, 2)
    data = np.ascontiguousarray(data)
    n = len(off) - 1
    labels = np.full(4096, -7, dtype=np.int32)
    scores = np.full((4096, m.L), -1.0)

    def host(width, stride, offsets=off, n_docs=n, lab=labels, byt=data):
        return lib.ldgpu_score_spans(m.h, _ptr(byt), _ptr(np.ascontiguousarray(offsets, dtype=np.int64)), n_docs,
                                     width, stride, _ptr(lab), _ptr(scores))

    E, U = _lib.LDGPU_EINVAL, _lib.LDGPU_EUNSUPPORTED
    assert host(0, 1) == E and host(-1, 1) == E and host(4, 0) == E and host(4, 5) == E
    assert host(1 << 28, 1) == U and b"width" in lib.ldgpu_last_error()
    bad = np.array(off)
    bad[3] = bad[4] + 1
    assert host(4, 2, offsets=bad) == E and b"decrease" in lib.ldgpu_last_error()
    assert host(4, 2, n_docs=-1) == E
    assert host(4, 2, lab=None) == E
    assert host(4, 2, byt=None) == E
    assert lib.ldgpu_score_spans(None, _ptr(data), _ptr(off), n, 4, 2, _ptr(labels), None) == E
    assert (labels == -7).all() and (scores == -1.0).all()
    with pytest.raises(ValueError):
        m.score_spans(data, off, 4, 5)
    with pytest.raises(NotImplementedError):
        m.score_spans(data, off, 1 << 28, 1)

    dev = torch.device("cuda", 0)
    d_bytes = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.array(off)).to(dev)
    d_soff = torch.from_numpy(spans.span_offsets(off, 4, 2)).to(dev)
    d_lab = torch.full((4096,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def device(width, stride, p_bytes=d_bytes.data_ptr(), n_docs=n, n_spans=100, p_lab=d_lab.data_ptr()):
        return lib.ldgpu_score_spans_device(m.h, ctypes.c_void_p(p_bytes), int(off[-1]),
                                            ctypes.c_void_p(d_off.data_ptr()), n_docs, width, stride,
                                            ctypes.c_void_p(d_soff.data_ptr()), n_spans,
                                            ctypes.c_void_p(p_lab) if p_lab else None, None, ctypes.c_void_p(st))

    assert device(0, 1) == E and device(4, 0) == E and device(4, 5) == E and device(1 << 28, 1) == U
    assert device(4, 2, n_docs=-1) == E and device(4, 2, n_spans=-1) == E and device(4, 2, p_lab=0) == E
    assert device(4, 2, p_bytes=d_bytes.data_ptr() + 1) == E and b"aligned" in lib.ldgpu_last_error()
    assert lib.ldgpu_span_offsets_device(m.ctx, ctypes.c_void_p(d_off.data_ptr()), n, 4, 5,
                                         ctypes.c_void_p(d_soff.data_ptr()), ctypes.c_void_p(st)) == E
    assert lib.ldgpu_span_offsets_device(None, ctypes.c_void_p(d_off.data_ptr()), n, 4, 2,
                                         ctypes.c_void_p(d_soff.data_ptr()), ctypes.c_void_p(st)) == E
    torch.cuda.synchronize()
    assert (d_lab.cpu().numpy() == -7).all()
    assert np.array_equal(d_soff.cpu().numpy(), spans.span_offsets(off, 4, 2))
    assert device(4, 2, n_spans=0) == _lib.LDGPU_OK


def test_wrong_length_row_raises_only_inside_a_span():
    m = DeviceModel({b"ab": [1.0], b"xy": [0.0, 1.0]}, 2, [2])
    data, off = encoding.pack([b"xyxy", b"zzabzz"])
    # (3, 3): the spans "zza" and "bzz" -- "ab" lies across their boundary, in no span
    labels, _, soff = m.score_spans(data, off, 3, 3)
    assert soff.tolist() == [0, 2, 4] and labels.tolist() == [1, 0, 0, 0]
    assert device_spans(m, data, off, 3, 3)[0].tolist() == [1, 0, 0, 0]
    # (4, 2): the spans "zzab" and "abzz" hold it
    with pytest.raises(ValueError, match="requirement failed"):
        m.score_spans(data, off, 4, 2)
    with pytest.raises(ValueError, match="requirement failed"):
        device_spans(m, data, off, 4, 2)
    # the error word is cleared: the next calls succeed
    assert m.score_spans(data, off, 3, 3)[0].tolist() == [1, 0, 0, 0]
    assert device_spans(m, data, off, 3, 3)[0].tolist() == [1, 0, 0, 0]


# ------------------------------------------------------------- Python API
def test_transform_spans_on_the_reference_kat():
    import pandas as pd
    kat = load("reference_kats.json")["score_kat"]
    model = LanguageDetectorModel(gramProbabilities=kat["table"], gramLengths=kat["gram_lengths"],
                                  languages=kat["languages"])
    table = {encoding.gram_key(k): v for k, v in kat["table"].items()}
    width, stride = 8, 4
    found = model.predict_spans(kat["docs"], width, stride)
    for text, runs in zip(kat["docs"], found):
        data, off = encoding.pack_score([text])
        ol, _, _, _ = oracle(table, 2, kat["gram_lengths"], data, off, width, stride)
        assert runs == [(a, b, kat["languages"][l]) for a, b, l in spans.runs(len(text), ol, width, stride)]
        assert runs[0][0] == 0 and runs[-1][1] == len(text)
    # "This ..." starts with the English key: an "en" run first, then the no-hit label "de"
    assert found[2][0] == (0, 4, "en") and found[2][1][2] == "de"
    assert found[0] == [(0, len(kat["docs"][0]), "de")]
    df = pd.DataFrame({"fulltext": kat["docs"]})
    out = model.transformSpans(df, width, stride)
    assert list(out.columns) == ["fulltext", "langSpans"]
    assert list(out["langSpans"]) == found
    assert list(model.transformSpans(df, width, stride, outputCol="runs").columns) == ["fulltext", "runs"]
    with pytest.raises(ValueError, match="Column langSpans already exists"):
        model.transformSpans(out, width, stride)
    with pytest.raises(ValueError, match="does not exist"):
        model.transformSpans(pd.DataFrame({"text": kat["docs"]}), width, stride)
    with pytest.raises(ValueError, match="stride"):
        model.predict_spans(kat["docs"], 4, 5)
