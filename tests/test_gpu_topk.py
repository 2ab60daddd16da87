"""SCORE's top-k output (ldgpu_score_topk / ldgpu_score_topk_device) against
languagedetection.topk.rank applied to the C oracle's scores: labels exact,
scores bit for bit, entry 0 equal to the label SCORE gives."""
import functools
import json
import math
import os
import threading

import numpy as np
import pytest

import ldoracle_c as OC
from conftest import GOLDEN
from languagedetection import LanguageDetectorModel, _lib, encoding, topk
from languagedetection.runtime import DeviceModel, PinnedArray

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b"abcdefgh ", dtype=np.uint8)
NAN, INF = float("nan"), float("inf")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_table(rng, L, n_keys, key_lens, form, alphabet=ALPHABET, values=None):
    """form "dense": normal rows; "mask": one value per row (log(1 + 1/k), or
    drawn from `values`) at a random language set; "count": log 2 everywhere."""
    if form == "count":
        values = [math.log(2.0)]
    table = {}
    for _ in range(n_keys):
        key = bytes(rng.choice(alphabet, size=int(rng.choice(key_lens))))
        if form == "dense":
            table[key] = rng.normal(size=L).tolist()
            continue
        m = rng.random(L) < rng.uniform(0.02, 0.6)
        if not m.any():
            m[int(rng.integers(0, L))] = True
        v = float(rng.choice(values)) if values else math.log(1.0 + 1.0 / int(m.sum()))
        table[key] = [v if b else 0.0 for b in m]
    return table


def make_docs(rng, n, max_len=300, alphabet=ALPHABET, first=(0, 1, 2, 3, 64, 65)):
    lens = rng.integers(0, max_len, size=n)
    lens[:len(first)] = first
    return encoding.pack([bytes(rng.choice(alphabet, size=int(x))) for x in lens])


def oracle_scores(table, L, grams, data, off):
    return OC.Table(table, L).score(grams, data, off, want_scores=True, nthreads=8)[1]


def expected(scores, k):
    """topk.rank over every row, and the scores it selects."""
    labels = np.array([topk.rank(row, k) for row in scores.tolist()], dtype=np.int32).reshape(len(scores), k)
    return labels, np.take_along_axis(scores, labels.astype(np.int64), axis=1)


def assert_topk(got, scores, k, first_labels=None):
    tl, ts = got
    el, es = expected(scores, k)
    assert tl.dtype == np.int32 and tl.shape == el.shape
    assert np.array_equal(tl, el), np.nonzero((tl != el).any(axis=1))[0][:10]
    if ts is not None:
        assert np.array_equal(bits(ts), bits(es))
    if first_labels is not None:
        assert np.array_equal(tl[:, 0], first_labels)


def check_model(m, scores, data, off, ks):
    labels, _ = m.score(data, off)
    for k in ks:
        assert_topk(m.score_topk(data, off, k), scores, k, labels)


def device_topk(m, data, off, k, want_scores=True, own_stream=True):
    """ldgpu_score_topk_device on torch tensors (a non-default stream)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(off) - 1
    d_bytes = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
    kk = max(k, 1)  # (an invalid k is rejected before any buffer is touched)
    d_lab = torch.full((n, kk), -1, dtype=torch.int32, device=dev)
    d_sc = torch.full((n, kk), -1.0, dtype=torch.float64, device=dev) if want_scores else None
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream()
    m.score_topk_device(d_bytes.data_ptr(), int(len(data)), d_off.data_ptr(), n, k, d_lab.data_ptr(),
                        d_sc.data_ptr() if want_scores else 0, stream.cuda_stream)
    stream.synchronize()
    return d_lab.cpu().numpy(), d_sc.cpu().numpy() if want_scores else None


# ------------------------------------------------------------------ golden
@pytest.mark.parametrize("case", load("score_cases.json"), ids=lambda c: c["name"])
def test_golden_cases_every_k(case):
    table = {bytes.fromhex(k): [float.fromhex(v) for v in row] for k, row in case["table"]}
    L = len(case["languages"])
    data, off = encoding.pack([bytes.fromhex(h) for h in case["docs_hex"]])
    scores = np.array([[float.fromhex(v) for v in row] for row in case["scores"]], dtype=np.float64)
    m = DeviceModel(table, L, case["gram_lengths"])
    for k in range(1, min(L, 16) + 1):
        assert_topk(m.score_topk(data, off, k), scores, k, np.array(case["labels"], dtype=np.int32))
    assert_topk(device_topk(m, data, off, min(L, 16)), scores, min(L, 16))


# ------------------------------------------------- slice and block edges
@pytest.mark.parametrize("L,form", [(1, "mask"), (2, "mask"), (3, "mask"), (63, "mask"), (64, "mask"), (65, "mask"),
                                    (128, "mask"), (129, "mask"), (256, "mask"), (3, "dense"), (100, "dense"),
                                    (256, "dense")])
def test_slice_edges(L, form):
    rng = np.random.default_rng(1000 + L + len(form))
    grams = [1, 2, 3]
    table = make_table(rng, L, 300, grams, form)
    data, off = make_docs(rng, 400)
    scores = oracle_scores(table, L, grams, data, off)
    m = DeviceModel(table, L, grams)
    check_model(m, scores, data, off, sorted({1, min(L, 2), min(L, 16)}))


@pytest.mark.parametrize("L", [257, 300, 520])
@pytest.mark.parametrize("form", ["count", "mask", "dense"])
def test_language_blocks_looped_variant(L, form):
    """More than 256 languages: the scores come from one launch per language
    block, the selection from the looped kernel; uniform-value tables make ties
    across a block boundary common."""
    rng = np.random.default_rng(2000 + L + len(form))
    grams = [1, 2, 3, 4]
    table = make_table(rng, L, 300, grams, form)
    data, off = make_docs(rng, 250)
    scores = oracle_scores(table, L, grams, data, off)
    m = DeviceModel(table, L, grams)
    assert "lang_blocks" in m.info()["layout"]
    check_model(m, scores, data, off, [1, 16])


def test_4096_languages_from_masks():
    L, S, n_keys = 4096, 64, 50
    rng = np.random.default_rng(4096)
    keys = sorted({bytes(rng.choice(ALPHABET, size=int(n))) for n in rng.integers(1, 3, size=n_keys)})
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    ko = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=ko[1:])
    dense = rng.random((len(keys), L)) < 0.01
    dense[:, 4095] |= rng.random(len(keys)) < 0.5   # the last language of the last block takes part
    dense[:, 0] |= rng.random(len(keys)) < 0.3
    masks = np.zeros((len(keys), S), dtype=np.uint64)
    for l in range(L):
        masks[:, l // 64] |= dense[:, l].astype(np.uint64) << np.uint64(l % 64)
    v = math.log(2.0)
    vals = np.full(len(keys), v)
    table = {k: np.where(dense[i], v, 0.0).tolist() for i, k in enumerate(keys)}
    data, off = make_docs(rng, 60, max_len=120)
    scores = oracle_scores(table, L, [1, 2], data, off)
    m = DeviceModel.from_masks(kb, ko, masks, vals, L, [1, 2])
    check_model(m, scores, data, off, [1, 16])


# ------------------------------------------------------------ model kinds
def test_model_kind_count_mode():
    rng = np.random.default_rng(31)
    table = make_table(rng, 20, 400, [1, 2, 3], "count")
    data, off = make_docs(rng, 600)
    m = DeviceModel(table, 20, [1, 2, 3])
    assert m.info()["mode"] == 2
    check_model(m, oracle_scores(table, 20, [1, 2, 3], data, off), data, off, [1, 3, 16])


def test_model_kind_three_values():
    """A table of 3 distinct values: labels-only calls take class mode; the
    top-k call needs the scores and goes through the ordered replay."""
    rng = np.random.default_rng(32)
    table = make_table(rng, 20, 400, [1, 2, 3], "mask", values=[math.log(2.0), math.log(1.5), math.log(1.25)])
    data, off = make_docs(rng, 600)
    m = DeviceModel(table, 20, [1, 2, 3])
    assert "classes" in m.info()["layout"]
    check_model(m, oracle_scores(table, 20, [1, 2, 3], data, off), data, off, [1, 3, 16])


@pytest.mark.parametrize("grams,key_lens,flag", [([8, 12], [5, 8, 9, 12], "wide_keys"),
                                               ([16], [1, 2, 13, 16], "general_keys"),
                                               ([2, 20], [1, 2, 17, 20], "general_keys")])
@pytest.mark.parametrize("form", ["mask", "dense"])
def test_model_kind_long_keys(grams, key_lens, flag, form):
    rng = np.random.default_rng(33 + sum(grams) + len(form))
    alphabet = np.frombuffer(b"ab ", dtype=np.uint8)
    L = 12
    table = make_table(rng, L, 500, key_lens, form, alphabet=alphabet)
    data, off = make_docs(rng, 500, max_len=140, alphabet=alphabet, first=(0, 1, 2, 3, 64, 65, 8, 12, 16, 20))
    m = DeviceModel(table, L, grams)
    assert flag in m.info()["layout"]
    check_model(m, oracle_scores(table, L, grams, data, off), data, off, [1, 12])


# --------------------------------------------------------- special values
@pytest.mark.parametrize("L,at", [(300, (0, 5, 256, 3, 290, 1, 260, 2, 280, 299)), (5, (0, 1, 2, 3, 4, 1, 2, 3, 4, 4))])
def test_nan_inf_signed_zero_rows(L, at):
    """NaN / +-inf / -0.0 rows: a NaN first score stays first, a NaN elsewhere
    (also inf + -inf) goes last, after -inf; a document without a hit and the
    empty document give 0 .. k-1 with zero scores."""
    a = at
    row = lambda pairs: [pairs.get(l, 0.0) for l in range(L)]
    table = {b"a": row({a[0]: NAN, a[1]: 1.0}), b"b": row({a[2]: NAN, a[3]: 2.0}), b"c": row({a[4]: INF, a[5]: 5.0}),
             b"d": row({a[6]: 7.0, a[7]: 7.0}), b"e": row({a[8]: 9.0}), b"f": row({a[9]: -0.0, a[3]: -0.0}),
             b"g": row({a[4]: -INF, a[1]: -INF}), b"h": row({l: -1.0 for l in range(L) if l != a[2]})}
    docs = [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"h", b"ab", b"bc", b"de", b"cg", b"gh", b"bgh", b"abcdefgh",
            b"fh", b"", b"zz"]
    data, off = encoding.pack(docs)
    scores = oracle_scores(table, L, [1], data, off)
    m = DeviceModel(table, L, [1])
    check_model(m, scores, data, off, sorted({1, 5, min(L, 16)}))
    tl, ts = m.score_topk(data, off, 5)
    for d in (len(docs) - 2, len(docs) - 1):
        assert tl[d].tolist() == [0, 1, 2, 3, 4] and bits(ts[d]).tolist() == [0] * 5
    assert_topk(device_topk(m, data, off, 5), scores, 5)


# --------------------------------------------------------------- chunking
@functools.lru_cache(maxsize=None)
def chunked_corpus():
    """(table, L, grams, data, off, the oracle's scores): 100 documents for
    chunks of 7 -- empty ones first and last of a chunk (0, 6, 7, 13, 14, 98,
    99), and lengths 1, 2, 64 and 65 around a chunk boundary."""
    rng = np.random.default_rng(41)
    L, grams = 20, [1, 2, 3]
    table = make_table(rng, L, 300, grams, "mask")
    lens = rng.integers(1, 200, size=100)
    lens[[0, 6, 7, 13, 14, 50, 98, 99]] = 0
    lens[[20, 21, 27, 28]] = [1, 2, 64, 65]
    data, off = encoding.pack([bytes(rng.choice(ALPHABET, size=int(x))) for x in lens])
    scores = oracle_scores(table, L, grams, data, off)
    for a in (data, scores):  # (off stays writable: torch.from_numpy takes it as it is)
        a.setflags(write=False)
    return table, L, grams, data, off, scores


def test_chunked_device_call(monkeypatch):
    """The diagnostics library with chunks of 7 documents: 100 documents, some
    empty, some first / last of a chunk, on torch tensors and a non-default
    stream, equal the unchunked product result and the oracle."""
    monkeypatch.setenv("LDGPU_TOPK_CHUNK_DOCS", "7")
    table, L, grams, data, off, scores = chunked_corpus()
    diag = DeviceModel(table, L, grams, variant="diag")
    prod = DeviceModel(table, L, grams)
    for k in (1, 3, 16):
        got = device_topk(diag, data, off, k)
        assert_topk(got, scores, k)
        ref = prod.score_topk(data, off, k)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1]))
        assert_topk(diag.score_topk(data, off, k), scores, k)  # the host pipeline in chunks of 7 too
    labels_only = device_topk(diag, data, off, 3, want_scores=False)
    assert labels_only[1] is None
    assert_topk(labels_only, scores, 3)
    # no document, and one document in a chunk of 7
    tl, ts = device_topk(diag, data[:0], off[:1], 3)
    assert tl.shape == (0, 3) and ts.shape == (0, 3)
    one = slice(20, 22)
    assert_topk(device_topk(diag, data, off[one], 3), scores[20:21], 3)
    tl, ts = diag.score_topk(data[:0], off[:1], 3)
    assert tl.shape == (0, 3)


@pytest.mark.parametrize("want_scores", [False, True])
def test_failed_call_leaves_pipeline_clean(want_scores, monkeypatch):
    """The host call in chunks of 7 documents, a failure injected at chunk 2
    (diagnostics library): chunks 0 and 1 are in flight when the call fails.
    It drains, and the next call on the pooled pipeline gives the oracle's top
    3 -- into pageable arrays, and (after another failed call) into pinned
    arrays pre-filled with -1."""
    table, L, grams, data, off, scores = chunked_corpus()
    n, k = len(off) - 1, 3
    m = DeviceModel(table, L, grams, variant="diag")
    monkeypatch.setenv("LDGPU_TOPK_CHUNK_DOCS", "7")
    pl, ps = PinnedArray((n, k), np.int32), PinnedArray((n, k), np.float64)
    for out in ({}, {"out_labels": pl.array, "out_scores": ps.array if want_scores else None}):
        monkeypatch.setenv("LDGPU_FAIL_CHUNK", "2")
        with pytest.raises(_lib.LdgpuError, match="injected failure"):
            m.score_topk(data, off, k, want_scores=want_scores)
        monkeypatch.delenv("LDGPU_FAIL_CHUNK")
        pl.array[:] = -1
        ps.array[:] = -1.0
        got = m.score_topk(data, off, k, want_scores=want_scores, **out)
        assert (got[1] is None) == (not want_scores)
        assert not out or (got[0] is pl.array and (got[1] is ps.array or not want_scores))
        assert_topk(got, scores, k)
    pl.close()
    ps.close()


def test_failed_call_resets_the_error_word(monkeypatch):
    """A model with a wrong-length row, chunks of 7 documents: documents of
    chunks 0 and 1 hit the row, then the call fails by injection at chunk 2.
    The message is the injected one, and the pipeline's error word is cleared:
    the next call (no hit of the row) succeeds, one that hits it still raises."""
    m = DeviceModel({b"ab": [1.0], b"xy": [0.0, 1.0]}, 2, [2], variant="diag")
    monkeypatch.setenv("LDGPU_TOPK_CHUNK_DOCS", "7")
    docs = [b"xyxy", b"zz"] * 15
    bad = list(docs)
    bad[3] = bad[9] = b"zzabzz"   # in chunks 0 and 1
    monkeypatch.setenv("LDGPU_FAIL_CHUNK", "2")
    with pytest.raises(_lib.LdgpuError, match="injected failure"):
        m.score_topk(*encoding.pack(bad), 2)
    monkeypatch.delenv("LDGPU_FAIL_CHUNK")
    assert m.score_topk(*encoding.pack(docs), 2)[0].tolist() == [[1, 0], [0, 1]] * 15
    with pytest.raises(ValueError, match="BLAS.axpy size mismatch"):
        m.score_topk(*encoding.pack(bad), 2)
    assert m.score_topk(*encoding.pack(docs), 2)[0].tolist() == [[1, 0], [0, 1]] * 15


# ---------------------------------------------------------- host pipeline
def test_host_pipeline_pinned_pageable_and_threads():
    rng = np.random.default_rng(51)
    L, grams, k = 20, [1, 2, 3], 4
    table = make_table(rng, L, 300, grams, "mask")
    data, off = make_docs(rng, 600)
    n = len(off) - 1
    scores = oracle_scores(table, L, grams, data, off)
    m = DeviceModel(table, L, grams)
    tl, ts = m.score_topk(data, off, k)
    assert_topk((tl, ts), scores, k)
    pin = PinnedArray(len(data) + 16, np.uint8)
    pin.array[:len(data)] = data
    pl, ps = PinnedArray((n, k), np.int32), PinnedArray((n, k), np.float64)
    pl.array[:] = -1
    m.score_topk(pin.array[:len(data)], off, k, out_labels=pl.array, out_scores=ps.array)
    assert np.array_equal(pl.array, tl) and np.array_equal(bits(ps.array), bits(ts))
    # labels only: no score buffer
    pl.array[:] = -1
    l2, s2 = m.score_topk(pin.array[:len(data)], off, k, want_scores=False, out_labels=pl.array)
    assert s2 is None and np.array_equal(pl.array, tl)
    l3, s3 = m.score_topk(data, off, k, want_scores=False)
    assert s3 is None and np.array_equal(l3, tl)
    for p in (pin, pl, ps):
        p.close()

    # 4 threads on one context (ctypes drops the GIL)
    batches = [make_docs(np.random.default_rng(60 + i), 2000 + 500 * i) for i in range(4)]
    expect = [m.score_topk(d, o, k) for d, o in batches]
    assert_topk(expect[0], oracle_scores(table, L, grams, *batches[0]), k)
    errors = []

    def run(i):
        try:
            for _ in range(3):
                gl, gs = m.score_topk(*batches[i], k)
                assert np.array_equal(gl, expect[i][0]) and np.array_equal(bits(gs), bits(expect[i][1]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ----------------------------------------------------------------- errors
def test_invalid_k():
    rng = np.random.default_rng(71)
    data, off = make_docs(rng, 10)
    m3 = DeviceModel(make_table(rng, 3, 50, [1, 2], "mask"), 3, [1, 2])
    m20 = DeviceModel(make_table(rng, 20, 50, [1, 2], "mask"), 20, [1, 2])
    for m, k in ((m3, 0), (m3, 4), (m20, 0), (m20, 17), (m20, 21), (m20, -1)):
        with pytest.raises(ValueError, match="k = "):
            m.score_topk(data, off, k)
        with pytest.raises(ValueError, match="k = "):
            device_topk(m, data, off, k)
    assert m20.score_topk(data, off, 16)[0].shape == (10, 16)
    assert m3.score_topk(data, off, 3)[0].shape == (10, 3)


def test_wrong_length_row_raises_when_hit():
    m = DeviceModel({b"ab": [1.0], b"xy": [0.0, 1.0]}, 2, [2])
    data, off = encoding.pack([b"xyxy", b"zz"])
    assert m.score_topk(data, off, 2)[0].tolist() == [[1, 0], [0, 1]]
    assert device_topk(m, data, off, 2)[0].tolist() == [[1, 0], [0, 1]]
    data, off = encoding.pack([b"xyxy", b"zzabzz"])
    with pytest.raises(ValueError, match="requirement failed"):
        m.score_topk(data, off, 2)
    with pytest.raises(ValueError, match="requirement failed"):
        device_topk(m, data, off, 2)
    # the error word is cleared: the next calls succeed
    data, off = encoding.pack([b"xyxy"])
    assert m.score_topk(data, off, 1)[0].tolist() == [[1]]
    assert device_topk(m, data, off, 1)[0].tolist() == [[1]]


# ------------------------------------------------------------- Python API
def test_predict_topk_and_transform_topk_on_the_reference_kat():
    import pandas as pd
    kat = load("reference_kats.json")["score_kat"]
    model = LanguageDetectorModel(gramProbabilities=kat["table"], gramLengths=kat["gram_lengths"],
                                  languages=kat["languages"])
    langs, scores = model.predict_topk(kat["docs"], 2)
    assert [row[0] for row in langs] == ["de", "de", "en", "en"]
    assert [sorted(row) for row in langs] == [["de", "en"]] * 4
    assert scores.shape == (4, 2) and (scores[:, 0] >= scores[:, 1]).all()
    idx, full = model.predict_indices(kat["docs"], want_scores=True)
    assert np.array_equal(bits(scores[:, 0]), bits(full[np.arange(4), idx]))
    df = pd.DataFrame({"fulltext": kat["docs"]})
    out = model.transformTopK(df, 2)
    assert list(out.columns) == ["fulltext", "lang_candidates", "lang_scores"]
    assert [c[0] for c in out["lang_candidates"]] == ["de", "de", "en", "en"]
    assert [list(s) for s in out["lang_scores"]] == scores.tolist()
    assert list(model.transform(df)["lang"]) == [c[0] for c in out["lang_candidates"]]
    with pytest.raises(ValueError, match="Column lang_candidates already exists"):
        model.transformTopK(out, 2)
    with pytest.raises(ValueError, match="Column lang_scores already exists"):
        model.transformTopK(out.drop(columns=["lang_candidates"]), 1)
    with pytest.raises(ValueError, match="k = "):
        model.predict_topk(kat["docs"], 3)
