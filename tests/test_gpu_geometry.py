"""GPU parity of SCORE where a wave scores SEVERAL documents, and over the
document lengths at which the kernels switch paths.

A call with fewer than 12 * CUs * wg_per_cu documents (3072 to 9216 on an
MI355X) gives every wave at most one document: no group of documents, no pack,
no state carried from one document to the next, no second staging buffer.
The tests here put many documents on a wave in two ways -- the diagnostics
library's LDGPU_SCORE_GRID (one or two workgroups: 12 or 24 waves over the
whole corpus) and, on the product library, geometry.tile (the corpus repeated
to 16 * 12 * CUs * 3 documents and more) -- on corpora built so that the host
model (tests/geometry.py) finds every kind of group and pack under those
grids; test_geometry_model.py asserts that on the CPU, and that the tables
would tell a read past a document's end.  Every comparison is exact: labels
and the bits of the fp64 scores against the C oracle."""
import functools
import math

import numpy as np
import pytest
import torch

import geometry as G
import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

FORM_NAMES = [f.name for f in G.FORMS]
PRODUCT_FORMS = [f.name for f in G.FORMS if f.variant == "product"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def expect(corpus, spec):
    """The oracle's (labels, scores) of one period of the corpus, read-only."""
    c = G.CORPORA[corpus]()
    ol, os_ = OC.Table(G.table_for(corpus, *spec), spec[1]).score(list(spec[2]), c.data, c.off, want_scores=True,
                                                                  nthreads=8)
    ol.setflags(write=False)
    os_.setflags(write=False)
    return ol, os_


def spec_of(f):
    return (f.kind, f.L, f.grams, f.n_cls, f.total_keys)


def make_model(f, corpus, monkeypatch=None, variant=None):
    """The form's model on `variant` (default: the form's own library), its
    mode and layout as the form states them."""
    variant = variant or f.variant
    if variant == "diag" and f.env:
        for k, v in f.env.items():
            monkeypatch.setenv(k, v)
    m = DeviceModel(G.form_table(f, corpus), f.L, list(f.grams), variant=variant)
    if variant == f.variant or not f.env:
        info = m.info()
        assert f.mode is None or info["mode"] == f.mode, info
        assert all(x in info["layout"] for x in f.has) and not any(x in info["layout"] for x in f.hasnt), info
        if f.total_keys:
            assert info["filter_bits"] > 64 * 1024 * 8, info   # a keyed bloom in global memory
    return m


def same(got, want, times, what):
    """`got` equals `want` tiled `times` times (rows of documents)."""
    g = np.asarray(got).reshape(times, -1)
    w = np.asarray(want).reshape(1, -1)
    eq = g == w
    assert eq.all(), (what, "first mismatches at documents",
                      (np.nonzero(~eq.reshape(-1))[0][:10] // max(1, w.size // len(want))).tolist())


def labels_device(m, data, n_bytes, off):
    dev = torch.device("cuda", 0)
    d_bytes = torch.from_numpy(np.array(data, dtype=np.uint8)).to(dev)     # (a copy: the corpora are read-only)
    d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
    n = len(off) - 1
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    m.score_device(d_bytes.data_ptr(), int(n_bytes), d_off.data_ptr(), n, d_lab.data_ptr(), 0,
                   torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return d_lab.cpu().numpy()


def check(m, f, data, off, ol, os_, times=1):
    if f.scores:
        labels, scores = m.score(data, off, want_scores=True)
        same(labels, ol, times, "labels of the scores call")
        same(bits(scores), bits(os_), times, "score bits")
        del scores
    only, _ = m.score(data, off, want_scores=False)
    same(only, ol, times, "labels-only call")
    if not f.scores:
        same(labels_device(m, data, int(off[-1]), off), ol, times, "labels-only device call")


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("form", FORM_NAMES)
def test_short_corpus_small_grid(form, grid, monkeypatch):
    """Corpus SHORT on one and two workgroups: 150 and 75 documents per wave,
    groups of 63, packs of 2 to 4 and everything that ends one
    (test_short_corpus_under_small_grids)."""
    f = G.FORM_BY_NAME[form]
    c = G.short_corpus()
    monkeypatch.setenv("LDGPU_SCORE_GRID", str(grid))
    m = make_model(f, "short", monkeypatch, variant="diag")
    ol, os_ = expect("short", spec_of(f))
    assert len(np.unique(ol)) > 2
    check(m, f, c.data, c.off, ol, os_)


@pytest.mark.parametrize("form", PRODUCT_FORMS)
def test_short_corpus_tiled_product(form):
    """The product library on SHORT tiled until every wave of its grid has 16
    documents or more (a model keeps at most three workgroups per CU:
    test_lds_floor_bounds_workgroups_per_cu); the expected output is the
    one-period oracle, tiled."""
    f = G.FORM_BY_NAME[form]
    c = G.short_corpus()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    at_least = 16 * G.SCORE_WAVES * cus * 3
    times = G.tiles_for(c.n, at_least)
    data, off = G.tile(c.data, c.off, times)
    assert len(off) - 1 >= at_least and (len(off) - 1) // G.product_waves(len(off) - 1, cus, 3) >= 16
    m = make_model(f, "short")
    ol, os_ = expect("short", spec_of(f))
    check(m, f, data, off, ol, os_, times)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_long_corpus(form, monkeypatch):
    """Corpus LONG -- documents of 1000..1048 bytes at every start modulo 16
    (staged or in place), of 2, 3, 4, 5, 8, 16, 20 and 79 superblocks, around
    the general-key kernel's 4096 staged bytes -- on the product library (one
    document per wave) and on one and two workgroups of the diagnostics
    library (about 135 and 67 documents per wave: a long document's group
    holds the filler after it whenever both fit the buffer)."""
    f = G.FORM_BY_NAME[form]
    c = G.long_corpus()
    ol, os_ = expect("long", spec_of(f))
    assert len(np.unique(ol)) > 2
    check(make_model(f, "long", variant="product"), f, c.data, c.off, ol, os_)
    m = make_model(f, "long", monkeypatch, variant="diag")
    for grid in ("1", "2"):
        monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
        check(m, f, c.data, c.off, ol, os_)


@pytest.mark.parametrize("v", [math.log(2.0), -0.75], ids=["positive", "negative"])
def test_count_argmax_length_limit(v):
    """Labels-only count mode takes the integer argmax of the counts up to
    count_argmax_len = (2^24 - 1) / nG bytes -- 524287 with 32 gram lengths --
    and the fold of the counts beyond.  Documents of 524286, 524287 and
    524288 bytes, every window a hit: 'a' counts for both languages, the
    leading 'b' for language 1 alone, which so leads by 32 hits of 1.7e7 (and
    trails by them when the value is negative: count_sign < 0).  At 524288
    bytes its count is exactly 2^24."""
    grams = [1] * 32
    assert ((1 << 24) - 1) // len(grams) == 524287
    table = {b"a": [v, v], b"b": [0.0, v]}
    docs = [b"b" + b"a" * (n - 1) for n in (524286, 524287, 524288)]
    assert len(docs[2]) * len(grams) == 1 << 24
    data, off = encoding.pack(docs)
    m = DeviceModel(table, 2, grams)
    assert m.info()["mode"] == 2, m.info()
    ol, _ = OC.Table(table, 2).score(grams, data, off, want_scores=False, nthreads=8)
    assert ol.tolist() == ([1, 1, 1] if v > 0 else [0, 0, 0])
    labels, _ = m.score(data, off, want_scores=False)
    assert labels.tolist() == ol.tolist()


def device_call(m, L, buf, n_bytes, off, want_scores):
    dev = torch.device("cuda", 0)
    d_bytes = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
    n = len(off) - 1
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_sc = torch.full((n, L), -7.0, dtype=torch.float64, device=dev) if want_scores else None
    m.score_device(d_bytes.data_ptr(), int(n_bytes), d_off.data_ptr(), n, d_lab.data_ptr(),
                   d_sc.data_ptr() if want_scores else 0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return d_lab.cpu().numpy(), d_sc.cpu().numpy() if want_scores else None


@pytest.mark.parametrize("rem", [1, 2, 3])
def test_device_call_bytes_end_inside_a_dword(rem, monkeypatch):
    """ldgpu_score_device with n_bytes = 1, 2 and 3 modulo 4 and no pad:
    corpus SHORT and one more document, which ends in keys of every length;
    0xA5 fills the buffer beyond n_bytes, and 0xA5 and 0xA5A5 are keys.  The
    last group of the last wave is staged across n_bytes: what lies beyond
    must read as nothing."""
    f = G.FORM_BY_NAME["count"]
    c = G.short_corpus()
    total = int(c.off[-1])
    k = 40 + (rem - (total + 40)) % 4
    tail = bytes(np.random.default_rng(rem).choice(G.ALPHABET[4:13], size=k))
    n = total + k
    assert n % 4 == rem
    table = dict(G.form_table(f, "short"))

    def one(lang):
        return [math.log(2.0) if l == lang else 0.0 for l in range(f.L)]
    for g in f.grams:
        table[tail[k - g:]] = one(3 + g)
    table[b"\xa5"] = one(17)
    table[b"\xa5\xa5"] = one(18)
    edata = np.zeros(((n + 3) & ~3) + 32, dtype=np.uint8)
    edata[:total] = c.data[:total]
    edata[total:n] = np.frombuffer(tail, dtype=np.uint8)
    buf = edata.copy()
    buf[n:] = 0xA5
    off = np.concatenate([c.off, [n]])
    ol, os_ = OC.Table(table, f.L).score(list(f.grams), edata, off, want_scores=True, nthreads=8)
    assert os_[-1].sum() >= len(f.grams) * math.log(2.0) * 0.99      # the last windows hit
    for variant, grid in (("product", None), ("diag", "1")):
        if grid:
            monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
        m = DeviceModel(table, f.L, list(f.grams), variant=variant)
        info = m.info()
        assert info["mode"] == 2 and "direct" in info["layout"] and "packs" in info["layout"], info
        labels, scores = device_call(m, f.L, buf, n, off, True)
        same(labels, ol, 1, "labels of the scores call")
        same(bits(scores), bits(os_), 1, "score bits")
        only, _ = device_call(m, f.L, buf, n, off, False)
        same(only, ol, 1, "labels-only call")
