"""SCORE on UTF-8 documents: the device decoder (ldgpu_utf8_decode[_device],
csrc/ldgpu_utf8.hip) against CPython's codec -- bytes.decode("utf-8") accepts
exactly the well-formed strings of Unicode Table 3-7 --, and the fused calls
(ldgpu_score_utf8[_device]) against ldgpu_score on encoding.pack_score of the
decoded texts: labels and fp64 score bits equal, ill-formed documents -1."""
import ctypes
import functools

import numpy as np
import pytest

import bytecorpus as B
import utf8corpus
from languagedetection import LanguageDetectorModel, _lib, encoding, utf8
from languagedetection.preprocessing import _casemap, intended_special_char_clean, java_lower
from languagedetection.runtime import (DeviceCaseMap, DeviceModel, PinnedArray, locale_class, utf8_decode,
                                       utf8_decode_device)
from test_gpu_preprocess import _random_texts

pytestmark = pytest.mark.gpu

S = utf8.STEP_BYTES
SEED = 11
SEQS = [b"a"] + utf8corpus.VALID_SEQS     # sequence lengths 1-4
ILL = [b"\xe2\x82", b"\xc0\x80", b"ab\xff", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"x" * 300 + b"\xf0\x9f\x98"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def filler(n, k=0):
    return bytes(97 + (i + k) % 26 for i in range(n))


def decode_and_check(docs, lead=b""):
    """Both output forms of ldgpu_utf8_decode over `docs` packed behind `lead`
    (offsets[0] = len(lead)) equal the codec's."""
    data, off = utf8.pack_utf8([lead] + list(docs))
    off = off[1:]
    for low in (False, True):
        utf8corpus.check(utf8_decode(data, off, low), docs, low)


# ------------------------------------------------------------------- decode
def test_exhaustive_small_sequences():
    """Every 2-byte string, the 3- and 4-byte strings around every rule's edges
    and every prefix of a valid sequence, one tiny document each, in one call:
    more documents than the grid has waves, so the grid-stride loop runs."""
    docs = utf8corpus.small_sequences()
    assert len(docs) > 256 * 8 * 4 * 2
    decode_and_check(docs)


def boundary_docs():
    docs = []
    for around in (S, 2 * S):
        for p in range(around - 4, around + 2):
            for k, seq in enumerate(SEQS):
                docs.append(filler(p, k) + seq + filler(7, p))
                docs += [filler(p, k) + seq[:cut] for cut in range(1, len(seq) + 1)]
    return docs


@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_step_boundaries(base):
    """One sequence of every length at every position around the wave's step
    (and twice the step), whole and cut after each of its bytes, every document
    starting at `base` mod 4 (a padding document of stray continuation bytes
    before each puts it there): followers from the next lane and the next
    step, the two-unit rank across a step, the alignment mask."""
    docs, at, real = [], 0, []
    for d in boundary_docs():
        pad = b"\x80" * ((base - at) % 4)
        docs += [pad, d]
        real.append(at + len(pad))
        at += len(pad) + len(d)
    assert all(r % 4 == base for r in real)
    decode_and_check(docs)


def test_document_boundaries():
    cut3, cut4 = b"ab\xe2\x82", b"x\xf0\x9f\x98"
    euro, grin = utf8corpus.VALID_SEQS[1], utf8corpus.VALID_SEQS[2]
    # a cut sequence, then a document that begins with the missing bytes: both flagged
    decode_and_check([cut3, b"\xac", cut4, b"\x80z"])
    decode_and_check([cut3, b"", b"\xac", cut4, b"", b"\x80z"])
    # a flagged document between two valid ones; empty documents at both ends
    good = "Grüße, κόσμε €😀".encode("utf-8")
    docs = [b"", good, b"\xc3(", good, b""]
    decode_and_check(docs)
    data, off = utf8.pack_utf8(docs)
    out, out_off, host = utf8_decode(data, off)
    assert host.tolist() == [0, 0, 1, 0, 0] and out_off[1] == 0 and out_off[3] == out_off[2] > 0
    assert out[out_off[3]:out_off[4]].astype("<u2").tobytes() == good.decode().encode("utf-16-le")
    # offsets[0] > 0, the bytes before it a lead that would claim the first document's
    for lead in (b"\xf0", b"\xf0\x9f", b"zz\xe2", b"\xc3\xa9\xf0\x9f\x98"):
        decode_and_check([b"\x9f\x98\x80abc", b"abc", euro, b"\xac"], lead=lead)
        decode_and_check([grin[1:], grin], lead=lead)
    # no documents
    for offs in ([0], [5]):
        out, out_off, host = utf8_decode(np.zeros(8, np.uint8), np.array(offs, dtype=np.int64))
        assert len(out) == 0 and out_off.tolist() == [0] and len(host) == 0
    # 4-byte characters only: 3 S + 1 bytes (the last one cut: flagged), 3 S and 3 S + 4
    assert (3 * S) % 4 == 0
    for lead in (b"", b"q", b"qq", b"qqq"):
        decode_and_check([(grin * S)[:3 * S + 1], grin * (3 * S // 4), grin * (3 * S // 4 + 1)], lead=lead)


def test_decode_then_preprocess_then_score():
    """Units from ldgpu_utf8_decode_device into ldgpu_preprocess_device (lower +
    clean + low bytes), then score_device, on device buffers: the flags and
    bytes equal the preprocessors' own on the texts' units, the labels those
    of java_lower + intended_special_char_clean + pack_score + score."""
    import torch
    rng = np.random.default_rng(5)
    texts, langs = _random_texts(rng, 2000)
    # ... and without the characters whose lower-casing needs context, so that
    # whole documents stay on the device
    texts += [t.translate({ord(c): None for c in "\u03a3\u0130\u0307\u0301"}) for t in texts[:1000]]
    langs += ["en"] * 1000
    n = len(texts)
    dev = torch.device("cuda", 0)
    cm = _casemap(0)
    table = {b"ab": [0.5, 0.0], b"x": [0.0, 0.25], b"\xe4": [0.0, 1.0], b"\xdf": [0.75, 0.0], b"i": [0.1, 0.1]}
    m = DeviceModel(table, 2, [1, 2])
    data, off = utf8.pack_utf8([t.encode("utf-8") for t in texts])
    nb = int(off[-1])
    loc = np.array([locale_class(l) for l in langs], dtype=np.uint8)
    flags = _lib.PRE_LOWER | _lib.PRE_CLEAN | _lib.PRE_LOW_BYTES
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_utf8, d_off, d_loc = (torch.from_numpy(np.array(a)).to(dev) for a in (data, off, loc))
        d_units = torch.zeros(nb + 8, dtype=torch.int16, device=dev)
        d_uoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_bad = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(nb + 8, dtype=torch.uint8, device=dev)
        d_ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_host = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
        st = stream.cuda_stream
        utf8_decode_device(d_utf8.data_ptr(), d_off.data_ptr(), n, d_units.data_ptr(), d_uoff.data_ptr(),
                           d_bad.data_ptr(), stream=st)
        _lib.check(cm.lib.ldgpu_preprocess_device(cm.h, ctypes.c_void_p(d_units.data_ptr()),
                                                  ctypes.c_void_p(d_uoff.data_ptr()), n,
                                                  ctypes.c_void_p(d_loc.data_ptr()), flags,
                                                  ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(d_ooff.data_ptr()),
                                                  ctypes.c_void_p(d_host.data_ptr()), ctypes.c_void_p(st)), cm.lib)
        m.score_device(d_out.data_ptr(), nb, d_ooff.data_ptr(), n, d_lab.data_ptr(), stream=st)
    stream.synchronize()
    assert not d_bad.cpu().numpy().any()
    units, uoff = DeviceCaseMap.pack_units(texts)
    assert np.array_equal(d_uoff.cpu().numpy(), uoff)
    assert np.array_equal(d_units.cpu().numpy().view(np.uint16)[:int(uoff[-1])], units[:int(uoff[-1])])
    out, out_off, host = cm.run(units, uoff, loc, flags)
    assert np.array_equal(d_host.cpu().numpy(), host) and np.array_equal(d_ooff.cpu().numpy(), out_off)
    assert np.array_equal(d_out.cpu().numpy()[:int(out_off[-1])], out[:int(out_off[-1])])
    want, _ = m.score(*encoding.pack_score([intended_special_char_clean(java_lower(t, l))
                                            for t, l in zip(texts, langs)]))
    keep = host == 0   # (the preprocessors leave a context-dependent document to the host: empty here)
    assert keep[2000:].all() and keep.sum() > 1000
    assert np.array_equal(d_lab.cpu().numpy()[keep], want[keep])


# -------------------------------------------------------------------- fused
# (name: L, gram lengths, key lengths, table form, check of DeviceModel.info())
TABLES = {
    "mask": (20, (1, 2, 3), (1, 2, 3), "mask", lambda i: i["mode"] == 0),
    "count": (20, (1, 2, 3), (1, 2, 3), "uniform", lambda i: i["mode"] == 2),
    "dense": (9, (1, 2, 3), (1, 2, 3), "dense", lambda i: i["mode"] == 1),
}


@functools.lru_cache(maxsize=None)
def fused_model(kind, variant="product"):
    L, grams, key_lens, form, ok = TABLES[kind]
    m = DeviceModel(B.byte_table(SEED, L, list(key_lens), 300, form), L, list(grams), variant=variant)
    assert ok(m.info()), (kind, m.info())
    return m


@functools.lru_cache(maxsize=None)
def fused_corpus(kind, n_docs=3000):
    """(texts, their UTF-8 documents, ldgpu_score's labels and scores of their
    SCORE encoding, the score row of an empty document)."""
    L = TABLES[kind][0]
    _, texts = B.texts(SEED, L, n_docs, 0, 300)
    docs = [t.encode("utf-8") for t in texts]
    m = fused_model(kind)
    labels, scores = m.score(*encoding.pack_score(texts), want_scores=True)
    empty = m.score(*encoding.pack([b""]), want_scores=True)[1][0]
    for a in (labels, scores, empty):
        a.setflags(write=False)
    return texts, docs, labels, scores, empty


def splice(docs, labels, scores, empty, at):
    """`docs` with ill-formed documents put in front of the indices `at`, and
    what the fused call must give: -1 and the empty row there."""
    out, lab, sc, bad = [], [], [], []
    at = set(at)
    for i, d in enumerate(docs):
        if i in at:
            bad.append(len(out))
            out.append(ILL[len(bad) % len(ILL)])
            lab.append(-1)
            sc.append(empty)
        out.append(d)
        lab.append(int(labels[i]))
        sc.append(scores[i])
    return out, np.array(lab, dtype=np.int32), np.array(sc), bad


def pinned(a):
    p = PinnedArray(a.shape, a.dtype)
    p.array[...] = a
    return p


@pytest.mark.parametrize("kind", ["mask", "count", "dense"])
def test_fused_host_form(kind):
    texts, docs, labels, scores, empty = fused_corpus(kind)
    m = fused_model(kind)
    data, off = utf8.pack_utf8(docs)
    assert sum(not t.isascii() for t in texts) > 0.8 * len(texts)
    got_l, got_s = m.score_utf8(data, off, want_scores=True)
    assert (got_l >= 0).all()       # no document left out of the comparison
    assert np.array_equal(got_l, labels) and np.array_equal(bits(got_s), bits(scores))
    assert np.array_equal(m.score_utf8(data, off)[0], labels)          # the labels-only paths
    # ill-formed documents at known indices, first and last among them
    at = [0, 1, 7, 1500, 1501, len(docs) - 1]
    docs2, lab2, sc2, bad = splice(docs, labels, scores, empty, at)
    docs2.append(ILL[0])
    lab2, sc2 = np.append(lab2, np.int32(-1)), np.vstack([sc2, empty])
    data2, off2 = utf8.pack_utf8(docs2)
    got_l, got_s = m.score_utf8(data2, off2, want_scores=True)
    assert np.array_equal(got_l, lab2) and np.array_equal(bits(got_s), bits(sc2))
    assert np.flatnonzero(got_l < 0).tolist() == bad + [len(docs2) - 1]
    assert np.array_equal(m.score_utf8(data2, off2)[0], lab2)
    # page-locked buffers: copied from / to directly
    pd, po, pl = pinned(data2), pinned(off2), PinnedArray(len(lab2), np.int32)
    pl.array[:] = -7
    out_l, _ = m.score_utf8(pd.array, po.array, out=pl.array)
    assert out_l is pl.array and np.array_equal(out_l, lab2)
    for p in (pd, po, pl):
        p.close()


@pytest.mark.parametrize("kind", ["mask", "count", "dense"])
def test_fused_host_form_in_chunks(kind, monkeypatch):
    """The diagnostics library with chunks of 5 documents: an ill-formed
    document first and last of a chunk, the results unchanged."""
    monkeypatch.setenv("LDGPU_SCORE_CHUNK_DOCS", "5")
    _, docs, labels, scores, empty = fused_corpus(kind)
    docs, labels, scores = docs[:203], labels[:203], scores[:203]
    docs2, lab2, sc2, bad = splice(docs, labels, scores, empty, [0, 3, 4, 7, 200])
    assert bad == [0, 4, 6, 10, 204]
    for shift in range(5):          # every position of a chunk, whatever the splice made of it
        d = [b"ok"] * shift + docs2
        data, off = utf8.pack_utf8(d)
        m = fused_model(kind, "diag")
        got_l, got_s = m.score_utf8(data, off, want_scores=True)
        assert np.array_equal(got_l[shift:], lab2) and np.array_equal(bits(got_s[shift:]), bits(sc2))
        assert np.array_equal(m.score_utf8(data, off)[0][shift:], lab2)


@pytest.mark.parametrize("kind", ["mask", "count", "dense"])
def test_fused_device_form(kind, monkeypatch):
    """Torch tensors on a non-default stream equal the host form; the
    diagnostics library in chunks of 7 documents too."""
    import torch
    _, docs, labels, scores, empty = fused_corpus(kind)
    docs2, lab2, sc2, _ = splice(docs[:500], labels[:500], scores[:500], empty, [0, 6, 7, 250, 499])
    data, off = utf8.pack_utf8(docs2)
    n, L = len(docs2), TABLES[kind][0]
    host_l, host_s = fused_model(kind).score_utf8(data, off, want_scores=True)
    assert np.array_equal(host_l, lab2) and np.array_equal(bits(host_s), bits(sc2))
    dev = torch.device("cuda", 0)
    monkeypatch.setenv("LDGPU_UTF8_CHUNK_DOCS", "7")
    for variant in ("product", "diag"):
        m = fused_model(kind, variant)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            d_data, d_off = torch.from_numpy(np.array(data)).to(dev), torch.from_numpy(np.array(off)).to(dev)
            d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
            d_lab2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
            d_sc = torch.full((n, L), -7.0, dtype=torch.float64, device=dev)
            m.score_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, d_lab.data_ptr(),
                                d_sc.data_ptr(), stream=stream.cuda_stream)
            m.score_utf8_device(d_data.data_ptr(), len(data), d_off.data_ptr(), n, d_lab2.data_ptr(),
                                stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_lab.cpu().numpy(), host_l) and np.array_equal(d_lab2.cpu().numpy(), host_l)
        assert np.array_equal(bits(d_sc.cpu().numpy()), bits(host_s))


# --------------------------------------------------------------- Python API
def test_python_api():
    import pandas as pd
    L, grams = TABLES["mask"][0], list(TABLES["mask"][1])
    texts, docs, labels, _, _ = fused_corpus("mask")
    model = LanguageDetectorModel(B.byte_table(SEED, L, [1, 2, 3], 300, "mask"), grams, [f"l{i}" for i in range(L)],
                                  device=0)
    docs2 = list(docs[:400])
    for i, ill in zip((0, 17, 200, 399), ILL):
        docs2[i] = docs2[i][:40] + ill + docs2[i][40:]
    bad = [i for i, d in enumerate(docs2) if utf8corpus.codec(d)[0]]
    assert set(bad) >= {0, 17, 399}
    want_l, want_s = model.predict_indices([d.decode("utf-8", "replace") for d in docs2], want_scores=True)
    got_l, got_s = model.predict_indices_utf8(docs2, want_scores=True)
    assert np.array_equal(got_l, want_l) and np.array_equal(bits(got_s), bits(want_s))
    assert np.array_equal(model.predict_indices_utf8(utf8.pack_utf8(docs2))[0], want_l)
    with pytest.raises(UnicodeDecodeError) as e:
        model.predict_indices_utf8(docs2, errors="strict")
    assert e.value.object == docs2[bad[0]]
    assert np.array_equal(model.predict_indices_utf8(docs[:400], errors="strict")[0], labels[:400])
    with pytest.raises(ValueError):
        model.predict_indices_utf8(docs2, errors="ignore")
    df = pd.DataFrame({"fulltext": docs2, "id": range(len(docs2))})
    out = model.transformUtf8(df)
    assert list(out.columns) == ["fulltext", "id", "lang"]
    assert list(out["lang"]) == [f"l{i}" for i in want_l]
    with pytest.raises(ValueError, match="already exists"):
        model.transformUtf8(out)
    with pytest.raises(ValueError, match="BinaryType"):
        model.transformUtf8(pd.DataFrame({"fulltext": ["text"]}))


# ---------------------------------------------------------- argument checks
def test_argument_checks():
    import torch
    lib = _lib.load()
    ctx = _lib.context(0)
    m = fused_model("mask")
    E, U, OK = _lib.LDGPU_EINVAL, _lib.LDGPU_EUNSUPPORTED, _lib.LDGPU_OK

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    data, off = utf8.pack_utf8([b"ab", b"\xc3\xa9", b""])
    out, ooff, host = np.zeros(8, np.uint16), np.zeros(4, np.int64), np.zeros(3, np.uint8)

    def dec(ctx=ctx, data=data, off=off, n=3, flags=0, out=out, ooff=ooff, host=host):
        return lib.ldgpu_utf8_decode(ctx, ptr(data), ptr(off), n, flags, ptr(out), ptr(ooff), ptr(host))

    assert dec() == OK and ooff.tolist() == [0, 2, 3, 3]
    assert dec(flags=_lib.PRE_LOWER) == E and b"flags" in lib.ldgpu_last_error()
    assert dec(flags=8) == E and dec(flags=_lib.PRE_LOW_BYTES | _lib.PRE_CLEAN) == E
    assert dec(ctx=None) == E and dec(out=None) == E and dec(ooff=None) == E and dec(host=None) == E
    assert b"NULL" in lib.ldgpu_last_error()
    assert dec(data=None) == E and dec(off=None) == E and dec(n=-1) == E
    assert dec(off=np.array([0, 3, 2, 4], dtype=np.int64)) == E and b"decrease" in lib.ldgpu_last_error()
    assert dec(off=np.array([-1, 2, 4, 4], dtype=np.int64)) == E
    assert dec(n=0, data=None, out=None, host=None) == OK and ooff[0] == 0

    dev = torch.device("cuda", 0)
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(off).to(dev)
    d_o = torch.zeros(8, dtype=torch.int64, device=dev)

    def ddec(ctx=ctx, p=d.data_ptr(), off=d_off.data_ptr(), n=3, flags=0, out=d.data_ptr() + 16, ooff=d_o.data_ptr(),
             host=d.data_ptr() + 48):
        c = ctypes.c_void_p
        return lib.ldgpu_utf8_decode_device(ctx, c(p), c(off), n, flags, c(out), c(ooff), c(host), None)

    assert ddec() == OK
    assert ddec(flags=2) == E and b"flags" in lib.ldgpu_last_error()
    assert ddec(ctx=None) == E and ddec(n=-1) == E and ddec(off=0) == E and ddec(out=0) == E and ddec(ooff=0) == E
    assert ddec(host=0) == E and b"NULL" in lib.ldgpu_last_error()
    assert ddec(p=d.data_ptr() + 1) == E and b"aligned" in lib.ldgpu_last_error()
    assert ddec(n=2 ** 31 - 1) == U
    torch.cuda.synchronize()

    labels = np.full(3, -7, dtype=np.int32)

    def sc(model=m.h, data=data, off=off, n=3, lab=labels):
        return lib.ldgpu_score_utf8(model, ptr(data), ptr(off), n, ptr(lab), None)

    assert sc() == OK and (labels >= 0).all()
    assert sc(model=None) == E and sc(lab=None) == E and sc(data=None) == E and sc(off=None) == E and sc(n=-1) == E
    assert sc(off=np.array([0, 3, 2, 4], dtype=np.int64)) == E and b"decrease" in lib.ldgpu_last_error()
    assert sc(n=0, lab=None, data=None) == OK
    # a document of 2^28 bytes: offsets only, no buffer of that size behind them
    assert sc(off=np.array([0, 2, 2 + (1 << 28), 3 + (1 << 28)], dtype=np.int64)) == U
    assert b"limit" in lib.ldgpu_last_error()
    with pytest.raises(NotImplementedError):
        m.score_utf8(data, np.array([0, 1 << 28], dtype=np.int64))

    d_lab = torch.zeros(4, dtype=torch.int32, device=dev)

    def dsc(model=m.h, p=d.data_ptr(), nb=8, off=d_off.data_ptr(), n=3, lab=d_lab.data_ptr()):
        c = ctypes.c_void_p
        return lib.ldgpu_score_utf8_device(model, c(p), nb, c(off), n, c(lab), None, None)

    assert dsc() == OK
    assert dsc(model=None) == E and dsc(n=-1) == E and dsc(off=0) == E and dsc(lab=0) == E and dsc(p=0) == E
    assert dsc(nb=-1) == E and dsc(p=d.data_ptr() + 2) == E and b"aligned" in lib.ldgpu_last_error()
    assert dsc(n=0, off=0, lab=0) == OK
    torch.cuda.synchronize()
