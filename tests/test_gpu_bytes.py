"""GPU parity of FIT and SCORE on non-ASCII bytes (tests/bytecorpus.py): UTF-8
text of many scripts, the low bytes of its UTF-16 units, runs of 0x00 and
0xFF.  Every other random-parity test draws from a few ASCII letters, where a
read past a document's end, a signed byte compare, a short sort-bit range or
an unexercised rank of the direct tables cannot show.  Every comparison is
exact, against the C restatement (itself pinned on these bytes against the
Python oracle in test_oracle.py)."""
import functools
import math

import numpy as np
import pytest

import bytecorpus as B
import geometry
import ldoracle as O
import ldoracle_c as OC
from languagedetection import LanguageDetector, encoding
from languagedetection.runtime import DeviceCounts, DeviceModel
from test_gpu_fit import COUNT_VARIANTS

pytestmark = pytest.mark.gpu

SEED = 11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ FIT counts
@functools.lru_cache(maxsize=None)
def fit_corpus(L):
    """600 text documents of 0-300 units in UTF-8 followed by raw_docs.  The
    0xFF runs belong to the highest language id, the 0x00 runs alternate
    between language 0 and the highest; some text and some random documents
    carry the unsupported label -1."""
    labels, txts = B.texts(SEED, L, 600, 0, 300)
    raw = B.raw_docs(SEED)
    rng = np.random.default_rng(SEED + L)
    rl = rng.integers(0, L, size=len(raw)).astype(np.int32)
    n_edge = 2 * len(B.EDGE_LENGTHS)
    rl[1:n_edge:2] = L - 1
    rl[0:n_edge:4] = 0
    rl[2:n_edge:4] = L - 1
    rl[n_edge + 20::11] = -1
    labels = labels.copy()
    labels[::29] = -1
    data, off = encoding.pack([encoding.fit_bytes(t) for t in txts] + raw)
    for a in (data, off):
        a.setflags(write=False)
    return data, off, np.concatenate([labels, rl])


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def fit_expect(L, grams):
    """The C restatement's counts of the corpus in sparse form (key bytes, key
    offsets, pair offsets, pair languages, pair counts, in (length, bytes,
    language) order: no dense row of L per gram), once per shape."""
    data, off, dl = fit_corpus(L)
    return _frozen(OC.count_sparse(data, off, dl, L, list(grams)))


@functools.lru_cache(maxsize=None)
def fit_expect_two_calls(L, grams):
    """... of the corpus followed by its first 300 documents once more: what two
    accumulating calls must leave."""
    data, off, dl = fit_corpus(L)
    n, n2 = int(off[-1]), int(off[300])
    d2 = np.concatenate([data[:n], data[:n2], np.zeros(8, np.uint8)])
    return _frozen(OC.count_sparse(d2, np.concatenate([off, n + off[1:301]]), np.concatenate([dl, dl[:300]]), L,
                                   list(grams)))


def keys_of(sparse):
    kb, ko = sparse[0].tobytes(), sparse[1]
    return [kb[ko[i]:ko[i + 1]] for i in range(len(ko) - 1)]


def dense_of(sparse, L):
    _, ko, po, pl, pc = sparse
    rows = np.zeros((len(ko) - 1, L), dtype=np.int64)
    rows[np.repeat(np.arange(len(ko) - 1), np.diff(po)), pl] = pc
    return rows


def assert_sparse_equal(got, expect, times=1):
    assert len(got[1]) == len(expect[1])
    for i, (g, e) in enumerate(zip(got, expect)):
        assert np.array_equal(g, e * times if i == 4 else e), ("key_bytes", "key_offsets", "pair_offsets",
                                                                 "pair_langs", "pair_counts")[i]


FIT_SHAPES = [
    (20, (1, 2, 3, 4, 5)),            # one-word records
    (200, (1, 2, 3, 4, 5, 6, 7)),     # FIT v5, the sort key's 64 bits all in use
    (255, (7, 2)),                    # the largest L on FIT v5: language 254 beside 0xFF bytes and the sentinel
    (256, (1, 2, 7)),                 # the first L on two-word FIT v4
    (5, (2, 9, 15)), (30, (8, 1)),    # three-word records, wide keys
    (4, (3, 20)),                     # general keys
]


@pytest.mark.parametrize("variant,env", COUNT_VARIANTS)
@pytest.mark.parametrize("L,grams", FIT_SHAPES)
def test_count_paths_match_oracle_on_bytes(L, grams, variant, env, monkeypatch):
    """test_count_paths_match_oracle's variant matrix on the byte corpus, two
    calls that accumulate: keys and every (gram, language) count exactly the
    oracle's (compared in sparse form: the 600k grams of L = 200 have no
    dense rows here)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    data, off, dl = fit_corpus(L)
    expect = fit_expect_two_calls(L, grams)
    counts = DeviceCounts(L, list(grams), variant=variant)
    counts.count(data, off, dl)
    counts.count(data[:int(off[300])], off[:301], dl[:300])
    got = counts.export_sparse()
    counts.close()
    assert_sparse_equal(got, expect)
    first = expect[0][expect[1][:-1]]                       # each key's first byte
    assert (first >= 0x80).sum() > len(first) // 3 and (expect[0] == 0).any()
    assert expect[3].max() == L - 1


def _counted(L, grams):
    data, off, dl = fit_corpus(L)
    c = DeviceCounts(L, list(grams))
    c.count(data, off, dl)
    return c


@pytest.mark.parametrize("L,grams", [(20, (1, 2, 3, 4, 5)), (200, (1, 2, 3, 4, 5, 6, 7)), (255, (7, 2))])
def test_device_export_add_roundtrip_on_bytes(L, grams):
    """export_device / add_device: a packed u64 key holds its bytes
    little-endian under the length byte, so 0x00 bytes are payload and a 7-byte
    key ending in 0xFF puts it right below the length.  Added twice."""
    expect = fit_expect(L, grams)
    a = _counted(L, grams)
    k, c = a.export_device()
    b = DeviceCounts(L, list(grams))
    b.add_device(k, c)
    b.add_device(k, c)
    del k, c
    assert_sparse_equal(a.export_sparse(), expect)
    assert_sparse_equal(b.export_sparse(), expect, times=2)
    a.close()
    b.close()
    kb, ko = expect[0], expect[1]
    full = np.diff(ko) == max(grams)
    assert (kb[ko[1:][full] - 1] == 0xFF).any() and (kb[ko[1:][full] - 1] == 0x00).any()


@pytest.mark.parametrize("L,grams", [(20, (1, 2, 3, 4, 5)), (5, (2, 9, 15)), (4, (3, 20))])
def test_sparse_export_add_roundtrip_on_bytes(L, grams):
    """export_sparse in ranges / add_sparse, each range added twice."""
    expect = fit_expect(L, grams)
    okeys, ocnt = keys_of(expect), dense_of(expect, L)
    a = _counted(L, grams)
    n = len(okeys)
    assert a.size() == n
    b = DeviceCounts(L, list(grams))
    cuts = [0, 1, n // 3, n // 2, n]
    for first, last in zip(cuts[:-1], cuts[1:]):
        part = a.export_sparse(first, last - first)
        assert keys_of(part) == okeys[first:last]
        assert np.array_equal(dense_of(part, L), ocnt[first:last])
        b.add_sparse(*part)
        b.add_sparse(*part)
    assert_sparse_equal(b.export_sparse(), expect, times=2)


@pytest.mark.parametrize("L,grams", [(5, (2, 9, 15)), (4, (3, 20))])
def test_counts_add_wide_and_long_keys_on_bytes(L, grams):
    """ldgpu_counts_add of keys of every length (one-word, wide, long) into a
    table created for other gram lengths, twice."""
    expect = fit_expect(L, grams)
    okeys, ocnt = keys_of(expect), dense_of(expect, L)
    assert max(len(k) for k in okeys) == max(grams)
    b = DeviceCounts(L, [1])
    b.add(okeys, ocnt)
    b.add(okeys[::-1], ocnt[::-1])
    assert_sparse_equal(b.export_sparse(), expect, times=2)


# ----------------------------------------------------------------------- top-K
@pytest.mark.parametrize("L,grams,n_docs,len_hi", [
    (8, (1, 2, 3), 500, 120), (70, (1, 2, 3), 1200, 80),
    (520, (1, 2, 3), 4160, 5),        # more than 512 languages: the single-rank top-K without the per-length split
    (8, (2, 9), 400, 60),             # wide keys: host selection
    (8, (3, 20), 400, 60),            # general keys
])
def test_fit_table_tie_order_on_bytes(L, grams, n_docs, len_hi):
    """fit_table and fit_table_masks against the rule over the oracle's
    counts, at three profile sizes: (a) the cut inside a tie group whose keys
    start below and at or above 0x80 (the (length, unsigned bytes) order
    decides which are kept), (b) some languages padded with zero-valued grams
    and others not, (c) every gram."""
    labels, txts = B.texts(SEED + 1, L, n_docs, 2, len_hi)
    data, off = B.fit_pack(txts)
    okeys, ocnt = OC.count(data, off, labels, L, list(grams))
    Ka, Kb, Kc, split = B.k_regimes(okeys, ocnt)
    present = (ocnt > 0).sum(axis=0)
    assert split, "no language's cut splits a mixed-sign tie group"
    assert Ka < present.min() < Kb <= present.max() < Kc and Kc > len(okeys)
    counts = DeviceCounts(L, list(grams))
    counts.count(data, off, labels)
    for K in (Ka, Kb, Kc):
        dense = counts.fit_table(K)
        expect = B._topk_table_from_counts(okeys, ocnt, L, K)
        assert dense.keys() == expect.keys(), (K, sorted(dense.keys() ^ expect.keys())[:5])
        assert dense == expect
        kb, ko, masks, vals = counts.fit_table_masks(K)
        b = kb.tobytes()
        mkeys = [b[ko[i]:ko[i + 1]] for i in range(len(ko) - 1)]
        assert len(set(mkeys)) == len(mkeys) and set(mkeys) == expect.keys()
        rows = np.array([expect[k] for k in mkeys]).reshape(len(mkeys), L)
        lang = np.arange(L)
        member = ((masks[:, lang // 64] >> (lang % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert np.array_equal(bits(np.where(member, np.asarray(vals)[:, None], 0.0)), bits(rows))
    counts.close()


# ------------------------------------------------------------------------ SCORE
def score_docs(L, n_text, len_hi):
    """score_pack's bytes of `n_text` texts interleaved with raw_docs; all-zero
    documents in the middle (raw_docs' own) and last in the buffer."""
    _, txts = B.texts(SEED, L, n_text, 0, len_hi)
    docs = B.interleave([encoding.score_bytes(t) for t in txts], B.raw_docs(SEED))
    return docs + [b"\x00" * 17, b"", b"\x00" * 64, b"\x00" * 9, b"\x00" * 7]


def check(model, table, L, grams, data, off, edata=None):
    """Labels and fp64 score bits of `model` on (data, off) equal the C
    restatement's on (edata or data, off); labels-only too."""
    ol, os_ = OC.Table(table, L).score(list(grams), data if edata is None else edata, off, want_scores=True,
                                       nthreads=8)
    labels, scores = model.score(data, off, want_scores=True)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    assert np.array_equal(bits(scores), bits(os_))
    only, _ = model.score(data, off, want_scores=False)
    assert np.array_equal(only, ol), np.nonzero(only != ol)[0][:10]
    return ol, os_


def score_device(model, L, buf, n_bytes, off):
    """ldgpu_score_device on a torch copy of `buf` (its tail beyond n_bytes included)."""
    import torch
    dev = torch.device("cuda", 0)
    d_bytes = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
    n = len(off) - 1
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_sc = torch.full((n, L), -7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    model.score_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, d_lab.data_ptr(), d_sc.data_ptr(), st)
    d_only = torch.full((n,), -7, dtype=torch.int32, device=dev)
    model.score_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, d_only.data_ptr(), 0, st)
    torch.cuda.synchronize()
    return d_lab.cpu().numpy(), d_sc.cpu().numpy(), d_only.cpu().numpy()


@pytest.fixture(params=["mask", "dense", "uniform", "uniform-replay"])
def form_path(request, monkeypatch):
    """(table form, library variant, expected mode): uniform tables on the
    count kernel and, through the diagnostics library, on the ordered replay."""
    if request.param == "uniform-replay":
        monkeypatch.setenv("LDGPU_NO_COUNT_MODE", "1")
        return "uniform", "diag", 0
    return request.param, "product", {"mask": 0, "dense": 1, "uniform": 2}[request.param]


@pytest.mark.parametrize("L", [3, 65, 256])
@pytest.mark.parametrize("grams", [(1, 2, 3, 4, 5), (1, 2, 7)])
def test_score_zero_keys_and_reads_past_a_document(L, grams, form_path):
    """Keys of 0x00 bytes (and 0xFF, and keys cut from the documents) on
    documents that end in, consist of, or are followed by 0x00: a window read
    past a document's end -- into the zero pad or the next document -- is then
    a key and changes the score.  Then the pad beyond the last document holds
    0xA5 and 0xA5 / 0xA5A5 are keys: nothing may change, through the host call
    and through ldgpu_score_device."""
    form, variant, mode = form_path
    table = B.byte_table(SEED, L, list(grams), 700, form)
    docs = score_docs(L, 150, 120)
    data, off = encoding.pack(docs)
    m = DeviceModel(table, L, list(grams), variant=variant)
    assert m.info()["mode"] == mode
    ol, os_ = check(m, table, L, grams, data, off)
    assert len(np.unique(ol)) > 1
    m.close()
    # what a read of one byte past each document's end into a zero pad would give: other scores everywhere
    d1, o1 = encoding.pack([d + b"\x00" for d in docs])
    _, over = OC.Table(table, L).score(list(grams), d1, o1, want_scores=True, nthreads=8)
    assert (bits(over) != bits(os_)).any(axis=1).all()
    # the same documents, 0xA5 beyond the last one
    row = next(iter(table.values()))
    table2 = dict(table)
    table2[b"\xa5"] = row
    table2[b"\xa5\xa5"] = row[::-1]
    n = int(off[-1])
    padded = np.concatenate([data[:n], np.full(((n + 3) & ~3) + 32 - n, 0xA5, dtype=np.uint8)])
    m2 = DeviceModel(table2, L, list(grams), variant=variant)
    assert m2.info()["mode"] == mode
    ol2, os2 = check(m2, table2, L, grams, padded, off, edata=data)
    dl, ds, donly = score_device(m2, L, padded, n, off)
    assert np.array_equal(dl, ol2) and np.array_equal(bits(ds), bits(os2)) and np.array_equal(donly, ol2)


@pytest.mark.parametrize("L,n_keys", [(20, 2500), (100, 900), (255, 900)])
def test_packs_of_zero_and_ff_documents(L, n_keys):
    """Labels-only count mode on 3000 documents of 0-100 bytes (packs of short
    documents in one superblock), among them runs of adjacent all-0x00 and
    all-0xFF documents: a window that crossed a document boundary would be one
    of the table's 0x00 / 0xFF keys.  (A model packs only where the packs'
    counters cost no resident workgroup: with one slice of languages, where the
    filter image is larger -- hence the key counts.)"""
    grams = [1, 2, 3, 4, 5]
    table = B.byte_table(SEED, L, grams, n_keys, "uniform")
    for k in (b"\x00" * 3, b"\x00" * 5, b"\xff" * 2, b"\xff" * 4, b"\x00\xff", b"\xff\x00"):
        table.setdefault(k, table[b"\x00"][::-1])
    rng = np.random.default_rng(SEED + L)
    _, txts = B.texts(SEED, L, 2520, 0, 50)     # an astral unit is two bytes: 0-100 bytes
    t = [encoding.score_bytes(x) for x in txts]

    def run(byte):
        return [byte * int(n) for n in rng.integers(1, 70, size=80)]
    docs = (t[:300] + run(b"\x00") + t[300:900] + run(b"\xff") + t[900:1500] + B.interleave(run(b"\x00"), run(b"\xff"))
            + t[1500:] + run(b"\xff") + run(b"\x00"))
    assert max(len(d) for d in docs) <= 100 and len(docs) == 3000
    data, off = encoding.pack(docs)
    m = DeviceModel(table, L, grams)
    info = m.info()
    assert info["mode"] == 2 and "packs" in info["layout"], info
    ol, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    labels, _ = m.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    assert len(np.unique(ol)) > 2
    # 3000 documents are one per wave: packs form only on the tiled corpus
    geometry.check_tiled_labels(m, data, off, ol, max(grams))


# ---------------------------------------------------------------- direct tables
def direct_keys(rng, n2):
    """All 256 one-byte keys, n2 distinct two-byte keys drawn uniformly from
    0..65535, 300 three-byte keys."""
    two = rng.choice(65536, size=n2, replace=False)
    keys = [bytes([c]) for c in range(256)] + [bytes([int(v) & 0xFF, int(v) >> 8]) for v in two]
    keys += list({bytes(r) for r in rng.integers(0, 256, size=(300, 3), dtype=np.uint8)})
    # a two-byte key's entry sits at its word's rank (the keys in the bitmap
    # words before its own: base2, 16 bits) plus its rank in the word: most
    # word ranks pass 255 (a byte), and nearly every one of the 2048 words
    # holds a key
    per_word = np.bincount(two >> 5, minlength=2048)
    word_rank = np.cumsum(per_word) - per_word
    assert (word_rank > 255).mean() > 0.9 and word_rank.max() > 5000
    assert (per_word > 0).mean() > 0.9, (per_word > 0).sum()
    assert all((two >> 14 == q).sum() > 1000 for q in range(4))       # every quarter of the bitmap
    return keys


def direct_docs(rng):
    lens = rng.integers(0, 400, size=800)
    lens[:10] = [0, 1, 2, 3, 6, 7, 64, 65, 256, 255]
    return encoding.pack([bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8)) for n in lens])


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("L", [20, 255])
def test_direct_tables_full_byte_range(L, direct, monkeypatch):
    """One-language rows of one value with 6000 of the 65536 two-byte keys:
    the direct tables' word ranks (base2), the bitmap word mapping and every
    quarter of the bitmaps in use, on uniformly random documents; then all of
    them through verification (LDGPU_NO_DIRECT, diagnostics library)."""
    if not direct:
        monkeypatch.setenv("LDGPU_NO_DIRECT", "1")
    rng = np.random.default_rng(L)
    v = math.log(2.0)
    table = {}
    for k in direct_keys(rng, 6000):
        row = [0.0] * L
        row[int(rng.integers(0, L))] = v
        table[k] = row
    assert any(table[k][L - 1] for k in table if len(k) == 2)
    data, off = direct_docs(rng)
    grams = [1, 2, 3]
    m = DeviceModel(table, L, grams, variant="product" if direct else "diag")
    info = m.info()
    assert info["mode"] == 2 and ("direct" in info["layout"]) == direct, info
    check(m, table, L, grams, data, off)


def test_class_mode_direct_tables_full_byte_range():
    """Class mode's direct tables (an entry = language | class << 6) at L = 40
    with two values, labels only."""
    L, grams = 40, [1, 2, 3]
    rng = np.random.default_rng(40)
    values = [math.log(2.0), math.log(1.5)]
    table = {}
    for k in direct_keys(rng, 6000):
        v = values[int(rng.integers(0, 2))]
        if len(k) <= 2:
            row = [0.0] * L
            row[int(rng.integers(0, L))] = v
        else:
            m = rng.random(L) < 0.2
            m[int(rng.integers(0, L))] = True
            row = [v if b else 0.0 for b in m]
        table[k] = row
    data, off = direct_docs(rng)
    m = DeviceModel(table, L, grams)
    lay = m.info()["layout"]
    assert "classes" in lay and "direct" in lay, lay
    ol, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    labels, _ = m.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    _, _, donly = score_device(m, L, np.concatenate([data, np.zeros(16, np.uint8)]), len(data), off)
    assert np.array_equal(donly, ol)


# ------------------------------------------------------- wide and general keys
@pytest.mark.parametrize("grams", [(8,), (1, 3, 8, 12, 15), (16,), (3, 20)])
@pytest.mark.parametrize("form", ["uniform", "mask", "dense"])
def test_wide_and_general_keys_on_bytes(grams, form):
    """Keys of 8..15 bytes (two words) and beyond (the general table), among
    them the all-0x00 and all-0xFF key of every length: documents of 7 / 8 / 9
    and 15 / 16 / 17 zero bytes, the last ones at the end of the buffer, are a
    partial window (the whole document, a shorter key) or full windows."""
    L = 70 if form == "mask" and max(grams) > 15 else 12
    lens = sorted(set(grams) | {max(1, g - 3) for g in grams} | {max(1, g - 1) for g in grams})
    table = B.byte_table(SEED, L, lens, 700, form)
    for n in (7, 8, 9, 15, 16, 17):
        if n <= max(grams):
            table.setdefault(b"\x00" * n, table[b"\x00"])
    docs = score_docs(L, 200, 120) + [b"\x00" * n for n in (15, 16, 17, 7, 8, 9)]
    data, off = encoding.pack(docs)
    m = DeviceModel(table, L, list(grams))
    lay = m.info()["layout"]
    assert ("general_keys" in lay) == (max(grams) > 15), lay
    assert max(grams) > 15 or max(grams) < 8 or "wide_keys" in lay, lay
    ol, os_ = check(m, table, L, grams, data, off)
    assert os_[-6:].any(axis=1).all()        # each of the six zero documents hits


# ------------------------------------------------------------------ end to end
def test_fit_then_transform_end_to_end_on_bytes():
    """LanguageDetector.fit on text of six scripts, transform of other text:
    the model is fitted on UTF-8 bytes and scored on the low bytes of UTF-16
    units (LanguageDetector.scala:37, LanguageDetectorModel.scala:161), so the
    two encodings differ -- table and labels equal the oracle's."""
    import pandas as pd
    L, grams, K = 6, [1, 2, 3], 200
    names = [f"l{i}" for i in range(L)]
    tl, train = B.texts(SEED, L, 400, 10, 120)
    df = pd.DataFrame({"lang": [names[i] for i in tl], "fulltext": train})
    model = LanguageDetector(names, grams, K).fit(df)
    expect_table = O.fit(list(zip(df["lang"], train)), names, grams, K)
    got = {encoding.gram_key(g): list(r) for g, r in model.gramProbabilities.items()}
    assert got == expect_table
    _, texts = B.texts(SEED, L, 300, 0, 100)      # the same languages, other documents
    assert any(encoding.fit_bytes(t) != encoding.score_bytes(t) for t in texts)
    out = model.transform(pd.DataFrame({"fulltext": texts}))
    expect = O.transform(texts, expect_table, names, grams)
    assert list(out["lang"]) == expect
    assert len(set(expect)) > 1
