"""GPU parity of count mode's direct 2-byte tables where a lane resolves the
hits of all its sub-blocks in one batch (direct_count<2>, ldgpu_score.hip): a
hand-built table whose 2-byte keys sit on the edges of the bitmap / rank-base /
language lookup, and documents that put hits on the edges of the batch.  Every
case compares with the C oracle (labels, and the fp64 scores bit for bit where
the path gives them), and asserts on the host -- from the table and the bytes --
that its corpus has the property it is there for."""
import math

import numpy as np
import pytest

import geometry
import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

L = 5
GRAMS = [1, 2, 3]
FILL = 0x2E  # '.': in no key

# 2-byte keys -> language.  Key b0 b1 is bit (b0 & 31) of bitmap word
# (b0 | b1 << 8) >> 5; its language is entry (keys in the words before) + (keys
# of its word below its bit) of the language list.
KEYS2 = {
    b"\x60a": 4,      # bit 0 of the word of `a..\x7fa
    b"aa": 0,         # bit 1: rank 1
    b"ba": 1,         # rank 2
    b"ca": 2,         # rank 3
    b"ea": 3,
    b"za": 4,
    b"\x7fa": 3,      # bit 31: the word's last rank
    b"\x00\x00": 2,   # first word, bit 0: entry 0 of the language list
    b"\xff\xff": 1,   # last word, bit 31: the list's last entry
    b"ab": 3,         # other words
    b"bc": 0,
    b"\x00a": 1,
}
KEYS1 = {b"q": 3, b"z": 2}          # "za" starts with a 1-byte key: both hit one position
KEYS3 = {b"xyz": 0, b"a.b": 4, b"q.q": 1}
QUAD = [b"aa", b"ba", b"ca", b"\x7fa"]  # four languages: one per sub-block of a lane


def word_of(k):
    return (k[0] | k[1] << 8) >> 5


def table_of(values):
    """Rows of one language each; values[i % len(values)] for the i-th key."""
    t = {}
    for i, (k, lang) in enumerate({**KEYS1, **KEYS2, **KEYS3}.items()):
        row = [0.0] * L
        row[lang] = values[i % len(values)]
        t[k] = row
    return t


def hits2(doc):
    """Positions of the document's 2-byte windows that are table keys."""
    return [p for p in range(len(doc) - 1) if bytes(doc[p:p + 2]) in KEYS2]


def doc_with(n, at):
    """n filler bytes with the given byte strings at the given positions
    (past n: the bytes spill into what follows the document)."""
    end = max([n] + [p + len(s) for p, s in at])
    d = bytearray([FILL]) * end
    for p, s in at:
        d[p:p + len(s)] = s
    return bytes(d[:n]), bytes(d[n:])


def corpus(lens_tail, quad_lanes):
    """-> (documents, kinds).  A document that must see a key just past its
    end is followed by a document that begins with those bytes."""
    docs, kinds = [], []

    def add(d, kind):
        docs.append(d)
        kinds.append(kind)

    # a 2-byte hit at one lane of all four sub-blocks, four languages
    for j in quad_lanes:
        d, _ = doc_with(256, [(64 * k + j, QUAD[k]) for k in range(4)])
        add(d, "quad")
        add(bytes([FILL]) * 256, "none")
    # the last window a key, and keys on the bytes just past the end: "ba" at
    # len - 2, then the next document starts "aa": "aa" straddles the end
    # (position len - 1) and sits at len
    for n in lens_tail:
        at = [(n - 2, b"ba")]
        if n > 200:
            at += [(192, b"ca"), (n - 5, b"za")]  # more of sub-block 3 ("za": 1- and 2-byte hit)
        d, _ = doc_with(n, at)
        add(d, "tail%d" % n)
        add(b"aa" + bytes([FILL]) * 40 + b"xyz" + bytes([FILL]) * 7, "after")
        add(bytes([FILL]) * (n - 1) + b"q", "none")   # no 2-byte hit; a 1-byte key as the last window
    # words 0 and 2047, and the same position a 1-byte and a 2-byte key
    d, _ = doc_with(256, [(3, b"\x00\x00"), (70, b"\xff\xff"), (130, b"za"), (200, b"\x60a"), (250, b"\x00a")])
    add(d, "edges")
    add(b"xyz" * 20, "none")
    return docs, kinds


SINGLE_TAILS = [193, 200, 255, 256, 3, 64, 65, 128, 129, 192]
PACK_TAILS = [3, 4, 17, 63, 64, 65, 100, 127, 128]


def random_docs(rng, n, lo, hi):
    alphabet = np.frombuffer(b"abcezq.\x00\x60\x7f\xffxy", dtype=np.uint8)
    return [bytes(rng.choice(alphabet, size=int(x))) for x in rng.integers(lo, hi, size=n)]


@pytest.fixture(scope="module")
def single():
    docs, kinds = corpus(SINGLE_TAILS, [0, 1, 31, 62])
    docs += random_docs(np.random.default_rng(7), 300, 0, 300)
    kinds += ["random"] * 300
    data, off = encoding.pack(docs)
    return docs, kinds, data, off


@pytest.fixture(scope="module")
def count_table():
    return table_of([math.log(2.0)])


@pytest.fixture(scope="module")
def single_oracle(single, count_table):
    _, _, data, off = single
    return OC.Table(count_table, L).score(GRAMS, data, off, want_scores=True, nthreads=8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_table_has_the_edge_keys():
    """Not a GPU property, but every case below leans on it."""
    words = [word_of(k) for k in KEYS2]
    shared = [k for k in KEYS2 if words.count(word_of(k)) >= 3]
    assert len(shared) >= 3                                           # ranks 1, 2, ... within one word
    w = word_of(b"aa")
    assert {k[0] & 31 for k in KEYS2 if word_of(k) == w} >= {0, 31}   # a word's bit 0 and bit 31
    assert word_of(b"\x00\x00") == 0 and word_of(b"\xff\xff") == 2047
    assert len({KEYS2[k] for k in QUAD}) == 4
    assert all(k[:1] not in KEYS1 or k == b"za" for k in KEYS2)


def test_corpus_properties(single):
    docs, kinds, data, off = single
    by = lambda kind: [i for i, k in enumerate(kinds) if k == kind]
    # a lane with a hit in all four sub-blocks, four languages
    for i in by("quad"):
        h = hits2(docs[i])
        lanes = {p % 64 for p in h}
        assert len(docs[i]) == 256 and len(h) == 4 and len(lanes) == 1, (i, h)
        assert sorted(p // 64 for p in h) == [0, 1, 2, 3]
        assert len({KEYS2[docs[i][p:p + 2]] for p in h}) == 4
    assert {hits2(docs[i])[0] % 64 for i in by("quad")} == {0, 1, 31, 62}
    assert 192 + 62 == 256 - 2                                        # lane 62: sub-block 3's hit is the last window
    # documents with no 2-byte hit, between the others
    none = by("none")
    assert len(none) >= 10 and all(not hits2(docs[i]) for i in none)
    assert all(kinds[i - 1] != "none" for i in none)
    # tails: the last window a key; keys on the bytes just past the end
    for n in SINGLE_TAILS:
        (i,) = by("tail%d" % n)
        d, b = docs[i], int(off[i])
        assert len(d) == n and hits2(d)[-1] == n - 2
        assert bytes(data[b + n - 1:b + n + 1]) in KEYS2 and bytes(data[b + n:b + n + 2]) in KEYS2
        # sub-block 3 alone -- but for 193 (and 192): a 193-byte document's
        # 2-byte windows end at position 191, so its last window, the hit, is
        # in sub-block 2 (its sub-block 3 holds only the 1-byte window 192)
        if n >= 195:
            assert all(p >= 192 for p in hits2(d)), (n, hits2(d))
    # a 1-byte and a 2-byte key at one position
    (e,) = by("edges")
    p = docs[e].index(b"za")
    assert docs[e][p:p + 1] in KEYS1 and docs[e][p:p + 2] in KEYS2
    assert {word_of(docs[e][p:p + 2]) for p in hits2(docs[e])} >= {0, 2047}


def test_single_documents(single, count_table, single_oracle):
    """Labels and scores of the product library, single documents of every
    sub-block count (1..4, the last one cut)."""
    _, _, data, off = single
    m = DeviceModel(count_table, L, GRAMS)
    info = m.info()
    assert info["mode"] == 2 and "direct" in info["layout"], info
    ol, os_ = single_oracle
    labels, scores = m.score(data, off, want_scores=True)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    assert np.array_equal(bits(scores), bits(os_))
    only, _ = m.score(data, off, want_scores=False)   # labels only: the count argmax
    assert np.array_equal(only, ol), np.nonzero(only != ol)[0][:10]
    assert len(np.unique(ol)) > 2


def test_without_direct_tables(single, count_table, single_oracle, monkeypatch):
    """The cross-check: the diagnostics library with LDGPU_NO_DIRECT verifies
    every 1-/2-byte candidate instead; then its direct path."""
    _, _, data, off = single
    ol, os_ = single_oracle
    for no_direct in (True, False):
        if no_direct:
            monkeypatch.setenv("LDGPU_NO_DIRECT", "1")
        else:
            monkeypatch.delenv("LDGPU_NO_DIRECT")
        m = DeviceModel(count_table, L, GRAMS, variant="diag")
        assert ("direct" in m.info()["layout"]) != no_direct, m.info()
        labels, scores = m.score(data, off, want_scores=True)
        assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
        assert np.array_equal(bits(scores), bits(os_))


def test_packs(count_table, monkeypatch):
    """The same cases as packs of short documents (3..128 bytes, labels only):
    one sub-block at a time, a hit counted into its own document's block.
    445 documents alone give every wave one document and no pack: the corpus
    is scored again on one workgroup (diagnostics library, LDGPU_SCORE_GRID)
    and, tiled, on the product grid, where the host model (tests/geometry.py)
    says which documents share a pack."""
    docs, kinds = [], []
    for j in (0, 1, 31, 61):
        # a pack of four 64-byte documents: lane j a hit in every sub-block
        for k in range(4):
            docs.append(doc_with(64, [(j, QUAD[k])])[0])
            kinds.append("quad")
    d2, k2 = corpus(PACK_TAILS, [])
    d2 = [d[:128] for d in d2]
    docs += d2 + random_docs(np.random.default_rng(11), 400, 3, 129)
    assert all(3 <= len(d) <= 128 for d in docs)
    assert sum(not hits2(d) for d in docs) >= 10
    for i in range(0, 16, 4):
        assert [hits2(d) for d in docs[i:i + 4]] == [[(0, 1, 31, 61)[i // 4]]] * 4
        assert len({KEYS2[d[hits2(d)[0]:][:2]] for d in docs[i:i + 4]}) == 4
    for n in PACK_TAILS:
        i = 16 + k2.index("tail%d" % n)
        assert hits2(docs[i])[-1] == n - 2 and docs[i + 1][:2] in KEYS2 and docs[i][-1:] + docs[i + 1][:1] in KEYS2
    data, off = encoding.pack(docs)
    m = DeviceModel(count_table, L, GRAMS)
    info = m.info()
    assert info["mode"] == 2 and "direct" in info["layout"] and "packs" in info["layout"], info
    ol, _ = OC.Table(count_table, L).score(GRAMS, data, off, want_scores=False, nthreads=8)
    labels, _ = m.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    assert len(np.unique(ol)) > 2
    # one workgroup: the sixteen quad documents are the first group of wave 0, each lane's four in one pack
    pf = geometry.survey(off, max(GRAMS), geometry.SCORE_WAVES).pack_first
    assert [pf[i:i + 4].tolist() for i in range(0, 16, 4)] == [[i] * 4 for i in range(0, 16, 4)]
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    diag = DeviceModel(count_table, L, GRAMS, variant="diag")
    assert "packs" in diag.info()["layout"], diag.info()
    labels, _ = diag.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    # the product grid on the tiled corpus: in some period every quad, and
    # every tail case with the document after it, is in one pack, at one,
    # two or three workgroups per CU
    to, times, cus = geometry.check_tiled_labels(m, data, off, ol, max(GRAMS))
    tails = [16 + k2.index("tail%d" % n) for n in PACK_TAILS]
    for w in (1, 2, 3):
        pf = geometry.survey(to, max(GRAMS), geometry.product_waves(len(to) - 1, cus, w)).pack_first
        pf = pf.reshape(times, len(docs))
        for i in range(0, 16, 4):
            assert ((pf[:, i:i + 4] == pf[:, i:i + 1]).all(axis=1) & (pf[:, i] >= 0)).any(), (w, i)
        for i in tails:
            assert ((pf[:, i] == pf[:, i + 1]) & (pf[:, i] >= 0)).any(), (w, i)


def test_class_mode(single, monkeypatch):
    """Two values: class mode, whose direct entries are language | class << 6
    (labels only)."""
    _, _, data, off = single
    table = table_of([math.log(2.0), math.log(1.5)])
    assert len({v for k in KEYS2 for v in table[k] if v}) == 2
    m = DeviceModel(table, L, GRAMS)
    lay = m.info()["layout"]
    assert "classes" in lay and "direct" in lay, lay
    ol, _ = OC.Table(table, L).score(GRAMS, data, off, want_scores=False, nthreads=8)
    labels, _ = m.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
    # the cross-check for class mode: the diagnostics library without direct tables
    monkeypatch.setenv("LDGPU_NO_DIRECT", "1")
    plain = DeviceModel(table, L, GRAMS, variant="diag")
    lay = plain.info()["layout"]
    assert "classes" in lay and "direct" not in lay, lay
    labels, _ = plain.score(data, off, want_scores=False)
    assert np.array_equal(labels, ol), np.nonzero(labels != ol)[0][:10]
