"""GPU parity of count mode on the exact LDS trie (LDGPU_LAYOUT_TRIE;
csrc/ldgpu_trie.h, csrc/ldgpu_trie.hip): a table whose keys all have at most 4
bytes and one language each is walked from LDS, lane i owning window positions
4 i .. 4 i + 3, by labels-only calls on documents that are not packed (mean
length >= 192).  Documents shorter than max(grams), longer than 256 bytes or in
unstaged groups are left to an indirect launch of the LDS-Bloom kernel.

Labels must equal the C oracle's exactly, on the product library (one document
per wave, and tiled for 16 and more per wave) and on the diagnostics library
with several documents per wave (LDGPU_SCORE_GRID = 1, 2); the same corpora run
with LDGPU_NO_TRIE=1 keep the LDS-Bloom path of these tables covered.

  placement  a key of each length 1..4 at every slot k of lanes 0, 1, 31, 32,
             62, 63; a prefix chain with a language per depth; a 4-byte key
             whose 3-byte prefix is no key; two keys that differ in the last
             byte; bytes 0x00 and 0xff
  geometry   lengths max(grams) - 1 .. + 1, 253..257, 264, above 1,024; a key of
             every length on the document's last bytes, and one byte past its
             end (the next document's first bytes); a group's first document at
             every residue modulo 16; groups of 1 to 8 documents
  leftovers  calls with none, one, many and only leftovers
  grams      [1] .. [4], [2, 4], [1, 2, 3, 4], a repeated length, a listed
             length without a key (5, and 3 on a table without 3-byte keys)
  ties       the first maximum; a document without a hit gets label 0
  ineligible a 5-byte key, a two-language row, a table too large for the LDS
  languages  70, 134, 200 and 254 languages (2, 3, 4 counter slices), the
             winners at or above 64, 128 and 192
  scores     the same model asked for scores or top-k gives unchanged results
             (device-pointer, UTF-8 and chunked calls, and a negative table
             value: test_gpu_trie_calls.py)

Hand mutations of ldgpu_trie.hip, each built once and not committed (the check
compare dropped; the tail condition dropped for depth 4): see DESIGN.md for the
cases that fail."""
import functools
import math

import numpy as np
import pytest

import geometry
import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

L = 8
V = math.log(2.0)
FILL = ord(".")
RUN = ord("r")  # "r" * N is a key for N = 1..4
KEYS = {
    b"q": 3, b"\x00": 1, b"\xff": 2,
    b"ab": 3, b"\x00\xff": 0, b"qa": 4,
    b"xyz": 0, b"qab": 5, b"\xff\xff\xff": 4,
    b"wxyz": 1, b"qabc": 6, b"mnop": 2, b"mnoq": 7, b"\x00\x00\x00\x00": 5, b"\xff\x00\xff\x00": 6,
}
for _n in range(1, 5):
    KEYS[bytes([RUN]) * _n] = _n % L
KEY_OF = {1: b"q", 2: b"ab", 3: b"xyz", 4: b"wxyz"}
ALPHABET = np.frombuffer(b"ab.qxyzwmnopc\x00\xff", dtype=np.uint8)
SLOT_LANES = (0, 1, 31, 32, 62, 63)
END_LENGTHS = (256, 201, 70, 67)
GROUP_SECTIONS = [[1000], [500, 500], [340] * 3, [250] * 4, [200] * 5, [168] * 6, [144] * 7, [126] * 8]
GRAM_LISTS = [[1], [2], [3], [4], [2, 4], [1, 2, 3, 4], [1, 2, 3, 4, 4, 4], [1, 2, 3, 4, 5]]


def table_of(keys=KEYS, lengths=(1, 2, 3, 4)):
    t = {}
    for k, l in keys.items():
        if len(k) in lengths:
            row = [0.0] * L
            row[l] = V
            t[k] = row
    return t


def soup(rng, n):
    keys = list(KEYS)
    d = b""
    while len(d) < n:
        d += keys[int(rng.integers(len(keys)))] + bytes(rng.choice(ALPHABET, size=int(rng.integers(0, 4))))
    return d[:n]


@functools.lru_cache(maxsize=None)
def corpus(maxg):
    rng = np.random.default_rng(1400 + maxg)
    docs, kinds = [], []

    def add(d, kind):
        docs.append(bytes(d))
        kinds.append(kind)

    # base: documents of varying lengths, so that a group's first document starts at every residue modulo 16
    for i in range(48):
        n = 193 + (5 * i) % 23
        d = bytearray(rng.choice(ALPHABET, size=n).tobytes())
        k = KEY_OF[1 + i % 4]
        d[i % 4:i % 4 + len(k)] = k
        add(d, "base")
    # slots: the key of length N at slot k of SLOT_LANES (cut by the document's end at lane 63)
    for n, key in KEY_OF.items():
        for k in range(4):
            d = bytearray([FILL]) * 260
            for j in SLOT_LANES:
                d[4 * j + k:4 * j + k + n] = key
            add(d[:256], "slot%d.%d" % (n, k))
            add(bytes(rng.choice(ALPHABET, size=200 + 4 * n + k)), "after")
    # chains, a missing prefix, a last byte that differs, 0x00 / 0xff
    for i, piece in enumerate((b"qabc", b"qab.", b"qa.c", b"q.bc", b"mnop", b"mnoq", b"mnox", b"mno", b"\x00\x00\x00\x00\x00",
                               b"\xff\xff\xff\xff", b"\xff\x00\xff\x00\xff", b"\x00\xff\x00\xff")):
        d = bytearray([FILL]) * 256
        for at in (i, 61 + i, 126 + i, 250 - i):
            d[at:at + len(piece)] = piece
        add(d[:256], "piece")
    # ties (first maximum) and a document without a hit
    add(b"." * 100 + b"mnoq" + b"." * 100 + b"mnop" + b"." * 48, "tie")
    add(b"." * 96 + b"wxyz" + b"." * 156, "tie")
    add(b"." * 256, "empty")
    add(b"." * 193, "empty")
    # lengths: the last window of every length a key ("r" * N); the next document goes on with the same byte
    for n in [maxg - 1, maxg, maxg + 1, 253, 254, 255, 256, 257, 264, 1025, 1100, 1500, 5000]:
        d = bytearray(rng.choice(ALPHABET, size=n).tobytes())
        d[max(0, n - 4):] = bytes([RUN]) * min(n, 4)
        add(d, "len%d" % n)
        add(bytes([RUN]) * 3 + soup(rng, 220), "after")
    # end: the key on the document's last bytes; the key one byte later, completed by the next document
    for m in END_LENGTHS:
        for n, key in KEY_OF.items():
            add(bytes([FILL]) * (m - n) + key, "end%d" % n)
            add(bytes([FILL]) * 230, "after")
            add(bytes([FILL]) * (m - n + 1) + key[:-1], "poison%d" % n)
            add(key[-1:] + bytes([FILL]) * 230, "after")
    # groups of 1 to 8 documents
    for rep in range(3):
        for sec in GROUP_SECTIONS:
            add(soup(rng, 1030 + rep), "long")
            for n in sec:
                add(soup(rng, n), "group")
    # short documents (partial windows) and empty ones among fast ones
    for n in (0, 1, 2, 3, 4, 0, 2):
        add(soup(rng, n), "short")
        add(soup(rng, 256), "soup")
    for n in rng.integers(190, 300, size=80):
        add(soup(rng, int(n)), "soup")
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0  # the launch does not pack
    return docs, kinds, data, off


@functools.lru_cache(maxsize=None)
def oracle(grams, lengths=(1, 2, 3, 4)):
    docs, kinds, data, off = corpus(max(grams))
    return OC.Table(table_of(lengths=lengths), L).score(list(grams), data, off, want_scores=True, nthreads=8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_labels(m, data, off, labels, kinds=None):
    got, _ = m.score(data, off, want_scores=False)
    bad = np.nonzero(got != labels)[0]
    assert not len(bad), [(int(i), kinds[i] if kinds else None, int(got[i]), int(labels[i])) for i in bad[:10]]


def test_corpus_has_the_edge_cases():
    """Host-side: what the GPU cases lean on, from the table and the text."""
    grams = (1, 2, 3, 4)
    docs, kinds, data, off = corpus(4)
    labels, scores = oracle(grams)
    o = [int(x) for x in off]
    fast = {i for i, d in enumerate(docs) if 4 <= len(d) <= 256}
    assert {o[i] % 16 for i in fast if kinds[i] == "base"} == set(range(16))
    for nw in (geometry.SCORE_WAVES, 2 * geometry.SCORE_WAVES):
        sizes, first_res, left = set(), set(), 0
        for lo, hi in geometry.wave_ranges(len(docs), nw):
            for g0, cnt, staged in geometry.groups(o, lo, hi):
                sizes.add(cnt)
                if staged and g0 in fast:
                    first_res.add(o[g0] % 16)
                left += sum(1 for i in range(g0, g0 + cnt) if not staged or i not in fast)
        assert sizes >= set(range(1, 9)), (nw, sizes)
        assert first_res == set(range(16)), (nw, first_res)
        assert 20 <= left < len(docs) // 2
    # every slot, and keys that matter: an end key and its poison twin score differently
    assert {o[i] % 4 for i, k in enumerate(kinds) if k.startswith("slot")} == {0, 1, 2, 3}
    for i, k in enumerate(kinds):
        if k.startswith("end"):
            n = int(k[3:])
            assert bytes(data[o[i + 1] - n:o[i + 1]]) == KEY_OF[n] and scores[i].any()
        if k.startswith("poison"):
            n = int(k[6:])
            b = o[i + 1] - (n - 1)
            assert bytes(data[b:b + n]) == KEY_OF[n] and not scores[i].any()
    assert {o[i + 1] % 4 for i, k in enumerate(kinds) if k.startswith("poison")} == {0, 1, 2, 3}
    # ties take the first maximum; no hit: label 0
    for i, k in enumerate(kinds):
        if k == "tie":
            top = np.nonzero(scores[i] == scores[i].max())[0]
            assert len(top) >= 2 and labels[i] == top[0] and scores[i].max() > 0
        if k == "empty":
            assert not scores[i].any() and labels[i] == 0
    assert len(np.unique(labels)) >= 4


@pytest.mark.parametrize("grams", GRAM_LISTS, ids=str)
def test_labels_match_the_oracle(grams, monkeypatch):
    docs, kinds, data, off = corpus(max(grams))
    labels, scores = oracle(tuple(grams))
    table = table_of()
    m = DeviceModel(table, L, grams)
    assert "trie" in m.info()["layout"], m.info()
    check_labels(m, data, off, labels, kinds)          # one document per wave
    if grams == [1, 2, 3, 4]:
        # the product grid, 16 and more documents per wave
        td, to, times, _ = geometry.tile_for_product(data, off)
        got, _ = m.score(td, to, want_scores=False)
        bad = np.nonzero(got.reshape(times, -1) != labels.reshape(1, -1))
        assert not len(bad[0]), ("period, document", bad[0][:10].tolist(), bad[1][:10].tolist())
    # scores and top-k requested: the LDS-Bloom kernel, unchanged results
    _, sc = m.score(data, off, want_scores=True)
    assert np.array_equal(bits(sc), bits(scores))
    tl, ts = m.score_topk(data, off, 3)
    m.close()
    for grid in ("1", "2"):
        monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
        d = DeviceModel(table, L, grams, variant="diag")
        assert "trie" in d.info()["layout"], d.info()
        check_labels(d, data, off, labels, kinds)
        d.close()
    # the same corpus on the LDS-Bloom path
    monkeypatch.setenv("LDGPU_NO_TRIE", "1")
    d = DeviceModel(table, L, grams, variant="diag")
    assert "trie" not in d.info()["layout"] and "direct" in d.info()["layout"], d.info()
    check_labels(d, data, off, labels, kinds)
    tl0, ts0 = d.score_topk(data, off, 3)
    d.close()
    assert np.array_equal(tl, tl0) and np.array_equal(bits(ts), bits(ts0))


@pytest.mark.parametrize("nl", [70, 134, 200, 254])
def test_many_languages(nl, monkeypatch):
    """Two, three and four slices of language counters (64 each), the labels one
    byte each in LDS up to language 253: KEYS' language l becomes nl - 1 - l, so
    the winners lie in the last slice, at or above 64, 128 and 192."""
    grams = [1, 2, 3, 4]
    docs, kinds, data, off = corpus(4)
    table = {}
    for k, l in KEYS.items():
        row = [0.0] * nl
        row[nl - 1 - l] = V
        table[k] = row
    labels, _ = OC.Table(table, nl).score(grams, data, off, want_scores=False, nthreads=8)
    top = 64 * ((nl - 1) // 64)   # the last slice's first language: 64, 128, 192
    assert (labels >= top).sum() >= 200 and len(np.unique(labels[labels >= top])) >= 4 and labels.max() == nl - 1
    m = DeviceModel(table, nl, grams)
    assert "trie" in m.info()["layout"], m.info()
    check_labels(m, data, off, labels, kinds)
    m.close()
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    d = DeviceModel(table, nl, grams, variant="diag")
    check_labels(d, data, off, labels, kinds)
    d.close()


def test_listed_length_without_a_key(monkeypatch):
    """3 is listed, no key has 3 bytes: only the 2-byte terminals count."""
    grams = (2, 3)
    docs, kinds, data, off = corpus(3)
    labels, _ = oracle(grams, lengths=(1, 2, 4))
    table = table_of(lengths=(1, 2, 4))
    m = DeviceModel(table, L, list(grams))
    assert "trie" in m.info()["layout"], m.info()
    check_labels(m, data, off, labels, kinds)
    m.close()
    monkeypatch.setenv("LDGPU_SCORE_GRID", "2")
    d = DeviceModel(table, L, list(grams), variant="diag")
    check_labels(d, data, off, labels, kinds)
    d.close()


@pytest.mark.parametrize("name", ["none", "one", "many", "only"])
def test_leftovers(name, monkeypatch):
    """Calls with 0, 1 and many documents left to the indirect launch, and with nothing else."""
    rng = np.random.default_rng(77)
    lens = {"none": [256] * 40,
            "one": [256] * 19 + [300] + [256] * 20,
            "many": [256, 300, 3, 257, 250, 0, 1500, 200] * 6,
            "only": [300] * 30 + [2000] * 5 + [257] * 5}[name]
    docs = [soup(rng, n) for n in lens]
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0
    grams = [1, 2, 3, 4]
    table = table_of()
    labels, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) >= 3
    m = DeviceModel(table, L, grams)
    assert "trie" in m.info()["layout"]
    check_labels(m, data, off, labels)
    m.close()
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    d = DeviceModel(table, L, grams, variant="diag")
    check_labels(d, data, off, labels)
    d.close()


def _ineligible(name):
    if name == "5-byte key":
        t = table_of()
        t[b"wxyz."] = [V if l == 2 else 0.0 for l in range(L)]
        return t
    if name == "two languages":
        t = table_of()
        t[b"xyz"] = [V if l in (0, 5) else 0.0 for l in range(L)]
        return t
    rng = np.random.default_rng(5)   # too large: 14,000 random 4-byte keys over every byte
    t = table_of()
    for k in rng.integers(0, 256, size=(14000, 4), dtype=np.uint8):
        row = [0.0] * L
        row[int(k[0]) % L] = V
        t.setdefault(bytes(k), row)
    return t


@pytest.mark.parametrize("name", ["5-byte key", "two languages", "too large"])
def test_ineligible_tables_keep_the_old_path(name):
    grams = [1, 2, 3, 4, 5]
    docs, kinds, data, off = corpus(5)
    table = _ineligible(name)
    labels, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    m = DeviceModel(table, L, grams)
    assert "trie" not in m.info()["layout"], m.info()
    check_labels(m, data, off, labels, kinds)
    m.close()


def test_random_keys_on_random_text(monkeypatch):
    """3,000 random keys over a-z, 20 languages, on random a-z text."""
    rng = np.random.default_rng(3000)
    nl = 20
    table = {}
    while len(table) < 3000:
        # (mostly 3 and 4 bytes, none of 1: a key of one letter hits a document of random letters ten times)
        k = bytes(rng.integers(97, 123, size=int(rng.choice([2, 3, 4], p=[0.01, 0.29, 0.7])), dtype=np.uint8))
        row = [0.0] * nl
        row[int(rng.integers(nl))] = V
        table.setdefault(k, row)
    docs = [bytes(rng.integers(97, 123, size=int(n), dtype=np.uint8))
            for n in list(rng.integers(200, 257, size=300)) + [3, 0, 257, 1200, 256, 256]]
    data, off = encoding.pack(docs)
    grams = [1, 2, 3, 4]
    labels, _ = OC.Table(table, nl).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) >= 10
    m = DeviceModel(table, nl, grams)
    assert "trie" in m.info()["layout"], m.info()
    check_labels(m, data, off, labels)
    m.close()
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    d = DeviceModel(table, nl, grams, variant="diag")
    check_labels(d, data, off, labels)
    d.close()
    monkeypatch.setenv("LDGPU_NO_TRIE", "1")
    d = DeviceModel(table, nl, grams, variant="diag")
    assert "trie" not in d.info()["layout"]
    check_labels(d, data, off, labels)
    d.close()
