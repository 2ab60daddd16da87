"""GPU parity of count / class mode where a document's candidates of lengths
3..7 are queued by one wave scan (scan_append, ldgpu_score.hip): each lane
gathers its filter bits of every (length, sub-block) into one word, a DPP prefix
sum places them, and the lane stores its entries itself.  Hand-built tables and
documents put the candidates on the edges of that scan -- twenty in one lane,
none in its neighbour, totals of 0, 64, 65, 288 (the queue's capacity) and 289
(the per-length fallback), keys that straddle a document's end -- and every case
compares with the C oracle: labels exactly, fp64 scores bit for bit.

The totals are asserted on the host from the table and the text, with a
restatement of the prefix Bloom (ldgpu_common.h: pf_word, pf_bit) sized by the
model's own filter_bits.  Each corpus runs one document per wave (the product
grid on a few hundred documents), several per wave on one and two workgroups
(diagnostics library, LDGPU_SCORE_GRID) and tiled for the product grid."""
import math

import numpy as np
import pytest

import geometry
import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

L = 6
FILL = 0x2E          # '.': in no key
QUEUE_CAP = 288      # kQueueCap
BLOOM_WORDS = 64     # the smallest prefix Bloom: every table here (asserted against info())
EVERY = b"klmnopq"   # its prefixes of 3..7 bytes are keys: a position where a key of every length starts
RUN = ord("a")       # 'a' * N is a key for N = 3..7
RUN3 = ord("b")      # 'bbb' alone is a key

# key -> languages of its row
KEYS = {
    b"q": [3], b"z": [2], b"\x80": [1],
    b"ab": [3], b"za": [4], b"\x00\xff": [0], b"k.": [5],
    b"bbb": [1],
    b"xyz": [0], b"wxyz": [1, 4], b"vwxyz": [2], b"uvwxyz": [3], b"tuvwxyz": [0, 5],
    b"\x00\x80\xff": [4], b"\xff\xff\xff\xff": [5], b"\x80\x00\x00\x80\xff": [1, 2, 3],
    b"\xff\x00\x80\x80\x00\xff": [2], b"\x00\x00\x00\x00\x00\x00\x00": [3],
}
for _n in range(3, 8):
    KEYS[bytes([RUN]) * _n] = [_n % L]
    KEYS[EVERY[:_n]] = [(_n + 2) % L] if _n != 5 else [0, 1]


def table_of(values, lengths=range(1, 8), extra=()):
    """Rows of values[i % len(values)] at the key's languages, for the keys of
    the given lengths (and the `extra` (key, languages) pairs)."""
    t = {}
    items = [(k, v) for k, v in KEYS.items() if len(k) in lengths] + list(extra)
    for i, (k, langs) in enumerate(items):
        row = [0.0] * L
        for l in langs:
            row[l] = values[i % len(values)]
        t[k] = row
    return t


# ------------------------------------------------- the prefix Bloom, restated
def _mul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & 0xFFFFFFFF


def _mulhi24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) >> 32


def _pf_word(b3, words):
    return _mul24(int.from_bytes(b3, "little"), 0x9E3779) >> (32 - int(math.log2(words)))


def _pf_bit(n, w):
    sh = 8 * (n - 3 if n < 6 else 3)
    return _mulhi24(int.from_bytes(w[:n].ljust(8, b"\0"), "little") >> sh, (n * 0x6F4F2B + 0x7F4A7D) & 0xFFFFFF) & 31


def bloom_of(table, words=BLOOM_WORDS):
    b = [0] * words
    for k in table:
        if 3 <= len(k) <= 7:
            b[_pf_word(k[:3], words)] |= 1 << _pf_bit(len(k), k)
    return b


def fast_lengths(table, grams):
    """The distinct listed lengths of 3..7 bytes that have keys (fast_mask)."""
    return sorted({n for n in grams if 3 <= n <= 7 and any(len(k) == n for k in table)})


def candidates(bloom, lens, doc):
    """[(length, position)] of the document's windows that pass the filter."""
    out = []
    for n in lens:
        for p in range(len(doc) - n + 1):
            if (bloom[_pf_word(doc[p:p + 3], len(bloom))] >> _pf_bit(n, doc[p:p + n])) & 1:
                out.append((n, p))
    return out


# --------------------------------------------------------------------- corpus
ALPHABET = np.frombuffer(b"ab.klmnopqxyzwvut\x00\x80\xff", dtype=np.uint8)
LENGTHS = [5, 7, 63, 64, 65, 191 + 5, 192 + 5, 191 + 7, 192 + 7, 255, 256]
TOTALS = [0, 64, 65, QUEUE_CAP, QUEUE_CAP + 1]
LANES = [0, 1, 37, 57]


def total_doc(bloom, lens, target):
    """'a' * m + 'b' * r (+ filler) with exactly `target` candidates, by the model."""
    if target == 0:
        for c in range(0x21, 0x7F):
            d = bytes([c]) * 256
            if not candidates(bloom, lens, d):
                return d
    for r in range(0, 257):
        for m in range(0, 257 - r):
            d = bytes([RUN]) * m + bytes([RUN3]) * r
            if len(d) >= max(lens) and len(candidates(bloom, lens, d)) == target:
                return d
    raise AssertionError(("no document with that many candidates", target))


def soup(rng, n):
    """n bytes of keys (3 bytes and more) with a few other bytes between them."""
    keys = [k for k in KEYS if len(k) >= 3]
    d = b""
    while len(d) < n:
        d += keys[int(rng.integers(len(keys)))] * int(rng.integers(1, 3)) + bytes(rng.choice(ALPHABET, size=int(rng.integers(0, 3))))
    return d[:n]


def build_corpus(table, grams):
    bloom = bloom_of(table)
    lens = fast_lengths(table, grams)
    rng = np.random.default_rng(31)
    docs, kinds = [], []

    def add(d, kind):
        docs.append(bytes(d))
        kinds.append(kind)

    for t in TOTALS:
        add(total_doc(bloom, lens, t), "total%d" % t)
        add(bytes(rng.choice(ALPHABET, size=90)), "random")
    # twenty entries from one lane: a key of every length at j, j + 64, j + 128, j + 192
    for j in LANES:
        d = bytearray([FILL]) * 256
        for k in range(4):
            d[64 * k + j:64 * k + j + 7] = EVERY
        add(d, "lane%d" % j)
        add(bytes([FILL]) * 256, "filler")
    # every switch of the length: 'a' * 7 ends the document (its last window of
    # every length a key), and the next document goes on with 'a's
    for n in LENGTHS:
        d = bytearray(rng.choice(ALPHABET, size=n).tobytes())
        d[max(0, n - 7):] = bytes([RUN]) * min(n, 7)
        add(d, "len%d" % n)
        add(bytes([RUN]) * 6 + bytes(rng.choice(ALPHABET, size=30)), "after")
    # a key of length N on the last N - 1 bytes of a document, its last byte the next document's first
    for n in (256, 200, 70):
        for key in (b"xyz", b"wxyz", b"vwxyz", b"uvwxyz", b"tuvwxyz", b"\x00\x80\xff", b"\xff\xff\xff\xff"):
            add(bytes([FILL]) * (n - len(key) + 1) + key[:-1], "poison%d" % len(key))
            add(key[-1:] + bytes([FILL]) * 40, "after")
    for n in rng.integers(0, 300, size=80):
        add(bytes(rng.choice(ALPHABET, size=int(n))), "random")
    for n in rng.integers(0, 300, size=120):
        add(soup(rng, int(n)), "soup")
    data, off = encoding.pack(docs)
    return docs, kinds, data, off


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Case:
    """A table, a gram list and the corpus built for them, with its oracle."""

    def __init__(self, table, grams, n_values=1):
        self.table, self.grams, self.n_values = table, list(grams), n_values
        self.docs, self.kinds, self.data, self.off = build_corpus(table, grams)
        self.labels, self.scores = OC.Table(table, L).score(self.grams, self.data, self.off, want_scores=True,
                                                            nthreads=8)
        self.bloom = bloom_of(table)
        self.lens = fast_lengths(table, grams)

    def by(self, kind):
        return [i for i, k in enumerate(self.kinds) if k == kind]

    def check(self, m, want_scores):
        labels, scores = m.score(self.data, self.off, want_scores=want_scores)
        bad = np.nonzero(labels != self.labels)[0]
        assert not len(bad), [(int(i), self.kinds[i]) for i in bad[:10]]
        if want_scores:
            bad = np.nonzero((bits(scores) != bits(self.scores)).any(axis=1))[0]
            assert not len(bad), [(int(i), self.kinds[i]) for i in bad[:10]]

    def run_all_grids(self, monkeypatch, has=("direct",), hasnt=("wide_keys",)):
        scores = self.n_values == 1   # class mode: labels only
        m = DeviceModel(self.table, L, self.grams)
        info = m.info()
        assert info["filter_bits"] == 32 * BLOOM_WORDS, info
        assert set(has) <= set(info["layout"]) and not set(hasnt) & set(info["layout"]), info
        assert ("classes" in info["layout"]) == (self.n_values > 1), info
        # one document per wave
        self.check(m, False)
        if scores:
            self.check(m, True)
        # the product grid, 16 and more documents per wave
        td, to, times, _ = geometry.tile_for_product(self.data, self.off)
        labels, sc = m.score(td, to, want_scores=scores)
        bad = np.nonzero(labels.reshape(times, -1) != self.labels.reshape(1, -1))
        assert not len(bad[0]), ("period, document", bad[0][:10].tolist(), bad[1][:10].tolist())
        if scores:
            assert np.array_equal(bits(sc).reshape(times, -1), np.tile(bits(self.scores).reshape(1, -1), (times, 1)))
        m.close()
        # one and two workgroups: 12 and 24 waves over the corpus
        for grid in ("1", "2"):
            monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
            d = DeviceModel(self.table, L, self.grams, variant="diag")
            assert set(has) <= set(d.info()["layout"]), d.info()
            self.check(d, False)
            if scores:
                self.check(d, True)
            d.close()


@pytest.fixture(scope="module")
def main():
    return Case(table_of([math.log(2.0)]), [3, 4, 5])


def test_corpus_has_the_edge_cases(main):
    """Host-side: what the GPU cases lean on, from the table and the text."""
    c = main
    assert c.lens == [3, 4, 5]
    cand = [candidates(c.bloom, c.lens, d) if max(c.lens) <= len(d) <= 256 else None for d in c.docs]
    # the totals: none, the verify's first batch full, its second batch of one, the queue full, one more
    for t in TOTALS:
        (i,) = c.by("total%d" % t)
        assert max(c.lens) <= len(c.docs[i]) <= 256 and len(cand[i]) == t, (t, len(cand[i]))
    # a repeated-byte document, every window a key, has 3 len - 9 candidates whatever else the Bloom holds
    (i,) = c.by("total%d" % QUEUE_CAP)
    assert c.docs[i] == bytes([RUN]) * 99 and all(bytes([RUN]) * n in c.table for n in c.lens)
    # twenty entries from one lane would need grams 3..7 (test_all_lengths); here twelve, and a lane with none
    for j in LANES:
        (i,) = c.by("lane%d" % j)
        per_lane = np.bincount([p % 64 for _, p in cand[i]], minlength=64)
        assert per_lane[j] == 4 * len(c.lens)
        assert per_lane[(j + 1) % 64] == 0 or per_lane[(j - 1) % 64] == 0, per_lane
        assert {p // 64 for _, p in cand[i] if p % 64 == j} == {0, 1, 2, 3}
    # poison: the key is in the table, starts inside the document and ends past it
    for i in [i for i, k in enumerate(c.kinds) if k.startswith("poison")]:
        n = int(c.kinds[i][6:])
        b = int(c.off[i + 1]) - (n - 1)
        assert bytes(c.data[b:b + n]) in KEYS and b + n == int(c.off[i + 1]) + 1
    # the lengths: the last window of every length a key, and keys on the bytes past the end
    for n in LENGTHS:
        (i,) = c.by("len%d" % n)
        e = int(c.off[i + 1])
        assert len(c.docs[i]) == n and all(bytes(c.data[e - g:e]) in c.table for g in c.lens)
        assert all(bytes(c.data[e - g + 1:e + 1]) in c.table for g in c.lens)
    assert len(np.unique(c.labels)) >= 5
    assert {0x00, 0x80, 0xFF} <= {b for k in c.table for b in k} and {0x00, 0x80, 0xFF} <= set(ALPHABET.tolist())


def test_count_mode_345(main, monkeypatch):
    main.run_all_grids(monkeypatch)


@pytest.mark.parametrize("grams", [[3, 5], [1, 2, 3, 4, 5, 6, 7], [3, 3, 5]], ids=str)
def test_gram_lists(grams, monkeypatch):
    """[3, 5]: the table's 4-byte keys are not listed.  1..7: twenty entries
    from one lane.  [3, 3, 5]: a repeated length counts twice (mult)."""
    c = Case(table_of([math.log(2.0)]), grams)
    assert c.lens == sorted({g for g in grams if g >= 3})
    for t in TOTALS:
        (i,) = c.by("total%d" % t)
        assert len(candidates(c.bloom, c.lens, c.docs[i])) == t
    if len(c.lens) == 5:
        for j in LANES:
            (i,) = c.by("lane%d" % j)
            per_lane = np.bincount([p % 64 for _, p in candidates(c.bloom, c.lens, c.docs[i])], minlength=64)
            assert per_lane[j] == 20 and (per_lane[(j + 1) % 64] == 0 or per_lane[(j - 1) % 64] == 0), per_lane
    if grams == [3, 3, 5]:
        # the repeated length shows in the scores: twice the hits of [3, 5]
        once = OC.Table(c.table, L).score([3, 5], c.data, c.off, want_scores=True, nthreads=8)[1]
        assert not np.array_equal(once, c.scores)
    c.run_all_grids(monkeypatch)


def test_listed_length_without_keys(monkeypatch):
    """No 4-byte key in the table: the length's fast_mask bit is clear."""
    c = Case(table_of([math.log(2.0)], lengths=(1, 2, 3, 5)), [3, 4, 5])
    assert c.lens == [3, 5]
    c.run_all_grids(monkeypatch)


def test_class_mode(monkeypatch):
    """Two values: class mode (labels only; a near-tie document is replayed exactly)."""
    c = Case(table_of([math.log(2.0), math.log(1.5)]), [3, 4, 5, 6, 7], n_values=2)
    assert len({v for r in c.table.values() for v in r if v}) == 2
    c.run_all_grids(monkeypatch)


def test_fallback_forms(monkeypatch):
    """Tables the scan does not serve keep the per-length path: a wide key (8
    bytes), and 1-/2-byte keys of two languages (no direct tables)."""
    wide = Case(table_of([math.log(2.0)], extra=[(b"klmnopqr", [2]), (b"aaaaaaaa", [4])]), [3, 4, 5, 8])
    wide.run_all_grids(monkeypatch, has=("direct", "wide_keys"), hasnt=())
    plain = Case(table_of([math.log(2.0)], extra=[(b"yz", [1, 3])]), [1, 2, 3, 4, 5])
    plain.run_all_grids(monkeypatch, has=(), hasnt=("direct", "wide_keys"))
