"""GPU parity of count / class mode on the run-format queue entries of the
lane-run path (ldgpu_score.hip: entry_pos / entry_len, run_store,
direct_count_runs, the staged loop's 32-bit geometry).  A lane-run candidate is
queued as (4 lane + k) << 3 | (N - 3) by an unrolled store loop, and the narrow
verify, the full-slot verify and the flush of the candidates past the first 64
decode that format; a document without a 1-byte key byte leaves the 1-byte direct
counts in one branch; a staged document's base and length come from the low
halves of its offsets.  Hand-built tables and documents put keys where each of
these can go wrong:

  entry map   a key of every length 3..7 at every slot k = 0..3 of lanes 0, 1, 31,
              32, 62 and 63 (the key's language is its length less 2, the filler
              is in no key: a wrong position or length loses the only hit);
  store loop  one lane holding exactly c candidates, c on both sides of the
              unroll (4), 12 and 20, every other lane empty; then lane 0 with c
              and the last lanes with what a 256-byte document leaves them
              (lane 63 owns positions 252..255: three windows at the most, so
              "c in lane 63" is min(c, 3), and lane 62 min(c, 17));
  tail        documents with exactly 64, 65, 128, 129 and 288 candidates (the
              flush from 64 reads the run format) and 289 (the per-length
              fallback, old layout), each between ordinary documents of one
              staged group;
  1-byte skip one staged group holding a document with no 1-byte key byte, one
              whose only hit is its last byte (lengths 256, 201, 70, 67: the
              hit falls on every slot k, at 256 in lane 63), one whose only key
              byte is the next document's first; a second group holds the same
              with 2-byte hits (the two do not fit one 1,024-byte group);
  geometry    staged groups whose first document starts at every residue
              modulo 16 and that hold 1 to 8 documents, lengths maxg - 1, maxg,
              256 and 257 among them.

Candidate counts are asserted on the host from the table and the text with the
prefix Bloom restated in test_gpu_scan_append.py, the groups with the model of
geometry.py.  Every case compares with the C oracle -- labels exactly, fp64
scores bit for bit in count mode -- on the product library (one document per
wave) and on the diagnostics library's grids of one and two workgroups
(several documents per wave)."""
import math

import numpy as np
import pytest

import geometry
import ldoracle_c as OC
import test_gpu_scan_append as SA
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

L = 6
V = math.log(2.0)
FILL = bytes([SA.FILL])
QUEUE_CAP = SA.QUEUE_CAP
UNROLL = 4                                   # kRunStoreUnroll
ENTRY = {3: b"xyz", 4: b"wvut", 5: b"srpon", 6: b"mlkjih", 7: b"gfedcZY"}    # language N - 2; no key inside another
SHORT = {b"q": [3], b"ab": [5]}              # direct tables: one language each
T = b"ABCDEFGHIJ"                            # T[p:p + N], p = 0..3, N = 3..7: twenty keys of one lane
ENTRY_LANES = ((0, 31, 62), (1, 32, 63))     # neighbours apart: a 7-byte key runs into the next lane's bytes

KEYS_FULL = dict(SHORT)
for _n, _k in ENTRY.items():
    KEYS_FULL[_k] = [_n - 2]
for _p in range(4):
    for _n in range(3, 8):
        KEYS_FULL[T[_p:_p + _n]] = [(_p + _n) % L]
for _n in range(3, 8):
    KEYS_FULL[b"a" * _n] = [_n % L]
KEYS_FULL[b"bbb"] = [1]
# every key of 3 bytes and more has at most 4 and one language: the narrow slot table
KEYS_NARROW = {k: v for k, v in KEYS_FULL.items() if len(k) <= 4}
# ... and one two-language 3-byte key puts the same keys back on the full slots
KEYS_TWO = {**KEYS_NARROW, b"fbc": [1, 4]}
ALPHABET = np.frombuffer(b"ab.xyzwq.ABCDEF.\x00\x80\xff", dtype=np.uint8)


def table_of(keys, values=(V,)):
    t = {}
    for i, (k, langs) in enumerate(sorted(keys.items())):
        row = [0.0] * L
        for l in langs:
            row[l] = values[i % len(values)]
        t[k] = row
    return t


def soup(rng, n, keys):
    ks = sorted(keys)
    d = b""
    while len(d) < n:
        d += ks[int(rng.integers(len(ks)))] + bytes(rng.choice(ALPHABET, size=int(rng.integers(0, 4))))
    return d[:n]


class Case:
    """A table, a gram list and documents, with the oracle's labels and scores
    (computed once; the runs below only read them)."""

    def __init__(self, keys, grams, docs, kinds, values=(V,)):
        self.keys, self.table, self.grams = keys, table_of(keys, values), list(grams)
        self.docs, self.kinds, self.count_mode = docs, kinds, len(values) == 1
        self.data, self.off = encoding.pack(docs)
        self.labels, self.scores = OC.Table(self.table, L).score(self.grams, self.data, self.off, want_scores=True,
                                                                 nthreads=8)
        self.bloom = SA.bloom_of(self.table)
        self.lens = SA.fast_lengths(self.table, self.grams)
        for a in (self.labels, self.scores):
            a.setflags(write=False)

    def by(self, kind):
        return [i for i, k in enumerate(self.kinds) if k == kind]

    def candidates(self, i):
        return SA.candidates(self.bloom, self.lens, self.docs[i])

    def check(self, m, want_scores):
        labels, scores = m.score(self.data, self.off, want_scores=want_scores)
        bad = np.nonzero(labels != self.labels)[0]
        assert not len(bad), [(int(i), self.kinds[i], int(labels[i]), int(self.labels[i])) for i in bad[:10]]
        if want_scores:
            bad = np.nonzero((SA.bits(scores) != SA.bits(self.scores)).any(axis=1))[0]
            assert not len(bad), [(int(i), self.kinds[i], scores[i].tolist(), self.scores[i].tolist()) for i in bad[:4]]

    def run(self, monkeypatch, narrow):
        def one(m):
            info = m.info()
            assert info["filter_bits"] == 32 * SA.BLOOM_WORDS, info
            assert ("narrow_slots" in info["layout"]) == narrow, info
            assert {"direct", "lds_bloom"} <= set(info["layout"]) and "wide_keys" not in info["layout"], info
            assert ("classes" in info["layout"]) == (not self.count_mode), info
            self.check(m, False)
            if self.count_mode:
                self.check(m, True)
            m.close()

        one(DeviceModel(self.table, L, self.grams))             # one document per wave
        for grid in ("1", "2"):                                 # 12 and 24 waves over the corpus
            monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
            one(DeviceModel(self.table, L, self.grams, variant="diag"))


def staged_groups(off, n_waves):
    """[(first, count)] of the staged groups of a launch of n_waves waves."""
    off = [int(x) for x in off]
    out = []
    for lo, hi in geometry.wave_ranges(len(off) - 1, n_waves):
        out += [(g0, cnt) for g0, cnt, staged in geometry.groups(off, lo, hi) if staged]
    return out


# ------------------------------------------------------------------ entry map
def entry_docs():
    rng = np.random.default_rng(61)
    docs, kinds = [], []
    for n, key in ENTRY.items():
        for k in range(4):
            for lanes in ENTRY_LANES:
                d = bytearray(FILL * 256)
                for j in lanes:
                    d[4 * j + k:4 * j + k + n] = key
                docs.append(bytes(d[:256]))
                kinds.append("slot%d.%d.%d" % (n, k, lanes[0]))
                docs.append(soup(rng, int(rng.integers(8, 60)), KEYS_FULL))
                kinds.append("ordinary")
    return docs, kinds


ENTRY_CASES = [
    ("full-345", KEYS_FULL, [3, 4, 5], False, (V,)),
    ("full-7", KEYS_FULL, [7], False, (V,)),
    ("full-1234567", KEYS_FULL, [1, 2, 3, 4, 5, 6, 7], False, (V,)),
    ("narrow-334", KEYS_NARROW, [3, 3, 4], True, (V,)),
    ("two-languages-334", KEYS_TWO, [3, 3, 4], False, (V,)),
    ("class-full-1234567", KEYS_FULL, [1, 2, 3, 4, 5, 6, 7], False, (V, math.log(1.5))),
    ("class-narrow-334", KEYS_NARROW, [3, 3, 4], True, (V, math.log(1.5))),
    ("class-two-languages-334", KEYS_TWO, [3, 3, 4], False, (V, math.log(1.5))),
]


@pytest.mark.parametrize("name,keys,grams,narrow,values", ENTRY_CASES, ids=[c[0] for c in ENTRY_CASES])
def test_entry_map(name, keys, grams, narrow, values, monkeypatch):
    docs, kinds = entry_docs()
    c = Case(keys, grams, docs, kinds, values)
    # host side: the key is the document's only hit, so its language is the label wherever the key counts
    for i, kind in enumerate(c.kinds):
        if kind.startswith("slot"):
            n, k, lane0 = (int(x) for x in kind[4:].split("."))
            listed = n in grams and ENTRY[n] in c.table
            assert int(c.labels[i]) == (n - 2 if listed else 0), (kind, int(c.labels[i]))
            if listed:    # every planted key that fits the document is a candidate at 4 lane + k
                at = {p for m, p in c.candidates(i) if m == n}
                assert {4 * j + k for j in (lane0, lane0 + 31, lane0 + 62) if 4 * j + k + n <= 256} <= at
    c.run(monkeypatch, narrow)


# ----------------------------------------------------------------- store loop
def lane_text(bloom, lane, c):
    """(n, at, text): bytes [a, b) of T at 4 lane + a, which make the windows
    (p, N), a <= p <= 3, p + N <= b, keys (grams 3..7) -- the choice of a, b with
    n = c candidates in `lane` by the filter's model (a window cut by the text's
    end can still pass: lengths 6 and 7 test three of their bytes), or with the
    most below c where the document's end leaves the lane fewer."""
    best = None
    for a in range(4):
        for b in range(a + 3, len(T) + 1):
            d = bytearray(FILL * 256)
            d[4 * lane + a:4 * lane + b] = T[a:b]
            cand = SA.candidates(bloom, [3, 4, 5, 6, 7], bytes(d[:256]))
            if all(p // 4 == lane for _, p in cand) and len(cand) <= c and (best is None or len(cand) > best[0]):
                best = (len(cand), 4 * lane + a, T[a:b][:256 - (4 * lane + a)])
    return best


def store_docs():
    rng = np.random.default_rng(67)
    bloom = SA.bloom_of(table_of(KEYS_FULL))
    docs, kinds = [], []
    for c in (1, UNROLL - 1, UNROLL, UNROLL + 1, 12, 20):
        for lanes in ((0,), (17,), (37,), (0, 63), (0, 62)):
            d = bytearray(FILL * 256)
            want = {}
            for j in lanes:
                want[j], at, text = lane_text(bloom, j, c)
                d[at:at + len(text)] = text
            docs.append(bytes(d[:256]))
            kinds.append("store%d:" % c + ",".join("%d=%d" % kv for kv in sorted(want.items())))
            docs.append(soup(rng, int(rng.integers(8, 60)), KEYS_FULL))
            kinds.append("ordinary")
    return docs, kinds


@pytest.mark.parametrize("values", [(V,), (V, math.log(1.5))], ids=["count", "class"])
def test_store_loop_bounds(values, monkeypatch):
    docs, kinds = store_docs()
    c = Case(KEYS_FULL, [3, 4, 5, 6, 7], docs, kinds, values)
    seen = set()
    for i, kind in enumerate(c.kinds):
        if kind.startswith("store"):
            want = {int(a): int(b) for a, b in (kv.split("=") for kv in kind.split(":")[1].split(","))}
            per_lane = np.bincount([p // 4 for _, p in c.candidates(i)], minlength=64)
            assert {j: int(n) for j, n in enumerate(per_lane) if n} == want, (kind, per_lane.tolist())
            seen |= set(want.values())
    # both sides of the unroll, the back edge taken twice and four times, and what the last lanes can hold
    assert {1, UNROLL - 1, UNROLL, UNROLL + 1, 12, 20, 17} <= seen, seen
    assert len(np.unique(c.labels)) >= 3
    c.run(monkeypatch, False)


# ----------------------------------------------------------------- tail flush
TOTALS = (64, 65, 128, 129, QUEUE_CAP, QUEUE_CAP + 1)


def tail_case(keys, grams, values=(V,)):
    """24 units of [ordinary, document of the total, ordinary, ordinary]: a wave
    of a 24-wave launch has one unit, of a 12-wave launch two, as one staged
    group either way."""
    rng = np.random.default_rng(71)
    bloom, lens = SA.bloom_of(table_of(keys)), SA.fast_lengths(table_of(keys), grams)
    total = {t: SA.total_doc(bloom, lens, t) for t in TOTALS}
    docs, kinds = [], []
    for u in range(24):
        t = TOTALS[u % len(TOTALS)]
        for d, kind in ((soup(rng, 40, keys), "ordinary"), (total[t], "total%d" % t), (soup(rng, 33, keys), "ordinary"),
                        (soup(rng, 21, keys), "ordinary")):
            docs.append(d)
            kinds.append(kind)
    return Case(keys, grams, docs, kinds, values)


TAIL_CASES = [("narrow-34", KEYS_NARROW, [3, 4], True, (V,)), ("two-languages-34", KEYS_TWO, [3, 4], False, (V,)),
              ("full-345", KEYS_FULL, [3, 4, 5], False, (V,)), ("class-narrow-34", KEYS_NARROW, [3, 4], True, (V, math.log(1.5)))]


@pytest.mark.parametrize("name,keys,grams,narrow,values", TAIL_CASES, ids=[c[0] for c in TAIL_CASES])
def test_tail_flush(name, keys, grams, narrow, values, monkeypatch):
    c = tail_case(keys, grams, values)
    for t in TOTALS:
        for i in c.by("total%d" % t):
            assert max(c.grams) <= len(c.docs[i]) <= 256 and len(c.candidates(i)) == t, (t, len(c.candidates(i)))
    # each such document between ordinary ones of its staged group
    for waves in (geometry.SCORE_WAVES, 2 * geometry.SCORE_WAVES):
        inside = set()
        for g0, cnt in staged_groups(c.off, waves):
            inside |= set(range(g0 + 1, g0 + cnt - 1))
        assert all(i in inside for i, k in enumerate(c.kinds) if k.startswith("total")), waves
    assert len(np.unique(c.labels)) >= 2
    c.run(monkeypatch, narrow)


# ---------------------------------------------------------------- 1-byte skip
SKIP_LENGTHS = (256, 201, 70, 67)


def skip_unit(two):
    """One staged group (655 bytes).  two: every document also holds 2-byte hits."""
    def body(n):
        d = bytearray(FILL * n)
        if two:
            d[3:5] = b"ab"
            d[9:11] = b"ab"
        return d

    docs = [(bytes(body(20)), "none")]
    for n in SKIP_LENGTHS:
        d = body(n)
        d[n - 1:] = b"q"
        docs.append((bytes(d), "last%d" % n))
    docs.append((bytes(body(20)), "poison"))            # ... its only key byte is the next document's first
    d = body(21)
    d[0:1] = b"q"
    docs.append((bytes(d), "after"))
    return docs


@pytest.mark.parametrize("grams", [[1], [1, 2], [1, 2, 3]], ids=str)
def test_one_byte_skip(grams, monkeypatch):
    docs, kinds = [], []
    for u in range(24):
        for d, kind in skip_unit(u % 2 == 1):
            docs.append(d)
            kinds.append(kind + (".2" if u % 2 else ""))
    c = Case(KEYS_NARROW, grams, docs, kinds)
    q, ab = 3, 5                                                   # SHORT's languages
    for i, kind in enumerate(c.kinds):
        two = kind.endswith(".2") and 2 in grams
        want = [0.0] * L
        if kind.startswith(("last", "after")):
            want[q] = V
        if two:
            want[ab] = V + V
        assert c.scores[i].tolist() == want, (kind, c.scores[i].tolist())
        if kind.startswith("poison"):
            assert bytes(c.data[int(c.off[i + 1]):int(c.off[i + 1]) + 1]) == b"q" and b"q" not in c.docs[i]
    # the hit's slot k and lane: every k, and lane 63 alone
    assert {(n - 1) % 4 for n in SKIP_LENGTHS} == {0, 1, 2, 3} and (256 - 1) // 4 == 63
    # a unit is one staged group of a 24-wave launch
    n_unit = len(skip_unit(False))
    assert sorted(staged_groups(c.off, 2 * geometry.SCORE_WAVES)) == [(n_unit * u, n_unit) for u in range(24)]
    c.run(monkeypatch, max(grams) >= 3)           # (no listed length of 3 bytes or more: no narrow table)


# ------------------------------------------------------------------- geometry
def geometry_docs(maxg):
    """For every residue r modulo 16 and every count 1..8: a document above
    1,024 bytes (scored alone, in place) that ends at residue r, then `count`
    documents that fit one staged group."""
    rng = np.random.default_rng(73)
    lengths = [maxg, 256, maxg - 1, 257, 33, 70, maxg + 1, 255]
    big = soup(rng, 1100, KEYS_FULL)
    docs, kinds = [], []
    pos = 0
    for r in range(16):
        for count in range(1, 9):
            n = 1025 + (r - (pos + 1025)) % 16
            docs.append(big[:n])
            kinds.append("big")
            pos += n
            assert pos % 16 == r
            for j in range(count):
                ln = lengths[(j + count + r) % len(lengths)]
                d = bytearray(soup(rng, ln, KEYS_FULL))
                d[max(0, ln - 4):] = b"aaaa"[:min(ln, 4)]          # the last windows keys, and 'a's follow
                docs.append(bytes(d[:ln]))
                kinds.append("g%d.%d" % (r, count))
                pos += ln
    return docs, kinds


@pytest.mark.parametrize("name,keys,grams,narrow", [("narrow", KEYS_NARROW, [1, 2, 3, 4], True),
                                                    ("full", KEYS_FULL, [1, 2, 3, 4, 5], False)],
                         ids=["narrow", "full"])
def test_geometry(name, keys, grams, narrow, monkeypatch):
    maxg = max(grams)
    docs, kinds = geometry_docs(maxg)
    c = Case(keys, grams, docs, kinds)
    off = [int(x) for x in c.off]
    seen, lens = set(), set()
    for waves in (geometry.SCORE_WAVES, 2 * geometry.SCORE_WAVES):
        for g0, cnt in staged_groups(off, waves):
            if c.kinds[g0] != "big":
                seen.add((off[g0] % 16, cnt))
                lens |= {off[i + 1] - off[i] for i in range(g0, g0 + cnt)}
    # every residue of a group's first document, every group size 1..8, most pairs of the two
    assert {r for r, _ in seen} == set(range(16)) and {n for _, n in seen} >= set(range(1, 9)), seen
    assert len({(r, n) for r, n in seen if n <= 8}) >= 100, len(seen)
    assert {maxg - 1, maxg, 256, 257} <= lens, lens
    assert len(np.unique(c.labels)) >= 3
    c.run(monkeypatch, narrow)
