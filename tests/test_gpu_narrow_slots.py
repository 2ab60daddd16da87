"""GPU parity of count / class mode on the narrow slot table
(LDGPU_LAYOUT_NARROW_SLOTS; NarrowSlot, ldgpu_common.h): a table whose keys of
3 bytes and more all have at most 4, one language each, carries them a second
time in 8-byte slots -- key bytes | counter index, multiplicity, length -- and
the order-free LDS-Bloom kernels verify a candidate against those: a 32-bit key
masked to its length, two 24-bit multiplies per slot position, a compare of
key and length.  Hand-built tables and documents put keys where that can go
wrong:

  length    "abc" and "abc\\0" (and the all-zero and all-0xff pairs) in one
            table under different languages, the key followed by 0x00, by
            another byte and by the document's end (the 4-byte window is cut);
            the all-zero keys present and absent (an empty slot equals no
            window);
  bytes     keys that differ only in their fourth byte, only in their first;
  cuckoo    3,000 random keys over 12 letters: the placement walk moves keys to
            their second slot, and every language's count shows in the scores;
  mult      gram lists that repeat a length (the slot's multiplicity);
  sites     every place that verifies: the first 64 candidates of a document
            (split path), the tail up to 288, the per-length path past 288, the
            general path (documents of 257..300 bytes and shorter than
            max(grams)), packs of short documents; tables without direct tables,
            whose 1-/2-byte queue entries read the full slots beside them;
  old path  one 5-byte key, one row of two languages, or LDGPU_NO_NARROW_SLOTS=1
            on the diagnostics library: the flag is clear, the results the same.

Every case asserts the layout flag it expects and compares with the C oracle:
labels exactly, fp64 scores bit for bit where scores are requested."""
import math

import numpy as np
import pytest

import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

L = 6
V = math.log(2.0)
FILL = b"."            # in no key
ZERO3, FF3 = b"\x00" * 3, b"\xff" * 3
PAIRS = [(b"abc", b"abc\x00"), (ZERO3, ZERO3 + b"\x00"), (FF3, FF3 + b"\xff")]
SHORT = {b"q": [3], b"\x00": [4], b"zq": [4], b"\xff\x00": [5]}          # direct tables
BYTES = {b"abcd": [0], b"abce": [1], b"abcf": [2], b"bbcd": [3], b"cbcd": [4], b"dbc": [5], b"ebc": [2]}
RUNS = {b"aaa": [1], b"aaaa": [2]}


def pair_keys(zero=True):
    t = {}
    for k3, k4 in PAIRS:
        if k3 == ZERO3 and not zero:
            continue
        t[k3], t[k4] = [0], [1]
    return t


def table_of(keys, values=(V,)):
    t = {}
    for i, (k, langs) in enumerate(sorted(keys.items())):
        row = [0.0] * L
        for l in langs:
            row[l] = values[i % len(values)]
        t[k] = row
    return t


MAIN_KEYS = {**SHORT, **BYTES, **RUNS, **pair_keys()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# --------------------------------------------------------------------- corpus
def pair_docs():
    """Each key of PAIRS followed by 0x00, by another byte, by the document's
    end -- at every residue of the position modulo 4 -- and the byte that would
    complete the 4-byte key opening the next document."""
    docs = []
    for k3, k4 in PAIRS:
        for pad in range(4):
            lead = FILL * (9 + pad)
            docs += [lead + k3 + b"\x00" + FILL * 7, lead + k3 + b"x" + FILL * 7, lead + k3 + k4[-1:] + FILL * 5,
                     lead + k4 + b"\x00" + FILL * 6, lead + k4 + k4[-1:] + FILL * 3]
            docs += [lead + k3, k4[-1:] + FILL * 11, lead + k4, k4[-1:] * 2 + FILL * 9]
    return docs


def site_docs(rng):
    """The verify sites (grams of 3 and 4 bytes: 'a' * n has 2 n - 5 true candidates)."""
    docs = []
    for n in (35, 36, 100, 146):                 # 65, 67, 195, 287 candidates: the tail past the first 64
        docs += [b"a" * n + FILL * (256 - n), b"a" * n]
    for n in (147, 200, 256):                    # 289 and more: the per-length path
        docs += [b"a" * n + FILL * (256 - n)]
    alphabet = np.frombuffer(b"abcdefq.z\x00\xff", dtype=np.uint8)
    for n in (257, 258, 259, 260, 283, 300):     # the general path: long documents
        d = bytearray(rng.choice(alphabet, size=n).tobytes())
        d[n - 4:] = b"abc\x00"
        d[100:108] = b"aaaaaaaa"
        docs.append(bytes(d))
    # ... and documents shorter than max(grams): partial windows (the whole document as a key)
    docs += [b"", b"q", b"zq", b"abc", b"aaa", b"dbc", ZERO3, FF3, b"ab", b"\x00", b"abc\x00", b"aaaa"]
    # runs of 20..60-byte documents: packs
    for n in rng.integers(20, 61, size=120):
        d = bytearray(rng.choice(alphabet, size=int(n)).tobytes())
        k = list(MAIN_KEYS)[int(rng.integers(len(MAIN_KEYS)))]
        at = int(rng.integers(0, int(n) - 4))
        d[at:at + len(k)] = k
        docs.append(bytes(d[:int(n)]))
    for n in rng.integers(4, 257, size=80):      # fast-path documents of every alignment
        docs.append(rng.choice(alphabet, size=int(n)).tobytes())
    return docs


def main_docs():
    return pair_docs() + site_docs(np.random.default_rng(53))


class Case:
    """A table, a gram list and documents, with the oracle's labels and scores."""

    def __init__(self, keys, grams, docs, values=(V,)):
        self.table, self.grams, self.docs = table_of(keys, values), list(grams), docs
        self.data, self.off = encoding.pack(docs)
        self.labels, self.scores = OC.Table(self.table, L).score(self.grams, self.data, self.off, want_scores=True,
                                                                 nthreads=8)

    def check(self, m, want_scores):
        labels, scores = m.score(self.data, self.off, want_scores=want_scores)
        bad = np.nonzero(labels != self.labels)[0]
        assert not len(bad), [(int(i), self.docs[i][:24]) for i in bad[:8]]
        if want_scores:
            bad = np.nonzero((bits(scores) != bits(self.scores)).any(axis=1))[0]
            assert not len(bad), [(int(i), self.docs[i][:24], scores[i].tolist(), self.scores[i].tolist()) for i in bad[:4]]

    def run(self, monkeypatch, narrow, has=(), hasnt=(), scores=True, grids=("1",), env=()):
        """The product library (labels only: packs; with scores), then the
        diagnostics library on few workgroups (many documents per wave)."""
        def one(m):
            info = m.info()
            assert ("narrow_slots" in info["layout"]) == narrow, info
            assert set(has) <= set(info["layout"]) and not set(hasnt) & set(info["layout"]), info
            self.check(m, False)
            if scores:
                self.check(m, True)
            m.close()

        if not env:
            one(DeviceModel(self.table, L, self.grams))
        for k, v in env:
            monkeypatch.setenv(k, v)
        for grid in grids:
            monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
            one(DeviceModel(self.table, L, self.grams, variant="diag"))


@pytest.fixture(scope="module")
def main():
    return Case(MAIN_KEYS, [1, 2, 3, 4], main_docs())


# ---------------------------------------------------------------------- tests
def test_corpus_reaches_the_cases(main):
    """Host-side: what the GPU cases lean on."""
    t = main.table
    for k3, k4 in PAIRS:
        assert t[k3][0] and t[k4][1] and not t[k3][1] and not t[k4][0]
    assert max(len(k) for k in t) == 4 and all(sum(1 for v in r if v) == 1 for r in t.values())
    n = [len(d) for d in main.docs]
    assert any(257 <= x <= 300 for x in n) and any(x < 4 for x in n) and sum(20 <= x <= 60 for x in n) >= 100
    # candidates of the 'a' runs (true keys alone): both sides of 64 and of the queue's 288
    runs = sorted({2 * len(d.rstrip(FILL)) - 5 for d in main.docs if d.startswith(b"a" * 35) and set(d) <= set(b"a.")})
    assert runs[0] == 65 and 287 in runs and 289 in runs and runs[-1] == 507, runs
    # the length matters: a key of each pair scores differently from its twin
    assert len(np.unique(main.labels)) >= 5
    i3 = main.docs.index(FILL * 9 + b"abc")
    i4 = main.docs.index(FILL * 9 + b"abc\x00")
    assert main.scores[i3].tolist() != main.scores[i4].tolist()


def test_main_table(main, monkeypatch):
    """Length in the compare, fourth and first byte, every verify site; packs on the labels-only call."""
    main.run(monkeypatch, True, has=("direct", "packs", "lds_bloom"), grids=("1", "2"))


@pytest.mark.parametrize("grams", [[3, 4], [3, 3, 4], [1, 2, 3, 4, 4, 4], [4], [3]], ids=str)
def test_gram_lists(grams, monkeypatch):
    """Multiplicity: a repeated length counts that many times; a length not listed does not count."""
    c = Case(MAIN_KEYS, grams, main_docs())
    if grams == [3, 3, 4]:
        once = OC.Table(c.table, L).score([3, 4], c.data, c.off, want_scores=True, nthreads=8)[1]
        assert not np.array_equal(once, c.scores)
    c.run(monkeypatch, True, has=("direct",))


def test_zero_keys_absent(monkeypatch):
    """No all-zero key: windows of zeros (what an empty slot holds) hit nothing."""
    keys = {**SHORT, **BYTES, **RUNS, **pair_keys(zero=False)}
    docs = main_docs() + [b"\x00" * n for n in (3, 4, 5, 64, 256)] + [FILL * 5 + b"\x00" * 40 + FILL * 3]
    c = Case(keys, [1, 2, 3, 4], docs)
    i = c.docs.index(b"\x00" * 64)
    assert np.nonzero(c.scores[i])[0].tolist() == [4]      # the 1-byte key b"\x00" alone
    c.run(monkeypatch, True, has=("direct",))
    # ... and with neither short keys nor direct counts: a document of zeros scores nothing at all
    c2 = Case({**BYTES, **pair_keys(zero=False)}, [3, 4], docs)
    assert not c2.scores[i].any()
    c2.run(monkeypatch, True)


def test_both_cuckoo_slots(monkeypatch):
    """3,000 random keys of 3 and 4 bytes over 12 letters; documents of the same letters."""
    rng = np.random.default_rng(59)
    letters = np.frombuffer(b"abcdefghijkl", dtype=np.uint8)
    keys = {}
    while len(keys) < 3000:
        k = rng.choice(letters, size=int(rng.integers(3, 5))).tobytes()
        keys.setdefault(k, [int(rng.integers(L))])
    docs = [rng.choice(letters, size=int(n)).tobytes() for n in rng.integers(4, 257, size=240)]
    docs += [rng.choice(letters, size=int(n)).tobytes() for n in rng.integers(20, 61, size=60)]
    c = Case(keys, [3, 4], docs)
    assert (c.scores > 0).all(axis=1).sum() > 100      # every language counted in most documents
    c.run(monkeypatch, True)


def test_without_direct_tables(main, monkeypatch):
    """A 2-byte key of two languages: no direct tables, so 1-/2-byte entries are
    queued and read the full slots beside the narrow ones (flush)."""
    c = Case({**MAIN_KEYS, b"yz": [1, 3]}, [1, 2, 3, 4], main.docs + [b"yz" * 20, b"abcyzabc\x00yz"])
    c.run(monkeypatch, True, hasnt=("direct",))


@pytest.mark.parametrize("change", ["five_bytes", "two_languages", "env"])
def test_ineligible_tables_keep_the_full_slots(main, change, monkeypatch):
    keys, grams, env = dict(MAIN_KEYS), [1, 2, 3, 4], ()
    if change == "five_bytes":
        keys[b"abcde"] = [2]
        grams = [1, 2, 3, 4, 5]
    elif change == "two_languages":
        keys[b"fbc"] = [1, 3]
    else:
        env = (("LDGPU_NO_NARROW_SLOTS", "1"),)
    docs = main.docs + [FILL * 7 + b"abcde" + FILL * 4, FILL * 6 + b"fbc" + FILL * 4]
    Case(keys, grams, docs).run(monkeypatch, False, has=("direct",), env=env)


def test_class_mode(main, monkeypatch):
    """Two row values: class mode (labels only) counts per (class, language) from the narrow slots."""
    c = Case(MAIN_KEYS, [1, 2, 3, 4], main.docs, values=(V, math.log(1.5)))
    assert len({v for r in c.table.values() for v in r if v}) == 2
    c.run(monkeypatch, True, has=("classes", "direct"), scores=False, grids=("1", "2"))
    # ... and a table outside the rule keeps class mode on the full slots
    Case({**MAIN_KEYS, b"abcde": [2]}, [1, 2, 3, 4, 5], main.docs, values=(V, math.log(1.5))).run(
        monkeypatch, False, has=("classes",), scores=False)
