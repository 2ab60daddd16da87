"""GPU parity of count mode on the LDS trie's pair form (LDGPU_LAYOUT_TRIE_PAIR;
csrc/ldgpu_trie.h, csrc/ldgpu_trie.hip): a table in the path-sum form whose
largest path count Wmax times its language count L is at most 63 gives every
(language l, W) pair a counter of its own, slot 1 + l + L (W - 1); a node holds
its counter's byte offset, a walk adds 1 there, and the label's argmax weighs
the counters, c(l) = sum of w * counter(l, w).

Labels must equal the C oracle's exactly.  Every table runs on the product
library and on the diagnostics library under LDGPU_SCORE_GRID=1 (one workgroup:
several documents per wave, so a counter left uncleared meets the next
document), LDGPU_NO_TRIE_PAIR=1 (the path-sum form), LDGPU_NO_TRIE_SUM=1 (the
plain trie; it must switch the pair form off too) and LDGPU_NO_TRIE=1 (the
LDS-Bloom kernel, the control); the layout is asserted each time.

  benchmark  the 10,000 rows of bench.py's config 2 have the form (60 slots)
  corpus     test_gpu_trie's 412 documents (lengths max(grams) - 1 .. + 1,
             253..257, above 1,024, every slot, the tail cases) under KEYS_U with
             L = 8 and the lists [1, 2, 3, 4] (Wmax = 4), [2, 4] (2) and [1] (1)
  bounds     L = 21 with a chain of W = 3 for language 20: slot 63 decides;
             L = 15 with W = 4 (slot 60); L = 63 with Wmax = 1, winner 62;
             L = 16 with W = 4 (64 slots): no pair form, the path-sum form
  weights    language 0 has five hits of W = 1, language 1 two hits of W = 3
             and wins 6 : 5; the twin document with one hit of W = 3 goes to
             language 0.  The two alternate, 16,384 documents, so that on the
             product library too a wave scores several in a row
  negative   the same documents under a negative table value: the smallest
             weighted count wins
  lengths    max(grams), 5, 253, 255, 256 with a hit of W = 3 on the last bytes,
             and leftovers (2 bytes, 257 bytes) in the same call
  calls      0, 1 and 25 documents; ldgpu_score_device on torch tensors

Hand mutations of ldgpu_trie.hip, each built once and not committed: see
DESIGN.md for the cases that fail."""
import functools

import numpy as np
import pytest

import ldoracle_c as OC
from languagedetection import encoding
from languagedetection.runtime import DeviceModel
from test_gpu_trie import FILL, V, check_labels, corpus
from test_gpu_trie_sum import KEYS_U, oracle as corpus_oracle, table_of

pytestmark = pytest.mark.gpu

DIAG_RUNS = (  # (environment, "trie" / "trie_sum" / "trie_pair" expected where the table has the pair form)
    ({"LDGPU_SCORE_GRID": "1"}, (True, True, True)),
    ({"LDGPU_NO_TRIE_PAIR": "1"}, (True, True, False)),
    ({"LDGPU_NO_TRIE_SUM": "1"}, (True, False, False)),
    ({"LDGPU_NO_TRIE": "1"}, (False, False, False)),
)


def layout_of(m):
    lay = m.info()["layout"]
    return "trie" in lay, "trie_sum" in lay, "trie_pair" in lay


def run_all(table, nl, grams, data, off, labels, monkeypatch, has_pair=True, kinds=None, call=check_labels):
    """Product library and the four diagnostics runs; yields nothing, asserts layout and labels each time."""
    m = DeviceModel(table, nl, grams)
    assert layout_of(m) == (True, True, has_pair), m.info()
    call(m, data, off, labels, kinds)
    m.close()
    for env, (trie, tsum, pair) in DIAG_RUNS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = DeviceModel(table, nl, grams, variant="diag")
        assert layout_of(d) == (trie, tsum, pair and has_pair), (env, d.info())
        call(d, data, off, labels, kinds)
        d.close()
        for k in env:
            monkeypatch.delenv(k)


def rows(keys, nl, value=V):
    t = {}
    for k, l in keys.items():
        row = [0.0] * nl
        row[l] = value
        t[k] = row
    return t


def chain(lang, depth, byte=b"r"):
    return {byte * d: lang for d in range(1, depth + 1)}


def doc_of(pieces, n=240):
    """A document of n fill bytes with the pieces three bytes apart from byte 8 on."""
    d, at = bytearray([FILL]) * n, 8
    for p in pieces:
        d[at:at + len(p)] = p
        at += len(p) + 3
    assert at <= n
    return bytes(d)


def scored(table, nl, grams, docs):
    data, off = encoding.pack(docs)
    assert len(docs) == 0 or off[-1] / len(docs) >= 192.0   # the launch does not pack
    labels, scores = OC.Table(table, nl).score(list(grams), data, off, want_scores=True, nthreads=8)
    return data, off, labels, scores


# ---------------------------------------------------------------- the corpus
@pytest.mark.parametrize("grams", [[1, 2, 3, 4], [2, 4], [1]], ids=str)
def test_corpus_labels_match_the_oracle(grams, monkeypatch):
    docs, kinds, data, off = corpus(max(grams))
    labels, _ = corpus_oracle(tuple(grams))
    assert len(np.unique(labels)) >= 4
    run_all(table_of(KEYS_U), 8, grams, data, off, labels, monkeypatch, kinds=kinds)


def test_benchmark_table_has_the_pair_form(monkeypatch):
    """The 10,000 rows of bench.py's config 2 (L = 20, grams 1..5, Wmax = 3: 60 slots) on 2,000 documents of 256 bytes."""
    from languagedetection import synth
    from test_gpu_trie_sum import FIXTURE
    rec = np.fromfile(FIXTURE, dtype=np.uint8).reshape(-1, 6)
    table = rows({bytes(r[:int(r[4])]): int(r[5]) for r in rec}, 20)
    assert len(table) == 10000
    data, off, _ = synth.generate(synth.make_languages(20), 2000, 256, 256, seed=synth.SEED_BASE + 2)
    grams = [1, 2, 3, 4, 5]
    labels, _ = OC.Table(table, 20).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) == 20
    run_all(table, 20, grams, data, off, labels, monkeypatch)


# ---------------------------------------------------------------- the bounds
def test_slot_63_decides(monkeypatch):
    """L = 21, "r" / "rr" / "rrr" of language 20: one "rrr." counts 3 + 2 + 1 at the slots 63, 42 and 21, against
    4, 5 (language 20 wins only with slot 63's three) and 6 (a tie: the first maximum) hits of language 5."""
    nl, grams = 21, [1, 2, 3]
    table = rows({**chain(20, 3), b"q": 5}, nl)
    docs = [doc_of([b"rrr"] + [b"q"] * n) for n in (4, 5, 6, 2)] + [doc_of([b"q"] * 3), doc_of([b"rr", b"q", b"q"])]
    data, off, labels, scores = scored(table, nl, grams, docs)
    assert labels.tolist() == [20, 20, 5, 20, 5, 20]
    assert [round(s[20] / V) for s in scores] == [6, 6, 6, 6, 0, 3]
    run_all(table, nl, grams, data, off, labels, monkeypatch)


def test_fifteen_languages_weight_4(monkeypatch):
    """L = 15, the chain "r" .. "rrrr" of language 14 (W = 4, slot 60): "rrrr." counts 10, against 9, 10 and 11 of language 3."""
    nl, grams = 15, [1, 2, 3, 4]
    table = rows({**chain(14, 4), b"q": 3}, nl)
    docs = [doc_of([b"rrrr"] + [b"q"] * n) for n in (9, 10, 11)]
    data, off, labels, scores = scored(table, nl, grams, docs)
    assert labels.tolist() == [14, 3, 3] and [round(s[14] / V) for s in scores] == [10] * 3
    run_all(table, nl, grams, data, off, labels, monkeypatch)


def test_63_languages_weight_1(monkeypatch):
    """L = 63 with Wmax = 1 (63 slots): language 62 wins, and loses the tie to language 0."""
    nl, grams = 63, [1, 2]
    table = rows({b"q": 62, b"a": 0, b"xy": 30}, nl)
    docs = [doc_of([b"q"] * 3 + [b"a"] * 2 + [b"xy"]), doc_of([b"q"] * 2 + [b"a"] * 2), doc_of([b"xy"] * 2 + [b"q"])]
    data, off, labels, _ = scored(table, nl, grams, docs)
    assert labels.tolist() == [62, 0, 30]
    run_all(table, nl, grams, data, off, labels, monkeypatch)


def test_sixteen_languages_weight_4_keeps_the_sum_form(monkeypatch):
    """L = 16 with W = 4 would need 64 slots: no "trie_pair", the path-sum form, the same labels."""
    nl, grams = 16, [1, 2, 3, 4]
    table = rows({**chain(15, 4), b"q": 3}, nl)
    docs = [doc_of([b"rrrr"] + [b"q"] * n) for n in (9, 10, 11)]
    data, off, labels, _ = scored(table, nl, grams, docs)
    assert labels.tolist() == [15, 3, 3]
    run_all(table, nl, grams, data, off, labels, monkeypatch, has_pair=False)


# --------------------------------------------------------------- the weights
WEIGHT_KEYS = {b"q": 0, b"x": 1, b"xy": 1, b"xyz": 1, b"m": 2}   # "xyz" is ONE hit of W = 3 ("y", "z" are no keys)
B_WINS = doc_of([b"q"] * 5 + [b"xyz"] * 2 + [b"m"] * 7)   # hits 5 : 2 : 7, weighted 5 : 6 : 7
A_WINS = doc_of([b"q"] * 5 + [b"xyz"] + [b"m"] * 7)       # hits 5 : 1 : 7, weighted 5 : 3 : 7


@functools.lru_cache(maxsize=None)
def weight_case(value, tiles, with_m=True):
    """B_WINS and A_WINS alternating, then each twice; with_m=False: a table without language 2's key."""
    table = rows({k: l for k, l in WEIGHT_KEYS.items() if with_m or l != 2}, 3, value)
    return (table,) + scored(table, 3, [1, 2, 3], [B_WINS, A_WINS] * tiles + [A_WINS, A_WINS, B_WINS, B_WINS])


def test_weighted_total_beats_hit_count(monkeypatch):
    """Without language 2's key the documents are language 1's (6 : 5) and language 0's (5 : 3): a dropped weight
    gives both to language 0, a W = 3 counter left uncleared gives the second to language 1."""
    table, data, off, labels, scores = weight_case(V, 1, with_m=False)
    assert labels.tolist() == [1, 0, 0, 0, 1, 1]
    assert [[round(x / V) for x in s] for s in scores[:2]] == [[5, 6, 0], [5, 3, 0]]
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


def test_opposite_winners_back_to_back(monkeypatch):
    """16,388 alternating documents: more than two per wave on the product library's grid too."""
    table, data, off, labels, _ = weight_case(V, 8192, with_m=False)
    assert len(labels) == 16388 and labels[:4].tolist() == [1, 0, 1, 0] and labels[-4:].tolist() == [0, 0, 1, 1]
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


def test_negative_table_value(monkeypatch):
    """Every language is hit and the value is negative: the smallest weighted count wins -- language 0 (5 of 5 : 6 : 7)
    and language 1 (3 of 5 : 3 : 7); by hits alone both were language 1's."""
    table, data, off, labels, scores = weight_case(-0.75, 12)
    assert labels[:2].tolist() == [0, 1] and labels[-4:].tolist() == [1, 1, 0, 0]
    assert [[round(x / -0.75) for x in s] for s in scores[:2]] == [[5, 6, 7], [5, 3, 7]]
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


# ------------------------------------------------------- lengths and leftovers
def test_lengths_and_leftovers(monkeypatch):
    """Documents of max(grams) = 3, 5, 253, 255 and 256 bytes that end in "xyz" (a hit of W = 3 on the last window),
    and their twins one byte shorter that end in "xy" (W = 2) with the next document going on with "z": the walk
    ends with the document.  2 and 257 bytes are left to the other kernel in the same call."""
    table = rows(WEIGHT_KEYS, 3)
    docs, ends = [], []
    for n in (3, 5, 253, 255, 256, 2, 257):
        d = bytearray([FILL]) * n
        if n >= 16:
            d[8:9], d[12:13] = b"q", b"m"
        d[max(0, n - 3):] = b"xyz"[-min(n, 3):] if n >= 3 else b"xy"
        ends.append(len(docs))
        docs += [bytes(d), bytes([FILL]) * 256, bytes(d[:-1]), b"z" + doc_of([b"m", b"m"], 255), doc_of([b"q"] * 3, 256)]
    data, off, labels, scores = scored(table, 3, [1, 2, 3], docs)
    # (a document shorter than a gram length is one partial window of that length: "xy" and "x" count 3 too)
    assert [round(scores[i][1] / V) for i in ends] == [3, 3, 3, 3, 3, 3, 3]
    assert [round(scores[i + 2][1] / V) for i in ends] == [3, 2, 2, 2, 2, 3, 2]
    assert len(np.unique(labels)) == 3
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


# ------------------------------------------------------------------ the calls
def test_document_counts_and_device_call(monkeypatch):
    """0, 1 and 25 documents through the host call and through ldgpu_score_device on torch tensors."""
    from test_gpu_trie_calls import device_labels
    table, data, off, labels, _ = weight_case(-0.75, 12)
    assert len(labels) >= 25 and len(np.unique(labels[:25])) == 2

    def few(m, data, off, labels, kinds):
        for n in (0, 1, 25):
            got, _ = m.score(data[:int(off[n]) + 8], off[:n + 1], want_scores=False)
            assert np.array_equal(got, labels[:n]), n
            dev = device_labels(m, data, int(off[n]), off[:n + 1], n_docs=n)
            assert len(dev) == n and np.array_equal(dev, labels[:n]), n

    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch, call=few)
