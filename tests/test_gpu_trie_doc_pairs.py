"""GPU parity of the LDS trie's pair form with two documents per counter pass
(csrc/ldgpu_trie.hip: pair_argmax2; L <= 32): the first document of a pair counts
1 and the second 0x10000 at the same counters, and one pass over the counters
labels both -- the low halves in lanes 0..31, the high halves in lanes 32..63.

Labels must equal the C oracle's exactly.  Every case runs on the product
library and on the diagnostics library under LDGPU_SCORE_GRID=1 (one workgroup
of 12 waves: a wave scores its documents in a row, so pairs form),
LDGPU_NO_TRIE_DOC_PAIRS=1 (also on one workgroup: the per-document pass),
LDGPU_NO_TRIE_PAIR=1 (the path-sum form) and LDGPU_NO_TRIE=1 (the LDS-Bloom
kernel, the control); the layout is asserted each time.  Which documents share
a pair depends on the grid and on the staged groups, so the cases that lean on
a pairing assert it on the host model of the kernel's geometry (pairs_of).

  counts     calls of 0, 1, 2, 3, 4, 5 and 25 documents
  odd groups lengths 256, 256, 256, 257, ... and 200, 201, ...: groups of odd and
             even numbers of scored documents, the last one labelled alone
  leftovers  a document left to the other kernel (2 bytes; 257 bytes) where the
             first of a pair would be, between a first and its second, and
             between two pairs
  bleed      256 hits of one W = 1 counter (a half of 0x100) beside a document
             with one hit of another language, in both orders; 254 walks of a
             W = 3 path (a weighted half of 765) beside a document of language 0
  winners    opposite winners in a pair; both winners language L - 1; 24,576
             documents, so that the product library's grid forms pairs too
  languages  L = 32 with Wmax = 1 (pairs on, lane 31 and lane 63 decide), L = 33
             (pairs off: the labels say so), L = 1, L = 21 with Wmax = 3 (slot 63)
  sign       a negative table value
  device     ldgpu_score_device with offsets[0] = 17

Hand mutations of ldgpu_trie.hip, each built once and not committed: see
DESIGN.md for the cases that fail."""
import numpy as np
import pytest

import geometry
import ldoracle_c as OC
from test_gpu_trie import FILL, V, check_labels
from test_gpu_trie_pair import A_WINS, B_WINS, WEIGHT_KEYS, chain, doc_of, layout_of, rows, scored, weight_case
from languagedetection.runtime import DeviceModel

pytestmark = pytest.mark.gpu

GRID1 = {"LDGPU_SCORE_GRID": "1"}
DIAG_RUNS = (  # (environment, "trie" / "trie_sum" / "trie_pair" expected where the table has the pair form)
    (GRID1, (True, True, True)),
    ({**GRID1, "LDGPU_NO_TRIE_DOC_PAIRS": "1"}, (True, True, True)),
    ({"LDGPU_NO_TRIE_PAIR": "1"}, (True, True, False)),
    ({"LDGPU_NO_TRIE": "1"}, (False, False, False)),
)


def run_all(table, nl, grams, data, off, labels, monkeypatch, call=check_labels):
    """Product library and the four diagnostics runs; asserts layout and labels each time."""
    m = DeviceModel(table, nl, grams)
    assert layout_of(m) == (True, True, True), m.info()
    call(m, data, off, labels, None)
    m.close()
    for env, lay in DIAG_RUNS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = DeviceModel(table, nl, grams, variant="diag")
        assert layout_of(d) == lay, (env, d.info())
        call(d, data, off, labels, None)
        d.close()
        for k in env:
            monkeypatch.delenv(k)


def pairs_of(off, maxg, n_waves=geometry.SCORE_WAVES):
    """The kernel's pairing on a grid of n_waves waves, restated: (pairs, alone, roles).  pairs = [(first, second)],
    alone = the documents labelled at their group's end, roles = {what a document left to the other kernel sat at:
    "first" (no document pending, a scored one follows in the group), "inside" (between a first and its second),
    "between" (after a whole pair and before another scored document of the group)}."""
    off = [int(x) for x in off]
    pairs, alone, roles = [], [], set()
    for lo, hi in geometry.wave_ranges(len(off) - 1, n_waves):
        for g0, cnt, staged in (geometry.groups(off, lo, hi) if lo < hi else []):
            ok = [staged and maxg <= off[i + 1] - off[i] <= 256 for i in range(g0, g0 + cnt)]
            pend, done = None, 0
            for j, i in enumerate(range(g0, g0 + cnt)):
                if not ok[j]:
                    if any(ok[j + 1:]):
                        roles.add("inside" if pend is not None else ("between" if done else "first"))
                elif pend is None:
                    pend = i
                else:
                    pairs.append((pend, i))
                    pend, done = None, done + 1
            if pend is not None:
                alone.append(pend)
    return pairs, alone, roles


def sized(doc, n):
    """`doc` cut or filled to n bytes (the pieces of A_WINS and B_WINS sit in their first 72 bytes)."""
    assert n >= 72
    return (doc + bytes([FILL]) * n)[:n]


NO_M = {k: l for k, l in WEIGHT_KEYS.items() if l != 2}   # B_WINS is language 1's (6 : 5), A_WINS language 0's (5 : 3)


# ------------------------------------------------------------ document counts
def test_document_counts(monkeypatch):
    table, data, off, labels, _ = weight_case(V, 12, with_m=False)
    assert len(labels) >= 25 and labels[:5].tolist() == [1, 0, 1, 0, 1]

    def few(m, data, off, labels, kinds):
        for n in (0, 1, 2, 3, 4, 5, 25):
            got, _ = m.score(data[:int(off[n]) + 8], off[:n + 1], want_scores=False)
            assert np.array_equal(got, labels[:n]), (n, got.tolist())

    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch, call=few)


# ----------------------------------------------------------------- odd groups
@pytest.mark.parametrize("lengths", [[256, 256, 256, 257] * 48, list(range(200, 257)) * 4], ids=["256x3+257", "200.."])
def test_odd_and_even_groups(lengths, monkeypatch):
    """Groups of 3 and 4 documents of 256 bytes (one cut short by the 257 that follows: 1 and 2 scored documents),
    and of 3 to 5 documents of 200.. bytes: the last document of an odd group is labelled alone."""
    table = rows(NO_M, 3)
    docs = [sized((B_WINS, A_WINS, A_WINS, B_WINS, B_WINS)[i % 5], n) for i, n in enumerate(lengths)]
    data, off, labels, _ = scored(table, 3, [1, 2, 3], docs)
    pairs, alone, _ = pairs_of(off, 3)
    assert len(pairs) >= 40 and len(alone) >= 12
    assert {(int(labels[a]), int(labels[b])) for a, b in pairs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {int(labels[a]) for a in alone} == {0, 1}
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


# ------------------------------------------------------------------ leftovers
def test_leftovers_do_not_break_a_pair(monkeypatch):
    """Documents of 2 and of 257 bytes among scored ones of 230..256: they are left to the other kernel and touch no
    counter, wherever they stand in a group."""
    table = rows(NO_M, 3)
    a, b = sized(A_WINS, 240), sized(B_WINS, 232)
    x2, x257 = b"xy", sized(B_WINS, 257)
    docs = []
    for rep in range(12):
        for pat in ([x2, a, b], [a, x2, b], [b, a, x2, a, b], [b, x257, a], [x257, b, a, a], [a, b, x257, b, a]):
            docs += pat
        docs += [a, b][:rep % 3]     # (the patterns fall on other places of their groups from repeat to repeat)
    data, off, labels, _ = scored(table, 3, [1, 2, 3], docs)
    pairs, alone, roles = pairs_of(off, 3)
    assert roles == {"first", "inside", "between"} and len(pairs) >= 40 and alone
    assert len({(int(labels[p]), int(labels[q])) for p, q in pairs}) == 4
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


# ---------------------------------------------------------------------- bleed
def bleed_case(table, nl, grams, big, small, want_big, want_small, monkeypatch):
    docs = [big, small] * 24 + [small, big] * 24 + [big, big, small, small, small] * 10
    data, off, labels, _ = scored(table, nl, grams, docs)
    assert labels[:2].tolist() == [want_big, want_small]
    pairs, alone, _ = pairs_of(off, max(grams))
    assert {(int(labels[p]), int(labels[q])) for p, q in pairs} == {(x, y) for x in (want_big, want_small)
                                                                     for y in (want_big, want_small)}
    assert {int(labels[p]) for p in alone} == {want_big, want_small}
    run_all(table, nl, grams, data, off, labels, monkeypatch)


def test_a_half_of_0x100_beside_one_hit(monkeypatch):
    """256 hits at one W = 1 counter of language 0: the half holds 0x100, bit 8 and nothing below.  The other document's
    one hit is language 1's."""
    table = rows({b"a": 0, b"q": 1}, 2)
    bleed_case(table, 2, [1], b"a" * 256, doc_of([b"q"], 250), 0, 1, monkeypatch)


def test_largest_weighted_half(monkeypatch):
    """"r" * 256 under the chain "r", "rr", "rrr" of language 2: 254 walks of W = 3, one of W = 2 and one of W = 1, a
    weighted half of 765, beside a document with three hits of language 0."""
    table = rows({**chain(2, 3), b"q": 0}, 3)
    bleed_case(table, 3, [1, 2, 3], b"r" * 256, doc_of([b"q"] * 3, 250), 2, 0, monkeypatch)


# -------------------------------------------------------------------- winners
def test_winners_on_the_product_grid(monkeypatch):
    """Opposite winners and twice the last language, 24,576 documents: four and more per wave on the product library's
    grid of at most 12 * 2 * 256 waves, so pairs form there too."""
    table = rows({**NO_M, b"m": 3}, 4)                            # L = 4; "m" names language 3 = L - 1
    last = doc_of([b"m"] * 8 + [b"q"] * 2)
    period = [doc_of([b"q"] * 5 + [b"xyz"] * 2), doc_of([b"q"] * 5 + [b"xyz"]), last, last]   # 5 : 6, 5 : 3, 2 : 0 : 0 : 8
    period += period[1::-1]
    data, off, labels, _ = scored(table, 4, [1, 2, 3], period)
    assert labels.tolist() == [1, 0, 3, 3, 0, 1]
    td, to = geometry.tile(data, off, 4096)
    tl = np.tile(labels, 4096)
    for waves in (geometry.SCORE_WAVES, geometry.SCORE_WAVES * 512):
        pairs, _, _ = pairs_of(to, 3, waves)
        assert {(int(tl[p]), int(tl[q])) for p, q in pairs} >= {(1, 0), (0, 1), (3, 3)}
    run_all(table, 4, [1, 2, 3], td, to, tl, monkeypatch)


# ------------------------------------------------------------ language counts
def lang_docs():
    hi, lo, mid = doc_of([b"q"] * 3 + [b"a"] * 2 + [b"xy"]), doc_of([b"q"] * 2 + [b"a"] * 2), doc_of([b"xy"] * 2 + [b"q"])
    return [hi, lo, mid, hi, hi, mid, lo, lo, mid, mid] * 12


@pytest.mark.parametrize("nl", [32, 33])
def test_32_languages_pair_and_33_do_not(nl, monkeypatch):
    """Wmax = 1.  L = 32: lanes 31 and 63 hold the last language's counts, and it loses the tie to language 0.
    L = 33: the kernel keeps the per-document pass (nothing but the labels can say so)."""
    table = rows({b"q": nl - 1, b"a": 0, b"xy": 30}, nl)
    data, off, labels, _ = scored(table, nl, [1, 2], lang_docs())
    assert labels[:3].tolist() == [nl - 1, 0, 30]
    run_all(table, nl, [1, 2], data, off, labels, monkeypatch)


def test_one_language(monkeypatch):
    table = rows({b"q": 0, b"xy": 0}, 1)
    data, off, labels, _ = scored(table, 1, [1, 2], lang_docs())
    assert not labels.any()
    run_all(table, 1, [1, 2], data, off, labels, monkeypatch)


def test_slot_63_in_a_pair(monkeypatch):
    """L = 21, "r" / "rr" / "rrr" of language 20 (slots 21, 42, 63): "rrr." counts 6 against 4, 5 and 6 hits of language 5."""
    table = rows({**chain(20, 3), b"q": 5}, 21)
    docs = ([doc_of([b"rrr"] + [b"q"] * n) for n in (4, 5, 6, 2)] + [doc_of([b"q"] * 3), doc_of([b"rr", b"q", b"q"])]) * 16
    data, off, labels, _ = scored(table, 21, [1, 2, 3], docs)
    assert labels[:6].tolist() == [20, 20, 5, 20, 5, 20]
    run_all(table, 21, [1, 2, 3], data, off, labels, monkeypatch)


# ----------------------------------------------------------------------- sign
def test_negative_table_value(monkeypatch):
    """The smallest weighted count wins: language 0 (5 of 5 : 6 : 7) and language 1 (3 of 5 : 3 : 7) in turn."""
    table, data, off, labels, _ = weight_case(-0.75, 48)
    assert labels[:2].tolist() == [0, 1] and labels[-4:].tolist() == [1, 1, 0, 0]
    run_all(table, 3, [1, 2, 3], data, off, labels, monkeypatch)


# --------------------------------------------------------------------- device
def test_device_call_with_offsets_from_17(monkeypatch):
    """ldgpu_score_device on torch tensors, 17 key bytes in front that belong to no document."""
    from test_gpu_trie_calls import device_labels
    table = rows(NO_M, 3)
    docs = [sized((B_WINS, A_WINS, A_WINS)[i % 3], 200 + i % 57) for i in range(100)]
    lead = (b"qxyzxyzqqxyzqqqxyz")[:17]
    raw = lead + b"".join(docs)
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    off[0] = 17
    off[1:] = 17 + np.cumsum([len(d) for d in docs])
    buf = np.zeros(((len(raw) + 3) & ~3) + 64, dtype=np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    labels, _ = OC.Table(table, 3).score([1, 2, 3], buf, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) == 2

    def dev(m, data, off, labels, kinds):
        got = device_labels(m, data, int(off[-1]), off)
        assert np.array_equal(got, labels), np.nonzero(got != labels)[0][:10].tolist()

    run_all(table, 3, [1, 2, 3], buf, off, labels, monkeypatch, call=dev)
