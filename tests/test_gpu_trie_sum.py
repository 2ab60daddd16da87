"""GPU parity of count mode on the LDS trie's path-sum form
(LDGPU_LAYOUT_TRIE_SUM; csrc/ldgpu_trie.h, csrc/ldgpu_trie.hip): a table whose
root paths each name one language (at most 63 languages) and count at most 4
carries, in every node, the language and the count W of the whole path to it, so
a window position is counted once -- at the deepest node its walk reaches inside
the document -- and not once per key length.

The corpus, the gram lists and the label check are test_gpu_trie's; the table is
KEYS_U: the same keys, each with the language of its shortest prefix that is a
key.  Labels must equal the C oracle's exactly, on the product library and on
the diagnostics library with several documents per wave (LDGPU_SCORE_GRID = 1,
2); LDGPU_NO_TRIE_SUM=1 keeps the other form of these tables covered.

  rule       a Python restatement of the kernel's rule equals the oracle on
             every fast document; three mutations of it flip labels
  grams      test_gpu_trie's lists; [1, 2, 3, 4, 4, 4] has W = 6: the other form
  weights    a run "rrrr" adds 10 to language 1, against 9, 10 (a tie: the first
             maximum) and 11 single hits of language 3; the run on the
             document's last bytes, the next document going on with "r"
  limits     63 languages, language 62 with W = 4 (payload 255); 64 languages
             and a mixed-language path: the other form
  leftovers  calls with none, one, many and only leftovers
  random     3,000 random keys on random text
  benchmark  the 10,000 rows of bench.py's config 2 on its kind of documents"""
import functools
import os

import numpy as np
import pytest

import ldoracle_c as OC
from languagedetection import encoding, synth
from languagedetection.runtime import DeviceModel
from test_gpu_trie import FILL, GRAM_LISTS, KEYS, L, RUN, V, check_labels, corpus, soup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trie_config2_keys.bin")


def shortest_prefix_language(keys):
    """The same keys, each with the language of its shortest prefix that is a key."""
    return {k: next(keys[k[:d]] for d in range(1, len(k) + 1) if k[:d] in keys) for k in keys}


KEYS_U = shortest_prefix_language(KEYS)
SUM_LISTS = [g for g in GRAM_LISTS if g != [1, 2, 3, 4, 4, 4]]


def table_of(keys, nl=L, lang=lambda l: l):
    t = {}
    for k, l in keys.items():
        row = [0.0] * nl
        row[lang(l)] = V
        t[k] = row
    return t


@functools.lru_cache(maxsize=None)
def oracle(grams):
    docs, kinds, data, off = corpus(max(grams))
    return OC.Table(table_of(KEYS_U), L).score(list(grams), data, off, want_scores=True, nthreads=8)


# ------------------------------------------------ the kernel's rule, restated
def path_nodes(keys, grams):
    """{node: (language, W) or None}: W = the sum of the multiplicities of the counted keys on the node's path."""
    mult = {n: list(grams).count(n) for n in range(1, 5)}
    nodes = {}
    for k in keys:
        for d in range(1, len(k) + 1):
            nodes.setdefault(k[:d], None)
    for s in nodes:
        hits = [d for d in range(1, len(s) + 1) if s[:d] in keys and mult[d]]
        assert len({keys[s[:d]] for d in hits}) <= 1, "a path with two languages"
        if hits:
            nodes[s] = (keys[s[:hits[0]]], sum(mult[d] for d in hits))
    return nodes


def rule_label(nodes, raw, b, ln, w_one=False, no_tail=False, no_position=False):
    """The label of the document raw[b : b + ln] by the rule of trie_doc_sum:
    per position the deepest node reached by steps that end inside the document,
    counted once with its W.  Mutations: W replaced by 1; the tail mask dropped
    from the steps (a walk goes on into the following bytes); the per-slot
    position test dropped (cut.in[0] for cut.in[k]: every slot of a lane that
    begins inside the document counts its depth-1 entry)."""
    cnt = [0] * L
    for p in range((ln + 3) & ~3 if no_position else ln):
        s = raw[b + p:b + p + 1]
        if s not in nodes:
            continue
        best = nodes[s]
        for d in range(1, 4):
            if not (no_tail or p + d + 1 <= ln) or s + raw[b + p + d:b + p + d + 1] not in nodes:
                break
            s += raw[b + p + d:b + p + d + 1]
            best = nodes[s] or best
        if best:
            cnt[best[0]] += 1 if w_one else best[1]
    return int(np.argmax(cnt))


def test_table_corpus_and_rule():
    """Host-side: KEYS_U is path-uniform and keeps the corpus' edge cases; the
    restated rule equals the oracle, and each mutation of it flips labels."""
    for k, l in KEYS_U.items():
        assert {KEYS_U[k[:d]] for d in range(1, len(k) + 1) if k[:d] in KEYS_U} == {l}
    assert set(KEYS_U) == set(KEYS) and KEYS_U != KEYS
    for grams in GRAM_LISTS:
        docs, kinds, data, off = corpus(max(grams))
        labels, scores = oracle(tuple(grams))
        assert len(docs) == 412 and 4 <= len(np.unique(labels)) <= 5, (grams, np.unique(labels))
        for i, k in enumerate(kinds):
            # (a key of the document's last bytes counts only under a list with its length)
            if k.startswith("end") and int(k[3:]) in grams:
                assert scores[i].any(), (grams, i, k)
            if k.startswith("poison"):
                assert not scores[i].any(), (grams, i, k)
        raw = bytes(data)
        nodes = path_nodes(KEYS_U, grams)
        fast = [i for i, d in enumerate(docs) if max(grams) <= len(d) <= 256]
        assert len(fast) >= 320
        flips = {}
        for name in (None, "w_one", "no_tail", "no_position"):
            kw = {name: True} if name else {}
            flips[name] = sum(rule_label(nodes, raw, int(off[i]), len(docs[i]), **kw) != labels[i] for i in fast)
        assert flips[None] == 0, (grams, flips)
        if grams == [1, 2, 3, 4]:
            assert not any(not scores[i].any() for i, k in enumerate(kinds) if k.startswith("end"))
            assert (flips["w_one"], flips["no_tail"], flips["no_position"]) == (12, 6, 5), flips


# ------------------------------------------------------------------ GPU cases
def run_forms(table, nl, grams, data, off, labels, kinds=None, has_sum=True, monkeypatch=None, grids=("1", "2")):
    """Product library, diagnostics library with LDGPU_SCORE_GRID, and the other form (LDGPU_NO_TRIE_SUM=1)."""
    m = DeviceModel(table, nl, grams)
    lay = m.info()["layout"]
    assert "trie" in lay and ("trie_sum" in lay) == has_sum, m.info()
    check_labels(m, data, off, labels, kinds)
    m.close()
    if monkeypatch is None:
        return
    for grid in grids:
        monkeypatch.setenv("LDGPU_SCORE_GRID", grid)
        d = DeviceModel(table, nl, grams, variant="diag")
        lay = d.info()["layout"]
        assert "trie" in lay and ("trie_sum" in lay) == has_sum, d.info()
        check_labels(d, data, off, labels, kinds)
        d.close()
    monkeypatch.setenv("LDGPU_NO_TRIE_SUM", "1")
    d = DeviceModel(table, nl, grams, variant="diag")
    lay = d.info()["layout"]
    assert "trie" in lay and "trie_sum" not in lay, d.info()
    check_labels(d, data, off, labels, kinds)
    d.close()
    monkeypatch.delenv("LDGPU_NO_TRIE_SUM")   # (a test may go on to another table)
    monkeypatch.delenv("LDGPU_SCORE_GRID")


@pytest.mark.parametrize("grams", GRAM_LISTS, ids=str)
def test_labels_match_the_oracle(grams, monkeypatch):
    docs, kinds, data, off = corpus(max(grams))
    labels, _ = oracle(tuple(grams))
    # [1, 2, 3, 4, 4, 4]: "rrrr" has W = 1 + 1 + 1 + 3 = 6, so the table keeps the other form
    run_forms(table_of(KEYS_U), L, grams, data, off, labels, kinds, has_sum=grams in SUM_LISTS, monkeypatch=monkeypatch)


def _weight_docs(n, at_end):
    """A document of "." with one "rrrr" (10 for language 1) and n separate "q"
    (1 each for language 3); at_end: the run on the document's last four bytes,
    the next document going on with "r"."""
    d = bytearray([FILL]) * 240
    for j in range(n):
        d[8 + 3 * j] = ord("q")
    if at_end:
        d[-4:] = bytes([RUN]) * 4
        nxt = bytes([RUN]) * 2 + bytes([FILL]) * 230
    else:
        d[100:104] = bytes([RUN]) * 4
        nxt = bytes([FILL]) * 232
    return [bytes(d), nxt]


def test_weights(monkeypatch):
    grams = [1, 2, 3, 4]
    docs, want = [], []
    for at_end in (False, True):
        for n, label in ((9, 1), (10, 1), (11, 3)):
            docs += _weight_docs(n, at_end)
            want += [label, 1 if at_end else 0]   # (the following document: "rr" = 3 for language 1, or no hit)
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0
    table = table_of(KEYS_U)
    labels, scores = OC.Table(table, L).score(grams, data, off, want_scores=True, nthreads=8)
    assert labels.tolist() == want
    for i in range(0, len(docs), 2):
        assert round(scores[i][1] / V) == 10 and round(scores[i][3] / V) == 9 + (i // 2) % 3
    run_forms(table, L, grams, data, off, labels, monkeypatch=monkeypatch)


def test_encoding_limits(monkeypatch):
    grams = [1, 2, 3, 4]
    docs, kinds, data, off = corpus(4)
    with_run = [i for i, d in enumerate(docs) if 4 <= len(d) <= 256 and bytes([RUN]) * 4 in d]
    # KEYS_U's language l as 62 - l: 63 languages have the form (language 62 is "xyz"'s), 64 have not.
    # "r" .. "rrrr" are language 1 of KEYS_U, so the second mapping, l -> (l + 61) % 63, puts the chain
    # at language 62: its last node has W = 4 and payload 255, the largest.
    for nl, lang, has_sum in ((63, lambda l: 62 - l, True), (63, lambda l: (l + 61) % 63, True),
                              (64, lambda l: 62 - l, False)):
        table = table_of(KEYS_U, nl, lang)
        labels, _ = OC.Table(table, nl).score(grams, data, off, want_scores=False, nthreads=8)
        assert len(np.unique(labels)) >= 4 and (labels == 62).sum() >= 5
        if lang(1) == 62:
            assert len(with_run) >= 5 and (labels[with_run] == 62).sum() >= 5
        run_forms(table, nl, grams, data, off, labels, kinds, has_sum=has_sum,
                  monkeypatch=monkeypatch if has_sum else None, grids=("1",))
    # the unmodified KEYS: "qa" (4) below "q" (3) is a mixed path
    table = table_of(KEYS)
    labels, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    run_forms(table, L, grams, data, off, labels, kinds, has_sum=False)


def favoured_soup(rng, n):
    """test_gpu_trie's soup with the keys of one language of KEYS_U drawn three times in four (plain soup of
    KEYS_U is language 1 nearly always: the chain "r" .. "rrrr" alone counts 10)."""
    lang = int(rng.choice(sorted(set(KEYS_U.values()))))
    own = [k for k, l in KEYS_U.items() if l == lang]
    keys = list(KEYS_U)
    d = b""
    while len(d) < n:
        k = own[int(rng.integers(len(own)))] if rng.random() < 0.75 else keys[int(rng.integers(len(keys)))]
        d += k + bytes([FILL]) * int(rng.integers(1, 4))
    return d[:n]


@pytest.mark.parametrize("name", ["none", "one", "many", "only"])
def test_leftovers(name, monkeypatch):
    soup = favoured_soup
    rng = np.random.default_rng(77)
    lens = {"none": [256] * 40,
            "one": [256] * 19 + [300] + [256] * 20,
            "many": [256, 300, 3, 257, 250, 0, 1500, 200] * 6,
            "only": [300] * 30 + [2000] * 5 + [257] * 5}[name]
    docs = [soup(rng, n) for n in lens]
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0
    grams = [1, 2, 3, 4]
    table = table_of(KEYS_U)
    labels, _ = OC.Table(table, L).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) >= 3
    run_forms(table, L, grams, data, off, labels, monkeypatch=monkeypatch, grids=("1",))


def test_random_keys_on_random_text(monkeypatch):
    """3,000 random a-z keys of 2 to 4 bytes, 20 languages (a key's language: that of its shortest key prefix)."""
    rng = np.random.default_rng(3016)
    nl = 20
    keys = {}
    while len(keys) < 3000:
        k = bytes(rng.integers(97, 123, size=int(rng.choice([2, 3, 4], p=[0.01, 0.29, 0.7])), dtype=np.uint8))
        keys.setdefault(k, int(rng.integers(nl)))
    keys = shortest_prefix_language(keys)
    table = table_of(keys, nl)
    docs = [bytes(rng.integers(97, 123, size=int(n), dtype=np.uint8))
            for n in list(rng.integers(200, 257, size=300)) + [3, 0, 257, 1200]]
    data, off = encoding.pack(docs)
    grams = [1, 2, 3, 4]
    labels, _ = OC.Table(table, nl).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) >= 10
    run_forms(table, nl, grams, data, off, labels, monkeypatch=monkeypatch, grids=("1",))


def test_benchmark_table():
    """The 10,000 rows of bench.py's config 2 (L = 20, grams 1..5, one value) on 2,000 documents of 256 bytes."""
    rec = np.fromfile(FIXTURE, dtype=np.uint8).reshape(-1, 6)
    assert len(rec) == 10000
    nl = 20
    table = {}
    for r in rec:
        row = [0.0] * nl
        row[int(r[5])] = V
        table[bytes(r[:int(r[4])])] = row
    assert len(table) == 10000
    data, off, _ = synth.generate(synth.make_languages(nl), 2000, 256, 256, seed=synth.SEED_BASE + 2)
    grams = [1, 2, 3, 4, 5]
    labels, _ = OC.Table(table, nl).score(grams, data, off, want_scores=False, nthreads=8)
    assert len(np.unique(labels)) == nl
    run_forms(table, nl, grams, data, off, labels)
