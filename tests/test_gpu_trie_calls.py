"""GPU parity of the LDS-trie kernel (csrc/ldgpu_trie.hip, both forms) on the
calls and values test_gpu_trie and test_gpu_trie_sum do not reach it with: a
negative table value (count_sign < 0: the fewest hits win, the first such
language on a tie), the device-pointer form, the UTF-8 forms, and chunked host
calls whose chunks choose differently between packs and the trie.

The tables are test_gpu_trie's KEYS (plain form) and test_gpu_trie_sum's
KEYS_U (path-sum form), each with V = log 2 and with -0.75.  Expected labels
come from the C oracle on the SCORE bytes, never from the library.  Every case
asserts the layout it means to run on ("trie", and "trie_sum" for KEYS_U), and
runs on the product library, on the diagnostics library with
LDGPU_SCORE_GRID=1 (many documents per wave), on the other form
(LDGPU_NO_TRIE_SUM=1) and, as the control, on the LDS-Bloom path
(LDGPU_NO_TRIE=1).

  negative   test_gpu_trie's corpus under -0.75: 8 distinct labels on KEYS, 280
             of 328 fast documents differ from the positive value's labels and
             181 from a last-minimum rule; KEYS_U with three key-less languages;
             the chain "r" .. "rrrr" (W = 4) against single hits, where a kernel
             that adds 1 for W flips 4 of 6 labels; 70 and 254 languages, with
             every hit in the last counter slice and with every language hit
  device     ldgpu_score_device on torch tensors: n_bytes = 1, 2, 3 modulo 4 with
             the byte that completes a key, then a run of "r", behind the last
             document, which one hit decides (its poison twins: the oracle
             labels it differently with that byte, and with all of them);
             n_bytes beyond offsets[n_docs], the mean on both sides of 192;
             offsets[0] = 3, 16, 17; 0, 1, 2, 11, 12, 13 and 25 documents; two
             calls in flight on two streams
  UTF-8      texts of 1-, 2-, 3- and 4-byte characters whose SCORE bytes are
             KEYS' bytes: ldgpu_score_utf8 (labels; scores as the control), in
             chunks of 5, ldgpu_score_utf8_device in chunks of 7; a corpus only
             the UTF-8 mean sends to the trie; ill-formed documents; decoded
             bytes a previous call left behind the last document
  chunks     ldgpu_score in chunks of 8 documents that alternate between the
             trie and packs

Stale decoded bytes (test_utf8_stale_decoded_bytes): on the GPU the mutation
that lets the last document's windows run past its end fails that test, so the
stage's decode buffer does keep the previous call's bytes behind the decoded
end; only the tail cut keeps them out of the count.

Hand mutations of ldgpu_trie.hip, each built once and not committed: see
DESIGN.md for the cases that fail."""
import functools

import numpy as np
import pytest

import ldoracle_c as OC
import utf8corpus
from languagedetection import encoding, utf8
from languagedetection.runtime import DeviceModel
from test_gpu_trie import FILL, KEY_OF, KEYS, L, RUN, V, check_labels, corpus, soup
from test_gpu_trie_sum import KEYS_U, favoured_soup, path_nodes, run_forms, table_of

pytestmark = pytest.mark.gpu

NEG = -0.75
# KEYS_U's languages that own keys (1: the chain "r" .. "rrrr", 0x00 and "wxyz",
# 3: "q" and its chain, 2: 0xff and "mnop", 7: "mnoq", 0: "xyz") as languages 0..4
LANG_U = {1: 0, 3: 1, 2: 2, 7: 3, 0: 4}
# (keys, value, languages, a key's language, the path-sum form).  Under the
# negative value KEYS_U has its five languages that own keys and no other: with
# a key-less language in the table, that one has the fewest hits always.
CONFIGS = {"plain+": (KEYS, V, L, None, False), "plain-": (KEYS, NEG, L, None, False),
           "sum+": (KEYS_U, V, L, None, True), "sum-": (KEYS_U, NEG, 5, LANG_U.get, True)}
GRAMS = [1, 2, 3, 4]
# the last document of the UTF-8 corpora ends in these bytes and "xy"
LAST = b"qabc.xyz.mnoq.mnop.xyz.xyz.xyz."


def valued(table, v):
    """The table with `v` in place of its one value."""
    return {k: [v if x else 0.0 for x in row] for k, row in table.items()}


def config(name):
    """(table, languages, the path-sum form)"""
    keys, v, nl, lang, has_sum = CONFIGS[name]
    return valued(table_of(keys, nl, lang or (lambda l: l)), v), nl, has_sum


def text_bytes(rng, n, i):
    """Document i of n bytes: test_gpu_trie's soup, or test_gpu_trie_sum's, which favours one language."""
    return soup(rng, n) if i % 2 else favoured_soup(rng, n)


def want(table, nl, grams, data, off, scores=False):
    return OC.Table(table, nl).score(list(grams), data, off, want_scores=scores, nthreads=8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, labels, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(labels))[0]
    assert not len(bad), (what, [(int(i), int(got[i]), int(labels[i])) for i in bad[:10]])


def each_model(table, nl, grams, has_sum, monkeypatch):
    """(name, model): the product library; the diagnostics library with
    LDGPU_SCORE_GRID=1; a path-sum table in the other form; the LDS-Bloom path."""
    def made(variant, trie=True, trie_sum=has_sum):
        m = DeviceModel(table, nl, grams, variant=variant)
        lay = m.info()["layout"]
        assert ("trie" in lay) == trie and ("trie_sum" in lay) == (trie and trie_sum), m.info()
        return m

    m = made("product")
    yield "product", m
    m.close()
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    m = made("diag")
    yield "diag, one workgroup", m
    m.close()
    if has_sum:
        monkeypatch.setenv("LDGPU_NO_TRIE_SUM", "1")
        m = made("diag", trie_sum=False)
        yield "diag, the other form", m
        m.close()
        monkeypatch.delenv("LDGPU_NO_TRIE_SUM")
    monkeypatch.setenv("LDGPU_NO_TRIE", "1")
    m = made("diag", trie=False)
    yield "diag, no trie", m
    m.close()
    monkeypatch.delenv("LDGPU_NO_TRIE")
    monkeypatch.delenv("LDGPU_SCORE_GRID")


def run_control(table, nl, grams, data, off, labels, kinds, monkeypatch):
    """The host call on the LDS-Bloom path (LDGPU_NO_TRIE=1): the control of a case that run_forms ran."""
    monkeypatch.setenv("LDGPU_NO_TRIE", "1")
    d = DeviceModel(table, nl, grams, variant="diag")
    assert "trie" not in d.info()["layout"], d.info()
    check_labels(d, data, off, labels, kinds)
    d.close()
    monkeypatch.delenv("LDGPU_NO_TRIE")


# ---------------------------------------------------------------- A. negative
def counts_of(scores, v):
    return np.rint(np.asarray(scores) / v).astype(np.int64)


def corpus_table(keys_name):
    """The table test_gpu_trie's corpus is scored with under the negative value
    (with V: valued() puts -0.75 in): KEYS, or KEYS_U numbered by LANG_U."""
    keys, lang = {"KEYS": (KEYS, lambda l: l), "KEYS_U": (KEYS_U, LANG_U.get)}[keys_name]
    return table_of(keys, L, lang)


@functools.lru_cache(maxsize=None)
def negative_case(keys_name, grams):
    """(labels under -0.75, labels under V, the counts) of test_gpu_trie's corpus, from the oracle."""
    docs, kinds, data, off = corpus(max(grams))
    nl = L
    t = corpus_table(keys_name)
    neg, sc = want(valued(t, NEG), nl, grams, data, off, scores=True)
    pos, _ = want(t, nl, grams, data, off)
    for a in (neg, pos, sc):
        a.setflags(write=False)
    return neg, pos, counts_of(sc, NEG)


def check_negative_corpus(keys_name, grams, distinct):
    """Host-side: the negative value's labels discriminate on the fast documents.
    (KEYS_U: the last language owns no key, so the last minimum is language 7
    always and that figure says nothing; it is asked of KEYS alone.)"""
    docs, kinds, data, off = corpus(max(grams))
    neg, pos, cnt = negative_case(keys_name, tuple(grams))
    fast = np.array([i for i, d in enumerate(docs) if max(grams) <= len(d) <= 256])
    assert len(fast) >= 320
    assert np.array_equal(neg, cnt.argmin(axis=1))         # the fewest hits, the first such language
    last_min = L - 1 - cnt[:, ::-1].argmin(axis=1)
    figures = (len(np.unique(neg[fast])), int((neg[fast] != pos[fast]).sum()), int((neg[fast] != last_min[fast]).sum()))
    assert figures[0] >= distinct and 2 * figures[1] >= len(fast) and (figures[2] >= 50 or keys_name != "KEYS"), figures
    empty = [i for i, k in enumerate(kinds) if k == "empty"]
    assert empty and not cnt[empty].any() and not neg[empty].any()   # no hit: label 0
    return figures


@pytest.mark.parametrize("grams", [[1, 2, 3, 4], [2, 4]], ids=str)
def test_negative_value_plain_form(grams, monkeypatch):
    figures = check_negative_corpus("KEYS", grams, distinct=5)
    if grams == [1, 2, 3, 4]:
        assert figures == (8, 280, 181), figures
    docs, kinds, data, off = corpus(max(grams))
    labels = negative_case("KEYS", tuple(grams))[0]
    table = valued(corpus_table("KEYS"), NEG)
    run_forms(table, L, grams, data, off, labels, kinds, has_sum=False, monkeypatch=monkeypatch, grids=("1",))
    run_control(table, L, grams, data, off, labels, kinds, monkeypatch)


@pytest.mark.parametrize("grams", [[1, 2, 3, 4], [2, 4], [1, 2, 3, 4, 4, 4]], ids=str)
def test_negative_value_path_sum_form(grams, monkeypatch):
    """KEYS_U's five languages that own keys as languages 0..4 (LANG_U), and three
    that own none (L = 8): a document's label is the first language without a
    hit, 5 at the most.  (As KEYS_U numbers them, language 0 owns "xyz" alone
    and wins every document under [2, 4]; with more key-less languages behind
    the labels are the same.)  [1, 2, 3, 4, 4, 4] has W = 6: the plain form."""
    nl = L
    check_negative_corpus("KEYS_U", grams, distinct=4)
    docs, kinds, data, off = corpus(max(grams))
    labels = negative_case("KEYS_U", tuple(grams))[0]
    assert labels.max() <= 5
    table = valued(corpus_table("KEYS_U"), NEG)
    has_sum = grams != [1, 2, 3, 4, 4, 4]
    run_forms(table, nl, grams, data, off, labels, kinds, has_sum=has_sum, monkeypatch=monkeypatch, grids=("1",))
    run_control(table, nl, grams, data, off, labels, kinds, monkeypatch)


def sum_counts(nodes, doc, nl, w_one=False):
    """The path-sum form's counts of one document: per position the deepest
    node reached inside it, counted once with its W (w_one: with 1)."""
    cnt = [0] * nl
    for p in range(len(doc)):
        best = None
        for d in range(1, min(4, len(doc) - p) + 1):
            if doc[p:p + d] not in nodes:
                break
            best = nodes[doc[p:p + d]] or best
        if best:
            cnt[best[0]] += 1 if w_one else best[1]
    return cnt


def test_negative_value_weights(monkeypatch):
    """Two languages, both with hits in every document, so the weight decides
    the minimum: "rrrr" counts 10 for language 1 (its nodes' W = 1, 2, 3, 4),
    against 9, 10 and 11 single "q" for language 0 (every other key of KEYS_U).
    Fewest hits win: language 0 with 9 and with 10 (the tie), language 1 with
    11.  A kernel that adds 1 for W gives language 1 four hits: label 1 always."""
    def lang(l):
        return int(l == 1)

    docs = []
    for at_end in (False, True):
        for n in (9, 10, 11):
            d = bytearray([FILL]) * 240
            for j in range(n):
                d[8 + 3 * j] = ord("q")
            at = 236 if at_end else 100
            d[at:at + 4] = bytes([RUN]) * 4
            docs += [bytes(d), (bytes([RUN]) * 2 if at_end else b"q") + bytes([FILL]) * 230]
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0
    table = valued(table_of(KEYS_U, 2, lang), NEG)
    labels, scores = want(table, 2, GRAMS, data, off, scores=True)
    cnt = counts_of(scores, NEG)
    assert cnt[0::2].tolist() == [[9, 10], [10, 10], [11, 10]] * 2 and labels[0::2].tolist() == [0, 0, 1] * 2
    assert labels[1::2].tolist() == [1, 1, 1, 0, 0, 0]    # the following document: one "q", or "rr" = 3
    # the rule restated, and its mutation W -> 1
    nodes = path_nodes({k: lang(l) for k, l in KEYS_U.items()}, GRAMS)
    rule = [sum_counts(nodes, d, 2) for d in docs]
    assert rule == cnt.tolist()
    flipped = [i for i, d in enumerate(docs) if int(np.argmin(sum_counts(nodes, d, 2, w_one=True))) != labels[i]]
    assert len(flipped) >= 1 and flipped == [0, 2, 6, 8], flipped
    run_forms(table, 2, GRAMS, data, off, labels, monkeypatch=monkeypatch, grids=("1",))
    run_control(table, 2, GRAMS, data, off, labels, None, monkeypatch)


@pytest.mark.parametrize("nl", [70, 254])
def test_negative_value_many_languages(nl, monkeypatch):
    """test_many_languages' mapping (KEYS' language l becomes nl - 1 - l) under
    -0.75: two and four counter slices.  Every hit is counted in the last slice,
    the languages below own no key, so language 0 wins every document on the
    tie-break byte 255 - l; the positive value's labels lie in the last slice."""
    docs, kinds, data, off = corpus(4)
    table = table_of(KEYS, nl, lambda l: nl - 1 - l)
    pos, _ = want(table, nl, GRAMS, data, off)
    table = valued(table, NEG)
    labels, _ = want(table, nl, GRAMS, data, off)
    assert not labels.any() and (pos >= 64 * ((nl - 1) // 64)).sum() >= 200
    for name, m in each_model(table, nl, GRAMS, False, monkeypatch):
        check_labels(m, data, off, labels, kinds)


@pytest.mark.parametrize("nl", [70, 254])
def test_negative_value_every_language_hit(nl, monkeypatch):
    """... and a table of its own with a hit for every language in every
    document, so that the minimum is decided inside the slices: language l owns
    the byte l, and every third byte pair (l, l + 1) is a key of language l + 7.
    A document is every byte below nl in random order (three times over with
    70 languages), in two of three documents with one byte taken out -- its
    language has the fewest hits --, in every second one with two bytes added."""
    rng = np.random.default_rng(nl)
    keys = {bytes([l]): l for l in range(nl)}
    keys.update({bytes([l, (l + 1) % nl]): (l + 7) % nl for l in range(0, nl, 3)})
    table = valued(table_of(keys, nl), NEG)
    docs = []
    for i in range(60):
        d = np.concatenate([rng.permutation(nl) for _ in range(1 if nl == 254 else 3)])
        if i % 3:                  # (the languages taken out: nl - 2, nl - 5, ... and 10, 25, ...)
            d = np.delete(d, np.flatnonzero(d == ((nl - 1 - i) if i % 3 == 1 else 5 * i) % nl)[0])
        if i % 2 == 0:
            d = np.append(d, rng.integers(0, nl, size=2))
        docs.append(d.astype(np.uint8).tobytes())
    data, off = encoding.pack(docs)
    assert off[-1] / len(docs) >= 192.0 and max(len(d) for d in docs) <= 256
    labels, scores = want(table, nl, GRAMS, data, off, scores=True)
    cnt = counts_of(scores, NEG)
    assert cnt[0::3].min() >= 1 and cnt.sum(axis=1).min() >= nl - 1     # nothing taken out: every language is hit
    top = 64 * ((nl - 1) // 64)
    assert len(np.unique(labels)) >= 25 and (labels >= top).sum() >= 2 and (labels < 64).sum() >= 5, np.unique(labels)
    for name, m in each_model(table, nl, GRAMS, False, monkeypatch):
        check_labels(m, data, off, labels)


# ------------------------------------------------------------------ B. device
@functools.lru_cache(maxsize=None)
def last_document(name, n, length):
    """A document of `length` bytes that ends in KEY_OF[n] without its last byte
    and that one hit decides: under the configuration `name` the oracle gives
    it another label with the key's last byte behind it, and with that byte
    and 64 times "r".  The first such among the documents of "." with up to two
    keys of KEYS in front."""
    table, nl, _ = config(name)
    tail, more = KEY_OF[n][:-1], KEY_OF[n][-1:]
    pieces = [b""] + sorted(KEYS)
    docs = []
    for front in (a + b"." + b + b"." for a in pieces for b in pieces):
        d = front + bytes([FILL]) * (length - len(front) - len(tail)) + tail
        docs += [d, d + more, d + more + bytes([RUN]) * 64]
    data, off = encoding.pack(docs)
    lab = want(table, nl, GRAMS, data, off)[0].reshape(-1, 3)
    found = np.flatnonzero((lab[:, 0] != lab[:, 1]) & (lab[:, 0] != lab[:, 2]))
    assert len(found), (name, n)
    return docs[3 * int(found[0])]


@functools.lru_cache(maxsize=None)
def end_corpus(name, n, rem, pre=0, lo=200, hi=256, slack=64):
    """(buf, poison, off): 60 documents of soup and last_document(name, n),
    behind `pre` key bytes that belong to no document; off[-1] = rem modulo 4.
    buf is zero beyond off[-1]; poison holds the key's last byte and "r" there."""
    rng = np.random.default_rng(9000 + 400 * n + 100 * rem + pre + hi)
    docs = [text_bytes(rng, int(x), i) for i, x in enumerate(rng.integers(lo, hi + 1, size=60))]
    body = sum(len(d) for d in docs)
    k = 200 + (rem - (pre + body + 200)) % 4
    docs.append(last_document(name, n, k))
    raw = (b"qabcwxyzmnoprrrrab" * 2)[:pre] + b"".join(docs)
    end = len(raw)
    assert end % 4 == rem
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    off[0] = pre
    off[1:] = pre + np.cumsum([len(d) for d in docs])
    buf = np.zeros(((end + 3) & ~3) + slack, dtype=np.uint8)
    buf[:end] = np.frombuffer(raw, dtype=np.uint8)
    poison = buf.copy()
    poison[end] = KEY_OF[n][-1]
    poison[end + 1:] = RUN
    for a in (buf, poison, off):
        a.setflags(write=False)
    return buf, poison, off


def poison_twin(table, nl, buf, poison, off):
    """The oracle's labels of the zero-padded buffer; with the poison in place
    of the zeros, and one byte or all of it counted to the last document, its
    last label differs."""
    labels, _ = want(table, nl, GRAMS, buf, off)
    for end in (int(off[-1]) + 1, len(poison)):
        off2 = off.copy()
        off2[-1] = end
        twin, _ = want(table, nl, GRAMS, poison, off2)
        assert np.array_equal(twin[:-1], labels[:-1]) and twin[-1] != labels[-1], (int(twin[-1]), int(labels[-1]))
    return labels


def device_labels(m, buf, n_bytes, off, n_docs=None, stream=None, sync=True):
    """ldgpu_score_device on torch tensors; the labels prefilled with -7."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(off) - 1 if n_docs is None else n_docs
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        d_bytes = torch.from_numpy(np.array(buf)).to(dev)
        d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
        d_lab = torch.full((len(off),), -7, dtype=torch.int32, device=dev)
        m.score_device(d_bytes.data_ptr(), int(n_bytes), d_off.data_ptr(), n, d_lab.data_ptr(), stream=s.cuda_stream)
    if not sync:
        return d_bytes, d_off, d_lab
    s.synchronize()
    got = d_lab.cpu().numpy()
    assert (got[n:] == -7).all()          # nothing written behind the call's documents
    return got[:n]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_bytes_past_the_end(name, monkeypatch):
    """n_bytes = offsets[n_docs] = 1, 2, 3 (and 0) modulo 4; the caller's bytes
    behind it complete the key the last document ends in.  Then the same
    buffer with its whole length as n_bytes: the staging reads those bytes, and
    the labels are unchanged."""
    table, nl, has_sum = config(name)
    cases = []
    for n, rem in [(n, rem) for n in (2, 3, 4) for rem in (1, 2, 3)] + [(4, 0)]:
        buf, poison, off = end_corpus(name, n, rem)
        assert off[-1] / (len(off) - 1) >= 192.0
        cases.append((n, rem, poison, off, poison_twin(table, nl, buf, poison, off)))
    bad = []      # (every failing case is reported: which ones fail tells a staging bound from a tail cut)
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        for n, rem, poison, off, labels in cases:
            for what, n_bytes in (("n_bytes = offsets[n_docs]", off[-1]), ("n_bytes = the buffer", len(poison))):
                got = device_labels(m, poison, n_bytes, off)
                bad += [(mname, n, rem, what, int(i), int(got[i]), int(labels[i])) for i in np.nonzero(got != labels)[0][:2]]
    assert not bad, "\n".join(str(b) for b in bad)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_n_bytes_decides_the_path(name, monkeypatch):
    """Documents of 150..185 bytes: n_bytes = offsets[n_docs] + 64 keeps the mean
    below 192 (packs), the whole buffer as n_bytes lifts it above (the trie).
    The labels are the same."""
    table, nl, has_sum = config(name)
    buf, poison, off = end_corpus(name, 3, 2, lo=150, hi=185, slack=4096)
    n = len(off) - 1
    labels = poison_twin(table, nl, buf, poison, off)
    assert (int(off[-1]) + 64) / n < 192.0 <= len(poison) / n
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        assert "packs" in m.info()["layout"] or mname == "diag, no trie", m.info()
        same(device_labels(m, poison, int(off[-1]) + 64, off), labels, (mname, "below 192"))
        same(device_labels(m, poison, len(poison), off), labels, (mname, "above 192"))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_offsets_start_inside_the_buffer(name, monkeypatch):
    """offsets[0] = 3, 16 and 17: key bytes in front that belong to no document."""
    table, nl, has_sum = config(name)
    cases = []
    for pre, n, rem in ((3, 2, 1), (16, 3, 3), (17, 4, 2)):
        buf, poison, off = end_corpus(name, n, rem, pre=pre)
        assert off[0] == pre and (off[-1] - off[0]) / (len(off) - 1) >= 192.0
        cases.append((pre, poison, off, poison_twin(table, nl, buf, poison, off)))
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        for pre, poison, off, labels in cases:
            same(device_labels(m, poison, off[-1], off), labels, (mname, pre))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_few_documents(name, monkeypatch):
    """Below, at and above the 12 waves of one workgroup and of two; no document
    at all.  n_bytes = offsets[n_docs]: the next document's bytes follow."""
    table, nl, has_sum = config(name)
    buf, poison, off = end_corpus(name, 4, 1)
    labels, _ = want(table, nl, GRAMS, buf, off)
    assert len(np.unique(labels[:25])) >= 2
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        for n in (0, 1, 2, 11, 12, 13, 25):
            got = device_labels(m, poison, off[n], off[:n + 1], n_docs=n)
            assert len(got) == n and (got != -7).all()       # every entry overwritten
            same(got, labels[:n], (mname, n))


def leftover_corpus(seed):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(200, 257, size=40)]
    for at, n in ((3, 300), (9, 3), (17, 0), (22, 1500), (31, 300), (39, 2)):
        lens[at] = n
    return encoding.pack([text_bytes(rng, n, i) for i, n in enumerate(lens)])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_two_streams(name, monkeypatch):
    """Two calls in flight on two streams of one model, each with leftovers (the
    model's pool, the indirect launch): once per model, no repetition."""
    import torch
    table, nl, has_sum = config(name)
    corpora = [leftover_corpus(seed) for seed in (61, 62)]
    wants = [want(table, nl, GRAMS, data, off)[0] for data, off in corpora]
    assert all(off[-1] / (len(off) - 1) >= 192.0 for _, off in corpora) and not np.array_equal(*wants)
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        streams = [torch.cuda.Stream(torch.device("cuda", 0)) for _ in corpora]
        held = [device_labels(m, data, off[-1], off, stream=s, sync=False) for (data, off), s in zip(corpora, streams)]
        for s in streams:
            s.synchronize()
        for (d_bytes, d_off, d_lab), labels in zip(held, wants):
            same(d_lab.cpu().numpy()[:len(labels)], labels, mname)


# ------------------------------------------------------------------- C. UTF-8
def char_of(b, size):
    """A character of `size` UTF-8 bytes whose UTF-16 unit has the low byte b."""
    return chr(b) if size == 1 and b < 0x80 else chr((0x400 if size <= 2 else 0x4E00) + b)


def text_of(rng, score, p):
    """A text whose SCORE bytes are `score`, of 1-, 2-, 3- and 4-byte characters
    drawn with the probabilities p (a 4-byte character gives two units: two bytes)."""
    out, i = [], 0
    while i < len(score):
        size = 1 + int(rng.choice(4, p=p))
        if size == 4 and i + 1 < len(score):
            # high surrogate 0xD800 + score[i], low surrogate 0xDC00 + (two free bits, score[i + 1])
            out.append(chr(0x10000 + ((score[i] << 10) | (int(rng.integers(4)) << 8) | score[i + 1])))
            i += 2
        else:
            out.append(char_of(score[i], min(size, 3)))
            i += 1
    text = "".join(out)
    assert encoding.score_bytes(text) == bytes(score)
    return text


def utf8_packs(texts):
    data, off = encoding.pack_score(texts)
    udata, uoff = utf8.pack_utf8([t.encode("utf-8") for t in texts])
    return data, off, udata, uoff


@functools.lru_cache(maxsize=None)
def utf8_texts(kind):
    rng = np.random.default_rng({"ascii": 501, "cjk": 502, "mix": 503}[kind])
    if kind == "ascii":
        lens, p = rng.integers(200, 257, size=80), (0.9, 0.05, 0.04, 0.01)
    elif kind == "cjk":
        lens, p = rng.integers(70, 121, size=120), (0.08, 0.05, 0.85, 0.02)
    else:
        lens, p = list(rng.integers(190, 257, size=49)), (0.6, 0.1, 0.25, 0.05)
        for at, n in enumerate((0, 1, 3, 4, 256, 257, 300)):
            lens.insert(7 * at, n)
    scores = [text_bytes(rng, int(n), i) for i, n in enumerate(lens)]
    scores[-1] = scores[-1][:len(scores[-1]) - len(LAST) - 2] + LAST + KEY_OF[3][:-1]
    return tuple(text_of(rng, s, p) for s in scores)


def test_utf8_alphabet_and_means():
    """Host-side: the characters, and which form takes the trie on which corpus."""
    for b in sorted(set(b"".join(KEYS))):
        sizes = [len(char_of(b, s).encode("utf-8")) for s in (1, 2, 3)]
        assert sizes == [1 if b < 0x80 else 2, 2, 3] and all(encoding.score_bytes(char_of(b, s)) == bytes([b]) for s in (1, 2, 3))
    assert char_of(ord("q"), 3) == "乱"
    means = {}
    for kind in ("ascii", "cjk", "mix"):
        texts = utf8_texts(kind)
        data, off, udata, uoff = utf8_packs(texts)
        assert {len(c.encode("utf-8")) for t in texts for c in t} == {1, 2, 3, 4}
        means[kind] = (off[-1] / len(texts), uoff[-1] / len(texts))
    assert means["ascii"][0] >= 192.0 and means["ascii"][1] >= 192.0
    assert means["cjk"][0] < 192.0 <= means["cjk"][1]          # only the UTF-8 form takes the trie
    assert means["mix"][1] >= 192.0
    assert {0, 1, 3, 4, 256, 257, 300} <= {len(encoding.score_bytes(t)) for t in utf8_texts("mix")}


def utf8_device_labels(m, udata, uoff):
    import torch
    dev = torch.device("cuda", 0)
    n = len(uoff) - 1
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        d_data = torch.from_numpy(np.array(udata)).to(dev)
        d_off = torch.from_numpy(np.array(uoff, dtype=np.int64)).to(dev)
        d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
        m.score_utf8_device(d_data.data_ptr(), int(uoff[-1]), d_off.data_ptr(), n, d_lab.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    return d_lab.cpu().numpy()


def utf8_forms(table, nl, has_sum, udata, uoff, labels, scores, monkeypatch):
    """Every UTF-8 form on every library: the host form (labels; scores as the
    control on the other kernel), the diagnostics library in chunks of 5
    documents, the device form (the diagnostics library in chunks of 7)."""
    monkeypatch.setenv("LDGPU_SCORE_CHUNK_DOCS", "5")
    monkeypatch.setenv("LDGPU_UTF8_CHUNK_DOCS", "7")
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        same(m.score_utf8(udata, uoff)[0], labels, (mname, "host form"))
        same(utf8_device_labels(m, udata, uoff), labels, (mname, "device form"))
        if mname == "product":
            got, sc = m.score_utf8(udata, uoff, want_scores=True)
            same(got, labels, (mname, "labels of the scores call"))
            keep = labels >= 0                      # (an ill-formed document: the empty document's row)
            assert np.array_equal(bits(sc[keep]), bits(scores[keep])) and not sc[~keep].any()
    monkeypatch.delenv("LDGPU_SCORE_CHUNK_DOCS")
    monkeypatch.delenv("LDGPU_UTF8_CHUNK_DOCS")
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    m = DeviceModel(table, nl, GRAMS, variant="diag")
    assert "trie" in m.info()["layout"] and ("trie_sum" in m.info()["layout"]) == has_sum, m.info()
    same(m.score_utf8(udata, uoff)[0], labels, "diag, one chunk")
    m.close()


@pytest.mark.parametrize("kind", ["ascii", "cjk", "mix"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_utf8_forms(name, kind, monkeypatch):
    table, nl, has_sum = config(name)
    data, off, udata, uoff = utf8_packs(utf8_texts(kind))
    labels, scores = want(table, nl, GRAMS, data, off, scores=True)
    assert len(np.unique(labels)) >= 3
    utf8_forms(table, nl, has_sum, udata, uoff, labels, scores, monkeypatch)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_utf8_ill_formed_documents(name, monkeypatch):
    """Ill-formed documents first, last and inside a group of fast ones: -1
    there, the neighbours' labels unchanged, nothing else left out."""
    table, nl, has_sum = config(name)
    texts = list(utf8_texts("ascii"))
    good = texts[5].encode("utf-8")
    ill = {0: utf8corpus.VALID_SEQS[1][:2], 30: good[:120] + b"\xc0\x80" + good[120:], 31: good + utf8corpus.VALID_SEQS[2][:3],
           47: b"\xed\xa0\x80", len(texts) - 1: good[:200] + b"\xff"}
    assert all(utf8corpus.codec(d)[0] for d in ill.values())
    docs = [ill.get(i, t.encode("utf-8")) for i, t in enumerate(texts)]
    data, off = encoding.pack_score(["" if i in ill else t for i, t in enumerate(texts)])
    udata, uoff = utf8.pack_utf8(docs)
    assert uoff[-1] / len(docs) >= 192.0
    labels, scores = want(table, nl, GRAMS, data, off, scores=True)
    labels = labels.copy()
    labels[sorted(ill)] = -1
    assert np.flatnonzero(labels < 0).tolist() == sorted(ill)
    utf8_forms(table, nl, has_sum, udata, uoff, labels, scores, monkeypatch)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_utf8_stale_decoded_bytes(name, monkeypatch):
    """Two host calls on one model.  Call 1 decodes, right behind where call 2's
    last document will end, the byte that completes the key that document ends
    in, then a run of "r"; call 2 is call 1's corpus cut there.  Its UTF-8 byte
    count, which the kernel takes as the size of the decoded buffer, reaches far
    beyond its decoded end (3-byte characters)."""
    table, nl, has_sum = config(name)
    rng = np.random.default_rng(77)
    p = (0.08, 0.05, 0.85, 0.02)
    cases = []
    for n in (2, 3, 4):
        scores = [text_bytes(rng, int(x), i) for i, x in enumerate(rng.integers(90, 121, size=30))]
        scores.append(last_document(name, n, 100 + n))
        second = [text_of(rng, s, p) for s in scores]
        stale = KEY_OF[n][-1:] + bytes([RUN]) * 80
        first = second[:-1] + [second[-1] + text_of(rng, stale, p)] + [text_of(rng, soup(rng, 100), p) for _ in range(4)]
        d1, o1, u1, uo1 = utf8_packs(first)
        d2, o2, u2, uo2 = utf8_packs(second)
        end = int(o2[-1])
        assert bytes(d1[:end]) == bytes(d2[:end]) and bytes(d1[end:end + 81]) == stale
        assert uo2[-1] / len(second) >= 192.0 and uo2[-1] >= end + 81      # staged as far as the stale bytes
        l1, _ = want(table, nl, GRAMS, d1, o1)
        l2, _ = want(table, nl, GRAMS, d2, o2)
        for more in (1, 81):                                               # the poison twins
            o3 = o2.copy()
            o3[-1] += more
            twin, _ = want(table, nl, GRAMS, d1, o3)
            assert twin[-1] != l2[-1] and np.array_equal(twin[:-1], l2[:-1])
        cases.append((u1, uo1, l1, u2, uo2, l2))
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        for n, (u1, uo1, l1, u2, uo2, l2) in zip((2, 3, 4), cases):
            same(m.score_utf8(u1, uo1)[0], l1, (mname, n, "call 1"))
            same(m.score_utf8(u2, uo2)[0], l2, (mname, n, "call 2"))


# ------------------------------------------------------------------ D. chunks
@functools.lru_cache(maxsize=None)
def chunk_corpus():
    """Chunks of 8 documents: long ones (the trie) and short ones (packs) in
    turn, two chunks that mix both on either side of the mean of 192, a last
    chunk of one document."""
    rng = np.random.default_rng(808)
    lens = []
    for rep in range(3):
        lens += [int(x) for x in rng.integers(200, 257, size=8)] + [int(x) for x in rng.integers(20, 121, size=8)]
    lens += [250, 60, 250, 250, 60, 250, 250, 250]     # mean 202.5
    lens += [250, 60, 250, 60, 250, 60, 250, 250]      # mean 178.75
    lens += [230]
    docs = [text_bytes(rng, n, i) for i, n in enumerate(lens)]
    data, off = encoding.pack(docs)
    means = [(off[min(i + 8, len(docs))] - off[i]) / (min(i + 8, len(docs)) - i) for i in range(0, len(docs), 8)]
    return data, off, means


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunks_choose_differently(name, monkeypatch):
    table, nl, has_sum = config(name)
    data, off, means = chunk_corpus()
    assert [m >= 192.0 for m in means] == [True, False] * 3 + [True, False, True], means
    labels, _ = want(table, nl, GRAMS, data, off)
    assert len(np.unique(labels)) >= 3
    monkeypatch.setenv("LDGPU_SCORE_CHUNK_DOCS", "8")
    for mname, m in each_model(table, nl, GRAMS, has_sum, monkeypatch):
        assert mname == "diag, no trie" or "packs" in m.info()["layout"], m.info()
        check_labels(m, data, off, labels)          # (the product library: one chunk)
    monkeypatch.delenv("LDGPU_SCORE_CHUNK_DOCS")
    monkeypatch.setenv("LDGPU_SCORE_GRID", "1")
    m = DeviceModel(table, nl, GRAMS, variant="diag")    # one chunk, no switch
    assert "trie" in m.info()["layout"] and ("trie_sum" in m.info()["layout"]) == has_sum, m.info()
    check_labels(m, data, off, labels)
    m.close()
