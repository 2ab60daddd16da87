"""GPU parity of the LDS trie's walks in the path-sum and pair forms
(csrc/ldgpu_trie.hip: trie_doc_sum): a walk is counted once, at its deepest live
node, whatever happens to its registers after it died.  The cases were written
for walks that run under per-slot live lane masks (the read of a dead walk not
issued, the entry register written in live lanes only); that build measured
slower and is not in the tree, and the cases hold for the walk as it
is: the dead entry, the maximum over the depths and the depth-4 skip.

Labels must equal the C oracle's exactly, on the product library and on the
diagnostics library under LDGPU_SCORE_GRID=1, LDGPU_NO_TRIE_DOC_PAIRS=1,
LDGPU_NO_TRIE_PAIR=1 (the path-sum form runs the same walk) and LDGPU_NO_TRIE=1
(the control): test_gpu_trie_doc_pairs.run_all.

The table: twelve keys of four languages, grams [1, 2, 3, 4].  "s" and "stuv"
(language 1), "wx" and "wxyz" (2), "mno" and the chain "e" .. "efgh" (3), "q",
"ab" and "abcd" (0): nodes that count without being a key's end ("st", "stu",
"wxy"), prefixes that count nothing ("w", "m", "mn") and W from 1 to 4.

  deepest    for every slot k and two lanes, one walk that is live to depth 1,
             2, 3 or 4 and then dies, the deepest counted key one, two and
             three levels above the death ("s.", "st.", "stu.", "wx.", "wxy.",
             "mno.", "efg.", ...), no count at all ("w.", "mn."), and whole keys;
             beside as many hits of "q" as the walk counts (a tie: language 0)
             and one fewer (the walk's language)
  every 4    every window of four bytes over the keys' 21 bytes (a de Bruijn
             sequence cut into pieces of 24 bytes, one per document, at moving
             slots): whatever the packing of the rows, every mismatch at depth 2
             or 3 that lands on an entry of another row is followed by every
             byte, the children of that row among them -- a stale entry that
             walked on would count
  dead, live a document where no walk is live after depth 2, then one whose
             walks reach depth 4 at the same positions, and back: stale
             registers from one document to the next
  the end    a walk alive up to the last byte of documents of 4, 5, 255 and 256
             bytes, the next document's first byte completing "stuv"

The walk itself is not changed by the step that added this file; of that step's
hand mutations these cases see the ones of the label pass, which
every document's label goes through."""
import functools

import numpy as np
import pytest

from test_gpu_trie import FILL, V
from test_gpu_trie_doc_pairs import run_all
from test_gpu_trie_pair import rows, scored

pytestmark = pytest.mark.gpu

KEYS = {b"s": 1, b"stuv": 1, b"wx": 2, b"wxyz": 2, b"mno": 3, b"e": 3, b"ef": 3, b"efg": 3, b"efgh": 3,
        b"q": 0, b"ab": 0, b"abcd": 0}
NL, GRAMS = 4, [1, 2, 3, 4]
TABLE = rows(KEYS, NL)
# (piece, its language, what its walks count together)
PIECES = [(b"s.", 1, 1), (b"st.", 1, 1), (b"stu.", 1, 1), (b"stuv", 1, 2), (b"w.", 2, 0), (b"wx.", 2, 1), (b"wxy.", 2, 1),
          (b"wxyz", 2, 2), (b"mn.", 3, 0), (b"mno.", 3, 1), (b"e.", 3, 1), (b"ef.", 3, 2), (b"efg.", 3, 3), (b"efgh", 3, 4),
          (b"ab.", 0, 1), (b"abc.", 0, 1)]


def test_the_deepest_live_node_counts(monkeypatch):
    docs, want = [], []
    for piece, lang, c in PIECES:
        for k in range(4):
            for lane, q_at in ((3, 100), (47, 8)):
                for nq in (c, c - 1):
                    if nq < 0:
                        continue
                    d = bytearray([FILL]) * 200
                    at = 4 * lane + k
                    d[at:at + len(piece)] = piece
                    for j in range(nq):
                        d[q_at + 4 * j] = ord("q")
                    docs.append(bytes(d))
                    want.append(0 if nq == c or lang == 0 else lang)
    data, off, labels, _ = scored(TABLE, NL, GRAMS, docs)
    assert labels.tolist() == want and len(np.unique(labels)) == 4
    run_all(TABLE, NL, GRAMS, data, off, labels, monkeypatch)


def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) over 0..k-1 (every word of n letters once, cyclically)."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


@functools.lru_cache(maxsize=None)
def every_window():
    letters = sorted({c for key in KEYS for c in key} | {FILL})
    assert len(letters) == 21
    s = bytes(letters[i] for i in de_bruijn(21, 4))
    s += s[:3]
    assert len(s) == 21 ** 4 + 3
    docs = []
    for i, at in enumerate(range(0, len(s) - 3, 21)):       # 24 bytes = 21 windows a piece, three bytes shared
        d = bytearray([FILL]) * 200
        p = 8 + (i * 7) % 160                               # every slot, lanes 2 .. 41
        d[p:p + 24] = s[at:at + 24]
        docs.append(bytes(d))
    return docs


def test_every_window_of_four_key_bytes(monkeypatch):
    docs = every_window()
    assert len(docs) == 9261
    data, off, labels, _ = scored(TABLE, NL, GRAMS, docs)
    assert np.bincount(labels, minlength=4).min() >= 150     # (every language wins documents: 5160, 1389, 189, 2523)
    run_all(TABLE, NL, GRAMS, data, off, labels, monkeypatch)


def test_dead_and_live_documents_and_the_last_byte(monkeypatch):
    dead = bytes([FILL]) * 256                              # no walk passes depth 1
    live = [(b"stuv" * 65)[j:j + 256] for j in range(4)]    # slot (4 - j) % 4 of every lane reaches depth 4
    docs, want = [], []
    for rep in range(6):
        for y in live:
            docs += [dead, y, y, dead]
            want += [0, 1, 1, 0]
    # "stu" on the last bytes beside one "q" (a tie: language 0); the next document goes on with "v"; and the twin that
    # ends in "stuv" (language 1)
    after = b"v" + bytes([FILL]) * 239
    for n in (4, 5, 255, 256):
        body = bytes([FILL]) * (n - 4) + b"q"
        docs += [body + b"stu", after, (body + b"stuv")[-min(n + 1, 256):], after]
        want += [0, 0, 1, 0]
    docs = docs * 4
    data, off, labels, _ = scored(TABLE, NL, GRAMS, docs)
    assert labels.tolist() == want * 4
    run_all(TABLE, NL, GRAMS, data, off, labels, monkeypatch)
