"""Non-ASCII test corpora: UTF-8 text of many scripts (FIT), the low bytes of
its UTF-16 units (SCORE), and adversarial raw byte documents.

synth is ASCII by design, so the two encodings coincide there and no byte
>= 0x80 -- nor 0x00 -- ever reaches a kernel.  Here every language writes in
one Unicode block: most FIT bytes are >= 0x80 (lead and continuation bytes of
2-, 3- and 4-byte sequences), and the SCORE bytes take every value from 0x00
(U+0100, U+4E00, U+AC00) to 0xFF.  Deterministic from a seed, numpy only.

Also the vectorised top-K rule over oracle counts (_topk_table_from_counts,
_sparse_topk_masks), shared by the CPU and the GPU tests.
"""
import math

import numpy as np

from languagedetection import encoding

# (first code point, code points in the block)
BLOCKS = [
    (0x00C0, 64),     # Latin-1 letters U+00C0-00FF: 2-byte UTF-8, low bytes C0..FF
    (0x0100, 128),    # Latin Extended-A U+0100-017F: low bytes from 0x00
    (0x0391, 57),     # Greek U+0391-03C9
    (0x0410, 64),     # Cyrillic U+0410-044F
    (0x0905, 53),     # Devanagari U+0905-0939: 3-byte UTF-8
    (0x4E00, 256),    # CJK U+4E00-4EFF: low byte 0x00 at U+4E00
    (0xAC00, 256),    # Hangul U+AC00-ACFF: low byte 0x00 at U+AC00
    (0x1F600, 80),    # emoticons U+1F600-1F64F: surrogate pairs, 4-byte UTF-8
    (0x0061, 26),     # a-z
]
SHARED = [0x20, 0x2E, 0x37]      # space, '.', '7': in every language
RARE = [0x0000, 0x00FF]          # in every language, at _RARE_P each
_RARE_P = 0.004


def _languages(seed, L):
    """Per language: (code points, weights).  Its own 20-30 code points of
    block l mod len(BLOCKS) -- the block's first code point always among them
    (xx00 in the blocks that have one) --, the shared ASCII and the rare
    U+0000 / U+00FF; weights ~ Dirichlet(0.3) as synth's transition rows, so
    a few units carry most of the text and grams repeat."""
    rng = np.random.default_rng([seed, 0])
    out = []
    for l in range(L):
        first, size = BLOCKS[l % len(BLOCKS)]
        m = min(int(rng.integers(20, 31)), size)
        own = first + np.concatenate([[0], 1 + rng.choice(size - 1, size=m - 1, replace=False)])
        cps = np.concatenate([own, SHARED, RARE]).astype(np.int64)
        w = rng.dirichlet(np.full(len(own) + len(SHARED), 0.3)) * (1.0 - _RARE_P * len(RARE))
        out.append((cps, np.concatenate([w, np.full(len(RARE), _RARE_P)])))
    return out


def texts(seed, L, n_docs, len_lo, len_hi):
    """(labels int32 [n_docs], list of str): document i is U[len_lo, len_hi]
    units drawn from language labels[i]'s weights (a unit is one code point;
    an astral one is two UTF-16 units).  The languages depend on (seed, L)
    only, so corpora of one seed share their grams whatever their size."""
    langs = _languages(seed, L)
    rng = np.random.default_rng([seed, 1])
    labels = rng.integers(0, L, size=n_docs).astype(np.int32)
    lens = rng.integers(len_lo, len_hi + 1, size=n_docs)
    out = []
    for l, n in zip(labels.tolist(), lens.tolist()):
        cps, w = langs[l]
        out.append("".join(map(chr, rng.choice(cps, size=n, p=w).tolist())))
    return labels, out


def fit_pack(txts):
    """(data, offsets) of the FIT encoding (UTF-8), through the project's encoding module."""
    return encoding.pack_fit(txts)


def score_pack(txts):
    """(data, offsets) of the SCORE encoding (low byte of each UTF-16 unit)."""
    return encoding.pack_score(txts)


EDGE_LENGTHS = [1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def raw_docs(seed):
    """Adversarial documents for the byte-level APIs: runs of 0x00 and of 0xFF
    at every length around a window, a dword, a wave and a superblock;
    alternating 00/FF and 7F/80 (the sign bit); documents that differ only in
    trailing zeros; two all-zero documents side by side and around an empty
    one; uniformly random documents of 0-300 bytes."""
    rng = np.random.default_rng([seed, 2])
    docs = []
    for n in EDGE_LENGTHS:
        docs += [b"\x00" * n, b"\xff" * n]
    docs += [b"\x00\xff" * 40, b"\xff\x00" * 33 + b"\xff", b"\x7f\x80" * 40, b"\x80\x7f" * 33 + b"\x80"]
    docs += [b"ab", b"ab\x00", b"ab\x00\x00"]
    docs += [b"\x00" * 40, b"\x00" * 40, b"", b"\x00" * 24]
    docs += [bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8)) for n in rng.integers(0, 301, size=300)]
    return docs


FIXED_KEYS = [b"\x00", b"\x00\x00", b"a\x00", b"\x00a", b"\xff", b"\xff\xff\xff", b"\x7f\x80"]


def cut_keys(rng, data, off, lens, count):
    """`count` draws of windows of the documents, lengths from `lens` (a
    document shorter than the drawn length is skipped): keys that are hit."""
    d = rng.integers(0, len(off) - 1, size=count)
    n = rng.choice(np.asarray(lens), size=count)
    ln = off[d + 1] - off[d]
    ok = ln >= n
    d, n, ln = d[ok], n[ok], ln[ok]
    p = off[d] + (rng.random(len(d)) * (ln - n + 1)).astype(np.int64)
    return [bytes(data[a:a + k]) for a, k in zip(p.tolist(), n.tolist())]


def byte_table(seed, L, lens, n_keys, form, source=None):
    """A SCORE table {key: row of L} in `form`: "mask" (log(1 + 1/k) at k
    random languages), "dense" (normal draws) or "uniform" (one shared value
    at random languages: count mode).  About n_keys keys of the lengths in
    `lens`, cut from `source` = (data, offsets) -- by default the score bytes
    of texts(seed, L, 400, 0, 120) and raw_docs(seed) -- so that documents of
    the same seed hit them; plus FIXED_KEYS and, for each length n >= 8, the
    all-zero and the all-0xFF key."""
    rng = np.random.default_rng([seed, 3])
    if source is None:
        _, tx = texts(seed, L, 400, 0, 120)
        source = encoding.pack([encoding.score_bytes(t) for t in tx] + raw_docs(seed))
    keys = list(dict.fromkeys(cut_keys(rng, source[0], source[1], lens, n_keys)))
    keys += [k for k in FIXED_KEYS if k not in keys]
    for n in lens:
        if n >= 8:
            keys += [k for k in (b"\x00" * n, b"\xff" * n) if k not in keys]
    table = {}
    for k in keys:
        if form == "dense":
            table[k] = rng.normal(size=L).tolist()
            continue
        m = rng.random(L) < rng.uniform(0.02, 0.6)
        if not m.any():
            m[int(rng.integers(0, L))] = True
        v = math.log(2.0) if form == "uniform" else math.log(1.0 + 1.0 / int(m.sum()))
        table[k] = [v if b else 0.0 for b in m]
    return table


def interleave(a, b):
    """a[0], b[0], a[1], b[1], ... then the rest of the longer list."""
    out = []
    for i in range(max(len(a), len(b))):
        out += a[i:i + 1] + b[i:i + 1]
    return out


# ------------------------------------------------------------------ top-K rule
def _class_values(L):
    """v[k] = log(1 + 1 / k) for k = 1..L, v[0] = 0, by the oracle's own
    formula (math.log: the C library's).  numpy's vectorised log is another
    implementation: it differs from it in the last bit at k = 20, 59, 62, ..."""
    return np.array([0.0] + [math.log(1.0 + 1.0 / k) for k in range(1, L + 1)])


def _topk_table_from_counts(keys, cnt, L, K):
    """filterTopGrams (LanguageDetector.scala:100-132) over oracle counts,
    vectorised: v_l = log(1 + [l] / k); per language the K largest v_l, ties
    by ascending (length, bytes) = index order of the sorted keys."""
    pres = cnt > 0
    k = pres.sum(axis=1)
    w = _class_values(L)[k]
    chosen = np.zeros(len(keys), dtype=bool)
    idx = np.arange(len(keys))
    for l in range(L):
        v = np.where(pres[:, l], w, 0.0)
        order = np.lexsort((idx, -v))
        chosen[order[:K]] = True
    return {keys[i]: [float(w[i]) if pres[i, l] else 0.0 for l in range(L)] for i in np.nonzero(chosen)[0]}


def _sparse_topk_masks(expect, L, K):
    """filterTopGrams over the oracle's sparse counts (kb, ko, po, pl, pc in
    (length, bytes, language) order): every gram in some language's top K by
    (v_l desc, index asc), as (keys, mask words [n][ceil(L/64)], values)."""
    kb, ko, po, pl, pc = expect
    n = len(ko) - 1
    k = np.diff(po)
    w = _class_values(L)[k]
    g = np.repeat(np.arange(n), k)
    order = np.lexsort((g, -w[g], pl))
    sl = pl[order]
    chosen = np.zeros(n, dtype=bool)
    starts = np.searchsorted(sl, np.arange(L + 1))
    for l in range(L):
        chosen[g[order[starts[l]:min(starts[l + 1], starts[l] + K)]]] = True
    idx = np.nonzero(chosen)[0]
    b = kb.tobytes()
    keys = [b[ko[i]:ko[i + 1]] for i in idx]
    words = (L + 63) // 64
    masks = np.zeros((len(idx), words), dtype=np.uint64)
    for j, i in enumerate(idx):
        for l in pl[po[i]:po[i + 1]]:
            masks[j, l // 64] |= np.uint64(1) << np.uint64(l % 64)
    return keys, masks, w[idx]


def cut_splits_sign_group(keys, cnt, K):
    """The languages whose K-th gram falls strictly inside a group of equal
    (value, length) that holds keys with a first byte below 0x80 AND keys with
    one at or above it: there a signed byte compare, or a sort that drops the
    top bit, chooses other grams than (length, unsigned bytes) does.  `keys` in
    (length, bytes) order, cnt [n, L]."""
    return [l for l, s in enumerate(_split_cuts(keys, cnt)) if 0 < K <= len(s) and s[K - 1]]


def _split_cuts(keys, cnt):
    """Per language a bool array s: s[K - 1] = a cut after its K-th gram lies
    strictly inside a mixed-sign (value, length) group."""
    pres = cnt > 0
    k = pres.sum(axis=1)
    klen = np.fromiter((len(g) for g in keys), dtype=np.int64, count=len(keys))
    high = np.fromiter((g[0] >= 0x80 for g in keys), dtype=bool, count=len(keys))
    out = []
    for l in range(cnt.shape[1]):
        idx = np.nonzero(pres[:, l])[0]
        if len(idx) < 2:
            out.append(np.zeros(0, dtype=bool))
            continue
        order = idx[np.lexsort((idx, k[idx]))]            # value desc = k asc, then key order
        same = (k[order][1:] == k[order][:-1]) & (klen[order][1:] == klen[order][:-1])
        gid = np.concatenate([[0], np.cumsum(~same)])
        n_high = np.bincount(gid, weights=high[order])
        mixed = (n_high > 0) & (n_high < np.bincount(gid))
        out.append(same & mixed[gid[1:]])
    return out


def k_regimes(keys, cnt):
    """The three profile sizes of a corpus, from the oracle's presence matrix:
    (a) below every language's present count, one (the median) of those at which
    the cut splits a mixed-sign group for the most languages; (b) between the
    smallest and the largest present count: some languages take the
    zero-valued fill, others do not; (c) above the number of grams.  Returns
    (Ka, Kb, Kc, languages split at Ka)."""
    present = (cnt > 0).sum(axis=0)
    lo, hi = int(present.min()), int(present.max())
    assert 1 < lo < hi, (lo, hi)
    n_split = np.sum([s[:lo - 1] for s in _split_cuts(keys, cnt)], axis=0)   # K = 1 .. lo - 1
    best = np.nonzero(n_split == n_split.max())[0]
    Ka = int(best[len(best) // 2]) + 1
    return Ka, (lo + hi + 1) // 2, len(keys) + 7, cut_splits_sign_group(keys, cnt, Ka)
