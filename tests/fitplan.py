"""A host model of FIT v4's emit plan, and the corpora of the many-language
FIT tests (test_fitplan_model.py, test_gpu_fit_many_langs.py).

count_launch_v3 (ldgpu_api.hip, make_plan) cuts a call into batches of at most
batch_recs byte positions and gives every batch its emit workgroups: the
documents of a language, in order, split into ceil(lwin / target) ranges
balanced by records, target = ceil(Wk / share), share = 4 workgroups per CU.
Every language with a non-empty document in the batch keeps at least one
workgroup, so their number grows with the languages present, not with the
CUs; part2_kernel (ldgpu_fit.hip) holds a block prefix over the workgroups of
one of its kSplits groups in LDS.  Whether a corpus puts more than 256
workgroups into a group -- more than 2048 in all, where that prefix once
ended -- depends on the device's CU count, so the tests ask this model.

The model restates the plan in plain Python; its constants are compared with
the headers' by test_fitplan_model.py.
"""
import functools

import numpy as np

from languagedetection import encoding

# the plan's constants, named once (ldgpu_fit.h, ldgpu_api.hip, include/ldgpu.h)
SPLITS = 8                 # kSplits: emit workgroup groups; the count is padded to a multiple
MAX_EMIT_WG = 8192         # kMaxEmitWg: most emit workgroups of a batch
WG_PER_CU = 4              # the plan's share of workgroups for splitting: 4 per CU
BATCH_RECORDS = 1 << 29    # kBatchRecords: byte positions per batch of one-word records (/ K for wider ones)
MAX_LANGS = 4096           # LDGPU_MAX_LANGS
MAX_GRAM = 7               # kMaxGram: the longest gram of a one- or two-word record
OLD_EDGE = 2048            # 8 groups of 256 workgroups: the prefix array's former end


# ------------------------------------------------------------------ the model
def batches(off, batch_recs=None):
    """[(d0, d1)]: a batch takes documents while their bytes stay within
    batch_recs (labels and empty documents do not matter here), one at least."""
    if batch_recs is None:
        batch_recs = BATCH_RECORDS
    n = len(off) - 1
    out = []
    d0 = 0
    while True:
        d1, W = d0, 0
        while d1 < n:
            ln = int(off[d1 + 1]) - int(off[d1])
            if d1 > d0 and W + ln > batch_recs:
                break
            W += ln
            d1 += 1
        out.append((d0, d1))
        if d1 >= n:
            return out
        d0 = d1


def batch_parts(lens, lang, L, cus):
    """Emit workgroups of one batch before padding: lens / lang of its
    documents in order."""
    per_lang = {}
    for ln, l in zip(lens, lang):
        if 0 <= l < L and ln > 0:
            per_lang.setdefault(l, []).append(ln)
    Wk = sum(sum(v) for v in per_lang.values())
    share = min(WG_PER_CU * cus, MAX_EMIT_WG - SPLITS - len(per_lang))
    target = max(1, -(-Wk // share))
    n = 0
    for docs in per_lang.values():
        lwin = sum(docs)
        parts = max(1, -(-lwin // target))
        i = wacc = 0
        for k in range(parts):
            start, goal = i, lwin * (k + 1) // parts
            while i < len(docs) and (wacc < goal or k + 1 == parts):
                wacc += docs[i]
                i += 1
            n += i > start          # a part that got no document is dropped
    return n


def padded(n):
    """Empty workgroups fill the count up to a multiple of kSplits, one group each at least."""
    return max(SPLITS, -(-n // SPLITS) * SPLITS)


def emit_workgroups(off, lang, L, cus, batch_recs=None):
    """The emit workgroups (grid_a) of each batch of a count() call over
    documents off / lang into a table of L languages on a device of `cus`
    CUs.  batch_recs: LDGPU_FIT_BATCH_WINDOWS of the diagnostics library;
    None: the library's own, which no test corpus reaches."""
    lens = np.diff(np.asarray(off, dtype=np.int64)).tolist()
    lang = np.asarray(lang).tolist()
    return [padded(batch_parts(lens[a:b], lang[a:b], L, cus)) for a, b in batches(off, batch_recs)]


def _log2u(p):
    l = 0
    while (1 << l) < p:
        l += 1
    return l


def record_route(L, grams):
    """(K, path) of the product library's count() for a table of L languages
    and gram lengths `grams` (of <= 15 bytes): K words per record
    (counts_new), "v5" where two-word records are counted by sorting
    (sort_path), "v4" -- emit, part2, reduce -- otherwise."""
    maxg = max(grams)
    lb = max(1, _log2u(L))
    cb = 64 - (8 * min(maxg, MAX_GRAM) + 1) - lb
    K = 3 if maxg > MAX_GRAM else (1 if cb >= 8 else 2)
    sort = K == 2 and 8 * maxg + _log2u(L + 1) <= 64
    return K, "v5" if sort else "v4"


# ----------------------------------------------------------------- the corpora
A2 = bytes([0x61, 0xB5])                # 'a' and a byte with the top bit set
A3 = b"ab "
A4 = bytes([0x00, 0x61, 0xC3, 0xFF])    # 0x00, 'a', a UTF-8 lead byte, 0xFF


def corpus(P, alphabet, seed, docs_hi=3, heavy=None):
    """(data, off, lang) with every language of [0, P) present: language l has
    one document of 1..40 bytes and up to docs_hi - 1 more of 0..40 (some
    empty); language P - 1 has a single document of one byte, shorter than
    every gram length but 1 (a partial window).  About 3 % more documents are
    labelled -1.  heavy = (n, size): language 0 also gets n documents of
    `size` bytes each.  Bytes are uniform over `alphabet`; the documents are
    shuffled, so a language's documents are scattered over the call."""
    rng = np.random.default_rng([seed, P])
    abc = np.frombuffer(alphabet, dtype=np.uint8)
    lens, lang = [], []
    extra = rng.integers(0, docs_hi, size=P)
    for l in range(P):
        if l == P - 1:
            lens.append(1)
            lang.append(l)
            continue
        lens.append(int(rng.integers(1, 41)))
        lens += rng.integers(0, 41, size=int(extra[l])).tolist()
        lang += [l] * (1 + int(extra[l]))
    n_skip = max(3, P // 32)
    lens += rng.integers(0, 41, size=n_skip).tolist()
    lang += [-1] * n_skip
    if heavy:
        lens += [heavy[1]] * heavy[0]
        lang += [0] * heavy[0]
    order = rng.permutation(len(lens))
    docs = [bytes(rng.choice(abc, size=lens[i])) for i in order]
    data, off = encoding.pack(docs)
    return data, off, np.asarray(lang, dtype=np.int32)[order]


# name -> (L, P, grams, corpus arguments, K, path, regime at 256 CUs)
# regime: "below" (<= 2048 workgroups), "edge" (exactly 2048), "above"; None: no emit plan (FIT v5)
HEAVY = (2000, 1100)     # language 0: 2.2 MB in equal documents, the 1099 others ~45 KB together
CASES = {
    "1024-balanced": (1024, 1024, [1, 2, 5], dict(alphabet=A3, seed=1), 1, "v4", "below"),
    # one document per language: no language can be split, so 2041 workgroups, padded to 2048, on any device
    "2041-edge": (2048, 2041, [1, 2, 5], dict(alphabet=A3, seed=2, docs_hi=1), 1, "v4", "edge"),
    "2049-balanced": (2049, 2049, [1, 2, 5], dict(alphabet=A3, seed=3), 1, "v4", "above"),
    "4096-dup-length": (4096, 4096, [5, 1, 3, 3], dict(alphabet=A4, seed=4), 1, "v4", "above"),
    "1100-heavy": (1100, 1100, [1, 2, 3], dict(alphabet=A4, seed=5, heavy=HEAVY), 1, "v4", "above"),
    "1100-heavy-wide": (1100, 1100, [2, 9], dict(alphabet=A2, seed=6, heavy=HEAVY), 3, "v4", "above"),
    "4096-two-word": (4096, 4096, [7, 1], dict(alphabet=A2, seed=7), 2, "v4", "above"),
    "300-two-word": (300, 300, [7, 2], dict(alphabet=A3, seed=8), 2, "v4", "below"),
    "4096-sorted": (4096, 4096, [2, 6, 1], dict(alphabet=A3, seed=9), 2, "v5", None),
}


@functools.lru_cache(maxsize=None)
def case_corpus(name):
    """The case's (data, off, lang), made once and shared: do not modify."""
    _, P, _, kw, _, _, _ = CASES[name]
    data, off, lang = corpus(P, **kw)
    for a in (data, off, lang):
        a.setflags(write=False)
    return data, off, lang


def regime_of(grid):
    """"below", "edge" or "above" the 2048 workgroups at which a group of
    part2 holds more than 256 of them."""
    return "below" if grid < OLD_EDGE else ("edge" if grid == OLD_EDGE else "above")


def many_batches(name):
    """(data, off, lang, batch_recs) of the several-batches run of a case:
    the case's documents, the same again in reverse order, then its first
    third.  With batches of the corpus's own size the first two hold every
    document of it, the third a third."""
    data, off, lang = case_corpus(name)
    docs = [bytes(data[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    third = len(docs) // 3
    d, o = encoding.pack(docs + docs[::-1] + docs[:third])
    return d, o, np.concatenate([lang, lang[::-1], lang[:third]]), int(off[-1])
