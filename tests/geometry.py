"""A host model of the SCORE kernel's document geometry, and the corpora and
tables of the geometry tests (test_geometry_model.py, test_gpu_geometry.py).

score_kernel (ldgpu_score.hip) gives each wave a contiguous range of
documents and walks it in groups: as many documents as fit 1024 staged bytes
from a 16-byte-aligned start, 63 at the most; inside a staged group the count
kernels score consecutive short documents in packs of up to four.  Which
documents share a wave, a group or a pack depends on the grid, so a test
corpus reaches these paths only where the model below says it does: a call
with fewer than 12 * CUs * wg_per_cu documents gives every wave one document,
and none of this code runs.  The GPU tests therefore go through tile() (the
product library, enough documents for several per wave) or through the
diagnostics library's LDGPU_SCORE_GRID (a grid of one or two workgroups).

The model restates the kernel's rules in plain Python; its constants are
compared with the headers' by test_geometry_model.py.
"""
import bisect
import functools
import math
from types import SimpleNamespace

import numpy as np

# the kernel's constants, named once (ldgpu_internal.h, ldgpu_general.hip, ldgpu_api.hip)
SCORE_WAVES = 12       # kScoreWaves: waves per workgroup
GROUP_DOCS = 63        # ScoreParams.group: documents per group at the most
BUF_BYTES = 1024       # kBufBytes: staged bytes of a group
ALIGN = 16             # a group is staged from its first document's start rounded down to this
PACK_DOCS = 4          # kPackDocs
PACK_DOC_MAX = 128     # a pack starts at a document of maxg..128 bytes
SUPERBLOCK = 256       # 64 * kSub: a pack's bytes, and the fast path's longest document
GEN_BUF = 4096         # kGenBuf: the general-key kernel stages documents up to this length

POSITIONS = (0, 63, 64, 191, 192, 255, 256, 1023, 1024)


# ------------------------------------------------------------------ the model
def wave_ranges(n_docs, n_waves):
    """[(lo, hi)] of wave 0 .. n_waves - 1: documents [n_docs w / n_waves, n_docs (w + 1) / n_waves)."""
    return [(n_docs * w // n_waves, n_docs * (w + 1) // n_waves) for w in range(n_waves)]


def product_waves(n_docs, cus, wg_per_cu):
    """Waves of the product library's grid (score_grid, ldgpu_api.hip)."""
    return SCORE_WAVES * max(1, min(-(-n_docs // SCORE_WAVES), cus * wg_per_cu))


def groups(off, lo, hi):
    """[(first, count, staged)] of a wave's range [lo, hi).  `off` is a list
    (or array) of the n_docs + 1 offsets."""
    out = []
    g0 = lo
    while g0 < hi:
        s0 = int(off[g0]) & ~(ALIGN - 1)
        lim = min(GROUP_DOCS, hi - g0)
        count = max(1, bisect.bisect_right(off, s0 + BUF_BYTES, g0 + 1, g0 + lim + 1) - (g0 + 1))
        out.append((g0, count, int(off[g0 + count]) - s0 <= BUF_BYTES))
        g0 += count
    return out


def packs(lens, maxg):
    """The walk of a staged group's documents by the pack kernels:
    [(first, count, stop, refused)] with first an index into `lens` (the
    group's document lengths).  count >= 2 is a pack; count == 1 a document
    scored alone.  stop says what ended a unit that began as a pack: "full"
    (four documents), "group" (the group's end), "short" (the next document
    shorter than maxg) or "total" (the next document would pass 256 bytes;
    refused = the total it would have made); None for a document that cannot
    begin a pack."""
    out = []
    i, cnt = 0, len(lens)
    while i < cnt:
        nd, stop, refused = 1, None, None
        if maxg <= lens[i] <= PACK_DOC_MAX:
            tot = lens[i]
            while True:
                if nd == PACK_DOCS:
                    stop = "full"
                elif i + nd >= cnt:
                    stop = "group"
                elif lens[i + nd] < maxg:
                    stop = "short"
                elif tot + lens[i + nd] > SUPERBLOCK:
                    stop, refused = "total", tot + lens[i + nd]
                if stop:
                    break
                tot += lens[i + nd]
                nd += 1
        out.append((i, nd, stop, refused))
        i += nd
    return out


def path(length, maxg):
    """score_doc's path of a document scored alone."""
    if length < maxg or length > SUPERBLOCK:
        return "general"
    return "fast-FULL" if length >= 192 + maxg else "fast"


def survey(off, maxg, n_waves, packing=True):
    """What a launch of n_waves waves reaches on the corpus with offsets
    `off`: a namespace of
      group_sizes     {documents in a group}
      whole_range     a group of >= 2 documents ended by its wave's range (lim = hi - g0 binding)
      fills_buffer    a staged group of exactly 1024 bytes from its aligned start
      unstaged        one-document groups scored in place
      pack_sizes      {documents in a pack}, pack_stops {stop}, refused {totals refused}
      pack_ends_at_buffer   a pack whose last document ends at byte 1024 of its group
      nonfirst_paths  {path of a document that is not its group's first, scored alone}
      max_groups      the largest number of groups of one wave
      docs_per_wave   the largest range
      pack_first      per document: the first document of its pack, -1 outside packs
    packing=False: the kernels without packs (every document alone)."""
    off = [int(x) for x in off]
    n = len(off) - 1
    s = SimpleNamespace(group_sizes=set(), whole_range=0, fills_buffer=0, unstaged=0, pack_sizes=set(),
                        pack_stops=set(), refused=set(), pack_ends_at_buffer=0, nonfirst_paths=set(), max_groups=0,
                        docs_per_wave=0, pack_first=np.full(n, -1, dtype=np.int64), staged_multi=0)
    for lo, hi in wave_ranges(n, n_waves):
        if lo >= hi:
            continue
        gs = groups(off, lo, hi)
        s.max_groups = max(s.max_groups, len(gs))
        s.docs_per_wave = max(s.docs_per_wave, hi - lo)
        for g0, cnt, staged in gs:
            s.group_sizes.add(cnt)
            s0 = off[g0] & ~(ALIGN - 1)
            if not staged:
                s.unstaged += 1
                continue
            if cnt >= 2:
                s.staged_multi += 1
                if g0 + cnt == hi and cnt < GROUP_DOCS:
                    s.whole_range += 1
            if off[g0 + cnt] - s0 == BUF_BYTES:
                s.fills_buffer += 1
            lens = [off[g0 + i + 1] - off[g0 + i] for i in range(cnt)]
            units = packs(lens, maxg) if packing else [(i, 1, None, None) for i in range(cnt)]
            for i, nd, stop, refused in units:
                if nd >= 2:
                    s.pack_sizes.add(nd)
                    s.pack_stops.add(stop)
                    if refused is not None:
                        s.refused.add(refused)
                    if off[g0 + i + nd] - s0 == BUF_BYTES:
                        s.pack_ends_at_buffer += 1
                    s.pack_first[g0 + i:g0 + i + nd] = g0 + i
                elif i > 0:
                    s.nonfirst_paths.add(path(lens[i], maxg))
    return s


def reached(s):
    """The model paths of a survey as a sorted list of names (for reports)."""
    out = ["pack%d" % k for k in sorted(s.pack_sizes)]
    out += ["group63"] if GROUP_DOCS in s.group_sizes else []
    out += ["whole-range group"] if s.whole_range else []
    out += ["1024-byte group"] if s.fills_buffer else []
    out += ["unstaged"] if s.unstaged else []
    out += ["stop:" + x for x in sorted(s.pack_stops)]
    out += ["nonfirst:" + x for x in sorted(s.nonfirst_paths)]
    return out


def tile(data, off, times):
    """The packed corpus (data, off) `times` times over, padded like the
    original.  Scoring is per document, so the oracle of the result is
    np.tile of the oracle of one period."""
    off = np.asarray(off, dtype=np.int64)
    n = int(off[-1])
    assert off[0] == 0 and times >= 1
    total = n * times
    out = np.zeros(((total + 3) & ~3) + 32, dtype=np.uint8)
    out[:total] = np.tile(np.asarray(data[:n], dtype=np.uint8), times)
    starts = (off[:-1][None, :] + n * np.arange(times, dtype=np.int64)[:, None]).ravel()
    return out, np.concatenate([starts, [total]]).astype(np.int64)


def tiles_for(n_docs, at_least):
    return -(-at_least // n_docs)


def tile_for_product(data, off):
    """(data, off, times, CUs): the corpus tiled to 16 * 12 * CUs * 3 documents
    or more, so that the product library's grid (at most three workgroups per
    CU) has 16 or more documents on every wave.  Needs the GPU."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = len(off) - 1
    at_least = 16 * SCORE_WAVES * cus * 3
    times = tiles_for(n, at_least)
    td, to = tile(data, off, times)
    assert len(to) - 1 >= at_least and (len(to) - 1) // product_waves(len(to) - 1, cus, 3) >= 16
    return td, to, times, cus


def check_tiled_labels(model, data, off, labels, maxg):
    """Labels-only scoring of the corpus tiled for the product grid against
    the one-period labels, tiled; asserts first that packs of short
    documents form under that grid whatever the model's workgroups per CU.
    Returns (tiled offsets, times, CUs)."""
    td, to, times, cus = tile_for_product(data, off)
    for w in (1, 2, 3):
        assert survey(to, maxg, product_waves(len(to) - 1, cus, w)).pack_sizes >= {2, 3}, w
    got, _ = model.score(td, to, want_scores=False)
    bad = np.nonzero(got.reshape(times, -1) != np.asarray(labels).reshape(1, -1))
    assert not len(bad[0]), ("period, document", bad[0][:10].tolist(), bad[1][:10].tolist())
    return to, times, cus


# ------------------------------------------------------------------- corpora
ALPHABET = np.frombuffer(b"\x00\xff\x7f\x80abcdefgh \xc3\xa9\x01\xfe", dtype=np.uint8)
# the bytes of the class forms' order-dependent ties (in no other hand-made document)
TIE = {"a": 0xE0, "b": 0xE1, "c": 0xE2, "d": 0xE3}
TIE_DOCS = ["abbccd", "ccdabb", "abb", "ccd", "dcc", "bba"]


def _bytes(rng, n):
    """n bytes in one of several styles: a run of 0x00 or of 0xFF, 00/FF
    alternating, the full range 0..255, a small alphabet (so that short keys
    repeat) with runs of 0x00 and 0xFF in it."""
    style = int(rng.integers(0, 12))
    if style == 0:
        return b"\x00" * n
    if style == 1:
        return b"\xff" * n
    if style == 2:
        return (b"\x00\xff" * n)[:n]
    if style <= 6:
        return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
    d = bytearray(rng.choice(ALPHABET, size=n).tobytes())
    if n >= 24:
        p = int(rng.integers(0, n - 8))
        d[p:p + 8] = (b"\x00" if style & 1 else b"\xff") * 8
    return bytes(d)


def _pack(docs, kinds):
    lens = np.fromiter((len(d) for d in docs), dtype=np.int64, count=len(docs))
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    data = np.zeros(((total + 3) & ~3) + 32, dtype=np.uint8)
    data[:total] = np.frombuffer(b"".join(docs), dtype=np.uint8)
    for a in (data, off, lens):
        a.setflags(write=False)
    return SimpleNamespace(docs=docs, kinds=kinds, data=data, off=off, lens=lens, n=len(docs))


SHORT_REPEATS = 5
# (name, start of the section modulo 16 (None: wherever it falls), document lengths).
# A section with a start begins with a document above 1024 bytes that ends at
# that residue: it is scored alone and in place, and the next group begins
# with the section's first length.
SHORT_SECTIONS = [
    ("4x64", 3, [64, 64, 64, 64, 30]),
    ("128+128", 5, [128, 128, 50]),
    ("128+127+1", 9, [128, 127, 1, 50]),
    ("100+100+56", 2, [100, 100, 56, 20]),
    ("100+100+57", 7, [100, 100, 57, 20]),
    ("129+short", 11, [129, 40, 40, 40]),
    ("5x40", 13, [40, 40, 40, 40, 40]),
    ("pack-ends-at-1024", 0, [256, 256, 256, 64, 64, 64, 64, 33]),
    ("pack-cut-by-group", 0, [256, 256, 256, 190, 30, 30, 30, 30]),
    ("4x256", 0, [256, 256, 256, 256, 10]),
    ("4x256+1", 1, [256, 256, 256, 256, 10]),
    ("190..210", 6, list(range(190, 211))),
    ("250..260", 15, list(range(250, 261))),
    ("below-maxg", 4, [3, 64, 2, 70, 0, 5, 4, 90, 1, 6]),
]


@functools.lru_cache(maxsize=None)
def short_corpus():
    """Corpus SHORT: short documents of bytes 0..255, mean length below 192.
    330 consecutive documents of 0 or 1 bytes (70 empty, 130 of one byte, 130
    empty: groups at the 63-document cap), then SHORT_REPEATS times the
    sections above with random short documents between them, and the class
    forms' tie documents.  A repeat has the contents of the first; only the
    positions (alignment, wave, group) differ -- a launch of 24 waves has
    ranges of 63 documents and more only from about 1500 documents on, hence
    the size."""
    rng = np.random.default_rng(20240)
    docs, kinds = [], []

    def add(d, kind):
        docs.append(bytes(d))
        kinds.append(kind)

    for _ in range(70):
        add(b"", "empty")
    for c in rng.integers(0, 256, size=130, dtype=np.uint8).tolist():
        add(bytes([c]), "one")
    for _ in range(130):
        add(b"", "empty")
    big = bytes(rng.integers(0, 256, size=1100, dtype=np.uint8))
    body = {name: [_bytes(rng, n) for n in lens] for name, _, lens in SHORT_SECTIONS}
    fill = [[_bytes(rng, int(n)) for n in rng.integers(5, 101, size=45)] for _ in range(4)]
    tie = [bytes(TIE[c] for c in t) for t in TIE_DOCS]
    pos = sum(len(d) for d in docs)
    for _ in range(SHORT_REPEATS):
        for k, (name, start, _) in enumerate(SHORT_SECTIONS):
            if start is not None:
                n = 1025 + (start - (pos + 1025)) % ALIGN
                add(big[:n], "big")
                pos += n
                assert pos % ALIGN == start
            for d in body[name]:
                add(d, name)
                pos += len(d)
            if k % 4 == 3:
                for d in fill[k // 4]:
                    add(d, "fill")
                    pos += len(d)
        for d in fill[3]:
            add(d, "fill")
            pos += len(d)
        for d in tie:
            add(d, "tie")
            add(b"fgh" * 4, "after-tie")
            pos += len(d) + 12
    return _pack(docs, kinds)


LONG_BOUNDARY = list(range(1000, 1049))
LONG_OTHER = ([319, 320, 321, 511, 512, 513, 767, 768, 769, 1279, 1280, 1281, 2047, 2048, 2049, 4031, 4032, 4033,
               4095, 4096, 4097, 4159, 4160, 4161, 5000, 8191, 8192, 8193, 20000])


@functools.lru_cache(maxsize=None)
def long_corpus():
    """Corpus LONG (about 1 MB): every length 1000..1048 started at every
    residue 0..15 modulo 16 (so r + len takes every value around 1024: the
    staged / in-place switch), each after a filler document of 0..15 bytes
    that sets the residue; the lengths around every other switch of the
    kernels (superblocks, kGenBuf, ...), and the lengths 0..17.  A document of
    n bytes is the first n bytes of one of four fixed byte strings (fillers:
    of a fifth), so the keys cut from the documents repeat and a table of
    them stays small."""
    rng = np.random.default_rng(20241)
    base = []
    for k in range(4):
        b = bytearray(rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes())
        if k == 0:   # runs of 0x00 / 0xFF across the 64-, 256- and 1024-byte boundaries
            b[60:70] = b"\x00" * 10
            b[250:262] = b"\xff" * 12
            b[1018:1030] = b"\x00" * 12
        if k == 1:
            b[1000:1060] = bytes(rng.choice(ALPHABET, size=60))
        base.append(bytes(b))
    fbase = bytes(rng.choice(ALPHABET, size=32))
    docs, kinds = [], []
    pos = 0

    def add(d, kind):
        nonlocal pos
        docs.append(d)
        kinds.append(kind)
        pos += len(d)

    for r in range(ALIGN):
        for n in LONG_BOUNDARY:
            add(fbase[:(r - pos) % ALIGN], "filler")
            assert pos % ALIGN == r
            add(base[(r + n) % 4][:n], "boundary")
    for i, n in enumerate(LONG_OTHER):
        add(base[i % 4][:n], "other")
        if i < 18:
            add(fbase[3:3 + i], "tiny")
    return _pack(docs, kinds)


CORPORA = {"short": short_corpus, "long": long_corpus}


# -------------------------------------------------------------------- tables
def planted_keys(c, grams):
    """Keys cut out of corpus `c` for the gram lengths `grams`, in two lists.
    hits: per document and n, its last window (len - n) and its windows at
    POSITIONS (position 0 is also the first window of a pack's second, third
    and fourth document).  poison: the n bytes starting at len - n + 1 ..
    len - 1, which run into the following document or the pad (a window read
    past the document's end); of a document shorter than n, which is its own
    partial window, the document plus the byte after it.  The class forms'
    tie documents give no keys."""
    raw = c.data.tobytes()
    hits, poison = {}, {}
    for i in range(c.n):
        if c.kinds[i] == "tie":
            continue
        b, ln = int(c.off[i]), int(c.lens[i])
        for n in sorted(set(grams)):
            if ln >= n:
                for p in (ln - n,) + POSITIONS:
                    if p + n <= ln:
                        hits[raw[b + p:b + p + n]] = None
            elif ln >= 1:
                poison[raw[b:b + ln + 1]] = None
            for p in range(max(0, ln - n + 1), ln):
                poison[raw[b + p:b + p + n]] = None
    for k in hits:
        poison.pop(k, None)
    return list(hits), list(poison)


PRESENCE = [math.log(1.0 + 1.0 / k) for k in (1, 2, 3, 5)]


@functools.lru_cache(maxsize=None)
def table_for(corpus, kind, L, grams, n_cls=0, total_keys=0):
    """{key: row of L} for corpus "short" / "long": the planted and poison
    keys, 400 random keys (lengths from `grams` and shorter, the partial
    windows) and, up to total_keys, further windows of the corpus and random
    keys.  Every key has a row of its own draw.  kind: "dense" (normal
    draws), "mask" (log(1 + 1/k) at k random languages), "count" (one value;
    a key of 1 or 2 bytes names one language, so the direct tables apply),
    "class" (n_cls values; the tie documents' letters get the rows of
    test_class_mode_order_dependent_ties and no other window of a tie
    document is a key)."""
    c = CORPORA[corpus]()
    rng = np.random.default_rng([L, len(grams), sum(grams), n_cls, len(kind), int(corpus == "long")])
    hits, poison = planted_keys(c, grams)
    keys = dict.fromkeys(hits + poison)
    key_lens = sorted(set(grams) | {max(1, g - 3) for g in grams})
    for _ in range(400):
        keys[bytes(rng.choice(ALPHABET, size=int(rng.choice(key_lens))))] = None
    if total_keys:
        raw = c.data.tobytes()
        total = int(c.off[-1])
        for n in sorted(set(grams)):
            for p in rng.integers(0, total - n, size=2 * total_keys // len(set(grams))).tolist():
                if len(keys) >= total_keys * 3 // 4:
                    break
                keys[raw[p:p + n]] = None
        while len(keys) < total_keys:
            n = int(rng.choice([g for g in grams if g >= 3]))
            keys.update((bytes(r), None) for r in rng.integers(0, 256, size=(4096, n), dtype=np.uint8))
    keys = list(keys)
    nk = len(keys)
    if kind == "dense":
        return dict(zip(keys, rng.normal(size=(nk, L)).tolist()))
    m = rng.random((nk, L)) < rng.uniform(0.02, 0.6, size=nk)[:, None]
    one = rng.integers(0, L, size=nk)
    if kind == "count":
        m[[len(k) <= 2 for k in keys]] = False
    m[np.arange(nk), one] |= ~m.any(axis=1)
    if kind == "mask":
        v = np.array([0.0] + [math.log(1.0 + 1.0 / k) for k in range(1, L + 1)])[m.sum(axis=1)]
    elif kind == "count":
        v = np.full(nk, math.log(2.0))
    else:
        v = np.asarray(PRESENCE[:n_cls])[rng.integers(0, n_cls, size=nk)]
    table = dict(zip(keys, np.where(m, v[:, None], 0.0).tolist()))
    if kind == "class":
        for t in TIE_DOCS:
            d = bytes(TIE[ch] for ch in t)
            for n in range(2, len(d) + 1):
                for p in range(len(d) - n + 1):
                    table.pop(d[p:p + n], None)
        v1, v2 = PRESENCE[0], PRESENCE[1]
        for ch, lang, val in (("a", 0, v1), ("b", 0, v2), ("c", 1, v2), ("d", 1, v1)):
            row = [0.0] * L
            row[lang] = val
            table[bytes([TIE[ch]])] = row
    return table


def n_long_keys(table):
    """Keys of 3 bytes and more: what sizes the model's bloom (2.5 per word)."""
    return sum(len(k) >= 3 for k in table)


def plus_following_byte(c):
    """The corpus with every document one byte longer: what a kernel scores
    that reads one byte past each document's end."""
    raw = c.data.tobytes()
    docs = [raw[int(c.off[i]):int(c.off[i + 1]) + 1] for i in range(c.n)]
    return _pack(docs, c.kinds)


# --------------------------------------------------------------------- forms
def _form(name, kind, L, grams, variant="product", env=(), n_cls=0, total_keys=0, mode=None, has=(), hasnt=(),
          scores=True):
    return SimpleNamespace(name=name, kind=kind, L=L, grams=tuple(grams), variant=variant, env=dict(env), n_cls=n_cls,
                           total_keys=total_keys, mode=mode, has=tuple(has), hasnt=tuple(hasnt), scores=scores)


G5 = (1, 2, 3, 4, 5)
# the table forms of the geometry tests: (table, library variant and
# diagnostics switches, the mode / layout flags the model must report).
# scores=False: labels-only calls (class mode), through the host and the
# device entry points; every other form is scored with and without scores.
FORMS = [
    _form("dense", "dense", 9, (1, 3, 2, 1), mode=1),
    _form("mask", "mask", 70, (1, 2, 3, 4, 5, 6, 7), mode=0),
    _form("count", "count", 20, G5, mode=2, has=("direct", "packs")),
    _form("count-nopack", "count", 20, G5, "diag", {"LDGPU_NO_PACK": "1"}, mode=2, has=("direct",), hasnt=("packs",)),
    _form("count-nodirect", "count", 20, G5, "diag", {"LDGPU_NO_DIRECT": "1"}, mode=2, hasnt=("direct",)),
    _form("count-replay", "count", 20, G5, "diag", {"LDGPU_NO_COUNT_MODE": "1"}, mode=0),
    _form("class2", "class", 20, G5, n_cls=2, has=("classes",), scores=False),
    _form("class4", "class", 20, G5, n_cls=4, has=("classes",), scores=False),
    _form("wide-count", "count", 12, (2, 9, 12), mode=2, has=("wide_keys",)),
    _form("wide-dense", "dense", 12, (2, 9, 12), mode=1, has=("wide_keys",)),
    _form("lang-blocks-count", "count", 300, (1, 2, 3, 4), has=("lang_blocks",)),
    _form("lang-blocks-mask", "mask", 300, (1, 2, 3, 4), has=("lang_blocks",)),
    _form("general", "dense", 9, (20,), has=("general_keys",)),
    _form("mixed", "count", 9, (3, 20), has=("general_keys",)),
]
for _c in "01":
    for _b in "01":
        FORMS.append(_form("keyed-chunks%s-buckets%s" % (_c, _b), "count", 20, G5, "diag",
                           {"LDGPU_KB_CHUNKS": _c, "LDGPU_BUCKETS": _b}, total_keys=60000, mode=2,
                           has=(("keyed_bloom_chunks",) if _c == "1" else ()) + (("buckets",) if _b == "1" else ()),
                           hasnt=(("keyed_bloom_chunks",) if _c == "0" else ()) + (("buckets",) if _b == "0" else ())))
FORMS.append(_form("keyed-lines", "count", 20, G5, "diag", {"LDGPU_KB_LINES": "1"}, total_keys=60000, mode=2))
FORM_BY_NAME = {f.name: f for f in FORMS}


def form_table(f, corpus):
    return table_for(corpus, f.kind, f.L, f.grams, f.n_cls, f.total_keys)


def table_specs():
    """The distinct tables of FORMS (several forms share one)."""
    return sorted({(f.kind, f.L, f.grams, f.n_cls, f.total_keys) for f in FORMS}, key=str)
