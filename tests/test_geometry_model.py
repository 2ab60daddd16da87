"""The host model of the SCORE kernel's document geometry (tests/geometry.py)
against the kernel's own constants, and the properties the GPU geometry tests
(test_gpu_geometry.py) lean on: that the corpora, under the grids those tests
launch, put several documents on a wave and form every kind of group and
pack; and that a kernel reading past a document's end, or crossing into its
neighbour, would change what the oracle expects.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import geometry as G
import ldoracle_c as OC
from conftest import ROOT

CSRC = os.path.join(ROOT, "spark-languagedetector_amd", "csrc")


def _constants():
    text = ""
    for name in ("ldgpu_internal.h", "ldgpu_general.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text += f.read()
    env = {"LDGPU_SCORE_WAVES": int(re.search(r"#define LDGPU_SCORE_WAVES (\d+)", text).group(1))}
    for name in ("kScoreWaves", "kQueueCap", "kBufBytes", "kBufWords", "kPackDocs", "kGenBuf"):
        m = re.search(r"constexpr (?:int|uint32_t) %s = ([^;]+);" % name, text)
        assert m, name
        env[name] = int(eval(re.sub(r"(\d)u\b", r"\1", m.group(1)).replace("/", "//"), {}, dict(env)))
    return env


def test_constants_equal_the_headers():
    k = _constants()
    assert k["kScoreWaves"] == G.SCORE_WAVES
    assert k["kBufBytes"] == G.BUF_BYTES
    assert k["kPackDocs"] == G.PACK_DOCS
    assert k["kGenBuf"] == G.GEN_BUF
    assert G.SUPERBLOCK == 64 * G.PACK_DOCS and G.PACK_DOC_MAX * 2 == G.SUPERBLOCK
    assert G.GROUP_DOCS == 63 and G.ALIGN == 16 and G.BUF_BYTES == 64 * G.ALIGN   # one 16-B load per lane
    with open(os.path.join(CSRC, "ldgpu_api.hip")) as f:
        api = f.read()
    assert re.search(r"p\.group = %d;" % G.GROUP_DOCS, api)
    with open(os.path.join(CSRC, "ldgpu_score.hip")) as f:
        score = f.read()
    assert "len <= %d)" % G.PACK_DOC_MAX in score and "& ~(int64_t)%d" % (G.ALIGN - 1) in score


def test_lds_floor_bounds_workgroups_per_cu():
    """Queue, staging double buffer, the smallest hit area and the labels of
    twelve waves: no model has more than three workgroups on a CU, so
    16 * 12 * CUs * 3 documents put 16 or more on every wave."""
    k = _constants()
    assert 163840 // (k["kScoreWaves"] * (4 * k["kQueueCap"] + 8 * k["kBufWords"] + 256 + 256)) == 3


# ------------------------------------------------------------- the model itself
def test_groups_by_hand():
    off = [5, 5, 300, 1029, 1030, 2100, 2101]
    # from s0 = 0 the third document ends beyond 1024; from s0 = 288 two fit; 1070 bytes from s0 = 1024: in place
    assert G.groups(off, 0, 6) == [(0, 2, True), (2, 2, True), (4, 1, False), (5, 1, True)]
    assert G.groups(off, 0, 1) == [(0, 1, True)]
    assert G.groups([0] * 131, 0, 130) == [(0, 63, True), (63, 63, True), (126, 4, True)]
    assert G.groups([16, 1040, 1041], 0, 2) == [(0, 1, True), (1, 1, True)]      # 1024 from an aligned start: staged
    assert G.groups([17, 1041, 1042], 0, 2) == [(0, 1, False), (1, 1, True)]     # the same one byte on: in place
    assert G.wave_ranges(10, 4) == [(0, 2), (2, 5), (5, 7), (7, 10)]
    assert G.product_waves(3000, 256, 2) == 12 * 250 and G.product_waves(10 ** 6, 256, 2) == 12 * 512


def test_packs_by_hand():
    assert G.packs([64, 64, 64, 64, 30], 5) == [(0, 4, "full", None), (4, 1, "group", None)]
    assert G.packs([128, 127, 1, 50], 5) == [(0, 2, "short", None), (2, 1, None, None), (3, 1, "group", None)]
    assert G.packs([100, 100, 56, 20], 5)[0] == (0, 3, "total", 276)
    assert G.packs([100, 100, 57, 20], 5) == [(0, 2, "total", 257), (2, 2, "group", None)]
    assert G.packs([129, 40, 40], 5) == [(0, 1, None, None), (1, 2, "group", None)]
    assert G.packs([4, 5], 5) == [(0, 1, None, None), (1, 1, "group", None)]
    assert [G.path(n, 5) for n in (4, 5, 196, 197, 256, 257)] == ["general", "fast", "fast", "fast-FULL", "fast-FULL",
                                                                  "general"]


def test_tile():
    c = G.short_corpus()
    data, off = G.tile(c.data, c.off, 3)
    n, total = c.n, int(c.off[-1])
    assert len(off) == 3 * n + 1 and off[-1] == 3 * total and len(data) % 4 == 0 and len(data) >= 3 * total + 4
    assert np.array_equal(np.diff(off), np.tile(c.lens, 3))
    assert np.array_equal(data[total:2 * total], c.data[:total]) and not data[3 * total:].any()


# ------------------------------------------------------------------ the corpora
def _check_short(s, maxg, cap_reachable):
    if cap_reachable:
        assert G.GROUP_DOCS in s.group_sizes                  # a group of exactly 63 documents
    else:
        # fewer than 63 documents on every wave: the cap cannot bind; the
        # other bound of the group's size, its wave's range, does
        assert s.docs_per_wave < G.GROUP_DOCS and s.whole_range
    assert s.pack_sizes == {2, 3, 4}
    assert 257 in s.refused                                   # a pack refused at total 257
    assert s.pack_stops == {"full", "group", "short", "total"}
    assert s.fills_buffer and s.pack_ends_at_buffer           # a group, and a pack, ending at byte 1024
    assert s.unstaged                                         # a group of one document scored in place
    assert s.nonfirst_paths == {"fast", "fast-FULL", "general"}
    assert s.max_groups >= 8                                  # the double buffer flips many times


@pytest.mark.parametrize("grid", [1, 2])
def test_short_corpus_under_small_grids(grid):
    c = G.short_corpus()
    assert c.off[-1] / c.n < 192                              # the pack kernel is chosen
    _check_short(G.survey(c.off, 5, grid * G.SCORE_WAVES), 5, True)


@pytest.mark.parametrize("wg_per_cu", [1, 2, 3])
def test_short_corpus_tiled_under_the_product_grid(wg_per_cu):
    c = G.short_corpus()
    at_least = 16 * G.SCORE_WAVES * 256 * 3
    _, off = G.tile(c.data, c.off, G.tiles_for(c.n, at_least))
    assert len(off) - 1 >= at_least
    s = G.survey(off, 5, G.product_waves(len(off) - 1, 256, wg_per_cu))
    assert s.docs_per_wave >= 16
    _check_short(s, 5, False)


def test_short_corpus_contents():
    c = G.short_corpus()
    total = int(c.off[-1])
    assert len(np.unique(c.data[:total])) == 256
    for run in (b"\x00" * 30, b"\xff" * 30):
        assert run in c.data.tobytes()
    k = "".join("e" if x == "empty" else "o" if x == "one" else "." for x in c.kinds)
    assert "e" * 70 in k and "o" * 130 in k and "e" * 130 in k
    lens = set(c.lens.tolist())
    assert lens >= set(range(190, 211)) | set(range(250, 261)) and max(lens) > 1024
    # every section keeps the shape it is named for
    for name, _, shape in G.SHORT_SECTIONS:
        idx = [i for i, x in enumerate(c.kinds) if x == name]
        assert len(idx) == G.SHORT_REPEATS * len(shape)
        assert c.lens[idx[:len(shape)]].tolist() == shape
    # the aligned and the shifted 4 x 256: 1024 bytes from a 16-aligned start, and one byte on
    for name, r in (("4x256", 0), ("4x256+1", 1)):
        first = [i for i, x in enumerate(c.kinds) if x == name][::5]
        assert all(c.off[i] % 16 == r and c.kinds[i - 1] == "big" and c.lens[i - 1] > 1024 for i in first)


def test_long_corpus_contents():
    c = G.long_corpus()
    assert 800_000 < c.off[-1] < 1_200_000
    start = c.off[:-1] % 16
    have = set(zip(start.tolist(), c.lens.tolist()))
    assert have >= {(r, n) for r in range(16) for n in range(1000, 1049)}
    for r in range(16):
        assert {r + n for rr, n in have if rr == r} >= {1023, 1024, 1025}
    assert set(c.lens.tolist()) >= set(G.LONG_OTHER) | set(range(18))
    # under one and two workgroups: staged and in-place documents at the 1024 boundary, for every residue
    for grid in (1, 2):
        seen = set()
        for lo, hi in G.wave_ranges(c.n, grid * G.SCORE_WAVES):
            for g0, cnt, staged in G.groups(c.off.tolist(), lo, hi):
                r = int(c.off[g0] % 16)
                if r + c.lens[g0] in (1024, 1025):
                    seen.add((r, staged, cnt > 1))
        for r in range(16):
            assert (r, False, False) in seen and {x[1] for x in seen if x[0] == r} == {True, False}, (grid, r)
        assert any(multi for _, staged, multi in seen if staged)   # a 1024-byte group of a long document and its filler


# ------------------------------------------------------ what the tables can tell
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _oracle(corpus, spec):
    c = G.CORPORA[corpus]()
    t = OC.Table(G.table_for(corpus, *spec), spec[1])
    return t.score(list(spec[2]), c.data, c.off, want_scores=True, nthreads=8), t


@pytest.mark.parametrize("corpus", ["short", "long"])
@pytest.mark.parametrize("spec", G.table_specs(), ids=lambda s: "%s-L%d-g%s%s" % (s[0], s[1], "".join(map(str, s[2])),
                                                                                  "-%d" % s[4] if s[4] else ""))
def test_tables_tell_a_read_past_the_end(corpus, spec):
    """One byte too many at the end of a document changes the scores of at
    least 90 % of the documents that have a byte, and the labels take more
    than two values: a kernel that mixes neighbours up cannot pass."""
    c = G.CORPORA[corpus]()
    (ol, os_), t = _oracle(corpus, spec)
    over = G.plus_following_byte(c)
    _, s1 = t.score(list(spec[2]), over.data, over.off, want_scores=True, nthreads=8)
    differ = (_bits(s1) != _bits(os_)).any(axis=1)
    assert differ[c.lens >= 1].mean() >= 0.9, differ[c.lens >= 1].mean()
    assert len(np.unique(ol)) > 2
    if spec[0] == "count" and max(spec[2]) <= 5 and not spec[4]:
        # direct tables and an LDS bloom of at most 4096 words (2.5 keys of >= 3 bytes per word)
        table = G.table_for(corpus, *spec)
        assert G.n_long_keys(table) < 10240 * 3 // 4
        assert all(sum(v != 0.0 for v in row) == 1 for k, row in table.items() if len(k) <= 2)


@pytest.mark.parametrize("n_cls", [2, 4])
def test_class_tables_hold_order_dependent_ties(n_cls):
    """The tie documents of corpus SHORT (the construction of
    test_class_mode_order_dependent_ties): languages 0 and 1 hit the same
    values as often in another order, their folds differ in the last bits, and
    no rounding bound over counts can tell which leads."""
    c = G.short_corpus()
    spec = ("class", 20, G.G5, n_cls, 0)
    (ol, os_), _ = _oracle("short", spec)
    table = G.table_for("short", *spec)
    assert len({v for row in table.values() for v in row if v}) == n_cls
    tie = [i for i, k in enumerate(c.kinds) if k == "tie"][:2]
    assert [c.docs[i] for i in tie] == [bytes(G.TIE[ch] for ch in t) for t in G.TIE_DOCS[:2]]
    for i in tie:
        s = os_[i]
        assert s[0] != s[1] and np.argsort(s)[-2:].tolist() in ([0, 1], [1, 0])
        assert abs(int(_bits(s[:1])[0]) - int(_bits(s[1:2])[0])) <= 4
    assert ol[tie[0]] == int(os_[tie[0], 1] > os_[tie[0], 0])
