"""The host model of FIT v4's emit plan (tests/fitplan.py) against the
runtime's own constants and three plans worked out by hand, and what the
many-language GPU tests (test_gpu_fit_many_langs.py) lean on: that each of
their corpora, on a device of 256 CUs, lands on its side of the 2048 emit
workgroups at which a part2 group holds more than 256, and takes the record
form and path its case names.  No GPU."""
import os
import re

import numpy as np
import pytest

import fitplan as F
from conftest import ROOT

CSRC = os.path.join(ROOT, "spark-languagedetector_amd", "csrc")


def _read(*names):
    text = ""
    for name in names:
        with open(os.path.join(CSRC, name)) as f:
            text += f.read()
    return text


def test_constants_equal_the_sources():
    text = _read("ldgpu_common.h", "ldgpu_fit.h")
    for name, value in (("kSplits", F.SPLITS), ("kMaxEmitWg", F.MAX_EMIT_WG), ("kMaxGram", F.MAX_GRAM)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    api = _read("ldgpu_api.hip")
    assert re.search(r"constexpr int64_t kBatchRecords = 1ll << (\d+);", api).group(1) == str(F.BATCH_RECORDS.bit_length() - 1)
    # the share of workgroups for splitting, and the bound it keeps
    assert "std::min<int64_t>(%d * (int64_t)x->cus, kMaxEmitWg - kSplits - present)" % F.WG_PER_CU in api
    assert "if (grid_a > kMaxEmitWg)" in api
    with open(os.path.join(ROOT, "include", "ldgpu.h")) as f:
        assert re.search(r"#define LDGPU_MAX_LANGS (\d+)", f.read()).group(1) == str(F.MAX_LANGS)
    # part2's prefix array covers a group of the largest plan
    fit = _read("ldgpu_fit.hip")
    assert "int32_t gpre[kMaxEmitWg / kSplits + 1];" in fit
    assert "p.grid_a > kMaxEmitWg) return hipErrorInvalidValue" in fit
    assert F.MAX_EMIT_WG % F.SPLITS == 0 and F.MAX_EMIT_WG - F.SPLITS > F.MAX_LANGS
    assert F.OLD_EDGE == F.SPLITS * 256


# ------------------------------------------------------------ plans by hand
def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def test_single_language_by_hand():
    """4 CUs: a share of 16 workgroups.  Twenty documents of 10 bytes: target
    = ceil(200 / 16) = 13, ceil(200 / 13) = 16 parts with goals 12, 25, 37, 50,
    62, ...: a part takes documents until its goal is met -- 2, 1, 1, 1,
    2, 1, 1, 1, ... documents --, all sixteen get one.  Three documents of 100
    bytes: target 19, 16 parts, goals 18, 37, ..., 300; the first part takes
    the first document (100 bytes: the goals up to 93 are met), parts 2-5 get
    none and are dropped, part 6 (goal 112) takes the second, part 11 (goal
    206) the third: 3 workgroups, padded to 8."""
    assert F.batch_parts([10] * 20, [0] * 20, 1, 4) == 16
    assert F.emit_workgroups(_off([10] * 20), [0] * 20, 1, 4) == [16]
    assert F.batch_parts([100] * 3, [0] * 3, 1, 4) == 3
    assert F.emit_workgroups(_off([100] * 3), [0] * 3, 1, 4) == [8]
    # no document of a supported language: one empty workgroup per group
    assert F.emit_workgroups(_off([5, 0]), [-1, 0], 1, 4) == [8]


def test_balanced_languages_by_hand():
    """4 CUs, 5 of 8 languages present with two documents of 10 bytes each;
    an empty document, one labelled -1 and one labelled 8 do not count.  Wk =
    100, target = ceil(100 / 16) = 7; a language has ceil(20 / 7) = 3 parts
    with goals 6, 13, 20: one document each for the first two, none left for
    the third.  10 workgroups, padded to 16."""
    lens = [10, 10, 10, 0, 10, 10, 33, 10, 10, 10, 10, 7, 10]
    lang = [0, 2, 0, 3, 2, 5, -1, 6, 5, 6, 7, 8, 7]
    assert F.batch_parts(lens, lang, 8, 4) == 10
    assert F.emit_workgroups(_off(lens), lang, 8, 4) == [16]


def test_heavy_language_by_hand():
    """2 CUs (a share of 8): language 0 with ten documents of 100 bytes, thirty
    languages with one document of 2 bytes.  Wk = 1060, target = 133, language
    0 in ceil(1000 / 133) = 8 parts with goals 125, 250, ..., 1000 taking 2, 1,
    1, 1, 2, 1, 1, 1 documents; the light languages one workgroup each whatever
    the share: 38 workgroups, padded to 40 -- five times the share."""
    lens = [100] * 10 + [2] * 30
    lang = [0] * 10 + list(range(1, 31))
    assert F.batch_parts(lens, lang, 40, 2) == 38
    assert F.emit_workgroups(_off(lens), lang, 40, 2) == [40]
    # in batches of 500 bytes: 5 + 5 documents of language 0 (target 63, 8 parts, 5 with a document),
    # then the light languages
    assert F.batches(_off(lens), 500) == [(0, 5), (5, 10), (10, 40)]
    assert F.emit_workgroups(_off(lens), lang, 40, 2, batch_recs=500) == [8, 8, 32]


def test_plan_keeps_the_bound_where_the_cu_share_would_not():
    """Every language present, a thousand of them with twenty documents of 750
    bytes, on devices whose 4 per CU alone reach the bound: the share shrinks
    to what the present languages leave (4088 of 8192), so target = ceil(
    15204800 / 4088) = 3720 and a heavy language has ceil(15050 / 3720) = 5
    parts, where a share of 8192 would make it 9 -- 12096 workgroups.  Up to
    1022 CUs the share is the 4 per CU."""
    L = F.MAX_LANGS
    lens = [750] * 20000 + [50] * L
    lang = [l for l in range(1000) for _ in range(20)] + list(range(L))
    for cus in (1022, 1024, 2048, 8192):
        n = F.batch_parts(lens, lang, L, cus)
        assert n == 1000 * 5 + (L - 1000) and F.padded(n) <= F.MAX_EMIT_WG, (cus, n)
    assert F.batch_parts(lens, lang, L, 256) == 1000 * 2 + (L - 1000)   # share 1024: target 14849
    assert min(F.WG_PER_CU * 1022, F.MAX_EMIT_WG - F.SPLITS - L) == F.WG_PER_CU * 1022


def test_record_routes():
    assert F.record_route(20, [1, 2, 3, 4, 5]) == (1, "v4")
    assert F.record_route(200, [1, 2, 3, 4, 5, 6, 7]) == (2, "v5")
    assert F.record_route(4096, [2, 6, 1]) == (2, "v5")
    assert F.record_route(255, [7]) == (2, "v5") and F.record_route(256, [7]) == (2, "v4")
    assert F.record_route(5, [2, 9]) == (3, "v4")


# ------------------------------------------------- the GPU tests' corpora
@pytest.mark.parametrize("name", list(F.CASES))
def test_case_corpus_and_regime_at_256_cus(name):
    L, P, grams, kw, K, path, regime = F.CASES[name]
    data, off, lang = F.case_corpus(name)
    lens = np.diff(off)
    # every language of [0, P) has a non-empty document; some documents are
    # empty, some labelled -1; the last language's only document is one byte
    assert P <= L and set(lang[lens > 0].tolist()) - {-1} == set(range(P))
    assert (lang == -1).sum() >= 3 and (lens[lang >= 0] == 0).any() == (kw.get("docs_hi", 3) > 1)
    assert lens[lang == P - 1].tolist() == [1]
    assert set(bytes(data[:int(off[-1])])) == set(kw["alphabet"])
    if "heavy" in kw:
        n, size = kw["heavy"]
        mine = lens[lang == 0]
        assert n >= 1200 and (mine == size).sum() == n and mine.sum() >= 0.95 * lens[lang >= 0].sum()
    else:
        assert lens.max() <= 40
    assert F.record_route(L, grams) == (K, path)
    if K == 1:   # the record's language and count fields
        assert 64 - (8 * max(grams) + 1) - max(1, F._log2u(L)) >= 8
    grid = F.emit_workgroups(off, lang, L, 256)
    assert len(grid) == 1 and grid[0] <= F.MAX_EMIT_WG
    if regime is not None:
        assert F.regime_of(grid[0]) == regime, grid
        if regime == "edge":
            assert all(F.emit_workgroups(off, lang, L, cus) == [F.OLD_EDGE] for cus in (64, 304, 1024))


def test_some_alphabet_has_high_bytes():
    used = [kw["alphabet"] for _, _, _, kw, _, _, _ in F.CASES.values()]
    assert any(max(a) >= 0x80 for a in used) and any(0x00 in a and 0xFF in a for a in used)
    assert F.CASES["4096-dup-length"][2] == [5, 1, 3, 3]
    assert (max(1, F._log2u(4096)), 64 - 41 - 12) == (12, 11)   # lb, cb of that case


def test_many_batches_run_straddles_the_edge():
    """Batches of the 2049-language corpus's own size: the corpus, the corpus
    reversed, a third of it -- two plans above 2048 workgroups, one below."""
    L = F.CASES["2049-balanced"][0]
    data, off, lang, batch_recs = F.many_batches("2049-balanced")
    grid = F.emit_workgroups(off, lang, L, 256, batch_recs=batch_recs)
    assert len(grid) == 3
    assert grid[0] > F.OLD_EDGE and grid[1] > F.OLD_EDGE and grid[2] < F.OLD_EDGE
    assert F.emit_workgroups(off, lang, L, 256) != grid
