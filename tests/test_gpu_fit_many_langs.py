"""FIT with more than a thousand languages PRESENT in one call (a language
with a non-empty document; the table's L alone costs nothing).

FIT v4 gives every present language at least one emit workgroup, so a batch's
workgroup count grows with them -- 4 per CU for splitting the heavy languages
plus one per language -- and part2_kernel keeps a block prefix over the
workgroups of each of its 8 groups in LDS.  That array once ended at 256
workgroups per group: a plan of more than 2048 (more than 2048 balanced
languages on 256 CUs, or some 1030 with one language holding most of the
bytes) wrote and searched past it.  No other test reaches such a plan: the
largest FIT calls elsewhere have 520 languages present.  The cases sit
below, on and above that edge, in each record form (one, two and three words)
and on the sort path at its widest language field; tests/fitplan.py restates
the plan, and every test first asserts with it, for the CU count of the
device it runs on, that its corpus lands in the regime it is meant for.

Counts are compared bit-exact with the C restatement (ldoracle_c.count), in
the dense and in the sparse export, and one small top-K table per case with
the rule applied to the oracle's counts.
"""
import functools

import numpy as np
import pytest

import fitplan as F
import ldoracle_c as OC
from bytecorpus import _topk_table_from_counts
from languagedetection import _lib
from languagedetection.runtime import DeviceCounts

pytestmark = pytest.mark.gpu

PROFILE = 3   # languageProfileSize of the per-case table


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(_lib.default_device()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(keys, counts [n, L]) of the case's corpus, computed once: do not modify."""
    L, _, grams = F.CASES[name][:3]
    keys, cnt = OC.count(*F.case_corpus(name), L, grams)
    cnt.setflags(write=False)
    return keys, cnt


def _assert_exports(counts, okeys, expect, L):
    keys, cnt = counts.export()
    assert keys == okeys
    assert np.array_equal(cnt, expect)
    kb, ko, po, pl, pc = counts.export_sparse()
    b = kb.tobytes()
    assert [b[ko[i]:ko[i + 1]] for i in range(len(ko) - 1)] == okeys
    assert np.all(pc > 0) and int(po[-1]) == len(pl) == len(pc)
    dense = np.zeros_like(expect)
    dense[np.repeat(np.arange(len(okeys)), np.diff(po)), pl] = pc
    assert np.array_equal(dense, expect)
    assert counts.fit_table(PROFILE) == _topk_table_from_counts(okeys, expect, L, PROFILE)


@pytest.mark.parametrize("name", list(F.CASES))
def test_many_languages_present(name, cus):
    """The product library, one call, every language of [0, P) present."""
    L, P, grams, _, K, path, regime = F.CASES[name]
    data, off, lang = F.case_corpus(name)
    assert F.record_route(L, grams) == (K, path)
    if regime is not None:
        grid = F.emit_workgroups(off, lang, L, cus)
        print(name, "emit workgroups", grid, "on", cus, "CUs")
        assert len(grid) == 1 and F.regime_of(grid[0]) == regime, (grid, cus)
    counts = DeviceCounts(L, grams)
    counts.count(data, off, lang)
    okeys, ocnt = _oracle(name)
    _assert_exports(counts, okeys, ocnt, L)
    counts.close()


def test_second_call_accumulates_above_the_edge(cus):
    """4096 languages, grams [5, 1, 3, 3]: a second count() over the first
    5000 documents (themselves a plan above the edge) adds to the first."""
    name, n2 = "4096-dup-length", 5000
    L, _, grams = F.CASES[name][:3]
    data, off, lang = F.case_corpus(name)
    d2, o2, l2 = data[:int(off[n2])], off[:n2 + 1], lang[:n2]
    assert all(F.regime_of(F.emit_workgroups(o, l, L, cus)[0]) == "above" for o, l in ((off, lang), (o2, l2)))
    counts = DeviceCounts(L, grams)
    counts.count(data, off, lang)
    counts.count(d2, o2, l2)
    okeys, ocnt = _oracle(name)
    extra = dict(zip(*OC.count(d2, o2, l2, L, grams)))
    expect = np.array([ocnt[i] + extra.get(k, 0) for i, k in enumerate(okeys)])
    assert set(extra) <= set(okeys)
    _assert_exports(counts, okeys, expect, L)
    counts.close()


def test_batches_on_both_sides_of_the_edge(cus, monkeypatch):
    """The diagnostics library with LDGPU_FIT_BATCH_WINDOWS at the size of the
    2049-language corpus, over that corpus, its reverse and a third of it:
    three batches in one call, two above 2048 emit workgroups and one below."""
    name = "2049-balanced"
    L, _, grams = F.CASES[name][:3]
    data, off, lang, batch_recs = F.many_batches(name)
    grid = F.emit_workgroups(off, lang, L, cus, batch_recs=batch_recs)
    print("emit workgroups per batch", grid, "on", cus, "CUs")
    assert len(grid) >= 3 and max(grid) > F.OLD_EDGE and min(grid) < F.OLD_EDGE, (grid, cus)
    monkeypatch.setenv("LDGPU_FIT_BATCH_WINDOWS", str(batch_recs))
    counts = DeviceCounts(L, grams, variant="diag")
    counts.count(data, off, lang)
    okeys, ocnt = OC.count(data, off, lang, L, grams)
    _assert_exports(counts, okeys, ocnt, L)
    counts.close()
