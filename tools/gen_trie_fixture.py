"""tests/golden/trie_config2_keys.bin: config 2's top-K table rebuilt on the CPU
(numpy only, about 20 s) from bench.build_table's generator and seeds under
bench.topk_table_from_counts' rule -- 6-byte records: key u32 LE, length u8,
language u8 (0xff: a row that names several languages).

    python tools/gen_trie_fixture.py tests/golden/trie_config2_keys.bin

Run it again whenever bench.py's config 2 (languages, grams, profile size,
training documents), its seeds or synth's generator change: tests/test_trie_host.py
asserts that THIS table packs into the LDS, and the GPU's table is the same
rows only while the two stay in step."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spark-languagedetector_amd"))
from languagedetection import synth  # noqa: E402

L, K, grams, train = 20, 500, [1, 2, 3, 4, 5], 1000
ls = synth.make_languages(L)
lang = np.repeat(np.arange(L, dtype=np.int32), train)
data, off, lang = synth.generate(ls, len(lang), 200, 2000, seed=synth.SEED_BASE + 100, doc_lang=lang)
print("train bytes", off[-1])
doc_of = np.repeat(np.arange(len(lang)), np.diff(off))
keys_all, pres_all = [], []
for n in grams:
    # windows inside one document
    idx = np.arange(len(data) - n + 1)
    ok = doc_of[idx] == doc_of[idx + n - 1]
    idx = idx[ok]
    # (length, bytes) order: big-endian packing
    v = np.zeros(len(idx), dtype=np.uint64)
    for d in range(n):
        v = (v << np.uint64(8)) | data[idx + d].astype(np.uint64)
    wl = lang[doc_of[idx]].astype(np.uint64)
    u = np.unique(v * np.uint64(32) + wl)
    g, l = u // np.uint64(32), (u % np.uint64(32)).astype(np.int64)
    ug, inv = np.unique(g, return_inverse=True)
    pres = np.zeros((len(ug), L), dtype=bool)
    pres[inv, l] = True
    keys_all.append((n, ug))
    pres_all.append(pres)
pres = np.concatenate(pres_all)
klen = np.concatenate([np.full(len(ug), n) for n, ug in keys_all])
kval = np.concatenate([ug for n, ug in keys_all])
k = pres.sum(axis=1)
w = np.log(1.0 + 1.0 / k)
chosen = np.zeros(len(k), dtype=bool)
idx = np.arange(len(k))
for l in range(L):
    v = np.where(pres[:, l], w, 0.0)
    chosen[np.lexsort((idx, -v))[:K]] = True
sel = np.nonzero(chosen)[0]
print("rows", len(sel), "by length", {n: int((klen[sel] == n).sum()) for n in grams})
rec = bytearray()
for i in sel:
    n, be = int(klen[i]), int(kval[i])
    bs = be.to_bytes(n, "big")
    assert n <= 4
    le = int.from_bytes(bs, "little")
    langs = np.nonzero(pres[i])[0]
    rec += le.to_bytes(4, "little") + bytes([n, int(langs[0]) if len(langs) == 1 else 0xff])
open(sys.argv[1], "wb").write(bytes(rec))
print("multi-language rows", sum(1 for j in range(5, len(rec), 6) if rec[j] == 0xff))
