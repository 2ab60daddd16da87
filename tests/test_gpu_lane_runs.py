"""GPU parity of count / class mode on the lane-run window layout
(LDGPU_LANE_RUNS, ldgpu_score.hip): on the scanned split path of a staged
fast-path document lane i owns the four consecutive window positions
4 i .. 4 i + 3, reads the three or four aligned dwords of its 11-byte run, and
derives every Bloom word, filter bit and direct key from the run's 3-byte
groups.  Hand-built tables (those of test_gpu_scan_append.py) and documents
put keys where that map can go wrong:

  base      consecutive documents of odd lengths, so that a document's staged
            base takes every residue modulo 16 (and so modulo 4: three dwords
            or four), as a group's first document and inside a group;
  lengths   every document length from max(grams) to 264 -- across the old
            192 + maxg switch, up to 256, and from 257 on the general path --
            each ending in a key of every length, the next document going on
            with the key's byte;
  slots     a key of every length 1..7 at each in-lane slot k = 0..3 of several
            lanes (from slot 1 on a key of 4 bytes or more runs into the next
            lane's bytes; the 7-byte key at slot 3 needs the run's third dword);
  end       for every length 1..7 a key that ends on the document's last byte
            (counts), and the same key one byte later, completed only by the
            next document's first byte (does not count), for document ends at
            every residue modulo 4;
  fallback  documents with more than 288 candidates (the per-length path, which
            reloads in the old layout) between ordinary ones.

Every case compares with the C oracle: labels exactly, fp64 scores bit for bit
where scores are requested.  Each corpus runs one document per wave, tiled for
the product grid, and several per wave on one and two workgroups (diagnostics
library, LDGPU_SCORE_GRID)."""
import math

import numpy as np
import pytest

import geometry
import ldoracle_c as OC
import test_gpu_scan_append as SA
from languagedetection import encoding

pytestmark = pytest.mark.gpu

L = SA.L
FILL = SA.FILL
QUEUE_CAP = SA.QUEUE_CAP
RUN = SA.RUN
# a key of every length 1..7 (SA.KEYS)
KEY_OF = {1: b"q", 2: b"ab", 3: b"xyz", 4: b"wxyz", 5: b"vwxyz", 6: b"uvwxyz", 7: b"tuvwxyz"}
SLOT_LANES = (0, 5, 21, 40, 62)     # a key at 4 lane + k (lane 62: the longest keys at slot 3 are cut by the document's end)
END_LENGTHS = (256, 201, 70, 67)    # document ends at every residue modulo 4
GRAM_LISTS = [[1, 2, 3, 4, 5], [3, 4, 5], [1, 2], [7], [2, 5, 5], [1, 2, 3, 4, 5, 6, 7]]


def build_corpus(table, grams):
    maxg = max(grams)
    rng = np.random.default_rng(47)
    docs, kinds = [], []

    def add(d, kind):
        docs.append(bytes(d))
        kinds.append(kind)

    # base: fast-path documents of odd lengths, a key of every length at slot 0..3 of their first lanes
    for i in range(48):
        n = max(maxg, 17 + (5 * i) % 23)
        d = bytearray(rng.choice(SA.ALPHABET, size=n).tobytes())
        k = KEY_OF[1 + i % 7]
        d[i % 4:i % 4 + len(k)] = k
        add(d[:n], "base")
    # lengths: the last window of every length a key ('a' * N), the next document goes on with 'a's
    for n in range(maxg, 265):
        d = bytearray(rng.choice(SA.ALPHABET, size=n).tobytes())
        d[max(0, n - 7):] = bytes([RUN]) * min(n, 7)
        add(d, "len%d" % n)
        add(bytes([RUN]) * 6 + bytes(rng.choice(SA.ALPHABET, size=int(rng.integers(maxg, 40)))), "after")
    # slots: the key of length N at slot k of SLOT_LANES
    for n, key in KEY_OF.items():
        for k in range(4):
            d = bytearray([FILL]) * 256
            for j in SLOT_LANES:
                d[4 * j + k:4 * j + k + n] = key
            add(d[:256], "slot%d.%d" % (n, k))
            add(bytes(rng.choice(SA.ALPHABET, size=maxg + 4 * n + k)), "after")
    # end: the key on the document's last bytes; the key one byte later, its last byte the next document's first
    for m in END_LENGTHS:
        for n, key in KEY_OF.items():
            add(bytes([FILL]) * (m - n) + key, "end%d" % n)
            add(bytes([FILL]) * (maxg + n), "after")
            add(bytes([FILL]) * (m - n + 1) + key[:-1], "poison%d" % n)
            add(key[-1:] + bytes([FILL]) * (maxg + 30), "after")
    # fallback: every window a key, more candidates than the queue holds (two lengths of 3..7 or more listed)
    for m in (256, 150):
        add(bytes([RUN]) * m, "dense%d" % m)
        add(SA.soup(rng, 90), "soup")
    for n in rng.integers(0, 300, size=60):
        add(SA.soup(rng, int(n)), "soup")
    data, off = encoding.pack(docs)
    return docs, kinds, data, off


class Case(SA.Case):
    def __init__(self, table, grams, n_values=1):
        self.table, self.grams, self.n_values = table, list(grams), n_values
        self.docs, self.kinds, self.data, self.off = build_corpus(table, grams)
        self.labels, self.scores = OC.Table(table, L).score(self.grams, self.data, self.off, want_scores=True,
                                                            nthreads=8)
        self.bloom = SA.bloom_of(table)
        self.lens = SA.fast_lengths(table, grams)

    def check_corpus(self):
        """Host-side: what the GPU run leans on, from the table and the text."""
        maxg = max(self.grams)
        off = [int(x) for x in self.off]
        fast = [i for i, d in enumerate(self.docs) if maxg <= len(d) <= 256]
        # one document per wave: the staged base is the start modulo 16
        assert {off[i] % 16 for i in fast if self.kinds[i] == "base"} == set(range(16))
        assert {off[i] % 4 for i in fast if self.kinds[i].startswith("slot")} == {0, 1, 2, 3}
        # several per wave (24 waves): bases inside a group, every residue modulo 4 and most modulo 16
        inner = set()
        for lo, hi in geometry.wave_ranges(len(self.docs), 2 * geometry.SCORE_WAVES):
            for g0, cnt, staged in geometry.groups(off, lo, hi):
                s0 = off[g0] & ~15
                inner |= {(off[i] - s0) % 16 for i in range(g0 + 1, g0 + cnt) if staged and i in set(fast)}
        assert len(inner) >= 12 and {r % 4 for r in inner} == {0, 1, 2, 3}, inner
        # every length, and its neighbour's bytes would complete longer keys
        assert [len(self.docs[i]) for i, k in enumerate(self.kinds) if k.startswith("len")] == list(range(maxg, 265))
        for i, k in enumerate(self.kinds):
            if k.startswith("len"):
                e = off[i + 1]
                assert all(bytes(self.data[e - g + 1:e + 1]) in self.table for g in self.lens)
            if k.startswith("poison"):
                n = int(k[6:])
                b = off[i + 1] - (n - 1)
                assert bytes(self.data[b:b + n]) == KEY_OF[n] and b + n == off[i + 1] + 1
            if k.startswith("end"):
                n = int(k[3:])
                assert bytes(self.data[off[i + 1] - n:off[i + 1]]) == KEY_OF[n]
        assert {off[i + 1] % 4 for i, k in enumerate(self.kinds) if k.startswith("poison")} == {0, 1, 2, 3}
        # the queue's overflow, where two listed lengths of 3..7 bytes can reach it
        if len(self.lens) >= 2:
            for i, k in enumerate(self.kinds):
                if k.startswith("dense"):
                    assert len(SA.candidates(self.bloom, self.lens, self.docs[i])) > QUEUE_CAP
        # the keys matter: an end key and its poison twin score differently, and labels vary
        if set(self.grams) & {1, 2, 3, 4, 5, 6, 7} and self.n_values == 1:
            ends = [i for i, k in enumerate(self.kinds) if k.startswith("end") and int(k[3:]) in self.grams]
            assert ends and all(self.scores[i].any() for i in ends)
        assert len(np.unique(self.labels)) >= 3


@pytest.mark.parametrize("grams", GRAM_LISTS, ids=str)
def test_count_mode(grams, monkeypatch):
    """Count mode, labels and (one value: count mode has scores) fp64 scores."""
    c = Case(SA.table_of([math.log(2.0)]), grams)
    c.check_corpus()
    c.run_all_grids(monkeypatch)


@pytest.mark.parametrize("grams", [[1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6, 7]], ids=str)
def test_class_mode(grams, monkeypatch):
    """Two row values: class mode (labels only; a near-tie document is replayed exactly)."""
    c = Case(SA.table_of([math.log(2.0), math.log(1.5)]), grams, n_values=2)
    assert len({v for r in c.table.values() for v in r if v}) == 2
    c.check_corpus()
    c.run_all_grids(monkeypatch)
