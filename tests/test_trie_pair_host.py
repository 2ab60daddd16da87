"""Host check of the LDS trie's pair form (trie_build_pair, csrc/ldgpu_trie.h; no
GPU).

tools/trie_pair_check.cpp -- a stand-alone program that includes the builder
header -- is compiled with AddressSanitizer and UBSan and run.  Over the random
path-uniform key sets of tools/trie_sum_check.cpp (the same generator, seed and
gram lists; a set whose largest W times its language count is above 63 must be
refused as it stands and is then checked with its languages folded to 63 / Wmax)
it checks, for every node, that the payload is 4 * (1 + l + L (W - 1)) with
(l, W) from the dictionary, that neither payload nor entry decreases along a
path, and -- slot by slot -- that base, check byte, dead entry and empty slots
are the path-sum image's.  The bound Wmax * L <= 63 from both sides: 21 x 3,
63 x 1 and 15 x 4 build and use their last slot (63, 63, 60); 16 x 4, 32 x 2
and 22 x 3 are refused and keep the path-sum form; a mixed-language path and a
language at or above L are refused.  The headline table (bench.py's config 2:
tests/golden/trie_config2_keys.bin, 20 languages) has the form with Wmax = 3:
44 distinct payloads, the largest slot 58 of 60."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(ROOT, "tests", "golden", "trie_config2_keys.bin")


@pytest.fixture(scope="module")
def trie_pair_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("trie_pair") / "trie_pair_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tools", "trie_pair_check.cpp")], check=True)
    return exe


def test_pair_builder_random_sets_bounds_and_config2(trie_pair_check):
    r = subprocess.run([trie_pair_check, KEYS], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trie_pair_check ok" in r.stdout
    # every alphabet at every size under every gram list, and at most the all-bytes sets of 10,000 keys too large
    sets = r"^%s: \d+ keys, L = (\d+), Wmax = (\d+), \d+ slots, \d+ with a payload, \d+ path nodes checked$"
    for name in ("12 letters", "a-z", "all bytes"):
        got = re.findall(sets % name, r.stdout, re.M)
        assert len(got) >= 9 - 3 * (name == "all bytes"), (name, got)
        assert all(int(l) * int(w) <= 63 for l, w in got), (name, got)
        assert {int(w) for _, w in got} >= {2, 4}, (name, got)   # (the weights above 1 are exercised)
    assert len(re.findall(r"too large", r.stdout)) <= 3
    for l, w in ((21, 3), (63, 1), (15, 4)):
        assert re.search(r"^bound L = %d, Wmax = %d: %d keys, L = %d, Wmax = %d, " % (l, w, w, l, w), r.stdout, re.M)
    for l, w in ((16, 4), (32, 2), (22, 3)):
        assert "refused: L = %d, Wmax = %d (%d slots)" % (l, w, l * w) in r.stdout
    m = re.search(r"^table: 10000 keys, L = 20, largest W (\d+), (\d+) distinct payloads, top slot (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    assert [int(x) for x in m.groups()] == [3, 44, 58]
