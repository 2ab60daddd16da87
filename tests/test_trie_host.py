"""Host check of the LDS trie builder (csrc/ldgpu_trie.h; no GPU).

tools/trie_check.cpp -- a stand-alone program that includes the builder header
-- is compiled with AddressSanitizer and UBSan and run.  It builds tries for
random key sets of 100 to 12,000 keys over four alphabets, chains with a
language per depth, keys whose prefixes are no keys and 0x00 / 0xff keys, and
checks each exhaustively: for every node and each of its 256 byte extensions the
walk equals dictionary membership and language, and neither the dead state nor
an empty slot ever matches.  It then builds the headline table (bench.py's
config 2: tests/golden/trie_config2_keys.bin, records of key u32 LE, length u8,
language u8 -- the 10,000 rows of bench.build_table's generator and seeds under
bench.topk_table_from_counts' rule; tools/gen_trie_fixture.py writes it again,
about 20 s of numpy, and must be run when the benchmark's table changes) and
asserts that it is eligible for two workgroups per CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(ROOT, "tests", "golden", "trie_config2_keys.bin")


@pytest.fixture(scope="module")
def trie_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("trie") / "trie_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tools", "trie_check.cpp")], check=True)
    return exe


def test_fixture_is_config2s_table():
    rec = open(KEYS, "rb").read()
    assert len(rec) == 6 * 10000
    lens = [rec[i + 4] for i in range(0, len(rec), 6)]
    assert [lens.count(n) for n in (1, 2, 3, 4)] == [13, 703, 6468, 2816]
    assert all(rec[i + 5] < 20 for i in range(0, len(rec), 6))  # one language each


def test_builder_exhaustive_and_config2_eligible(trie_check):
    r = subprocess.run([trie_check, KEYS], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trie_check ok" in r.stdout
    m = re.search(r"table: 10000 keys, (\d+) nodes, \d+ rows, image (\d+) B of (\d+) B .* LDS per workgroup (\d+) B",
                  r.stdout)
    assert m, r.stdout
    nodes, image, budget, lds = (int(x) for x in m.groups())
    assert nodes == 11456
    assert image <= budget and lds <= 81920
