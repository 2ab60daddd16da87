"""Host check of the LDS trie's path-sum form (trie_build_sum, csrc/ldgpu_trie.h;
no GPU).

tools/trie_sum_check.cpp -- a stand-alone program that includes the builder
header -- is compiled with AddressSanitizer and UBSan and run.  It builds the
path-sum image of random path-uniform key sets of 100 to 10,000 keys over 12
letters, a-z and all 256 bytes (every key has the language of its shortest
prefix that is a key) under the gram lists [1, 2, 3, 4], [2, 4] and
[1, 2, 3, 3], and checks each exhaustively: for every node and each of its 256
byte extensions the walk equals dictionary membership, the payload equals
(language, W) computed from the dictionary, payloads grow strictly along a path
wherever W does, the packing is the other form's, and the dead state and the
empty slots carry payload 0 and never match.  A mixed-language path, language
63 and a chain of W = 6 are refused; the chain with W = 4 and language 62 with
W = 4 (payload 255) build.  The headline table (bench.py's config 2:
tests/golden/trie_config2_keys.bin) with every multiplicity 1 must have the
form: 11,456 nodes, as many words as trie_build gives, largest W 3 and 44
distinct non-zero payloads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(ROOT, "tests", "golden", "trie_config2_keys.bin")


@pytest.fixture(scope="module")
def trie_sum_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("trie_sum") / "trie_sum_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tools", "trie_sum_check.cpp")], check=True)
    return exe


def test_path_sum_builder_exhaustive_and_config2_has_the_form(trie_sum_check):
    r = subprocess.run([trie_sum_check, KEYS], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trie_sum_check ok" in r.stdout
    # every alphabet at every size under every gram list, and at most the all-bytes sets of 10,000 keys too large
    for name in ("12 letters", "a-z", "all bytes"):
        assert len(re.findall(r"^%s: \d+ keys, \d+ nodes in \d+ slots$" % name, r.stdout, re.M)) >= 9 - 3 * (name == "all bytes")
    assert len(re.findall(r"too large", r.stdout)) <= 3
    m = re.search(r"table: 10000 keys, (\d+) nodes, image (\d+) words \(the other form (\d+)\), largest W (\d+), "
                  r"(\d+) distinct payloads", r.stdout)
    assert m, r.stdout
    nodes, words, other, max_w, payloads = (int(x) for x in m.groups())
    assert nodes == 11456
    assert words == other and words * 4 == 50784
    assert max_w == 3
    assert payloads == 44
