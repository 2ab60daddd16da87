"""languagedetection.utf8.decode -- the rule of include/ldgpu.h UTF-8 stated in
numpy, the checker that needs no GPU -- against CPython's codec: `host` must
equal "bytes.decode('utf-8') raises", and where it does not raise the units
must equal text.encode("utf-16-le") and the low bytes
encoding.score_bytes(text)."""
import os
import re

import numpy as np
import pytest

import utf8corpus
from conftest import ROOT
from languagedetection import _lib, encoding, utf8


@pytest.fixture(scope="module")
def docs():
    return utf8corpus.small_sequences()


def test_oracle_self_check(docs):
    """Exactly 128 * 128 + 30 * 64 of the 2-byte strings are well-formed."""
    two = docs[:65536]
    assert all(len(d) == 2 for d in two)
    assert sum(not utf8corpus.codec(d)[0] for d in two) == 128 * 128 + 30 * 64 == 18304


@pytest.mark.parametrize("low_bytes", [False, True])
def test_decode_matches_the_codec(docs, low_bytes):
    data, off = utf8.pack_utf8(docs)
    utf8corpus.check(utf8.decode(data, off, low_bytes), docs, low_bytes)


def test_every_document_on_its_own(docs):
    """Per document, not only as one packed corpus: flag, units and low bytes."""
    for d in docs[::97] + docs[-12:]:
        bad, units, low = utf8corpus.codec(d)
        out, off, host = utf8.decode(d, [0, len(d)])
        assert bool(host[0]) == bad
        if not bad:
            assert out.astype("<u2").tobytes() == units and off[1] == len(units) // 2
            assert utf8.decode(d, [0, len(d)], low_bytes=True)[0].tobytes() == low
        else:
            assert off[1] == 0 and len(out) == 0


def test_a_sequence_never_borrows_from_the_next_document():
    docs = [b"ab\xe2\x82", b"\xac", b"", b"\xf0\x9f\x98", b"", b"\x80z", b"ok\xef\xbb\xbf\x00"]
    data, off = utf8.pack_utf8(docs)
    out, out_off, host = utf8.decode(data, off)
    assert host.tolist() == [1, 1, 0, 1, 0, 1, 0]
    assert out.tolist() == [ord("o"), ord("k"), 0xFEFF, 0]
    utf8corpus.check((out, out_off, host), docs, False)


def test_offsets_from_the_middle_and_no_documents():
    data = np.frombuffer(b"\xa9xyz\xc3\xa9\xc3", dtype=np.uint8)
    out, out_off, host = utf8.decode(data, [1, 4, 6, 7])
    assert host.tolist() == [0, 0, 1] and out_off.tolist() == [0, 3, 4, 4] and out.tolist() == [120, 121, 122, 0xE9]
    out, out_off, host = utf8.decode(data, [3])
    assert len(out) == 0 and out_off.tolist() == [0] and len(host) == 0


def test_pack_utf8_and_step_constant():
    data, off = utf8.pack_utf8([b"ab", b"", b"\xc3\xa9"])
    assert off.tolist() == [0, 2, 2, 4] and data[:4].tobytes() == b"ab\xc3\xa9" and len(data) % 4 == 0
    assert utf8.STEP_BYTES == 256
    assert encoding.score_bytes("€") == utf8.decode(b"\xe2\x82\xac", [0, 3], True)[0].tobytes()


def test_library_exports_the_utf8_entry_points():
    """The four entry points are declared in include/ldgpu.h, bound by _lib and
    exported by both libraries (their names hold a digit, which the header
    scan of test_host.py does not match)."""
    src = open(os.path.join(ROOT, "include", "ldgpu.h")).read()
    declared = sorted(set(re.findall(r"\b(ldgpu_[a-z0-9_]*utf8[a-z0-9_]*)\s*\(", src)))
    assert declared == sorted(_lib.utf8_symbols()) == ["ldgpu_score_utf8", "ldgpu_score_utf8_device",
                                                       "ldgpu_utf8_decode", "ldgpu_utf8_decode_device"]
    for variant in ("product", "diag"):
        lib = _lib.load(variant=variant)
        for s in declared:
            assert getattr(lib, s).argtypes is not None
    assert int(re.search(r"#define LDGPU_UTF8_STEP_BYTES (\d+)", src).group(1)) == utf8.STEP_BYTES
