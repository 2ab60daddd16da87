"""Test corpora of the UTF-8 decoder (languagedetection.utf8, ldgpu_utf8_decode),
shared by the CPU and the GPU tests, and the codec oracle they are judged by:
CPython's ``bytes.decode("utf-8")`` accepts exactly the well-formed byte strings
of Unicode Table 3-7.
"""
import numpy as np

from languagedetection import encoding

VALID_SEQS = [b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80"]   # e-acute, euro sign, U+1F600


def small_sequences():
    """One document each: every 2-byte string; 3-byte strings of the leads with
    a rule of their own x every second byte x the third byte at the range
    edges; 4-byte strings likewise; every prefix of a valid 2-, 3- and 4-byte
    sequence."""
    docs = [bytes([a, b]) for a in range(256) for b in range(256)]
    edge = (0x7F, 0x80, 0xBF, 0xC0)
    docs += [bytes([a, b, c]) for a in (0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF) for b in range(256) for c in edge]
    docs += [bytes([a, b, c, d]) for a in (0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xF8, 0xFF) for b in range(256)
             for c in edge for d in edge]
    docs += [s[:k] for s in VALID_SEQS for k in range(len(s) + 1)]
    return docs


def codec(doc):
    """The oracle: (ill-formed, UTF-16 units as bytes, SCORE bytes) of one document."""
    try:
        text = bytes(doc).decode("utf-8")
    except UnicodeDecodeError:
        return True, b"", b""
    return False, text.encode("utf-16-le"), encoding.score_bytes(text)


def expected(docs, low_bytes):
    """(out bytes, out_offsets int64, host uint8) the codec gives for `docs`:
    offsets in units (or, low_bytes, in bytes)."""
    parts, host = [], np.zeros(len(docs), dtype=np.uint8)
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    for i, d in enumerate(docs):
        bad, units, low = codec(d)
        host[i] = bad
        parts.append(low if low_bytes else units)
        off[i + 1] = off[i] + (len(low) if low_bytes else len(units) // 2)
    return b"".join(parts), off, host


def check(got, docs, low_bytes):
    """`got` = (out, out_offsets, host) of a decoder equals the codec's, exactly."""
    out, off, host = got
    want_out, want_off, want_host = expected(docs, low_bytes)
    assert np.array_equal(np.asarray(host, dtype=np.uint8), want_host)
    assert np.array_equal(np.asarray(off, dtype=np.int64), want_off)
    n = int(want_off[-1])
    assert np.asarray(out)[:n].astype("<u2" if not low_bytes else np.uint8).tobytes() == want_out
