"""languagedetection.spans -- the span and run rules behind ldgpu_score_spans,
checked on the CPU against brute force, and ldgpu_span_offsets (host arithmetic
of the library: no context, no GPU) against spans.span_offsets."""
import ctypes

import numpy as np
import pytest

from languagedetection import _lib, spans


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib_span_offsets(off, width, stride, lib=None):
    lib = lib or _lib.load()
    off = np.ascontiguousarray(off, dtype=np.int64)
    out = np.full(len(off), -7, dtype=np.int64)
    rc = lib.ldgpu_span_offsets(_ptr(off), len(off) - 1, width, stride, _ptr(out))
    return rc, out


def test_span_bounds_against_brute_force():
    for width in range(1, 10):
        for stride in range(1, width + 1):
            for length in range(0, 3 * width + 3):
                b = spans.span_bounds(length, width, stride)
                n = len(b)
                # the count formula
                want = 1 if length <= width else 1 + -(-(length - width) // stride)
                assert n == want == spans.span_count(length, width, stride), (width, stride, length)
                # brute force: windows every `stride` until one reaches the end
                brute, s = [], 0
                while True:
                    brute.append((s, min(s + width, length)))
                    if s + width >= length:
                        break
                    s += stride
                assert b == brute, (width, stride, length)
                covered = set()
                for j, (a, e) in enumerate(b):
                    assert a == j * stride
                    assert e - a <= width
                    assert e > a or (n == 1 and length == 0)
                    covered.update(range(a, e))
                assert b[-1][1] == length
                assert covered == set(range(length))


def test_span_offsets_and_materialise_follow_span_bounds():
    rng = np.random.default_rng(5)
    for width, stride in ((1, 1), (3, 1), (4, 4), (5, 2), (9, 7)):
        lens = rng.integers(0, 3 * width + 3, size=60)
        lens[[0, 1, 2, 30, 31, 59]] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
        soff = spans.span_offsets(off, width, stride)
        assert soff[0] == 0 and soff.dtype == np.int64
        assert np.diff(soff).tolist() == [len(spans.span_bounds(int(x), width, stride)) for x in lens]
        sd, so = spans.materialise(data, off, width, stride)
        assert len(so) == soff[-1] + 1 and so[0] == 0 and len(sd) % 4 == 0 and len(sd) >= so[-1] + 4
        g = 0
        for d, ln in enumerate(lens):
            for a, e in spans.span_bounds(int(ln), width, stride):
                assert sd[so[g]:so[g + 1]].tobytes() == data[off[d] + a:off[d] + e].tobytes()
                g += 1
        assert g == soff[-1]
    # a nonzero first offset, and no document at all
    assert spans.span_offsets([5, 5, 12], 3, 2).tolist() == [0, 1, 4]
    assert spans.span_offsets([0], 3, 2).tolist() == [0]
    sd, so = spans.materialise(np.zeros(0, np.uint8), [0], 3, 2)
    assert so.tolist() == [0]


def test_library_span_offsets_equal_the_python_rule():
    rng = np.random.default_rng(6)
    for variant in ("product", "diag"):
        lib = _lib.load(variant=variant)
        for width, stride in ((1, 1), (3, 1), (4, 4), (5, 2), (64, 32), (257, 100), (300, 7), ((1 << 28) - 1, 1)):
            lens = rng.integers(0, 1500, size=400)
            lens[rng.random(400) < 0.2] = 0
            lens[:40] = 0                     # runs of empty documents, at both ends too
            lens[200:230] = 0
            lens[-25:] = 0
            off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
            rc, out = lib_span_offsets(off, width, stride, lib)
            assert rc == _lib.LDGPU_OK
            assert np.array_equal(out, spans.span_offsets(off, width, stride))
        rc, out = lib_span_offsets([0], 4, 2, lib)
        assert rc == _lib.LDGPU_OK and out.tolist() == [0]
        # a document far beyond 2^28 bytes: only spans are limited
        rc, out = lib_span_offsets([0, 1 << 40], 1 << 20, 1 << 19, lib)
        assert rc == _lib.LDGPU_OK and out.tolist() == [0, (1 << 21) - 1]


@pytest.mark.parametrize("width,stride,code", [(0, 1, _lib.LDGPU_EINVAL), (-3, 1, _lib.LDGPU_EINVAL),
                                               (4, 0, _lib.LDGPU_EINVAL), (4, -1, _lib.LDGPU_EINVAL),
                                               (4, 5, _lib.LDGPU_EINVAL), (1 << 28, 1, _lib.LDGPU_EUNSUPPORTED),
                                               (2147483647, 7, _lib.LDGPU_EUNSUPPORTED)])
def test_invalid_width_and_stride(width, stride, code):
    lib = _lib.load()
    rc, out = lib_span_offsets([0, 10, 20], width, stride)
    assert rc == code and (out == -7).all()
    assert str(width).encode() in lib.ldgpu_last_error() or str(stride).encode() in lib.ldgpu_last_error()
    exc = ValueError if code == _lib.LDGPU_EINVAL else NotImplementedError
    with pytest.raises(exc):
        _lib.check(rc)
    with pytest.raises(exc):
        spans.span_offsets([0, 10, 20], width, stride)
    with pytest.raises(exc):
        spans.span_bounds(10, width, stride)
    with pytest.raises(exc):
        spans.runs(10, [0], width, stride)


def test_invalid_offsets():
    lib = _lib.load()
    rc, out = lib_span_offsets([0, 10, 9], 4, 2)
    assert rc == _lib.LDGPU_EINVAL and b"decrease" in lib.ldgpu_last_error() and (out == -7).all()
    rc, out = lib_span_offsets([-1, 10], 4, 2)
    assert rc == _lib.LDGPU_EINVAL
    off = np.array([0, 4], dtype=np.int64)
    assert lib.ldgpu_span_offsets(_ptr(off), -1, 4, 2, _ptr(off)) == _lib.LDGPU_EINVAL
    assert lib.ldgpu_span_offsets(None, 1, 4, 2, _ptr(off)) == _lib.LDGPU_EINVAL
    assert lib.ldgpu_span_offsets(_ptr(off), 1, 4, 2, None) == _lib.LDGPU_EINVAL
    with pytest.raises(ValueError):
        spans.span_offsets([0, 10, 9], 4, 2)


def test_runs_hand_cases():
    # a single span owns the whole document
    assert spans.runs(5, [3], 8, 4) == [(0, 5, 3)]
    assert spans.runs(8, [2], 8, 4) == [(0, 8, 2)]
    # all labels equal: one run
    assert spans.runs(20, [1, 1, 1, 1], 8, 4) == [(0, 20, 1)]
    # alternating labels: span j owns [4 j, 4 j + 4), the last one to the end
    assert spans.runs(20, [0, 1, 0, 1], 8, 4) == [(0, 4, 0), (4, 8, 1), (8, 12, 0), (12, 20, 1)]
    # an empty document has one (empty) span and no run
    assert spans.runs(0, [0], 8, 4) == []
    # the last span owns the remainder: 21 bytes, spans at 0, 4, 8, 12, 16
    assert spans.span_count(21, 8, 4) == 5
    assert spans.runs(21, [0, 0, 1, 1, 2], 8, 4) == [(0, 8, 0), (8, 16, 1), (16, 21, 2)]
    # ... also a short one: 17 bytes, the last span [12, 17) owns [12, 17)
    assert spans.runs(17, [0, 0, 0, 5], 8, 4) == [(0, 12, 0), (12, 17, 5)]
    # stride == width: the spans themselves
    assert spans.runs(10, [7, 8, 7], 4, 4) == [(0, 4, 7), (4, 8, 8), (8, 10, 7)]
    # the runs of a document always tile [0, length)
    rng = np.random.default_rng(9)
    for _ in range(300):
        width = int(rng.integers(1, 10))
        stride = int(rng.integers(1, width + 1))
        length = int(rng.integers(0, 40))
        labels = rng.integers(0, 3, size=spans.span_count(length, width, stride)).tolist()
        r = spans.runs(length, labels, width, stride)
        assert [a for a, _, _ in r] == [0][:len(r)] + [b for _, b, _ in r][:-1]
        assert (r[-1][1] == length) if length else r == []
        assert all(x[2] != y[2] for x, y in zip(r, r[1:]))
    with pytest.raises(ValueError):
        spans.runs(20, [0, 1], 8, 4)
