"""Thin owners of libldgpu.so handles: device gram tables (SCORE) and device
count tables (FIT).  Everything here calls straight into the HIP library."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .encoding import pack, pack_table


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _grams(gram_lengths: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(gram_lengths), dtype=np.int32))


def _out(out: Optional[np.ndarray], shape: Tuple[int, ...], dtype) -> np.ndarray:
    """An output array: the caller's `out`, which must fit, or a new one."""
    if out is None:
        return np.zeros(shape, dtype=dtype)
    assert out.dtype == dtype and out.shape == shape and out.flags.c_contiguous
    return out


class _Owner:
    lib = None

    def _check(self, rc: int) -> None:
        _lib.check(rc, self.lib)


class PinnedArray(_Owner):
    """Page-locked host memory (ldgpu_host_alloc) viewed as a numpy array:
    host-buffer scoring copies from / to it directly, with no staging copy."""

    def __init__(self, shape, dtype, device: Optional[int] = None):
        self.lib = _lib.load()
        self.ctx = _lib.context(device)
        dt = np.dtype(dtype)
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) * dt.itemsize
        p = ctypes.c_void_p()
        self._check(self.lib.ldgpu_host_alloc(self.ctx, n, ctypes.byref(p)))
        self.p = p.value
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(self.p)
        self.array = np.frombuffer(buf, dtype=np.uint8, count=n).view(dt).reshape(shape)

    def close(self):
        if getattr(self, "p", None):
            self.array = None
            self.lib.ldgpu_host_free(self.ctx, ctypes.c_void_p(self.p))
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceModel(_Owner):
    """A gram -> probability-row table resident on one GPU
    (LanguageDetectorModel's broadcast table, LanguageDetectorModel.scala:222)."""

    def __init__(self, table: Dict, n_langs: int, gram_lengths: Sequence[int], device: Optional[int] = None,
                 variant: str = "product"):
        """variant="diag": the diagnostics library (tests of alternative paths)."""
        self.lib = _lib.load(variant=variant)
        self.ctx = _lib.context(device, variant)
        self.L = int(n_langs)
        self.gram_lengths = list(gram_lengths)
        kb, ko, rows, ok = pack_table(table, self.L)
        g = _grams(gram_lengths)
        out = ctypes.c_void_p()
        self._check(self.lib.ldgpu_model_create(self.ctx, len(ko) - 1, _ptr(kb), _ptr(ko), _ptr(rows), _ptr(ok),
                                               self.L, _ptr(g), len(g), ctypes.byref(out)))
        self.h = out.value

    @classmethod
    def from_masks(cls, key_bytes: np.ndarray, key_offsets: np.ndarray, masks: np.ndarray, vals: np.ndarray,
                   n_langs: int, gram_lengths: Sequence[int], device: Optional[int] = None,
                   variant: str = "product") -> "DeviceModel":
        """A mask-form table (row i = vals[i] at the languages set in masks[i])
        as packed arrays, e.g. DeviceCounts.fit_table_masks (ldgpu_model_create_masks)."""
        self = cls.__new__(cls)
        self.lib = _lib.load(variant=variant)
        self.ctx = _lib.context(device, variant)
        self.L = int(n_langs)
        self.gram_lengths = list(gram_lengths)
        kb = np.ascontiguousarray(key_bytes, dtype=np.uint8)
        ko = np.ascontiguousarray(key_offsets, dtype=np.int64)
        mk = np.ascontiguousarray(masks, dtype=np.uint64)
        vv = np.ascontiguousarray(vals, dtype=np.float64)
        assert mk.shape == (len(ko) - 1, (self.L + 63) // 64) and vv.shape == (len(ko) - 1,)
        g = _grams(gram_lengths)
        out = ctypes.c_void_p()
        self._check(self.lib.ldgpu_model_create_masks(self.ctx, len(ko) - 1, _ptr(kb), _ptr(ko), _ptr(mk), _ptr(vv),
                                                     self.L, _ptr(g), len(g), ctypes.byref(out)))
        self.h = out.value
        return self

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldgpu_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> Dict[str, int]:
        mode = ctypes.c_int32()
        vals = [ctypes.c_int64() for _ in range(4)]
        self._check(self.lib.ldgpu_model_info(self.h, ctypes.byref(mode), *[ctypes.byref(v) for v in vals]))
        flags = ctypes.c_int32()
        self._check(self.lib.ldgpu_model_layout(self.h, ctypes.byref(flags)))
        return {"mode": mode.value, "n_keys": vals[0].value, "table_slots": vals[1].value,
                "filter_bits": vals[2].value, "device_bytes": vals[3].value,
                "layout": sorted(k for k, b in _lib.LAYOUT_FLAGS.items() if flags.value & b)}

    def _score(self, fn, data, offsets, want_scores, out):
        """score / score_utf8 through the C entry point `fn`."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        labels = _out(out, (max(n, 0),), np.int32)
        scores = np.zeros((max(n, 0), self.L), dtype=np.float64) if want_scores else None
        self._check(fn(self.h, _ptr(data), _ptr(offsets), n, _ptr(labels), _ptr(scores)))
        return labels, scores

    def _score_topk(self, fn, data, offsets, k, want_scores, out_labels, out_scores):
        """score_topk / score_topk_utf8 through the C entry point `fn`."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n, k = max(len(offsets) - 1, 0), int(k)
        shape = (n, max(k, 0))
        labels = _out(out_labels, shape, np.int32)
        scores = _out(out_scores, shape, np.float64) if want_scores else None
        self._check(fn(self.h, _ptr(data), _ptr(offsets), len(offsets) - 1, k, _ptr(labels), _ptr(scores)))
        return labels, scores

    def _device_call(self, fn, stream: Optional[int], *args) -> None:
        """fn(*args, stream) on device pointers given as integers (0 = NULL:
        the entry points take them as void*); `stream` None = the context's."""
        self._check(fn(*args, self.stream() if stream is None else stream))

    def score(self, data: np.ndarray, offsets: np.ndarray, want_scores: bool = False,
              out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Host buffers -> (labels int32[n], scores fp64[n, L] or None);
        `out` (e.g. a PinnedArray's array) receives the labels."""
        return self._score(self.lib.ldgpu_score, data, offsets, want_scores, out)

    def stream(self) -> int:
        """The context's hipStream_t."""
        return self.lib.ldgpu_ctx_stream(self.ctx) or 0

    def score_device(self, d_bytes: int, n_bytes: int, d_offsets: int, n_docs: int, d_labels: int,
                     d_scores: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers (e.g. torch tensors' data_ptr()) -> labels in place,
        async on `stream` (a hipStream_t; 0 = the null stream, None = the
        context's stream)."""
        self._device_call(self.lib.ldgpu_score_device, stream, self.h, d_bytes, n_bytes, d_offsets, n_docs, d_labels,
                          d_scores)

    def score_topk(self, data: np.ndarray, offsets: np.ndarray, k: int, want_scores: bool = True,
                   out_labels: Optional[np.ndarray] = None, out_scores: Optional[np.ndarray] = None
                   ) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Host buffers -> (the k best languages in order int32[n, k], their
        scores fp64[n, k] or None), selected on the device (ldgpu_score_topk;
        the order: languagedetection.topk).  `out_labels` / `out_scores` (e.g.
        PinnedArray arrays) receive the results."""
        return self._score_topk(self.lib.ldgpu_score_topk, data, offsets, k, want_scores, out_labels, out_scores)

    def score_topk_device(self, d_bytes: int, n_bytes: int, d_offsets: int, n_docs: int, k: int, d_top_labels: int,
                          d_top_scores: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers -> the [n_docs, k] labels (and scores) in place,
        async on `stream` as score_device (ldgpu_score_topk_device)."""
        self._device_call(self.lib.ldgpu_score_topk_device, stream, self.h, d_bytes, n_bytes, d_offsets, n_docs,
                          int(k), d_top_labels, d_top_scores)

    # UTF-8 documents (an addition; the rule: languagedetection.utf8)
    def score_utf8(self, data: np.ndarray, offsets: np.ndarray, want_scores: bool = False,
                   out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Host buffers of UTF-8 documents -> (labels int32[n], scores fp64[n,
        L] or None) as score gives for their SCORE encoding, decoded on the
        device (ldgpu_score_utf8); an ill-formed document gets label -1 and an
        empty document's score row.  `out` receives the labels."""
        return self._score(self.lib.ldgpu_score_utf8, data, offsets, want_scores, out)

    def score_utf8_device(self, d_utf8: int, n_bytes: int, d_offsets: int, n_docs: int, d_labels: int,
                          d_scores: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers to UTF-8 documents -> labels (and scores) in place,
        async on `stream` as score_device (ldgpu_score_utf8_device)."""
        self._device_call(self.lib.ldgpu_score_utf8_device, stream, self.h, d_utf8, n_bytes, d_offsets, n_docs,
                          d_labels, d_scores)

    # Span scoring (an addition; the rule: languagedetection.spans)
    def span_offsets(self, offsets: np.ndarray, width: int, stride: int) -> np.ndarray:
        """int64[n_docs + 1]: every document's first span (ldgpu_span_offsets: host arithmetic)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.zeros(max(len(offsets), 1), dtype=np.int64)
        self._check(self.lib.ldgpu_span_offsets(_ptr(offsets), len(offsets) - 1, int(width), int(stride), _ptr(out)))
        return out

    def span_offsets_device(self, d_offsets: int, n_docs: int, width: int, stride: int, d_span_offsets: int,
                            stream: Optional[int] = None) -> None:
        """Device pointers -> d_span_offsets int64[n_docs + 1] in place, async
        on `stream` as score_device (ldgpu_span_offsets_device)."""
        self._device_call(self.lib.ldgpu_span_offsets_device, stream, self.ctx, d_offsets, n_docs, int(width),
                          int(stride), d_span_offsets)

    def score_spans(self, data: np.ndarray, offsets: np.ndarray, width: int, stride: int, want_scores: bool = False,
                    out_labels: Optional[np.ndarray] = None, out_scores: Optional[np.ndarray] = None
                    ) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
        """Host buffers -> (labels int32[n_spans], scores fp64[n_spans, L] or
        None, span_offsets int64[n_docs + 1]): every span of `width` bytes
        every `stride` bytes scored as a document of its own
        (ldgpu_score_spans).  `out_labels` / `out_scores` (e.g. PinnedArray
        arrays) receive the results."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        soff = self.span_offsets(offsets, width, stride)
        n = int(soff[-1])
        labels = _out(out_labels, (n,), np.int32)
        scores = _out(out_scores, (n, self.L), np.float64) if want_scores else None
        self._check(self.lib.ldgpu_score_spans(self.h, _ptr(data), _ptr(offsets), len(offsets) - 1, int(width),
                                               int(stride), _ptr(labels), _ptr(scores)))
        return labels, scores, soff

    def score_spans_device(self, d_bytes: int, n_bytes: int, d_offsets: int, n_docs: int, width: int, stride: int,
                           d_span_offsets: int, n_spans: int, d_labels: int, d_scores: int = 0,
                           stream: Optional[int] = None) -> None:
        """Device pointers -> the [n_spans] labels (and [n_spans, L] scores) in
        place, async on `stream` as score_device (ldgpu_score_spans_device)."""
        self._device_call(self.lib.ldgpu_score_spans_device, stream, self.h, d_bytes, n_bytes, d_offsets, n_docs,
                          int(width), int(stride), d_span_offsets, n_spans, d_labels, d_scores)

    # Smoothed span labels (an addition; the rule: languagedetection.segments)
    def score_segments(self, data: np.ndarray, offsets: np.ndarray, width: int, stride: int, penalty: float,
                       out_labels: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers -> (labels int32[n_spans], span_offsets int64[n_docs +
        1]): the span labels of score_spans smoothed on the device by a best
        path with `penalty` (score units, >= 0, inf allowed) per language
        change (ldgpu_score_segments).  `out_labels` (e.g. a PinnedArray's
        array) receives the labels."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        soff = self.span_offsets(offsets, width, stride)
        labels = _out(out_labels, (int(soff[-1]),), np.int32)
        self._check(self.lib.ldgpu_score_segments(self.h, _ptr(data), _ptr(offsets), len(offsets) - 1, int(width),
                                                  int(stride), float(penalty), _ptr(labels)))
        return labels, soff

    def score_segments_device(self, d_bytes: int, n_bytes: int, d_offsets: int, n_docs: int, width: int, stride: int,
                              penalty: float, d_span_offsets: int, n_spans: int, d_labels: int,
                              stream: Optional[int] = None) -> None:
        """Device pointers -> the [n_spans] smoothed labels in place, async on
        `stream` as score_device (ldgpu_score_segments_device)."""
        self._device_call(self.lib.ldgpu_score_segments_device, stream, self.h, d_bytes, n_bytes, d_offsets, n_docs,
                          int(width), int(stride), float(penalty), d_span_offsets, n_spans, d_labels)

    # Top-k, spans and segments of UTF-8 documents (an addition; the rule:
    # languagedetection.utf8)
    def span_offsets_utf8(self, data: np.ndarray, offsets: np.ndarray, width: int, stride: int
                          ) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers of UTF-8 documents -> (span_offsets int64[n_docs + 1],
        units int64[n_docs]: the document's UTF-16 unit count, -1 = ill-formed),
        from the device decoder's length pass (ldgpu_span_offsets_utf)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        soff = np.zeros(max(n, 0) + 1, dtype=np.int64)
        units = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.ldgpu_span_offsets_utf(self.ctx, _ptr(data), _ptr(offsets), n, int(width), int(stride),
                                                    _ptr(soff), _ptr(units)))
        return soff, units[:max(n, 0)]

    def span_offsets_utf8_device(self, d_utf8: int, d_offsets: int, n_docs: int, width: int, stride: int,
                                 d_span_offsets: int, d_units: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers -> d_span_offsets int64[n_docs + 1] (and d_units
        int64[n_docs]) in place, async on `stream` as score_device
        (ldgpu_span_offsets_utf_device)."""
        self._device_call(self.lib.ldgpu_span_offsets_utf_device, stream, self.ctx, d_utf8, d_offsets, n_docs,
                          int(width), int(stride), d_span_offsets, d_units)

    def score_topk_utf8(self, data: np.ndarray, offsets: np.ndarray, k: int, want_scores: bool = True,
                        out_labels: Optional[np.ndarray] = None, out_scores: Optional[np.ndarray] = None
                        ) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """score_topk over host buffers of UTF-8 documents, decoded on the
        device (ldgpu_score_topk_utf); an ill-formed document's row is -1 in
        every label and 0.0 in every score."""
        return self._score_topk(self.lib.ldgpu_score_topk_utf, data, offsets, k, want_scores, out_labels, out_scores)

    def score_topk_utf8_device(self, d_utf8: int, n_bytes: int, d_offsets: int, n_docs: int, k: int,
                               d_top_labels: int, d_top_scores: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers to UTF-8 documents -> the [n_docs, k] labels (and
        scores) in place, async on `stream` (ldgpu_score_topk_utf_device)."""
        self._device_call(self.lib.ldgpu_score_topk_utf_device, stream, self.h, d_utf8, n_bytes, d_offsets, n_docs,
                          int(k), d_top_labels, d_top_scores)

    def _utf8_spans(self, data, offsets, width, stride, span_offsets):
        """(data, offsets, span offsets) of a UTF-8 span / segment call:
        `span_offsets` is span_offsets_utf8's output when the caller has it."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        soff = (self.span_offsets_utf8(data, offsets, width, stride)[0] if span_offsets is None
                else np.ascontiguousarray(span_offsets, dtype=np.int64))
        return data, offsets, soff

    def score_spans_utf8(self, data: np.ndarray, offsets: np.ndarray, width: int, stride: int,
                         want_scores: bool = False, want_starts: bool = True,
                         span_offsets: Optional[np.ndarray] = None, out_labels: Optional[np.ndarray] = None,
                         out_scores: Optional[np.ndarray] = None, out_starts: Optional[np.ndarray] = None
                         ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray], np.ndarray]:
        """Host buffers of UTF-8 documents -> (labels int32[n_spans], scores
        fp64[n_spans, L] or None, starts int64[n_spans] or None, span_offsets
        int64[n_docs + 1]): score_spans of the documents' SCORE encoding, plus
        every span's start as a byte index into its document; an ill-formed
        document's single span gets -1 (ldgpu_score_spans_utf).  `span_offsets`
        is span_offsets_utf8's output when the caller has it already; the
        `out_*` arrays (e.g. PinnedArray arrays) receive the results."""
        data, offsets, soff = self._utf8_spans(data, offsets, width, stride, span_offsets)
        n = int(soff[-1])
        labels = _out(out_labels, (n,), np.int32)
        scores = _out(out_scores, (n, self.L), np.float64) if want_scores else None
        starts = _out(out_starts, (n,), np.int64) if want_starts else None
        self._check(self.lib.ldgpu_score_spans_utf(self.h, _ptr(data), _ptr(offsets), len(offsets) - 1, int(width),
                                                   int(stride), _ptr(soff), _ptr(labels), _ptr(scores), _ptr(starts)))
        return labels, scores, starts, soff

    def score_spans_utf8_device(self, d_utf8: int, n_bytes: int, d_offsets: int, n_docs: int, width: int, stride: int,
                                d_span_offsets: int, n_spans: int, d_labels: int, d_scores: int = 0,
                                d_starts: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers to UTF-8 documents -> the [n_spans] labels (and
        [n_spans, L] scores, [n_spans] starts) in place, async on `stream`
        (ldgpu_score_spans_utf_device)."""
        self._device_call(self.lib.ldgpu_score_spans_utf_device, stream, self.h, d_utf8, n_bytes, d_offsets, n_docs,
                          int(width), int(stride), d_span_offsets, n_spans, d_labels, d_scores, d_starts)

    def score_segments_utf8(self, data: np.ndarray, offsets: np.ndarray, width: int, stride: int, penalty: float,
                            want_starts: bool = True, span_offsets: Optional[np.ndarray] = None,
                            out_labels: Optional[np.ndarray] = None, out_starts: Optional[np.ndarray] = None
                            ) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
        """Host buffers of UTF-8 documents -> (labels int32[n_spans], starts
        int64[n_spans] or None, span_offsets int64[n_docs + 1]): score_segments
        of the documents' SCORE encoding with the spans' byte starts; an
        ill-formed document's single span gets -1 (ldgpu_score_segments_utf)."""
        data, offsets, soff = self._utf8_spans(data, offsets, width, stride, span_offsets)
        n = int(soff[-1])
        labels = _out(out_labels, (n,), np.int32)
        starts = _out(out_starts, (n,), np.int64) if want_starts else None
        self._check(self.lib.ldgpu_score_segments_utf(self.h, _ptr(data), _ptr(offsets), len(offsets) - 1, int(width),
                                                      int(stride), float(penalty), _ptr(soff), _ptr(labels),
                                                      _ptr(starts)))
        return labels, starts, soff

    def score_segments_utf8_device(self, d_utf8: int, n_bytes: int, d_offsets: int, n_docs: int, width: int,
                                   stride: int, penalty: float, d_span_offsets: int, n_spans: int, d_labels: int,
                                   d_starts: int = 0, stream: Optional[int] = None) -> None:
        """Device pointers to UTF-8 documents -> the [n_spans] smoothed labels
        (and starts) in place, async on `stream` (ldgpu_score_segments_utf_device)."""
        self._device_call(self.lib.ldgpu_score_segments_utf_device, stream, self.h, d_utf8, n_bytes, d_offsets,
                          n_docs, int(width), int(stride), float(penalty), d_span_offsets, n_spans, d_labels, d_starts)


class DeviceCounts(_Owner):
    """A (gram, language) -> count table on one GPU (computeGrams + reduceGrams)."""

    def __init__(self, n_langs: int, gram_lengths: Sequence[int], capacity_hint: int = 0,
                 device: Optional[int] = None, variant: str = "product"):
        """variant="diag": the diagnostics library (tests of alternative paths)."""
        self.lib = _lib.load(variant=variant)
        self.ctx = _lib.context(device, variant)
        self.device = device
        self.variant = variant
        self.L = int(n_langs)
        self.gram_lengths = list(gram_lengths)
        g = _grams(gram_lengths)
        out = ctypes.c_void_p()
        self._check(self.lib.ldgpu_counts_create(self.ctx, self.L, _ptr(g), len(g), int(capacity_hint),
                                                ctypes.byref(out)))
        self.h = out.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldgpu_counts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self, data: np.ndarray, offsets: np.ndarray, doc_lang: np.ndarray) -> None:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        doc_lang = np.ascontiguousarray(doc_lang, dtype=np.int32)
        self._check(self.lib.ldgpu_count(self.h, _ptr(data), _ptr(offsets), _ptr(doc_lang), len(offsets) - 1))

    def count_device(self, d_bytes: int, n_bytes: int, d_offsets: int, d_doc_lang: int, n_docs: int,
                     stream: Optional[int] = None) -> None:
        st = (self.lib.ldgpu_ctx_stream(self.ctx) or 0) if stream is None else stream
        self._check(self.lib.ldgpu_count_device(self.h, ctypes.c_void_p(d_bytes), n_bytes, ctypes.c_void_p(d_offsets),
                                               ctypes.c_void_p(d_doc_lang), n_docs,
                                               ctypes.c_void_p(st) if st else None))

    def size(self) -> int:
        n = ctypes.c_int64()
        self._check(self.lib.ldgpu_counts_size(self.h, ctypes.byref(n), None))
        return n.value

    def stats(self) -> Dict[str, int]:
        """Distinct grams, distinct (gram, language) pairs, total count."""
        v = [ctypes.c_int64() for _ in range(3)]
        self._check(self.lib.ldgpu_counts_stats(self.h, *[ctypes.byref(x) for x in v]))
        return {"grams": v[0].value, "pairs": v[1].value, "total": v[2].value}

    def export_arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(key_bytes uint8, key_offsets int64 [n+1], counts int64 [n, L]),
        sorted by (length, bytes): export() without per-key Python objects."""
        n = ctypes.c_int64()
        nb = ctypes.c_int64()
        self._check(self.lib.ldgpu_counts_size(self.h, ctypes.byref(n), ctypes.byref(nb)))
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n.value + 1, dtype=np.int64)
        cnt = np.zeros((n.value, self.L), dtype=np.int64)
        self._check(self.lib.ldgpu_counts_export(self.h, _ptr(kb), _ptr(ko), _ptr(cnt)))
        return kb[:int(ko[-1])], ko, cnt

    def export(self) -> Tuple[List[bytes], np.ndarray]:
        """Distinct grams sorted by (length, bytes) and int64 counts [n, L]."""
        n = ctypes.c_int64()
        nb = ctypes.c_int64()
        self._check(self.lib.ldgpu_counts_size(self.h, ctypes.byref(n), ctypes.byref(nb)))
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n.value + 1, dtype=np.int64)
        cnt = np.zeros((n.value, self.L), dtype=np.int64)
        self._check(self.lib.ldgpu_counts_export(self.h, _ptr(kb), _ptr(ko), _ptr(cnt)))
        b = kb.tobytes()
        return [b[ko[i]:ko[i + 1]] for i in range(n.value)], cnt

    def export_sparse(self, first: int = 0, n: Optional[int] = None):
        """Grams [first, first + n) in (length, bytes) order with their nonzero
        (language, count) pairs: (key_bytes uint8, key_offsets int64 [n+1],
        pair_offsets int64 [n+1], pair_langs int32, pair_counts int64)."""
        if n is None:
            n = self.size() - first
        nb = ctypes.c_int64()
        npairs = ctypes.c_int64()
        self._check(self.lib.ldgpu_counts_sparse_size(self.h, first, n, ctypes.byref(nb), ctypes.byref(npairs)))
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n + 1, dtype=np.int64)
        po = np.zeros(n + 1, dtype=np.int64)
        pl = np.zeros(max(npairs.value, 1), dtype=np.int32)
        pc = np.zeros(max(npairs.value, 1), dtype=np.int64)
        self._check(self.lib.ldgpu_counts_export_sparse(self.h, first, n, _ptr(kb), _ptr(ko), _ptr(po), _ptr(pl),
                                                       _ptr(pc)))
        return kb[:nb.value], ko, po, pl[:npairs.value], pc[:npairs.value]

    def add_sparse(self, key_bytes: np.ndarray, key_offsets: np.ndarray, pair_offsets: np.ndarray,
                   pair_langs: np.ndarray, pair_counts: np.ndarray) -> None:
        kb = np.ascontiguousarray(key_bytes, dtype=np.uint8)
        ko = np.ascontiguousarray(key_offsets, dtype=np.int64)
        po = np.ascontiguousarray(pair_offsets, dtype=np.int64)
        pl = np.ascontiguousarray(pair_langs, dtype=np.int32)
        pc = np.ascontiguousarray(pair_counts, dtype=np.int64)
        self._check(self.lib.ldgpu_counts_add_sparse(self.h, len(ko) - 1, _ptr(kb if len(kb) else np.zeros(1, np.uint8)),
                                                    _ptr(ko), _ptr(po), _ptr(pl), _ptr(pc)))

    def add(self, keys: Sequence[bytes], counts: np.ndarray) -> None:
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(len(keys), self.L)
        kb, ko = pack(list(keys))
        self._check(self.lib.ldgpu_counts_add(self.h, len(keys), _ptr(kb), _ptr(ko), _ptr(counts)))

    def export_device(self, stream: Optional[int] = None):
        """(keys int64 [n] packed u64, counts int64 [n, L]) as torch tensors on
        this context's GPU, unordered (ldgpu_counts_export_device)."""
        import torch
        n = self.size()
        dev = torch.device("cuda", _lib.default_device() if self.device is None else self.device)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        counts = torch.empty((max(n, 1), self.L), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        got = ctypes.c_int64()
        self._check(self.lib.ldgpu_counts_export_device(self.h, max(n, 1), ctypes.c_void_p(keys.data_ptr()),
                                                       ctypes.c_void_p(counts.data_ptr()), ctypes.byref(got),
                                                       ctypes.c_void_p(st) if st else None))
        return keys[:got.value], counts[:got.value]

    def add_device(self, keys, counts, stream: Optional[int] = None) -> None:
        """Add device tensors (packed u64 keys as int64 [n], int64 counts [n, L])."""
        import torch
        keys = keys.contiguous()
        counts = counts.contiguous()
        st = torch.cuda.current_stream(keys.device).cuda_stream if stream is None else stream
        self._check(self.lib.ldgpu_counts_add_device(self.h, int(keys.numel()), ctypes.c_void_p(keys.data_ptr()),
                                                    ctypes.c_void_p(counts.data_ptr()),
                                                    ctypes.c_void_p(st) if st else None))

    def fit_table(self, profile_size: int) -> Dict[bytes, List[float]]:
        """computeProbabilities + filterTopGrams -> {gram: row}."""
        n = ctypes.c_int64()
        nb = ctypes.c_int64()
        self._check(self.lib.ldgpu_fit_table_size(self.h, int(profile_size), ctypes.byref(n), ctypes.byref(nb)))
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n.value + 1, dtype=np.int64)
        rows = np.zeros((n.value, self.L), dtype=np.float64)
        self._check(self.lib.ldgpu_fit_table_export(self.h, _ptr(kb), _ptr(ko), _ptr(rows)))
        b = kb.tobytes()
        return {b[ko[i]:ko[i + 1]]: rows[i].tolist() for i in range(n.value)}

    def cached_table_masks(self):
        """The table of the last fit_table / fit_table_masks call, exported
        again (ldgpu_fit_table_info + ldgpu_fit_table_export_masks): the same
        arrays as fit_table_masks returned, without a rebuild."""
        n = ctypes.c_int64()
        nb = ctypes.c_int64()
        self._check(self.lib.ldgpu_fit_table_info(self.h, ctypes.byref(n), ctypes.byref(nb)))
        S = (self.L + 63) // 64
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n.value + 1, dtype=np.int64)
        masks = np.zeros((max(n.value, 1), S), dtype=np.uint64)
        vals = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(self.lib.ldgpu_fit_table_export_masks(self.h, _ptr(kb), _ptr(ko), _ptr(masks), _ptr(vals)))
        return kb, ko, masks[:n.value], vals[:n.value]

    def fit_table_masks(self, profile_size: int):
        """The fit table in mask form, as packed arrays: (key_bytes uint8,
        key_offsets int64 [n+1], masks uint64 [n, S], vals fp64 [n]) -- what
        DeviceModel.from_masks takes; no per-row Python objects, so tables of
        10M rows x 200 languages stay cheap."""
        n = ctypes.c_int64()
        nb = ctypes.c_int64()
        self._check(self.lib.ldgpu_fit_table_size(self.h, int(profile_size), ctypes.byref(n), ctypes.byref(nb)))
        S = (self.L + 63) // 64
        kb = np.zeros(max(nb.value, 1), dtype=np.uint8)
        ko = np.zeros(n.value + 1, dtype=np.int64)
        masks = np.zeros((max(n.value, 1), S), dtype=np.uint64)
        vals = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(self.lib.ldgpu_fit_table_export_masks(self.h, _ptr(kb), _ptr(ko), _ptr(masks), _ptr(vals)))
        return kb, ko, masks[:n.value], vals[:n.value]



def utf8_decode(data: np.ndarray, offsets: np.ndarray, low_bytes: bool = False, device: Optional[int] = None,
                variant: str = "product") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """UTF-8 documents decoded on the GPU (ldgpu_utf8_decode; the rule:
    languagedetection.utf8): (UTF-16 units uint16 -- or, low_bytes, the SCORE
    encoding uint8 --, output offsets int64[n + 1], host uint8[n]: 1 = the
    document is ill-formed and its output empty)."""
    lib = _lib.load(variant=variant)
    ctx = _lib.context(device, variant)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    cap = max(int(offsets[-1] - offsets[0]) if n > 0 else 0, 1)
    out = np.zeros(cap, dtype=np.uint8 if low_bytes else np.uint16)
    out_off = np.zeros(max(n, 0) + 1, dtype=np.int64)
    host = np.zeros(max(n, 1), dtype=np.uint8)
    _lib.check(lib.ldgpu_utf8_decode(ctx, _ptr(data), _ptr(offsets), n, _lib.PRE_LOW_BYTES if low_bytes else 0,
                                     _ptr(out), _ptr(out_off), _ptr(host)), lib)
    return out[:int(out_off[-1])], out_off, host[:max(n, 0)]


def utf8_decode_device(d_utf8: int, d_offsets: int, n_docs: int, d_out: int, d_out_offsets: int, d_host: int,
                       low_bytes: bool = False, stream: int = 0, device: Optional[int] = None,
                       variant: str = "product") -> None:
    """Device pointers -> the decoded units (or low bytes), their offsets and
    the flags in place, async on `stream` (ldgpu_utf8_decode_device)."""
    lib = _lib.load(variant=variant)
    ctx = _lib.context(device, variant)
    _lib.check(lib.ldgpu_utf8_decode_device(ctx, ctypes.c_void_p(d_utf8), ctypes.c_void_p(d_offsets), n_docs,
                                            _lib.PRE_LOW_BYTES if low_bytes else 0, ctypes.c_void_p(d_out),
                                            ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(d_host),
                                            ctypes.c_void_p(stream) if stream else None), lib)


def case_tables() -> Tuple[np.ndarray, np.ndarray]:
    """The host language's 1:1 lower-case mapping of UTF-16 units (str.lower of
    one character; Java: Character.toLowerCase) and the `special` bitmap of the
    units whose String.toLowerCase is not that mapping or needs context
    (include/ldgpu.h PREPROCESS): U+0130 (-> "i" + U+0307), capital sigma
    (Final_Sigma), and the high surrogates of supplementary planes holding
    cased letters."""
    global _CASE_TABLES
    if _CASE_TABLES is None:
        lower = np.arange(65536, dtype=np.uint16)
        special = np.zeros(65536, dtype=bool)
        for c in range(65536):
            if 0xD800 <= c <= 0xDFFF:
                continue
            low = chr(c).lower()
            if len(low) == 1 and ord(low) < 0x10000:
                lower[c] = ord(low)
            else:
                special[c] = True
        special[0x3A3] = True
        for c in range(0x10000, 0x110000):
            if chr(c).lower() != chr(c):
                special[0xD800 + ((c - 0x10000) >> 10)] = True
        _CASE_TABLES = (lower, np.packbits(special, bitorder="little"))
    return _CASE_TABLES


_CASE_TABLES = None


def locale_class(lang_tag) -> int:
    """Locale.forLanguageTag(tag).getLanguage() -> the device's locale class."""
    from .preprocessing import _language_of
    lang = _language_of(lang_tag)
    return _lib.LOCALE_TR_AZ if lang in ("tr", "az") else (_lib.LOCALE_LT if lang == "lt" else _lib.LOCALE_ROOT)


class DeviceCaseMap(_Owner):
    """The preprocessors on the GPU (ldgpu_preprocess; include/ldgpu.h
    PREPROCESS): lower-casing and the symbol / space cleanup over UTF-16 units."""

    def __init__(self, device: Optional[int] = None, variant: str = "product"):
        self.lib = _lib.load(variant=variant)
        self.ctx = _lib.context(device, variant=variant)
        lower, special = case_tables()
        h = ctypes.c_void_p()
        self._check(self.lib.ldgpu_casemap_create(self.ctx, _ptr(lower), _ptr(special), ctypes.byref(h)))
        self.h = h.value

    @staticmethod
    def pack_units(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """Java strings: UTF-16 code units (u16) and offsets in units."""
        enc = [t.encode("utf-16-le", "surrogatepass") for t in texts]
        lens = np.fromiter((len(e) // 2 for e in enc), dtype=np.int64, count=len(enc))
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        units = np.frombuffer(b"".join(enc) + b"\0\0", dtype=np.uint16)
        return np.ascontiguousarray(units), off

    def run(self, units: np.ndarray, offsets: np.ndarray, locale: Optional[np.ndarray], flags: int
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(output units or bytes, output offsets, host flags) of ldgpu_preprocess."""
        n = len(offsets) - 1
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if locale is not None:
            locale = np.ascontiguousarray(locale, dtype=np.uint8)
        cap = max(int(offsets[-1] - offsets[0]) if n else 0, 1)
        out = np.zeros(cap + 4, dtype=np.uint8 if flags & _lib.PRE_LOW_BYTES else np.uint16)
        out_off = np.zeros(n + 1, dtype=np.int64)
        host = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.ldgpu_preprocess(self.h, _ptr(units), _ptr(offsets), n, _ptr(locale), flags,
                                              _ptr(out), _ptr(out_off), _ptr(host)))
        return out, out_off, host[:n]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldgpu_casemap_destroy(ctypes.c_void_p(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
