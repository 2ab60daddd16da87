"""Segment SCORE timing beside what a caller runs today before smoothing on the
host.

On bench.py's config 2 table (20 languages, grams 1-5) and device-resident
corpora -- tools/bench_spans.py's shapes (documents of 1,024 B at (width,
stride) = (256, 128), (256, 256), (64, 32)) plus one of a few documents of about
10^6 spans each at (64, 32), which exposes the one-wave-per-document limit --
timed with device events, warmed, the two paths alternating in one process:

  (a) ldgpu_score_spans_device with d_scores: the [n_spans][L] fp64 matrix a
      caller needs today for a dynamic programme on the host.  Charitable to
      today: the device-to-host copy of the matrix (160 B per span at L = 20)
      and the host DP are not counted;
  (b) ldgpu_score_segments_device: the smoothed labels, 4 B per span.

One JSON line per (shape, path) to --json-out, each with _lib.provenance(), the
ratio (b) / (a) and -- from a kernel trace, below -- the kernel split of (b).

The split of (b) between its kernels comes from a kernel trace of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/bench_segments.py --profile-shape docs1k,64,32 --calls 3
runs (b) alone `--calls` times; `--split docs1k,64,32=KERNEL_TRACE.csv`
(repeatable) then adds that run's per-call kernel times to the shape's lines:
forward (segment_forward_kernel), backtrace (segment_backtrace_kernel), score
(score_kernel), other (the span geometry, scans and gather), and the forward
kernel's ns per span.

Usage: python tools/bench_segments.py [--docs N] [--long-docs N] [--steps S] [--warmup W] [--penalty P]
                                      [--json-out FILE] [--split NAME,W,S=CSV ...]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-languagedetector_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_spans import CFG, DOC_BYTES, build_packed, timed  # noqa: E402
from languagedetection import _lib, spans, synth  # noqa: E402
from languagedetection.runtime import DeviceModel  # noqa: E402

LONG_DOC_BYTES = 31_250 * DOC_BYTES  # 999,999 spans at (64, 32)
# (corpus, width, stride): "docs1k" = --docs documents of DOC_BYTES bytes,
# "long" = --long-docs documents of LONG_DOC_BYTES bytes
SHAPES = [("docs1k", 256, 128), ("docs1k", 256, 256), ("docs1k", 64, 32), ("long", 64, 32)]


def kernel_split(path, calls, n_spans):
    """Per-call ms by kernel class from the rocprofv3 kernel_trace.csv of a
    --profile-shape run of `calls` segment calls: the dispatches from the first
    span_geom_kernel to the last segment_backtrace_kernel."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if "span_geom_kernel" in r["Kernel_Name"])
    last = max(i for i, r in enumerate(rows) if "segment_backtrace_kernel" in r["Kernel_Name"])
    out = {"forward": 0.0, "backtrace": 0.0, "score": 0.0, "other": 0.0}
    for r in rows[first:last + 1]:
        name, ms = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        out["forward" if "segment_forward_kernel" in name else "backtrace" if "segment_backtrace_kernel" in name
            else "score" if "score_kernel" in name else "other"] += ms
    out = {k: round(v / calls, 4) for k, v in out.items()}
    out["launches_per_call"] = (last + 1 - first) // calls
    out["forward_ns_per_span"] = round(out["forward"] * 1e6 / n_spans, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--long-docs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--penalty", type=float, default=6.0)
    ap.add_argument("--json-out", type=str, default="")
    ap.add_argument("--profile-shape", type=str, default="", help="NAME,W,S: run the segment path alone (profiler)")
    ap.add_argument("--calls", type=int, default=3, help="segment calls of a --profile-shape run")
    ap.add_argument("--split", action="append", default=[], help="NAME,W,S=kernel_trace.csv of a --profile-shape run")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L, grams = CFG["langs"], CFG["grams"]
    ls = synth.make_languages(L)
    packed = build_packed(ls)
    model = DeviceModel.from_masks(*packed, L, grams, device=0)

    shapes = SHAPES
    if args.profile_shape:
        name, w, s = args.profile_shape.split(",")
        shapes = [(name, int(w), int(s))]
    split_of = {}
    for s in args.split:
        shape, path = s.split("=", 1)
        name, w, st = shape.split(",")
        split_of[(name, int(w), int(st))] = path

    corpora = {}

    def corpus(name):
        """(d_bytes, d_off, n_docs, n_bytes, doc_bytes).  "long" re-reads the
        first documents of "docs1k" as --long-docs documents of LONG_DOC_BYTES
        each: LONG_DOC_BYTES / DOC_BYTES drawn documents one after the other
        (the synthetic generator draws a document's bytes one position at a
        time over all documents, which suits many short documents only)."""
        if "docs1k" not in corpora:
            d_bytes, d_off, _ = synth.generate_device(ls, args.docs, DOC_BYTES, DOC_BYTES, seed=synth.SEED_BASE + 2,
                                                      device=dev, chunk_docs=1 << 18)
            corpora["docs1k"] = (d_bytes, d_off, args.docs, int(d_off[-1].item()), DOC_BYTES)
        if name == "long" and name not in corpora:
            d_bytes = corpora["docs1k"][0]
            k = min(args.long_docs, args.docs * DOC_BYTES // LONG_DOC_BYTES)
            assert k >= 1, "--docs too small for one long document"
            d_off = torch.arange(k + 1, dtype=torch.int64, device=dev) * LONG_DOC_BYTES
            corpora["long"] = (d_bytes, d_off, k, k * LONG_DOC_BYTES, LONG_DOC_BYTES)
        return corpora[name]

    lines = []
    for name, width, stride in shapes:
        d_bytes, d_off, n, n_bytes, doc_bytes = corpus(name)
        n_spans = n * spans.span_count(doc_bytes, width, stride)
        d_soff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        model.span_offsets_device(d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize(dev)
        assert int(d_soff[-1].item()) == n_spans
        d_raw = torch.empty(n_spans, dtype=torch.int32, device=dev)
        d_seg = torch.empty(n_spans, dtype=torch.int32, device=dev)

        def segment_path():
            model.score_segments_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, width, stride, args.penalty,
                                        d_soff.data_ptr(), n_spans, d_seg.data_ptr(), stream.cuda_stream)

        if args.profile_shape:
            for _ in range(args.calls):
                segment_path()
            torch.cuda.synchronize(dev)
            break

        d_scores = torch.empty((n_spans, L), dtype=torch.float64, device=dev)

        def scores_path():
            model.score_spans_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, width, stride,
                                     d_soff.data_ptr(), n_spans, d_raw.data_ptr(), d_scores.data_ptr(),
                                     stream.cuda_stream)

        ms = timed([("a_score_spans_device_scores", scores_path), ("b_score_segments_device", segment_path)],
                   args.steps, args.warmup, stream, dev)
        med = {k_: float(np.median(v)) for k_, v in ms.items()}
        ratio = round(med["b_score_segments_device"] / med["a_score_spans_device_scores"], 4)
        relabelled = float((d_raw != d_seg).double().mean().item())
        split = kernel_split(split_of[(name, width, stride)], args.calls, n_spans) \
            if (name, width, stride) in split_of else None
        for path, v in ms.items():
            line = {"tool": "tools/bench_segments.py", "config": 2, "corpus": name, "docs": n, "doc_bytes": doc_bytes,
                    "width": width, "stride": stride, "spans": n_spans, "languages": L, "gram_lengths": grams,
                    "penalty": args.penalty, "table_rows": int(len(packed[1]) - 1), "model": model.info(),
                    "path": path, "ms_median": med[path], "ms_min": min(v), "ms_all": v,
                    "spans_per_s": round(n_spans / (med[path] * 1e-3), 1), "ratio_segments_over_scores": ratio,
                    "spans_relabelled": round(relabelled, 4), "provenance": _lib.provenance()}
            if path.startswith("b_") and split:
                line["kernel_ms_per_call"] = split
            lines.append(line)
            print(json.dumps(line), flush=True)
        del d_scores, d_raw, d_seg
        torch.cuda.empty_cache()
    model.close()
    if args.json_out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
