"""Span SCORE timing beside scoring the same spans as materialised documents.

On bench.py's config 2 table (20 languages, grams 1-5), 1M documents of 1,024 B
resident in HBM, at (width, stride) = (256, 128), (256, 256) and (64, 32),
timed with device events, warmed, the two paths alternating in one process:

  (a) ldgpu_score_device on the spans already materialised as documents (numpy
      on the host, then resident on the device): the kernel time a caller
      without span scoring pays, not counting the materialising or the
      width / stride times larger transfer;
  (b) ldgpu_score_spans_device on the documents themselves (labels only, the
      span offsets computed before the timed region).

One JSON line per (shape, path) to --json-out, each with _lib.provenance() and
the ratio (b) / (a).

The split of (b) between its kernels comes from a kernel trace of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/bench_spans.py --profile-shape 256,128 --calls 3
runs (b) alone `--calls` times; `--split 256,128=KERNEL_TRACE.csv` (repeatable)
then adds that run's per-call kernel times to the shape's lines: geometry
(span_geom_kernel and the scan of the lengths), gather (span_gather_kernel),
score (score_kernel).  Only the dispatches of the span calls count: the run's
setup (building the table, drawing the documents) comes before them.

Usage: python tools/bench_spans.py [--docs N] [--steps S] [--warmup W] [--json-out FILE] [--split W,S=CSV ...]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-languagedetector_amd"))

import torch  # noqa: E402

from languagedetection import _lib, spans, synth  # noqa: E402
from languagedetection.runtime import DeviceCounts, DeviceModel  # noqa: E402

SHAPES = [(256, 128), (256, 256), (64, 32)]
DOC_BYTES = 1024
CFG = dict(langs=20, grams=[1, 2, 3, 4, 5], profile_size=500, train_docs=1000)  # bench.py's config 2


def build_packed(ls):
    """bench.py's table: FIT on the GPU, the profile table in mask form."""
    lang = np.repeat(np.arange(CFG["langs"], dtype=np.int32), CFG["train_docs"])
    data, off, lang = synth.generate(ls, len(lang), 200, 2000, seed=synth.SEED_BASE + 100, doc_lang=lang)
    counts = DeviceCounts(CFG["langs"], CFG["grams"], capacity_hint=1 << 20, device=0)
    counts.count(data, off, lang)
    packed = counts.fit_table_masks(CFG["profile_size"])
    counts.close()
    return packed


def materialised(host_bytes, n, width, stride):
    """The spans of n documents of DOC_BYTES bytes as documents: (bytes, offsets)."""
    per = spans.span_count(DOC_BYTES, width, stride)
    starts = np.arange(per) * stride
    assert starts[-1] + width >= DOC_BYTES and (per == 1 or starts[-2] + width < DOC_BYTES)
    docs = host_bytes[:n * DOC_BYTES].reshape(n, DOC_BYTES)
    parts = [docs[:, s:min(s + width, DOC_BYTES)] for s in starts]
    lens = np.array([p.shape[1] for p in parts], dtype=np.int64)
    out = np.concatenate(parts, axis=1).reshape(-1)
    off = np.zeros(n * per + 1, dtype=np.int64)
    np.cumsum(np.tile(lens, n), out=off[1:])
    return out, off


def timed(paths, steps, warmup, stream, dev):
    """ms of every path per step, the paths alternating step by step."""
    for _ in range(warmup):
        for _, fn in paths:
            fn()
    torch.cuda.synchronize(dev)
    ev = {name: [] for name, _ in paths}
    for _ in range(steps):
        for name, fn in paths:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream)
            fn()
            e.record(stream)
            ev[name].append((s, e))
    torch.cuda.synchronize(dev)
    return {name: [round(s.elapsed_time(e), 4) for s, e in v] for name, v in ev.items()}


def kernel_split(path, calls):
    """Per-call ms by kernel class from the rocprofv3 kernel_trace.csv of a
    --profile-shape run of `calls` span calls: the dispatches from the first
    span_geom_kernel to the last score_kernel (everything before is the run's
    setup), classed gather / score / geometry (span_geom_kernel and the scan's
    kernels: whatever else runs there)."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if "span_geom_kernel" in r["Kernel_Name"])
    last = max(i for i, r in enumerate(rows) if "score_kernel" in r["Kernel_Name"])
    out = {"geometry": 0.0, "gather": 0.0, "score": 0.0}
    for r in rows[first:last + 1]:
        name, ms = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        out["gather" if "span_gather_kernel" in name else "score" if "score_kernel" in name else "geometry"] += ms
    out = {k: round(v / calls, 4) for k, v in out.items()}
    out["launches_per_call"] = (last + 1 - first) // calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json-out", type=str, default="")
    ap.add_argument("--profile-shape", type=str, default="", help="W,S: run the span path alone (under a profiler)")
    ap.add_argument("--calls", type=int, default=3, help="span calls of a --profile-shape run")
    ap.add_argument("--split", action="append", default=[], help="W,S=kernel_trace.csv of a --profile-shape run")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L, grams = CFG["langs"], CFG["grams"]
    ls = synth.make_languages(L)
    packed = build_packed(ls)
    model = DeviceModel.from_masks(*packed, L, grams, device=0)
    n = args.docs
    d_bytes, d_off, _ = synth.generate_device(ls, n, DOC_BYTES, DOC_BYTES, seed=synth.SEED_BASE + 2, device=dev,
                                              chunk_docs=1 << 18)
    n_bytes = int(d_off[-1].item())
    d_soff = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def span_call(width, stride, n_spans, d_lab):
        model.score_spans_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, width, stride, d_soff.data_ptr(),
                                 n_spans, d_lab.data_ptr(), 0, stream.cuda_stream)

    if args.profile_shape:
        width, stride = (int(x) for x in args.profile_shape.split(","))
        n_spans = n * spans.span_count(DOC_BYTES, width, stride)
        model.span_offsets_device(d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), stream.cuda_stream)
        d_lab = torch.empty(n_spans, dtype=torch.int32, device=dev)
        for _ in range(args.calls):
            span_call(width, stride, n_spans, d_lab)
        torch.cuda.synchronize(dev)
        return

    splits = {}
    for s in args.split:
        shape, path = s.split("=", 1)
        splits[tuple(int(x) for x in shape.split(","))] = kernel_split(path, args.calls)
    host_bytes = d_bytes[:n_bytes].cpu().numpy()
    lines = []
    for width, stride in SHAPES:
        per = spans.span_count(DOC_BYTES, width, stride)
        n_spans = n * per
        mat, moff = materialised(host_bytes, n, width, stride)
        k = min(n, 64)   # the numpy short cut against the rule's restatement
        sd, so = spans.materialise(host_bytes[:k * DOC_BYTES], np.arange(k + 1, dtype=np.int64) * DOC_BYTES, width,
                                   stride)
        assert np.array_equal(so, moff[:k * per + 1]) and np.array_equal(sd[:so[-1]], mat[:so[-1]])
        m_bytes = int(moff[-1])
        d_mat = torch.from_numpy(np.concatenate([mat, np.zeros(16, np.uint8)])).to(dev)
        d_moff = torch.from_numpy(moff).to(dev)
        del mat, moff
        d_lab_a = torch.empty(n_spans, dtype=torch.int32, device=dev)
        d_lab_b = torch.empty(n_spans, dtype=torch.int32, device=dev)
        model.span_offsets_device(d_off.data_ptr(), n, width, stride, d_soff.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize(dev)
        assert int(d_soff[-1].item()) == n_spans

        def baseline():
            model.score_device(d_mat.data_ptr(), m_bytes, d_moff.data_ptr(), n_spans, d_lab_a.data_ptr(), 0,
                               stream.cuda_stream)

        def span_path():
            span_call(width, stride, n_spans, d_lab_b)

        ms = timed([("a_score_device_materialised", baseline), ("b_score_spans_device", span_path)], args.steps,
                   args.warmup, stream, dev)
        same = bool(torch.equal(d_lab_a, d_lab_b))
        med = {k_: float(np.median(v)) for k_, v in ms.items()}
        ratio = round(med["b_score_spans_device"] / med["a_score_device_materialised"], 4)
        for name, v in ms.items():
            line = {"tool": "tools/bench_spans.py", "config": 2, "docs": n, "doc_bytes": DOC_BYTES, "width": width,
                    "stride": stride, "spans": n_spans, "span_bytes": m_bytes, "languages": L, "gram_lengths": grams,
                    "table_rows": int(len(packed[1]) - 1), "model": model.info(), "path": name,
                    "ms_median": med[name], "ms_min": min(v), "ms_all": v,
                    "spans_per_s": round(n_spans / (med[name] * 1e-3), 1), "ratio_spans_over_materialised": ratio,
                    "labels_equal": same, "provenance": _lib.provenance()}
            if name.startswith("b_") and (width, stride) in splits:
                line["kernel_ms_per_call"] = splits[(width, stride)]
            lines.append(line)
            print(json.dumps(line), flush=True)
        del d_mat, d_moff, d_lab_a, d_lab_b
        torch.cuda.empty_cache()
    model.close()
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
