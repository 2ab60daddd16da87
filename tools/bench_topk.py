"""Top-k SCORE timing (k = 3) beside the two ways a caller had before it.

On bench.py's config 2 (10M x 256 B, 20 languages, grams 1-5) and config 5's
table (200 languages, grams 1-7), documents resident in HBM, timed with device
events, warmed, the paths alternating in one process:

  (a) ldgpu_score_device, labels only;
  (b) ldgpu_score_device with the full [n][L] score matrix, then
      torch.topk(scores, 3) -- what a caller needing a runner-up had to do;
  (c) ldgpu_score_topk_device, k = 3.

Then (c)'s scratch cap: the diagnostics library with chunks of 16 / 64 /
256 MiB of scores (LDGPU_TOPK_CHUNK_DOCS), alternating (diagnostics kernels
carry ablation branches: compare these three with each other only).

One JSON line per (config, path) to --json-out, each with _lib.provenance().
Usage: python tools/bench_topk.py [--configs 2,5] [--docs N] [--steps S] [--warmup W] [--json-out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-languagedetector_amd"))

import torch  # noqa: E402

from languagedetection import _lib, synth  # noqa: E402
from languagedetection.runtime import DeviceCounts, DeviceModel  # noqa: E402

K = 3
CAP_MIB = 256  # the library's scratch cap (kTopkScratchBytes, ldgpu_api.hip)
PRESET = {2: dict(langs=20, grams=[1, 2, 3, 4, 5], profile_size=500, train_docs=1000),
          5: dict(langs=200, grams=[1, 2, 3, 4, 5, 6, 7], profile_size=50_000, train_docs=80)}


def build_packed(cfg, ls):
    """bench.py's table: FIT on the GPU, the profile table in mask form."""
    lang = np.repeat(np.arange(cfg["langs"], dtype=np.int32), cfg["train_docs"])
    data, off, lang = synth.generate(ls, len(lang), 200, 2000, seed=synth.SEED_BASE + 100, doc_lang=lang)
    counts = DeviceCounts(cfg["langs"], cfg["grams"], capacity_hint=1 << 20, device=0)
    counts.count(data, off, lang)
    packed = counts.fit_table_masks(cfg["profile_size"])
    counts.close()
    return packed


def timed(paths, steps, warmup, stream, dev):
    """Median ms of every path, the paths alternating step by step."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=str, default="2,5")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json-out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for config in [int(c) for c in args.configs.split(",")]:
        cfg = PRESET[config]
        L, grams = cfg["langs"], cfg["grams"]
        ls = synth.make_languages(L)
        packed = build_packed(cfg, ls)
        model = DeviceModel.from_masks(*packed, L, grams, device=0)
        diag = DeviceModel.from_masks(*packed, L, grams, device=0, variant="diag")
        d_bytes, d_off, _ = synth.generate_device(ls, args.docs, 256, 256, seed=synth.SEED_BASE + config, device=dev,
                                                  chunk_docs=1 << 20)
        n = args.docs
        n_bytes = int(d_off[-1].item())
        d_lab = torch.empty(n, dtype=torch.int32, device=dev)
        d_scores = torch.empty((n, L), dtype=torch.float64, device=dev)
        d_tl = torch.empty((n, K), dtype=torch.int32, device=dev)
        d_ts = torch.empty((n, K), dtype=torch.float64, device=dev)
        keep = {}

        def labels_only():
            model.score_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, d_lab.data_ptr(), 0,
                               stream.cuda_stream)

        def scores_then_torch_topk():
            model.score_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, d_lab.data_ptr(),
                               d_scores.data_ptr(), stream.cuda_stream)
            keep["b"] = torch.topk(d_scores, K)

        def score_topk(m=model):
            m.score_topk_device(d_bytes.data_ptr(), n_bytes, d_off.data_ptr(), n, K, d_tl.data_ptr(),
                                d_ts.data_ptr(), stream.cuda_stream)

        def capped(mib):
            def fn():
                os.environ["LDGPU_TOPK_CHUNK_DOCS"] = str(max(1, (mib << 20) // (8 * L)))
                score_topk(diag)
            return fn

        ms = timed([("a_labels_only", labels_only), ("b_scores_then_torch_topk", scores_then_torch_topk),
                    ("c_score_topk_k3", score_topk)], args.steps, args.warmup, stream, dev)
        first_ok = bool(torch.equal(d_tl[:, 0], d_lab))
        values_ok = bool(torch.equal(d_ts[:, 0], keep["b"].values[:, 0]))
        keep.clear()
        ms.update(timed([(f"c_diag_cap_{mib}MiB", capped(mib)) for mib in (16, 64, 256)], args.steps, args.warmup,
                        stream, dev))
        os.environ.pop("LDGPU_TOPK_CHUNK_DOCS", None)
        scratch = {"a_labels_only": 0, "b_scores_then_torch_topk": n * L * 8,
                   "c_score_topk_k3": min(n, (CAP_MIB << 20) // (8 * L)) * (L * 8 + 4)}
        for name, v in ms.items():
            lines.append({"tool": "tools/bench_topk.py", "k": K, "config": config, "docs": n, "doc_bytes": 256,
                          "languages": L, "gram_lengths": grams, "table_rows": int(len(packed[1]) - 1),
                          "model": model.info(), "path": name, "ms_median": float(np.median(v)), "ms_min": min(v),
                          "ms_all": v, "docs_per_s": round(n / (float(np.median(v)) * 1e-3), 1),
                          "scratch_bytes": scratch.get(name),
                          "top1_equals_label": first_ok, "top1_score_equals_torch_topk": values_ok,
                          "provenance": _lib.provenance("diag" if "diag" in name else "product")})
            print(json.dumps(lines[-1]), flush=True)
        del d_scores, d_tl, d_ts, d_lab, d_bytes, d_off
        model.close()
        diag.close()
        torch.cuda.empty_cache()
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
