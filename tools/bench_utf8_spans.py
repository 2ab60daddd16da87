"""Span scoring of UTF-8 documents beside span scoring of the already-encoded
low bytes.

The corpora, tables and timing of tools/bench_utf8.py (config-2-shaped
documents of 256 UTF-16 units at about 0 %, 30 % and 100 % non-ASCII
characters, all of the BMP: no 4-byte sequence, so no split pair; resident in
HBM; device events, the paths alternating in one process, medians after
warm-up), the geometries of tools/bench_spans.py: (width, stride) = (256, 128)
and (64, 32).  Per corpus and geometry:

  (a) ldgpu_score_spans_device on the pre-encoded low bytes;
  (b) ldgpu_score_spans_utf_device on the UTF-8 of the same texts, with starts;
  (c) the same without starts (d_starts NULL);
  (d) ldgpu_span_offsets_utf_device alone (the length pass, the span counts and
      their scan);
  (e) host buffers, --host-docs documents, by the host clock:
      ldgpu_span_offsets_utf + ldgpu_score_spans_utf (with starts) on the UTF-8
      buffer against the route without them -- the documents as Python strings
      through encoding.pack_score, then ldgpu_score_spans.

(b) - (a) is what decoding and the starts cost on the device, (b) - (c) the
starts alone.  The labels of (a), (b) and (c) must be identical, the span
offsets of (d) those of ldgpu_span_offsets_device on the low bytes, and the
starts of a sample of documents those of languagedetection.utf8.span_geometry;
the tool fails otherwise.  One JSON line per corpus and geometry to --json-out.

Usage: python tools/bench_utf8_spans.py [--docs N] [--host-docs N] [--steps S] [--warmup W] [--json-out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_utf8 as U  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402

from languagedetection import _lib, encoding, utf8  # noqa: E402

GEOMETRIES = [(256, 128), (64, 32)]
SAMPLE_DOCS = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--host-docs", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json-out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    n, L = args.docs, U.CFG["langs"]
    lines, failed = [], False
    for ci, (name, frac) in enumerate(U.CORPORA):
        model, rows = U.build_model(frac, 100 + ci, dev)
        cp, _ = U.code_points(n, frac, 200 + ci, dev)
        d_low, d_loff = U.low_bytes_of(cp)
        d_utf, d_uoff = U.utf8_of(cp)
        nonascii = float((cp >= 0x80).float().mean().item())
        del cp
        low_bytes, utf_bytes = n * U.UNITS, int(d_uoff[-1].item())
        nh = min(args.host_docs, n)
        h_uoff = d_uoff[:nh + 1].cpu().numpy()
        h_utf = np.concatenate([d_utf[:int(h_uoff[-1])].cpu().numpy(), np.zeros(8, np.uint8)])
        raw = h_utf.tobytes()
        texts = [raw[h_uoff[i]:h_uoff[i + 1]].decode("utf-8") for i in range(nh)]   # what a String caller holds
        for width, stride in GEOMETRIES:
            d_soff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_soff_u = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_units = torch.zeros(n, dtype=torch.int64, device=dev)
            model.span_offsets_device(d_loff.data_ptr(), n, width, stride, d_soff.data_ptr(), st)
            torch.cuda.synchronize(dev)
            ns = int(d_soff[-1].item())
            d_lab = {k: torch.full((ns,), -7, dtype=torch.int32, device=dev) for k in "abc"}
            d_starts = torch.full((ns,), -7, dtype=torch.int64, device=dev)

            def a_spans():
                model.score_spans_device(d_low.data_ptr(), low_bytes, d_loff.data_ptr(), n, width, stride,
                                         d_soff.data_ptr(), ns, d_lab["a"].data_ptr(), 0, st)

            def b_spans_utf_starts():
                model.score_spans_utf8_device(d_utf.data_ptr(), utf_bytes, d_uoff.data_ptr(), n, width, stride,
                                              d_soff_u.data_ptr(), ns, d_lab["b"].data_ptr(), 0, d_starts.data_ptr(), st)

            def c_spans_utf():
                model.score_spans_utf8_device(d_utf.data_ptr(), utf_bytes, d_uoff.data_ptr(), n, width, stride,
                                              d_soff_u.data_ptr(), ns, d_lab["c"].data_ptr(), 0, 0, st)

            def d_span_offsets_utf():
                model.span_offsets_utf8_device(d_utf.data_ptr(), d_uoff.data_ptr(), n, width, stride,
                                               d_soff_u.data_ptr(), d_units.data_ptr(), st)

            d_span_offsets_utf()      # (b) and (c) take its output
            ms = U.timed([("a", a_spans), ("b", b_spans_utf_starts), ("c", c_spans_utf), ("d", d_span_offsets_utf)],
                         args.steps, args.warmup, stream, dev)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            offsets_equal = bool(torch.equal(d_soff, d_soff_u) and int((d_units != U.UNITS).sum().item()) == 0)
            labels_equal = bool(torch.equal(d_lab["a"], d_lab["b"]) and torch.equal(d_lab["a"], d_lab["c"]))
            # the starts of a sample against the numpy checker
            ks = min(SAMPLE_DOCS, n)
            s_off = d_uoff[:ks + 1].cpu().numpy()
            s_utf = np.concatenate([d_utf[:int(s_off[-1])].cpu().numpy(), np.zeros(8, np.uint8)])
            want_soff, _, want_starts = utf8.span_geometry(s_utf, s_off, width, stride)
            starts_equal = bool(np.array_equal(d_starts[:int(want_soff[-1])].cpu().numpy(), want_starts))

            # (e) host buffers
            def e_utf_route():
                soff, _ = model.span_offsets_utf8(h_utf, h_uoff, width, stride)
                return model.score_spans_utf8(h_utf, h_uoff, width, stride, span_offsets=soff)

            def e_parent_route():
                return model.score_spans(*encoding.pack_score(texts), width, stride)

            e_utf_route()
            e_parent_route()
            t_new, res_new = U.host_clock(e_utf_route, 5)
            t_old, res_old = U.host_clock(e_parent_route, 3)
            nsh = int(res_new[3][-1])
            host_equal = bool(np.array_equal(res_new[0], res_old[0]) and np.array_equal(res_new[3], res_old[2])
                              and np.array_equal(res_new[0], d_lab["a"][:nsh].cpu().numpy())
                              and np.array_equal(res_new[2], d_starts[:nsh].cpu().numpy()))
            line = {
                "tool": "tools/bench_utf8_spans.py", "config": 2, "corpus": name, "nonascii_target": frac,
                "nonascii_chars": round(nonascii, 4), "docs": n, "units_per_doc": U.UNITS, "width": width,
                "stride": stride, "spans": ns, "low_bytes": low_bytes, "utf8_bytes": utf_bytes, "languages": L,
                "gram_lengths": U.CFG["grams"], "table_rows": rows, "model": model.info(), "ms_all": ms,
                "ms_median": med,
                "a_spans_device_spans_per_s": round(ns / (med["a"] * 1e-3), 1),
                "b_spans_utf_device_spans_per_s": round(ns / (med["b"] * 1e-3), 1),
                "b_minus_a_ms": round(med["b"] - med["a"], 4), "b_over_a": round(med["b"] / med["a"], 4),
                "b_minus_c_ms_starts": round(med["b"] - med["c"], 4), "c_minus_a_ms": round(med["c"] - med["a"], 4),
                "d_span_offsets_utf_ms": round(med["d"], 4),
                "e_host_docs": nh, "e_host_spans": nsh, "e_utf_route_ms_all": t_new,
                "e_pack_score_then_score_spans_ms_all": t_old,
                "e_utf_route_docs_per_s": round(nh / (float(np.median(t_new)) * 1e-3), 1),
                "e_pack_score_then_score_spans_docs_per_s": round(nh / (float(np.median(t_old)) * 1e-3), 1),
                "e_ratio_parent_over_utf": round(float(np.median(t_old)) / float(np.median(t_new)), 2),
                "labels_equal_a_b_c": labels_equal, "span_offsets_equal": offsets_equal,
                "starts_equal_checker_sample": starts_equal, "starts_sample_docs": ks, "host_equal": host_equal,
                "provenance": _lib.provenance(),
            }
            lines.append(line)
            print(json.dumps(line), flush=True)
            failed = failed or not (labels_equal and offsets_equal and starts_equal and host_equal)
            del d_soff, d_soff_u, d_units, d_lab, d_starts
        model.close()
        del d_low, d_loff, d_utf, d_uoff
        torch.cuda.empty_cache()
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if failed:
        sys.exit("bench_utf8_spans: the UTF-8 route's labels, span offsets or starts differ from the checks'")


if __name__ == "__main__":
    main()
