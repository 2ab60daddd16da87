"""SCORE on UTF-8 documents beside SCORE on the already-encoded low bytes.

Config-2-shaped documents (256 UTF-16 units, 20 languages, grams 1-5), every
language writing in one Unicode block as tests/bytecorpus.py's do (Latin-1,
Latin Extended-A, Greek, Cyrillic: 2-byte UTF-8; Devanagari, CJK, Hangul:
3-byte) with ASCII letters mixed in, at about 0 %, 30 % and 100 % non-ASCII
characters.  The table of each corpus is fitted on the GPU from training
documents of the same languages (their SCORE bytes).  Per corpus, warmed, timed
with device events over several repeats, the paths alternating in one process,
medians reported:

  (a) ldgpu_score_device on the low bytes, resident on the device;
  (b) ldgpu_score_utf8_device on the UTF-8 of the same texts;
  (c) the decode passes alone (ldgpu_utf8_decode_device, low-byte output), as
      bytes in + bytes out per second, beside a device-to-device copy of the
      UTF-8 bytes (which reads and writes that many bytes once each);
  (d) host buffers, --host-docs documents, by the host clock: ldgpu_score_utf8
      on the UTF-8 buffer against the route without it -- the documents as
      Python strings through encoding.pack_score, then ldgpu_score.

(b) - (a) is what the feature costs on the device, (d)'s ratio what it gains a
caller that holds UTF-8.  The labels of (a) and (b) must be identical and none
may be -1; the tool fails otherwise.  One JSON line per corpus to --json-out.

The split of (c) between its kernels comes from a kernel trace of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/bench_utf8.py --profile-corpus mixed30 --calls 5
runs the decode passes of that corpus alone `--calls` times (utf8_len_kernel,
the scan's kernels, utf8_write_kernel in the trace's kernel_stats.csv).

Usage: python tools/bench_utf8.py [--docs N] [--host-docs N] [--steps S] [--warmup W] [--json-out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-languagedetector_amd"))

import torch  # noqa: E402

from languagedetection import _lib, encoding  # noqa: E402
from languagedetection.runtime import DeviceCounts, DeviceModel, utf8_decode_device  # noqa: E402

UNITS = 256
CFG = dict(langs=20, grams=[1, 2, 3, 4, 5], profile_size=500, train_docs=1000)  # bench.py's config 2
# (first code point, code points used) of a language's block: language l writes in BLOCKS[l % 7]
BLOCKS = [(0x00C0, 64), (0x0100, 128), (0x0391, 57), (0x0410, 64), (0x0905, 53), (0x4E00, 256), (0xAC00, 256)]
CORPORA = [("ascii", 0.0), ("mixed30", 0.3), ("nonascii", 1.0)]


def code_points(n, frac, seed, dev, lang=None):
    """(n, UNITS) int64 code points and the documents' languages: a unit is a
    character of the language's block with probability `frac`, else one of its
    ASCII letters and the space; both drawn from a skewed distribution of the
    language's own, so that grams repeat."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    L = CFG["langs"]
    if lang is None:
        lang = torch.randint(0, L, (n,), generator=g, device=dev)
    first = torch.tensor([BLOCKS[l % len(BLOCKS)][0] for l in range(L)], device=dev)[lang]
    size = torch.tensor([BLOCKS[l % len(BLOCKS)][1] for l in range(L)], device=dev)[lang]
    # skew: the square of a uniform draw favours a language's first symbols;
    # the language shifts which symbols those are
    u = torch.rand((n, UNITS), generator=g, device=dev)
    own = first[:, None] + ((u * u * 24).long() * (2 * (lang[:, None] // len(BLOCKS)) + 1) + lang[:, None]) % size[:, None]
    v = torch.rand((n, UNITS), generator=g, device=dev)
    letter = (v * v * 27).long()
    ascii_ = torch.where(letter == 0, torch.full_like(letter, 0x20), 0x61 + (letter * (2 * lang[:, None] + 1)) % 26)
    pick = torch.rand((n, UNITS), generator=g, device=dev) < frac
    return torch.where(pick, own, ascii_), lang


def utf8_of(cp):
    """(UTF-8 bytes uint8 padded by 16, offsets int64 [n + 1]) of (n, UNITS) BMP code points."""
    n = cp.shape[0]
    flat = cp.reshape(-1)
    ln = 1 + (flat >= 0x80).long() + (flat >= 0x800).long()
    end = torch.cumsum(ln, 0)
    pos = end - ln
    total = int(end[-1].item())
    out = torch.zeros(total + 16, dtype=torch.uint8, device=cp.device)
    one, two, three = ln == 1, ln == 2, ln == 3
    out[pos[one]] = flat[one].to(torch.uint8)
    out[pos[two]] = (0xC0 | (flat[two] >> 6)).to(torch.uint8)
    out[pos[two] + 1] = (0x80 | (flat[two] & 0x3F)).to(torch.uint8)
    out[pos[three]] = (0xE0 | (flat[three] >> 12)).to(torch.uint8)
    out[pos[three] + 1] = (0x80 | ((flat[three] >> 6) & 0x3F)).to(torch.uint8)
    out[pos[three] + 2] = (0x80 | (flat[three] & 0x3F)).to(torch.uint8)
    off = torch.zeros(n + 1, dtype=torch.int64, device=cp.device)
    off[1:] = end.reshape(n, UNITS)[:, -1]
    return out, off


def low_bytes_of(cp):
    n = cp.shape[0]
    out = torch.zeros(n * UNITS + 16, dtype=torch.uint8, device=cp.device)
    out[:n * UNITS] = (cp.reshape(-1) & 0xFF).to(torch.uint8)
    return out, torch.arange(n + 1, dtype=torch.int64, device=cp.device) * UNITS


def build_model(frac, seed, dev):
    """bench.py's config-2 table shape: FIT on the GPU over the SCORE bytes of
    training documents of the corpus's languages, the profile table in mask form."""
    L = CFG["langs"]
    lang = torch.arange(L, device=dev).repeat_interleave(CFG["train_docs"])
    cp, _ = code_points(len(lang), frac, seed, dev, lang=lang)
    data, off = low_bytes_of(cp)
    counts = DeviceCounts(L, CFG["grams"], capacity_hint=1 << 20, device=0)
    counts.count(data.cpu().numpy(), off.cpu().numpy(), lang.to(torch.int32).cpu().numpy())
    packed = counts.fit_table_masks(CFG["profile_size"])
    counts.close()
    return DeviceModel.from_masks(*packed, L, CFG["grams"], device=0), int(len(packed[1]) - 1)


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


def host_clock(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--host-docs", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json-out", type=str, default="")
    ap.add_argument("--profile-corpus", type=str, default="", help="run this corpus's decode passes alone (under a profiler)")
    ap.add_argument("--calls", type=int, default=5, help="decode calls of a --profile-corpus run")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    n, L = args.docs, CFG["langs"]
    lines, failed = [], False
    for ci, (name, frac) in enumerate(CORPORA):
        if args.profile_corpus:
            if name != args.profile_corpus:
                continue
            cp, _ = code_points(n, frac, 200 + ci, dev)
            d_utf, d_uoff = utf8_of(cp)
            del cp
            d_dec = torch.zeros(int(d_uoff[-1].item()) + 16, dtype=torch.uint8, device=dev)
            d_doff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_host = torch.zeros(n, dtype=torch.uint8, device=dev)
            for _ in range(args.calls):
                utf8_decode_device(d_utf.data_ptr(), d_uoff.data_ptr(), n, d_dec.data_ptr(), d_doff.data_ptr(),
                                   d_host.data_ptr(), low_bytes=True, stream=st)
            torch.cuda.synchronize(dev)
            return
        model, rows = build_model(frac, 100 + ci, dev)
        cp, _ = code_points(n, frac, 200 + ci, dev)
        d_low, d_loff = low_bytes_of(cp)
        d_utf, d_uoff = utf8_of(cp)
        nonascii = float((cp >= 0x80).float().mean().item())
        del cp
        low_bytes, utf_bytes = n * UNITS, int(d_uoff[-1].item())
        d_lab_a = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_lab_b = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_dec = torch.zeros(utf_bytes + 16, dtype=torch.uint8, device=dev)
        d_doff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_host = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_copy = torch.zeros(utf_bytes + 16, dtype=torch.uint8, device=dev)

        def a_score():
            model.score_device(d_low.data_ptr(), low_bytes, d_loff.data_ptr(), n, d_lab_a.data_ptr(), 0, st)

        def b_score_utf8():
            model.score_utf8_device(d_utf.data_ptr(), utf_bytes, d_uoff.data_ptr(), n, d_lab_b.data_ptr(), 0, st)

        def c_decode():
            utf8_decode_device(d_utf.data_ptr(), d_uoff.data_ptr(), n, d_dec.data_ptr(), d_doff.data_ptr(),
                               d_host.data_ptr(), low_bytes=True, stream=st)

        def c_memcpy():
            d_copy[:utf_bytes].copy_(d_utf[:utf_bytes], non_blocking=True)

        ms = timed([("a", a_score), ("b", b_score_utf8), ("c_decode", c_decode), ("c_memcpy", c_memcpy)], args.steps,
                   args.warmup, stream, dev)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        labels_equal = bool(torch.equal(d_lab_a, d_lab_b))
        minus_one = int((d_lab_b < 0).sum().item())
        decode_exact = bool(torch.equal(d_dec[:low_bytes], d_low[:low_bytes]) and torch.equal(d_doff, d_loff)
                            and int(d_host.sum().item()) == 0)
        # (d) host buffers: nh documents
        nh = min(args.host_docs, n)
        h_uoff = d_uoff[:nh + 1].cpu().numpy()
        h_utf = np.concatenate([d_utf[:int(h_uoff[-1])].cpu().numpy(), np.zeros(8, np.uint8)])
        raw = h_utf.tobytes()
        texts = [raw[h_uoff[i]:h_uoff[i + 1]].decode("utf-8") for i in range(nh)]   # what a String caller holds

        def d_utf8_route():
            return model.score_utf8(h_utf, h_uoff)[0]

        def d_parent_route():
            return model.score(*encoding.pack_score(texts))[0]

        d_utf8_route()
        d_parent_route()
        t_new, lab_new = host_clock(d_utf8_route, 5)
        t_old, lab_old = host_clock(d_parent_route, 3)
        host_equal = bool(np.array_equal(lab_new, lab_old) and np.array_equal(lab_new, d_lab_a[:nh].cpu().numpy()))
        line = {
            "tool": "tools/bench_utf8.py", "config": 2, "corpus": name, "nonascii_target": frac,
            "nonascii_chars": round(nonascii, 4), "docs": n, "units_per_doc": UNITS, "low_bytes": low_bytes,
            "utf8_bytes": utf_bytes, "languages": L, "gram_lengths": CFG["grams"], "table_rows": rows,
            "model": model.info(), "ms_all": ms, "ms_median": med,
            "a_score_device_docs_per_s": round(n / (med["a"] * 1e-3), 1),
            "b_score_utf8_device_docs_per_s": round(n / (med["b"] * 1e-3), 1),
            "b_minus_a_ms": round(med["b"] - med["a"], 4), "b_over_a": round(med["b"] / med["a"], 4),
            "c_decode_over_a": round(med["c_decode"] / med["a"], 4),
            "c_decode_gbytes_per_s_in_plus_out": round((utf_bytes + low_bytes) / (med["c_decode"] * 1e-3) / 1e9, 2),
            "c_memcpy_gbytes_per_s_read_plus_write": round(2 * utf_bytes / (med["c_memcpy"] * 1e-3) / 1e9, 2),
            "d_host_docs": nh, "d_score_utf8_ms_all": t_new, "d_pack_score_then_score_ms_all": t_old,
            "d_score_utf8_docs_per_s": round(nh / (float(np.median(t_new)) * 1e-3), 1),
            "d_pack_score_then_score_docs_per_s": round(nh / (float(np.median(t_old)) * 1e-3), 1),
            "d_ratio_parent_over_utf8": round(float(np.median(t_old)) / float(np.median(t_new)), 2),
            "labels_equal_a_b": labels_equal, "labels_minus_one": minus_one, "decode_equals_low_bytes": decode_exact,
            "host_labels_equal": host_equal, "provenance": _lib.provenance(),
        }
        lines.append(line)
        print(json.dumps(line), flush=True)
        failed = failed or not (labels_equal and minus_one == 0 and decode_exact and host_equal)
        model.close()
        del d_low, d_loff, d_utf, d_uoff, d_lab_a, d_lab_b, d_dec, d_doff, d_host, d_copy
        torch.cuda.empty_cache()
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if failed:
        sys.exit("bench_utf8: the UTF-8 route's labels differ from the pre-encoded route's, or a label is -1")


if __name__ == "__main__":
    main()
