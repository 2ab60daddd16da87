// ldgpu_utf8.hip -- UTF-8 documents to UTF-16 code units, or to the SCORE
// encoding (the low byte of each unit), on the device (gfx950).
//
// Reference: FIT counts a text's UTF-8 bytes (LanguageDetector.scala:37), SCORE
// scans the low byte of every UTF-16 code unit (LanguageDetectorModel.scala:161).
// A caller that stores UTF-8 hands its buffer over as it is; this file is the
// decoder in front of ldgpu_preprocess_device (units) and ldgpu_score_device
// (low bytes).  The rule (include/ldgpu.h UTF-8): a document is decoded iff it
// is well-formed by Unicode Table 3-7; an ill-formed one gets host[d] = 1 and
// an empty output.
//
// One wave per document, kUtf8Step = 256 bytes per step: lane l holds the
// 4-byte-aligned dword l of the step (the document's first step is aligned
// down, bytes outside [b, e) are masked by position), the followers of its
// last bytes come from lane l + 1's dword (lane 63: from the next step's, which
// is loaded one step ahead anyway).  Three passes as in ldgpu_pre.hip: lengths
// and validity, a device scan, the write.
//
// Validity in one sweep: every lead byte checks its own followers (the second
// byte's range for E0 / ED / F0 / F4, plain continuations otherwise, all inside
// the document).  A follower is a continuation and hence no lead, so sequences
// never overlap; the document is well-formed iff every lead passes and the
// lengths of all leads sum to the document's length -- the sum catches every
// continuation byte no lead claimed, so a continuation needs no look-behind.
#include <hipcub/hipcub.hpp>

#include "../../include/ldgpu.h"
#include "ldgpu_internal.h"

namespace ldgpu {
namespace {

constexpr int kUtf8Waves = 4;

// sequence length a lead byte announces: 1..4; 0 for a continuation byte
// (80..BF), -1 for a byte that no well-formed text holds (C0, C1, F5..FF)
__device__ __forceinline__ int utf8_lead_len(uint32_t c) {
    if (c < 0x80u) return 1;
    if (c < 0xC0u) return 0;
    if (c < 0xC2u) return -1;
    if (c < 0xE0u) return 2;
    if (c < 0xF0u) return 3;
    return c < 0xF5u ? 4 : -1;
}

// the followers of lead c (n = 2..4 bytes in all) are those of Table 3-7
__device__ __forceinline__ bool utf8_followers_ok(uint32_t c, int n, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (c == 0xE0u) lo = 0xA0u;   // no overlong 3-byte form
    if (c == 0xEDu) hi = 0x9Fu;   // no surrogate
    if (c == 0xF0u) lo = 0x90u;   // no overlong 4-byte form
    if (c == 0xF4u) hi = 0x8Fu;   // nothing beyond U+10FFFF
    bool ok = c1 >= lo && c1 <= hi;
    if (n >= 3) ok = ok && (c2 & 0xC0u) == 0x80u;
    if (n >= 4) ok = ok && (c3 & 0xC0u) == 0x80u;
    return ok;
}

// dword i of the buffer when it holds a byte below `end` (the document's end:
// at most d_offsets[n_docs], so the load stays below that rounded up to 4)
__device__ __forceinline__ uint32_t utf8_dword(const uint32_t* w, int64_t i, int64_t end) {
    return i * 4 < end ? w[i] : 0u;
}

// A step's bytes as lane-local 8-byte windows: the lane's dword and the one
// after it (the next lane's; lane 63: lane 0's of the next step).
__device__ __forceinline__ uint64_t utf8_window(uint32_t cur, uint32_t next_step, int lane) {
    uint32_t nxt = (uint32_t)__shfl_down((int)cur, 1);
    const uint32_t first_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_step);
    if (lane == 63) nxt = first_next;
    return (uint64_t)cur | ((uint64_t)nxt << 32);
}

// pass 1: units per document, and the ill-formed documents
__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_len_kernel(const Utf8Params p, int64_t* len_out) {
    const int lane = threadIdx.x & 63;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(p.utf8);
    const int64_t stride = (int64_t)gridDim.x * kUtf8Waves;
    for (int64_t d = (int64_t)blockIdx.x * kUtf8Waves + (threadIdx.x >> 6); d < p.n_docs; d += stride) {
        const int64_t b = p.offsets[d], e = p.offsets[d + 1];
        uint64_t claimed = 0, units = 0;  // this lane's sums: bytes its leads claim, units they give
        bool bad = false;
        int64_t dw = (b >> 2) + lane;     // the lane's dword of the step
        uint32_t cur = utf8_dword(words, dw, e);
        for (int64_t a = b & ~(int64_t)3; a < e && !bad; a += kUtf8Step, dw += 64) {
            const uint32_t ahead = utf8_dword(words, dw + 64, e);
            const uint64_t win = utf8_window(cur, ahead, lane);
            const int64_t pos0 = a + 4 * lane;
            bool lane_bad = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t pos = pos0 + j;
                const uint32_t q = (uint32_t)(win >> (8 * j));  // the byte and its three followers
                const uint32_t c = q & 0xFFu;
                const int n = utf8_lead_len(c);
                if (pos >= b && pos < e) {
                    if (n < 0 || pos + n > e ||
                        (n >= 2 && !utf8_followers_ok(c, n, (q >> 8) & 0xFFu, (q >> 16) & 0xFFu, q >> 24)))
                        lane_bad = true;
                    else {
                        claimed += (uint64_t)n;
                        units += n == 4 ? 2u : (n > 0 ? 1u : 0u);
                    }
                }
            }
            bad = __ballot(lane_bad) != 0ull;
            cur = ahead;
        }
        // wave adds of the two sums (every lane ends with the totals)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            claimed += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)claimed, s)) |
                       ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(claimed >> 32), s) << 32);
            units += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)units, s)) |
                     ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(units >> 32), s) << 32);
        }
        const bool host = bad || claimed != (uint64_t)(e - b);
        if (lane == 0) {
            len_out[d] = host ? 0 : (int64_t)units;
            p.host[d] = host ? 1 : 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len_out[p.n_docs] = 0;
}

// pass 3: the units (or their low bytes) of every well-formed document, at
// out_off[d].  A lane's four bytes give 0..5 units (three 1-byte characters and
// a 4-byte lead), so its write rank is the sum over k = 1..5 of
// mbcnt(ballot(units >= k)) -- the two-ballot rank of one lead per lane, taken
// over the lane's count -- and the step's total the sum of those popcounts.
template <bool kLowBytes>
__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_write_kernel(const Utf8Params p, const int64_t* out_off) {
    const int lane = threadIdx.x & 63;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(p.utf8);
    const int64_t stride = (int64_t)gridDim.x * kUtf8Waves;
    for (int64_t d = (int64_t)blockIdx.x * kUtf8Waves + (threadIdx.x >> 6); d < p.n_docs; d += stride) {
        if (p.host[d]) continue;
        const int64_t b = p.offsets[d], e = p.offsets[d + 1];
        int64_t o = out_off[d];
        int64_t dw = (b >> 2) + lane;
        uint32_t cur = utf8_dword(words, dw, e);
        for (int64_t a = b & ~(int64_t)3; a < e; a += kUtf8Step, dw += 64) {
            const uint32_t ahead = utf8_dword(words, dw + 64, e);
            const uint64_t win = utf8_window(cur, ahead, lane);
            const int64_t pos0 = a + 4 * lane;
            uint32_t u[5] = {0u, 0u, 0u, 0u, 0u};
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t pos = pos0 + j;
                const uint32_t q = (uint32_t)(win >> (8 * j));
                const uint32_t c = q & 0xFFu, c1 = (q >> 8) & 0x3Fu, c2 = (q >> 16) & 0x3Fu, c3 = (q >> 24) & 0x3Fu;
                const int n = pos >= b && pos < e ? utf8_lead_len(c) : 0;
                // (static indices only: a lane's units stay in registers)
                uint32_t first = c, second = 0;
                if (n == 2) first = ((c & 0x1Fu) << 6) | c1;
                if (n == 3) first = ((c & 0x0Fu) << 12) | (c1 << 6) | c2;
                if (n == 4) {
                    const uint32_t v = (((c & 0x07u) << 18) | (c1 << 12) | (c2 << 6) | c3) - 0x10000u;
                    first = 0xD800u + (v >> 10);
                    second = 0xDC00u + (v & 0x3FFu);
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    if (n >= 1 && cnt == k) u[k] = first;
                    if (n == 4 && cnt + 1 == k) u[k] = second;
                }
                cnt += n == 4 ? 2 : (n >= 1 ? 1 : 0);
            }
            uint32_t rank = 0, total = 0;
#pragma unroll
            for (int k = 1; k <= 5; ++k) {
                const uint64_t m = __ballot(cnt >= k);
                rank += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                total += (uint32_t)__popcll(m);
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (k < cnt) {
                    if (kLowBytes)
                        static_cast<uint8_t*>(p.out)[o + rank + k] = (uint8_t)u[k];
                    else
                        static_cast<uint16_t*>(p.out)[o + rank + k] = (uint16_t)u[k];
                }
            }
            o += total;
            cur = ahead;
        }
    }
}

// labels[d] = -1 for every document flagged ill-formed
__global__ void utf8_label_kernel(const uint8_t* host, int64_t n, int32_t* labels) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += stride)
        if (host[d]) labels[d] = -1;
}

// ---- spans of UTF-8 documents (include/ldgpu.h UTF-8: top-k, spans, segments)
// len[d]: in, document d's units (pass 1; 0 for an ill-formed one); out, its
// spans.  units (nullable) [n_docs]: the unit count, -1 for an ill-formed one.
__global__ __launch_bounds__(256) void utf8_span_count_kernel(int64_t* len, const uint8_t* host, int64_t n_docs,
                                                              int32_t width, int32_t stride, int64_t* units) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += n) {
        const int64_t u = len[d];
        if (units) units[d] = host[d] ? -1 : u;
        len[d] = u <= width ? 1 : 1 + (u - width + stride - 1) / stride;
    }
}

// Every span's start as a byte index into its document: span j of a document
// starts at unit j stride, and its start is the position of the lead byte that
// unit belongs to (both units of a 4-byte lead belong to it).  A kernel of its
// own in the shape of the write pass -- one wave per well-formed document, a
// dword per lane and step, the same masks and the same five-ballot unit rank
// -- which needs the leads alone: a lead's length says how many units it
// gives, so no follower is looked at and nothing is decoded.
//
// The wave keeps the next span start (unit nu = nj stride) across the steps:
// a step holding the units [o, o + total) has a start iff nu < o + total, a
// wave-uniform test, and only such a step divides (a lane's unit minus the
// step's first start, below 2^9, by stride); with stride beyond a step's units
// most steps skip all of it.  The loop ends with the document's last span:
// the spans' starts lie below u - width + stride, so the tail is not read.
__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_starts_kernel(const Utf8StartParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(p.utf8);
    const int64_t nw = (int64_t)gridDim.x * kUtf8Waves;
    const uint32_t stride = (uint32_t)p.stride;
    for (int64_t d = (int64_t)blockIdx.x * kUtf8Waves + (threadIdx.x >> 6); d < p.n_docs; d += nw) {
        if (p.host[d]) continue;
        const int64_t b = p.offsets[d], e = p.offsets[d + 1];
        const int64_t s0 = p.span_offsets[d];
        if (s0 < 0 || s0 >= p.n_spans) continue;
        // the document's spans, cut to the array
        const int64_t s1 = p.span_offsets[d + 1];
        const int64_t ns = (s1 < p.n_spans ? s1 : p.n_spans) - s0;
        int64_t o = 0;           // units before this step
        int64_t nu = 0, nj = 0;  // the next span start: unit nu of span nj
        int64_t dw = (b >> 2) + lane;
        uint32_t cur = utf8_dword(words, dw, e);
        for (int64_t a = b & ~(int64_t)3; a < e && nj < ns; a += kUtf8Step, dw += 64) {
            const uint32_t ahead = utf8_dword(words, dw + 64, e);
            const int64_t pos0 = a + 4 * lane;
            int n[4];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t pos = pos0 + j;
                n[j] = pos >= b && pos < e ? utf8_lead_len((cur >> (8 * j)) & 0xFFu) : 0;
                cnt += n[j] == 4 ? 2 : (n[j] >= 1 ? 1 : 0);
            }
            uint32_t rank = 0, total = 0;
#pragma unroll
            for (int k = 1; k <= 5; ++k) {
                const uint64_t m = __ballot(cnt >= k);
                rank += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                total += (uint32_t)__popcll(m);
            }
            const int64_t end = o + (int64_t)total;
            if (nu < end) {
                const uint32_t first = (uint32_t)(nu - o);  // the step's first start, in units of the step
                uint32_t r = rank;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int units = n[j] == 4 ? 2 : (n[j] >= 1 ? 1 : 0);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const uint32_t ru = r + (uint32_t)t;
                        if (t < units && ru >= first) {
                            const uint32_t q = (ru - first) / stride;
                            if (q * stride == ru - first && nj + (int64_t)q < ns)
                                p.starts[s0 + nj + (int64_t)q] = pos0 + j - b;
                        }
                    }
                    r += (uint32_t)units;
                }
                const int64_t k = (int64_t)((uint32_t)(end - 1 - nu) / stride) + 1;  // the step's starts
                nj += k;
                nu += k * (int64_t)stride;
            }
            o = end;
            cur = ahead;
        }
    }
}

// start 0 where no lead writes one: span 0 of an empty or ill-formed document,
// and the entries at and beyond span_offsets[n_docs]
__global__ __launch_bounds__(256) void utf8_start_fill_kernel(const Utf8StartParams p) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t d = t; d < p.n_docs; d += n) {
        const int64_t s = p.span_offsets[d];
        if ((p.host[d] || p.offsets[d + 1] <= p.offsets[d]) && s >= 0 && s < p.n_spans) p.starts[s] = 0;
    }
    const int64_t total = p.span_offsets[p.n_docs];
    for (int64_t g = (total > 0 ? total : 0) + t; g < p.n_spans; g += n) p.starts[g] = 0;
}

__global__ __launch_bounds__(256) void utf8_span_label_kernel(const uint8_t* host, const int64_t* span_offsets,
                                                              int64_t n_docs, int64_t n_spans, int32_t* labels) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += n) {
        const int64_t s = span_offsets[d];
        if (host[d] && s >= 0 && s < n_spans) labels[s] = -1;
    }
}

__global__ __launch_bounds__(256) void utf8_topk_label_kernel(const uint8_t* host, int64_t n_docs, int32_t k,
                                                              int32_t* top_labels, double* top_scores) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += n) {
        if (!host[d]) continue;
        for (int32_t i = 0; i < k; ++i) {
            top_labels[d * k + i] = -1;
            if (top_scores) top_scores[d * k + i] = 0.0;
        }
    }
}

int utf8_grid(int64_t n, int cus) {
    const int64_t want = (n + kUtf8Waves - 1) / kUtf8Waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 8));
}

int utf8_flat_grid(int64_t n, int cus) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)cus * 8));
}

}  // namespace

hipError_t launch_utf8_decode(const Utf8Params& p, int64_t* len_tmp, int64_t* out_off, void* scan_tmp,
                              size_t* scan_bytes, int cus, hipStream_t stream) {
    if (!scan_tmp) return hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, len_tmp, out_off, (int)(p.n_docs + 1), stream);
    if (p.n_docs <= 0) return hipMemsetAsync(out_off, 0, sizeof(int64_t), stream);
    const int grid = utf8_grid(p.n_docs, cus);
    hipLaunchKernelGGL(utf8_len_kernel, dim3(grid), dim3(kUtf8Waves * 64), 0, stream, p, len_tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, *scan_bytes, len_tmp, out_off, (int)(p.n_docs + 1), stream);
    if (e != hipSuccess) return e;
    if (p.flags & LDGPU_PRE_LOW_BYTES)
        hipLaunchKernelGGL(utf8_write_kernel<true>, dim3(grid), dim3(kUtf8Waves * 64), 0, stream, p, out_off);
    else
        hipLaunchKernelGGL(utf8_write_kernel<false>, dim3(grid), dim3(kUtf8Waves * 64), 0, stream, p, out_off);
    return hipGetLastError();
}

hipError_t launch_utf8_labels(const uint8_t* host, int64_t n_docs, int32_t* labels, int cus, hipStream_t stream) {
    if (n_docs <= 0) return hipSuccess;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_docs + 255) / 256, (int64_t)cus * 8));
    hipLaunchKernelGGL(utf8_label_kernel, dim3(grid), dim3(256), 0, stream, host, n_docs, labels);
    return hipGetLastError();
}

hipError_t launch_utf8_span_offsets(const Utf8Params& p, int32_t width, int32_t stride, int64_t* len_tmp,
                                    int64_t* span_offsets, int64_t* units, void* scan_tmp, size_t* scan_bytes,
                                    int cus, hipStream_t stream) {
    if (!scan_tmp)
        return hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, len_tmp, span_offsets, (int)(p.n_docs + 1), stream);
    if (p.n_docs <= 0) return hipMemsetAsync(span_offsets, 0, sizeof(int64_t), stream);
    hipLaunchKernelGGL(utf8_len_kernel, dim3(utf8_grid(p.n_docs, cus)), dim3(kUtf8Waves * 64), 0, stream, p, len_tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(utf8_span_count_kernel, dim3(utf8_flat_grid(p.n_docs, cus)), dim3(256), 0, stream, len_tmp,
                       p.host, p.n_docs, width, stride, units);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, *scan_bytes, len_tmp, span_offsets, (int)(p.n_docs + 1), stream);
}

hipError_t launch_utf8_starts(const Utf8StartParams& p, int cus, hipStream_t stream) {
    if (!p.starts || p.n_spans <= 0) return hipSuccess;
    if (p.n_docs > 0) {
        hipLaunchKernelGGL(utf8_starts_kernel, dim3(utf8_grid(p.n_docs, cus)), dim3(kUtf8Waves * 64), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(utf8_start_fill_kernel, dim3(utf8_flat_grid(std::max(p.n_docs, p.n_spans), cus)), dim3(256), 0,
                       stream, p);
    return hipGetLastError();
}

hipError_t launch_utf8_span_labels(const uint8_t* host, const int64_t* span_offsets, int64_t n_docs, int64_t n_spans,
                                   int32_t* labels, int cus, hipStream_t stream) {
    if (n_docs <= 0 || n_spans <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_span_label_kernel, dim3(utf8_flat_grid(n_docs, cus)), dim3(256), 0, stream, host,
                       span_offsets, n_docs, n_spans, labels);
    return hipGetLastError();
}

hipError_t launch_utf8_topk_labels(const uint8_t* host, int64_t n_docs, int32_t k, int32_t* top_labels,
                                   double* top_scores, int cus, hipStream_t stream) {
    if (n_docs <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_topk_label_kernel, dim3(utf8_flat_grid(n_docs, cus)), dim3(256), 0, stream, host, n_docs, k,
                       top_labels, top_scores);
    return hipGetLastError();
}

}  // namespace ldgpu
