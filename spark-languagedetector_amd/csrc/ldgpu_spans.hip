// ldgpu_spans.hip -- overlapping spans of every document, cut on the device
// (gfx950): the kernels around score_launch behind ldgpu_score_spans.
//
// A document of len bytes has one span if len <= width, otherwise
// 1 + ceil((len - width) / stride); span j is bytes [j stride, min(j stride +
// width, len)) of the document (include/ldgpu.h, ldgpu_score_spans).  Spans
// are numbered document by document: span_offsets[d] is the index of document
// d's first span.
//
//   span_count_kernel  spans per document, then a hipcub exclusive scan into
//                      span_offsets [n_docs + 1].
//   span_geom_kernel   for the spans [g0, g0 + nc) of a chunk: the span's
//                      document (a binary search in span_offsets: every
//                      document has a span, so the offsets strictly increase),
//                      its absolute source byte offset and its length; then a
//                      scan of the lengths into the chunk's own packed offsets
//                      coff [nc + 1].
//   span_gather_kernel span i's bytes from bytes + src[i] to out + coff[i],
//                      one wave per span, 64 consecutive bytes per step
//                      (source and destination are byte-aligned only).
//
// The gathered chunk (out, coff) is a corpus of nc documents: score_launch
// scores it like any other, so a span's bytes go through the scoring path of a
// document.
//
// Bounds: a span index at or beyond span_offsets[n_docs] is an empty span; a
// span is cut to [0, width] bytes, and one whose source range does not lie in
// [0, n_bytes) is empty -- so whatever the offsets hold, no read passes
// bytes + n_bytes and no write passes out + nc width.
#include <hipcub/hipcub.hpp>

#include "ldgpu_internal.h"

namespace ldgpu {
namespace {

constexpr int kSpanWaves = 4;  // waves (spans in flight) per workgroup of the gather

__device__ __forceinline__ int64_t span_count(int64_t len, int64_t width, int64_t stride) {
    return len <= width ? 1 : 1 + (len - width + stride - 1) / stride;
}

// cnt[d] = spans of document d; cnt[n_docs] = 0 (the scan's last input)
__global__ __launch_bounds__(256) void span_count_kernel(const int64_t* offsets, int64_t n_docs, int32_t width,
                                                         int32_t stride, int64_t* cnt) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += n)
        cnt[d] = d < n_docs ? span_count(offsets[d + 1] - offsets[d], width, stride) : 0;
}

__global__ __launch_bounds__(256) void span_geom_kernel(const SpanParams p) {
    const int64_t n = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = p.span_offsets[p.n_docs];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= p.nc; i += n) {
        int64_t src = 0, len = 0;
        const int64_t g = p.g0 + i;
        if (i < p.nc && g < total && g >= p.span_offsets[0]) {
            // the last document d in [0, n_docs) with span_offsets[d] <= g
            int64_t lo = 0, hi = p.n_docs - 1;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo + 1) / 2;
                if (p.span_offsets[mid] <= g)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const int64_t b = p.offsets[lo], dlen = p.offsets[lo + 1] - b;
            const int64_t s = (g - p.span_offsets[lo]) * p.stride;
            src = b + s;
            len = (s + p.width < dlen ? s + p.width : dlen) - s;
            if (len > p.width) len = p.width;
            if (len < 0 || src < 0 || src > p.n_bytes - len) len = 0;
            if (len == 0) src = 0;
        }
        if (i < p.nc) p.src[i] = src;
        p.len[i] = len;
    }
}

__global__ __launch_bounds__(kSpanWaves * 64) void span_gather_kernel(const SpanParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t nw = (int64_t)gridDim.x * kSpanWaves;
    for (int64_t i = (int64_t)blockIdx.x * kSpanWaves + (threadIdx.x >> 6); i < p.nc; i += nw) {
        const int64_t c0 = p.coff[i], len = p.coff[i + 1] - c0;
        const uint8_t* s = p.bytes + p.src[i];
        uint8_t* o = p.out + c0;
        for (int64_t k = lane; k < len; k += 64) o[k] = s[k];
    }
}

int flat_grid(int64_t n, int cus) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)cus * 8));
}

}  // namespace

hipError_t span_scan_bytes(int64_t n_items, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int)n_items,
                                            nullptr);
}

hipError_t launch_span_offsets(const int64_t* offsets, int64_t n_docs, int32_t width, int32_t stride, int64_t* cnt,
                               int64_t* span_offsets, void* scan_tmp, size_t scan_bytes, int cus, hipStream_t stream) {
    hipLaunchKernelGGL(span_count_kernel, dim3(flat_grid(n_docs + 1, cus)), dim3(256), 0, stream, offsets, n_docs,
                       width, stride, cnt);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, span_offsets, (int)(n_docs + 1), stream);
}

hipError_t launch_span_gather(const SpanParams& p, void* scan_tmp, size_t scan_bytes, int cus, hipStream_t stream) {
    if (p.nc <= 0) return hipSuccess;
    hipLaunchKernelGGL(span_geom_kernel, dim3(flat_grid(p.nc + 1, cus)), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, p.len, p.coff, (int)(p.nc + 1), stream);
    if (e != hipSuccess) return e;
    const int64_t want = (p.nc + kSpanWaves - 1) / kSpanWaves;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 32));
    hipLaunchKernelGGL(span_gather_kernel, dim3(grid), dim3(kSpanWaves * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ldgpu
