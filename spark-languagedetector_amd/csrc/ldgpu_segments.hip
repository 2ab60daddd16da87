// ldgpu_segments.hip -- smoothed span labels: a best path over a document's
// spans with a cost per language change (gfx950).  The rule (include/ldgpu.h,
// ldgpu_score_segments; languagedetection/segments.py restates it), for a
// document's spans 0 .. n-1 with score rows s_j[0..L):
//
//   first_max(v): m = v[0], a = 0; for l = 1 .. L-1: if (v[l] > m) { m = v[l]; a = l; }
//   dp_0[l] = s_0[l];  (m_j, a_j) = first_max(dp_j)
//   j >= 1, t = m_{j-1} - penalty:
//     switch_j[l] = (t > dp_{j-1}[l])
//     dp_j[l]     = s_j[l] + (switch_j[l] ? t : dp_{j-1}[l])
//   y_{n-1} = a_{n-1};  y_{j-1} = switch_j[y_j] ? a_{j-1} : y_j
//
// Only fp64 subtractions, additions and `>` appear: there is no multiply, so
// nothing can contract into an FMA (contraction is switched off below all the
// same).
//
//   segment_forward_kernel    the spans [g0, g0 + nc) of one scored chunk, one
//                             wave per document with a span in it, lane t
//                             owning the languages t + 64 s.  Per span: the
//                             switch bits as one ballot word per 64 languages
//                             (sw) and a_j (arg).  dp lives in registers for
//                             L <= 256 (S = ceil(L / 64) values per lane) and
//                             in LDS beyond (S = 0: one wave per workgroup, L
//                             doubles; a lane reads and writes its own
//                             languages only, so no barrier is needed).
//   segment_backtrace_kernel  after the last chunk, one wave per document: the
//                             spans backwards 64 at a time, a ballot finding
//                             the nearest span that switches under the current
//                             label.
//
// first_max across the wave is wave_pick over topk_key (ldgpu_wave.h).  That
// it equals the sequential `>` scan:
//   * the scan keeps index a until some later v[l] > v[a] holds, so it returns
//     the smallest index among the maxima of the order "x before y iff x > y";
//     wave_pick returns the smallest index among the maximal keys, and for
//     non-NaN values key(x) > key(y) iff x > y: the key is the IEEE bit
//     pattern made monotone (negative values complemented, the others with
//     the sign bit set), -inf and +inf included as the least and greatest;
//   * -0.0 and +0.0 map to one key: neither is > the other, the scan keeps the
//     earlier one -- the smaller index among equal keys;
//   * a NaN at index 0: no v[l] > NaN holds, the scan returns 0; its key ~0 is
//     above every other key (index 0 is the smallest index anyway);
//   * a NaN at l > 0: NaN > m never holds, the scan passes it; its key 1 is
//     below every key of index 0 (>= -inf's 2^52 - 1), so it never wins;
//   * a lane's language l >= L has key 0, below every key of a real element,
//     and index 0 is always a real element: it never wins.
// m is read from the winning lane's own value, bit for bit (a -0.0 maximum
// stays -0.0, a NaN at index 0 stays that NaN).
//
// Carry between chunks: a chunk may begin inside one document and end inside
// another.  The entering document's dp comes from carry_in, the leaving one's
// goes to carry_out; the host alternates the two rows by chunk parity, so
// within one launch the row read and the row written differ, and launches are
// ordered on the stream.  m is not carried: first_max of the carried dp gives
// it again.
//
// Bounds: a span index at or beyond min(span_offsets[n_docs], n_spans) is
// neither read nor written by the forward kernel and gets label 0 from the
// backtrace; every index into scores, sw, arg and labels is clamped to the
// chunk or to n_spans whatever span_offsets holds, and a label read back from
// arg is clamped to [0, L).
#include <algorithm>

#include "ldgpu_internal.h"
#include "ldgpu_wave.h"

#pragma clang fp contract(off)

namespace ldgpu {
namespace {

constexpr int kSegWaves = 4;  // waves (documents in flight) per workgroup; the LDS form runs one

// the last document d in [0, n_docs) with span_offsets[d] <= g (n_docs >= 1)
__device__ __forceinline__ int64_t seg_doc_of(const int64_t* so, int64_t n_docs, int64_t g) {
    int64_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (so[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

struct LaneBest {
    uint64_t key;
    int idx;
    double val;
};
__device__ __forceinline__ void lane_take(LaneBest& b, double v, int l, bool in) {
    const uint64_t q = in ? topk_key(v, l) : 0ull;
    if (q > b.key) {  // strictly: a lane keeps the smaller of its indices among equal keys
        b.key = q;
        b.idx = l;
        b.val = v;
    }
}
// (m, a) of the wave's dp from every lane's best; wave-uniform
__device__ __forceinline__ int wave_first_max(const LaneBest& b, double* m) {
    const Pick w = wave_pick(b.key, b.idx);
    *m = rdlaned(b.val, w.idx & 63);
    return w.idx;
}

template <int S>
__global__ __launch_bounds__(S > 0 ? kSegWaves * 64 : 64) void segment_forward_kernel(const SegmentParams p) {
    extern __shared__ double lds_dp[];  // S == 0: L doubles
    constexpr int kWaves = S > 0 ? kSegWaves : 1;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int L = p.L, W = (L + 63) >> 6;
    const int64_t* so = p.span_offsets;
    if (p.n_docs < 1) return;
    const int64_t gbeg = std::max(p.g0, so[0]);
    const int64_t gend = std::min(std::min(p.g0 + p.nc, so[p.n_docs]), p.n_spans);
    if (gend <= gbeg) return;
    const int64_t dA = seg_doc_of(so, p.n_docs, gbeg), dB = seg_doc_of(so, p.n_docs, gend - 1);
    const double penalty = p.penalty;
    for (int64_t d = dA + (int64_t)blockIdx.x * kWaves + wave; d <= dB; d += (int64_t)gridDim.x * kWaves) {
        const int64_t s0 = so[d], s1 = so[d + 1];
        const int64_t a = std::max(s0, gbeg), b = std::min(s1, gend);
        if (b <= a) continue;
        const double* row = p.scores + (a - p.g0) * L;
        double m = 0.0;
        if constexpr (S > 0) {
            double dp[S], cur[S], nxt[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int l = 64 * s + lane;
                cur[s] = l < L ? row[l] : 0.0;
                dp[s] = 0.0;
                nxt[s] = 0.0;
            }
            if (a != s0) {  // the document entered the chunk: its dp, and m again from it
                LaneBest best{0ull, 0, 0.0};
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int l = 64 * s + lane;
                    dp[s] = l < L ? p.carry_in[l] : 0.0;
                    lane_take(best, dp[s], l, l < L);
                }
                (void)wave_first_max(best, &m);
            }
            for (int64_t g = a; g < b; ++g) {
                row += L;
                if (g + 1 < b) {  // the next row's loads fly while this span's wave reduction runs
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const int l = 64 * s + lane;
                        nxt[s] = l < L ? row[l] : 0.0;
                    }
                }
                const bool head = g == s0;
                const double t = m - penalty;
                LaneBest best{0ull, 0, 0.0};
                uint64_t word = 0ull;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int l = 64 * s + lane;
                    const bool sw = !head && t > dp[s];
                    dp[s] = head ? cur[s] : cur[s] + (sw ? t : dp[s]);
                    const uint64_t bal = __builtin_amdgcn_ballot_w64(sw && l < L);
                    if (lane == s) word = bal;
                    lane_take(best, dp[s], l, l < L);
                }
                const int arg = wave_first_max(best, &m);
                if (lane < W) p.sw[g * W + lane] = word;
                if (lane == 0) p.arg[g] = arg;
#pragma unroll
                for (int s = 0; s < S; ++s) cur[s] = nxt[s];
            }
            if (b < s1) {  // the document leaves the chunk
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int l = 64 * s + lane;
                    if (l < L) p.carry_out[l] = dp[s];
                }
            }
        } else {
            if (a != s0) {
                LaneBest best{0ull, 0, 0.0};
                for (int s = 0; s < W; ++s) {
                    const int l = 64 * s + lane;
                    const double v = l < L ? p.carry_in[l] : 0.0;
                    if (l < L) lds_dp[l] = v;
                    lane_take(best, v, l, l < L);
                }
                (void)wave_first_max(best, &m);
            }
            for (int64_t g = a; g < b; ++g, row += L) {
                const bool head = g == s0;
                const double t = m - penalty;
                LaneBest best{0ull, 0, 0.0};
                uint64_t word = 0ull;  // lane s keeps word s (W <= 64)
                for (int s = 0; s < W; ++s) {
                    const int l = 64 * s + lane;
                    const bool in = l < L;
                    const double x = in ? row[l] : 0.0;
                    const double o = (in && !head) ? lds_dp[l] : 0.0;
                    const bool sw = !head && t > o;
                    const double v = head ? x : x + (sw ? t : o);
                    if (in) lds_dp[l] = v;
                    const uint64_t bal = __builtin_amdgcn_ballot_w64(sw && in);
                    if (lane == s) word = bal;
                    lane_take(best, v, l, in);
                }
                const int arg = wave_first_max(best, &m);
                if (lane < W) p.sw[g * W + lane] = word;
                if (lane == 0) p.arg[g] = arg;
            }
            if (b < s1)
                for (int l = lane; l < L; l += 64) p.carry_out[l] = lds_dp[l];
        }
    }
}

__global__ __launch_bounds__(kSegWaves * 64) void segment_backtrace_kernel(const SegmentParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int L = p.L, W = (L + 63) >> 6;
    const int64_t* so = p.span_offsets;
    // the entries beyond the corpus' spans (a caller's over-estimate of n_spans)
    const int64_t total = std::max<int64_t>(0, so[p.n_docs]);
    const int64_t nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = total + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_spans; i += nt) p.labels[i] = 0;
    for (int64_t d = (int64_t)blockIdx.x * kSegWaves + wave; d < p.n_docs; d += (int64_t)gridDim.x * kSegWaves) {
        const int64_t s0 = so[d], s1 = std::min(so[d + 1], p.n_spans);
        if (s0 < 0 || s1 <= s0) continue;
        auto label_at = [&](int64_t j) {
            const int y = __builtin_amdgcn_readfirstlane(p.arg[j]);
            return std::min(std::max(y, 0), L - 1);
        };
        int y = label_at(s1 - 1);
        for (int64_t hi = s1; hi > s0;) {
            const int64_t lo = std::max(s0, hi - 64);
            const int64_t j = lo + lane;
            const int n = (int)(hi - lo);
            int mine = 0;
            int rem = n;  // the lanes [0, rem) have no label yet
            while (rem > 0) {
                bool pred = false;
                if (lane < rem && j > s0) pred = (p.sw[j * W + (y >> 6)] >> (y & 63)) & 1ull;
                const uint64_t mask = __builtin_amdgcn_ballot_w64(pred);
                // the nearest switching span below the block's labelled part
                const int top = mask ? 63 - __builtin_clzll(mask) : 0;
                if (lane >= top && lane < rem) mine = y;
                if (!mask) break;
                y = label_at(lo + top - 1);  // top's span switched: below it the path is a_{j-1}
                rem = top;
            }
            if (lane < n) p.labels[j] = mine;
            hi = lo;
        }
    }
}

}  // namespace

hipError_t launch_segment_forward(const SegmentParams& p, int cus, hipStream_t stream) {
    if (p.nc <= 0 || p.n_docs <= 0) return hipSuccess;
    if (p.L < 1 || p.L > kTopkMaxLangs) return hipErrorInvalidValue;
    const int S = p.L <= kBlockLangs ? (p.L + 63) / 64 : 0;
    const int waves = S ? kSegWaves : 1;
    const int64_t want = (std::min(p.nc, p.n_docs) + waves - 1) / waves;  // every document has a span
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 32)));
    const dim3 block(waves * 64);
    switch (S) {
        case 1: hipLaunchKernelGGL(segment_forward_kernel<1>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(segment_forward_kernel<2>, grid, block, 0, stream, p); break;
        case 3: hipLaunchKernelGGL(segment_forward_kernel<3>, grid, block, 0, stream, p); break;
        case 4: hipLaunchKernelGGL(segment_forward_kernel<4>, grid, block, 0, stream, p); break;
        default:
            hipLaunchKernelGGL(segment_forward_kernel<0>, grid, block, sizeof(double) * (size_t)p.L, stream, p);
            break;
    }
    return hipGetLastError();
}

hipError_t launch_segment_backtrace(const SegmentParams& p, int cus, hipStream_t stream) {
    if (p.n_spans <= 0) return hipSuccess;
    if (p.L < 1 || p.L > kTopkMaxLangs) return hipErrorInvalidValue;
    const int64_t want = (std::max<int64_t>(p.n_docs, 1) + kSegWaves - 1) / kSegWaves;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 32)));
    hipLaunchKernelGGL(segment_backtrace_kernel, grid, dim3(kSegWaves * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ldgpu
