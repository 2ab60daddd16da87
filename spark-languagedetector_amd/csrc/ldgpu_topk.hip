// ldgpu_topk.hip -- top-k selection over a document's score vector, gfx950.
//
// Input: the [n][L] fp64 score matrix SCORE wrote (row stride given); output:
// per row the k best languages in order and, optionally, their scores bit for
// bit.  The order of a row s[0..L) (include/ldgpu.h, ldgpu_score_topk):
//   i before j  <=>  s[i] > s[j], or they compare equal and i < j;
//   -0.0 equals +0.0; a NaN at index 0 comes first; a NaN elsewhere comes after
//   every non-NaN value (-inf included), NaNs among themselves by index.
// Entry 0 is therefore breeze's first-maximum argmax (the label of SCORE).
//
// One wave per row, lane t owning the languages t + 64 j.  Every value maps to
// an order-preserving u64 key (topk_key); k rounds each take the wave maximum
// of the lanes' best keys by DPP (no LDS), then the smallest index among the
// lanes holding it, and the winning lane retires that element.  L <= 256: the
// row lives in registers (S = ceil(L / 64) values and keys per lane, a retired
// key becomes 0).  L > 256 (S = 0): each lane keeps only its best (key, index);
// a lane retires its elements in order, so its retired set is "everything not
// after the last one retired", and only the winning lane rescans its column.
// Lane r keeps result r: labels and scores leave in one coalesced store each.
#include <algorithm>

#include "ldgpu_internal.h"
#include "ldgpu_wave.h"

namespace ldgpu {
namespace {

constexpr int kTopkWaves = 4;  // waves (rows in flight) per workgroup

// (the order-preserving key topk_key and the wave pick: ldgpu_wave.h)

template <int S>
__global__ __launch_bounds__(kTopkWaves * 64) void topk_kernel(TopkParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nw = (int64_t)gridDim.x * kTopkWaves;
    const int L = p.L, k = p.k;
    for (int64_t row = (int64_t)blockIdx.x * kTopkWaves + wave; row < p.n; row += nw) {
        const double* src = p.scores + row * p.stride;
        int my_label = 0;
        double my_score = 0.0;
        if constexpr (S > 0) {
            double v[S];
            uint64_t key[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int l = 64 * s + lane;
                v[s] = l < L ? src[l] : 0.0;
                key[s] = l < L ? topk_key(v[s], l) : 0ull;
            }
            for (int r = 0; r < k; ++r) {
                uint64_t bk = key[0];
                int bi = lane;
#pragma unroll
                for (int s = 1; s < S; ++s)
                    if (key[s] > bk) {
                        bk = key[s];
                        bi = 64 * s + lane;
                    }
                const Pick w = wave_pick(bk, bi);
                const int ws = w.idx >> 6, wl = w.idx & 63;  // wave-uniform
                double wv = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (ws == s) {
                        wv = rdlaned(v[s], wl);
                        if (lane == wl) key[s] = 0ull;
                    }
                if (lane == r) {
                    my_label = w.idx;
                    my_score = wv;
                }
            }
        } else {
            uint64_t bk = 0ull;
            int bi = 0;
            for (int l = lane; l < L; l += 64) {
                const uint64_t q = topk_key(src[l], l);
                if (q > bk) {
                    bk = q;
                    bi = l;
                }
            }
            for (int r = 0; r < k; ++r) {
                const Pick w = wave_pick(bk, bi);
                if (lane == r) my_label = w.idx;
                if (lane == (w.idx & 63)) {
                    // this lane's next: its greatest element after (M, idx)
                    bk = 0ull;
                    bi = 0;
                    for (int l = lane; l < L; l += 64) {
                        const uint64_t q = topk_key(src[l], l);
                        const bool after = q < w.key || (q == w.key && l > w.idx);
                        if (after && q > bk) {
                            bk = q;
                            bi = l;
                        }
                    }
                }
            }
            if (p.top_scores && lane < k) my_score = src[my_label];
        }
        if (lane < k) {
            p.top_labels[row * k + lane] = my_label;
            if (p.top_scores) p.top_scores[row * k + lane] = my_score;
        }
    }
}

}  // namespace

hipError_t launch_topk(const TopkParams& p, int cus, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    if (p.L < 1 || p.L > kTopkMaxLangs || p.k < 1 || p.k > p.L || p.k > kMaxTopk || p.stride < p.L)
        return hipErrorInvalidValue;
    const int64_t want = (p.n + kTopkWaves - 1) / kTopkWaves;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 16)));
    const dim3 block(kTopkWaves * 64);
    switch (p.L <= kBlockLangs ? (p.L + 63) / 64 : 0) {
        case 1: hipLaunchKernelGGL(topk_kernel<1>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(topk_kernel<2>, grid, block, 0, stream, p); break;
        case 3: hipLaunchKernelGGL(topk_kernel<3>, grid, block, 0, stream, p); break;
        case 4: hipLaunchKernelGGL(topk_kernel<4>, grid, block, 0, stream, p); break;
        default: hipLaunchKernelGGL(topk_kernel<0>, grid, block, 0, stream, p); break;
    }
    return hipGetLastError();
}

}  // namespace ldgpu
