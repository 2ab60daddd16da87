// ldgpu_trie.hip -- SCORE count mode on an exact LDS trie (gfx950).
//
// A count-mode table whose keys all have at most kTrieMaxLen bytes and name one
// language each, and whose byte trie packs into the LDS two workgroups per CU
// leave (ldgpu_trie.h: layout and builder), is scored without Bloom filter,
// candidate queue, verify or global-memory lookup: every window position walks
// the trie, at most one LDS word per key length, and yields the hit and the
// language of lengths 1..4 on the way.
//
// The outer structure is score_kernel's (ldgpu_score.hip): a persistent grid of
// kScoreWaves waves per workgroup, one contiguous document range per wave,
// groups of consecutive documents staged by double-buffered LDS-DMA, the
// group's labels written in one coalesced store.  A staged document of
// maxg..256 bytes is scored in the lane-run layout, lane i owning positions
// 4 i .. 4 i + 3:
//   run bytes  bytes 0..6 of the lane's run from three staged dwords
//              (v_alignbyte by the wave-uniform base & 3), and their seven
//              scaled offsets 4 * byte: each serves up to four walks
//   depth 1    four entries of the direct table (the image's first 256 words)
//   depth d    entry.base + offset[k + d - 1], one ds_read_b32 per position,
//              the four of a depth back to back; a check byte that differs from
//              the text byte replaces the entry by the dead entry
//   counting   per depth one wave-level test "any lane holds a terminal", then
//              at most four exec-masked LDS adds of mult[depth]
//   tail       a window of N bytes at position p = 4 lane + k counts only if
//              p + N <= len, which depends on k + N alone: seven lane masks
//              in SGPRs, kept from one document to the next and rebuilt (one
//              v_cmp each) only when the length changes, and-ed into the
//              exec mask of a terminal's add -- the walks themselves run past
//              the document's end unchecked (the bytes there are the next
//              document's, or the buffer's padding)
//   label      the count argmax (first maximum), as score_kernel's
// A table in the path-sum form (ldgpu_trie.h: one language and a count of at
// most 4 per root path; trie_kernel<1, maxlen, kFormSum>) is counted once per
// window position instead of once per (position, depth): trie_doc_sum below.
// Its pair form (Wmax * L <= 63; trie_kernel<1, maxlen, kFormPair>) counts at
// the payload as it stands -- one counter per (language, W) -- and weighs the
// counters in the argmax: pair_argmax; with at most 32 languages two documents
// share a counter pass, one in each half of a counter and of the wave:
// pair_argmax2.
// Every other document -- shorter than maxg (partial windows), longer than 256
// bytes, or in a group the staging buffer does not hold -- gets label -1 and
// is appended to a list (p.left, its length counted in *p.n_left); an indirect
// launch of the mode-3 score_kernel then scores the listed documents in place
// and leaves at once when there is none (score_launch, ldgpu_api.hip).
#include "ldgpu_internal.h"
#include "ldgpu_wave.h"

namespace ldgpu {
namespace {

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint8_t lds_u8;

// what the image's entries say (ldgpu_trie.h)
constexpr int kFormPlain = 0, kFormSum = 1, kFormPair = 2;

__device__ __forceinline__ int64_t rdlane_i64(int64_t v, int l) {
    return (int64_t)((uint64_t)rdlane((uint32_t)v, l) | ((uint64_t)rdlane((uint32_t)((uint64_t)v >> 32), l) << 32));
}

// lane id recomputed in place (never spilled: see score_kernel's fresh_lane)
__device__ __forceinline__ uint32_t fresh_lane() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// LDS-DMA of a group's bytes [s0, s0 + kBufBytes) into dst (lane i's 16 B land
// at dst + 16 i), range-checked: bytes past n_bytes read as 0, never fault
__device__ __forceinline__ void group_dma(const TrieParams& p, int64_t s0, uint32_t* dst) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(p.bytes + s0));
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)(p.bytes + s0) >> 32));
    const int64_t left = ((p.n_bytes + 3) & ~(int64_t)3) - s0;
    const uint32_t nrec =
        __builtin_amdgcn_readfirstlane((uint32_t)(left < 0 ? 0 : (left > 0x7ffffff0 ? 0x7ffffff0 : left)));
    void* base = (void*)(((uint64_t)hi << 32) | lo);
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)nrec, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, 16 * fresh_lane(), 0,
                                             0, 0);
}

// the label of the document counted in cnt (first maximum of the counts: the
// fold of c adds of the table's one value is strictly monotone in c); clears
// the counters -- score_kernel's count_argmax.  Language l's counter is
// cnt[l + OFS] (the path-sum form counts at the payload's index, language + 1).
template <int S, int OFS = 0>
__device__ __forceinline__ int count_argmax(const TrieParams& p, uint32_t* cnt, int lane) {
    static_assert(OFS == 0 || S == 1, "the shifted counters are one slice");
    uint32_t best = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int l = 64 * s + lane;
        if (l < p.L) {
            const uint32_t c = cnt[l + OFS];
            cnt[l + OFS] = 0;
            const uint32_t k = p.count_sign > 0 ? c : (p.count_sign < 0 ? 0xffffffu - c : 0u);
            best = max(best, (k << 8) | (uint32_t)(255 - l));
        }
    }
    return 255 - (int)(wave_max_u32(best) & 255u);
}

// The pair form's label: language l's count is the sum over w = 1..wmax of
// w * cnt[1 + l + L (w - 1)] (consecutive words per w: no bank conflict); from
// there on count_argmax's key.  Every counter is read and cleared by ONE LDS
// exchange with 0 (the kernel stands at the LDS array's limit: a read and a
// write per w cost the array twice) -- all that a document can have touched.
// p.wmax is wave-uniform: scalar branches.
__device__ __forceinline__ uint32_t take_count(uint32_t* q) {
    return __hip_atomic_exchange(q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int pair_argmax(const TrieParams& p, uint32_t* cnt, int lane) {
    uint32_t best = 0;
    if (lane < p.L) {
        // (unrolled, shifts and adds: a loop over w, or a product by 3, compiles
        // to a 64-bit multiply-add)
        uint32_t* const q = cnt + 1 + lane;
        const uint32_t wmax = p.wmax, L = (uint32_t)p.L;
        uint32_t c = take_count(q);
        if (wmax >= 2) {
            c += take_count(q + L) << 1;
            if (wmax >= 3) {
                const uint32_t c3 = take_count(q + 2 * L);
                uint32_t c3x2 = c3 << 1;
                asm("" : "+v"(c3x2));  // (kept apart from c3: the sum would come back as the product)
                c += c3x2 + c3;
                if (wmax >= 4) c += take_count(q + 3 * L) << 2;
            }
        }
        const uint32_t k = p.count_sign > 0 ? c : (p.count_sign < 0 ? 0xffffffu - c : 0u);
        best = (k << 8) | (uint32_t)(255 - lane);
    }
    return 255 - (int)(wave_max_u32(best) & 255u);
}

// Two documents per counter pass (L <= 32; p.doc_pairs): the first document of
// a pair counted 1 and the second 0x10000 at the same counters, so a counter's
// halves hold at most 256 each, and the weighted sum, run ONCE on the packed
// word, at most 1,024 per half: nothing carries.  Lanes l < L take the counters
// as pair_argmax does (one exchange per w for BOTH documents); the high half
// goes to lanes 32 + l by one v_permlane32_swap (lanes 32..63 of its first
// operand take lanes 0..31 of its second), and each half of the wave finds its
// document's first maximum with the language lane & 31 in the key: the DPP
// maximum stops at row_bcast:15, which leaves the halves' maxima in lanes 31
// and 63.  A first document without a second (the end of a group) is labelled
// by the same pass: its high halves are 0 and lab[1] is not used.
struct PairLabels {
    int lab[2];
};
__device__ __forceinline__ PairLabels pair_argmax2(const TrieParams& p, uint32_t* cnt, int lane) {
    uint32_t c = 0;
    if (lane < p.L) {
        uint32_t* const q = cnt + 1 + lane;
        const uint32_t wmax = p.wmax, L = (uint32_t)p.L;
        c = take_count(q);
        if (wmax >= 2) {
            c += take_count(q + L) << 1;
            if (wmax >= 3) {
                const uint32_t c3 = take_count(q + 2 * L);
                uint32_t c3x2 = c3 << 1;
                asm("" : "+v"(c3x2));  // (as in pair_argmax)
                c += c3x2 + c3;
                if (wmax >= 4) c += take_count(q + 3 * L) << 2;
            }
        }
    }
    const uint32_t both = __builtin_amdgcn_permlane32_swap(c, c >> 16, false, false)[0];
    const uint32_t mine = both & 0xffffu;  // lane l: the first document's count of language l, lane 32 + l: the second's
    const uint32_t l = (uint32_t)lane & 31u;
    const uint32_t k = p.count_sign > 0 ? mine : (p.count_sign < 0 ? 0xffffffu - mine : 0u);
    uint32_t v = l < (uint32_t)p.L ? (k << 8) | (255u - l) : 0u;
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    return PairLabels{{255 - (int)(rdlane(v, 31) & 255u), 255 - (int)(rdlane(v, 63) & 255u)}};
}

// a staged label byte as the label: a language 0..253 as it stands, 0xff = -1
__device__ __forceinline__ int32_t label_of(uint8_t v) { return v == 0xffu ? -1 : (int32_t)v; }

__device__ __forceinline__ uint32_t lds_word(uint32_t byte_addr) { return *(const lds_u32*)(size_t)byte_addr; }

// The tail cut, kept from one document to the next: lane mask c - 1 = a window
// that ends c bytes after the lane's first position ends inside a document of
// `len` bytes.  Rebuilt only when the length changes (a wave-uniform compare).
struct TailCut {
    uint64_t in[7];
    int32_t len;  // the length the masks were built for (-1: none yet)
};

template <int MAXD>
__device__ __forceinline__ void tail_cut(TailCut& cut, int32_t len, int lane) {
    if (cut.len == len) return;
    const int32_t left = len - 4 * lane;
#pragma unroll
    for (int c = 1; c <= 3 + MAXD; ++c) cut.in[c - 1] = __builtin_amdgcn_ballot_w64(left >= c);
    cut.len = len;
}

// the terminals of depth D among the lane's four entries, counted
template <int D>
__device__ __forceinline__ void count_depth(const TrieParams& p, uint32_t* cnt, const uint32_t (&e)[4],
                                            const TailCut& cut, uint32_t inc) {
    // one wave-level test: a byte of 0xff in all four entries = no terminal
    // (a terminal past the document's end only keeps the wave on this path)
    const uint32_t all = e[0] & e[1] & e[2] & e[3];
    if (!__builtin_amdgcn_ballot_w64(__builtin_amdgcn_ubfe(all, 8, 8) != kTrieNoLang)) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lang = __builtin_amdgcn_ubfe(e[k], 8, 8);
        const bool in = __builtin_amdgcn_inverse_ballot_w64(cut.in[k + D - 1]);
        if (lang != kTrieNoLang && in)
            __hip_atomic_fetch_add(&cnt[lang], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// the pair form's count: inc (1; the second document of a pair: 0x10000) more
// at the counter's LDS byte address
__device__ __forceinline__ void pair_count(uint32_t addr, uint32_t inc) {
    __hip_atomic_fetch_add((lds_u32*)(size_t)addr, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The path-sum form (ldgpu_trie.h), from the run bytes on: every node's payload
// says what the whole path to it counts, so a walk is counted once, at the
// deepest node it reaches inside the document.
//   step d -> d + 1   live = check == text byte && the window of d + 1 bytes
//              ends inside the document (cut.in[k + d], and-ed into the
//              compare's lane mask); a walk that is not live goes dead
//   slot k     m = the maximum over the slot's entries of all depths (whole
//              entries order by payload, and the payload grows along a path);
//              payload(m) != 0 and position 4 lane + k inside the document
//              (cut.in[k]: the depth-1 read is unchecked): one LDS add of the
//              payload's weight at the payload's counter (language + 1 <= 63);
//              the pair form: an add of inc at cnt + payload, the payload being
//              the byte offset of the pair's counter (cnt_addr: the counters'
//              LDS byte address, wave-uniform)
// p.mult is not read: the weights are in the image.  The label is the caller's.
template <int MAXD, bool PAIR>
__device__ __forceinline__ void trie_doc_sum(uint32_t dead, uint32_t* cnt, uint32_t cnt_addr, const uint32_t (&b)[7],
                                             const uint32_t (&off)[7], const TailCut& cut, uint32_t inc) {
    uint32_t e[4], m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = e[k] = lds_word(off[k]);  // (the direct table at LDS address 0: no check)
    bool live[4] = {true, true, true, true};
#pragma unroll
    for (int d = 1; d < MAXD; ++d) {
        // The step to depth 4 only in the lanes where a walk is still live (about
        // one in eight on text): the other lanes' reads of the dead row took part
        // in the banking for nothing.  The test is three s_or_b64 of the previous
        // step's lane masks.  One branch for the four reads, never one per slot.
        // (The same branch around the step to depth 3 measured 6 % slower; every
        // read from depth 3 on under its slot's own live lane mask, 1.7 % slower
        // in six alternating runs: DESIGN.md.)
        if (d == 3 && !(live[0] | live[1] | live[2] | live[3])) continue;
        uint32_t n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] = lds_word((e[k] & 0xffffu) + off[k + d]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = __builtin_amdgcn_inverse_ballot_w64(cut.in[k + d]);
            live[k] = __builtin_amdgcn_ubfe(n[k], 16, 8) == b[k + d] && in;
            e[k] = live[k] ? n[k] : dead;
            m[k] = max(m[k], e[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pay = m[k] >> 24;
        const bool in = __builtin_amdgcn_inverse_ballot_w64(cut.in[k]);
        if (pay != 0 && in) {
            if constexpr (PAIR)
                pair_count(cnt_addr + pay, inc);
            else
                __hip_atomic_fetch_add(&cnt[pay & 63u], (pay >> 6) + 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// One staged document of maxg..256 bytes at byte `base` of the wave's buffer.
// FORM: what the image's entries say.  Returns the document's label; the pair
// form only counts (inc at each counter) and returns 0: the label is the
// document loop's, once per document or once per two (trie_kernel).
template <int S, int MAXD, int FORM>
__device__ __forceinline__ int trie_doc(const TrieParams& p, uint32_t dead, uint32_t* cnt, uint32_t cnt_addr,
                                        const uint32_t* buf, uint32_t base, int32_t len, int lane, TailCut& cut,
                                        uint32_t inc) {
    // run bytes 0..6 of the lane's four positions.  Bound: lane 63 reads dwords
    // (base >> 2) + 63 .. + 65, within what score_kernel's lane runs read.
    const uint32_t sh = base & 3u;  // wave-uniform
    const uint32_t* w = buf + (base >> 2) + lane;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    const uint32_t r0 = __builtin_amdgcn_alignbyte(w1, w0, sh);  // run bytes 0..3
    const uint32_t r1 = __builtin_amdgcn_alignbyte(w2, w1, sh);  // 4..7
    uint32_t b[7], off[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        b[j] = ((j < 4 ? r0 : r1) >> (8 * (j & 3))) & 0xffu;
        off[j] = b[j] << 2;
    }
    tail_cut<MAXD>(cut, len, lane);
    // (run byte 6 serves one walk only, and the compiler would form that walk's
    // address from the byte with three instructions: its offset as a value,
    // like the other six)
    if constexpr (FORM != kFormPlain && MAXD == 4) asm("" : "+v"(off[6]));
    if constexpr (FORM != kFormPlain) {
        trie_doc_sum<MAXD, FORM == kFormPair>(dead, cnt, cnt_addr, b, off, cut, inc);
        if constexpr (FORM == kFormPair) return 0;
        return count_argmax<1, 1>(p, cnt, lane);
    }
    uint32_t e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = lds_word(off[k]);  // (the direct table at LDS address 0: no check)
#pragma unroll
    for (int d = 1; d <= MAXD; ++d) {
        uint32_t n[4];
        if (d < MAXD) {
            // the next depth's four reads, issued before this depth is counted
#pragma unroll
            for (int k = 0; k < 4; ++k) n[k] = lds_word((e[k] >> 16) + off[k + d]);
        }
        const uint32_t mul = p.mult[d];
        if (mul) {
            if (d == 1) count_depth<1>(p, cnt, e, cut, mul);
            if (d == 2) count_depth<2>(p, cnt, e, cut, mul);
            if (d == 3) count_depth<3>(p, cnt, e, cut, mul);
            if (d == 4) count_depth<4>(p, cnt, e, cut, mul);
        }
        if (d < MAXD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = (n[k] & 0xffu) == b[k + d] ? n[k] : dead;
        }
    }
    return count_argmax<S>(p, cnt, lane);
}

template <int S, int MAXD, int FORM>
__global__ __launch_bounds__(kScoreWaves * 64, kScoreMinWgPerCu * kScoreWaves / 4) void trie_kernel(const TrieParams p) {
    static_assert(FORM == kFormPlain || S == 1, "the path-sum form has one counter slice");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // The image's bases are LDS byte addresses as they stand: the image starts
    // the dynamic region, which starts at LDS address 0 because this file has
    // no static __shared__ variable (the static size is a link-time constant;
    // were it ever not 0, the kernel would write no label and every test fail).
    if (__builtin_amdgcn_groupstaticsize() != 0) return;
    {
        const uint4* src = reinterpret_cast<const uint4*>(p.image);
        uint4* dst = reinterpret_cast<uint4*>(lds);
        for (uint32_t i = tid; i < (p.image_words >> 2); i += blockDim.x) dst[i] = src[i];
    }
    uint32_t dead = p.dead;
    // (path-sum form: the dead entry kept in a VGPR across the documents -- the
    // steps' selects would otherwise copy it from its SGPR twice per document)
    if constexpr (FORM != kFormPlain) asm volatile("" : "+v"(dead));
    __syncthreads();
    uint32_t* const cnt = lds + p.image_words + wave * (64 * S);
    // (the same counters as an LDS byte address: the dynamic region starts at 0)
    const uint32_t cnt_addr = 4u * (p.image_words + (uint32_t)wave * (64 * S));
    uint32_t* const buf0 = lds + p.image_words + kScoreWaves * (64 * S) + wave * 2 * kBufWords;
    uint32_t* const buf1 = buf0 + kBufWords;
    // (trie_lds_bytes still counts 64 B per wave behind the buffers, where the
    // group's labels were staged until they moved into a register: the
    // footprint, and with it the builder's slot budget, is unchanged)
#pragma unroll
    for (int s = 0; s < S; ++s) cnt[64 * s + lane] = 0;
    __builtin_amdgcn_wave_barrier();

    // this wave's contiguous range of documents, walked in groups of p.group
    const int64_t nwaves = (int64_t)gridDim.x * kScoreWaves;
    const int64_t wg = (int64_t)blockIdx.x * kScoreWaves + wave;
    const int64_t dbeg = (int64_t)((__int128)p.n_docs * wg / nwaves);
    const int64_t dend = (int64_t)((__int128)p.n_docs * (wg + 1) / nwaves);
    if (dbeg >= dend) return;
    const int G = p.group;

    // lane i <= G holds offsets[g0 + i] of the current group (clamped to dend)
    int64_t g0 = dbeg;
    int64_t offv = p.offsets[min(g0 + (int64_t)min(lane, G), dend)];
    group_dma(p, rdlane_i64(offv, 0) & ~(int64_t)15, buf0);
    bool par = false;
    int64_t prev_g0 = 0;
    int prev_cnt = 0;
    // The group's labels, document i's in lane i (launch_trie admits 1..63), and
    // the previous group's until its store: a byte written to LDS per document
    // and read back per group cost this kernel 1.6 % (it stands at the LDS
    // array's limit), a compare and a select per document do not.
    uint32_t labv = 0xffu, prev_labv = 0xffu;
    TailCut cut;
    cut.len = -1;

    while (g0 < dend) {
        // this group's bytes (DMA issued one group ago) have landed, and the
        // previous group's label store has drained
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // as many consecutive whole documents as the staging buffer holds from
        // s0 (at least one: the lanes that fit are a prefix)
        const int64_t s0 = rdlane_i64(offv, 0) & ~(int64_t)15;
        const int lim = (int)min((int64_t)G, dend - g0);
        const int fl = (int)fresh_lane();
        const int cntd = max(1, (int)__popcll(__ballot(fl >= 1 && fl <= lim && offv - s0 <= (int64_t)kBufBytes)));
        const int64_t g1 = g0 + cntd;
        const int64_t send = rdlane_i64(offv, cntd);
        const bool staged = send - s0 <= kBufBytes;
        uint32_t* const cur = par ? buf1 : buf0;
        // bytes and offsets of the next group (hidden behind this group's work)
        if (g1 < dend) group_dma(p, send & ~(int64_t)15, par ? buf0 : buf1);
        const int64_t n1 = min(g1 + (int64_t)G, dend);
        const int64_t offn = p.offsets[min(g1 + (int64_t)min((int)fresh_lane(), G), n1)];
        // the previous group's labels: one coalesced store (0xff = -1)
        {
            const uint32_t l = fresh_lane();
            if ((int)l < prev_cnt) p.labels[prev_g0 + l] = label_of((uint8_t)prev_labv);
        }
        __builtin_amdgcn_wave_barrier();
        // The pair form with p.doc_pairs: the documents the kernel scores are
        // labelled two at a time.  The first of a pair counts 1 and waits (pend:
        // its index in the group, -1: none), the second counts 0x10000 at the
        // same counters, and one pass labels both (pair_argmax2).  A document
        // left to score_kernel touches no counter and does not break a pair; a
        // first document still pending at the end of the group is labelled
        // alone, so the group's label store is what it was.
        int pend = -1;
        for (int i = 0; i < cntd; ++i) {
            // 32-bit geometry (a staged group: b - s0 and len lie in [0, kBufBytes])
            const uint32_t blo = rdlane((uint32_t)offv, i);
            const int32_t len = (int32_t)(rdlane((uint32_t)offv, i + 1) - blo);
            const uint32_t base = blo - (uint32_t)s0;
            if (staged && len >= p.maxg && len <= 256) {
                if constexpr (FORM == kFormPair) {
                    const int first = __builtin_amdgcn_readfirstlane(pend);  // (wave-uniform: kept scalar)
                    const uint32_t inc = first < 0 ? 1u : 0x10000u;
                    trie_doc<S, MAXD, FORM>(p, dead, cnt, cnt_addr, cur, base, len, lane, cut, inc);
                    if (!p.doc_pairs) {
                        const int lab = pair_argmax(p, cnt, lane);
                        labv = lane == i ? (uint32_t)lab : labv;
                    } else if (first < 0) {
                        pend = i;
                    } else {
                        const PairLabels two = pair_argmax2(p, cnt, lane);
                        labv = lane == first ? (uint32_t)two.lab[0] : labv;
                        labv = lane == i ? (uint32_t)two.lab[1] : labv;
                        pend = -1;
                    }
                } else {
                    const int lab = trie_doc<S, MAXD, FORM>(p, dead, cnt, cnt_addr, cur, base, len, lane, cut, 1u);
                    labv = lane == i ? (uint32_t)lab : labv;
                }
            } else {
                // left to the indirect launch of score_kernel
                if (lane == 0) p.left[atomicAdd(p.n_left, 1ull)] = g0 + i;
                labv = lane == i ? 0xffu : labv;
            }
        }
        if constexpr (FORM == kFormPair) {
            if (pend >= 0) {
                const PairLabels two = pair_argmax2(p, cnt, lane);
                labv = lane == pend ? (uint32_t)two.lab[0] : labv;
            }
        }
        __builtin_amdgcn_wave_barrier();
        prev_g0 = g0;
        prev_cnt = cntd;
        prev_labv = labv;
        offv = offn;
        g0 = g1;
        par = !par;
    }
    if (lane < prev_cnt) p.labels[prev_g0 + lane] = label_of((uint8_t)prev_labv);
}

template <int S, int MAXD, int FORM>
hipError_t launch_k(const TrieParams& p, int grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((trie_kernel<S, MAXD, FORM>), dim3(grid), dim3(kScoreWaves * 64), lds, stream, p);
    return hipGetLastError();
}
template <int S, int FORM = kFormPlain>
hipError_t launch_s(const TrieParams& p, int max_len, int grid, size_t lds, hipStream_t stream) {
    switch (max_len) {
        case 1: return launch_k<S, 1, FORM>(p, grid, lds, stream);
        case 2: return launch_k<S, 2, FORM>(p, grid, lds, stream);
        case 3: return launch_k<S, 3, FORM>(p, grid, lds, stream);
        case 4: return launch_k<S, 4, FORM>(p, grid, lds, stream);
        default: return hipErrorInvalidValue;
    }
}

template <int S, int MAXD, int FORM>
hipError_t prepare_k(size_t lds, int* blocks) {
    const void* f = reinterpret_cast<const void*>(&trie_kernel<S, MAXD, FORM>);
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, f, kScoreWaves * 64, lds);
}
template <int S, int FORM = kFormPlain>
hipError_t prepare_s(int max_len, size_t lds, int* blocks) {
    switch (max_len) {
        case 1: return prepare_k<S, 1, FORM>(lds, blocks);
        case 2: return prepare_k<S, 2, FORM>(lds, blocks);
        case 3: return prepare_k<S, 3, FORM>(lds, blocks);
        case 4: return prepare_k<S, 4, FORM>(lds, blocks);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_trie(const TrieParams& p, int slices, int max_len, bool sum, bool pair, int grid,
                       hipStream_t stream) {
    const size_t lds = trie_lds_bytes(p.image_words, slices, kScoreWaves, kBufWords);
    // lane i <= group holds a group's offsets, lane i < group its labels
    if (p.group < 1 || p.group > 63) return hipErrorInvalidValue;
    if (pair) {
        // the counters pair_argmax reads end at word wmax * L of the wave's 64
        if (!sum || slices != 1 || p.L < 1 || p.wmax < 1 || p.wmax * (uint32_t)p.L > kTriePairMaxSlot)
            return hipErrorInvalidValue;
        return launch_s<1, kFormPair>(p, max_len, grid, lds, stream);
    }
    if (sum) return slices == 1 ? launch_s<1, kFormSum>(p, max_len, grid, lds, stream) : hipErrorInvalidValue;
    switch (slices) {
        case 1: return launch_s<1>(p, max_len, grid, lds, stream);
        case 2: return launch_s<2>(p, max_len, grid, lds, stream);
        case 3: return launch_s<3>(p, max_len, grid, lds, stream);
        case 4: return launch_s<4>(p, max_len, grid, lds, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t trie_prepare(int slices, int max_len, bool sum, bool pair, size_t lds_bytes, int* blocks_per_cu) {
    if (pair)
        return sum && slices == 1 ? prepare_s<1, kFormPair>(max_len, lds_bytes, blocks_per_cu) : hipErrorInvalidValue;
    if (sum) return slices == 1 ? prepare_s<1, kFormSum>(max_len, lds_bytes, blocks_per_cu) : hipErrorInvalidValue;
    switch (slices) {
        case 1: return prepare_s<1>(max_len, lds_bytes, blocks_per_cu);
        case 2: return prepare_s<2>(max_len, lds_bytes, blocks_per_cu);
        case 3: return prepare_s<3>(max_len, lds_bytes, blocks_per_cu);
        case 4: return prepare_s<4>(max_len, lds_bytes, blocks_per_cu);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ldgpu
