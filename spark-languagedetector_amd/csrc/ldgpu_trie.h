// ldgpu_trie.h -- the exact LDS trie of a small count-mode table (host only, no
// HIP dependency: the model build includes it, and so does tools/trie_check.cpp).
//
// A table whose keys all have at most kTrieMaxLen bytes and name one language
// each is laid out as a byte trie in one double array of 32-bit entries:
//
//   entry = check byte | language << 8 | child base << 16
//
//   language   the language of the counted key that ends at this node, or
//              kTrieNoLang: none does (a pure prefix, or a key whose length the
//              model's gramLengths do not list)
//   child base BYTE offset of the node's row in the image (slot index * 4), so a
//              step is one add: the child for byte c sits at base + 4 c
//   check      the byte that leads to this node from its parent
//
// Every node with children has a DISTINCT base, so `slot - check = base` names
// the parent exactly: a probe from another row lands on an entry whose check
// differs from the probed byte.  The root's row is the image's first 256 slots,
// exclusive and read unchecked (depth 1 is a direct table).  A node without
// children, and every probe that misses, continues at the DEAD base: a base no
// row uses, so whatever slot a dead walk reads mismatches for ever.  An empty
// slot s carries a check c for which s - c is no used base (the dead base
// counts as used), language kTrieNoLang and the dead base.
//
// A walk reads slots up to base + 255 for any text byte, so every base leaves
// 256 slots to the end of the image.
//
// The PATH-SUM form (trie_build_sum) keeps the packing -- rows, bases, the dead
// base and the empty slots' check bytes are those of the form above -- and
// changes what an entry says:
//
//   entry = child base | check byte << 16 | payload << 24
//
//   payload    0: no counted key on the path from the root to this node (the
//              node included).  Otherwise 1 + language + 64 (W - 1): the one
//              language of the path's counted keys, and W = the sum of
//              mult[length] over them.  W grows along a path, so the payload
//              does, and the deepest node a walk reaches says all the walk
//              counts: `payload & 63` is the counter index (language + 1),
//              `(payload >> 6) + 1` the increment.  Whole entries compare by
//              payload first.
//
// A table has this form when every root path names at most one language, every
// language is below kTrieSumMaxLangs and every W is at most kTrieSumMaxW.
//
// The PAIR form (trie_build_pair) is the path-sum form with another payload:
// every pair (language l, W) has a counter of its own, and the payload is that
// counter's BYTE offset in the wave's counter area as it stands:
//
//   payload    0: nothing counted.  Otherwise 4 * slot, slot = 1 + l + L (W - 1),
//              L the model's language count.  Along a path the language is
//              fixed and W grows, so the payload still grows and whole entries
//              still compare by it.  A walk adds 1 at its payload's offset; the
//              label's count of language l is the sum of w * counter[1 + l +
//              L (w - 1)] over w = 1..Wmax.
//
// A table has this form when it has the path-sum form and Wmax * L <= 63, Wmax
// the largest W in the image (TrieImage::wmax): the counter area stays 64 words.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ldgpu {

constexpr int kTrieMaxLen = 4;
constexpr uint32_t kTrieNoLang = 0xffu;
constexpr uint32_t kTrieMaxLangs = 254;      // languages 0..253: the counter index is the entry's byte
constexpr uint32_t kTrieMaxSlots = 16384;    // 64 KiB: a byte offset fits the entry's 16 bits
constexpr uint32_t kTrieSumMaxLangs = 63;    // path-sum form: languages 0..62 (counter index language + 1 <= 63)
constexpr uint32_t kTrieSumMaxW = 4;         // path-sum form: the largest sum of multiplicities on a path
constexpr uint32_t kTriePairMaxSlot = 63;    // pair form: counters 1..63, Wmax * L <= 63 (slot 0: nothing counted)

struct TrieKey {
    uint32_t bytes;  // the key's bytes little-endian (byte 0 first), zero above len
    uint8_t len;     // 1..kTrieMaxLen
    uint8_t lang;    // < kTrieMaxLangs; kTrieNoLang: a key that is not counted (it adds nothing)
};

struct TrieImage {
    std::vector<uint32_t> words;  // the image, a multiple of 4 words
    uint32_t dead = 0;            // the dead entry (language kTrieNoLang, the dead base)
    uint32_t nodes = 0;           // trie nodes below the root
    uint32_t rows = 0;            // nodes with children (the root included)
    int max_len = 0;              // the longest counted key
    bool sum = false;             // the path-sum form (trie_build_sum, trie_build_pair)
    bool pair = false;            // ... with the pair payload (trie_build_pair)
    uint32_t wmax = 0;            // path-sum form: the largest W in the image
};

constexpr uint32_t trie_entry(uint32_t check, uint32_t lang, uint32_t base_slot) {
    return check | lang << 8 | (base_slot * 4u) << 16;
}
constexpr uint32_t trie_check(uint32_t e) { return e & 0xffu; }
constexpr uint32_t trie_lang(uint32_t e) { return (e >> 8) & 0xffu; }
constexpr uint32_t trie_base_slot(uint32_t e) { return e >> 18; }

// the walk the kernel makes, for the host check: the entry after byte c from
// entry e (root: the direct table); a miss gives the dead entry
inline uint32_t trie_root(const TrieImage& t, uint8_t c) { return t.words[c]; }
inline uint32_t trie_step(const TrieImage& t, uint32_t e, uint8_t c) {
    const uint32_t n = t.words[trie_base_slot(e) + c];
    return trie_check(n) == c ? n : t.dead;
}

// the path-sum form's entry and its parts
constexpr uint32_t trie_sum_payload_of(uint32_t lang, uint32_t w) { return 1u + lang + 64u * (w - 1u); }
constexpr uint32_t trie_sum_entry(uint32_t check, uint32_t payload, uint32_t base_slot) {
    return base_slot * 4u | check << 16 | payload << 24;
}
constexpr uint32_t trie_sum_check(uint32_t e) { return (e >> 16) & 0xffu; }
constexpr uint32_t trie_sum_payload(uint32_t e) { return e >> 24; }
constexpr uint32_t trie_sum_base_slot(uint32_t e) { return (e & 0xffffu) >> 2; }
constexpr uint32_t trie_sum_counter(uint32_t payload) { return payload & 63u; }   // language + 1
constexpr uint32_t trie_sum_weight(uint32_t payload) { return (payload >> 6) + 1u; }
inline uint32_t trie_sum_step(const TrieImage& t, uint32_t e, uint8_t c) {
    const uint32_t n = t.words[trie_sum_base_slot(e) + c];
    return trie_sum_check(n) == c ? n : t.dead;
}

// the pair form's payload and its parts (n_langs: the model's language count)
constexpr uint32_t trie_pair_slot_of(uint32_t lang, uint32_t w, uint32_t n_langs) {
    return 1u + lang + n_langs * (w - 1u);
}
constexpr uint32_t trie_pair_payload_of(uint32_t lang, uint32_t w, uint32_t n_langs) {
    return 4u * trie_pair_slot_of(lang, w, n_langs);
}
constexpr uint32_t trie_pair_slot(uint32_t payload) { return payload >> 2; }  // payload != 0
constexpr uint32_t trie_pair_lang(uint32_t payload, uint32_t n_langs) { return (trie_pair_slot(payload) - 1u) % n_langs; }
constexpr uint32_t trie_pair_weight(uint32_t payload, uint32_t n_langs) {
    return (trie_pair_slot(payload) - 1u) / n_langs + 1u;
}

// All forms' builder.  mult == nullptr: the form of trie_build.  Otherwise the
// path-sum form with mult[1..kTrieMaxLen], the multiplicity of each key length
// (a key whose length has multiplicity 0 is not counted, as one of kTrieNoLang);
// pair_langs != 0: the pair payload for a model of pair_langs languages.
inline bool trie_build_form(const std::vector<TrieKey>& keys, uint32_t max_slots, const uint32_t* mult,
                            TrieImage& out, uint32_t pair_langs = 0) {
    struct Node {
        uint32_t parent;
        uint8_t byte, lang;
        std::vector<uint32_t> kids;  // node indices
        uint32_t base = 0;           // slot index of the row (nodes with kids)
        uint32_t payload = 0;        // path-sum form
    };
    max_slots = std::min(max_slots, kTrieMaxSlots);
    if (max_slots < 512) return false;
    std::vector<Node> nodes(1, Node{0, 0, (uint8_t)kTrieNoLang, {}, 0});
    out = TrieImage{};
    // keys in (bytes as a string) order: every row's children come out sorted
    std::vector<TrieKey> ks;
    for (const TrieKey& k : keys) {
        if (k.len < 1 || k.len > kTrieMaxLen) return false;
        if (k.lang == kTrieNoLang || (mult && !mult[k.len])) continue;
        if (k.lang >= (mult ? kTrieSumMaxLangs : kTrieMaxLangs)) return false;
        ks.push_back(k);
    }
    // (every key is a node of its own and every node takes a slot: more counted
    // keys, or more nodes, than slots cannot pack -- found before the trie is built)
    if (ks.size() > max_slots) return false;
    for (const TrieKey& k : ks) {
        if (nodes.size() > max_slots + 1) return false;
        uint32_t at = 0;
        for (int d = 0; d < k.len; ++d) {
            const uint8_t c = (uint8_t)(k.bytes >> (8 * d));
            uint32_t next = 0;
            for (uint32_t kid : nodes[at].kids)
                if (nodes[kid].byte == c) next = kid;
            if (!next) {
                next = (uint32_t)nodes.size();
                nodes.push_back(Node{at, c, (uint8_t)kTrieNoLang, {}, 0});
                nodes[at].kids.push_back(next);
            }
            at = next;
        }
        if (nodes[at].lang != kTrieNoLang && nodes[at].lang != k.lang) return false;
        nodes[at].lang = k.lang;
        out.max_len = std::max(out.max_len, (int)k.len);
    }
    out.nodes = (uint32_t)nodes.size() - 1;
    out.sum = mult != nullptr;
    out.pair = mult != nullptr && pair_langs != 0;
    if (mult) {
        // (a node's index is above its parent's: one pass in index order)
        std::vector<uint8_t> depth(nodes.size(), 0), plang(nodes.size(), (uint8_t)kTrieNoLang);
        std::vector<uint32_t> w(nodes.size(), 0);
        for (uint32_t i = 1; i < nodes.size(); ++i) {
            const uint32_t up = nodes[i].parent;
            depth[i] = (uint8_t)(depth[up] + 1);
            plang[i] = plang[up];
            w[i] = w[up];
            if (nodes[i].lang != kTrieNoLang) {
                if (plang[i] != kTrieNoLang && plang[i] != nodes[i].lang) return false;  // two languages on a path
                plang[i] = nodes[i].lang;
                w[i] += mult[depth[i]];
            }
            if (w[i] > kTrieSumMaxW) return false;
            out.wmax = std::max(out.wmax, w[i]);
            nodes[i].payload = w[i] ? trie_sum_payload_of(plang[i], w[i]) : 0u;
        }
        if (pair_langs) {
            // every language below pair_langs, and the last counter within the area
            if (out.wmax * pair_langs > kTriePairMaxSlot) return false;
            for (uint32_t i = 1; i < nodes.size(); ++i) {
                if (!w[i]) continue;
                if (plang[i] >= pair_langs) return false;
                nodes[i].payload = trie_pair_payload_of(plang[i], w[i], pair_langs);
            }
        }
    }
    const auto entry = [&](uint32_t check, uint32_t lang, uint32_t payload, uint32_t base_slot) {
        return mult ? trie_sum_entry(check, payload, base_slot) : trie_entry(check, lang, base_slot);
    };

    // first-fit row displacement, largest rows first; the root's row is slots
    // 0..255, exclusive.  A row may start below slot 256 (its base only has to
    // keep its ENTRIES out of the root's row) but not past max_slots - 256.
    std::vector<uint32_t> rows;
    for (uint32_t i = 1; i < nodes.size(); ++i)
        if (!nodes[i].kids.empty()) rows.push_back(i);
    std::stable_sort(rows.begin(), rows.end(),
                     [&](uint32_t a, uint32_t b) { return nodes[a].kids.size() > nodes[b].kids.size(); });
    out.rows = (uint32_t)rows.size() + 1;
    std::vector<uint8_t> taken(max_slots, 0), used_base(max_slots, 0);
    std::vector<int32_t> owner(max_slots, -1);  // the node of an occupied slot
    for (uint32_t s = 0; s < 256; ++s) taken[s] = 1;
    for (uint32_t kid : nodes[0].kids) owner[nodes[kid].byte] = (int32_t)kid;
    used_base[0] = 1;
    const uint32_t last_base = max_slots - 256;
    uint32_t first_free = 256;
    for (uint32_t r : rows) {
        Node& n = nodes[r];
        uint8_t lo = 255;
        for (uint32_t kid : n.kids) lo = std::min(lo, nodes[kid].byte);
        while (first_free < max_slots && taken[first_free]) ++first_free;
        bool placed = false;
        // the row's lowest child on each free slot in turn
        for (uint32_t s = first_free; s < max_slots && !placed; ++s) {
            if (taken[s] || s < lo) continue;
            const uint32_t base = s - lo;
            if (base < 1 || base > last_base) continue;
            if (used_base[base]) continue;
            bool fits = true;
            for (uint32_t kid : n.kids) fits &= !taken[base + nodes[kid].byte];
            if (!fits) continue;
            n.base = base;
            used_base[base] = 1;
            for (uint32_t kid : n.kids) {
                taken[base + nodes[kid].byte] = 1;
                owner[base + nodes[kid].byte] = (int32_t)kid;
            }
            placed = true;
        }
        if (!placed) return false;
    }
    // the dead base: the lowest one no row uses
    uint32_t dead_base = 1;
    while (dead_base <= last_base && used_base[dead_base]) ++dead_base;
    if (dead_base > last_base) return false;
    used_base[dead_base] = 1;
    uint32_t top = 0;
    for (uint32_t b = 0; b <= last_base; ++b)
        if (used_base[b]) top = b;
    const uint32_t n_slots = (top + 256 + 3) & ~3u;
    if (n_slots > max_slots) return false;
    out.dead = entry(0, kTrieNoLang, 0, dead_base);
    out.words.assign(n_slots, 0u);
    for (uint32_t s = 0; s < n_slots; ++s) {
        if (owner[s] >= 0) {
            const Node& n = nodes[(size_t)owner[s]];
            out.words[s] = entry(n.byte, n.lang, n.payload, n.kids.empty() ? dead_base : n.base);
            continue;
        }
        // an empty slot: a check byte that names no row
        int c = -1;
        for (int t = 0; t < 256 && c < 0; ++t)
            if ((uint32_t)t > s || !used_base[s - (uint32_t)t]) c = t;
        if (c < 0) return false;
        out.words[s] = entry((uint32_t)c, kTrieNoLang, 0, dead_base);
    }
    return true;
}

// Builds the image of `keys` (distinct) within max_slots slots.  False: a key
// out of the rule, two languages for one key, or no packing within max_slots.
inline bool trie_build(const std::vector<TrieKey>& keys, uint32_t max_slots, TrieImage& out) {
    return trie_build_form(keys, max_slots, nullptr, out);
}

// The path-sum form of the same keys: mult[1..kTrieMaxLen] (mult[0] unused).
// False also for a table that has not this form: two languages on one root
// path, a language of kTrieSumMaxLangs or above, a W above kTrieSumMaxW.
inline bool trie_build_sum(const std::vector<TrieKey>& keys, const uint32_t (&mult)[kTrieMaxLen + 1],
                           uint32_t max_slots, TrieImage& out) {
    return trie_build_form(keys, max_slots, mult, out);
}

// The pair form of the same keys for a model of n_langs languages.  False also
// for a table that has the path-sum form but not this one: Wmax * n_langs above
// kTriePairMaxSlot, or a counted language of n_langs or above.
inline bool trie_build_pair(const std::vector<TrieKey>& keys, const uint32_t (&mult)[kTrieMaxLen + 1],
                            uint32_t n_langs, uint32_t max_slots, TrieImage& out) {
    return n_langs >= 1 && trie_build_form(keys, max_slots, mult, out, n_langs);
}

// bytes of LDS the trie kernel needs per workgroup of `waves` waves: the image,
// then per wave the language counters, the double-buffered staging and 64
// spare bytes.  The kernel staged a group's labels there until they moved into
// a register; nothing reads or writes them now.  They stay in the sum so that
// the footprint and the builder's slot budget (and with them every packed
// image) are the parent's; giving them to the builder is a step of its own.
constexpr uint32_t trie_lds_bytes(uint32_t image_words, int slices, int waves, uint32_t buf_words) {
    return image_words * 4u + (uint32_t)waves * (64u * (uint32_t)slices * 4u + 2u * buf_words * 4u + 64u);
}

}  // namespace ldgpu
