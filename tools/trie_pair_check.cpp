// trie_pair_check -- host check of the LDS trie's pair form (trie_build_pair,
// csrc/ldgpu_trie.h), built with -fsanitize=address,undefined and run by
// tests/test_trie_pair_host.py.
//
//   trie_pair_check [keys.bin]
//
// The random path-uniform key sets are trie_sum_check's (the same generator,
// seed and order) under its gram lists [1, 2, 3, 4], [2, 4] and [1, 2, 3, 3].
// A set whose largest W times its language count is above 63 must be refused
// as it stands; its languages are then folded (l mod L', L' = 63 / Wmax, which
// keeps every path's one language) and the folded set must build.  For every
// built set:
//   - along the path of every key, each node's payload is 4 * (1 + l + L (W - 1))
//     with (l, W) computed from the dictionary, 0 where nothing is counted, and
//     neither the payload nor the whole entry decreases;
//   - slot by slot, base and check byte are the path-sum image's, and the
//     payload is the path-sum payload's (l, W) re-encoded -- empty slots and the
//     dead entry included, which are identical in both images.
// Then the bounds from both sides (L x Wmax = 21 x 3, 63 x 1, 15 x 4 build with
// the last slot used; 16 x 4, 32 x 2, 22 x 3 are refused and have the path-sum
// form), a mixed-language path, and a language at or above L.
// keys.bin (records of key u32 LE, length u8, language u8; the benchmark's
// table, 20 languages) with every multiplicity 1 must have the form.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../spark-languagedetector_amd/csrc/ldgpu_trie.h"

using namespace ldgpu;

static int g_fail = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            fprintf(stderr, "FAIL %s: ", #c); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
            if (++g_fail > 20) exit(1);       \
        }                                     \
    } while (0)

typedef uint32_t Mult[kTrieMaxLen + 1];

static TrieKey mk(const std::string& s, int lang) {
    TrieKey k{0, (uint8_t)s.size(), (uint8_t)lang};
    for (size_t i = 0; i < s.size(); ++i) k.bytes |= (uint32_t)(uint8_t)s[i] << (8 * i);
    return k;
}
static std::string str(const TrieKey& k) {
    std::string s;
    for (int d = 0; d < k.len; ++d) s.push_back((char)(uint8_t)(k.bytes >> (8 * d)));
    return s;
}
static void mult_of(const std::vector<int>& grams, Mult& m) {
    for (uint32_t& x : m) x = 0;
    for (int g : grams)
        if (g >= 1 && g <= kTrieMaxLen) ++m[g];
}

struct Stats {
    uint32_t wmax = 0, top_slot = 0;
    std::set<uint32_t> payloads;  // distinct, non-zero
};

// the pair image of `keys` (path-uniform, languages below n_langs, within the
// bound) against the dictionary and against the path-sum image
static bool check_set(const char* name, const std::vector<TrieKey>& keys, const Mult& mult, uint32_t n_langs,
                      uint32_t max_slots = kTrieMaxSlots, Stats* stats = nullptr) {
    TrieImage s, t;
    if (!trie_build_sum(keys, mult, max_slots, s)) {
        CHECK(!trie_build_pair(keys, mult, n_langs, max_slots, t), "%s: the pair form builds where the sum form does not",
              name);
        printf("%s: no path-sum image in %u slots\n", name, max_slots);
        return false;
    }
    const bool ok = trie_build_pair(keys, mult, n_langs, max_slots, t);
    CHECK(ok, "%s: build failed (L = %u, Wmax = %u)", name, n_langs, s.wmax);
    if (!ok) return false;
    CHECK(t.sum && t.pair && !s.pair, "%s: the forms' marks", name);
    CHECK(t.wmax == s.wmax && t.wmax * n_langs <= kTriePairMaxSlot, "%s: wmax %u, the sum form's %u", name, t.wmax, s.wmax);
    CHECK(t.nodes == s.nodes && t.rows == s.rows && t.max_len == s.max_len, "%s: nodes, rows or max_len differ", name);
    CHECK(t.dead == s.dead, "%s: dead entry %08x, the sum form's %08x", name, t.dead, s.dead);
    CHECK(t.words.size() == s.words.size(), "%s: %zu words, the sum form %zu", name, t.words.size(), s.words.size());
    if (t.words.size() != s.words.size()) return false;
    // slot by slot: the packing is the sum form's, the payload its (l, W) re-encoded
    size_t paid = 0;
    for (size_t i = 0; i < t.words.size(); ++i) {
        const uint32_t a = s.words[i], b = t.words[i];
        CHECK((a & 0xffffffu) == (b & 0xffffffu), "%s: slot %zu base / check %06x, the sum form's %06x", name, i,
              b & 0xffffffu, a & 0xffffffu);
        const uint32_t ps = trie_sum_payload(a), pp = trie_sum_payload(b);
        const uint32_t want = ps ? trie_pair_payload_of(trie_sum_counter(ps) - 1u, trie_sum_weight(ps), n_langs) : 0u;
        CHECK(pp == want, "%s: slot %zu payload %u, want %u (sum payload %u)", name, i, pp, want, ps);
        if (!ps) CHECK(a == b, "%s: slot %zu carries nothing and differs", name, i);
        paid += pp != 0;
    }
    // along every key's path: the payload from the dictionary, never decreasing
    std::map<std::string, int> dict;
    for (const TrieKey& k : keys)
        if (k.lang != kTrieNoLang && mult[k.len]) dict[str(k)] = k.lang;
    size_t walked = 0;
    for (const auto& kv : dict) {
        uint32_t e = 0, w = 0, lang = kTrieNoLang;
        for (size_t d = 1; d <= kv.first.size(); ++d) {
            const uint32_t up = e;
            e = d == 1 ? trie_root(t, (uint8_t)kv.first[0]) : trie_sum_step(t, e, (uint8_t)kv.first[d - 1]);
            CHECK(e != t.dead && trie_sum_check(e) == (uint8_t)kv.first[d - 1], "%s: a key's node is missing", name);
            const auto it = dict.find(kv.first.substr(0, d));
            if (it != dict.end()) {
                CHECK(lang == kTrieNoLang || lang == (uint32_t)it->second, "%s: the key set is not path-uniform", name);
                lang = (uint32_t)it->second;
                w += mult[d];
            }
            const uint32_t pay = trie_sum_payload(e);
            const uint32_t want = w ? 4u * (1u + lang + n_langs * (w - 1u)) : 0u;
            CHECK(pay == want, "%s: payload %u at depth %zu, want %u (l = %u, W = %u)", name, pay, d, want, lang, w);
            if (pay) {
                CHECK(pay % 4 == 0 && trie_pair_slot(pay) >= 1 && trie_pair_slot(pay) <= t.wmax * n_langs,
                      "%s: payload %u is no counter offset", name, pay);
                CHECK(trie_pair_lang(pay, n_langs) == lang && trie_pair_weight(pay, n_langs) == w, "%s: payload %u decodes to (%u, %u)",
                      name, pay, trie_pair_lang(pay, n_langs), trie_pair_weight(pay, n_langs));
                if (stats) {
                    stats->payloads.insert(pay);
                    stats->top_slot = std::max(stats->top_slot, trie_pair_slot(pay));
                }
            }
            if (d > 1) {
                const uint32_t pu = trie_sum_payload(up);
                CHECK(pay >= pu, "%s: payload %u after %u", name, pay, pu);
                CHECK(pay == pu || e > up, "%s: entries do not order by payload", name);
            }
            ++walked;
        }
    }
    if (stats) stats->wmax = t.wmax;
    printf("%s: %zu keys, L = %u, Wmax = %u, %zu slots, %zu with a payload, %zu path nodes checked\n", name, dict.size(),
           n_langs, t.wmax, t.words.size(), paid, walked);
    return true;
}

// trie_sum_check's generator: random distinct keys, each with the language of its shortest prefix that is a key
static std::vector<TrieKey> uniform_keys(std::mt19937& rng, size_t n, const std::vector<uint8_t>& alpha, int langs) {
    std::map<std::string, int> keys;
    size_t tries = 0;
    while (keys.size() < n && tries++ < 50 * n) {
        const int len = 1 + (int)(rng() % 4);
        std::string s;
        for (int d = 0; d < len; ++d) s.push_back((char)alpha[rng() % alpha.size()]);
        keys.emplace(s, (int)(rng() % (unsigned)langs));
    }
    std::vector<TrieKey> out;
    for (auto& kv : keys) {
        for (size_t d = 1; d < kv.first.size(); ++d) {
            const auto it = keys.find(kv.first.substr(0, d));
            if (it != keys.end()) {
                kv.second = it->second;
                break;
            }
        }
        out.push_back(mk(kv.first, kv.second));
    }
    return out;
}

// a random set as it stands where it is within the bound; otherwise refused as it stands, and checked folded
static void random_set(const char* name, std::vector<TrieKey> keys, const Mult& mult, uint32_t langs) {
    TrieImage s, t;
    if (!trie_build_sum(keys, mult, kTrieMaxSlots, s)) {
        CHECK(!trie_build_pair(keys, mult, langs, kTrieMaxSlots, t), "%s: pair builds where sum does not", name);
        printf("%s: too large for %u slots\n", name, kTrieMaxSlots);
        return;
    }
    uint32_t L = langs;
    if (s.wmax * langs > kTriePairMaxSlot) {
        CHECK(!trie_build_pair(keys, mult, langs, kTrieMaxSlots, t), "%s: L = %u with Wmax = %u builds", name, langs, s.wmax);
        L = kTriePairMaxSlot / s.wmax;
        for (TrieKey& k : keys) k.lang = (uint8_t)(k.lang % L);
    }
    check_set(name, keys, mult, L);
}

int main(int argc, char** argv) {
    std::mt19937 rng(20261021);
    std::vector<uint8_t> a12, az, all;
    for (int c = 'a'; c < 'a' + 12; ++c) a12.push_back((uint8_t)c);
    for (int c = 'a'; c <= 'z'; ++c) az.push_back((uint8_t)c);
    for (int c = 0; c < 256; ++c) all.push_back((uint8_t)c);
    const std::vector<std::vector<int>> lists = {{1, 2, 3, 4}, {2, 4}, {1, 2, 3, 3}};
    const size_t sizes[] = {100, 1000, 10000};
    for (const auto& grams : lists) {
        Mult mult;
        mult_of(grams, mult);
        for (size_t n : sizes) {
            random_set("12 letters", uniform_keys(rng, n, a12, 20), mult, 20);
            random_set("a-z", uniform_keys(rng, n, az, 63), mult, 63);
            random_set("all bytes", uniform_keys(rng, n, all, 40), mult, 40);
        }
    }
    Mult m1234, m1, m24;
    mult_of({1, 2, 3, 4}, m1234);
    mult_of({1}, m1);
    mult_of({2, 4}, m24);
    // a chain of `depth` keys "r", "rr", ... of one language: W = depth under [1, 2, 3, 4]
    const auto chain = [](int lang, int depth) {
        std::vector<TrieKey> k;
        for (int d = 1; d <= depth; ++d) k.push_back(mk(std::string((size_t)d, 'r'), lang));
        return k;
    };
    {  // the bound from below: the last slot, 63 or 60, is used
        const struct { uint32_t L; int w; uint32_t top; } builds[] = {{21, 3, 63}, {63, 1, 63}, {15, 4, 60}};
        for (const auto& b : builds) {
            Stats st;
            char name[64];
            snprintf(name, sizeof name, "bound L = %u, Wmax = %d", b.L, b.w);
            const bool ok = check_set(name, chain((int)b.L - 1, b.w), m1234, b.L, kTrieMaxSlots, &st);
            CHECK(ok && st.wmax == (uint32_t)b.w && st.top_slot == b.top && st.payloads.count(4 * b.top),
                  "%s: Wmax %u, top slot %u", name, st.wmax, st.top_slot);
        }
        // (63 languages under [1] alone: every language's one key)
        std::vector<TrieKey> k63;
        for (int l = 0; l < 63; ++l) k63.push_back(mk(std::string(1, (char)('A' + l)), l));
        Stats st;
        CHECK(check_set("63 one-byte keys", k63, m1, 63, kTrieMaxSlots, &st) && st.payloads.size() == 63 && st.top_slot == 63,
              "63 one-byte keys");
    }
    {  // the bound from above, and what else is refused; each has the path-sum form
        const struct { uint32_t L; int w; } refused[] = {{16, 4}, {32, 2}, {22, 3}};
        for (const auto& r : refused) {
            TrieImage t;
            CHECK(!trie_build_pair(chain((int)r.L - 1, r.w), m1234, r.L, kTrieMaxSlots, t), "L = %u, Wmax = %d builds", r.L, r.w);
            CHECK(!trie_build_pair(chain(0, r.w), m1234, r.L, kTrieMaxSlots, t), "L = %u, Wmax = %d (language 0) builds", r.L,
                  r.w);
            CHECK(trie_build_sum(chain((int)r.L - 1, r.w), m1234, kTrieMaxSlots, t) && t.sum && !t.pair &&
                      t.wmax == (uint32_t)r.w,
                  "L = %u, Wmax = %d has no path-sum form", r.L, r.w);
            printf("refused: L = %u, Wmax = %d (%u slots)\n", r.L, r.w, r.L * (uint32_t)r.w);
        }
        TrieImage t;
        CHECK(!trie_build_pair({mk("ab", 1), mk("abc", 2)}, m1234, 8, kTrieMaxSlots, t), "a mixed-language path builds");
        CHECK(!trie_build_pair({mk("a", 1), mk("abcd", 2)}, m1234, 8, kTrieMaxSlots, t),
              "a mixed-language path (a gap between the keys) builds");
        CHECK(!trie_build_pair({mk("a", 8)}, m1234, 8, kTrieMaxSlots, t), "language 8 of 8 builds");
        CHECK(!trie_build_pair({mk("a", 0)}, m1234, 0, kTrieMaxSlots, t), "no language at all builds");
        CHECK(!trie_build_pair({TrieKey{0, 5, 0}}, m1234, 8, kTrieMaxSlots, t), "a 5-byte key builds");
        // an uncounted length between two keys adds nothing: Wmax = 2 under [2, 4], so L = 31 builds and 32 does not
        Stats s24;
        CHECK(check_set("chain, [2, 4], L = 31", chain(30, 4), m24, 31, kTrieMaxSlots, &s24) && s24.wmax == 2 &&
                  s24.payloads == (std::set<uint32_t>{4 * 31, 4 * 62}),
              "the chain's payloads under [2, 4]");
        CHECK(!trie_build_pair(chain(30, 4), m24, 32, kTrieMaxSlots, t), "[2, 4] with L = 32 builds");
        check_set("uncounted key", {mk("ab", (int)kTrieNoLang), mk("abc", 4)}, m1234, 8);
    }
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        std::vector<TrieKey> keys;
        uint8_t r[6];
        while (fread(r, 1, 6, f) == 6) {
            uint32_t b;
            memcpy(&b, r, 4);
            keys.push_back(TrieKey{b, r[4], r[5]});
        }
        fclose(f);
        // two workgroups of twelve waves per CU: 81,920 B each, one slice, 260-word staging buffers
        constexpr uint32_t kBudget = 81920, kPerWave = trie_lds_bytes(0, 1, 12, 260);
        Stats st;
        const bool ok = check_set("table", keys, m1234, 20, (kBudget - kPerWave) / 4, &st);
        CHECK(ok, "the table has not the pair form");
        if (ok)
            printf("table: %zu keys, L = 20, largest W %u, %zu distinct payloads, top slot %u\n", keys.size(), st.wmax,
                   st.payloads.size(), st.top_slot);
    }
    if (g_fail) return 1;
    printf("trie_pair_check ok\n");
    return 0;
}
