// trie_sum_check -- host check of the LDS trie's path-sum form (trie_build_sum,
// csrc/ldgpu_trie.h), built with -fsanitize=address,undefined and run by
// tests/test_trie_sum_host.py.
//
//   trie_sum_check [keys.bin]
//
// Builds the path-sum image of random path-uniform key sets (every key has the
// language of its shortest prefix that is a key) under the gram lists
// [1, 2, 3, 4], [2, 4] and [1, 2, 3, 3], and checks each exhaustively: for
// every trie node (the root included) and each of its 256 byte extensions the
// walk equals dictionary membership, the payload equals (language, W) computed
// from the dictionary, payloads grow strictly along a path wherever W does,
// and neither the dead state nor an empty slot matches or carries a payload.
// Then the refusals (two languages on a path, language 63, W = 6) and the
// limits that must build (W = 4; language 62 with W = 4: payload 255).
// keys.bin (records of key u32 LE, length u8, language u8; the benchmark's
// table) with every multiplicity 1 must have the form; its figures are printed.
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
    uint32_t max_w = 0;
    std::set<uint32_t> payloads;  // distinct, non-zero
};

// exhaustive check of the path-sum image of `keys` under `mult`; the keys must have the form
static bool check_set(const char* name, const std::vector<TrieKey>& keys, const Mult& mult,
                      uint32_t max_slots = kTrieMaxSlots, Stats* stats = nullptr, TrieImage* image = nullptr) {
    std::map<std::string, int> dict;  // counted keys
    std::set<std::string> prefixes{std::string()};
    for (const TrieKey& k : keys) {
        if (k.lang == kTrieNoLang || !mult[k.len]) continue;
        const std::string s = str(k);
        for (size_t d = 1; d <= s.size(); ++d) prefixes.insert(s.substr(0, d));
        dict[s] = k.lang;
    }
    // (language, W) of a string: over its prefixes that are counted keys
    const auto expect = [&](const std::string& s) {
        uint32_t w = 0, lang = kTrieNoLang;
        for (size_t d = 1; d <= s.size(); ++d) {
            const auto it = dict.find(s.substr(0, d));
            if (it == dict.end()) continue;
            CHECK(lang == kTrieNoLang || lang == (uint32_t)it->second, "%s: the key set is not path-uniform", name);
            lang = (uint32_t)it->second;
            w += mult[d];
        }
        return w ? trie_sum_payload_of(lang, w) : 0u;
    };
    TrieImage t;
    const bool ok = trie_build_sum(keys, mult, max_slots, t);
    if (prefixes.size() - 1 > max_slots) {
        // more nodes than the image has slots: no form packs
        CHECK(!ok, "%s: %zu nodes built in %u slots?", name, prefixes.size() - 1, max_slots);
        printf("%s: %zu keys, %zu nodes: too large for %u slots\n", name, dict.size(), prefixes.size() - 1, max_slots);
        return false;
    }
    CHECK(ok,"%s: build failed (%zu keys, %zu nodes)", name, keys.size(), prefixes.size() - 1);
    if (!ok) return false;
    CHECK(t.sum, "%s: not marked as the path-sum form", name);
    CHECK(t.nodes + 1 == prefixes.size(), "%s: %u nodes, %zu prefixes", name, t.nodes, prefixes.size());
    CHECK(t.words.size() % 4 == 0 && t.words.size() <= max_slots, "%s: %zu words", name, t.words.size());
    // the packing is the other form's: the same slot count, bases and checks
    {
        std::vector<TrieKey> counted;
        for (const TrieKey& k : keys)
            if (k.lang != kTrieNoLang && mult[k.len]) counted.push_back(k);
        TrieImage o;
        CHECK(trie_build(counted, max_slots, o), "%s: the other form does not build", name);
        CHECK(o.words.size() == t.words.size() && !o.sum, "%s: %zu words, the other form %zu", name, t.words.size(),
              o.words.size());
        bool same = o.words.size() == t.words.size();
        for (size_t s = 0; s < t.words.size() && same; ++s)
            same = trie_base_slot(o.words[s]) == trie_sum_base_slot(t.words[s]) &&
                   trie_check(o.words[s]) == trie_sum_check(t.words[s]);
        CHECK(same, "%s: the packing differs from the other form's", name);
    }
    CHECK(trie_sum_payload(t.dead) == 0, "%s: the dead entry has a payload", name);
    const uint32_t dead_base = trie_sum_base_slot(t.dead);
    CHECK(dead_base + 256 <= t.words.size(), "%s: dead base %u past the image", name, dead_base);
    for (int c = 0; c < 256; ++c) CHECK(trie_sum_step(t, t.dead, (uint8_t)c) == t.dead, "%s: dead matches %d", name, c);
    std::set<uint32_t> bases{0u, dead_base};
    std::vector<uint8_t> occupied(t.words.size(), 0);
    for (const std::string& pre : prefixes) {
        uint32_t e = 0, up = 0;
        for (size_t d = 0; d < pre.size(); ++d) {
            up = e;
            e = d == 0 ? trie_root(t, (uint8_t)pre[d]) : trie_sum_step(t, e, (uint8_t)pre[d]);
        }
        const uint32_t pay = pre.empty() ? 0u : trie_sum_payload(e);
        if (!pre.empty()) {
            CHECK(pay == expect(pre), "%s: payload %u of a node, want %u", name, pay, expect(pre));
            CHECK(trie_sum_base_slot(e) + 256 <= t.words.size(), "%s: a base past the image", name);
            if (pre.size() > 1) {
                // strictly growing wherever W does, never falling; whole entries order the same way
                const uint32_t pu = trie_sum_payload(up);
                const uint32_t wu = pu ? trie_sum_weight(pu) : 0u, w = pay ? trie_sum_weight(pay) : 0u;
                CHECK(w >= wu && pay >= pu && (w == wu ? pay == pu : pay > pu), "%s: payload %u after %u", name, pay, pu);
                CHECK(pay == pu || e > up, "%s: entries do not order by payload", name);
            }
            if (pay) {
                CHECK(trie_sum_counter(pay) >= 1 && trie_sum_counter(pay) <= kTrieSumMaxLangs, "%s: counter", name);
                CHECK(trie_sum_weight(pay) <= kTrieSumMaxW, "%s: weight", name);
                if (stats) {
                    stats->max_w = std::max(stats->max_w, trie_sum_weight(pay));
                    stats->payloads.insert(pay);
                }
            }
        }
        if (pre.size() == (size_t)kTrieMaxLen) {
            CHECK(trie_sum_base_slot(e) == dead_base, "%s: a node of the last depth has a row", name);
            continue;
        }
        bool kids = false;
        for (int c = 0; c < 256; ++c) {
            const std::string s = pre + (char)c;
            const uint32_t n = pre.empty() ? trie_root(t, (uint8_t)c) : trie_sum_step(t, e, (uint8_t)c);
            if (prefixes.count(s)) {
                kids = true;
                CHECK(trie_sum_check(n) == (uint32_t)c, "%s: check byte of a node", name);
                CHECK(trie_sum_payload(n) == expect(s), "%s: payload %u of an extension, want %u", name,
                      trie_sum_payload(n), expect(s));
                occupied[(pre.empty() ? 0u : trie_sum_base_slot(e)) + (uint32_t)c] = 1;
            } else {
                // no node: the walk is dead from here on and carries nothing
                CHECK(trie_sum_base_slot(n) == dead_base && trie_sum_payload(n) == 0, "%s: a missing node is not dead",
                      name);
                if (!pre.empty()) CHECK(n == t.dead, "%s: a miss is not the dead entry", name);
            }
        }
        if (kids && !pre.empty()) CHECK(bases.insert(trie_sum_base_slot(e)).second, "%s: a base used twice", name);
        if (!kids && !pre.empty()) CHECK(trie_sum_base_slot(e) == dead_base, "%s: a leaf has a row", name);
    }
    // empty slots: no payload, the dead base, and slot - check is no used base
    for (uint32_t s = 0; s < t.words.size(); ++s) {
        if (occupied[s]) continue;
        const uint32_t c = trie_sum_check(t.words[s]);
        CHECK(c > s ||!bases.count(s - c), "%s: empty slot %u matches base %u", name, s, s - c);
        CHECK(trie_sum_payload(t.words[s]) == 0 && trie_sum_base_slot(t.words[s]) == dead_base,
              "%s: empty slot %u is not dead", name, s);
    }
    printf("%s: %zu keys, %zu nodes in %zu slots\n", name, dict.size(), prefixes.size() - 1, t.words.size());
    if (image) *image = t;
    return true;
}

// random distinct keys, each with the language of its shortest prefix that is a key
static std::vector<TrieKey> uniform_keys(std::mt19937& rng, size_t n, const std::vector<uint8_t>& alpha, int langs) {
    std::map<std::string, int> keys;  // (in string order: a prefix comes before its extensions)
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
                kv.second = it->second;  // (already that of ITS shortest prefix)
                break;
            }
        }
        out.push_back(mk(kv.first, kv.second));
    }
    return out;
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
            check_set("12 letters", uniform_keys(rng, n, a12, 20), mult);
            check_set("a-z", uniform_keys(rng, n, az, 63), mult);
            check_set("all bytes", uniform_keys(rng, n, all, 40), mult);
        }
    }
    Mult m1234, m123444;
    mult_of({1, 2, 3, 4}, m1234);
    mult_of({1, 2, 3, 4, 4, 4}, m123444);
    const auto chain = [](int lang) {
        return std::vector<TrieKey>{mk("r", lang), mk("rr", lang), mk("rrr", lang), mk("rrrr", lang)};
    };
    {  // refusals: not this form
        TrieImage t;
        CHECK(!trie_build_sum({mk("ab", 1), mk("abc", 2)}, m1234, kTrieMaxSlots, t), "a mixed-language path builds");
        CHECK(!trie_build_sum({mk("a", 1), mk("abcd", 2)}, m1234, kTrieMaxSlots, t),
              "a mixed-language path (a gap between the keys) builds");
        CHECK(!trie_build_sum({mk("a", 63)}, m1234, kTrieMaxSlots, t), "language 63 builds");
        CHECK(!trie_build_sum(chain(1), m123444, kTrieMaxSlots, t), "W = 6 builds");
        CHECK(!trie_build_sum({TrieKey{0, 5, 0}}, m1234, kTrieMaxSlots, t), "a 5-byte key builds");
        // ... and each of them has the other form
        CHECK(trie_build({mk("ab", 1), mk("abc", 2)}, kTrieMaxSlots, t) && !t.sum, "the mixed path has no form at all");
        CHECK(trie_build({mk("a", 63)}, kTrieMaxSlots, t) && !t.sum, "language 63 has no form at all");
    }
    {  // the limits that build
        Stats st;
        check_set("chain, W = 4", chain(1), m1234, kTrieMaxSlots, &st);
        CHECK(st.max_w == 4 && st.payloads == (std::set<uint32_t>{2, 66, 130, 194}), "the chain's payloads");
        Stats s62;
        TrieImage t;
        if (check_set("language 62, W = 4", chain(62), m1234, kTrieMaxSlots, &s62, &t)) {
            uint32_t e = trie_root(t, 'r');
            for (int d = 1; d < 4; ++d) e = trie_sum_step(t, e, 'r');
            CHECK(trie_sum_payload(e) == 255 && trie_sum_counter(255) == 63 && trie_sum_weight(255) == 4,
                  "payload %u of rrrr", trie_sum_payload(e));
        }
        // an uncounted length between two keys adds nothing; its key is no node of its own
        Mult m24;
        mult_of({2, 4}, m24);
        Stats s24;
        check_set("chain, [2, 4]", chain(5), m24, kTrieMaxSlots, &s24);
        CHECK(s24.max_w == 2 && s24.payloads == (std::set<uint32_t>{6, 70}), "the chain's payloads under [2, 4]");
        check_set("uncounted key", {mk("ab", (int)kTrieNoLang), mk("abc", 4)}, m1234);
        check_set("one key", {mk("q", 0)}, m1234);
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
        TrieImage o, t;
        Stats st;
        CHECK(trie_build(keys, (kBudget - kPerWave) / 4, o), "the table does not fit %u B", kBudget - kPerWave);
        const bool ok = check_set("table", keys, m1234, (kBudget - kPerWave) / 4, &st, &t);
        CHECK(ok, "the table has not the path-sum form");
        if (ok) {
            CHECK(t.words.size() == o.words.size(), "%zu words, the other form %zu", t.words.size(), o.words.size());
            printf("table: %zu keys, %u nodes, image %zu words (the other form %zu), largest W %u, %zu distinct payloads\n",
                   keys.size(), t.nodes, t.words.size(), o.words.size(), st.max_w, st.payloads.size());
        }
    }
    if (g_fail) return 1;
    printf("trie_sum_check ok\n");
    return 0;
}
