// trie_check -- host check of the LDS trie builder (csrc/ldgpu_trie.h), built
// with -fsanitize=address,undefined and run by tests/test_trie_host.py.
//
//   trie_check [keys.bin]
//
// Builds tries for random and hand-made key sets and checks each exhaustively:
// for every trie node (the root included) and each of its 256 byte extensions
// the walk equals dictionary membership and language, and neither the dead
// state nor an empty slot ever matches.  keys.bin (records of key u32 LE,
// length u8, language u8): the table must be eligible for two workgroups of
// twelve waves per CU; the packed size is printed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../spark-languagedetector_amd/csrc/ldgpu_trie.h"

using namespace ldgpu;

static int g_fail = 0;
#define CHECK(c, ...)                       \
    do {                                    \
        if (!(c)) {                         \
            fprintf(stderr, "FAIL %s: ", #c); \
            fprintf(stderr, __VA_ARGS__);   \
            fprintf(stderr, "\n");          \
            if (++g_fail > 20) exit(1);     \
        }                                   \
    } while (0)

static TrieKey mk(const std::string& s, int lang) {
    TrieKey k{0, (uint8_t)s.size(), (uint8_t)lang};
    for (size_t i = 0; i < s.size(); ++i) k.bytes |= (uint32_t)(uint8_t)s[i] << (8 * i);
    return k;
}

// a byte string of at most 4 bytes as one word: its bytes little-endian, its length above them
static uint64_t sid(uint32_t bytes, int len) { return (uint64_t)len << 32 | (len == 4 ? bytes : bytes & ((1u << (8 * len)) - 1u)); }
static uint64_t sext(uint64_t s, int c) {
    const int len = (int)(s >> 32);
    return sid((uint32_t)s | (uint32_t)c << (8 * len), len + 1);
}

// exhaustive: every prefix of a key (and the empty one) extended by every byte
// fits: the expected outcome of the build (the key sets are drawn from fixed
// seeds): a set that is expected to pack must pack, whatever its fill
static void check_set(const char* name, const std::vector<TrieKey>& keys, uint32_t max_slots = kTrieMaxSlots,
                      bool fits = true) {
    std::unordered_map<uint64_t, int> dict;   // counted keys
    std::unordered_set<uint64_t> prefixes{0}; // trie nodes
    for (const TrieKey& k : keys) {
        if (k.lang == kTrieNoLang) continue;
        for (int d = 1; d <= k.len; ++d) prefixes.insert(sid(k.bytes, d));
        dict[sid(k.bytes, k.len)] = k.lang;
    }
    TrieImage t;
    const bool ok = trie_build(keys, max_slots, t);
    if (!fits) {
        // more nodes than the image has slots: the table is not eligible
        CHECK(!ok && prefixes.size() - 1 > max_slots, "%s: %zu nodes built in %u slots?", name, prefixes.size() - 1, max_slots);
        printf("%s: %zu keys, %zu nodes: too large for %u slots\n", name, keys.size(), prefixes.size() - 1, max_slots);
        return;
    }
    CHECK(ok, "%s: build failed (%zu keys, %zu nodes)", name, keys.size(), prefixes.size() - 1);
    if (!ok) return;
    printf("%s: %zu keys, %zu nodes in %zu slots (fill %.3f)\n", name, keys.size(), prefixes.size() - 1, t.words.size(),
           (double)(prefixes.size() - 1) / (double)t.words.size());
    CHECK(t.nodes + 1 == prefixes.size(), "%s: %u nodes, %zu prefixes", name, t.nodes, prefixes.size());
    CHECK(t.words.size() % 4 == 0 && t.words.size() <= max_slots, "%s: %zu words", name, t.words.size());
    CHECK(trie_lang(t.dead) == kTrieNoLang, "%s: dead entry has a language", name);
    const uint32_t dead_base = trie_base_slot(t.dead);
    CHECK(dead_base + 256 <= t.words.size(), "%s: dead base %u past the image", name, dead_base);
    // the dead state never matches
    for (int c = 0; c < 256; ++c) CHECK(trie_step(t, t.dead, (uint8_t)c) == t.dead, "%s: dead matches %d", name, c);
    std::set<uint32_t> bases{0u, dead_base};
    std::vector<uint8_t> occupied(t.words.size(), 0);
    for (const uint64_t pre : prefixes) {
        const int plen = (int)(pre >> 32);
        uint32_t e = 0;
        for (int d = 0; d < plen; ++d) {
            const uint8_t c = (uint8_t)(pre >> (8 * d));
            e = d == 0 ? trie_root(t, c) : trie_step(t, e, c);
        }
        if (plen) {
            const auto it = dict.find(pre);
            CHECK(trie_lang(e) == (it == dict.end() ? kTrieNoLang : (uint32_t)it->second), "%s: language of a node", name);
            CHECK(trie_base_slot(e) + 256 <= t.words.size(), "%s: a base past the image", name);
        }
        if (plen == kTrieMaxLen) {
            CHECK(trie_base_slot(e) == dead_base, "%s: a node of the last depth has a row", name);
            continue;
        }
        bool kids = false;
        for (int c = 0; c < 256; ++c) {
            const uint64_t s = sext(pre, c);
            const uint32_t n = plen == 0 ? trie_root(t, (uint8_t)c) : trie_step(t, e, (uint8_t)c);
            const bool node = prefixes.count(s) != 0;
            const auto it = dict.find(s);
            const uint32_t want = it == dict.end() ? kTrieNoLang : (uint32_t)it->second;
            CHECK(trie_lang(n) == want, "%s: %llx + %d language %u, want %u", name, (unsigned long long)pre, c,
                  trie_lang(n), want);
            if (!node) {
                // no node: the walk is dead from here on
                CHECK(trie_base_slot(n) == dead_base, "%s: a missing node is not dead", name);
            } else {
                kids = true;
                occupied[(plen == 0 ? 0u : trie_base_slot(e)) + (uint32_t)c] = 1;
            }
        }
        if (kids && plen) CHECK(bases.insert(trie_base_slot(e)).second, "%s: a base used twice", name);
        if (!kids && plen) CHECK(trie_base_slot(e) == dead_base, "%s: a leaf has a row", name);
    }
    // empty slots match no probe that can reach them: slot - check is no used base
    for (uint32_t s = 0; s < t.words.size(); ++s) {
        if (occupied[s]) continue;
        const uint32_t c = trie_check(t.words[s]);
        CHECK(c > s || !bases.count(s - c), "%s: empty slot %u matches base %u", name, s, s - c);
        CHECK(trie_lang(t.words[s]) == kTrieNoLang && trie_base_slot(t.words[s]) == dead_base,
              "%s: empty slot %u is not dead", name, s);
    }
}

static std::vector<TrieKey> random_keys(std::mt19937& rng, size_t n, const std::vector<uint8_t>& alpha, int langs) {
    std::set<std::string> seen;
    std::vector<TrieKey> keys;
    size_t tries = 0;
    while (keys.size() < n && tries++ < 50 * n) {
        const int len = 1 + (int)(rng() % 4);
        std::string s;
        for (int d = 0; d < len; ++d) s.push_back((char)alpha[rng() % alpha.size()]);
        if (seen.insert(s).second) keys.push_back(mk(s, (int)(rng() % (unsigned)langs)));
    }
    return keys;
}

int main(int argc, char** argv) {
    std::mt19937 rng(20261020);
    std::vector<uint8_t> a12, az, all, low;
    for (int c = 'a'; c < 'a' + 12; ++c) a12.push_back((uint8_t)c);
    for (int c = 'a'; c <= 'z'; ++c) az.push_back((uint8_t)c);
    for (int c = 0; c < 256; ++c) all.push_back((uint8_t)c);
    for (int c = 0; c < 12; ++c) low.push_back((uint8_t)c);
    const size_t sizes[] = {100, 1000, 5000, 12000};
    for (size_t n : sizes) {
        check_set("12 letters", random_keys(rng, n, a12, 20));
        check_set("a-z", random_keys(rng, n, az, 254));
        check_set("all bytes", random_keys(rng, n, all, 200), kTrieMaxSlots, n < 12000);  // (12,000: 22,971 nodes)
        check_set("bytes 0..11", random_keys(rng, n, low, 3));
    }
    check_set("chain", {mk("a", 0), mk("ab", 1), mk("abc", 2), mk("abcd", 3)});
    check_set("no prefix keys", {mk("abcd", 1), mk("abce", 2), mk("xyz", 3), mk("xq", 0)});
    check_set("uncounted prefix", {mk("ab", (int)kTrieNoLang), mk("abc", 4)});
    {
        std::vector<TrieKey> k;
        for (int len = 1; len <= 4; ++len) {
            k.push_back(mk(std::string((size_t)len, '\0'), len));
            k.push_back(mk(std::string((size_t)len, (char)0xff), 10 + len));
        }
        k.push_back(mk(std::string("\0\xff\0\xff", 4), 7));
        k.push_back(mk(std::string("\xff\0", 2), 8));
        check_set("0x00 / 0xff", k);
    }
    check_set("one key", {mk("q", 0)});
    check_set("empty", {});
    {  // out of the rule
        TrieImage t;
        CHECK(!trie_build({TrieKey{0, 5, 0}}, kTrieMaxSlots, t), "a 5-byte key builds");
        CHECK(!trie_build({mk("a", 254)}, kTrieMaxSlots, t), "language 254 builds");
        CHECK(!trie_build({mk("ab", 1), mk("ab", 2)}, kTrieMaxSlots, t), "two languages for one key build");
        CHECK(!trie_build(random_keys(rng, 12000, all, 20), 4096, t), "12,000 keys build in 4,096 slots");
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
        bool one = true;
        for (const TrieKey& k : keys) one &= k.lang != kTrieNoLang && k.len <= kTrieMaxLen;
        CHECK(one, "the table has a row out of the rule");
        // two workgroups of twelve waves per CU: 81,920 B each, one slice, 260-word staging buffers
        constexpr uint32_t kBudget = 81920, kPerWave = trie_lds_bytes(0, 1, 12, 260);
        TrieImage t;
        const bool ok = trie_build(keys, (kBudget - kPerWave) / 4, t);
        CHECK(ok, "the table does not fit %u B", kBudget - kPerWave);
        check_set("table", keys, (kBudget - kPerWave) / 4);
        if (ok)
            printf("table: %zu keys, %u nodes, %u rows, image %zu B of %u B (fill %.3f), LDS per workgroup %u B\n",
                   keys.size(), t.nodes, t.rows, t.words.size() * 4, kBudget - kPerWave,
                   (double)(t.nodes + 206) / (double)t.words.size(), trie_lds_bytes((uint32_t)t.words.size(), 1, 12, 260));
    }
    if (g_fail) return 1;
    printf("trie_check ok\n");
    return 0;
}
