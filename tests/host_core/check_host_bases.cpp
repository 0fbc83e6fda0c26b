// check_host_bases.cpp - the host's one definition each of "a base from the 2-bit words", "a column's code", "four columns to a byte" and "a loop dealt
// out to threads" (necat_amd/csrc/host_bases.h, host_threads.h), on the CPU, against restatements that take one base / one column / one index at a time.
//
//   usage: check_host_bases        exit status 0 and "check_host_bases: ok" when everything holds
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "host_bases.h"
#include "host_threads.h"

using namespace necat_host;

static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

// ---- (a) decode: a volume whose reads start at offsets = 0, 1, 31, 32, 33 (mod 32), one of them empty, the last one ending on the volume's last base
static void check_decode()
{
    // lengths that put the reads at offsets 0, 1, 31, 31 (behind the empty read), 64, 97, 161, 192, 289
    const uint64_t len[] = {1, 30, 0, 33, 33, 64, 31, 97, 70};
    const size_t nseq = sizeof len / sizeof len[0];
    std::vector<uint64_t> off(nseq + 1, 0);
    for (size_t i = 0; i < nseq; ++i) off[i + 1] = off[i] + len[i];
    const uint64_t nbases = off[nseq];
    const uint64_t want_mod[] = {0, 1, 31, 31, 0, 1, 1, 0, 1};
    for (size_t i = 0; i < nseq; ++i) CHECK(off[i] % 32 == want_mod[i], "read %zu starts at %lu", i, (unsigned long)off[i]);
    bool m32 = false, m33 = false;
    std::vector<uint64_t> len2 = {32, 1, 40};                             // a second volume for the offsets 32 and 33
    std::vector<uint64_t> off2(len2.size() + 1, 0);
    for (size_t i = 0; i < len2.size(); ++i) off2[i + 1] = off2[i] + len2[i];
    for (uint64_t o : off2) { m32 = m32 || o == 32; m33 = m33 || o == 33; }
    CHECK(m32 && m33, "the second volume has no read at offset 32 / 33");

    auto run = [&](const std::vector<uint64_t>& so, uint64_t nb) {
        std::vector<uint8_t> base(nb);                                    // the volume one base per byte: the restatement reads this
        uint64_t x = 0x9e3779b97f4a7c15ULL;
        for (uint64_t g = 0; g < nb; ++g) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; base[g] = (uint8_t)(x & 3); }
        std::vector<uint64_t> words((nb + 31) / 32, 0);                    // exactly the words that hold bases: a read past the last one is an error under the sanitizers
        for (uint64_t g = 0; g < nb; ++g) words[g >> 5] |= (uint64_t)base[g] << ((g & 31) * 2);
        const size_t ns = so.size() - 1;
        CHECK(so[ns] == nb, "the last read does not end on the volume's last base");
        for (size_t id = 0; id < ns; ++id) {
            const uint64_t b = so[id], n = so[id + 1] - b;
            // the whole array, and the slice that starts at the read's first word (exactly its words)
            BaseWords whole; whole.w = words.data(); whole.word0 = 0; whole.seq_off = so.data();
            std::vector<uint64_t> slice;
            if (n) slice.assign(words.begin() + (ptrdiff_t)(b >> 5), words.begin() + (ptrdiff_t)((b + n - 1) >> 5) + 1);
            BaseWords part; part.w = slice.data(); part.word0 = b >> 5; part.seq_off = so.data();
            CHECK(whole.size((int64_t)id) == n, "size of read %zu", id);
            std::vector<std::pair<int64_t, int64_t>> ranges = {{0, (int64_t)n}, {0, 0}, {(int64_t)n, (int64_t)n}};
            if (n) { ranges.push_back({0, 1}); ranges.push_back({(int64_t)n - 1, (int64_t)n}); ranges.push_back({(int64_t)n / 2, (int64_t)n / 2}); ranges.push_back({(int64_t)n / 2, (int64_t)n / 2 + 1}); }
            if (n > 3) { ranges.push_back({1, (int64_t)n - 1}); ranges.push_back({(int64_t)n / 3, (int64_t)(2 * n / 3)}); }
            for (int rev = 0; rev < 2; ++rev)
                for (auto& r : ranges) {
                    const size_t m = (size_t)(r.second - r.first);
                    std::vector<uint8_t> want(m);
                    for (int64_t i = r.first; i < r.second; ++i)
                        want[(size_t)(i - r.first)] = rev ? (uint8_t)(3 - base[b + n - 1 - (uint64_t)i]) : base[b + (uint64_t)i];
                    for (const BaseWords* v : {&whole, &part}) {
                        std::vector<uint8_t> got(m + 2, 0xAA);             // guard bytes on both sides
                        v->decode((int64_t)id, rev, r.first, r.second, got.data() + 1);
                        CHECK(got[0] == 0xAA && got[m + 1] == 0xAA, "read %zu rev %d [%ld, %ld): wrote outside its range", id, rev, (long)r.first, (long)r.second);
                        CHECK(m == 0 || memcmp(got.data() + 1, want.data(), m) == 0, "read %zu rev %d [%ld, %ld) from word %lu", id, rev, (long)r.first, (long)r.second,
                              (unsigned long)v->word0);
                    }
                }
            for (int rev = 0; rev < 2; ++rev) {
                std::vector<uint8_t> got(7, 9), want(n);
                part.strand((int64_t)id, rev, got);
                for (uint64_t i = 0; i < n; ++i) want[i] = rev ? (uint8_t)(3 - base[b + n - 1 - i]) : base[b + i];
                CHECK(got == want, "strand %d of read %zu", rev, id);
            }
        }
    };
    run(off, nbases);
    run(off2, off2.back());
}

// ---- (a2) slices and stretches: what the stages decode that is no whole sequence - a slice (g0, dir, comp, len) as the kernels address one, and the n bases
// from base g on either strand - inside a word, on word boundaries, of length 0 (also where no word exists any more) and on the volume's last base
static void check_slices()
{
    const uint64_t nb = 5 * 32 + 7;                                       // the last base lies inside the sixth word
    std::vector<uint8_t> base(nb);
    uint64_t x = 0x2545f4914f6cdd1dULL;
    for (uint64_t g = 0; g < nb; ++g) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; base[g] = (uint8_t)(x & 3); }
    std::vector<uint64_t> words((nb + 31) / 32, 0);                        // exactly the words that hold bases
    for (uint64_t g = 0; g < nb; ++g) words[g >> 5] |= (uint64_t)base[g] << ((g & 31) * 2);
    // (first base, length) on the forward strand: inside a word, from a boundary to a boundary, across boundaries from inside to inside, one word and two,
    // length 0 at a boundary, inside a word and behind the last base, the last base alone, a stretch that ends on it, the whole volume
    const std::pair<uint64_t, int64_t> spans[] = {{5, 20}, {32, 32}, {32, 64}, {37, 70}, {31, 2}, {63, 1}, {64, 1}, {0, 0}, {32, 0}, {45, 0}, {nb, 0}, {nb - 1, 1}, {nb - 9, 9},
                                                  {128, (int64_t)nb - 128}, {0, (int64_t)nb}};
    for (const auto& sp : spans) {
        const uint64_t g = sp.first;
        const int64_t n = sp.second;
        // the view of the whole array, and one that starts at the span's first word and holds exactly its words
        BaseWords whole; whole.w = words.data();
        std::vector<uint64_t> part_words;
        if (n) part_words.assign(words.begin() + (ptrdiff_t)(g >> 5), words.begin() + (ptrdiff_t)((g + (uint64_t)n - 1) >> 5) + 1);
        BaseWords part; part.w = part_words.data(); part.word0 = g >> 5;
        for (int rev = 0; rev < 2; ++rev) {
            std::vector<uint8_t> want((size_t)n);
            for (int64_t i = 0; i < n; ++i) want[(size_t)i] = rev ? (uint8_t)(3 - base[g + (uint64_t)(n - 1 - i)]) : base[g + (uint64_t)i];
            for (const BaseWords* v : {&whole, &part}) {
                std::vector<uint8_t> got((size_t)n + 2, 0xAA), got2((size_t)n + 2, 0xAA);
                v->stretch(g, n, rev, got.data() + 1);
                if (rev) v->slice((int64_t)g + n - 1, -1, 1, n, got2.data() + 1); else v->slice((int64_t)g, 1, 0, n, got2.data() + 1);
                CHECK(got[0] == 0xAA && got[(size_t)n + 1] == 0xAA && got2[0] == 0xAA && got2[(size_t)n + 1] == 0xAA, "bases %lu + %ld rev %d: wrote outside the range", (unsigned long)g, (long)n, rev);
                CHECK(n == 0 || memcmp(got.data() + 1, want.data(), (size_t)n) == 0, "stretch of bases %lu + %ld rev %d from word %lu", (unsigned long)g, (long)n, rev, (unsigned long)v->word0);
                CHECK(n == 0 || memcmp(got2.data() + 1, want.data(), (size_t)n) == 0, "slice of bases %lu + %ld rev %d from word %lu", (unsigned long)g, (long)n, rev, (unsigned long)v->word0);
            }
        }
        // the two mixed forms a slice also allows: backwards without the complement, forwards with it
        if (n) {
            std::vector<uint8_t> got((size_t)n), want((size_t)n);
            for (int64_t i = 0; i < n; ++i) want[(size_t)i] = base[g + (uint64_t)(n - 1 - i)];
            whole.slice((int64_t)g + n - 1, -1, 0, n, got.data());
            CHECK(got == want, "slice of bases %lu + %ld backwards, not complemented", (unsigned long)g, (long)n);
            for (int64_t i = 0; i < n; ++i) want[(size_t)i] = (uint8_t)(3 - base[g + (uint64_t)i]);
            whole.slice((int64_t)g, 1, 1, n, got.data());
            CHECK(got == want, "slice of bases %lu + %ld forwards, complemented", (unsigned long)g, (long)n);
        }
    }
}

// ---- (b) columns
static void check_columns()
{
    const char* sym = "ACGT-";
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
            if (a == 4 && b == 4) continue;                                // a column of two gaps does not occur
            const char q = sym[a], t = sym[b];
            int want;
            if (q == '-') want = 2; else if (t == '-') want = 1; else if (q == t) want = 0; else want = 3;
            CHECK(col_code(q, t) == want, "col_code('%c', '%c') = %d, not %d", q, t, col_code(q, t), want);
        }
    for (size_t n : {0, 1, 3, 4, 5, 9}) {
        std::vector<uint8_t> codes(n);
        for (size_t j = 0; j < n; ++j) codes[j] = (uint8_t)((j * 7 + 3) & 3);
        const size_t nb = (n + 3) / 4;
        std::vector<uint8_t> got(nb + 2, 0xAA), want(nb, 0);
        for (size_t j = 0; j < n; ++j) want[j / 4] = (uint8_t)(want[j / 4] + (codes[j] << (2 * (j % 4))));
        pack_cols(codes.data(), n, got.data() + 1);
        CHECK(got[0] == 0xAA && got[nb + 1] == 0xAA, "pack_cols(%zu) wrote outside its %zu bytes", n, nb);
        CHECK(nb == 0 || memcmp(got.data() + 1, want.data(), nb) == 0, "pack_cols(%zu)", n);
        std::vector<uint8_t> got2(nb + 1, 0xFF);                           // the callable form, over bytes that were not zero
        pack_cols_of(n, got2.data(), [&](size_t j) { return codes[j]; });
        CHECK(got2[nb] == 0xFF && (nb == 0 || memcmp(got2.data(), want.data(), nb) == 0), "pack_cols_of(%zu)", n);
    }
}

// ---- (c) threads: every index exactly once, thread ids below nt
static void check_threads()
{
    for (uint64_t n : {0, 1, 63, 64, 65, 1000})
        for (unsigned nt : {1u, 2u, 7u})
            for (uint64_t grain : {1, 8, 64}) {
                std::vector<int> seen(n, 0);
                std::mutex mu;
                unsigned max_tid = 0;
                bool past = false;
                deal(n, nt, grain, [&](uint64_t i, unsigned tid) {
                    std::lock_guard<std::mutex> lk(mu);
                    if (i < n) ++seen[i]; else past = true;
                    max_tid = std::max(max_tid, tid);
                });
                bool once = !past;
                for (uint64_t i = 0; i < n; ++i) once = once && seen[i] == 1;
                CHECK(once, "deal(n %lu, nt %u, grain %lu) did not visit every index exactly once", (unsigned long)n, nt, (unsigned long)grain);
                CHECK(max_tid < nt, "deal(n %lu, nt %u, grain %lu) passed thread id %u", (unsigned long)n, nt, (unsigned long)grain, max_tid);
            }
    std::vector<int> ran(7, 0);                                            // on_threads: each id once (distinct elements: no lock needed)
    on_threads(7, [&](unsigned tid) { ++ran[tid]; });
    for (int r : ran) CHECK(r == 1, "on_threads(7) ran an id %d times", r);
}

int main()
{
    check_decode();
    check_slices();
    check_columns();
    check_threads();
    if (g_fail) { printf("check_host_bases: %ld checks failed\n", g_fail); return 1; }
    printf("check_host_bases: ok\n");
    return 0;
}
