// check_vol_gather.cpp - necat_volume_gather's plan and word function (necat_amd/csrc/volume_gather.h) and oc2cns's chunk planner (cns_chunks.h), on the CPU.
// The word function - the one k_vol_gather runs per destination word - is run for EVERY destination word of a gather and compared against a base-by-base
// merge: three source volumes of 1 003, 4 097 and 64 bases tiled with reads of 1, 2, 31, 32, 33, 63, 64, 65, 97 and 1 000 bases, a random half of the reads
// gathered, tiling after tiling until every one of the 32 x 32 pairs (source offset mod 32, destination offset mod 32) has been seen with a read of at least 65
// bases and with a read below 32 (asserted).  The source words are held without a word of slack, so a read outside a sequence's own words is an error under
// -fsanitize=address.  Then: ten one-base reads in one word, the first and the last read of a volume, a last read that ends in mid-word with zero bits behind
// it, the empty list, every refusal of the plan (the 2^32 total with sizes only), the field swap of pac bytes, and the chunk planner.
//
//   usage: check_vol_gather [first_base]        exit status 0 and "check_vol_gather: ok" when everything holds
// first_base ("straddle" or "top", high_base.h): instead of the above, one source volume whose test reads lie behind filler sequences of zero bases (at most 2^29
// each) in a words buffer that really is that large - around base 2^31, or ending at base 2^32 - 2.  The test reads are gathered alone (source high, destination
// low), then all sequences (every destination word from the test reads' first on: word indices above 2^26), then all but the first filler with every other test
// read (source and destination out of step by an odd count).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "volume_gather.h"
#include "cns_chunks.h"
#include "host_bases.h"
#include "high_base.h"

using namespace necat;

static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static u64 g_rng = 0x9E3779B97F4A7C15ULL;
static u64 rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct Vol {
    std::vector<u8> codes;           // one base per byte
    std::vector<u64> seq_off;        // nseq + 1
    std::vector<u64> words;          // exactly (nbases + 31) / 32 of them
    u64 nseq() const { return seq_off.size() - 1; }
};

static void pack_words(Vol& v)
{
    v.words.assign((v.codes.size() + 31) / 32, 0);
    for (size_t g = 0; g < v.codes.size(); ++g) v.words[g >> 5] |= (u64)v.codes[g] << (2 * (g & 31));
}

static Vol make_vol(u64 nbases, const std::vector<u64>& sizes)
{
    Vol v;
    v.codes.resize(nbases);
    for (auto& c : v.codes) c = (u8)(rnd() & 3);
    v.seq_off.push_back(0);
    for (u64 s : sizes) v.seq_off.push_back(v.seq_off.back() + s);
    CHECK(v.seq_off.back() == nbases, "the reads tile %lu bases, the volume has %lu", (unsigned long)v.seq_off.back(), (unsigned long)nbases);
    pack_words(v);
    return v;
}

static const u64 kLens[] = {1, 2, 31, 32, 33, 63, 64, 65, 97, 1000};

static std::vector<u64> random_tiling(u64 nbases)
{
    std::vector<u64> sizes;
    for (u64 left = nbases; left;) {
        u64 len = kLens[rnd() % 10];
        if (len > left) continue;          // (1 always fits)
        sizes.push_back(len); left -= len;
    }
    return sizes;
}

// the plan, every destination word through gather_word, and both against the base-by-base merge; returns the plan's total
static u64 gather_and_compare(const std::vector<Vol>& vols, const std::vector<i64>& start, const std::vector<i64>& ids, const char* what, vgather::Plan* plan_out = nullptr)
{
    std::vector<const u64*> so, words; std::vector<u64> ns;
    for (const Vol& v : vols) { so.push_back(v.seq_off.data()); words.push_back(v.words.data()); ns.push_back(v.nseq()); }
    vgather::Plan p;
    char err[256] = "";
    const bool ok = vgather::make_plan(so.data(), ns.data(), start.data(), vols.size(), ids.data(), ids.size(), &p, err, sizeof err);
    CHECK(ok, "%s: the plan was refused: %s", what, err);
    if (!ok) return 0;
    std::vector<u8> want;                  // the merge, base by base
    std::vector<u64> want_off(1, 0);
    for (i64 id : ids) {
        size_t k = 0;
        while (!(id >= start[k] && (u64)(id - start[k]) < vols[k].nseq())) ++k;
        const u64 b = vols[k].seq_off[id - start[k]], e = vols[k].seq_off[id - start[k] + 1];
        want.insert(want.end(), vols[k].codes.begin() + b, vols[k].codes.begin() + e);
        want_off.push_back(want.size());
    }
    CHECK(p.dst_off == want_off, "%s: the destination offsets differ", what);
    CHECK(p.n() == ids.size() && p.nbases() == want.size(), "%s: %lu sequences of %lu bases planned, %zu of %zu wanted", what, (unsigned long)p.n(), (unsigned long)p.nbases(), ids.size(), want.size());
    const u64 nwords = (want.size() + 31) / 32;
    for (u64 w = 0; w < nwords; ++w) {
        u64 expect = 0;
        for (u64 g = 32 * w; g < 32 * w + 32 && g < want.size(); ++g) expect |= (u64)want[g] << (2 * (g & 31));
        const u64 got = vgather::gather_word(w, p.dst_off.data(), p.src_off.data(), p.src_vol.data(), p.n(), words.data());
        CHECK(got == expect, "%s: word %lu of %lu is %016lx, the merge has %016lx", what, (unsigned long)w, (unsigned long)nwords, (unsigned long)got, (unsigned long)expect);
    }
    if (plan_out) *plan_out = p;
    return p.nbases();
}

static void check_pairs()
{
    static bool seen_long[32][32], seen_short[32][32];
    long left = 2 * 32 * 32, rounds = 0;
    while (left > 0 && rounds < 200000) {
        ++rounds;
        std::vector<Vol> vols;
        std::vector<i64> st(3);
        i64 at = (i64)(rnd() % 5);              // (global ids need not start at 0, and a gap between volumes is fine)
        for (int k = 0; k < 3; ++k) {
            const u64 nb = k == 0 ? 1003 : (k == 1 ? 4097 : 64);
            vols.push_back(make_vol(nb, random_tiling(nb)));
            st[k] = at; at += (i64)vols.back().nseq() + (i64)(rnd() % 3);
        }
        std::vector<i64> ids;
        for (int k = 0; k < 3; ++k) for (u64 i = 0; i < vols[k].nseq(); ++i) if (rnd() & 1) ids.push_back(st[k] + (i64)i);
        vgather::Plan p;
        gather_and_compare(vols, st, ids, "random tiling", &p);
        for (u64 i = 0; i < p.n(); ++i) {
            const u64 len = p.dst_off[i + 1] - p.dst_off[i];
            const unsigned s = (unsigned)(p.src_off[i] & 31), d = (unsigned)(p.dst_off[i] & 31);
            if (len >= 65 && !seen_long[s][d]) { seen_long[s][d] = true; --left; }
            if (len < 32 && !seen_short[s][d]) { seen_short[s][d] = true; --left; }
        }
    }
    CHECK(left == 0, "%ld of the 2 x 32 x 32 (source offset, destination offset) cases were never generated in %ld tilings", left, rounds);
    printf("pairs: all 32 x 32 offset pairs with a read >= 65 and with a read < 32 after %ld tilings\n", rounds);
}

static void check_edges()
{
    // ten one-base reads in one word, between two longer ones
    {
        std::vector<u64> sizes = {40};
        for (int i = 0; i < 10; ++i) sizes.push_back(1);
        sizes.push_back(50);
        std::vector<Vol> vols = {make_vol(100, sizes)};
        std::vector<i64> ids;
        for (i64 i = 1; i <= 10; ++i) ids.push_back(i);
        CHECK(gather_and_compare(vols, {0}, ids, "ten one-base reads") == 10, "ten one-base reads are ten bases");
        gather_and_compare(vols, {0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, "the whole volume");
        gather_and_compare(vols, {7}, {8, 10, 12, 14, 16, 18}, "every other read, ids from 7");
    }
    // the first and the last read of every volume; the last read ends in mid-word: the bits behind it are zero (the comparison's expectation has them zero)
    {
        std::vector<Vol> vols = {make_vol(1003, {500, 3, 500}), make_vol(4097, {1, 4095, 1}), make_vol(64, {32, 32})};
        const std::vector<i64> st = {0, 3, 6};
        gather_and_compare(vols, st, {0, 2, 3, 5, 6, 7}, "first and last reads");
        CHECK(gather_and_compare(vols, st, {2}, "the last read of volume 0 alone") == 500, "500 bases");
        CHECK(gather_and_compare(vols, st, {5}, "one base") == 1, "1 base");
        gather_and_compare(vols, st, {0, 1, 2, 3, 4, 5, 6, 7}, "everything");
        // volumes given in another order than their ids
        std::vector<Vol> swapped = {vols[2], vols[0], vols[1]};
        gather_and_compare(swapped, {6, 0, 3}, {0, 2, 3, 5, 6, 7}, "volumes out of id order");
    }
    // a read of no bases takes no bits and keeps its id
    {
        std::vector<Vol> vols = {make_vol(70, {33, 0, 0, 37})};
        vgather::Plan p;
        gather_and_compare(vols, {0}, {0, 1, 2, 3}, "empty reads", &p);
        CHECK(p.n() == 4 && p.dst_off[1] == 33 && p.dst_off[2] == 33 && p.dst_off[3] == 33, "empty reads keep their places");
        gather_and_compare(vols, {0}, {1, 2}, "only empty reads");
    }
    // the empty list
    {
        std::vector<Vol> vols = {make_vol(64, {64})};
        vgather::Plan p;
        CHECK(gather_and_compare(vols, {0}, {}, "the empty list", &p) == 0 && p.n() == 0 && p.dst_off.size() == 1, "the empty list gives an empty plan");
        CHECK(gather_and_compare({}, {}, {}, "no volumes, no ids") == 0, "nothing from nothing");
    }
}

static bool refused(const std::vector<std::vector<u64>>& seq_off, const std::vector<i64>& start, const std::vector<i64>& ids, const char* word)
{
    std::vector<const u64*> so; std::vector<u64> ns;
    for (auto& s : seq_off) { so.push_back(s.data()); ns.push_back(s.size() - 1); }
    vgather::Plan p;
    char err[256] = "";
    const bool ok = vgather::make_plan(so.data(), ns.data(), start.data(), seq_off.size(), ids.data(), ids.size(), &p, err, sizeof err);
    if (ok) { printf("not refused (expected: %s)\n", word); return false; }
    if (!strstr(err, word)) { printf("refused with '%s', expected a message with '%s'\n", err, word); return false; }
    return true;
}

static void check_refusals()
{
    const std::vector<std::vector<u64>> two = {{0, 10, 20, 30}, {0, 5, 9}};       // ids 0 .. 2 and 5 .. 6
    const std::vector<i64> st = {0, 5};
    CHECK(refused(two, st, {1, 1}, "ascend"), "an id twice");
    CHECK(refused(two, st, {2, 1}, "ascend"), "ids descending");
    CHECK(refused(two, st, {0, 6, 5}, "ascend"), "ids descending across volumes");
    CHECK(refused(two, st, {3}, "in no volume"), "an id in the gap between the volumes");
    CHECK(refused(two, st, {0, 7}, "in no volume"), "an id past the last volume");
    CHECK(refused(two, st, {-1, 0}, "in no volume"), "a negative id");
    CHECK(refused(two, {0, 2}, {0}, "overlap"), "volumes whose id ranges overlap");
    CHECK(refused(two, {5, 5}, {}, "overlap"), "two volumes from the same id, no ids asked for");
    {   // adjacent ranges, given out of order, are accepted
        std::vector<const u64*> so = {two[0].data(), two[1].data()}; std::vector<u64> ns = {3, 2};
        const std::vector<i64> s2 = {2, 0}, ids = {0, 1, 2, 4};
        vgather::Plan p; char err[256] = "";
        CHECK(vgather::make_plan(so.data(), ns.data(), s2.data(), 2, ids.data(), ids.size(), &p, err, sizeof err) && p.nbases() == 5 + 4 + 10 + 10, "adjacent id ranges: %s", err);
    }
    // 2^32 bases in all: sizes only, no bases anywhere
    {
        std::vector<u64> big = {0};
        for (int i = 0; i < 5; ++i) big.push_back(big.back() + 1000000000ULL);
        const std::vector<std::vector<u64>> vols = {big, {0, (1ULL << 32) - 4000000000ULL - 1, (1ULL << 32) - 4000000000ULL}};
        CHECK(refused(vols, {0, 5}, {0, 1, 2, 3, 4}, "2^32"), "five reads of 10^9 bases");
        CHECK(refused(vols, {0, 5}, {0, 1, 2, 3, 5, 6}, "2^32"), "exactly 2^32 bases across two volumes");
        std::vector<const u64*> so = {vols[0].data(), vols[1].data()}; std::vector<u64> ns = {5, 2};
        const std::vector<i64> st2 = {0, 5}, ids = {0, 1, 2, 3, 5};
        vgather::Plan p; char err[256] = "";
        CHECK(vgather::make_plan(so.data(), ns.data(), st2.data(), 2, ids.data(), ids.size(), &p, err, sizeof err) && p.nbases() == (1ULL << 32) - 1, "2^32 - 1 bases are a volume: %s", err);
    }
}

static void check_swap()
{
    // pac bytes -> words and back: the first base of a byte sits in its top two bits, base g of a word in bits 2 (g & 31)
    std::vector<u8> codes(64), back(64);
    for (auto& c : codes) c = (u8)(rnd() & 3);
    u8 pac[16] = {0};
    for (int g = 0; g < 64; ++g) pac[g >> 2] |= (u8)(codes[g] << ((~g & 3) << 1));
    u64 w[2];
    memcpy(w, pac, 16);
    for (int k = 0; k < 2; ++k) {
        const u64 x = vgather::swap_fields(w[k]);
        for (int g = 0; g < 32; ++g) CHECK(((x >> (2 * g)) & 3) == codes[32 * k + g], "base %d of word %d after the swap", g, k);
        CHECK(vgather::swap_fields(x) == w[k], "the swap is its own inverse");
    }
    necat_host::decode_pac(pac, 0, 64, back.data());
    CHECK(back == codes, "decode_pac of the whole");
    necat_host::decode_pac(pac, 5, 40, back.data());
    CHECK(memcmp(back.data(), codes.data() + 5, 40) == 0, "decode_pac from base 5");
}

// ---- the chunk planner
using necat_host::cns_chunks::Plan;
using necat_host::cns_chunks::plan_chunks;

static std::vector<uint32_t> records(const std::vector<std::pair<uint32_t, uint32_t>>& tq)
{
    std::vector<uint32_t> r;
    uint32_t k = 0;
    for (auto& p : tq) { const uint32_t w[7] = {100 + k, p.first, 1, 2, p.second, 3, 4}; r.insert(r.end(), w, w + 7); ++k; }
    return r;
}

// what every plan must hold: whole templates in ascending order, every record once, per chunk the ids of its records' reads, sorted, each once, and their bases
static void check_plan(const std::vector<uint32_t>& rec, const std::vector<u64>& size, u64 bound, const Plan& p, const char* what)
{
    const u64 n = rec.size() / 7;
    CHECK(p.order.size() == n, "%s: %zu records ordered of %lu", what, p.order.size(), (unsigned long)n);
    u64 at = 0;
    long last_tid = -1;
    for (const auto& c : p.chunks) {
        CHECK(c.rec_begin == at && c.rec_end > c.rec_begin && c.n_templates > 0, "%s: a chunk's record range", what);
        at = c.rec_end;
        std::vector<i64> ids;
        u64 nt = 0;
        for (u64 k = c.rec_begin; k < c.rec_end; ++k) {
            const uint32_t tid = rec[7 * p.order[k] + 1], qid = rec[7 * p.order[k] + 4];
            if (k == c.rec_begin) CHECK((long)tid > last_tid, "%s: a template in two chunks", what);
            else CHECK((long)tid >= last_tid, "%s: templates do not ascend", what);
            if ((long)tid != last_tid) ++nt;
            last_tid = (long)tid;
            ids.push_back(tid); ids.push_back(qid);
        }
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        u64 bases = 0;
        for (i64 id : ids) bases += size[(size_t)id];
        CHECK(ids == c.ids && bases == c.bases && nt == c.n_templates, "%s: a chunk's reads, bases or template count", what);
        CHECK(c.bases <= bound || c.n_templates == 1, "%s: %lu bases in a chunk of %lu templates, the bound is %lu", what, (unsigned long)c.bases, (unsigned long)c.n_templates, (unsigned long)bound);
        std::vector<uint32_t> out((size_t)(c.rec_end - c.rec_begin) * 7);
        necat_host::cns_chunks::chunk_records(rec.data(), p, c, out.data());
        for (u64 k = c.rec_begin; k < c.rec_end; ++k) {
            const uint32_t* a = rec.data() + 7 * p.order[k]; const uint32_t* b = out.data() + 7 * (k - c.rec_begin);
            CHECK(b[1] < c.ids.size() && b[4] < c.ids.size() && c.ids[b[1]] == (i64)a[1] && c.ids[b[4]] == (i64)a[4], "%s: a rewritten id does not map back", what);
            CHECK(a[0] == b[0] && a[2] == b[2] && a[3] == b[3] && a[5] == b[5] && a[6] == b[6], "%s: a rewritten record's other words changed", what);
        }
    }
    CHECK(at == n, "%s: the chunks cover %lu of %lu records", what, (unsigned long)at, (unsigned long)n);
    // the order is stable inside a template: file order
    for (u64 k = 1; k < n; ++k) if (rec[7 * p.order[k] + 1] == rec[7 * p.order[k - 1] + 1]) CHECK(p.order[k] > p.order[k - 1], "%s: a template's records left file order", what);
}

static void check_chunks()
{
    // eight reads of 100 bases and read 8 of 1 000; templates 0 .. 5 (records in shuffled file order), each with two queries; read 7 is a query of templates 1 and 4
    const std::vector<u64> size = {100, 100, 100, 100, 100, 100, 100, 100, 1000};
    const std::vector<uint32_t> rec = records({{4, 7}, {0, 1}, {2, 3}, {1, 7}, {5, 6}, {0, 2}, {3, 4}, {1, 0}, {2, 1}, {4, 5}, {5, 4}, {3, 2}});
    std::string err;
    Plan p;
    CHECK(plan_chunks(rec.data(), rec.size() / 7, size.data(), size.size(), 1ULL << 31, &p, &err) && p.chunks.size() == 1, "one chunk under a large bound");
    check_plan(rec, size, 1ULL << 31, p, "one chunk");
    CHECK(p.chunks[0].n_templates == 6 && p.chunks[0].bases == 800, "one chunk: six templates, eight reads of 100 bases");
    CHECK(plan_chunks(rec.data(), rec.size() / 7, size.data(), size.size(), 400, &p, &err) && p.chunks.size() == 3, "three chunks at 400 bases: %zu", p.chunks.size());
    check_plan(rec, size, 400, p, "three chunks");
    // read 7 is in the chunk of template 1 and in the chunk of template 4; reads 2 .. 4 are shared by neighbours too
    {
        int with7 = 0;
        for (const auto& c : p.chunks) with7 += std::binary_search(c.ids.begin(), c.ids.end(), (i64)7);
        CHECK(with7 == 2, "read 7 is gathered for %d chunks, two name it", with7);
    }
    CHECK(plan_chunks(rec.data(), rec.size() / 7, size.data(), size.size(), 1, &p, &err) && p.chunks.size() == 6, "a chunk per template at a bound of one base: %zu", p.chunks.size());
    check_plan(rec, size, 1, p, "n chunks");
    for (const auto& c : p.chunks) CHECK(c.n_templates == 1 && c.bases == 300, "a template with two queries is 300 bases");
    // a template alone above the bound: a chunk of its own, its neighbours in theirs
    const std::vector<uint32_t> big = records({{0, 1}, {1, 2}, {2, 8}, {2, 3}, {3, 4}, {4, 5}});
    CHECK(plan_chunks(big.data(), big.size() / 7, size.data(), size.size(), 500, &p, &err) && p.chunks.size() == 3, "a template above the bound: %zu chunks", p.chunks.size());
    check_plan(big, size, 500, p, "a template above the bound");
    CHECK(p.chunks.size() == 3 && p.chunks[1].n_templates == 1 && p.chunks[1].bases == 1200 && p.chunks[0].n_templates == 2 && p.chunks[2].n_templates == 2, "the big template is alone");
    // nothing, and a record that names a read the project does not have
    CHECK(plan_chunks(nullptr, 0, size.data(), size.size(), 500, &p, &err) && p.chunks.empty() && p.order.empty(), "no records, no chunks");
    const std::vector<uint32_t> bad = records({{0, 1}, {1, 9}});
    CHECK(!plan_chunks(bad.data(), 2, size.data(), size.size(), 500, &p, &err) && err.find("record 1") != std::string::npos, "a query outside the read set: '%s'", err.c_str());
}

// ---- the high form
static void check_high(const char* arg)
{
    const u64 kFill = 1ULL << 29;
    std::vector<u64> sizes = random_tiling(20011);          // reads of 1 .. 1 000 bases
    sizes.insert(sizes.begin() + (long)sizes.size() / 2, 4097);          // the one that straddles
    u64 total = 0;
    for (u64 x : sizes) total += x;
    const u64 first = high_base::first_base(arg, total);
    CHECK(first > kFill + 7, "the first base %lu leaves no room for the fillers", (unsigned long)first);
    std::vector<u64> seq_off(1, 0);
    seq_off.push_back(kFill - 7);          // (an odd filler first: leaving it out moves every later base by a count that is no multiple of 32)
    while (first - seq_off.back() > kFill) seq_off.push_back(seq_off.back() + kFill);
    seq_off.push_back(first);
    const u64 k = seq_off.size() - 1;          // fillers in front
    for (u64 x : sizes) seq_off.push_back(seq_off.back() + x);
    const u64 nbases = seq_off.back(), nseq = seq_off.size() - 1;
    CHECK(nbases == first + total && nbases < (1ULL << 32), "%lu bases", (unsigned long)nbases);
    std::vector<u8> codes(total);
    for (auto& c : codes) c = (u8)(rnd() & 3);
    std::vector<u64> words((size_t)((nbases + 31) / 32), 0);          // no slack
    CHECK(words.size() > (1ULL << 26), "%zu words", words.size());
    for (u64 i = 0; i < total; ++i) words[(size_t)((first + i) >> 5)] |= (u64)codes[i] << (2 * ((first + i) & 31));
    bool straddles = false;
    for (u64 i = k; i < nseq; ++i) straddles |= seq_off[i] < (1ULL << 31) && (1ULL << 31) < seq_off[i + 1];
    if (!strcmp(arg, "straddle")) CHECK(straddles && first % 32 == 13, "no test read straddles base 2^31 (first base %lu)", (unsigned long)first);
    if (!strcmp(arg, "top")) CHECK(nbases == (1ULL << 32) - 1 && first > (1ULL << 31), "top: %lu bases", (unsigned long)nbases);
    auto base = [&](u64 g) { return g < first ? (u8)0 : codes[(size_t)(g - first)]; };
    const u64* so = seq_off.data(); const u64* wp = words.data(); const i64 st = 0;
    // ids, and the destination words [w_from, end) compared with the merge (the words before hold filler zeros: a few are sampled)
    auto run = [&](const std::vector<i64>& ids, const char* what) {
        vgather::Plan p; char err[256] = "";
        const bool ok = vgather::make_plan(&so, &nseq, &st, 1, ids.data(), ids.size(), &p, err, sizeof err);
        CHECK(ok, "%s: the plan was refused: %s", what, err);
        if (!ok) return;
        u64 want_total = 0, first_test = ~0ULL;
        for (size_t i = 0; i < ids.size(); ++i) {
            if ((u64)ids[i] >= k && first_test == ~0ULL) first_test = want_total;
            CHECK(p.src_off[i] == seq_off[(size_t)ids[i]] && p.dst_off[i] == want_total, "%s: sequence %zu planned from %lu to %lu", what, i, (unsigned long)p.src_off[i], (unsigned long)p.dst_off[i]);
            want_total += seq_off[(size_t)ids[i] + 1] - seq_off[(size_t)ids[i]];
        }
        CHECK(p.nbases() == want_total, "%s: %lu bases planned, %lu wanted", what, (unsigned long)p.nbases(), (unsigned long)want_total);
        const u64 nwords = (want_total + 31) / 32, w_from = first_test == ~0ULL ? nwords : first_test / 32;
        auto expect_word = [&](u64 w) {
            u64 e = 0;
            for (u64 g = 32 * w; g < 32 * w + 32 && g < want_total; ++g) {
                const size_t i = (size_t)(std::upper_bound(p.dst_off.begin(), p.dst_off.end(), g) - p.dst_off.begin()) - 1;
                e |= (u64)base(p.src_off[i] + (g - p.dst_off[i])) << (2 * (g & 31));
            }
            return e;
        };
        u64 n_checked = 0;
        for (u64 w = w_from ? w_from - 1 : 0; w < nwords; ++w, ++n_checked) {
            const u64 got = vgather::gather_word(w, p.dst_off.data(), p.src_off.data(), p.src_vol.data(), p.n(), &wp);
            const u64 expect = expect_word(w);
            CHECK(got == expect, "%s: word %lu of %lu is %016lx, the merge has %016lx", what, (unsigned long)w, (unsigned long)nwords, (unsigned long)got, (unsigned long)expect);
        }
        for (u64 w = 0; w + 1 < w_from; w += 1 + w_from / 257) CHECK(vgather::gather_word(w, p.dst_off.data(), p.src_off.data(), p.src_vol.data(), p.n(), &wp) == 0, "%s: filler word %lu is not zero", what, (unsigned long)w);
        printf("%s: %lu sequences, %lu bases, %lu destination words from word %lu compared\n", what, (unsigned long)p.n(), (unsigned long)want_total, (unsigned long)n_checked, (unsigned long)(w_from ? w_from - 1 : 0));
    };
    std::vector<i64> ids;
    for (u64 i = k; i < nseq; ++i) ids.push_back((i64)i);
    run(ids, "the test reads alone");
    ids.clear();
    for (u64 i = 0; i < nseq; ++i) ids.push_back((i64)i);
    run(ids, "every sequence");
    CHECK((nbases + 31) / 32 > (1ULL << 26), "the destination does not pass word 2^26");
    ids.clear();
    for (u64 i = 1; i < nseq; ++i) if (i < k || ((i - k) & 1) == 0) ids.push_back((i64)i);
    run(ids, "all but the first filler, every other test read");
    printf("first_base=%lu last_base=%lu fillers=%lu\n", (unsigned long)first, (unsigned long)(nbases - 1), (unsigned long)k);
}

int main(int argc, char** argv)
{
    if (argc > 1) {
        check_high(argv[1]);
        if (g_fail) { printf("check_vol_gather: %ld checks FAILED\n", g_fail); return 1; }
        printf("check_vol_gather: ok\n");
        return 0;
    }
    check_pairs();
    check_edges();
    check_refusals();
    check_swap();
    check_chunks();
    if (g_fail) { printf("check_vol_gather: %ld checks FAILED\n", g_fail); return 1; }
    printf("check_vol_gather: ok\n");
    return 0;
}
