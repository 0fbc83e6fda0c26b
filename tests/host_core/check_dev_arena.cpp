// check_dev_arena.cpp - the layout half of the batch stages' device arena (necat_amd/csrc/arena_layout.h), on the CPU: slots of mixed element sizes and of
// counts 0, 1, 63, 64, 65 taken in order, and one sequence whose total passes 2^32 bytes, against the rules the stages rely on - every offset a multiple of
// 256, offsets ascending in take order, no slot reaching into the next, the last one ending inside bytes(), take(0) leaving the cursor, bytes() the sum of
// the rounded sizes.  The expected offsets are recomputed here with a division, not with the header's mask.  Then the stages' own arena structs
// (necat_amd/csrc/stage_arenas.h) at the smallest shapes the stages see - one template with one overlap of one column, one range of one position, one job with
// zero seeds, one anchor - and at a larger odd shape: the same rules, the slot order and counts the stage's kernels and clears rely on, and a total equal to the
// byte expressions the stages carved with before the structs existed.
//
//   usage: check_dev_arena        exit status 0 and "check_dev_arena: ok" when everything holds
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "arena_layout.h"
#include "stage_arenas.h"

using namespace necat;

static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

struct B12 { uint32_t a, b, c; };
struct B16 { uint64_t a, b; };
struct B24 { uint64_t a, b, c; };
static_assert(sizeof(B12) == 12 && sizeof(B16) == 16 && sizeof(B24) == 24, "the element sizes this program is about");

struct Slot { size_t off, n, elem; };
static size_t rounded(size_t bytes) { return (bytes + 255) / 256 * 256; }

// takes n elements of T, checks the span against the cursor before and after, and notes the slot
template <class T>
static void take(ArenaLayout& L, size_t n, std::vector<Slot>& slots)
{
    const size_t before = L.bytes();
    const Span<T> s = L.take<T>(n);
    CHECK(s.off == before, "a slot of %zu x %zu bytes begins at %zu, the cursor was at %zu", n, sizeof(T), s.off, before);
    CHECK(s.n == n && s.bytes() == n * sizeof(T) && s.end() == s.off + n * sizeof(T), "a span of %zu x %zu bytes says n %zu, bytes %zu, end %zu", n, sizeof(T), s.n, s.bytes(), s.end());
    CHECK(L.bytes() == before + rounded(n * sizeof(T)), "taking %zu x %zu bytes moved the cursor from %zu to %zu", n, sizeof(T), before, L.bytes());
    if (n == 0) CHECK(L.bytes() == before, "take(0) moved the cursor from %zu to %zu", before, L.bytes());
    slots.push_back(Slot{s.off, n, sizeof(T)});
}

static void check_slots(const ArenaLayout& L, const std::vector<Slot>& slots, const char* what)
{
    size_t sum = 0;
    for (size_t i = 0; i < slots.size(); ++i) {
        const Slot& s = slots[i];
        CHECK(s.off % 256 == 0, "%s: slot %zu begins at %zu", what, i, s.off);
        CHECK(s.off == sum, "%s: slot %zu begins at %zu, the rounded sizes before it add up to %zu", what, i, s.off, sum);
        const size_t end = s.off + s.n * s.elem;
        if (i + 1 < slots.size()) {
            CHECK(slots[i + 1].off >= s.off, "%s: slot %zu begins before slot %zu", what, i + 1, i);
            CHECK(end <= slots[i + 1].off, "%s: slot %zu ends at %zu, slot %zu begins at %zu", what, i, end, i + 1, slots[i + 1].off);
        } else {
            CHECK(end <= L.bytes(), "%s: the last slot ends at %zu, the arena at %zu", what, end, L.bytes());
        }
        sum += rounded(s.n * s.elem);
    }
    CHECK(L.bytes() == sum, "%s: bytes() is %zu, the rounded sizes add up to %zu", what, L.bytes(), sum);
}

// every element size at one count, in two orders (ascending sizes, then the reverse)
static void one_count(size_t n)
{
    char what[64];
    snprintf(what, sizeof what, "count %zu", n);
    ArenaLayout L;
    std::vector<Slot> slots;
    take<uint8_t>(L, n, slots); take<uint16_t>(L, n, slots); take<uint32_t>(L, n, slots); take<uint64_t>(L, n, slots); take<B12>(L, n, slots); take<B16>(L, n, slots); take<B24>(L, n, slots);
    take<B24>(L, n, slots); take<B16>(L, n, slots); take<B12>(L, n, slots); take<uint64_t>(L, n, slots); take<uint32_t>(L, n, slots); take<uint16_t>(L, n, slots); take<uint8_t>(L, n, slots);
    check_slots(L, slots, what);
}

template <class T> static Slot slot_of(const Span<T>& s) { return Slot{s.off, s.n, sizeof(T)}; }

static void check_cns_chunk(size_t nt, size_t NO, size_t ops_bytes, size_t T, size_t P, size_t S)
{
    const CnsChunkArena a(nt, NO, ops_bytes, T, P, S);
    const std::vector<Slot> slots = {slot_of(a.tm), slot_of(a.ov), slot_of(a.w), slot_of(a.ops), slot_of(a.key), slot_of(a.key2), slot_of(a.cnt), slot_of(a.off), slot_of(a.cur), slot_of(a.cov),
                                     slot_of(a.node_of_tag), slot_of(a.l_w), slot_of(a.l_e), slot_of(a.l_pred), slot_of(a.n_lfirst), slot_of(a.n_nlink), slot_of(a.n_pos), slot_of(a.n_dc),
                                     slot_of(a.n_score), slot_of(a.n_err), slot_of(a.n_best), slot_of(a.t_nodes), slot_of(a.flags), slot_of(a.seg_n), slot_of(a.seg), slot_of(a.out)};
    check_slots(a.lay, slots, "CnsChunkArena");
    // k_cns_scan writes off[P] and cur[P] (P + 1 entries), the clears cover cnt and cov whole; the columns and the bases have 8 bytes to spare
    CHECK(a.cnt.n == P + 1 && a.off.n == P + 1 && a.cur.n == P + 1 && a.cov.n == P + 1, "CnsChunkArena: the per-position slots hold %zu, %zu, %zu, %zu for %zu positions", a.cnt.n, a.off.n, a.cur.n, a.cov.n, P);
    CHECK(a.tm.n == nt && a.flags.n == nt && a.seg_n.n == nt && a.ov.n == NO && a.w.n == NO && a.key.n == T && a.key2.n == T && a.seg.n == S, "CnsChunkArena: a slot's count");
    CHECK(a.ops.n == ops_bytes + 8 && a.out.n == T + 8, "CnsChunkArena: the byte slots");
    const size_t want = rounded(nt * sizeof(cns_dev::DevTmpl)) + rounded(NO * sizeof(cns_dev::DevOvl)) + rounded(NO * 8) + rounded(ops_bytes + 8) + 2 * rounded(T * 8) + 4 * rounded((P + 1) * 4) +
                        rounded(T * 4) + 2 * rounded(T * 8) + 5 * rounded(T * 4) + 2 * rounded(T * 8) + rounded(T * 4) + 3 * rounded(nt * 4) + rounded(S * sizeof(cns_dev::Seg)) + rounded(T + 8);
    CHECK(a.lay.bytes() == want, "CnsChunkArena: %zu bytes, the stage's expressions give %zu", a.lay.bytes(), want);
}

static void check_ctg_range(size_t ops_bytes, size_t NO, size_t T, size_t P)
{
    const CtgRangeArena a(ops_bytes, NO, T, P);
    const std::vector<Slot> slots = {slot_of(a.ops), slot_of(a.ov), slot_of(a.tm), slot_of(a.key), slot_of(a.key2), slot_of(a.cnt), slot_of(a.off), slot_of(a.cur), slot_of(a.cov), slot_of(a.pos_node),
                                     slot_of(a.tile_cnt), slot_of(a.tile_base), slot_of(a.n_pos), slot_of(a.n_db), slot_of(a.n_link0), slot_of(a.l_pred), slot_of(a.l_tag0), slot_of(a.big)};
    check_slots(a.lay, slots, "CtgRangeArena");
    const size_t n_tiles = (P + 255) / 256;
    // cnt is cleared over rs + 2 entries and off[rs] is read back (rs <= P); the tiles' total is read at tile_base[n_tiles]; big[0] is the list's length
    CHECK(a.cnt.n == P + 2 && a.off.n == P + 2 && a.cur.n == P + 2 && a.cov.n == P + 1 && a.pos_node.n == P + 1, "CtgRangeArena: the per-position slots for %zu positions", P);
    CHECK(a.tile_cnt.n == n_tiles + 1 && a.tile_base.n == n_tiles + 1 && a.tm.n == 1 && a.big.n == T / 1024 + 2 && a.ops.n == ops_bytes && a.ov.n == NO, "CtgRangeArena: a slot's count");
    const size_t want = rounded(ops_bytes) + rounded(NO * sizeof(ctg_dev::RangeOvl)) + rounded(sizeof(cns_dev::DevTmpl)) + 2 * rounded(T * 8) + 3 * rounded((P + 2) * 4) + 2 * rounded((P + 1) * 4) +
                        2 * rounded((n_tiles + 1) * 8) + 5 * rounded(T * 4) + rounded((T / 1024 + 2) * 4);
    CHECK(a.lay.bytes() == want, "CtgRangeArena: %zu bytes, the stage's expressions give %zu", a.lay.bytes(), want);
}

static void check_ctg_seed(size_t R, size_t tab_words, size_t seeds)
{
    const CtgSeedRunArena a(R, tab_words);
    const std::vector<Slot> slots = {slot_of(a.jobs), slot_of(a.out), slot_of(a.sel), slot_of(a.bad), slot_of(a.tab)};
    check_slots(a.lay, slots, "CtgSeedRunArena");
    // the run's one clear starts at `out` and runs to the end: it must leave the jobs alone and reach the selection, the error counts and the tables
    CHECK(a.jobs.off == 0 && a.jobs.end() <= a.out.off && a.out.off < a.sel.off && a.sel.off < a.bad.off && a.bad.off < a.tab.off && a.tab.end() <= a.lay.bytes(), "CtgSeedRunArena: what the clear from `out` covers");
    CHECK(a.jobs.n == R && a.out.n == R && a.sel.n == R && a.bad.n == 2 && a.tab.n == tab_words, "CtgSeedRunArena: a slot's count");
    const size_t want = rounded(R * sizeof(ctg_seed::JobDev)) + rounded(R * sizeof(ctg_seed::DCan)) + rounded(R * 4) + rounded(8) + rounded(tab_words * 4);
    CHECK(a.lay.bytes() == want, "CtgSeedRunArena: %zu bytes, the stage's expressions give %zu", a.lay.bytes(), want);
    const CtgSeedPoolArena p(seeds);
    const std::vector<Slot> pslots = {slot_of(p.tmp), slot_of(p.seeds), slot_of(p.tmp_mems), slot_of(p.mems), slot_of(p.chain)};
    check_slots(p.lay, pslots, "CtgSeedPoolArena");
    CHECK(p.tmp.n == seeds && p.seeds.n == seeds && p.tmp_mems.n == seeds && p.mems.n == seeds && p.chain.n == 4 * seeds, "CtgSeedPoolArena: a slot's count");
    const size_t pwant = 2 * rounded(seeds * sizeof(ctg_seed::SeedRec)) + 2 * rounded(seeds * sizeof(ctg_seed::DMem)) + rounded(seeds * 4 * 4);
    CHECK(p.lay.bytes() == pwant, "CtgSeedPoolArena: %zu bytes, the stage's expressions give %zu", p.lay.bytes(), pwant);
}

static void check_asm_ends(size_t na)
{
    const AsmEndsArena a(na);
    const std::vector<Slot> slots = {slot_of(a.plans), slot_of(a.recs), slot_of(a.kept), slot_of(a.counts)};
    check_slots(a.lay, slots, "AsmEndsArena");
    CHECK(a.plans.n == na && a.recs.n == na && a.kept.n == na && a.counts.n == 64 && a.counts.n >= (size_t)aends::C_COUNT, "AsmEndsArena: a slot's count");
    const size_t want = rounded(na * sizeof(aends::Plan)) + rounded(na * sizeof(necat_m4)) + rounded(na) + 256;
    CHECK(a.lay.bytes() == want, "AsmEndsArena: %zu bytes, the stage's expressions give %zu", a.lay.bytes(), want);
}

int main()
{
    check_cns_chunk(1, 1, 8, 1, 2, 1);               // one template of one base with one overlap of one column (8 bytes of packed columns)
    check_cns_chunk(7, 131, 4104, 60001, 9013, 77);
    check_ctg_range(16, 1, 1, 1);                    // one range of one position, one overlap of one column
    check_ctg_range(100008, 65, 70001, 257);         // (two tiles, a second entry in the list of big buckets)
    check_ctg_seed(1, 128, 0);                       // one job (the smallest table: 64 slots) with zero seeds
    check_ctg_seed(65, 3 * 128 + 2 * 4096, 12345);
    check_asm_ends(1);                               // one anchor
    check_asm_ends(4097);
    { ArenaLayout L; CHECK(L.bytes() == 0, "an empty layout has %zu bytes", L.bytes()); }
    for (size_t n : {0, 1, 63, 64, 65}) one_count(n);
    {   // the counts mixed, empty slots between full ones: an empty slot shares its offset with the next one and has no byte of its own
        ArenaLayout L;
        std::vector<Slot> slots;
        take<B24>(L, 65, slots); take<uint32_t>(L, 0, slots); take<uint8_t>(L, 1, slots); take<B12>(L, 0, slots); take<B12>(L, 0, slots); take<uint16_t>(L, 63, slots);
        take<uint64_t>(L, 64, slots); take<B16>(L, 65, slots); take<uint8_t>(L, 0, slots);
        check_slots(L, slots, "mixed counts");
        CHECK(slots[1].off == slots[2].off && slots[3].off == slots[5].off, "an empty slot does not share its offset with the next slot");
    }
    {   // past 2^32 bytes: offsets and the total are size_t, nothing wraps
        static_assert(sizeof(size_t) == 8, "a 64-bit host");
        ArenaLayout L;
        std::vector<Slot> slots;
        const size_t big = ((size_t)1 << 29) + 1;          // x 8 bytes: 4 GB and 8 bytes
        take<uint8_t>(L, 65, slots); take<uint64_t>(L, big, slots); take<B24>(L, 1, slots); take<uint32_t>(L, big, slots); take<B12>(L, 63, slots);
        check_slots(L, slots, "past 2^32");
        CHECK(slots[2].off == 256 + ((size_t)1 << 32) + 256, "the slot behind 4 GB + 8 bytes begins at %zu", slots[2].off);
        CHECK(L.bytes() > ((size_t)3 << 31), "the total of the big layout is %zu", L.bytes());
    }
    if (g_fail) { printf("check_dev_arena: %ld checks failed\n", g_fail); return 1; }
    printf("check_dev_arena: ok\n");
    return 0;
}
