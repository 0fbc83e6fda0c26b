// check_ckpool.cpp - the host's carve of the checkpoint pool against the kernels' indexing (necat_amd/csrc/ext_ckpool.h), on the CPU.
// The kernels address the pool through rc_at<NW>; the host sizes it from CkLayout, puts the deltas behind the checkpoints (ck_delta_offset) and sends a list
// through it in chunks (ck_chunk, ck_for_chunks, the pieces of the piped round).  A disagreement between the two is a store outside the pool, so for every
// geometry and chunk size this program walks the whole index domain: in bounds, injective, the deltas exactly behind the checkpoints; the chunk loop covers a list once.
//   usage: check_ckpool            exit status 0 and "check_ckpool: ok" when everything holds
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <thread>
#include <vector>
#include "ext_ckpool.h"
using namespace necat;

static std::atomic<int> g_fail{0};
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// k_rcwalk3 keeps a block's base address instead of calling rc_at per access; this is its formula (ext_rcwalk3.h, `ck_blk` / `hc_blk`) transcribed by hand.
// (A transcription, not the kernel's own line: the kernel is HIP-only and cannot be compiled in here, so this check shows that the formula as written today
// equals rc_at - it cannot notice the kernel's line drifting later; whoever edits that line edits this copy with it.)
template <int NW> static size_t rcwalk3_block_base(u64 x, int slots)
{
    constexpr u64 GI = RcLay<NW>::kGI;
    return (size_t)((x / GI) * (u64)(slots * NW * GI) + x % GI);
}

// one region (checkpoints: elem = 16 bytes, or deltas: elem = 8) of a pool of `chunk` work indices: every index below the region's size, no index twice
template <int NW> static void check_region(const char* what, u32 chunk, int slots, size_t elem, size_t per, std::vector<u64>& seen)
{
    const size_t size = (size_t)chunk * per;              // bytes the host gives the region
    CHECK(per == (size_t)slots * NW * elem, "%s", what);
    seen.assign((size / elem + 63) / 64, 0);
    size_t top = 0, twice = 0, n = 0;
    for (u64 x = 0; x < chunk; ++x) {
        CHECK(rcwalk3_block_base<NW>(x, slots) == rc_at<NW>(x, slots, 0, 0), "%s x %llu", what, (unsigned long long)x);
        for (int s = 0; s < slots; ++s)
            for (int w = 0; w < NW; ++w, ++n) {
                const size_t i = rc_at<NW>(x, slots, (size_t)s, (size_t)w);
                if (i > top) top = i;
                if (i * elem >= size) continue;           // (reported below through `top`)
                u64& word = seen[i >> 6];
                twice += (word >> (i & 63)) & 1;
                word |= 1ULL << (i & 63);
            }
    }
    CHECK(n == 0 || top * elem < size, "%s chunk %u: largest index %zu x %zu bytes against %zu", what, chunk, top, elem, size);
    CHECK(twice == 0, "%s chunk %u: %zu indices twice", what, chunk, twice);
}

template <class Lay, int NW> static void check_layout(const char* name)
{
    std::vector<u64> seen;
    // chunk sizes: one group, three, what NECAT_ASM_RC_POOL_MB=256 gives the 2048-bp list A, and one whose byte offsets pass 2^32 in the larger geometries
    for (u32 chunk : {64u, 192u, 3264u, 65600u}) {
        check_region<NW>(name, chunk, Lay::kSlots, 16, Lay::kPerCk, seen);
        check_region<NW>(name, chunk, Lay::kSegs, 8, Lay::kPerHc, seen);
        // the deltas start where the checkpoints end, the pool ends where the deltas do
        CHECK(ck_delta_offset(chunk, Lay::kPerCk) == (size_t)chunk * Lay::kSlots * NW * 16, "%s", name);
        CHECK(ck_pool_bytes(chunk, Lay::kPerCk, Lay::kPerHc) == ck_delta_offset(chunk, Lay::kPerCk) + (size_t)chunk * Lay::kSegs * NW * 8, "%s", name);
        // (d) a list of `bound` work indices in steps of `chunk`
        for (u32 bound : {1u, 63u, 64u, 65u, chunk - 1, chunk, chunk + 1, 3 * chunk + 17})
            for (CkCount count : {CK_PADDED, CK_ITEMS}) {
                const u32 want = count == CK_ITEMS ? bound : (bound + 63) / 64 * 64;      // the items, or the padded work indices
                u32 next = 0, lasts = 0, turns = 0;
                const int rc = ck_for_chunks(bound, chunk, count, [&](const CkChunk& c) {
                    CHECK(c.lo == next && c.lo % 64 == 0 && c.cn > 0 && c.cn <= chunk, "%s bound %u chunk %u lo %u", name, bound, chunk, c.lo);
                    CHECK(c.hi <= (bound + 63) / 64 * 64 && c.hi - c.lo <= chunk, "%s bound %u chunk %u hi %u", name, bound, chunk, c.hi);
                    CHECK(c.cn == (count == CK_ITEMS ? (c.hi < bound ? c.hi : bound) - c.lo : c.hi - c.lo), "%s bound %u chunk %u cn %u", name, bound, chunk, c.cn);
                    CHECK(!lasts, "%s bound %u chunk %u: a chunk after the last", name, bound, chunk);
                    lasts += c.last; ++turns;
                    next = c.lo + c.cn;
                    if (!c.last) CHECK(c.cn == chunk && c.hi == c.lo + chunk, "%s bound %u chunk %u: a short chunk in the middle", name, bound, chunk);
                    return 0;
                });
                CHECK(rc == 0 && next == want && lasts == 1 && turns == (bound + chunk - 1) / chunk, "%s bound %u chunk %u: covered %u of %u, %u last", name, bound, chunk, next, want, lasts);
            }
        CHECK(ck_for_chunks(3 * chunk, chunk, CK_PADDED, [&](const CkChunk& c) { return c.lo ? 7 : 0; }) == 7, "%s: the body's error is handed on", name);
    }
    // pool sizes from a budget: whole groups, at least one, never more than the list
    CHECK(ck_chunk(0, Lay::kPerCk, Lay::kPerHc, 5) == 64 && ck_chunk(~(size_t)0, Lay::kPerCk, Lay::kPerHc, 5) == 320 && ck_chunk(~(size_t)0, Lay::kPerCk, Lay::kPerHc, 0) == 64, "%s", name);
    CHECK(ck_chunk(200 * (Lay::kPerCk + Lay::kPerHc), Lay::kPerCk, Lay::kPerHc, 1000) == 192, "%s", name);
    // (e) the piped round: the pool holds the whole list, piece i's checkpoints and deltas at their own place in it
    if (Lay::kSegs) for (u32 groups : {1u, 7u, 64u, 1000u})
        for (u32 pieces = 2; pieces <= 8; ++pieces) {
            const u32 bound = groups * 64 - 5, step = ck_piece_step(groups, pieces), pool = ck_chunk(~(size_t)0, Lay::kPerCk, Lay::kPerHc, groups);
            size_t end_ck = 0, end_hc = 0; u32 turns = 0;
            ck_for_chunks(bound, step, CK_PADDED, [&](const CkChunk& c) {
                const size_t at_ck = ck_piece_ck(c.lo, Lay::kPerCk), at_hc = ck_piece_hc(c.lo, Lay::kPerHc);
                CHECK(at_ck >= end_ck && at_hc >= end_hc, "%s %u groups in %u pieces: piece at %u overlaps the one before", name, groups, pieces, c.lo);
                end_ck = at_ck + rc_at<NW>(c.cn - 1, Lay::kSlots, Lay::kSlots - 1, NW - 1) + 1;
                end_hc = at_hc + rc_at<NW>(c.cn - 1, Lay::kSegs, Lay::kSegs - 1, NW - 1) + 1;
                ++turns;
                return 0;
            });
            CHECK(step % 64 == 0 && turns <= pieces && pool == groups * 64, "%s %u groups in %u pieces of %u: %u turns", name, groups, pieces, step, turns);
            CHECK(end_ck * 16 <= ck_delta_offset(pool, Lay::kPerCk) && end_hc * 8 <= (size_t)pool * Lay::kPerHc, "%s %u groups in %u pieces: past the pool", name, groups, pieces);
        }
}

// the four block shapes of the library (words, columns: kWordsA x kColsA and kWordsB x kColsB of ext_kernels.h, kAsmWordsA x kAsmBlock of asm_coop.h and
// kAsmWords x kAsmCols of asm_kernels.h - stage_ck_round.inl asserts that its geometry bundles are these numbers) and list A without carries
typedef CkLayout<8, 512> LayA;
typedef CkLayout<13, 794> LayB;
typedef CkLayout<32, 2048> LayAsmA;
typedef CkLayout<44, 2791> LayAsmB;
typedef CkLayout<8, 512, false> LayA0;

int main()
{
    // (one thread per layout: the largest domain, 65 600 blocks of asm list B, is 5 x 10^8 checkpoints)
    std::thread th[] = {std::thread(check_layout<LayA, 8>, "list A"), std::thread(check_layout<LayB, 13>, "list B"), std::thread(check_layout<LayAsmA, 32>, "asm list A"),
                        std::thread(check_layout<LayAsmB, 44>, "asm list B"), std::thread(check_layout<LayA0, 8>, "list A, no carries")};
    for (std::thread& t : th) t.join();
    // (f) the bytes per block the library has always used
    CHECK(LayA::kPerCk + LayA::kPerHc == 5120, "list A");
    CHECK(LayA::kPerCk == (size_t)kRcCk16 * 8 * 16 && LayA::kPerHc == (size_t)kRcCk * 8 * 8, "list A: the kRcCk16 / kRcCk spelling");
    CHECK(LayA0::kPerCk == (size_t)kRcCk * 8 * 16 && LayA0::kSlots == 16 && LayA0::kPerHc == 0, "list A, no carries");
    CHECK(LayB::kPerCk + LayB::kPerHc == 13000, "list B");
    CHECK(LayAsmA::kPerCk + LayAsmA::kPerHc == 81920, "asm list A");
    // asm list B: RcGeom<kAsmCols = 2791> is 175 checkpoint slots and 88 delta segments, kAsmWords = 44 words: 175 x 44 x 16 + 88 x 44 x 8 bytes
    // (stage_asm_align.inl's kCkB + kHcB before the layout moved here)
    CHECK(RcGeom<2791>::kCk == 175 && RcGeom<2791>::kSeg == 88 && LayAsmB::kPerCk == 123200 && LayAsmB::kPerHc == 30976, "asm list B");
    if (g_fail) { printf("check_ckpool: %d checks failed\n", (int)g_fail); return 1; }
    printf("check_ckpool: ok\n");
    return 0;
}
