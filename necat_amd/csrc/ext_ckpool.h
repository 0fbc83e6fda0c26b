// ext_ckpool.h - the checkpoint pool of the checkpoint-pass round (ext_rcwalk.h): where a checkpoint / a delta word of a block lives, how many bytes a block
// takes, and how a list goes through a pool of bounded size.  THE definition of the layout: the kernels index the pool through rc_at, the host (stage_ck_round.inl)
// sizes, carves and chunks it through CkLayout and the ck_* functions below, and tests/host_core/check_ckpool.cpp holds the two against each other on the CPU
// (plain C++: g++ compiles this file on its own).
#pragma once
#include "dev_common.h"

namespace necat {

constexpr int kRcSeg = 32;                       // columns per segment = per checkpoint
constexpr int kRcCk = kOcaBlockSize / kRcSeg;    // checkpoint slots per block (the last one is never read)
constexpr int kRcCk16 = kOcaBlockSize / 16;      // .. of the CARRY variant

// ---- where a checkpoint / a delta word lives.  Slot `slot` (of `slots` per block), word w of block x (work index minus the launch's `lo`):
// the blocks whose word-w lanes store in ONE instruction of the checkpoint pass - the 8 blocks of a list-A wave, the 4 of a list-B wave -
// sit side by side, so that instruction writes one 128- (64-) byte line instead of 16 bytes in 8 (4) lines 4 KB apart: 5 - 7 % of the pass
// (tools/ck_microbench.hip).  The walk reads a block's two words of a slot as two 16-byte pieces either way.
template <int NW> struct RcLay { static constexpr int kGI = NW == 8 ? 8 : NW == 13 ? 4 : 1; };       // blocks per group (the 2048-bp geometries: one block per wave)
template <int NW>
NECAT_D size_t rc_at(u64 x, int slots, size_t slot, size_t w)
{
    constexpr u64 GI = RcLay<NW>::kGI;
    return (size_t)((((x / GI) * (u64)slots + slot) * NW + w) * GI + x % GI);
}
template <int NW> constexpr int kRcStride = NW * RcLay<NW>::kGI;          // elements between two slots' same word

// checkpoint / delta slots of a block of up to COLS columns
template <int COLS> struct RcGeom { static constexpr int kCk = (COLS + 15) / 16, kSeg = (COLS + 31) / 32; };

// ---- a geometry's share of the pool: checkpoints (16 bytes: a word's Pv, Mv) every 16 columns and one delta word (8 bytes) per 32 columns and word;
// CARRY = false (cross-check build, k_myers_ck<.., false> + k_rcwalk4): checkpoints every 32 columns, no deltas
template <int NW, int COLS, bool CARRY = true> struct CkLayout {
    static constexpr int kSlots = CARRY ? RcGeom<COLS>::kCk : RcGeom<COLS>::kSeg;      // checkpoint slots per block
    static constexpr int kSegs = CARRY ? RcGeom<COLS>::kSeg : 0;                       // delta segments per block
    static constexpr size_t kPerCk = (size_t)kSlots * NW * 16, kPerHc = (size_t)kSegs * NW * 8;      // bytes per work index
};

// work indices a pool of `budget` bytes holds at a time: whole groups of 64, at least one, no more than the list's `groups`
inline u32 ck_chunk(size_t budget, size_t per_ck, size_t per_hc, u32 groups)
{
    const size_t fit = (budget / (per_ck + per_hc)) & ~(size_t)63, all = (size_t)groups * 64, n = fit < all ? fit : all;
    return (u32)(n > 64 ? n : 64);
}
// a pool of `chunk` work indices: the checkpoints first, the deltas right behind them
inline size_t ck_pool_bytes(u32 chunk, size_t per_ck, size_t per_hc) { return (size_t)chunk * (per_ck + per_hc); }
inline size_t ck_delta_offset(u32 chunk, size_t per_ck) { return (size_t)chunk * per_ck; }
// a piece of the piped round keeps its place in a pool that holds the whole list: elements in front of work index lo (a multiple of 64)
inline size_t ck_piece_ck(u32 lo, size_t per_ck) { return (size_t)lo * (per_ck / 16); }
inline size_t ck_piece_hc(u32 lo, size_t per_hc) { return (size_t)lo * (per_hc / 8); }
inline u32 ck_piece_step(u32 groups, u32 pieces) { return (u32)(((((u64)groups * 64 + pieces - 1) / pieces) + 63) & ~63ULL); }      // work indices per piece: whole groups

// one launch's share [lo, hi) of the work indices [0, bound); cn: what the grids are sized by -
//   CK_PADDED  hi - lo, the padded work indices (a two-ended list A: `bound` is an upper bound, the kernels read the exact size)
//   CK_ITEMS   min(hi, bound) - lo, the items (a plain list of exactly `bound` items: list B, the hook)
enum CkCount { CK_PADDED, CK_ITEMS };
struct CkChunk { u32 lo, hi, cn; bool last; };
inline CkChunk ck_chunk_at(u32 lo, u32 step, u32 bound, CkCount count)
{
    const u64 pad = ((u64)bound + 63) / 64 * 64, end = (u64)lo + step;
    CkChunk c; c.lo = lo; c.hi = (u32)(end < pad ? end : pad);
    c.cn = (count == CK_ITEMS && bound < c.hi ? bound : c.hi) - lo;
    c.last = end >= bound;
    return c;
}
// body(chunk) for every chunk of [0, bound) in steps of `step` work indices (a multiple of 64); stops at the first non-zero return and hands it on
template <class F> inline int ck_for_chunks(u32 bound, u32 step, CkCount count, F&& body)
{
    for (u32 lo = 0; lo < bound; lo += step) if (int rc = body(ck_chunk_at(lo, step, bound, count))) return rc;
    return 0;
}

}  // namespace necat
