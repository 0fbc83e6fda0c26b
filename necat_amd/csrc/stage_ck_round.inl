// stage_ck_round.inl - the launches of the checkpoint-pass round (ext_rcwalk.h): an SHW pass that leaves checkpoints and deltas in a pool, the walk that recomputes
// its cells from them, chunk by chunk of what the pool holds, then one finishing k_traceback over the whole list.  Every alignment of the product goes through this
// sequence - the extension rounds' two lists (stage_extend.inl), the 2048-bp aligner's two (stage_asm_align.inl), the cross-check build's no-carry round and its
// block-by-block hook - and they all size, carve and chunk the pool through ext_ckpool.h and launch through the wrappers here.
// Included by necat_hip.hip in front of its extern "C" block (templates), after the host helpers it uses.

namespace {

// ---- one bundle per block shape: words per block, target words, columns, ops per block, lanes per block of the pass, the block size the finishing kernel plans with
template <int NW_, int TW_, int COLS_, int MAXOPS_, int G_, int BLOCK_ = kOcaBlockSize> struct CkGeom {
    static constexpr int NW = NW_, TW = TW_, COLS = COLS_, MAXOPS = MAXOPS_, G = G_, BLOCK = BLOCK_;
    using Lay = CkLayout<NW, COLS>;
};
using GeomA = CkGeom<kWordsA, kTWordsA, kColsA, kOpsA, 8>;                                    // list A: blocks up to 512 x 512
using GeomB = CkGeom<kWordsB, kTWordsB, kColsB, kOpsB, 16>;                                   // list B: the longer last blocks
using GeomAsmA = CkGeom<kAsmWordsA, kAsmTWordsA, kAsmBlock, kAsmOpsA, 32, kAsmBlock>;         // the 2048-bp aligner's list A
using GeomAsmB = CkGeom<kAsmWords, kAsmTWords, kAsmCols, kAsmMaxOps, 64, kAsmBlock>;          // .. and its list B: a wave per block
using LayA0 = CkLayout<kWordsA, kColsA, false>;                                               // list A without carries (cross-check build)
// (the shapes tests/host_core/check_ckpool.cpp walks through)
static_assert(kWordsA == 8 && kColsA == 512 && kWordsB == 13 && kColsB == 794 && kAsmWordsA == 32 && kAsmBlock == 2048 && kAsmWords == 44 && kAsmCols == 2791, "check_ckpool.cpp's geometries");

// a block list as the round's kernels take it (d_n / cap: ListView - a two-ended list A reads its exact size on the device; a plain list has d_n = nullptr, cap = 0)
struct CkList { const BlockItem* items; u32 bound; const u32* d_n; u32 cap; const u64* frag; BlockResult* res; u8* ops; WalkOut* wout; };
// a carved pool: checkpoints, deltas, the work indices it holds
struct CkPool { ulonglong2* ck; u64* hc; u32 chunk; };
// what every launch of a round shares
struct CkEnv { double error; unsigned long long* stats; ExtTask* tasks; int keep_cols, tail_match_len; int* d_err; };

// the pool of `groups` x 64 work indices inside `budget` bytes: (re)allocated, checkpoints first, deltas behind them
int ck_pool_carve(necat_ctx* ctx, DevBuf& b, size_t per_ck, size_t per_hc, size_t budget, u32 groups, CkPool& p)
{
    p.chunk = ck_chunk(budget, per_ck, per_hc, groups);
    if (int rc = buf_ensure(ctx, b, ck_pool_bytes(p.chunk, per_ck, per_hc))) return rc;
    p.ck = (ulonglong2*)b.p; p.hc = (u64*)((char*)b.p + ck_delta_offset(p.chunk, per_ck));
    return NECAT_OK;
}
template <class Lay> int ck_pool_carve(necat_ctx* ctx, DevBuf& b, size_t budget, u32 groups, CkPool& p) { return ck_pool_carve(ctx, b, Lay::kPerCk, Lay::kPerHc, budget, groups, p); }

// workgroups of one wave for cn blocks: `per_wave` blocks share a wave (ck_waves), or a block takes G lanes of it (ck_grid)
constexpr unsigned ck_waves(u32 cn, u32 per_wave) { return (cn + per_wave - 1) / per_wave; }
template <int G> constexpr unsigned ck_grid(u32 cn) { return ck_waves(cn, 64 / G); }

// ---- the pass.  List A's own: full blocks, and with flag bit 27 the ragged ones too; bit 22: the fragments cut by the pass itself (q_bases / t_bases)
template <class Geo>
void launch_ck(const CkList& l, const CkPool& p, const CkChunk& k, hipStream_t s, const CkEnv& e, u32 flags, const u64* q_bases, const u64* t_bases)
{
    hipLaunchKernelGGL((k_myers_ck<Geo::NW, Geo::TW, true>), dim3(ck_grid<Geo::G>(k.cn)), dim3(64), knob().ck_lds, s, l.items, l.d_n, l.cap, l.frag, p.ck, p.hc, e.error, l.res, e.stats,
                       knob().rc_maxdist, k.lo, k.hi, flags, q_bases, t_bases);
}
// the general pass (any block; G: lanes per block) and its fast form for blocks of at most 16 words
template <class Geo, int G = Geo::G>
void launch_ckg(const CkList& l, const CkPool& p, const CkChunk& k, hipStream_t s, const CkEnv& e, u32 epoch)
{
    hipLaunchKernelGGL((k_myers_ckg<Geo::NW, Geo::TW, Geo::COLS, G>), dim3(ck_grid<G>(k.cn)), dim3(64), 0, s, l.items, l.bound, l.d_n, l.cap, l.frag, p.ck, p.hc, e.error, l.res, e.stats, epoch, k.lo, k.hi);
}
template <class Geo, int G = Geo::G>
void launch_ckf(const CkList& l, const CkPool& p, const CkChunk& k, hipStream_t s, const CkEnv& e, u32 epoch)
{
    hipLaunchKernelGGL((k_myers_ckf<Geo::NW, Geo::TW, Geo::COLS, G>), dim3(ck_grid<G>(k.cn)), dim3(64), 0, s, l.items, l.bound, l.d_n, l.cap, l.frag, p.ck, p.hc, e.error, l.res, e.stats,
                       epoch | (knob().ckr_fast ? 0u : 1u << 28), k.lo, k.hi);
}

// ---- the recompute walk of a chunk (launch_rcwalk2 until the launches moved here): one workgroup per 64 blocks (two waves: k_rcwalk3; four: k_rcwalk2w) or one
// wave per 16 (k_rcwalk2)
template <class Geo>
void launch_ck_walk(const CkList& l, const CkPool& p, const CkChunk& k, hipStream_t s, const CkEnv& e, u32 fl)
{
    constexpr int NW = Geo::NW, TW = Geo::TW, COLS = Geo::COLS, MAXOPS = Geo::MAXOPS;
    const u32 pr = ((NW == kWordsA ? (knob().rc_prio & 1u) : NW == kWordsB ? (knob().rc_prio & 4u) : 0u) ? 8u : 0u) | ((NW == kWordsA ? (knob().rc_prio & 8u) : NW == kWordsB ? (knob().rc_prio & 16u) : 0u) ? 16u : 0u);
    auto go = [&](auto kern, unsigned blocks, unsigned threads, auto... opts) {          // `blocks` blocks per workgroup of `threads`
        hipLaunchKernelGGL(kern, dim3((k.cn + blocks - 1) / blocks), dim3(threads), 0, s, l.items, l.bound, l.d_n, l.cap, l.frag, (const ulonglong2*)p.ck, (const u64*)p.hc, (const BlockResult*)l.res,
                           (const ExtTask*)e.tasks, e.keep_cols, e.tail_match_len, l.ops, l.wout, e.stats, e.d_err, fl, k.lo, k.hi, opts...);
    };
    // (k_rcwalk3's walking wave alone at raised priority where k_rcwalk2w raises every wave: 39.2 against 39.5 ms per step, tools/r05/run5.sh)
    if (knob().rc_ww == 1 && NW == kWordsA && k.cn >= knob().rc3_min) {
        if (knob().rc3_band == 16) go(k_rcwalk3<NW, TW, COLS, MAXOPS, 16>, 64, 128, (pr & 8u) ? 16u : pr);
        else go(k_rcwalk3<NW, TW, COLS, MAXOPS, 32>, 64, 128, (pr & 8u) ? 16u : pr);
    }
    else if (knob().rc_ww >= 2 && knob().rc3_band == 16) go(k_rcwalk3<NW, TW, COLS, MAXOPS, 16>, 64, 128, pr);
    else if (knob().rc_ww >= 2) go(k_rcwalk3<NW, TW, COLS, MAXOPS, 32>, 64, 128, pr);
    else if (knob().rc_ww) go(k_rcwalk2w<NW, TW, COLS, MAXOPS>, 64, 256, knob().rc_prefetch | knob().rc_dbg | pr);
#if NECAT_XCHECK
    else go(k_rcwalk2<NW, TW, COLS, MAXOPS>, 16, 64);
#endif
    // (NECAT_RC_WW=0 in the product build: necat_ctx_create refuses it - read_knobs)
}

// ---- the finishing launch over the whole list: the walked blocks' results joined to their tasks, the successors appended to `next`
template <class Geo>
void launch_ck_finish(const CkList& l, hipStream_t s, const char* slabs, size_t slab_bytes, const CkEnv& e, const ExtLists& next, u32 fl)
{
    hipLaunchKernelGGL((k_traceback<Geo::NW, Geo::TW, Geo::COLS, Geo::MAXOPS, false, 5, Geo::BLOCK, false, 4>), dim3(((l.bound + 63) / 64 + 3) / 4), dim3(256), 0, s, l.items, l.bound, l.d_n, l.cap,
                       l.frag, slabs, slab_bytes, (const BlockResult*)l.res, l.ops, e.tasks, e.tail_match_len, (i32*)nullptr, e.d_err, next, fl, 0u, (const WalkOut*)l.wout);
}

}  // namespace
