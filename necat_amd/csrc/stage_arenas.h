// stage_arenas.h - the batch stages' device arenas: for each allocation that holds several arrays, ONE struct that takes every slot once, in the order and with
// the element type and count that size it (arena_layout.h).  The stage binds the struct to its DevBuf (runtime.h: ArenaView).  No HIP in this header: the record
// types come from the *_core.h headers, and tests/host_core/check_dev_arena.cpp checks every struct at the smallest shapes its stage sees.
#pragma once
#include "arena_layout.h"
#include "asm_ends_core.h"
#include "cns_dev_core.h"
#include "ctg_dev_core.h"
#include "ctg_seed_core.h"

namespace necat {

// necat_ctx::cns_dev for one chunk of the consensus proper (stage_cns_consensus.inl): nt templates with NO overlaps (ops_bytes of packed columns), T tags,
// P positions and S segment slots.
struct CnsChunkArena {
    ArenaLayout lay;
    Span<cns_dev::DevTmpl> tm; Span<cns_dev::DevOvl> ov; Span<double> w; Span<u8> ops; Span<u64> key, key2; Span<u32> cnt, off, cur; Span<i32> cov;
    Span<u32> node_of_tag; Span<double> l_w, l_e; Span<i32> l_pred; Span<u32> n_lfirst, n_nlink; Span<i32> n_pos; Span<u32> n_dc; Span<double> n_score, n_err; Span<i32> n_best;
    Span<u32> t_nodes, flags, seg_n; Span<cns_dev::Seg> seg; Span<u8> out;
    CnsChunkArena(size_t nt, size_t NO, size_t ops_bytes, size_t T, size_t P, size_t S)
    {
        tm = lay.take<cns_dev::DevTmpl>(nt); ov = lay.take<cns_dev::DevOvl>(NO); w = lay.take<double>(NO); ops = lay.take<u8>(ops_bytes + 8);
        key = lay.take<u64>(T); key2 = lay.take<u64>(T); cnt = lay.take<u32>(P + 1); off = lay.take<u32>(P + 1); cur = lay.take<u32>(P + 1); cov = lay.take<i32>(P + 1);
        node_of_tag = lay.take<u32>(T); l_w = lay.take<double>(T); l_e = lay.take<double>(T); l_pred = lay.take<i32>(T); n_lfirst = lay.take<u32>(T); n_nlink = lay.take<u32>(T);
        n_pos = lay.take<i32>(T); n_dc = lay.take<u32>(T); n_score = lay.take<double>(T); n_err = lay.take<double>(T); n_best = lay.take<i32>(T);
        t_nodes = lay.take<u32>(nt); flags = lay.take<u32>(nt); seg_n = lay.take<u32>(nt); seg = lay.take<cns_dev::Seg>(S); out = lay.take<u8>(T + 8);
    }
};

// necat_ctx::cns_dev for one segment of contig polishing's consensus (stage_ctg_consensus.inl): its packed columns, then what its largest range needs - NO overlaps,
// T tag slots, P positions.  cnt / off / cur have the bucket of dropped tags and the total behind the positions (P + 2), the per-position arrays of the links one
// entry to spare (P + 1).
struct CtgRangeArena {
    ArenaLayout lay;
    Span<u8> ops; Span<ctg_dev::RangeOvl> ov; Span<cns_dev::DevTmpl> tm; Span<u64> key, key2; Span<u32> cnt, off, cur; Span<i32> cov; Span<u32> pos_node; Span<u64> tile_cnt, tile_base;
    Span<u32> n_pos, n_db, n_link0, l_pred, l_tag0, big;
    CtgRangeArena(size_t ops_bytes, size_t NO, size_t T, size_t P)
    {
        const size_t n_tiles = (P + ctg_dev::kTilePositions - 1) / ctg_dev::kTilePositions;
        ops = lay.take<u8>(ops_bytes); ov = lay.take<ctg_dev::RangeOvl>(NO); tm = lay.take<cns_dev::DevTmpl>(1); key = lay.take<u64>(T); key2 = lay.take<u64>(T);
        cnt = lay.take<u32>(P + 2); off = lay.take<u32>(P + 2); cur = lay.take<u32>(P + 2); cov = lay.take<i32>(P + 1); pos_node = lay.take<u32>(P + 1);
        tile_cnt = lay.take<u64>(n_tiles + 1); tile_base = lay.take<u64>(n_tiles + 1);
        n_pos = lay.take<u32>(T); n_db = lay.take<u32>(T); n_link0 = lay.take<u32>(T); l_pred = lay.take<u32>(T); l_tag0 = lay.take<u32>(T);
        big = lay.take<u32>(T / ctg_dev::kBigBucket + 2);
    }
};

// ctg_seed_buf[CSB_JOBS] (stage_ctg_seed.inl) for a run of R jobs whose read tables hold tab_words words: the jobs, their candidates, the selection of a chunk, the
// two error counts (jobs whose seeds were not the counted ones; pairs of surviving matches that share a start), the tables.  Everything from `out` on is cleared per run.
struct CtgSeedRunArena {
    ArenaLayout lay;
    Span<ctg_seed::JobDev> jobs; Span<ctg_seed::DCan> out; Span<u32> sel, bad, tab;
    CtgSeedRunArena(size_t R, size_t tab_words) { jobs = lay.take<ctg_seed::JobDev>(R); out = lay.take<ctg_seed::DCan>(R); sel = lay.take<u32>(R); bad = lay.take<u32>(2); tab = lay.take<u32>(tab_words); }
};

// ctg_seed_buf[CSB_POOL] for a chunk of n seeds: the seeds before and after their sort, the matches before and after theirs, the chain's four arrays
struct CtgSeedPoolArena {
    ArenaLayout lay;
    Span<ctg_seed::SeedRec> tmp, seeds; Span<ctg_seed::DMem> tmp_mems, mems; Span<i32> chain;
    explicit CtgSeedPoolArena(size_t n) { tmp = lay.take<ctg_seed::SeedRec>(n); seeds = lay.take<ctg_seed::SeedRec>(n); tmp_mems = lay.take<ctg_seed::DMem>(n); mems = lay.take<ctg_seed::DMem>(n); chain = lay.take<i32>(n * 4); }
};

// scratch[SC_ASM_OUT] for the end extension of na anchors (stage_asm_ends.inl): plans, records, flags, and the counters (aends::C_*) in a slot of their own
struct AsmEndsArena {
    static constexpr size_t kCounters = 64;
    ArenaLayout lay;
    Span<aends::Plan> plans; Span<necat_m4> recs; Span<u8> kept; Span<u32> counts;
    explicit AsmEndsArena(size_t na) { plans = lay.take<aends::Plan>(na); recs = lay.take<necat_m4>(na); kept = lay.take<u8>(na); counts = lay.take<u32>(kCounters); }
    static_assert(aends::C_COUNT <= kCounters, "the counters' slot holds them all");
};

}  // namespace necat
