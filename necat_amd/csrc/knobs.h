// knobs.h - the tuning / test knobs of the library: ONE table, one line per knob.  Until round 5 these were process-wide globals re-read from the environment whenever ANY
// context was created: two contexts made with different environments raced on them.  Now every context holds the values its creator's environment had (necat_ctx::knobs,
// read ONCE in necat_ctx_create - the library does not look at its host's environment while calls are running), and an entry point of the C ABI makes its context's knobs the
// current ones for the length of the call (KnobScope, thread-local: one host thread per context, as include/necat_hip.h asks).  knob() is the current set.  A knob is read on
// the CALLING thread only: the worker threads the library starts itself (all through host_threads.h: stage_refmap.inl, stage_cns.inl, stage_cns_consensus.inl, and cns::parallel_for - which is handed
// its thread count - wherever it is called) do not inherit the thread-local.
//
// The kinds of line (struct Knobs below, read_knobs / finish_knobs / necat_knob_get in necat_hip.hip and tests/test_knobs.py are all made from this list):
//   NUM(field, type, "NAME", default, min, max)   a number: strtoull(text, 10), clamped to [min, max], then cast to `type` (u32, int, size_t, ull)
//   INT(field, "NAME", default)                   a signed number: atoi(text)
//   SET(field, "NAME")                            "is it set at all" (KnobSet: .set, and .v = atoi(text) where the number then matters): NAME=0 is SET
//   STR(field, "NAME")                            text (std::string; unset = "")
// Rules that need another knob or are no min / max (rc_listb, rc_ragged, rc_maxdist, rc3_band, split_threads, rc_dbg, MB -> bytes) are in finish_knobs().
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>

#define NECAT_KNOBS(NUM, INT, SET, STR) \
    /* ---- index build */ \
    NUM(index_lds,         int,    "NECAT_INDEX_LDS",         1, 0, ~0ull)           /* LDS-slice index passes; 0: global-atomic bucket passes */ \
    NUM(split_threads,     ull,    "NECAT_SPLIT_THREADS",     512, 0, ~0ull)         /* 512, or 256 = until round 5 (nothing else): threads of a workgroup of the index build's split kernels (k_split_bases, k_split_recs, k_subpart), each on a 4096-record tile */ \
    INT(index_own_offsets,         "NECAT_INDEX_OWN_OFFSETS", 0)                     /* != 0: the offset list never takes over the partition arena (SC_PART) */ \
    INT(index_emit_big,            "NECAT_INDEX_EMIT_BIG",    -1)                    /* 1 / 0: tests force either instance of the emit kernel; -1 = by size */ \
    INT(index_dense_bases,         "NECAT_INDEX_DENSE_BASES", 0)                     /* != 0 (A/B, fallback): the unsharded LDS-slice build counts its slices first (k_slice_count, k_bucket_base, a host wait for the two sizes) and packs them without holes, as the sharded build does; 0: record-space bases, holes at the slices' ends */ \
    INT(no_lend,                   "NECAT_NO_LEND",          0)                     /* != 0: buf_ensure_lend never takes a donor's buffer (runtime.h) */ \
    /* ---- seeding */ \
    NUM(seed_budget,       ull,    "NECAT_SEED_BUDGET",       48ull << 20, 0, ~0ull) /* seeding scratch budget per chunk, in k-mer hits */ \
    NUM(seed_wave,         int,    "NECAT_SEED_WAVE",         1, 0, ~0ull)           /* wave-per-strand seed collection; 0: the lane-per-strand kernel */ \
    NUM(seed_kst,          int,    "NECAT_SEED_KST",          1, 0, ~0ull)           /* 0: k_seed_collect_wave looks the table up again instead of reading the words k_seed_hits kept (A/B tests) */ \
    INT(seed_debug,                "NECAT_SEED_DEBUG",        0)                     /* SeedParams::debug_phase: 1 = stop after seed collection (profiling only) */ \
    INT(chain_wave,                "NECAT_CHAIN_WAVE",        1)                     /* SeedParams::chain_wave: chain DP of an evaluation on all lanes of its wave, or (0) on lane 0 (tests compare the two) */ \
    SET(seed_clear_kernel,         "NECAT_SEED_CLEAR_KERNEL")                        /* A/B: the hash slots cleared by a launch of their own (k_seed_clear), as in round 3, instead of inside k_seed_eval */ \
    /* ---- extension: the batches of a call */ \
    NUM(batch_cap,         u32,    "NECAT_BATCH",             786432, 64, ~0ull)     /* candidates per extension batch */ \
    /* ext_overlap: a call of two or more batches runs them two at a time, side by side (two lanes: ExtLane, stage_extend.inl) - the other batch's kernels fill the drain / \
       ramp-up of every round's kernels and the ~ 15 latency-bound rounds a batch ends in.  0 = one batch after the other. \
       ext_overlap_pct: the next batch starts as soon as a lane is free; < 100: only when fewer than that per cent of the batch started last still have a block to align \
       (70: 293.7 against 277.5 ms per step at yeast size). \
       ext_overlap_min (0 = never): a call of ONE batch of at least this many candidates is cut in two for the same effect, ext_overlap_split per cent (the longest chains) in \
       the first.  E. coli size: 36.8 - 39.6 ms per step against 38.8 - 39.3 on one lane, depending on which of the process's streams the runtime has put on one hardware \
       queue (tools/r05/run19, run22, run24): not a reliable gain, so not the default - which also keeps the bench line's roofline (priced on its kernels' event durations) \
       free of launches that share the chip. */ \
    NUM(ext_overlap,       u32,    "NECAT_EXT_OVERLAP",       1, 0, ~0ull) \
    NUM(ext_overlap_min,   u32,    "NECAT_EXT_OVERLAP_MIN",   0, 0, ~0ull) \
    NUM(ext_overlap_pct,   u32,    "NECAT_EXT_OVERLAP_PCT",   100, 0, 100) \
    NUM(ext_overlap_split, u32,    "NECAT_EXT_OVERLAP_SPLIT", 20, 5, 95) \
    NUM(ext_overlap_order, u32,    "NECAT_EXT_ORDER",         1, 0, ~0ull)           /* 0: several batches take the candidates as they come instead of longest expected chain first (A/B) */ \
    NUM(ext_lanes,         u32,    "NECAT_EXT_LANES",         2, 1, kMaxExtLanes)    /* lanes a call of several batches runs its batches on side by side (stage_extend.inl; 1 = NECAT_EXT_OVERLAP=0) */ \
    INT(lane1_prio,                "NECAT_LANE1_PRIO",        1)                     /* stream priority of lanes 1 ..: 0 = normal, 1 = the device's lowest, 2 = highest (ext_lane, stage_extend.inl) */ \
    INT(serial,                    "NECAT_SERIAL",            0)                     /* != 0 (profiling): the four streams of the extension rounds are ONE stream (ext_streams) */ \
    INT(stream_prio,               "NECAT_STREAM_PRIO",       0)                     /* 1: the streams of list B and of the ragged / wide blocks at the device's highest priority; 2: list A's stream instead (ext_streams; with the stream graph of NECAT_STREAM_GRAPH=1 list A's stream is the context's own, made at that priority) */ \
    /* stream_graph: 1 (default) = a context's stream graph needs few of the runtime's hardware queues - list A's chain of lane 0 runs on the context's own stream (index build, seeding, \
       k_ext_init, the rounds, k_ext_result, k_m4_filter are one sequence per call), list B's streams are made in necat_ctx_create, in a fixed order, the stream of the un-merged ragged chain \
       only where the knobs select a path that launches on it (NECAT_RC_MERGE=0, NECAT_RC_PIPE, the cross-check build); 0 = the graph until then: five streams per context (four of them made \
       by the first extension call, whichever host thread gets there first), list A on a stream of its own.  listb_prio: the priority pool of lane 0's list-B streams under the new graph \
       (the runtime keeps a set of hardware queues per priority level: streams of another level never share a queue with any context's list-A chain) - 0 = normal, 1 = the device's lowest, \
       2 = highest (NECAT_STREAM_PRIO=1 overrides it).  listb_streams: 2 = small lists alternate between two streams (plan_b), 1 = one stream.  Four steps in flight on the runtime's \
       default of four queues, ms per step: graph 0 33.5; graph 1 with two list-B streams normal / lowest / highest 29.9 - 30.5 / 28.0 - 28.3 / 28.0 - 28.2, with one stream \
       28.8 - 29.0 / 28.4 - 29.6 / 28.3 - 28.7; one step at a time 36.0 - 36.1 / 36.1 - 36.4 / 35.9 - 36.1 / 36.0 - 36.3 with two streams, 36.5 - 36.9 with one \
       (profiles/stream_graph_notes.md) */ \
    NUM(stream_graph,      u32,    "NECAT_STREAM_GRAPH",      1, 0, 1) \
    INT(listb_prio,                "NECAT_LISTB_PRIO",        1) \
    NUM(listb_streams,     u32,    "NECAT_LISTB_STREAMS",     2, 1, 2) \
    /* ---- extension: which kernels a round's lists go through */ \
    NUM(coop_threshold,    u32,    "NECAT_COOP_THRESHOLD",    0xffffffffu, 0, ~0ull) /* lists with at most this many blocks use the cooperative DP kernel (k_myers_coop), longer ones the lane-per-block kernel (k_myers).  With the band store filter the cooperative kernel is the faster one at every size measured on MI355X (200 k blocks: 2.66 vs 2.80 ms; 50 k: 0.77 vs 1.38 ms), so the default is "always"; 0 selects the lane-per-block kernel (tests compare the two). */ \
    NUM(coop_filter,       int,    "NECAT_COOP_FILTER",       1, 0, ~0ull)           /* 0: the cooperative kernel stores every word (A/B tests) */ \
    NUM(single_pass,       u32,    "NECAT_SINGLE_PASS",       4096, 0, ~0ull)        /* lists up to this many blocks use the single-pass DP kernel (0 = never) */ \
    NUM(sort_b,            int,    "NECAT_SORT_B",            1, 0, ~0ull)           /* 0 disables the size sort of list B */ \
    NUM(fast,              int,    "NECAT_FAST",              1, 0, ~0ull)           /* 0: the list-A DP kernel never takes its full-block fast path (A/B measurements); 2: fast path without band stores (profiling only, results invalid) */ \
    NUM(fast16,            int,    "NECAT_FAST16",            0, 0, ~0ull)           /* 1: list A's big rounds through k_myers_a16 (16 full blocks per workgroup: SHW 8 lanes, NW 4 lanes per block); measured: no gain on the bench workload */ \
    NUM(band_pool,         size_t, "NECAT_BAND_POOL_MB",      16384, 0, ~0ull)       /* cap of one band-record pool (bytes in the field); a bigger list runs in several DP + walk launches (0 = no cap).  16 GB = 250 k list-A blocks per launch: as efficient as the whole list, and the first call does not allocate 50 - 100 GB */ \
    NUM(walk,              int,    "NECAT_WALK",              0, 0, ~0ull)           /* k_traceback's walk: 0 = the reference formulation (default until the restated walk wins), 1 = walk_block, 2 = walk_block without record prefetch (A/B measurements) */ \
    NUM(walk_wave,         u32,    "NECAT_WALK_WAVE",         12288, 0, ~0ull)       /* lists of at most this many blocks are walked by one WAVE per block through an LDS window (k_walk_wave, ext_tail.h); 0 = off */ \
    NUM(tail_fused,        u32,    "NECAT_TAIL_FUSED",        512, 0, ~0ull)         /* 512 = one workgroup per block at 2 per CU; 0 = off: lists of at most this many blocks run as ONE launch per round with the band in LDS (ext_tail.h) */ \
    NUM(dbg,               int,    "NECAT_DBG",               0, 0, ~0ull)           /* profiling-only variants of the lane-per-block DP kernel (1 = no band stores, 2 = no NW pass) */ \
    /* ---- extension: the checkpoint pass + recompute walk (ext_rcwalk.h, ext_rcwalk3.h) */ \
    NUM(rcwalk,            u32,    "NECAT_RCWALK",            512, 0, ~0ull)         /* 512 = every list the one-launch tail kernel does not take; 0 = off: list-A rounds of more than this many blocks run through k_myers_ck / k_myers_ckg + k_rcwalk2 (no NW pass, no band records, the walk recomputes its cells) */ \
    NUM(rc_pool,           size_t, "NECAT_RC_POOL_MB",        8192, 1, ~0ull)        /* 8192 = 1.6 M list-A blocks per launch; a 0.6 Gbp volume: 182 -> 174 ms per pass against 2048: cap of the checkpoint buffer of those rounds (bytes in the field); a longer list goes through it in several launches */ \
    NUM(rc_carry,          u32,    "NECAT_RC_CARRY",          1, 0, ~0ull)           /* the recompute walk on an exact two-word window (k_myers_ck<CARRY> keeps the words' horizontal deltas, k_rcwalk2); 0 = the 4-word band window (k_rcwalk4) */ \
    NUM(rc_listb,          u32,    "NECAT_RC_LISTB",          1, 0, ~0ull)           /* needs rc_carry: list B (blocks up to 794 x 794) through k_myers_ckg + k_rcwalk2 too; 0 = two-pass kernel + band pool + walk */ \
    NUM(rc_ragged,         u32,    "NECAT_RC_RAGGED",         1, 0, ~0ull)           /* needs rc_carry: the ragged blocks of those rounds through k_myers_ckg + k_rcwalk2 as well (0: two-pass kernel + lane walk on a stream of their own) */ \
    NUM(rc_merge,          u32,    "NECAT_RC_MERGE",          1, 0, ~0ull)           /* needs rc_ragged: the ragged list-A blocks of a big round through k_myers_ck's ragged fast path and the full blocks' walk launch; 0 = k_myers_ckg + a walk launch of their own on stream d */ \
    NUM(frag_fuse,         u32,    "NECAT_FRAG_FUSE",         1, 0, ~0ull)           /* needs the merged big-round path: list A's checkpoint pass cuts its blocks' fragments out of the volumes itself (k_myers_ck flag bit 22) and k_round_ctl does the round's bookkeeping; 0 = k_ext_frag in a launch of its own before every pass, as until round 5 */ \
    NUM(item_sort,         u32,    "NECAT_ITEM_SORT",         1, 0, ~0ull)           /* the ragged list-A items and the list-B items of every round in size-class order, 32 target columns per class, longest first (item_order.h: staged by the appends, put in place by k_round_ctl - which then has several workgroups); 0 = appended in place in arrival order, as before (A/B, parity fallback).  The cross-check build always appends in place */ \
    SET(rc_ckg_all,                "NECAT_RC_CKG_ALL")                               /* debugging: every block of a big round through the general pass k_myers_ckg (no fragment fusion, no merged ragged blocks) */ \
    NUM(rc_maxdist,        int,    "NECAT_RC_MAXDIST",        1 << 20, 0, ~0ull)     /* full blocks of a larger distance take the old kernels (tests lower it); without rc_carry at most kRcMaxDist = 160 */ \
    NUM(ck_lds,            u32,    "NECAT_CK_LDS",            0, 0, ~0ull)           /* bytes of dynamic LDS claimed by every workgroup (one wave) of k_myers_ck - caps how many of its waves a CU holds (160 KB / (1 KB + this)), leaving wave slots to the chains of the other streams (A/B measurements) */ \
    NUM(ck_post,           u32,    "NECAT_CK_POST",           1, 0, ~0ull)           /* k_myers_ck finds the bottom row's minimum after the pass, from word 7's deltas, and unrolls its windows (fast_shw8_ckp); 0 = tracked inside the pass */ \
    NUM(ckr_fast,          u32,    "NECAT_CKR_FAST",          1, 0, ~0ull)           /* list B's checkpoint pass (fast_shw_ckr in k_myers_ckf) runs the windows in which every lane of the wave is inside its block unrolled and without a per-step lane mask; 0 = every window rolled, as until round 5 */ \
    NUM(rc_fastb,          u32,    "NECAT_RC_FASTB",          1, 0, ~0ull)           /* list B's checkpoint pass through k_myers_ckf (32-bit halves, bitop3, DPP carries); 0 = the general pass k_myers_ckg */ \
    NUM(rc_prio,           u32,    "NECAT_RC_PRIO",           1, 0, ~0ull)           /* bits (1: 41.6 -> 41.0 ms per step; 2 costs 0.5 ms, 4 nothing): waves that raise their issue priority (s_setprio 3) - 1: list A's walk (k_rcwalk2w: every wave; k_rcwalk3: its walking wave), 2: list A's checkpoint pass, 4: list B's walk, 8 / 16: only the WALKING wave of list A's / list B's walk, for the length of its walk (kernel opts bit 16) */ \
    /* rc_pipe (1 = off: 2 - 4 pieces cost 1.8 - 2.3 ms per step, tools/r04/run28.sh, run29.sh) / rc_pipe_min (blocks): list A of a big round in pieces, walk of piece i beside the pass of piece i + 1 */ \
    NUM(rc_pipe,           u32,    "NECAT_RC_PIPE",           1, 1, 8) \
    NUM(rc_pipe_min,       u32,    "NECAT_RC_PIPE_MIN",       49152, 0, ~0ull) \
    NUM(rc_dbg,            u32,    "NECAT_RC_DBG",            0, 0, ~0ull)           /* timing only (bits 2 and 4, the rest is dropped): 2 = k_rcwalk2w walks every segment twice (once into a sink), 4 = recomputes every segment twice */ \
    NUM(rc_prefetch,       u32,    "NECAT_RC_PREFETCH",       0, 0, ~0ull)           /* measured 0.4 ms per step SLOWER, profiles/NOTES_r04.md 3: k_rcwalk2w loads the next segment's checkpoints / deltas / planes a segment ahead */ \
    NUM(rc_ww,             u32,    "NECAT_RC_WW",             1, 0, ~0ull)           /* which recompute walk runs.  1 = k_rcwalk2w (64-row records, one LDS read per walk step), except that list-A launches of at least rc3_min blocks go through k_rcwalk3; 2 = k_rcwalk3 everywhere (ext_rcwalk3.h: a workgroup of TWO waves recomputes 64 blocks - two lanes per block, both words of the pair per lane - into 32-DIAGONAL records, one of the two then walks the blocks column by column: faster alone, slower in the bench's small launches, profiles/NOTES_r05.md 1); 0 = k_rcwalk2 (every lane of a quad walks its block: cross-check build only - the product library refuses it when the context is created, necat_ctx_create prints why) */ \
    NUM(rc3_band,          ull,    "NECAT_RC3_BAND",          32, 0, ~0ull)          /* 32 or 16 (nothing else): diagonals per record of k_rcwalk3 (16: half the LDS per block in flight, 7 waves per SIMD instead of 4.5, a few per cent of the segments redone) */ \
    NUM(rc3_min,           u32,    "NECAT_RC3_MIN",           160000, 0, ~0ull)      /* blocks (4294967295 = never): with rc_ww = 1, list-A launches of at least this many blocks go through k_rcwalk3 (throughput form: fewer instructions per block, longer chain per segment) instead of k_rcwalk2w */ \
    /* ---- the batch Edlib_align hook (stage_edlib_batch.inl) */ \
    NUM(batch_chunk,       u32,    "NECAT_BATCH_CHUNK",       65536, 0, ~0ull)       /* blocks per launch of necat_edlib_align_batch (tests: several chunks) */ \
    SET(batch_rc,                  "NECAT_BATCH_RC")                                 /* set: the hook's blocks through the checkpoint pass + recomputing walk instead of the band kernels; the number then picks the pass - 2 = k_myers_ckf, 64 = k_myers_ckg with one wave per block (list B), anything else = k_myers_ckg */ \
    /* ---- oc2asmpm's stages */ \
    NUM(asm_rc,            u32,    "NECAT_ASM_RC",            1, 0, ~0ull)           /* the 2048-bp block aligner of oc2asmpm through k_myers_ckg + k_rcwalk2 (no NW pass, no band records); 0 = two-pass kernel + band + wave walk */ \
    NUM(asm_rc_pool,       size_t, "NECAT_ASM_RC_POOL_MB",    2048, 256, ~0ull)      /* checkpoint pool of that aligner, list A (list B: half of it; bytes in the field) */ \
    NUM(asm_lane,          int,    "NECAT_ASM_LANE",          0, 0, ~0ull)           /* 1: necat_asm_align_batch through the lane-per-alignment kernel (k_asm_align), the second implementation */ \
    NUM(asm_vote_budget,   ull,    "NECAT_ASM_VOTE_BUDGET",   16ull << 20, 1024, ~0ull)  /* 384-byte vote blocks per chunk and arena set of necat_asm_plan (stage_asm_plan.inl; then capped by the free memory) */ \
    NUM(asm_seed_budget,   ull,    "NECAT_ASM_SEED_BUDGET",   32ull << 20, 1024, ~0ull)  /* seeds per chunk of necat_asm_plan */ \
    NUM(asm_ends_device,   int,    "NECAT_ASM_ENDS_DEVICE",   0, 0, 1)               /* oc2asmpm asks for it (necat_knob_get): 1 = block aligner, end extension and records of a run of reads in one necat_asm_map_batch call (no columns downloaded, no one-byte copy of the volumes), 0 = necat_asm_align_batch + Extender::ends_packed on the host threads.  The entry point necat_asm_map_batch itself always runs on the device */ \
    NUM(asm_ends_diags,    u32,    "NECAT_ASM_ENDS_DIAGS",    128, 4, 2048)          /* diagonals the window of an end extension's DALIGNER job may hold in the first launch of necat_asm_map_batch (hangs of at most 300 bases: 32 bytes of LDS each, rounded up to a power of two); the jobs that outgrow it run once more at NECAT_DALIGN_DIAGS */ \
    SET(asm_no_overlap,            "NECAT_ASM_NO_OVERLAP")                           /* A/B: necat_asm_plan on one arena set and one stream, chunk after chunk */ \
    STR(asm_dump_votes,            "NECAT_ASM_DUMP_VOTES")                           /* a path: necat_asm_plan appends every read's ranked candidates to it (tests/host_core/check_asm_plan.cpp) */ \
    /* ---- consensus loop, several GPUs, everything */ \
    INT(cns_spec_extra,            "NECAT_CNS_SPEC_EXTRA",    1)                     /* speculation width of the consensus loop (may be negative) */ \
    NUM(cns_spec_cover,    int,    "NECAT_CNS_SPEC",          12, 0, ~0ull)          /* .. its cover; 0 = adaptive */ \
    NUM(cns_device,        int,    "NECAT_CNS_DEVICE",        1, 0, 1)               /* oc2cns asks for it (necat_knob_get): 1 = the consensus proper through necat_cns_consensus_batch's device path (path 0: certified, flagged templates recomputed on the host), 0 = its host path (path 1).  The library's entry point itself takes the path from its options */ \
    STR(cns_reads,                 "NECAT_CNS_READS")                                /* oc2cns asks for it (necat_knob_get): merged = the directory's volumes as ONE volume (fewer than 2^32 bases), gather = a resident volume per file and, per chunk of templates, the reads it names gathered by necat_volume_gather, auto or "" = merged below 2^32 bases, gather from there on */ \
    NUM(cns_chunk_bases,   ull,    "NECAT_CNS_CHUNK_BASES",   1ull << 31, 1, 1ull << 40)   /* oc2cns asks for it: the bases of the reads one chunk of templates may name on the gather path (cns_chunks.h); a template that names more goes alone, and the program refuses 2^32 */ \
    NUM(cns_tag_budget,    ull,    "NECAT_CNS_TAG_BUDGET",   32ull << 20, 1, 1ull << 30)  /* alignment columns (= tags) per chunk of templates of the device consensus (about 90 bytes of device memory per tag); a template with more goes alone */ \
    NUM(cns_tol_scale,     ull,    "NECAT_CNS_TOL_SCALE",     1, 1, 1ull << 40)      /* tests only: multiplies the error bound the scores of the device consensus carry (10000000 sends every template back to the host) */ \
    NUM(nw_device,         int,    "NECAT_NW_DEVICE",         0, 0, 1)               /* oc2cns -r 1 (necat_cns_extension_batch with rescue_long_indels): 1 = the rescue pair's global alignment with path through the kernels of necat_nw_path_batch, 0 = rescue::EdlibGo on the host threads.  The entry point necat_nw_path_batch itself always runs on the device */ \
    NUM(nw_pool,           size_t, "NECAT_NW_POOL_MB",        1024, 1, 1ull << 20)   /* cap of the arena the leaves of necat_nw_path_batch keep their walk flags in (16 bytes per band word and column; bytes in the field); more leaves go through it in several launches.  One leaf needs less than 1 MB */ \
    NUM(dalign_device,     int,    "NECAT_DALIGN_DEVICE",     0, 0, 1)               /* oc2cns -r 1: 1 = the rescue pair's local alignment (DALIGNER around the anchor) through the kernel of necat_local_align_batch, 0 = rescue::Dalign on the host threads.  With NECAT_NW_DEVICE=1 as well the reads' words stay on the device.  The entry point necat_local_align_batch itself always runs on the device */ \
    NUM(dalign_diags,      u32,    "NECAT_DALIGN_DIAGS",      512, 4, 2048)          /* diagonals the wave's window may hold in necat_local_align_batch (32 bytes of LDS each, rounded up to a power of two); a job whose window outgrows it is recomputed by the host code.  Widest measured: 333 in oc2cns -r 1, 511 in oc2rm_worker with NECAT_RM_RESCUE_DEVICE=1 on indels of up to 1500 bases */ \
    NUM(rm_rescue_device,  int,    "NECAT_RM_RESCUE_DEVICE",  0, 0, 1)               /* necat_map_reference (oc2rm_worker): 1 = the rescue pair once, ahead of the walk, for every candidate that can need it - DALIGNER on the candidate's stretch of the reference through the kernel of necat_local_align_batch (capacity NECAT_DALIGN_DIAGS), edlib's path through the kernels of necat_nw_path_batch - and the walk on the host threads reads a table: the volumes' words stay on the device; 0 = rescue::Dalign + rescue::EdlibGo inside the walk */ \
    NUM(ctg_seed_lds,      u32,    "NECAT_CTG_SEED_LDS",      512, 0, 2048)          /* necat_ctg_seed_batch: matches of a job whose chain arrays (28 bytes each) live in LDS; a job with more chains in the call's scratch (tests lower it) */ \
    NUM(ctg_seed_budget,   ull,    "NECAT_CTG_SEED_BUDGET",   4ull << 20, 1, 1ull << 28)  /* necat_ctg_seed_batch: seeds per chunk of jobs (72 bytes of device memory each); a job with more seeds than this is computed by the host form inside the call (n_fallback) */ \
    NUM(ctg_seed_job_max,  ull,    "NECAT_CTG_SEED_JOB_MAX",  16384, 1, 1ull << 28)       /* necat_ctg_seed_batch: seeds of ONE job on the device; its rank sorts are quadratic in them (16384: some 4 M steps per lane), so a job with more - a long read in repeats - is computed by the host form inside the call (n_fallback) */ \
    INT(cns_threads,               "NECAT_CNS_THREADS",       32)                    /* host threads of the parallel host loops (cns::parallel_for; <= 0: 32), never more than the machine has */ \
    STR(comm,                      "NECAT_COMM")                                     /* auto / rccl / ipc: the transport of necat_comm_create where its argument leaves the choice ("" = auto) */ \
    NUM(trace,             int,    "NECAT_TRACE",             0, 0, ~0ull)           /* bits: 1 = extension rounds, 2 = host stages */

namespace necat {

struct KnobSet { bool set; int v; };

struct Knobs {
    typedef uint32_t u32;
    typedef unsigned long long ull;
#define NECAT_KNOB_NUM(field, type, name, dflt, lo, hi) type field;
#define NECAT_KNOB_INT(field, name, dflt) int field;
#define NECAT_KNOB_SET(field, name) KnobSet field;
#define NECAT_KNOB_STR(field, name) std::string field;
    NECAT_KNOBS(NECAT_KNOB_NUM, NECAT_KNOB_INT, NECAT_KNOB_SET, NECAT_KNOB_STR)
};

extern thread_local const Knobs* tl_knobs;      // the knobs of the context whose call is running on this thread (necat_hip.hip)
inline const Knobs& knob() { return *tl_knobs; }

// ---- read per call: the entry point has no context.  necat_index_plan is the only one, and these two are the only variables the library reads outside necat_ctx_create:
//   NECAT_XGMI_GBS     link bandwidth (GB/s) the plan prices the exchange with where the caller passes none (default 100)
//   NECAT_INDEX_SHARD  forces the plan's decision: 0 = replicate, anything else = shard (*shard stays -1 when unset)
inline void index_plan_env(double* link_gbs, int* shard)
{
    const char *g = getenv("NECAT_XGMI_GBS"), *s = getenv("NECAT_INDEX_SHARD");
    *link_gbs = g && atof(g) > 0 ? atof(g) : 100.0; *shard = s ? atoi(s) != 0 : -1;
}

}  // namespace necat
