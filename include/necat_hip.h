/*
 * necat_hip.h - C ABI of libnecat_hip.so, the MI355X (gfx950) implementation of NECAT's all-vs-all
 * overlap stage (oc2pmov: k-mer index -> seeding / DDF vote / chain DP -> block-wise banded Myers
 * extension -> candidate / M4 records).
 *
 * NECAT has no in-process plugin interface for this stage: the drop-in boundary is the
 * oc2pmov process (argv + volume files in, one record file out), which necat_amd/csrc/oc2pmov_main.cpp
 * reproduces on top of this ABI.  The entry points below mirror, at batch granularity, the three calls
 * the reference's worker (pm_one_volume/pm_worker.c) makes into libontcns, so that a maintainer could
 * also bind them directly:
 *
 *   necat_index_build      <- build_lookup_table      lookup_table/lookup_table.h:23-27, lookup_table.c:149
 *   necat_find_candidates  <- find_candidates (+ the per-read sort/truncate of pm_search_one_volume)
 *                                                     word_finder/word_finder.h:33-45, pm_worker.c:100-140,163-171
 *   necat_extend           <- extend_candidates/onc_align
 *                                                     pm_worker.c:29-83, gapped_align/oc_aligner.h:45-55
 *   necat_map_pair         <- pm_search_one_volume, -j 1: the two calls above fused (candidates stay on the device)
 *                                                     pm_worker.c:85-173
 *   necat_volume_upload    <- pdb_load                common/packed_db.c:386 (the 2-bit pac + SequenceInfo)
 *   necat_onc_align_batch  <- onc_align with its gapped strings, for the consensus client
 *   necat_nw_path_batch    <- edlib_go: the rescue pair's global alignment with its path
 *                                                     gapped_align/oc_aligner.h:45-55, consensus_aux.c:124-215
 *   necat_local_align_batch <- ocda_go: the rescue pair's local alignment around the anchor, DALIGNER's wave
 *                                                     gapped_align/oc_daligner.c:36-79, gapped_align/align.c:382,1043
 *
 * Conventions: plain C types only; every function returns 0 on success and a negative code on failure
 * (necat_last_error() gives the text); output arrays are malloc'ed by the library and released with
 * necat_free(); handles are opaque; one host thread per context.  There is no CPU fallback: every entry
 * point fails with NECAT_ERR_DEVICE if no gfx950 device is usable.
 */
#ifndef NECAT_HIP_H
#define NECAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header.  It changes whenever a struct an entry point copies into caller memory changes size or layout (round 5 grew
 * necat_timings and necat_shard_timings, round 6 necat_timings again) or an entry point is added (7: the trimming stage; 8: necat_knob_get; 9: necat_cns_consensus_batch; 12: necat_asm_map_batch; 13: necat_get_rm_stats_sized; 14: necat_ctg_consensus_batch; 15: necat_ctg_seed_batch; 16: necat_ctg_extend_batch): a caller built against another header must not pass its smaller struct to
 * necat_get_timings / necat_get_shard_timings.  Check necat_abi_version() == NECAT_ABI_VERSION once after loading the library, or use the
 * *_sized getters, which copy at most the bytes the caller says its struct has (new fields are always appended). */
#define NECAT_ABI_VERSION   16
int  necat_abi_version(void);

#define NECAT_OK            0
#define NECAT_ERR_ARG      (-1)
#define NECAT_ERR_DEVICE   (-2)   /* no usable GPU / HIP runtime error */
#define NECAT_ERR_MEMORY   (-3)
#define NECAT_ERR_CAPACITY (-4)   /* an internal device buffer overflowed (reported, never silent) */
#define NECAT_ERR_INTERNAL (-5)
#define NECAT_ERR_COMM     (-6)   /* rank-to-rank exchange failed (RCCL / HIP IPC / the host all-gather callback) */

typedef struct necat_ctx necat_ctx;
typedef struct necat_volume necat_volume;
typedef struct necat_index necat_index;
typedef struct necat_comm necat_comm;

/* common/map_options.h:10-25 (same fields, same meaning) */
typedef struct {
    int    kmer_size;           /* -k */
    int    scan_window;         /* -z */
    int    kmer_cnt_cutoff;     /* -q */
    int    block_size;          /* -b */
    int    block_score_cutoff;  /* -s */
    int    num_candidates;      /* -n */
    int    align_size_cutoff;   /* -a */
    double ddfs_cutoff;         /* -d (parsed, ignored by the reference: word_finder.c:10) */
    double error;               /* -e */
    int    num_output;          /* -m (unused by oc2pmov) */
    int    num_threads;         /* -t */
    int    job;                 /* -j 0 = candidates, 1 = align */
    int    binary_output;       /* -u */
    int    use_hdr_as_id;       /* -i */
} necat_map_options;

/* common/gapped_candidate.h:9-19 (GappedCandidate; idx fields are 64-bit unsigned there) */
typedef struct {
    int32_t  qid, sid, qdir, sdir, score;
    int32_t  _pad;
    uint64_t qbeg, qend, qsize;
    uint64_t sbeg, send, ssize;
    uint64_t qoff, soff;
} necat_candidate;

/* common/m4_record.h:10-25 (M4Record, 96 bytes, identical field order) */
typedef struct {
    int32_t  qid, qdir;
    uint64_t qoff, qend, qext, qsize;
    int32_t  sid, sdir;
    uint64_t soff, send, sext, ssize;
    double   ident_perc;
    int32_t  vscore;
    int32_t  _pad;
} necat_m4;

/* what onc_align leaves in OcAlignData (gapped_align/oc_aligner.h:6-15): strand coordinates of the
 * alignment, its length in gapped columns and identity; ok = onc_align's return value */
typedef struct {
    int32_t ok;
    int32_t qoff, qend, toff, tend;
    int32_t align_size;
    double  ident_perc;
} necat_alignment;

/* wall-clock (ms, HIP events) of the last call of each stage + work counters of the extension */
typedef struct {
    double   index_ms, seed_ms, extend_ms;
    double   myers_ms;          /* sum over launches of the block Myers DP kernel */
    double   traceback_ms;
    uint64_t myers_launches;
    uint64_t myers_blocks;      /* block alignments (Edlib_align equivalents) */
    uint64_t myers_word_updates;/* 64-row word updates actually computed (SHW + NW) */
    uint64_t myers_cells_bases; /* sum over blocks of query+target fragment bases */
    uint64_t rounds;
    /* the list-A kernels alone (blocks <= 512 x 512), launches of more than NECAT_SINGLE_PASS blocks: the two-pass
     * DP kernel k_myers_coop<8,16,512,8,false> and its traceback k_traceback<8,16,512,..> */
    double   myersA_ms;
    uint64_t myersA_launches, myersA_blocks;
    double   tracebackA_ms;
    /* the list-A DP launch with the most blocks (the throughput-bound regime of the dominant kernel) */
    double   myersA_big_ms;
    uint64_t myersA_big_blocks;
    /* band words the NW passes stored (= the word updates the reference's banded NW pass needs, edlib_ex.c:311-325 with
     * k = the block's distance): with myers_word_updates, the redundant part of the computed work */
    uint64_t myers_band_words;
    /* the small lists of the late rounds: fragments + single-pass DP + walk + plan of the next block in ONE launch per list and
     * round, the band in LDS (necat_amd/csrc/ext_tail.h); their blocks are part of myers_blocks, their time is not in myers_ms /
     * traceback_ms */
    double   fused_ms;
    uint64_t fused_launches, fused_blocks;
    /* the full 512 x 512 blocks of the big list-A rounds (necat_amd/csrc/ext_rcwalk.h): k_myers_ck (SHW pass + checkpoints; its time is
     * what myersA_ms holds for those rounds) and k_rcwalk4 (the walk that recomputes its cells: rc_ms); rc_blocks of them, rc_words word
     * updates recomputed by the walk (each block also cost 4096 in the SHW pass) */
    double   rc_ms;
    uint64_t rc_launches, rc_blocks, rc_words;
    double   rc_ck_ms;          /* k_myers_ck of those rounds (beside the ragged blocks' DP kernel on another stream) */
    /* work counters of the last seeding call (necat_find_candidates* / the seeding part of necat_map_pair*), the terms of SURVEY 8d's
     * B_seed = L / 4 + 8 lookups + 8 hits + 28 candidates: bases of the query strands walked (both strands of every read of the
     * call), sampled k-mers looked up in the table (word_finder.c:66-83, one kmer_stats word each), offset-list entries those k-mers
     * own (what collect_seeds reads, word_finder.c:107-139) and candidates emitted */
    uint64_t seed_bases, seed_lookups, seed_hits, seed_cands;
} necat_timings;

/* Threads.  A context is used by ONE host thread at a time (its streams, arenas, timings and last-error text are its own); DIFFERENT contexts -
 * of one device or of several - may be called from different threads at the same moment, and nothing else in the library is shared but the pool
 * of pinned result blocks behind necat_free (a mutex).  Volumes and indexes are plain device allocations: made through one context, they may be
 * read by calls on any other context of that device once the call that made them has returned (necat_volume_free / necat_index_free when no call
 * uses them any more).  That is how several pairs are kept in flight on one device - one context + host thread per pair, one shared index:
 * INTEGRATION.md 2g, the programs' NECAT_PAIR_LANES, bench.py --in-flight (reference analogue: pm_main's thread pool on one lookup table,
 * pm_worker.c:335-390).  necat_ctx_trim synchronises the whole DEVICE: not while another context has calls in flight. */
void        necat_default_options(necat_map_options* o);            /* map_options.c:12-28 */
int         necat_ctx_create(int device_id, necat_ctx** out);
void        necat_ctx_destroy(necat_ctx* ctx);

/* Release the context's cached device scratch (index-build partitions, seeding arenas, band pools ...); it is allocated again on
 * demand.  For short-lived processes that build an index once: on MI355X a fresh process pays tens of ms per GB of VRAM that is
 * still being cleaned after the previous one, so a command-line program keeps its peak small.  (No reference counterpart.) */
void        necat_ctx_trim(necat_ctx* ctx);
const char* necat_last_error(const necat_ctx* ctx);    /* ctx == NULL: why this thread's last necat_ctx_create failed */
int         necat_device_name(const necat_ctx* ctx, char* buf, size_t n);

/* pac: NECAT 2-bit bases (first base of a byte in its top two bits, ontcns_aux.h:118-119);
 * seq_offset/seq_size: SequenceInfo.offset/.size (packed_db.h:12-18). Host buffers are not retained. */
int  necat_volume_upload(necat_ctx* ctx, const uint8_t* pac, uint64_t nbases,
                         const uint64_t* seq_offset, const uint64_t* seq_size, uint64_t nseq,
                         necat_volume** out);
/* <- pdb_add_one_seq (packed_db.c:229-252) for a whole volume: ASCII bases (A C G T in either case; '-' and every other
 * character as common/nst_nt4_table.c codes them, OR-ed into the pac byte exactly like the reference) packed on the device.
 * pac_out (may be NULL): (nbases + 3) / 4 bytes, what oc2mkdb writes after the volume's headers.  out (may be NULL): the
 * uploaded volume, as necat_volume_upload of those bytes would give. */
int  necat_volume_pack(necat_ctx* ctx, const char* ascii, uint64_t nbases, const uint64_t* seq_offset,
                       const uint64_t* seq_size, uint64_t nseq, uint8_t* pac_out, necat_volume** out);
/* A volume holds fewer than 2^32 bases, and that stays: a read set of more keeps one volume per file (as oc2mkdb cut them) and a stage that reads
 * across files - the consensus entries, whose candidates name reads of any volume - works on a GATHERED volume: the sequences `ids` of the resident
 * volumes vols[0 .. n_vols), copied on the device into one compact volume (<- merge_volumes with its 64-bit offsets, common/makedb_aux.c:137-153,
 * restricted to the reads in hand).  vols[k] holds the sequences with the global ids vol_start_id[k] .. + its sequence count; ids are global and
 * strictly ascending, so the result's local id i is ids[i] and every comparison between ids comes out as on the merged set.  The result is word for
 * word what necat_volume_upload of those sequences' bases, concatenated on the host, would give (guard words and the unused bits of the last word
 * zero); it is freed with necat_volume_free and does not refer to vols afterwards.  n_ids = 0 gives an empty volume.
 * NECAT_ERR_ARG with a message, nothing launched: ids that do not ascend, an id in no volume, volumes whose id ranges overlap, 2^32 bases or more. */
int  necat_volume_gather(necat_ctx* ctx, const necat_volume* const* vols, const int64_t* vol_start_id, uint64_t n_vols,
                         const int64_t* ids, uint64_t n_ids, necat_volume** out);
/* the context's last necat_volume_gather: its kernel alone (ms, HIP events) and the bytes it read and wrote - the result's words once each way.
 * (necat_volume_gather, necat_volume_gather_stats and necat_volume_download came after ABI version 16 and leave it as it is: they are additions, no struct
 * an entry point copies into caller memory changed.  A caller that needs them checks for the symbols.) */
int  necat_volume_gather_stats(const necat_ctx* ctx, double* kernel_ms, uint64_t* bytes);
/* a resident volume's bases as pac bytes, as necat_volume_upload took them: pac_out holds (nbases + 3) / 4 bytes */
int  necat_volume_download(necat_ctx* ctx, const necat_volume* v, uint8_t* pac_out);
void necat_volume_free(necat_ctx* ctx, necat_volume* v);

/* Final LookupTable contents (lookup_table.h:6-21): kmer_stats[h] = cnt<<34 | start for k-mers with
 * 1..max_occ occurrences (0 otherwise); offset_list = base offsets grouped by hash, ascending inside
 * one hash. */
int  necat_index_build(necat_ctx* ctx, const necat_volume* ref, int kmer_size, int max_occ,
                       necat_index** out);
int  necat_index_size(const necat_index* ix, uint64_t* table_entries, uint64_t* n_offsets);
/* copy the index to host buffers (either may be NULL); used by parity tests */
int  necat_index_download(necat_ctx* ctx, const necat_index* ix, uint64_t* kmer_stats, uint64_t* offset_list);
/* The table as the device holds it when it was built in the sparse layout (k >= 11): per 64 table entries one pair of words
 * (bits: which of the 64 entries are non-zero; base: position in `compact` of the first of them), and `compact`, the non-zero
 * `cnt<<34 | start` entries in hash order - kmer_stats[h] = bit (h & 63) of bits[h >> 6] set ? compact[base[h >> 6] + popcount(bits
 * below it)] : 0.  0.27 + (8 bytes per distinct kept k-mer) GB at k = 15 instead of the 8.6 GB of the dense table: what a host-side
 * reader of the table (the vote of oc2asmpm, asm_pm_common.c:509-702) copies.  necat_index_sparse_size: n_pairs = 0 for an index in
 * the dense layout (small k: use necat_index_download).  Outputs of the download may be NULL (skipped); pairs = 2 * n_pairs words. */
int  necat_index_sparse_size(const necat_index* ix, uint64_t* n_pairs, uint64_t* n_compact);
int  necat_index_download_sparse(necat_ctx* ctx, const necat_index* ix, uint64_t* pairs, uint64_t* compact, uint64_t* offset_list);
void necat_index_free(necat_ctx* ctx, necat_index* ix);

/* All reads of `reads` (both strands) against `ref`.  Output: per read, its candidates in exactly the
 * order pm_search_one_volume would hand them on (job 0: discovery order FWD then REV, sorted by
 * GappedCandidate_PmScoreGT and cut to num_candidates only when more than num_candidates; job 1:
 * always sorted and cut), reads in ascending id; ids are GLOBAL (+= read_start_id / ref_start_id,
 * pm_worker.c:165-166).  `pairwise` as in find_candidates (self-volume: only subjects before the
 * query, word_finder.c:121-127). */
int  necat_find_candidates(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref,
                           const necat_volume* reads, int read_start_id, int ref_start_id,
                           int pairwise, const necat_map_options* opt,
                           necat_candidate** out, uint64_t* n_out);

/* onc_align on every candidate (ids global, as produced above; block size kOcaBlockSize = 512,
 * edlib_ex_aux.h:23), then the per-read containment filter of extend_candidates in candidate order
 * (pm_worker.c:44, map_aux.c:4).  Output records carry global ids; REV query coordinates are flipped
 * to forward-strand numbering (pm_worker.c:73-78). */
int  necat_extend(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads,
                  int read_start_id, int ref_start_id,
                  const necat_candidate* cands, uint64_t n, const necat_map_options* opt,
                  int tail_match_len, necat_m4** out, uint64_t* n_out);

/* pm_search_one_volume of a mapping job (pm_worker.c:85-173 with -j 1) for every read of `reads` in one call:
 * necat_find_candidates followed by necat_extend, with the candidates never leaving the device.  Same M4
 * records as the two calls made one after the other; *n_candidates (optional) = candidates examined. */
int  necat_map_pair(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                    int read_start_id, int ref_start_id, int pairwise, const necat_map_options* opt,
                    int tail_match_len, necat_m4** out, uint64_t* n_out, uint64_t* n_candidates);

/* rm_search_one_volume (reference_mapping/rm_worker.c:198-291) for every read of `reads` against the reference volume `ref`
 * (oc2rm_worker, necat.pl:661): candidates of both strands against the whole reference (pairwise = FALSE), sorted and cut to
 * num_candidates; every candidate is aligned block-wise against the stretch of its reference sequence the read can reach from the
 * anchor (calc_reference_range, :43-59; tail_match_len = ONC_TAIL_MATCH_LEN_SHORT) on the device; then, per read and in candidate
 * order on the host threads (rm_extend_candidates, :165-196): anchors inside an accepted record are skipped, failed alignments
 * dropped, alignments more than 500 bp short of the chained range replaced by the rescue pair's (ocda_go + edlib_go, :113-140) or
 * dropped with it.  Records as rm_extend_candidate leaves them (:143-163), ids global.  *n_rescued (optional) = records that came
 * from the rescue pair. */
int  necat_map_reference(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                         int read_start_id, int ref_start_id, const necat_map_options* opt,
                         necat_m4** out, uint64_t* n_out, uint64_t* n_candidates, uint64_t* n_rescued);

/* What the context's last necat_map_reference did with the rescue pair.  With NECAT_RM_RESCUE_DEVICE=1 (default 0) the pair is run
 * ahead of the walk, once, for EVERY candidate whose block-wise alignment succeeded and falls short of its chain (n_need) - DALIGNER
 * through the kernel of necat_local_align_batch on the candidate's stretch of the reference as a slice of the resident volume, edlib's
 * path over the ranges it found through the kernels of necat_nw_path_batch - and the walk on the host threads reads the answers from a
 * table: a candidate the walk never reaches (its anchor lies inside a record accepted earlier) was computed for nothing, n_need -
 * n_tried of them.  The volumes' words are not copied to the host on that path unless a job is handed back to the host code
 * (words_fetched).  The kernels' limits hold: a read of 2^30 bases or more, a reference sequence of 2^31 or more or a DALIGNER range of 2^26 or more
 * make the call fail with NECAT_ERR_ARG under the knob (it runs with the knob at 0).  With the knob at 0 the pair runs on the host threads inside the walk and the device counters are 0.
 * necat_get_rm_stats_sized copies at most `bytes` bytes (new fields are appended). */
typedef struct {
    uint64_t n_candidates;      /* candidates of the call */
    uint64_t n_need;            /* .. with a block-wise alignment that falls short of the chain: the jobs of the speculative pass */
    uint64_t n_tried;           /* rescue pairs the walk consumed */
    uint64_t n_rescued;         /* .. that gave the record */
    uint64_t n_dalign_device;   /* local halves decided on the device */
    uint64_t n_dalign_host;     /* .. handed back to the host code = n_dalign_over_cap + n_dalign_selfcheck */
    uint64_t n_dalign_over_cap; /* .. because the window outgrew NECAT_DALIGN_DIAGS */
    uint64_t n_dalign_selfcheck;/* .. because the job flagged itself */
    uint64_t n_nw_jobs;         /* jobs DALIGNER gave a range for: the global halves */
    uint64_t n_nw_device;       /* .. decided on the device */
    uint64_t n_nw_host;         /* .. handed back to the host code (a self-check failure: 0 unless there is a bug) */
    uint32_t max_diags;         /* the widest DALIGNER window of the call */
    uint32_t words_fetched;     /* 1: the volumes' words were copied to the host (always, when a pair runs with the knob at 0) */
    double   dalign_ms, nw_ms;  /* the device's share of the two halves: upload, launches and downloads, without the host code of a job handed back (0 with the knob at 0) */
    double   replay_ms;         /* the walk on the host threads (with the knob at 0: the pairs inside it) */
} necat_rm_stats;
int  necat_get_rm_stats_sized(const necat_ctx* ctx, void* stats, size_t bytes);

/* What the checkpoint passes of this context's last extension call (necat_extend, necat_map_pair, necat_onc_align_batch, ..) issued against what their blocks
 * needed.  A pass runs the blocks of one wave - 8 ragged blocks of list A, 4 blocks of list B - for as many steps as the wave's longest block has
 * (a block needs tn + nblk - 1): issued = blocks of a wave x the wave's steps, needed = the sum of the blocks' own steps, both in lane-steps of a block.
 * The rounds order those blocks by size class (NECAT_ITEM_SORT), which is what keeps issued close to needed.  An addition after ABI version 16,
 * which it leaves as it is: no struct of a caller grows. */
typedef struct {
    uint64_t a_issued, a_needed, a_blocks;      /* list A's ragged waves (a wave that holds full blocks too counts them) */
    uint64_t b_issued, b_needed, b_blocks;      /* list B's waves */
} necat_item_order_stats;
int  necat_get_item_order_stats(const necat_ctx* ctx, necat_item_order_stats* stats);

/* onc_align (gapped_align/oc_aligner.h:45-55) on every candidate WITH the alignment itself - the call the
 * consensus stage makes (cns_extension, consensus/consensus_aux.c:124-215, tail_match_len =
 * ONC_TAIL_MATCH_LEN_LONG = 4).  No containment filter: aln[i] and the columns at ops + ops_off[i] belong to
 * cands[i].  TWO BITS per gapped column, in alignment order, four columns per byte from the low bits up
 * (column j of an alignment = bits 2 (j & 3) of its byte j >> 2): 0 match, 1 query base over '-' in
 * target_align, 2 '-' in query_align over a target base, 3 mismatch; aln[i].align_size columns, every alignment
 * starts on an 8-byte boundary (ops_off[i] = byte offset, ops_off[n] = total bytes); necat_gapped_strings()
 * turns them into the reference's two "ACGT-" strings. */
int  necat_onc_align_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads,
                           int read_start_id, int ref_start_id,
                           const necat_candidate* cands, uint64_t n, const necat_map_options* opt,
                           int tail_match_len, necat_alignment** aln, uint8_t** ops, uint64_t** ops_off);

/* blockwise_edlib_align (asm_pm/blockwise_edlib.c:1205-1371) for n anchors at once: the block aligner of oc2asmpm = onc_align with
 * 2048-bp blocks and tail match length 8 (hbn_align.c:8, blockwise_edlib.c:910-911), the read on its forward strand against the subject
 * on strand sdir (asm_pm_common.c:133-143 turns a reverse query into a reverse subject).  anchors[i]: ids global, qoff on the forward
 * read, soff on strand sdir of the subject.  Outputs as necat_onc_align_batch: aln[i] (ok = at least min_align_size columns; the
 * identity test, hbn_align.c / blockwise_edlib.c:1357, is the caller's) and the columns, two bits each, at ops + ops_off[i]; expand them
 * with necat_gapped_strings (tseq = the subject ON ITS STRAND). */
typedef struct { int32_t qid, sid, sdir, qoff, soff; } necat_asm_anchor;
int  necat_asm_align_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                           const necat_asm_anchor* anchors, uint64_t n, double error, int min_align_size,
                           necat_alignment** aln, uint8_t** ops, uint64_t** ops_off);

/* oc2asmpm's candidate stage for all reads of a volume at once (asm_pm/asm_pm_common.c): the 1000-bp block vote of both strands of every read
 * (pairwise_mapping :509-702, find_location :479-507), the per-read order and cut (AsmGappedCandidate_ScoreGT :145-153, the first -n candidates,
 * extend_candidates :329-345) and, for every distinct (subject, strand) among those in that order, the chained range of compute_align_range_1
 * (asm_pm/find_mem.c:222-265: 10-mer matches -> maximal exact matches -> mem_find_best_can, asm_pm/km_chain.c:322-445).  opt: kmer_size (the index's),
 * scan_window (BC), num_candidates.  out[first[r] .. first[r + 1]): read r's entries in the walk's order; ids global; qoff (forward read) / soff (on
 * strand sdir of the subject) = the anchor, score = the chain's score; qoff < 0: no chain of score >= 100, nothing to align.  Both arrays: necat_free. */
typedef struct { int32_t qid, sid, sdir, qoff, soff, score, ssize; } necat_asm_plan;
int  necat_asm_plan_batch(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                          const necat_map_options* opt, necat_asm_plan** out, uint64_t** first);

/* hbn_map_extend (asm_pm/hbn_align.c:282-326) for n planned anchors at once, from the anchor to the record: the block aligner of
 * necat_asm_align_batch, then - for an alignment of at least min_align_size columns and identity >= min_ident_perc (65.0 in the reference) - DALIGNER's
 * extension of either end whose overhang min(read, subject) is 1 .. 300 bases (left_extend :88-176, right_extend :178-262; error 0.35 and minimum
 * size 1 are the reference's constants), fix_ident_perc (:264-280) and the record as extend_candidates builds it (asm_pm_common.c:329-422: qdir 0,
 * vscore = the chain's score, qext / sext = the anchor, a reverse subject's range turned to forward coordinates).  The alignments' columns never
 * leave the device.  plans: necat_asm_plan_batch's entries unchanged (ids global); an entry with qoff < 0 is skipped.  recs[i] / kept[i] belong to
 * plans[i]; kept[i] = 1 iff the entry has a record (recs[i] is zero otherwise).  The DALIGNER jobs are the kernel of necat_local_align_batch on
 * prefixes / suffixes of the two sequences: first with room for NECAT_ASM_ENDS_DIAGS diagonals (default 128), the jobs that outgrow it once more
 * with NECAT_DALIGN_DIAGS, what is still flagged through the host code inside the call.  error: the block aligner's (0.5 in the reference).
 * Argument errors as necat_asm_align_batch.  Both arrays: necat_free. */
typedef struct {
    uint64_t n_anchors;        /* entries with qoff >= 0 */
    uint64_t n_ok;             /* alignments of at least min_align_size columns */
    uint64_t n_low_ident;      /* .. of those, below min_ident_perc (no record) */
    /* per side, [0] left and [1] right, over the alignments that have a record: */
    uint64_t n_tried[2];       /* overhang of 1 .. 300 bases */
    uint64_t n_extended[2];    /* .. and DALIGNER's extension accepted */
    uint64_t n_hang0[2];       /* no overhang */
    uint64_t n_hang_long[2];   /* overhang above 300 */
    uint64_t n_no_run[2];      /* tried, but the alignment has no run of 8 equal columns: no DALIGNER job */
    uint64_t n_jobs;           /* DALIGNER jobs = n_tier1 + n_tier2 + n_host */
    uint64_t n_tier1;          /* decided with NECAT_ASM_ENDS_DIAGS diagonals */
    uint64_t n_tier2;          /* .. with NECAT_DALIGN_DIAGS */
    uint64_t n_host;           /* .. by the host code (window above both, or a job that flagged itself) */
    uint64_t n_steps;          /* wave steps over all launches */
    uint64_t diag_hist[12];    /* jobs by their widest window w: [k] counts 2^k <= w < 2^(k+1), the last bucket is open-ended */
    uint32_t max_diags;        /* the widest window a step began with */
    uint32_t _pad;
    double   device_ms;        /* the call without .. */
    double   host_ms;          /* .. the host's share: arguments, the host code's jobs, the records' ids */
} necat_asm_map_stats;
int  necat_asm_map_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                         const necat_asm_plan* plans, uint64_t n, double error, int min_align_size, double min_ident_perc,
                         necat_m4** recs, uint8_t** kept, necat_asm_map_stats* stats);

/* Host helper: expand `n` packed columns into query_align / target_align (each n bytes, no terminator).
 * qseq / tseq: byte codes 0..3 of the query STRAND (reverse complement for qdir = 1) and of the subject;
 * qoff / toff: the alignment's start in them (necat_alignment.qoff / .toff).  Returns 0, or NECAT_ERR_ARG
 * if the columns run past qsize / tsize. */
int  necat_gapped_strings(const uint8_t* ops, uint64_t n, const uint8_t* qseq, uint64_t qsize, uint64_t qoff,
                          const uint8_t* tseq, uint64_t tsize, uint64_t toff, char* query_align, char* target_align);

/* ---- consensus stage (oc2cns), extension loop only - SURVEY 8f.1 ------------------------------------------
 * What consensus_one_read (consensus/consensus_one_read.c:221-372) does for ONE template before it hands
 * over to the consensus proper (tasc/cbcns.c): align its candidates in score order - first until 15
 * end-to-end overlaps give an identity cutoff (get_good_overlaps, consensus/error_estimate.c:96-183), then in
 * groups of 50 until the template is covered max_cov deep - and pass every accepted alignment to
 * add_one_align (tasc/cbcns.c:47) with a weight.  necat_cns_extension_batch does that for MANY templates in
 * one call: the candidates each template's loop would reach next are aligned speculatively, all templates
 * together, on the device (the DP kernels of necat_onc_align_batch, tail_match_len = 4); the loop's
 * sequential decisions (read already used, region already covered, cutoff) are then replayed in order on
 * the results, so the overlaps, their order and the per-template numbers are those of the sequential loop.
 * With rescue_long_indels (-r 1; default 0: cns_options.c:19) a candidate whose block-wise extension failed or stopped more than
 * 200 bp short of its chained range is aligned again as in the reference (consensus_aux.c:168-199), after each device pass:
 * DALIGNER's local alignment around the anchor on all host threads (necat_amd/csrc/rescue.h, cns_rescue.h) - with
 * NECAT_DALIGN_DEVICE=1 through the kernel of necat_local_align_batch instead - then edlib's global path over the range it
 * found - with NECAT_NW_DEVICE=1 on the device for all such candidates of the pass at once (the kernels of necat_nw_path_batch
 * on the resident reads), with 0 on the host threads.  With both set the reads' words never come back to the host. */

/* the fields of CnsOptions (consensus/cns_options.h:6-18) the loop reads; defaults cns_options.c:10-22 */
typedef struct {
    int    min_align_size;          /* -a 400 */
    int    min_cov;                 /* -x 4   */
    int    max_cov;                 /* -y 12  */
    double error;                   /* -e 0.5 */
    double mapping_ratio;           /* -p 0.8 */
    int    use_fixed_ident_cutoff;  /* -u 0   */
    int    rescue_long_indels;      /* -r 0   */
} necat_cns_options;
void necat_cns_default_options(necat_cns_options* o);

/* one add_one_align call: the overlap of candidate `cand` with its template */
typedef struct {
    uint64_t cand;            /* index into the cands array of the call */
    int32_t  qoff, qend, toff, tend;   /* as in necat_alignment */
    int32_t  align_size;      /* gapped columns */
    uint32_t ops_block;       /* the columns start at result->ops[ops_block] + ops_off (bytes), align_size of them, */
    uint64_t ops_off;         /* packed 2 bits per column as in necat_onc_align_batch                               */
    double   ident_perc;
    double   weight;          /* calc_cns_weight, consensus_one_read.c:11-16 */
} necat_cns_overlap;

/* what consensus_one_read leaves for one template */
typedef struct {
    int32_t  examined;        /* 0: fewer than min_cov candidates, the template is skipped (:223) */
    int32_t  num_can;         /* CnsSeq.num_can   (common/cns_seq.h:12) */
    int32_t  num_ovlps;       /* CnsSeq.num_ovlps (:13) = ovlp_end - ovlp_begin */
    int32_t  _pad;
    double   ident_cutoff;    /* CnsSeq.ident_cutoff (:14) */
    uint64_t ovlp_begin, ovlp_end;     /* its add_one_align calls, in call order: overlaps[ovlp_begin .. ovlp_end) */
    uint64_t range_begin, range_end;   /* its cov_ranges: pairs ranges[2 i], ranges[2 i + 1] */
} necat_cns_template;

typedef struct {
    uint64_t            n_templates;
    necat_cns_template* templates;
    uint64_t            n_overlaps;
    necat_cns_overlap*  overlaps;
    uint64_t            n_ranges;
    int32_t*            ranges;
    uint32_t            n_ops_blocks;
    uint8_t**           ops;           /* blocks of alignment columns (pinned host memory) */
    /* work counters */
    uint64_t            n_aligned;     /* alignments computed, speculative ones included */
    uint64_t            n_used;        /* alignments the sequential loop computes (cns_extension calls) */
    uint32_t            n_rounds;      /* device passes (one necat_onc_align_batch-like call each) */
    double              device_ms;     /* sum of the passes (HIP events, result copies included) */
    double              host_ms;       /* select + replay on the host */
    /* -r 1 */
    uint64_t            n_rescue_tried, n_rescued;   /* candidates handed to the pair / alignments it replaced */
    double              rescue_ms;     /* wall time of the pair over all passes (not part of host_ms) */
    /* the two halves of rescue_ms (the rest of it: picking the candidates, copying the columns) and who decided the global half */
    double              rescue_dalign_ms;    /* DALIGNER's local alignment: the host threads, or the device call (NECAT_DALIGN_DEVICE=1) */
    double              rescue_nw_ms;        /* edlib's global path over the ranges it found: the device call (NECAT_NW_DEVICE=1) or the host threads */
    uint64_t            n_rescue_nw;         /* candidates DALIGNER gave a range for: the jobs of the global half */
    uint64_t            n_rescue_nw_device;  /* of those, decided on the device (NECAT_NW_DEVICE=0: 0) */
    uint64_t            n_rescue_nw_host;    /* .. handed back to the host code by the device path (a self-check failure: 0 unless there is a bug) */
    /* who decided the local half (NECAT_DALIGN_DEVICE=0: both 0) */
    uint64_t            n_rescue_dalign_device;  /* candidates whose local alignment the device decided */
    uint64_t            n_rescue_dalign_host;    /* .. handed back to the host code: a window above NECAT_DALIGN_DIAGS diagonals, or a flagged job */
} necat_cns_result;

/* ---- the rescue pair's first half for many anchors at once: ocda_go (gapped_align/oc_daligner.c:36-79) on the device ------------
 * rescue::Dalign::go (necat_amd/csrc/rescue.h; Local_Alignment, gapped_align/align.c:1754 with low == hgh == the anchor's diagonal)
 * for n jobs on resident volumes: DALIGNER's furthest-reaching wave from (qstart, sstart) forward and backward - read qid of
 * `reads` on strand qdir (1 = its reverse complement; qstart on that strand) against sequence sid of `ref` (forward).  All state
 * is integers and the kernel follows the host statement rule for rule, so the results are equal, not close.  Ids are global
 * (-= read_start_id / ref_start_id).  One wave per job and direction, a lane per diagonal; the wave's window of diagonals may hold
 * NECAT_DALIGN_DIAGS (default 512; the widest measured are 333 for oc2cns and 511 for oc2rm_worker) - a job that outgrows it is recomputed by rescue::Dalign inside the
 * call (stats->n_over_cap), and so is a job that flags itself because a step met an empty window or read a diagonal without
 * history (the one case in which the two directions are not independent; never seen: stats->n_selfcheck).
 * res[i], in job order: ok (both ranges at least min_align_size long), how (0 = the device decided, 1 = the host code), the
 * ranges query [qoff, qend) and subject [soff, send) - filled also when ok is 0 - the difference count and, when ok,
 * ident_perc = 100 - 200 diffs / (both ranges' lengths).  error in (0, 1]; a bad job gives NECAT_ERR_ARG.  res: necat_free. */
typedef struct { int32_t qid, qdir, qstart, sid, sstart; } necat_dalign_job;
typedef struct { int32_t ok, how, qoff, qend, soff, send, diffs; double ident_perc; } necat_dalign_result;
typedef struct {
    uint64_t n_device;        /* jobs decided on the device (rejected ones included) */
    uint64_t n_host;          /* jobs handed to the host code = n_selfcheck + n_over_cap */
    uint64_t n_selfcheck;     /* .. because they flagged themselves */
    uint64_t n_over_cap;      /* .. because their window outgrew NECAT_DALIGN_DIAGS */
    uint64_t n_steps;         /* wave steps over all jobs and both directions */
    uint32_t max_diags;       /* the widest window a step began with */
    double   device_ms;       /* upload, launch and download (ends in a synchronise) */
    double   host_ms;         /* the rest of the call */
} necat_dalign_stats;
int  necat_local_align_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                             const necat_dalign_job* jobs, uint64_t n, double error, int min_align_size,
                             necat_dalign_result** res, necat_dalign_stats* stats);

/* ---- the rescue pair's second half for many ranges at once: edlib_go (edlib/edlib_wrapper.c:111-242) on the device -----------
 * rescue::EdlibGo::go (necat_amd/csrc/rescue.h) rule for rule, for n jobs on resident volumes: the global alignment of
 * query[qfrom, qto) - read qid of `reads` on strand qdir (1 = its reverse complement; coordinates on that strand) - with
 * subject[sfrom, sto) of sequence sid of `ref` (forward), accepted when its distance is at most `tolerance`
 * (consensus_aux.c:168-199 passes DALIGNER's diffs) and at most error * (sto - sfrom - 1) and the subject range is longer than
 * min_align_size; the path is the one edlib's NW mode returns - a problem whose traceback store stays under 1 MB is walked back
 * preferring up, then left, then the diagonal (obtainAlignmentTraceback, edlib.cpp:887), a larger one is split at the middle
 * column of the subject at the first query row where prefix and suffix cost add up to the optimum (obtainAlignmentHirschberg,
 * edlib.cpp:1177) - cut at both ends to the first run of match_size matches (4 in both callers, edlib_wrapper.c:177-229).
 * Every level of that recursion is one launch over all jobs' subproblems; the host sees one distance per score pass and
 * (row, left cost, right cost) per split.  Ids are global (-= read_start_id / ref_start_id).
 * res[i]: ok, the trimmed range (qoff .. tend in the coordinates the job was given in), align_size columns, their distance
 * and ident_perc; how = 0 decided on the device, 1 recomputed by rescue::EdlibGo inside the call because a leaf's self-check
 * failed (its path did not cost what the level above had found, or it asked for a cell outside the stored band): a bug
 * indicator, stats->n_selfcheck.  The columns, two bits each in the packing and codes of necat_onc_align_batch, at
 * ops + ops_off[i] (8-byte aligned, ops_off[n] = total bytes); necat_gapped_strings expands them.  There is no cap on the
 * band's width (rows go through 64 words at a time); ranges of 2^26 bases and more are refused (NECAT_ERR_ARG).
 * Leaf flags go through a per-context arena of at most NECAT_NW_POOL_MB, in chunks.  res / ops / ops_off: necat_free. */
typedef struct { int32_t qid, qdir, qfrom, qto, sid, sfrom, sto, tolerance; } necat_nw_job;
typedef struct {
    int32_t ok, how;
    int32_t qoff, qend, toff, tend;
    int32_t align_size, dist;
    double  ident_perc;
} necat_nw_result;
typedef struct {
    uint64_t n_device;        /* jobs decided on the device (rejected ones included) */
    uint64_t n_host;          /* jobs handed to the host code */
    uint64_t n_selfcheck;     /* jobs with a failed self-check (all of n_host: there is no other reason) */
    uint32_t n_levels;        /* recursion levels (launch rounds of score passes) */
    uint32_t n_leaf_chunks;   /* launches of the leaf kernel */
    uint64_t n_passes, n_splits, n_leaves;      /* score passes, split nodes, leaves over all jobs */
    double   device_ms;       /* wall time of all launches with their copies (each ends in a synchronise) */
    double   cols_ms, split_ms, leaf_ms, finish_ms;      /* .. by kernel */
    double   host_ms;         /* the rest of the call: planning the levels, packing the result */
} necat_nw_stats;
int  necat_nw_path_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                         const necat_nw_job* jobs, uint64_t n, double error, int min_align_size, int match_size,
                         necat_nw_result** res, uint8_t** ops, uint64_t** ops_off, necat_nw_stats* stats);

/* Order and cut of one partition file's candidates as oc2cns does it: records of one template together
 * (load_partition_candidates, consensus/consensus_one_partition.c:10-52), subject strand normalised to
 * forward (normalise_pcan_sdir, common/gapped_candidate.c:71-93), each template's candidates sorted by
 * PackedGappedCandidate_CnsScoreGT (gapped_candidate.c:95-121) and cut to MAX_EXAMINED_CAN = 300
 * (consensus_aux.h:15, consensus_one_read.c:250-260).  packed = n 28-byte PackedGappedCandidate records with
 * ids global in `reads`.  Outputs (necat_free each): cands; tmpl_off[n_templates + 1] (template t owns
 * cands[tmpl_off[t] .. tmpl_off[t+1])); n_all[n_templates] = candidates of the template before the cut. */
int  necat_cns_load_partition(necat_ctx* ctx, const necat_volume* reads, const void* packed, uint64_t n,
                              necat_candidate** cands, uint64_t** tmpl_off, uint64_t** n_all, uint64_t* n_templates);

/* cands: per template in examination order (as necat_cns_load_partition leaves them): sid = the template,
 * sdir = 0, ids global in `reads` (the merged read set, common/makedb_aux.c:137), qsize / ssize filled.
 * n_all may be NULL (= the counts given). */
int  necat_cns_extension_batch(necat_ctx* ctx, const necat_volume* reads, const necat_candidate* cands,
                               const uint64_t* tmpl_off, const uint64_t* n_all, uint64_t n_templates,
                               const necat_cns_options* opt, necat_cns_result** out);
void necat_cns_result_free(necat_cns_result* r);

/* ---- consensus stage (oc2cns), the consensus proper (tasc/cbcns.c: alignment tags -> backbone -> best path) -----------------
 * What consensus_one_read does with a template's add_one_align calls (consensus/consensus_one_read.c:373-395 -> consensus_broken /
 * consensus_unbroken, tasc/cbcns.c:108-264), for every template of one necat_cns_extension_batch result: the stretches covered at
 * least min_cov deep and at least 0.85 min_size long, each with the best-scoring path through its backbone, kept when that is
 * at least min_size bases.  Input: the result of necat_cns_extension_batch and the arrays that call was given.
 * path 0: on the device.  The device adds the weights of a link's tags in overlap-index order, the reference in the order its
 *   unstable sort leaves equal tags in; every device score carries a bound on the difference, and a template one of whose
 *   comparisons falls inside the bounds is recomputed by the host form inside the same call (on_host = 1, n_fallback).  The
 *   output is the host form's either way.
 * path 1: the host form (necat_amd/csrc/cns_consensus.h) on host_threads host threads; on_host = 1.
 * The host form reads query bases from host memory and a volume lives on the device: the reads its templates' overlaps name are
 *   copied back inside the call (path 1: in effect the volume, at 1 byte per base of host memory until the call returns).
 * Record text, the raw intervals between segments and the -f 1 stitching are the caller's (cns_consensus.h: emit_template). */
typedef struct {
    int min_cov;          /* -x 4   */
    int min_size;         /* -l 500 (>= 2) */
    int full_consensus;   /* -f 0: decides only what `corrected` means */
    int path;             /* 0 = device with certified fallback, 1 = host only */
    int host_threads;     /* threads of the host form and of the call's host loops; 0: NECAT_CNS_THREADS (oc2cns passes -t) */
} necat_cns_consensus_options;
void necat_cns_consensus_default_options(necat_cns_consensus_options* o);

typedef struct {
    int32_t  corrected;   /* the template counts as corrected: examined and (-f 0, or at least one segment) */
    int32_t  on_host;     /* computed by the host form (path 1, or handed back by the device path) */
    uint64_t seg_begin, seg_end;       /* its kept stretches, in template order: segments[seg_begin .. seg_end) */
} necat_cns_consensus_template;

typedef struct {
    int32_t  left, right;         /* the covered stretch [left, right) (consensus_broken's record range) */
    int32_t  cns_from, cns_to;    /* what the best path spans (consensus_unbroken's raw_from / raw_to) */
    uint64_t off;                 /* its consensus: bases[off .. off + len), base codes 0..3 */
    uint32_t len, _pad;
} necat_cns_segment;

typedef struct {
    uint64_t n_templates;
    necat_cns_consensus_template* templates;
    uint64_t n_segments;
    necat_cns_segment* segments;
    uint64_t n_bases;
    uint8_t* bases;
    uint64_t n_device;            /* examined templates whose output is the device's */
    uint64_t n_fallback;          /* examined templates the device path handed to the host (path 1: 0) */
    double   device_ms;           /* wall time of the device chunks: column upload, kernels, result download */
    double   host_ms;             /* wall time of the host form (path 1: everything) */
    double   tags_ms, sort_ms, backbone_ms, path_ms;      /* the kernels of the chunks (HIP events) */
    uint32_t n_chunks, _pad;
    uint64_t n_uncertain;         /* of n_fallback: handed back because a comparison fell inside the error bounds (the rest: bounds or arrays the
                                     analysis does not cover, sizes the key format cannot hold, or a NECAT_CNS_TOL_SCALE that makes the bounds too loose) */
} necat_cns_consensus;

/* reads / cands / tmpl_off / n_templates: as given to necat_cns_extension_batch, ext: what it returned.  *out is owned by the
 * result and released by necat_cns_consensus_free. */
int  necat_cns_consensus_batch(necat_ctx* ctx, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off,
                               uint64_t n_templates, const necat_cns_result* ext, const necat_cns_consensus_options* opt,
                               necat_cns_consensus** out);
void necat_cns_consensus_free(necat_cns_consensus* r);

/* ---- contig polishing (ctgcns), the consensus half (ctg_cns/fc_correct_one_read.c: alignment tags -> backbone -> best path; the splice of
 * ctg_cns/cns_ctg_subseq.c:212-233) -------------------------------------------------------------------------------------------
 * What cns_ctg_subseq does with one contig segment once its overlaps are chosen and aligned, for n_segments segments at once: the
 * consensus string with its case (lower: covered less than min_cov deep), the segment position of every consensus base, and - when
 * `contigs` is given - the polished segment: upper-case runs of at least min_run bases spliced into the raw bases.  The rule is
 * restated in necat_amd/csrc/ctg_consensus.h.  Every overlap weighs 1.0, so a link's weight is a count and both paths are exact:
 * path 0: tags, sort and the run boundaries (nodes, links, coverage) on the device, position range by position range under
 *   NECAT_CNS_TAG_BUDGET tags; the score pass, the traceback and the splice on the host over the downloaded nodes and links
 *   (DESIGN 6b).  There is no fallback: n_fallback is always 0.
 * path 1: the host form on host_threads threads, one segment per thread.
 * segment: contig id (a sequence of `contigs`; ignored without it), where the segment starts on the contig, its size (below 2^24)
 *   and its overlaps[ovlp_begin .. ovlp_end).  overlap: the read (global id: -= read_start_id), its strand (1 = reverse complement;
 *   qoff / qend on that strand), the range on the segment (toff / tend relative to `from`), align_size columns at ops + ops_off, two
 *   bits each in the packing and codes of necat_onc_align_batch - what the aligners and necat_nw_path_batch emit passes unchanged.
 * NECAT_ERR_ARG with a message, never a wrong answer: an overlap whose columns do not add up to its coordinates, an overlap that
 *   leaves its read or its segment (a query base in front of the segment's first base included), a segment of 2^24 bases or more. */
typedef struct { int32_t ctg_id, size; int64_t from; uint64_t ovlp_begin, ovlp_end; } necat_ctg_segment;
typedef struct { int32_t qid, qdir, qoff, qend, toff, tend, align_size, _pad; uint64_t ops_off; } necat_ctg_overlap;
typedef struct {
    int min_cov;          /* 4 (MIN_CNS_COV) */
    int min_run;          /* 1000 */
    int path;             /* 0 = device, 1 = host */
    int host_threads;     /* threads of the host path and of the call's host loops; 0: NECAT_CNS_THREADS */
} necat_ctg_consensus_options;
void necat_ctg_consensus_default_options(necat_ctg_consensus_options* o);
typedef struct {
    uint64_t cns_off, cns_len;             /* cns[cns_off .. + cns_len), t_pos likewise */
    uint64_t polished_off, polished_len;   /* polished[..]; 0, 0 without `contigs` */
    uint64_t n_tags, n_nodes, n_links;
    uint32_t n_chunks, _pad;               /* position ranges the segment was processed in (path 1: 0) */
} necat_ctg_consensus_segment;
typedef struct {
    uint64_t n_segments;
    necat_ctg_consensus_segment* segments;
    uint64_t n_cns;
    char*    cns;                 /* consensus characters with case */
    int32_t* t_pos;               /* the segment position of each */
    uint64_t n_polished;
    char*    polished;
    uint64_t n_fallback;          /* segments the device path did not compute itself: always 0 */
    uint32_t n_chunks, _pad;
    double   device_ms;           /* wall time of the ranges on the device: upload, kernels, download */
    double   tags_ms, sort_ms, links_ms;      /* .. the kernels (HIP events) */
    double   plan_ms;             /* checking the overlaps and planning the ranges (host) */
    double   score_ms;            /* score pass, traceback and splice (host) */
    double   host_ms;             /* path 1: the whole host form */
} necat_ctg_consensus;
int  necat_ctg_consensus_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs /* may be NULL */,
                               const necat_ctg_segment* segments, uint64_t n_segments, const necat_ctg_overlap* overlaps,
                               const uint8_t* ops, const necat_ctg_consensus_options* opt, necat_ctg_consensus** out);
void necat_ctg_consensus_free(necat_ctg_consensus* r);

/* ---- contig polishing (ctgcns), the seeding (ctg_cns/mem_finder.c, ctg_cns/chain_dp.c) ----------------------------------------------
 * What extend_ctg_m4s does first with every read-to-contig record (cns_ctg_subseq.c:157-161), for every job of every segment at
 * once: MaximalExactMatchWorkData_FindCandidates of the read on its strand against the segment - sampled 15-mers of the read looked up
 * among all of the segment's, the product rule on occurrences, extension to maximal exact matches of at least 20 bases, the chain -
 * and of its result can_list[0], or "none".  The rule, its quirks included, is restated in necat_amd/csrc/ctg_seed.h.  A job does not
 * depend on the coverage state of the program's loop, so a caller may seed every record of a segment ahead of that loop.
 * path 0: a table of the segment's 15-mers and one wave per job on the device; the chain's arrays of a job with at most
 *   NECAT_CTG_SEED_LDS matches live in LDS, of a larger one in the call's scratch; jobs run in chunks of at most NECAT_CTG_SEED_BUDGET
 *   seeds, and a job with more seeds than that - or than NECAT_CTG_SEED_JOB_MAX - is computed by the host form inside the call and
 *   counted in n_fallback.
 * path 1: the host form on host_threads threads.  One index per segment is shared by its jobs on both paths; the outputs are equal.
 * segment: a necat_ctg_segment whose ovlp_begin .. ovlp_end index `jobs`; `contigs` is required, the segment is bases from .. from +
 *   size of sequence ctg_id, read where they lie.  job: the read (global id: -= read_start_id) and its strand (1 = reverse complement).
 * All coordinates of the result are relative to the segment; qsize, ssize, ids and directions of a candidate are the caller's.
 * NECAT_ERR_ARG with a message, never a wrong answer: a segment of 2^24 bases or more, of fewer than 15 bases (the reference reads an
 *   empty list's storage there), or one that leaves its contig; a read id outside the volume; a read of 2^30 bases or more. */
typedef struct { int32_t qid, qdir; } necat_ctg_seed_job;
typedef struct {
    int path;             /* 0 = device, 1 = host */
    int host_threads;     /* threads of the host path and of the fallback; 0: NECAT_CNS_THREADS */
    int keep_mems;        /* != 0: the result holds every job's sorted matches */
    int _pad;
} necat_ctg_seed_options;
void necat_ctg_seed_default_options(necat_ctg_seed_options* o);
typedef struct { int32_t qoff, soff, size; } necat_ctg_seed_mem;
typedef struct {
    int32_t  found;                                          /* 0: can_list was empty, the seven numbers are 0 */
    int32_t  qbeg, qend, sbeg, send, qoff, soff, score;      /* can_list[0] */
    uint32_t n_matches;                                      /* seeds before extension */
    uint32_t n_mems;                                         /* maximal exact matches of at least 20 bases that went into the chain */
    int32_t  chain_len;                                      /* matches of the candidate's chain */
    int32_t  how;                                            /* who decided: 0 device (chain in LDS), 1 device (chain in scratch), 2 the host form */
    uint64_t mems_off;                                       /* keep_mems: mems[mems_off .. + n_mems), sorted by (soff, qoff) */
} necat_ctg_seed_result;
typedef struct {
    uint64_t n_jobs;                  /* the largest ovlp_end; a job no segment names stays all zero */
    necat_ctg_seed_result* jobs;
    uint64_t n_mems;
    necat_ctg_seed_mem* mems;         /* keep_mems only */
    uint64_t n_fallback;              /* jobs of path 0 the host form computed */
    uint64_t n_lds, n_scratch;        /* jobs of path 0 by the tier of their chain */
    uint32_t max_matches, max_mems;   /* the largest of a job */
    double   index_ms, match_ms, chain_ms;      /* the kernels (HIP events): the segments' tables; counting, seeds and matches; chains */
    double   device_ms;               /* wall time of path 0's device part: uploads, kernels, downloads */
    double   host_ms;                 /* path 1: the whole host form; path 0: the fallback jobs */
} necat_ctg_seed;
int  necat_ctg_seed_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs,
                          const necat_ctg_segment* segments, uint64_t n_segments, const necat_ctg_seed_job* jobs,
                          const necat_ctg_seed_options* opt, necat_ctg_seed** out);
void necat_ctg_seed_free(necat_ctg_seed* r);

/* ---- contig polishing (ctgcns), the aligner and the coverage cap (ctg_cns/cns_ctg_subseq.c:17-197) -----------------------------------
 * The middle of extend_ctg_m4s: what turns necat_ctg_seed_batch's candidates into the overlaps necat_ctg_consensus_batch takes.  For
 * every job (a read-to-contig record) of every segment: cns_extension of can_list[0] against the SEGMENT's bases (min_align_size
 * 1000, error 0.5, rescue on) - the block-wise aligner with columns kept and tail length 4, and where that fails or stops more than
 * 200 bases short of the chained range, DALIGNER around the anchor and edlib's path over its range - all of them ahead of the loop;
 * then, per segment and in the order of its jobs (the program sorts by soff, the entry does not), the loop itself on the host: the
 * cap (fewer than 200 positions of the record's range below 10 deep: skipped), the accept rule (ident_perc >= 90 and at least 0.6
 * of the read aligned; the reference's second alternative is never true and is kept that way) and the counters over the accepted
 * alignment's own range.  The rule is restated in necat_amd/csrc/ctg_extend.h.  All coordinates are relative to the segment.
 * jobs: the read (global id: -= read_start_id), its strand (1 = reverse complement) and the record's range soff .. send on the contig.
 * seeds: the result of necat_ctg_seed_batch over the same segments and jobs; NULL: the entry makes that call at its defaults.
 * opt: cap 1 = the loop, 0 = no loop: every job's alignment is reported and every accepted one is an overlap; rescue_path 0 = the
 *   pair on the device (the kernels of necat_local_align_batch and necat_nw_path_batch on slices of the resident contig), 1 =
 *   the host code on host_threads threads over the fetched bases.  Both give equal results.
 * out: per job the verdict, who decided, the alignment (none for a job the cap skipped) and the index of its overlap or -1; the
 *   overlaps with their packed columns in loop order and a copy of `segments` whose ovlp_begin .. ovlp_end index them: the three
 *   arrays pass into necat_ctg_consensus_batch unchanged.
 * NECAT_ERR_ARG with a message, never a wrong answer: a record that ends at or before its segment's start (the reference asserts), a
 *   read id outside the volume, a strand that is neither 0 nor 1, a job two segments name, a segment that leaves its contig, of 2^24
 *   bases or more or of fewer than 15, a seed table whose n_jobs is not this call's, and - rescue_path 0 - a segment that ends 2^31 bases
 *   or more into its contig. */
typedef struct { int32_t qid, qdir; int64_t soff, send; } necat_ctg_extend_job;
typedef struct {
    int cap;              /* 1 = the loop with its coverage cap, 0 = every job */
    int rescue_path;      /* 0 = device, 1 = host */
    int host_threads;     /* threads of the host loops; 0: NECAT_CNS_THREADS */
    int _pad;
} necat_ctg_extend_options;
void necat_ctg_extend_default_options(necat_ctg_extend_options* o);
#define NECAT_CTG_EXT_CAPPED       0   /* the cap skipped the record: no alignment is reported */
#define NECAT_CTG_EXT_NO_SEED      1
#define NECAT_CTG_EXT_NO_ALIGNMENT 2
#define NECAT_CTG_EXT_REJECTED     3   /* aligned, but not by the accept rule */
#define NECAT_CTG_EXT_ACCEPTED     4
typedef struct {
    int32_t state;                                /* NECAT_CTG_EXT_* */
    int32_t decided;                              /* 0 none, 1 the block-wise aligner, 2 the pair, 3 the block-wise result kept after the pair failed */
    int32_t qoff, qend, toff, tend, align_size;   /* on the read's strand / relative to the segment */
    int32_t _pad;
    double  ident_perc;
    int64_t overlap;                              /* index into overlaps, -1: none */
} necat_ctg_extend_result;
typedef struct {
    uint64_t n_jobs;                  /* the largest ovlp_end; a job no segment names stays all zero with overlap -1 */
    necat_ctg_extend_result* jobs;
    uint64_t n_segments;
    necat_ctg_segment* segments;      /* the call's, ovlp_begin .. ovlp_end indexing `overlaps` */
    uint64_t n_overlaps;
    necat_ctg_overlap* overlaps;      /* loop order, segment by segment */
    uint64_t n_ops;
    uint8_t* ops;                     /* their columns, 8-byte aligned each */
    uint64_t n_seeded;                /* jobs with a candidate */
    uint64_t n_aligned;               /* jobs whose cns_extension was computed (all seeded ones: ahead of the loop) */
    uint64_t n_used;                  /* jobs the loop reached cns_extension with: the reference's "extended m4" */
    uint64_t n_pair_tried, n_pair_accepted;
    uint64_t n_dalign_device, n_dalign_host, n_dalign_over_cap, n_dalign_selfcheck;
    uint64_t n_nw_jobs, n_nw_device, n_nw_host;
    uint64_t cols_bytes_downloaded;   /* column bytes of every aligned job */
    uint64_t cols_bytes_used;         /* .. of the overlaps */
    double   seed_ms, align_ms, rescue_ms, replay_ms;      /* wall times: the seeding call (0 with `seeds`), the block-wise aligner, the pair, the loop with the gather of its columns */
} necat_ctg_extend;
int  necat_ctg_extend_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs,
                            const necat_ctg_segment* segments, uint64_t n_segments, const necat_ctg_extend_job* jobs,
                            const necat_ctg_seed* seeds /* may be NULL */, const necat_ctg_extend_options* opt, necat_ctg_extend** out);
void necat_ctg_extend_free(necat_ctg_extend* r);

/* ---- the candidate partitioner of the consensus stage ------------------------------------------
 * <- partition_candidates/pcan.c:39-103 for candidates that are still in this process (what necat_find_candidates just
 * returned), instead of the write + read of the candidates file: every candidate is offered as it is (template = its subject)
 * and with the roles exchanged (change_pcan_roles, common/gapped_candidate.c:54-69); partition i holds the records whose
 * template id lies in [i * batch_size, (i + 1) * batch_size), i < num_parts = ceil(num_reads / batch_size).  Outputs (necat_free
 * both): records = 28-byte PackedGappedCandidate records (7 x uint32), grouped by partition, in no particular order inside one
 * (as in the reference); part_off[num_parts + 1] in records. */
int  necat_pcan_partition(necat_ctx* ctx, const necat_candidate* cands, uint64_t n, int batch_size, int num_reads,
                          uint32_t** records, uint64_t** part_off, int* num_parts);

/* ---- the read trimming stage on records ------------------------------------------------------------
 * <- trim_bases/pm4_aux.c:129-196 (oc2pm4) and trim_bases/largest_cover_range.c:290-325 + largest_cover_range_main.c:43-52 (oc2lcr), for
 * the binary M4 records `oc2asmpm -u 1` wrote.  Read ids are 0 .. num_reads + 1 (the reference's table has num_reads + 2 rows; reads are
 * numbered from 1).
 *
 * necat_trim_partition: a record with ident_perc >= min_ident_perc is kept under its subject as it is and, with query and subject
 * exchanged and the new subject on the forward strand (fix_asm_m4_offsets), under its query; the records are then grouped by
 * subject id.  The groups stay on the device for necat_trim_ranges.  Optional outputs (necat_free both): the grouped records, in no
 * particular order inside a read, and read_off[num_reads + 3] (read i owns [read_off[i], read_off[i + 1])).
 *
 * necat_trim_ranges: one range per read id, out[num_reads + 2] (caller's memory), final pass included (a read without a range, or with
 * one shorter than min_size, has left = -1).  grouped / read_off: records grouped by subject id as above, or both NULL = the groups the
 * last necat_trim_partition of this context left on the device.  how == NECAT_TRIM_HOST (left = -1, right = size = 0): the read is
 * not decided here, because the reference's answer for it depends on the order it held the records in - a record below
 * min_ident_perc, more than 300 records, or two records with the same (qid, qdir) and the same largest vscore in a pair the chimera
 * test evaluates; the caller decides it with necat_amd/csrc/trim_core.h on the records in partition-file order.  *n_host = their number. */
#define NECAT_TRIM_NONE     0   /* no record, or no covered range */
#define NECAT_TRIM_COMPLETE 1   /* one overlap spans the read (is_complete_read) */
#define NECAT_TRIM_CHIMERIC 2   /* is_chimeric_read */
#define NECAT_TRIM_COVER    3   /* largest_cover_range */
#define NECAT_TRIM_HOST     4
typedef struct { int32_t left, right, size, how; } necat_clip_range;
int  necat_trim_partition(necat_ctx* ctx, const necat_m4* recs, uint64_t n, int num_reads, double min_ident_perc,
                          necat_m4** grouped, uint64_t** read_off, uint64_t* n_grouped);
int  necat_trim_ranges(necat_ctx* ctx, const necat_m4* grouped, const uint64_t* read_off, int num_reads, double min_ident_perc,
                       int min_ovlp_size, int min_cov, int min_size, necat_clip_range* out, uint64_t* n_host);

/* ---- one reference volume on several GPUs (fine granularity) -------------------------------------
 * The reference parallelises ONE volume over threads that pull 500-read chunks from a counter
 * (pm_worker.c:13,354-362; common/map_aux.c:59-77) against one shared lookup table.  The multi-GPU equivalent:
 * one process per GPU (rank), every rank holds the volume,
 *   - the index is built in hash-range slices - rank g counts, filters and ranks only the k-mers whose hash falls
 *     in its range of the 4^k table - and the slices of the table / of offset_list are all-gathered (starts already
 *     final: shifted by the exclusive scan of the slice sizes before they are written), so every rank ends up with the
 *     COMPLETE index (necat_index_download gives the reference-layout arrays): necat_index_build_sharded;
 *   - the query reads are dealt out in chunks of `chunk_reads` reads, chunk c to rank c % nranks (reads late in the
 *     volume see more subjects - word_finder.c:121-127 - so contiguous ranges would not balance); every read is
 *     processed exactly as on one GPU, so the union of the ranks' records IS the single-GPU record set;
 *   - the records are gathered (gather-v, device to device) on rank `root`.
 * Device memory moves by RCCL send/recv groups (direct all-pairs over xGMI) or, for ranks that share a device,
 * by HIP IPC copies (transport "ipc"; "auto" picks RCCL unless two ranks sit on one device).  Small host-side
 * values (slice sizes, the RCCL id, IPC handles) travel through the caller's all-gather callback. */

/* all-gather of `bytes` bytes per rank among the job's ranks: recv = nranks * bytes, rank order; returns 0 on success */
typedef int (*necat_host_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);

int  necat_comm_create(necat_ctx* ctx, int rank, int nranks, necat_host_allgather_fn fn, void* user,
                       const char* transport /* "auto" | "rccl" | "ipc" */, necat_comm** out);
void necat_comm_destroy(necat_comm* c);
/* "rccl" or "ipc" */
int  necat_comm_transport(const necat_comm* c, char* buf, size_t n);

/* wall-clock of the last sharded calls on this rank */
typedef struct {
    double   index_local_ms;     /* this rank's slice of the build (HIP events) */
    double   index_exchange_ms;  /* all-gather of the table and offset_list slices (wall) */
    uint64_t index_exchange_bytes; /* bytes this rank received */
    double   gather_ms;          /* gather-v of the records on the root (wall) */
    uint64_t gather_bytes;
    uint64_t reads_local;        /* query reads this rank processed */
    /* how the last necat_index_build_sharded built its index: 1 = hash-range slices + all-gather, 0 = every rank built the whole table (no
     * exchange), and the two costs necat_index_plan priced for it */
    uint64_t index_sharded;
    double   index_plan_replicate_ms, index_plan_shard_ms;
} necat_shard_timings;
int  necat_get_shard_timings(const necat_ctx* ctx, necat_shard_timings* t);
int  necat_get_shard_timings_sized(const necat_ctx* ctx, void* t, size_t bytes);

/* The cost model behind necat_index_build_sharded's choice (no reference counterpart: build_lookup_table, lookup_table.c:149, is one thread).
 * SURVEY 8e's sharded build was specified against a 66 s CPU build; on the device ONE rank builds an E. coli-size table in 5 ms, so slicing the build
 * pays only when (build time saved) > (time to move the other ranks' slices over the links):
 *     replicate_ms = (scan + work) nbases
 *     shard_ms     = scan nbases + work nbases / nranks + 3 exchanges' latency + bytes / nranks / link rate
 * with scan = the passes every rank makes over ALL bases (k_part_hist, k_split_bases), work = the passes that shrink with the rank's hash range
 * (both measured on MI355X: 6.0 / 22.3 ps per base - 5.2 ms at 184 Mbp, 58 ms at 2.0 Gbp), bytes = the sparse table words + 8 per distinct k-mer +
 * 8 per offset, every peer's slice on its own xGMI link (direct all-pairs groups).  link_gbs <= 0: NECAT_XGMI_GBS or 100 (of a link's nominal 153).
 * NECAT_INDEX_SHARD=0 / 1 overrides the choice (tests run both); every rank computes the same plan from the same arguments. */
typedef struct {
    int32_t  shard;              /* 1: slices + all-gather is the cheaper plan */
    int32_t  _pad;
    double   replicate_ms, shard_ms, exchange_ms;
    uint64_t exchange_bytes;     /* all ranks' slices together */
} necat_index_plan_t;
int  necat_index_plan(uint64_t nbases, int kmer_size, int nranks, double link_gbs, necat_index_plan_t* out);

/* Test hook: runs the RCCL transport's call path (librccl opened at run time, communicator, send/recv group on the context's
 * stream) with ONE rank sending `bytes` bytes to itself, and compares them. */
int  necat_comm_selftest_rccl(necat_ctx* ctx, uint64_t bytes);
/* The same between TWO devices: rank 0 on the context's device, rank 1 on another one of this process, each sends `bytes` to the other and
 * checks what it received (one ncclSend / ncclRecv group per rank, comm.h's exchange pattern).  Returns 1 (and no error) when the box has fewer
 * than two devices - a test skips then, with that reason. */
int  necat_comm_selftest_rccl2(necat_ctx* ctx, uint64_t bytes);

/* necat_index_build with the work split by hash range and the result all-gathered: the returned index is the
 * complete one, bit-identical to necat_index_build's, on every rank.  Collective: every rank of `comm` calls it.
 * (k < 11 - tables that fit the L2 - are simply built whole on every rank.) */
int  necat_index_build_sharded(necat_ctx* ctx, necat_comm* comm, const necat_volume* ref, int kmer_size, int max_occ,
                               necat_index** out);

/* necat_find_candidates / necat_map_pair for this rank's chunks of the query reads, then the gather-v on `root`.
 * On the root: out = the records of ALL ranks (this rank's first), *n_out their number.  On the other ranks: out =
 * this rank's own records.  *n_local (optional) = this rank's own records, *n_candidates its candidates examined.
 * Collective. */
int  necat_find_candidates_sharded(necat_ctx* ctx, necat_comm* comm, const necat_index* ix, const necat_volume* ref,
                                   const necat_volume* reads, int read_start_id, int ref_start_id, int pairwise,
                                   const necat_map_options* opt, int chunk_reads, int root,
                                   necat_candidate** out, uint64_t* n_out, uint64_t* n_local);
int  necat_map_pair_sharded(necat_ctx* ctx, necat_comm* comm, const necat_index* ix, const necat_volume* ref,
                            const necat_volume* reads, int read_start_id, int ref_start_id, int pairwise,
                            const necat_map_options* opt, int tail_match_len, int chunk_reads, int root,
                            necat_m4** out, uint64_t* n_out, uint64_t* n_local, uint64_t* n_candidates);

/* ---- several volumes on several GPUs (both granularities combined; BASELINE configs[3] / [4]) ---------------------
 * <- the job list of pm_main (pm_worker.c:372-390: reference volume v against query volumes v .. V - 1) and its distribution
 * over grid nodes (necat.pl:190-202), re-cut for the GPUs of one node.  The V (V + 1) / 2 (reference, query) pairs are laid end to
 * end on one cost line (cost ~ bases(query) x bases(reference), halved for the self pair) and rank g takes the g-th of nranks equal
 * stretches; a pair a boundary cuts through is split by query reads - chunks of `chunk_reads` reads, chunk c in slot c % slots, a
 * rank takes a contiguous slot range (necat_amd/csrc/pair_sched.h).  A rank's units are consecutive pairs, so it touches few
 * reference volumes, in ascending order, and the ranks of one reference volume are consecutive ranks: team_lo[v] .. team_hi[v]
 * (inclusive).  A team of several ranks builds that volume's index with necat_index_build_sharded over a communicator of the team.
 * Host-only arithmetic (no device is touched).  Outputs (necat_free each): units = all ranks' units, rank by rank;
 * rank_off[nranks + 1]; team[2 * num_volumes] = (team_lo, team_hi) per reference volume. */
typedef struct { int32_t ref_vol, query_vol, slot_lo, slot_hi; } necat_pair_unit;
/* query reads per chunk for a query volume of `query_reads` reads: 64, fewer for small volumes so that every slot gets several chunks */
int  necat_pair_chunk_reads(uint64_t query_reads, int slots);
int  necat_pair_schedule(const uint64_t* vol_bases, int num_volumes, int nranks, int slots,
                         necat_pair_unit** units, uint64_t** rank_off, int32_t** team);

/* necat_find_candidates / necat_map_pair for ONE share of a pair: only the query chunks c (of chunk_reads reads) with
 * slot_lo <= c % slots < slot_hi are processed, each read exactly as in a whole-pair call - the union of the shares [0, slots) IS the
 * whole pair's record set.  No collective; the records come back on the host as from the whole-pair calls. */
int  necat_find_candidates_part(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                                int read_start_id, int ref_start_id, int pairwise, const necat_map_options* opt,
                                int chunk_reads, int slot_lo, int slot_hi, int slots,
                                necat_candidate** out, uint64_t* n_out);
int  necat_map_pair_part(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                         int read_start_id, int ref_start_id, int pairwise, const necat_map_options* opt, int tail_match_len,
                         int chunk_reads, int slot_lo, int slot_hi, int slots,
                         necat_m4** out, uint64_t* n_out, uint64_t* n_candidates);

/* Test / profiling hook for the dominant kernel: n independent Edlib_align calls
 * (edlib_ex.c:733) on byte-coded (0..3) sequences.  seqs = concatenated fragments, q_off/t_off =
 * start of each fragment in `seqs`.  Outputs per block: edit distance (-1 = fail), qend, tend, and
 * the alignment as one op per column (0 match, 1 ins(query base vs gap), 2 del, 3 mismatch) in
 * forward order, ops_off[i]..ops_off[i+1]. */
int  necat_edlib_align_batch(necat_ctx* ctx, const uint8_t* seqs, uint64_t seqs_len,
                             const uint64_t* q_off, const int32_t* q_len,
                             const uint64_t* t_off, const int32_t* t_len, uint64_t n, double error,
                             int32_t* dist, int32_t* qend, int32_t* tend,
                             uint8_t** ops, uint64_t** ops_off);

int  necat_get_timings(const necat_ctx* ctx, necat_timings* t);
/* the first min(bytes, sizeof(necat_timings)) bytes of the timings: safe for a caller built against an older (smaller) struct */
int  necat_get_timings_sized(const necat_ctx* ctx, void* t, size_t bytes);
/* The value a context holds for one of the library's NECAT_* tuning / test knobs, as text (a number; the text itself for NECAT_COMM and NECAT_ASM_DUMP_VOTES; "" for a
 * knob that only asks whether it is set and is not; the pool sizes given in MB come back in bytes).  A context reads the knobs from the environment ONCE, in
 * necat_ctx_create: this is how a caller checks that the setting it exported took.  NECAT_ERR_ARG: not a knob of a context (INTEGRATION.md lists them). */
int  necat_knob_get(const necat_ctx* ctx, const char* name, char* buf, size_t n);
void necat_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* NECAT_HIP_H */
