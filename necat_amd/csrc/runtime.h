// runtime.h - host-side plumbing of libnecat_hip.so: context, error capture, grow-only device
// buffers, HIP event timers.  No torch types, no CPU fallback: every failure is reported.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/necat_hip.h"
#include "knobs.h"
#include "dev_common.h"
#include "stage_arenas.h"

namespace necat {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

}  // namespace necat

constexpr int kNumEvents = 48;
// Who owns which of a context's events (necat_ctx::ev; ExtLane1::ev of the lanes 1 .. uses the extension's names the same way).  Two edges that can be in
// flight together never share an index: the ranges below are disjoint, the one declared alias excepted.
enum EventId {
    EV_CALL_BEGIN = 0, EV_CALL_END = 1,            // index, seed, extend, asm stages: begin / end of the call (the *_ms timings)
    EV_ASM_A0 = 2, EV_ASM_A1 = 3,                  // stage_asm_align.inl, list A: pass begins / pass ends (walk ends: EV_ASM_A2)
    EV_A0 = 4, EV_A1 = 5, EV_A2 = 6,               // stage_extend.inl: a0 / a1 / a2 of list buffer j < 4 at + kEvListStride * j
    EV_EDLIB_A0 = EV_A0, EV_EDLIB_A1 = EV_A1, EV_EDLIB_A2 = EV_A2,      // ALIAS - stage_edlib_batch.inl: the hook's fragments / pass / walk (never beside an extension on that context)
    EV_COLS_READY = 16, EV_COLS_COPIED = 17,       // stage_extend.inl, alignment-keeping mode: columns ready for the copy stream / copy finished (copy_pending)
    EV_B0 = 18, EV_B1 = 19, EV_B2 = 20,            // stage_extend.inl: b0 / b1 / b2 of list-B slot j < 2 at + kEvListStride * j
    EV_ASM_A2 = 24,                                // stage_asm_align.inl, list A: walk ends
    EV_SIDE_CHAIN = 25,                            // stage_extend_xcheck.inl: the band-kernel side chain on stream d (ragged via k_myers_coop, wide blocks) finished
    EV_RC_WALK_END = 26,                           // stage_extend.inl: end of the recompute walk of round r at + (r & 3)
    EV_RAGGED_WALKED = 30,                         // stage_extend.inl: the un-merged ragged chain on stream d has been walked
    EV_LANE_RESULT = 31,                           // stage_extend.inl, lane scheduler: the lane's k_ext_result finished
    EV_ASM_FORK = 34, EV_ASM_JOIN = 35,            // stage_asm_align.inl: fork to / join from stream B
    EV_ASM_B0 = 36, EV_ASM_B1 = 37, EV_ASM_B2 = 38,        // stage_asm_align.inl, list B: pass begins / pass ends / walk ends
    EV_PIPE_PIECE = 40,                            // stage_extend.inl (NECAT_RC_PIPE): piece ci at + (ci & 7): pass done, its walk may start
};                                                 // (32, 33, 39: unused)
constexpr int kEvListStride = 3, kEvRcRounds = 4, kEvPipePieces = 8;
struct EvRange { int first, count; };
constexpr EvRange kEvRanges[] = {{EV_CALL_BEGIN, 2}, {EV_ASM_A0, 2}, {EV_A0, kEvListStride * 4}, {EV_COLS_READY, 2}, {EV_B0, kEvListStride * 2}, {EV_ASM_A2, 1}, {EV_SIDE_CHAIN, 1},
                                 {EV_RC_WALK_END, kEvRcRounds}, {EV_RAGGED_WALKED, 1}, {EV_LANE_RESULT, 1}, {EV_ASM_FORK, 2}, {EV_ASM_B0, 3}, {EV_PIPE_PIECE, kEvPipePieces}};
constexpr bool ev_ranges_disjoint() { int end = 0; for (const EvRange& r : kEvRanges) { if (r.first < end) return false; end = r.first + r.count; } return end <= kNumEvents; }
static_assert(ev_ranges_disjoint(), "two owners of one event index, or a range past kNumEvents (kEvRanges is in ascending order)");
static_assert(EV_CALL_END == EV_CALL_BEGIN + 1 && EV_ASM_A1 == EV_ASM_A0 + 1 && EV_A2 == EV_A0 + 2 && EV_B2 == EV_B0 + 2 && EV_COLS_COPIED == EV_COLS_READY + 1 &&
              EV_ASM_JOIN == EV_ASM_FORK + 1 && EV_ASM_B2 == EV_ASM_B0 + 2 && EV_EDLIB_A0 == EV_A0 && EV_EDLIB_A2 == EV_A2, "the ranges above are these names' ranges");
constexpr unsigned kRoundRing = 1024;  // entries of necat_ctx::round_ring per lane (the ring holds kMaxExtLanes lanes' worth)
constexpr int kMaxExtLanes = 4;        // lanes of the extension rounds: the context's own set + up to three ExtLane1 (NECAT_EXT_LANES, default 2)

// The second lane of the extension rounds (stage_extend.inl, ExtLane): while one batch of candidates is in its last, latency-bound rounds
// the next batch runs its first, chip-filling ones beside it - on buffers, streams, events and a ring half of its own.  Lane 0 is the
// context's own set (scratch[SC_EXT_*], stream_a .. stream_d, ev[]); this is lane 1, created the first time two batches overlap.
struct ExtLane1 {
    necat::DevBuf buf[16];             // by role: ExtLaneBuf in stage_extend.inl
    hipStream_t st[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev[kNumEvents] = {};    // (null = not created: ext_lane creates the missing ones, necat_ctx_destroy destroys the others)
    unsigned long long round_seq = 0;
    bool ready = false;
};

struct necat_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream_a = nullptr, stream_b = nullptr;   // extension rounds: list A / list B run concurrently (NECAT_STREAM_GRAPH=1, the default: stream_a IS `stream`)
    hipStream_t stream_c = nullptr;                       // second list-B stream (small lists alternate; NECAT_LISTB_STREAMS=1: stream_b again)
    hipStream_t stream_d = nullptr;                       // list A's ragged / wide blocks of a round whose full blocks run through ext_rcwalk.h (NECAT_STREAM_GRAPH=1: only where the knobs select such a path)
    bool serial_streams = false;                          // NECAT_SERIAL=1: stream_a .. stream_d are aliases of `stream`
    bool graph_streams = false;                           // NECAT_STREAM_GRAPH=1 and not NECAT_SERIAL: necat_ctx_create made the streams (ctx_streams, necat_hip.hip), in a fixed order
    bool need_stream_d = true;                            // .. and whether a path of this context's knobs launches on stream_d (lanes 1 .. make theirs by the same rule)
    hipStream_t stream_copy = nullptr;                    // deferred device-to-host copies (alignment columns of the consensus loop)
    bool copy_pending = false;                            // a copy on stream_copy still reads SC_EXT_COLS_OUT (ev[EV_COLS_COPIED] marks its end)
    char err[1024] = {0};
    necat_timings tm;
    necat_shard_timings shard_tm;      // last sharded calls (necat_index_build_sharded, necat_*_sharded)
    hipEvent_t ev[kNumEvents];
    void* pin_plan = nullptr; size_t pin_plan_cap = 0;   // pinned host scratch of the seeding plan (hit counts down, order + scratch layout up)
    void* round_ring = nullptr;        // pinned, device-visible ring of RoundPub entries: list sizes published by the round kernels
    void* round_ring_dev = nullptr;    // the same memory as the device addresses it
    unsigned long long round_seq = 0;  // rounds published so far (the next round publishes round_seq + 1)
    necat::DevBuf scratch[64];         // grow-only arenas, indexed by purpose (ScratchId; SC_COUNT <= 64)
    uint64_t scratch_live = 0;         // bit i: a call in progress holds pointers into scratch[i] (necat::ArenaUse) - buf_ensure_lend never hands such an arena to another phase
    void* seed_ht_ptr = nullptr;       // the seeding hash arena (SC_SEED_HT) whose first seed_ht_clean bytes are known to be all-empty (0xFF):
    size_t seed_ht_cap = 0;            // .. and its capacity when that was established (a reallocation at the same address is a new arena)
    size_t seed_ht_clean = 0;          // every call leaves the arena as it found it (k_seed_clear resets the slots it used), so it is filled once per allocation
    char devname[256] = {0};
    int num_cu = 0;
    uint32_t epoch = 0;
    void* cns_scratch = nullptr;       // host buffers of the consensus loop kept between calls (necat::cns::Scratch)
    necat::Knobs knobs;                // this context's tuning / test knobs (knobs.h: read from the environment in necat_ctx_create)
    necat::DevBuf idx_cache[4];        // released index arrays (table, offset list) kept for the next build (8.6 GB hipMalloc/hipFree per step otherwise): [0], [1] of the builds with dense
                                       // bases, [kIdxCacheHoles], [+ 1] of the builds with record-space bases.  Apart, because a sharded build publishes its arrays to its peers (HIP IPC) and a
                                       // context of the pair scheduler runs both kinds: with the bigger record-space table in the one cache, the sharded build of the next step adopted it and
                                       // hipIpcGetMemHandle / the peer copy failed with "invalid argument" (tests/test_gpu_pairs.py, two ranks) - it publishes only what a build of its own kind allocated
    ExtLane1 lanex[kMaxExtLanes - 1];  // lanes 1 .. of the extension rounds (each created on first use)
    int trim_nids = 0;                 // necat_trim_partition left the records of this many read ids grouped in scratch[SC_TRIM_RECS] / [SC_TRIM_OFF] (0: nothing)
    uint64_t trim_total = 0;           // .. this many records
    necat::DevBuf nw_buf[8];           // the arenas of necat_nw_path_batch (stage_nw.inl: NwBuf, one array each, typed by NwDevice::buf), grow-only; the leaf flags' one is capped by NECAT_NW_POOL_MB
    necat::DevBuf dal_buf[5];          // necat_local_align_batch, necat_asm_map_batch (stage_dalign.inl: DalBuf, one array each, typed by as<T>): tasks, outputs, the second tier's, and the table / score pair of ..
    double dal_error = 0.0; int dal_ave_path = 0;      // .. this error (0: none yet)
    double gather_ms = 0; uint64_t gather_bytes = 0;      // the last necat_volume_gather: its kernel (HIP events), the bytes it read and wrote (necat_volume_gather_stats)
    necat_item_order_stats item_order = {};      // the last extension call's checkpoint passes: lane-steps issued / needed (read_stats, stage_extend.inl; necat_get_item_order_stats)
    necat_rm_stats rm_stats = {};      // the last necat_map_reference (stage_refmap.inl; necat_get_rm_stats_sized)
    necat::DevBuf cns_dev;             // the arena of the consensus proper on the device: laid out per chunk by CnsChunkArena (stage_cns_consensus.inl), per segment by CtgRangeArena (stage_ctg_consensus.inl)
    necat::DevBuf ctg_seed_buf[3];     // necat_ctg_seed_batch (stage_ctg_seed.inl: CsBuf): a segment's table (three u32 arrays), a run of jobs with their tables and outputs (CtgSeedRunArena), a chunk's pool of seeds (CtgSeedPoolArena)
};

constexpr int kIdxCacheHoles = 2;

struct necat_volume {
    uint64_t nbases = 0, nseq = 0;
    uint64_t* bases_alloc = nullptr;   // guarded allocation
    uint64_t* bases = nullptr;         // bases_alloc + guard
    uint64_t* seq_off = nullptr;       // [nseq + 1]
    std::vector<uint64_t> h_seq_off;   // host copy (offsets are tiny; used for planning)
};

struct necat_index {
    int k = 0;
    uint64_t table_entries = 0, n_offsets = 0;
    // the table: ONE allocation (`table`, stats_cap bytes) holding either the dense reference layout (kmer_stats) or the sparse
    // one (words: table_entries / 64 IdxWords, then n_compact non-zero entries) - necat::IndexView in dev_common.h
    void* table = nullptr;
    uint64_t* kmer_stats = nullptr;
    void* words = nullptr;
    uint64_t* compact = nullptr;
    uint64_t n_compact = 0;
    uint64_t* offset_list = nullptr;
    size_t stats_cap = 0, offs_cap = 0;   // allocation sizes in bytes
    // Record-space bases (the unsharded LDS-slice build, stage_index.inl): slice s (4096 table entries) keeps its offsets AND its compact entries from
    // slice_start[s] on, dense from there: slice_kept[s] offsets, slice_pres[s] compact entries, then a hole up to slice_start[s + 1].  Lookups never see
    // the holes (a table entry carries its own start and count); the downloads close them.  n_offsets / n_compact stay what they were - kept entries,
    // non-zero table entries - and the arrays are offsets_cap / compact_cap entries long (+ 1).  All three arrays live behind `compact` in `table`.
    uint64_t n_slices = 0, offsets_cap = 0, compact_cap = 0;
    uint64_t* slice_start = nullptr;      // [n_slices + 1]; nullptr: no holes (dense bases)
    uint32_t *slice_kept = nullptr, *slice_pres = nullptr;
};

namespace necat {

// an entry point of the C ABI makes its context's knobs the current ones of this thread for the length of the call (knobs.h)
struct KnobScope {
    const Knobs* prev;
    explicit KnobScope(const necat_ctx* c) : prev(tl_knobs) { if (c) tl_knobs = &c->knobs; }
    ~KnobScope() { tl_knobs = prev; }
    KnobScope(const KnobScope&) = delete; KnobScope& operator=(const KnobScope&) = delete;
};

inline int set_err(necat_ctx* ctx, int code, const char* fmt, ...)
{
    if (ctx) {
        va_list ap; va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define NECAT_HIP(ctx, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) \
    return necat::set_err(ctx, NECAT_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); } while (0)

#define NECAT_CHECK_LAUNCH(ctx, name) do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) \
    return necat::set_err(ctx, NECAT_ERR_DEVICE, "launch of %s failed: %s", name, hipGetErrorString(e__)); } while (0)

constexpr int kGuardWords = 4;   // 128 bases of slack on both sides of a volume's bases

inline int buf_ensure(necat_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return NECAT_OK;
    if (b.p) { hipError_t e = hipFree(b.p); (void)e; b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr; b.cap = 0;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = tot = 0;
        char own[512]; int at = 0; size_t sum = 0;          // this context's arenas of 256 MB and more (ScratchId : MB)
        own[0] = 0;
        if (ctx) for (int i = 0; i < (int)(sizeof ctx->scratch / sizeof ctx->scratch[0]); ++i) {
            sum += ctx->scratch[i].cap;
            if (ctx->scratch[i].cap >= ((size_t)256 << 20) && at < 480) at += snprintf(own + at, sizeof own - (size_t)at, " %d:%zu", i, ctx->scratch[i].cap >> 20);
        }
        return set_err(ctx, NECAT_ERR_MEMORY, "hipMalloc(%zu) failed: %s (device memory: %zu MB free of %zu MB; this context's arenas: %zu MB, the big ones [id:MB]%s)", want,
                       hipGetErrorString(e), fr >> 20, tot >> 20, sum >> 20, own);
    }
    b.cap = want;
    return NECAT_OK;
}

// grow keeping the first `keep` bytes (device-to-device copy; capacity doubles)
inline int buf_grow(necat_ctx* ctx, DevBuf& b, size_t bytes, size_t keep, hipStream_t s)
{
    if (bytes <= b.cap) return NECAT_OK;
    size_t want = bytes > 2 * b.cap ? bytes + bytes / 8 + 256 : 2 * b.cap;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess) return set_err(ctx, NECAT_ERR_MEMORY, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    if (b.p && keep) {
        e = hipMemcpyAsync(q, b.p, keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(q); return set_err(ctx, NECAT_ERR_DEVICE, "device copy failed: %s", hipGetErrorString(e)); }
    }
    if (b.p) (void)hipFree(b.p);
    b.p = q; b.cap = want;
    return NECAT_OK;
}

// a role-indexed buffer that holds ONE array (nw_buf, dal_buf, a segment's table): that array
template <class T> inline T* as(const DevBuf& b) { return (T*)b.p; }

// An arena (arena_layout.h) on the device: buf_ensure(ctx, buf, layout.bytes()) first, then this view of `buf` turns a span into the pointer a kernel receives and
// issues the copies and fills of a slot on stream `s` - one hipMem*Async each, its byte count the given element count times the span's element size, the count checked
// against the span's own (assert, active in the shipped build: a host bug, not an error of the call).  What it does NOT check: that a kernel stays inside the slot it was handed.
struct ArenaView {
    char* base; size_t total; hipStream_t s;
    ArenaView(const DevBuf& b, const ArenaLayout& l, hipStream_t st) : base((char*)b.p), total(l.bytes()), s(st) { assert(total <= b.cap); }
    template <class T> T* ptr(Span<T> sp) const { assert(sp.end() <= total); return (T*)(base + sp.off); }
    template <class T> const T* cptr(Span<T> sp) const { return ptr(sp); }
    template <class T> hipError_t upload(Span<T> sp, const T* src, size_t n) const { assert(n <= sp.n); return hipMemcpyAsync(ptr(sp), src, n * sizeof(T), hipMemcpyHostToDevice, s); }
    // elements first .. first + n of the slot
    template <class T> hipError_t download(T* dst, Span<T> sp, size_t n, size_t first = 0) const { assert(first + n <= sp.n); return hipMemcpyAsync(dst, ptr(sp) + first, n * sizeof(T), hipMemcpyDeviceToHost, s); }
    template <class T> hipError_t fill(Span<T> sp, int byte, size_t n) const { assert(n <= sp.n); return hipMemsetAsync(ptr(sp), byte, n * sizeof(T), s); }
    template <class T> hipError_t zero(Span<T> sp, size_t n) const { return fill(sp, 0, n); }
    // the slot and every slot taken after it, padding included
    template <class T> hipError_t zero_from(Span<T> sp) const { assert(sp.off <= total); return hipMemsetAsync(base + sp.off, 0, total - sp.off, s); }
};

inline double ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0; return ms; }

// The events of ONE call of a batch stage (the context's own, EventId, belong to the stages that overlap streams): created at the entry point, destroyed on every
// way out.  ms(i): from event i to event i + 1, after a synchronise.
template <int N>
struct CallEvents {
    hipEvent_t ev[N] = {};
    CallEvents() = default;
    CallEvents(const CallEvents&) = delete; CallEvents& operator=(const CallEvents&) = delete;
    ~CallEvents() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
    int create(necat_ctx* ctx) { for (auto& e : ev) NECAT_HIP(ctx, hipEventCreate(&e)); return NECAT_OK; }
    hipError_t record(int i, hipStream_t s) const { return hipEventRecord(ev[i], s); }
    double ms(int i) const { return ev_ms(ev[i], ev[i + 1]); }
};

// The arrays a call has allocated for its caller (result_alloc): necat_free'd on every way out but the one that release()s them into the out-parameters.
struct ResultOwner {
    void* held[2] = {nullptr, nullptr}; int n = 0;
    ResultOwner() = default;
    ResultOwner(const ResultOwner&) = delete; ResultOwner& operator=(const ResultOwner&) = delete;
    ~ResultOwner() { for (int i = 0; i < n; ++i) necat_free(held[i]); }
    template <class T> T* own(void* p) { assert(n < 2); held[n++] = p; return (T*)p; }
    void release() { n = 0; }
};

enum ScratchId {
    SC_CNT32 = 0, SC_PARTIAL, SC_TMPLIST, SC_MISC,
    SC_SEED_META, SC_SEED_HT, SC_SEED_POOL, SC_SEED_CHAIN, SC_SEED_OUT, SC_SEED_FINAL,
    SC_EXT_TASKS, SC_EXT_LISTS, SC_EXT_FRAG, SC_EXT_MAT, SC_EXT_OPS, SC_EXT_RES, SC_EXT_CAND, SC_SMALL, SC_PART,
    SC_EXT_COLS, SC_EXT_COLS_OUT, SC_PART2, SC_SEED_ALL, SC_EXT_MATB, SC_EXT_MATB2, SC_EXT_PERM, SC_GATHER, SC_SPLIT, SC_SPLIT2,
    SC_ASM_BAND, SC_ASM_OPS, SC_ASM_COLS, SC_ASM_MISC, SC_ASM_FRAG, SC_ASM_OUT, SC_SEED_KST, SC_EXT_CKPT, SC_EXT_WOUT, SC_EXT_CKPTB, SC_EXT_CKPTB2, SC_EXT_WOUTB, SC_EXT_WOUTB2,
    SC_ASM_OCC, SC_ASM_TAB, SC_ASM_VMETA, SC_ASM_VHT, SC_ASM_VPOOL, SC_ASM_VOUT, SC_ASM_SEL, SC_ASM_RIDX, SC_ASM_RNEXT, SC_ASM_PAIRS, SC_ASM_SEEDS,
    SC_ASM_VMETA2, SC_ASM_VHT2, SC_ASM_VPOOL2, SC_ASM_VOUT2, SC_ASM_SEL2, SC_ASM_RIDX2, SC_ASM_RNEXT2,
    SC_STATS,
    SC_TRIM_IN, SC_TRIM_RECS, SC_TRIM_OFF,      // stage_trim.inl: input records + cursors, records grouped by read, read_off + clip ranges + count
    SC_COUNT
};

// buf_ensure for arenas of DIFFERENT phases of a context (the index build's split buffers / the seeding arenas: never live at the same
// time, every call that uses them has finished with them when it returns): before allocating, take the buffer of a donor that is big
// enough and leave it this one's - the phases then hand ONE allocation back and forth instead of holding two (a 2 Gbp volume: 17 GB of
// split records and 14 GB of seed blocks; a process waits 30 - 55 ms per GB for device memory it maps the first time).
// What keeps that safe is no longer only the order of the donor lists: a phase marks the arenas it holds pointers into (ArenaUse, for the length of
// the call) and a marked arena is never taken - an index build running beside a candidate search of the same context would allocate instead of aliasing.
struct ArenaUse {
    necat_ctx* ctx; uint64_t mine;
    ArenaUse(necat_ctx* c, std::initializer_list<int> ids) : ctx(c), mine(0) { for (int i : ids) mine |= 1ULL << i; mine &= ~c->scratch_live; c->scratch_live |= mine; }
    ~ArenaUse() { ctx->scratch_live &= ~mine; }
    ArenaUse(const ArenaUse&) = delete; ArenaUse& operator=(const ArenaUse&) = delete;
};
inline int buf_ensure_lend(necat_ctx* ctx, int id, size_t bytes, std::initializer_list<int> donors)
{
    DevBuf& b = ctx->scratch[id];
    if (bytes <= b.cap) return NECAT_OK;
    if (!ctx->knobs.no_lend) for (int d : donors) {
        DevBuf& o = ctx->scratch[d];
        if (d != id && o.cap >= bytes && !((ctx->scratch_live >> d) & 1ULL)) { std::swap(b, o); return NECAT_OK; }
    }
    return buf_ensure(ctx, b, bytes);
}

}  // namespace necat
