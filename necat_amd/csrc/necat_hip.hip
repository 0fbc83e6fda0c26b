// necat_hip.hip - libnecat_hip.so: C ABI (include/necat_hip.h) + host orchestration of the gfx950
// kernels.  Written for MI355X only (wave64, 256 CUs, 288 GB HBM3E): buffers are sized for HBM
// residency of whole volumes, work lists and the traceback band of 10^5 concurrent alignments.
#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <time.h>
#include <unistd.h>
#include <numeric>
#include <atomic>
#include <type_traits>

// Two builds of these sources.  libnecat_hip.so - the product - launches the kernels of the default paths only; the kernel families those paths replaced and the tests keep
// as independent implementations of the same results (k_myers_coop / k_myers with the band-record k_traceback and k_walk_wave, k_myers_a16, k_rcwalk2, k_rcwalk4, k_myers_ck
// without carries, the lane-per-strand seed collection, the global-atomic index passes, k_asm_align, and the batch Edlib_align hook that drives them block by block) are
// compiled with -DNECAT_BUILD_CROSSCHECK into libnecat_hip_xcheck.so, which the tests' alternative-path cases load (necat_amd/capi.py).  A knob that selects such a path
// in the product build fails the call with NECAT_ERR_ARG and says so - it never falls back to another path.
#ifdef NECAT_BUILD_CROSSCHECK
#define NECAT_XCHECK 1
#else
#define NECAT_XCHECK 0
#endif

#include "runtime.h"
#include "index_kernels.h"
#include "volume_kernels.h"
#include "seed_kernels.h"
#include "pcan_kernels.h"
#include "trim_kernels.h"
#include "ext_kernels.h"
#include "ext_tail.h"
#include "ext_rcwalk.h"
#include "ext_rcwalk3.h"
#include "asm_kernels.h"
#include "asm_coop.h"
#include "asm_plan.h"
#include "host_bases.h"
#include "host_threads.h"
#include "cns_loop.h"
#include "cns_rescue.h"
#include "cns_consensus.h"
#include "cns_dev_kernels.h"
#include "ctg_consensus.h"
#include "ctg_dev_kernels.h"
#include "ctg_seed.h"
#include "ctg_seed_kernels.h"
#include "ctg_extend.h"
#include "nw_kernels.h"
#include "dal_kernels.h"
#include "asm_ends_core.h"
#include "rm_host.h"
#include "rescue_pair.h"
#include "comm.h"
#include "pair_sched.h"

// The two lanes of the extension rounds are eight streams; the HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and kernels of streams
// that share a queue run one after the other - with 4 queues the second lane gains 3.7 % at yeast size, with 8 it gains 7.7 % (tools/r05/run20.sh).  The variable is read
// when the runtime initialises (the first HIP call of the process): the command-line programs (necat_cli_env, pm_job.h) and bench.py set it before their first HIP
// call; the LIBRARY does not touch its host's environment (until round 6 a load-time constructor did: a setenv behind the back of a multi-threaded host, and without
// effect where the runtime was already up).  What the library does instead is need few queues (NECAT_STREAM_GRAPH=1, ctx_streams below: a context's list-A chain on its own
// stream, its other streams made with the context, in a fixed order); under NECAT_TRACE a context says once how many streams it made and at which priority.

namespace necat { thread_local const Knobs* tl_knobs = nullptr; }      // knobs.h: set by KnobScope in every entry point that takes a context; read through knob()
using namespace necat;

#define NECAT_RETIRED(ctx, what) return necat::set_err(ctx, NECAT_ERR_ARG, "%s: a cross-check path this library is built without (it is in libnecat_hip_xcheck.so, -DNECAT_BUILD_CROSSCHECK)", what)

static_assert(SC_COUNT <= (int)(sizeof(necat_ctx::scratch) / sizeof(necat::DevBuf)), "a ScratchId without an arena");

namespace {

// (re)allocate a band-record pool; a fresh allocation is zeroed once (not needed for correctness - the walk only reads
// records its round stored - but it keeps a run reproducible should that invariant ever break)
int ensure_zeroed(necat_ctx* ctx, DevBuf& b, size_t bytes, hipStream_t s)
{
    const void* before = b.p; const size_t cap0 = b.cap;
    int rc = buf_ensure(ctx, b, bytes);
    if (rc) return rc;
    if (b.p != before || b.cap != cap0) { hipError_t e = hipMemsetAsync(b.p, 0, b.cap, s); if (e != hipSuccess) return set_err(ctx, NECAT_ERR_DEVICE, "memset failed"); }
    return NECAT_OK;
}

inline unsigned grid_for(uint64_t n, unsigned block, unsigned cap = 1u << 20)
{
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

DevVolume dev_view(const necat_volume* v)
{
    DevVolume d; d.bases = v->bases; d.seq_off = v->seq_off; d.nbases = v->nbases; d.nseq = v->nseq;
    return d;
}

// (the knobs: knobs.h - per context since round 5)

// Tuning / test knobs of ONE context: read from the environment when it is created, defaults otherwise.  The three expansions of knobs.h's table: this reader,
// necat_knob_get below, struct Knobs itself.
void finish_knobs(necat::Knobs& K)
{   // the rules that are no min / max of one knob
    if (!K.rc_carry) { K.rc_listb = K.rc_ragged = 0; K.rc_maxdist = std::min(K.rc_maxdist, kRcMaxDist); }
    K.rc3_band = K.rc3_band == 16 ? 16 : 32;
    K.split_threads = K.split_threads == 256 ? 256 : 512;
    K.rc_dbg &= 6u;
    K.band_pool <<= 20; K.rc_pool <<= 20; K.asm_rc_pool <<= 20; K.nw_pool <<= 20;        // MB in the environment, bytes in the field
    if (K.cns_threads <= 0) K.cns_threads = 32;
}

void read_knobs(necat::Knobs& K)
{
#define READ_NUM(field, type, name, dflt, lo, hi) { const char* e = getenv(name); K.field = (decltype(K.field))std::min<Knobs::ull>(hi, std::max<Knobs::ull>(lo, e ? strtoull(e, nullptr, 10) : (Knobs::ull)(dflt))); }
#define READ_INT(field, name, dflt) { const char* e = getenv(name); K.field = e ? atoi(e) : (dflt); }
#define READ_SET(field, name) { const char* e = getenv(name); K.field.set = e != nullptr; K.field.v = e ? atoi(e) : 0; }
#define READ_STR(field, name) { const char* e = getenv(name); K.field = e ? e : ""; }
    NECAT_KNOBS(READ_NUM, READ_INT, READ_SET, READ_STR)
    finish_knobs(K);
}

// a knob's value as text (necat_knob_get)
template <class T> int knob_text(char* buf, size_t n, T v) { if (std::is_signed<T>::value) snprintf(buf, n, "%lld", (long long)v); else snprintf(buf, n, "%llu", (unsigned long long)v); return NECAT_OK; }
int knob_text(char* buf, size_t n, const necat::KnobSet& v) { if (v.set) snprintf(buf, n, "%d", v.v); else buf[0] = 0; return NECAT_OK; }       // (not set: "")
int knob_text(char* buf, size_t n, const std::string& v) { snprintf(buf, n, "%s", v.c_str()); return NECAT_OK; }

double wall_ms() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// A stream of priority class `cls`: 0 = normal, 1 = the device's lowest, 2 = its highest.  The runtime keeps a pool of hardware queues per priority level, so streams of
// different classes never share a queue (kernels of streams that share a queue run one after the other, whichever context they belong to).
hipError_t make_stream(hipStream_t* st, int cls)
{
    int least = 0, greatest = 0;
    if (cls && hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
    return cls && least != greatest ? hipStreamCreateWithPriority(st, hipStreamDefault, cls == 1 ? least : greatest) : hipStreamCreate(st);
}

// The streams of a context under NECAT_STREAM_GRAPH=1 (the default), made by necat_ctx_create in this order - four host threads that create their contexts
// one after the other get the same stream-to-queue table from run to run, where the first extension call of each used to race for the queues:
//   stream      the context's own: index build, seeding, and list A's chain of the extension (k_ext_init, the rounds, k_ext_result, k_m4_filter) - one sequence per call
//   stream_b/c  list B's chains, which trail list A's by a round (NECAT_LISTB_STREAMS=1: one stream; NECAT_LISTB_PRIO: their priority pool)
//   stream_d    only where this context's knobs select a path that launches on it: the un-merged ragged chain, NECAT_RC_PIPE, the cross-check build's side chain
// (stream_copy stays lazy: ext_streams; lanes 1 .. are made on first use: ext_lane.)  NECAT_SERIAL=1 keeps meaning one stream for everything: nothing is made here.
int ctx_streams(necat_ctx* ctx)
{
    const necat::Knobs& K = ctx->knobs;
    ctx->need_stream_d = NECAT_XCHECK || !(K.rc_merge && K.rc_ragged && K.rc_carry && !K.rc_ckg_all.set) || K.rc_pipe > 1;
    ctx->graph_streams = K.stream_graph && !K.serial;
    if (!ctx->graph_streams) return hipStreamCreate(&ctx->stream) == hipSuccess ? NECAT_OK : NECAT_ERR_DEVICE;      // (the others: ext_streams, on the first call that needs them)
    const int cls_a = K.stream_prio == 2 ? 2 : 0;
    const int cls_b = K.stream_prio == 1 ? 2 : K.listb_prio == 1 || K.listb_prio == 2 ? K.listb_prio : 0;
    if (make_stream(&ctx->stream, cls_a) != hipSuccess) return NECAT_ERR_DEVICE;
    ctx->stream_a = ctx->stream;
    if (make_stream(&ctx->stream_b, cls_b) != hipSuccess) return NECAT_ERR_DEVICE;
    if (K.listb_streams < 2) ctx->stream_c = ctx->stream_b;
    else if (make_stream(&ctx->stream_c, cls_b) != hipSuccess) return NECAT_ERR_DEVICE;
    if (ctx->need_stream_d && make_stream(&ctx->stream_d, cls_b) != hipSuccess) return NECAT_ERR_DEVICE;
    if (K.trace)
        fprintf(stderr, "[necat] context streams (NECAT_STREAM_GRAPH=1): %d made - its own and list A's (priority class %d), %d for list B (class %d)%s; classes: 0 normal, 1 lowest, 2 highest\n",
                1 + (K.listb_streams < 2 ? 1 : 2) + (ctx->need_stream_d ? 1 : 0), cls_a, K.listb_streams < 2 ? 1 : 2, cls_b, ctx->need_stream_d ? ", 1 for the ragged / piped chain (list B's class)" : "");
    return NECAT_OK;
}

// every stream once: stream_a .. stream_d may be aliases of `stream` or of one another (NECAT_SERIAL, NECAT_STREAM_GRAPH=1, NECAT_LISTB_STREAMS=1)
void destroy_streams(std::initializer_list<hipStream_t> all)
{
    std::vector<hipStream_t> seen;
    for (hipStream_t st : all) if (st && std::find(seen.begin(), seen.end(), st) == seen.end()) { seen.push_back(st); (void)hipStreamDestroy(st); }
}

// A volume's 2-bit words from the device, for the host code that reads bases as byte codes (host_bases.h): all of them, or those of one read.
// These two are the only copies of a volume's bases to the host; when a stage makes them is the stage's business.
int fetch_words(necat_ctx* ctx, const necat_volume* v, std::vector<u64>* words)
{
    words->resize((v->nbases + 31) / 32 + 1);
    NECAT_HIP(ctx, hipMemcpy(words->data(), v->bases, (words->size() - 1) * 8, hipMemcpyDeviceToHost));
    return NECAT_OK;
}

int fetch_read_words(necat_ctx* ctx, const necat_volume* v, uint64_t id, std::vector<u64>* words, u64* word0)      // (*words)[0]: word *word0 of the volume
{
    const u64 b = v->h_seq_off[id], e = v->h_seq_off[id + 1];
    *word0 = b >> 5;
    words->resize(e == b ? 0 : ((e - 1) >> 5) - *word0 + 1);
    if (!words->empty()) NECAT_HIP(ctx, hipMemcpy(words->data(), v->bases + *word0, words->size() * 8, hipMemcpyDeviceToHost));
    return NECAT_OK;
}

necat_host::BaseWords host_view(const necat_volume* v, const std::vector<u64>& words, u64 word0 = 0)
{
    necat_host::BaseWords b; b.w = words.data(); b.word0 = word0; b.seq_off = v->h_seq_off.data();
    return b;
}

// the host threads a call of a batch stage may start: its options' host_threads, NECAT_CNS_THREADS when that is 0; never more than 256 or than the machine has
unsigned call_threads(const necat_ctx* ctx, int host_threads)
{
    const unsigned want = host_threads ? (unsigned)std::min(host_threads, 256) : (unsigned)ctx->knobs.cns_threads;
    return std::max(1u, std::min(want, std::min(necat_host::hardware_threads(), 256u)));
}

// Sequence `id` of a volume whose first sequence has the id `start_id`: its index there, its first base and its length.  false: the volume has no such sequence.
struct SeqAt { int64_t k; u64 begin, len; };
bool seq_at(const necat_volume* v, int64_t id, int64_t start_id, SeqAt* s)
{
    s->k = id - start_id;
    if (s->k < 0 || (uint64_t)s->k >= v->nseq) return false;
    s->begin = v->h_seq_off[s->k]; s->len = v->h_seq_off[s->k + 1] - s->begin;
    return true;
}

// Segment s of a contig polishing call: sizes, the range of its `what` (overlaps, jobs), and - where the call has the contigs - that it lies inside its contig.
// min_size: seeding's 15 bases (0: none).
int ctg_segment_check(necat_ctx* ctx, const necat_volume* contigs, const necat_ctg_segment& S, uint64_t s, int min_size, const char* what)
{
    if (S.size < 0 || S.from < 0 || S.ovlp_begin > S.ovlp_end) return set_err(ctx, NECAT_ERR_ARG, "segment %lu: bad size, start or %s range", (unsigned long)s, what);
    if ((int64_t)S.size >= necat_host::ctg::kMaxSegment) return set_err(ctx, NECAT_ERR_ARG, "segment %lu has %d bases: 2^24 or more", (unsigned long)s, S.size);
    if (S.size < min_size) return set_err(ctx, NECAT_ERR_ARG, "segment %lu has %d bases: fewer than %d, the reference has no defined answer", (unsigned long)s, S.size, min_size);
    SeqAt c;
    if (contigs && (!seq_at(contigs, S.ctg_id, 0, &c) || (u64)S.from + (u64)S.size > c.len)) return set_err(ctx, NECAT_ERR_ARG, "segment %lu leaves its contig", (unsigned long)s);
    return NECAT_OK;
}
static_assert(necat_host::ctg::kMaxSegment == necat_host::ctg_seed::kMaxSegment, "one bound on a segment for both contig stages");

}  // namespace

#include "stage_ck_round.inl"      // (templates: in front of the extern "C" block)

extern "C" {

void necat_default_options(necat_map_options* o)
{   // map_options.c:12-28 (sDefaultPairwiseMapingOptions)
    o->kmer_size = 15; o->scan_window = 10; o->kmer_cnt_cutoff = 500; o->block_size = 2000;
    o->block_score_cutoff = 3; o->num_candidates = 500; o->align_size_cutoff = 500;
    o->ddfs_cutoff = 0.25; o->error = 0.5; o->num_output = 500; o->num_threads = 1;
    o->job = 1; o->binary_output = 0; o->use_hdr_as_id = 1;
}

// why the last necat_ctx_create of this thread failed (there is no context to hold that text): necat_last_error(NULL)
static thread_local char g_create_err[256] = "no context";
#define NECAT_CREATE_FAIL(code, ...) do { snprintf(g_create_err, sizeof g_create_err, __VA_ARGS__); return (code); } while (0)

int necat_ctx_create(int device_id, necat_ctx** out)
{
    if (!out) return NECAT_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); NECAT_CREATE_FAIL(NECAT_ERR_DEVICE, "no usable HIP device (there is no CPU fallback)"); }
    if (device_id < 0 || device_id >= ndev) NECAT_CREATE_FAIL(NECAT_ERR_ARG, "device %d of %d", device_id, ndev);
    if (hipSetDevice(device_id) != hipSuccess) NECAT_CREATE_FAIL(NECAT_ERR_DEVICE, "hipSetDevice(%d) failed", device_id);
    necat_ctx* ctx = new necat_ctx();
    ctx->device = device_id;
    read_knobs(ctx->knobs);
#if !NECAT_XCHECK
    if (ctx->knobs.rc_ww == 0) {      // (the one retired path chosen inside a launcher that cannot fail: refused here)
        fprintf(stderr, "[necat] NECAT_RC_WW=0 selects k_rcwalk2, a cross-check kernel this library is built without (libnecat_hip_xcheck.so has it)\n");
        delete ctx; NECAT_CREATE_FAIL(NECAT_ERR_ARG, "NECAT_RC_WW=0 selects k_rcwalk2, a cross-check kernel this library is built without (libnecat_hip_xcheck.so has it)");
    }
#endif
    memset(&ctx->tm, 0, sizeof ctx->tm);
    memset(&ctx->shard_tm, 0, sizeof ctx->shard_tm);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        snprintf(ctx->devname, sizeof ctx->devname, "%s (%s), %d CUs", prop.name, prop.gcnArchName, prop.multiProcessorCount);
        ctx->num_cu = prop.multiProcessorCount;
    }
    // the context's streams, in a fixed order (ctx_streams; NECAT_STREAM_GRAPH=0: one stream now, the extension's when the first extension runs)
    if (ctx_streams(ctx) != NECAT_OK) {
        destroy_streams({ctx->stream, ctx->stream_a, ctx->stream_b, ctx->stream_c, ctx->stream_d});
        delete ctx; NECAT_CREATE_FAIL(NECAT_ERR_DEVICE, "hipStreamCreate failed");
    }
    for (int i = 0; i < kNumEvents; ++i) if (hipEventCreate(&ctx->ev[i]) != hipSuccess) { delete ctx; return NECAT_ERR_DEVICE; }
    // the list sizes of the extension rounds reach the host through this pinned ring (RoundPub, ext_kernels.h)
    if (hipHostMalloc(&ctx->round_ring, kMaxExtLanes * kRoundRing * sizeof(RoundPub), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&ctx->round_ring_dev, ctx->round_ring, 0) != hipSuccess) { delete ctx; return NECAT_ERR_DEVICE; }
    memset(ctx->round_ring, 0, kMaxExtLanes * kRoundRing * sizeof(RoundPub));      // (a stretch per lane: ExtLane1)
    *out = ctx;
    return NECAT_OK;
}

void necat_ctx_destroy(necat_ctx* ctx)
{
    KnobScope knob_scope_(ctx);
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (knob().trace & 2) {        // what the context holds at its end: the arenas of 64 MB and more (ScratchId : MB)
        size_t sum = 0; char own[1024]; int at = 0; own[0] = 0;
        for (int i = 0; i < (int)(sizeof ctx->scratch / sizeof ctx->scratch[0]); ++i) {
            sum += ctx->scratch[i].cap;
            if (ctx->scratch[i].cap >= ((size_t)64 << 20) && at < 980) at += snprintf(own + at, sizeof own - (size_t)at, " %d:%zu", i, ctx->scratch[i].cap >> 20);
        }
        fprintf(stderr, "[necat] context arenas at destroy: %zu MB in all; [id:MB]%s\n", sum >> 20, own);
    }
    if (ctx->stream_copy) (void)hipStreamSynchronize(ctx->stream_copy);
    for (auto& b : ctx->scratch) if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->idx_cache) if (b.p) (void)hipFree(b.p);
    if (ctx->cns_dev.p) (void)hipFree(ctx->cns_dev.p);
    for (auto& b : ctx->nw_buf) if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->dal_buf) if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->ctg_seed_buf) if (b.p) (void)hipFree(b.p);
    for (auto& lx : ctx->lanex) {
        for (auto& b : lx.buf) if (b.p) (void)hipFree(b.p);
        for (int i = 0; i < kNumEvents; ++i) if (lx.ev[i]) (void)hipEventDestroy(lx.ev[i]);          // (every event that exists, also those of a creation that failed half-way)
        destroy_streams({lx.st[0], lx.st[1], lx.st[2], lx.st[3]});
    }
    delete (cns::Scratch*)ctx->cns_scratch;
    if (ctx->pin_plan) (void)hipHostFree(ctx->pin_plan);
    for (int i = 0; i < kNumEvents; ++i) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->round_ring) (void)hipHostFree(ctx->round_ring);
    destroy_streams({ctx->stream, ctx->stream_a, ctx->stream_b, ctx->stream_c, ctx->stream_d, ctx->stream_copy});
    delete ctx;
}

void necat_ctx_trim(necat_ctx* ctx)
{
    KnobScope knob_scope_(ctx);
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& b : ctx->scratch) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    for (auto& b : ctx->idx_cache) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    if (ctx->cns_dev.p) { (void)hipFree(ctx->cns_dev.p); ctx->cns_dev = DevBuf(); }
    for (auto& b : ctx->nw_buf) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    for (auto& b : ctx->dal_buf) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    for (auto& b : ctx->ctg_seed_buf) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    for (auto& lx : ctx->lanex) for (auto& b : lx.buf) if (b.p) { (void)hipFree(b.p); b = DevBuf(); }
    ctx->seed_ht_ptr = nullptr; ctx->seed_ht_clean = 0; ctx->seed_ht_cap = 0;
}

const char* necat_last_error(const necat_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

int necat_device_name(const necat_ctx* ctx, char* buf, size_t n)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !buf || !n) return NECAT_ERR_ARG;
    snprintf(buf, n, "%s", ctx->devname);
    return NECAT_OK;
}

int necat_get_timings(const necat_ctx* ctx, necat_timings* t)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !t) return NECAT_ERR_ARG;
    *t = ctx->tm;
    return NECAT_OK;
}

int necat_get_timings_sized(const necat_ctx* ctx, void* t, size_t bytes)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !t) return NECAT_ERR_ARG;
    memcpy(t, &ctx->tm, bytes < sizeof(necat_timings) ? bytes : sizeof(necat_timings));
    return NECAT_OK;
}

int necat_get_rm_stats_sized(const necat_ctx* ctx, void* stats, size_t bytes)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !stats) return NECAT_ERR_ARG;
    memcpy(stats, &ctx->rm_stats, bytes < sizeof(necat_rm_stats) ? bytes : sizeof(necat_rm_stats));
    return NECAT_OK;
}

int necat_get_item_order_stats(const necat_ctx* ctx, necat_item_order_stats* stats)
{
    if (!ctx || !stats) return NECAT_ERR_ARG;
    *stats = ctx->item_order;
    return NECAT_OK;
}

int necat_knob_get(const necat_ctx* ctx, const char* name, char* buf, size_t n)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !name || !buf || !n) return NECAT_ERR_ARG;
#define GET_KNOB(field, env) if (!strcmp(name, env)) return knob_text(buf, n, ctx->knobs.field);
#define GET_NUM(field, type, env, dflt, lo, hi) GET_KNOB(field, env)
#define GET_INT(field, env, dflt) GET_KNOB(field, env)
    NECAT_KNOBS(GET_NUM, GET_INT, GET_KNOB, GET_KNOB)
    return NECAT_ERR_ARG;         // not a knob of the table
}

int necat_abi_version(void) { return NECAT_ABI_VERSION; }

// Result blocks handed to the caller.  Big ones are pinned host memory (the device copies straight into
// them) and are recycled: necat_free() parks up to kPoolBlocks of them for the next call instead of
// returning 20 MB of freshly faulted pages to the OS every pass.
namespace {
struct ResultPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> live;              // pinned blocks currently owned by callers
    std::vector<std::pair<void*, size_t>> parked;         // never released at exit: the HIP runtime may be gone by then
};
ResultPool g_results;
constexpr size_t kPinnedMin = 256 << 10, kPoolBlocks = 16, kPoolBytes = (size_t)8 << 30;   // parked: <= 16 blocks, <= 8 GiB

void* result_alloc(size_t bytes)
{
    if (bytes < kPinnedMin) return malloc(bytes ? bytes : 1);
    std::lock_guard<std::mutex> lk(g_results.mu);
    int best = -1;
    for (int i = 0; i < (int)g_results.parked.size(); ++i) {
        const size_t sz = g_results.parked[i].second;
        if (sz >= bytes && sz <= 2 * bytes + (1 << 20) && (best < 0 || sz < g_results.parked[best].second)) best = i;
    }
    void* p = nullptr; size_t sz = 0;
    if (best >= 0) { p = g_results.parked[best].first; sz = g_results.parked[best].second; g_results.parked.erase(g_results.parked.begin() + best); }
    else {
        sz = (bytes + (bytes >> 3) + 4095) & ~(size_t)4095;          // a little slack so the next pass fits too
        if (hipHostMalloc(&p, sz, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return malloc(bytes); }
    }
    g_results.live[p] = sz;
    return p;
}
}  // namespace

void necat_free(void* p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_results.mu);
        auto it = g_results.live.find(p);
        if (it != g_results.live.end()) {
            const size_t sz = it->second;
            g_results.live.erase(it);
            // park it; when the pool is full the smallest blocks go first (pinning costs ~0.15 s per GB, so the big
            // ones are the ones worth keeping)
            g_results.parked.emplace_back(p, sz);
            size_t held = 0;
            for (auto& b : g_results.parked) held += b.second;
            while (g_results.parked.size() > kPoolBlocks || (held > kPoolBytes && !g_results.parked.empty())) {
                size_t k = 0;
                for (size_t i = 1; i < g_results.parked.size(); ++i) if (g_results.parked[i].second < g_results.parked[k].second) k = i;
                held -= g_results.parked[k].second;
                (void)hipHostFree(g_results.parked[k].first);
                g_results.parked.erase(g_results.parked.begin() + k);
            }
            return;
        }
    }
    free(p);
}

// ---- the stages, one file each: same translation unit, included here in dependency order
#include "stage_volumes.inl"
#include "stage_index.inl"
#include "stage_seed.inl"
#include "stage_extend.inl"
#include "stage_asm_align.inl"
#include "stage_asm_plan.inl"
#include "stage_pcan.inl"
#include "stage_trim.inl"
#include "stage_multi.inl"
#include "stage_align_batch.inl"
#include "stage_nw.inl"
#include "stage_dalign.inl"
#include "stage_refmap.inl"      // (its speculative rescue pass runs dal_solve and nw_run)
#include "stage_asm_ends.inl"
#include "stage_cns.inl"
#include "stage_cns_consensus.inl"
#include "stage_ctg_consensus.inl"
#include "stage_ctg_seed.inl"
#include "stage_ctg_extend.inl"      // (after the seeding it may call, the aligner and the pair it runs)
#include "stage_edlib_batch.inl"

}  // extern "C"
