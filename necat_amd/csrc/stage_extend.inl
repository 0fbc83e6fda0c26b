// stage_extend.inl - the extension rounds (ext_*.h): lanes, BatchRun, extend_impl, necat_extend / necat_map_pair.
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ extension

namespace {

// One batch of candidates advancing through its rounds.  A candidate has one scheduled block at a time; the
// blocks of a round sit in list A (<= 512 x 512) or list B (bigger last blocks).  The chain that bounds the
// run is the list-A chain (frag -> DP -> traceback, round after round), so list B trails it by one round:
//
//     round r    stream a:  A(r)  = blocks of lists[r % 4].A      appends successors to lists[(r + 1) % 4]
//                stream b:  B(r)  = blocks of lists[r % 4].B      appends successors to lists[(r + 2) % 4]
//     lists[r] is complete when A(r - 1) and B(r - 2) are done; B(r) runs under A(r + 1).
//
// The host never waits for the device inside the loop.  The first kernel of A(r) publishes the sizes of lists[r]
// to a pinned ring and resets the counters of lists[(r + 2) % 4]; the host, one round behind, launches B(r - 1)
// with its exact size and A(r) with an upper bound (what was alive a round earlier - every kernel reads the exact
// size on the device); stream-to-stream order is kept by events.  Four list buffers: lists[(r + 2) % 4] receives
// appends from B(r) and A(r + 1) while lists[(r + 1) % 4] is filled by A(r) and B(r - 1), lists[r % 4] is consumed by
// A(r) and B(r), and lists[(r - 1) % 4] may still be read by B(r - 1).  B(r) and B(r - 1) run side by side on two
// streams with two sets of buffers and band pools (list A's pool is reused by A(r + 1) while they run).
struct Batch {
    ExtTask* tasks; u32* count;            // count[4][4]: (full list-A blocks, nB, other list-A blocks, -) per list buffer
    u32 cap;                               // capacity of every item array (list A is filled from both ends)
    BlockItem* itemsA[4]; BlockItem* itemsB[4];
    u64* fragA; u8* opsA; BlockResult* resA;
    // list B: two sets (round parity) - B(r) and B(r - 1) are independent and run side by side
    u64* fragB[2]; u8* opsB[2]; BlockResult* resB[2];
    BlockItem* sortedB[2]; u32* bins[2];    // list B of the round, sorted by size
    BlockItem* stage[4]; u32* cls[4];       // size-class order (item_order.h): staging array and class words per list buffer; nullptr = NECAT_ITEM_SORT=0, items appended in place
    hipStream_t sa, sb[2];
    hipEvent_t a0[4], a1[4], a2[4], b0[2], b1[2], b2[2];
    u64 base; u32 n;
    ExtLists lists_at(int j, u8* task_ops = nullptr) const       // list buffer j as the kernels append to it
    {
        ExtLists l; l.count = count + 4 * j; l.itemsA = itemsA[j]; l.itemsB = itemsB[j]; l.task_ops = task_ops; l.capA = cap;
        l.stage = stage[j]; l.cls = cls[j];
        return l;
    }
};

struct ExtShared {
    const necat_candidate* d_cands; necat_m4* d_m4; u8* d_ok; int* d_err; unsigned long long* stats;
    double error; int tail_match_len, min_align, read_start_id, ref_start_id;
    const u64* reads_off; const u64* ref_off;
    u8* task_ops = nullptr;      // alignment columns per task (necat_onc_align_batch)
};

// One lane of the extension rounds: everything run-to-run state of a batch in flight lives in - arenas, streams, events, its half of the
// published-sizes ring.  Lane 0 is the context's own set; lane 1 (ExtLane1, runtime.h) exists so that the NEXT batch can run its first,
// chip-filling rounds while this one is in its last, latency-bound ones (extend_impl).
enum ExtLaneBuf { LB_TASKS = 0, LB_LISTS, LB_FRAG, LB_OPS, LB_RES, LB_MAT, LB_CKPT, LB_WOUT, LB_CKPTB, LB_CKPTB2, LB_WOUTB, LB_WOUTB2, LB_MATB, LB_MATB2, LB_COUNT };
static_assert(LB_COUNT <= (int)(sizeof(ExtLane1::buf) / sizeof(necat::DevBuf)), "a lane-1 arena without a slot");
static_assert(LB_CKPTB2 == LB_CKPTB + 1 && LB_WOUTB2 == LB_WOUTB + 1 && LB_MATB2 == LB_MATB + 1, "list B's arenas of slot 1 follow those of slot 0");
struct ExtLane {
    DevBuf* buf[LB_COUNT];                            // by role
    DevBuf& at(ExtLaneBuf b, int slot = 0) const { return *buf[b + slot]; }       // (slot: list B's round parity, LB_*B only)
    hipStream_t sa, sb[2], sd;
    hipEvent_t* ev;                                   // kNumEvents of them, used as necat_ctx::ev is
    volatile RoundPub* ring; RoundPub* ring_dev;      // kRoundRing entries
    unsigned long long* round_seq;
};

// role -> arena of lane 0, the context's own scratch (lanes 1 .. keep theirs in ExtLane1::buf, by role)
constexpr ScratchId kLane0Arena[LB_COUNT] = {SC_EXT_TASKS, SC_EXT_LISTS, SC_EXT_FRAG, SC_EXT_OPS, SC_EXT_RES, SC_EXT_MAT, SC_EXT_CKPT, SC_EXT_WOUT,
                                             SC_EXT_CKPTB, SC_EXT_CKPTB2, SC_EXT_WOUTB, SC_EXT_WOUTB2, SC_EXT_MATB, SC_EXT_MATB2};

int ext_lane(necat_ctx* ctx, int id, ExtLane& L)
{
    if (id == 0) {
        for (int b = 0; b < LB_COUNT; ++b) L.buf[b] = ctx->scratch + kLane0Arena[b];
        L.sa = ctx->stream_a; L.sb[0] = ctx->stream_b; L.sb[1] = ctx->stream_c; L.sd = ctx->stream_d;
        L.ev = ctx->ev;
        L.ring = (volatile RoundPub*)ctx->round_ring; L.ring_dev = (RoundPub*)ctx->round_ring_dev; L.round_seq = &ctx->round_seq;
        return NECAT_OK;
    }
    if (id < 1 || id >= kMaxExtLanes) return set_err(ctx, NECAT_ERR_ARG, "extension lane %d of %d", id, kMaxExtLanes);
    ExtLane1& Q = ctx->lanex[id - 1];
    if (!Q.ready) {
        // Four streams of its own, at the device's LOWEST stream priority (NECAT_LANE1_PRIO: 0 = normal, 1 = lowest - the default -, 2 = highest): the runtime keeps
        // a pool of hardware queues per priority level (GPU_MAX_HW_QUEUES each), so these streams never share a queue with lane 0's - kernels of streams that share
        // a queue run one after the other, and which streams share is the runtime's choice (tools/r05/run22.sh: the same two-lane step took 36 or 45 ms depending on
        // the streams another context had made before) - and lane 0, which holds the longest chains of a call, is served first where both have waves to place.
        const int lane_prio = ctx->knobs.lane1_prio;
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        const int pr = lane_prio == 1 ? least : lane_prio == 2 ? greatest : 0;
        // (NECAT_STREAM_GRAPH=1: a stream only where a path launches on it, as the context's own - one list-B stream with NECAT_LISTB_STREAMS=1, no fourth without a path for it)
        const bool one_b = ctx->graph_streams && ctx->knobs.listb_streams < 2, no_d = ctx->graph_streams && !ctx->need_stream_d;
        for (hipStream_t& st : Q.st) {
            if (st || (one_b && &st == &Q.st[2]) || (no_d && &st == &Q.st[3])) continue;
            if ((lane_prio && least != greatest ? hipStreamCreateWithPriority(&st, hipStreamDefault, pr) : hipStreamCreate(&st)) != hipSuccess)
                return set_err(ctx, NECAT_ERR_DEVICE, "hipStreamCreate failed (second extension lane)");
        }
        if (one_b) Q.st[2] = Q.st[1];
        if (ctx->knobs.trace) fprintf(stderr, "[necat] extension lane %d: %d streams made at priority %d (device range %d .. %d)\n", id, 4 - (one_b ? 1 : 0) - (no_d ? 1 : 0), pr, least, greatest);
        // (events that exist are kept: a creation that failed half-way is completed by the next call, and necat_ctx_destroy destroys every non-null one)
        for (int i = 0; i < kNumEvents; ++i) if (!Q.ev[i] && hipEventCreate(&Q.ev[i]) != hipSuccess) { Q.ev[i] = nullptr; return set_err(ctx, NECAT_ERR_DEVICE, "hipEventCreate failed (second extension lane)"); }
        Q.ready = true;
    }
    for (int b = 0; b < LB_COUNT; ++b) L.buf[b] = Q.buf + b;
    L.sa = Q.st[0]; L.sb[0] = Q.st[1]; L.sb[1] = Q.st[2]; L.sd = Q.st[3];
    L.ev = Q.ev;
    L.ring = (volatile RoundPub*)ctx->round_ring + (size_t)id * kRoundRing; L.ring_dev = (RoundPub*)ctx->round_ring_dev + (size_t)id * kRoundRing; L.round_seq = &Q.round_seq;
    return NECAT_OK;
}

// All rounds of one batch (its first blocks are already in lists[0], appended by k_ext_init on stream a; every list counter but lists[0]'s is
// zero) as a resumable loop: run() is the whole of it; with several lanes the scheduler (ExtendCall::run_lanes) calls step() on whichever batch has its next
// sizes published.
//
// Streams and events of a lane, in the order the host issues them (NECAT_STREAM_GRAPH=1: lane 0's `sa` is the context's own stream, so everything a call queued before -
// candidates uploaded, counters zeroed, k_ext_init - precedes round 0 by stream order, and k_ext_result / k_m4_filter follow the last round the same way; NECAT_LISTB_STREAMS=1:
// sb[0] == sb[1]).  A stream only ever waits for an event the host has ALREADY recorded in this call, or never recorded / recorded by an earlier, drained call - both of
// which HIP treats as "nothing to wait for", which is what the first rounds need:
//   turn r of step():   wait_pub(r - 1) on the host (A(r - 1)'s first kernel has run: A(r - 2), B(r - 3) are done)
//     launch_b(r - 1):  sb waits a0[(r - 1) % 4]   recorded by begin_a(r - 1) in turn r - 1                      (lists[r - 1] complete, the counters of lists[r + 1] reset)
//                       sb waits b2[(r - 1) & 1]   recorded by launch_b(r - 3) in turn r - 2, or not in this call  (previous user of the slot's buffers, appended to lists[r - 1])
//                       records b0, b1, b2 of slot (r - 1) & 1 on sb
//     launch_a(r):      sa waits b2[r & 1]         (r >= 2) recorded by launch_b(r - 2) in turn r - 1, or - no list B in round r - 2 - an older, completed one
//                       records a0[r % 4] on sa after k_round_ctl / k_ext_frag, then a1, (EV_RC_WALK_END + r % 4), a2 behind their kernels
//                       (un-merged ragged chain / NECAT_RC_PIPE: sd waits a0[r % 4] or EV_PIPE_PIECE recorded just before on sa; sa waits EV_RAGGED_WALKED / EV_RC_WALK_END
//                       recorded just before on sd)
//   finish():           the host synchronises sa, sb[0], sb[1] - nothing of the batch is in flight when k_ext_result is queued on sa
// B(r - 1) is issued BEFORE A(r) in a turn, so A(r + 1)'s wait for b2[(r + 1) & 1] = b2[(r - 1) & 1] names B(r - 1)'s record; with one list-B stream B(r) queues behind
// B(r - 1) and its own wait for b2 of B(r - 2) is implied by the stream.
struct BatchRun {
    necat_ctx* ctx; const DevVolume& dref; const DevVolume& drd; Batch& c; const ExtShared& X; const ExtLane& L;
    struct Cnt { u32 nA, nB; };
    std::vector<Cnt> hist;                      // published sizes of lists[r]
    std::vector<u32> rc_round;                  // rounds whose full blocks ran through ext_rcwalk.h (L.ev[EV_RC_WALK_END + r % 4] marks the end of the walk kernel)
    std::vector<u8> a_timed;                    // A(r) ran its DP + traceback kernels (events recorded); 2 = as one fused launch (ext_tail.h)
    const unsigned long long seq0;
    volatile RoundPub* const ring;
    RoundPub* const ring_dev;
    bool b_pending[2] = {false, false}, b_fused[2] = {false, false};
    u32 b_blocks[2] = {0, 0};
    double last_wall;
    u32 rnd = 0, launched = 0;                  // the next round to launch; rounds launched
    bool tail = false;                          // fewer than NECAT_EXT_OVERLAP_PCT per cent of the batch's candidates still have a block: the next batch may start beside this one
    bool over = false;                          // nothing alive (or an error): finish() is next
    BatchRun(necat_ctx* ctx_, const DevVolume& dref_, const DevVolume& drd_, Batch& c_, const ExtShared& X_, const ExtLane& L_)
        : ctx(ctx_), dref(dref_), drd(drd_), c(c_), X(X_), L(L_), seq0(*L_.round_seq), ring(L_.ring), ring_dev(L_.ring_dev), last_wall(wall_ms()) {}

    int wait_pub(u32 r, Cnt& out)
    {
        const unsigned long long want = seq0 + r + 1;
        volatile RoundPub* e = &ring[(seq0 + r) % kRoundRing];
        const double t0 = wall_ms();
        for (u64 spin = 0; e->seq != want; ++spin) {
            if ((spin & 0xfffff) == 0xfffff) {
                // a failed kernel never publishes: look at the stream instead of spinning forever
                const hipError_t q = hipStreamQuery(c.sa);
                if (q != hipSuccess && q != hipErrorNotReady) return set_err(ctx, NECAT_ERR_DEVICE, "extension round %u failed: %s", r, hipGetErrorString(q));
                if (wall_ms() - t0 > 120e3) return set_err(ctx, NECAT_ERR_DEVICE, "extension round %u: no progress for 120 s", r);
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        out.nA = e->nA; out.nB = e->nB;
        return NECAT_OK;
    }
    void account_a(u32 r)
    {
        if (r >= a_timed.size() || !a_timed[r]) return;
        const int q = r % 4;
        const u32 nA = hist[r].nA;
        if (a_timed[r] == 2) {
            const double f = ev_ms(c.a0[q], c.a2[q]);
            ctx->tm.fused_ms += f; ctx->tm.fused_launches += 1; ctx->tm.fused_blocks += nA;
            ctx->tm.myers_blocks += nA;
            if (knob().trace & 1) fprintf(stderr, "[necat] batch@%lu round %3u: list A %7u blocks  fused DP + walk %.3f ms\n", (unsigned long)c.base, r, nA, f);
            a_timed[r] = 0;
            return;
        }
        const double mA = ev_ms(c.a0[q], c.a1[q]), tA = ev_ms(c.a1[q], c.a2[q]);
        ctx->tm.myers_ms += mA; ctx->tm.traceback_ms += tA;
        if (std::find(rc_round.begin(), rc_round.end(), r) != rc_round.end()) { ctx->tm.rc_ms += ev_ms(c.a1[q], L.ev[EV_RC_WALK_END + (r & 3)]); ctx->tm.rc_ck_ms += mA; ctx->tm.rc_launches += 1; }
        if (nA > knob().single_pass) {      // the two-pass instantiation k_myers_coop<8,16,512,8,false> (bench.py's roofline kernel)
            ctx->tm.myersA_ms += mA; ctx->tm.tracebackA_ms += tA; ctx->tm.myersA_launches += 1; ctx->tm.myersA_blocks += nA;
        }
        if (nA > ctx->tm.myersA_big_blocks) { ctx->tm.myersA_big_blocks = nA; ctx->tm.myersA_big_ms = mA; }
        ctx->tm.myers_launches += 1; ctx->tm.myers_blocks += nA;
        if (knob().trace & 1) {
            const double now = wall_ms();
            fprintf(stderr, "[necat] batch@%lu round %3u: list A %7u blocks  myers %.3f ms traceback %.3f ms | host wall since last %.3f ms\n",
                    (unsigned long)c.base, r, nA, mA, tA, now - last_wall);
            last_wall = now;
        }
        a_timed[r] = 0;
    }
    void account_b(int slot)
    {
        if (!b_pending[slot]) return;
        if (b_fused[slot]) {
            const double f = ev_ms(c.b0[slot], c.b2[slot]);
            ctx->tm.fused_ms += f; ctx->tm.fused_launches += 1; ctx->tm.fused_blocks += b_blocks[slot]; ctx->tm.myers_blocks += b_blocks[slot];
            if (knob().trace & 1) fprintf(stderr, "[necat]          list B: %7u blocks  fused DP + walk %.3f ms\n", b_blocks[slot], f);
            b_pending[slot] = false; b_fused[slot] = false;
            return;
        }
        const double mB = ev_ms(c.b0[slot], c.b1[slot]), tB = ev_ms(c.b1[slot], c.b2[slot]);
        ctx->tm.myers_ms += mB; ctx->tm.traceback_ms += tB;
        ctx->tm.myers_launches += 1; ctx->tm.myers_blocks += b_blocks[slot];
        if (knob().trace & 1) fprintf(stderr, "[necat]          list B: %7u blocks  myers %.3f ms traceback %.3f ms\n", b_blocks[slot], mB, tB);
        b_pending[slot] = false;
    }
    ExtLists lists(int j) const { return c.lists_at(j, X.task_ops); }

    // ---- What a round consists of is decided ONCE, in plan_b / plan_a: the launchers below read the plan and never a knob combination again.  A plan the product
    // library has no kernels for (a band-record path, a checkpoint pass without carries, ragged or wide blocks through the band kernels) is refused by the dispatch,
    // launch_b / launch_a, before anything of the round is launched; the cross-check build runs it through stage_extend_xcheck.inl instead.
    struct PlanB {
        int slot, cur; u32 nB, gB;
        hipStream_t sb;
        bool tail;          // a small list: one launch (ext_tail.h)
        bool use_rc;        // checkpoint pass + recomputing walk (ext_rcwalk.h); neither: band records (cross-check build)
    };
    PlanB plan_b(u32 q, u32 nB) const
    {
        PlanB p; p.slot = q & 1; p.cur = q % 4; p.nB = nB; p.gB = (nB + 63) / 64;
        // small lists (the late rounds, where a round lasts as long as its slowest chain) get alternating streams so
        // that B(q) need not queue behind B(q - 1); big ones stay in one stream - three busy chains only add contention
        p.sb = c.sb[nB < 4096 ? p.slot : 0];
        p.tail = knob().tail_fused && nB <= knob().tail_fused;
        p.use_rc = knob().rc_listb && knob().rc_carry && nB <= knob().coop_threshold;
        return p;
    }
    struct PlanA {
        u32 gA, gchunk;             // groups of 64 work indices; groups per launch of a capped band pool (NECAT_BAND_POOL_MB)
        bool wide_possible;         // NECAT_RC_MAXDIST below what a block's distance can be: some blocks are too wide for the recomputing walk
        bool use_rc;                // a big round: checkpoint pass + recomputing walk (ext_rcwalk.h); otherwise band records
        bool product;               // .. with carries, the ragged blocks on the recompute path too, no wide blocks: what the product library runs
        bool ckg_all;               // NECAT_RC_CKG_ALL (debugging): every block through the general pass k_myers_ckg
        bool merged;                // NECAT_RC_MERGE (default): the ragged blocks ride the same two launches as the full ones (k_myers_ck's ragged fast path, the walk
                                    // over the whole list) instead of a chain of their own (k_myers_ckg + walk, on stream d when the list is one chunk)
        bool fuse_frag;             // NECAT_FRAG_FUSE (default): the merged pass cuts its fragments itself (k_myers_ck flag bit 22); the round's bookkeeping - list sizes published,
                                    // the counters of the list after next reset - is then the one-wave k_round_ctl, and list B's chain of the round (which waits for a0) starts that much earlier
        bool one_chunk;             // the whole list fits the checkpoint buffer (NECAT_RC_POOL_MB)
        bool piped;                 // NECAT_RC_PIPE (default 1 = off): a big list in that many pieces, the walk of piece i on stream d beside the checkpoint pass of piece
                                    // i + 1 on stream a - the pass is bound by VALU issue, the walk by the latency of its one walker wave per 64 blocks (a third of the
                                    // pass's instruction rate), and one after the other they are the critical chain of every big round.  Measured: both kernels just
                                    // take longer side by side, 41.6 -> 43.4 - 43.9 ms per step with 2 - 4 pieces, with or without raised priority for the walk
        size_t per_ck, per_hc;      // bytes of checkpoints / of deltas per work index
        u32 rc_chunk, step_chunk;   // work indices the checkpoint buffer holds; per turn of the chunk loop (a piece when piped)
        u32 epoch, fl_all, fl_rag, fl_ck, fl_walk;      // the round's epoch; flag words of the finishing kernel, the ragged chain, the checkpoint pass, the walk
    };
    PlanA plan_a(u32 bound)
    {
        PlanA p; p.gA = (bound + 63) / 64;
        // the band pools are sized by what a round needs (round 0 of the first call sets them: 35 GB instead of the
        // 76 GB worst case "every block in list B" at E. coli size - hipMalloc costs ~13 ms per GB); with a capped pool
        // (NECAT_BAND_POOL_MB, the command-line programs: a fresh process pays 30 - 55 ms per GB of VRAM the previous one
        // dirtied) the list runs in chunks of what the pool holds, DP + walk per chunk
        p.gchunk = p.gA;
        if (knob().band_pool && (size_t)p.gA * kSlabA > knob().band_pool) p.gchunk = (u32)std::max<size_t>(1, knob().band_pool / kSlabA);
        p.wide_possible = knob().rc_maxdist < (int)((double)kOcaBlockSize * X.error * 1.1);       // (edlib_ex.c:751: no block has a larger distance)
        const bool rc_band = !knob().rc_ragged || p.wide_possible;                                  // the round still needs the band pool (whole list: slabs are indexed by work index)
        p.use_rc = knob().rcwalk && bound > knob().rcwalk && bound <= knob().coop_threshold && knob().fast == 1 && knob().coop_filter && (!rc_band || p.gchunk == p.gA);
        p.product = p.use_rc && knob().rc_carry && knob().rc_ragged && !p.wide_possible;
        // checkpoints (+ deltas) of at most knob().rc_pool bytes: a longer list goes through the buffer in several launches, one after the other on stream a
        p.per_ck = knob().rc_carry ? GeomA::Lay::kPerCk : LayA0::kPerCk; p.per_hc = knob().rc_carry ? GeomA::Lay::kPerHc : LayA0::kPerHc;
        p.rc_chunk = ck_chunk(knob().rc_pool, p.per_ck, p.per_hc, p.gA);
        p.one_chunk = p.rc_chunk >= bound;
        p.ckg_all = knob().rc_ckg_all.set;
        p.merged = knob().rc_merge && knob().rc_ragged && knob().rc_carry && !p.ckg_all;
        p.fuse_frag = knob().frag_fuse && p.use_rc && p.merged && !p.wide_possible;
        p.piped = knob().rc_pipe > 1 && p.one_chunk && p.merged && !p.wide_possible && bound >= knob().rc_pipe_min;
        p.step_chunk = p.piped ? ck_piece_step(p.gA, knob().rc_pipe) : p.rc_chunk;
        p.epoch = ++ctx->epoch & 0x3fffffu;
        p.fl_rag = p.epoch | (1u << 26); p.fl_all = knob().rc_ragged ? p.epoch | (1u << 27) : p.epoch;
        p.fl_ck = (p.merged ? p.fl_all : p.epoch) | (knob().ck_post ? 0u : 1u << 24) | (knob().rc_prio & 2u ? 1u << 23 : 0u) | (p.fuse_frag ? 1u << 22 : 0u);
        p.fl_walk = (knob().rc_ragged && p.one_chunk && !p.merged) ? p.epoch : p.fl_all;        // (the un-merged ragged blocks of a one-chunk list are walked on stream d)
        return p;
    }
    // the rounds only libnecat_hip_xcheck.so has kernels for: defined in stage_extend_xcheck.inl (cross-check build only; the product build never calls them)
    int xcheck_round_b(u32 q, const PlanB& p);
    int xcheck_launch_a(u32 r, u32 bound, const PlanA& p);
    int xcheck_round_a_band(u32 r, u32 bound, const PlanA& p);
    int xcheck_round_a_ck(u32 r, u32 bound, const PlanA& p);

    // ---- B(q): exact size known (published by A(q)'s first kernel)
    int launch_b(u32 q, u32 nB)
    {
        const PlanB p = plan_b(q, nB);
        account_b(p.slot);                                      // B(q - 2), the previous user of this slot, is done (A(q + 0) started after it)
        if (p.tail) return round_b_tail(q, p);
        if (p.use_rc) return round_b_ck(q, p);
#if NECAT_XCHECK
        return xcheck_round_b(q, p);
#else
        NECAT_RETIRED(ctx, "list B through the band-record kernels (NECAT_RC_LISTB=0 / NECAT_RC_CARRY=0 / NECAT_COOP_THRESHOLD)");
#endif
    }
    // B(q) may start: lists[q] is complete (A(q - 1) done, the counters of lists[q + 2] reset) and B(q - 2) - which appended to lists[q] and was the previous user of the
    // slot's buffers - is over.  (B(q - 1) on the other stream reads lists[q - 1] and appends to lists[q + 1]; this round appends to lists[q + 2]: four list buffers keep
    // the two apart - with three, lists[q + 2] WAS lists[q - 1])
    int begin_b(const PlanB& p)
    {
        NECAT_HIP(ctx, hipStreamWaitEvent(p.sb, c.a0[p.cur], 0));
        NECAT_HIP(ctx, hipStreamWaitEvent(p.sb, c.b2[p.slot], 0));
        return NECAT_OK;
    }
    // a small list: fragments, DP, walk and the next block's plan in one launch, the band in LDS (ext_tail.h)
    int round_b_tail(u32 q, const PlanB& p)
    {
        const int slot = p.slot;
        if (int rc = begin_b(p)) return rc;
        NECAT_HIP(ctx, hipEventRecord(c.b0[slot], p.sb));
        hipLaunchKernelGGL((k_tail_fused<kWordsB, kTWordsB, kTailCapB, kOpsB>), dim3(p.nB), dim3(kTailThreads), 0, p.sb, drd, dref, (const BlockItem*)c.itemsB[p.cur], p.nB,
                           (const u32*)(c.count + 4 * p.cur + 1), 0u, X.error, c.tasks, X.tail_match_len, X.d_err, lists((q + 2) % 4), X.stats);
        NECAT_CHECK_LAUNCH(ctx, "k_tail_fused<B>");
        NECAT_HIP(ctx, hipEventRecord(c.b1[slot], p.sb));
        NECAT_HIP(ctx, hipEventRecord(c.b2[slot], p.sb));
        b_pending[slot] = true; b_fused[slot] = true; b_blocks[slot] = p.nB;
        return NECAT_OK;
    }
    // list B through the checkpoint pass + recomputing walk as well (ext_rcwalk.h at 13 words / 16 lanes per block): one DP pass instead of two, no band records, the
    // walk on LDS.  Launches: k_ext_frag, then per chunk of the checkpoint buffer k_myers_ckf (NECAT_RC_FASTB=0: k_myers_ckg) + the walk, then the finishing k_traceback
    int round_b_ck(u32 q, const PlanB& p)
    {
        const int slot = p.slot; hipStream_t sb = p.sb;
        CkPool pool;
        int rc;
        if ((rc = ck_pool_carve<GeomB::Lay>(ctx, L.at(LB_CKPTB, slot), knob().rc_pool, p.gB, pool)) || (rc = buf_ensure(ctx, L.at(LB_WOUTB, slot), (size_t)p.gB * 64 * sizeof(WalkOut)))) return rc;
        const CkList lb = {c.itemsB[p.cur], p.nB, c.count + 4 * p.cur + 1, 0u, c.fragB[slot], c.resB[slot], c.opsB[slot], (WalkOut*)L.at(LB_WOUTB, slot).p};
        const CkEnv env = ck_env();
        if ((rc = begin_b(p))) return rc;
        const u32 epoch = ++ctx->epoch & 0x3fffffu, fl = epoch | (1u << 27);
        RoundCtl ctl; ctl.zero_bins = c.bins[slot];
        hipLaunchKernelGGL((k_ext_frag<kWordsB, kTWordsB>), dim3(grid_for((u64)p.gB * 64 * kFragSplit, 256)), dim3(256), 0, sb,
                           drd, dref, lb.items, lb.bound, lb.d_n, 0u, c.fragB[slot], ctl);
        NECAT_CHECK_LAUNCH(ctx, "k_ext_frag<B>");
        NECAT_HIP(ctx, hipEventRecord(c.b0[slot], sb));
        rc = ck_for_chunks(lb.bound, pool.chunk, CK_ITEMS, [&](const CkChunk& k) -> int {
            if (knob().rc_fastb) launch_ckf<GeomB>(lb, pool, k, sb, env, epoch);
            else launch_ckg<GeomB>(lb, pool, k, sb, env, epoch);
            if (k.last) NECAT_HIP(ctx, hipEventRecord(c.b1[slot], sb));
            launch_ck_walk<GeomB>(lb, pool, k, sb, env, fl);
            NECAT_CHECK_LAUNCH(ctx, "k_myers_ckg / k_rcwalk2<B>");
            return NECAT_OK;
        });
        if (rc) return rc;
        launch_ck_finish<GeomB>(lb, sb, (const char*)nullptr, (size_t)0, env, lists((q + 2) % 4), fl);
        NECAT_CHECK_LAUNCH(ctx, "k_traceback<B, rc>");
        NECAT_HIP(ctx, hipEventRecord(c.b2[slot], sb));
        b_pending[slot] = true; b_blocks[slot] = p.nB;
        return NECAT_OK;
    }

    // ---- A(r): grid sized by an upper bound (>= 16: step()), the kernels read the exact size of lists[r]
    int launch_a(u32 r, u32 bound)
    {
        if (knob().tail_fused && bound <= knob().tail_fused) return round_a_tail(r, bound);
        const PlanA p = plan_a(bound);
        if (p.product) return round_a_ck(r, bound, p);
#if NECAT_XCHECK
        return xcheck_launch_a(r, bound, p);
#else
        NECAT_RETIRED(ctx, "list A through the band-record kernels (NECAT_RCWALK=0, NECAT_TAIL_FUSED=0 without NECAT_RCWALK=1, NECAT_RC_CARRY=0, NECAT_RC_RAGGED=0, NECAT_RC_MAXDIST, NECAT_FAST, NECAT_COOP_*)");
#endif
    }
    // The first launch of A(r), after B(r - 2) has appended to lists[r]: the round's bookkeeping - the sizes of lists[r] published, the counters of lists[r + 2] reset - as
    // k_round_ctl (`ctl_only`; one wave, or - NECAT_ITEM_SORT - the workgroups that also put the round's staged items in place) or as part of k_ext_frag, which cuts the
    // blocks' fragments; then a0, which list B's chain of the round waits for
    int begin_a(u32 r, u32 bound, bool ctl_only)
    {
        const int cur = r % 4;
        const u32* d_nA = c.count + 4 * cur;            // [0] full blocks (front of itemsA), [2] the others (back)
        if (r >= 2) NECAT_HIP(ctx, hipStreamWaitEvent(c.sa, c.b2[r & 1], 0));
        RoundCtl ctl; ctl.count = d_nA; ctl.zero = c.count + 4 * ((r + 2) % 4); ctl.seq = seq0 + r + 1; ctl.pub = ring_dev + (seq0 + r) % kRoundRing;
        // the size-class order of lists[r] (item_order.h): k_round_ctl moves the staged items to their places - before anything reads the lists, so k_ext_frag follows it
        // where it runs.  The staged items are at most the candidates alive: `bound`, which also counts B(r - 2)'s successors
        ItemSort so;
        if (c.stage[cur]) { so.stage = c.stage[cur]; so.itemsA = c.itemsA[cur]; so.itemsB = c.itemsB[cur]; so.cls = c.cls[cur]; so.zero_cls = c.cls[(r + 2) % 4]; so.cap = c.cap; }
        if (ctl_only || so.stage) {
            const u32 g_ctl = so.stage ? std::min<u32>(grid_for(bound, kRoundCtlThreads), 1024u) : 1u;
            hipLaunchKernelGGL(k_round_ctl, dim3(g_ctl), dim3(so.stage ? kRoundCtlThreads : 64), 0, c.sa, ctl, so);
            NECAT_CHECK_LAUNCH(ctx, "k_round_ctl");
            ctl = RoundCtl();
        }
        if (!ctl_only) {
            hipLaunchKernelGGL((k_ext_frag<kWordsA, kTWordsA>), dim3(grid_for((u64)((bound + 63) / 64) * 64 * kFragSplit, 256)), dim3(256), 0, c.sa,
                               drd, dref, (const BlockItem*)c.itemsA[cur], bound, d_nA, c.cap, c.fragA, ctl);
            NECAT_CHECK_LAUNCH(ctx, "k_ext_frag<A>");
        }
        NECAT_HIP(ctx, hipEventRecord(c.a0[cur], c.sa));
        a_timed.push_back(0);
        return NECAT_OK;
    }
    // a small list: one launch for the round (ext_tail.h); the round's bookkeeping first, as a launch of its own - list B's chain of this round waits for a0, not for the fused kernel
    int round_a_tail(u32 r, u32 bound)
    {
        const int cur = r % 4;
        if (int rc = begin_a(r, bound, true)) return rc;
        hipLaunchKernelGGL((k_tail_fused<kWordsA, kTWordsA, kColsA * kWordsA, kOpsA>), dim3(bound), dim3(kTailThreads), 0, c.sa, drd, dref, (const BlockItem*)c.itemsA[cur], bound,
                           (const u32*)(c.count + 4 * cur), c.cap, X.error, c.tasks, X.tail_match_len, X.d_err, lists((r + 1) % 4), X.stats);
        NECAT_CHECK_LAUNCH(ctx, "k_tail_fused<A>");
        NECAT_HIP(ctx, hipEventRecord(c.a1[cur], c.sa));
        NECAT_HIP(ctx, hipEventRecord(c.a2[cur], c.sa));
        a_timed[r] = 2;
        return NECAT_OK;
    }
    // A big round: no NW pass and no band records - SHW with checkpoints (k_myers_ck), then the walk that recomputes its cells (ext_rcwalk.h), chunk by chunk through the
    // checkpoint buffer; then one finishing k_traceback for the whole list.  The default round is k_round_ctl, k_myers_ck, the walk, k_traceback, all on stream a.
    int round_a_ck(u32 r, u32 bound, const PlanA& p)
    {
        const int cur = r % 4;
        CkPool all;
        int rc;
        if ((rc = begin_a(r, bound, p.fuse_frag)) || (rc = pool_a(p, all))) return rc;
        const CkList la = list_a(cur, bound);
        const CkEnv env = ck_env();
        hipStream_t sd = L.sd, sw = p.piped ? sd : c.sa;            // the stream of the full blocks' walk
        int ci = 0;
        rc = ck_for_chunks(bound, p.step_chunk, CK_PADDED, [&](const CkChunk& k) -> int {
            // (a piece's checkpoints and deltas at its own place in the buffer, which holds the whole list then: the kernels index by item - lo)
            const CkPool pool = {p.piped ? all.ck + ck_piece_ck(k.lo, p.per_ck) : all.ck, p.piped ? all.hc + ck_piece_hc(k.lo, p.per_hc) : all.hc, all.chunk};      // (chunk: carried along, the wrappers read ck and hc only)
            if (!p.ckg_all) launch_ck<GeomA>(la, pool, k, c.sa, env, p.fl_ck, (const u64*)drd.bases, (const u64*)dref.bases);
            if (p.piped) { NECAT_HIP(ctx, hipEventRecord(L.ev[EV_PIPE_PIECE + (ci & 7)], c.sa)); NECAT_HIP(ctx, hipStreamWaitEvent(sw, L.ev[EV_PIPE_PIECE + (ci & 7)], 0)); }
            if (!p.merged) { if (int rcr = ragged_chain(cur, p, la, pool, k)) return rcr; }
            NECAT_CHECK_LAUNCH(ctx, "k_myers_ck");
            if (k.last) NECAT_HIP(ctx, hipEventRecord(c.a1[cur], c.sa));
            launch_ck_walk<GeomA>(la, pool, k, sw, env, p.fl_walk);
            NECAT_CHECK_LAUNCH(ctx, "k_rcwalk");
            ++ci;
            return NECAT_OK;
        });
        if (rc) return rc;
        NECAT_HIP(ctx, hipEventRecord(L.ev[EV_RC_WALK_END + (r & 3)], sw));       // a1 -> this: the walk kernel alone (account_a; of the last chunk, normally the only one)
        if (p.piped) NECAT_HIP(ctx, hipStreamWaitEvent(c.sa, L.ev[EV_RC_WALK_END + (r & 3)], 0));          // the finishing kernel reads what the walks left
        if (p.one_chunk && !p.merged) NECAT_HIP(ctx, hipStreamWaitEvent(c.sa, L.ev[EV_RAGGED_WALKED], 0));       // the ragged blocks are walked
        if ((rc = finish_a_ck(r, bound, p))) return rc;
        NECAT_HIP(ctx, hipEventRecord(c.a2[cur], c.sa));
        a_timed[r] = 1;
        return NECAT_OK;
    }
    // list A of round `cur` and what the launches of a round share, as stage_ck_round.inl's wrappers take them; the round's checkpoint pool and walk results
    CkList list_a(int cur, u32 bound) const { return {c.itemsA[cur], bound, c.count + 4 * cur, c.cap, c.fragA, c.resA, c.opsA, (WalkOut*)L.at(LB_WOUT).p}; }
    CkEnv ck_env() const { return {X.error, X.stats, c.tasks, X.task_ops ? 1 : 0, X.tail_match_len, X.d_err}; }
    int pool_a(const PlanA& p, CkPool& pool)
    {
        if (int rc = ck_pool_carve(ctx, L.at(LB_CKPT), p.per_ck, p.per_hc, knob().rc_pool, p.gA, pool)) return rc;
        return buf_ensure(ctx, L.at(LB_WOUT), (size_t)p.gA * 64 * sizeof(WalkOut));
    }
    // the ragged blocks of a chunk (the back of the work index space) when they do not ride the full blocks' launches: the general SHW pass, same checkpoints.  A tenth of
    // the blocks, few waves, latency bound: beside the full blocks' pass on stream d when the list is one chunk - and their walk there too: the full blocks' walk need not
    // wait for this pass (as long as the full blocks' own)
    int ragged_chain(int cur, const PlanA& p, const CkList& la, const CkPool& pool, const CkChunk& k)
    {
        hipStream_t sd = L.sd, sr = p.one_chunk ? sd : c.sa;
        if (p.one_chunk) NECAT_HIP(ctx, hipStreamWaitEvent(sd, c.a0[cur], 0));            // the fragments are there
        launch_ckg<GeomA>(la, pool, k, sr, ck_env(), p.ckg_all ? p.epoch : p.fl_rag);
        if (!p.one_chunk) return NECAT_OK;
        launch_ck_walk<GeomA>(la, pool, k, sd, ck_env(), p.fl_rag);
        NECAT_HIP(ctx, hipEventRecord(L.ev[EV_RAGGED_WALKED], sd));
        return NECAT_OK;
    }
    // the finishing launch of a checkpoint-pass round: the walked blocks' results joined to their tasks, the successors appended to lists[r + 1]
    int finish_a_ck(u32 r, u32 bound, const PlanA& p)
    {
        rc_round.push_back(r);
        launch_ck_finish<GeomA>(list_a(r % 4, bound), c.sa, (const char*)L.at(LB_MAT).p, kSlabA, ck_env(), lists((r + 1) % 4), p.fl_all);
        NECAT_CHECK_LAUNCH(ctx, "k_traceback<A, rc>");
        return NECAT_OK;
    }
    // the sizes of lists[rnd] have been published (round 0: k_ext_init filled them): step() will not wait
    bool ready() const { return rnd == 0 || ring[(seq0 + rnd - 1) % kRoundRing].seq == seq0 + rnd; }
    // one turn of the round loop: the published sizes of lists[rnd], list B of round rnd - 1, list A of round rnd
    int step()
    {
        int rc;
        u32 bound = c.n + 16;
        if (rnd > 0) {
            Cnt prev;
            if ((rc = wait_pub(rnd - 1, prev))) { over = true; return rc; }          // A(rnd - 1) has started: A(rnd - 2) and B(rnd - 3) are done
            hist.push_back(prev);
            if (rnd >= 2) account_a(rnd - 2);
            const u32 nB2 = rnd >= 2 ? hist[rnd - 2].nB : 0;     // B(rnd - 2) may still be running: its successors join lists[rnd]
            const u64 alive = (u64)prev.nA + prev.nB + nB2;
            if (alive * 100 < (u64)c.n * knob().ext_overlap_pct) tail = true;
            if (alive == 0) { over = tail = true; return NECAT_OK; }          // nothing alive
            if (prev.nB) { if ((rc = launch_b(rnd - 1, prev.nB))) { over = true; return rc; } }
            bound = prev.nA + nB2 + 16;                     // work indices: the full blocks rounded up to 16, then the others
        }
        if ((rc = launch_a(rnd, bound))) { over = true; return rc; }
        launched = ++rnd;
        return NECAT_OK;
    }
    // nothing of this batch is in flight any more (two lanes: the scheduler polls this instead of blocking in finish())
    bool drained() const
    {
        for (hipStream_t s : {c.sa, c.sb[0], c.sb[1]}) if (hipStreamQuery(s) == hipErrorNotReady) { (void)hipGetLastError(); return false; }      // ("not ready" is no error to the next launch check)
        return true;
    }
    // drain whatever is still in flight, the last rounds' accounts; rc = what step() returned
    int finish(int rc)
    {
        over = tail = true;
        hipError_t e1 = hipStreamSynchronize(c.sa), e2 = hipStreamSynchronize(c.sb[0]), e3 = hipStreamSynchronize(c.sb[1]);
        *L.round_seq = seq0 + launched;
        if (!rc) for (hipError_t e : {e1, e2, e3}) if (e != hipSuccess) rc = set_err(ctx, NECAT_ERR_DEVICE, "extension rounds: %s", hipGetErrorString(e));
        if (rc) return rc;
        if (launched) {
            // the last launched round published too (its lists are empty unless the loop ended on an error)
            Cnt last; if ((rc = wait_pub(launched - 1, last))) return rc;
            if (hist.size() < launched) hist.push_back(last);
            if (launched >= 2) account_a(launched - 2);
            account_a(launched - 1);
        }
        account_b(0); account_b(1);
        for (const Cnt& h : hist) ctx->tm.rounds += (h.nA + h.nB) ? 1 : 0;
        return NECAT_OK;
    }
    // all rounds, one after the other (one lane)
    int run()
    {
        int rc = NECAT_OK;
        while (!over && !(rc = step())) {}
        return finish(rc);
    }
};
#if NECAT_XCHECK
#include "stage_extend_xcheck.inl"
#endif
}  // namespace

namespace {
// outputs of the alignment-keeping mode (necat_onc_align_batch)
struct AlignOut {
    necat_alignment* aln = nullptr;
    std::vector<std::pair<u8*, u64>> parts;     // one pinned block of columns per batch
    u64 total = 0;
    std::vector<u64> off;
    bool defer_copy = false;    // the columns' device-to-host copy runs on ctx->stream_copy and is NOT waited for: the caller
                                // synchronises that stream before it reads (or frees) the blocks
    const u64* sub_off = nullptr;   // per candidate: its subject is c.ssize bases from this base of sequence c.sid on (a contig's segment, necat_ctg_extend_batch)
};

struct DevOut { const necat_m4* d = nullptr; uint64_t n = 0; };      // records left on the device (sharded calls gather them there)
// read-to-reference mapping (necat_map_reference): every candidate aligned against its stretch of the reference (rm_window), and
// instead of the filtered records every candidate's own record + flag come back, with the candidates: the caller's loop decides
struct RmOut { std::vector<necat_candidate> cands; std::vector<necat_m4> m4; std::vector<u8> ok; std::vector<u64> group_off; };

int ext_streams(necat_ctx* ctx, bool with_copy = false)
{
    // NECAT_SERIAL=1 (profiling): the four streams of the extension rounds are ONE stream, so that every kernel has the chip to itself and its
    // duration is its own work, not its wait for wave slots behind the other chains (tools/r04_profile.sh: the exclusive-time table)
    if (ctx->knobs.serial && !ctx->stream_a) { ctx->stream_a = ctx->stream_b = ctx->stream_c = ctx->stream_d = ctx->stream; ctx->serial_streams = true; }
    // NECAT_STREAM_GRAPH=1 (default): necat_ctx_create made the streams this context's knobs can launch on (ctx_streams, necat_hip.hip); only the copy stream is made here
    if (ctx->graph_streams) {
        if (with_copy && !ctx->stream_copy && hipStreamCreate(&ctx->stream_copy) != hipSuccess) return set_err(ctx, NECAT_ERR_DEVICE, "hipStreamCreate failed");
        return NECAT_OK;
    }
    // NECAT_STREAM_PRIO=1: the streams of list B and of the ragged / wide blocks at the device's highest priority - their kernels are small and sit
    // behind list A's issue-bound launches (k_ext_frag<13,25>: 0.03 ms alone, 0.5 ms in the round), which delays the chain that trails list A
    // (= 2: list A's stream instead - its chain is the round's critical one)
    const int prio = ctx->knobs.stream_prio;
    int least = 0, greatest = 0;
    if (prio && hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
    // (the copy stream - deferred column copies of the consensus loop - only for the calls that use it: every stream is a share of the runtime's hardware queues,
    // GPU_MAX_HW_QUEUES, and kernels of streams that share a queue run one after the other; with the second lane's two streams a context has eight)
    for (hipStream_t* st : {&ctx->stream_a, &ctx->stream_b, &ctx->stream_c, &ctx->stream_d, &ctx->stream_copy}) {
        if (*st || (st == &ctx->stream_copy && !with_copy)) continue;
        const bool high = prio && greatest != least && (prio == 2 ? st == &ctx->stream_a : (st == &ctx->stream_b || st == &ctx->stream_c || st == &ctx->stream_d));
        if ((high ? hipStreamCreateWithPriority(st, hipStreamDefault, greatest) : hipStreamCreate(st)) != hipSuccess) return set_err(ctx, NECAT_ERR_DEVICE, "hipStreamCreate failed");
    }
    return NECAT_OK;
}

// One call of the extension loop, cut into its steps; extend_impl runs them in order.  Nothing here waits for the device inside a batch's rounds (BatchRun).
struct ExtendCall {
    necat_ctx* ctx; const necat_volume* ref; const necat_volume* reads; int read_start_id, ref_start_id;
    const necat_candidate* cands; uint64_t n; const necat_map_options* opt; int tail_match_len;
    AlignOut* ao; const DevCands* dev; RmOut* rm;      // dev != nullptr (necat_map_pair): the candidates are this library's own, still on the device
    hipStream_t s; DevVolume dref, drd;
    std::vector<u32> bsize; u32 cap = 64, groups = 2; int nlanes = 1;      // the batch plan
    // the candidate-wide arrays (SC_EXT_CAND)
    necat_candidate* d_cands; necat_m4* d_m4; necat_m4* d_out; u64* d_goff;
    u32* d_outcnt;          // [0..1] output counter, [2 + 32 l .. 17 + 32 l] list counters (4 buffers x 4) of lane l < kMaxExtLanes
    int* d_err; u8* d_ok;
    u64* d_sub = nullptr;   // AlignOut::sub_off on the device
    u32* d_perm = nullptr;  // the candidates by expected chain length, longest first (several batches)
    ExtLane lane[kMaxExtLanes]; Batch kb[kMaxExtLanes]; ExtShared X;
    std::vector<u64> goff;  // groups of equal qid for the containment filter
    uint64_t next_base = 0; size_t started = 0;        // the candidates / batches handed to start_batch so far
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();

    void tick(const char* what)
    {
        if (!(knob().trace & 2)) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[necat] extend %-28s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    }
    int validate() const
    {
        if (n >= (1ULL << 31)) return set_err(ctx, NECAT_ERR_ARG, "too many candidates in one call");
        for (uint64_t i = 0; i < (dev ? 0 : n); ++i) {
            const necat_candidate& c = cands[i];
            const int64_t lq = (int64_t)c.qid - read_start_id, ls = (int64_t)c.sid - ref_start_id;
            if (lq < 0 || (uint64_t)lq >= reads->nseq || ls < 0 || (uint64_t)ls >= ref->nseq)
                return set_err(ctx, NECAT_ERR_ARG, "candidate %lu refers to a read outside the volumes", (unsigned long)i);
            const u64 slen = ref->h_seq_off[ls + 1] - ref->h_seq_off[ls];
            const bool sfits = ao && ao->sub_off ? ao->sub_off[i] <= slen && c.ssize <= slen - ao->sub_off[i] && c.ssize < (1ULL << 31) : c.ssize == slen;
            if (c.qsize != reads->h_seq_off[lq + 1] - reads->h_seq_off[lq] || !sfits || c.qoff > c.qsize || c.soff > c.ssize)
                return set_err(ctx, NECAT_ERR_ARG, "candidate %lu has inconsistent sizes/anchor", (unsigned long)i);
        }
        return NECAT_OK;
    }
    // the timers of the call, its begin event
    int begin_call()
    {
        NECAT_HIP(ctx, hipSetDevice(ctx->device));
        s = ctx->stream; dref = dev_view(ref); drd = dev_view(reads);
        ctx->tm.myers_ms = ctx->tm.traceback_ms = 0; ctx->tm.myers_launches = ctx->tm.myers_blocks = ctx->tm.rounds = 0;
        ctx->tm.myers_word_updates = ctx->tm.myers_cells_bases = ctx->tm.myers_band_words = 0;
        ctx->tm.myersA_ms = ctx->tm.tracebackA_ms = 0; ctx->tm.myersA_launches = ctx->tm.myersA_blocks = 0;
        ctx->tm.myersA_big_ms = 0; ctx->tm.myersA_big_blocks = 0;
        ctx->tm.fused_ms = 0; ctx->tm.fused_launches = ctx->tm.fused_blocks = 0;
        ctx->tm.rc_ms = ctx->tm.rc_ck_ms = 0; ctx->tm.rc_launches = ctx->tm.rc_blocks = ctx->tm.rc_words = 0;
        NECAT_HIP(ctx, hipEventRecord(ctx->ev[EV_CALL_BEGIN], s));
        return NECAT_OK;
    }
    // Batches of <= 786 432 candidates: every batch ends in ~20 latency-bound rounds, so fewer and bigger is better
    // (yeast-size: 654 -> 615 ms against 393 216); their band records need <= 103 GB for list A + a few GB for list B
    // of the 288 GB (NECAT_BATCH overrides)
    // Two lanes (NECAT_EXT_OVERLAP, default on; not in the alignment-keeping mode, whose batches hand columns to the host in between): two batches run their
    // rounds side by side.  A round is a chain of kernels (fragments -> pass -> walk -> finish) each of which drains before the next ramps up - 0.14 + 0.21 ms of a
    // 110 k-block round's 1.0 ms (NOTES_r05 6) - and a batch ends in ~ 15 rounds that are one block's dependent chain each whatever their size; the other lane's
    // kernels fill both.  Yeast size (four batches): 300.7 -> 278 - 283 ms per step.  NECAT_EXT_OVERLAP_MIN > 0 cuts ONE batch of at least that many candidates in
    // two for the same effect (E. coli size, first batch = the 20 % longest chains: 36.8 - 39.6 against 38.8 - 39.3 ms - not a reliable gain, not the default: knobs.h).
    void plan_batches()
    {
        const bool overlap = knob().ext_overlap && !ao && !ctx->serial_streams;
        uint64_t n_batches = (n + knob().batch_cap - 1) / knob().batch_cap;
        if (overlap && n_batches == 1 && knob().ext_overlap_min && n >= knob().ext_overlap_min) n_batches = 2;
        // batch sizes: equal shares, or - one batch cut in two - NECAT_EXT_OVERLAP_SPLIT per cent (default 20) of the candidates in the first
        if (n) {
            const bool cut = overlap && (n + knob().batch_cap - 1) / knob().batch_cap == 1 && n_batches == 2;
            const u64 share = cut ? std::min<u64>(n, std::max<u64>(64, (n * knob().ext_overlap_split / 100 + 63) & ~63ULL)) : (((n + n_batches - 1) / n_batches) + 63) & ~63ULL;
            for (u64 at = 0; at < n;) { const u64 m = std::min<u64>(n - at, cut && at ? n - at : share); bsize.push_back((u32)m); at += m; }
        }
        cap = n ? (*std::max_element(bsize.begin(), bsize.end()) + 63) & ~63u : 64u;
        nlanes = overlap && bsize.size() > 1 && knob().ext_lanes > 1 ? (int)std::min<uint64_t>(knob().ext_lanes, bsize.size()) : 1;
        groups = cap / 64 + 1;
    }
    // the candidate-wide arrays, carved from one arena; the candidates uploaded, counters and error flag zeroed
    int carve_candidates()
    {
        const bool sub = ao && ao->sub_off;
        const size_t cand_bytes = n * sizeof(necat_candidate) + 2 * n * sizeof(necat_m4) + ((n + 63) & ~63ULL) + (n + 1) * 8 + 2048 + (sub ? n * 8 + 64 : 0);
        if (int rc = buf_ensure(ctx, ctx->scratch[SC_EXT_CAND], cand_bytes)) return rc;
        char* cb = (char*)ctx->scratch[SC_EXT_CAND].p;
        d_cands = (necat_candidate*)cb; cb += n * sizeof(necat_candidate);
        d_m4 = (necat_m4*)cb; cb += n * sizeof(necat_m4);
        d_out = (necat_m4*)cb; cb += n * sizeof(necat_m4);
        d_goff = (u64*)cb; cb += (n + 1) * 8;           // (at most one group per candidate)
        d_outcnt = (u32*)cb; cb += 1024;
        d_err = (int*)cb; cb += 64;
        d_ok = (u8*)cb; cb += (n + 63) & ~63ULL;
        if (sub) { d_sub = (u64*)cb; NECAT_HIP(ctx, hipMemcpyAsync(d_sub, ao->sub_off, n * 8, hipMemcpyHostToDevice, s)); }
        NECAT_HIP(ctx, hipMemcpyAsync(d_cands, dev ? dev->d : cands, n * sizeof(necat_candidate), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        static_assert((2 + 32 * (kMaxExtLanes - 1) + 16) * 4 <= 1024, "the lanes' list counters");
        NECAT_HIP(ctx, hipMemsetAsync(d_outcnt, 0, 1024 + 64, s));        // (the counters and the error flag behind them)
        return NECAT_OK;
    }
    int lane_arenas()
    {
        for (int l = 0; l < nlanes; ++l) {
            int rc;
            if ((rc = ext_lane(ctx, l, lane[l])) ||
                (rc = buf_ensure(ctx, lane[l].at(LB_TASKS), (size_t)cap * sizeof(ExtTask) + 64)) ||
                (rc = buf_ensure(ctx, lane[l].at(LB_LISTS), (size_t)cap * (10 + (item_sort() ? 4 : 0)) * sizeof(BlockItem) + 2 * 4096 + 4 * kItemClsBytes + 64)) ||
                (rc = buf_ensure(ctx, lane[l].at(LB_FRAG), (size_t)groups * 64 * (kFragWordsA + 2 * kFragWordsB) * 8)) ||
                (rc = buf_ensure(ctx, lane[l].at(LB_OPS), (size_t)groups * 64 * (kOpsA + 2 * kOpsB))) ||
                (rc = buf_ensure(ctx, lane[l].at(LB_RES), (size_t)groups * 64 * 3 * sizeof(BlockResult)))) return rc;
        }
        return NECAT_OK;
    }
    // Several batches: every batch runs as many rounds as its longest chain of blocks and ends in latency-bound rounds,
    // so the candidates are dealt to the batches by expected chain length (what is left of the two reads beyond the
    // anchor, in blocks), longest first: the first batch has the ~30-round chains, the last ones a handful of rounds.
    int order_by_chain_length()
    {
        if (bsize.size() <= 1 || ao || !knob().ext_overlap_order) return NECAT_OK;
        // on the device (k_len_order): the candidates may never have been on the host (necat_map_pair), and a host counting sort of
        // millions of 88-byte records costs more than a batch's first rounds
        if (int rc = buf_ensure(ctx, ctx->scratch[SC_EXT_PERM], n * 4 + 2 * kLenBins * 4 + 64)) return rc;
        d_perm = (u32*)ctx->scratch[SC_EXT_PERM].p;
        u32* d_cur = d_perm + n;
        NECAT_HIP(ctx, hipMemsetAsync(d_cur, 0, kLenBins * 4, s));
        hipLaunchKernelGGL(k_len_order<0>, dim3(grid_for(n, 256, 1u << 23)), dim3(256), 0, s, (const necat_candidate*)d_cands, (u32)n, d_cur, (u32*)nullptr);
        u32 cnt[kLenBins], start[kLenBins];
        NECAT_HIP(ctx, hipMemcpyAsync(cnt, d_cur, sizeof cnt, hipMemcpyDeviceToHost, s));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        u32 run = 0;
        for (int b = 0; b < kLenBins; ++b) { start[b] = run; run += cnt[b]; }
        NECAT_HIP(ctx, hipMemcpyAsync(d_cur, start, sizeof start, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_len_order<1>, dim3(grid_for(n, 256, 1u << 23)), dim3(256), 0, s, (const necat_candidate*)d_cands, (u32)n, d_cur, d_perm);
        NECAT_CHECK_LAUNCH(ctx, "k_len_order");
        NECAT_HIP(ctx, hipStreamSynchronize(s));       // `start` is a local
        return NECAT_OK;
    }
    // NECAT_ITEM_SORT: the ragged list-A items and the list-B items of every round in size-class order (item_order.h).  The cross-check build appends in place: its
    // band-record rounds order list B themselves (stage_extend_xcheck.inl)
    bool item_sort() const { return !NECAT_XCHECK && knob().item_sort != 0; }
    // a lane's arenas, streams and events as the Batch its rounds run on
    int bind(Batch& k, const ExtLane& E, int l)
    {
        k.tasks = (ExtTask*)E.at(LB_TASKS).p;
        BlockItem* q = (BlockItem*)E.at(LB_LISTS).p;
        for (int j = 0; j < 4; ++j) { k.itemsA[j] = q + (size_t)(2 * j) * cap; k.itemsB[j] = q + (size_t)(2 * j + 1) * cap; }
        k.fragA = (u64*)E.at(LB_FRAG).p;
        k.opsA = (u8*)E.at(LB_OPS).p;
        k.resA = (BlockResult*)E.at(LB_RES).p;
        for (int j = 0; j < 2; ++j) {
            k.sortedB[j] = q + (size_t)(8 + j) * cap; k.bins[j] = (u32*)(q + 10 * (size_t)cap) + 1024 * j;
            k.fragB[j] = k.fragA + (size_t)groups * 64 * (kFragWordsA + j * kFragWordsB);
            k.opsB[j] = k.opsA + (size_t)groups * 64 * (kOpsA + j * kOpsB);
            k.resB[j] = k.resA + (size_t)groups * 64 * (1 + j);
        }
        k.count = d_outcnt + 2 + 32 * l; k.cap = cap;
        k.sa = E.sa; k.sb[0] = E.sb[0]; k.sb[1] = E.sb[1];
        for (int j = 0; j < 4; ++j) { k.a0[j] = E.ev[EV_A0 + kEvListStride * j]; k.a1[j] = E.ev[EV_A1 + kEvListStride * j]; k.a2[j] = E.ev[EV_A2 + kEvListStride * j]; }
        for (int j = 0; j < 2; ++j) { k.b0[j] = E.ev[EV_B0 + kEvListStride * j]; k.b1[j] = E.ev[EV_B1 + kEvListStride * j]; k.b2[j] = E.ev[EV_B2 + kEvListStride * j]; }
        NECAT_HIP(ctx, hipMemsetAsync(k.bins[0], 0, 2 * 4096, k.sa));     // size-sort counters of list B: reset by the kernels after every use
        // size-class order: a staging array and the class words per list buffer, behind the rest of the arena (start_batch zeroes the class words)
        BlockItem* const q2 = (BlockItem*)((char*)(q + 10 * (size_t)cap) + 2 * 4096);
        for (int j = 0; j < 4; ++j) {
            k.stage[j] = item_sort() ? q2 + (size_t)j * cap : nullptr;
            k.cls[j] = item_sort() ? (u32*)(q2 + 4 * (size_t)cap) + (size_t)j * (kItemClsBytes / 4) : nullptr;      // (cap is a multiple of 64: the class words start on a 128-byte line)
        }
        k.base = 0; k.n = 0;
        return NECAT_OK;
    }
    // what every round of every batch reads; the work counters, kStatSlots copies (stat_add, ext_kernels.h)
    int bind_shared()
    {
        if (int rc = buf_ensure(ctx, ctx->scratch[SC_STATS], kStatBytes)) return rc;
        NECAT_HIP(ctx, hipMemsetAsync(ctx->scratch[SC_STATS].p, 0, kStatBytes, s));
        X.d_cands = d_cands; X.d_m4 = d_m4; X.d_ok = d_ok; X.d_err = d_err; X.stats = (unsigned long long*)ctx->scratch[SC_STATS].p;
        X.error = opt->error; X.tail_match_len = tail_match_len; X.min_align = opt->align_size_cutoff;
        X.read_start_id = read_start_id; X.ref_start_id = ref_start_id; X.reads_off = reads->seq_off; X.ref_off = ref->seq_off;
        return NECAT_OK;
    }
    // alignment-keeping mode, before a batch starts: the column region of every task - left stream (<= qoff + soff columns) then right stream
    // (<= what is left of both reads from the anchor the left extension moved back)
    int plan_columns(const Batch& k, const u64** d_ops_base)
    {
        std::vector<u64> base(k.n + 1, 0);
        for (u32 i = 0; i < k.n; ++i) {
            const necat_candidate& c = cands[k.base + i];
            base[i + 1] = base[i] + ((c.qsize + c.ssize + c.qoff + c.soff + 64) / 32 + 2) * 8;      // bytes: 2 bits per column
        }
        if (int rc = buf_ensure(ctx, ctx->scratch[SC_EXT_COLS], base[k.n] + (size_t)(k.n + 1) * 8 + 64)) return rc;
        X.task_ops = (u8*)ctx->scratch[SC_EXT_COLS].p;
        u64* d_base = (u64*)(X.task_ops + ((base[k.n] + 63) & ~63ULL));
        NECAT_HIP(ctx, hipMemcpyAsync(d_base, base.data(), (size_t)k.n * 8, hipMemcpyHostToDevice, k.sa));
        NECAT_HIP(ctx, hipStreamSynchronize(k.sa));
        *d_ops_base = d_base;
        return NECAT_OK;
    }
    // The next batch on lane l: its list counters zeroed, its first blocks appended to lists[0] by k_ext_init; and, while those first kernels run (once per call),
    // the groups of equal qid for the containment filter (candidates arrive grouped per read: pm_worker.c:100-140)
    int start_batch(int l)
    {
        Batch& b = kb[l];
        b.base = next_base; b.n = bsize[started++]; next_base += b.n;
        NECAT_HIP(ctx, hipMemsetAsync(b.count, 0, 64, b.sa));
        if (b.cls[0]) NECAT_HIP(ctx, hipMemsetAsync(b.cls[0], 0, 4 * kItemClsBytes, b.sa));
        const u64* d_ops_base = nullptr;
        if (ao) if (int rc = plan_columns(b, &d_ops_base)) return rc;
        hipLaunchKernelGGL(k_ext_init, dim3(grid_for(b.n, 256)), dim3(256), 0, b.sa, (const necat_candidate*)d_cands, b.n, (u32)b.base,
                           read_start_id, ref_start_id, X.reads_off, X.ref_off, b.tasks, b.lists_at(0), d_ops_base, (const u32*)d_perm, rm ? 1 : 0, (const u64*)d_sub);
        NECAT_CHECK_LAUNCH(ctx, "k_ext_init");
        if (goff.empty() && dev) goff = dev->group_off;
        if (goff.empty() && !ao) {
            goff.push_back(0);
            for (uint64_t i = 1; i < n; ++i) if (cands[i].qid != cands[i - 1].qid) goff.push_back(i);
            goff.push_back(n);
        }
        return NECAT_OK;
    }
    // a finished batch's records (M4 + flag per candidate)
    void launch_result(const Batch& b)
    {
        hipLaunchKernelGGL(k_ext_result, dim3(grid_for(b.n, 256)), dim3(256), 0, b.sa, (const ExtTask*)b.tasks, b.n, (const necat_candidate*)d_cands,
                           opt->align_size_cutoff, d_m4, d_ok, rm ? 1 : 0);
    }
    // ---- several lanes: batch i + 1 starts on a free lane once batch i is in its tail (BatchRun::tail); ONE host thread turns all round loops,
    // whichever has its next list sizes published (BatchRun::ready) - the host still never waits for the device inside a loop
    int run_lanes()
    {
        struct LaneRun { std::unique_ptr<BatchRun> run; int state = 0; int rc = NECAT_OK; u32 polls = 0; };      // state: 0 free, 1 in its rounds, 2 draining, 3 its result kernel in flight
        LaneRun lr[kMaxExtLanes];
        const uint64_t n_batches = bsize.size();
        uint64_t done = 0;
        int last = -1;                              // the lane of the batch started last
        int err = NECAT_OK;
        u64 idle = 0; double t_idle = wall_ms();
        while (done < n_batches && !err) {
            bool progressed = false;
            if (next_base < n && (last < 0 || lr[last].state != 1 || lr[last].run->tail || knob().ext_overlap_pct >= 100)) {
                for (int l = 0; l < nlanes; ++l) if (lr[l].state == 0) {
                    if ((err = start_batch(l))) break;
                    lr[l].run.reset(new BatchRun(ctx, dref, drd, kb[l], X, lane[l])); lr[l].state = 1; lr[l].rc = NECAT_OK; last = l;
                    if (knob().trace & 1) fprintf(stderr, "[necat] batch@%lu (%u candidates) starts on lane %d\n", (unsigned long)kb[l].base, kb[l].n, l);
                    progressed = true;
                    break;
                }
                if (err) break;
            }
            for (int l = 0; l < nlanes && !err; ++l) {
                LaneRun& R = lr[l];
                if (R.state == 1 && R.run->ready()) { R.rc = R.run->step(); progressed = true; if (R.run->over) R.state = 2; }
                // (a draining lane is looked at every 64th turn of the loop: three hipStreamQuery calls per turn would be the OTHER lane's launch latency)
                if (R.state == 2 && (R.rc || ((++R.polls & 63u) == 0 && R.run->drained()))) {
                    if (!(err = R.run->finish(R.rc))) {
                        // the batch's records: launched and left to an event - the host thread goes on turning the other lane's rounds instead of waiting here
                        launch_result(kb[l]);
                        if (hipGetLastError() != hipSuccess || hipEventRecord(lane[l].ev[EV_LANE_RESULT], kb[l].sa) != hipSuccess) err = set_err(ctx, NECAT_ERR_DEVICE, "k_ext_result failed");
                    }
                    R.run.reset(); R.state = err ? 0 : 3; R.polls = 0; progressed = true;
                    if (err) ++done;
                }
                if (R.state == 3 && (++R.polls & 15u) == 0) {
                    const hipError_t q = hipEventQuery(lane[l].ev[EV_LANE_RESULT]);
                    if (q == hipErrorNotReady) (void)hipGetLastError();
                    else {
                        if (q != hipSuccess) err = set_err(ctx, NECAT_ERR_DEVICE, "k_ext_result failed: %s", hipGetErrorString(q));
                        R.state = 0; ++done; progressed = true;
                    }
                }
            }
            if (progressed) { idle = 0; t_idle = wall_ms(); continue; }
            if ((++idle & 0xfffff) == 0) {
                // a failed kernel never publishes: look at the streams instead of spinning forever
                for (int l = 0; l < nlanes && !err; ++l) if (lr[l].state == 1) {
                    const hipError_t q = hipStreamQuery(kb[l].sa);
                    if (q != hipSuccess && q != hipErrorNotReady) err = set_err(ctx, NECAT_ERR_DEVICE, "extension rounds (lane %d) failed: %s", l, hipGetErrorString(q));
                }
                if (!err && wall_ms() - t_idle > 120e3) err = set_err(ctx, NECAT_ERR_DEVICE, "extension rounds: no progress for 120 s");
            }
        }
        if (err)        // nothing of a lane is in flight when its buffers are handed on
            for (int l = 0; l < nlanes; ++l) { LaneRun& R = lr[l]; if (R.state == 3) (void)hipStreamSynchronize(kb[l].sa); else if (R.state) { (void)R.run->finish(err); R.run.reset(); } }
        return err;
    }
    // ---- one lane: batch after batch
    int run_serial()
    {
        Batch& k = kb[0];
        int rc;
        while (next_base < n) {
            if ((rc = start_batch(0))) return rc;
            { BatchRun run(ctx, dref, drd, k, X, lane[0]); if ((rc = run.run())) return rc; }
            if (ao) { if ((rc = collect_alignments(k))) return rc; continue; }
            launch_result(k);
            NECAT_CHECK_LAUNCH(ctx, "k_ext_result");
            NECAT_HIP(ctx, hipStreamSynchronize(k.sa));
        }
        return NECAT_OK;
    }
    // alignment-keeping mode, after a batch's rounds: per-candidate results + the batch's alignment columns, packed in candidate order
    int collect_alignments(const Batch& k)
    {
        int rc;
        necat_alignment* d_aln = (necat_alignment*)d_m4;          // the M4 arrays are not used in this mode
        u32* d_len = (u32*)d_out;
        hipLaunchKernelGGL(k_ext_alignment, dim3(grid_for(k.n, 256)), dim3(256), 0, k.sa, (const ExtTask*)k.tasks, k.n, 0u,
                           opt->align_size_cutoff, d_aln, d_len);
        NECAT_CHECK_LAUNCH(ctx, "k_ext_alignment");
        std::vector<u32> len(k.n);
        NECAT_HIP(ctx, hipMemcpyAsync(len.data(), d_len, (size_t)k.n * 4, hipMemcpyDeviceToHost, k.sa));
        NECAT_HIP(ctx, hipMemcpyAsync(ao->aln + k.base, d_aln, (size_t)k.n * sizeof(necat_alignment), hipMemcpyDeviceToHost, k.sa));
        NECAT_HIP(ctx, hipStreamSynchronize(k.sa));
        // every alignment starts on a 64-bit word: 32 columns per word
        std::vector<u64> off(k.n + 1, 0);
        for (u32 i = 0; i < k.n; ++i) off[i + 1] = off[i] + (len[i] + 31) / 32;
        const u64 tot = off[k.n] * 8, at = ao->total;
        for (u32 i = 0; i < k.n; ++i) ao->off[k.base + i] = at + off[i] * 8;
        ao->off[k.base + k.n] = at + tot;
        if (!tot) return NECAT_OK;
        const size_t need_out = tot + (size_t)(k.n + 1) * 8 + 64;
        if (ctx->copy_pending && need_out > ctx->scratch[SC_EXT_COLS_OUT].cap) {      // the buffer is about to be replaced
            NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream_copy)); ctx->copy_pending = false;
        }
        if ((rc = buf_ensure(ctx, ctx->scratch[SC_EXT_COLS_OUT], need_out))) return rc;
        if (ctx->copy_pending) { NECAT_HIP(ctx, hipStreamWaitEvent(k.sa, ctx->ev[EV_COLS_COPIED], 0)); ctx->copy_pending = false; }
        u8* d_cols = (u8*)ctx->scratch[SC_EXT_COLS_OUT].p;
        u64* d_off = (u64*)(d_cols + ((tot + 63) & ~63ULL));
        NECAT_HIP(ctx, hipMemcpyAsync(d_off, off.data(), (size_t)k.n * 8, hipMemcpyHostToDevice, k.sa));
        hipLaunchKernelGGL(k_ext_strings, dim3(grid_for((u64)k.n * 64, 256)), dim3(256), 0, k.sa, (const ExtTask*)k.tasks, k.n,
                           (const u8*)X.task_ops, (const u64*)d_off, (u64*)d_cols);
        NECAT_CHECK_LAUNCH(ctx, "k_ext_strings");
        u8* part = (u8*)result_alloc(tot);
        if (!part) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        ao->parts.emplace_back(part, tot); ao->total += tot;
        if (ao->defer_copy) {
            NECAT_HIP(ctx, hipEventRecord(ctx->ev[EV_COLS_READY], k.sa));
            NECAT_HIP(ctx, hipStreamWaitEvent(ctx->stream_copy, ctx->ev[EV_COLS_READY], 0));
            NECAT_HIP(ctx, hipMemcpyAsync(part, d_cols, tot, hipMemcpyDeviceToHost, ctx->stream_copy));
            NECAT_HIP(ctx, hipEventRecord(ctx->ev[EV_COLS_COPIED], ctx->stream_copy));
            ctx->copy_pending = true;
        } else
            NECAT_HIP(ctx, hipMemcpyAsync(part, d_cols, tot, hipMemcpyDeviceToHost, k.sa));
        NECAT_HIP(ctx, hipStreamSynchronize(k.sa));      // the batch's kernels are done (its buffers are reused next)
        return NECAT_OK;
    }
    int read_stats()
    {
        unsigned long long hs[kStatStepsBlocks + kStatStepsListB + 1] = {};
        std::vector<unsigned long long> copies((size_t)kStatSlots * kStatStride);
        NECAT_HIP(ctx, hipMemcpyAsync(copies.data(), X.stats, kStatBytes, hipMemcpyDeviceToHost, s));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        for (int c = 0; c < kStatSlots; ++c) for (int q = 0; q <= kStatStepsBlocks + kStatStepsListB; ++q) hs[q] += copies[(size_t)c * kStatStride + q];
        ctx->tm.myers_word_updates = hs[0]; ctx->tm.myers_cells_bases = hs[1]; ctx->tm.myers_band_words = hs[2];
        ctx->tm.rc_blocks = hs[3]; ctx->tm.rc_words = hs[4];
        necat_item_order_stats& io = ctx->item_order;
        io.a_issued = hs[kStatStepsIssued]; io.a_needed = hs[kStatStepsNeeded]; io.a_blocks = hs[kStatStepsBlocks];
        io.b_issued = hs[kStatStepsListB + kStatStepsIssued]; io.b_needed = hs[kStatStepsListB + kStatStepsNeeded]; io.b_blocks = hs[kStatStepsListB + kStatStepsBlocks];
        return NECAT_OK;
    }
    // the end of every call: whatever is queued on the call's stream done, extend_ms.  (The kernels' error word, copied on that stream, may be read only after this)
    int end_call()
    {
        NECAT_HIP(ctx, hipEventRecord(ctx->ev[EV_CALL_END], s));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        ctx->tm.extend_ms = ev_ms(ctx->ev[EV_CALL_BEGIN], ctx->ev[EV_CALL_END]);
        return NECAT_OK;
    }
    int kernel_error(int herr) { return herr ? set_err(ctx, NECAT_ERR_INTERNAL, "extension kernels reported error code %d", herr) : NECAT_OK; }
    // what the call hands back: nothing more (alignment-keeping mode: collect_alignments has), every candidate's record + flag (read-to-reference mapping), or the
    // records the containment filter keeps - left on the device (`devout`) or in a result block of the host
    int deliver(necat_m4** out, uint64_t* n_out, DevOut* devout)
    {
        int herr = 0;
        if (ao || rm) {
            if (rm) {
                rm->cands.resize(n); rm->m4.resize(n); rm->ok.resize(n); rm->group_off = goff;
                NECAT_HIP(ctx, hipMemcpyAsync(rm->cands.data(), d_cands, n * sizeof(necat_candidate), hipMemcpyDeviceToHost, s));
                NECAT_HIP(ctx, hipMemcpyAsync(rm->m4.data(), d_m4, n * sizeof(necat_m4), hipMemcpyDeviceToHost, s));
                NECAT_HIP(ctx, hipMemcpyAsync(rm->ok.data(), d_ok, n, hipMemcpyDeviceToHost, s));
            }
            NECAT_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, s));
            if (int rc = end_call()) return rc;
            return kernel_error(herr);
        }
        const u32 ng = (u32)goff.size() - 1;
        NECAT_HIP(ctx, hipMemcpyAsync(d_goff, goff.data(), goff.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_m4_filter, dim3(grid_for((u64)ng * 64, 256)), dim3(256), 0, s, (const necat_candidate*)d_cands, (const u64*)d_goff, ng,
                           (const necat_m4*)d_m4, d_ok, d_out, d_outcnt);
        NECAT_CHECK_LAUNCH(ctx, "k_m4_filter");
        u32 nout = 0;
        NECAT_HIP(ctx, hipMemcpyAsync(&nout, d_outcnt, 4, hipMemcpyDeviceToHost, s));
        NECAT_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, s));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        if (herr) return kernel_error(herr);
        if (devout) { devout->d = d_out; devout->n = nout; return end_call(); }
        tick("filter");
        necat_m4* res = (necat_m4*)result_alloc(std::max<size_t>(1, nout) * sizeof(necat_m4));
        if (!res) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        tick("result block");
        if (nout) NECAT_HIP(ctx, hipMemcpyAsync(res, d_out, (size_t)nout * sizeof(necat_m4), hipMemcpyDeviceToHost, s));
        if (int rc = end_call()) return rc;
        tick("copy to host");
        *out = res; *n_out = nout;
        return NECAT_OK;
    }
};

// The extension loop behind necat_extend (M4 records, containment filter) and necat_onc_align_batch (every candidate's alignment with its columns, `ao` != nullptr)
int extend_impl(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                const necat_candidate* cands, uint64_t n, const necat_map_options* opt, int tail_match_len,
                necat_m4** out, uint64_t* n_out, AlignOut* ao, const DevCands* dev = nullptr, DevOut* devout = nullptr, RmOut* rm = nullptr)
{
    int rc;
    if ((rc = ext_streams(ctx, ao && ao->defer_copy))) return rc;
    ExtendCall E{ctx, ref, reads, read_start_id, ref_start_id, cands, n, opt, tail_match_len, ao, dev, rm};
    if ((rc = E.validate())) return rc;
    E.tick("validate candidates");
    if ((rc = E.begin_call())) return rc;
    E.plan_batches();
    if ((rc = E.carve_candidates()) || (rc = E.lane_arenas()) || (rc = E.order_by_chain_length())) return rc;
    // candidates + zeroed counters are in place before the batch streams start.  (One lane whose list-A stream is the call's own, NECAT_STREAM_GRAPH=1: stream order says
    // the same, and list B's streams start behind an event of that stream - no hand-over, the host goes on queueing)
    if (E.nlanes > 1 || E.lane[0].sa != E.s) NECAT_HIP(ctx, hipStreamSynchronize(E.s));
    E.tick("buffers + upload");
    for (int l = 0; l < E.nlanes; ++l) if ((rc = E.bind(E.kb[l], E.lane[l], l))) return rc;
    if ((rc = E.bind_shared())) return rc;
    if ((rc = E.nlanes >= 2 ? E.run_lanes() : E.run_serial())) return rc;
    E.tick("rounds");
    if ((rc = E.read_stats())) return rc;
    return E.deliver(out, n_out, devout);
}
}  // namespace

int necat_extend(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                 const necat_candidate* cands, uint64_t n, const necat_map_options* opt, int tail_match_len,
                 necat_m4** out, uint64_t* n_out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ref || !reads || !opt || !out || !n_out || (n && !cands)) return NECAT_ERR_ARG;
    *out = nullptr; *n_out = 0;
    if (n == 0) return NECAT_OK;
    return extend_impl(ctx, ref, reads, read_start_id, ref_start_id, cands, n, opt, tail_match_len, out, n_out, nullptr);
}

int necat_map_pair(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                   int read_start_id, int ref_start_id, int pairwise, const necat_map_options* opt, int tail_match_len,
                   necat_m4** out, uint64_t* n_out, uint64_t* n_candidates)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ix || !ref || !reads || !opt || !out || !n_out) return NECAT_ERR_ARG;
    *out = nullptr; *n_out = 0;
    if (n_candidates) *n_candidates = 0;
    necat_map_options o = *opt;
    o.job = 1;                                   // the candidates of a mapping job: always sorted, cut to num_candidates
    DevCands dev;
    int rc = find_impl(ctx, ix, ref, reads, read_start_id, ref_start_id, pairwise, &o, nullptr, nullptr, &dev);
    if (rc) return rc;
    if (n_candidates) *n_candidates = dev.n;
    if (dev.n == 0) return NECAT_OK;
    return extend_impl(ctx, ref, reads, read_start_id, ref_start_id, nullptr, dev.n, &o, tail_match_len, out, n_out, nullptr, &dev);
}
