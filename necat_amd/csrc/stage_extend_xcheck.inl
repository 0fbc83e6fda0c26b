// stage_extend_xcheck.inl - the extension rounds that only the cross-check build (libnecat_hip_xcheck.so, NECAT_XCHECK) has kernels for: the band-record paths of
// both lists (k_myers_coop / k_myers / k_myers_a16 + the band-record k_traceback forms / k_walk_wave, list B sorted by size) and the checkpoint-pass round's retired
// variants (no carries: k_myers_ck<.., false> + k_rcwalk4; ragged or wide blocks through the band kernels on stream d).  Member functions of BatchRun, declared in
// stage_extend.inl, which includes this file after the struct; its dispatch (launch_b, launch_a) calls in here with the plan it has filled and found not to be a product plan.

// ---- B(q) through band records; a capped band pool (NECAT_BAND_POOL_MB): the list in chunks of what the pool holds, DP + walk per chunk
int BatchRun::xcheck_round_b(u32 q, const BatchRun::PlanB& p)
{
    const int slot = p.slot; const u32 nB = p.nB, gB = p.gB; hipStream_t sb = p.sb;
    DevBuf& poolB = L.at(LB_MATB, slot);
    u32 gchunk = gB;
    if (knob().band_pool && (size_t)gB * kSlabB > knob().band_pool) gchunk = (u32)std::max<size_t>(1, knob().band_pool / kSlabB);
    if ((size_t)gchunk * kSlabB > poolB.cap) {
        const size_t need = (size_t)gchunk * kSlabB;
        int rc = ensure_zeroed(ctx, poolB, gchunk < gB ? need : need + need / 4, sb);
        if (rc) return rc;
    }
    const BlockItem* itB = c.itemsB[p.cur];
    const u32* d_nB = c.count + 4 * p.cur + 1;
    if (int rc = begin_b(p)) return rc;
    const u32 epoch = ++ctx->epoch & 0x3fffffu;
    const ExtLists next = lists((q + 2) % 4);
    // (below ~2 k blocks every wave is resident at once and the round lasts as long as its longest walk: order is irrelevant)
    if (nB >= 2048 && knob().sort_b) {
        hipLaunchKernelGGL(k_items_hist, dim3(grid_for(nB, 256)), dim3(256), 0, sb, itB, nB, c.bins[slot]);
        hipLaunchKernelGGL(k_items_scan, dim3(1), dim3(64), 0, sb, c.bins[slot]);
        hipLaunchKernelGGL(k_items_scatter, dim3(grid_for(nB, 256)), dim3(256), 0, sb, itB, nB, c.bins[slot], c.sortedB[slot]);
        NECAT_CHECK_LAUNCH(ctx, "k_items_sort");
        itB = c.sortedB[slot];
    }
    RoundCtl ctl; ctl.zero_bins = c.bins[slot];
    hipLaunchKernelGGL((k_ext_frag<kWordsB, kTWordsB>), dim3(grid_for((u64)gB * 64 * kFragSplit, 256)), dim3(256), 0, sb,
                       drd, dref, itB, nB, d_nB, 0u, c.fragB[slot], ctl);
    NECAT_CHECK_LAUNCH(ctx, "k_ext_frag<B>");
    NECAT_HIP(ctx, hipEventRecord(c.b0[slot], sb));
    for (u32 g0 = 0; g0 < gB; g0 += gchunk) {
        const u32 lo = g0 * 64, hi = std::min(nB, (g0 + gchunk) * 64), cn = hi - lo;       // work items of this chunk
        char* slabsB = (char*)poolB.p - (size_t)g0 * kSlabB;                              // the kernels index slabs by item / 64
        if (nB <= knob().single_pass && nB <= knob().coop_threshold)
            hipLaunchKernelGGL((k_myers_coop<kWordsB, kTWordsB, kColsB, 16, true>), dim3((cn + 3) / 4), dim3(64), 0, sb, itB, hi, d_nB, 0u,
                               (const u64*)c.fragB[slot], slabsB, kSlabB, X.error, c.resB[slot], X.stats, epoch, lo);
        else if (nB <= knob().coop_threshold)
            hipLaunchKernelGGL((k_myers_coop<kWordsB, kTWordsB, kColsB, 16>), dim3((cn + 3) / 4), dim3(64), 0, sb, itB, hi, d_nB, 0u,
                               (const u64*)c.fragB[slot], slabsB, kSlabB, X.error, c.resB[slot], X.stats, epoch | (knob().coop_filter ? 0u : 1u << 30) | (knob().fast == 0 ? 1u << 29 : 0u) | (knob().fast == 2 ? 1u << 28 : 0u), lo);
        else
            hipLaunchKernelGGL((k_myers<kWordsB, kTWordsB, kColsB, false>), dim3((cn + 63) / 64), dim3(64), 0, sb, itB, hi, d_nB, 0u,
                               (const u64*)c.fragB[slot], slabsB, kSlabB, X.error, c.resB[slot], X.stats, epoch, lo);
        NECAT_CHECK_LAUNCH(ctx, "k_myers<B>");
        if (g0 + gchunk >= gB) NECAT_HIP(ctx, hipEventRecord(c.b1[slot], sb));
#define NECAT_TB_LAUNCH(WALK) hipLaunchKernelGGL((k_traceback<kWordsB, kTWordsB, kColsB, kOpsB, false, WALK>), dim3((cn + 63) / 64), dim3(64), 0, sb, itB, hi, d_nB, 0u, \
                       (const u64*)c.fragB[slot], (const char*)slabsB, kSlabB, (const BlockResult*)c.resB[slot], c.opsB[slot], c.tasks, X.tail_match_len, \
                       (i32*)nullptr, X.d_err, next, epoch, lo)
        if (knob().walk_wave && nB <= knob().walk_wave)       // a small list: one wave per block, band records through an LDS window
            hipLaunchKernelGGL((k_walk_wave<kWordsB, kTWordsB, kOpsB>), dim3(cn), dim3(64), 0, sb, itB, hi, d_nB, 0u, (const u64*)c.fragB[slot], (const char*)slabsB, kSlabB,
                               (const BlockResult*)c.resB[slot], c.tasks, X.tail_match_len, X.d_err, next, lo);
        else if (knob().walk == 1) NECAT_TB_LAUNCH(1); else if (knob().walk == 2) NECAT_TB_LAUNCH(2); else if (knob().walk == 3) NECAT_TB_LAUNCH(3); else if (knob().walk == 4) NECAT_TB_LAUNCH(4); else NECAT_TB_LAUNCH(0);
#undef NECAT_TB_LAUNCH
        NECAT_CHECK_LAUNCH(ctx, "k_traceback<B>");
    }
    NECAT_HIP(ctx, hipEventRecord(c.b2[slot], sb));
    b_pending[slot] = true; b_blocks[slot] = nB;
    return NECAT_OK;
}

// ---- A(r) on a plan the product library refuses
int BatchRun::xcheck_launch_a(u32 r, u32 bound, const BatchRun::PlanA& p)
{
    DevBuf& mat = L.at(LB_MAT);
    if ((!p.use_rc || !knob().rc_ragged || p.wide_possible) && (size_t)p.gchunk * kSlabA > mat.cap) {      // the round needs the band pool
        const size_t need = (size_t)p.gchunk * kSlabA;
        int rc = ensure_zeroed(ctx, mat, p.gchunk < p.gA ? need : need + need / 8, c.sa);
        if (rc) return rc;
    }
    return p.use_rc ? xcheck_round_a_ck(r, bound, p) : xcheck_round_a_band(r, bound, p);
}
// band records, DP + walk per chunk of the band pool
int BatchRun::xcheck_round_a_band(u32 r, u32 bound, const BatchRun::PlanA& p)
{
    const int cur = r % 4;
    const u32 gA = p.gA, gchunk = p.gchunk, epoch = p.epoch;
    const BlockItem* itA = c.itemsA[cur];
    const u32* d_nA = c.count + 4 * cur;
    if (int rc = begin_a(r, bound, false)) return rc;
    const ExtLists next = lists((r + 1) % 4);
    for (u32 g0 = 0; g0 < gA; g0 += gchunk) {
        const u32 lo = g0 * 64, hi = std::min(gA, g0 + gchunk) * 64, cn = hi - lo;           // work indices of this chunk (the kernels know the exact list)
        char* slabsA = (char*)L.at(LB_MAT).p - (size_t)g0 * kSlabA;             // the kernels index slabs by work index / 64
        if (bound <= knob().single_pass && bound <= knob().coop_threshold)
            hipLaunchKernelGGL((k_myers_coop<kWordsA, kTWordsA, kColsA, 8, true>), dim3(cn / 8), dim3(64), 0, c.sa, itA, bound, d_nA, c.cap,
                               (const u64*)c.fragA, slabsA, kSlabA, X.error, c.resA, X.stats, epoch, lo);
        else if (bound <= knob().coop_threshold) {
            const bool f16 = knob().fast16 && knob().fast == 1 && knob().coop_filter && gchunk == gA;
            const u32 fl = epoch | (knob().coop_filter ? 0u : 1u << 30) | (knob().fast == 0 ? 1u << 29 : 0u) | (knob().fast == 2 ? 1u << 28 : 0u);
            if (f16)      // workgroups of 16 work items: 16 full blocks take the 16-block path (ext_fast16.h), anything else the general one
                hipLaunchKernelGGL((k_myers_a16<kWordsA, kTWordsA, kColsA>), dim3((bound + 15) / 16), dim3(128), 0, c.sa, itA, bound, d_nA, c.cap,
                                   (const u64*)c.fragA, slabsA, kSlabA, X.error, c.resA, X.stats, fl | 1u << 27);
            else
                hipLaunchKernelGGL((k_myers_coop<kWordsA, kTWordsA, kColsA, 8>), dim3(cn / 8), dim3(64), 0, c.sa, itA, bound, d_nA, c.cap,
                                   (const u64*)c.fragA, slabsA, kSlabA, X.error, c.resA, X.stats, fl, lo);
        }
        else
            hipLaunchKernelGGL((k_myers<kWordsA, kTWordsA, kColsA, false>), dim3(cn / 64), dim3(64), 0, c.sa, itA, bound, d_nA, c.cap,   // list A also holds last blocks <= 512 x 512
                               (const u64*)c.fragA, slabsA, kSlabA, X.error, c.resA, X.stats, epoch, lo);
        NECAT_CHECK_LAUNCH(ctx, "k_myers<A>");
        if (g0 + gchunk >= gA) NECAT_HIP(ctx, hipEventRecord(c.a1[cur], c.sa));
#define NECAT_TB_LAUNCH(WALK) hipLaunchKernelGGL((k_traceback<kWordsA, kTWordsA, kColsA, kOpsA, false, WALK>), dim3(cn / 64), dim3(64), 0, c.sa, itA, bound, d_nA, c.cap, \
                       (const u64*)c.fragA, (const char*)slabsA, kSlabA, (const BlockResult*)c.resA, c.opsA, c.tasks, X.tail_match_len, \
                       (i32*)nullptr, X.d_err, next, epoch, lo)
        if (knob().walk_wave && bound <= knob().walk_wave)
            hipLaunchKernelGGL((k_walk_wave<kWordsA, kTWordsA, kOpsA>), dim3(cn), dim3(64), 0, c.sa, itA, bound, d_nA, c.cap, (const u64*)c.fragA, (const char*)slabsA, kSlabA,
                               (const BlockResult*)c.resA, c.tasks, X.tail_match_len, X.d_err, next, lo);
        else if (knob().walk == 1) NECAT_TB_LAUNCH(1); else if (knob().walk == 2) NECAT_TB_LAUNCH(2); else if (knob().walk == 3) NECAT_TB_LAUNCH(3); else if (knob().walk == 4) NECAT_TB_LAUNCH(4); else NECAT_TB_LAUNCH(0);
#undef NECAT_TB_LAUNCH
        NECAT_CHECK_LAUNCH(ctx, "k_traceback<A>");
    }
    NECAT_HIP(ctx, hipEventRecord(c.a2[cur], c.sa));
    a_timed[r] = 1;
    return NECAT_OK;
}
// The checkpoint-pass round (round_a_ck) as it was before carries, the ragged fast path and the wide-band walk: without carries the pass is k_myers_ck<.., false> and
// the walk k_rcwalk4; NECAT_RC_RAGGED=0 sends the ragged blocks, NECAT_RC_MAXDIST the blocks k_myers_ck has flagged as too wide, through k_myers_coop + band records
// on stream d, beside the full blocks' chain (a lane-per-block walk of a tenth of the list is as long as one of the whole list: latency bound).  The same chunk loop,
// pool and wrappers as round_a_ck (stage_ck_round.inl) with this round's own pass and walk per chunk, never piped, never with fused fragments: the product's body
// stays free of the branches these variants need.
int BatchRun::xcheck_round_a_ck(u32 r, u32 bound, const BatchRun::PlanA& p)
{
    const int cur = r % 4;
    const bool carry = knob().rc_carry, ragged = knob().rc_ragged, side_chain = !ragged || p.wide_possible;
    const u32 gA = p.gA, fl_wide = p.epoch | (1u << 25);
    const BlockItem* itA = c.itemsA[cur];
    const u32* d_nA = c.count + 4 * cur;
    CkPool pool;
    int rc;
    if ((rc = begin_a(r, bound, false))) return rc;
    const ExtLists next = lists((r + 1) % 4);
    if ((rc = pool_a(p, pool))) return rc;
    const CkList la = list_a(cur, bound);
    const CkEnv env = ck_env();
    char* slabsA = (char*)L.at(LB_MAT).p;
    hipStream_t sd = L.sd;
    // one band-kernel chain over the blocks whose flag word selects them: DP + lane-per-block walk on stream d
    auto band_chain = [&](u32 fl, const char* what) -> int {
        hipLaunchKernelGGL((k_myers_coop<kWordsA, kTWordsA, kColsA, 8>), dim3(gA * 8), dim3(64), 0, sd, itA, bound, d_nA, c.cap,
                           (const u64*)c.fragA, slabsA, kSlabA, X.error, c.resA, X.stats, fl, 0u);
        hipLaunchKernelGGL((k_traceback<kWordsA, kTWordsA, kColsA, kOpsA, false, 0>), dim3(gA), dim3(64), 0, sd, itA, bound, d_nA, c.cap,
                           (const u64*)c.fragA, (const char*)slabsA, kSlabA, (const BlockResult*)c.resA, c.opsA, c.tasks, X.tail_match_len,
                           (i32*)nullptr, X.d_err, next, fl, 0u);
        NECAT_CHECK_LAUNCH(ctx, what);
        return NECAT_OK;
    };
    if (!ragged) {
        NECAT_HIP(ctx, hipStreamWaitEvent(sd, c.a0[cur], 0));            // the fragments are there
        if ((rc = band_chain(p.fl_rag, "k_myers / k_traceback<A, ragged>"))) return rc;
    }
    rc = ck_for_chunks(bound, p.rc_chunk, CK_PADDED, [&](const CkChunk& k) -> int {
        if (p.ckg_all && ragged) {}
        else if (carry) launch_ck<GeomA>(la, pool, k, c.sa, env, p.fl_ck, (const u64*)drd.bases, (const u64*)dref.bases);
        else
            hipLaunchKernelGGL((k_myers_ck<kWordsA, kTWordsA, false>), dim3(ck_grid<GeomA::G>(k.cn)), dim3(64), 0, c.sa, itA, d_nA, c.cap, (const u64*)c.fragA, pool.ck, pool.hc, X.error, c.resA, X.stats,
                               knob().rc_maxdist, k.lo, k.hi, p.epoch);
        if (ragged && !p.merged) { if (int rcr = ragged_chain(cur, p, la, pool, k)) return rcr; }
        NECAT_CHECK_LAUNCH(ctx, "k_myers_ck");
        if (k.last) NECAT_HIP(ctx, hipEventRecord(c.a1[cur], c.sa));
        if (carry) launch_ck_walk<GeomA>(la, pool, k, c.sa, env, p.fl_walk);
        else      // (k_rcwalk4: 4 lanes per block, 16 blocks per wave)
            hipLaunchKernelGGL((k_rcwalk4<kWordsA, kTWordsA, kOpsA>), dim3(ck_waves(k.cn, 16)), dim3(64), 0, c.sa, itA, d_nA, c.cap, (const u64*)c.fragA, (const ulonglong2*)pool.ck,
                               (const BlockResult*)c.resA, (const ExtTask*)c.tasks, X.task_ops ? 1 : 0, X.tail_match_len, c.opsA, la.wout, X.stats, X.d_err, k.lo, k.hi);
        NECAT_CHECK_LAUNCH(ctx, "k_rcwalk");
        return NECAT_OK;
    });
    if (rc) return rc;
    NECAT_HIP(ctx, hipEventRecord(L.ev[EV_RC_WALK_END + (r & 3)], c.sa));
    if (p.wide_possible) {
        NECAT_HIP(ctx, hipStreamWaitEvent(sd, c.a1[cur], 0));            // k_myers_ck has flagged the wide blocks
        if ((rc = band_chain(fl_wide, "k_myers / k_traceback<A, wide>"))) return rc;
    }
    if (side_chain) NECAT_HIP(ctx, hipEventRecord(L.ev[EV_SIDE_CHAIN], sd));
    if (ragged && p.one_chunk && !p.merged) NECAT_HIP(ctx, hipStreamWaitEvent(c.sa, L.ev[EV_RAGGED_WALKED], 0));       // the ragged blocks are walked
    if ((rc = finish_a_ck(r, bound, p))) return rc;
    if (side_chain) NECAT_HIP(ctx, hipStreamWaitEvent(c.sa, L.ev[EV_SIDE_CHAIN], 0));          // the round is over when both chains are
    NECAT_HIP(ctx, hipEventRecord(c.a2[cur], c.sa));
    a_timed[r] = 1;
    return NECAT_OK;
}
