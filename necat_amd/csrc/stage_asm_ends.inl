// stage_asm_ends.inl - oc2asmpm from the anchor to the record on the device (necat_asm_map_batch): the rounds of the block aligner (stage_asm_align.inl), then
// hbn_map_extend's end extension on the resident ExtTasks and columns (asm_ends_core.h) with its DALIGNER jobs through k_dal_wave (stage_dalign.inl: dal_solve).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ hbn_map_extend for many anchors at once

extern "C++" {
namespace necat {
namespace aends {

// adds the number of lanes with `bit` set to *counter (one atomic per wave); every lane of the wave calls it
NECAT_D void count_lanes(bool bit, u32* counter)
{
    const u64 m = __ballot(bit);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (u32)popc64(m));
}

// A lane per anchor: plan_ends on its finished task; the jobs of a wave's anchors take consecutive slots of `jobs` (left ends first), claimed by one atomic per wave.
__global__ void __launch_bounds__(256)
k_asm_ends_plan(const ExtTask* __restrict__ tasks, u32 n, const u64* __restrict__ qbases, const u64* __restrict__ sbases, const u8* __restrict__ cols, int min_align_size,
                double min_ident_perc, Plan* __restrict__ plans, dal::Task* __restrict__ jobs, u32* __restrict__ counts)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const bool valid = i < n;
    Plan p;
    p.state = 0;
    dal::Task T[2];
    if (valid) {
        const ExtTask t = tasks[i];
        p = plan_ends(t, qbases, sbases, reinterpret_cast<const u64*>(cols + t.ops_base), min_align_size, min_ident_perc, T);
    }
    const int left = p.state >> side_shift(0), right = p.state >> side_shift(1);
    const u64 ml = __ballot(left & kJob), mr = __ballot(right & kJob);
    u32 base = 0;
    if (lane == 0 && (ml | mr)) base = atomicAdd(counts + C_JOBS, (u32)(popc64(ml) + popc64(mr)));
    base = (u32)__shfl((int)base, 0);
    const u64 below = (1ULL << lane) - 1;
    if (left & kJob) { p.job[0] = (i32)(base + (u32)popc64(ml & below)); jobs[p.job[0]] = T[0]; }
    if (right & kJob) { p.job[1] = (i32)(base + (u32)popc64(ml) + (u32)popc64(mr & below)); jobs[p.job[1]] = T[1]; }
    if (valid) plans[i] = p;
    count_lanes(p.state & kOk, counts + C_OK);
    count_lanes(p.state & kLowIdent, counts + C_LOW_IDENT);
    for (int side = 0; side < 2; ++side) {
        const int b = p.state >> side_shift(side);
        count_lanes(b & kTried, counts + C_TRIED + side);
        count_lanes(b & kHang0, counts + C_HANG0 + side);
        count_lanes(b & kHangLong, counts + C_HANG_LONG + side);
        count_lanes(b & kNoRun, counts + C_NO_RUN + side);
    }
}

// A lane per anchor: finish_ends on the jobs' tips; the record (without ids and score: the host has them) and whether there is one.
__global__ void __launch_bounds__(256)
k_asm_ends_finish(const ExtTask* __restrict__ tasks, const AsmAnchor* __restrict__ anchors, u32 n, const Plan* __restrict__ plans, const dal::Out* __restrict__ outs,
                  necat_m4* __restrict__ recs, u8* __restrict__ kept, u32* __restrict__ counts)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    int ext[2] = {0, 0};
    if (i < n) {
        const ExtTask t = tasks[i];
        const AsmAnchor a = anchors[i];
        necat_m4 m;
        const bool has = finish_ends(t, plans[i], outs, a.qoff, a.soff, &m, ext);
        kept[i] = has ? 1 : 0;
        if (has) recs[i] = m;
    }
    count_lanes(ext[0], counts + C_EXTENDED);
    count_lanes(ext[1], counts + C_EXTENDED + 1);
}

}  // namespace aends
}  // namespace necat
}  // extern "C++"

int necat_asm_map_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id,
                        const necat_asm_plan* plans, uint64_t n, double error, int min_align_size, double min_ident_perc,
                        necat_m4** recs, uint8_t** kept, necat_asm_map_stats* stats)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ref || !reads || !recs || !kept || (n && !plans)) return NECAT_ERR_ARG;
    *recs = nullptr; *kept = nullptr;
    necat_asm_map_stats st;
    memset(&st, 0, sizeof st);
    const double w0 = wall_ms();
    if (!(error > 0.0 && error <= 1.0) || n >= (1ULL << 31)) return set_err(ctx, NECAT_ERR_ARG, "error rate / count out of range");
    NECAT_HIP(ctx, hipSetDevice(ctx->device));          // (nothing allocated yet)
    hipStream_t s = ctx->stream;
    std::vector<AsmAnchor> h;
    std::vector<uint64_t> entry;          // the plan entry of anchor k
    h.reserve(n); entry.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        const necat_asm_plan& a = plans[i];
        if (a.qoff < 0) continue;
        SeqAt q, t;
        if (!seq_at(reads, a.qid, read_start_id, &q) || !seq_at(ref, a.sid, ref_start_id, &t) || (a.sdir != 0 && a.sdir != 1))
            return set_err(ctx, NECAT_ERR_ARG, "anchor %lu refers to a read outside the volumes", (unsigned long)i);
        if ((u64)a.qoff > q.len || a.soff < 0 || (u64)a.soff > t.len || q.len >= (1ULL << 30) || t.len >= (1ULL << 30))
            return set_err(ctx, NECAT_ERR_ARG, "anchor %lu lies outside its reads", (unsigned long)i);
        AsmAnchor x; x.q = (i32)q.k; x.s = (i32)t.k; x.sdir = a.sdir; x.qoff = a.qoff; x.soff = a.soff;
        h.push_back(x); entry.push_back(i);
    }
    const uint64_t na = h.size();
    st.n_anchors = na;
    ResultOwner own;
    necat_m4* out = own.own<necat_m4>(result_alloc(std::max<uint64_t>(1, n) * sizeof(necat_m4)));
    uint8_t* keep = own.own<uint8_t>(result_alloc(std::max<uint64_t>(1, n)));
    if (!out || !keep) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    memset(out, 0, std::max<uint64_t>(1, n) * sizeof(necat_m4)); memset(keep, 0, std::max<uint64_t>(1, n));
    if (na == 0) {
        st.host_ms = wall_ms() - w0;
        if (stats) *stats = st;
        own.release();
        *recs = out; *kept = keep;
        return NECAT_OK;
    }
    if (knob().asm_lane) return set_err(ctx, NECAT_ERR_ARG, "necat_asm_map_batch needs the cooperative block aligner: NECAT_ASM_LANE=1 leaves no tasks on the device");
    double host_ms = wall_ms() - w0;
    AsmResident R;
    int rc = asm_align_rounds(ctx, ref, reads, h, error, &R);
    if (rc) return rc;
    // plans, records, flags and counters of the end extension; the jobs (at most two per anchor) and their tips in the arenas of necat_local_align_batch
    const AsmEndsArena e(na);
    if ((rc = buf_ensure(ctx, ctx->scratch[SC_ASM_OUT], e.lay.bytes())) || (rc = buf_ensure(ctx, ctx->dal_buf[DLB_TASKS], 2 * na * sizeof(dal::Task)))) return rc;
    const ArenaView E(ctx->scratch[SC_ASM_OUT], e.lay, s);
    dal::Task* d_jobs = as<dal::Task>(ctx->dal_buf[DLB_TASKS]);
    u32 counts[aends::C_COUNT];
    int herr = 0;
    NECAT_HIP(ctx, E.zero(e.counts, AsmEndsArena::kCounters));
    hipLaunchKernelGGL(aends::k_asm_ends_plan, dim3(grid_for(na, 256)), dim3(256), 0, s, (const ExtTask*)R.d_tasks, (u32)na, (const u64*)reads->bases, (const u64*)ref->bases,
                       (const u8*)R.d_cols, min_align_size, min_ident_perc, E.ptr(e.plans), d_jobs, E.ptr(e.counts));
    NECAT_CHECK_LAUNCH(ctx, "k_asm_ends_plan");
    NECAT_HIP(ctx, E.download(counts, e.counts, aends::C_COUNT));
    NECAT_HIP(ctx, hipMemcpyAsync(&herr, R.d_err, 4, hipMemcpyDeviceToHost, s));
    NECAT_HIP(ctx, hipStreamSynchronize(s));
    if (herr) return set_err(ctx, NECAT_ERR_INTERNAL, "asm aligner: the kernels reported error code %d", herr);
    const uint64_t nj = counts[aends::C_JOBS];
    if (nj > 2 * na) return set_err(ctx, NECAT_ERR_INTERNAL, "asm ends: %lu jobs for %lu anchors", (unsigned long)nj, (unsigned long)na);
    st.n_jobs = nj;
    std::vector<dal::Out> outs;          // (uploaded again below when a later tier or the host code decided a job: lives until the synchronise)
    if (nj) {
        // the first capacity, then - when it is the smaller one - the capacity of necat_local_align_batch
        const int cap2 = std::min((int)knob().dalign_diags, dal::kMaxDiags);
        const int caps[2] = {std::min((int)knob().asm_ends_diags, dal::kMaxDiags), cap2};
        std::vector<u8> how;
        DalSolved sv;
        if ((rc = dal_solve(ctx, ref, reads, d_jobs, nj, 0.35 /* hbn_align.c:9 */, caps, caps[0] < cap2 ? 2 : 1, outs, how, &sv))) return rc;
        if (sv.out_changed) NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_OUT].p, outs.data(), 2 * nj * sizeof(dal::Out), hipMemcpyHostToDevice, s));
        st.n_tier1 = sv.n_tier[0]; st.n_tier2 = sv.n_tier[1]; st.n_host = sv.n_host; st.n_steps = sv.n_steps; st.max_diags = sv.max_diags;
        for (int k = 0; k < 12; ++k) st.diag_hist[k] = sv.hist[k];
        host_ms += sv.host_ms;
    }
    hipLaunchKernelGGL(aends::k_asm_ends_finish, dim3(grid_for(na, 256)), dim3(256), 0, s, (const ExtTask*)R.d_tasks, R.d_anchor, (u32)na, E.cptr(e.plans),
                       as<const dal::Out>(ctx->dal_buf[DLB_OUT]), E.ptr(e.recs), E.ptr(e.kept), E.ptr(e.counts));
    NECAT_CHECK_LAUNCH(ctx, "k_asm_ends_finish");
    {
        std::vector<necat_m4> hr(na);
        std::vector<u8> hk(na);
        NECAT_HIP(ctx, E.download(hr.data(), e.recs, na));
        NECAT_HIP(ctx, E.download(hk.data(), e.kept, na));
        NECAT_HIP(ctx, E.download(counts, e.counts, aends::C_COUNT));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        // the ids and the chain's score are the plan's
        const double h0 = wall_ms();
        for (uint64_t k = 0; k < na; ++k) {
            if (!hk[k]) continue;
            const necat_asm_plan& a = plans[entry[k]];
            necat_m4& m = out[entry[k]];
            m = hr[k];
            m.qid = a.qid; m.sid = a.sid; m.vscore = a.score;
            keep[entry[k]] = 1;
        }
        host_ms += wall_ms() - h0;
    }
    st.n_ok = counts[aends::C_OK]; st.n_low_ident = counts[aends::C_LOW_IDENT];
    for (int side = 0; side < 2; ++side) {
        st.n_tried[side] = counts[aends::C_TRIED + side]; st.n_extended[side] = counts[aends::C_EXTENDED + side]; st.n_hang0[side] = counts[aends::C_HANG0 + side];
        st.n_hang_long[side] = counts[aends::C_HANG_LONG + side]; st.n_no_run[side] = counts[aends::C_NO_RUN + side];
    }
    st.host_ms = host_ms; st.device_ms = wall_ms() - w0 - host_ms;
    if (knob().trace & 2)
        fprintf(stderr, "[necat] asm_map: %lu anchors, %lu ok, %lu below the identity cut; ends tried %lu + %lu, extended %lu + %lu; %lu jobs: %lu at %u diagonals, %lu at %u, %lu on the host; "
                "widest window %u; device %.2f ms, host %.2f ms\n", (unsigned long)na, (unsigned long)st.n_ok, (unsigned long)st.n_low_ident, (unsigned long)st.n_tried[0],
                (unsigned long)st.n_tried[1], (unsigned long)st.n_extended[0], (unsigned long)st.n_extended[1], (unsigned long)nj, (unsigned long)st.n_tier1,
                (unsigned)knob().asm_ends_diags, (unsigned long)st.n_tier2, (unsigned)knob().dalign_diags, (unsigned long)st.n_host, st.max_diags, st.device_ms, st.host_ms);
    if (stats) *stats = st;
    own.release();
    *recs = out; *kept = keep;
    return NECAT_OK;
}
