// stage_dalign.inl - the rescue pair's local alignment (DALIGNER around the anchor, ocda_go) on the device (necat_local_align_batch; dal_core.h, dal_kernels.h).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ ocda_go for many anchors at once

extern "C++" {
namespace {

enum DalBuf { DLB_TASKS = 0, DLB_OUT, DLB_SPEC, DLB_TASKS2, DLB_OUT2 };      // (.. 2: the second tier of dal_solve)

// New_Align_Spec's two tables on the device, made on the host as rescue::Dalign makes them: uploaded when the context sees a new error
int dal_spec(necat_ctx* ctx, double error, dal::Spec* S)
{
    const size_t n = (size_t)dal::kTrimMask + 1;
    if (!ctx->dal_buf[DLB_SPEC].p || ctx->dal_error != error) {
        const rescue::DalignSpec hs = rescue::spec_for_error(error);
        const int rc = buf_ensure(ctx, ctx->dal_buf[DLB_SPEC], 2 * n * sizeof(i16));
        if (rc) return rc;
        NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_SPEC].p, hs.table.data(), n * sizeof(i16), hipMemcpyHostToDevice, ctx->stream));
        NECAT_HIP(ctx, hipMemcpyAsync(as<i16>(ctx->dal_buf[DLB_SPEC]) + n, hs.score.data(), n * sizeof(i16), hipMemcpyHostToDevice, ctx->stream));
        NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (hs goes out of scope)
        ctx->dal_error = error; ctx->dal_ave_path = hs.ave_path;
    }
    S->ave_path = ctx->dal_ave_path; S->table = as<const i16>(ctx->dal_buf[DLB_SPEC]); S->score = S->table + n;
    return NECAT_OK;
}

// One launch of k_dal_wave as it is: two waves per task (forward, reverse), tips to d_out[2 i], d_out[2 i + 1].  The tasks are on the device already.
int dal_launch(necat_ctx* ctx, const u64* abases, const u64* bbases, const dal::Task* d_tasks, uint64_t n, const dal::Spec& S, int cap, dal::Out* d_out)
{
    const int R = dal::ring_size(cap);
    hipLaunchKernelGGL(dal::k_dal_wave, dim3((unsigned)(2 * n)), dim3(64), dal::ring_bytes(R), ctx->stream, abases, bbases, d_tasks, S, cap, R, d_out);
    NECAT_CHECK_LAUNCH(ctx, "k_dal_wave");
    return NECAT_OK;
}

// what became of n prepared tasks (dal_solve)
struct DalSolved {
    uint64_t n_tier[2] = {0, 0};      // decided at caps[0] / at caps[1]
    uint64_t n_host = 0, n_selfcheck = 0, n_over_cap = 0, n_steps = 0;
    uint32_t max_diags = 0;
    uint64_t hist[12] = {};           // jobs by their widest window w: bucket floor(log2 w), the last one open-ended
    bool out_changed = false;         // `out` is no longer what DLB_OUT holds (a later tier or the host code decided some job)
    double host_ms = 0;               // spent in the host code
};

// n tasks that lie on the device (d_tasks; a: slices of `reads`, b: of `ref`) through k_dal_wave at caps[0]; the jobs whose window outgrew it once more at caps[1]
// (ncaps == 2); what is still flagged - a window above the last capacity, a self-check - through rescue::Dalign on the slices (the volumes' words are fetched when the
// first such job turns up), its result put back as the pair of tips that decodes to it.  out: 2 n tips, flags 0.  how[i]: 0 the device decided, 1 the host code.
int dal_solve(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, const dal::Task* d_tasks, uint64_t n, double error, const int* caps, int ncaps,
              std::vector<dal::Out>& out, std::vector<u8>& how, DalSolved* sv)
{
    dal::Spec S;
    int rc = dal_spec(ctx, error, &S);
    if (rc || (rc = buf_ensure(ctx, ctx->dal_buf[DLB_OUT], 2 * n * sizeof(dal::Out)))) return rc;
    out.resize(2 * n); how.assign(n, 0);
    if ((rc = dal_launch(ctx, reads->bases, ref->bases, d_tasks, n, S, caps[0], as<dal::Out>(ctx->dal_buf[DLB_OUT])))) return rc;
    NECAT_HIP(ctx, hipMemcpyAsync(out.data(), ctx->dal_buf[DLB_OUT].p, 2 * n * sizeof(dal::Out), hipMemcpyDeviceToHost, ctx->stream));
    NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> flagged;
    for (uint64_t i = 0; i < n; ++i) {
        sv->n_steps += (uint64_t)out[2 * i].steps + (uint64_t)out[2 * i + 1].steps;
        if (out[2 * i].flag | out[2 * i + 1].flag) flagged.push_back(i); else ++sv->n_tier[0];
    }
    std::vector<dal::Task> ts;          // the flagged jobs' tasks, in the order of `flagged`
    if (!flagged.empty()) {
        sv->out_changed = true;
        // (the tasks may have been made on the device: all of them come back once, the flagged ones are picked out here)
        std::vector<dal::Task> all(n);
        NECAT_HIP(ctx, hipMemcpy(all.data(), d_tasks, n * sizeof(dal::Task), hipMemcpyDeviceToHost));
        ts.resize(flagged.size());
        for (size_t k = 0; k < flagged.size(); ++k) ts[k] = all[flagged[k]];
    }
    if (!flagged.empty() && ncaps > 1) {
        // second tier: only jobs that did not flag themselves can gain from a wider ring
        std::vector<uint64_t> again; std::vector<dal::Task> tt;
        for (size_t k = 0; k < flagged.size(); ++k) {
            const uint64_t i = flagged[k];
            if (!((out[2 * i].flag | out[2 * i + 1].flag) & (dal::kFlagStale | dal::kFlagEmpty))) { again.push_back(k); tt.push_back(ts[k]); }
        }
        if (!again.empty()) {
            const uint64_t m = again.size();
            if ((rc = buf_ensure(ctx, ctx->dal_buf[DLB_TASKS2], m * sizeof(dal::Task))) || (rc = buf_ensure(ctx, ctx->dal_buf[DLB_OUT2], 2 * m * sizeof(dal::Out)))) return rc;
            NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_TASKS2].p, tt.data(), m * sizeof(dal::Task), hipMemcpyHostToDevice, ctx->stream));
            if ((rc = dal_launch(ctx, reads->bases, ref->bases, as<const dal::Task>(ctx->dal_buf[DLB_TASKS2]), m, S, caps[1], as<dal::Out>(ctx->dal_buf[DLB_OUT2])))) return rc;
            std::vector<dal::Out> o2(2 * m);
            NECAT_HIP(ctx, hipMemcpyAsync(o2.data(), ctx->dal_buf[DLB_OUT2].p, 2 * m * sizeof(dal::Out), hipMemcpyDeviceToHost, ctx->stream));
            NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));
            std::vector<uint64_t> left; std::vector<dal::Task> tl;
            std::vector<u8> redone(flagged.size(), 0);
            for (uint64_t k = 0; k < m; ++k) {
                const uint64_t i = flagged[again[k]];
                sv->n_steps += (uint64_t)o2[2 * k].steps + (uint64_t)o2[2 * k + 1].steps;
                out[2 * i] = o2[2 * k]; out[2 * i + 1] = o2[2 * k + 1];
                if (!(o2[2 * k].flag | o2[2 * k + 1].flag)) { ++sv->n_tier[1]; redone[again[k]] = 1; }
            }
            for (size_t k = 0; k < flagged.size(); ++k) if (!redone[k]) { left.push_back(flagged[k]); tl.push_back(ts[k]); }
            flagged.swap(left); ts.swap(tl);
        }
    }
    if (!flagged.empty()) {
        const double h0 = wall_ms();
        std::vector<u64> wq, wt;
        if ((rc = fetch_words(ctx, reads, &wq)) || (rc = fetch_words(ctx, ref, &wt))) return rc;
        const rescue::DalignSpec hs = rescue::spec_for_error(error);
        const necat_host::BaseWords hq = host_view(reads, wq), ht = host_view(ref, wt);
        std::vector<u8> qseq, tseq;
        for (size_t k = 0; k < flagged.size(); ++k) {
            const uint64_t i = flagged[k];
            const dal::Task& T = ts[k];
            ++sv->n_host; how[i] = 1;
            if ((out[2 * i].flag | out[2 * i + 1].flag) & (dal::kFlagStale | dal::kFlagEmpty)) ++sv->n_selfcheck; else ++sv->n_over_cap;
            qseq.resize((size_t)T.a.len); hq.slice(T.a.s.g0, T.a.s.dir, T.a.s.comp, T.a.len, qseq.data());          // the slices the task names, as byte codes
            tseq.resize((size_t)T.b.len); ht.slice(T.b.s.g0, T.b.s.dir, T.b.s.comp, T.b.len, tseq.data());
            rescue::Dalign D(hs);
            (void)D.go((const char*)qseq.data(), (T.mida + T.k0) / 2, T.a.len, (const char*)tseq.data(), (T.mida - T.k0) / 2, T.b.len, 1);
            pair::tips_of(D.r, &out[2 * i], &out[2 * i + 1]);
        }
        sv->host_ms = wall_ms() - h0;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t w = (uint32_t)std::max(out[2 * i].max_diags, out[2 * i + 1].max_diags);
        sv->max_diags = std::max(sv->max_diags, w);
        int bkt = 0;
        while (bkt < 11 && (w >> (bkt + 1))) ++bkt;
        ++sv->hist[bkt];
    }
    return NECAT_OK;
}

// The pair's local half on the device for jobs of rescue_pair.h's form (a: slices of `reads`, b: of `ref`): their tasks go up, through dal_solve at the capacity
// NECAT_DALIGN_DIAGS names (cap), and the tips are decoded.  res[i]: job i's range on its slice, with ok, how and ident_perc; ms: upload to download without sv.host_ms.
struct PairLocal { DalSolved sv; int cap = 0; double ms = 0; };
int pair_local(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, const std::vector<pair::Job>& jobs, double error, int min_align_size, necat_dalign_result* res, PairLocal* L)
{
    const uint64_t n = jobs.size();
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    L->cap = std::min((int)knob().dalign_diags, dal::kMaxDiags);
    if (!n) return NECAT_OK;
    std::vector<dal::Task> ts(n);
    for (uint64_t i = 0; i < n; ++i) ts[i] = pair::task_of(jobs[i]);
    if (int rc = buf_ensure(ctx, ctx->dal_buf[DLB_TASKS], n * sizeof(dal::Task))) return rc;
    const double d0 = wall_ms();
    NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_TASKS].p, ts.data(), n * sizeof(dal::Task), hipMemcpyHostToDevice, ctx->stream));
    std::vector<dal::Out> out;
    std::vector<u8> how;
    if (int rc = dal_solve(ctx, ref, reads, as<const dal::Task>(ctx->dal_buf[DLB_TASKS]), n, error, &L->cap, 1, out, how, &L->sv)) return rc;
    L->ms = wall_ms() - d0 - L->sv.host_ms;
    memset(res, 0, n * sizeof *res);
    for (uint64_t i = 0; i < n; ++i) { res[i].how = how[i]; pair::decode(out[2 * i], out[2 * i + 1], min_align_size, &res[i]); }
    return NECAT_OK;
}

// The jobs through k_dal_wave, two waves each; a job whose window outgrew NECAT_DALIGN_DIAGS, or that flagged itself, is recomputed by rescue::Dalign.
int dal_run(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const necat_dalign_job* jobs, uint64_t n, double error,
            int min_align_size, necat_dalign_result* res, necat_dalign_stats* st)
{
    memset(st, 0, sizeof *st);
    const double w0 = wall_ms();
    if (!(error > 0.0 && error <= 1.0)) return set_err(ctx, NECAT_ERR_ARG, "error outside (0, 1]");
    if (n >= (1ULL << 30)) return set_err(ctx, NECAT_ERR_ARG, "2^30 jobs or more in one call");
    std::vector<pair::Job> pj(n);
    for (uint64_t i = 0; i < n; ++i) {
        const necat_dalign_job& j = jobs[i];
        SeqAt q, s;
        if (!seq_at(reads, j.qid, read_start_id, &q) || !seq_at(ref, j.sid, ref_start_id, &s) || (j.qdir != 0 && j.qdir != 1))
            return set_err(ctx, NECAT_ERR_ARG, "job %lu names a sequence outside its volume (or a strand that is neither 0 nor 1)", (unsigned long)i);
        if (q.len >= (1ULL << 30) || s.len >= (1ULL << 30)) return set_err(ctx, NECAT_ERR_ARG, "job %lu: a sequence of 2^30 bases or more", (unsigned long)i);
        if (j.qstart < 0 || (u64)j.qstart > q.len || j.sstart < 0 || (u64)j.sstart > s.len) return set_err(ctx, NECAT_ERR_ARG, "job %lu: a start outside its sequence", (unsigned long)i);
        pj[i] = pair::Job{j.qid, j.qdir, j.sid, (i64)q.begin, (i64)q.len, (i64)s.begin, 0, (i64)s.len, j.qstart, j.sstart};          // the whole subject
    }
    PairLocal L;
    if (int rc = pair_local(ctx, ref, reads, pj, error, min_align_size, res, &L)) return rc;
    const DalSolved& sv = L.sv;
    st->n_device = sv.n_tier[0]; st->n_host = sv.n_host; st->n_selfcheck = sv.n_selfcheck; st->n_over_cap = sv.n_over_cap; st->n_steps = sv.n_steps; st->max_diags = sv.max_diags;
    st->device_ms = L.ms; st->host_ms = wall_ms() - w0 - L.ms;
    if (n && (knob().trace & 2))
        fprintf(stderr, "[necat] local align: %lu jobs (%lu on the host: %lu above %d diagonals, %lu flagged), %lu steps, widest window %u; device %.2f ms, host %.2f ms\n", (unsigned long)n,
                (unsigned long)st->n_host, (unsigned long)st->n_over_cap, L.cap, (unsigned long)st->n_selfcheck, (unsigned long)st->n_steps, st->max_diags, st->device_ms, st->host_ms);
    return NECAT_OK;
}

}  // namespace
}  // extern "C++"

int necat_local_align_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const necat_dalign_job* jobs, uint64_t n,
                            double error, int min_align_size, necat_dalign_result** res, necat_dalign_stats* stats)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ref || !reads || !res || (n && !jobs)) return NECAT_ERR_ARG;
    *res = nullptr;
    necat_dalign_stats st;
    ResultOwner own;
    necat_dalign_result* r = own.own<necat_dalign_result>(result_alloc(std::max<uint64_t>(1, n) * sizeof(necat_dalign_result)));
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    const int rc = dal_run(ctx, ref, reads, read_start_id, ref_start_id, jobs, n, error, min_align_size, r, &st);
    if (rc) return rc;
    if (stats) *stats = st;
    own.release();
    *res = r;
    return NECAT_OK;
}
