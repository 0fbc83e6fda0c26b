// stage_dalign.inl - the rescue pair's local alignment (DALIGNER around the anchor, ocda_go) on the device (necat_local_align_batch; dal_core.h, dal_kernels.h).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ ocda_go for many anchors at once

extern "C++" {
namespace {

enum DalBuf { DLB_TASKS = 0, DLB_OUT, DLB_SPEC };

// New_Align_Spec's two tables on the device, made on the host as rescue::Dalign makes them: uploaded when the context sees a new error
int dal_spec(necat_ctx* ctx, double error, dal::Spec* S)
{
    const size_t n = (size_t)dal::kTrimMask + 1;
    if (!ctx->dal_buf[DLB_SPEC].p || ctx->dal_error != error) {
        const rescue::DalignSpec hs = rescue::spec_for_error(error);
        const int rc = buf_ensure(ctx, ctx->dal_buf[DLB_SPEC], 2 * n * sizeof(i16));
        if (rc) return rc;
        NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_SPEC].p, hs.table.data(), n * sizeof(i16), hipMemcpyHostToDevice, ctx->stream));
        NECAT_HIP(ctx, hipMemcpyAsync((i16*)ctx->dal_buf[DLB_SPEC].p + n, hs.score.data(), n * sizeof(i16), hipMemcpyHostToDevice, ctx->stream));
        NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (hs goes out of scope)
        ctx->dal_error = error; ctx->dal_ave_path = hs.ave_path;
    }
    S->ave_path = ctx->dal_ave_path; S->table = (const i16*)ctx->dal_buf[DLB_SPEC].p; S->score = S->table + n;
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
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<dal::Task> ts(n);
    for (uint64_t i = 0; i < n; ++i) {
        const necat_dalign_job& j = jobs[i];
        const int64_t q = (int64_t)j.qid - read_start_id, s = (int64_t)j.sid - ref_start_id;
        if (q < 0 || (uint64_t)q >= reads->nseq || s < 0 || (uint64_t)s >= ref->nseq || (j.qdir != 0 && j.qdir != 1))
            return set_err(ctx, NECAT_ERR_ARG, "job %lu names a sequence outside its volume (or a strand that is neither 0 nor 1)", (unsigned long)i);
        const u64 qb = reads->h_seq_off[q], qs = reads->h_seq_off[q + 1] - qb, sb = ref->h_seq_off[s], ss = ref->h_seq_off[s + 1] - sb;
        if (qs >= (1ULL << 30) || ss >= (1ULL << 30)) return set_err(ctx, NECAT_ERR_ARG, "job %lu: a sequence of 2^30 bases or more", (unsigned long)i);
        if (j.qstart < 0 || (u64)j.qstart > qs || j.sstart < 0 || (u64)j.sstart > ss) return set_err(ctx, NECAT_ERR_ARG, "job %lu: a start outside its sequence", (unsigned long)i);
        dal::Task& T = ts[i];
        T.a.s = j.qdir ? nw::Seq{(i64)(qb + qs - 1), -1, 1} : nw::Seq{(i64)qb, 1, 0};
        T.a.len = (int)qs;
        T.b.s = nw::Seq{(i64)sb, 1, 0};
        T.b.len = (int)ss;
        T.k0 = j.qstart - j.sstart; T.mida = j.qstart + j.sstart;
    }
    if (!n) { st->host_ms = wall_ms() - w0; return NECAT_OK; }
    const int cap = std::min((int)knob().dalign_diags, dal::kMaxDiags), R = dal::ring_size(cap);
    dal::Spec S;
    int rc = dal_spec(ctx, error, &S);
    if (rc || (rc = buf_ensure(ctx, ctx->dal_buf[DLB_TASKS], n * sizeof(dal::Task))) || (rc = buf_ensure(ctx, ctx->dal_buf[DLB_OUT], 2 * n * sizeof(dal::Out)))) return rc;
    const double d0 = wall_ms();
    NECAT_HIP(ctx, hipMemcpyAsync(ctx->dal_buf[DLB_TASKS].p, ts.data(), n * sizeof(dal::Task), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dal::k_dal_wave, dim3((unsigned)(2 * n)), dim3(64), dal::ring_bytes(R), ctx->stream, reads->bases, ref->bases, (const dal::Task*)ctx->dal_buf[DLB_TASKS].p, S,
                       cap, R, (dal::Out*)ctx->dal_buf[DLB_OUT].p);
    NECAT_CHECK_LAUNCH(ctx, "k_dal_wave");
    std::vector<dal::Out> out(2 * n);
    NECAT_HIP(ctx, hipMemcpyAsync(out.data(), ctx->dal_buf[DLB_OUT].p, 2 * n * sizeof(dal::Out), hipMemcpyDeviceToHost, ctx->stream));
    NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    st->device_ms = wall_ms() - d0;
    std::vector<u64> wq, wt;          // the volumes' words on the host: fetched when the first job is handed back
    std::vector<u8> qseq, tseq;
    rescue::DalignSpec hs;
    for (uint64_t i = 0; i < n; ++i) {
        const dal::Out &f = out[2 * i], &b = out[2 * i + 1];
        const necat_dalign_job& j = jobs[i];
        necat_dalign_result& r = res[i];
        memset(&r, 0, sizeof r);
        st->n_steps += (uint64_t)f.steps + (uint64_t)b.steps;
        st->max_diags = std::max(st->max_diags, (uint32_t)std::max(f.max_diags, b.max_diags));
        const int flags = f.flag | b.flag;
        if (flags) {
            ++st->n_host;
            if (flags & (dal::kFlagStale | dal::kFlagEmpty)) ++st->n_selfcheck; else ++st->n_over_cap;
            if (wq.empty()) {
                if ((rc = fetch_words(ctx, reads, &wq)) || (rc = fetch_words(ctx, ref, &wt))) return rc;
                hs = rescue::spec_for_error(error);
            }
            host_view(reads, wq).strand((int64_t)j.qid - read_start_id, j.qdir, qseq);
            host_view(ref, wt).strand((int64_t)j.sid - ref_start_id, 0, tseq);
            rescue::Dalign D(hs);
            r.ok = D.go((const char*)qseq.data(), j.qstart, (int)qseq.size(), (const char*)tseq.data(), j.sstart, (int)tseq.size(), min_align_size) ? 1 : 0;
            r.how = 1; r.qoff = D.r.abpos; r.qend = D.r.aepos; r.soff = D.r.bbpos; r.send = D.r.bepos; r.diffs = D.r.diffs; r.ident_perc = D.ident_perc;
            continue;
        }
        ++st->n_device;
        r.qoff = b.a - b.y; r.qend = f.a - f.y; r.soff = b.y; r.send = f.y; r.diffs = f.d + b.d;
        const int asize = r.qend - r.qoff, bsize = r.send - r.soff;
        r.ok = asize >= min_align_size && bsize >= min_align_size;
        if (r.ok) r.ident_perc = 100.0 - 200.0 * r.diffs / (asize + bsize);
    }
    st->host_ms = wall_ms() - w0 - st->device_ms;
    if (knob().trace & 2)
        fprintf(stderr, "[necat] local align: %lu jobs (%lu on the host: %lu above %d diagonals, %lu flagged), %lu steps, widest window %u; device %.2f ms, host %.2f ms\n", (unsigned long)n,
                (unsigned long)st->n_host, (unsigned long)st->n_over_cap, cap, (unsigned long)st->n_selfcheck, (unsigned long)st->n_steps, st->max_diags, st->device_ms, st->host_ms);
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
    necat_dalign_result* r = (necat_dalign_result*)result_alloc(std::max<uint64_t>(1, n) * sizeof(necat_dalign_result));
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    const int rc = dal_run(ctx, ref, reads, read_start_id, ref_start_id, jobs, n, error, min_align_size, r, &st);
    if (rc) { necat_free(r); return rc; }
    if (stats) *stats = st;
    *res = r;
    return NECAT_OK;
}
