// stage_nw.inl - the rescue pair's global alignment with its path on the device (necat_nw_path_batch; nw_core.h, nw_kernels.h).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ edlib_go for many ranges at once

extern "C++" {      // (templates: not in the extern "C" block the stage files are included in)
namespace {

enum NwBuf { NWB_TASKS = 0, NWB_COLS, NWB_BND, NWB_FLAGS, NWB_OPS, NWB_LEAF, NWB_OUT, NWB_PACK };

// nw::solve's four launches on the device.  Every call ends in a synchronise (the host needs the few bytes it downloads to plan the next level),
// so its wall time is the device's.
struct NwDevice {
    necat_ctx* ctx;
    const u64 *qbases, *tbases;
    necat_nw_stats* st;
    bool keep_pack = true;         // false: the caller wants no columns, finish() leaves them on the device
    std::vector<u8> pack;          // the packed columns of the last finish()
    size_t n_leaves = 0;

    template <class T> T* buf(int id) { return as<T>(ctx->nw_buf[id]); }
    int ensure(int id, size_t bytes) { return buf_ensure(ctx, ctx->nw_buf[id], bytes + 64); }
    template <class T> int upload(int id, const T* p, size_t n)
    {
        int rc = ensure(id, n * sizeof(T)); if (rc) return rc;
        NECAT_HIP(ctx, hipMemcpyAsync(ctx->nw_buf[id].p, p, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return NECAT_OK;
    }
    template <class T> int download(std::vector<T>* dst, int id, size_t n)
    {
        dst->resize(n);
        NECAT_HIP(ctx, hipMemcpyAsync(dst->data(), ctx->nw_buf[id].p, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return NECAT_OK;
    }
    int cols(const std::vector<nw::ColsTask>& ts, u64 col_ints, u64 bnd_ints, std::vector<int>* last)
    {
        const double w0 = wall_ms();
        int rc = upload(NWB_TASKS, ts.data(), ts.size()); if (rc) return rc;
        if ((rc = ensure(NWB_COLS, col_ints * 4)) || (rc = ensure(NWB_BND, bnd_ints * 4)) || (rc = ensure(NWB_OUT, ts.size() * 4))) return rc;
        hipLaunchKernelGGL(nw::k_nw_cols, dim3((unsigned)ts.size()), dim3(64), 0, ctx->stream, qbases, tbases, buf<nw::ColsTask>(NWB_TASKS), buf<int>(NWB_COLS),
                           buf<int>(NWB_BND), buf<int>(NWB_OUT));
        NECAT_CHECK_LAUNCH(ctx, "k_nw_cols");
        rc = download(last, NWB_OUT, ts.size());
        st->cols_ms += wall_ms() - w0;
        return rc;
    }
    int split(const std::vector<nw::SplitTask>& ts, std::vector<nw::SplitOut>* out)
    {
        const double w0 = wall_ms();
        int rc = upload(NWB_TASKS, ts.data(), ts.size()); if (rc) return rc;
        if ((rc = ensure(NWB_OUT, ts.size() * sizeof(nw::SplitOut)))) return rc;
        hipLaunchKernelGGL(nw::k_nw_split, dim3((unsigned)ts.size()), dim3(64), 0, ctx->stream, buf<nw::SplitTask>(NWB_TASKS), buf<int>(NWB_COLS), buf<nw::SplitOut>(NWB_OUT));
        NECAT_CHECK_LAUNCH(ctx, "k_nw_split");
        rc = download(out, NWB_OUT, ts.size());
        st->split_ms += wall_ms() - w0;
        return rc;
    }
    int begin_paths(u64 ops_bytes, size_t n)
    {
        n_leaves = n;
        int rc = ensure(NWB_OPS, ops_bytes); if (rc) return rc;
        return ensure(NWB_LEAF, n * (sizeof(nw::LeafOut) + 8));
    }
    int leaves(const nw::LeafTask* ts, size_t n, size_t first, u64 flag_recs, u64 bnd_ints)
    {
        const double w0 = wall_ms();
        int rc = upload(NWB_TASKS, ts, n); if (rc) return rc;
        if ((rc = ensure(NWB_FLAGS, flag_recs * 16)) || (rc = ensure(NWB_BND, bnd_ints * 4))) return rc;
        hipLaunchKernelGGL(nw::k_nw_leaf, dim3((unsigned)n), dim3(64), 0, ctx->stream, qbases, tbases, buf<nw::LeafTask>(NWB_TASKS), buf<ulonglong2>(NWB_FLAGS),
                           buf<int>(NWB_BND), buf<u8>(NWB_OPS), buf<nw::LeafOut>(NWB_LEAF) + first);
        NECAT_CHECK_LAUNCH(ctx, "k_nw_leaf");
        NECAT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        st->leaf_ms += wall_ms() - w0;
        return NECAT_OK;
    }
    int finish(const std::vector<nw::FinTask>& ts, const std::vector<u64>& leaf_end, u64 pack_bytes, std::vector<nw::FinOut>* out)
    {
        out->clear(); pack.clear();
        if (ts.empty()) return NECAT_OK;
        const double w0 = wall_ms();
        int rc = upload(NWB_TASKS, ts.data(), ts.size()); if (rc) return rc;
        u64* d_end = (u64*)(buf<nw::LeafOut>(NWB_LEAF) + n_leaves);       // (LeafOut is 8 bytes: the array behind it is 8-byte aligned)
        if (!leaf_end.empty()) NECAT_HIP(ctx, hipMemcpyAsync(d_end, leaf_end.data(), leaf_end.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = ensure(NWB_PACK, pack_bytes)) || (rc = ensure(NWB_OUT, ts.size() * sizeof(nw::FinOut)))) return rc;
        hipLaunchKernelGGL(nw::k_nw_finish, dim3((unsigned)ts.size()), dim3(64), 0, ctx->stream, buf<nw::FinTask>(NWB_TASKS), buf<nw::LeafOut>(NWB_LEAF), d_end,
                           buf<u8>(NWB_OPS), buf<u8>(NWB_PACK), buf<nw::FinOut>(NWB_OUT));
        NECAT_CHECK_LAUNCH(ctx, "k_nw_finish");
        if (keep_pack) pack.resize(pack_bytes);
        if (keep_pack && pack_bytes) NECAT_HIP(ctx, hipMemcpyAsync(pack.data(), ctx->nw_buf[NWB_PACK].p, pack_bytes, hipMemcpyDeviceToHost, ctx->stream));
        rc = download(out, NWB_OUT, ts.size());
        st->finish_ms += wall_ms() - w0;
        return rc;
    }
};
static_assert(sizeof(nw::LeafOut) == 8, "NwDevice::finish places the leaves' end offsets behind the LeafOut array");

// The jobs through nw::solve on the device; a job whose self-check failed is recomputed by rescue::EdlibGo.  res[i]: job i's result, (*packed)[i]: its
// columns, two bits each (empty unless ok); packed == nullptr: the caller wants no columns, none are copied from the device or kept.
int nw_run(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const necat_nw_job* jobs, uint64_t n, double error,
           int min_align_size, int match_size, necat_nw_result* res, std::vector<std::vector<u8>>* packed, necat_nw_stats* st)
{
    memset(st, 0, sizeof *st);
    const double w0 = wall_ms();
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<nw::Job> js(n);
    for (uint64_t i = 0; i < n; ++i) {
        const necat_nw_job& j = jobs[i];
        SeqAt q, s;
        if (!seq_at(reads, j.qid, read_start_id, &q) || !seq_at(ref, j.sid, ref_start_id, &s) || (j.qdir != 0 && j.qdir != 1))
            return set_err(ctx, NECAT_ERR_ARG, "job %lu names a sequence outside its volume (or a strand that is neither 0 nor 1)", (unsigned long)i);
        if (j.qfrom < 0 || j.qto < j.qfrom || (u64)j.qto > q.len || j.sfrom < 0 || j.sto < j.sfrom || (u64)j.sto > s.len)
            return set_err(ctx, NECAT_ERR_ARG, "job %lu: a range outside its sequence", (unsigned long)i);
        if (j.qto - j.qfrom >= nw::kMaxLen || j.sto - j.sfrom >= nw::kMaxLen) return set_err(ctx, NECAT_ERR_ARG, "job %lu: a range of 2^26 bases or more", (unsigned long)i);
        nw::Job& J = js[i];
        J.m = j.qto - j.qfrom; J.n = j.sto - j.sfrom; J.tolerance = j.tolerance;
        J.q = pair::strand_seq((i64)q.begin, (i64)q.len, j.qdir, j.qfrom);
        J.t = pair::strand_seq((i64)s.begin, (i64)s.len, 0, j.sfrom);
    }
    NwDevice dev{ctx, reads->bases, ref->bases, st};
    dev.keep_pack = packed != nullptr;
    if (packed) packed->assign(n, std::vector<u8>());
    std::vector<u8> unused_cols;
    std::vector<u64> wq, wt;          // the volumes' words on the host: fetched when the first job fails its self-check
    std::vector<u8> qseq, tseq;
    // chunks of jobs whose ops (one byte per row and column) stay under 1 GB
    for (uint64_t a = 0; a < n;) {
        uint64_t e = a; u64 bytes = 0;
        while (e < n && (e == a || bytes + (u64)js[e].m + js[e].n <= (1ULL << 30))) { bytes += (u64)js[e].m + js[e].n; ++e; }
        std::vector<nw::Job> part(js.begin() + (ptrdiff_t)a, js.begin() + (ptrdiff_t)e);
        std::vector<nw::JobOut> out;
        nw::Stats ns;
        const int rc = nw::solve(dev, part, error, min_align_size, match_size, (u64)knob().nw_pool, &out, &ns);
        if (rc) return rc;
        st->n_levels += (uint32_t)ns.levels; st->n_leaf_chunks += (uint32_t)ns.leaf_chunks; st->n_passes += ns.cols_tasks; st->n_splits += ns.splits; st->n_leaves += ns.leaves;
        for (uint64_t i = a; i < e; ++i) {
            const nw::JobOut& o = out[i - a];
            const necat_nw_job& j = jobs[i];
            necat_nw_result& r = res[i];
            if (o.fail) {          // certified fallback: the host code decides this job
                ++st->n_host; ++st->n_selfcheck;
                int rc2 = NECAT_OK;
                if (wq.empty() && ((rc2 = fetch_words(ctx, reads, &wq)) || (rc2 = fetch_words(ctx, ref, &wt)))) return rc2;
                host_view(reads, wq).strand((int64_t)j.qid - read_start_id, j.qdir, qseq);
                host_view(ref, wt).strand((int64_t)j.sid - ref_start_id, 0, tseq);
                rescue::EdlibGo edl(error);
                cns::edlib_job(edl, qseq.data(), tseq.data(), j, min_align_size, match_size, &r, packed ? &(*packed)[i] : &unused_cols);
                continue;
            }
            memset(&r, 0, sizeof r);
            ++st->n_device;
            if (!o.ok) continue;
            r.ok = 1; r.qoff = j.qfrom + o.qoff; r.qend = j.qfrom + o.qend; r.toff = j.sfrom + o.toff; r.tend = j.sfrom + o.tend;
            r.align_size = o.asz; r.dist = o.dist;
            r.ident_perc = 100.0 * (o.asz - o.dist) / o.asz;
            if (packed) (*packed)[i].assign(dev.pack.begin() + (ptrdiff_t)o.pack_off, dev.pack.begin() + (ptrdiff_t)(o.pack_off + ((u64)o.asz + 3) / 4));
        }
        a = e;
    }
    st->device_ms = st->cols_ms + st->split_ms + st->leaf_ms + st->finish_ms;
    st->host_ms = wall_ms() - w0 - st->device_ms;
    if (knob().trace & 2)
        fprintf(stderr, "[necat] nw path: %lu jobs (%lu on the host), %u levels, %lu passes, %lu splits, %lu leaves in %u chunks; device %.2f ms (cols %.2f, split %.2f, leaf %.2f, finish %.2f), host %.2f ms\n",
                (unsigned long)n, (unsigned long)st->n_host, st->n_levels, (unsigned long)st->n_passes, (unsigned long)st->n_splits, (unsigned long)st->n_leaves, st->n_leaf_chunks,
                st->device_ms, st->cols_ms, st->split_ms, st->leaf_ms, st->finish_ms, st->host_ms);
    return NECAT_OK;
}

// The pair's global half on the device: edlib's path over the ranges the local half accepted, as jobs on the sequences (a range on a slice lies `from` further on its
// sequence) through nw_run; the accepted results come back on the slices.  job_of[x]: the entry of `jobs` result x belongs to; cols[x]: its columns, if asked for.
struct PairGlobal { std::vector<uint64_t> job_of; std::vector<necat_nw_result> res; std::vector<std::vector<u8>> cols; necat_nw_stats ns; };
int pair_global(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const std::vector<pair::Job>& jobs,
                const necat_dalign_result* ranges, double error, int min_align_size, bool want_cols, PairGlobal* G)
{
    memset(&G->ns, 0, sizeof G->ns);
    std::vector<necat_nw_job> nj;
    for (uint64_t k = 0; k < jobs.size(); ++k)
        if (ranges[k].ok) { nj.push_back(pair::nw_job(jobs[k].qid, jobs[k].qdir, jobs[k].sid, jobs[k].from, ranges[k])); G->job_of.push_back(k); }
    G->res.resize(nj.size());
    if (nj.empty()) return NECAT_OK;
    if (int rc = nw_run(ctx, ref, reads, read_start_id, ref_start_id, nj.data(), nj.size(), error, min_align_size, 4 /* EdlibGo::go's default, as rm_host.h and cns_ctg_subseq.c:83 call it */,
                        G->res.data(), want_cols ? &G->cols : nullptr, &G->ns)) return rc;
    for (size_t x = 0; x < nj.size(); ++x) if (G->res[x].ok) pair::to_slice(jobs[G->job_of[x]].from, &G->res[x]);
    return NECAT_OK;
}

}  // namespace
}  // extern "C++"

int necat_nw_path_batch(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const necat_nw_job* jobs, uint64_t n,
                        double error, int min_align_size, int match_size, necat_nw_result** res, uint8_t** ops, uint64_t** ops_off, necat_nw_stats* stats)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ref || !reads || !res || !ops || !ops_off || (n && !jobs)) return NECAT_ERR_ARG;
    *res = nullptr; *ops = nullptr; *ops_off = nullptr;
    if (match_size < 1 || match_size > 64 || !(error >= 0.0)) return set_err(ctx, NECAT_ERR_ARG, "match_size outside 1 .. 64, or a negative error");
    necat_nw_stats st;
    std::vector<std::vector<u8>> packed;
    ResultOwner own;
    necat_nw_result* r = own.own<necat_nw_result>(result_alloc(std::max<uint64_t>(1, n) * sizeof(necat_nw_result)));
    uint64_t* off = own.own<uint64_t>(result_alloc((n + 1) * 8));
    if (!r || !off) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    const int rc = nw_run(ctx, ref, reads, read_start_id, ref_start_id, jobs, n, error, min_align_size, match_size, r, &packed, &st);
    if (rc) return rc;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) { off[i] = total; total += (packed[i].size() + 7) & ~(uint64_t)7; }
    off[n] = total;
    uint8_t* o = (uint8_t*)result_alloc(std::max<uint64_t>(1, total));
    if (!o) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    memset(o, 0, std::max<uint64_t>(1, total));
    for (uint64_t i = 0; i < n; ++i) if (!packed[i].empty()) memcpy(o + off[i], packed[i].data(), packed[i].size());
    if (stats) *stats = st;
    own.release();
    *res = r; *ops = o; *ops_off = off;
    return NECAT_OK;
}
