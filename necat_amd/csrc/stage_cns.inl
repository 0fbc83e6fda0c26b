// stage_cns.inl - the consensus stage's extension loop (cns_loop.h).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ consensus stage: the extension loop

void necat_cns_default_options(necat_cns_options* o)
{   // consensus/cns_options.c:10-22
    o->min_align_size = 400; o->min_cov = 4; o->max_cov = 12; o->error = 0.5; o->mapping_ratio = 0.8; o->use_fixed_ident_cutoff = 0;
    o->rescue_long_indels = 0;
}

int necat_cns_load_partition(necat_ctx* ctx, const necat_volume* reads, const void* packed, uint64_t n,
                             necat_candidate** cands, uint64_t** tmpl_off, uint64_t** n_all, uint64_t* n_templates)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || (n && !packed) || !cands || !tmpl_off || !n_all || !n_templates) return NECAT_ERR_ARG;
    *cands = nullptr; *tmpl_off = nullptr; *n_all = nullptr; *n_templates = 0;
    std::vector<cns::Packed> recs(n);
    if (n) memcpy(recs.data(), packed, n * sizeof(cns::Packed));
    std::vector<necat_candidate> c; std::vector<uint64_t> off, na;
    const uint64_t bad = cns::load_partition(recs, reads->h_seq_off.data(), reads->nseq, c, off, na, (unsigned)ctx->knobs.cns_threads);
    if (bad) return set_err(ctx, NECAT_ERR_ARG, "candidate record %lu refers to a read outside the read set or has a range outside its reads", (unsigned long)(bad - 1));
    necat_candidate* oc = (necat_candidate*)malloc(std::max<size_t>(1, c.size()) * sizeof(necat_candidate));
    uint64_t* oo = (uint64_t*)malloc(off.size() * 8);
    uint64_t* on = (uint64_t*)malloc(std::max<size_t>(1, na.size()) * 8);
    if (!oc || !oo || !on) { free(oc); free(oo); free(on); return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed"); }
    if (!c.empty()) memcpy(oc, c.data(), c.size() * sizeof(necat_candidate));
    memcpy(oo, off.data(), off.size() * 8);
    if (!na.empty()) memcpy(on, na.data(), na.size() * 8);
    *cands = oc; *tmpl_off = oo; *n_all = on; *n_templates = na.size();
    return NECAT_OK;
}

void necat_cns_result_free(necat_cns_result* r)
{
    if (!r) return;
    for (uint32_t b = 0; b < r->n_ops_blocks; ++b) necat_free(r->ops[b]);
    free(r->ops); free(r->templates); free(r->overlaps); free(r->ranges);
    free(r);
}

namespace {

// the call's templates from its arrays; every candidate checked against the read set (nothing below checks again)
int cns_templates(necat_ctx* ctx, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off, const uint64_t* n_all, uint64_t n_templates,
                  std::vector<cns::Template>* ts)
{
    ts->assign(n_templates, cns::Template());
    for (uint64_t t = 0; t < n_templates; ++t) {
        const uint64_t lo = tmpl_off[t], hi = tmpl_off[t + 1];
        if (hi < lo || hi - lo >= (1ULL << 31)) return set_err(ctx, NECAT_ERR_ARG, "template %lu: bad candidate range", (unsigned long)t);
        cns::Template& T = (*ts)[t];
        T.c = cands + lo; T.c_base = lo; T.n = (uint32_t)(hi - lo); T.n_all = n_all ? (uint32_t)std::min<uint64_t>(n_all[t], 0xffffffffu) : T.n;
        for (uint64_t i = lo; i < hi; ++i) {
            const necat_candidate& c = cands[i];
            if (c.sid != cands[lo].sid || c.sdir != 0 || c.sid < 0 || (uint64_t)c.sid >= reads->nseq || c.qid < 0 || (uint64_t)c.qid >= reads->nseq ||
                c.ssize != reads->h_seq_off[c.sid + 1] - reads->h_seq_off[c.sid] || c.qsize != reads->h_seq_off[c.qid + 1] - reads->h_seq_off[c.qid] ||
                c.sbeg > c.send || c.send > c.ssize || c.qoff > c.qsize || c.soff > c.ssize || c.ssize >= (1ULL << 31) || c.qsize >= (1ULL << 31))
                return set_err(ctx, NECAT_ERR_ARG, "candidate %lu of template %lu is inconsistent (one forward subject per template, ranges inside the reads)",
                               (unsigned long)(i - lo), (unsigned long)t);
        }
        T.tsize = T.n ? (int)cands[lo].ssize : 0;
    }
    return NECAT_OK;
}

// One pass of the loop on the device: the block-wise extension of the candidates cns::run selected.  The columns stay where the device copied them,
// one block per batch of the pass (`blocks`: the call's column blocks, also the rescue's).
struct CnsDevicePass {
    necat_ctx* ctx; const necat_volume* reads; necat_map_options mo;
    std::vector<u8*>* blocks;
    double device_ms = 0, wall = 0;

    int run(const necat_candidate* c, uint64_t m, cns::Aligned* res)
    {
        const double a0 = wall_ms();
        AlignOut ao;
        ao.defer_copy = true;       // the loop only needs the coordinates to go on; the columns arrive while it does
        ao.aln = (necat_alignment*)result_alloc(std::max<uint64_t>(1, m) * sizeof(necat_alignment));
        if (!ao.aln) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        ao.off.assign(m + 1, 0);
        const int rc = extend_impl(ctx, reads, reads, 0, 0, c, m, &mo, 4 /* ONC_TAIL_MATCH_LEN_LONG, oc_aligner.h:42 */, nullptr, nullptr, &ao);
        if (rc) {
            if (ctx->stream_copy) (void)hipStreamSynchronize(ctx->stream_copy);
            ctx->copy_pending = false;
            necat_free(ao.aln); for (auto& pr : ao.parts) necat_free(pr.first); return rc;
        }
        device_ms += ctx->tm.extend_ms;
        size_t p = 0; u64 p_start = 0;
        const u32 b0 = (u32)blocks->size();
        for (auto& pr : ao.parts) blocks->push_back(pr.first);
        for (uint64_t i = 0; i < m; ++i) {
            res[i].a = ao.aln[i];
            const u64 at = ao.off[i];
            while (p < ao.parts.size() && at >= p_start + ao.parts[p].second && ao.off[i + 1] > at) { p_start += ao.parts[p].second; ++p; }
            res[i].block = b0 + (u32)std::min(p, ao.parts.empty() ? 0 : ao.parts.size() - 1);
            res[i].off = at - p_start;
        }
        necat_free(ao.aln);
        wall += wall_ms() - a0;
        if (knob().trace & 2) fprintf(stderr, "[necat] cns pass: %lu alignments, %.2f ms\n", (unsigned long)m, wall_ms() - a0);
        return NECAT_OK;
    }
};

// -r 1: the rescue pair (cns_rescue.h) on the candidates of a pass whose block-wise extension failed or fell short.  DALIGNER's local alignment on
// the host threads - or, with NECAT_DALIGN_DEVICE=1, through necat_local_align_batch's kernel on the resident reads - then the global path over the ranges it found as one list of necat_nw_path_batch jobs - through its kernels on the resident
// reads (NECAT_NW_DEVICE=1: no sequence goes up) or through rescue::EdlibGo on the host threads - and the results into a block of columns.
struct CnsRescue {
    necat_ctx* ctx; const necat_volume* reads; const necat_cns_options* opt;
    std::vector<u8*>* blocks;
    rescue::DalignSpec dspec;
    bool nw_on_device, dalign_on_device;      // knob().nw_device / dalign_device, read on the calling thread
    std::vector<u64> words;             // the reads' 2-bit words: they come back from the device once per call, on the first pass whose rescue has a half on the host
    struct Counters {                   // the necat_cns_result fields of these names
        uint64_t n_rescue_tried = 0, n_rescued = 0, n_rescue_nw = 0, n_rescue_nw_device = 0, n_rescue_nw_host = 0, n_rescue_dalign_device = 0, n_rescue_dalign_host = 0;
        double rescue_ms = 0, rescue_dalign_ms = 0, rescue_nw_ms = 0;
    } n;

    CnsRescue(necat_ctx* ctx_, const necat_volume* reads_, const necat_cns_options* opt_, std::vector<u8*>* blocks_)
        : ctx(ctx_), reads(reads_), opt(opt_), blocks(blocks_), dspec(opt_->rescue_long_indels ? rescue::spec_for_error(opt_->error) : rescue::DalignSpec()),
          nw_on_device(knob().nw_device != 0), dalign_on_device(knob().dalign_device != 0) {}

    static unsigned threads_for(size_t items) { return (unsigned)std::min<size_t>(std::min(necat_host::hardware_threads(), 32u), items); }

    // the local half of every candidate in `need`; the survivors' ranges as jobs, in candidate order (cand_of[x]: job x's candidate)
    void local_half(const necat_candidate* c, const std::vector<uint64_t>& need, std::vector<necat_nw_job>* jobs, std::vector<uint64_t>* cand_of) const
    {
        const necat_host::BaseWords hb = host_view(reads, words);
        std::vector<necat_nw_job> job(need.size());
        std::vector<u8> found(need.size(), 0);
        necat_host::Deal deal(need.size());
        necat_host::on_threads(threads_for(need.size()), [&](unsigned) {
            rescue::Dalign dal(dspec);
            std::vector<u8> q, t;
            deal.run([&](uint64_t k) {
                const necat_candidate& cc = c[need[k]];
                hb.strand(cc.qid, cc.qdir, q); hb.strand(cc.sid, 0, t);
                found[k] = cns::rescue_local(dal, cc, q.data(), t.data(), opt->min_align_size);
                if (found[k]) job[k] = cns::rescue_job(cc, dal.r);
            });
        });
        for (size_t k = 0; k < need.size(); ++k) if (found[k]) { jobs->push_back(job[k]); cand_of->push_back(need[k]); }
    }

    // the same through the kernel of necat_local_align_batch: one call for the pass (a job it hands back is recomputed by rescue::Dalign in there)
    int local_half_on_device(const necat_candidate* c, const std::vector<uint64_t>& need, std::vector<necat_nw_job>* jobs, std::vector<uint64_t>* cand_of)
    {
        std::vector<necat_dalign_job> dj(need.size());
        for (size_t k = 0; k < need.size(); ++k) { const necat_candidate& cc = c[need[k]]; dj[k] = necat_dalign_job{cc.qid, cc.qdir, (int32_t)cc.qoff, cc.sid, (int32_t)cc.soff}; }
        std::vector<necat_dalign_result> dr(need.size());
        necat_dalign_stats ds;
        if (int rc = dal_run(ctx, reads, reads, 0, 0, dj.data(), dj.size(), opt->error, opt->min_align_size, dr.data(), &ds)) return rc;
        n.n_rescue_dalign_device += ds.n_device; n.n_rescue_dalign_host += ds.n_host;
        for (size_t k = 0; k < need.size(); ++k) {
            const necat_candidate& cc = c[need[k]];
            if (dr[k].ok) { jobs->push_back(pair::nw_job(cc.qid, cc.qdir, cc.sid, 0, dr[k])); cand_of->push_back(need[k]); }          // (from 0: the subject is the whole template)
        }
        return NECAT_OK;
    }

    // the global half on the host threads: what nw_run gives for the same jobs
    void global_on_host(const std::vector<necat_nw_job>& jobs, necat_nw_result* nr, std::vector<std::vector<u8>>* packed) const
    {
        const necat_host::BaseWords hb = host_view(reads, words);
        packed->assign(jobs.size(), std::vector<u8>());
        necat_host::Deal deal(jobs.size());
        necat_host::on_threads(threads_for(jobs.size()), [&](unsigned) {
            rescue::EdlibGo edl(opt->error);
            std::vector<u8> q, t;
            deal.run([&](uint64_t x) {
                hb.strand(jobs[x].qid, jobs[x].qdir, q); hb.strand(jobs[x].sid, 0, t);
                cns::edlib_job(edl, q.data(), t.data(), jobs[x], opt->min_align_size, 4, &nr[x], &(*packed)[x]);
            });
        });
    }

    // the accepted jobs' columns into one block of the call, their coordinates over the block-wise ones
    int store(const std::vector<uint64_t>& cand_of, const necat_nw_result* nr, const std::vector<std::vector<u8>>& packed, cns::Aligned* res)
    {
        u64 bytes = 0;
        for (size_t x = 0; x < cand_of.size(); ++x) if (nr[x].ok) bytes += (packed[x].size() + 7) & ~(u64)7;
        if (!bytes) return NECAT_OK;
        u8* blk = (u8*)result_alloc(bytes);
        if (!blk) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        const u32 bi = (u32)blocks->size();
        blocks->push_back(blk);
        u64 at = 0;
        for (size_t x = 0; x < cand_of.size(); ++x) {
            if (!nr[x].ok) continue;
            memcpy(blk + at, packed[x].data(), packed[x].size());
            cns::Aligned& o = res[cand_of[x]];
            cns::take_rescued(nr[x], &o.a); o.block = bi; o.off = at;
            at += (packed[x].size() + 7) & ~(u64)7;
            ++n.n_rescued;
        }
        return NECAT_OK;
    }

    int run(const necat_candidate* c, uint64_t m, cns::Aligned* res)
    {
        const double r0 = wall_ms();
        std::vector<uint64_t> need;
        for (uint64_t i = 0; i < m; ++i) if (cns::extension_short(c[i], res[i].a)) need.push_back(i);
        if (need.empty()) return NECAT_OK;
        int rc = words.empty() && !(dalign_on_device && nw_on_device) ? fetch_words(ctx, reads, &words) : NECAT_OK;
        if (rc) return rc;
        std::vector<necat_nw_job> jobs;
        std::vector<uint64_t> cand_of;
        if (!dalign_on_device) local_half(c, need, &jobs, &cand_of);
        else if ((rc = local_half_on_device(c, need, &jobs, &cand_of))) return rc;
        const double r1 = wall_ms();
        n.rescue_dalign_ms += r1 - r0;
        n.n_rescue_nw += jobs.size();
        std::vector<necat_nw_result> nr(jobs.size());
        std::vector<std::vector<u8>> packed;
        if (nw_on_device && !jobs.empty()) {
            necat_nw_stats ns;
            if ((rc = nw_run(ctx, reads, reads, 0, 0, jobs.data(), jobs.size(), opt->error, opt->min_align_size, 4, nr.data(), &packed, &ns))) return rc;
            n.n_rescue_nw_device += ns.n_device; n.n_rescue_nw_host += ns.n_host;
        } else if (!jobs.empty()) global_on_host(jobs, nr.data(), &packed);
        const double r2 = wall_ms();
        n.rescue_nw_ms += r2 - r1;
        n.n_rescue_tried += need.size();
        if ((rc = store(cand_of, nr.data(), packed, res))) return rc;
        n.rescue_ms += wall_ms() - r0;
        if (knob().trace & 2) fprintf(stderr, "[necat] cns rescue: %zu of %lu candidates tried, %zu with a range, %.2f ms (local %.2f on the %s, global %.2f on the %s)\n", need.size(),
                                 (unsigned long)m, jobs.size(), wall_ms() - r0, r1 - r0, dalign_on_device ? "device" : "host", r2 - r1, nw_on_device ? "device" : "host");
        return NECAT_OK;
    }
};

// the finished templates as a result the caller owns (counters and times are the caller's to fill); nullptr: out of memory
necat_cns_result* cns_result_of(const std::vector<cns::Template>& ts, const std::vector<u8*>& blocks, unsigned threads)
{
    const uint64_t n_templates = ts.size();
    necat_cns_result* r = (necat_cns_result*)calloc(1, sizeof(necat_cns_result));
    uint64_t n_ov = 0, n_rg = 0;
    for (auto& T : ts) { n_ov += T.overlaps.size(); n_rg += T.ranges.size() / 2; }
    if (r) {
        r->templates = (necat_cns_template*)calloc(std::max<uint64_t>(1, n_templates), sizeof(necat_cns_template));
        r->overlaps = (necat_cns_overlap*)malloc(std::max<uint64_t>(1, n_ov) * sizeof(necat_cns_overlap));
        r->ranges = (int32_t*)malloc(std::max<uint64_t>(1, n_rg) * 8);
        r->ops = (uint8_t**)malloc(std::max<size_t>(1, blocks.size()) * sizeof(uint8_t*));
    }
    if (!r || !r->templates || !r->overlaps || !r->ranges || !r->ops) {
        if (r) { free(r->templates); free(r->overlaps); free(r->ranges); free(r->ops); free(r); }
        return nullptr;
    }
    uint64_t ov = 0, rg = 0;
    for (uint64_t t = 0; t < n_templates; ++t) {
        necat_cns_template& o = r->templates[t];
        o.ovlp_begin = ov; o.range_begin = rg;
        ov += ts[t].overlaps.size(); rg += ts[t].ranges.size() / 2;
        o.ovlp_end = ov; o.range_end = rg;
    }
    cns::parallel_for(n_templates, [&](size_t t) {
        const cns::Template& T = ts[t];
        necat_cns_template& o = r->templates[t];
        o.examined = T.examined ? 1 : 0; o.num_can = T.num_can; o.num_ovlps = T.num_ovlps; o.ident_cutoff = T.ident_cutoff;
        if (!T.overlaps.empty()) memcpy(r->overlaps + o.ovlp_begin, T.overlaps.data(), T.overlaps.size() * sizeof(necat_cns_overlap));
        if (!T.ranges.empty()) memcpy(r->ranges + 2 * o.range_begin, T.ranges.data(), T.ranges.size() * 4);
    }, threads);
    r->n_templates = n_templates; r->n_overlaps = n_ov; r->n_ranges = n_rg;
    r->n_ops_blocks = (uint32_t)blocks.size();
    for (size_t b = 0; b < blocks.size(); ++b) r->ops[b] = blocks[b];
    return r;
}

}  // namespace

int necat_cns_extension_batch(necat_ctx* ctx, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off,
                              const uint64_t* n_all, uint64_t n_templates, const necat_cns_options* opt, necat_cns_result** out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || !opt || !out || (n_templates && (!tmpl_off || !cands))) return NECAT_ERR_ARG;
    *out = nullptr;
    if (opt->max_cov < 1 || opt->max_cov > 60000 || opt->min_align_size < 0 || !(opt->error > 0.0 && opt->error <= 1.0))
        return set_err(ctx, NECAT_ERR_ARG, "consensus options out of range");
    const double w0 = wall_ms();
    std::vector<cns::Template> ts;
    int rc = cns_templates(ctx, reads, cands, tmpl_off, n_all, n_templates, &ts);
    if (rc) return rc;
    std::vector<u8*> blocks;
    CnsDevicePass pass{ctx, reads, necat_map_options(), &blocks};
    necat_default_options(&pass.mo);
    pass.mo.error = opt->error; pass.mo.align_size_cutoff = opt->min_align_size;
    CnsRescue rescue_pass(ctx, reads, opt, &blocks);
    cns::AlignFn fn = [&](const necat_candidate* c, uint64_t m, cns::Aligned* res) -> int {
        const int e = pass.run(c, m, res);
        return e || !opt->rescue_long_indels ? e : rescue_pass.run(c, m, res);
    };
    cns::Knobs kn; kn.threads = (unsigned)ctx->knobs.cns_threads; kn.spec_estimate_extra = knob().cns_spec_extra; kn.spec_cover = knob().cns_spec_cover;
    cns::Stats st;
    const double w_run = wall_ms();
    if (!ctx->cns_scratch) ctx->cns_scratch = new cns::Scratch();
    rc = cns::run(ts, *opt, kn, fn, &st, (cns::Scratch*)ctx->cns_scratch);
    if (knob().trace & 2) fprintf(stderr, "[necat] cns host: setup %.2f ms, init %.2f, select %.2f, gather %.2f, replay %.2f ms\n", w_run - w0, st.init_ms, st.select_ms,
                             st.gather_ms, st.replay_ms);
    auto drop = [&]() { for (u8* b : blocks) necat_free(b); };
    {   // the last columns may still be on their way
        const hipError_t e = ctx->stream_copy ? hipStreamSynchronize(ctx->stream_copy) : hipSuccess;
        ctx->copy_pending = false;
        if (e != hipSuccess && !rc) { drop(); return set_err(ctx, NECAT_ERR_DEVICE, "column copy failed: %s", hipGetErrorString(e)); }
    }
    if (rc) { drop(); return rc; }
    necat_cns_result* r = cns_result_of(ts, blocks, kn.threads);
    if (!r) { drop(); return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed"); }
    const CnsRescue::Counters& n = rescue_pass.n;
    r->n_aligned = st.n_aligned; r->n_used = st.n_used; r->n_rounds = st.n_rounds;
    r->device_ms = pass.device_ms; r->host_ms = wall_ms() - w0 - pass.wall - n.rescue_ms;
    r->n_rescue_tried = n.n_rescue_tried; r->n_rescued = n.n_rescued; r->rescue_ms = n.rescue_ms;
    r->rescue_dalign_ms = n.rescue_dalign_ms; r->rescue_nw_ms = n.rescue_nw_ms;
    r->n_rescue_nw = n.n_rescue_nw; r->n_rescue_nw_device = n.n_rescue_nw_device; r->n_rescue_nw_host = n.n_rescue_nw_host;
    r->n_rescue_dalign_device = n.n_rescue_dalign_device; r->n_rescue_dalign_host = n.n_rescue_dalign_host;
    if (knob().trace & 2) fprintf(stderr, "[necat] cns total %.2f ms: passes %.2f (device events %.2f), host %.2f\n", wall_ms() - w0, pass.wall, pass.device_ms, r->host_ms);
    ctx->tm.extend_ms = pass.device_ms;
    *out = r;
    return NECAT_OK;
}
