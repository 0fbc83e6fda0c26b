// stage_cns_consensus.inl - the consensus proper of oc2cns (tasc/: tags -> backbone -> best path) behind the C ABI: on the device with a certified fallback
// (cns_dev_core.h, cns_dev_kernels.h), or on the library's host threads (cns_consensus.h).  One of the stage files of libnecat_hip.so's single translation unit.

// ------------------------------------------------------------------------------------------ consensus stage: the consensus proper

void necat_cns_consensus_default_options(necat_cns_consensus_options* o)
{   // consensus/cns_options.c:10-22
    o->min_cov = 4; o->min_size = 500; o->full_consensus = 0; o->path = 0; o->host_threads = 0;
}

void necat_cns_consensus_free(necat_cns_consensus* r)
{
    if (!r) return;
    free(r->templates); free(r->segments); free(r->bases);
    free(r);
}

namespace {

namespace hc = necat_host::cns;
namespace cd = necat::cns_dev;

struct CnsDevChunk { std::vector<uint64_t> tmpl; uint64_t tags = 0, pos = 0, ovs = 0, segs = 0; };

// what a device chunk holds besides the context's arena: released on every way out of the call
struct CnsDevScratch {
    CallEvents<5> ev;
    uint8_t* h_ops = nullptr; uint8_t* h_out = nullptr;
    void drop_host() { necat_free(h_ops); necat_free(h_out); h_ops = h_out = nullptr; }
    ~CnsDevScratch() { drop_host(); }
};

// One call of necat_cns_consensus_batch: its arguments, what the steps hand on to each other, and the steps in the order the entry point takes them.
struct CnsConsensusCall {
    necat_ctx* ctx; const necat_volume* reads; const necat_candidate* cands; const uint64_t* tmpl_off; uint64_t n_templates;
    const necat_cns_result* ext; const necat_cns_consensus_options* opt;
    unsigned threads = 1;
    std::vector<std::vector<hc::SegCodes>> kept;      // per template: its segments, from the device or from the host form
    std::vector<uint8_t> on_host;
    std::vector<uint64_t> host_list;                  // the templates of the host form: all examined ones (path 1), or what the device handed back
    uint64_t n_device = 0, n_fallback = 0, n_uncertain = 0;
    double device_ms = 0, host_ms = 0, k_ms[4] = {0, 0, 0, 0};
    uint32_t n_chunks = 0;

    uint64_t n_ov_of(uint64_t t) const { return ext->templates[t].ovlp_end - ext->templates[t].ovlp_begin; }
    void hand_back(uint64_t t) { host_list.push_back(t); on_host[t] = 1; ++n_fallback; }

    // the options, and the overlaps inside their reads: nothing below checks again
    int validate()
    {
        if (ext->n_templates != n_templates) return set_err(ctx, NECAT_ERR_ARG, "the extension result has %lu templates, the call %lu", (unsigned long)ext->n_templates, (unsigned long)n_templates);
        if (opt->min_cov < 0 || opt->min_size < 2 || (opt->path != 0 && opt->path != 1)) return set_err(ctx, NECAT_ERR_ARG, "consensus options out of range (min_cov >= 0, min_size >= 2, path 0 or 1)");
        const uint64_t n_cands = n_templates ? tmpl_off[n_templates] : 0;
        if (opt->host_threads < 0) return set_err(ctx, NECAT_ERR_ARG, "consensus options out of range (host_threads >= 0)");
        threads = call_threads(ctx, opt->host_threads);
        for (uint64_t t = 0; t < n_templates; ++t) {
            const necat_cns_template& T = ext->templates[t];
            if (!T.examined) continue;
            if (T.ovlp_begin > T.ovlp_end || T.ovlp_end > ext->n_overlaps || tmpl_off[t] >= tmpl_off[t + 1] || tmpl_off[t + 1] > n_cands)
                return set_err(ctx, NECAT_ERR_ARG, "template %lu: bad overlap or candidate range", (unsigned long)t);
            const necat_candidate& c0 = cands[tmpl_off[t]];
            if (c0.sid < 0 || (uint64_t)c0.sid >= reads->nseq || c0.ssize != reads->h_seq_off[c0.sid + 1] - reads->h_seq_off[c0.sid] || c0.ssize >= (1ULL << 31))
                return set_err(ctx, NECAT_ERR_ARG, "template %lu: its read is not a read of the volume", (unsigned long)t);
            for (uint64_t k = T.ovlp_begin; k < T.ovlp_end; ++k) {
                const necat_cns_overlap& ov = ext->overlaps[k];
                if (ov.cand >= n_cands || ov.ops_block >= ext->n_ops_blocks || ov.align_size < 0) return set_err(ctx, NECAT_ERR_ARG, "overlap %lu: bad candidate, column block or size", (unsigned long)k);
                const necat_candidate& c = cands[ov.cand];
                if (c.qid < 0 || (uint64_t)c.qid >= reads->nseq || c.qsize != reads->h_seq_off[c.qid + 1] - reads->h_seq_off[c.qid] || c.qsize >= (1ULL << 31) || c.sid != c0.sid ||
                    ov.qoff < 0 || ov.qend < ov.qoff || (uint64_t)ov.qend > c.qsize || ov.toff < 0 || ov.tend < ov.toff || (uint64_t)ov.tend > c0.ssize ||
                    ov.align_size < ov.qend - ov.qoff || ov.align_size < ov.tend - ov.toff)
                    return set_err(ctx, NECAT_ERR_ARG, "overlap %lu lies outside its reads", (unsigned long)k);
            }
        }
        kept.assign(n_templates, std::vector<hc::SegCodes>());
        on_host.assign(n_templates, 0);
        return NECAT_OK;
    }

    // chunks of templates under the tag budget (a template that exceeds it goes alone; one the key format cannot hold goes to the host)
    std::vector<CnsDevChunk> plan_chunks()
    {
        const uint64_t budget = knob().cns_tag_budget;
        std::vector<CnsDevChunk> chunks;
        for (uint64_t t = 0; t < n_templates; ++t) {
            const necat_cns_template& T = ext->templates[t];
            if (!T.examined) continue;
            const uint64_t tsize = cands[tmpl_off[t]].ssize;
            uint64_t tags = 0;
            bool wide = false;
            for (uint64_t k = T.ovlp_begin; k < T.ovlp_end; ++k) { tags += (uint64_t)ext->overlaps[k].align_size; wide = wide || ext->overlaps[k].align_size >= (1 << 24); }
            if (!tags) { ++n_device; continue; }              // nothing to sort: no stretch, no segment
            if (wide || tsize > cd::kMaxTsize || n_ov_of(t) > cd::kMaxOverlaps || tags + tsize >= (1ULL << 30)) { hand_back(t); continue; }
            if (chunks.empty() || (chunks.back().tags && chunks.back().tags + tags > budget) || chunks.back().tags + tags >= (1ULL << 31) || chunks.back().pos + tsize + 2 >= (1ULL << 31))
                chunks.emplace_back();
            CnsDevChunk& C = chunks.back();
            C.tmpl.push_back(t); C.tags += tags; C.pos += tsize + 1; C.ovs += n_ov_of(t);
            C.segs += tsize / (uint64_t)std::max(1, (int)ceil(opt->min_size * 0.85)) + 1;
        }
        return chunks;
    }

    // one chunk on the device: its templates and overlaps packed, the context's arena carved up, upload, the six kernels, download; the segments of
    // the templates the device certified into `kept`, the others handed back
    int run_chunk(const CnsDevChunk& C, CnsDevScratch& sc, double tol)
    {
        hipStream_t s = ctx->stream;
        const CallEvents<5>& ev = sc.ev;
        const double c0 = wall_ms();
        const size_t nt = C.tmpl.size(), T_ = C.tags, P = C.pos, NO = C.ovs, S = C.segs;
        std::vector<cd::DevTmpl> h_tm(nt);
        std::vector<cd::DevOvl> h_ov(NO);
        std::vector<double> h_w(NO);
        std::vector<const uint8_t*> src(NO);
        uint64_t ops_bytes = 0;
        {
            uint64_t tag = 0, pos = 0, ovi = 0, seg = 0;
            for (size_t x = 0; x < nt; ++x) {
                const uint64_t t = C.tmpl[x];
                const necat_cns_template& T = ext->templates[t];
                const uint64_t tsize = cands[tmpl_off[t]].ssize;
                cd::DevTmpl& D = h_tm[x];
                D.tag_base = (u32)tag; D.pos_base = (u32)pos; D.tsize = (i32)tsize; D.ov_base = (u32)ovi; D.n_ov = (u32)n_ov_of(t); D.seg_base = (u32)seg;
                D.seg_cap = (u32)(tsize / (uint64_t)std::max(1, (int)ceil(opt->min_size * 0.85)) + 1);
                for (uint64_t k = T.ovlp_begin; k < T.ovlp_end; ++k, ++ovi) {
                    const necat_cns_overlap& ov = ext->overlaps[k];
                    const necat_candidate& c = cands[ov.cand];
                    cd::DevOvl& o = h_ov[ovi];
                    o.ops_off = ops_bytes; o.read_begin = reads->h_seq_off[c.qid]; o.weight = ov.weight; o.ncols = ov.align_size; o.toff = ov.toff;
                    o.qsize = (i32)c.qsize; o.qoff = ov.qoff; o.qdir = c.qdir; o.tmpl = (u32)x; o.k = (u32)(k - T.ovlp_begin); o.tag_base = (u32)tag;
                    h_w[ovi] = ov.weight;
                    src[ovi] = ext->ops[ov.ops_block] + ov.ops_off;
                    ops_bytes += ((uint64_t)(ov.align_size + 3) / 4 + 7) & ~7ULL;
                    tag += (uint64_t)ov.align_size;
                }
                D.ntags = (u32)(tag - D.tag_base);
                pos += tsize + 1; seg += D.seg_cap;
            }
        }
        uint8_t* h_ops = sc.h_ops = (uint8_t*)result_alloc(std::max<uint64_t>(8, ops_bytes));
        if (!h_ops) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        cns::parallel_for(NO, [&](size_t i) { memcpy(h_ops + h_ov[i].ops_off, src[i], (size_t)(h_ov[i].ncols + 3) / 4); }, threads);
        const CnsChunkArena a(nt, NO, ops_bytes, T_, P, S);
        if (int rc = buf_ensure(ctx, ctx->cns_dev, a.lay.bytes())) return rc;
        const ArenaView A(ctx->cns_dev, a.lay, s);
        NECAT_HIP(ctx, A.upload(a.tm, h_tm.data(), nt));
        NECAT_HIP(ctx, A.upload(a.ov, h_ov.data(), NO));
        NECAT_HIP(ctx, A.upload(a.w, h_w.data(), NO));
        if (ops_bytes) NECAT_HIP(ctx, A.upload(a.ops, h_ops, ops_bytes));
        NECAT_HIP(ctx, A.zero(a.cnt, P + 1));
        NECAT_HIP(ctx, A.zero(a.cov, P + 1));
        NECAT_HIP(ctx, A.zero(a.flags, nt));
        const cd::DevTmpl* d_tm = A.cptr(a.tm); const cd::DevOvl* d_ov = A.cptr(a.ov);
        cd::DevGraph G;
        G.l_w = A.ptr(a.l_w); G.l_e = A.ptr(a.l_e); G.l_pred = A.ptr(a.l_pred); G.n_lfirst = A.ptr(a.n_lfirst); G.n_nlink = A.ptr(a.n_nlink);
        G.n_pos = A.ptr(a.n_pos); G.n_dc = A.ptr(a.n_dc); G.n_score = A.ptr(a.n_score); G.n_err = A.ptr(a.n_err); G.n_best = A.ptr(a.n_best);
        G.node_of_tag = A.ptr(a.node_of_tag); G.cov = A.ptr(a.cov); G.t_nodes = A.ptr(a.t_nodes); G.flags = A.ptr(a.flags);
        const unsigned g_ov = (unsigned)((NO + 3) / 4);
        NECAT_HIP(ctx, ev.record(0, s));
        hipLaunchKernelGGL(cd::k_cns_tags, dim3(g_ov), dim3(256), 0, s, d_ov, (u32)NO, d_tm, A.cptr(a.ops), (const u64*)reads->bases, A.ptr(a.key), A.ptr(a.cnt));
        NECAT_CHECK_LAUNCH(ctx, "k_cns_tags");
        NECAT_HIP(ctx, ev.record(1, s));
        hipLaunchKernelGGL(cd::k_cns_scan, dim3((unsigned)nt), dim3(256), 0, s, d_tm, A.cptr(a.cnt), A.ptr(a.off), A.ptr(a.cur));
        NECAT_CHECK_LAUNCH(ctx, "k_cns_scan");
        hipLaunchKernelGGL(cd::k_cns_scatter, dim3(g_ov), dim3(256), 0, s, d_ov, (u32)NO, d_tm, A.cptr(a.key), A.ptr(a.cur), A.ptr(a.key2));
        NECAT_CHECK_LAUNCH(ctx, "k_cns_scatter");
        hipLaunchKernelGGL(cd::k_cns_sort, dim3(grid_for(P, 4, 1u << 16)), dim3(256), 0, s, A.cptr(a.off), A.cptr(a.cnt), (u32)P, A.cptr(a.key2), A.ptr(a.key));
        NECAT_CHECK_LAUNCH(ctx, "k_cns_sort");
        NECAT_HIP(ctx, ev.record(2, s));
        hipLaunchKernelGGL(cd::k_cns_backbone, dim3((unsigned)nt), dim3(256), 0, s, d_tm, A.cptr(a.key), A.cptr(a.off), A.cptr(a.w), tol, G);
        NECAT_CHECK_LAUNCH(ctx, "k_cns_backbone");
        NECAT_HIP(ctx, ev.record(3, s));
        hipLaunchKernelGGL(cd::k_cns_path, dim3((unsigned)nt), dim3(64), 0, s, d_tm, A.cptr(a.off), G, opt->min_cov, opt->min_size, A.ptr(a.out), A.ptr(a.seg), A.ptr(a.seg_n));
        NECAT_CHECK_LAUNCH(ctx, "k_cns_path");
        NECAT_HIP(ctx, ev.record(4, s));
        std::vector<u32> h_fl(nt), h_sn(nt);
        std::vector<cd::Seg> h_seg(S);
        uint8_t* h_out = sc.h_out = (uint8_t*)result_alloc(T_ + 8);
        if (!h_out) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        NECAT_HIP(ctx, A.download(h_fl.data(), a.flags, nt));
        NECAT_HIP(ctx, A.download(h_sn.data(), a.seg_n, nt));
        NECAT_HIP(ctx, A.download(h_seg.data(), a.seg, S));
        NECAT_HIP(ctx, A.download(h_out, a.out, T_));
        NECAT_HIP(ctx, hipStreamSynchronize(s));
        for (int q = 0; q < 4; ++q) k_ms[q] += ev.ms(q);
        for (size_t x = 0; x < nt; ++x) {
            const uint64_t t = C.tmpl[x];
            n_uncertain += h_fl[x] & 1u;
            if (h_fl[x] || h_sn[x] > h_tm[x].seg_cap) { hand_back(t); continue; }
            ++n_device;
            kept[t].resize(h_sn[x]);
            for (u32 q = 0; q < h_sn[x]; ++q) {
                const cd::Seg& sg = h_seg[h_tm[x].seg_base + q];
                hc::SegCodes& o = kept[t][q];
                o.left = sg.left; o.right = sg.right; o.cns_from = sg.cns_from; o.cns_to = sg.cns_to;
                o.seq.assign((const char*)h_out + sg.off, sg.len);
            }
        }
        sc.drop_host();
        ++n_chunks;
        device_ms += wall_ms() - c0;
        if (knob().trace & 2) fprintf(stderr, "[necat] cns consensus chunk: %zu templates, %zu tags, %.2f ms\n", nt, T_, wall_ms() - c0);
        return NECAT_OK;
    }

    // The host form (cns_consensus.h) for the templates of host_list.  It reads query bases as byte codes; a volume lives on the device only, so the reads
    // these templates' overlaps name come back from it - read by read when they are a small part of the volume (the fallback's case), in one copy otherwise
    // (path 1: 1/4 byte per base over the link, 1 byte per base of host memory for the reads in use, for the length of the call).
    int host_form()
    {
        const double h0 = wall_ms();
        std::vector<uint64_t> code_off(reads->nseq, ~0ULL);          // where a needed read's codes start
        std::vector<uint64_t> need;
        uint64_t need_bases = 0;
        for (uint64_t t : host_list)
            for (uint64_t k = ext->templates[t].ovlp_begin; k < ext->templates[t].ovlp_end; ++k) {
                const uint64_t q = (uint64_t)cands[ext->overlaps[k].cand].qid;
                if (code_off[q] == ~0ULL) { code_off[q] = need_bases; need_bases += reads->h_seq_off[q + 1] - reads->h_seq_off[q]; need.push_back(q); }
            }
        std::vector<uint8_t> codes(need_bases + 1);
        auto expand = [&](uint64_t q, const necat_host::BaseWords& hb) { hb.decode((int64_t)q, 0, 0, (int64_t)hb.size((int64_t)q), codes.data() + code_off[q]); };
        std::vector<u64> words;
        int rc = NECAT_OK;
        if (need_bases * 4 >= reads->nbases) {
            if ((rc = fetch_words(ctx, reads, &words))) return rc;
            const necat_host::BaseWords hb = host_view(reads, words);
            cns::parallel_for(need.size(), [&](size_t x) { expand(need[x], hb); }, threads);
        } else {
            for (uint64_t q : need) {
                u64 word0 = 0;
                if ((rc = fetch_read_words(ctx, reads, q, &words, &word0))) return rc;
                expand(q, host_view(reads, words, word0));
            }
        }
        if (opt->path == 1) std::sort(host_list.begin(), host_list.end());
        necat_host::Deal deal(host_list.size());
        necat_host::on_threads((unsigned)std::min<size_t>(threads, host_list.size()), [&](unsigned) {
            hc::Worker w;
            std::vector<hc::OverlapIn> ovs;
            deal.run([&](uint64_t x) {
                const uint64_t t = host_list[x];
                const necat_cns_template& T = ext->templates[t];
                const necat_candidate& c0 = cands[tmpl_off[t]];
                ovs.clear();
                for (uint64_t k = T.ovlp_begin; k < T.ovlp_end; ++k) {
                    const necat_cns_overlap& ov = ext->overlaps[k];
                    const necat_candidate& c = cands[ov.cand];
                    hc::OverlapIn o;
                    o.ops = ext->ops[ov.ops_block] + ov.ops_off; o.ncols = ov.align_size; o.toff = ov.toff; o.weight = ov.weight;
                    o.qfwd = codes.data() + code_off[(uint64_t)c.qid]; o.qsize = (int)c.qsize; o.qoff = ov.qoff; o.qdir = c.qdir;
                    ovs.push_back(o);
                }
                hc::template_segments(w, ovs.data(), ovs.size(), (int)c0.ssize, c0.sid, opt->min_cov, opt->min_size, kept[t]);
                on_host[t] = 1;
            });
        });
        host_ms = wall_ms() - h0;
        return NECAT_OK;
    }

    // everything in three arrays the result owns; nullptr: out of memory
    necat_cns_consensus* result() const
    {
        uint64_t n_seg = 0, n_bases = 0;
        for (auto& v : kept) { n_seg += v.size(); for (auto& sg : v) n_bases += sg.seq.size(); }
        necat_cns_consensus* r = (necat_cns_consensus*)calloc(1, sizeof(necat_cns_consensus));
        if (r) {
            r->templates = (necat_cns_consensus_template*)calloc(std::max<uint64_t>(1, n_templates), sizeof(necat_cns_consensus_template));
            r->segments = (necat_cns_segment*)calloc(std::max<uint64_t>(1, n_seg), sizeof(necat_cns_segment));
            r->bases = (uint8_t*)malloc(std::max<uint64_t>(1, n_bases));
        }
        if (!r || !r->templates || !r->segments || !r->bases) { necat_cns_consensus_free(r); return nullptr; }
        uint64_t sg_at = 0, b_at = 0;
        for (uint64_t t = 0; t < n_templates; ++t) {
            necat_cns_consensus_template& o = r->templates[t];
            o.seg_begin = sg_at;
            for (const hc::SegCodes& sg : kept[t]) {
                necat_cns_segment& q = r->segments[sg_at++];
                q.left = sg.left; q.right = sg.right; q.cns_from = sg.cns_from; q.cns_to = sg.cns_to; q.off = b_at; q.len = (uint32_t)sg.seq.size();
                memcpy(r->bases + b_at, sg.seq.data(), sg.seq.size());
                b_at += sg.seq.size();
            }
            o.seg_end = sg_at;
            o.on_host = on_host[t];
            o.corrected = ext->templates[t].examined ? (opt->full_consensus ? (kept[t].empty() ? 0 : 1) : 1) : 0;
        }
        r->n_templates = n_templates; r->n_segments = n_seg; r->n_bases = n_bases;
        r->n_device = n_device; r->n_fallback = n_fallback; r->device_ms = device_ms; r->host_ms = host_ms; r->n_chunks = n_chunks; r->n_uncertain = n_uncertain;
        r->tags_ms = k_ms[0]; r->sort_ms = k_ms[1]; r->backbone_ms = k_ms[2]; r->path_ms = k_ms[3];
        return r;
    }
};

}  // namespace

int necat_cns_consensus_batch(necat_ctx* ctx, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off, uint64_t n_templates,
                              const necat_cns_result* ext, const necat_cns_consensus_options* opt, necat_cns_consensus** out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || !ext || !opt || !out || (n_templates && (!tmpl_off || !cands))) return NECAT_ERR_ARG;
    *out = nullptr;
    CnsConsensusCall call{ctx, reads, cands, tmpl_off, n_templates, ext, opt};
    int rc = call.validate();
    if (rc) return rc;
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    const double w0 = wall_ms();
    if (opt->path == 1) { for (uint64_t t = 0; t < n_templates; ++t) if (ext->templates[t].examined) call.host_list.push_back(t); }
    else {
        const std::vector<CnsDevChunk> chunks = call.plan_chunks();
        CnsDevScratch sc;
        if ((rc = sc.ev.create(ctx))) return rc;
        const double tol = (double)knob().cns_tol_scale;
        for (const CnsDevChunk& C : chunks) if ((rc = call.run_chunk(C, sc, tol))) return rc;
    }
    if (!call.host_list.empty() && (rc = call.host_form())) return rc;
    necat_cns_consensus* r = call.result();
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    if (knob().trace & 2) fprintf(stderr, "[necat] cns consensus %.2f ms: %lu templates on the device (%u chunks, %.2f ms: tags %.2f, sort %.2f, backbone %.2f, path %.2f), %lu handed back, host %.2f ms\n",
                             wall_ms() - w0, (unsigned long)r->n_device, r->n_chunks, r->device_ms, r->tags_ms, r->sort_ms, r->backbone_ms, r->path_ms, (unsigned long)r->n_fallback, r->host_ms);
    *out = r;
    return NECAT_OK;
}
