// stage_ctg_consensus.inl - the consensus half of contig polishing (ctg_cns/: tags -> backbone -> best path -> splice) behind the C ABI: tags, sort and run
// boundaries on the device range by range (ctg_dev_core.h, ctg_dev_kernels.h) with the score pass on the host, or all of it on the library's host threads
// (ctg_consensus.h).  One of the stage files of libnecat_hip.so's single translation unit.

// ------------------------------------------------------------------------------------------ contig polishing: the consensus half

void necat_ctg_consensus_default_options(necat_ctg_consensus_options* o)
{   // cns_ctg_subseq.h:12, cns_ctg_subseq.c:223.  The path: DESIGN 6b's rule (the device's slowest run against the host's fastest, profiles/ctg_consensus_bench.json)
    o->min_cov = necat_host::ctg::kMinCov; o->min_run = necat_host::ctg::kMinRun; o->path = 0; o->host_threads = 0;
}

void necat_ctg_consensus_free(necat_ctg_consensus* r)
{
    if (!r) return;
    free(r->segments); free(r->cns); free(r->t_pos); free(r->polished);
    free(r);
}

namespace {

namespace hg = necat_host::ctg;
namespace gd = necat::ctg_dev;

// One call of necat_ctg_consensus_batch: its arguments, what the steps hand on to each other, and the steps in the order the entry point takes them.
struct CtgConsensusCall {
    necat_ctx* ctx; const necat_volume* reads; int read_start_id; const necat_volume* contigs; const necat_ctg_segment* segs; uint64_t n_segs;
    const necat_ctg_overlap* ovl; const uint8_t* ops; const necat_ctg_consensus_options* opt;
    unsigned threads = 1;
    std::vector<hg::SegmentOut> res;
    std::vector<std::string> polished;
    std::vector<uint32_t> seg_chunks;
    std::vector<u64> ctg_words;
    double device_ms = 0, host_ms = 0, plan_ms = 0, score_ms = 0, k_ms[3] = {0, 0, 0};
    uint32_t n_chunks = 0;

    uint64_t read_of(const necat_ctg_overlap& o) const { return (uint64_t)((int64_t)o.qid - read_start_id); }
    int qsize_of(const necat_ctg_overlap& o) const { const uint64_t q = read_of(o); return (int)(reads->h_seq_off[q + 1] - reads->h_seq_off[q]); }

    // the options, the segments, and every overlap against its read, its segment and its own columns: nothing below checks again
    int validate()
    {
        if (opt->min_cov < 0 || opt->min_run < 1 || (opt->path != 0 && opt->path != 1) || opt->host_threads < 0)
            return set_err(ctx, NECAT_ERR_ARG, "contig consensus options out of range (min_cov >= 0, min_run >= 1, path 0 or 1, host_threads >= 0)");
        threads = call_threads(ctx, opt->host_threads);
        for (uint64_t s = 0; s < n_segs; ++s) if (int rc = ctg_segment_check(ctx, contigs, segs[s], s, 0, "overlap")) return rc;
        std::atomic<uint64_t> bad{~0ULL};
        std::vector<std::pair<uint64_t, uint64_t>> list;        // (segment, overlap)
        for (uint64_t s = 0; s < n_segs; ++s) for (uint64_t k = segs[s].ovlp_begin; k < segs[s].ovlp_end; ++k) list.emplace_back(s, k);
        std::vector<const char*> why(list.size(), nullptr);
        necat_host::deal(list.size(), (unsigned)std::min<size_t>(threads, std::max<size_t>(1, list.size())), 16, [&](uint64_t x, unsigned) {
            const necat_ctg_overlap& o = ovl[list[x].second];
            SeqAt q;
            if (!seq_at(reads, o.qid, read_start_id, &q) || q.len >= (1ULL << 31)) why[x] = "names no read of the volume";
            else if (o.qdir != 0 && o.qdir != 1) why[x] = "has a strand that is neither 0 nor 1";
            else why[x] = hg::overlap_fault(ops + o.ops_off, o.align_size, o.qoff, o.qend, o.toff, o.tend, qsize_of(o), segs[list[x].first].size);
            if (why[x]) { uint64_t cur = bad.load(); while (x < cur && !bad.compare_exchange_weak(cur, x)) {} }
        });
        if (bad.load() != ~0ULL) { const uint64_t x = bad.load(); return set_err(ctx, NECAT_ERR_ARG, "overlap %lu (segment %lu) %s", (unsigned long)list[x].second, (unsigned long)list[x].first, why[x]); }
        res.assign(n_segs, hg::SegmentOut());
        polished.assign(n_segs, std::string());
        seg_chunks.assign(n_segs, 0);
        return NECAT_OK;
    }

    void finish_segment(uint64_t s)
    {
        if (!contigs) return;
        const necat_ctg_segment& S = segs[s];
        const u64 b0 = contigs->h_seq_off[S.ctg_id] + (u64)S.from;
        const necat_host::BaseWords w = host_view(contigs, ctg_words);
        hg::splice(res[s].cns, res[s].t_pos, [&](int x) { return (unsigned)w.base(b0 + (u64)x); }, S.size, opt->min_run, polished[s]);
    }

    // path 1: the host form, one segment per thread
    int host_form()
    {
        const double h0 = wall_ms();
        std::vector<u64> words;
        int rc = fetch_words(ctx, reads, &words);
        if (rc) return rc;
        necat_host::deal(n_segs, (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(1, n_segs)), 1, [&](uint64_t s, unsigned) {
            std::vector<hg::OverlapIn> in;
            for (uint64_t k = segs[s].ovlp_begin; k < segs[s].ovlp_end; ++k) {
                const necat_ctg_overlap& o = ovl[k];
                hg::OverlapIn q;
                q.ops = ops + o.ops_off; q.ncols = o.align_size; q.toff = o.toff; q.words = words.data(); q.read_begin = reads->h_seq_off[read_of(o)];
                q.qsize = qsize_of(o); q.qoff = o.qoff; q.qdir = o.qdir;
                in.push_back(q);
            }
            hg::segment_consensus(in.data(), in.size(), segs[s].size, opt->min_cov, res[s]);
            finish_segment(s);
        });
        host_ms = wall_ms() - h0;
        return NECAT_OK;
    }

    // path 0, one segment: plan, then range by range on the device, then the host's score pass on the downloaded nodes and links
    int device_segment(uint64_t s, const CallEvents<4>& ev)
    {
        const necat_ctg_segment& S = segs[s];
        const u32 size = (u32)S.size;
        const uint64_t n_ov = S.ovlp_end - S.ovlp_begin;
        hipStream_t st = ctx->stream;
        // ---- plan
        const double p0 = wall_ms();
        std::vector<gd::OvlPlan> plans(n_ov);
        std::vector<u64> ops_at(n_ov + 1, 0);
        for (uint64_t k = 0; k < n_ov; ++k) ops_at[k + 1] = ops_at[k] + ((((u64)ovl[S.ovlp_begin + k].align_size + 3) / 4 + 7) & ~7ULL);
        std::vector<u8> h_ops(ops_at[n_ov] + 8);
        necat_host::deal(n_ov, (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(1, n_ov)), 4, [&](uint64_t k, unsigned) {
            const necat_ctg_overlap& o = ovl[S.ovlp_begin + k];
            gd::plan_overlap(ops + o.ops_off, o.align_size, o.toff, plans[k]);
            memcpy(h_ops.data() + ops_at[k], ops + o.ops_off, ((size_t)o.align_size + 3) / 4);
        });
        std::vector<u64> block_tags(((size_t)size + (1u << gd::kBlockShift) - 1) >> gd::kBlockShift, 0);
        for (uint64_t k = 0; k < n_ov; ++k) for (size_t m = 0; m < plans[k].marks.size(); ++m) block_tags[(size_t)plans[k].block0 + m] += plans[k].marks[m].tags;
        const std::vector<gd::Range> ranges = gd::plan_ranges(block_tags, size, knob().cns_tag_budget);
        std::vector<std::vector<gd::RangeOvl>> r_ov(ranges.size());
        u64 max_slots = 0, max_pos = 0, max_ov = 0;
        for (size_t r = 0; r < ranges.size(); ++r) {
            u64 slots = 0;
            if (ranges[r].tags) for (uint64_t k = 0; k < n_ov; ++k) {
                gd::RangeOvl o;
                if (!gd::range_overlap(plans[k], ranges[r], &o.st, &o.slots) || !o.slots) continue;
                const necat_ctg_overlap& v = ovl[S.ovlp_begin + k];
                o.ops_off = ops_at[k]; o.read_begin = reads->h_seq_off[read_of(v)]; o.toff = v.toff - (i32)ranges[r].p0; o.qsize = qsize_of(v); o.qoff = v.qoff; o.qdir = v.qdir;
                o.slot_base = (u32)slots;
                slots += o.slots;
                r_ov[r].push_back(o);
            }
            if (slots >= (1ULL << 31)) return set_err(ctx, NECAT_ERR_ARG, "segment %lu: one block of 64 positions holds 2^31 alignment columns or more", (unsigned long)s);
            max_slots = std::max(max_slots, slots); max_pos = std::max<u64>(max_pos, ranges[r].p1 - ranges[r].p0); max_ov = std::max<u64>(max_ov, r_ov[r].size());
        }
        plan_ms += wall_ms() - p0;
        hg::Graph G;
        gd::graph_begin(G, size);
        if (max_slots) {
            // ---- one arena for the segment: its columns, then what the largest range needs
            const double d0 = wall_ms();
            const CtgRangeArena a(h_ops.size(), max_ov, max_slots, max_pos);
            if (int rc = buf_ensure(ctx, ctx->cns_dev, a.lay.bytes())) return rc;
            const ArenaView A(ctx->cns_dev, a.lay, st);
            NECAT_HIP(ctx, A.upload(a.ops, h_ops.data(), h_ops.size()));
            gd::DevLinks L;
            L.n_pos = A.ptr(a.n_pos); L.n_db = A.ptr(a.n_db); L.n_link0 = A.ptr(a.n_link0); L.l_pred = A.ptr(a.l_pred); L.l_tag0 = A.ptr(a.l_tag0);
            L.pos_node = A.ptr(a.pos_node); L.cov = A.ptr(a.cov);
            for (size_t r = 0; r < ranges.size(); ++r) {
                const gd::Range& R = ranges[r];
                gd::RangeOut O;
                if (r_ov[r].empty()) { gd::graph_append(G, O, R); continue; }
                const u32 rs = R.p1 - R.p0, NO = (u32)r_ov[r].size(), slots = r_ov[r].back().slot_base + r_ov[r].back().slots, n_tiles = (rs + gd::kTilePositions - 1) / gd::kTilePositions;
                cd::DevTmpl tm = {};
                tm.tag_base = 0; tm.ntags = slots; tm.pos_base = 0; tm.tsize = (i32)rs;
                NECAT_HIP(ctx, A.upload(a.ov, r_ov[r].data(), NO));
                NECAT_HIP(ctx, A.upload(a.tm, &tm, 1));
                NECAT_HIP(ctx, A.zero(a.cnt, (size_t)rs + 2));
                NECAT_HIP(ctx, A.zero(a.cov, rs));
                NECAT_HIP(ctx, A.fill(a.pos_node, 0xff, rs));
                NECAT_HIP(ctx, A.zero(a.big, 1));
                NECAT_HIP(ctx, ev.record(0, st));
                hipLaunchKernelGGL(gd::k_ctg_tags, dim3((NO + 3) / 4), dim3(256), 0, st, A.cptr(a.ov), NO, rs, A.cptr(a.ops), (const u64*)reads->bases, A.ptr(a.key), A.ptr(a.cnt));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_tags");
                NECAT_HIP(ctx, ev.record(1, st));
                hipLaunchKernelGGL(cd::k_cns_scan, dim3(1), dim3(256), 0, st, A.cptr(a.tm), A.cptr(a.cnt), A.ptr(a.off), A.ptr(a.cur));
                NECAT_CHECK_LAUNCH(ctx, "k_cns_scan");
                hipLaunchKernelGGL(gd::k_ctg_scatter, dim3(grid_for(slots, 256, 1u << 16)), dim3(256), 0, st, A.cptr(a.key), slots, rs, A.ptr(a.cur), A.ptr(a.key2));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_scatter");
                hipLaunchKernelGGL(gd::k_ctg_sort, dim3(grid_for(rs, 4, 1u << 16)), dim3(256), 0, st, A.cptr(a.off), A.cptr(a.cnt), rs, A.cptr(a.key2), A.ptr(a.key), A.ptr(a.big));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_sort");
                hipLaunchKernelGGL(gd::k_ctg_sort_big, dim3(1024), dim3(256), 0, st, A.cptr(a.off), A.cptr(a.cnt), A.cptr(a.big), A.cptr(a.key2), A.ptr(a.key));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_sort_big");
                NECAT_HIP(ctx, ev.record(2, st));
                hipLaunchKernelGGL(gd::k_ctg_count, dim3(n_tiles), dim3(256), 0, st, A.cptr(a.key), A.cptr(a.off), rs, A.ptr(a.tile_cnt));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_count");
                hipLaunchKernelGGL(gd::k_ctg_tile_scan, dim3(1), dim3(256), 0, st, A.cptr(a.tile_cnt), n_tiles, A.ptr(a.tile_base));
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_tile_scan");
                hipLaunchKernelGGL(gd::k_ctg_links, dim3(n_tiles), dim3(256), 0, st, A.cptr(a.key), A.cptr(a.off), rs, R.p0, A.cptr(a.tile_base), L);
                NECAT_CHECK_LAUNCH(ctx, "k_ctg_links");
                NECAT_HIP(ctx, ev.record(3, st));
                u64 total = 0; u32 live = 0;
                NECAT_HIP(ctx, A.download(&total, a.tile_base, 1, n_tiles));
                NECAT_HIP(ctx, A.download(&live, a.off, 1, rs));
                NECAT_HIP(ctx, hipStreamSynchronize(st));
                const u32 nn = (u32)total, nl = (u32)(total >> 32);
                if (live != R.tags || nn > live || nl > live || nl < nn)
                    return set_err(ctx, NECAT_ERR_INTERNAL, "segment %lu, positions %u .. %u: the device counted %u tags, %u nodes, %u links, the plan %lu tags", (unsigned long)s, R.p0, R.p1, live, nn, nl, (unsigned long)R.tags);
                O.n_tags = live;
                O.n_pos.resize(nn); O.n_db.resize(nn); O.n_link0.resize(nn); O.l_pred.resize(nl); O.l_tag0.resize(nl); O.pos_node.resize(rs); O.cov.resize(rs);
                if (nn) {
                    NECAT_HIP(ctx, A.download(O.n_pos.data(), a.n_pos, nn));
                    NECAT_HIP(ctx, A.download(O.n_db.data(), a.n_db, nn));
                    NECAT_HIP(ctx, A.download(O.n_link0.data(), a.n_link0, nn));
                    NECAT_HIP(ctx, A.download(O.l_pred.data(), a.l_pred, nl));
                    NECAT_HIP(ctx, A.download(O.l_tag0.data(), a.l_tag0, nl));
                }
                NECAT_HIP(ctx, A.download(O.pos_node.data(), a.pos_node, rs));
                NECAT_HIP(ctx, A.download(O.cov.data(), a.cov, rs));
                NECAT_HIP(ctx, hipStreamSynchronize(st));
                for (int q = 0; q < 3; ++q) k_ms[q] += ev.ms(q);
                gd::graph_append(G, O, R);
                ++n_chunks; ++seg_chunks[s];
                if (knob().trace & 2) fprintf(stderr, "[necat] ctg consensus: segment %lu, positions %u .. %u: %u overlaps, %u tags, %u nodes, %u links\n", (unsigned long)s, R.p0, R.p1, NO, live, nn, nl);
            }
            device_ms += wall_ms() - d0;
        } else {
            for (const gd::Range& R : ranges) gd::graph_append(G, gd::RangeOut(), R);
        }
        gd::graph_end(G, size);
        // ---- the host's part: a chain of dependent steps as long as the segment
        const double s0 = wall_ms();
        res[s].n_tags = G.n_tags; res[s].n_nodes = G.nodes(); res[s].n_links = G.links();
        hg::best_path(G, opt->min_cov, res[s].cns, res[s].t_pos);
        finish_segment(s);
        score_ms += wall_ms() - s0;
        return NECAT_OK;
    }

    // everything in four arrays the result owns; nullptr: out of memory
    necat_ctg_consensus* result() const
    {
        uint64_t n_cns = 0, n_pol = 0;
        for (uint64_t s = 0; s < n_segs; ++s) { n_cns += res[s].cns.size(); n_pol += polished[s].size(); }
        necat_ctg_consensus* r = (necat_ctg_consensus*)calloc(1, sizeof(necat_ctg_consensus));
        if (r) {
            r->segments = (necat_ctg_consensus_segment*)calloc(std::max<uint64_t>(1, n_segs), sizeof(necat_ctg_consensus_segment));
            r->cns = (char*)malloc(std::max<uint64_t>(1, n_cns)); r->t_pos = (int32_t*)malloc(std::max<uint64_t>(1, n_cns) * 4); r->polished = (char*)malloc(std::max<uint64_t>(1, n_pol));
        }
        if (!r || !r->segments || !r->cns || !r->t_pos || !r->polished) { necat_ctg_consensus_free(r); return nullptr; }
        uint64_t c_at = 0, p_at = 0;
        for (uint64_t s = 0; s < n_segs; ++s) {
            necat_ctg_consensus_segment& o = r->segments[s];
            o.cns_off = c_at; o.cns_len = res[s].cns.size(); o.polished_off = p_at; o.polished_len = polished[s].size();
            o.n_tags = res[s].n_tags; o.n_nodes = res[s].n_nodes; o.n_links = res[s].n_links; o.n_chunks = seg_chunks[s];
            if (o.cns_len) { memcpy(r->cns + c_at, res[s].cns.data(), o.cns_len); memcpy(r->t_pos + c_at, res[s].t_pos.data(), o.cns_len * 4); }
            if (o.polished_len) memcpy(r->polished + p_at, polished[s].data(), o.polished_len);
            c_at += o.cns_len; p_at += o.polished_len;
        }
        r->n_segments = n_segs; r->n_cns = n_cns; r->n_polished = n_pol; r->n_fallback = 0; r->n_chunks = n_chunks;
        r->device_ms = device_ms; r->tags_ms = k_ms[0]; r->sort_ms = k_ms[1]; r->links_ms = k_ms[2]; r->plan_ms = plan_ms; r->score_ms = score_ms; r->host_ms = host_ms;
        return r;
    }
};

}  // namespace

int necat_ctg_consensus_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs, const necat_ctg_segment* segments, uint64_t n_segments,
                              const necat_ctg_overlap* overlaps, const uint8_t* ops, const necat_ctg_consensus_options* opt, necat_ctg_consensus** out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || !opt || !out || (n_segments && !segments)) return NECAT_ERR_ARG;
    *out = nullptr;
    for (uint64_t s = 0; s < n_segments; ++s)
        if (segments[s].ovlp_begin < segments[s].ovlp_end && (!overlaps || !ops)) return set_err(ctx, NECAT_ERR_ARG, "segment %lu has overlaps, the call none", (unsigned long)s);
    CtgConsensusCall call{ctx, reads, read_start_id, contigs, segments, n_segments, overlaps, ops, opt};
    const double w0 = wall_ms();
    int rc = call.validate();
    if (rc) return rc;
    call.plan_ms = wall_ms() - w0;
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    if (contigs && (rc = fetch_words(ctx, contigs, &call.ctg_words))) return rc;
    if (opt->path == 1) { if ((rc = call.host_form())) return rc; }
    else {
        CallEvents<4> ev;
        if ((rc = ev.create(ctx))) return rc;
        for (uint64_t s = 0; s < n_segments; ++s) if ((rc = call.device_segment(s, ev))) return rc;
    }
    necat_ctg_consensus* r = call.result();
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    if (knob().trace & 2) fprintf(stderr, "[necat] ctg consensus %.2f ms: %lu segments, %u ranges, plan %.2f ms, device %.2f ms (tags %.2f, sort %.2f, links %.2f), score %.2f ms, host form %.2f ms\n",
                             wall_ms() - w0, (unsigned long)n_segments, r->n_chunks, r->plan_ms, r->device_ms, r->tags_ms, r->sort_ms, r->links_ms, r->score_ms, r->host_ms);
    *out = r;
    return NECAT_OK;
}
