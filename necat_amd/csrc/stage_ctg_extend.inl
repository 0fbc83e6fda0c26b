// stage_ctg_extend.inl - the aligner and the coverage cap of contig polishing (the middle of extend_ctg_m4s, ctg_cns/cns_ctg_subseq.c:119-197) behind the C ABI:
// cns_extension of every seeded record against its SEGMENT ahead of the loop - the block-wise aligner through extend_impl with a per-candidate base offset into
// the contig (ext_kernels.h: k_ext_init's third way to place a subject), the rescue pair through pair_local / pair_global on slices of the resident contig
// (rescue_pair.h), or through cns::Rescuer on the host threads - then the loop itself as one serial host pass per segment over that table (ctg_extend.h).
// One of the stage files of libnecat_hip.so's single translation unit.

// ------------------------------------------------------------------------------------------ contig polishing: the aligner and the coverage cap

void necat_ctg_extend_default_options(necat_ctg_extend_options* o)
{
    o->cap = 1; o->rescue_path = 0; o->host_threads = 0; o->_pad = 0;
}

void necat_ctg_extend_free(necat_ctg_extend* r)
{
    if (!r) return;
    free(r->jobs); free(r->segments); free(r->overlaps); free(r->ops);
    free(r);
}

namespace {

namespace cx = necat_host::ctg_ext;
static_assert(cx::kMaxSegment == necat_host::ctg::kMaxSegment, "one bound on a segment for the contig stages");
static_assert(NECAT_CTG_EXT_CAPPED == cx::kCapped && NECAT_CTG_EXT_NO_SEED == cx::kNoSeed && NECAT_CTG_EXT_NO_ALIGNMENT == cx::kNoAlignment &&
              NECAT_CTG_EXT_REJECTED == cx::kRejected && NECAT_CTG_EXT_ACCEPTED == cx::kAccepted, "the header's verdicts are ctg_extend.h's");

// One call of necat_ctg_extend_batch: its arguments, what the steps hand on to each other, and the steps in the order the entry point takes them.
struct CtgExtendCall {
    necat_ctx* ctx; const necat_volume* reads; int read_start_id; const necat_volume* contigs; const necat_ctg_segment* segs; uint64_t n_segs;
    const necat_ctg_extend_job* jobs; const necat_ctg_seed* seeds; const necat_ctg_extend_options* opt;
    unsigned threads = 1;
    uint64_t n_jobs = 0;
    necat_ctg_seed* own_seeds = nullptr;
    std::vector<uint32_t> seg_of;                   // job -> its segment
    // the seeded jobs, segment by segment: entry x of `list` is candidate x of the aligner's call
    std::vector<uint64_t> list;
    std::vector<necat_candidate> cands;
    std::vector<u64> sub;                           // the segment's first base on its contig
    struct Got { necat_alignment a; const u8* cols; int32_t decided; };
    std::vector<Got> got;
    necat_alignment* aln = nullptr;                 // the block-wise results and their column blocks (result_alloc)
    std::vector<std::pair<u8*, u64>> parts;
    std::vector<std::vector<u8>> pair_cols;         // the accepted pairs' columns
    necat_ctg_extend st;                            // the counters and times (the arrays stay null until result())

    ~CtgExtendCall()
    {
        necat_ctg_seed_free(own_seeds);
        necat_free(aln);
        for (auto& pr : parts) necat_free(pr.first);
    }

    uint64_t read_of(uint64_t k) const { return (uint64_t)((int64_t)jobs[k].qid - read_start_id); }
    int qsize_of(uint64_t k) const { const uint64_t q = read_of(k); return (int)(reads->h_seq_off[q + 1] - reads->h_seq_off[q]); }
    u64 seg_base(const necat_ctg_segment& S) const { return contigs->h_seq_off[S.ctg_id] + (u64)S.from; }

    // the options, the segments and every job: nothing below checks again
    int validate()
    {
        memset(&st, 0, sizeof st);
        if ((opt->cap != 0 && opt->cap != 1) || (opt->rescue_path != 0 && opt->rescue_path != 1) || opt->host_threads < 0)
            return set_err(ctx, NECAT_ERR_ARG, "contig extension options out of range (cap 0 or 1, rescue_path 0 or 1, host_threads >= 0)");
        threads = call_threads(ctx, opt->host_threads);
        for (uint64_t s = 0; s < n_segs; ++s) {
            if (int rc = ctg_segment_check(ctx, contigs, segs[s], s, necat_host::ctg_seed::kK, "job")) return rc;
            n_jobs = std::max<uint64_t>(n_jobs, segs[s].ovlp_end);
        }
        if (seeds && seeds->n_jobs != n_jobs)
            return set_err(ctx, NECAT_ERR_ARG, "the seed table holds %lu jobs, the segments name %lu", (unsigned long)seeds->n_jobs, (unsigned long)n_jobs);
        seg_of.assign(n_jobs, ~0u);
        for (uint64_t s = 0; s < n_segs; ++s) {
            const necat_ctg_segment& S = segs[s];
            if (opt->rescue_path == 0 && (u64)S.from + (u64)S.size >= (1ULL << 31) && S.ovlp_begin < S.ovlp_end)
                return set_err(ctx, NECAT_ERR_ARG, "segment %lu ends 2^31 bases or more into its contig (rescue_path 0)", (unsigned long)s);
            for (uint64_t k = S.ovlp_begin; k < S.ovlp_end; ++k) {
                SeqAt q;
                if (!seq_at(reads, jobs[k].qid, read_start_id, &q)) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu) names no read of the volume", (unsigned long)k, (unsigned long)s);
                if (q.len >= (u64)necat_host::ctg_seed::kMaxRead) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu): a read of 2^30 bases or more", (unsigned long)k, (unsigned long)s);
                if (jobs[k].qdir != 0 && jobs[k].qdir != 1) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu) has a strand that is neither 0 nor 1", (unsigned long)k, (unsigned long)s);
                int32_t sb, se;
                if (!cx::record_range(jobs[k].soff, jobs[k].send, S.from, S.size, &sb, &se))
                    return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu) ends at or before its segment's start", (unsigned long)k, (unsigned long)s);
                if (seg_of[k] != ~0u) return set_err(ctx, NECAT_ERR_ARG, "job %lu is named by segments %lu and %lu", (unsigned long)k, (unsigned long)seg_of[k], (unsigned long)s);
                seg_of[k] = (uint32_t)s;
            }
        }
        return NECAT_OK;
    }

    // step 3 for every job: the caller's table, or necat_ctg_seed_batch at its defaults
    int seed()
    {
        if (seeds) return NECAT_OK;
        const double t0 = wall_ms();
        std::vector<necat_ctg_seed_job> sj(std::max<uint64_t>(1, n_jobs));
        for (uint64_t k = 0; k < n_jobs; ++k) sj[k] = necat_ctg_seed_job{jobs[k].qid, jobs[k].qdir};
        necat_ctg_seed_options so;
        necat_ctg_seed_default_options(&so);
        so.host_threads = opt->host_threads;
        if (int rc = necat_ctg_seed_batch(ctx, reads, read_start_id, contigs, segs, n_segs, sj.data(), &so, &own_seeds)) return rc;
        seeds = own_seeds;
        st.seed_ms = wall_ms() - t0;
        return NECAT_OK;
    }

    // step 4, first half: can_list[0] with qsize = the read's length and ssize = the segment's (cns_ctg_subseq.c:159-161) through the block-wise aligner,
    // tail length ONC_TAIL_MATCH_LEN_LONG, columns kept; the subject of candidate x is `size` bases from base sub[x] of the contig on
    int align()
    {
        const double t0 = wall_ms();
        for (uint64_t s = 0; s < n_segs; ++s) {
            const necat_ctg_segment& S = segs[s];
            for (uint64_t k = S.ovlp_begin; k < S.ovlp_end; ++k) {
                const necat_ctg_seed_result& R = seeds->jobs[k];
                if (!R.found) continue;
                const int rl = qsize_of(k);
                if (R.qbeg < 0 || R.qbeg > R.qend || R.qend > rl || R.sbeg < 0 || R.sbeg > R.send || R.send > S.size || R.qoff < 0 || R.qoff > rl || R.soff < 0 || R.soff > S.size)
                    return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu): the seed table's candidate lies outside the read or the segment", (unsigned long)k, (unsigned long)s);
                necat_candidate c;
                memset(&c, 0, sizeof c);
                c.qid = jobs[k].qid; c.sid = S.ctg_id; c.qdir = jobs[k].qdir; c.sdir = 0; c.score = R.score;
                c.qbeg = (u64)R.qbeg; c.qend = (u64)R.qend; c.qsize = (u64)rl; c.sbeg = (u64)R.sbeg; c.send = (u64)R.send; c.ssize = (u64)S.size;
                c.qoff = (u64)R.qoff; c.soff = (u64)R.soff;
                list.push_back(k); cands.push_back(c); sub.push_back((u64)S.from);
            }
        }
        const uint64_t m = list.size();
        st.n_seeded = st.n_aligned = m;
        got.assign(m, Got{necat_alignment(), nullptr, cx::kByNone});
        if (!m) return NECAT_OK;
        if (m >= (1ULL << 31)) return set_err(ctx, NECAT_ERR_ARG, "2^31 seeded jobs or more in one call");
        AlignOut ao;
        ao.aln = (necat_alignment*)result_alloc(m * sizeof(necat_alignment));
        if (!ao.aln) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
        ao.off.assign(m + 1, 0);
        ao.sub_off = sub.data();
        necat_map_options mo;
        necat_default_options(&mo);
        mo.error = cx::kError; mo.align_size_cutoff = cx::kMinAlignSize;
        const int rc = extend_impl(ctx, contigs, reads, read_start_id, 0, cands.data(), m, &mo, 4 /* ONC_TAIL_MATCH_LEN_LONG, oc_aligner.h:42 */, nullptr, nullptr, &ao);
        aln = ao.aln; parts.swap(ao.parts);
        if (rc) return rc;
        size_t p = 0; u64 p_start = 0;
        for (uint64_t x = 0; x < m; ++x) {
            Got& g = got[x];
            g.a = aln[x];
            g.decided = g.a.ok ? cx::kByBlocks : cx::kByNone;
            if (ao.off[x + 1] == ao.off[x]) continue;          // no columns
            while (p < parts.size() && ao.off[x] >= p_start + parts[p].second) { p_start += parts[p].second; ++p; }
            if (p >= parts.size() || ao.off[x + 1] > p_start + parts[p].second) return set_err(ctx, NECAT_ERR_INTERNAL, "contig extension: the columns of job %lu lie in no block", (unsigned long)list[x]);
            g.cols = parts[p].first + (ao.off[x] - p_start);
        }
        st.cols_bytes_downloaded += ao.total;
        st.align_ms = wall_ms() - t0;
        return NECAT_OK;
    }

    // the pair's accepted result over the block-wise one (cns_ctg_subseq.c:84-93)
    void take_pair(uint64_t x, const necat_nw_result& r, std::vector<u8>& packed)
    {
        cns::take_rescued(r, &got[x].a);
        pair_cols.emplace_back();
        pair_cols.back().swap(packed);
        got[x].cols = pair_cols.back().data();
        got[x].decided = cx::kByPair;
        st.cols_bytes_downloaded += pair_cols.back().size();
        ++st.n_pair_accepted;
    }

    // rescue_path 0: the device pair (pair_local, pair_global) for every entry of `need` on (read on its strand, the segment as a slice of the resident contig)
    int pair_on_device(const std::vector<uint64_t>& need)
    {
        const uint64_t n = need.size();
        if (n >= (1ULL << 30)) return set_err(ctx, NECAT_ERR_ARG, "2^30 rescue jobs or more in one call");
        std::vector<pair::Job> pj(n);
        for (uint64_t k = 0; k < n; ++k) {
            const necat_candidate& c = cands[need[k]];
            SeqAt q;
            (void)seq_at(reads, c.qid, read_start_id, &q);
            pj[k] = pair::Job{c.qid, c.qdir, c.sid, (i64)q.begin, (i64)q.len, (i64)contigs->h_seq_off[c.sid], (i64)sub[need[k]], (i64)c.ssize, (i64)c.qoff, (i64)c.soff};
        }
        std::vector<necat_dalign_result> ranges(n);
        PairLocal L;
        int rc = pair_local(ctx, contigs, reads, pj, cx::kError, cx::kMinAlignSize, ranges.data(), &L);
        if (rc) return rc;
        st.n_dalign_device += L.sv.n_tier[0]; st.n_dalign_host += L.sv.n_host; st.n_dalign_over_cap += L.sv.n_over_cap; st.n_dalign_selfcheck += L.sv.n_selfcheck;
        PairGlobal G;
        if ((rc = pair_global(ctx, contigs, reads, read_start_id, 0, pj, ranges.data(), cx::kError, cx::kMinAlignSize, true, &G))) return rc;
        st.n_nw_jobs += G.job_of.size(); st.n_nw_device += G.ns.n_device; st.n_nw_host += G.ns.n_host;
        for (size_t j = 0; j < G.res.size(); ++j) if (G.res[j].ok) take_pair(need[G.job_of[j]], G.res[j], G.cols[j]);
        return NECAT_OK;
    }

    // rescue_path 1: cns::Rescuer on the call's threads over the fetched words, the segment decoded where it lies
    int pair_on_host(const std::vector<uint64_t>& need)
    {
        std::vector<u64> rwords, cwords;
        int rc = fetch_words(ctx, reads, &rwords);
        if (rc || (rc = fetch_words(ctx, contigs, &cwords))) return rc;
        const necat_host::BaseWords hr = host_view(reads, rwords), hc = host_view(contigs, cwords);
        const rescue::DalignSpec dspec = rescue::spec_for_error(cx::kError);
        std::vector<necat_nw_result> nr(need.size());
        std::vector<std::vector<u8>> packed(need.size());
        std::vector<u8> okv(need.size(), 0), ranged(need.size(), 0);
        necat_host::deal(need.size(), (unsigned)std::min<size_t>(threads, std::max<size_t>(1, need.size())), 1, [&](uint64_t k, unsigned) {
            const necat_candidate& c = cands[need[k]];
            rescue::Dalign dal(dspec);
            rescue::EdlibGo edl(cx::kError);
            std::vector<u8> q, t((size_t)c.ssize);
            hr.strand((int64_t)c.qid - read_start_id, c.qdir, q);
            hc.stretch(contigs->h_seq_off[c.sid] + sub[need[k]], (int64_t)c.ssize, 0, t.data());
            if (!cns::rescue_local(dal, c, q.data(), t.data(), cx::kMinAlignSize)) return;
            ranged[k] = 1;
            okv[k] = cns::edlib_job(edl, q.data(), t.data(), cns::rescue_job(c, dal.r), cx::kMinAlignSize, 4, &nr[k], &packed[k]);
        });
        for (size_t k = 0; k < need.size(); ++k) {
            st.n_dalign_host += 1; st.n_nw_jobs += ranged[k]; st.n_nw_host += ranged[k];
            if (okv[k]) take_pair(need[k], nr[k], packed[k]);
        }
        return NECAT_OK;
    }

    // step 4, second half: the pair once for all jobs the hang rule names (cns_ctg_subseq.c:44-51, :63-95); where it gives nothing the block-wise result stands if it was ok
    int rescue_pair()
    {
        const double t0 = wall_ms();
        std::vector<uint64_t> need;
        for (uint64_t x = 0; x < list.size(); ++x) if (cns::extension_short(cands[x], got[x].a)) need.push_back(x);
        st.n_pair_tried = need.size();
        if (need.empty()) return NECAT_OK;
        pair_cols.reserve(need.size());          // (take_pair keeps pointers into its elements)
        if (int rc = opt->rescue_path == 0 ? pair_on_device(need) : pair_on_host(need)) return rc;
        for (uint64_t x : need) if (got[x].decided != cx::kByPair) got[x].decided = got[x].a.ok ? cx::kByBlocksKept : cx::kByNone;
        st.rescue_ms = wall_ms() - t0;
        return NECAT_OK;
    }

    // steps 1, 2, 5 and 6: the loop, segment by segment over the table, and everything in arrays the result owns; nullptr: out of memory
    necat_ctg_extend* result()
    {
        const double t0 = wall_ms();
        std::vector<cx::Aligned> tab(n_jobs, cx::Aligned{0, 0, 0, 0, 0, 0, 0.0});
        std::vector<uint64_t> entry(n_jobs, ~0ULL);
        for (uint64_t x = 0; x < list.size(); ++x) {
            const necat_alignment& a = got[x].a;
            tab[list[x]] = cx::Aligned{1, a.ok, a.qoff, a.qend, a.toff, a.tend, a.ident_perc};
            entry[list[x]] = x;
        }
        std::vector<cx::Pass> pass(n_segs);
        necat_host::deal(n_segs, (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(1, n_segs)), 1, [&](uint64_t s, unsigned) {
            const necat_ctg_segment& S = segs[s];
            cx::replay(S.size, S.ovlp_end - S.ovlp_begin, opt->cap != 0,
                       [&](uint64_t k, int32_t* sb, int32_t* se) { (void)cx::record_range(jobs[S.ovlp_begin + k].soff, jobs[S.ovlp_begin + k].send, S.from, S.size, sb, se); },
                       [&](uint64_t k) { return qsize_of(S.ovlp_begin + k); }, [&](uint64_t k) -> const cx::Aligned& { return tab[S.ovlp_begin + k]; }, &pass[s]);
        });
        uint64_t n_ov = 0, n_ops = 0;
        for (uint64_t s = 0; s < n_segs; ++s) {
            st.n_used += pass[s].n_used;
            for (uint64_t k : pass[s].order) { ++n_ov; n_ops += (((u64)got[entry[segs[s].ovlp_begin + k]].a.align_size + 3) / 4 + 7) & ~7ULL; }
        }
        necat_ctg_extend* r = (necat_ctg_extend*)calloc(1, sizeof(necat_ctg_extend));
        if (r) {
            *r = st;
            r->jobs = (necat_ctg_extend_result*)calloc(std::max<uint64_t>(1, n_jobs), sizeof(necat_ctg_extend_result));
            r->segments = (necat_ctg_segment*)calloc(std::max<uint64_t>(1, n_segs), sizeof(necat_ctg_segment));
            r->overlaps = (necat_ctg_overlap*)calloc(std::max<uint64_t>(1, n_ov), sizeof(necat_ctg_overlap));
            r->ops = (uint8_t*)calloc(std::max<uint64_t>(1, n_ops) + 8, 1);
        }
        if (!r || !r->jobs || !r->segments || !r->overlaps || !r->ops) { necat_ctg_extend_free(r); return nullptr; }
        r->n_jobs = n_jobs; r->n_segments = n_segs; r->n_overlaps = n_ov; r->n_ops = n_ops;
        for (uint64_t k = 0; k < n_jobs; ++k) r->jobs[k].overlap = -1;
        uint64_t ov = 0, at = 0;
        for (uint64_t s = 0; s < n_segs; ++s) {
            const necat_ctg_segment& S = segs[s];
            r->segments[s] = S;
            r->segments[s].ovlp_begin = ov;
            for (uint64_t k = S.ovlp_begin; k < S.ovlp_end; ++k) {
                necat_ctg_extend_result& J = r->jobs[k];
                J.state = pass[s].state[k - S.ovlp_begin];
                if (J.state == cx::kCapped || J.state == cx::kNoSeed) continue;
                const Got& g = got[entry[k]];
                J.decided = g.decided;
                if (!g.a.ok) continue;
                J.qoff = g.a.qoff; J.qend = g.a.qend; J.toff = g.a.toff; J.tend = g.a.tend; J.align_size = g.a.align_size; J.ident_perc = g.a.ident_perc;
            }
            for (uint64_t k : pass[s].order) {
                const uint64_t j = S.ovlp_begin + k;
                const Got& g = got[entry[j]];
                const u64 bytes = ((u64)g.a.align_size + 3) / 4;
                if (bytes) memcpy(r->ops + at, g.cols, bytes);
                r->overlaps[ov] = necat_ctg_overlap{jobs[j].qid, jobs[j].qdir, g.a.qoff, g.a.qend, g.a.toff, g.a.tend, g.a.align_size, 0, at};
                r->jobs[j].overlap = (int64_t)ov;
                r->cols_bytes_used += bytes;
                at += (bytes + 7) & ~7ULL; ++ov;
            }
            r->segments[s].ovlp_end = ov;
        }
        r->replay_ms = wall_ms() - t0;
        return r;
    }
};

}  // namespace

int necat_ctg_extend_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs, const necat_ctg_segment* segments, uint64_t n_segments,
                           const necat_ctg_extend_job* jobs, const necat_ctg_seed* seeds, const necat_ctg_extend_options* opt, necat_ctg_extend** out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || !opt || !out || (n_segments && !segments)) return NECAT_ERR_ARG;
    *out = nullptr;
    if (!contigs) return set_err(ctx, NECAT_ERR_ARG, "contig extension needs the contigs' volume: a segment is read where it lies");
    for (uint64_t s = 0; s < n_segments; ++s)
        if (segments[s].ovlp_begin < segments[s].ovlp_end && !jobs) return set_err(ctx, NECAT_ERR_ARG, "segment %lu has jobs, the call none", (unsigned long)s);
    const double w0 = wall_ms();
    CtgExtendCall call{ctx, reads, read_start_id, contigs, segments, n_segments, jobs, seeds, opt};
    int rc = call.validate();
    if (rc || (rc = call.seed()) || (rc = call.align()) || (rc = call.rescue_pair())) return rc;
    necat_ctg_extend* r = call.result();
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    if (knob().trace & 2)
        fprintf(stderr, "[necat] ctg extension %.2f ms: %lu segments, %lu jobs, %lu seeded and aligned, %lu reached by the loop, %lu overlaps; pair tried %lu, accepted %lu (local %lu device + %lu host, "
                "global %lu jobs, %lu device + %lu host); columns %lu bytes down, %lu used; seeds %.2f, aligner %.2f, pair %.2f, loop %.2f ms\n", wall_ms() - w0, (unsigned long)n_segments,
                (unsigned long)r->n_jobs, (unsigned long)r->n_aligned, (unsigned long)r->n_used, (unsigned long)r->n_overlaps, (unsigned long)r->n_pair_tried, (unsigned long)r->n_pair_accepted,
                (unsigned long)r->n_dalign_device, (unsigned long)r->n_dalign_host, (unsigned long)r->n_nw_jobs, (unsigned long)r->n_nw_device, (unsigned long)r->n_nw_host,
                (unsigned long)r->cols_bytes_downloaded, (unsigned long)r->cols_bytes_used, r->seed_ms, r->align_ms, r->rescue_ms, r->replay_ms);
    *out = r;
    return NECAT_OK;
}
