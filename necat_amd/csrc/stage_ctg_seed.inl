// stage_ctg_seed.inl - the seeding of contig polishing (ctg_cns/mem_finder.c, chain_dp.c: sampled 15-mers -> maximal exact matches -> chain -> can_list[0]) behind the
// C ABI: a table per segment and a wave per job on the device (ctg_seed_core.h, ctg_seed_kernels.h), or all of it on the library's host threads (ctg_seed.h), which is
// also what the device path hands the jobs it has no room for.  One of the stage files of libnecat_hip.so's single translation unit.

// ------------------------------------------------------------------------------------------ contig polishing: the seeding

void necat_ctg_seed_default_options(necat_ctg_seed_options* o)
{   // the path: DESIGN 6b's rule (the device's slowest run against the host's fastest, profiles/ctg_seed_bench.json)
    o->path = 0; o->host_threads = 0; o->keep_mems = 0; o->_pad = 0;
}

void necat_ctg_seed_free(necat_ctg_seed* r)
{
    if (!r) return;
    free(r->jobs); free(r->mems);
    free(r);
}

namespace {

namespace hsd = necat_host::ctg_seed;
namespace dsd = necat::ctg_seed;

enum CsBuf { CSB_TABLE, CSB_JOBS, CSB_POOL };
constexpr u64 kCsRunTabWords = 32ull << 20;       // u32 words of read tables (two per slot) a run of jobs may hold: 128 MB
static_assert(sizeof(dsd::DMem) == sizeof(necat_ctg_seed_mem) && sizeof(hsd::Mem) == sizeof(necat_ctg_seed_mem), "a match is three int32 everywhere");

// One call of necat_ctg_seed_batch: its arguments, what the steps hand on to each other, and the steps in the order the entry point takes them.
struct CtgSeedCall {
    necat_ctx* ctx; const necat_volume* reads; int read_start_id; const necat_volume* contigs; const necat_ctg_segment* segs; uint64_t n_segs;
    const necat_ctg_seed_job* jobs; const necat_ctg_seed_options* opt;
    unsigned threads = 1;
    uint64_t n_jobs = 0, n_fallback = 0;
    std::vector<necat_ctg_seed_result> res;
    std::vector<std::vector<hsd::Mem>> mems;      // keep_mems
    std::vector<u64> rwords, cwords;              // the volumes' words on the host: path 1, and path 0 once a job falls back
    bool have_words = false;
    std::atomic<uint64_t> shared_start{~0ULL};
    double index_ms = 0, match_ms = 0, chain_ms = 0, device_ms = 0, host_ms = 0;

    uint64_t read_of(uint64_t k) const { return (uint64_t)((int64_t)jobs[k].qid - read_start_id); }
    int qsize_of(uint64_t k) const { const uint64_t q = read_of(k); return (int)(reads->h_seq_off[q + 1] - reads->h_seq_off[q]); }
    u64 seg_base(const necat_ctg_segment& S) const { return contigs->h_seq_off[S.ctg_id] + (u64)S.from; }

    // the options, the segments and every job: nothing below checks again
    int validate()
    {
        if ((opt->path != 0 && opt->path != 1) || opt->host_threads < 0) return set_err(ctx, NECAT_ERR_ARG, "contig seeding options out of range (path 0 or 1, host_threads >= 0)");
        threads = call_threads(ctx, opt->host_threads);
        for (uint64_t s = 0; s < n_segs; ++s) {
            const necat_ctg_segment& S = segs[s];
            if (int rc = ctg_segment_check(ctx, contigs, S, s, hsd::kK, "job")) return rc;
            n_jobs = std::max<uint64_t>(n_jobs, S.ovlp_end);
            for (uint64_t k = S.ovlp_begin; k < S.ovlp_end; ++k) {
                SeqAt q;
                if (!seq_at(reads, jobs[k].qid, read_start_id, &q)) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu) names no read of the volume", (unsigned long)k, (unsigned long)s);
                if (q.len >= (u64)hsd::kMaxRead) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu): a read of 2^30 bases or more", (unsigned long)k, (unsigned long)s);
                if (jobs[k].qdir != 0 && jobs[k].qdir != 1) return set_err(ctx, NECAT_ERR_ARG, "job %lu (segment %lu) has a strand that is neither 0 nor 1", (unsigned long)k, (unsigned long)s);
            }
        }
        necat_ctg_seed_result zero;
        memset(&zero, 0, sizeof zero);
        res.assign(n_jobs, zero);
        if (opt->keep_mems) mems.assign(n_jobs, std::vector<hsd::Mem>());
        return NECAT_OK;
    }

    int need_words()
    {
        if (have_words) return NECAT_OK;
        int rc = fetch_words(ctx, reads, &rwords);
        if (rc || (rc = fetch_words(ctx, contigs, &cwords))) return rc;
        have_words = true;
        return NECAT_OK;
    }

    // jobs `list` of segment S through the host form on the call's threads; false: two surviving matches of a job share a start
    bool host_jobs(const necat_ctg_segment& S, const std::vector<uint64_t>& list)
    {
        hsd::SegIndex ix;
        ix.build(cwords.data(), seg_base(S), S.size);
        necat_host::deal(list.size(), (unsigned)std::min<size_t>(threads, std::max<size_t>(1, list.size())), 1, [&](uint64_t x, unsigned) {
            const uint64_t k = list[x];
            std::vector<uint8_t> r;
            hsd::decode(rwords.data(), reads->h_seq_off[read_of(k)], qsize_of(k), jobs[k].qdir, r);
            hsd::JobOut o;
            if (!hsd::seed_job(ix, r.data(), qsize_of(k), o)) { uint64_t cur = shared_start.load(); while (k < cur && !shared_start.compare_exchange_weak(cur, k)) {} }
            necat_ctg_seed_result& R = res[k];
            R.found = o.can.found; R.qbeg = o.can.qbeg; R.qend = o.can.qend; R.sbeg = o.can.sbeg; R.send = o.can.send; R.qoff = o.can.qoff; R.soff = o.can.soff; R.score = o.can.score;
            R.n_matches = o.n_matches; R.n_mems = (uint32_t)o.mems.size(); R.chain_len = o.can.chain_len; R.how = 2;
            if (opt->keep_mems) mems[k].swap(o.mems);
        });
        return shared_start.load() == ~0ULL;
    }
    int host_segment(uint64_t s, const std::vector<uint64_t>& list)
    {
        if (list.empty()) return NECAT_OK;
        const double h0 = wall_ms();
        int rc = need_words();
        if (rc) return rc;
        if (!host_jobs(segs[s], list))
            return set_err(ctx, NECAT_ERR_INTERNAL, "job %lu (segment %lu): two maximal exact matches share a start, the reference's unstable sort decides their order", (unsigned long)shared_start.load(), (unsigned long)s);
        host_ms += wall_ms() - h0;
        return NECAT_OK;
    }

    // path 0, one segment: its table, then its jobs run by run (what the read tables may hold), each run chunk by chunk (what the pool may hold)
    int device_segment(uint64_t s, const CallEvents<2>& ev)
    {
        const necat_ctg_segment& S = segs[s];
        hipStream_t st = ctx->stream;
        const double d0 = wall_ms();
        const dsd::Seq seg = {(const u64*)contigs->bases, (i64)seg_base(S), S.size, 0};
        const u32 ne = (u32)dsd::n_entries(S.size, 1);
        u32 cap = 64; while (cap < 2 * ne) cap <<= 1;
        int rc = buf_ensure(ctx, ctx->ctg_seed_buf[CSB_TABLE], ((size_t)2 * cap + ne) * 4);
        if (rc) return rc;
        u32* const d_keys = as<u32>(ctx->ctg_seed_buf[CSB_TABLE]);
        dsd::SegDev T; T.keys = d_keys; T.head = d_keys + cap; T.next = d_keys + 2 * (size_t)cap; T.cap = cap;
        NECAT_HIP(ctx, hipMemsetAsync(d_keys, 0, (size_t)2 * cap * 4, st));
        NECAT_HIP(ctx, ev.record(0, st));
        hipLaunchKernelGGL(dsd::k_ctgs_index, dim3(grid_for(ne, 256, 1u << 16)), dim3(256), 0, st, seg, cap, d_keys, d_keys + cap, d_keys + 2 * (size_t)cap);
        NECAT_CHECK_LAUNCH(ctx, "k_ctgs_index");
        NECAT_HIP(ctx, ev.record(1, st));
        NECAT_HIP(ctx, hipStreamSynchronize(st));
        index_ms += ev.ms(0);
        const u64 budget = knob().ctg_seed_budget, job_max = std::min<u64>(budget, knob().ctg_seed_job_max);      // (a job's two rank sorts are quadratic in its seeds)
        const u32 lds_cap = knob().ctg_seed_lds;
        std::vector<uint64_t> fallback;
        for (uint64_t k0 = S.ovlp_begin; k0 < S.ovlp_end;) {
            // ---- a run of jobs: tables of their own, counted in one launch
            std::vector<dsd::JobDev> jd;
            std::vector<uint64_t> jk;
            u64 tab_words = 0;
            uint64_t k = k0;
            for (; k < S.ovlp_end; ++k) {
                const u32 ns = (u32)dsd::n_entries(qsize_of(k), hsd::kReadWindow);
                u32 qcap = 64; while (qcap < 2 * ns) qcap <<= 1;
                if (2 * (u64)qcap > kCsRunTabWords) { fallback.push_back(k); continue; }
                if (tab_words + 2 * (u64)qcap > kCsRunTabWords) break;
                dsd::JobDev J; J.read_g0 = (i64)reads->h_seq_off[read_of(k)]; J.qlen = qsize_of(k); J.qrev = jobs[k].qdir; J.qtab_off = tab_words; J.qcap = qcap; J.n_matches = 0; J.seed_off = 0;
                tab_words += 2 * (u64)qcap;
                jd.push_back(J); jk.push_back(k);
            }
            k0 = k;
            const u32 R = (u32)jd.size();
            if (!R) continue;
            const CtgSeedRunArena a(R, tab_words);
            if ((rc = buf_ensure(ctx, ctx->ctg_seed_buf[CSB_JOBS], a.lay.bytes()))) return rc;
            const ArenaView A(ctx->ctg_seed_buf[CSB_JOBS], a.lay, st);
            NECAT_HIP(ctx, A.zero_from(a.out));          // outputs, selection, the error counts, the tables
            NECAT_HIP(ctx, A.upload(a.jobs, jd.data(), R));
            NECAT_HIP(ctx, ev.record(0, st));
            hipLaunchKernelGGL(dsd::k_ctgs_count, dim3(R), dim3(64), 0, st, (const u64*)reads->bases, T, A.ptr(a.jobs), R, A.ptr(a.tab));
            NECAT_CHECK_LAUNCH(ctx, "k_ctgs_count");
            NECAT_HIP(ctx, ev.record(1, st));
            NECAT_HIP(ctx, A.download(jd.data(), a.jobs, R));
            NECAT_HIP(ctx, hipStreamSynchronize(st));
            match_ms += ev.ms(0);
            std::vector<dsd::DCan> out(R);
            std::vector<dsd::DMem> hm;
            for (u32 j0 = 0; j0 < R;) {
                // ---- a chunk of the run: the jobs whose seeds the pool holds together
                std::vector<u32> sel;
                u64 total = 0;
                u32 j = j0;
                for (; j < R; ++j) {
                    res[jk[j]].n_matches = jd[j].n_matches;
                    if (jd[j].n_matches == 0) continue;                                    // no seed: no match, no chain - the zeroed output stands
                    if ((u64)jd[j].n_matches > job_max) { fallback.push_back(jk[j]); continue; }
                    if (total + jd[j].n_matches > budget) break;
                    jd[j].seed_off = total; total += jd[j].n_matches;
                    sel.push_back(j);
                }
                j0 = j;
                if (sel.empty()) continue;
                const CtgSeedPoolArena p(total);
                if ((rc = buf_ensure(ctx, ctx->ctg_seed_buf[CSB_POOL], p.lay.bytes()))) return rc;
                const ArenaView P(ctx->ctg_seed_buf[CSB_POOL], p.lay, st);
                const u32 n_sel = (u32)sel.size();
                NECAT_HIP(ctx, A.upload(a.jobs, jd.data(), R));
                NECAT_HIP(ctx, A.upload(a.sel, sel.data(), n_sel));
                NECAT_HIP(ctx, ev.record(0, st));
                hipLaunchKernelGGL(dsd::k_ctgs_mems, dim3(n_sel), dim3(64), 0, st, (const u64*)reads->bases, seg, T, A.cptr(a.jobs), A.cptr(a.sel), n_sel, A.cptr(a.tab),
                                   P.ptr(p.tmp), P.ptr(p.seeds), P.ptr(p.tmp_mems), P.ptr(p.mems), A.ptr(a.out), A.ptr(a.bad));
                NECAT_CHECK_LAUNCH(ctx, "k_ctgs_mems");
                NECAT_HIP(ctx, ev.record(1, st));
                NECAT_HIP(ctx, hipStreamSynchronize(st));
                match_ms += ev.ms(0);
                NECAT_HIP(ctx, ev.record(0, st));
                hipLaunchKernelGGL(dsd::k_ctgs_chain, dim3(n_sel), dim3(64), (size_t)lds_cap * (sizeof(dsd::DMem) + 4 * sizeof(i32)), st, A.cptr(a.jobs), A.cptr(a.sel), n_sel,
                                   P.cptr(p.mems), P.ptr(p.chain), lds_cap, A.ptr(a.out));
                NECAT_CHECK_LAUNCH(ctx, "k_ctgs_chain");
                NECAT_HIP(ctx, ev.record(1, st));
                u32 bad[2] = {0, 0};          // jobs whose seeds were not the counted ones; pairs of surviving matches that share a start
                NECAT_HIP(ctx, A.download(bad, a.bad, 2));
                NECAT_HIP(ctx, A.download(out.data(), a.out, R));
                if (opt->keep_mems) { hm.resize(total); NECAT_HIP(ctx, P.download(hm.data(), p.mems, total)); }
                NECAT_HIP(ctx, hipStreamSynchronize(st));
                chain_ms += ev.ms(0);
                if (bad[0]) return set_err(ctx, NECAT_ERR_INTERNAL, "segment %lu: %u jobs gave other seeds than were counted for them", (unsigned long)s, bad[0]);
                if (bad[1]) return set_err(ctx, NECAT_ERR_INTERNAL, "segment %lu: two maximal exact matches of a job share a start, the reference's unstable sort decides their order", (unsigned long)s);
                for (u32 x : sel) {
                    const dsd::DCan& c = out[x];
                    if (c.n_mems < 0 || (u32)c.n_mems > jd[x].n_matches) return set_err(ctx, NECAT_ERR_INTERNAL, "segment %lu, job %lu: %d matches of %u seeds", (unsigned long)s, (unsigned long)jk[x], c.n_mems, jd[x].n_matches);
                    necat_ctg_seed_result& Q = res[jk[x]];
                    Q.found = c.found; Q.qbeg = c.qbeg; Q.qend = c.qend; Q.sbeg = c.sbeg; Q.send = c.send; Q.qoff = c.qoff; Q.soff = c.soff; Q.score = c.score;
                    Q.n_mems = (uint32_t)c.n_mems; Q.chain_len = c.chain_len; Q.how = c.tier;
                    if (opt->keep_mems && c.n_mems) { mems[jk[x]].resize((size_t)c.n_mems); memcpy(mems[jk[x]].data(), hm.data() + jd[x].seed_off, (size_t)c.n_mems * sizeof(dsd::DMem)); }
                }
                if (knob().trace & 2) fprintf(stderr, "[necat] ctg seeding: segment %lu, a chunk of %u jobs, %lu seeds\n", (unsigned long)s, n_sel, (unsigned long)total);
            }
        }
        device_ms += wall_ms() - d0;
        n_fallback += fallback.size();
        return host_segment(s, fallback);
    }

    // everything in two arrays the result owns; nullptr: out of memory
    necat_ctg_seed* result() const
    {
        uint64_t nm = 0;
        if (opt->keep_mems) for (uint64_t k = 0; k < n_jobs; ++k) nm += mems[k].size();
        necat_ctg_seed* r = (necat_ctg_seed*)calloc(1, sizeof(necat_ctg_seed));
        if (r) { r->jobs = (necat_ctg_seed_result*)calloc(std::max<uint64_t>(1, n_jobs), sizeof(necat_ctg_seed_result)); r->mems = (necat_ctg_seed_mem*)malloc(std::max<uint64_t>(1, nm) * sizeof(necat_ctg_seed_mem)); }
        if (!r || !r->jobs || !r->mems) { necat_ctg_seed_free(r); return nullptr; }
        uint64_t at = 0;
        for (uint64_t k = 0; k < n_jobs; ++k) {
            r->jobs[k] = res[k];
            r->jobs[k].mems_off = at;
            if (opt->keep_mems && !mems[k].empty()) { memcpy(r->mems + at, mems[k].data(), mems[k].size() * sizeof(necat_ctg_seed_mem)); at += mems[k].size(); }
            r->max_matches = std::max(r->max_matches, res[k].n_matches); r->max_mems = std::max(r->max_mems, res[k].n_mems);
        }
        r->n_jobs = n_jobs; r->n_mems = nm; r->n_fallback = n_fallback;
        if (opt->path == 0) for (uint64_t s = 0; s < n_segs; ++s) for (uint64_t k = segs[s].ovlp_begin; k < segs[s].ovlp_end; ++k) { r->n_lds += res[k].how == 0; r->n_scratch += res[k].how == 1; }
        r->index_ms = index_ms; r->match_ms = match_ms; r->chain_ms = chain_ms; r->device_ms = device_ms; r->host_ms = host_ms;
        return r;
    }
};

}  // namespace

int necat_ctg_seed_batch(necat_ctx* ctx, const necat_volume* reads, int read_start_id, const necat_volume* contigs, const necat_ctg_segment* segments, uint64_t n_segments,
                         const necat_ctg_seed_job* jobs, const necat_ctg_seed_options* opt, necat_ctg_seed** out)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !reads || !opt || !out || (n_segments && !segments)) return NECAT_ERR_ARG;
    *out = nullptr;
    if (!contigs) return set_err(ctx, NECAT_ERR_ARG, "contig seeding needs the contigs' volume: a segment is read where it lies");
    for (uint64_t s = 0; s < n_segments; ++s)
        if (segments[s].ovlp_begin < segments[s].ovlp_end && !jobs) return set_err(ctx, NECAT_ERR_ARG, "segment %lu has jobs, the call none", (unsigned long)s);
    CtgSeedCall call{ctx, reads, read_start_id, contigs, segments, n_segments, jobs, opt};
    const double w0 = wall_ms();
    int rc = call.validate();
    if (rc) return rc;
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    if (opt->path == 1) {
        for (uint64_t s = 0; s < n_segments; ++s) {
            std::vector<uint64_t> list;
            for (uint64_t k = segments[s].ovlp_begin; k < segments[s].ovlp_end; ++k) list.push_back(k);
            if ((rc = call.host_segment(s, list))) return rc;
        }
    } else {
        CallEvents<2> ev;
        if ((rc = ev.create(ctx))) return rc;
        for (uint64_t s = 0; s < n_segments; ++s) if ((rc = call.device_segment(s, ev))) return rc;
    }
    necat_ctg_seed* r = call.result();
    if (!r) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    if (knob().trace & 2) fprintf(stderr, "[necat] ctg seeding %.2f ms: %lu segments, %lu jobs (%lu in LDS, %lu in scratch, %lu on the host), kernels: index %.2f, matches %.2f, chains %.2f ms; device %.2f ms, host %.2f ms\n",
                             wall_ms() - w0, (unsigned long)n_segments, (unsigned long)r->n_jobs, (unsigned long)r->n_lds, (unsigned long)r->n_scratch, (unsigned long)r->n_fallback, r->index_ms, r->match_ms,
                             r->chain_ms, r->device_ms, r->host_ms);
    *out = r;
    return NECAT_OK;
}
