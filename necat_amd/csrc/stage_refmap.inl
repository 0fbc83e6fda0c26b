// stage_refmap.inl - reads against a reference (oc2rm_worker).
// One of the stage files of libnecat_hip.so's single translation unit: necat_hip.hip includes them in order, inside its extern "C" block, after the
// context / knob / result-pool code they all use (the kernels are header templates and the stages share host helpers: one device code object, one 30 s build).

// ------------------------------------------------------------------------------------------ reads against a reference (oc2rm_worker)

extern "C++" {
namespace {

// The rescue pair ahead of the walk (NECAT_RM_RESCUE_DEVICE=1): for every candidate of `need` (ok && rm::needs_rescue, candidate order) the device pair (pair_local,
// pair_global) on the read on its strand against the candidate's STRETCH of the reference, the slice [from, to) of the resident volume that rescue::Dalign sees decoded
// on the host.  table[i] for candidate i, in rm::Rescue's convention: subject coordinates relative to `from`.  A read of 2^30 bases or more, a reference sequence of
// 2^31 or more, or (nw_run) a range of 2^26 or more give NECAT_ERR_ARG - never a quiet switch to the host code; with the knob at 0 such a call runs as before.
int rm_speculate(necat_ctx* ctx, const necat_volume* ref, const necat_volume* reads, int read_start_id, int ref_start_id, const RmOut& ro, const std::vector<uint64_t>& need,
                 const necat_map_options& o, std::vector<rm::Rescue>& table, necat_rm_stats* st)
{
    const uint64_t n = need.size();
    if (n >= (1ULL << 30)) return set_err(ctx, NECAT_ERR_ARG, "map_reference: 2^30 rescue jobs or more in one call (NECAT_RM_RESCUE_DEVICE=1)");
    std::vector<pair::Job> jobs(n);
    for (uint64_t k = 0; k < n; ++k) {
        const necat_candidate& c = ro.cands[need[k]];
        const int64_t q = (int64_t)c.qid - read_start_id, s = (int64_t)c.sid - ref_start_id;
        if (q < 0 || (uint64_t)q >= reads->nseq || s < 0 || (uint64_t)s >= ref->nseq || (c.qdir != 0 && c.qdir != 1))
            return set_err(ctx, NECAT_ERR_INTERNAL, "map_reference: candidate %lu names a sequence outside its volume", (unsigned long)need[k]);
        const u64 qb = reads->h_seq_off[q], qs = reads->h_seq_off[q + 1] - qb, sb = ref->h_seq_off[s], ss = ref->h_seq_off[s + 1] - sb;
        if (c.qsize != qs || c.ssize != ss || c.qoff > qs || c.soff > ss)
            return set_err(ctx, NECAT_ERR_INTERNAL, "map_reference: candidate %lu does not fit its sequences", (unsigned long)need[k]);
        if (qs >= (1ULL << 30) || ss >= (1ULL << 31))
            return set_err(ctx, NECAT_ERR_ARG, "map_reference: candidate %lu: a read of 2^30 bases or more, or a reference sequence of 2^31 or more (NECAT_RM_RESCUE_DEVICE=1)", (unsigned long)need[k]);
        i64 from, to, woff;
        rm_window((i64)c.qoff, (i64)qs, (i64)c.soff, (i64)ss, &from, &to, &woff);          // 0 <= from <= soff <= to <= ss: the slice lies inside sequence s
        jobs[k] = pair::Job{c.qid, c.qdir, c.sid, (i64)qb, (i64)qs, (i64)sb, from, to - from, (i64)c.qoff, woff};
        table[need[k]] = rm::Rescue{1, 0, 0, 0, 0, 0, 0.0};
    }
    std::vector<necat_dalign_result> ranges(n);
    PairLocal L;
    int rc = pair_local(ctx, ref, reads, jobs, o.error, o.align_size_cutoff, ranges.data(), &L);
    if (rc) return rc;
    st->dalign_ms = L.ms;          // (as dal_run's device_ms: without the host code's share)
    st->n_dalign_device = L.sv.n_tier[0]; st->n_dalign_host = L.sv.n_host; st->n_dalign_over_cap = L.sv.n_over_cap; st->n_dalign_selfcheck = L.sv.n_selfcheck;
    st->max_diags = L.sv.max_diags;
    PairGlobal G;          // (no columns: oc2rm_worker writes none)
    if ((rc = pair_global(ctx, ref, reads, read_start_id, ref_start_id, jobs, ranges.data(), o.error, o.align_size_cutoff, false, &G))) return rc;
    st->n_nw_jobs = G.job_of.size(); st->nw_ms = G.ns.device_ms;
    st->n_nw_device = G.ns.n_device; st->n_nw_host = G.ns.n_host;
    if (L.sv.n_host || G.ns.n_host) st->words_fetched = 1;
    for (size_t x = 0; x < G.res.size(); ++x) {
        const necat_nw_result& r = G.res[x];          // on the stretch, which is where the walk adds `from`
        if (r.ok) table[need[G.job_of[x]]] = rm::Rescue{1, 1, r.qoff, r.qend, r.toff, r.tend, r.ident_perc};
    }
    return NECAT_OK;
}

}  // namespace
}  // extern "C++"

int necat_map_reference(necat_ctx* ctx, const necat_index* ix, const necat_volume* ref, const necat_volume* reads,
                        int read_start_id, int ref_start_id, const necat_map_options* opt,
                        necat_m4** out, uint64_t* n_out, uint64_t* n_candidates, uint64_t* n_rescued)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !ix || !ref || !reads || !opt || !out || !n_out) return NECAT_ERR_ARG;
    *out = nullptr; *n_out = 0;
    if (n_candidates) *n_candidates = 0;
    if (n_rescued) *n_rescued = 0;
    necat_rm_stats st;
    memset(&st, 0, sizeof st);
    ctx->rm_stats = st;
    necat_map_options o = *opt;
    o.job = 1;                                   // rm_worker.c:251-252: sorted, cut to num_candidates
    DevCands dev;
    int rc = find_impl(ctx, ix, ref, reads, read_start_id, ref_start_id, 0 /* pairwise = FALSE, rm_worker.c:231 */, &o, nullptr, nullptr, &dev);
    if (rc) return rc;
    if (n_candidates) *n_candidates = dev.n;
    st.n_candidates = dev.n;
    if (dev.n == 0) { ctx->rm_stats = st; *out = (necat_m4*)result_alloc(sizeof(necat_m4)); return *out ? NECAT_OK : set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed"); }
    RmOut ro;
    necat_m4* unused = nullptr; uint64_t unused_n = 0;
    if ((rc = extend_impl(ctx, ref, reads, read_start_id, ref_start_id, nullptr, dev.n, &o, 1 /* ONC_TAIL_MATCH_LEN_SHORT, rm_worker.c:92 */,
                          &unused, &unused_n, nullptr, &dev, nullptr, &ro))) return rc;
    const double w0 = wall_ms();
    const uint64_t ng = ro.group_off.empty() ? 0 : ro.group_off.size() - 1;
    // the candidates that can need the rescue pair; the walk reaches those no earlier record of their read contains
    std::vector<uint64_t> need;
    for (uint64_t i = 0; i < dev.n; ++i) if (ro.ok[i] && rm::needs_rescue(ro.cands[i], ro.m4[i])) need.push_back(i);
    st.n_need = need.size();
    // the pair ahead of the walk on the device, its answers in a table - or inside the walk on the host threads
    std::vector<rm::Rescue> table;
    const bool spec = knob().rm_rescue_device && !need.empty();
    if (spec) {
        table.assign(dev.n, rm::Rescue{0, 0, 0, 0, 0, 0, 0.0});
        if ((rc = rm_speculate(ctx, ref, reads, read_start_id, ref_start_id, ro, need, o, table, &st))) return rc;
    }
    // otherwise the bases come back to the host, and only if some candidate needs the pair
    std::vector<u64> w_reads, w_ref;
    if (!spec && !need.empty()) {
        if ((rc = fetch_words(ctx, reads, &w_reads)) || (rc = fetch_words(ctx, ref, &w_ref))) return rc;
        st.words_fetched = 1;
    }
    const necat_host::BaseWords hr = host_view(reads, w_reads), hf = host_view(ref, w_ref);
    const rescue::DalignSpec dspec = rescue::spec_for_error(o.error);
    // groups (reads) are dealt out in runs of 16; every run's records are kept apart and joined in read order
    const double r0 = wall_ms();
    const uint64_t run = 16, nruns = (ng + run - 1) / run;
    std::vector<std::vector<necat_m4>> parts(nruns);
    std::atomic<uint64_t> tried(0), rescued(0), missing(0);
    necat_host::Deal runs(nruns);
    const unsigned nt = (unsigned)std::min<uint64_t>(std::min(necat_host::hardware_threads(), 32u), std::max<uint64_t>(1, nruns));
    necat_host::on_threads(nt, [&](unsigned) {
        // the provider in use, on every read of the thread's runs
        auto replay_runs = [&](auto& wk, auto&& replay) {
            runs.run([&](uint64_t r) { for (uint64_t g = r * run; g < std::min(ng, (r + 1) * run); ++g) replay(ro.group_off[g], ro.group_off[g + 1], parts[r]); });
            tried += wk.n_rescue_tried; rescued += wk.n_rescued; missing += wk.n_missing;
        };
        if (spec) {
            rm::TableWorker tw(table.data());
            replay_runs(tw, [&](uint64_t lo, uint64_t hi, std::vector<necat_m4>& acc) { tw.replay(ro.cands.data(), ro.m4.data(), ro.ok.data(), lo, hi, acc); });
        } else {
            rm::Worker wk(dspec, o.error);
            replay_runs(wk, [&](uint64_t lo, uint64_t hi, std::vector<necat_m4>& acc) {
                wk.replay(ro.cands.data(), ro.m4.data(), ro.ok.data(), lo, hi, hr, hf, read_start_id, ref_start_id, o.align_size_cutoff, acc);
            });
        }
    });
    st.replay_ms = wall_ms() - r0;
    st.n_tried = tried.load(); st.n_rescued = rescued.load();
    ctx->rm_stats = st;
    if (missing.load()) return set_err(ctx, NECAT_ERR_INTERNAL, "map_reference: the walk asked for %lu rescue pairs the table does not hold", (unsigned long)missing.load());
    uint64_t total = 0;
    for (auto& p : parts) total += p.size();
    necat_m4* res = (necat_m4*)result_alloc(std::max<uint64_t>(1, total) * sizeof(necat_m4));
    if (!res) return set_err(ctx, NECAT_ERR_MEMORY, "host malloc failed");
    uint64_t at = 0;
    for (auto& p : parts) { if (!p.empty()) memcpy(res + at, p.data(), p.size() * sizeof(necat_m4)); at += p.size(); }
    if (n_rescued) *n_rescued = rescued.load();
    if (knob().trace & 2)
        fprintf(stderr, "[necat] map_reference host: %.2f ms, %lu candidates, %lu rescue attempts, %lu rescued, %lu records; %lu need the pair, %s: local %lu device + %lu host "
                "(%lu above the cap, %lu flagged; widest window %u) %.2f ms, global %lu jobs, %lu device + %lu host, %.2f ms; words %s; walk %.2f ms\n", wall_ms() - w0,
                (unsigned long)dev.n, (unsigned long)st.n_tried, (unsigned long)st.n_rescued, (unsigned long)total, (unsigned long)st.n_need,
                spec ? "computed ahead on the device" : "computed inside the walk", (unsigned long)st.n_dalign_device, (unsigned long)st.n_dalign_host,
                (unsigned long)st.n_dalign_over_cap, (unsigned long)st.n_dalign_selfcheck, st.max_diags, st.dalign_ms, (unsigned long)st.n_nw_jobs,
                (unsigned long)st.n_nw_device, (unsigned long)st.n_nw_host, st.nw_ms, st.words_fetched ? "fetched" : "not fetched", st.replay_ms);
    *out = res; *n_out = total;
    return NECAT_OK;
}
