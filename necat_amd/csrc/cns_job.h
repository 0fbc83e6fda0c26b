// cns_job.h - one oc2cns job (consensus/main.c:51-78 over consensus_one_partition.c:110): the candidate partitions of a project through the extension loop on
// the device and the consensus proper, records to cns_out / raw_out.  Host code only, no HIP: tests/host_core/check_cns_job.cpp compiles this header against a
// fake library on the CPU.
// The job is a sequence of UNITS in two stages one unit apart: CnsUnitSource makes a unit on the first context (read the partition, gather its reads, load, extension
// loop), CnsHandoff runs the source on a thread of its own one finished unit ahead, CnsConsumer does the consensus proper of the unit on the second context and writes
// its records - 88 % of a partition's time is host work, the device loop of the next unit hides behind it.  consensus_one_partition.c runs the two one
// after the other; the files come out the same.
// The read set (CnsReadSet): one volume while the directory holds fewer than 2^32 bases (a volume's limit).  From there on, or with NECAT_CNS_READS=gather, every
// volume file stays a resident volume of its own and a partition is worked in chunks of whole templates (cns_chunks.h, NECAT_CNS_CHUNK_BASES): the reads a chunk's
// candidates name are gathered on the device into one compact volume (necat_volume_gather), the entries run on it with the records' ids rewritten, and the ids are
// mapped back when the records are written.  A merged partition is the same unit with an empty id map on the resident volume.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>

#include "host_io.h"
#include "host_threads.h"
#include "host_bases.h"
#include "cns_chunks.h"
#include "cns_consensus.h"

namespace necat_host {

struct CnsError { std::string what, detail; };

// all volumes of a project as one read set with global ids (merge_volumes, common/makedb_aux.c:137-153), on the host and on the device.  merged: the bases at one
// byte each, one device volume.  gather: the volume files' pac bytes as they are, a read's bases decoded when a record needs them; one device volume per file.
struct CnsReadSet {
    std::vector<uint64_t> size;
    std::vector<std::string> names;
    std::vector<int64_t> vol_start;        // the global id of each volume file's first read
    bool gathered = false;
    necat_volume* merged = nullptr;        // merged: the read set on the device
    std::vector<necat_volume*> file_vols;  // gather: the volume files, resident as oc2mkdb wrote them

    CnsReadSet() = default;
    CnsReadSet(const CnsReadSet&) = delete; CnsReadSet& operator=(const CnsReadSet&) = delete;
    ~CnsReadSet() { release(); }
    void release()                         // the device volumes (an owner that destroys their context itself calls this first)
    {
        if (merged) necat_volume_free(ctx_, merged);
        for (necat_volume* v : file_vols) necat_volume_free(ctx_, v);
        merged = nullptr; file_vols.clear();
    }
    // mode: merged - the whole directory as one volume, which holds fewer than 2^32 bases; gather - one resident volume per file; auto - merged while the
    // directory's total allows it
    bool load(const VolumesInfo& vi, const std::string& mode, CnsError* e)
    {
        if (mode != "merged" && mode != "gather" && mode != "auto") { *e = {"NECAT_CNS_READS", "merged, gather or auto"}; return false; }
        log_line("", "load reads");
        const double t0 = now_sec();
        uint64_t total = 0;
        vols_.resize((size_t)vi.num_volumes);
        for (int v = 0; v < vi.num_volumes; ++v) {
            if (!load_volume(vi.names[v].c_str(), &vols_[v], &e->detail)) { e->what = "volume"; return false; }
            total += vols_[v].nbases;
        }
        gathered = mode == "gather" || (mode == "auto" && total >= cns_chunks::kMaxChunkBases);
        if (!gathered) codes_.resize(total);
        uint64_t at = 0;
        for (const HostVolume& hv : vols_) {
            vol_start.push_back((int64_t)size.size());
            for (uint64_t i = 0; i < hv.offset.size(); ++i) { offset_.push_back(at + hv.offset[i]); size.push_back(hv.size[i]); names.emplace_back(hv.name(i)); }
            if (!gathered) decode_pac(hv.pac.data(), 0, hv.nbases, codes_.data() + at);
            at += hv.nbases;
        }
        if (!gathered) { vols_.clear(); vols_.shrink_to_fit(); }
        log_line("[%s] INFO: '%s' takes %.2lf secs.\n", "load reads", now_sec() - t0);
        return true;
    }
    // the device volumes, made through (and later freed through) `ctx`
    bool upload(necat_ctx* ctx, CnsError* e)
    {
        ctx_ = ctx;
        auto failed = [&]() { *e = {"necat_volume_upload", necat_last_error(ctx)}; return false; };
        if (!gathered) {
            // NECAT pac of the merged set (first base of a byte in its top two bits)
            std::vector<uint8_t> pac((codes_.size() + 3) / 4 + 8, 0);
            for (uint64_t i = 0; i < codes_.size(); ++i) pac[i >> 2] |= (uint8_t)(codes_[i] << ((~i & 3) << 1));
            if (necat_volume_upload(ctx, pac.data(), codes_.size(), offset_.data(), size.data(), size.size(), &merged)) return failed();
        } else {
            for (const HostVolume& hv : vols_) {
                necat_volume* dv = nullptr;
                if (necat_volume_upload(ctx, hv.pac.data(), hv.nbases, hv.offset.data(), hv.size.data(), hv.offset.size(), &dv)) return failed();
                file_vols.push_back(dv);
            }
        }
        return true;
    }
    // the bases of read `id`: in place (merged), or decoded into buf
    const uint8_t* read(uint64_t id, std::vector<uint8_t>& buf) const
    {
        if (!gathered) return codes_.data() + offset_[id];
        const size_t v = (size_t)(std::upper_bound(vol_start.begin(), vol_start.end(), (int64_t)id) - vol_start.begin()) - 1;
        const HostVolume& hv = vols_[v];
        const uint64_t k = id - (uint64_t)vol_start[v];
        buf.resize(hv.size[k]);
        decode_pac(hv.pac.data(), hv.offset[k], hv.size[k], buf.data());
        return buf.data();
    }

private:
    std::vector<uint8_t> codes_;           // merged: one byte per base (0..3)
    std::vector<uint64_t> offset_;
    std::vector<HostVolume> vols_;         // gather: the volume files (merged: released after the load)
    necat_ctx* ctx_ = nullptr;
};

// one unit of the job's two stages: a partition (merged: empty id map, the resident volume, first == last), or a chunk of a partition's templates on the volume
// gathered for it.  Move-only; what it still holds when it goes is released through `owner`, the context of the thread that holds it.
struct CnsUnitFields {
    bool done = false;                       // no more units
    int pid = -1; bool first = true, last = true, empty = false; int rc = 0; std::string what, detail;
    necat_candidate* cands = nullptr; uint64_t* tmpl_off = nullptr; uint64_t* n_all = nullptr; uint64_t nt = 0;
    necat_cns_result* res = nullptr; double t_gpu = 0, t0 = 0;
    necat_volume* vol = nullptr; bool own_vol = false;      // the volume its ids refer to: the resident one, or its own gathered one
    necat_ctx* owner = nullptr;
    std::vector<int64_t> ids;                // gather: local id -> global id
    uint64_t n_chunks = 0, gathered_bases = 0; double gather_ms = 0, gather_kernel_ms = 0;
};
struct CnsUnit : CnsUnitFields {
    CnsUnit() = default;
    CnsUnit(CnsUnit&& o) noexcept : CnsUnitFields(std::move(o)) { static_cast<CnsUnitFields&>(o) = CnsUnitFields(); }
    CnsUnit& operator=(CnsUnit&& o) noexcept
    {
        if (this != &o) { release(owner); static_cast<CnsUnitFields&>(*this) = std::move(o); static_cast<CnsUnitFields&>(o) = CnsUnitFields(); }
        return *this;
    }
    ~CnsUnit() { release(owner); }
    int global_id(int local) const { return ids.empty() ? local : (int)ids[(size_t)local]; }
    void release(necat_ctx* c)
    {
        necat_cns_result_free(res);
        necat_free(cands); necat_free(tmpl_off); necat_free(n_all);
        if (own_vol) necat_volume_free(c, vol);
        res = nullptr; cands = nullptr; tmpl_off = nullptr; n_all = nullptr; vol = nullptr; own_vol = false;
    }
};

// the units of the partitions pids[0], pids[1], ... in order, each through its device stage on `ctx`: a state machine over (partition, chunk)
struct CnsUnitSource {
    necat_ctx* ctx; const CnsReadSet& rs; std::string can_path; std::vector<int> pids; uint64_t chunk_bases; necat_cns_options co;
    size_t pi = 0, ci = 0; bool open = false; std::vector<uint8_t> packed; cns_chunks::Plan plan;

    CnsUnit next()
    {
        CnsUnit w; w.t0 = now_sec(); w.owner = ctx;
        auto failed = [&w](const char* what, const std::string& detail) { w.rc = 1; w.what = what; w.detail = detail; return std::move(w); };
        if (!open) {
            if (pi == pids.size()) { w.done = true; return w; }
            w.pid = pids[pi];
            char suffix[32];
            snprintf(suffix, sizeof suffix, ".p%d", w.pid);
            FILE* in = fopen((can_path + suffix).c_str(), "rb");
            if (!in) return failed("candidates", "cannot open " + can_path + suffix);
            fseek(in, 0, SEEK_END);
            const long bytes = ftell(in);
            fseek(in, 0, SEEK_SET);
            packed.resize((size_t)(bytes / 28) * 28);
            if (!packed.empty() && fread(packed.data(), 1, packed.size(), in) != packed.size()) { fclose(in); return failed("candidates", "short read"); }
            fclose(in);
            open = true; ci = 0; plan = cns_chunks::Plan();
            std::string why;
            if (rs.gathered && !packed.empty() && !cns_chunks::plan_chunks((const uint32_t*)packed.data(), packed.size() / 28, rs.size.data(), rs.size.size(), chunk_bases, &plan, &why))
                return failed("candidates", why);
        }
        w.pid = pids[pi];
        auto partition_done = [&]() { open = false; ++pi; packed.clear(); };
        if (packed.empty()) { w.empty = true; partition_done(); return w; }
        const void* recs = packed.data(); uint64_t nrecs = packed.size() / 28;
        std::vector<uint32_t> local;
        if (!rs.gathered) w.vol = rs.merged;
        else {
            const cns_chunks::Chunk& c = plan.chunks[ci];
            w.first = ci == 0; w.last = ci + 1 == plan.chunks.size(); w.n_chunks = plan.chunks.size();
            if (c.bases >= cns_chunks::kMaxChunkBases)
                return failed("chunk", "the candidates of template " + std::to_string(((const uint32_t*)packed.data())[7 * plan.order[c.rec_begin] + 1]) + " name reads of " +
                                       std::to_string(c.bases) + " bases: 2^32 or more, too many for one gathered volume");
            const double g0 = now_sec();
            if (necat_volume_gather(ctx, rs.file_vols.data(), rs.vol_start.data(), rs.file_vols.size(), c.ids.data(), c.ids.size(), &w.vol)) return failed("necat_volume_gather", necat_last_error(ctx));
            w.own_vol = true;
            w.gather_ms = (now_sec() - g0) * 1e3; w.gathered_bases = c.bases; w.ids = c.ids;
            uint64_t moved = 0;
            (void)necat_volume_gather_stats(ctx, &w.gather_kernel_ms, &moved);
            local.resize((size_t)(c.rec_end - c.rec_begin) * 7);
            cns_chunks::chunk_records((const uint32_t*)packed.data(), plan, c, local.data());
            recs = local.data(); nrecs = c.rec_end - c.rec_begin;
        }
        if (necat_cns_load_partition(ctx, w.vol, recs, nrecs, &w.cands, &w.tmpl_off, &w.n_all, &w.nt)) return failed("necat_cns_load_partition", necat_last_error(ctx));
        ++ci;
        if (w.last) partition_done();
        if (necat_cns_extension_batch(ctx, w.vol, w.cands, w.tmpl_off, w.n_all, w.nt, &co, &w.res)) return failed("necat_cns_extension_batch", necat_last_error(ctx));
        w.t_gpu = now_sec() - w.t0;
        return w;
    }
};

// the source one finished unit ahead of take()'s caller, on a thread of its own: one producer, one consumer, one slot (the alignment columns of a unit are
// hundreds of MB of pinned memory; at most two gathered volumes are alive).  The context of the source is that thread's alone while this lives.  Not threaded:
// take() is next(), one unit after the other on the caller's thread.  The thread stops after a failed unit or the end, or when this goes.
struct CnsHandoff {
    CnsUnitSource& src;
    std::mutex mu; std::condition_variable cv;
    CnsUnit slot; bool full = false, stop = false;
    std::thread producer;

    CnsHandoff(CnsUnitSource& s, bool threaded) : src(s)
    {
        if (threaded) producer = std::thread([this]() {
            for (;;) {
                { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return !full || stop; }); if (stop) return; }
                CnsUnit w = src.next();
                const bool last = w.rc != 0 || w.done;
                { std::lock_guard<std::mutex> lk(mu); slot = std::move(w); full = true; }
                cv.notify_all();
                if (last) return;
            }
        });
    }
    CnsUnit take()
    {
        if (!producer.joinable()) return src.next();
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return full; });
        CnsUnit w = std::move(slot); full = false;
        lk.unlock(); cv.notify_all();
        return w;
    }
    ~CnsHandoff()
    {
        if (!producer.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        producer.join();
    }
};

// the second stage: the consensus proper of a unit on `cctx` (necat_cns_consensus_batch: on the device with its certified fallback, or on the library's host
// threads - NECAT_CNS_DEVICE), the record text on `nthreads` host threads (cns_consensus.h: emit_template), written in template order with global ids; and what a
// partition's units add up to
struct CnsConsumer {
    necat_ctx* cctx; const CnsReadSet& rs; const std::vector<int>& pids; necat_cns_consensus_options cco; bool small_memory, pipelined; uint64_t chunk_bases;
    FILE* cns_out; FILE* raw_out; int trace;
    struct PartAcc {         // its log lines, and the reads of its id range nobody corrected
        double t0 = 0, t_gpu = 0, t_host = 0, gather_ms = 0, gather_kernel_ms = 0;
        uint64_t nt = 0, gathered_reads = 0, gathered_bases = 0;
        int min_id = 0, max_id = 0;
        std::vector<int> corrected;
    } acc;
    size_t pi = 0; bool begun = false; char job[128] = ""; double t_prev_done = now_sec();

    void begin_partition() { if (!begun && pi < pids.size()) { snprintf(job, sizeof job, "consensus partition %d", pids[pi]); log_line("", job); begun = true; } }
    bool consume(CnsUnit& W, CnsError* e)
    {
        if (W.first) { acc = PartAcc(); acc.t0 = pipelined ? t_prev_done : W.t0; }          // what this partition added to the wall clock: from here
        if (W.empty) return true;
        const uint64_t nt = W.nt;
        const int nthreads = cco.host_threads;
        const double t_host0 = now_sec();
        necat_cns_consensus* con = nullptr;
        if (necat_cns_consensus_batch(cctx, W.vol, W.cands, W.tmpl_off, nt, W.res, &cco, &con)) { *e = {"necat_cns_consensus_batch", necat_last_error(cctx)}; return false; }
        uint64_t n_host = 0;
        for (uint64_t t = 0; t < nt; ++t) n_host += con->templates[t].on_host != 0;
        if (trace & 2) fprintf(stderr, "[oc2cns] partition %d: consensus proper of %lu templates on the device, %lu on the host (%s path; device %.2f ms, host %.2f ms)\n", W.pid,
                               (unsigned long)con->n_device, (unsigned long)n_host, cco.path ? "host" : "device", con->device_ms, con->host_ms);
        std::vector<std::string> out_cns((size_t)nt), out_raw((size_t)nt);
        std::vector<uint8_t> corrected((size_t)nt, 0);
        Deal templates(nt);
        on_threads((unsigned)nthreads, [&](unsigned) {
            cns::Worker w;
            std::vector<cns::SegCodes> kept;
            std::vector<uint8_t> tbases;
            templates.run([&](uint64_t t) {
                const necat_cns_template& T = W.res->templates[t];
                if (!T.examined) return;
                const necat_candidate& c0 = W.cands[W.tmpl_off[t]];
                const int tid = W.global_id(c0.sid), tsize = (int)c0.ssize;
                const necat_cns_consensus_template& CT = con->templates[t];
                kept.clear();
                for (uint64_t k = CT.seg_begin; k < CT.seg_end; ++k) {
                    const necat_cns_segment& sg = con->segments[k];
                    cns::SegCodes o; o.left = sg.left; o.right = sg.right; o.cns_from = sg.cns_from; o.cns_to = sg.cns_to;
                    o.seq.assign((const char*)con->bases + sg.off, sg.len);
                    kept.push_back(std::move(o));
                }
                corrected[t] = cns::emit_template(w, kept, rs.read((uint64_t)tid, tbases), tsize, tid, rs.names[(size_t)tid].c_str(), cco.full_consensus != 0, T.num_can, T.num_ovlps,
                                                  T.ident_cutoff, out_cns[t], out_raw[t]) ? 1 : 0;
            });
        });
        necat_cns_consensus_free(con);
        bool wok = true;
        for (uint64_t t = 0; t < nt; ++t) {
            if (!out_cns[t].empty()) wok = wok && fwrite(out_cns[t].data(), 1, out_cns[t].size(), cns_out) == out_cns[t].size();
            if (!out_raw[t].empty()) wok = wok && fwrite(out_raw[t].data(), 1, out_raw[t].size(), raw_out) == out_raw[t].size();
        }
        for (uint64_t t = 0; t < nt; ++t) {
            const int id = W.global_id(W.cands[W.tmpl_off[t]].sid);
            if (!acc.nt && !t) acc.min_id = acc.max_id = id;
            acc.min_id = std::min(acc.min_id, id); acc.max_id = std::max(acc.max_id, id);
            if (corrected[t]) acc.corrected.push_back(id);
        }
        acc.nt += nt; acc.t_gpu += W.t_gpu; acc.gather_ms += W.gather_ms; acc.gather_kernel_ms += W.gather_kernel_ms;
        acc.gathered_reads += W.ids.size(); acc.gathered_bases += W.gathered_bases;
        W.release(cctx);
        acc.t_host += now_sec() - t_host0;
        if (!wok) *e = {"output", "write failed"};
        return wok;
    }
    // after the partition's last unit
    bool finish_partition(const CnsUnit& W, CnsError* e)
    {
        if (!W.empty) {
            // the reads of the partition's id range nobody corrected go out whole (consensus_one_partition.c:172-194; the last id
            // of the range is left out there: `i < max_read_id`) - only with -s 0: the reference does this inside `if (reads)`, and with
            // -s 1 it never loads `reads` (the small-memory path reads sequences per partition), so it writes none of them
            if (!small_memory && acc.nt) {
                const double t_raw0 = now_sec();
                std::vector<uint8_t> done((size_t)(acc.max_id - acc.min_id + 1), 0), bases;
                for (int id : acc.corrected) done[(size_t)(id - acc.min_id)] = 1;
                std::string rec;
                for (int id = acc.min_id; id < acc.max_id; ++id) {
                    if (done[(size_t)(id - acc.min_id)]) continue;
                    rec.clear();
                    cns::uncorrected_record(rec, rs.read((uint64_t)id, bases), (int)rs.size[(size_t)id], id, rs.names[(size_t)id].c_str());
                    if (fwrite(rec.data(), 1, rec.size(), raw_out) != rec.size()) { *e = {"output", "write failed"}; return false; }
                }
                acc.t_host += now_sec() - t_raw0;
            }
            if (!W.ids.empty() && (trace & 2))
                fprintf(stderr, "[oc2cns] partition %d: %lu chunks of at most %lu bases, %lu reads and %lu bases gathered in %.2f ms (the gather kernels: %.3f ms)\n", W.pid, (unsigned long)W.n_chunks,
                        (unsigned long)chunk_bases, (unsigned long)acc.gathered_reads, (unsigned long)acc.gathered_bases, acc.gather_ms, acc.gather_kernel_ms);
            fprintf(stdout, "[oc2cns] partition %d: %lu templates, extension loop %.2f s%s, consensus %.2f s (%d host threads)\n", W.pid, (unsigned long)acc.nt, acc.t_gpu,
                    pipelined && pi ? " (beside the previous partition's consensus)" : "", acc.t_host, cco.host_threads);
        }
        log_line("[%s] INFO: '%s' takes %.2lf secs.\n", job, now_sec() - acc.t0);
        t_prev_done = now_sec();
        ++pi; begun = false;
        return true;
    }
};

// co / cco: the parsed options (cco.host_threads = -t; cco.path is decided here, by NECAT_CNS_DEVICE); small_memory: -s; -mn's pair: the partitions node_id,
// node_id + num_nodes, ...  Returns 0, or 1 after printing "[oc2cns] ERROR: what: detail" (every fatal error of the reference is OC_ERROR -> exit 1).
inline int cns_run_job(const necat_cns_options& co, necat_cns_consensus_options cco, bool small_memory, const char* wrk_dir, const std::string& can_path,
                       const char* cns_out_path, const char* raw_out_path, int node_id, int num_nodes, int device)
{
    auto fail = [](const std::string& what, const std::string& detail) { fprintf(stderr, "[oc2cns] ERROR: %s: %s\n", what.c_str(), detail.c_str()); return 1; };
    // everything the job holds, released on EVERY way out, last made first: the producer thread is joined before anything it uses goes
    struct Held {
        necat_ctx* ctx = nullptr; necat_ctx* cctx = nullptr; FILE* cns_out = nullptr; FILE* raw_out = nullptr;
        CnsReadSet rs;
        ~Held()
        {
            if (cns_out) fclose(cns_out);
            if (raw_out) fclose(raw_out);
            rs.release();
            if (cctx && cctx != ctx) necat_ctx_destroy(cctx);
            if (ctx) necat_ctx_destroy(ctx);
        }
    } H;
    CnsError e;
    VolumesInfo vi;
    if (!load_volumes_info(wrk_dir, &vi, &e.detail)) return fail("volume directory", e.detail);
    // (NECAT_CNS_READS and NECAT_CNS_CHUNK_BASES are knobs of the library's table, knobs.h, read when the context is created)
    if (necat_ctx_create(device, &H.ctx)) { H.ctx = nullptr; return fail("GPU", "no usable gfx950 device (libnecat_hip has no CPU fallback)"); }
    std::string reads_mode = "auto";
    uint64_t chunk_bases = cns_chunks::kDefaultChunkBases;
    char buf[256];
    if (necat_knob_get(H.ctx, "NECAT_CNS_READS", buf, sizeof buf) == 0 && buf[0]) reads_mode = buf;
    if (necat_knob_get(H.ctx, "NECAT_CNS_CHUNK_BASES", buf, sizeof buf) == 0 && buf[0]) chunk_bases = strtoull(buf, nullptr, 10);
    if (!H.rs.load(vi, reads_mode, &e)) return fail(e.what, e.detail);
    int num_partitions = 0;
    {
        FILE* in = fopen((can_path + ".partitions").c_str(), "r");
        const bool ok = in && fscanf(in, "%d", &num_partitions) == 1;
        if (in) fclose(in);
        if (!ok) return fail("candidates", "cannot read the .partitions file (run oc2pcan first)");
    }
    H.cns_out = fopen(cns_out_path, "w");
    H.raw_out = fopen(raw_out_path, "w");
    if (!H.cns_out || !H.raw_out) return fail("output", "cannot open for writing");
    if (!H.rs.upload(H.ctx, &e)) return fail(e.what, e.detail);

    CnsUnitSource src{H.ctx, H.rs, can_path, {}, chunk_bases, co};
    for (int pid = node_id; pid < num_partitions; pid += num_nodes) src.pids.push_back(pid);
    const char* pipeline_env = getenv("NECAT_CNS_PIPELINE");
    const bool pipelined = (src.pids.size() > 1 || (H.rs.gathered && !src.pids.empty())) && !(pipeline_env && atoi(pipeline_env) == 0);
    CnsHandoff units(src, pipelined);
    // the consensus proper runs on this thread beside the producer's extension loop: one host thread per context (include/necat_hip.h), so it gets a context of its own
    H.cctx = H.ctx;
    if (pipelined && necat_ctx_create(device, &H.cctx)) { H.cctx = nullptr; return fail("GPU", "no second context for the consensus proper"); }
    cco.path = necat_knob_get(H.cctx, "NECAT_CNS_DEVICE", buf, sizeof buf) == 0 && atoi(buf) != 0 ? 0 : 1;
    int trace = 0;
    if (necat_knob_get(H.cctx, "NECAT_TRACE", buf, sizeof buf) == 0) trace = atoi(buf);
    CnsConsumer C{H.cctx, H.rs, src.pids, cco, small_memory, pipelined, chunk_bases, H.cns_out, H.raw_out, trace};
    for (;;) {
        C.begin_partition();
        CnsUnit W = units.take();
        W.owner = H.cctx;               // this thread's from here on (a gathered volume is freed through the second context)
        if (W.rc) return fail(W.what, W.detail);
        if (W.done) break;
        if (!C.consume(W, &e) || (W.last && !C.finish_partition(W, &e))) return fail(e.what, e.detail);
    }
    const bool ok = fclose(H.cns_out) == 0;
    const bool ok2 = fclose(H.raw_out) == 0;
    H.cns_out = H.raw_out = nullptr;
    if (!ok || !ok2) return fail("output", "write failed");
    return 0;
}

}  // namespace necat_host
