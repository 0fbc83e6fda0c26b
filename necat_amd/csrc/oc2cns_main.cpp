// oc2cns - drop-in replacement of NECAT's oc2cns (consensus/main.c:51-78):
//   oc2cns [options] wrk_dir candidates cns_out raw_out [-mn node_id num_nodes]
// Same argv (consensus/cns_options.c:10, -mn as consensus/main.c:37-41), same inputs (the volume directory, the
// candidate partitions `candidates.p<i>` written by oc2pcan), same two FASTA outputs: corrected reads / stretches
// (cns_out) and the uncorrected rest (raw_out), record format DUMP_CNS_SEQ (common/cns_seq.h:24-44).
//
// Partitions go through two stages one partition apart: the extension loop of partition p + 1 on the GPU (a producer thread) beside the host
// consensus of partition p (consensus_one_partition.c:110 runs them one after the other; the files come out the same).
// Per partition: the extension loop of every template runs on the GPU (necat_cns_extension_batch: which candidates get
// aligned, which alignments count, with what weight - consensus/consensus_one_read.c:221-372), the consensus proper
// (tasc/) through necat_cns_consensus_batch: on the library's host threads (cns_consensus.h; NECAT_CNS_DEVICE=0) or on the
// device with a certified fallback to that code (NECAT_CNS_DEVICE=1); the record text is written here.  Records come out in template order (the reference's order with -t 1;
// with more threads the reference's order depends on scheduling).
// -r 1 (rescue_long_indels): candidates whose block-wise extension failed or fell short go through DALIGNER's local alignment and
// edlib's global path after each device pass, as in the reference (cns_rescue.h): on the host threads, or on the device with
// NECAT_DALIGN_DEVICE=1 / NECAT_NW_DEVICE=1 (necat_local_align_batch / necat_nw_path_batch).  -s 1 (small memory: reads
// loaded per partition) behaves like -s 0 - the read set is resident in HBM either way.  There is no CPU fallback for the
// block-wise alignments: without a usable GPU the program exits 1.
// The read set: one volume while the directory holds fewer than 2^32 bases (a volume's limit).  From there on, or with NECAT_CNS_READS=gather, every volume
// file stays a resident volume of its own and a partition is worked in chunks of whole templates (cns_chunks.h, NECAT_CNS_CHUNK_BASES): the reads a chunk's
// candidates name are gathered on the device into one compact volume (necat_volume_gather), the entries above run on it with the records' ids rewritten, and the
// ids are mapped back when the records are written.  The two stages then run one CHUNK apart; the files are the same.
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "host_io.h"
#include "host_threads.h"
#include "host_bases.h"
#include "cns_chunks.h"
#include "cns_consensus.h"

using namespace necat_host;

namespace {

struct CnsOpts {             // consensus/cns_options.h:6-18, defaults cns_options.c:10-22
    int min_align_size = 400, min_cov = 4, max_cov = 12, min_size = 500, full_consensus = 0;
    double error = 0.5, mapping_ratio = 0.8;
    int num_threads = 1, rescue_long_indels = 0, use_fixed_ident_cutoff = 0, small_memory = 0;
};

void describe(FILE* out)
{
    fprintf(out, "-a <Integer>\talign length cutoff\n-x <Integer>\tminimal coverage\n-y <Integer>\tmaximal coverage\n"
                 "-l <Integer>\tminimal length of corrected reads.\n-f <0 or 1>\tfull consensus or not: 1 = yes, 0 = no\n"
                 "-e <Real>\tsequencing error\n-p <Real>\tminimal mapping ratio\n-t <Integer>\tnumber of cpu threads\n"
                 "-r <0 or 1>\trescue long indels or not: 1 = yes, 0 = no\n-u <0 or 1>\tuse dynamic or fixed ident cutoff: 1 = fixed, 0 = dynamic\n"
                 "-s <0 or 1>\tuse small memoty\nDEFAULT OPTIONS:\n");
    CnsOpts d;
    fprintf(out, "-a %d -x %d -y %d -l %d -f %d -e %f -p %f -t %d -r %d -u %d -s %d\t\n", d.min_align_size, d.min_cov, d.max_cov, d.min_size, d.full_consensus,
            d.error, d.mapping_ratio, d.num_threads, d.rescue_long_indels, d.use_fixed_ident_cutoff, d.small_memory);
}

bool parse(int argc, char** argv, CnsOpts* o)
{
    optind = 1;
    int c;
    while ((c = getopt(argc, argv, "a:x:y:l:f:e:p:t:r:u:s:")) != -1) {
        switch (c) {
        case 'a': o->min_align_size = atoi(optarg); break;
        case 'x': o->min_cov = atoi(optarg); break;
        case 'y': o->max_cov = atoi(optarg); break;
        case 'l': o->min_size = atoi(optarg); break;
        case 'f': o->full_consensus = atoi(optarg); break;
        case 'e': o->error = atof(optarg); break;
        case 'p': o->mapping_ratio = atof(optarg); break;
        case 't': o->num_threads = atoi(optarg); break;
        case 'r': o->rescue_long_indels = atoi(optarg); break;
        case 'u': o->use_fixed_ident_cutoff = atoi(optarg); break;
        case 's': o->small_memory = atoi(optarg); break;
        default: return false;
        }
    }
    return true;
}

int usage(const char* prog)
{
    fprintf(stderr, "USAGE:\n%s [options] wrk_dir candidates cns_out raw_out\n\nIf Multiple Nodes Are Used:\n"
                    "%s [options] wrk_dir candidates cns_out raw_out -mn node_id num_nodes\n\nOPTIONS AND DESCRIPTIONS:\n", prog, prog);
    describe(stderr);
    return 1;
}

int fail(const char* what, const char* detail) { fprintf(stderr, "[oc2cns] ERROR: %s: %s\n", what, detail); return 1; }

// all volumes as one read set with global ids (merge_volumes, common/makedb_aux.c:137-153).  merged: the bases at one byte each.  gather (a project of 2^32
// bases and more, NECAT_CNS_READS): the volume files' pac bytes as they are, a read's bases decoded when a record needs them.
struct ReadSet {
    std::vector<uint8_t> codes;            // merged: one byte per base (0..3)
    std::vector<uint64_t> offset, size;
    std::vector<std::string> names;
    std::vector<HostVolume> vols;          // gather: the volume files (merged: released after the load)
    std::vector<int64_t> vol_start;        // .. and the global id of each one's first read
    bool gathered = false;
    // the bases of read `id`: in place (merged), or decoded into buf
    const uint8_t* read(uint64_t id, std::vector<uint8_t>& buf) const
    {
        if (!gathered) return codes.data() + offset[id];
        const size_t v = (size_t)(std::upper_bound(vol_start.begin(), vol_start.end(), (int64_t)id) - vol_start.begin()) - 1;
        const HostVolume& hv = vols[v];
        const uint64_t k = id - (uint64_t)vol_start[v];
        buf.resize(hv.size[k]);
        decode_pac(hv.pac.data(), hv.offset[k], hv.size[k], buf.data());
        return buf.data();
    }
};

// one unit of the program's two stages: a partition (merged), or a chunk of a partition's templates on the volume gathered for it (gather)
struct Unit {
    bool done = false;                       // no more units
    int pid = -1; bool first = true, last = true, empty = false; int rc = 0; std::string what, detail;
    necat_candidate* cands = nullptr; uint64_t* tmpl_off = nullptr; uint64_t* n_all = nullptr; uint64_t nt = 0;
    necat_cns_result* res = nullptr; double t_gpu = 0, t0 = 0;
    necat_volume* vol = nullptr;             // the volume its ids refer to: the merged one, or its own gathered one
    std::vector<int64_t> ids;                // gather: local id -> global id
    uint64_t n_chunks = 0, gathered_bases = 0; double gather_ms = 0, gather_kernel_ms = 0;
};

}  // namespace

int main(int argc, char** argv)
{
    necat_host::necat_cli_env();          // (before the first HIP call: host_io.h)
    CnsOpts opt;
    int spid = 0, nnode = 1;
    int ac = argc;
    if (ac >= 8 && strcmp(argv[ac - 3], "-mn") == 0) { spid = atoi(argv[ac - 2]); nnode = atoi(argv[ac - 1]); ac -= 3; }
    if (ac < 5 || !parse(ac - 4, argv, &opt) || nnode < 1 || spid < 0) return usage(argv[0]);
    const char* wrk_dir = argv[ac - 4];
    const std::string can_path = argv[ac - 3];
    const char* cns_out_path = argv[ac - 2];
    const char* raw_out_path = argv[ac - 1];
    if (opt.max_cov < 1 || opt.min_cov < 0) return fail("options", "coverage limits out of range");

    std::string err;
    VolumesInfo vi;
    if (!load_volumes_info(wrk_dir, &vi, &err)) return fail("volume directory", err.c_str());
    // NECAT_CNS_READS: merged - the whole directory as one volume, which holds fewer than 2^32 bases; gather - one resident volume per file and, per chunk of
    // templates, the reads its candidates name gathered on the device (cns_chunks.h); auto (the default) - merged while the directory's total allows it
    // (both are knobs of the library's table, knobs.h, read when the context is created)
    necat_ctx* ctx = nullptr;
    const char* dev_env = getenv("NECAT_GPU");
    if (necat_ctx_create(dev_env ? atoi(dev_env) : 0, &ctx)) return fail("GPU", "no usable gfx950 device (libnecat_hip has no CPU fallback)");
    std::string reads_mode = "auto";
    uint64_t chunk_bases = cns_chunks::kDefaultChunkBases;
    {
        char buf[256];
        if (necat_knob_get(ctx, "NECAT_CNS_READS", buf, sizeof buf) == 0 && buf[0]) reads_mode = buf;
        if (necat_knob_get(ctx, "NECAT_CNS_CHUNK_BASES", buf, sizeof buf) == 0 && buf[0]) chunk_bases = strtoull(buf, nullptr, 10);
    }
    if (reads_mode != "merged" && reads_mode != "gather" && reads_mode != "auto") return fail("NECAT_CNS_READS", "merged, gather or auto");
    ReadSet rs;
    {
        log_line("", "load reads");
        const double t0 = now_sec();
        uint64_t total = 0;
        std::vector<HostVolume>& vols = rs.vols;
        vols.resize((size_t)vi.num_volumes);
        for (int v = 0; v < vi.num_volumes; ++v) {
            if (!load_volume(vi.names[v].c_str(), &vols[v], &err)) return fail("volume", err.c_str());
            total += vols[v].nbases;
        }
        rs.gathered = reads_mode == "gather" || (reads_mode == "auto" && total >= cns_chunks::kMaxChunkBases);
        if (!rs.gathered) rs.codes.resize(total);
        uint64_t at = 0;
        for (int v = 0; v < vi.num_volumes; ++v) {
            const HostVolume& hv = vols[v];
            rs.vol_start.push_back((int64_t)rs.size.size());
            for (uint64_t i = 0; i < hv.offset.size(); ++i) {
                rs.offset.push_back(at + hv.offset[i]); rs.size.push_back(hv.size[i]); rs.names.emplace_back(hv.name(i));
            }
            if (!rs.gathered) decode_pac(hv.pac.data(), 0, hv.nbases, rs.codes.data() + at);
            at += hv.nbases;
        }
        if (!rs.gathered) { rs.vols.clear(); rs.vols.shrink_to_fit(); }
        log_line("[%s] INFO: '%s' takes %.2lf secs.\n", "load reads", now_sec() - t0);
    }
    const uint64_t nreads = rs.size.size();

    int num_partitions = 0;
    {
        FILE* in = fopen((can_path + ".partitions").c_str(), "r");
        if (!in || fscanf(in, "%d", &num_partitions) != 1) return fail("candidates", "cannot read the .partitions file (run oc2pcan first)");
        fclose(in);
    }
    FILE* cns_out = fopen(cns_out_path, "w");
    FILE* raw_out = fopen(raw_out_path, "w");
    if (!cns_out || !raw_out) return fail("output", "cannot open for writing");

    necat_volume* reads = nullptr;                  // merged: the read set
    std::vector<necat_volume*> file_vols;           // gather: the volume files, resident as oc2mkdb wrote them
    if (!rs.gathered) {
        // NECAT pac of the merged set (first base of a byte in its top two bits)
        std::vector<uint8_t> pac((rs.codes.size() + 3) / 4 + 8, 0);
        for (uint64_t i = 0; i < rs.codes.size(); ++i) pac[i >> 2] |= (uint8_t)(rs.codes[i] << ((~i & 3) << 1));
        if (necat_volume_upload(ctx, pac.data(), rs.codes.size(), rs.offset.data(), rs.size.data(), nreads, &reads)) return fail("necat_volume_upload", necat_last_error(ctx));
    } else {
        for (const HostVolume& hv : rs.vols) {
            necat_volume* dv = nullptr;
            if (necat_volume_upload(ctx, hv.pac.data(), hv.nbases, hv.offset.data(), hv.size.data(), hv.offset.size(), &dv)) return fail("necat_volume_upload", necat_last_error(ctx));
            file_vols.push_back(dv);
        }
    }
    necat_cns_options co; necat_cns_default_options(&co);
    co.min_align_size = opt.min_align_size; co.min_cov = opt.min_cov; co.max_cov = opt.max_cov; co.error = opt.error;
    co.mapping_ratio = opt.mapping_ratio; co.use_fixed_ident_cutoff = opt.use_fixed_ident_cutoff;
    co.rescue_long_indels = opt.rescue_long_indels != 0;
    const int nthreads = std::max(1, std::min(opt.num_threads, 256));       // -t: host threads of the consensus proper (its host form and fallback) and of the record text

    // ---- two stages, one unit apart (round 6): a producer thread reads partition p + 1 and runs its extension loop on the device
    // (necat_cns_load_partition + necat_cns_extension_batch: the context is that thread's alone from here on) while the host threads do the
    // consensus proper of partition p - 88 % of a partition's time is host work, the device loop of the next one hides behind it.
    // One finished unit waits at most (the alignment columns of a partition are hundreds of MB of pinned memory).  Output order =
    // partition order, as before.  NECAT_CNS_PIPELINE=0: one unit after the other on the main thread (the round-5 form).
    // The unit is the partition, or - gather - a chunk of its templates: the producer gathers the chunk's reads first, and the gathered volume lives until the
    // chunk's consensus is done, so at most two of them are alive.
    std::vector<int> pids;
    for (int pid = spid; pid < num_partitions; pid += nnode) pids.push_back(pid);
    struct Source { size_t pi = 0, ci = 0; bool open = false; std::vector<uint8_t> packed; cns_chunks::Plan plan; } src;
    auto next_unit = [&]() -> Unit {
        Unit w; w.t0 = now_sec();
        auto failed = [&w](const char* what, const std::string& detail) -> Unit& { w.rc = 1; w.what = what; w.detail = detail; return w; };
        if (!src.open) {
            if (src.pi == pids.size()) { w.done = true; return w; }
            w.pid = pids[src.pi];
            std::vector<uint8_t>& packed = src.packed;
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
            src.open = true; src.ci = 0; src.plan = cns_chunks::Plan();
            std::string why;
            if (rs.gathered && !packed.empty() && !cns_chunks::plan_chunks((const uint32_t*)packed.data(), packed.size() / 28, rs.size.data(), nreads, chunk_bases, &src.plan, &why))
                return failed("candidates", why);
        }
        w.pid = pids[src.pi];
        auto partition_done = [&]() { src.open = false; ++src.pi; src.packed.clear(); };
        if (src.packed.empty()) { w.empty = true; partition_done(); return w; }
        if (!rs.gathered) {
            w.vol = reads;
            if (necat_cns_load_partition(ctx, reads, src.packed.data(), src.packed.size() / 28, &w.cands, &w.tmpl_off, &w.n_all, &w.nt)) return failed("necat_cns_load_partition", necat_last_error(ctx));
            partition_done();
        } else {
            const cns_chunks::Chunk& c = src.plan.chunks[src.ci];
            w.first = src.ci == 0; w.last = src.ci + 1 == src.plan.chunks.size(); w.n_chunks = src.plan.chunks.size();
            if (c.bases >= cns_chunks::kMaxChunkBases)
                return failed("chunk", "the candidates of template " + std::to_string(((const uint32_t*)src.packed.data())[7 * src.plan.order[c.rec_begin] + 1]) + " name reads of " +
                                       std::to_string(c.bases) + " bases: 2^32 or more, too many for one gathered volume");
            const double g0 = now_sec();
            if (necat_volume_gather(ctx, file_vols.data(), rs.vol_start.data(), file_vols.size(), c.ids.data(), c.ids.size(), &w.vol)) return failed("necat_volume_gather", necat_last_error(ctx));
            w.gather_ms = (now_sec() - g0) * 1e3; w.gathered_bases = c.bases; w.ids = c.ids;
            uint64_t moved = 0;
            (void)necat_volume_gather_stats(ctx, &w.gather_kernel_ms, &moved);
            std::vector<uint32_t> recs((size_t)(c.rec_end - c.rec_begin) * 7);
            cns_chunks::chunk_records((const uint32_t*)src.packed.data(), src.plan, c, recs.data());
            if (necat_cns_load_partition(ctx, w.vol, recs.data(), c.rec_end - c.rec_begin, &w.cands, &w.tmpl_off, &w.n_all, &w.nt)) return failed("necat_cns_load_partition", necat_last_error(ctx));
            if (++src.ci == src.plan.chunks.size()) partition_done();
        }
        if (necat_cns_extension_batch(ctx, w.vol, w.cands, w.tmpl_off, w.n_all, w.nt, &co, &w.res)) return failed("necat_cns_extension_batch", necat_last_error(ctx));
        w.t_gpu = now_sec() - w.t0;
        return w;
    };
    const bool pipelined = (pids.size() > 1 || (rs.gathered && !pids.empty())) && !(getenv("NECAT_CNS_PIPELINE") && atoi(getenv("NECAT_CNS_PIPELINE")) == 0);
    std::mutex qmu; std::condition_variable qcv;
    std::deque<Unit> ready;                  // finished device stages, in order (at most one waits)
    bool stop = false;
    std::thread producer;
    if (pipelined) producer = std::thread([&]() {
        for (;;) {
            { std::unique_lock<std::mutex> lk(qmu); qcv.wait(lk, [&] { return ready.size() < 1 || stop; }); if (stop) return; }
            Unit w = next_unit();
            const bool last = w.rc != 0 || w.done;
            { std::lock_guard<std::mutex> lk(qmu); ready.push_back(std::move(w)); }
            qcv.notify_all();
            if (last) return;
        }
    });
    auto stop_producer = [&]() { if (producer.joinable()) { { std::lock_guard<std::mutex> lk(qmu); stop = true; } qcv.notify_all(); producer.join(); } };
    // the consensus proper runs on this thread beside the producer's extension loop: one host thread per context (include/necat_hip.h), so it gets a context of its own
    necat_ctx* cctx = ctx;
    if (pipelined && necat_ctx_create(dev_env ? atoi(dev_env) : 0, &cctx)) { stop_producer(); return fail("GPU", "no second context for the consensus proper"); }
    necat_cns_consensus_options cco; necat_cns_consensus_default_options(&cco);
    cco.min_cov = opt.min_cov; cco.min_size = opt.min_size; cco.full_consensus = opt.full_consensus != 0; cco.host_threads = nthreads;
    int trace = 0;
    {
        char buf[64];
        cco.path = necat_knob_get(cctx, "NECAT_CNS_DEVICE", buf, sizeof buf) == 0 && atoi(buf) != 0 ? 0 : 1;
        if (necat_knob_get(cctx, "NECAT_TRACE", buf, sizeof buf) == 0) trace = atoi(buf);
    }
    double t_prev_done = now_sec();
    // what a partition's units add up to: its log lines, and the reads of its id range nobody corrected
    struct PartAcc {
        double t0 = 0, t_gpu = 0, t_host = 0, gather_ms = 0, gather_kernel_ms = 0;
        uint64_t nt = 0, gathered_reads = 0, gathered_bases = 0;
        int min_id = 0, max_id = 0;
        std::vector<int> corrected;
    } acc;
    size_t pi = 0;
    bool begun = false;
    char job[128] = "";
    for (;;) {
        if (!begun && pi < pids.size()) { snprintf(job, sizeof job, "consensus partition %d", pids[pi]); log_line("", job); begun = true; }
        Unit W;
        if (pipelined) {
            std::unique_lock<std::mutex> lk(qmu);
            qcv.wait(lk, [&] { return !ready.empty(); });
            W = std::move(ready.front()); ready.pop_front();
            lk.unlock(); qcv.notify_all();
        } else W = next_unit();
        if (W.rc) { stop_producer(); return fail(W.what.c_str(), W.detail.c_str()); }
        if (W.done) break;
        const int pid = W.pid;
        if (W.first) { acc = PartAcc(); acc.t0 = pipelined ? t_prev_done : W.t0; }          // what this partition added to the wall clock: from here
        if (W.empty) { log_line("[%s] INFO: '%s' takes %.2lf secs.\n", job, now_sec() - acc.t0); t_prev_done = now_sec(); ++pi; begun = false; continue; }
        necat_candidate* cands = W.cands; uint64_t* tmpl_off = W.tmpl_off; uint64_t* n_all = W.n_all; const uint64_t nt = W.nt;
        necat_cns_result* res = W.res;
        const double t_host0 = now_sec();
        auto global_id = [&W](int local) { return W.ids.empty() ? local : (int)W.ids[(size_t)local]; };
        // ---- consensus proper: the segments of every template from the library (necat_cns_consensus_batch: on the device with its certified fallback, or on
        // the library's host threads - NECAT_CNS_DEVICE), the records from them here, templates in parallel (cns_consensus.h: emit_template)
        necat_cns_consensus* con = nullptr;
        if (necat_cns_consensus_batch(cctx, W.vol, cands, tmpl_off, nt, res, &cco, &con)) { stop_producer(); return fail("necat_cns_consensus_batch", necat_last_error(cctx)); }
        uint64_t n_host = 0;
        for (uint64_t t = 0; t < nt; ++t) n_host += con->templates[t].on_host != 0;
        if (trace & 2) fprintf(stderr, "[oc2cns] partition %d: consensus proper of %lu templates on the device, %lu on the host (%s path; device %.2f ms, host %.2f ms)\n", pid,
                               (unsigned long)con->n_device, (unsigned long)n_host, cco.path ? "host" : "device", con->device_ms, con->host_ms);
        std::vector<std::string> out_cns((size_t)nt), out_raw((size_t)nt);
        std::vector<uint8_t> corrected((size_t)nt, 0);
        Deal templates(nt);
        on_threads((unsigned)nthreads, [&](unsigned) {
            cns::Worker w;
            std::vector<cns::SegCodes> kept;
            std::vector<uint8_t> tbases;
            templates.run([&](uint64_t t) {
                const necat_cns_template& T = res->templates[t];
                if (!T.examined) return;
                const necat_candidate& c0 = cands[tmpl_off[t]];
                const int tid = global_id(c0.sid), tsize = (int)c0.ssize;
                const necat_cns_consensus_template& CT = con->templates[t];
                kept.clear();
                for (uint64_t k = CT.seg_begin; k < CT.seg_end; ++k) {
                    const necat_cns_segment& sg = con->segments[k];
                    cns::SegCodes o; o.left = sg.left; o.right = sg.right; o.cns_from = sg.cns_from; o.cns_to = sg.cns_to;
                    o.seq.assign((const char*)con->bases + sg.off, sg.len);
                    kept.push_back(std::move(o));
                }
                corrected[t] = cns::emit_template(w, kept, rs.read((uint64_t)tid, tbases), tsize, tid, rs.names[(size_t)tid].c_str(), opt.full_consensus != 0, T.num_can, T.num_ovlps,
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
            const int id = global_id(cands[tmpl_off[t]].sid);
            if (!acc.nt && !t) acc.min_id = acc.max_id = id;
            acc.min_id = std::min(acc.min_id, id); acc.max_id = std::max(acc.max_id, id);
            if (corrected[t]) acc.corrected.push_back(id);
        }
        acc.nt += nt; acc.t_gpu += W.t_gpu; acc.gather_ms += W.gather_ms; acc.gather_kernel_ms += W.gather_kernel_ms;
        acc.gathered_reads += W.ids.size(); acc.gathered_bases += W.gathered_bases;
        necat_cns_result_free(res);
        necat_free(cands); necat_free(tmpl_off); necat_free(n_all);
        if (rs.gathered) necat_volume_free(cctx, W.vol);
        acc.t_host += now_sec() - t_host0;
        if (!W.last) { if (!wok) { stop_producer(); return fail("output", "write failed"); } continue; }
        // the reads of the partition's id range nobody corrected go out whole (consensus_one_partition.c:172-194; the last id
        // of the range is left out there: `i < max_read_id`) - only with -s 0: the reference does this inside `if (reads)`, and with
        // -s 1 it never loads `reads` (the small-memory path reads sequences per partition), so it writes none of them
        if (!opt.small_memory && acc.nt) {
            const double t_raw0 = now_sec();
            std::vector<uint8_t> done((size_t)(acc.max_id - acc.min_id + 1), 0), bases;
            for (int id : acc.corrected) done[(size_t)(id - acc.min_id)] = 1;
            std::string rec;
            for (int id = acc.min_id; id < acc.max_id; ++id) {
                if (done[(size_t)(id - acc.min_id)]) continue;
                rec.clear();
                cns::uncorrected_record(rec, rs.read((uint64_t)id, bases), (int)rs.size[(size_t)id], id, rs.names[(size_t)id].c_str());
                wok = wok && fwrite(rec.data(), 1, rec.size(), raw_out) == rec.size();
            }
            acc.t_host += now_sec() - t_raw0;
        }
        if (!wok) { stop_producer(); return fail("output", "write failed"); }
        if (rs.gathered && (trace & 2))
            fprintf(stderr, "[oc2cns] partition %d: %lu chunks of at most %lu bases, %lu reads and %lu bases gathered in %.2f ms (the gather kernels: %.3f ms)\n", pid, (unsigned long)W.n_chunks,
                    (unsigned long)chunk_bases, (unsigned long)acc.gathered_reads, (unsigned long)acc.gathered_bases, acc.gather_ms, acc.gather_kernel_ms);
        fprintf(stdout, "[oc2cns] partition %d: %lu templates, extension loop %.2f s%s, consensus %.2f s (%d host threads)\n", pid, (unsigned long)acc.nt, acc.t_gpu,
                pipelined && pi ? " (beside the previous partition's consensus)" : "", acc.t_host, nthreads);
        log_line("[%s] INFO: '%s' takes %.2lf secs.\n", job, now_sec() - acc.t0);
        t_prev_done = now_sec();
        ++pi; begun = false;
    }
    stop_producer();
    const bool ok = fclose(cns_out) == 0;
    const bool ok2 = fclose(raw_out) == 0;
    if (!ok || !ok2) return fail("output", "write failed");
    if (reads) necat_volume_free(ctx, reads);
    for (necat_volume* v : file_vols) necat_volume_free(ctx, v);
    if (cctx != ctx) necat_ctx_destroy(cctx);
    necat_ctx_destroy(ctx);
    return 0;
}
