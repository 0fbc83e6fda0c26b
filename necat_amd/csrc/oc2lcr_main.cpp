// oc2lcr - drop-in for the clip-range program of NECAT's read trimming stage (reference: trim_bases/largest_cover_range_main.c,
// largest_cover_range.c, detect_chimeric_reads.c, range_list.c), the program after oc2pm4 in the default pipeline (pipeline/necat.pl).
//
//   oc2lcr m4 packed_reads_dir error_cutoff min_ovlp_size min_cov min_read_size num_threads lcrv_path
//
// For every partition m4.p<i> of oc2pm4: the records sorted by subject id as the reference sorts them (klib's introsort), one range per read from
// necat_trim_ranges (include/necat_hip.h: one wave per read on the GPU), and the reads the device hands back - those whose answer depends on the
// order the records are held in - decided here by trim_core.h on the records in exactly that order.  Output: lcrv_path, the reference's text
// ("0\t0\t0\t0", then "id\tleft\tright\tsize" per read; left = -1: no usable range).  On stderr: the number of reads and how many the host decided.
//
// NECAT_TRIM_HOST=1: every read through trim_core.h and no GPU context - the A/B of the device path, and what runs on a machine without a GPU.
// NECAT_GPU: device index (default 0).  num_threads is accepted and unused (the device decides the reads; the few host reads are serial).
#include "host_io.h"
#include "trim_io.h"

using namespace necat_host::trim;

static_assert(sizeof(necat_m4) == sizeof(M4) && sizeof(necat_clip_range) == sizeof(Clip), "the library's records are trim_core.h's");

int main(int argc, char** argv)
{
    if (argc != 9) {
        fprintf(stdout, "USAGE:\n");
        fprintf(stdout, "%s m4 packed_reads_dir error_cutoff min_ovlp_size min_cov min_read_size num_threads lcrv_path\n", argv[0]);
        return 1;
    }
    const char* m4_path = argv[1];
    const char* reads_dir = argv[2];
    const double min_ident_perc = 100.0 - 100.0 * atof(argv[3]);
    const int min_ovlp_size = atoi(argv[4]), min_cov = atoi(argv[5]), min_size = atoi(argv[6]);
    const char* output = argv[8];
    const char* host_env = getenv("NECAT_TRIM_HOST");
    const bool host_only = host_env && atoi(host_env) != 0;

    int num_reads = 0, num_partitions = 0;
    if (!load_num_reads(reads_dir, &num_reads) || !load_num_partitions(m4_path, &num_partitions)) return 1;
    const int nids = num_reads + 2;
    std::vector<Clip> lcrv((size_t)nids, Clip{0, 0, 0, kNone});
    for (int p = 0; p < num_partitions; ++p) {                       // every input is checked before anything is computed or written
        uint64_t n;
        if (!record_count(partition_name(m4_path, p).c_str(), &n)) return 1;
    }
    necat_ctx* ctx = nullptr;
    if (!host_only) {
        if (necat_ctx_create(necat_host::cli_device(), &ctx)) {
            fprintf(stderr, "oc2lcr: no usable gfx950 device: %s (NECAT_TRIM_HOST=1 decides every read on the host)\n", necat_last_error(nullptr));
            return 1;
        }
    }
    int status = 0;
    uint64_t n_host = 0, n_with_records = 0;
    std::vector<M4> recs;
    std::vector<size_t> run_off;
    std::vector<uint64_t> read_off;
    std::vector<Clip> dev;
    for (int p = 0; p < num_partitions && !status; ++p) {
        if (!load_records(partition_name(m4_path, p).c_str(), recs)) { status = 1; break; }
        if (recs.empty()) continue;
        group_partition(recs, run_off);
        const size_t nrun = run_off.size() - 1;
        for (size_t r = 0; r < nrun; ++r) {
            const int sid = recs[run_off[r]].sid;
            if (sid < 0 || sid >= nids) { fprintf(stderr, "oc2lcr: read id %d in %s, the volumes hold %d reads\n", sid, partition_name(m4_path, p).c_str(), num_reads); status = 1; break; }
        }
        if (status) break;
        n_with_records += nrun;
        if (!host_only) {
            read_off.assign((size_t)nids + 1, 0);
            for (size_t r = 0; r < nrun; ++r) read_off[(size_t)recs[run_off[r]].sid + 1] = run_off[r + 1] - run_off[r];
            for (int i = 0; i < nids; ++i) read_off[(size_t)i + 1] += read_off[i];
            dev.resize((size_t)nids);
            uint64_t nh = 0;
            if (necat_trim_ranges(ctx, (const necat_m4*)recs.data(), read_off.data(), num_reads, min_ident_perc, min_ovlp_size, min_cov, min_size,
                                  (necat_clip_range*)dev.data(), &nh)) {
                fprintf(stderr, "oc2lcr: %s\n", necat_last_error(ctx));
                status = 1; break;
            }
        }
        for (size_t r = 0; r < nrun; ++r) {
            M4* m4v = recs.data() + run_off[r];
            const int sid = m4v[0].sid;
            if (!host_only && dev[(size_t)sid].how != kHost) { lcrv[(size_t)sid] = dev[(size_t)sid]; continue; }
            Clip c{0, 0, 0, kNone};
            if (decide_read(m4v, (int)(run_off[r + 1] - run_off[r]), min_ident_perc, min_ovlp_size, min_cov, &c) != kNone) lcrv[(size_t)sid] = c;
            ++n_host;
        }
    }
    if (ctx) necat_ctx_destroy(ctx);
    if (status) return status;
    OutFile out;
    if (!out.open(output, "w")) return 1;
    fprintf(out.f, "0\t0\t0\t0\n");
    for (int i = 1; i <= num_reads; ++i) {
        finish_clip(lcrv[(size_t)i], min_size);
        fprintf(out.f, "%d\t%d\t%d\t%d\n", i, lcrv[(size_t)i].left, lcrv[(size_t)i].right, lcrv[(size_t)i].size);
    }
    if (!out.commit()) return 1;
    fprintf(stderr, "oc2lcr: %d reads, %llu with overlaps, %llu decided on the host%s\n", num_reads, (unsigned long long)n_with_records,
            (unsigned long long)n_host, host_only ? " (NECAT_TRIM_HOST)" : "");
    return 0;
}
