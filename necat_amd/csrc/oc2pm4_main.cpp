// oc2pm4 - drop-in for the record partitioner of NECAT's read trimming stage (reference: trim_bases/pm4_main.c, pm4_aux.c), the program between
// `oc2asmpm -u 1` and oc2lcr in the default pipeline (pipeline/necat.pl: runTrimBasesFast).
//
//   oc2pm4 wrk_dir m4 error_cutoff num_threads
//
// `m4` = binary 96-byte M4 records of corrected reads.  A record whose identity reaches 100 - 100 * error_cutoff is kept under its subject as it is
// and, with query and subject exchanged and the new subject on the forward strand, under its query.  Reads are grouped in partitions of 100 000
// ids, 100 partition files open per pass over the input.  Output: m4.p<i> for every partition (empty ones included) and m4.partitions.
//
// The order inside a partition file is part of the contract: oc2lcr's answer for a few reads depends on the order their records are held in (equal
// keys under klib's unstable sort, trim_core.h), so this program does what the reference does - chunks of 256 MB / 96 records; in a chunk the
// survivors in input order, then the exchanged copies appended; klib's introsort by subject id; one run per partition appended to its file - and
// is byte-identical to it at num_threads = 1.  With more threads the chunks are appended in the order the threads finish, as in the reference: the
// same records per file.  Host code: the stage is one sequential read per pass.  (The same transformation on records still in memory:
// necat_trim_partition, include/necat_hip.h.)
//
// NECAT_PM4_CHUNK overrides the chunk size in records (tests only; the reference's is a constant, pm4_aux.c:89-90).
#include <mutex>
#include <thread>

#include "trim_io.h"

using namespace necat_host::trim;

namespace {

struct Job {
    FILE* in = nullptr;
    std::mutex read_lock, write_lock;
    std::vector<OutFile>* out = nullptr;
    int min_read_id = 0, max_read_id = 0, batch_size = 0;
    double cutoff = 0;
    size_t chunk = 0;
    bool ok = true;
};

// pm4_thread_func, pm4_aux.c:129-196
void worker(Job* J)
{
    std::vector<M4> v(2 * J->chunk);
    std::vector<size_t> idx_range;
    auto in_range = [&](int id) { return id >= J->min_read_id && id < J->max_read_id; };
    for (;;) {
        size_t n;
        {
            std::lock_guard<std::mutex> lk(J->read_lock);
            n = fread(v.data(), sizeof(M4), J->chunk, J->in);
        }
        if (n == 0) break;
        M4* m4s = v.data();
        size_t m = 0;
        for (size_t i = 0; i < n; ++i) {
            if (m4s[i].ident_perc < J->cutoff) continue;
            if (in_range(m4s[i].qid) || in_range(m4s[i].sid)) m4s[m++] = m4s[i];
        }
        if (m == 0) continue;
        n = m;
        for (size_t i = 0; i < m; ++i) {
            const bool sid_is_in = in_range(m4s[i].sid);
            if (in_range(m4s[i].qid)) {
                const M4 x = exchanged(m4s[i]);
                if (sid_is_in) m4s[n++] = x;
                else m4s[i] = x;
            }
        }
        necat_host::klib_introsort(n, m4s, SidLess());
        idx_range.clear();
        size_t i = 0;
        while (i < n) {
            const int sid_to = (m4s[i].sid / J->batch_size) * J->batch_size + J->batch_size;
            size_t j = i + 1;
            while (j < n && m4s[j].sid < sid_to) ++j;
            idx_range.push_back(i);
            i = j;
        }
        idx_range.push_back(n);
        std::lock_guard<std::mutex> lk(J->write_lock);
        for (size_t r = 0; r + 1 < idx_range.size(); ++r) {
            const size_t from = idx_range[r], cnt = idx_range[r + 1] - from;
            const int bid = (m4s[from].sid - J->min_read_id) / J->batch_size;
            if (bid < 0 || bid >= (int)J->out->size() || fwrite(m4s + from, sizeof(M4), cnt, (*J->out)[bid].f) != cnt) J->ok = false;
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 5) {
        fprintf(stderr, "USAGE:\n");
        fprintf(stderr, "%s wrk_dir m4 error_cutoff num_threads\n", argv[0]);
        return 1;
    }
    const char* wrk_dir = argv[1];
    const char* m4_path = argv[2];
    const double min_ident_perc = 100.0 - 100.0 * atof(argv[3]);
    int num_threads = atoi(argv[4]);
    if (num_threads > 8) num_threads = 8;
    if (num_threads < 1) num_threads = 1;
    const int num_dumpped_files = 100, partition_size = 100000;          // pm4_main.c:22-23
    int num_reads = 0;
    uint64_t nrec = 0;
    if (!load_num_reads(wrk_dir, &num_reads) || !record_count(m4_path, &nrec)) return 1;
    const int num_batches = (num_reads + partition_size - 1) / partition_size;
    Job J;
    J.batch_size = partition_size;
    J.cutoff = min_ident_perc;
    J.chunk = ((size_t)256 * 1024 * 1024) / sizeof(M4);
    if (const char* e = getenv("NECAT_PM4_CHUNK")) { if (atoll(e) > 0) J.chunk = (size_t)atoll(e); }
    if (J.chunk > nrec + 1) J.chunk = (size_t)nrec + 1;                  // the buffer, not the chunking: a smaller file is one chunk either way
    std::vector<std::vector<OutFile>> all;
    bool ok = true;
    for (int sfid = 0; ok && sfid < num_batches; sfid += num_dumpped_files) {
        const int efid = sfid + num_dumpped_files < num_batches ? sfid + num_dumpped_files : num_batches;
        all.emplace_back(efid - sfid);
        std::vector<OutFile>& out = all.back();
        for (int i = sfid; ok && i < efid; ++i) ok = out[i - sfid].open(partition_name(m4_path, i), "wb");
        if (!ok) break;
        J.min_read_id = sfid * partition_size; J.max_read_id = efid * partition_size;
        J.out = &out;
        J.in = fopen(m4_path, "rb");
        if (!J.in) { fprintf(stderr, "cannot open %s\n", m4_path); ok = false; break; }
        std::vector<std::thread> th;
        for (int t = 0; t < num_threads; ++t) th.emplace_back(worker, &J);
        for (auto& t : th) t.join();
        ok = J.ok && !ferror(J.in);
        fclose(J.in);
        for (auto& o : out) if (fflush(o.f) != 0) ok = false;
        for (auto& o : out) { fclose(o.f); o.f = nullptr; }              // at most 100 files open at a time; renamed when every pass is done
    }
    OutFile index;
    if (ok) ok = index.open(std::string(m4_path) + ".partitions", "w");
    if (ok) fprintf(index.f, "%d\n", num_batches);
    if (!ok) {
        fprintf(stderr, "oc2pm4: failed, no partition file written\n");
        for (auto& pass : all) for (auto& o : pass) o.discard();
        index.discard();
        return 1;
    }
    for (auto& pass : all) for (auto& o : pass) {
        if (rename((o.path + ".part").c_str(), o.path.c_str()) != 0) { fprintf(stderr, "cannot rename %s.part\n", o.path.c_str()); return 1; }
        o.path.clear();
    }
    return index.commit() ? 0 : 1;
}
