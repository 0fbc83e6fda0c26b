// oc2etr - drop-in for the read extractor of NECAT's read trimming stage (reference: trim_bases/extract_trimmed_reads.c), the program after oc2lcr
// in the default pipeline (pipeline/necat.pl).  Host code: one pass over the reads, one over the records.
//
//   oc2etr lcrv_path input_reads all_ovlps complete_reads trimmed_reads complete_ovlps
//
// lcrv_path = oc2lcr's ranges; input_reads = FASTA / FASTQ, plain or gzip, the i-th record being read i, named by its number (oc2renumberSeqs).
// A read whose range leaves at most 20 bases off either end is complete and written whole to complete_reads; another read with a range is
// written as [left, right) to trimmed_reads; a read without one is dropped.  Names are written up to their first white space.  complete_ovlps =
// the records of all_ovlps (binary, 96 bytes) whose two reads are both complete, as text with the reads' names (DUMP_ASM_M4_HDR_ID).
// Where the reference asserts (a range that does not fit its read, a name that is not the read's number) this program stops with exit status 1.
#include "../../include/necat_hip.h"
#include "host_fmt.h"
#include "seq_reader.h"
#include "trim_io.h"

using namespace necat_host::trim;

static_assert(sizeof(necat_m4) == sizeof(M4), "M4Record");

int main(int argc, char** argv)
{
    if (argc != 7) {
        fprintf(stderr, "USAGE:\n");
        fprintf(stderr, "%s lcrv_path input_reads all_ovlps complete_reads trimmed_reads complete_ovlps\n", argv[0]);
        return 1;
    }
    const char* lcrv_path = argv[1];
    const char* input_reads = argv[2];
    const char* all_ovlps = argv[3];
    std::vector<Clip> lcrv;                                      // load_lcrs, largest_cover_range.c:27-43: row i = read i (row 0 is the header row)
    {
        FILE* in = fopen(lcrv_path, "r");
        if (!in) { fprintf(stderr, "cannot open %s\n", lcrv_path); return 1; }
        char line[256];
        while (fgets(line, sizeof line, in)) {
            int id; Clip c{0, 0, 0, 0};
            if (sscanf(line, "%d%d%d%d", &id, &c.left, &c.right, &c.size) != 4) { fprintf(stderr, "%s: cannot parse '%s'\n", lcrv_path, line); fclose(in); return 1; }
            lcrv.push_back(c);
        }
        fclose(in);
    }
    uint64_t nrec = 0;
    if (!record_count(all_ovlps, &nrec)) return 1;
    necat_host::Reader rd;
    rd.ks.f = gzopen(input_reads, "r");
    if (!rd.ks.f) { fprintf(stderr, "cannot open %s\n", input_reads); return 1; }
    OutFile complete_out, trimmed_out, ovlp_out;
    if (!complete_out.open(argv[4], "w") || !trimmed_out.open(argv[5], "w") || !ovlp_out.open(argv[6], "w")) { gzclose(rd.ks.f); return 1; }
    auto is_complete = [&](const Clip& c) { return range_is_complete(c.left, c.right, c.size); };
    std::vector<std::string> headers(1);                         // by read id
    size_t read_id = 0;
    int r;
    while ((r = rd.next()) >= 0) {
        ++read_id;
        size_t k = 0;
        while (k < rd.name.size() && !isspace((unsigned char)rd.name[k])) ++k;
        headers.push_back(rd.name.substr(0, k));
        if (read_id >= lcrv.size()) { fprintf(stderr, "oc2etr: read %zu has no range in %s\n", read_id, lcrv_path); gzclose(rd.ks.f); return 1; }
        const Clip& c = lcrv[read_id];
        if (c.left < 0) continue;
        if ((size_t)c.size != rd.seq.size()) { fprintf(stderr, "oc2etr: read %zu has %zu bases, its range says %d\n", read_id, rd.seq.size(), c.size); gzclose(rd.ks.f); return 1; }
        const bool whole = is_complete(c);
        const int from = whole ? 0 : c.left, to = whole ? c.size : c.right;
        if (!(from >= 0 && from < to && to <= c.size)) { fprintf(stderr, "oc2etr: read %zu: range [%d, %d) of %d\n", read_id, from, to, c.size); gzclose(rd.ks.f); return 1; }
        FILE* out = whole ? complete_out.f : trimmed_out.f;
        fputc('>', out);
        fwrite(rd.name.data(), 1, rd.name.size(), out);
        fputc('\n', out);
        fwrite(rd.seq.data() + from, 1, (size_t)(to - from), out);
        fputc('\n', out);
    }
    const bool read_err = rd.ks.err || r == -2 || r == -3;
    gzclose(rd.ks.f);
    if (read_err) { fprintf(stderr, "oc2etr: %s is damaged\n", input_reads); return 1; }

    // dump_complete_m4s, extract_trimmed_reads.c:35-73
    FILE* in = fopen(all_ovlps, "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", all_ovlps); return 1; }
    necat_m4 m4;
    char line[2048];
    while (fread(&m4, sizeof m4, 1, in) == 1) {
        if (m4.qid < 0 || m4.sid < 0 || (size_t)m4.qid >= lcrv.size() || (size_t)m4.sid >= lcrv.size()) { fprintf(stderr, "oc2etr: record of reads %d, %d: no such range\n", m4.qid, m4.sid); fclose(in); return 1; }
        if (!(is_complete(lcrv[(size_t)m4.qid]) && is_complete(lcrv[(size_t)m4.sid]))) continue;
        bool ok = (size_t)m4.qid < headers.size() && (size_t)m4.sid < headers.size() && m4.qsize == (uint64_t)lcrv[(size_t)m4.qid].size && m4.ssize == (uint64_t)lcrv[(size_t)m4.sid].size;
        ok = ok && atoi(headers[(size_t)m4.qid].c_str()) == m4.qid && atoi(headers[(size_t)m4.sid].c_str()) == m4.sid;
        if (!ok) { fprintf(stderr, "oc2etr: record of reads %d, %d does not fit the reads (sizes or names)\n", m4.qid, m4.sid); fclose(in); return 1; }
        if (headers[(size_t)m4.qid].size() + headers[(size_t)m4.sid].size() + 400 > sizeof line) { fprintf(stderr, "oc2etr: read names too long\n"); fclose(in); return 1; }
        char* e = necat_host::put_m4(line, m4, headers[(size_t)m4.qid].c_str(), headers[(size_t)m4.sid].c_str());
        fwrite(line, 1, (size_t)(e - line), ovlp_out.f);
    }
    fclose(in);
    bool ok = complete_out.commit();
    ok = trimmed_out.commit() && ok;
    ok = ovlp_out.commit() && ok;
    return ok ? 0 : 1;
}
