// oc2orderResults - drop-in for the last program of NECAT's read trimming stage (reference: trim_bases/order_results.c).  Host code.
//
//   oc2orderResults input_reads input_m4 output_reads output_m4
//
// input_reads = the complete and the trimmed reads (FASTA / FASTQ, plain or gzip) under the numbers they had before trimming; they are renumbered
// 1 .. in file order (">id", the sequence on one line), and the ids of the overlaps (12-column text, DUMP_ASM_M4) are rewritten to the new numbers.
// An overlap of a read that is not in input_reads is an error (the reference asserts), as is a line that does not parse.
#include "../../include/necat_hip.h"
#include "host_fmt.h"
#include "seq_reader.h"
#include "trim_io.h"

using namespace necat_host::trim;

int main(int argc, char** argv)
{
    if (argc != 5) {
        fprintf(stderr, "USAGE:\n");
        fprintf(stderr, "%s input_reads input_m4 output_reads output_m4\n", argv[0]);
        return 1;
    }
    const char* input_reads = argv[1];
    const char* input_m4 = argv[2];
    FILE* min = fopen(input_m4, "r");
    if (!min) { fprintf(stderr, "cannot open %s\n", input_m4); return 1; }
    necat_host::Reader rd;
    rd.ks.f = gzopen(input_reads, "r");
    if (!rd.ks.f) { fprintf(stderr, "cannot open %s\n", input_reads); fclose(min); return 1; }
    OutFile reads_out, m4_out;
    if (!reads_out.open(argv[3], "w") || !m4_out.open(argv[4], "w")) { gzclose(rd.ks.f); fclose(min); return 1; }
    // order_reads, order_results.c:36-63 (one pass: the map grows with the largest old number instead of being sized by a first pass)
    std::vector<int> id_maps;
    int id = 1, r;
    while ((r = rd.next()) >= 0) {
        const int oid = atoi(rd.name.c_str());
        if (oid < 0) { fprintf(stderr, "oc2orderResults: read name '%s' is not a read number\n", rd.name.c_str()); gzclose(rd.ks.f); fclose(min); return 1; }
        if ((size_t)oid >= id_maps.size()) id_maps.resize((size_t)oid + 1, -1);
        id_maps[(size_t)oid] = id;
        fprintf(reads_out.f, ">%d\n", id);
        ++id;
        fwrite(rd.seq.data(), 1, rd.seq.size(), reads_out.f);
        fputc('\n', reads_out.f);
    }
    const bool read_err = rd.ks.err || r == -2 || r == -3;
    gzclose(rd.ks.f);
    if (read_err) { fprintf(stderr, "oc2orderResults: %s is damaged\n", input_reads); fclose(min); return 1; }
    char line[4096], text[512];
    while (fgets(line, sizeof line, min)) {
        necat_m4 m4;
        memset(&m4, 0, sizeof m4);
        unsigned long qoff, qend, qsize, soff, send, ssize;
        if (sscanf(line, "%d%d%lf%d%d%lu%lu%lu%d%lu%lu%lu", &m4.qid, &m4.sid, &m4.ident_perc, &m4.vscore, &m4.qdir, &qoff, &qend, &qsize, &m4.sdir, &soff, &send, &ssize) != 12) {
            fprintf(stderr, "oc2orderResults: %s: cannot parse '%s'\n", input_m4, line); fclose(min); return 1;
        }
        m4.qoff = qoff; m4.qend = qend; m4.qsize = qsize; m4.soff = soff; m4.send = send; m4.ssize = ssize;
        auto mapped = [&](int old) { return old >= 0 && (size_t)old < id_maps.size() ? id_maps[(size_t)old] : -1; };
        const int q = mapped(m4.qid), s = mapped(m4.sid);
        if (q < 0 || s < 0) { fprintf(stderr, "oc2orderResults: overlap of reads %d, %d: not among the reads\n", m4.qid, m4.sid); fclose(min); return 1; }
        m4.qid = q; m4.sid = s;
        char* e = necat_host::put_m4(text, m4, nullptr, nullptr);
        fwrite(text, 1, (size_t)(e - text), m4_out.f);
    }
    fclose(min);
    bool ok = reads_out.commit();
    ok = m4_out.commit() && ok;
    return ok ? 0 : 1;
}
