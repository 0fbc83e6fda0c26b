/* ctg_ext_ref_harness.c - TEST ONLY, ours.  A logging shim around the calls the reference's cns_ctg_subseq (ctg_cns/cns_ctg_subseq.c) makes, linked with
 * -Wl,--wrap into the reference's objects, which are compiled from the reference's sources where they lie and never copied (tests/ctg_ext_cases.py:
 * build_harness, tests/golden/make_golden_ctgext.py).
 *
 * The shim writes one text line per call to $CTG_EXT_LOG (or stdout):
 *     B from size n            cns_ctg_subseq begins, then n lines "M qid qdir soff send" (the records as the caller handed them, in loop order)
 *     X qid strand             pdb_extract_sequence: the record passed the cap
 *     F found                  MaximalExactMatchWorkData_FindCandidates' return value
 *     A r qoff qend toff tend ident      onc_align's return value and what it leaves in OcAlignData
 *     D r qb qe tb te diffs              ocda_go's and its path
 *     L r qoff qend toff tend ident      edlib_go's and what it leaves in FullEdlibAlignData
 *     T qoff qend toff tend n            add_align_tags, then the query line and the target line (n characters each)
 *     Z                        cns_ctg_subseq is over
 * Doubles are printed with %.17g.
 *
 * Without -DCTG_EXT_SHIM there is a main too (with it the file is linked into the reference's ctgcns program in place of nothing: the program's own main runs).
 * It reads one file of binary records (little endian):
 *     'R' i32 size, size byte codes               a read is added to the PackedDB
 *     'S' i64 from, i32 size, size byte codes     the segment
 *     'M' i32 qid, i32 qdir, i64 soff, i64 send   a record of the segment
 *     'G'                                         cns_ctg_subseq on (reads, segment, records so far); the records are dropped
 *     'E'                                         every record so far on its own, no cap: the read extracted, seeded, cns_extension called as extend_ctg_m4s calls
 *                                                 it; "J k" before record k, "C r qoff qend toff tend ident n" and the two gapped strings after it (r = 0: no
 *                                                 strings); the records are dropped */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctg_cns/cns_ctg_subseq.h"
#include "ctg_cns/chain_dp.h"
#include "ctg_cns/mem_finder.h"
#include "ctg_cns/fc_correct_one_read.h"
#include "gapped_align/oc_aligner.h"
#include "gapped_align/oc_daligner.h"
#include "edlib/edlib_wrapper.h"

static FILE* shim_log(void)
{
    static FILE* f = NULL;
    if (!f) { const char* p = getenv("CTG_EXT_LOG"); f = p ? fopen(p, "wb") : stdout; }
    return f;
}

void __real_cns_ctg_subseq(PackedDB* reads, u8* ctg_subseq, const idx ctg_subseq_offset, const int ctg_subseq_size, M4Record* m4_array, const int m4_count, kstring_t* cns_ctg);
void __wrap_cns_ctg_subseq(PackedDB* reads, u8* ctg_subseq, const idx ctg_subseq_offset, const int ctg_subseq_size, M4Record* m4_array, const int m4_count, kstring_t* cns_ctg)
{
    FILE* f = shim_log();
    fprintf(f, "B %ld %d %d\n", (long)ctg_subseq_offset, ctg_subseq_size, m4_count);
    for (int i = 0; i < m4_count; ++i) fprintf(f, "M %d %d %ld %ld\n", m4_array[i].qid, m4_array[i].qdir, (long)m4_array[i].soff, (long)m4_array[i].send);
    __real_cns_ctg_subseq(reads, ctg_subseq, ctg_subseq_offset, ctg_subseq_size, m4_array, m4_count, cns_ctg);
    fprintf(f, "Z\n");
    fflush(f);
}

void __real_pdb_extract_sequence(PackedDB* pdb, const idx i, const int strand, kstring_t* s);
void __wrap_pdb_extract_sequence(PackedDB* pdb, const idx i, const int strand, kstring_t* s)
{
    fprintf(shim_log(), "X %d %d\n", (int)i, strand);
    __real_pdb_extract_sequence(pdb, i, strand, s);
}

int __real_MaximalExactMatchWorkData_FindCandidates(MaximalExactMatchWorkData* data, ChainDpWorkData* chain_data, const u8* read, const int read_size);
int __wrap_MaximalExactMatchWorkData_FindCandidates(MaximalExactMatchWorkData* data, ChainDpWorkData* chain_data, const u8* read, const int read_size)
{
    const int r = __real_MaximalExactMatchWorkData_FindCandidates(data, chain_data, read, read_size);
    fprintf(shim_log(), "F %d\n", r);
    return r;
}

BOOL __real_onc_align(const char* query, const int query_start, const int query_size, const char* target, const int target_start, const int target_size, OcAlignData* oca_data,
                      const int block_size, const int min_align_size, const int tail_match_len);
BOOL __wrap_onc_align(const char* query, const int query_start, const int query_size, const char* target, const int target_start, const int target_size, OcAlignData* oca_data,
                      const int block_size, const int min_align_size, const int tail_match_len)
{
    const BOOL r = __real_onc_align(query, query_start, query_size, target, target_start, target_size, oca_data, block_size, min_align_size, tail_match_len);
    fprintf(shim_log(), "A %d %d %d %d %d %.17g\n", (int)r, oca_data->qoff, oca_data->qend, oca_data->toff, oca_data->tend, oca_data->ident_perc);
    return r;
}

BOOL __real_ocda_go(const char* query, const int query_start, const int query_size, const char* target, const int target_start, const int target_size, OcDalignData* ocda,
                    const int min_align_size);
BOOL __wrap_ocda_go(const char* query, const int query_start, const int query_size, const char* target, const int target_start, const int target_size, OcDalignData* ocda,
                    const int min_align_size)
{
    const BOOL r = __real_ocda_go(query, query_start, query_size, target, target_start, target_size, ocda, min_align_size);
    fprintf(shim_log(), "D %d %d %d %d %d %d\n", (int)r, ocda->path.abpos, ocda->path.aepos, ocda->path.bbpos, ocda->path.bepos, ocda->path.diffs);
    return r;
}

int __real_edlib_go(const char* query, const int query_from, const int query_to, const char* target, const int target_from, const int target_to, FullEdlibAlignData* align_data,
                    const int tolerance, const int min_align_size, const BOOL find_path, const int kMatchSize);
int __wrap_edlib_go(const char* query, const int query_from, const int query_to, const char* target, const int target_from, const int target_to, FullEdlibAlignData* align_data,
                    const int tolerance, const int min_align_size, const BOOL find_path, const int kMatchSize)
{
    const int r = __real_edlib_go(query, query_from, query_to, target, target_from, target_to, align_data, tolerance, min_align_size, find_path, kMatchSize);
    fprintf(shim_log(), "L %d %d %d %d %d %.17g\n", r, align_data->qoff, align_data->qend, align_data->toff, align_data->tend, align_data->ident_perc);
    return r;
}

void __real_add_align_tags(const char* qaln, const char* taln, const cns_pos_t aln_size, const cns_pos_t qoff, const cns_pos_t qend, const cns_pos_t toff, const cns_pos_t tend,
                           double weight, vec_align_tag* tags);
void __wrap_add_align_tags(const char* qaln, const char* taln, const cns_pos_t aln_size, const cns_pos_t qoff, const cns_pos_t qend, const cns_pos_t toff, const cns_pos_t tend,
                           double weight, vec_align_tag* tags)
{
    FILE* f = shim_log();
    fprintf(f, "T %d %d %d %d %d\n", qoff, qend, toff, tend, aln_size);
    fwrite(qaln, 1, (size_t)aln_size, f); fputc('\n', f);
    fwrite(taln, 1, (size_t)aln_size, f); fputc('\n', f);
    __real_add_align_tags(qaln, taln, aln_size, qoff, qend, toff, tend, weight, tags);
}

#ifndef CTG_EXT_SHIM
/* external in cns_ctg_subseq.o, declared in no header */
BOOL cns_extension(GappedCandidate* can, OcAlignData* align_data, OcDalignData* dalign_data, FullEdlibAlignData* falign_data, const char* query, const char* target,
                   int min_align_size, BOOL rescue_long_indels, int* qoff, int* qend, int* toff, int* tend, double* ident_perc, kstring_t** qaln, kstring_t** taln);

typedef struct { int qid, qdir; long soff, send; } Rec;

static void each_alone(PackedDB* reads, const u8* seg, int size, const Rec* rec, int n)
{
    FILE* f = shim_log();
    /* the constants and the calls of extend_ctg_m4s, cns_ctg_subseq.c:128-133, :153-177 */
    MaximalExactMatchWorkData* mem = MaximalExactMatchWorkDataNew(CNS_MEM_KMER_SIZE, CNS_MEM_WINDOW_SIZE, CNS_MEM_MEM_SIZE);
    MaximalExactMatchWorkData_Init(mem, seg, size);
    ChainDpWorkData* chain = ChainDpWorkDataNew(1, 200);
    OcAlignData* ad = new_OcAlignData(0.5);
    OcDalignData* dd = new_OcDalignData(0.5);
    FullEdlibAlignData* fd = new_FullEdlibAlignData(0.5);
    new_kstring(read);
    for (int k = 0; k < n; ++k) {
        fprintf(f, "J %d\n", k);
        pdb_extract_sequence(reads, rec[k].qid, rec[k].qdir, &read);
        const u8* rs = (const u8*)kstr_data(read);
        const int rl = (int)kstr_size(read);
        if (!MaximalExactMatchWorkData_FindCandidates(mem, chain, rs, rl)) continue;
        GappedCandidate can = kv_A(mem->can_list, 0);
        can.qsize = rl; can.ssize = size;
        int qb = 0, qe = 0, sb = 0, se = 0;
        double ident = 0.0;
        kstring_t *qa = NULL, *sa = NULL;
        const int r = cns_extension(&can, ad, dd, fd, (const char*)rs, (const char*)seg, 1000, 1, &qb, &qe, &sb, &se, &ident, &qa, &sa);
        if (!r) { fprintf(f, "C 0 0 0 0 0 0 0\n"); continue; }
        fprintf(f, "C 1 %d %d %d %d %.17g %d\n", qb, qe, sb, se, ident, (int)kstr_size(*qa));
        fwrite(kstr_data(*qa), 1, kstr_size(*qa), f); fputc('\n', f);
        fwrite(kstr_data(*sa), 1, kstr_size(*sa), f); fputc('\n', f);
    }
    MaximalExactMatchWorkDataFree(mem);
    ChainDpWorkDataFree(chain);
    free_OcAlignData(ad);
    free_OcDalignData(dd);
    free_FullEdlibAlignData(fd);
    free_kstring(read);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    PackedDB* reads = new_PackedDB();
    u8* seg = NULL;
    long from = 0;
    int size = 0, n = 0, cap = 0, c;
    Rec* rec = NULL;
    new_kstring(txt);
    new_kstring(cns);
    while ((c = fgetc(in)) != EOF) {
        if (c == 'R' || c == 'S') {
            int m;
            if (c == 'S' && fread(&from, 8, 1, in) != 1) return 3;
            if (fread(&m, 4, 1, in) != 1 || m < 0) return 3;
            u8* buf = (u8*)malloc((size_t)m + 16);
            if (m && fread(buf, 1, (size_t)m, in) != (size_t)m) return 3;
            if (c == 'S') { free(seg); seg = buf; size = m; continue; }
            kstr_clear(txt);
            for (int i = 0; i < m; ++i) kputc("ACGT"[buf[i] & 3], &txt);
            pdb_add_string_seq(reads, &txt, 0);
            free(buf);
        } else if (c == 'M') {
            if (n == cap) { cap = cap ? 2 * cap : 64; rec = (Rec*)realloc(rec, (size_t)cap * sizeof(Rec)); }
            if (fread(&rec[n].qid, 4, 1, in) != 1 || fread(&rec[n].qdir, 4, 1, in) != 1 || fread(&rec[n].soff, 8, 1, in) != 1 || fread(&rec[n].send, 8, 1, in) != 1) return 3;
            ++n;
        } else if (c == 'G') {
            M4Record* m4 = (M4Record*)calloc((size_t)n + 1, sizeof(M4Record));
            for (int i = 0; i < n; ++i) {
                m4[i].qid = rec[i].qid; m4[i].qdir = rec[i].qdir; m4[i].soff = (idx)rec[i].soff; m4[i].send = (idx)rec[i].send; m4[i].sdir = FWD;
                m4[i].qsize = PDB_SEQ_SIZE(reads, rec[i].qid);
            }
            u8* copy = (u8*)malloc((size_t)size + 16);          /* (cns_ctg_subseq decodes its segment in place) */
            memcpy(copy, seg, (size_t)size);
            kstr_clear(cns);
            cns_ctg_subseq(reads, copy, (idx)from, size, m4, n, &cns);
            free(copy); free(m4);
            n = 0;
        } else if (c == 'E') {
            each_alone(reads, seg, size, rec, n);
            n = 0;
        } else return 3;
    }
    return 0;
}
#endif
