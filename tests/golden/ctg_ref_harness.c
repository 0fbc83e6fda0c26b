/* ctg_ref_harness.c - TEST ONLY, ours.  Two small programs around the reference's add_align_tags and get_cns_from_align_tags (ctg_cns/fc_correct_one_read.c), which are
 * compiled from the reference's sources where they lie and never copied (tests/ctg_cases.py: build_harness, tests/golden/make_golden_ctgcns.py).
 *
 * Without -DCTG_SHIM: a main that reads overlaps as gapped strings and hands them to the two functions:
 *     O qid qdir qoff qend toff tend n        then the query line and the target line (n characters each)
 *     S size min_cov                          consensus of the overlaps since the last S: answers "C <cns_seq>" and "T <t_pos ...>"
 * With -DCTG_SHIM: no main; linked into the reference's ctgcns with -Wl,--wrap=add_align_tags,--wrap=get_cns_from_align_tags,--wrap=pdb_extract_sequence it
 * writes the same lines to the file $CTG_SHIM_LOG for every call the program makes (qid / qdir: the read the program extracted last). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctg_cns/fc_correct_one_read.h"
#include "common/packed_db.h"

static void answer(FILE* out, CnsData* d)
{
    fprintf(out, "C ");
    fwrite(kstr_data(d->cns_seq), 1, kstr_size(d->cns_seq), out);
    fprintf(out, "\nT");
    for (size_t i = 0; i < kv_size(d->t_pos); ++i) fprintf(out, " %d", kv_A(d->t_pos, i));
    fprintf(out, "\n");
}

#ifndef CTG_SHIM
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    CnsData* d = cns_data_new();
    char *line = NULL, *qa = NULL, *ta = NULL;
    size_t lc = 0, qc = 0, tc = 0;
    while (getline(&line, &lc, in) > 0) {
        if (line[0] == 'O') {
            int qid, qdir, qoff, qend, toff, tend, n;
            if (sscanf(line + 2, "%d %d %d %d %d %d %d", &qid, &qdir, &qoff, &qend, &toff, &tend, &n) != 7) return 3;
            if (getline(&qa, &qc, in) < n || getline(&ta, &tc, in) < n) return 3;
            add_align_tags(qa, ta, n, qoff, qend, toff, tend, 1.0, &d->tags);
        } else if (line[0] == 'S') {
            int size, min_cov;
            if (sscanf(line + 2, "%d %d", &size, &min_cov) != 2) return 3;
            get_cns_from_align_tags(d, size, min_cov);
            answer(stdout, d);
            cns_data_clear(d);
        }
    }
    return 0;
}
#else
static FILE* shim_log(void)
{
    static FILE* f = NULL;
    if (!f) f = fopen(getenv("CTG_SHIM_LOG"), "wb");
    return f;
}
static int last_id = -1, last_strand = 0;

void __real_pdb_extract_sequence(PackedDB* pdb, const idx i, const int strand, kstring_t* s);
void __wrap_pdb_extract_sequence(PackedDB* pdb, const idx i, const int strand, kstring_t* s)
{
    last_id = (int)i; last_strand = strand;
    __real_pdb_extract_sequence(pdb, i, strand, s);
}

void __real_add_align_tags(const char* qaln, const char* taln, const cns_pos_t aln_size, const cns_pos_t qoff, const cns_pos_t qend, const cns_pos_t toff, const cns_pos_t tend,
                           double weight, vec_align_tag* tags);
void __wrap_add_align_tags(const char* qaln, const char* taln, const cns_pos_t aln_size, const cns_pos_t qoff, const cns_pos_t qend, const cns_pos_t toff, const cns_pos_t tend,
                           double weight, vec_align_tag* tags)
{
    FILE* f = shim_log();
    fprintf(f, "O %d %d %d %d %d %d %d\n", last_id, last_strand, qoff, qend, toff, tend, aln_size);
    fwrite(qaln, 1, (size_t)aln_size, f); fputc('\n', f);
    fwrite(taln, 1, (size_t)aln_size, f); fputc('\n', f);
    __real_add_align_tags(qaln, taln, aln_size, qoff, qend, toff, tend, weight, tags);
}

void __real_get_cns_from_align_tags(CnsData* data, cns_pos_t target_size, cns_pos_t min_cov);
void __wrap_get_cns_from_align_tags(CnsData* data, cns_pos_t target_size, cns_pos_t min_cov)
{
    FILE* f = shim_log();
    __real_get_cns_from_align_tags(data, target_size, min_cov);
    fprintf(f, "S %d %d\n", target_size, min_cov);
    answer(f, data);
    fflush(f);
}
#endif
