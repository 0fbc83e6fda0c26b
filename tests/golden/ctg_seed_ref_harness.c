/* ctg_seed_ref_harness.c - TEST ONLY, ours.  A main around the reference's MaximalExactMatchWorkData_Init / _FindCandidates (ctg_cns/mem_finder.c, chain_dp.c),
 * which are compiled from the reference's sources where they lie and never copied (tests/ctg_seed_cases.py: build_harness, tests/golden/make_golden_ctgseed.py).
 * Input, one file of binary records (little endian):
 *     'S' i32 size, size byte codes       a segment: every later read is seeded against it
 *     'R' i32 size, size byte codes       a read on its strand
 * Output per read, text: "J n_mems found qbeg qend sbeg send qoff soff score", then one line of n_mems x "qoff soff size" (chain_data->seeds after the call: the
 * sorted matches), with the constants of extend_ctg_m4s (cns_ctg_subseq.c: MaximalExactMatchWorkDataNew(15, 6, 20), ChainDpWorkDataNew(1, 200)). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctg_cns/mem_finder.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    MaximalExactMatchWorkData* mem = MaximalExactMatchWorkDataNew(15, 6, 20);
    ChainDpWorkData* chain = ChainDpWorkDataNew(1, 200);
    u8 *seg = NULL, *read = NULL;
    int c;
    while ((c = fgetc(in)) != EOF) {
        int n;
        if (fread(&n, 4, 1, in) != 1 || n < 0) return 3;
        u8* buf = (u8*)malloc((size_t)n + 16);
        if (n && fread(buf, 1, (size_t)n, in) != (size_t)n) return 3;
        if (c == 'S') {
            free(seg); seg = buf;
            MaximalExactMatchWorkData_Init(mem, seg, n);
        } else if (c == 'R') {
            free(read); read = buf;
            const int found = MaximalExactMatchWorkData_FindCandidates(mem, chain, read, n);
            GappedCandidate can;
            memset(&can, 0, sizeof can);
            if (found) can = kv_A(mem->can_list, 0);
            const size_t nm = kv_size(chain->seeds);
            printf("J %zu %d %d %d %d %d %d %d %d\n", nm, found, (int)can.qbeg, (int)can.qend, (int)can.sbeg, (int)can.send, (int)can.qoff, (int)can.soff, (int)can.score);
            for (size_t i = 0; i < nm; ++i) printf("%d %d %d ", kv_A(chain->seeds, i).qoff, kv_A(chain->seeds, i).soff, kv_A(chain->seeds, i).match_size);
            printf("\n");
        } else return 3;
    }
    return 0;
}
