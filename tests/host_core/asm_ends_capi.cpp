// flat entry point over necat_amd/csrc/asm_core.h's Extender::ends for the GPU tests of necat_asm_map_batch (tests/test_gpu_asm_ends.py): hbn_map_extend on one
// block alignment given as its two gapped strings
#include "../../necat_amd/csrc/asm_core.h"

// query / target: byte codes 0 .. 3, the target ON ITS STRAND; io: qoff qend toff tend in, the same out followed by "left end extended", "right end extended";
// ident: the alignment's identity in, fix_ident_perc's out
extern "C" void mine_asm_ends(const unsigned char* query, int qsize, const unsigned char* target, int tsize, const char* qaln, const char* taln, int ncols, int* io, double* ident)
{
    static necat::asmpm::Extender ext;
    necat::asmpm::BlockAlignment a;
    a.qoff = io[0]; a.qend = io[1]; a.toff = io[2]; a.tend = io[3]; a.ident_perc = *ident;
    a.qaln.assign(qaln, (size_t)ncols); a.taln.assign(taln, (size_t)ncols);
    ext.ends(query, qsize, target, tsize, a);
    io[0] = a.qoff; io[1] = a.qend; io[2] = a.toff; io[3] = a.tend; io[4] = ext.last_ext[0]; io[5] = ext.last_ext[1];
    *ident = a.ident_perc;
}
