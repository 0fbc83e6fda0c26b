// cns_rescue.h - the second half of cns_extension (consensus/consensus_aux.c:124-215) for oc2cns -r 1 (rescue_long_indels):
// a candidate whose block-wise extension failed, or stopped more than 200 bp short of the candidate's chained range in the
// query, is aligned again around its anchor with DALIGNER's local alignment and, if that gives an overlap, globally over exactly
// that range with edlib's path (rescue.h); the block-wise result is kept when the pair gives nothing.
//
// Host code as in the reference, run after a device pass on the candidates that need it (stage_cns.inl, which with NECAT_NW_DEVICE=1
// hands the second half to the kernels of necat_nw_path_batch instead, and with NECAT_DALIGN_DEVICE=1 the first half to
// necat_local_align_batch's; tests/host_core/check_cns.cpp plugs the pair behind the
// oracle's aligner).  No HIP in this header.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/necat_hip.h"
#include "host_bases.h"
#include "rescue.h"

namespace necat {
namespace cns {

// consensus_aux.c:152-159: is the block-wise result (ok / coordinates) final?
inline bool extension_short(const necat_candidate& c, const necat_alignment& a)
{
    if (!a.ok) return true;
    const int qbeg = (int)c.qbeg, qend = (int)c.qend;
    const int lhang = a.qoff > qbeg ? a.qoff - qbeg : 0;
    const int rhang = a.qend < qend ? qend - a.qend : 0;
    return lhang + rhang > 200;
}

// The pair in pieces, for callers that run the halves apart (stage_cns.inl: every candidate's local half on the host threads, then the global
// halves as one list of jobs, on the device or on the host threads).  qstrand: the query read on the candidate's strand, tseq: the template, codes 0..3.
// local half: DALIGNER around the anchor; true: dal.r holds the range and the difference count the global half is handed
inline bool rescue_local(rescue::Dalign& dal, const necat_candidate& c, const uint8_t* qstrand, const uint8_t* tseq, int min_align_size)
{
    return dal.go((const char*)qstrand, (int)c.qoff, (int)c.qsize, (const char*)tseq, (int)c.soff, (int)c.ssize, min_align_size);
}
// .. as a job of necat_nw_path_batch: the global path over exactly that range, with the difference count as the tolerance
inline necat_nw_job rescue_job(const necat_candidate& c, const rescue::DalignResult& d)
{
    return necat_nw_job{c.qid, c.qdir, d.abpos, d.aepos, c.sid, d.bbpos, d.bepos, d.diffs};
}
// one job on the host: edlib's path over the job's ranges.  *r: what necat_nw_path_batch reports for a job the host decided (how = 1);
// *packed: its columns, four to a byte (empty unless ok).  Also the certified fallback of necat_nw_path_batch (stage_nw.inl).
inline bool edlib_job(rescue::EdlibGo& E, const uint8_t* qstrand, const uint8_t* tseq, const necat_nw_job& j, int min_align_size, int match_size,
                      necat_nw_result* r, std::vector<uint8_t>* packed)
{
    memset(r, 0, sizeof *r);
    r->how = 1;
    packed->clear();
    if (!E.go((const char*)qstrand, j.qfrom, j.qto, (const char*)tseq, j.sfrom, j.sto, j.tolerance, min_align_size, match_size)) return false;
    r->ok = 1; r->qoff = E.qoff; r->qend = E.qend; r->toff = E.toff; r->tend = E.tend;
    r->align_size = (int32_t)E.query_align.size(); r->dist = E.dist; r->ident_perc = E.ident_perc;
    packed->resize((E.query_align.size() + 3) / 4);
    necat_host::pack_cols_of(E.query_align.size(), packed->data(), [&E](size_t i) { return necat_host::col_code(E.query_align[i], E.target_align[i]); });
    return true;
}
// an accepted job's result over the block-wise one (consensus_aux.c:186-199)
inline void take_rescued(const necat_nw_result& r, necat_alignment* a)
{
    a->ok = 1; a->qoff = r.qoff; a->qend = r.qend; a->toff = r.toff; a->tend = r.tend;
    a->align_size = r.align_size; a->ident_perc = r.ident_perc;
}

// the pair on one candidate in the reference's order (tests/host_core/check_cns.cpp)
struct Rescuer {
    rescue::Dalign dal;
    rescue::EdlibGo edl;
    std::vector<uint8_t> cols, packed;      // the rescued alignment's columns, one code per column as in necat_onc_align_batch / four to a byte
    Rescuer(const rescue::DalignSpec& spec, double error) : dal(spec), edl(error) {}

    // True: *a and cols hold the pair's alignment (consensus_aux.c:170-199); false: the block-wise result stands.
    bool go(const necat_candidate& c, const uint8_t* qstrand, const uint8_t* tseq, int min_align_size, necat_alignment* a)
    {
        necat_nw_result r;
        if (!rescue_local(dal, c, qstrand, tseq, min_align_size) || !edlib_job(edl, qstrand, tseq, rescue_job(c, dal.r), min_align_size, 4, &r, &packed)) return false;
        take_rescued(r, a);
        cols.resize((size_t)r.align_size);
        for (size_t i = 0; i < cols.size(); ++i) cols[i] = necat_host::col_code(edl.query_align[i], edl.target_align[i]);
        return true;
    }
};

}  // namespace cns
}  // namespace necat
