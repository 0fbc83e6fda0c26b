// rescue_pair.h - the one formulation of the rescue pair's device jobs (DALIGNER around an anchor through k_dal_wave, then edlib's path over the range it found
// through nw_run): plain functions over plain numbers - a sequence's first base in its volume, its length, a strand, a slice of the subject, the anchor - that
// stage_dalign.inl, stage_nw.inl, stage_refmap.inl, stage_ctg_extend.inl and stage_cns.inl call, and that g++ builds for tests/host_core/check_dalign.cpp,
// check_rm_spec.cpp and check_pair_jobs.cpp, which add an offset to the positions to address word buffers of their own.  No HIP in this header.
// (asm_ends_core.h builds its tasks on the device and has an accept rule of its own: not here.)
#pragma once
#include "../../include/necat_hip.h"
#include "dal_core.h"
#include "nw_core.h"
#include "rescue.h"

namespace necat {
namespace pair {

// a sequence of `len` bases whose first is base `begin` of the words, from its base `from` on, as the kernels address it; rev: its reverse complement (`from` counts on that strand)
inline nw::Seq strand_seq(i64 begin, i64 len, int rev, i64 from = 0) { return rev ? nw::Seq{begin + len - 1 - from, -1, 1} : nw::Seq{begin + from, 1, 0}; }

// One job of the pair: the read on strand qdir against the slice [from, from + len) of the subject sequence, forward - a whole sequence is from = 0, len = its size -
// around the anchor (qoff on the read's strand, soff INSIDE THE SLICE).  qbegin / sbegin: the sequences' first bases; qid / sid: what the global half's job names.
struct Job { int32_t qid, qdir, sid; i64 qbegin, qlen, sbegin, from, len, qoff, soff; };

// the local half's task: the wave ends where the slice ends and never reads the subject's neighbours
inline dal::Task task_of(const Job& j)
{
    dal::Task T;
    T.a.s = strand_seq(j.qbegin, j.qlen, j.qdir); T.a.len = (int)j.qlen;
    T.b.s = strand_seq(j.sbegin, j.len, 0, j.from); T.b.len = (int)j.len;
    T.k0 = (int)(j.qoff - j.soff); T.mida = (int)(j.qoff + j.soff);
    return T;
}

// a job's range from its two tips, on the read's strand and the slice (rescue::Dalign::go's last lines)
inline void decode(const dal::Out& f, const dal::Out& b, int min_align_size, necat_dalign_result* r)
{
    r->qoff = b.a - b.y; r->qend = f.a - f.y; r->soff = b.y; r->send = f.y; r->diffs = f.d + b.d;
    const int asize = r->qend - r->qoff, bsize = r->send - r->soff;
    r->ok = asize >= min_align_size && bsize >= min_align_size;
    if (r->ok) r->ident_perc = 100.0 - 200.0 * r->diffs / (asize + bsize);
}
// .. and back: the host code's result as the pair of tips that decodes to it
inline void tips_of(const rescue::DalignResult& d, dal::Out* f, dal::Out* b)
{
    f->a = d.aepos + d.bepos; f->y = d.bepos; f->d = d.diffs; f->flag = 0;
    b->a = d.abpos + d.bbpos; b->y = d.bbpos; b->d = 0; b->flag = 0;
}

// the global half's job: a range on the slice is a range on the sequence, `from` further on; the difference count is the tolerance
inline necat_nw_job nw_job(int32_t qid, int32_t qdir, int32_t sid, i64 from, const necat_dalign_result& r)
{
    return necat_nw_job{qid, qdir, r.qoff, r.qend, sid, (int32_t)(from + r.soff), (int32_t)(from + r.send), r.diffs};
}
// .. and its accepted result back on the slice
inline void to_slice(i64 from, necat_nw_result* r) { r->toff -= (int32_t)from; r->tend -= (int32_t)from; }

}  // namespace pair
}  // namespace necat
