// asm_ends_core.h - oc2asmpm's end extension (hbn_map_extend, asm_pm/hbn_align.c:282-326; asm_core.h Extender::ends / ends_packed) for the device: what happens
// to a block alignment before and after its up to two DALIGNER jobs, per anchor, written so that g++ builds the same functions for a CPU model that runs them
// lane by lane (tests/host_core/check_asm_ends.cpp).
//
//   plan_ends    from the anchor's finished ExtTask: `ok` and the identity cut, the two hang tests, the scan of the alignment's columns from either end to the
//                first run of 8 equal ones, the unequal columns outside [from, to), and the dal::Tasks of the two ends (dal_core.h: prefixes / suffixes of the read
//                and of the subject on strand sdir)
//   finish_ends  the acceptance tests on the waves' tips, fix_ident_perc, the strand turn, the record
// The columns are read where the block aligner left them: the task's region of 2-bit columns (ExtTask::ops_base), left stream [s_lfrom, s_lto) reversed, then right
// stream [s_lto + s_rfrom, s_lto + s_rto).  Everything is integers but the identities: one IEEE division each, in the host's own expression.
#pragma once
#include "../../include/necat_hip.h"
#include "dal_core.h"
#include "ext_core.h"

namespace necat {
namespace aends {

constexpr int kMaxHang = 300, kMatchSize = 8;                  // hbn_align.c:10-11
// Plan::state: the alignment's bits, then per side (0 left, 1 right) the side's bits shifted by side_shift
enum { kOk = 1, kLowIdent = 2, kAlive = 4 };
enum { kHang0 = 1, kHangLong = 2, kTried = 4, kNoRun = 8, kJob = 16 };
NECAT_HD int side_shift(int side) { return 8 + 8 * side; }

// an anchor between the two kernels.  from / to: fix_ident_perc's range; uneq: the unequal columns of [0, from) and [to, n) (counted when from < to);
// (qls, tls) / (qrs, trs): where the end's DALIGNER job is anchored; job[side]: the job's index
struct Plan { i32 state, from, to, uneq, qls, tls, qrs, trs, job[2]; };

// what the device counts (one u32 each): C_JOBS is also the job allocator
enum { C_JOBS = 0, C_OK, C_LOW_IDENT, C_TRIED, C_EXTENDED = C_TRIED + 2, C_HANG0 = C_EXTENDED + 2, C_HANG_LONG = C_HANG0 + 2, C_NO_RUN = C_HANG_LONG + 2, C_COUNT = C_NO_RUN + 2 };

NECAT_HD int base_of(const u64* bases, i64 g) { return (int)((bases[g >> 5] >> ((g & 31) * 2)) & 3); }
NECAT_HD int query_at(const u64* qbases, const ExtTask& t, int p) { return base_of(qbases, t.q_g0 + p); }                    // the read is forward
NECAT_HD int subject_at(const u64* sbases, const ExtTask& t, int p)                                                          // position p of strand sdir
{
    return t.sdir ? 3 - base_of(sbases, t.s_g0 + t.slen - 1 - p) : base_of(sbases, t.s_g0 + p);
}
// column j of the final alignment: 0 a base of both, 1 a query base against a gap, 2 a subject base against a gap
NECAT_HD int op_at(const ExtTask& t, const u64* reg, int j)
{
    const int nl = t.s_lto - t.s_lfrom;
    const u32 src = j < nl ? (u32)(t.s_lto - 1 - j) : (u32)(t.s_lto + t.s_rfrom + (j - nl));
    return (int)((reg[src >> 5] >> ((src & 31) * 2)) & 3);
}

NECAT_HD dal::DSeq slice(i64 g0, int dir, int comp, int len) { dal::DSeq s; s.s.g0 = g0; s.s.dir = dir; s.s.comp = comp; s.len = len; return s; }
// [from, from + len) of the subject on strand sdir
NECAT_HD dal::DSeq subject_slice(const ExtTask& t, int from, int len)
{
    return t.sdir ? slice(t.s_g0 + t.slen - 1 - from, -1, 1, len) : slice(t.s_g0 + from, +1, 0, len);
}

// Extender::ends_packed up to its two calls of DALIGNER.  qbases / sbases: the words of the reads' / the subjects' volume; reg: the task's column region.
// tasks[side] is written when the side's kJob bit is set.
NECAT_HD Plan plan_ends(const ExtTask& t, const u64* qbases, const u64* sbases, const u64* reg, int min_align_size, double min_ident_perc, dal::Task* tasks)
{
    Plan p;
    p.state = 0; p.from = 0; p.to = t.r_cols; p.uneq = 0; p.qls = p.tls = p.qrs = p.trs = 0; p.job[0] = p.job[1] = -1;
    const int n = t.r_cols;
    if (n < min_align_size) return p;
    p.state |= kOk;
    const double ident = n ? 100.0 * (double)t.r_mat / (double)n : 0.0;             // k_ext_alignment's
    if (!(ident >= min_ident_perc)) { p.state |= kLowIdent; return p; }
    p.state |= kAlive;
    const int qbeg = t.r_qoff, tbeg = t.r_toff, qend = t.r_qend, tend = t.r_tend;
    {   // left_extend (:88-176)
        const int ls = qbeg < tbeg ? qbeg : tbeg;
        int side = ls == 0 ? kHang0 : ls > kMaxHang ? kHangLong : kTried;
        if (side & kTried) {
            int run = 0, qi = 0, ti = 0, i = 0;
            for (; run < kMatchSize && i < n; ++i) {
                const int op = op_at(t, reg, i);
                const bool same = op == 0 && query_at(qbases, t, qbeg + qi) == subject_at(sbases, t, tbeg + ti);
                if (op != 2) ++qi;
                if (op != 1) ++ti;
                run = same ? run + 1 : 0;
            }
            if (run >= kMatchSize) {
                p.from = i + 1;                    // one column past the run, as the reference has it
                p.qls = qbeg + qi; p.tls = tbeg + ti;
                side |= kJob;
                dal::Task& T = tasks[0];
                T.a = slice(t.q_g0, +1, 0, p.qls); T.b = subject_slice(t, 0, p.tls);
                T.k0 = p.qls - p.tls; T.mida = p.qls + p.tls;
            } else side |= kNoRun;
        }
        p.state |= side << side_shift(0);
    }
    {   // right_extend (:178-262)
        const int qr = t.qlen - qend, tr = t.slen - tend, rs = qr < tr ? qr : tr;
        int side = rs == 0 ? kHang0 : rs > kMaxHang ? kHangLong : kTried;
        if (side & kTried) {
            int run = 0, qi = 0, ti = 0, i = n;
            while (i && run < kMatchSize) {
                --i;
                const int op = op_at(t, reg, i);
                if (op != 2) ++qi;
                if (op != 1) ++ti;
                const bool same = op == 0 && query_at(qbases, t, qend - qi) == subject_at(sbases, t, tend - ti);
                run = same ? run + 1 : 0;
            }
            if (run >= kMatchSize) {
                p.to = i;
                p.qrs = qend - qi; p.trs = tend - ti;
                side |= kJob;
                dal::Task& T = tasks[1];
                T.a = slice(t.q_g0 + p.qrs, +1, 0, t.qlen - p.qrs); T.b = subject_slice(t, p.trs, t.slen - p.trs);
                T.k0 = 0; T.mida = 0;
            } else side |= kNoRun;
        }
        p.state |= side << side_shift(1);
    }
    // fix_ident_perc's count (:264-280) is the alignment's unequal columns less those outside [from, to): the latter here, the former is n - r_mat
    const bool any_job = ((p.state >> side_shift(0)) | (p.state >> side_shift(1))) & kJob;
    if (any_job && p.from < p.to) {
        int q = qbeg, s = tbeg, u = 0;
        for (int i = 0; i < p.from; ++i) { const int op = op_at(t, reg, i); if (!(op == 0 && query_at(qbases, t, q) == subject_at(sbases, t, s))) ++u; q += op != 2; s += op != 1; }
        q = qend; s = tend;
        for (int i = n; i > p.to; --i) { const int op = op_at(t, reg, i - 1); q -= op != 2; s -= op != 1; if (!(op == 0 && query_at(qbases, t, q) == subject_at(sbases, t, s))) ++u; }
        p.uneq = u;
    }
    return p;
}

// asm_pm/daligner.c:37-105 with min_align_size 1 and min_ident_perc 0.0 on the two tips of a job (f: forward wave, b: reverse wave), as dal_run decodes them
struct Local { int ok, abpos, aepos, bbpos, bepos, diffs; };
NECAT_HD Local local_of(const dal::Out& f, const dal::Out& b)
{
    Local r;
    r.abpos = b.a - b.y; r.aepos = f.a - f.y; r.bbpos = b.y; r.bepos = f.y; r.diffs = f.d + b.d;
    const int asize = r.aepos - r.abpos, bsize = r.bepos - r.bbpos;
    r.ok = asize >= 1 && bsize >= 1;
    if (r.ok) { const double ident = 100.0 - 200.0 * r.diffs / (asize + bsize); r.ok = ident >= 0.0; }
    return r;
}

// The rest of Extender::ends_packed and the record of BatchMapper::finish_packed (ids and the chain's score are the caller's).  outs: the jobs' tips, two per job.
// ext[side]: the side was extended.  Returns false when the anchor has no record.
NECAT_HD bool finish_ends(const ExtTask& t, const Plan& p, const dal::Out* outs, i32 qext, i32 sext, necat_m4* m, int* ext)
{
    ext[0] = ext[1] = 0;
    if (!(p.state & kAlive)) return false;
    const int n = t.r_cols;
    int qbeg = t.r_qoff, tbeg = t.r_toff, qend = t.r_qend, tend = t.r_tend, left_dist = 0, right_dist = 0;
    if ((p.state >> side_shift(0)) & kJob) {
        const Local r = local_of(outs[2 * p.job[0]], outs[2 * p.job[0] + 1]);
        if (r.ok && r.aepos == p.qls && r.bepos == p.tls) { qbeg = r.abpos; tbeg = r.bbpos; left_dist = r.diffs; ext[0] = 1; }
    }
    if ((p.state >> side_shift(1)) & kJob) {
        const Local r = local_of(outs[2 * p.job[1]], outs[2 * p.job[1] + 1]);
        if (r.ok && r.abpos == 0 && r.bbpos == 0) { qend = p.qrs + r.aepos; tend = p.trs + r.bepos; right_dist = r.diffs; ext[1] = 1; }
    }
    double ident = n ? 100.0 * (double)t.r_mat / (double)n : 0.0;
    if (ext[0] || ext[1]) {
        int diff = left_dist + right_dist;
        if (p.from < p.to) diff += n - t.r_mat - p.uneq;
        ident = 100.0 - 200.0 * diff / (qend + tend - qbeg - tbeg);
    }
    m->qid = 0; m->qdir = 0; m->qoff = (u64)qbeg; m->qend = (u64)qend; m->qext = (u64)qext; m->qsize = (u64)t.qlen;
    m->sid = 0; m->sdir = t.sdir; m->soff = (u64)tbeg; m->send = (u64)tend; m->sext = (u64)sext; m->ssize = (u64)t.slen;
    m->ident_perc = ident; m->vscore = 0; m->_pad = 0;
    if (m->sdir == 1) { const u64 so = m->ssize - m->send, se = m->ssize - m->soff; m->soff = so; m->send = se; }
    return true;
}

}  // namespace aends
}  // namespace necat
