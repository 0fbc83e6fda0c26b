// trim_core.h - host restatement of the read trimming stage's per-read decision (trim_bases/largest_cover_range.c:290-325, lcr_worker) on an array
// of 96-byte M4 records IN A GIVEN ORDER: truncate_m4_list -> is_complete_read -> is_chimeric_read -> largest_cover_range, and the final pass of
// largest_cover_range_main.c:43-52.  Plain C++17.  It is the CPU model of the tests, what `NECAT_TRIM_HOST=1 oc2lcr` runs for every read, and what
// oc2lcr runs for the reads the device hands back (necat_clip_range::how == host).
//
// Quirks of the reference that are part of the result and kept:
//   * remove_low_quality_m4 (detect_chimeric_reads.c:5-16) compacts the array in place but only its callee-local count shrinks: after
//     is_complete_read the tail of the array holds stale copies, is_chimeric_read filters and sorts a prefix of THAT, and largest_cover_range reads
//     all nm4 slots.  With oc2pm4 and oc2lcr on the same cutoff (the pipeline's call) nothing is below it and the compaction is the identity.
//   * the sorts are klib's unstable introsort (klib_sort.h); where equal keys decide the answer - the 300-record truncation by identity, the chimera
//     test's (qid, qdir, -vscore) order - the answer depends on the order the records arrive in, which is why oc2pm4's files are byte-identical to
//     the reference's at one thread and why the device hands exactly those reads back (classify below).
//   * the sweeps of range_list.c and the int * double comparisons of the chimera tests: trim_sweep.h, shared with the device kernel.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "klib_sort.h"
#include "trim_sweep.h"

namespace necat_host {
namespace trim {

using namespace necat_trim;

// common/m4_record.h:10-25 (M4Record); the same 96 bytes as necat_m4 of include/necat_hip.h
struct M4 {
    int32_t  qid, qdir;
    uint64_t qoff, qend, qext, qsize;
    int32_t  sid, sdir;
    uint64_t soff, send, sext, ssize;
    double   ident_perc;
    int32_t  vscore;
    int32_t  _pad;
};
static_assert(sizeof(M4) == 96, "M4Record");

struct Clip { int32_t left, right, size, how; };     // necat_clip_range

// why a read is not decided by the device (0 = it is)
enum HostReason { kDevice = 0, kLowIdent = 1, kTruncated = 2, kTopTie = 3 };

struct SidLess { bool operator()(const M4& a, const M4& b) const { return a.sid < b.sid; } };
struct IdentGreater { bool operator()(const M4& a, const M4& b) const { return a.ident_perc > b.ident_perc; } };
// m4_record_chimeric_cmp, detect_chimeric_reads.c:160-168
struct ChimeraLess {
    bool operator()(const M4& a, const M4& b) const
    {
        return (a.qid < b.qid) || (a.qid == b.qid && a.qdir < b.qdir) || (a.qid == b.qid && a.qdir == b.qdir && a.vscore > b.vscore);
    }
};

// pm4_aux.c:103-127 (fix_asm_m4_offsets with query_is_target): the record seen from its query, on the forward strand of the new subject
inline M4 exchanged(const M4& c)
{
    M4 n = c;
    n.qid = c.sid; n.qdir = c.sdir; n.qoff = c.soff; n.qend = c.send; n.qext = c.sext; n.qsize = c.ssize;
    n.sid = c.qid; n.sdir = c.qdir; n.soff = c.qoff; n.send = c.qend; n.sext = c.qext; n.ssize = c.qsize;
    if (n.sdir == 1) { n.sdir = 1 - n.sdir; n.qdir = 1 - n.qdir; }
    return n;
}

inline int remove_low_quality(M4* m4v, int nm4, double min_ident_perc)
{
    int k = 0;
    for (int i = 0; i < nm4; ++i) if (m4v[i].ident_perc >= min_ident_perc) m4v[k++] = m4v[i];
    return k;
}

// largest_cover_range.c:71-90
inline void truncate_list(M4* m4v, int* nm4, double ident_perc)
{
    int n = *nm4;
    if (n > kMaxRecs) n = remove_low_quality(m4v, n, ident_perc);
    if (n > kMaxRecs) { klib_introsort((size_t)n, m4v, IdentGreater()); n = kMaxRecs; }
    *nm4 = n;
}

// detect_chimeric_reads.c:18-36
inline bool is_complete_read(M4* m4v, int nm4, double min_ident_perc, int* fbgn, int* fend)
{
    nm4 = remove_low_quality(m4v, nm4, min_ident_perc);
    const int size = (int)m4v[0].ssize;
    *fbgn = 0; *fend = size;
    for (int i = 0; i < nm4; ++i) if (range_is_complete((int)m4v[i].soff, (int)m4v[i].send, size)) return true;
    return false;
}

// detect_chimeric_reads.c:170-217.  top_tie (optional): a pair that was evaluated had a second record with its (qid, qdir) and vscore - which of
// the two the unstable sort put first chose the pair.
inline bool is_chimeric_read(M4* m4v, int nm4, double min_ident_perc, int* fbgn, int* fend, bool* top_tie = nullptr)
{
    nm4 = remove_low_quality(m4v, nm4, min_ident_perc);
    klib_introsort((size_t)nm4, m4v, ChimeraLess());
    int i = 0, max_size = 0, num_chimeric_reads = 0;
    while (i < nm4) {
        int j = i + 1;
        while (j < nm4 && m4v[j].qid == m4v[i].qid) ++j;
        int k = i + 1;
        while (k < j && m4v[k].qdir == m4v[i].qdir) ++k;
        if (k < j) {
            if (top_tie) {
                if (i + 1 < k && m4v[i + 1].vscore == m4v[i].vscore) *top_tie = true;
                if (k + 1 < j && m4v[k + 1].qdir == m4v[k].qdir && m4v[k + 1].vscore == m4v[k].vscore) *top_tie = true;
            }
            const bool r = chimera_pair((int)m4v[i].qoff, (int)m4v[i].qend, (int)m4v[k].qoff, (int)m4v[k].qend,
                                        (int)m4v[i].soff, (int)m4v[i].send, (int)m4v[k].soff, (int)m4v[k].send, (int)m4v[i].qsize, (int)m4v[i].ssize);
            if (r) {
                ++num_chimeric_reads;
                if ((int)m4v[i].send - (int)m4v[i].soff > max_size) { max_size = (int)m4v[i].send - (int)m4v[i].soff; *fbgn = (int)m4v[i].soff; *fend = (int)m4v[i].send; }
                if ((int)m4v[k].send - (int)m4v[k].soff > max_size) { max_size = (int)m4v[k].send - (int)m4v[k].soff; *fbgn = (int)m4v[k].soff; *fend = (int)m4v[k].send; }
            }
        }
        i = j;
    }
    return max_size > 0 && num_chimeric_reads > 1;
}

// largest_cover_range.c:80-196 on ALL nm4 slots.  CovRange_LT and IntervalDepthRegion_LT tie only on elements that are equal in every field, so any
// sort gives the arrays klib's introsort gives.
inline bool largest_cover_range(const M4* m4v, int nm4, int* fbgn, int* fend, int min_ovlp_size, int min_cov)
{
    std::vector<int> opens((size_t)nm4), closes((size_t)nm4);
    std::vector<Range> il((size_t)nm4), de((size_t)2 * nm4 + 1), id((size_t)2 * nm4 + 1), fi((size_t)3 * nm4 + 1);
    for (int i = 0; i < nm4; ++i) {
        const int tbgn = (int)m4v[i].soff, tend = (int)m4v[i].send;
        opens[i] = tbgn; closes[i] = tbgn + (tend - tbgn);
        il[i].lo = tbgn; il[i].hi = tbgn + (tend - tbgn); il[i].ct = 1;
    }
    std::sort(opens.begin(), opens.end());
    std::sort(closes.begin(), closes.end());
    std::sort(il.begin(), il.end(), [](const Range& a, const Range& b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
    return cover_range(opens.data(), closes.data(), il.data(), nm4, min_ovlp_size, min_cov, de.data(), id.data(), fi.data(), fbgn, fend);
}

// one read as lcr_worker decides it (largest_cover_range.c:303-320), m4v[0 .. nm4) in the reference's order; m4v is permuted and partly overwritten
// as the reference's array is.  Returns how the read was decided (kNone: no range; out keeps calloc's zeros) - the final pass is the caller's.
inline int decide_read(M4* m4v, int nm4, double min_ident_perc, int min_ovlp_size, int min_cov, Clip* out, bool* top_tie = nullptr)
{
    int left = 0, right = 0, how;
    truncate_list(m4v, &nm4, min_ident_perc);
    if (is_complete_read(m4v, nm4, min_ident_perc, &left, &right)) how = kComplete;
    else if (is_chimeric_read(m4v, nm4, min_ident_perc, &left, &right, top_tie)) how = kChimeric;
    else if (largest_cover_range(m4v, nm4, &left, &right, min_ovlp_size, min_cov)) how = kCover;
    else { out->left = 0; out->right = 0; out->size = 0; out->how = kNone; return kNone; }
    out->left = left; out->right = right; out->size = (int)m4v[0].ssize; out->how = how;
    return how;
}

// Which reads the device decides, and why not the others: (a) a record below the cutoff - the stale-tail quirk makes the answer depend on
// array order; (b) more than 300 records - the truncation stays on the host; (c) the read is not complete and a pair the chimera test evaluates was
// chosen among records with equal (qid, qdir, vscore).  Order-independent itself: counts and key comparisons only.
inline int classify(const M4* m4v, int nm4, double min_ident_perc)
{
    for (int i = 0; i < nm4; ++i) if (m4v[i].ident_perc < min_ident_perc) return kLowIdent;
    if (nm4 > kMaxRecs) return kTruncated;
    const int size = (int)m4v[0].ssize;
    for (int i = 0; i < nm4; ++i) if (range_is_complete((int)m4v[i].soff, (int)m4v[i].send, size)) return kDevice;
    std::vector<M4> v(m4v, m4v + nm4);
    std::sort(v.begin(), v.end(), ChimeraLess());
    int i = 0;
    while (i < nm4) {
        int j = i + 1;
        while (j < nm4 && v[j].qid == v[i].qid) ++j;
        int k = i + 1;
        while (k < j && v[k].qdir == v[i].qdir) ++k;
        if (k < j) {
            if (i + 1 < k && v[i + 1].vscore == v[i].vscore) return kTopTie;
            if (k + 1 < j && v[k + 1].qdir == v[k].qdir && v[k + 1].vscore == v[k].vscore) return kTopTie;
        }
        i = j;
    }
    return kDevice;
}

// a partition file as oc2lcr holds it (load_partition_m4, largest_cover_range.c:198-224): sorted by subject id with klib's introsort, runs of equal
// ids.  run_off: the start of every run + the total.
inline void group_partition(std::vector<M4>& recs, std::vector<size_t>& run_off)
{
    klib_introsort(recs.size(), recs.data(), SidLess());
    run_off.clear();
    size_t i = 0;
    while (i < recs.size()) {
        size_t j = i + 1;
        while (j < recs.size() && recs[j].sid == recs[i].sid) ++j;
        run_off.push_back(i);
        i = j;
    }
    run_off.push_back(recs.size());
}

// the last pass + the text of clipped_ranges.txt's line i (largest_cover_range_main.c:43-52)
inline void finish_clip(Clip& c, int min_size) { final_pass(c.left, c.right, c.size, min_size); }

}  // namespace trim
}  // namespace necat_host
