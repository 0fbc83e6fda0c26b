// trim_sweep.h - the integer decisions of the read trimming stage that do not depend on the order of the records: the two chimera tests on a pair
// of overlaps (trim_bases/detect_chimeric_reads.c:40-158) and the sweeps that turn a read's overlap intervals into its largest covered range
// (trim_bases/range_list.c, largest_cover_range.c:80-196).  Plain functions on arrays that are already sorted, so that the host restatement
// (trim_core.h, after klib's introsort / std::sort) and the device kernel (trim_kernels.h, after its rank sorts in LDS) run the SAME code: what one
// computes the other computes, instruction for instruction in the integer / double domain (-ffp-contract=off on both sides; the only floating-point
// operations are int * 0.9 and int * 0.4, exact products of a 31-bit integer and a double rounded once).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TRIM_HD __host__ __device__ inline
#else
#define TRIM_HD inline
#endif

namespace necat_trim {

constexpr int kMaxEnd = 20;          // largest_cover_range.c:11: a read whose unclipped ends are at most this long is complete
constexpr int kMaxRecs = 300;        // largest_cover_range.c:76 (MaxNm4): overlaps of one read that take part

// how a read's range was decided (necat_clip_range::how, include/necat_hip.h)
enum How { kNone = 0, kComplete = 1, kChimeric = 2, kCover = 3, kHost = 4 };

struct Range { int lo, hi, ct; };    // CovRange (range_list.h:14-19) without `va`: every range of this stage is added with value 0, so va stays 0

// lcr_is_complete (largest_cover_range.c:13-17) for a valid range
TRIM_HD bool range_is_complete(int left, int right, int size) { return left >= 0 && left <= kMaxEnd && size - right <= kMaxEnd; }

// the part both chimera cases share (detect_chimeric_reads.c:46-85 = :110-149): the pair ordered by query start and by target start, overlap sizes
// within 10 % of each other, and each overlap sharing 90 % of its query bases with the other.  The int * double comparisons are the reference's.
struct ChimeraPair { int lqb, lqe, rqb, rqe, ltb, lte, rtb, rte; };
TRIM_HD bool chimera_common(int qb1, int qe1, int qb2, int qe2, int tb1, int te1, int tb2, int te2, ChimeraPair& p)
{
    if (qb1 < qb2) { p.lqb = qb1; p.lqe = qe1; p.rqb = qb2; p.rqe = qe2; } else { p.lqb = qb2; p.lqe = qe2; p.rqb = qb1; p.rqe = qe1; }
    if (tb1 < tb2) { p.ltb = tb1; p.lte = te1; p.rtb = tb2; p.rte = te2; } else { p.ltb = tb2; p.lte = te2; p.rtb = tb1; p.rte = te1; }
    const int ov1 = p.lqe - p.lqb, ov2 = p.rqe - p.rqb;
    const int max_ov = ov1 > ov2 ? ov1 : ov2, min_ov = ov1 < ov2 ? ov1 : ov2;
    if (min_ov < max_ov * 0.9) return false;
    int common_read_bps = 0;
    if (p.lqe > p.rqb) common_read_bps = p.lqe - p.rqb;
    return (common_read_bps >= (p.lqe - p.lqb) * 0.9) && (common_read_bps >= (p.rqe - p.rqb) * 0.9);
}
// case I: the query twice on most of the target (:40-99), case II: most of the query twice, on target ranges within 1000 bases (:103-158).
// Returns 1, 2 or 0 as `is_chimeric_read_case_i(..) || is_chimeric_read_case_ii(..)` is non-zero or not (only that is used).
TRIM_HD bool chimera_pair(int qb1, int qe1, int qb2, int qe2, int tb1, int te1, int tb2, int te2, int qsize, int tsize)
{
    ChimeraPair p;
    if (!chimera_common(qb1, qe1, qb2, qe2, tb1, te1, tb2, te2, p)) return false;
    {   // case I
        int mapped_target_bps = p.rte - p.ltb;
        if (p.rtb > p.lte) mapped_target_bps -= (p.rtb - p.lte);
        bool r = mapped_target_bps >= tsize * 0.9;
        if (r && p.lte > p.rtb) {
            const int ov = p.lte - p.rtb;
            r = (ov < (p.lte - p.ltb) * 0.4) && (ov < (p.rte - p.rtb) * 0.4);
        }
        if (r) return true;
    }
    {   // case II
        bool r = (p.lqe - p.lqb >= qsize * 0.9) && (p.rqe - p.rqb >= qsize * 0.9);
        if (!r) return false;
        if (p.lte > p.rtb) r = p.lte - p.rtb <= 1000;
        else r = p.rtb - p.lte <= 1000;
        return r;
    }
}

// compute_depth_for_CovRangeList (range_list.c:113-176) on the events in IntervalDepthRegion_LT's order, which puts EVERY opening event before
// every closing event and orders by position inside each kind: the n interval starts ascending, then the n interval ends ascending.  (Not a depth
// profile - it is what the reference computes.)  With va == 0 throughout, "va != nva" is false and the va comparison of the merge is true.  The
// element being built when the events run out is dropped, as the reference's final kv_resize(list_len) drops it.  out: room for 2 n entries.
TRIM_HD int depth_list(const int* opens, const int* closes, int n, Range* crl)
{
    if (n <= 0) return 0;
    const int id_len = 2 * n;
    int list_len = 0;
    crl[0].lo = opens[0]; crl[0].hi = opens[0]; crl[0].ct = 1;
    int prev_pos = opens[0];
    for (int i = 1; i < id_len; ++i) {
        const bool open = i < n;
        const int pos = open ? opens[i] : closes[i - n];
        crl[list_len].hi = pos;
        const int nct = open ? crl[list_len].ct + 1 : crl[list_len].ct - 1;
        if (prev_pos != pos && crl[list_len].lo != crl[list_len].hi) {
            ++list_len;
            crl[list_len].lo = pos;
            crl[list_len].ct = crl[list_len - 1].ct;
        }
        crl[list_len].hi = pos;
        crl[list_len].ct = nct;
        if (list_len > 1 && crl[list_len - 1].hi == crl[list_len].lo && crl[list_len - 1].ct == crl[list_len].ct) {
            crl[list_len - 1].hi = crl[list_len].hi;
            --list_len;
        }
        prev_pos = pos;
    }
    return list_len;
}

// the runs of that list with depth >= min_cov (largest_cover_range.c:113-137).  ib == 0 && ie == 0 means "no run open", also for a run that
// really starts and ends at 0.  out: room for nde entries.
TRIM_HD int deep_runs(const Range* de, int nde, int min_cov, Range* id)
{
    int nid = 0, ib = 0, ie = 0;
    for (int it = 0; it < nde; ++it) {
        if (de[it].ct < min_cov) {
            if (ie > ib) { id[nid].lo = ib; id[nid].hi = ie; id[nid].ct = 1; ++nid; }
            ib = 0; ie = 0;
        } else if (ib == 0 && ie == 0) {
            ib = de[it].lo; ie = de[it].hi;
        } else if (ie == de[it].lo) {
            ie = de[it].hi;
        } else {
            if (ie > ib) { id[nid].lo = ib; id[nid].hi = ie; id[nid].ct = 1; ++nid; }
            ib = de[it].lo; ie = de[it].hi;
        }
    }
    if (ie > ib) { id[nid].lo = ib; id[nid].hi = ie; id[nid].ct = 1; ++nid; }
    return nid;
}

// merge_CovRangeList (range_list.c:66-105) on ranges sorted by (lo, hi): in place, returns the new length.  (0, 0) marks a slot as taken.
TRIM_HD int merge_ranges(Range* crl, int nrange, int min_ovlp)
{
    if (nrange == 0) return 0;
    int curr = 0, next = 1;
    while (next < nrange) {
        if (crl[curr].lo == 0 && crl[curr].hi == 0) {
            crl[curr] = crl[next];
            crl[next].lo = 0; crl[next].hi = 0;
            ++next;
        } else {
            bool intersect = false;
            if (crl[curr].lo <= crl[next].lo && crl[next].hi <= crl[curr].hi) intersect = true;
            if (crl[curr].hi - min_ovlp >= crl[next].lo) intersect = true;
            if (intersect) {
                if (crl[curr].hi < crl[next].hi) crl[curr].hi = crl[next].hi;
                crl[curr].ct += crl[next].ct;
                crl[next].lo = 0; crl[next].hi = 0;
                ++next;
            } else {
                ++curr;
                if (curr != next) crl[curr] = crl[next];
                ++next;
            }
        }
    }
    return curr + 1;
}

// the merged ranges cut down to the deep runs (largest_cover_range.c:141-174).  out: room for nil + nid entries.
TRIM_HD int intersect_ranges(const Range* il, int nil, const Range* id, int nid, Range* fi)
{
    int nfi = 0, li = 0, di = 0;
    while (li < nil && di < nid) {
        const int ll = il[li].lo, lh = il[li].hi, dl = id[di].lo, dh = id[di].hi;
        int nl = 0, nh = 0;
        if (ll <= dl && dl < lh) { nl = dl; nh = lh < dh ? lh : dh; }
        if (dl <= ll && ll < dh) { nl = ll; nh = lh < dh ? lh : dh; }
        if (nl < nh) { fi[nfi].lo = nl; fi[nfi].hi = nh; fi[nfi].ct = 1; ++nfi; }
        if (lh <= dh) ++li;
        if (dh <= lh) ++di;
    }
    return nfi;
}

// largest_cover_range (largest_cover_range.c:80-196) from its three sorted inputs: the interval starts ascending, the interval ends ascending, the
// intervals by (lo, hi) (ct = 1).  il is merged in place; de (2 n), id (2 n) and fi (3 n) are work space.  false: no range.
TRIM_HD bool cover_range(const int* opens, const int* closes, Range* il, int n, int min_ovlp, int min_cov, Range* de, Range* id, Range* fi, int* fbgn, int* fend)
{
    int nid = 0;
    if (min_cov > 0) {
        const int nde = depth_list(opens, closes, n, de);
        nid = deep_runs(de, nde, min_cov, id);
    }
    int nil = merge_ranges(il, n, min_ovlp);
    const Range* fin = il;
    if (min_cov > 0) {
        nil = intersect_ranges(il, nil, id, nid, fi);
        fin = fi;
    }
    if (nil == 0) return false;
    int max_l = 0, max_r = 0;
    for (int i = 0; i < nil; ++i) {
        if (fin[i].hi - fin[i].lo > max_r - max_l) { max_l = fin[i].lo; max_r = fin[i].hi; }
    }
    *fbgn = max_l; *fend = max_r;
    return true;
}

// the last pass of oc2lcr (largest_cover_range_main.c:45-50): a read nothing was decided for, or whose range is shorter than min_size, is invalid
TRIM_HD void final_pass(int& left, int right, int size, int min_size)
{
    if (size == 0) left = -1;
    else if (right - left < min_size) left = -1;
}

}  // namespace necat_trim
