// ctg_extend.h - the middle of contig polishing's loop over the records of one contig segment (extend_ctg_m4s, ctg_cns/cns_ctg_subseq.c:119-197): which
// read-to-contig records are aligned, which alignments are kept, in which order they become the segment's overlaps.  No HIP in this header: the aligners are
// a table the caller filled (stage_ctg_extend.inl computes it for every record ahead of the pass; tests/host_core/check_ctg_extend.cpp feeds it the reference's
// own results).  The arrangement of rm::walk with its table provider (rm_host.h).
//
// The rule, for one segment [from, from + size) and its records in the order given (the program sorts by soff; nothing here sorts):
//   1. range   sb = max(soff - from, 0), se = min(send - from, size)                                     (:145-148; send > from is asserted there, refused here)
//   2. cap     the positions of [sb, se) whose counter is below MAX_CNS_COV = 10 are counted; fewer than 200: the record is skipped       (:111-117, :149)
//   3. seed    can_list[0] of the read against the segment; none: skipped, and not counted as extended                                 (:157)
//   4. align   cns_extension with min_align_size 1000, error 0.5, rescue on: block-wise, final when ok and lhang + rhang <= 200; otherwise DALIGNER + edlib's
//              path over its range; otherwise the block-wise result if it was ok                                                  (:17-109, :163-178)
//   5. accept  ident_perc >= 90.0 && (qe - qb >= rl * 0.6 || sb - se >= size * 0.6), products in double.  The second alternative has its operands the wrong
//              way round in the reference (sb - se is never positive): it is never true, and is kept that way                      (:180)
//   6. count   ++counter over the ALIGNMENT's own [toff, tend) - not the record's range -, the alignment is the segment's next overlap.  The counters are u8
//              and wrap past 255 as the reference's do                                                                           (:183-185)
// Steps 3 and 4 read nothing of the loop's state (the reference resets its work buffers per call), so they are the table.
#pragma once
#include <stdint.h>

#include <vector>

namespace necat_host {
namespace ctg_ext {

constexpr int kMaxCov = 10;             // MAX_CNS_COV, cns_ctg_subseq.h
constexpr int kFullBelow = 200;         // cov_stats_is_full: fewer open positions than this
constexpr int kMinAlignSize = 1000;     // cns_ctg_subseq.c:169
constexpr double kError = 0.5;          // :131-133
constexpr double kMinIdent = 90.0, kMinRatio = 0.6;      // :180
constexpr int64_t kMaxSegment = 1 << 24;

enum State { kCapped = 0, kNoSeed = 1, kNoAlignment = 2, kRejected = 3, kAccepted = 4 };
enum Decided { kByNone = 0, kByBlocks = 1, kByPair = 2, kByBlocksKept = 3 };      // which aligner's result stands (cns_extension's three exits)

// what steps 3 and 4 gave for one record
struct Aligned { int32_t found, ok, qoff, qend, toff, tend; double ident_perc; };

// step 1.  false: the record ends at or before the segment's start (the reference asserts)
inline bool record_range(int64_t soff, int64_t send, int64_t from, int32_t size, int32_t* sb, int32_t* se)
{
    if (send <= from) return false;
    *sb = soff >= from ? (int32_t)(soff - from < (int64_t)size ? soff - from : size) : 0;
    const int64_t e = send - from;
    *se = e < (int64_t)size ? (int32_t)e : size;
    return true;
}

// step 2 (cov_stats_is_full): an empty range is full
inline bool is_full(const uint8_t* cov, int32_t sb, int32_t se)
{
    int n = 0;
    for (int32_t i = sb; i < se; ++i) if (cov[i] < kMaxCov) ++n;
    return n < kFullBelow;
}

// step 5, with the reference's second alternative as it is written there
inline bool accepted(const Aligned& a, int32_t rl, int32_t size)
{
    return a.ident_perc >= kMinIdent && (a.qend - a.qoff >= rl * kMinRatio || a.toff - a.tend >= size * kMinRatio);
}

struct Pass {
    std::vector<int32_t> state;         // per record: State
    std::vector<uint64_t> order;        // the accepted records, in the order they became overlaps
    uint64_t n_used = 0;                // records that reached cns_extension (the reference's "extended m4")
};

// Steps 1, 2, 5, 6 over records [0, n) of a segment of `size` bases.  range(k, &sb, &se): step 1 of record k (already checked); qsize(k): its read's length;
// table(k): its Aligned.  cap == false: no counters - every record is looked at, every accepted alignment is an overlap.
template <class Range, class QSize, class Table>
inline void replay(int32_t size, uint64_t n, bool cap, Range&& range, QSize&& qsize, Table&& table, Pass* out)
{
    out->state.assign(n, kCapped); out->order.clear(); out->n_used = 0;
    std::vector<uint8_t> cov(cap ? (size_t)size : 0, 0);
    for (uint64_t k = 0; k < n; ++k) {
        if (cap) {
            int32_t sb = 0, se = 0;
            range(k, &sb, &se);
            if (is_full(cov.data(), sb, se)) continue;
        }
        const Aligned& a = table(k);
        if (!a.found) { out->state[k] = kNoSeed; continue; }
        ++out->n_used;
        if (!a.ok) { out->state[k] = kNoAlignment; continue; }
        if (!accepted(a, qsize(k), size)) { out->state[k] = kRejected; continue; }
        if (cap) for (int32_t p = a.toff; p < a.tend; ++p) ++cov[p];
        out->state[k] = kAccepted;
        out->order.push_back(k);
    }
}

}  // namespace ctg_ext
}  // namespace necat_host
