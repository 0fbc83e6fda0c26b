// ctg_dev_core.h - the consensus half of contig polishing (ctg_consensus.h has the rule) as the DEVICE computes it: the per-lane cores of the kernels in
// ctg_dev_kernels.h, the host-side plan that cuts a segment into position ranges, and - for g++ - a CPU model of the device path (ctg_dev::model_segment,
// tests/host_core/check_ctg_consensus.cpp).  The device path is EXACT: a link's weight is the number of its tags (every overlap weighs 1.0), so nothing depends on the
// order equal tags are left in, and the scores are computed by ctg_consensus.h's own score pass on the nodes and links the device hands back.
//
// The sort key of a tag, 64 bits, no overlap index (equal tags are interchangeable):
//     t_pos 24 | delta 16 | q_base 3 | where 2 | p_delta 16 | p_q_base 3
// t_pos is relative to the position range being processed (a segment is shorter than 2^24 bases; the value `range size` marks a slot without a tag), delta and p_delta
// stop at 65 534 (the scan of an overlap ends at the column where one reaches 65 535), q_base is '-' 0, A C G T 1..4, p_q_base '-' 0, '.' 1, A C G T 2..5 - both in the
// reference's character order - and `where` says where the predecessor is: 0 nowhere (the overlap's first column: p_t_pos -1 sorts first), 1 at the position before,
// 2 at this position.  The low 21 bits are the link word ctg_consensus.h's Graph keeps.
#pragma once
#include <stdint.h>

#include "cns_dev_core.h"

namespace necat {
namespace ctg_dev {

using cns_dev::ColState;
using cns_dev::ColTag;

constexpr u32 kMaxSegment = 1u << 24;          // a segment must be SHORTER
constexpr u32 kStopDelta = 65535;              // MAX_CNS_DELTA
constexpr int kBlockShift = 6;                 // the plan's grain: ranges begin at multiples of 64 positions
constexpr u32 kTilePositions = 256;            // positions per workgroup of the link kernels
constexpr u32 kBigBucket = 1024;               // a position's bucket of more keys goes to k_ctg_sort_big (ctg_dev_kernels.h)
static_assert(24 + 16 + 3 + 2 + 16 + 3 == 64, "the key's fields fill 64 bits");
static_assert(kMaxSegment - 1 < (1u << 24) && kStopDelta - 1 < (1u << 16) && 4 < (1 << 3) && 2 < (1 << 2) && 5 < (1 << 3), "every field holds its largest value");

NECAT_HD u64 tag_key(u32 t_pos, u32 delta, u32 qs, u32 where, u32 p_delta, u32 p_qs)
{
    return (u64)t_pos << 40 | (u64)delta << 24 | (u64)qs << 21 | (u64)where << 19 | (u64)p_delta << 3 | (u64)p_qs;
}
NECAT_HD u32 key_pos(u64 k) { return (u32)(k >> 40); }
NECAT_HD u32 key_delta(u64 k) { return (u32)(k >> 24) & 0xffffu; }
NECAT_HD u32 key_db(u64 k) { return (u32)(k >> 21) & 0x7ffffu; }        // delta << 3 | q_base: a node inside its position
NECAT_HD u64 key_node(u64 k) { return k >> 21; }
NECAT_HD u32 key_link_word(u64 k) { return (u32)k & 0x1fffffu; }

// the key of a column's tag given the previous column's tag
NECAT_HD u64 col_key(const ColTag& t, const ColTag& prev, bool first)
{
    const u32 where = first ? 0u : (prev.t_pos == t.t_pos ? 2u : 1u);
    return tag_key((u32)t.t_pos, t.delta, t.qs, where, first ? 0u : prev.delta, first ? 1u : (prev.qs ? prev.qs + 1u : 0u));
}

// what tag i of the sorted array begins, given the tag before it
struct RunStart { bool node, link, pos; };
NECAT_HD RunStart run_start(u64 k, u64 kp, bool first)
{
    RunStart r;
    r.node = first || key_node(k) != key_node(kp);
    r.link = first || k != kp;
    r.pos = first || key_pos(k) != key_pos(kp);
    return r;
}
// is tag i the last tag at delta 0 of its position (bucket_end: one past the position's last tag; next: tag i + 1, read only inside the bucket)
NECAT_HD bool closes_coverage(u64 k, bool last_of_bucket, u64 next) { return key_delta(k) == 0 && (last_of_bucket || key_delta(next) != 0); }

// where a wave takes an overlap up in a position range: the column before the range's first one (its tag is the first tag's predecessor; it lies outside the range
// and is not kept), and what the columns before that one add up to
struct Start { i32 col0, tcnt, qcnt, last_t; };
// one overlap of one range (the columns col0 .. col0 + slots), as the kernels read it
struct RangeOvl { u64 ops_off, read_begin; i32 toff, qsize, qoff, qdir; u32 slots, slot_base; Start st; };

}  // namespace ctg_dev
}  // namespace necat

// ------------------------------------------------------------------------------------------ the plan (host): blocks, ranges, where every overlap enters a range
#include <algorithm>
#include <vector>

#include "ctg_consensus.h"

namespace necat {
namespace ctg_dev {

struct Mark { i32 first_col; Start st; u32 tags; };             // an overlap in one block of 64 positions: its first column there, the start for it, its tags there
struct OvlPlan { i32 ncols = 0, block0 = 0; std::vector<Mark> marks; };      // ncols: the columns that give tags (the stop rule applied)

inline void plan_overlap(const u8* ops, i32 ncols, i32 toff, OvlPlan& P)
{
    P = OvlPlan();
    ColState st = {0, 0, -1}, before_prev = st;
    i32 block = -1, i = 0;
    for (; i < ncols; ++i) {
        const int op = necat_host::ctg::op_at(ops, i);
        const ColTag t = cns_dev::col_tag(op, i, st, toff, [](i32) { return 0u; });
        if (t.delta >= kStopDelta) break;
        const i32 b = t.t_pos >> kBlockShift;
        if (b != block) {
            if (block < 0) P.block0 = b;
            Mark m; m.first_col = i; m.tags = 0;
            const ColState& s = i ? before_prev : st;
            m.st.col0 = i ? i - 1 : 0; m.st.tcnt = s.tcnt; m.st.qcnt = s.qcnt; m.st.last_t = s.last_t;
            P.marks.push_back(m);
            block = b;
        }
        ++P.marks.back().tags;
        before_prev = st;
        cns_dev::col_advance(op, i, st);
    }
    P.ncols = i;
}

struct Range { u32 p0, p1; u64 tags; };
// consecutive blocks while their tags stay within the budget (a block with more goes alone); the ranges cover [0, size)
inline std::vector<Range> plan_ranges(const std::vector<u64>& block_tags, u32 size, u64 budget)
{
    std::vector<Range> R;
    Range cur = {0, 0, 0};
    for (size_t b = 0; b < block_tags.size(); ++b) {
        if (cur.p1 > cur.p0 && cur.tags + block_tags[b] > budget) { R.push_back(cur); cur = {cur.p1, cur.p1, 0}; }
        cur.p1 = std::min<u64>(size, (u64)(b + 1) << kBlockShift);
        cur.tags += block_tags[b];
    }
    if (cur.p1 > cur.p0 || R.empty()) { cur.p1 = size; R.push_back(cur); }
    return R;
}

// the overlap's part in the range, or false when it has none
inline bool range_overlap(const OvlPlan& P, const Range& r, Start* st, u32* slots)
{
    const i64 bA = (i64)(r.p0 >> kBlockShift), bE = ((i64)r.p1 + (1 << kBlockShift) - 1) >> kBlockShift;
    const i64 lo = std::max<i64>(bA, P.block0) - P.block0, hi = bE - P.block0;
    if (lo >= (i64)P.marks.size() || hi <= lo) return false;
    const i32 end = hi < (i64)P.marks.size() ? P.marks[(size_t)hi].first_col : P.ncols;
    *st = P.marks[(size_t)lo].st;
    *slots = (u32)(end - st->col0);
    return true;
}

// what one range hands back (the kernels' outputs, downloaded): nodes with absolute positions, link indices and tag indices relative to the range
struct RangeOut {
    std::vector<u32> n_pos, n_db, n_link0, l_pred, l_tag0, pos_node;     // pos_node[p - p0]: first node of the position, ~0 for a position without tags
    std::vector<i32> cov;
    u64 n_tags = 0;
};

inline void graph_begin(necat_host::ctg::Graph& G, u32 size)
{
    G = necat_host::ctg::Graph();
    G.cov.assign(size, 0);
    G.pos_node.assign((size_t)size + 1, 0);
}
inline void graph_append(necat_host::ctg::Graph& G, const RangeOut& R, const Range& r)
{
    const u32 bn = (u32)G.nodes(), bl = (u32)G.links(), nn = (u32)R.n_pos.size(), nl = (u32)R.l_pred.size();
    G.n_pos.insert(G.n_pos.end(), R.n_pos.begin(), R.n_pos.end());
    G.n_db.insert(G.n_db.end(), R.n_db.begin(), R.n_db.end());
    for (u32 n = 0; n < nn; ++n) G.n_link0.push_back(bl + R.n_link0[n]);
    G.l_pred.insert(G.l_pred.end(), R.l_pred.begin(), R.l_pred.end());
    for (u32 l = 0; l < nl; ++l) G.l_count.push_back((l + 1 < nl ? R.l_tag0[l + 1] : (u32)R.n_tags) - R.l_tag0[l]);
    u32 next = bn + nn;
    for (u32 p = r.p1; p-- > r.p0;) {
        if (!R.pos_node.empty() && R.pos_node[p - r.p0] != ~0u) next = bn + R.pos_node[p - r.p0];
        G.pos_node[p] = next;
        if (!R.cov.empty()) G.cov[p] = R.cov[p - r.p0];
    }
    G.n_tags += R.n_tags;
}
inline void graph_end(necat_host::ctg::Graph& G, u32 size)
{
    G.pos_node[size] = (u32)G.nodes();
    G.n_link0.push_back((u32)G.links());
}

}  // namespace ctg_dev
}  // namespace necat

#if !defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the CPU model of the device path (tests only)
namespace necat {
namespace ctg_dev {

// k_ctg_tags for one overlap of one range, lane by lane: 64 columns per step, the carries as the wave keeps them
inline void model_tags(const RangeOvl& o, const u8* ops, const u64* words, u32 range_size, std::vector<u64>& keys)
{
    const u8* op_bytes = ops + o.ops_off;
    ColState carry = {o.st.tcnt, o.st.qcnt, o.st.last_t};
    ColTag prev_last = {-1, 0, 0};
    auto qb = [&](i32 qi) { return cns_dev::strand_base(words, o.read_begin, o.qsize, o.qdir, std::max(0, std::min(o.qoff + qi, o.qsize - 1))); };
    for (u32 base = 0; base < o.slots; base += 64) {
        ColTag lane_tag[64];
        ColState s = carry;
        for (u32 lane = 0; lane < 64 && base + lane < o.slots; ++lane) {
            const i32 i = o.st.col0 + (i32)(base + lane);
            const int op = (op_bytes[i >> 2] >> ((i & 3) * 2)) & 3;
            const ColTag t = cns_dev::col_tag(op, i, s, o.toff, qb);
            cns_dev::col_advance(op, i, s);
            const ColTag prev = lane ? lane_tag[lane - 1] : prev_last;
            lane_tag[lane] = t;
            if (t.t_pos >= 0 && (u32)t.t_pos < range_size) keys.push_back(col_key(t, prev, i == 0));
        }
        carry = s;
        prev_last = lane_tag[std::min<u32>(63, o.slots - base - 1)];
    }
}

// k_ctg_count / k_ctg_links on the sorted keys of a range
inline void model_links(const std::vector<u64>& K, const Range& r, RangeOut& R)
{
    const u32 n = (u32)K.size(), size = r.p1 - r.p0;
    R = RangeOut();
    R.n_tags = n;
    R.cov.assign(size, 0);
    R.pos_node.assign(size, ~0u);
    std::vector<u32> off((size_t)size + 1, 0);
    for (u64 k : K) ++off[key_pos(k) + 1];
    for (u32 p = 0; p < size; ++p) off[p + 1] += off[p];
    for (u32 i = 0; i < n; ++i) {
        const u64 k = K[i];
        const RunStart s = run_start(k, i ? K[i - 1] : 0, i == 0);
        const u32 pos = key_pos(k);
        if (s.node) { R.n_pos.push_back(r.p0 + pos); R.n_db.push_back(key_db(k)); R.n_link0.push_back((u32)R.l_pred.size()); }
        if (s.link) { R.l_pred.push_back(key_link_word(k)); R.l_tag0.push_back(i); }
        if (s.pos) R.pos_node[pos] = (u32)R.n_pos.size() - 1;
        if (closes_coverage(k, i + 1 == off[pos + 1], i + 1 < n ? K[i + 1] : 0)) R.cov[pos] = (i32)(i - off[pos] + 1);
    }
}

struct ModelOverlap { const u8* ops; i32 ncols, toff; const u64* words; u64 read_begin; i32 qsize, qoff, qdir; };

// one segment through plan, tags, sort, links, range by range, then the host's score pass; returns the number of ranges
inline u32 model_segment(const ModelOverlap* ov, size_t n_ov, u32 size, int min_cov, u64 budget, necat_host::ctg::SegmentOut& out)
{
    std::vector<OvlPlan> plans(n_ov);
    std::vector<u64> block_tags(((size_t)size + (1u << kBlockShift) - 1) >> kBlockShift, 0);
    for (size_t k = 0; k < n_ov; ++k) {
        plan_overlap(ov[k].ops, ov[k].ncols, ov[k].toff, plans[k]);
        for (size_t m = 0; m < plans[k].marks.size(); ++m) block_tags[(size_t)plans[k].block0 + m] += plans[k].marks[m].tags;
    }
    const std::vector<Range> ranges = plan_ranges(block_tags, size, budget);
    necat_host::ctg::Graph G;
    graph_begin(G, size);
    for (const Range& r : ranges) {
        std::vector<u64> keys;
        for (size_t k = 0; k < n_ov; ++k) {
            RangeOvl o;
            if (!range_overlap(plans[k], r, &o.st, &o.slots)) continue;
            o.ops_off = 0; o.read_begin = ov[k].read_begin; o.toff = ov[k].toff - (i32)r.p0; o.qsize = ov[k].qsize; o.qoff = ov[k].qoff; o.qdir = ov[k].qdir; o.slot_base = 0;
            model_tags(o, ov[k].ops, ov[k].words, r.p1 - r.p0, keys);
        }
        std::sort(keys.begin(), keys.end());
        RangeOut R;
        model_links(keys, r, R);
        graph_append(G, R, r);
    }
    graph_end(G, size);
    out.n_tags = G.n_tags; out.n_nodes = G.nodes(); out.n_links = G.links();
    necat_host::ctg::best_path(G, min_cov, out.cns, out.t_pos);
    return (u32)ranges.size();
}

}  // namespace ctg_dev
}  // namespace necat
#endif
