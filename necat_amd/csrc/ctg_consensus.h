// ctg_consensus.h - the consensus half of NECAT's contig polishing (ctg_cns/: alignment tags -> backbone -> best path -> splice), host side.
// What cns_ctg_subseq does with ONE contig segment once its overlaps are chosen (ctg_cns/cns_ctg_subseq.c:184,210-233; fc_correct_one_read.c:81-366), restated:
//   * tags.  One per gapped column of an overlap.  t_pos = index of the last target base at or before the column, delta = query bases since that target base, q_base =
//     the column's query character ('-' in a deletion); the three of the column before ride along as p_t_pos / p_delta / p_q_base, and before the first column they
//     are -1 / 0 / '.'.  The scan of an overlap STOPS FOR GOOD at the first column whose delta (or p_delta) reaches 65 535: the later columns give no tags.
//   * order.  Six keys: t_pos, delta, q_base, p_t_pos, p_delta, p_q_base, characters by their code ('-' < '.' < 'A' < 'C' < 'G' < 'T').  Tags with equal keys are
//     interchangeable (every overlap has weight 1.0, cns_ctg_subseq.c:184), so the reference's unstable sort does not reach the output.
//   * graph.  A node is (t_pos, delta, q_base); a link of a node is a run of its tags with equal (p_t_pos, p_delta, p_q_base), its weight the run's length as a double
//     (the reference adds 1.0 that many times: the same double).  coverage[t_pos] = the tags at delta 0 there.
//   * score.  score(link) = weight - 0.1 * coverage[t_pos], += the predecessor node's score when there is one (p_t_pos != -1); a node takes its first link that beats
//     every earlier one by strict >, from -1.0; a node none of whose links beats -1.0 keeps -1.0 and no predecessor.  Nodes are visited by position, delta and base
//     A C G T '-'; the global best is the first node that beats -1.0 and every earlier one by strict >.  Compile with -ffp-contract=off: the same additions in the same
//     order give the same doubles.
//   * traceback (:339-362, quirks included).  From the best node b with predecessors b -> n1 -> n2 .. -> nk: the FIRST step emits n1's base at b's position, then
//     every n_j its own base at its own position; b's own base is never emitted, a b without predecessor emits nothing.  Case follows coverage[position] < min_cov,
//     '-' emits nothing, both arrays are reversed at the end.
//   * splice (cns_ctg_subseq.c:212-233).  Runs of upper case of at least min_run bases replace the raw bases between the t_pos of their ends; the raw contig, in upper
//     case, everywhere else.  A run starts at the first upper-case base after lower-case ones and is extended over upper-case bases only from its SECOND base on.
// One segment per thread.  This header is `path = 1` of necat_ctg_consensus_batch and the model the device path (ctg_dev_core.h) is tested against; the score pass,
// the traceback and the splice below are also what the device path runs on the nodes and links it downloads.  No HIP here.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_bases.h"

namespace necat_host {
namespace ctg {

constexpr int kMaxDelta = 65535;             // MAX_CNS_DELTA (fc_correct_one_read.h:19)
constexpr int kMinCov = 4;                   // MIN_CNS_COV (cns_ctg_subseq.h:12)
constexpr int kMinRun = 1000;                // cns_ctg_subseq.c:223
constexpr int64_t kMaxSegment = 1 << 24;     // a segment must be shorter (the device key's 24 bits of t_pos; the entry refuses the others for both paths)

// one overlap: its columns two bits each (0 match, 1 query base over '-', 2 '-' over target base, 3 mismatch; column i in bits 2 (i & 3) of byte i >> 2), where they
// start on the segment, and the read: 2-bit words of a volume (base g in bits 2 (g & 31) of word g >> 5), the read's first base, its size, strand and start
struct OverlapIn { const uint8_t* ops; int ncols, toff; const uint64_t* words; uint64_t read_begin; int qsize, qoff, qdir; };

inline int op_at(const uint8_t* ops, int i) { return (ops[i >> 2] >> ((i & 3) * 2)) & 3; }
inline unsigned strand_code(const OverlapIn& o, int i)
{
    const unsigned b = BaseWords{o.words}.base(o.read_begin + (uint64_t)(o.qdir ? o.qsize - 1 - i : i));
    return o.qdir ? 3u - b : b;
}

struct Tag { int32_t t_pos, p_t_pos; uint16_t delta, p_delta; char q_base, p_q_base; };
inline bool tag_less(const Tag& a, const Tag& b)
{
    if (a.t_pos != b.t_pos) return a.t_pos < b.t_pos;
    if (a.delta != b.delta) return a.delta < b.delta;
    if (a.q_base != b.q_base) return a.q_base < b.q_base;
    if (a.p_t_pos != b.p_t_pos) return a.p_t_pos < b.p_t_pos;
    if (a.p_delta != b.p_delta) return a.p_delta < b.p_delta;
    return a.p_q_base < b.p_q_base;
}

// Why an overlap cannot be given to the rule, or nullptr: its columns must add up to its coordinates, it must stay inside the read and the segment, and its first
// column may not be a query base in front of the segment's first base (t_pos would be -1: the reference asserts).
inline const char* overlap_fault(const uint8_t* ops, int ncols, int qoff, int qend, int toff, int tend, int qsize, int64_t seg_size)
{
    if (ncols < 0 || qoff < 0 || qend < qoff || qend > qsize) return "leaves its read";
    if (toff < 0 || tend < toff || (int64_t)tend > seg_size) return "leaves its segment";
    int64_t nq = 0, nt = 0;
    for (int i = 0; i < ncols; ++i) { const int op = op_at(ops, i); nq += op != 2; nt += op != 1; }
    if (nq != qend - qoff || nt != tend - toff) return "has columns that do not add up to its coordinates";
    if (ncols && toff == 0 && op_at(ops, 0) == 1) return "leaves its segment";
    return nullptr;
}

inline void add_tags(const OverlapIn& o, std::vector<Tag>& tags)
{
    int qi = o.qoff - 1, j = o.toff - 1, jj = 0, p_j = -1, p_jj = 0;
    char p_q = '.';
    for (int k = 0; k < o.ncols; ++k) {
        const int op = op_at(o.ops, k);
        char q = '-';
        if (op != 2) { ++qi; ++jj; q = "ACGT"[strand_code(o, qi)]; }
        if (op != 1) { ++j; jj = 0; }
        if (jj >= kMaxDelta || p_jj >= kMaxDelta) break;
        Tag t; t.t_pos = j; t.p_t_pos = p_j; t.delta = (uint16_t)jj; t.p_delta = (uint16_t)p_jj; t.q_base = q; t.p_q_base = p_q;
        tags.push_back(t);
        p_j = j; p_jj = jj; p_q = q;
    }
}

// ---- the backbone as compact arrays: what the host form builds from its sorted tags and the device path downloads.  Nodes in tag order (position, delta, base by
// character code: '-' first), links of a node in tag order.  Base codes here: '-' 0, A C G T 1..4; a predecessor's: '-' 0, '.' 1, A C G T 2..5.
struct Graph {
    std::vector<uint32_t> n_pos, n_db, n_link0;      // node: position, delta << 3 | base code, first link (n_link0 has one entry more than there are nodes)
    std::vector<uint32_t> l_pred, l_count;           // link: where << 19 | p_delta << 3 | p base code (where: 0 no predecessor, 1 at the position before, 2 at this one), tags
    std::vector<int32_t> cov;                        // per position
    std::vector<uint32_t> pos_node;                  // per position: its first node (size + 1 entries)
    uint64_t n_tags = 0;
    size_t nodes() const { return n_pos.size(); }
    size_t links() const { return l_pred.size(); }
};

inline unsigned base_code(char c) { return c == '-' ? 0u : c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 3u : 4u; }
inline unsigned pred_code(char c) { return c == '-' ? 0u : c == '.' ? 1u : base_code(c) + 1u; }

inline void build_graph(std::vector<Tag>& tags, int size, Graph& G)
{
    std::sort(tags.begin(), tags.end(), tag_less);
    G = Graph();
    G.n_tags = tags.size();
    G.cov.assign((size_t)size, 0);
    G.pos_node.assign((size_t)size + 1, 0);
    size_t i = 0;
    int at = 0;                                      // positions whose pos_node is set
    while (i < tags.size()) {
        const Tag& a = tags[i];
        for (; at <= a.t_pos; ++at) G.pos_node[(size_t)at] = (uint32_t)G.nodes();
        G.n_pos.push_back((uint32_t)a.t_pos); G.n_db.push_back((uint32_t)a.delta << 3 | base_code(a.q_base)); G.n_link0.push_back((uint32_t)G.links());
        size_t j = i;
        while (j < tags.size() && tags[j].t_pos == a.t_pos && tags[j].delta == a.delta && tags[j].q_base == a.q_base) {
            const Tag& b = tags[j];
            size_t k = j + 1;
            while (k < tags.size() && tags[k].t_pos == a.t_pos && tags[k].delta == a.delta && tags[k].q_base == a.q_base && tags[k].p_t_pos == b.p_t_pos &&
                   tags[k].p_delta == b.p_delta && tags[k].p_q_base == b.p_q_base) ++k;
            const uint32_t where = b.p_t_pos == -1 ? 0u : b.p_t_pos == b.t_pos ? 2u : 1u;
            G.l_pred.push_back(where << 19 | (uint32_t)b.p_delta << 3 | pred_code(b.p_q_base));
            G.l_count.push_back((uint32_t)(k - j));
            j = k;
        }
        if (a.delta == 0) G.cov[(size_t)a.t_pos] += (int32_t)(j - i);
        i = j;
    }
    for (; at <= size; ++at) G.pos_node[(size_t)at] = (uint32_t)G.nodes();
    G.n_link0.push_back((uint32_t)G.links());
}

// the node (delta, base code) at position pos; it exists: it is the tag of the column before
inline uint32_t find_node(const Graph& G, uint32_t pos, uint32_t db)
{
    uint32_t a = G.pos_node[pos], b = G.pos_node[pos + 1];
    while (a < b) { const uint32_t m = a + (b - a) / 2; if (G.n_db[m] < db) a = m + 1; else b = m; }
    return a;
}

// score pass and traceback: cns (characters with case) and t_pos
inline void best_path(const Graph& G, int min_cov, std::string& cns, std::vector<int32_t>& t_pos)
{
    cns.clear(); t_pos.clear();
    const size_t nn = G.nodes();
    std::vector<double> score(nn);
    std::vector<int32_t> pred(nn);
    double g_best = -1.0; int64_t g_node = -1; uint64_t g_visit = 0;
    for (size_t n = 0; n < nn; ++n) {
        const uint32_t pos = G.n_pos[n];
        double best = -1.0; int32_t best_p = -1;
        for (uint32_t l = G.n_link0[n]; l < G.n_link0[n + 1]; ++l) {
            const uint32_t w = G.l_pred[l], where = w >> 19;
            double s = (double)G.l_count[l] - 0.1 * G.cov[pos];
            int32_t p = -1;
            if (where) { p = (int32_t)find_node(G, where == 2 ? pos : pos - 1, (w & 0x7fff8u) | ((w & 7u) ? (w & 7u) - 1u : 0u)); s += score[(size_t)p]; }
            if (s > best) { best = s; best_p = p; }
        }
        score[n] = best; pred[n] = best_p;
        // visiting order inside a (position, delta) level: A C G T '-'; the array has '-' first
        const uint32_t bc = G.n_db[n] & 7u;
        const uint64_t visit = (uint64_t)pos << 19 | (uint64_t)(G.n_db[n] >> 3) << 3 | (bc ? bc - 1u : 4u);
        if (best > g_best || (best == g_best && g_node >= 0 && visit < g_visit)) { g_best = best; g_node = (int64_t)n; g_visit = visit; }
    }
    if (g_node < 0) return;
    uint32_t at = G.n_pos[(size_t)g_node];
    int32_t p = pred[(size_t)g_node];
    bool first = true;
    while (p != -1) {
        const uint32_t bc = G.n_db[(size_t)p] & 7u;
        if (!first) at = G.n_pos[(size_t)p];
        if (bc) { const char c = "ACGT"[bc - 1]; cns.push_back(G.cov[at] < min_cov ? (char)(c + 32) : c); t_pos.push_back((int32_t)at); }
        if (first) first = false; else p = pred[(size_t)p];
    }
    std::reverse(cns.begin(), cns.end());
    std::reverse(t_pos.begin(), t_pos.end());
}

// the polished segment: raw = the segment's bases as codes 0..3 (size of them)
template <class RawCode>
inline void splice(const std::string& cns, const std::vector<int32_t>& t_pos, RawCode raw, int size, int min_run, std::string& out)
{
    out.clear();
    auto put_raw = [&](int from, int to) { for (int x = from; x < to; ++x) out.push_back("ACGT"[raw(x) & 3u]); };
    auto lower = [](char c) { return c >= 'a' && c <= 'z'; };
    auto upper = [](char c) { return c >= 'A' && c <= 'Z'; };
    const size_t n = cns.size();
    int last = 0;
    size_t i = 0;
    while (i < n) {
        while (i < n && lower(cns[i])) ++i;
        if (i >= n) break;
        size_t j = i + 1;
        while (j < n && upper(cns[j])) ++j;
        if (j - i >= (size_t)min_run) {
            if (t_pos[i] > last) put_raw(last, t_pos[i]);
            out.append(cns, i, j - i);
            last = t_pos[j - 1] + 1;
        }
        i = j;
    }
    if (size > last) put_raw(last, size);
}

// one segment, start to end
struct SegmentOut { std::string cns; std::vector<int32_t> t_pos; uint64_t n_tags = 0, n_nodes = 0, n_links = 0; };
inline void segment_consensus(const OverlapIn* ov, size_t n_ov, int size, int min_cov, SegmentOut& out)
{
    std::vector<Tag> tags;
    for (size_t k = 0; k < n_ov; ++k) add_tags(ov[k], tags);
    Graph G;
    build_graph(tags, size, G);
    std::vector<Tag>().swap(tags);
    out.n_tags = G.n_tags; out.n_nodes = G.nodes(); out.n_links = G.links();
    best_path(G, min_cov, out.cns, out.t_pos);
}

}  // namespace ctg
}  // namespace necat_host
