// cns_dev_core.h - the consensus proper of oc2cns (tags -> backbone -> best path) as the DEVICE computes it: the per-lane cores of the kernels in
// cns_dev_kernels.h, written so that g++ builds the same functions for a CPU model of the device path (cns_dev::model_template below, tests/host_core/
// check_cns_device_model.cpp).  The host form of the stage is cns_consensus.h; the two differ in ONE respect: the order in which the weights of a link's tags are
// added up.  The host adds them in the order klib's unstable introsort leaves equal tags in (the reference's order); the device sorts on a TOTAL order - the six
// keys, then the overlap's index - and adds them in overlap-index order.  A sum of doubles depends on that order in its last bits, so every device number carries a
// bound on how far it can lie from the host's, and a template one of whose `>` decisions falls inside the bounds is handed back to the host code.
//
// The bounds (u = 2^-53, fl() = rounding to double; DESIGN 6b has the argument in full):
//   * link of c tags with weights w_1 .. w_c.  c <= 2: 0 + a is exact and a + b = b + a, so both orders give the same double: bound 0.  c >= 3: a recursive sum in
//     any order lies within g(c-1) S of the exact sum, S = sum |w_i|, g(n) = n u / (1 - n u) (Higham, Accuracy and Stability, 4.2), so two orders differ by at
//     most 2 g(c-1) S.  S itself is known as a computed sum S' >= S (1 - g(c-1)).  With c < 2^20: 2 g(c-1) / (1 - g(c-1)) <= 2 c u, so  E = 2 c u S'  holds.
//   * s = fl(a + b) with |a - a'| <= ea, |b - b'| <= eb (primed: the host's values): |s - s'| <= ea + eb + u |a + b| + u |a' + b'| <= (ea + eb)(1 + u) + 2 u |s| (1 + u).
//     err_add() returns (d + 4 u |s|)(1 + 1e-7) for d = ea + eb, which is larger - and EXACTLY 0 when d is 0: equal inputs give equal sums.
//   * a decision s1 > s2 (or its argmax form) is the host's decision whenever s1 - s2 > e1 + e2, and also when e1 + e2 = 0 (the values are the host's, bit for
//     bit).  certain() tests that with the margin's own rounding (relative u) covered by the factor 1 + 1e-7.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dev_common.h"

namespace necat {
namespace cns_dev {

// ---- the sort key of a tag: t_pos, delta, q_base, then p_t_pos, p_delta, p_q_base (AlignTag_LT, tasc/align_tags.c:6-18), then the overlap's index.
// Bases by their place in the reference's character order: '-' 0, A 1, C 2, G 3, T 4.  p_t_pos is -1 (first column of an overlap), t_pos - 1 or t_pos: 0 / 1 / 2.
constexpr int kPosBits = 24;                    // t_pos < 2^24 - 1 (the value 2^24 - 1 .. is free for the bucket of dropped overlaps)
constexpr u32 kMaxTsize = (1u << kPosBits) - 2;
constexpr u32 kMaxOverlaps = 65535;             // overlap index in 16 bits
constexpr double kU = 1.1102230246251565e-16;   // 2^-53
constexpr double kSlack = 1.0000001;
// A link bound above this does not certify anything: the reference's weights lie in (0, 1] (calc_cns_weight, consensus/consensus_one_read.c:11-16) and a template has at most
// 300 overlaps (MAX_EXAMINED_CAN), so 2 c u S' stays below 2 * 300^2 * u = 2e-11; a larger one means weights or counts the analysis above does not cover, and the template
// goes to the host (flag 2; the test is written so that a NaN bound fails it).  The bound NECAT_CNS_TOL_SCALE has multiplied is held against it as well (flag 4): a bound
// that loose certifies nothing, so a scale of 1e7 sends every template to the host whatever its comparisons say.  Flag 1 - a comparison inside the bounds, certain() - is
// worked out for every template regardless of the other two, and counted on its own (necat_cns_consensus::n_uncertain), so that tests can see certain() decide.
constexpr double kMaxLinkErr = 9.313225746154785e-10;      // 2^-30

NECAT_HD u64 tag_key(u32 t_pos, u32 delta, u32 qs, u32 pp, u32 p_delta, u32 p_qs, u32 ovl)
{
    return (u64)t_pos << 40 | (u64)delta << 32 | (u64)qs << 29 | (u64)pp << 27 | (u64)p_delta << 19 | (u64)p_qs << 16 | (u64)ovl;
}
NECAT_HD u32 key_pos(u64 k) { return (u32)(k >> 40); }
NECAT_HD u32 key_delta(u64 k) { return (u32)(k >> 32) & 255u; }
NECAT_HD u32 key_qs(u64 k) { return (u32)(k >> 29) & 7u; }
NECAT_HD u32 key_pp(u64 k) { return (u32)(k >> 27) & 3u; }
NECAT_HD u32 key_ovl(u64 k) { return (u32)k & 0xffffu; }
NECAT_HD u64 key_link(u64 k) { return k >> 16; }          // equal: same link (all six keys)
NECAT_HD u64 key_node(u64 k) { return k >> 29; }          // equal: same node (t_pos, delta, q_base)
NECAT_HD u64 key_pred_node(u64 k, u32 pos) { return (u64)pos << 11 | ((k >> 19) & 255u) << 3 | ((k >> 16) & 7u); }      // the node key of the predecessor at position pos
// q_base of a node in the reference's visiting order (encode_dna_base: A C G T 0..3, '-' 4) from its sort code
NECAT_HD u32 visit_code(u32 qs) { return qs ? qs - 1u : 4u; }

// ---- one column of an overlap (get_cns_tags, tasc/align_tags.c:44-70).  What the column needs from the columns before it: how many target bases and query
// bases came before (tcnt, qcnt: exclusive counts) and the index of the last column with a target base (last_t, -1: none).  op: 0 match, 1 query base over '-',
// 2 '-' over target base, 3 mismatch.  The kernel gets the three from wave scans, the model from a loop.
struct ColState { i32 tcnt, qcnt, last_t; };
struct ColTag { i32 t_pos; u32 delta, qs; };
template <class QBase>
NECAT_HD ColTag col_tag(int op, i32 i, const ColState& before, i32 toff, QBase qbase)
{
    ColTag t;
    const i32 tc = before.tcnt + (op != 1 ? 1 : 0);
    const i32 lt = op != 1 ? i : before.last_t;
    t.t_pos = toff - 1 + tc;
    t.delta = (u32)(i - lt);
    t.qs = op != 2 ? 1u + ((u32)qbase(before.qcnt) & 3u) : 0u;
    return t;
}
NECAT_HD void col_advance(int op, i32 i, ColState& s) { if (op != 1) { ++s.tcnt; s.last_t = i; } if (op != 2) ++s.qcnt; }

// the key of a column's tag given the previous column's (prev.t_pos = -1 before the first: p_delta 0, p_q_base '-')
NECAT_HD u64 col_key(const ColTag& t, const ColTag& prev, bool first, u32 ovl)
{
    const u32 pp = first ? 0u : (prev.t_pos == t.t_pos ? 2u : 1u);
    return tag_key((u32)t.t_pos, t.delta, t.qs, pp, first ? 0u : prev.delta, first ? 0u : prev.qs, ovl);
}

// base i of a read of the volume (2 bits per base, base g in bits 2 (g & 31) of word g >> 5), on the strand asked for
NECAT_HD u32 strand_base(const u64* words, u64 read_begin, i32 qsize, i32 qdir, i32 i)
{
    const u64 g = read_begin + (u64)(qdir ? qsize - 1 - i : i);
    const u32 b = (u32)(words[g >> 5] >> ((g & 31) * 2)) & 3u;
    return qdir ? 3u - b : b;
}

// ---- error bounds
NECAT_HD double err_add(double d, double s) { return d == 0.0 ? 0.0 : (d + 4.0 * kU * fabs(s)) * kSlack; }
// is "hi beats lo" (hi >= lo as computed) also the host's decision?
NECAT_HD bool certain(double hi, double e_hi, double lo, double e_lo)
{
    const double e = e_hi + e_lo;
    return !(e > 0.0) || (hi - lo) > e * kSlack;
}

// ---- one link: the tags keys[g .. ) of a bucket ending at `end` that share all six keys.  weight = their overlaps' weights added in array order (= overlap-index
// order: the index is the key's last field), err = the bound above, UNSCALED: the caller holds it against kMaxLinkErr as it is and multiplies what the scores carry by
// NECAT_CNS_TOL_SCALE (tests drive templates through certain() with it)
NECAT_HD u32 link_sum(const u64* keys, u32 g, u32 end, const double* ovl_weight, double* weight, double* err)
{
    const u64 lk = key_link(keys[g]);
    double s = 0.0, a = 0.0;
    u32 h = g;
    while (h < end && key_link(keys[h]) == lk) { const double w = ovl_weight[key_ovl(keys[h])]; s += w; a += fabs(w); ++h; }
    const u32 c = h - g;
    *weight = s;
    *err = c <= 2 ? 0.0 : 2.0 * (double)c * kU * a;
    return c;
}

// first tag of keys[lo, hi) (one bucket, sorted) whose node key is nk, or -1
NECAT_HD i64 find_node_tag(const u64* keys, u32 lo, u32 hi, u64 nk)
{
    u32 a = lo, b = hi;
    while (a < b) { const u32 m = a + (b - a) / 2; if (key_node(keys[m]) < nk) a = m + 1; else b = m; }
    return a < hi && key_node(keys[a]) == nk ? (i64)a : -1;
}

// ---- the backbone as flat arrays (indices global in a chunk; one template owns a contiguous range of each)
struct Graph {
    const double* l_w; const double* l_e; const i32* l_pred;          // links: weight, bound, predecessor node (-1: none)
    const u32* n_lfirst; const u32* n_nlink; const i32* n_pos; const u32* n_dc;      // nodes: links, position, delta << 3 | visit code
    double* n_score; double* n_err; i32* n_best;
};

// One node of the best-path recurrence (consensus_backbone_segment, tasc/cns_aux.c:150-176): the reference's `score > best_score` walk over the node's links in
// array order, best_score starting at -1.  Returns false when the host might decide otherwise.
NECAT_HD bool node_best(const Graph& G, u32 n, int coverage)
{
    const u32 lf = G.n_lfirst[n], nl = G.n_nlink[n];
    double best = -1.0, best_e = 0.0;
    i32 best_p = -1; u32 best_at = 0xffffffffu;
    for (u32 c = 0; c < nl; ++c) {
        const u32 l = lf + c;
        double s = G.l_w[l] - 0.4 * 0.5 * coverage;
        double e = err_add(G.l_e[l], s);
        const i32 p = G.l_pred[l];
        if (p != -1) { const double ps = G.n_score[p]; s += ps; e = err_add(e + G.n_err[p], s); }
        if (s > best) { best = s; best_e = e; best_p = p; best_at = c; }
    }
    bool ok = true;
    if (best_at != 0xffffffffu && !certain(best, best_e, -1.0, 0.0)) ok = false;
    for (u32 c = 0; c < nl; ++c) {             // every other link must lose on the host as well (and none may pass -1 there when none did here)
        if (c == best_at) continue;
        const u32 l = lf + c;
        double s = G.l_w[l] - 0.4 * 0.5 * coverage;
        double e = err_add(G.l_e[l], s);
        const i32 p = G.l_pred[l];
        if (p != -1) { const double ps = G.n_score[p]; s += ps; e = err_add(e + G.n_err[p], s); }
        if (!certain(best, best_e, s, e)) ok = false;
    }
    G.n_score[n] = best; G.n_err[n] = best_e; G.n_best[n] = best_p;
    return ok;
}

// the global best of a stretch: strict > in visiting order (position, delta, base A C G T '-'), i. e. the largest score, the earliest node among equals
NECAT_HD u64 visit_key(i32 pos, u32 dc) { return (u64)(u32)pos << 11 | dc; }
NECAT_HD bool better(double s, u64 vk, double bs, u64 bvk) { return s > bs || (s == bs && vk < bvk); }

// traceback (tasc/cns_aux.c:187-207) from node g: base codes written BACKWARDS ending at out_end (so they read forwards); returns the length, *cfrom as the reference's.
// The node whose predecessor is -1 is never emitted; gap nodes (code 4) are skipped.
NECAT_HD u32 traceback(const Graph& G, i32 g, u8* out_end, i32* cfrom)
{
    u32 len = 0;
    *cfrom = 0;
    while (g != -1) {
        const u32 code = G.n_dc[g] & 7u;
        const i32 p = G.n_best[g];
        if (p == -1) break;
        *cfrom = G.n_pos[p];
        if (code != 4u) { ++len; *(out_end - len) = (u8)code; }
        g = p;
    }
    return len;
}

struct Seg { i32 left, right, cns_from, cns_to; u32 off, len; };      // one kept stretch; off: where its bases start in the chunk's base blob
// an overlap and a template of a chunk, as the kernels (cns_dev_kernels.h) read them
struct DevOvl { u64 ops_off, read_begin; double weight; i32 ncols, toff, qsize, qoff, qdir; u32 tmpl, k, tag_base; };
struct DevTmpl { u32 tag_base, ntags, pos_base; i32 tsize; u32 ov_base, n_ov, seg_base, seg_cap; };

}  // namespace cns_dev
}  // namespace necat

#if !defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the CPU model of the device path (tests only)
#include <algorithm>
#include <string>
#include <vector>

namespace necat {
namespace cns_dev {

struct ModelOverlap { const u8* ops; i32 ncols, toff; double weight; const u64* words; u64 read_begin; i32 qsize, qoff, qdir; };
struct ModelLink { double weight, err; u32 count; };
struct ModelSeg { i32 left, right, cns_from, cns_to; std::string seq; };
struct ModelOut {
    std::vector<ModelSeg> segs; std::vector<ModelLink> links;
    bool flagged = false;        // flags != 0: the host recomputes the template
    bool uncertain = false;      // a `>` decision inside the error bounds (the kernels' flag 1)
    bool bad = false;            // a bound or an array the analysis does not cover (the kernels' flag 2)
    bool loose = false;          // a scaled link bound above kMaxLinkErr (the kernels' flag 4)
    double max_err = 0;          // largest link bound, unscaled
    std::vector<double> n_score, n_err; std::vector<i32> n_pos; std::vector<u32> n_dc; std::vector<uint8_t> n_scored;      // the nodes: score, its bound (scaled), was it scored
};

// the kernels' steps in the kernels' order, one template, one thread
inline void model_template(const ModelOverlap* ov, size_t n_ov, int tsize, int min_cov, int min_size, double tol, ModelOut& out)
{
    out = ModelOut();
    std::vector<u64> keys;
    std::vector<double> w(n_ov);
    for (size_t k = 0; k < n_ov; ++k) {                                      // k_cns_tags
        const ModelOverlap& o = ov[k];
        w[k] = o.weight;
        auto op_at = [&](int i) { return (o.ops[i >> 2] >> ((i & 3) * 2)) & 3; };
        auto qb = [&](i32 i) { return strand_base(o.words, o.read_begin, o.qsize, o.qdir, o.qoff + i); };
        ColState st = {0, 0, -1};
        bool dropped = false;
        for (i32 i = 0; i < o.ncols; ++i) { const int op = op_at(i); if (col_tag(op, i, st, o.toff, [](i32) { return 0u; }).delta >= 255u) dropped = true; col_advance(op, i, st); }
        if (dropped) continue;
        st = {0, 0, -1};
        ColTag prev = {-1, 0, 0};
        for (i32 i = 0; i < o.ncols; ++i) {
            const int op = op_at(i);
            const ColTag t = col_tag(op, i, st, o.toff, qb);
            col_advance(op, i, st);
            if (t.t_pos >= 0 && t.t_pos < tsize) keys.push_back(col_key(t, prev, i == 0, (u32)k));
            prev = t;
        }
    }
    std::sort(keys.begin(), keys.end());                                     // k_cns_hist .. k_cns_sort: the total order
    const u32 nt = (u32)keys.size();
    std::vector<u32> off((size_t)tsize + 1, 0);
    for (u64 k : keys) ++off[key_pos(k) + 1];
    for (int p = 0; p < tsize; ++p) off[p + 1] += off[p];
    // k_cns_backbone
    std::vector<u32> node_of_tag(nt), n_lfirst, n_nlink, n_dc; std::vector<i32> n_pos, l_pred, cov((size_t)tsize, 0);
    std::vector<double> l_w, l_e;
    for (u32 i = 0; i < nt; ++i) {
        const bool first = i == 0, new_node = first || key_node(keys[i]) != key_node(keys[i - 1]), new_link = first || key_link(keys[i]) != key_link(keys[i - 1]);
        const u32 pos = key_pos(keys[i]);
        if (new_node) { n_lfirst.push_back((u32)l_w.size()); n_pos.push_back((i32)pos); n_dc.push_back(key_delta(keys[i]) << 3 | visit_code(key_qs(keys[i]))); }
        node_of_tag[i] = (u32)n_pos.size() - 1;
        if (new_link) {
            double lw, le;
            const u32 c = link_sum(keys.data(), i, off[pos + 1], w.data(), &lw, &le);
            l_w.push_back(lw); l_e.push_back(le * tol); out.links.push_back({lw, le, c});
            out.max_err = std::max(out.max_err, le);
            if (!(le <= kMaxLinkErr)) out.bad = true;
            else if (!(le * tol <= kMaxLinkErr)) out.loose = true;
            const u32 pp = key_pp(keys[i]);
            i64 pt = -1;
            if (pp) {
                if (pp == 1 && pos == 0) out.bad = true;
                else {
                    const u32 ppos = pp == 2 ? pos : pos - 1;
                    pt = find_node_tag(keys.data(), off[ppos], off[ppos + 1], key_pred_node(keys[i], ppos));
                    if (pt < 0) out.bad = true;
                }
            }
            l_pred.push_back((i32)pt);           // (a tag index until the nodes are numbered)
        }
        if (key_delta(keys[i]) == 0 && (i + 1 == off[pos + 1] || key_delta(keys[i + 1]) != 0)) cov[pos] = (i32)(i - off[pos] + 1);
    }
    const u32 nn = (u32)n_pos.size(), nl = (u32)l_w.size();
    n_nlink.resize(nn);
    for (u32 n = 0; n < nn; ++n) n_nlink[n] = (n + 1 < nn ? n_lfirst[n + 1] : nl) - n_lfirst[n];
    for (u32 l = 0; l < nl; ++l) if (l_pred[l] >= 0) l_pred[l] = (i32)node_of_tag[(u32)l_pred[l]];
    std::vector<double> n_score(nn, 0.0), n_err(nn, 0.0); std::vector<i32> n_best(nn, -1);
    std::vector<uint8_t> n_scored(nn, 0);
    Graph G = {l_w.data(), l_e.data(), l_pred.data(), n_lfirst.data(), n_nlink.data(), n_pos.data(), n_dc.data(), n_score.data(), n_err.data(), n_best.data()};
    auto node_at = [&](int p) { return p >= tsize ? nn : (off[p] < nt ? node_of_tag[off[p]] : nn); };     // first node at or after position p
    std::vector<u8> buf;
    // k_cns_path
    int i = 0;
    while (i < tsize) {
        while (i < tsize && cov[i] < min_cov) ++i;
        int j = i + 1;
        while (j < tsize && cov[j] >= min_cov) ++j;
        if (i < tsize && j - i >= min_size * 0.85) {
            const u32 n0 = node_at(i), n1 = node_at(j);
            double bs = -1.0, be = 0.0; u64 bvk = ~0ull; i32 bn = -1;
            for (u32 n = n0; n < n1; ++n) {
                if (!node_best(G, n, cov[n_pos[n]])) out.uncertain = true;
                n_scored[n] = 1;
                const u64 vk = visit_key(n_pos[n], n_dc[n]);
                if (n_score[n] > -1.0 && better(n_score[n], vk, bs, bvk)) { bs = n_score[n]; be = n_err[n]; bvk = vk; bn = (i32)n; }
            }
            for (u32 n = n0; n < n1; ++n) if ((i32)n != bn && !certain(bs, be, n_score[n], n_err[n])) out.uncertain = true;
            if (bn >= 0 && !certain(bs, be, -1.0, 0.0)) out.uncertain = true;
            buf.assign((size_t)(n1 - n0) + 1, 0);
            ModelSeg sg;
            const u32 len = bn >= 0 ? traceback(G, bn, buf.data() + buf.size(), &sg.cns_from) : 0;
            if (bn < 0) sg.cns_from = 0;
            sg.cns_to = bn >= 0 ? n_pos[bn] + 1 : 1;
            if ((int)len >= min_size) { sg.left = i; sg.right = j; sg.seq.assign((const char*)buf.data() + buf.size() - len, len); out.segs.push_back(sg); }
        }
        i = j;
    }
    out.flagged = out.uncertain || out.bad || out.loose;
    out.n_score = n_score; out.n_err = n_err; out.n_pos = n_pos; out.n_dc = n_dc; out.n_scored = n_scored;
}

}  // namespace cns_dev
}  // namespace necat
#endif
