// check_asm_ends.cpp - CPU model of the device form of oc2asmpm's end extension (necat_amd/csrc/asm_ends_core.h: plan_ends, finish_ends, with dal_core.h's wave for the
// DALIGNER jobs, run lane by lane as tests/host_core/check_dalign.cpp runs it) against the host code, asm_core.h Extender::ends (gapped strings) and
// Extender::ends_packed (packed columns): equality of the four coordinates, the identity and which ends were extended, for every alignment.
//
//   check_asm_ends golden CAP1 CAP2 [map options] wrk_dir volume_id     the alignments of check_asmpm.cpp's batch walk on a volume directory (oracle reader, lookup table and
//                                                                       block aligner); link with oracle/necat_oracle.c
//   check_asm_ends crafted CAP1 CAP2 SEED N                             N made-up alignments: a related core with unrelated prefixes / suffixes of 20 - 299 bases at the anchor
//                                                                       on both sequences, cores below 400 columns and below 65 %, and hand-made column streams
//                                                                       (no run of 8 anywhere, from >= to); then 12 alignments with an end that the host
//                                                                       code tries and declines, and made-up tips
// A job runs at CAP1 diagonals, an over-capacity one again at CAP2, what is still flagged is the host code's.
// Last line of stdout: key=value pairs - the model's branch counts (tried_l= ...) and the host code's (h_tried_l= ...).  Exit status 1 on any difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../necat_amd/csrc/asm_core.h"
#include "../../necat_amd/csrc/asm_ends_core.h"
#ifdef CHECK_ASM_ENDS_ORACLE
#include "../../oracle/necat_oracle.h"
#endif

using namespace necat;

namespace {

constexpr int kGuard = 4;

struct Volume {
    std::vector<u64> words;           // 2-bit little-endian words with guard words on both sides
    const u64* bases() const { return words.data() + kGuard; }
    void set(const std::vector<u8>& codes)
    {
        words.assign((codes.size() + 31) / 32 + 2 * kGuard, 0);
        for (size_t i = 0; i < codes.size(); ++i) words[kGuard + i / 32] |= (u64)(codes[i] & 3) << (2 * (i % 32));
    }
};

struct Side { uint64_t tried = 0, extended = 0, hang0 = 0, hang_long = 0, no_run = 0, declined = 0; };      // declined: a job, and no extension
struct Counters {
    uint64_t cases = 0, bad = 0, ok = 0, low_ident = 0, both = 0, from_ge_to = 0, jobs = 0, tier1 = 0, tier2 = 0, host = 0, steps = 0;
    int max_diags = 0;
    Side m[2], h[2];                  // the model's, the host code's
    uint64_t h_both = 0;
};

// dal_kernels.h wave_dir, the 64 lanes in a loop (as tests/host_core/check_dalign.cpp)
template <int DIR>
dal::Out wave_dir(const u64* abases, const u64* bbases, const dal::Task& T, const dal::Spec& S, int cap)
{
    const int R = dal::ring_size(cap);
    std::vector<int> V((size_t)2 * R), M((size_t)2 * R);
    std::vector<u64> Tt((size_t)2 * R);
    dal::Ring W; W.V = V.data(); W.M = M.data(); W.T = Tt.data(); W.mask = R - 1;
    dal::Fold F;
    dal::wave0<DIR>(F, W, abases, bbases, T);
    if (!F.more) dal::clip<DIR>(F, W, 0, abases, bbases, T);
    int cur = 0, flag = 0, steps = 0, max_diags = 1;
    while (dal::goes_on<DIR>(F)) {
        const int ol = F.low, oh = F.hgh;
        flag = dal::step_begin(F, cap, T);
        if (flag & (dal::kFlagEmpty | dal::kFlagStale)) break;
        const int w = F.hgh - F.low + 1;
        if (w > max_diags) max_diags = w;
        if (flag) break;
        const int nw = cur ^ 1;
        u64 stale = 0;
        for (int base = 0; base < w; base += dal::kLanes) {
            const int k_first = DIR > 0 ? F.hgh - base : F.low + base;
            dal::LaneOut o[dal::kLanes];
            for (int l = 0; l < dal::kLanes; ++l) {
                o[l] = dal::lane_idle<DIR>();
                if (base + l < w) o[l] = dal::lane_point<DIR>(W, cur, ol, oh, k_first - DIR * l, abases, bbases, T);
            }
            for (int l = 0; l < dal::kLanes; ++l) if (base + l < w) dal::lane_store(W, nw, k_first - DIR * l, o[l]);
            u64 rec = 0, good = 0, trim = 0, hit_a = 0, hit_b = 0;
            int run = dal::worst<DIR>();
            for (int l = 0; l < dal::kLanes; ++l) {
                const int r = dal::better<DIR>(run, F.besta) ? run : F.besta;
                const int cls = base + l < w ? dal::lane_class<DIR>(S, o[l], r) : 0;
                if (cls & dal::kRecord) rec |= 1ULL << l;
                if (cls & dal::kGood) good |= 1ULL << l;
                if (cls & dal::kTrim) trim |= 1ULL << l;
                if (o[l].flags & dal::kHitA) hit_a |= 1ULL << l;
                if (o[l].flags & dal::kHitB) hit_b |= 1ULL << l;
                if (o[l].flags & dal::kStale) stale |= 1ULL << l;
                if (dal::better<DIR>(o[l].c, run)) run = o[l].c;
            }
            dal::fold_chunk<DIR>(F, k_first, rec, good, trim, hit_a, hit_b, [&](int l, int* c, int* y) { *c = o[l].c; *y = o[l].y; });
        }
        if (stale) { flag = dal::kFlagStale; break; }
        if (!F.more) dal::clip<DIR>(F, W, nw, abases, bbases, T);
        if (F.hgh >= F.low) {
            int lo = INT_MAX, hi = INT_MIN;
            for (int k = F.low; k <= F.hgh; ++k)
                if (dal::lane_stays<DIR>(F, W.V[W.at(nw, k)])) { if (lo == INT_MAX) lo = k; hi = k; }
            dal::lag_trim(F, lo, hi);
        }
        cur = nw;
        ++steps;
    }
    const dal::Tip t = dal::tip_of(F);
    dal::Out out; out.a = t.a; out.y = t.y; out.d = t.d; out.flag = flag; out.steps = steps; out.max_diags = max_diags;
    return out;
}

struct Checker {
    int cap1, cap2;
    Counters n;
    rescue::DalignSpec hs = rescue::spec_for_error(0.35);
    asmpm::Extender ext_strings, ext_packed;

    // a job as necat_asm_map_batch runs it: the first capacity, the second for what outgrew the first, the host code (stage_dalign.inl: dal_solve)
    void solve(const Volume& va, const Volume& vb, const dal::Task& T, dal::Out* f, dal::Out* b)
    {
        dal::Spec S; S.ave_path = hs.ave_path; S.table = hs.table.data(); S.score = hs.score.data();
        ++n.jobs;
        const int caps[2] = {cap1, cap2};
        for (int tier = 0; tier < (cap1 < cap2 ? 2 : 1); ++tier) {
            *f = wave_dir<+1>(va.bases(), vb.bases(), T, S, caps[tier]);
            *b = wave_dir<-1>(va.bases(), vb.bases(), T, S, caps[tier]);
            n.steps += (uint64_t)f->steps + (uint64_t)b->steps;
            const int flags = f->flag | b->flag;
            if (!flags) { ++(tier ? n.tier2 : n.tier1); n.max_diags = std::max(n.max_diags, std::max(f->max_diags, b->max_diags)); return; }
            if (flags & (dal::kFlagStale | dal::kFlagEmpty)) break;
        }
        ++n.host;
        std::vector<u8> qs((size_t)T.a.len), ts((size_t)T.b.len);
        dal::WordCache wc; wc.w = LLONG_MIN; wc.v = 0;
        for (int i = 0; i < T.a.len; ++i) qs[(size_t)i] = (u8)dal::seq_at(va.bases(), T.a, i, wc);
        wc.w = LLONG_MIN;
        for (int i = 0; i < T.b.len; ++i) ts[(size_t)i] = (u8)dal::seq_at(vb.bases(), T.b, i, wc);
        rescue::Dalign D(hs);
        (void)D.go((const char*)qs.data(), (T.mida + T.k0) / 2, T.a.len, (const char*)ts.data(), (T.mida - T.k0) / 2, T.b.len, 1);
        f->a = D.r.aepos + D.r.bepos; f->y = D.r.bepos; f->d = D.r.diffs; f->flag = 0;
        b->a = D.r.abpos + D.r.bbpos; b->y = D.r.bbpos; b->d = 0; b->flag = 0;
    }

    // q: the read; t: the subject ON ITS STRAND; a: the block alignment with its strings; ok: it has at least 400 columns
    void one(const std::vector<u8>& q, const std::vector<u8>& t, int sdir, bool ok, const asmpm::BlockAlignment& a, int qext, int sext)
    {
        ++n.cases;
        const int cols = (int)a.qaln.size(), qsize = (int)q.size(), tsize = (int)t.size();
        // ---- the device's view: volumes of 2-bit words (the subject stored forward), the finished task, the column region in the aligner's stream layout
        const int qpad = 37, tpad = 91;       // the sequences do not start their volumes
        std::vector<u8> rv((size_t)qpad, 2), sv((size_t)tpad, 1);
        rv.insert(rv.end(), q.begin(), q.end()); rv.push_back(3);
        for (int i = 0; i < tsize; ++i) sv.push_back(sdir ? (u8)(3 - t[(size_t)(tsize - 1 - i)]) : t[(size_t)i]);
        sv.push_back(0);
        Volume va, vb; va.set(rv); vb.set(sv);
        ExtTask x;
        memset(&x, 0, sizeof x);
        x.q_g0 = qpad; x.s_g0 = tpad; x.qlen = qsize; x.slen = tsize; x.sdir = sdir; x.phase = 2;
        x.r_qoff = a.qoff; x.r_qend = a.qend; x.r_toff = a.toff; x.r_tend = a.tend; x.r_cols = cols;
        int mat = 0;
        for (int i = 0; i < cols; ++i) mat += a.qaln[(size_t)i] == a.taln[(size_t)i];
        x.r_mat = mat;
        const int split = cols / 3;
        x.s_lfrom = 5; x.s_lto = 5 + split; x.s_rfrom = 3; x.s_rto = 3 + (cols - split);
        std::vector<u64> reg((size_t)(x.s_lto + x.s_rto) / 32 + 2, ~0ULL);        // (columns outside the two kept ranges: all ones)
        auto put = [&](int src, int op) { reg[(size_t)src >> 5] = (reg[(size_t)src >> 5] & ~(3ULL << ((src & 31) * 2))) | ((u64)op << ((src & 31) * 2)); };
        std::vector<u8> packed((size_t)(cols + 3) / 4 + 1, 0);
        for (int j = 0; j < cols; ++j) {
            const int op = a.qaln[(size_t)j] == '-' ? 2 : a.taln[(size_t)j] == '-' ? 1 : 0;
            put(j < split ? x.s_lto - 1 - j : x.s_lto + x.s_rfrom + (j - split), op);
            packed[(size_t)j >> 2] |= (u8)(op << ((j & 3) * 2));
        }
        // ---- the model
        dal::Task T[2];
        aends::Plan p = aends::plan_ends(x, va.bases(), vb.bases(), reg.data(), 400, 65.0, T);
        std::vector<dal::Out> outs;
        for (int side = 0; side < 2; ++side) {
            if (!((p.state >> aends::side_shift(side)) & aends::kJob)) continue;
            p.job[side] = (i32)(outs.size() / 2);
            outs.resize(outs.size() + 2);
            solve(va, vb, T[side], &outs[outs.size() - 2], &outs[outs.size() - 1]);
        }
        necat_m4 m;
        int ext[2];
        const bool has = aends::finish_ends(x, p, outs.data(), qext, sext, &m, ext);
        if (p.state & aends::kOk) ++n.ok;
        if (p.state & aends::kLowIdent) ++n.low_ident;
        for (int side = 0; side < 2; ++side) {
            const int b = p.state >> aends::side_shift(side);
            n.m[side].tried += (b & aends::kTried) != 0; n.m[side].hang0 += (b & aends::kHang0) != 0; n.m[side].hang_long += (b & aends::kHangLong) != 0;
            n.m[side].no_run += (b & aends::kNoRun) != 0; n.m[side].extended += ext[side]; n.m[side].declined += (b & aends::kJob) && !ext[side];
        }
        n.both += ext[0] && ext[1];
        if (has && p.from >= p.to) ++n.from_ge_to;
        // ---- the host code, on the strings and on the packed columns
        const bool want = ok && a.ident_perc >= 65.0;
        bool same = has == want;
        if (ok && a.ident_perc != (cols ? 100.0 * (double)mat / (double)cols : 0.0)) same = false;      // (the aligner's identity is the columns')
        if (want && same) {
            asmpm::BlockAlignment s1 = a, s2 = a;
            s2.qaln.clear(); s2.taln.clear();
            ext_strings.ends(q.data(), qsize, t.data(), tsize, s1);
            ext_packed.ends_packed(q.data(), qsize, t.data(), tsize, packed.data(), (size_t)cols, s2);
            const int ls = std::min(a.qoff, a.toff), rs = std::min(qsize - a.qend, tsize - a.tend);
            const int hang[2] = {ls, rs};
            for (int side = 0; side < 2; ++side) {
                n.h[side].hang0 += hang[side] == 0; n.h[side].hang_long += hang[side] > 300; n.h[side].tried += hang[side] != 0 && hang[side] <= 300;
                n.h[side].extended += ext_strings.last_ext[side];
                if (ext_strings.last_ext[side] != ext_packed.last_ext[side] || (int)ext_strings.last_ext[side] != ext[side]) same = false;
            }
            // (no run of 8 equal columns = the same from either end)
            int run = 0, best = 0;
            for (int i = 0; i < cols; ++i) { run = a.qaln[(size_t)i] == a.taln[(size_t)i] ? run + 1 : 0; best = std::max(best, run); }
            for (int side = 0; side < 2; ++side) {
                const bool tried = hang[side] != 0 && hang[side] <= 300;
                n.h[side].no_run += tried && best < 8; n.h[side].declined += tried && best >= 8 && !ext_strings.last_ext[side];
            }
            n.h_both += ext_strings.last_ext[0] && ext_strings.last_ext[1];
            uint64_t so = (uint64_t)s1.toff, se = (uint64_t)s1.tend;
            if (sdir == 1) { so = (uint64_t)tsize - (uint64_t)s1.tend; se = (uint64_t)tsize - (uint64_t)s1.toff; }
            if (s1.qoff != s2.qoff || s1.qend != s2.qend || s1.toff != s2.toff || s1.tend != s2.tend || s1.ident_perc != s2.ident_perc) same = false;
            if (m.qoff != (uint64_t)s1.qoff || m.qend != (uint64_t)s1.qend || m.soff != so || m.send != se || m.ident_perc != s1.ident_perc) same = false;
            if (m.qext != (uint64_t)qext || m.sext != (uint64_t)sext || m.qsize != (uint64_t)qsize || m.ssize != (uint64_t)tsize || m.sdir != sdir || m.qdir != 0) same = false;
            if (!same)
                fprintf(stderr, "case %lu: model %lu %lu %lu %lu %.17g ext %d %d, strings %d %d %lu %lu %.17g ext %d %d, packed %d %d %d %d %.17g\n", (unsigned long)n.cases - 1,
                        (unsigned long)m.qoff, (unsigned long)m.qend, (unsigned long)m.soff, (unsigned long)m.send, m.ident_perc, ext[0], ext[1], s1.qoff, s1.qend, (unsigned long)so,
                        (unsigned long)se, s1.ident_perc, (int)ext_strings.last_ext[0], (int)ext_strings.last_ext[1], s2.qoff, s2.qend, s2.toff, s2.tend, s2.ident_perc);
        } else if (!same) fprintf(stderr, "case %lu: model %s a record, the host code %s\n", (unsigned long)n.cases - 1, has ? "has" : "has not", want ? "has" : "has not");
        if (!same) ++n.bad;
    }

    int report()
    {
        printf("cases=%lu bad=%lu ok=%lu low_ident=%lu both=%lu h_both=%lu from_ge_to=%lu jobs=%lu tier1=%lu tier2=%lu host=%lu steps=%lu max_diags=%d", (unsigned long)n.cases,
               (unsigned long)n.bad, (unsigned long)n.ok, (unsigned long)n.low_ident, (unsigned long)n.both, (unsigned long)n.h_both, (unsigned long)n.from_ge_to, (unsigned long)n.jobs,
               (unsigned long)n.tier1, (unsigned long)n.tier2, (unsigned long)n.host, (unsigned long)n.steps, n.max_diags);
        const char* names[2] = {"l", "r"};
        for (int side = 0; side < 2; ++side) {
            printf(" tried_%s=%lu extended_%s=%lu hang0_%s=%lu hang_long_%s=%lu no_run_%s=%lu", names[side], (unsigned long)n.m[side].tried, names[side], (unsigned long)n.m[side].extended,
                   names[side], (unsigned long)n.m[side].hang0, names[side], (unsigned long)n.m[side].hang_long, names[side], (unsigned long)n.m[side].no_run);
            printf(" declined_%s=%lu h_declined_%s=%lu", names[side], (unsigned long)n.m[side].declined, names[side], (unsigned long)n.h[side].declined);
            printf(" h_tried_%s=%lu h_extended_%s=%lu h_hang0_%s=%lu h_hang_long_%s=%lu h_no_run_%s=%lu", names[side], (unsigned long)n.h[side].tried, names[side],
                   (unsigned long)n.h[side].extended, names[side], (unsigned long)n.h[side].hang0, names[side], (unsigned long)n.h[side].hang_long, names[side], (unsigned long)n.h[side].no_run);
        }
        printf("\n");
        return n.bad ? 1 : 0;
    }
};

// ---- crafted alignments ---------------------------------------------------------------------------------------------------------------

typedef std::mt19937_64 Rng;
int uni(Rng& g, int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }      // [lo, hi]
void random_bases(Rng& g, int n, std::vector<u8>& out) { for (int i = 0; i < n; ++i) out.push_back((u8)(g() & 3)); }

// A core of `len` read bases copied into the subject with substitutions, insertions and deletions at rate err, its first and last `edge` columns equal;
// appends the core's bases to q and t and its columns to the strings.  stride > 0 instead: a substitution every stride-th column, nothing else.
void core(Rng& g, int len, double err, int edge, int stride, std::vector<u8>& q, std::vector<u8>& t, std::string& qa, std::string& ta)
{
    const char* L = "ACGT";
    for (int i = 0; i < len; ++i) {
        const u8 c = (u8)(g() & 3);
        const bool inner = i >= edge && i < len - edge;
        const double r = (double)(g() >> 11) / 9007199254740992.0;
        if (stride > 0) {
            const u8 d = (i % stride) == stride - 1 ? (u8)((c + 1) & 3) : c;
            q.push_back(c); t.push_back(d); qa.push_back(L[c]); ta.push_back(L[d]);
        } else if (inner && r < err / 3) { const u8 d = (u8)((c + 1 + (g() % 3)) & 3); q.push_back(c); t.push_back(d); qa.push_back(L[c]); ta.push_back(L[d]); }
        else if (inner && r < 2 * err / 3) { q.push_back(c); qa.push_back(L[c]); ta.push_back('-'); }
        else if (inner && r < err) { const u8 d = (u8)(g() & 3); t.push_back(d); qa.push_back('-'); ta.push_back(L[d]); q.push_back(c); t.push_back(c); qa.push_back(L[c]); ta.push_back(L[c]); }
        else { q.push_back(c); t.push_back(c); qa.push_back(L[c]); ta.push_back(L[c]); }
    }
}

void crafted(Checker& C, uint64_t seed, int count)
{
    Rng g(seed);
    for (int it = 0; it < count; ++it) {
        std::vector<u8> q, t;
        asmpm::BlockAlignment a;
        const int kind = it % 16;
        // the hangs: unrelated bases in front of and behind the core on both sequences; 0 and above 300 on some
        int hl = uni(g, 20, 299), hr = uni(g, 20, 299);
        if (kind == 3) hl = 0;
        if (kind == 4) hr = 0;
        if (kind == 5) hl = uni(g, 301, 500);
        if (kind == 6) hr = uni(g, 301, 500);
        const bool related = kind >= 8;        // the hang continues the core's relation: DALIGNER runs far into it
        const int ql = hl + (kind == 7 ? 0 : uni(g, 0, 40)), tl = hl + (kind == 7 ? uni(g, 0, 40) : 0);       // min(ql, tl) = hl
        const int qr = hr + (it & 1 ? uni(g, 0, 40) : 0), tr = hr + (it & 1 ? 0 : uni(g, 0, 40));
        std::string junk_q, junk_t;
        if (related) {
            std::vector<u8> a0, b0;
            core(g, std::min(ql, tl), 0.04, 0, 0, a0, b0, junk_q, junk_t);
            random_bases(g, std::max(0, ql - (int)a0.size()), q); random_bases(g, std::max(0, tl - (int)b0.size()), t);
            q.insert(q.end(), a0.begin(), a0.end()); t.insert(t.end(), b0.begin(), b0.end());
        } else { random_bases(g, ql, q); random_bases(g, tl, t); }
        a.qoff = (int)q.size(); a.toff = (int)t.size();
        int len = uni(g, 450, 1500), edge = 12, stride = 0;
        double err = 0.01 * uni(g, 1, 12);
        if (kind == 1) len = uni(g, 100, 380);                     // fewer than 400 columns
        if (kind == 2) { err = 0.6; }                              // below the identity cut
        if (it % 32 == 9) { stride = 5; edge = 0; }                // no run of 8 anywhere
        if (it % 32 == 25) { stride = 7; edge = 0; }
        core(g, len, err, edge, stride, q, t, a.qaln, a.taln);
        if (it % 32 == 10) {       // one run of 8 only, in the middle: the left scan ends behind where the right scan ends (from >= to)
            a.qaln.clear(); a.taln.clear(); q.resize((size_t)a.qoff); t.resize((size_t)a.toff);
            core(g, 240, 0, 0, 4, q, t, a.qaln, a.taln);
            core(g, 9, 0, 0, 0, q, t, a.qaln, a.taln);
            core(g, 240, 0, 0, 4, q, t, a.qaln, a.taln);
        }
        a.qend = (int)q.size(); a.tend = (int)t.size();
        if (related) {
            std::vector<u8> a0, b0;
            core(g, std::min(qr, tr), 0.04, 0, 0, a0, b0, junk_q, junk_t);
            q.insert(q.end(), a0.begin(), a0.end()); t.insert(t.end(), b0.begin(), b0.end());
            random_bases(g, 5, q); random_bases(g, 9, t);
        } else { random_bases(g, qr, q); random_bases(g, tr, t); }
        const int cols = (int)a.qaln.size();
        int mat = 0;
        for (int i = 0; i < cols; ++i) mat += a.qaln[(size_t)i] == a.taln[(size_t)i];
        a.ident_perc = cols ? 100.0 * (double)mat / (double)cols : 0.0;
        C.one(q, t, (it / 3) & 1, cols >= 400, a, (a.qoff + a.qend) / 2, (a.toff + a.tend) / 2);
    }
}

// Ends that the host code tries and declines (found by a hill climb on rescue::Dalign's identity; tests/test_gpu_asm_ends.py has more of them): a prefix of the read and
// of the subject that ends in a run of 8 equal bases, or a suffix that begins with one.  The unrelated parts are of low complexity on nearly disjoint letters: the wave
// meets a sequence end on a path of more differences than half its bases, and daligner.c's identity is below 0.
struct End { int side; const char* q; const char* t; };
const End kDeclined[] = {
    {0, "TTCCTTAAATTTAATTTTTTATTTAGATCGTAAGT", "CGGGACGGGAGAAGGGCGGCGCGCGCGCGGCGCCCTCGTAAGT"},
    {0, "TGGCAACGAAAAAAAAAAAAAAAAAACAAAAGACCGTATCA", "TTCAGCCGGGTCTCTTTTCCCCTCCTGTGGTCCCCGTATCA"},
    {0, "TAAAAAAATAAAAAACCCCCCCAGCCCTCAACAAA", "AACCCGACAATCCCTCATTTCCGGGCGGGGGGGGGGTATTTCAACAAA"},
    {1, "CCAGAGAATTGGTGGGGTGGGTGGGGGAGAGGGTATCC", "CCAGAGAACACCAAACCAACAAACACCCCCTCTC"},
    {1, "TAAACCTCAGCAACAAACCCCACCACACACTT", "TAAACCTCTTTGGTGTGGTGGGGGCGGGGCGGCAGCACCGATAG"},
    {1, "TAGACGCTCCAACAAAAAAAACAACAAAGAATATTCTTAGAGAC", "TAGACGCTAGGTTTGTGTTTTGGTTGGTTGGCCG"},
};

// an alignment of a related core that begins (side 0) or ends (side 1) with the run of 8 of such an end; the other end has no hang
void declined_ends(Checker& C, uint64_t seed)
{
    Rng g(seed);
    auto code = [](char c) { return (u8)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3); };
    for (const End& e : kDeclined) {
        const int lq = (int)strlen(e.q), lt = (int)strlen(e.t);
        std::vector<u8> q, t;
        asmpm::BlockAlignment a;
        if (e.side == 0) {
            for (int i = 0; i < lq; ++i) q.push_back(code(e.q[i]));
            for (int i = 0; i < lt; ++i) t.push_back(code(e.t[i]));
            a.qoff = lq - 8; a.toff = lt - 8;
            a.qaln.assign(e.q + lq - 8, 8); a.taln.assign(e.t + lt - 8, 8);
            core(g, 600, 0.05, 12, 0, q, t, a.qaln, a.taln);
            a.qend = (int)q.size(); a.tend = (int)t.size();
        } else {
            a.qoff = a.toff = 0;
            core(g, 600, 0.05, 12, 0, q, t, a.qaln, a.taln);
            a.qaln.append(e.q, 8); a.taln.append(e.t, 8);
            for (int i = 0; i < lq; ++i) q.push_back(code(e.q[i]));
            for (int i = 0; i < lt; ++i) t.push_back(code(e.t[i]));
            a.qend = (int)q.size() - (lq - 8); a.tend = (int)t.size() - (lt - 8);
        }
        const int cols = (int)a.qaln.size();
        int mat = 0;
        for (int i = 0; i < cols; ++i) mat += a.qaln[(size_t)i] == a.taln[(size_t)i];
        a.ident_perc = 100.0 * (double)mat / (double)cols;
        for (int sdir = 0; sdir < 2; ++sdir) C.one(q, t, sdir, true, a, (a.qoff + a.qend) / 2, (a.toff + a.tend) / 2);
    }
}

// finish_ends on made-up tips: the acceptance tests one by one (of these the wave itself only ever produces an identity below 0).  Returns the number of wrong answers.
int declined_tips()
{
    ExtTask x;
    memset(&x, 0, sizeof x);
    x.qlen = 1000; x.slen = 1200; x.r_qoff = 50; x.r_toff = 60; x.r_qend = 900; x.r_tend = 910; x.r_cols = 860; x.r_mat = 840;
    aends::Plan p;
    memset(&p, 0, sizeof p);
    p.state = aends::kOk | aends::kAlive | ((aends::kTried | aends::kJob) << aends::side_shift(0)) | ((aends::kTried | aends::kJob) << aends::side_shift(1));
    p.from = 9; p.to = 852; p.uneq = 0; p.qls = 58; p.tls = 68; p.qrs = 892; p.trs = 902; p.job[0] = 0; p.job[1] = 1;
    auto tip = [](int a, int y, int d) { dal::Out o; o.a = a; o.y = y; o.d = d; o.flag = 0; o.steps = 0; o.max_diags = 1; return o; };
    // tips (forward, reverse) of the left job and of the right job, and which ends they extend
    struct Row { int fl[3], bl[3], fr[3], br[3], want[2]; };
    const Row rows[] = {
        {{126, 68, 0}, {90, 50, 3}, {40, 20, 2}, {0, 0, 0}, {1, 1}},           // both accepted
        {{124, 67, 0}, {90, 50, 3}, {40, 20, 2}, {2, 1, 0}, {0, 0}},           // the left wave ends short of the anchor; the right one does not start at it
        {{126, 68, 0}, {126, 68, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0}},            // no base of either
        {{126, 68, 0}, {120, 64, 9}, {10, 4, 7}, {0, 0, 0}, {0, 0}},           // more differences than half the bases: identity below 0
    };
    int bad = 0;
    for (const Row& r : rows) {
        const dal::Out outs[4] = {tip(r.fl[0], r.fl[1], r.fl[2]), tip(r.bl[0], r.bl[1], r.bl[2]), tip(r.fr[0], r.fr[1], r.fr[2]), tip(r.br[0], r.br[1], r.br[2])};
        necat_m4 m;
        int ext[2];
        const bool has = aends::finish_ends(x, p, outs, 400, 410, &m, ext);
        bool same = has && ext[0] == r.want[0] && ext[1] == r.want[1];
        if (same && !ext[0] && !ext[1]) same = m.qoff == 50 && m.qend == 900 && m.soff == 60 && m.send == 910 && m.ident_perc == 100.0 * 840 / 860;
        if (same && ext[0] && ext[1]) same = m.qoff == 40 && m.soff == 50 && m.qend == 912 && m.send == 922 && m.ident_perc == 100.0 - 200.0 * (3 + 2 + 20) / (912 + 922 - 40 - 50);
        if (!same) { ++bad; fprintf(stderr, "made-up tips, row %d: wrong\n", (int)(&r - rows)); }
    }
    return bad;
}

#ifdef CHECK_ASM_ENDS_ORACLE
// check_asmpm.cpp's batch walk up to the block alignments
int golden(Checker& C, int argc, char** argv)
{
    ora_options opt;
    ora_options_default(&opt);
    opt.num_candidates = opt.num_output = 100;          // asmpm.c:14 (MAXC)
    if (ora_options_parse(argc - 2, argv, &opt)) return 2;
    const char* wrk = argv[argc - 2];
    const int vid = atoi(argv[argc - 1]);
    ora_volumes_info vi;
    if (ora_volumes_info_load(wrk, &vi)) return 2;
    ora_volume ref;
    if (ora_volume_load(vi.names[vid], &ref)) return 2;
    const int ref_start = vi.read_start_id[vid];
    ora_index* ix = ora_index_build(&ref, opt.kmer_size, opt.kmer_cnt_cutoff);
    std::vector<uint64_t> ref_off(ref.nseq + 1, 0);
    for (uint64_t i = 0; i < ref.nseq; ++i) ref_off[i + 1] = ref_off[i] + ref.size[i];
    asmpm::RefView rv;
    rv.seq_off = ref_off.data(); rv.nseq = ref.nseq;
    rv.kmer_list = [&](uint64_t h, uint64_t* n) -> const uint64_t* {
        const uint64_t u = ix->kmer_stats[h], cnt = u >> 34, start = u & ((1ULL << 34) - 1);
        *n = cnt;
        return cnt ? ix->offset_list + start : nullptr;
    };
    ora_aligner* al = ora_aligner_new(0.5);
    auto subject_of = [&](int sid, int strand, std::vector<uint8_t>& s) { s.resize(ref.size[sid] + 1); ora_volume_extract(&ref, (uint64_t)sid, strand, s.data()); s.resize(ref.size[sid]); };
    asmpm::Voter voter;
    voter.init(ref.nbases);
    asmpm::BatchMapper batch;
    for (int v = vid; v < vi.num_volumes; ++v) {
        ora_volume reads;
        if (ora_volume_load(vi.names[v], &reads)) return 2;
        const int read_start = vi.read_start_id[v];
        std::vector<uint8_t> fwd, rev, subj;
        std::vector<asmpm::VoteCandidate> votes;
        for (uint64_t i = 0; i < reads.nseq; ++i) {
            const int L = (int)reads.size[i], gid = (int)i + read_start;
            fwd.resize((size_t)L + 1); rev.resize((size_t)L + 1);
            ora_volume_extract(&reads, i, 0, fwd.data());
            ora_volume_extract(&reads, i, 1, rev.data());
            int64_t soff_max = INT32_MAX;
            if (gid >= ref_start && gid < ref_start + (int)ref.nseq) soff_max = (int64_t)ref_off[(size_t)(gid - ref_start)];
            votes.clear();
            voter.strand(fwd.data(), L, 0, (int)i, gid, ref_start, rv, opt.kmer_size, opt.scan_window, soff_max, votes);
            voter.strand(rev.data(), L, 1, (int)i, gid, ref_start, rv, opt.kmer_size, opt.scan_window, soff_max, votes);
            std::vector<asmpm::Planned> pl;
            batch.plan(votes, opt.num_candidates, fwd.data(), L, subject_of, pl);
            const std::vector<u8> q(fwd.begin(), fwd.begin() + L);
            for (size_t k = 0; k < pl.size(); ++k) {
                if (pl[k].qoff < 0) continue;
                subject_of(pl[k].sid, pl[k].sdir, subj);
                ora_align_result r;
                asmpm::BlockAlignment a;
                const bool ok = ora_onc_align(al, q.data(), pl[k].qoff, L, subj.data(), pl[k].soff, pl[k].ssize, 2048, 400, 8, &r) != 0;
                a.qoff = r.qoff; a.qend = r.qend; a.toff = r.toff; a.tend = r.tend; a.ident_perc = r.ident_perc;
                a.qaln.assign(r.query_align, (size_t)r.align_size); a.taln.assign(r.target_align, (size_t)r.align_size);
                C.one(q, subj, pl[k].sdir, ok, a, pl[k].qoff, pl[k].soff);
            }
        }
        ora_volume_free(&reads);
    }
    return 0;
}
#endif

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: check_asm_ends golden|crafted CAP1 CAP2 ...\n"); return 2; }
    Checker C;
    C.cap1 = atoi(argv[2]); C.cap2 = atoi(argv[3]);
    if (!strcmp(argv[1], "crafted")) { crafted(C, (uint64_t)atoll(argv[4]), atoi(argv[5])); declined_ends(C, (uint64_t)atoll(argv[4]) + 1); C.n.bad += (uint64_t)declined_tips(); }
    else {
#ifdef CHECK_ASM_ENDS_ORACLE
        const int rc = golden(C, argc - 3, argv + 3);
        if (rc) return rc;
#else
        fprintf(stderr, "built without the oracle\n");
        return 2;
#endif
    }
    return C.report();
}
