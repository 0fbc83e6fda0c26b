// nw_core.h - the global alignment with its path of the rescue pair (rescue::EdlibGo::go, rescue.h; edlib_go, edlib/edlib_wrapper.c:111) for the
// device: per-lane cores of the kernels of nw_kernels.h and the host orchestration of the recursion levels (nw::solve), written so that g++ builds the
// same functions for a CPU model that runs them lane by lane (tests/host_core/check_nw.cpp).
//
// One WAVE owns one (sub)problem.  A lane owns one 64-row word of Myers' bit-vector column; the lanes are skewed one column per lane, so the
// horizontal delta a word needs from the word above it in the same column is what the lane above computed one step earlier (Carry).  Problems of more
// than 64 words go stripe after stripe, 64 words at a time; the last word of a stripe leaves its carries in a boundary array for the first word of the
// next.  The band is the host's, word for word and column for column (rescue::detail::BitColumns::run: words [fb(c), lb(c)] of column c, a word that
// enters starts at "one more per row than the word above", the row above the band counts as one more per column), so every number is the host's and
// the path rules - the leaf rule, the split rule, the walk's up > left > diagonal - read the same values (DESIGN 6b has the argument why any band
// that contains Ukkonen's would do).
#pragma once
#include <limits.h>

#include "dev_common.h"

namespace necat {
namespace nw {

constexpr int kFar = INT32_MAX / 4;            // "outside the band" (rescue::detail::kFar)
constexpr int kLanes = 64;
constexpr int kStripeRows = kLanes * 64;
constexpr int kMaxLen = 1 << 26;               // m, n below this: a packed carry holds a word's bottom value in 28 bits

// a sequence as the kernels read it: element i = base (g0 + dir * i) of a volume, complemented when comp
struct Seq { i64 g0; int dir, comp; };
NECAT_HD Seq seq_from(Seq s, int from) { s.g0 += (i64)s.dir * from; return s; }
NECAT_HD Seq seq_reversed(Seq s, int len) { s.g0 += (i64)s.dir * (len - 1); s.dir = -s.dir; return s; }
// elements c .. c + 31 as one 2-bit packed word
NECAT_HD u64 seq_load32(const u64* bases, Seq s, int c) { return load32_dir(bases, s.g0 + (i64)s.dir * c, s.dir, s.comp); }

// BitColumns::set_band: the diagonals r - c in [dmin, dmax] of a problem of m rows and n_total columns whose optimum is at most k
struct Band { int m, dmin, dmax; };
NECAT_HD Band make_band(int m, int n_total, int k)
{
    const int delta = m - n_total;
    Band b; b.m = m; b.dmin = -((k - delta) / 2); b.dmax = (delta + k) / 2;
    return b;
}
NECAT_HD int band_fb(const Band& bd, int c) { const int x = c + bd.dmin; return (x > 0 ? x : 0) >> 6; }
NECAT_HD int band_lb(const Band& bd, int c) { const int x = c + bd.dmax, y = bd.m - 1; return (x < y ? x : y) >> 6; }
// words a column of the band holds at most: what a leaf's flag store reserves per column
NECAT_HD int band_width(const Band& bd)
{
    const int nb = (bd.m + 63) / 64;
    const int d = bd.dmax - bd.dmin;
    const int w = (d > 0 ? d : 0) / 64 + 2;
    return w < nb ? w : nb;
}
// the columns in which a word of stripe j (words [64 j, 64 j + 63]) can be inside the band, and one more: the carries of the column in which the
// next stripe's first word enters are always written
NECAT_HD void stripe_columns(const Band& bd, int j, int n_stop, int* c_lo, int* c_hi)
{
    const i64 r0 = (i64)j * kStripeRows;
    i64 lo = r0 - bd.dmax, hi = r0 + kStripeRows - bd.dmin + 1;
    if (lo < 0) lo = 0;
    if (hi > n_stop) hi = n_stop;
    if (hi < lo) hi = lo;
    *c_lo = (int)lo; *c_hi = (int)hi;
}

// one 64-row word of the column: vertical deltas, the query's complemented bit-planes (rows past m: never equal), the value at its last row
struct Lane { u64 P, M, nlo, nhi, valid; int bot, botp, in; };
// what a word hands to the word below it after a column: its horizontal delta at the last row, its bottom value BEFORE the column, the column's base
struct Carry { int hout, botp, code; };
NECAT_HD int carry_pack(const Carry& c) { return (c.botp << 4) | (c.code << 2) | (c.hout + 1); }
NECAT_HD Carry carry_unpack(int v) { Carry c; c.hout = (v & 3) - 1; c.code = (v >> 2) & 3; c.botp = v >> 4; return c; }

NECAT_HD void lane_load(Lane& L, const u64* bases, Seq q, int m, int b)
{
    L.P = ~0ULL; L.M = 0; L.bot = L.botp = 0; L.in = 0;
    const int rows = m - 64 * b;
    if (rows <= 0) { L.nlo = L.nhi = L.valid = 0; return; }
    u64 lo, hi;
    load64_planes(bases, q.g0, q.dir, q.comp, 64 * b, &lo, &hi);
    L.nlo = ~lo; L.nhi = ~hi;
    L.valid = rows >= 64 ? ~0ULL : ((1ULL << rows) - 1);
}

// Column c of word b (BitColumns::run's inner loop for one b).  `in`: the carry of word b - 1 for this column.  STORE: the walk's decision at each of
// the 64 cells, two bits per cell as in dp_core.h (A, B) = (1, 0) up, (0, 1) left, (0, 0) diagonal on equal bases, (1, 1) diagonal on different ones -
// up <=> the vertical +1 flag after the column, left <=> the horizontal +1 flag (NwPath::leaf reads sv, then sh, then compares the bases).
// Returns whether the word was inside the band (then A, B are set).
template <bool STORE>
NECAT_HD bool lane_step(Lane& L, const Band& bd, int b, int c, Carry in, Carry* out, u64* A, u64* B)
{
    const int fb = band_fb(bd, c), lb = band_lb(bd, c);
    if (!L.in && b <= lb && L.valid) { L.P = ~0ULL; L.M = 0; L.bot = (b ? in.botp : c) + 64; L.in = 1; }
    out->code = in.code; out->botp = L.bot; out->hout = 0;
    L.botp = L.bot;
    if (!L.in || b < fb) return false;
    const int hin = b == fb ? 1 : in.hout;
    const u64 ma = (in.code & 1) ? ~0ULL : 0ULL, mb = (in.code & 2) ? ~0ULL : 0ULL;
    const u64 eq = (L.nlo ^ ma) & (L.nhi ^ mb) & L.valid;
    const u64 pv = L.P, mv = L.M;
    const u64 hneg = hin < 0 ? 1ULL : 0ULL;
    const u64 xv = eq | mv;
    const u64 x = eq | hneg;
    const u64 xh = (((x & pv) + pv) ^ pv) | x;
    u64 ph = mv | ~(xh | pv), mh = pv & xh;
    const int hout = (int)(ph >> 63) - (int)(mh >> 63);
    const u64 sh = ph;
    ph = (ph << 1) | (hin > 0 ? 1ULL : 0ULL); mh = (mh << 1) | hneg;
    L.P = mh | ~(xv | ph); L.M = ph & xv;
    L.bot += hout;
    out->hout = hout;
    if (STORE) { *A = L.P | (~sh & ~eq); *B = ~L.P & (sh | ~eq); }
    return true;
}

// BitColumns::column for word b after the last column c_last: D(r, c_last) of its rows below m, kFar outside the band
NECAT_HD void lane_column(const Lane& L, const Band& bd, int b, int c_last, int* col)
{
    const bool inside = L.in && b >= band_fb(bd, c_last) && b <= band_lb(bd, c_last);
    int s = L.bot;
    for (int r = 63; r >= 0; --r) {
        if (64 * b + r < bd.m) col[64 * b + r] = inside ? s : kFar;
        s -= (int)((L.P >> r) & 1) - (int)((L.M >> r) & 1);
    }
}
// .. and of the one row m - 1 (the problem's distance when c_last is its last column)
NECAT_HD int lane_last(const Lane& L, const Band& bd, int b, int c_last)
{
    if (!(L.in && b >= band_fb(bd, c_last) && b <= band_lb(bd, c_last))) return kFar;
    int s = L.bot;
    for (int r = 63; r > ((bd.m - 1) & 63); --r) s -= (int)((L.P >> r) & 1) - (int)((L.M >> r) & 1);
    return s;
}

// NwPath::solve's split row among rows [0, m - 1): does the prefix cost to row i plus the suffix cost from row i + 1 give the optimum
NECAT_HD bool split_hit(const int* Lc, const int* Rc, int m, int best, int i) { return i + 1 < m && Lc[i] + Rc[m - 2 - i] == best; }
struct SplitOut { int row, ls, rs; };      // row -2: no row gives the optimum (the host returns "no path")
// the two fallbacks, in the host's order: everything of the left half against nothing ("row -1"), then the last row
NECAT_HD SplitOut split_fallback(const int* Lc, const int* Rc, int m, int best, int lw, int rw)
{
    SplitOut o; o.row = -2; o.ls = o.rs = 0;
    if (lw + Rc[m - 1] == best) { o.row = -1; o.ls = lw; o.rs = Rc[m - 1]; }
    else if (Lc[m - 1] + rw == best) { o.row = m - 1; o.ls = Lc[m - 1]; o.rs = rw; }
    return o;
}

// NwPath::leaf's walk from the last cell.  Mat::rec(c, b, A, B): the flags of word b of column c, false = not stored (outside the band: a walk that
// stays on optimal paths never asks).  Sink::put(i, op): op number i counted from the END of the path.  Returns the number of ops, -1 when a flag
// was missing; *cost = the ops that are no match.
template <class Mat, class Sink>
NECAT_HD int walk_leaf(int m, int n, Mat& mat, Sink& sink, int* cost)
{
    int r = m - 1, c = n - 1, cnt = 0, nm = 0;
    while (r >= 0 && c >= 0) {
        u64 A, B;
        if (!mat.rec(c, r >> 6, A, B)) return -1;
        const int a = (int)((A >> (r & 63)) & 1), b = (int)((B >> (r & 63)) & 1);
        const int op = a | (b << 1);
        sink.put(cnt++, op);
        nm += op != 0;
        r -= op != 2; c -= op != 1;
    }
    for (; r >= 0; --r) { sink.put(cnt++, 1); ++nm; }
    for (; c >= 0; --c) { sink.put(cnt++, 2); ++nm; }
    *cost = nm;
    return cnt;
}

// the end trimming of edlib_go (edlib_wrapper.c:177-229) on the ops of the whole path, one byte each: does a run of ms matches end at / start at p
NECAT_HD bool run_ends_at(const u8* ops, i64 len, i64 p, int ms)
{
    if (p >= len || p + 1 < ms) return false;
    for (int i = 0; i < ms; ++i) if (ops[p - i]) return false;
    return true;
}
NECAT_HD bool run_starts_at(const u8* ops, i64 len, i64 p, int ms)
{
    if (p < 0 || p + ms > len) return false;
    for (int i = 0; i < ms; ++i) if (ops[p + i]) return false;
    return true;
}

// ---- what the kernels are handed, one record per wave
struct ColsTask {          // k_nw_cols: columns [0, n_stop) of q[0, m) against t, score only
    Seq q, t;
    int m, n_stop;
    Band bd;
    u64 col_off;           // ints: where the last column's m values go (~0: only the last row's)
    u64 bnd_off;           // ints: 2 * n_stop of boundary carries (problems of more than one stripe)
};
struct SplitTask { u64 l_off, r_off; int m, best, lw, rw; };
struct LeafTask {          // k_nw_leaf: the same pass over all n columns storing the flags, then the walk
    Seq q, t;
    int m, n, best, W;
    Band bd;
    u64 flag_off;          // 16-byte records: n * W of them, record (c, b) at c * W + b - fb(c)
    u64 bnd_off;
    u64 ops_end;           // bytes: the leaf's ops end here (they are written backwards from the end of the path)
};
struct LeafOut { int cnt, fail; };        // fail: 1 a flag outside the band was asked for, 2 the path does not cost `best`
struct FinTask { u64 ops_base, pack_off; u32 leaf_begin, leaf_end; int m, n, match_size, bad; };
struct FinOut { int ok, pq, pt, tq, tt, asz, same, fail; };

}  // namespace nw
}  // namespace necat

// ------------------------------------------------------------------------------------------------------------------------------------
// Host side: the levels of NwPath::solve over many jobs at once.  Backend: the four launches, on the device (stage_nw.inl) or lane by lane
// on the CPU (check_nw.cpp).  Between levels the host sees one int per score pass (the distance) and three per split (row, ls, rs).
#include <algorithm>
#include <vector>

namespace necat {
namespace nw {

struct Job { Seq q, t; int m, n, tolerance; };         // q, t: the two ranges, already as the kernels address them
struct JobOut { int ok, qoff, qend, toff, tend, asz, dist, fail; u64 pack_off; };      // offsets relative to the ranges; fail: recompute on the host

struct Stats { uint64_t levels = 0, cols_tasks = 0, splits = 0, leaves = 0, leaf_chunks = 0; };

// is (m, n) a leaf of NwPath::solve
inline bool is_leaf(int m, int n) { return 20LL * ((m + 63) / 64) * n + 8LL * n < 1024 * 1024; }

// Backend:
//   int cols(const std::vector<ColsTask>&, u64 col_ints, u64 bnd_ints, std::vector<int>* last)     last[i] = the last row's value of task i
//   int split(const std::vector<SplitTask>&, std::vector<SplitOut>*)                                 reads the columns the preceding cols() left
//   int begin_paths(u64 ops_bytes, size_t n_leaves)
//   int leaves(const LeafTask* t, size_t n, size_t first, u64 flag_recs, u64 bnd_ints)              leaf i's LeafOut stays with the backend at first + i
//   int finish(const std::vector<FinTask>&, const std::vector<u64>& leaf_end, u64 pack_bytes, std::vector<FinOut>*)
// every call returns 0 or an error code that solve() passes on.
template <class Backend>
int solve(Backend& be, const std::vector<Job>& jobs, double error, int min_align_size, int match_size, u64 pool_bytes, std::vector<JobOut>* out, Stats* st)
{
    const size_t nj = jobs.size();
    out->assign(nj, JobOut());
    std::vector<int> best(nj, 0);
    std::vector<uint32_t> alive;
    {   // the score pass of edlib_go and its reject rules
        std::vector<ColsTask> ct; std::vector<uint32_t> who;
        u64 bnd = 0;
        for (size_t j = 0; j < nj; ++j) {
            const Job& J = jobs[j];
            if (J.m <= 0 || J.n <= 0 || J.tolerance < 0) continue;
            if (J.tolerance < (J.m > J.n ? J.m - J.n : J.n - J.m)) continue;
            ColsTask t; t.q = J.q; t.t = J.t; t.m = J.m; t.n_stop = J.n;
            t.bd = make_band(J.m, J.n, std::min(J.tolerance, std::max(J.m, J.n)));
            t.col_off = ~0ULL; t.bnd_off = bnd;
            if (J.m > kStripeRows) bnd += 2 * (u64)J.n;
            ct.push_back(t); who.push_back((uint32_t)j);
        }
        std::vector<int> last;
        if (!ct.empty()) { const int rc = be.cols(ct, 0, bnd, &last); if (rc) return rc; }
        st->cols_tasks += ct.size();
        for (size_t i = 0; i < ct.size(); ++i) {
            const Job& J = jobs[who[i]];
            const int b = last[i];
            if (b > J.tolerance) continue;
            const int align_len = J.n - 1;
            if (align_len < min_align_size) continue;
            if ((double)b / (double)align_len > error) continue;
            best[who[i]] = b; alive.push_back(who[i]);
        }
    }
    if (alive.empty()) return 0;

    struct Node { uint32_t job; int q0, m, t0, n, best; };
    std::vector<Node> level, next, leaf_nodes;
    std::vector<char> bad(nj, 0);
    for (uint32_t j : alive) level.push_back(Node{j, 0, jobs[j].m, 0, jobs[j].n, best[j]});
    while (!level.empty()) {
        ++st->levels;
        std::vector<ColsTask> ct; std::vector<SplitTask> sp; std::vector<Node> sn;
        u64 cols = 0, bnd = 0;
        for (const Node& N : level) {
            if (bad[N.job]) continue;
            if (N.m == 0 || N.n == 0 || is_leaf(N.m, N.n)) { leaf_nodes.push_back(N); continue; }
            const Job& J = jobs[N.job];
            const int lw = N.n / 2, rw = N.n - lw;
            const Seq q = seq_from(J.q, N.q0), t = seq_from(J.t, N.t0);
            ColsTask a; a.q = q; a.t = t; a.m = N.m; a.n_stop = lw; a.bd = make_band(N.m, N.n, N.best);
            a.col_off = cols; cols += (u64)N.m; a.bnd_off = bnd; if (N.m > kStripeRows) bnd += 2 * (u64)lw;
            ColsTask b; b.q = seq_reversed(q, N.m); b.t = seq_reversed(seq_from(t, lw), rw); b.m = N.m; b.n_stop = rw; b.bd = a.bd;
            b.col_off = cols; cols += (u64)N.m; b.bnd_off = bnd; if (N.m > kStripeRows) bnd += 2 * (u64)rw;
            ct.push_back(a); ct.push_back(b);
            sp.push_back(SplitTask{a.col_off, b.col_off, N.m, N.best, lw, rw});
            sn.push_back(N);
        }
        next.clear();
        if (!sp.empty()) {
            std::vector<int> last; std::vector<SplitOut> so;
            int rc = be.cols(ct, cols, bnd, &last); if (rc) return rc;
            rc = be.split(sp, &so); if (rc) return rc;
            st->cols_tasks += ct.size(); st->splits += sp.size();
            for (size_t i = 0; i < sp.size(); ++i) {
                const Node& N = sn[i];
                const SplitOut& o = so[i];
                const int lw = sp[i].lw, rw = sp[i].rw;
                // a split the two halves cannot have (no row, or costs outside what lengths allow): the job is recomputed on the host
                if (o.row < -1 || o.row >= N.m || o.ls < 0 || o.rs < 0 || o.ls > N.m + lw || o.rs > N.m + rw) { bad[N.job] = 1; continue; }
                const int uh = o.row + 1;
                next.push_back(Node{N.job, N.q0, uh, N.t0, lw, o.ls});
                next.push_back(Node{N.job, N.q0 + uh, N.m - uh, N.t0 + lw, rw, o.rs});
            }
        }
        level.swap(next);
    }

    // the leaves, in path order inside every job; a job's ops live in m + n bytes, leaf (q0, t0) ending at q0 + t0 + m + n of them
    std::sort(leaf_nodes.begin(), leaf_nodes.end(), [](const Node& a, const Node& b) { return a.job != b.job ? a.job < b.job : a.q0 + a.t0 < b.q0 + b.t0; });
    std::vector<u64> ops_base(nj, 0), pack_off(nj, 0);
    u64 ops_bytes = 0, pack_bytes = 0;
    for (uint32_t j : alive) {
        ops_base[j] = ops_bytes; ops_bytes += ((u64)jobs[j].m + jobs[j].n + 7) & ~7ULL;
        pack_off[j] = pack_bytes; pack_bytes += (((u64)jobs[j].m + jobs[j].n + 3) / 4 + 7) & ~7ULL;
    }
    std::vector<LeafTask> lt(leaf_nodes.size());
    std::vector<u64> leaf_end(leaf_nodes.size());
    for (size_t i = 0; i < leaf_nodes.size(); ++i) {
        const Node& N = leaf_nodes[i];
        const Job& J = jobs[N.job];
        LeafTask& t = lt[i];
        t.q = seq_from(J.q, N.q0); t.t = seq_from(J.t, N.t0); t.m = N.m; t.n = N.n; t.best = N.best;
        t.bd = make_band(N.m, N.n, N.best); t.W = N.m && N.n ? band_width(t.bd) : 0;
        t.flag_off = 0; t.bnd_off = 0;
        t.ops_end = ops_base[N.job] + (u64)N.q0 + N.t0 + N.m + N.n;
        leaf_end[i] = t.ops_end;
    }
    st->leaves += lt.size();
    int rc = be.begin_paths(ops_bytes, lt.size()); if (rc) return rc;
    const u64 pool_recs = std::max<u64>(pool_bytes / 16, 1);
    for (size_t i = 0; i < lt.size();) {        // chunks of leaves whose flags fit the pool (one leaf always does: it is below 2^20 / 20 records)
        size_t e = i; u64 recs = 0, bnd = 0;
        while (e < lt.size()) {
            const u64 need = (u64)lt[e].n * (u64)lt[e].W;
            if (e > i && recs + need > pool_recs) break;
            lt[e].flag_off = recs; recs += need;
            lt[e].bnd_off = bnd; if (lt[e].m > kStripeRows) bnd += 2 * (u64)lt[e].n;
            ++e;
        }
        rc = be.leaves(lt.data() + i, e - i, i, recs, bnd); if (rc) return rc;
        ++st->leaf_chunks;
        i = e;
    }
    std::vector<FinTask> ft; std::vector<uint32_t> who;
    for (size_t i = 0; i < leaf_nodes.size();) {
        size_t e = i;
        while (e < leaf_nodes.size() && leaf_nodes[e].job == leaf_nodes[i].job) ++e;
        const uint32_t j = leaf_nodes[i].job;
        ft.push_back(FinTask{ops_base[j], pack_off[j], (u32)i, (u32)e, jobs[j].m, jobs[j].n, match_size, (int)bad[j]});
        who.push_back(j);
        i = e;
    }
    std::vector<FinOut> fo;
    rc = be.finish(ft, leaf_end, pack_bytes, &fo); if (rc) return rc;
    for (size_t i = 0; i < ft.size(); ++i) {
        const uint32_t j = who[i];
        const Job& J = jobs[j];
        const FinOut& f = fo[i];
        JobOut& o = (*out)[j];
        o.pack_off = pack_off[j];
        if (f.fail || bad[j]) { o.fail = 1; continue; }
        if (!f.ok) continue;
        o.ok = 1; o.qoff = f.pq; o.qend = J.m - f.tq; o.toff = f.pt; o.tend = J.n - f.tt; o.asz = f.asz; o.dist = f.asz - f.same;
    }
    for (uint32_t j : alive) if (bad[j]) (*out)[j].fail = 1;      // (a job whose every node was dropped before it reached a leaf)
    return 0;
}

}  // namespace nw
}  // namespace necat
