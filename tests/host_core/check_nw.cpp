// check_nw.cpp - CPU model of the device form of edlib_go (necat_amd/csrc/nw_core.h): the per-lane cores of the kernels in nw_kernels.h run lane by
// lane, under the same host orchestration of the recursion levels (nw::solve) the library uses, against rescue::EdlibGo::go (rescue.h) - equality
// of ok, coordinates, distance, identity and both gapped strings on every case of the input file.
//
//   check_nw CASES OUT [pool_bytes [first_base]]
// CASES: one line "qdir qf qt tf tt tol min_size error" per case followed by the read and the template as ACGT lines (qdir 1: the query is the reverse
// complement of the read).  OUT: per case "ret qoff qend toff tend dist n ident qa ta" as the model gave them.  All cases go through ONE solve() call.
// first_base (a number, "straddle" or "top": high_base.h): the cases' bases begin there in a buffer that really is that large.
// Exit status 1 when the model and the host code disagree anywhere, or a self-check failed.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../necat_amd/csrc/nw_core.h"
#include "../../necat_amd/csrc/rescue.h"
#include "high_base.h"

using namespace necat;

namespace {

constexpr int kGuard = 4;

struct Model {
    std::vector<u64> words;           // the volume: 2-bit little-endian words with guard words on both sides
    const u64* bases() const { return words.data() + kGuard; }
    std::vector<int> colbuf, bndbuf;
    std::vector<u64> fa, fb_;         // flag records
    std::vector<u8> ops, pack;
    std::vector<nw::LeafOut> leaf_out;
    uint64_t selfcheck = 0;

    // nw_kernels.h wave_pass, the 64 lanes in a loop
    template <bool STORE>
    void pass(const nw::Seq q, const nw::Seq t, int m, int n_stop, const nw::Band bd, int* bnd, u64 flag_off, int W, int* fail, int* col, int* last)
    {
        const int nb = (m + 63) / 64, ns = (nb + nw::kLanes - 1) / nw::kLanes;
        for (int j = 0; j < ns; ++j) {
            nw::Lane L[nw::kLanes];
            for (int l = 0; l < nw::kLanes; ++l) nw::lane_load(L[l], bases(), q, m, j * nw::kLanes + l);
            int c_lo, c_hi;
            nw::stripe_columns(bd, j, n_stop, &c_lo, &c_hi);
            const bool more = j + 1 < ns;
            const int* bin = bnd + (size_t)((j + 1) & 1) * (size_t)n_stop;
            int* bout = bnd + (size_t)(j & 1) * (size_t)n_stop;
            const int steps = c_hi > c_lo ? c_hi - c_lo + nw::kLanes - 1 : 0;
            int pk[nw::kLanes] = {0}, nxt[nw::kLanes];
            for (int s = 0; s < steps; ++s) {
                const int ch = c_lo + s;
                for (int l = 0; l < nw::kLanes; ++l) {
                    const int b = j * nw::kLanes + l;
                    int inp = l ? pk[l - 1] : 0;
                    if (l == 0) {
                        nw::Carry c0; c0.hout = 1; c0.botp = 0;
                        c0.code = ch < n_stop ? (int)(nw::seq_load32(bases(), t, ch & ~31) >> (2 * (ch & 31))) & 3 : 0;
                        if (j > 0 && ch < c_hi) { const nw::Carry p = nw::carry_unpack(bin[ch]); c0.hout = p.hout; c0.botp = p.botp; }
                        inp = nw::carry_pack(c0);
                    }
                    const int c = ch - l;
                    nw::Carry out; out.hout = 0; out.botp = 0; out.code = 0;
                    if (c >= c_lo && c < c_hi) {
                        u64 A = 0, B = 0;
                        const bool act = nw::lane_step<STORE>(L[l], bd, b, c, nw::carry_unpack(inp), &out, &A, &B);
                        if (STORE && act) {
                            const int idx = b - nw::band_fb(bd, c);
                            if (idx >= 0 && idx < W) { fa[flag_off + (size_t)c * W + idx] = A; fb_[flag_off + (size_t)c * W + idx] = B; }
                            else *fail = 1;
                        }
                        if (more && l == nw::kLanes - 1) bout[c] = nw::carry_pack(out);
                    }
                    nxt[l] = nw::carry_pack(out);
                }
                memcpy(pk, nxt, sizeof pk);
            }
            for (int l = 0; l < nw::kLanes; ++l) {
                const int b = j * nw::kLanes + l;
                if (64 * b >= m) continue;
                if (col) nw::lane_column(L[l], bd, b, n_stop - 1, col);
                if (b == ((m - 1) >> 6)) *last = nw::lane_last(L[l], bd, b, n_stop - 1);
            }
        }
    }

    int cols(const std::vector<nw::ColsTask>& ts, u64 col_ints, u64 bnd_ints, std::vector<int>* last)
    {
        colbuf.assign(col_ints + 1, -7); bndbuf.assign(bnd_ints + 1, 0);
        last->assign(ts.size(), 0);
        for (size_t i = 0; i < ts.size(); ++i) {
            const nw::ColsTask& T = ts[i];
            int dummy = 0;
            pass<false>(T.q, T.t, T.m, T.n_stop, T.bd, bndbuf.data() + T.bnd_off, 0, 0, &dummy, T.col_off == ~0ULL ? nullptr : colbuf.data() + T.col_off, &(*last)[i]);
        }
        return 0;
    }
    int split(const std::vector<nw::SplitTask>& ts, std::vector<nw::SplitOut>* out)
    {
        out->resize(ts.size());
        for (size_t i = 0; i < ts.size(); ++i) {
            const nw::SplitTask& T = ts[i];
            const int *Lc = colbuf.data() + T.l_off, *Rc = colbuf.data() + T.r_off;
            int first = -1;
            for (int r = 0; r + 1 < T.m && first < 0; ++r) if (nw::split_hit(Lc, Rc, T.m, T.best, r)) first = r;
            nw::SplitOut o;
            if (first >= 0) { o.row = first; o.ls = Lc[first]; o.rs = Rc[T.m - 2 - first]; }
            else o = nw::split_fallback(Lc, Rc, T.m, T.best, T.lw, T.rw);
            (*out)[i] = o;
        }
        return 0;
    }
    int begin_paths(u64 ops_bytes, size_t n_leaves) { ops.assign(ops_bytes + 1, 9); leaf_out.assign(n_leaves, nw::LeafOut()); return 0; }

    struct Mat {
        const Model* M; u64 off; nw::Band bd; int W;
        bool rec(int c, int b, u64& A, u64& B)
        {
            const int f = nw::band_fb(bd, c);
            if (b < f || b > nw::band_lb(bd, c) || b - f >= W) return false;
            A = M->fa[off + (size_t)c * W + (b - f)]; B = M->fb_[off + (size_t)c * W + (b - f)];
            return true;
        }
    };
    struct Sink { u8* end; void put(int i, int op) { end[-1 - (i64)i] = (u8)op; } };

    int leaves(const nw::LeafTask* ts, size_t n, size_t first, u64 flag_recs, u64 bnd_ints)
    {
        fa.assign(flag_recs + 1, 0); fb_.assign(flag_recs + 1, 0); bndbuf.assign(bnd_ints + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            const nw::LeafTask& T = ts[i];
            nw::LeafOut o; o.cnt = 0; o.fail = 0;
            if (T.m == 0 || T.n == 0) {
                const int len = T.m + T.n;
                for (int k = 0; k < len; ++k) ops[T.ops_end - 1 - (u64)k] = T.m == 0 ? 2 : 1;
                o.cnt = len; o.fail = len != T.best ? 2 : 0;
            } else {
                int fail = 0, last = 0;
                pass<true>(T.q, T.t, T.m, T.n, T.bd, bndbuf.data() + T.bnd_off, T.flag_off, T.W, &fail, nullptr, &last);
                Mat mat{this, T.flag_off, T.bd, T.W};
                Sink sink{ops.data() + T.ops_end};
                int cost = 0;
                o.cnt = nw::walk_leaf(T.m, T.n, mat, sink, &cost);
                o.fail = fail ? 1 : (o.cnt < 0 ? 1 : (cost != T.best ? 2 : 0));
            }
            if (o.fail) ++selfcheck;
            leaf_out[first + i] = o;
        }
        return 0;
    }
    int finish(const std::vector<nw::FinTask>& ts, const std::vector<u64>& leaf_end, u64 pack_bytes, std::vector<nw::FinOut>* out)
    {
        pack.assign(pack_bytes + 1, 0);
        out->assign(ts.size(), nw::FinOut());
        for (size_t x = 0; x < ts.size(); ++x) {
            const nw::FinTask& T = ts[x];
            nw::FinOut o; memset(&o, 0, sizeof o); o.fail = T.bad ? 1 : 0;
            i64 len = 0;
            for (u32 l = T.leaf_begin; l < T.leaf_end && !o.fail; ++l) { if (leaf_out[l].fail || leaf_out[l].cnt < 0) o.fail = 1; len += leaf_out[l].cnt; }
            if (len > (i64)T.m + T.n) o.fail = 1;
            if (!o.fail) {
                u8* P = ops.data() + T.ops_base;
                i64 dst = 0;
                for (u32 l = T.leaf_begin; l < T.leaf_end; ++l) {
                    const int cnt = leaf_out[l].cnt;
                    const u8* src = ops.data() + (leaf_end[l] - (u64)cnt);
                    for (int i = 0; i < cnt; ++i) P[dst + i] = src[i];
                    dst += cnt;
                }
                const int ms = T.match_size;
                i64 e = -1, sb = -1;
                for (i64 p = 0; p < len && e < 0; ++p) if (nw::run_ends_at(P, len, p, ms)) e = p;
                if (e >= 0) for (i64 p = len - ms; p >= 0 && sb < 0; --p) if (nw::run_starts_at(P, len, p, ms)) sb = p;
                if (e >= 0 && sb >= 0) {
                    const i64 from = e + 1 - ms, to = sb + ms;
                    for (i64 i = 0; i < from; ++i) { o.pq += P[i] != 2; o.pt += P[i] != 1; }
                    for (i64 i = to; i < len; ++i) { o.tq += P[i] != 2; o.tt += P[i] != 1; }
                    for (i64 i = from; i < to; ++i) o.same += P[i] == 0;
                    o.ok = 1; o.asz = (int)(to - from);
                    for (i64 i = from; i < to; ++i) pack[T.pack_off + (u64)((i - from) >> 2)] |= (u8)((P[i] & 3) << (2 * ((i - from) & 3)));
                }
            }
            (*out)[x] = o;
        }
        return 0;
    }
};

struct Case { int qdir, qf, qt, tf, tt, tol, min_size; double error; std::string read, tmpl; u64 roff, toff; };

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: check_nw CASES OUT [pool_bytes [first_base]]\n"); return 2; }
    const u64 pool = argc > 3 ? strtoull(argv[3], nullptr, 10) : (64ULL << 20);
    std::ifstream in(argv[1]);
    std::vector<Case> cs;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        Case c; std::istringstream ss(line);
        ss >> c.qdir >> c.qf >> c.qt >> c.tf >> c.tt >> c.tol >> c.min_size >> c.error;
        std::getline(in, c.read); std::getline(in, c.tmpl);
        cs.push_back(c);
    }
    Model M;
    u64 total = 0;
    for (const Case& c : cs) total += c.read.size() + c.tmpl.size();
    const u64 first = high_base::first_base(argc > 4 ? argv[4] : nullptr, total);
    u64 nbases = first;
    for (Case& c : cs) { c.roff = nbases; nbases += c.read.size(); c.toff = nbases; nbases += c.tmpl.size(); }
    M.words.assign((nbases + 31) / 32 + 2 * kGuard, 0);
    {
        u64* W = M.words.data() + kGuard;
        for (const Case& c : cs) {
            for (size_t i = 0; i < c.read.size(); ++i) W[(c.roff + i) >> 5] |= (u64)code_of(c.read[i]) << (2 * ((c.roff + i) & 31));
            for (size_t i = 0; i < c.tmpl.size(); ++i) W[(c.toff + i) >> 5] |= (u64)code_of(c.tmpl[i]) << (2 * ((c.toff + i) & 31));
        }
    }
    // all cases share one error / min_size per solve() call: group them
    std::vector<nw::JobOut> outs(cs.size());
    std::vector<char> done(cs.size(), 0);
    nw::Stats st;
    std::vector<std::vector<u8>> packs(cs.size());
    for (size_t a = 0; a < cs.size(); ++a) {
        if (done[a]) continue;
        std::vector<nw::Job> jobs; std::vector<size_t> who;
        for (size_t b = a; b < cs.size(); ++b) {
            if (done[b] || cs[b].error != cs[a].error || cs[b].min_size != cs[a].min_size) continue;
            const Case& c = cs[b];
            nw::Job J;
            J.m = c.qt - c.qf; J.n = c.tt - c.tf; J.tolerance = c.tol;
            if (c.qdir) J.q = nw::Seq{(i64)(c.roff + c.read.size() - 1 - c.qf), -1, 1};
            else J.q = nw::Seq{(i64)(c.roff + c.qf), 1, 0};
            J.t = nw::Seq{(i64)(c.toff + c.tf), 1, 0};
            jobs.push_back(J); who.push_back(b); done[b] = 1;
        }
        std::vector<nw::JobOut> o;
        const int rc = nw::solve(M, jobs, cs[a].error, cs[a].min_size, 4, pool, &o, &st);
        if (rc) { fprintf(stderr, "solve failed: %d\n", rc); return 2; }
        for (size_t i = 0; i < who.size(); ++i) {
            outs[who[i]] = o[i];
            if (o[i].ok) packs[who[i]].assign(M.pack.begin() + (ptrdiff_t)o[i].pack_off, M.pack.begin() + (ptrdiff_t)(o[i].pack_off + ((u64)o[i].asz + 3) / 4));
        }
    }
    FILE* fo = fopen(argv[2], "w");
    if (!fo) { perror(argv[2]); return 2; }
    int bad = 0; size_t n_ok = 0;
    for (size_t x = 0; x < cs.size(); ++x) {
        const Case& c = cs[x];
        std::vector<char> q(c.read.size()), t(c.tmpl.size());
        for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(c.qdir ? 3 - code_of(c.read[q.size() - 1 - i]) : code_of(c.read[i]));
        for (size_t i = 0; i < t.size(); ++i) t[i] = (char)code_of(c.tmpl[i]);
        rescue::EdlibGo E(c.error);
        const bool hok = E.go(q.data(), c.qf, c.qt, t.data(), c.tf, c.tt, c.tol, c.min_size);
        const nw::JobOut& o = outs[x];
        if (o.fail) { fprintf(stderr, "case %zu: the model flagged the job\n", x); bad = 1; }
        if ((bool)o.ok != hok) { fprintf(stderr, "case %zu: ok %d, host %d\n", x, o.ok, (int)hok); bad = 1; fprintf(fo, "-1\n"); continue; }
        if (!hok) { fprintf(fo, "0\n"); continue; }
        ++n_ok;
        std::string qa((size_t)o.asz, '?'), ta((size_t)o.asz, '?');
        {
            size_t qi = (size_t)(c.qf + o.qoff), ti = (size_t)(c.tf + o.toff);
            for (int i = 0; i < o.asz; ++i) {
                const int op = (packs[x][(size_t)i >> 2] >> (2 * (i & 3))) & 3;
                qa[(size_t)i] = op == 2 ? '-' : "ACGT"[q[qi] & 3]; ta[(size_t)i] = op == 1 ? '-' : "ACGT"[t[ti] & 3];
                qi += op != 2; ti += op != 1;
            }
        }
        const int same = o.asz - o.dist;
        const double ident = 100.0 * same / o.asz;
        const int qoff = c.qf + o.qoff, qend = c.qf + o.qend, toff = c.tf + o.toff, tend = c.tf + o.tend;
        if (qoff != E.qoff || qend != E.qend || toff != E.toff || tend != E.tend || o.dist != E.dist || ident != E.ident_perc || qa != E.query_align || ta != E.target_align) {
            fprintf(stderr, "case %zu: model (%d %d %d %d dist %d n %d) host (%d %d %d %d dist %d n %zu)\n", x, qoff, qend, toff, tend, o.dist, o.asz, E.qoff, E.qend, E.toff,
                    E.tend, E.dist, E.query_align.size());
            bad = 1;
        }
        fprintf(fo, "1 %d %d %d %d %d %d %.17g %s %s\n", qoff, qend, toff, tend, o.dist, o.asz, ident, qa.c_str(), ta.c_str());
    }
    fclose(fo);
    if (M.selfcheck) { fprintf(stderr, "%llu leaves failed their self-check\n", (unsigned long long)M.selfcheck); bad = 1; }
    printf("first_base=%llu last_base=%llu ", (unsigned long long)first, (unsigned long long)(nbases - 1));
    printf("cases=%zu ok=%zu levels=%llu passes=%llu splits=%llu leaves=%llu leaf_chunks=%llu selfcheck=%llu\n", cs.size(), n_ok, (unsigned long long)st.levels,
           (unsigned long long)st.cols_tasks, (unsigned long long)st.splits, (unsigned long long)st.leaves, (unsigned long long)st.leaf_chunks, (unsigned long long)M.selfcheck);
    return bad;
}
