// ctg_seed_core.h - the seeding of contig polishing (ctg_seed.h has the rule) as the DEVICE computes it: the per-lane cores of the kernels in ctg_seed_kernels.h and -
// for g++ - a CPU model of the device path (ctg_seed::model_index / model_job, tests/host_core/check_ctg_seed.cpp) that runs the same cores lane by lane and the
// wave-wide steps as loops over 64 lanes.
//   * both sequences stay 2-bit words of their volumes: a strand is (first base, length, reverse?), a 15-mer or a 32-base window of it comes out of two words at any
//     alignment, the reverse complement from the words themselves (strand_word);
//   * the segment's index is an open-addressing table key -> chain of positions (key = hash + 1, the entry at offset 0 has hash 0); the order inside a chain comes from
//     atomics and nothing reads it: seeds are sorted by (soff, qoff), unique among seeds, before anything looks at them;
//   * a seed is extended on its own, word-wise, whether it will die or not; the reference's sweep (a seed dies iff an earlier seed of its diagonal, alive when its turn
//     came, reached beyond its start) is then a test against the NEAREST earlier seed of the diagonal alone: a seed whose 15 bases were compared lies inside the match
//     of the seed that killed it and reaches exactly as far, and a seed whose 15 bases were not compared (one of the two offsets is 0) is the first of its diagonal
//     and never dies.  The nearest one cannot start more than 15 bases before this seed's own left end (seed_dropped);
//   * the chain is ctg_seed.h's scoring_seeds with the predecessor scan 64 entries at a time (the t[] / n_skip rule as prefix operations, as chain_fill_wave of
//     seed_kernels.h has it); the candidate is the walk from the largest (f[peak], peak).
#pragma once
#include <stdint.h>

#include "dev_common.h"

namespace necat {
namespace ctg_seed {

constexpr int kK = 15, kReadWindow = 6, kMinMem = 20, kMaxOcc = 20;
constexpr int kMaxDist = 3000, kBand = 1500, kMaxSkip = 25, kMinScore = 200;

struct Seq { const u64* bases; i64 g0; i32 len, rev; };        // a strand of bases g0 .. g0 + len of a volume (rev: its reverse complement)
struct SeedRec { i32 s, q, ql, qr; };                          // a seed at segment offset s, read offset q, and the read's [ql, qr) it extends to
struct DMem { i32 qoff, soff, size; };                         // a maximal exact match (necat_ctg_seed_mem)
struct DCan { i32 found, qbeg, qend, sbeg, send, qoff, soff, score, n_mems, chain_len, tier, _pad; };
// a job of a chunk: its read, its table (2 * qcap u32 at qtab_off), and - once counted - its seeds and its share of the pool (seed_off, in seeds)
struct JobDev { i64 read_g0; i32 qlen, qrev; u64 qtab_off; u32 qcap, n_matches; u64 seed_off; };

// 32 elements of a strand from strand position x on in direction d (+1 / -1): element e = strand[x + d e].  Reads up to 31 bases beyond the strand's ends: the
// volumes' guard words
NECAT_HD u64 strand_word(const Seq& s, int x, int d)
{
    return s.rev ? load32_dir(s.bases, s.g0 + s.len - 1 - x, -d, 1) : load32_dir(s.bases, s.g0 + x, d, 0);
}
// the hash of the 15-mer at strand position x (its first base is the top digit) as a table key; the entry at offset 0 never got its hash (mem_finder.c:87-89)
NECAT_HD u32 kmer_key(const Seq& s, int x) { return (x ? (u32)(rev2(strand_word(s, x, +1)) >> (64 - 2 * kK)) : 0u) + 1u; }
NECAT_HD int n_entries(int len, int window) { return len >= kK ? (len - kK) / window + 1 : 0; }
NECAT_HD u32 slot_of(u32 key, u32 cap) { return (u32)(((u64)(key * 0x9E3779B1u) * (u64)cap) >> 32); }

// agreeing elements of two strands from (xa, xb) on in direction d, at most lim
NECAT_HD int match_run(const Seq& a, int xa, const Seq& b, int xb, int d, int lim)
{
    int nrun = 0;
    while (nrun < lim) {
        const u64 x = strand_word(a, xa + d * nrun, d) ^ strand_word(b, xb + d * nrun, d);
        int m = x ? ctz64(x) >> 1 : 32;
        const bool stop = m < 32;
        if (m > lim - nrun) m = lim - nrun;
        nrun += m;
        if (stop) break;
    }
    return nrun;
}
// extend_kmer_match's two runs for the seed (s, q): to the left from the seed's start, to the right from its start + 15, bounded by the four ends
NECAT_HD SeedRec extend_seed(const Seq& seg, const Seq& read, int s, int q)
{
    const int lmax = s < q ? s : q;
    const int l = lmax ? match_run(seg, s - 1, read, q - 1, -1, lmax) : 0;
    const int rs = seg.len - (s + kK), rq = read.len - (q + kK);
    const int rmax = rs < rq ? rs : rq;
    const int r = rmax > 0 ? match_run(seg, s + kK, read, q + kK, +1, rmax) : 0;
    SeedRec o; o.s = s; o.q = q; o.ql = q - l; o.qr = q + kK + r;
    return o;
}
NECAT_HD u64 seed_order(const SeedRec& x) { return (u64)(u32)x.s << 32 | (u64)(u32)x.q; }
NECAT_HD u64 mem_order(const DMem& x) { return (u64)(u32)x.soff << 32 | (u64)(u32)x.qoff; }
NECAT_HD DMem mem_of(const SeedRec& x) { DMem m; m.qoff = x.ql; m.soff = x.s - (x.q - x.ql); m.size = x.qr - x.ql; return m; }

// seed a of the seeds sorted by (s, q): does the sweep of extend_kmer_match drop it before its turn
NECAT_HD bool seed_dropped(const SeedRec* sd, i64 a)
{
    const SeedRec x = sd[a];
    const int sl = x.s - (x.q - x.ql), diag = x.s - x.q;
    for (i64 j = a - 1; j >= 0; --j) {
        const SeedRec o = sd[j];
        if (o.s < sl - kK) break;
        if (o.s - o.q == diag) return o.qr > x.q;
    }
    return false;
}

// one predecessor of scoring_seeds' inner loop (chain_dp.c:101-113): false = `continue`
NECAT_HD bool pair_score(const DMem& mi, const DMem& mj, int fj, int avg_cov, int* sc_out)
{
    if (mj.qoff >= mi.qoff || mj.soff >= mi.soff) return false;
    const int dr = mi.soff - mj.soff, dq = mi.qoff - mj.qoff;
    if (dq > kMaxDist || dr > kMaxDist) return false;
    const int dd = dr > dq ? dr - dq : dq - dr;
    if (dd > kBand) return false;
    const int min_d = dq < dr ? dq : dr;
    int sc = min_d > mi.size ? mi.size : min_d;
    const int log_dd = dd ? 31 - __builtin_clz((unsigned)dd) : 0;
    sc -= (int)((double)dd * .01 * (double)avg_cov) + (log_dd >> 1);
    *sc_out = sc + fj;
    return true;
}

}  // namespace ctg_seed
}  // namespace necat

#if !defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the CPU model of the device path
#include <algorithm>
#include <vector>

namespace necat {
namespace ctg_seed {

struct SegTable { u32 cap = 0; std::vector<u32> keys, head, next; };
struct ModelStats { uint64_t breaks_inside = 0, breaks_at_63 = 0, breaks_later_step = 0, lds_jobs = 0, global_jobs = 0; };
struct ModelOut { u32 n_matches = 0; std::vector<DMem> mems; DCan can; bool unique_starts = true; };      // unique_starts: no two surviving matches share a start (their order would be the reference's unstable sort's)

inline u32 table_cap(u32 n) { u32 cap = 64; while (cap < 2 * n) cap <<= 1; return cap; }

// k_ctgs_index; backwards: the entries in the opposite order, which only changes the order inside the chains
inline void model_index(const Seq& seg, SegTable& T, bool backwards)
{
    const int ne = n_entries(seg.len, 1);
    T.cap = table_cap((u32)ne);
    T.keys.assign(T.cap, 0); T.head.assign(T.cap, 0); T.next.assign((size_t)ne + 1, 0);
    for (int i = 0; i < ne; ++i) {
        const int e = backwards ? ne - 1 - i : i;
        const u32 key = kmer_key(seg, e);
        u32 p = slot_of(key, T.cap);
        while (T.keys[p] && T.keys[p] != key) if (++p == T.cap) p = 0;
        T.keys[p] = key;
        T.next[(size_t)e] = T.head[p]; T.head[p] = (u32)e + 1u;
    }
}
// the segment's entries with this key, counted up to 21: their number, the chain's head in *first
inline int probe(const SegTable& T, u32 key, u32* first)
{
    u32 p = slot_of(key, T.cap);
    for (;;) { const u32 kx = T.keys[p]; if (!kx) return 0; if (kx == key) break; if (++p == T.cap) p = 0; }
    int c = 0;
    for (u32 x = T.head[p]; x && c <= kMaxOcc; x = T.next[x - 1]) ++c;
    *first = T.head[p];
    return c;
}

inline void model_job(const Seq& seg, const SegTable& T, const Seq& read, u32 lds_cap, ModelOut& out, ModelStats& st)
{
    out = ModelOut();
    DCan none = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    out.can = none;
    const int ns = n_entries(read.len, kReadWindow);
    // ---- k_ctgs_count: the read's own occurrences in a table of its own, then the product rule per sample
    const u32 qcap = table_cap((u32)ns);
    std::vector<u32> qtab(2 * (size_t)qcap, 0);
    auto qslot = [&](u32 key) { u32 p = slot_of(key, qcap); while (qtab[2 * p] && qtab[2 * p] != key) if (++p == qcap) p = 0; return p; };
    for (int e = 0; e < ns; ++e) { const u32 key = kmer_key(read, e * kReadWindow); const u32 p = qslot(key); qtab[2 * p] = key; ++qtab[2 * p + 1]; }
    std::vector<SeedRec> tmp, sd;
    for (int e = 0; e < ns; ++e) {
        const u32 key = kmer_key(read, e * kReadWindow);
        u32 first = 0;
        const int tocc = probe(T, key, &first);
        const u32 qocc = qtab[2 * qslot(key) + 1];
        if (tocc == 0 || (uint64_t)qocc * (uint64_t)tocc > (uint64_t)kMaxOcc) continue;
        // ---- k_ctgs_mems: every seed extended where it is emitted
        for (u32 x = first; x; x = T.next[x - 1]) tmp.push_back(extend_seed(seg, read, (int)x - 1, e * kReadWindow));
    }
    out.n_matches = (u32)tmp.size();
    const size_t n = tmp.size();
    sd.resize(n);
    for (size_t a = 0; a < n; ++a) { size_t rk = 0; for (size_t b = 0; b < n; ++b) rk += seed_order(tmp[b]) < seed_order(tmp[a]); sd[rk] = tmp[a]; }
    std::vector<DMem> tm;
    for (size_t a = 0; a < n; ++a) if (!seed_dropped(sd.data(), (i64)a) && sd[a].qr - sd[a].ql >= kMinMem) tm.push_back(mem_of(sd[a]));
    const int nm = (int)tm.size();
    out.mems.resize((size_t)nm);
    for (int a = 0; a < nm; ++a) {
        int rk = 0;
        for (int b = 0; b < nm; ++b) rk += mem_order(tm[(size_t)b]) < mem_order(tm[(size_t)a]) || (mem_order(tm[(size_t)b]) == mem_order(tm[(size_t)a]) && b < a);
        out.mems[(size_t)rk] = tm[(size_t)a];
    }
    for (int a = 1; a < nm; ++a) if (mem_order(out.mems[(size_t)a]) == mem_order(out.mems[(size_t)a - 1])) out.unique_starts = false;
    out.can.n_mems = nm;
    if (nm == 0) return;
    // ---- k_ctgs_chain: the arrays in LDS up to lds_cap matches, in the job's scratch above (the same steps either way)
    out.can.tier = (u32)nm <= lds_cap ? 0 : 1;
    ++((u32)nm <= lds_cap ? st.lds_jobs : st.global_jobs);
    const DMem* m = out.mems.data();
    std::vector<int> f((size_t)nm, 0), p((size_t)nm, -1), t((size_t)nm, 0), v((size_t)nm, 0);
    int sum = 0;
    for (int a = 0; a < nm; ++a) sum += m[a].size;
    const int avg_cov = sum / nm;
    int stt = 0;
    for (int i = 0; i < nm; ++i) {
        while (stt < i && m[i].soff > m[stt].soff + kMaxDist) ++stt;
        int max_f = m[i].size, max_j = -1, n_skip = 0, step = 0;
        for (int top = i - 1; top >= stt; top -= 64, ++step) {
            int sc[64]; bool valid[64], marked[64];
            for (int l = 0; l < 64; ++l) {
                const int j = top - l;
                sc[l] = INT32_MIN; valid[l] = false;
                if (j >= stt) {
                    valid[l] = pair_score(m[i], m[j], f[(size_t)j], avg_cov, &sc[l]);
                    if (valid[l]) { if (p[(size_t)j] >= 0) t[(size_t)p[(size_t)j]] = i; } else sc[l] = INT32_MIN;
                }
            }
            for (int l = 0; l < 64; ++l) marked[l] = valid[l] && t[(size_t)(top - l)] == i;
            // prefix maximum of the lanes before, new bests, the floored walk of n_skip
            int run = max_f, S = 0, floor_ = -n_skip, stop = -1, last_best = -1, W_last = n_skip;
            bool any_skip = false;
            u64 NM = 0;
            for (int l = 0; l < 64; ++l) {
                const bool newmax = valid[l] && sc[l] > run;
                if (newmax) { run = sc[l]; NM |= 1ULL << l; }
                const bool skip = marked[l] && !newmax;
                any_skip |= skip;
                S += (skip ? 1 : 0) - (newmax ? 1 : 0);
                if (S < floor_) floor_ = S;
                const int W = S - floor_;
                if (stop < 0 && W > kMaxSkip) stop = l;
                W_last = W;
            }
            u64 live = ~0ULL;
            if (any_skip) { if (stop >= 0) live = (1ULL << stop) - 1ULL; else n_skip = W_last; }
            else { n_skip -= popc64(NM); if (n_skip < 0) n_skip = 0; }
            const u64 best = NM & live;
            if (best) { last_best = 63 - __builtin_clzll(best); max_f = sc[last_best]; max_j = top - last_best; }
            if (live != ~0ULL) { ++(step ? st.breaks_later_step : stop == 63 ? st.breaks_at_63 : st.breaks_inside); break; }
        }
        f[(size_t)i] = max_f; p[(size_t)i] = max_j;
        v[(size_t)i] = (max_j >= 0 && v[(size_t)max_j] > max_f) ? v[(size_t)max_j] : max_f;
    }
    std::fill(t.begin(), t.end(), 0);
    for (int a = 0; a < nm; ++a) if (p[(size_t)a] >= 0) t[(size_t)p[(size_t)a]] = 1;
    i64 bestk = -1;
    for (int a = 0; a < nm; ++a) {
        if (t[(size_t)a] || v[(size_t)a] < kMinScore) continue;
        int j = a;
        while (j >= 0 && f[(size_t)j] < v[(size_t)j]) j = p[(size_t)j];
        if (j < 0) j = a;
        const i64 key = ((i64)f[(size_t)j] << 32) | (i64)(u32)j;
        if (key > bestk) bestk = key;
    }
    if (bestk < 0) return;
    const int peak = (int)(u32)(bestk & 0xffffffffLL);
    DCan& c = out.can;
    c.found = 1; c.score = (int)(bestk >> 32); c.qend = m[peak].qoff + m[peak].size; c.send = m[peak].soff + m[peak].size;
    int max_size = 0;
    for (int j = peak; j >= 0; j = p[(size_t)j]) {
        ++c.chain_len; c.qbeg = m[j].qoff; c.sbeg = m[j].soff;
        if (m[j].size >= max_size) { max_size = m[j].size; c.qoff = m[j].qoff + max_size / 2; c.soff = m[j].soff + max_size / 2; }
    }
}

}  // namespace ctg_seed
}  // namespace necat
#endif
