// ctg_seed.h - the seeding of NECAT's contig polishing (ctg_cns/mem_finder.c, ctg_cns/chain_dp.c), host side.
// What extend_ctg_m4s does first with every read-to-contig record (cns_ctg_subseq.c:157-161): MaximalExactMatchWorkData_FindCandidates on the read's strand
// against the contig segment, of which it keeps can_list[0].  Restated, quirks included:
//   * lists (build_kmif_list, mem_finder.c:54-107).  15-mers of the segment at every offset, of the read at offsets 0, 6, 12 ..; the first base is the hash's top
//     digit.  The entry at offset 0 NEVER gets its hash (:87-89 assign `offset` twice): in both lists it carries 0, the hash of fifteen A's.
//   * matches (find_kmer_match, :136-172).  Groups of equal hash; a group pair gives occ_read x occ_segment seeds of 15 bases iff that PRODUCT is at most 20 (:156-157).
//     The offset-0 entries are members of the poly-A groups: they count, and they give seeds whose 15 bases nobody compared.
//   * extension (extend_kmer_match, :214-267).  Seeds in (soff, qoff) order.  A seed still alive is extended to the left from its start and to the right from its
//     start + 15 (:235-244: the 15 bases themselves are never compared) as far as bases agree and neither the read's nor the SEGMENT's end is reached; then every later
//     seed of its diagonal that starts before its right end dies (:249-257); only then is it dropped itself if shorter than 20 (:259).
//     A seed of unverified bases (one of its offsets is 0, it is the first of its diagonal) can so survive as a "match" whose first 15 bases differ, and swallow the
//     true seeds of its diagonal.  It cannot kill a true seed and then die: dropped for being shorter than 20, it ended at a mismatch (or an end) at most 4 bases
//     behind its 15-mer, and every sampled 15-mer of the diagonal that starts before that place (6, 12 or 18 bases on) contains it.
//   * the survivors are sorted by their new (soff, qoff) (:349).  unique_starts() says whether two share a start: the reference's introsort is unstable, so the
//     callers assert it instead of replaying that sort.
//   * chain (scoring_seeds, chain_dp.c:72-130; ChainDpWorkDataNew(1, 200), :22-27: 3000 / 3000 / 1500 / 25).  Predecessor j < i of i needs qoff_j < qoff_i and
//     soff_j < soff_i - starts only, overlapping matches chain (:101) -, both gaps <= 3000, |gap difference| <= 1500.  score = min(gaps, size_i) -
//     (int)(dd * .01 * avg) - (ilog2(dd) >> 1) + f[j] with avg = sum of sizes / n as an int and the product in double (-ffp-contract=off).  The t[] / n_skip rule stops
//     the scan after more than 25 marked non-improving predecessors.  v[i] = the best f on i's chain.
//   * candidate (chaining_find_candidates, :230-351, min_cnt 1).  Chain ends (nobody's predecessor) with v >= 200 give (f[peak], peak), peak = the first j from the end
//     down with f[j] == v[j]; sorted by IntPair_LT (a total order) and reversed.  The first one's walk meets no visited seed, ends at a root and is accepted, so
//     can_list[0] = the chain root .. peak of the largest (f[peak], peak): qend / send from the peak, qbeg / sbeg from the root, score f[peak], qoff / soff the middle
//     of the first strictly longest match in root-to-peak order (:338-342).  full_loop_first() is the loop itself, for the tests.
// Coordinates are relative to the segment.  This header is `path = 1` of necat_ctg_seed_batch, what its device path falls back to, and the model the device
// cores (ctg_seed_core.h) are tested against.  One index per segment, shared by its jobs.  No HIP here.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "host_bases.h"

namespace necat_host {
namespace ctg_seed {

constexpr int kK = 15;                       // extend_ctg_m4s: MaximalExactMatchWorkDataNew(15, 6, 20), cns_ctg_subseq.c
constexpr int kReadWindow = 6;
constexpr int kMinMem = 20;
constexpr int kMaxOcc = 20;                  // kMaxKmOcc (mem_finder.c:328)
constexpr int kMaxDist = 3000, kBand = 1500, kMaxSkip = 25, kMinScore = 200;      // chain_dp.c:22-27, ChainDpWorkDataNew(1, 200)
constexpr int64_t kMaxSegment = 1 << 24;     // a segment must be shorter (the device's tables and sort keys hold 24 bits of a segment offset)
constexpr int64_t kMaxRead = 1 << 30;        // a read must be shorter

struct Mem { int32_t qoff, soff, size; };
inline bool mem_before(const Mem& a, const Mem& b) { return a.soff < b.soff || (a.soff == b.soff && a.qoff < b.qoff); }      // chain_seed_soff_lt (chain_dp.c:5-9)
struct Candidate { int32_t found, qbeg, qend, sbeg, send, qoff, soff, score, chain_len; };
struct JobOut { Candidate can; uint32_t n_matches = 0; std::vector<Mem> mems; };

// bases g .. g + n of a volume's 2-bit words as byte codes; rev: the reverse complement of that stretch (the decoder itself is host_bases.h's)
inline void decode(const uint64_t* words, uint64_t g, int64_t n, int rev, std::vector<uint8_t>& out) { out.resize((size_t)n); BaseWords{words}.stretch(g, n, rev, out.data()); }

// the list of build_kmif_list as hash << 32 | offset, every `window`-th offset; entry 0 keeps hash 0
inline void kmer_list(const uint8_t* s, int64_t n, int window, std::vector<uint64_t>& out)
{
    out.clear();
    if (n < kK) return;
    const uint64_t mask = (1ULL << (2 * kK)) - 1;
    uint64_t h = 0;
    for (int64_t x = 0; x < n; ++x) {
        h = ((h << 2) | s[x]) & mask;
        const int64_t off = x - (kK - 1);
        if (off >= 0 && off % window == 0) out.push_back((off ? h : 0) << 32 | (uint64_t)off);
    }
}

// the segment's sorted list (MaximalExactMatchWorkData_Init, :124-134): built once per segment
struct SegIndex {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> list;          // sorted: by hash, then offset (kmif_hash_lt, :13-17)
    void build(const uint64_t* words, uint64_t g, int size)
    {
        decode(words, g, size, 0, bases);
        kmer_list(bases.data(), size, 1, list);
        std::sort(list.begin(), list.end());
    }
    // the group of `hash`: its first entry and size
    std::pair<size_t, int> group(uint64_t hash) const
    {
        const auto lo = std::lower_bound(list.begin(), list.end(), hash << 32), hi = std::lower_bound(lo, list.end(), (hash + 1) << 32);
        return std::make_pair((size_t)(lo - list.begin()), (int)(hi - lo));
    }
};

// find_kmer_match: the seeds, in any order (extend sorts them; (soff, qoff) is unique among seeds)
inline void matches(const std::vector<uint64_t>& qlist_sorted, const SegIndex& ix, std::vector<Mem>& out)
{
    out.clear();
    for (size_t i = 0; i < qlist_sorted.size();) {
        size_t j = i + 1;
        while (j < qlist_sorted.size() && (qlist_sorted[j] >> 32) == (qlist_sorted[i] >> 32)) ++j;
        const std::pair<size_t, int> g = ix.group(qlist_sorted[i] >> 32);
        if (g.second && (int64_t)(j - i) * g.second <= kMaxOcc)
            for (size_t a = i; a < j; ++a) for (int b = 0; b < g.second; ++b)
                out.push_back(Mem{(int32_t)(uint32_t)qlist_sorted[a], (int32_t)(uint32_t)ix.list[g.first + (size_t)b], kK});
        i = j;
    }
}

// extend_kmer_match, as it stands
inline void extend(std::vector<Mem>& a, const uint8_t* q, int qsize, const uint8_t* t, int tsize)
{
    std::sort(a.begin(), a.end(), mem_before);
    const size_t n = a.size();
    for (size_t i = 0; i < n; ++i) {
        if (a[i].size == 0) continue;
        int ql = a[i].qoff, tl = a[i].soff, qr = ql + a[i].size, tr = tl + a[i].size;
        while (ql && tl && q[ql - 1] == t[tl - 1]) { --ql; --tl; }
        while (qr < qsize && tr < tsize && q[qr] == t[tr]) { ++qr; ++tr; }
        a[i].qoff = ql; a[i].soff = tl; a[i].size = qr - ql;
        for (size_t j = i + 1; j < n && a[j].soff < tr; ++j)
            if (a[j].qoff < qr && a[j].soff < tr && qr - a[j].qoff == tr - a[j].soff) a[j].size = 0;
        if (a[i].size < kMinMem) a[i].size = 0;
    }
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) if (a[i].size) a[k++] = a[i];
    a.resize(k);
    std::sort(a.begin(), a.end(), mem_before);
}

inline bool unique_starts(const std::vector<Mem>& a)
{
    for (size_t i = 1; i < a.size(); ++i) if (a[i].soff == a[i - 1].soff && a[i].qoff == a[i - 1].qoff) return false;
    return true;
}

inline int ilog2_32(uint32_t v) { return v ? 31 - __builtin_clz(v) : -1; }

// one predecessor of scoring_seeds' inner loop (chain_dp.c:101-113): false = `continue`
inline bool pair_score(const Mem& mi, const Mem& mj, int fj, int avg_cov, int* sc_out)
{
    if (mj.qoff >= mi.qoff || mj.soff >= mi.soff) return false;
    const int dr = mi.soff - mj.soff, dq = mi.qoff - mj.qoff;
    if (dq > kMaxDist || dr > kMaxDist) return false;
    const int dd = dr > dq ? dr - dq : dq - dr;
    if (dd > kBand) return false;
    const int min_d = dq < dr ? dq : dr;
    int sc = min_d > mi.size ? mi.size : min_d;
    const int log_dd = dd ? ilog2_32((uint32_t)dd) : 0;
    sc -= (int)(dd * .01 * avg_cov) + (log_dd >> 1);
    *sc_out = sc + fj;
    return true;
}

struct Chain {
    std::vector<int> f, p, t, v;
    // scoring_seeds
    void score(const Mem* m, int n)
    {
        int sum = 0;
        for (int i = 0; i < n; ++i) sum += m[i].size;
        const int avg_cov = sum / n;
        f.assign((size_t)n, 0); p.assign((size_t)n, -1); t.assign((size_t)n, 0); v.assign((size_t)n, 0);
        int st = 0;
        for (int i = 0; i < n; ++i) {
            int max_j = -1, max_f = m[i].size, n_skip = 0;
            while (st < i && m[i].soff > m[st].soff + kMaxDist) ++st;
            for (int j = i - 1; j >= st; --j) {
                int sc;
                if (!pair_score(m[i], m[j], f[(size_t)j], avg_cov, &sc)) continue;
                if (sc > max_f) { max_f = sc; max_j = j; if (n_skip) --n_skip; }
                else if (t[(size_t)j] == i) { if (++n_skip > kMaxSkip) break; }
                if (p[(size_t)j] >= 0) t[(size_t)p[(size_t)j]] = i;
            }
            f[(size_t)i] = max_f; p[(size_t)i] = max_j;
            v[(size_t)i] = (max_j >= 0 && v[(size_t)max_j] > max_f) ? v[(size_t)max_j] : max_f;
        }
    }
    // the chain root .. peak as a candidate
    static Candidate from_peak(const Mem* m, const std::vector<int>& f, const std::vector<int>& p, int peak)
    {
        Candidate c = {1, 0, m[peak].qoff + m[peak].size, 0, m[peak].soff + m[peak].size, 0, 0, f[(size_t)peak], 0};
        int max_size = 0;
        for (int j = peak; j >= 0; j = p[(size_t)j]) {
            ++c.chain_len;
            c.qbeg = m[j].qoff; c.sbeg = m[j].soff;
            if (m[j].size >= max_size) { max_size = m[j].size; c.qoff = m[j].qoff + max_size / 2; c.soff = m[j].soff + max_size / 2; }      // (>= from the peak down = > from the root up)
        }
        return c;
    }
    // can_list[0] by the reduction of the header comment
    Candidate first(const Mem* m, int n)
    {
        Candidate none = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (n == 0) return none;
        score(m, n);
        std::fill(t.begin(), t.end(), 0);
        for (int i = 0; i < n; ++i) if (p[(size_t)i] >= 0) t[(size_t)p[(size_t)i]] = 1;
        int64_t best = -1;
        for (int i = 0; i < n; ++i) {
            if (t[(size_t)i] || v[(size_t)i] < kMinScore) continue;
            int j = i;
            while (j >= 0 && f[(size_t)j] < v[(size_t)j]) j = p[(size_t)j];
            if (j < 0) j = i;
            best = std::max(best, (int64_t)f[(size_t)j] << 32 | (int64_t)j);
        }
        if (best < 0) return none;
        return from_peak(m, f, p, (int)(best & 0xffffffff));
    }
};

// chaining_find_candidates' own loop up to its first candidate (chain_dp.c:254-346), for the tests: must equal Chain::first
inline Candidate full_loop_first(const Mem* m, int n)
{
    Candidate none = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n == 0) return none;
    Chain c;
    c.score(m, n);
    std::vector<int>&f = c.f, &p = c.p, &t = c.t, &v = c.v;
    std::vector<std::pair<int, int>> u;
    std::fill(t.begin(), t.end(), 0);
    for (int i = 0; i < n; ++i) if (p[(size_t)i] >= 0) t[(size_t)p[(size_t)i]] = 1;
    for (int i = 0; i < n; ++i) {
        if (t[(size_t)i] == 0 && v[(size_t)i] >= kMinScore) {
            int j = i;
            while (j >= 0 && f[(size_t)j] < v[(size_t)j]) j = p[(size_t)j];
            if (j < 0) j = i;
            u.push_back(std::make_pair(f[(size_t)j], j));
        }
    }
    if (u.empty()) return none;
    std::sort(u.begin(), u.end());
    std::reverse(u.begin(), u.end());
    std::fill(t.begin(), t.end(), 0);
    const int n_u = (int)u.size(), min_cnt = 1;
    int n_v = 0, k = 0;
    for (int i = 0; i < n_u; ++i) {
        const int n_v0 = n_v, k0 = k;
        int j = u[(size_t)i].second;
        bool find_can = false;
        do { v[(size_t)n_v++] = j; t[(size_t)j] = 1; j = p[(size_t)j]; } while (j >= 0 && t[(size_t)j] == 0);
        if (j < 0) { if (n_v - n_v0 >= min_cnt) { u[(size_t)k].first = u[(size_t)i].first; u[(size_t)k].second = n_v - n_v0; ++k; find_can = true; } }
        else if (u[(size_t)i].first - f[(size_t)j] >= kMinScore) { if (n_v - n_v0 >= min_cnt) { u[(size_t)k].first = u[(size_t)i].first - f[(size_t)j]; u[(size_t)k].second = n_v - n_v0; ++k; find_can = true; } }
        if (find_can) {
            Candidate can = {1, 0, 0, 0, 0, 0, 0, 0, n_v - n_v0};
            can.qend = m[v[(size_t)n_v0]].qoff + m[v[(size_t)n_v0]].size; can.send = m[v[(size_t)n_v0]].soff + m[v[(size_t)n_v0]].size;
            can.qbeg = m[v[(size_t)n_v - 1]].qoff; can.sbeg = m[v[(size_t)n_v - 1]].soff;
            can.score = u[(size_t)k - 1].first;
            int max_size = 0;
            for (int x = n_v; x > n_v0; --x) {
                const int y = v[(size_t)x - 1];
                if (m[y].size > max_size) { max_size = m[y].size; can.qoff = m[y].qoff + max_size / 2; can.soff = m[y].soff + max_size / 2; }
            }
            return can;
        }
        if (k0 == k) n_v = n_v0;
    }
    return none;
}

// one job: the read on its strand (byte codes) against an indexed segment.  false: two surviving matches share a start (no defined order; never seen)
inline bool seed_job(const SegIndex& ix, const uint8_t* read, int qsize, JobOut& out)
{
    std::vector<uint64_t> ql;
    kmer_list(read, qsize, kReadWindow, ql);
    std::sort(ql.begin(), ql.end());
    matches(ql, ix, out.mems);
    out.n_matches = (uint32_t)out.mems.size();
    extend(out.mems, read, qsize, ix.bases.data(), (int)ix.bases.size());
    const bool ok = unique_starts(out.mems);
    Chain c;
    out.can = c.first(out.mems.data(), (int)out.mems.size());
    return ok;
}

}  // namespace ctg_seed
}  // namespace necat_host
