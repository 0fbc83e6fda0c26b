// check_dalign.cpp - CPU model of the device form of ocda_go (necat_amd/csrc/dal_core.h): the per-lane core of k_dal_wave (dal_kernels.h) run lane by lane,
// the two directions of a job as separate jobs, against rescue::Dalign::go (rescue.h) - equality of ok, the four coordinates, diffs and ident_perc on
// every case of the input file.
//
//   check_dalign CASES OUT [capacity [first_base]]
// CASES: one line "qdir qstart sstart min_size error" per case followed by the read and the template as ACGT lines (qdir 1: the query is the reverse
// complement of the read; qstart is on that strand).  OUT: per case "ok abpos aepos bbpos bepos diffs ident how" as the model gave them (how 1: the window
// outgrew the capacity, or the job was flagged, and the host code decided).  The model carries every point's `org` and counts the records whose org is not
// the anchor's diagonal.  Last line of stdout: cases= stale= empty= over_cap= max_diags= steps= org_bad=.
// first_base (a number, "straddle" or "top": high_base.h, per case over its read and template): both sequences of a case lie in ONE buffer that really is that
// large, the read from first_base and the template behind it, and the job carries those positions.
// Exit status 1 when the model and the host code disagree anywhere, or a record's org was not the anchor's diagonal.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define NECAT_DAL_TRACK_ORG 1
#include "../../necat_amd/csrc/dal_core.h"
#include "../../necat_amd/csrc/rescue.h"
#include "../../necat_amd/csrc/rescue_pair.h"
#include "high_base.h"

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
    // the high form: one buffer for all cases, a case's codes written at `at` and taken out again
    void reserve_bases(u64 n) { words.assign((size_t)((n + 31) / 32) + 2 * kGuard, 0); }
    void put(u64 at, const std::vector<u8>& codes) { for (u64 i = 0; i < codes.size(); ++i) words[kGuard + (size_t)((at + i) >> 5)] |= (u64)(codes[i] & 3) << (2 * ((at + i) & 31)); }
    void clear(u64 at, u64 n) { for (u64 w = at >> 5; w <= (at + n) >> 5; ++w) words[kGuard + (size_t)w] = 0; }
};

struct Counters { uint64_t stale = 0, empty = 0, over_cap = 0, steps = 0, org_bad = 0; int max_diags = 0; };

// dal_kernels.h wave_dir, the 64 lanes in a loop
template <int DIR>
dal::Out wave_dir(const u64* abases, const u64* bbases, const dal::Task& T, const dal::Spec& S, int cap, Counters* n)
{
    const int R = dal::ring_size(cap);
    std::vector<int> V((size_t)2 * R), M((size_t)2 * R), O((size_t)2 * R);
    std::vector<u64> Tt((size_t)2 * R);
    dal::Ring W; W.V = V.data(); W.M = M.data(); W.T = Tt.data(); W.O = O.data(); W.mask = R - 1;
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
                if (cls & dal::kRecord) { rec |= 1ULL << l; if (o[l].o != T.k0) ++n->org_bad; }
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
    n->steps += (uint64_t)steps;
    if (max_diags > n->max_diags) n->max_diags = max_diags;
    return out;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: check_dalign CASES OUT [capacity [first_base]]\n"); return 2; }
    const int cap = argc > 3 ? atoi(argv[3]) : 512;
    const char* high = argc > 4 ? argv[4] : nullptr;
    Volume vhigh;
    u64 highest_first = 0, highest_last = 0;
    if (high) {          // the largest end any case needs
        std::ifstream pre(argv[1]);
        std::string h, r, t;
        u64 need = 0;
        while (std::getline(pre, h)) {
            if (h.empty()) continue;
            if (!std::getline(pre, r) || !std::getline(pre, t)) break;
            const u64 total = r.size() + t.size();
            need = std::max<u64>(need, high_base::first_base(high, total) + total);
        }
        vhigh.reserve_bases(need);
    }
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    Counters n;
    uint64_t cases = 0, bad = 0;
    std::string head, rs, ts;
    double spec_error = -1;
    rescue::DalignSpec hs;
    while (std::getline(in, head)) {
        if (head.empty()) continue;
        int qdir, qs, ss, min_size; double error;
        std::istringstream is(head);
        is >> qdir >> qs >> ss >> min_size >> error;
        if (!is || !std::getline(in, rs) || !std::getline(in, ts)) { fprintf(stderr, "bad case %lu\n", (unsigned long)cases); return 2; }
        auto code = [](char c) { return (u8)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3); };
        std::vector<u8> read(rs.size()), tmpl(ts.size()), strand(rs.size());
        for (size_t i = 0; i < rs.size(); ++i) read[i] = code(rs[i]);
        for (size_t i = 0; i < ts.size(); ++i) tmpl[i] = code(ts[i]);
        for (size_t i = 0; i < rs.size(); ++i) strand[i] = qdir ? (u8)(3 - read[rs.size() - 1 - i]) : read[i];
        if (error != spec_error) { hs = rescue::spec_for_error(error); spec_error = error; }
        const int alen = (int)rs.size(), blen = (int)ts.size();
        // the host code
        rescue::Dalign dal_host(hs);
        const bool want_ok = dal_host.go((const char*)strand.data(), qs, alen, (const char*)tmpl.data(), ss, blen, min_size);
        // the model: the read as the volume holds it, read on its strand through the Seq
        Volume va, vb;
        const u64 first = high ? high_base::first_base(high, (u64)alen + (u64)blen) : 0;
        if (high) { vhigh.put(first, read); vhigh.put(first + (u64)alen, tmpl); highest_first = std::max(highest_first, first); highest_last = std::max(highest_last, first + (u64)alen + (u64)blen - 1); }
        else { va.set(read); vb.set(tmpl); }
        // each volume holds one sequence from its base 0 - or both lie in the high buffer; the whole template
        const dal::Task T = pair::task_of(high ? pair::Job{0, qdir, 0, (i64)first, alen, (i64)(first + (u64)alen), 0, blen, qs, ss} : pair::Job{0, qdir, 0, 0, alen, 0, 0, blen, qs, ss});
        dal::Spec S; S.ave_path = hs.ave_path; S.table = hs.table.data(); S.score = hs.score.data();
        const u64* abases = high ? vhigh.bases() : va.bases();
        const u64* bbases = high ? vhigh.bases() : vb.bases();
        dal::Out f = wave_dir<+1>(abases, bbases, T, S, cap, &n);
        dal::Out b = wave_dir<-1>(abases, bbases, T, S, cap, &n);
        if (high) vhigh.clear(first, (u64)alen + (u64)blen);
        const int flags = f.flag | b.flag;
        if (flags & dal::kFlagStale) ++n.stale;
        if (flags & dal::kFlagEmpty) ++n.empty;
        if (flags & dal::kFlagOverCap) ++n.over_cap;
        const int how = flags ? 1 : 0;
        if (how) pair::tips_of(dal_host.r, &f, &b);          // dal_solve's last tier: the host code's result as the tips that decode to it
        necat_dalign_result r;
        memset(&r, 0, sizeof r);
        pair::decode(f, b, min_size, &r);
        const bool same = r.ok == (int)want_ok && r.qoff == dal_host.r.abpos && r.qend == dal_host.r.aepos && r.soff == dal_host.r.bbpos && r.send == dal_host.r.bepos &&
                          r.diffs == dal_host.r.diffs && r.ident_perc == dal_host.ident_perc;
        if (!same) {
            ++bad;
            fprintf(stderr, "case %lu: model %d %d %d %d %d %d, host %d %d %d %d %d %d\n", (unsigned long)cases, r.ok, r.qoff, r.qend, r.soff, r.send, r.diffs, (int)want_ok,
                    dal_host.r.abpos, dal_host.r.aepos, dal_host.r.bbpos, dal_host.r.bepos, dal_host.r.diffs);
        }
        fprintf(out, "%d %d %d %d %d %d %.17g %d\n", r.ok, r.qoff, r.qend, r.soff, r.send, r.diffs, r.ident_perc, how);
        ++cases;
    }
    fclose(out);
    if (high) printf("first_base=%llu last_base=%llu ", (unsigned long long)highest_first, (unsigned long long)highest_last);
    printf("cases=%lu stale=%lu empty=%lu over_cap=%lu max_diags=%d steps=%lu org_bad=%lu\n", (unsigned long)cases, (unsigned long)n.stale, (unsigned long)n.empty,
           (unsigned long)n.over_cap, n.max_diags, (unsigned long)n.steps, (unsigned long)n.org_bad);
    return bad || n.org_bad ? 1 : 0;
}
