// item_order_waste.cpp - MEASUREMENT ONLY (tools/item_order_waste.py runs it).  What the consumers of a round's lists issue for nothing because the
// ragged blocks arrive in mixed sizes, and what the size-class order (necat_amd/csrc/item_order.h) leaves of it - on the CPU, before any kernel is touched.
// Every candidate of a volume (the oracle's, as check_core.cpp takes them) is replayed block by block with the product's cores (ext_plan, myers_block, the walk,
// ext_finish_block), and every NON-FULL block is put into the list of the round it would run in: a candidate starts in round 0, the successor of a list-A block
// runs a round later, that of a list-B block two rounds later (stage_extend.inl).  Arrival order = candidate order within a round (the device's order is what its
// atomics give: no better model).  One batch.  Per list - A's ragged part, B - over all rounds:
//     needed = sum of the blocks' steps (tn + nblk - 1)
//     issued = sum over groups of g neighbouring items of (items x the group's longest block's steps), g = 4, 8, 64
// in arrival order and in size-class order.
// usage: item_order_waste <wrk_dir> <vid> k z q b s n a e
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>

#include "../../necat_amd/csrc/seed_core.h"
#include "../../necat_amd/csrc/dp_core.h"
#include "../../necat_amd/csrc/ext_core.h"
#include "../../necat_amd/csrc/item_order.h"
extern "C" {
#include "../../oracle/necat_oracle.h"
}
using namespace necat;

constexpr int kBlk = kOcaBlockSize, kNwMax = kMaxWords;

struct HostVol { std::vector<u64> words; std::vector<u64> off; DevVolume dv; };
static void make_vol(const ora_volume& v, HostVol& h)
{
    const int G = 4;
    h.words.assign((v.nbases + 31) / 32 + 2 * G, 0);
    for (u64 i = 0; i < v.nbases; ++i) h.words[G + (i >> 5)] |= (u64)((v.pac[i >> 2] >> ((~i & 3) << 1)) & 3) << ((i & 31) * 2);
    h.off.resize(v.nseq + 1);
    for (u64 i = 0; i < v.nseq; ++i) h.off[i] = v.offset[i];
    h.off[v.nseq] = v.nbases;
    h.dv.bases = h.words.data() + G; h.dv.seq_off = h.off.data(); h.dv.nbases = v.nbases; h.dv.nseq = v.nseq;
}
struct HTgt { const u64* w; int code(int c) { return (int)((w[c >> 5] >> ((c & 31) * 2)) & 3); } };
struct HMat {
    std::vector<u64> Pv, Ph; int nw;
    void init(int cols, int nw_) { nw = nw_; Pv.assign((size_t)cols * nw, 0); Ph.assign((size_t)cols * nw, 0); }
    void store(int c, int b, u64 pv, u64 ph) { Pv[(size_t)c * nw + b] = pv; Ph[(size_t)c * nw + b] = ph; }
    bool skip_nw() const { return false; }
};
struct HMatR { const HMat* m; void rec(int c, int b, u64& Pv, u64& Ph) const { Pv = m->Pv[(size_t)c * m->nw + b]; Ph = m->Ph[(size_t)c * m->nw + b]; } };
struct HOps { std::vector<int> v; TailScan ts; void push(int op) { v.push_back(op); tail_push(ts, op); } };
struct HRops { const std::vector<int>* v; int operator()(int j) const { return (*v)[j]; } };
struct HSame {
    const MyersRegs<kNwMax>* R; const u64* tw;
    bool operator()(int i) const {
        int q = (int)((~R->nlo[i >> 6] >> (i & 63)) & 1) | ((int)((~R->nhi[i >> 6] >> (i & 63)) & 1) << 1);
        return q == (int)((tw[i >> 5] >> ((i & 31) * 2)) & 3);
    }
};

struct Blk { int qn, tn; };
static int steps_of(const Blk& b) { return b.tn + (b.qn + 63) / 64 - 1; }
static unsigned long long issued(const std::vector<Blk>& v, int g)
{
    unsigned long long s = 0;
    for (size_t i = 0; i < v.size(); i += g) {
        const size_t e = std::min(v.size(), i + g); int mx = 0;
        for (size_t q = i; q < e; ++q) mx = std::max(mx, steps_of(v[q]));
        s += (unsigned long long)(e - i) * mx;
    }
    return s;
}

int main(int argc, char** argv)
{
    if (argc < 11) { fprintf(stderr, "usage: %s wrk_dir vid k z q b s n a e\n", argv[0]); return 2; }
    const char* wrk = argv[1]; const int vid = atoi(argv[2]);
    ora_options opt; ora_options_default(&opt);
    opt.kmer_size = atoi(argv[3]); opt.scan_window = atoi(argv[4]); opt.kmer_cnt_cutoff = atoi(argv[5]); opt.block_size = atoi(argv[6]);
    opt.block_score_cutoff = atoi(argv[7]); opt.num_candidates = atoi(argv[8]); opt.align_size_cutoff = atoi(argv[9]); opt.error = atof(argv[10]);
    opt.job = 1;
    ora_volumes_info vi;
    if (ora_volumes_info_load(wrk, &vi)) return 2;
    ora_volume ref;
    if (ora_volume_load(vi.names[vid], &ref)) return 2;
    ora_index* ix = ora_index_build(&ref, opt.kmer_size, opt.kmer_cnt_cutoff);
    HostVol href; make_vol(ref, href);
    ora_wfd* w = ora_wfd_new(ref.nbases, opt.block_size, opt.kmer_size, opt.block_score_cutoff);
    ora_can_vec oc = {0, 0, 0};
    std::vector<uint8_t> fwd, rev;
    static MyersRegs<kNwMax> R; HMat mat; static u64 tw[2 * kNwMax + 2];
    std::vector<std::vector<Blk>> rounds[2];          // [0] list A's ragged blocks, [1] list B, per round
    long n_cand = 0, n_full = 0, n_blocks = 0;
    for (int r = 0; r < (int)ref.nseq; ++r) {
        const size_t L = ref.size[r];
        fwd.resize(L + 1); rev.resize(L + 1);
        oc.n = 0;
        ora_volume_extract(&ref, r, 0, fwd.data());
        ora_find_candidates(fwd.data(), (int)L, r, 0, vi.read_start_id[vid], vi.read_start_id[vid], 1, &ref, ix, &opt, w, &oc);
        ora_volume_extract(&ref, r, 1, rev.data());
        ora_find_candidates(rev.data(), (int)L, r, 1, vi.read_start_id[vid], vi.read_start_id[vid], 1, &ref, ix, &opt, w, &oc);
        std::vector<ora_candidate> ocv(oc.a, oc.a + oc.n);
        auto before = [](const ora_candidate& a, const ora_candidate& b) {
            if (a.score != b.score) return a.score > b.score; if (a.qdir != b.qdir) return a.qdir < b.qdir;
            if (a.sid != b.sid) return a.sid < b.sid; if (a.qoff != b.qoff) return a.qoff < b.qoff; return a.soff < b.soff; };
        std::sort(ocv.begin(), ocv.end(), before);
        if ((int)ocv.size() > opt.num_candidates) ocv.resize(opt.num_candidates);
        for (const ora_candidate& c : ocv) {
            ++n_cand;
            ExtTask tk;
            ext_init(tk, 0, c.qdir, (i64)href.off[c.qid], (i32)c.qsize, (i64)href.off[c.sid], (i32)c.ssize, (i32)c.qoff, (i32)c.soff);
            size_t round = 0;
            while (ext_plan<kBlk>(tk)) {
                const FragGeom g = ext_frag_geom(tk);
                const int qn = tk.qblk, tn = tk.tblk;
                const bool listA = qn <= kBlk && tn <= kBlk, full = qn == kBlk && tn == kBlk;
                ++n_blocks;
                if (full) ++n_full;
                else {
                    auto& rl = rounds[listA ? 0 : 1];
                    if (rl.size() <= round) rl.resize(round + 1);
                    rl[round].push_back(Blk{qn, tn});
                }
                round += listA ? 1 : 2;
                for (int b = 0; b < kNwMax; ++b) {
                    u64 lo = 0, hi = 0;
                    if (b * 64 < qn) load64_planes(href.dv.bases, g.q_base, g.q_dir, g.q_comp, b * 64, &lo, &hi);
                    R.nlo[b] = ~lo; R.nhi[b] = ~hi;
                }
                for (int x = 0; x * 32 < tn; ++x) tw[x] = load32_dir(href.dv.bases, g.t_base + (i64)g.t_dir * (x * 32), g.t_dir, 0);
                HTgt tg; tg.w = tw;
                mat.init(tn, kNwMax);
                const MyersResult mr = myers_block<kNwMax, false>(R, qn, tn, opt.error, tg, mat);
                const int done = ext_block_done(tk, mr.dist, mr.endc);
                HOps ops; tail_init(ops.ts, done ? 1 : kOcaMatCnt);
                if (mr.dist >= 0) { HMatR m{&mat}; traceback_block(qn, mr.endc + 1, m, ops); }
                HRops ro{&ops.v}; HSame sm{&R, tw};
                ext_finish_block(tk, mr.dist, mr.endc, done, ops.ts, ro, sm);
            }
        }
    }
    size_t n_rag = 0;
    for (const auto& v : rounds[0]) n_rag += v.size();
    printf("candidates=%ld blocks=%ld full=%ld ragged share of list A=%.4f\n", n_cand, n_blocks, n_full, n_full + n_rag ? (double)n_rag / (double)(n_full + n_rag) : 0.0);
    const char* names[2] = {"list A ragged", "list B"};
    for (int l = 0; l < 2; ++l) {
        unsigned long long needed = 0, arr[3] = {0, 0, 0}, srt[3] = {0, 0, 0}, nb = 0; const int gs[3] = {4, 8, 64};
        for (const auto& v : rounds[l]) {
            std::vector<Blk> s(v);
            std::stable_sort(s.begin(), s.end(), [](const Blk& a, const Blk& b) { return item_order_key(a.tn) < item_order_key(b.tn); });
            for (const Blk& b : v) needed += steps_of(b);
            nb += v.size();
            for (int k = 0; k < 3; ++k) { arr[k] += issued(v, gs[k]); srt[k] += issued(s, gs[k]); }
        }
        printf("%s: blocks=%llu rounds=%zu needed=%llu\n", names[l], nb, rounds[l].size(), needed);
        for (int k = 0; k < 3; ++k)
            printf("  groups of %2d: issued arrival=%llu (x%.3f)  size-class=%llu (x%.3f)  saved=%.1f%% of arrival\n", gs[k], arr[k], needed ? (double)arr[k] / needed : 0.0,
                   srt[k], needed ? (double)srt[k] / needed : 0.0, arr[k] ? 100.0 * (double)(arr[k] - srt[k]) / arr[k] : 0.0);
    }
    ora_wfd_free(w); free(oc.a);
    return 0;
}
