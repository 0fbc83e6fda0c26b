// check_rm_spec.cpp - CPU model of necat_map_reference's speculative rescue pass (NECAT_RM_RESCUE_DEVICE=1, necat_amd/csrc/stage_refmap.inl): for EVERY candidate of a
// read whose block-wise alignment succeeded and falls short of its chain the rescue pair is computed ahead of the walk in the DEVICE's formulation - DALIGNER's wave of
// dal_core.h on a task whose subject is the candidate's stretch of the reference as a SLICE of the volume's words (the lane-by-lane model of check_dalign.cpp), edlib's
// path through nw_core.h's solve (the model of check_nw.cpp) - into a table of rm::Rescue, the walk of rm_host.h replays the read with the table provider, and every
// record is compared for EQUALITY with what rm::Worker::replay (the host provider: rescue::Dalign + rescue::EdlibGo on the decoded stretch) gives.
//
//   check_rm_spec [map options as oc2rm_worker takes them] wrk_dir reference out      (built with -DCHECK_RM_SPEC_ORACLE and the oracle's object)
// candidates and block-wise records exactly as check_rm.cpp produces them (that file is included, its rm::Worker replaced by the comparing one below); the records
// are written for the test to compare with the reference's own program.  CHECK_RM_SPEC_DIAGS in the environment: the model's capacity (default 512 diagonals).
//   check_rm_spec crafted CAPACITY SEED
// crafted reads on two contigs that are adjacent pieces of one genome: stretches clipped at a sequence's start and end, a read across the junction, slice starts at
// many residues mod 32, both strands, long indels (windows of hundreds of diagonals), a candidate inside an earlier RESCUED record, jobs DALIGNER rejects and jobs edlib rejects.
// What this models is the FORMULATION (the job filter, the task's slice, k0 / mida, the decode, the job of the global half and the `from` convention) and the seam of
// rm_host.h.  The formulation is rescue_pair.h's: tasks, decode, tips, the global half's jobs and their way back come from the functions rm_speculate calls, on jobs
// filled as it fills them, with the sequences' first bases moved into the checker's own word buffer.
// Last line of stdout: need= tried= rescued= dal_host= nw_jobs= max_diags= (crafted: more).  Exit status 1 on any difference, a failed self-check or a missed expectation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define NECAT_DAL_TRACK_ORG 1          // check_dalign.cpp's model carries every point's org
#include "../../necat_amd/csrc/dal_core.h"
#include "../../necat_amd/csrc/nw_core.h"
#include "../../necat_amd/csrc/rescue.h"
#include "../../necat_amd/csrc/rescue_pair.h"
#include "../../necat_amd/csrc/rm_host.h"
#include "high_base.h"          // (what the two files below include for their own first-base argument: here, outside the namespaces)

// the two models, as the files that test them alone define them (their main()s are not used)
namespace dal_model {
#define main check_dalign_main
#include "check_dalign.cpp"
#undef main
}
namespace nw_model {
#define main check_nw_main
#include "check_nw.cpp"
#undef main
}

using namespace necat;

namespace rmspec {

constexpr int kGuard = 4;
int g_cap = 512;                    // NECAT_DALIGN_DIAGS of the model
uint64_t g_need = 0, g_tried = 0, g_rescued = 0, g_dal_host = 0, g_dal_rejected = 0, g_nw_jobs = 0, g_nw_rejected = 0, g_reads = 0, g_unused = 0;
int g_max_diags = 0;
std::set<int> g_residues;           // (slice start in the volume) mod 32 over all jobs
uint64_t g_strand[2] = {0, 0}, g_from0 = 0, g_to_end = 0;

[[noreturn]] void die(const char* what, uint64_t i)
{
    fprintf(stderr, "check_rm_spec: %s (candidate %lu of read %lu)\n", what, (unsigned long)i, (unsigned long)g_reads);
    exit(1);
}

// One buffer of 2-bit words for a read's jobs, guard words around every piece: place() copies the words that hold bases [g_lo, g_hi) of a volume - the bases that share
// the first and the last word with the piece are the volume's own, as on the device - and returns what to add to a position of the volume to address the copy.
struct Pieces {
    std::vector<u64> w;
    Pieces() { w.assign(kGuard, 0); }
    i64 place(const necat_host::BaseWords& v, u64 g_lo, u64 g_hi)
    {
        const u64 w_lo = g_lo >> 5, w_hi = g_hi > g_lo ? (g_hi - 1) >> 5 : w_lo;
        const i64 shift = (i64)(w.size() << 5) - (i64)(w_lo << 5);
        for (u64 x = w_lo; x <= w_hi; ++x) w.push_back(g_hi > g_lo ? v.w[x - v.word0] : 0);
        w.insert(w.end(), kGuard, 0);
        return shift;
    }
};

// rm::Worker's interface for check_rm.cpp's loop: replay() computes the read's table as the device path does, replays with both providers and compares
struct SpecWorker {
    rm::Worker host;
    rescue::DalignSpec hs;
    double error;
    uint64_t n_rescue_tried = 0, n_rescued = 0;
    std::vector<rm::Rescue> table;
    SpecWorker(const rescue::DalignSpec& s, double e) : host(s, e), hs(s), error(e) {}

    void make_table(const necat_candidate* c, const necat_m4* m4, const uint8_t* ok, uint64_t lo, uint64_t hi, const necat_host::BaseWords& reads, const necat_host::BaseWords& ref,
                    int read_start_id, int ref_start_id, int min_align_size)
    {
        table.assign(hi, rm::Rescue{0, 0, 0, 0, 0, 0, 0.0});
        std::vector<uint64_t> need;
        for (uint64_t i = lo; i < hi; ++i) if (ok[i] && rm::needs_rescue(c[i], m4[i])) need.push_back(i);
        g_need += need.size();
        if (need.empty()) return;
        // ---- the local half: one dal::Task per job, a = the whole read on strand qdir, b = the stretch as a slice
        Pieces P;
        const int64_t q = c[need[0]].qid - read_start_id;
        const u64 qb = reads.seq_off[q], qs = reads.size(q);
        const i64 qshift = P.place(reads, qb, qb + qs);
        std::vector<pair::Job> pj(need.size());          // rescue_pair.h's jobs as rm_speculate fills them, the sequences' first bases moved into P
        for (size_t k = 0; k < need.size(); ++k) {
            const necat_candidate& cc = c[need[k]];
            if (cc.qid - read_start_id != q || cc.qsize != qs) die("a read's candidates name two reads", need[k]);
            const int64_t s = cc.sid - ref_start_id;
            const u64 sb = ref.seq_off[s], ss = ref.size(s);
            if (cc.ssize != ss) die("ssize is not the sequence's", need[k]);
            i64 from, to, woff;
            rm_window((i64)cc.qoff, (i64)qs, (i64)cc.soff, (i64)ss, &from, &to, &woff);
            if (from < 0 || to > (i64)ss || from > to) die("the stretch leaves its sequence", need[k]);
            const i64 tshift = P.place(ref, sb + (u64)from, sb + (u64)to);
            pj[k] = pair::Job{cc.qid, cc.qdir, cc.sid, (i64)qb + qshift, (i64)qs, (i64)sb + tshift, from, to - from, (i64)cc.qoff, woff};
            g_residues.insert((int)((sb + (u64)from) & 31));
            ++g_strand[cc.qdir ? 1 : 0];
            if (from == 0) ++g_from0;
            if (to == (i64)ss) ++g_to_end;
        }
        const u64* bases = P.w.data();
        dal::Spec S; S.ave_path = hs.ave_path; S.table = hs.table.data(); S.score = hs.score.data();
        std::vector<nw::Job> jobs;
        std::vector<necat_nw_job> nj;
        std::vector<size_t> job_of;
        std::vector<uint8_t> qseq, tseq;
        for (size_t k = 0; k < need.size(); ++k) {
            const necat_candidate& cc = c[need[k]];
            const i64 from = pj[k].from;
            const dal::Task T = pair::task_of(pj[k]);
            dal_model::Counters n;
            dal::Out f = dal_model::wave_dir<+1>(bases, bases, T, S, g_cap, &n);
            dal::Out b = dal_model::wave_dir<-1>(bases, bases, T, S, g_cap, &n);
            if (n.org_bad) die("a record's org is not the anchor's diagonal", need[k]);
            if (n.max_diags > g_max_diags) g_max_diags = n.max_diags;
            if (f.flag | b.flag) {          // dal_solve's last tier: rescue::Dalign on the slices, its result as the pair of tips that decodes to it
                ++g_dal_host;
                qseq.resize(qs); reads.decode(q, cc.qdir, 0, (int64_t)qs, qseq.data());
                tseq.resize((size_t)T.b.len); ref.decode(cc.sid - ref_start_id, 0, from, from + T.b.len, tseq.data());
                rescue::Dalign D(hs);
                (void)D.go((const char*)qseq.data(), (T.mida + T.k0) / 2, T.a.len, (const char*)tseq.data(), (T.mida - T.k0) / 2, T.b.len, 1);
                pair::tips_of(D.r, &f, &b);
            }
            necat_dalign_result r;
            pair::decode(f, b, min_align_size, &r);
            table[need[k]].tried = 1;
            if (r.soff < 0 || r.send > T.b.len || r.qoff < 0 || r.qend > T.a.len) die("DALIGNER's range leaves the stretch", need[k]);
            if (!r.ok) { ++g_dal_rejected; continue; }
            // ---- the global half: the job pair_global hands to nw_run, addressed as nw_run addresses it
            const necat_nw_job j = pair::nw_job(cc.qid, cc.qdir, cc.sid, from, r);
            nw::Job J;
            J.m = j.qto - j.qfrom; J.n = j.sto - j.sfrom; J.tolerance = j.tolerance;
            J.q = pair::strand_seq(pj[k].qbegin, pj[k].qlen, j.qdir, j.qfrom);
            J.t = pair::strand_seq(pj[k].sbegin, (i64)cc.ssize, 0, j.sfrom);
            jobs.push_back(J); nj.push_back(j); job_of.push_back(k);
        }
        g_nw_jobs += jobs.size();
        if (jobs.empty()) return;
        nw_model::Model M;
        M.words.assign(kGuard, 0);          // (Model::bases() skips its own guard words)
        M.words.insert(M.words.end(), P.w.begin(), P.w.end());
        std::vector<nw::JobOut> o;
        nw::Stats st;
        if (nw::solve(M, jobs, error, min_align_size, 4, 64ULL << 20, &o, &st)) die("nw::solve failed", need[0]);
        if (M.selfcheck) die("a leaf failed its self-check", need[0]);
        for (size_t x = 0; x < jobs.size(); ++x) {
            const size_t k = job_of[x];
            if (o[x].fail) die("the model flagged a global job", need[k]);
            if (!o[x].ok) { ++g_nw_rejected; continue; }
            // what nw_run reports for the job, on the sequence; pair_global takes it back to the STRETCH (rm::Rescue's convention)
            necat_nw_result r;
            memset(&r, 0, sizeof r);
            r.ok = 1; r.qoff = nj[x].qfrom + o[x].qoff; r.qend = nj[x].qfrom + o[x].qend; r.toff = nj[x].sfrom + o[x].toff; r.tend = nj[x].sfrom + o[x].tend;
            pair::to_slice(pj[k].from, &r);
            table[need[k]] = rm::Rescue{1, 1, r.qoff, r.qend, r.toff, r.tend, 100.0 * (o[x].asz - o[x].dist) / o[x].asz};
        }
    }

    void replay(const necat_candidate* c, const necat_m4* m4, const uint8_t* ok, uint64_t lo, uint64_t hi, const necat_host::BaseWords& reads, const necat_host::BaseWords& ref,
                int read_start_id, int ref_start_id, int min_align_size, std::vector<necat_m4>& out)
    {
        std::vector<necat_m4> want, got;
        const uint64_t t0 = host.n_rescue_tried, r0 = host.n_rescued;
        host.replay(c, m4, ok, lo, hi, reads, ref, read_start_id, ref_start_id, min_align_size, want);
        const uint64_t need0 = g_need;
        make_table(c, m4, ok, lo, hi, reads, ref, read_start_id, ref_start_id, min_align_size);
        rm::TableWorker tw(table.data());
        tw.replay(c, m4, ok, lo, hi, got);
        if (tw.n_missing) die("the walk asked for a pair the table does not hold", lo);
        if (tw.n_rescue_tried != host.n_rescue_tried - t0 || tw.n_rescued != host.n_rescued - r0) die("the two providers' counters differ", lo);
        if (got.size() != want.size()) die("the two providers give different numbers of records", lo);
        for (size_t j = 0; j < got.size(); ++j) {
            const necat_m4 &a = got[j], &b = want[j];
            const bool same = a.qid == b.qid && a.qdir == b.qdir && a.qoff == b.qoff && a.qend == b.qend && a.qext == b.qext && a.qsize == b.qsize && a.sid == b.sid &&
                              a.sdir == b.sdir && a.soff == b.soff && a.send == b.send && a.sext == b.sext && a.ssize == b.ssize && a.ident_perc == b.ident_perc &&
                              a.vscore == b.vscore;
            if (!same) {
                fprintf(stderr, "record %zu: table %lu %lu %lu %lu %.17g, host %lu %lu %lu %lu %.17g\n", j, (unsigned long)a.qoff, (unsigned long)a.qend, (unsigned long)a.soff,
                        (unsigned long)a.send, a.ident_perc, (unsigned long)b.qoff, (unsigned long)b.qend, (unsigned long)b.soff, (unsigned long)b.send, b.ident_perc);
                die("a record differs between the providers", lo);
            }
            if (a.send > a.ssize || a.soff > a.send || a.qend > a.qsize) die("a record leaves its sequences", lo);
        }
        n_rescue_tried += tw.n_rescue_tried; n_rescued += tw.n_rescued;
        g_tried += tw.n_rescue_tried; g_rescued += tw.n_rescued;
        g_unused += (g_need - need0) - tw.n_rescue_tried;
        ++g_reads;
        out.insert(out.end(), got.begin(), got.end());
    }
};

}  // namespace rmspec

#ifdef CHECK_RM_SPEC_ORACLE
// check_rm.cpp's seeding, block-wise records and output, its rm::Worker being the comparing one
namespace necat { namespace rm { typedef rmspec::SpecWorker SpecWorker; } }
#define Worker SpecWorker
#define main check_rm_main
#include "check_rm.cpp"
#undef main
#undef Worker
#endif

namespace {

// ---------------------------------------------------------------------------------------------------------------- crafted cases
typedef std::mt19937_64 Rng;

struct Vol {
    std::vector<uint64_t> w, off;
    std::vector<std::vector<uint8_t>> seqs;
    void add(const std::vector<uint8_t>& s) { seqs.push_back(s); }
    void pack()
    {
        off.assign(1, 0);
        for (auto& s : seqs) off.push_back(off.back() + s.size());
        w.assign((off.back() + 31) / 32 + 1, 0);
        for (size_t i = 0; i < seqs.size(); ++i)
            for (size_t k = 0; k < seqs[i].size(); ++k) { const uint64_t g = off[i] + k; w[g >> 5] |= (uint64_t)seqs[i][k] << ((g & 31) * 2); }
    }
    necat_host::BaseWords view() const { necat_host::BaseWords b; b.w = w.data(); b.seq_off = off.data(); return b; }
};

std::vector<uint8_t> revcomp(const std::vector<uint8_t>& s)
{
    std::vector<uint8_t> r(s.size());
    for (size_t i = 0; i < s.size(); ++i) r[i] = (uint8_t)(3 - s[s.size() - 1 - i]);
    return r;
}

void mutate(const std::vector<uint8_t>& G, size_t a, size_t b, int per_mille, Rng& rng, std::vector<uint8_t>& out)
{
    for (size_t i = a; i < b; ++i) {
        const int r = (int)(rng() % 1000);
        if (r < per_mille / 3) out.push_back((uint8_t)((G[i] + 1 + rng() % 3) & 3));
        else if (r < 2 * per_mille / 3) continue;
        else if (r < per_mille) { out.push_back((uint8_t)(rng() & 3)); out.push_back(G[i]); }
        else out.push_back(G[i]);
    }
}

// G[a, b) with errors, 40 exact bases around every anchor (genome positions, ascending, 20 inside [a, b) and 60 apart); qoff[k]: anchor k on the read
// indel != 0: 300 bases behind the last anchor the read skips `indel` bases of the genome (> 0) or carries -indel random bases the genome lacks (< 0)
std::vector<uint8_t> make_read(const std::vector<uint8_t>& G, size_t a, size_t b, const std::vector<size_t>& anchors, int per_mille, Rng& rng, std::vector<size_t>* qoff, int indel = 0)
{
    std::vector<uint8_t> r;
    size_t at = a;
    qoff->clear();
    for (size_t p : anchors) {
        mutate(G, at, p - 20, per_mille, rng, r);
        qoff->push_back(r.size() + 20);
        r.insert(r.end(), G.begin() + (ptrdiff_t)(p - 20), G.begin() + (ptrdiff_t)(p + 20));
        at = p + 20;
    }
    if (indel) {
        mutate(G, at, at + 300, per_mille, rng, r);
        at += 300;
        if (indel > 0) at += (size_t)indel;
        else for (int i = 0; i < -indel; ++i) r.push_back((uint8_t)(rng() & 3));
    }
    mutate(G, at, b, per_mille, rng, r);
    return r;
}

struct Crafted {
    Vol reads, ref;
    std::vector<necat_candidate> c;
    std::vector<necat_m4> m4;
    std::vector<uint8_t> ok;
    std::vector<uint64_t> group;          // candidates [group[r], group[r + 1]) are read r's
};

// a candidate with its anchor at (qoff on the read's strand qdir, soff on sequence sid) and a block-wise record that covers `cover` bases on either side of it
void add_candidate(Crafted& X, int qid, size_t qsize, int qdir, size_t qoff, int sid, size_t ssize, size_t soff, size_t cover, int is_ok)
{
    necat_candidate c;
    memset(&c, 0, sizeof c);
    c.qid = qid; c.sid = sid; c.qdir = qdir; c.sdir = 0; c.score = 50;
    c.qsize = qsize; c.ssize = ssize; c.qoff = qoff; c.soff = soff;
    c.qbeg = qoff > 1000 ? qoff - 1000 : 0; c.qend = std::min(qsize, qoff + 1000);
    c.sbeg = soff > 1000 ? soff - 1000 : 0; c.send = std::min(ssize, soff + 1000);
    necat_m4 m;
    memset(&m, 0, sizeof m);
    m.qid = qid; m.qdir = qdir; m.qoff = qoff > cover ? qoff - cover : 0; m.qend = std::min(qsize, qoff + cover); m.qext = qoff; m.qsize = qsize;
    m.sid = sid; m.sdir = 0; m.soff = soff > cover ? soff - cover : 0; m.send = std::min(ssize, soff + cover); m.sext = soff; m.ssize = ssize;
    m.ident_perc = 90.0; m.vscore = c.score;
    if (qdir == 1) { const uint64_t qo = m.qsize - m.qend, qe = m.qsize - m.qoff; m.qoff = qo; m.qend = qe; }
    X.c.push_back(c); X.m4.push_back(m); X.ok.push_back((uint8_t)is_ok);
}

#define EXPECT(cond, what) do { if (!(cond)) { fprintf(stderr, "check_rm_spec crafted: %s\n", what); return 1; } } while (0)

int crafted(int cap, uint64_t seed)
{
    rmspec::g_cap = cap;
    Rng rng(seed);
    // one genome of 11000 bases as two adjacent contigs; 6000 % 32 == 16: ctg1 begins inside a word
    const size_t L0 = 6000, L1 = 5000;
    std::vector<uint8_t> G(L0 + L1);
    for (auto& b : G) b = (uint8_t)(rng() & 3);
    Crafted X;
    X.ref.add(std::vector<uint8_t>(G.begin(), G.begin() + (ptrdiff_t)L0));
    X.ref.add(std::vector<uint8_t>(G.begin() + (ptrdiff_t)L0, G.end()));
    X.ref.pack();
    const size_t ssize[2] = {L0, L1}, sbase[2] = {0, L0};
    struct Plan { size_t a, b; std::vector<size_t> anchors; int qdir, per_mille; size_t prefix, cover2; int indel = 0; };          // prefix: unrelated bases in front of the read
    std::vector<Plan> plans;
    // (a) stretches clipped at a sequence's start (from == 0) and end (to == ssize), on both contigs and both strands
    for (int qdir = 0; qdir < 2; ++qdir) {
        plans.push_back(Plan{100, 2600, {1300}, qdir, 120, 0, 0});
        plans.push_back(Plan{L0 - 2500, L0 - 80, {L0 - 1300}, qdir, 120, 0, 0});
        plans.push_back(Plan{L0 + 60, L0 + 2500, {L0 + 1200}, qdir, 120, 0, 0});
        plans.push_back(Plan{L0 + L1 - 2400, L0 + L1 - 50, {L0 + L1 - 1200}, qdir, 120, 0, 0});
        // (b) across the junction: an anchor on either contig; the alignment stops at the contig's end / start
        plans.push_back(Plan{L0 - 1600, L0 + 1500, {L0 - 700, L0 + 600}, qdir, 100, 0, 0});
    }
    const size_t n_fixed = plans.size();
    // (c), (d) stretches inside the contigs: slice starts at whatever residue mod 32 they fall on, strands alternate
    for (int i = 0; i < 40; ++i) {
        const int on = i & 1;
        const size_t len = 1800 + rng() % 700, a = sbase[on] + 900 + rng() % (ssize[on] - 1800 - len), p = a + 600 + rng() % (len - 1200);
        plans.push_back(Plan{a, a + len, {p}, (i >> 1) & 1, 60 + (int)(rng() % 120), 0, 0});
    }
    const size_t n_inside = plans.size();
    // (e) two anchors of one read, both short of the chain: the second lies inside the record the first one's rescue gives, not inside its block-wise record
    for (int qdir = 0; qdir < 2; ++qdir) plans.push_back(Plan{1000, 4000, {1800, 3100}, qdir, 100, 0, 60});
    const size_t n_contained = plans.size();
    // (f) DALIGNER rejects: a read that hangs 1500 bases off the start of ctg0 with its anchor 150 bases from its end - a stretch of under 300 bases, below the 400 asked for
    for (int qdir = 0; qdir < 2; ++qdir) plans.push_back(Plan{0, 250, {100}, qdir, 100, 1500, 0});
    const size_t n_reject = plans.size();
    // long indels behind the anchor, what the pair is for: a stretch of 350 bases missing from the read, 350 bases the genome lacks - windows of hundreds of diagonals
    for (int qdir = 0; qdir < 2; ++qdir)
        for (int indel : {350, -350}) { Plan P{1200, 4600, {2200}, qdir, 80, 0, 0}; P.indel = indel; plans.push_back(P); }
    std::vector<std::vector<size_t>> qoffs(plans.size());
    for (size_t r = 0; r < plans.size(); ++r) {
        const Plan& P = plans[r];
        std::vector<uint8_t> rd = make_read(G, P.a, P.b, P.anchors, P.per_mille, rng, &qoffs[r], P.indel);
        if (P.prefix) {
            std::vector<uint8_t> pre(P.prefix);
            for (auto& b : pre) b = (uint8_t)(rng() & 3);
            rd.insert(rd.begin(), pre.begin(), pre.end());
            for (size_t& x : qoffs[r]) x += P.prefix;
        }
        X.reads.add(P.qdir ? revcomp(rd) : rd);
    }
    X.reads.pack();
    for (size_t r = 0; r < plans.size(); ++r) {
        const Plan& P = plans[r];
        X.group.push_back(X.c.size());
        for (size_t k = 0; k < P.anchors.size(); ++k) {
            const int sid = P.anchors[k] >= L0 ? 1 : 0;
            add_candidate(X, (int)r, X.reads.seqs[r].size(), P.qdir, qoffs[r][k], sid, ssize[sid], P.anchors[k] - sbase[sid], k && P.cover2 ? P.cover2 : 80, 1);
        }
        // one more of the same anchor whose block-wise alignment failed: dropped, or skipped as contained
        add_candidate(X, (int)r, X.reads.seqs[r].size(), P.qdir, qoffs[r][0], P.anchors[0] >= L0 ? 1 : 0, ssize[P.anchors[0] >= L0 ? 1 : 0], P.anchors[0] - sbase[P.anchors[0] >= L0 ? 1 : 0], 80, 0);
    }
    X.group.push_back(X.c.size());
    const necat_host::BaseWords hr = X.reads.view(), hf = X.ref.view();
    uint64_t records = 0;
    auto run = [&](double error, size_t r_lo, size_t r_hi, int min_align, std::vector<std::vector<necat_m4>>* keep) {
        const rescue::DalignSpec hs = rescue::spec_for_error(error);
        rmspec::SpecWorker wk(hs, error);
        for (size_t r = r_lo; r < r_hi; ++r) {
            std::vector<necat_m4> acc;
            wk.replay(X.c.data(), X.m4.data(), X.ok.data(), X.group[r], X.group[r + 1], hr, hf, 0, 0, min_align, acc);
            records += acc.size();
            if (keep) keep->push_back(acc);
        }
    };
    // ---- (a), (b)
    std::vector<std::vector<necat_m4>> fixed;
    run(0.5, 0, n_fixed, 400, &fixed);
    EXPECT(rmspec::g_from0 >= 4 && rmspec::g_to_end >= 4, "no stretch was clipped at a sequence's start / end");
    EXPECT(rmspec::g_need == 12 && rmspec::g_tried == rmspec::g_need && rmspec::g_rescued == rmspec::g_need, "(a), (b): every anchor is rescued once");
    for (size_t r = 4; r < n_fixed; r += 5) {          // the junction reads: one record per contig, each ending at the junction
        EXPECT(fixed[r].size() == 2, "(b): two records, one per contig");
        const necat_m4 &m0 = fixed[r][0], &m1 = fixed[r][1];
        EXPECT(m0.sid == 0 && m0.send <= L0 && m0.send + 200 > L0 && m1.sid == 1 && m1.soff < 200, "(b): the alignments stop at the junction");
    }
    // ---- (c), (d)
    run(0.5, n_fixed, n_inside, 400, nullptr);
    EXPECT(rmspec::g_residues.size() >= 12 && rmspec::g_residues.count(16), "(c): the slice starts cover few residues mod 32");
    EXPECT(rmspec::g_strand[0] >= 20 && rmspec::g_strand[1] >= 20, "(d): both strands");
    EXPECT(rmspec::g_tried == rmspec::g_need && rmspec::g_rescued >= rmspec::g_need - 2, "(c), (d): the reads inside the contigs are rescued");
    // ---- (e)
    const uint64_t need0 = rmspec::g_need, tried0 = rmspec::g_tried, rec0 = records, unused0 = rmspec::g_unused;
    run(0.5, n_inside, n_contained, 400, nullptr);
    EXPECT(rmspec::g_need - need0 == 4 && rmspec::g_tried - tried0 == 2 && records - rec0 == 2 && rmspec::g_unused - unused0 == 2, "(e): the contained candidate's entry is not used");
    // ---- (f) DALIGNER rejects
    const uint64_t rej0 = rmspec::g_dal_rejected, rec1 = records;
    run(0.5, n_contained, n_reject, 400, nullptr);
    EXPECT(rmspec::g_dal_rejected - rej0 == 2 && records == rec1, "(f): DALIGNER's rejection drops the candidate");
    // ---- long indels: rescued across the indel, through windows far wider than the error-only reads give
    {
        const uint64_t resc0 = rmspec::g_rescued;
        const int w0 = rmspec::g_max_diags;
        std::vector<std::vector<necat_m4>> ind;
        run(0.5, n_reject, plans.size(), 400, &ind);
        EXPECT(rmspec::g_rescued - resc0 == 4 && w0 < 64, "the long-indel reads are rescued");
        // (a window above 64 diagonals goes through the wave in several chunks of lanes, above 128 in three or more: the path the error-only reads never take)
        EXPECT(rmspec::g_cap <= 128 || rmspec::g_max_diags > 128, "the long indels do not widen the window");
        for (auto& v : ind) EXPECT(v.size() == 1 && v[0].qend - v[0].qoff > 2500, "a long-indel record does not span the indel");
    }
    // ---- (f) edlib rejects: at a low error rate DALIGNER's range is accepted by its own test and its distance is above error x the subject range
    const uint64_t nwrej0 = rmspec::g_nw_rejected;
    run(0.08, n_fixed, n_inside, 400, nullptr);
    EXPECT(rmspec::g_nw_rejected - nwrej0 >= 1, "(f): no job that edlib rejects");
    printf("reads=%lu records=%lu need=%lu tried=%lu rescued=%lu unused=%lu dal_host=%lu dal_rejected=%lu nw_jobs=%lu nw_rejected=%lu max_diags=%d residues=%zu from0=%lu to_end=%lu\n",
           (unsigned long)rmspec::g_reads, (unsigned long)records, (unsigned long)rmspec::g_need, (unsigned long)rmspec::g_tried, (unsigned long)rmspec::g_rescued,
           (unsigned long)rmspec::g_unused, (unsigned long)rmspec::g_dal_host, (unsigned long)rmspec::g_dal_rejected, (unsigned long)rmspec::g_nw_jobs, (unsigned long)rmspec::g_nw_rejected,
           rmspec::g_max_diags, rmspec::g_residues.size(), (unsigned long)rmspec::g_from0, (unsigned long)rmspec::g_to_end);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "crafted")) return crafted(argc > 2 ? atoi(argv[2]) : 512, argc > 3 ? strtoull(argv[3], nullptr, 10) : 11);
#ifdef CHECK_RM_SPEC_ORACLE
    if (const char* e = getenv("CHECK_RM_SPEC_DIAGS")) rmspec::g_cap = atoi(e);
    const int rc = check_rm_main(argc, argv);
    if (rc) return rc;
    printf("need=%lu tried=%lu rescued=%lu dal_host=%lu nw_jobs=%lu max_diags=%d\n", (unsigned long)rmspec::g_need, (unsigned long)rmspec::g_tried, (unsigned long)rmspec::g_rescued,
           (unsigned long)rmspec::g_dal_host, (unsigned long)rmspec::g_nw_jobs, rmspec::g_max_diags);
    return 0;
#else
    fprintf(stderr, "usage: check_rm_spec crafted [capacity] [seed]   (the data sets need a build with -DCHECK_RM_SPEC_ORACLE)\n");
    return 2;
#endif
}
