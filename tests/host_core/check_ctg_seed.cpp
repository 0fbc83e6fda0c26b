// check_ctg_seed.cpp - TEST ONLY.  The seeding of contig polishing on the CPU: the host form (necat_amd/csrc/ctg_seed.h) and the CPU model of the device cores
// (necat_amd/csrc/ctg_seed_core.h: table, seeds, word-wise extension, the per-diagonal kill test, the chain 64 predecessors at a time) against
//   * every job of the case files given (tests/ctg_seed_cases.py has the format): the sorted matches and the candidate, number for number; the model with the
//     segment's table filled forwards and backwards (the chains' order must not matter) and with the chain's arrays at the default LDS capacity and at 8;
//   * each other on `n_random` seeded random cases: segment 2 - 50 kb, reads at 1 - 15 % error on either strand, every third segment with repeats;
//   * for the candidate, the literal loop of chaining_find_candidates (ctg_seed::full_loop_first) against the reduction both use.
// usage: check_ctg_seed n_random seed [case file ..]
// prints  jobs= mismatches= random= random_mismatches= found= max_matches= max_mems= global_jobs= breaks_inside= breaks_at_63= breaks_later_step=
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../necat_amd/csrc/ctg_seed.h"
#include "../../necat_amd/csrc/ctg_seed_core.h"

namespace hs = necat_host::ctg_seed;
namespace ds = necat::ctg_seed;

constexpr uint32_t kLdsDefault = 512;      // NECAT_CTG_SEED_LDS
constexpr size_t kGuard = 4;               // words in front of and behind a volume, as the device's volumes have them

static int mismatches = 0, found = 0;
static uint32_t max_matches = 0, max_mems = 0;
static ds::ModelStats stats;

static void complain(const char* name, uint64_t job, const char* what) { ++mismatches; fprintf(stderr, "MISMATCH %s job %lu: %s\n", name, (unsigned long)job, what); }

struct Volume {
    std::vector<uint64_t> off, store;
    const uint64_t* words() const { return store.data() + kGuard; }
    void set(const std::vector<uint64_t>& o, const uint64_t* w, size_t nw) { off = o; store.assign(nw + 2 * kGuard, 0); if (nw) memcpy(store.data() + kGuard, w, 8 * nw); }
};

struct Expect { int32_t found, qbeg, qend, sbeg, send, qoff, soff, score; const int32_t* mems; int32_t n_mems; };

static bool same_can(const hs::Candidate& a, const ds::DCan& b)
{
    return a.found == b.found && a.qbeg == b.qbeg && a.qend == b.qend && a.sbeg == b.sbeg && a.send == b.send && a.qoff == b.qoff && a.soff == b.soff && a.score == b.score &&
           a.chain_len == b.chain_len;
}
static bool same_mems(const std::vector<hs::Mem>& a, const std::vector<ds::DMem>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].qoff != b[i].qoff || a[i].soff != b[i].soff || a[i].size != b[i].size) return false;
    return true;
}

// one job through the host form and the model (two tables, two capacities); e: the reference's answer, or nullptr
static void one_job(const char* name, uint64_t job, const hs::SegIndex& ix, const ds::Seq& seg, const ds::SegTable tabs[2], const Volume& reads, uint64_t qid, int qdir, const Expect* e)
{
    const int qsize = (int)(reads.off[qid + 1] - reads.off[qid]);
    std::vector<uint8_t> r;
    hs::decode(reads.words(), reads.off[qid], qsize, qdir, r);
    hs::JobOut h;
    if (!hs::seed_job(ix, r.data(), qsize, h)) complain(name, job, "two surviving matches share a start");
    if (h.can.found) ++found;
    max_matches = std::max(max_matches, h.n_matches); max_mems = std::max<uint32_t>(max_mems, (uint32_t)h.mems.size());
    const hs::Candidate full = hs::full_loop_first(h.mems.data(), (int)h.mems.size());
    if (memcmp(&full, &h.can, sizeof full)) complain(name, job, "the loop of chaining_find_candidates against the reduction");
    const ds::Seq rd = {reads.words(), (int64_t)reads.off[qid], qsize, qdir};
    for (int k = 0; k < 4; ++k) {
        ds::ModelOut m;
        ds::model_job(seg, tabs[k & 1], rd, k < 2 ? kLdsDefault : 8u, m, stats);
        if (m.n_matches != h.n_matches) complain(name, job, "the model's number of seeds");
        if (!m.unique_starts) complain(name, job, "two surviving matches of the model share a start");
        if (!same_mems(h.mems, m.mems)) complain(name, job, "the model's matches against the host form's");
        if (!same_can(h.can, m.can)) complain(name, job, "the model's candidate against the host form's");
    }
    if (e) {
        bool ok = (size_t)e->n_mems == h.mems.size();
        for (size_t i = 0; ok && i < h.mems.size(); ++i) ok = h.mems[i].qoff == e->mems[3 * i] && h.mems[i].soff == e->mems[3 * i + 1] && h.mems[i].size == e->mems[3 * i + 2];
        if (!ok) complain(name, job, "host form against the reference's matches");
        const hs::Candidate& c = h.can;
        if (c.found != e->found || (c.found && (c.qbeg != e->qbeg || c.qend != e->qend || c.sbeg != e->sbeg || c.send != e->send || c.qoff != e->qoff || c.soff != e->soff || c.score != e->score)))
            complain(name, job, "host form against the reference's candidate");
    }
}

static void one_segment(const Volume& contigs, int64_t ctg_id, int64_t from, int64_t size, hs::SegIndex& ix, ds::Seq& seg, ds::SegTable tabs[2])
{
    ix.build(contigs.words(), contigs.off[(size_t)ctg_id] + (uint64_t)from, (int)size);
    seg = ds::Seq{contigs.words(), (int64_t)(contigs.off[(size_t)ctg_id] + (uint64_t)from), (int)size, 0};
    ds::model_index(seg, tabs[0], false);
    ds::model_index(seg, tabs[1], true);
}

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static uint64_t run_file(const char* path)
{
    const std::vector<uint8_t> raw = slurp(path);
    if (raw.size() < 64 || memcmp(raw.data(), "CTGSEED1", 8)) { fprintf(stderr, "%s is no case file\n", path); exit(2); }
    uint64_t hd[7];
    memcpy(hd, raw.data() + 8, 56);
    const uint64_t nc = hd[0], ncw = hd[1], nr = hd[2], nrw = hd[3], ns = hd[4], nj = hd[5], nm = hd[6];
    size_t at = 64;
    auto volume = [&](uint64_t n, uint64_t nw, Volume& v) {
        std::vector<uint64_t> off(n + 1);
        memcpy(off.data(), raw.data() + at, 8 * (n + 1)); at += 8 * (n + 1);
        std::vector<uint64_t> w(nw + 1);
        if (nw) memcpy(w.data(), raw.data() + at, 8 * nw);
        at += 8 * nw;
        v.set(off, w.data(), nw);
    };
    Volume contigs, reads;
    volume(nc, ncw, contigs); volume(nr, nrw, reads);
    const size_t seg_at = at, job_at = at + 72 * ns, mem_at = job_at + 48 * nj;
    if (mem_at + 12 * nm != raw.size()) { fprintf(stderr, "%s: %zu bytes, the header says %zu\n", path, raw.size(), mem_at + 12 * (size_t)nm); exit(2); }
    std::vector<int32_t> jobs(12 * nj), mems(3 * nm + 3);
    if (nj) memcpy(jobs.data(), raw.data() + job_at, 48 * nj);
    if (nm) memcpy(mems.data(), raw.data() + mem_at, 12 * nm);
    std::vector<uint64_t> mem_off(nj + 1, 0);
    for (uint64_t j = 0; j < nj; ++j) mem_off[j + 1] = mem_off[j] + (uint64_t)jobs[12 * j + 10];
    for (uint64_t s = 0; s < ns; ++s) {
        char name[33] = {0};
        memcpy(name, raw.data() + seg_at + 72 * s, 32);
        int64_t v[5];
        memcpy(v, raw.data() + seg_at + 72 * s + 32, 40);
        hs::SegIndex ix; ds::Seq seg; ds::SegTable tabs[2];
        one_segment(contigs, v[0], v[1], v[2], ix, seg, tabs);
        for (int64_t j = v[3]; j < v[4]; ++j) {
            const int32_t* J = jobs.data() + 12 * j;
            const Expect e = {J[2], J[3], J[4], J[5], J[6], J[7], J[8], J[9], mems.data() + 3 * mem_off[(size_t)j], J[10]};
            one_job(name, (uint64_t)j, ix, seg, tabs, reads, (uint64_t)J[0], J[1], &e);
        }
    }
    return nj;
}

static void random_case(std::mt19937_64& rng, int id)
{
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int size = rnd(2000, 50000), pre = rnd(0, 70), post = rnd(0, 1) ? 0 : rnd(0, 70);
    std::vector<uint8_t> ctg((size_t)(pre + size + post));
    for (auto& b : ctg) b = (uint8_t)(rng() & 3);
    if (id % 3 == 0) {          // repeats: a unit of 30 - 400 bases copied to 2 - 25 places, and a poly-A run
        const int ul = rnd(30, 400), copies = rnd(2, 25);
        for (int c = 0; c < copies; ++c) { const int at = pre + rnd(0, size - ul - 1); for (int i = 0; i < ul; ++i) ctg[(size_t)(at + i)] = ctg[(size_t)(pre + 100 + i)]; }
        const int pa = pre + rnd(0, size - 60);
        for (int i = 0; i < rnd(15, 50); ++i) ctg[(size_t)(pa + i)] = 0;
    }
    const int n_reads = rnd(1, 4);
    std::vector<std::vector<uint8_t>> rs;
    for (int k = 0; k < n_reads; ++k) {
        const int a = rnd(0, size - 1000), len = rnd(200, std::min(12000, size - a));
        const double err = rnd(1, 15) / 100.0;
        std::vector<uint8_t> r;
        for (int i = 0; i < rnd(0, 40); ++i) r.push_back((uint8_t)(rng() & 3));
        for (int i = 0; i < len; ++i) {
            const double u = (double)(rng() % 100000) / 100000.0;
            const uint8_t b = ctg[(size_t)(pre + a + i)];
            if (u < err / 3) r.push_back((uint8_t)((b + 1 + rng() % 3) & 3));
            else if (u < 2 * err / 3) { r.push_back(b); r.push_back((uint8_t)(rng() & 3)); }
            else if (u >= err) r.push_back(b);
        }
        if (k == 0 && id % 5 == 0) for (int i = 0; i < 15 && i < (int)r.size(); ++i) r[(size_t)i] = 0;          // a read that begins with fifteen A's
        rs.push_back(r);
    }
    auto pack = [](const std::vector<std::vector<uint8_t>>& seqs, Volume& v) {
        std::vector<uint64_t> off(1, 0);
        uint64_t nb = 0;
        for (const auto& s : seqs) { nb += s.size(); off.push_back(nb); }
        std::vector<uint64_t> w(nb / 32 + 2, 0);
        uint64_t g = 0;
        for (const auto& s : seqs) for (uint8_t b : s) { w[g >> 5] |= (uint64_t)b << ((g & 31) * 2); ++g; }
        v.set(off, w.data(), w.size());
    };
    Volume contigs, reads;
    pack({ctg}, contigs); pack(rs, reads);
    hs::SegIndex ix; ds::Seq seg; ds::SegTable tabs[2];
    char name[32];
    snprintf(name, sizeof name, "random %d", id);
    one_segment(contigs, 0, pre, size, ix, seg, tabs);
    for (int k = 0; k < n_reads; ++k) one_job(name, (uint64_t)k, ix, seg, tabs, reads, (uint64_t)k, (int)(rng() & 1), nullptr);
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s n_random seed [case file ..]\n", argv[0]); return 2; }
    const int n_random = atoi(argv[1]);
    uint64_t jobs = 0;
    for (int a = 3; a < argc; ++a) jobs += run_file(argv[a]);
    const int file_mismatches = mismatches;
    std::mt19937_64 rng((uint64_t)atoll(argv[2]));
    for (int i = 0; i < n_random; ++i) random_case(rng, i);
    printf("jobs=%lu mismatches=%d random=%d random_mismatches=%d found=%d max_matches=%u max_mems=%u global_jobs=%lu breaks_inside=%lu breaks_at_63=%lu breaks_later_step=%lu\n",
           (unsigned long)jobs, file_mismatches, n_random, mismatches - file_mismatches, found, max_matches, max_mems, (unsigned long)stats.global_jobs,
           (unsigned long)stats.breaks_inside, (unsigned long)stats.breaks_at_63, (unsigned long)stats.breaks_later_step);
    return mismatches ? 1 : 0;
}
