// check_ctg_consensus.cpp - TEST ONLY.  The consensus half of contig polishing on the CPU: the host form (necat_amd/csrc/ctg_consensus.h) and the CPU model of the
// device cores (necat_amd/csrc/ctg_dev_core.h: plan, tags lane by lane, run boundaries, range by range) against
//   * every case of the case files given (tests/ctg_cases.py has the format): cns, t_pos and - where the file has one - the polished segment, byte for byte, the
//     model at the default budget (a file of cases alone, n_reads = 0, takes the reads of the file before it) and at one small enough for at least 4 ranges; a case without expected output (cns_len 0 and no polished) only compares the two;
//   * each other on `n_random` seeded random cases: segment 500 - 5000 bases, 2 - 40 overlaps, random column strings.
// usage: check_ctg_consensus n_random seed [case file ..]      prints  cases= mismatches= random= random_mismatches= min_ranges= tags= stopped=
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../necat_amd/csrc/ctg_consensus.h"
#include "../../necat_amd/csrc/ctg_dev_core.h"

namespace hg = necat_host::ctg;
namespace gd = necat::ctg_dev;

struct Ovl { int32_t qid, qdir, qoff, qend, toff, tend, align_size, pad; uint64_t ops_off; };
static_assert(sizeof(Ovl) == 40, "the case file's overlap record");

static int mismatches = 0;
static uint32_t min_ranges = ~0u;
static uint64_t total_tags = 0, stopped = 0;

static void complain(const char* name, const char* what) { ++mismatches; fprintf(stderr, "MISMATCH %s: %s\n", name, what); }

// both forms on one segment; returns the host form's output
static hg::SegmentOut both(const char* name, const std::vector<hg::OverlapIn>& in, int size, const uint8_t* contig, std::string* polished, bool want_ranges)
{
    hg::SegmentOut h;
    hg::segment_consensus(in.data(), in.size(), size, hg::kMinCov, h);
    total_tags += h.n_tags;
    uint64_t cols = 0;
    std::vector<gd::ModelOverlap> mo;
    for (const hg::OverlapIn& o : in) { gd::ModelOverlap m = {o.ops, o.ncols, o.toff, o.words, o.read_begin, o.qsize, o.qoff, o.qdir}; mo.push_back(m); cols += (uint64_t)o.ncols; }
    if (cols > h.n_tags) ++stopped;
    auto raw = [&](int x) { return (unsigned)contig[x]; };
    if (polished) hg::splice(h.cns, h.t_pos, raw, size, hg::kMinRun, *polished);
    const uint64_t budgets[2] = {32ull << 20, std::max<uint64_t>(1, h.n_tags / 6)};
    for (int b = 0; b < 2; ++b) {
        hg::SegmentOut m;
        const uint32_t nr = gd::model_segment(mo.data(), mo.size(), (uint32_t)size, hg::kMinCov, budgets[b], m);
        if (b == 1 && want_ranges) min_ranges = std::min(min_ranges, nr);
        if (m.cns != h.cns || m.t_pos != h.t_pos) complain(name, b ? "device model (small budget) against host form" : "device model against host form");
        if (m.n_tags != h.n_tags || m.n_nodes != h.n_nodes || m.n_links != h.n_links) complain(name, "tag, node or link counts of the device model");
        if (polished) { std::string p; hg::splice(m.cns, m.t_pos, raw, size, hg::kMinRun, p); if (p != *polished) complain(name, "polished segment of the device model"); }
    }
    return h;
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

static std::vector<uint64_t> off, words;      // the reads of the last file that had some: a file of cases alone uses them

static int run_file(const char* path)
{
    const std::vector<uint8_t> raw = slurp(path);
    if (raw.size() < 32 || memcmp(raw.data(), "CTGCASE1", 8)) { fprintf(stderr, "%s is no case file\n", path); exit(2); }
    auto u64_at = [&](size_t at) { uint64_t v; memcpy(&v, raw.data() + at, 8); return v; };
    auto p8 = [](uint64_t n) { return (n + 7) & ~7ull; };
    const uint64_t nc = u64_at(8), nr = u64_at(16), nw = u64_at(24);
    size_t at = 32;
    if (nr) {
        off.assign(nr + 1, 0); words.assign(nw + 1, 0);
        memcpy(off.data(), raw.data() + at, 8 * (nr + 1));
        memcpy(words.data(), raw.data() + at + 8 * (nr + 1), 8 * nw);
    }
    at += 8 * (nr + 1) + 8 * nw;
    for (uint64_t c = 0; c < nc; ++c) {
        char name[33] = {0};
        memcpy(name, raw.data() + at, 32); at += 32;
        const uint64_t size = u64_at(at), n_ov = u64_at(at + 8), ob = u64_at(at + 16), cl = u64_at(at + 24), hp = u64_at(at + 32), pl = u64_at(at + 40);
        at += 48;
        std::vector<Ovl> ov(n_ov);
        if (n_ov) memcpy(ov.data(), raw.data() + at, 40 * n_ov);
        at += 40 * n_ov;
        std::vector<uint8_t> ops(raw.begin() + at, raw.begin() + at + ob); at += ob;
        ops.resize(ob + 8, 0);
        const uint8_t* contig = raw.data() + at; at += p8(size);
        const std::string cns((const char*)raw.data() + at, cl); at += p8(cl);
        std::vector<int32_t> t_pos(cl);
        if (cl) memcpy(t_pos.data(), raw.data() + at, 4 * cl);
        at += p8(4 * cl);
        const std::string pol((const char*)raw.data() + at, pl); at += p8(pl);
        std::vector<hg::OverlapIn> in;
        for (const Ovl& o : ov) {
            if (o.qid < 0 || (size_t)o.qid + 1 >= off.size()) { complain(name, "names no read"); continue; }
            const int qsize = (int)(off[o.qid + 1] - off[o.qid]);
            const char* why = hg::overlap_fault(ops.data() + o.ops_off, o.align_size, o.qoff, o.qend, o.toff, o.tend, qsize, (int64_t)size);
            if (why) { complain(name, why); continue; }
            hg::OverlapIn q = {ops.data() + o.ops_off, o.align_size, o.toff, words.data(), off[o.qid], qsize, o.qoff, o.qdir};
            in.push_back(q);
        }
        std::string polished;
        const hg::SegmentOut h = both(name, in, (int)size, contig, &polished, size >= 1500);
        const bool expect = cl || hp;
        if (expect && (h.cns != cns || h.t_pos != t_pos)) complain(name, "host form against the reference's cns / t_pos");
        if (hp && polished != pol) complain(name, "host form against the reference's polished segment");
    }
    if (at != raw.size()) { fprintf(stderr, "%s: %zu bytes read of %zu\n", path, at, raw.size()); exit(2); }
    return (int)nc;
}

static void random_case(std::mt19937_64& rng, int id)
{
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int size = rnd(500, 5000), n_ov = rnd(2, 40);
    std::vector<uint8_t> contig((size_t)size);
    for (auto& b : contig) b = (uint8_t)(rng() & 3);
    std::vector<std::vector<uint8_t>> ops((size_t)n_ov);
    std::vector<uint64_t> words;
    std::vector<hg::OverlapIn> in;
    std::vector<uint64_t> begin((size_t)n_ov);
    std::vector<int> qlen((size_t)n_ov), toffs((size_t)n_ov), qoffs((size_t)n_ov), ncols((size_t)n_ov);
    uint64_t nb = 0;
    const int style = id % 4;          // 0: mostly matches, 1: uniform ops, 2: insertion-rich, 3: deletion-rich with long runs
    for (int k = 0; k < n_ov; ++k) {
        const int toff = rnd(0, size - 1), span = rnd(1, size - toff);
        std::vector<uint8_t> col;
        int nt = 0, nq = 0;
        if (toff == 0 || rng() % 3) { col.push_back((uint8_t)(rng() % 2 ? 0 : 2)); ++nt; nq += col[0] != 2; }        // (a query base in front of position 0 is no valid input)
        while (nt < span) {
            const unsigned u = (unsigned)(rng() % 100);
            int op;
            if (style == 0) op = u < 85 ? 0 : u < 90 ? 3 : u < 95 ? 1 : 2;
            else if (style == 1) op = (int)(u & 3);
            else if (style == 2) op = u < 50 ? 1 : u < 90 ? 0 : u < 95 ? 3 : 2;
            else op = u < 40 ? 2 : u < 80 ? 0 : u < 90 ? 3 : 1;
            int run = (style == 3 && u % 7 == 0) ? rnd(1, 90) : 1;
            for (; run > 0 && nt < span; --run) { col.push_back((uint8_t)op); nt += op != 1; nq += op != 2; }
        }
        const int lo = rnd(0, 20), hi = rnd(0, 20);
        begin[(size_t)k] = nb; qlen[(size_t)k] = lo + nq + hi; toffs[(size_t)k] = toff; qoffs[(size_t)k] = lo; ncols[(size_t)k] = (int)col.size();
        nb += (uint64_t)qlen[(size_t)k];
        ops[(size_t)k].assign((col.size() + 3) / 4 + 8, 0);
        for (size_t i = 0; i < col.size(); ++i) ops[(size_t)k][i >> 2] |= (uint8_t)(col[i] << ((i & 3) * 2));
    }
    words.assign(nb / 32 + 2, 0);
    for (auto& w : words) w = rng();
    for (int k = 0; k < n_ov; ++k) {
        hg::OverlapIn q = {ops[(size_t)k].data(), ncols[(size_t)k], toffs[(size_t)k], words.data(), begin[(size_t)k], qlen[(size_t)k], qoffs[(size_t)k], (int)(rng() & 1)};
        in.push_back(q);
    }
    char name[32];
    snprintf(name, sizeof name, "random %d", id);
    std::string polished;
    both(name, in, size, contig.data(), &polished, false);
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s n_random seed [case file ..]\n", argv[0]); return 2; }
    const int n_random = atoi(argv[1]);
    int cases = 0;
    for (int a = 3; a < argc; ++a) cases += run_file(argv[a]);
    const int file_mismatches = mismatches;
    std::mt19937_64 rng((uint64_t)atoll(argv[2]));
    for (int i = 0; i < n_random; ++i) random_case(rng, i);
    printf("cases=%d mismatches=%d random=%d random_mismatches=%d min_ranges=%u tags=%lu stopped=%lu\n", cases, file_mismatches, n_random, mismatches - file_mismatches,
           min_ranges == ~0u ? 0u : min_ranges, (unsigned long)total_tags, (unsigned long)stopped);
    return mismatches ? 1 : 0;
}
