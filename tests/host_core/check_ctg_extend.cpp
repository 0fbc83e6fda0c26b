// check_ctg_extend.cpp - TEST ONLY.  The serial pass of contig polishing's loop (necat_amd/csrc/ctg_extend.h: ctg_ext::replay and its pieces) on g++ alone, fed
// with the reference's own per-record aligner results (tests/ctg_ext_cases.py: checker_input writes them from tests/golden/ctg_x): the verdict of every record, the
// order of the overlaps and the count of records that reached cns_extension must be the reference's, number for number.  Then the pieces at their edges.
//   usage: check_ctg_extend FILE...      each FILE: "n_segments cap", per segment "from size n n_used n_overlaps", n lines
//                                         "soff send rl found ok qoff qend toff tend ident(hex float) state", one line with the overlaps' record indices
// prints "segments=.. records=.. mismatches=.. accepted=.. capped=.. unit_failures=.."; exit status 1 on any mismatch
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../necat_amd/csrc/ctg_extend.h"

namespace cx = necat_host::ctg_ext;

struct Rec { long soff, send; int rl, state; cx::Aligned a; };

static int unit_checks()
{
    int bad = 0;
    int32_t sb, se;
    // step 1: a record from before the segment, to behind it, ending at its start
    bad += !(cx::record_range(100, 5000, 1000, 3000, &sb, &se) && sb == 0 && se == 3000);
    bad += !(cx::record_range(1200, 1500, 1000, 3000, &sb, &se) && sb == 200 && se == 500);
    bad += cx::record_range(100, 1000, 1000, 3000, &sb, &se);
    bad += !(cx::record_range(100, 1001, 1000, 3000, &sb, &se) && sb == 0 && se == 1);
    bad += !(cx::record_range((1L << 40) + 5, (1L << 40) + 9, 1L << 40, 3000, &sb, &se) && sb == 5 && se == 9);
    bad += !(cx::record_range(9000, 9500, 1000, 3000, &sb, &se) && sb >= se);          // behind the segment: an empty range
    // step 2: 199 / 200 open positions, an empty range
    std::vector<uint8_t> cov(1000, 10);
    for (int i = 0; i < 199; ++i) cov[(size_t)(3 * i)] = 9;
    bad += !cx::is_full(cov.data(), 0, 1000);
    cov[999] = 0;
    bad += cx::is_full(cov.data(), 0, 1000);
    bad += !cx::is_full(cov.data(), 500, 500);
    // step 5: the identity bound, the ratio in double, the second alternative never true
    cx::Aligned a = {1, 1, 0, 3000, 0, 3000, 90.0};
    bad += !cx::accepted(a, 5000, 20000);
    a.ident_perc = 89.99999999;
    bad += cx::accepted(a, 5000, 20000);
    a.ident_perc = 95.0; a.qend = 2999;
    bad += cx::accepted(a, 5000, 20000);
    a.qend = 3001;
    bad += cx::accepted(a, 5002, 20000);          // 3001 < 3001.2: the product is a double, not an int
    bad += !cx::accepted(a, 5001, 20000);         // 3001 >= 3000.6
    bad += !cx::accepted(a, 5000, 20000);
    cx::Aligned w = {1, 1, 3500, 12500, 0, 9000, 95.0};
    bad += cx::accepted(w, 16000, 9000);          // the whole segment, 9000 of 16 000 read bases: rejected
    // step 6: the counters run over the alignment's own range, whatever the record's; they are u8 and wrap as the reference's do
    {
        cx::Aligned one = {1, 1, 0, 2000, 0, 1000, 99.0};          // every alignment covers [0, 1000)
        auto table = [&](uint64_t) -> const cx::Aligned& { return one; };
        auto rl = [](uint64_t) { return 2000; };
        cx::Pass p;
        // records on [0, 1000): ten are accepted, then the range is full
        cx::replay(2000, 300, true, [](uint64_t, int32_t* b, int32_t* e) { *b = 0; *e = 1000; }, rl, table, &p);
        bad += !(p.order.size() == 10 && p.n_used == 10 && p.state[9] == cx::kAccepted && p.state[10] == cx::kCapped && p.state[299] == cx::kCapped);
        // no cap: all of them
        cx::replay(2000, 300, false, [](uint64_t, int32_t* b, int32_t* e) { *b = 0; *e = 1000; }, rl, table, &p);
        bad += !(p.order.size() == 300 && p.n_used == 300);
        // records on [0, 2000) keep finding [1000, 2000) open and keep counting on [0, 1000): after 255 of them a record on [0, 1000) is capped (record 255), after
        // 261 the counters there stand at 5 again and such a record is let in (record 262)
        auto range = [](uint64_t k, int32_t* b, int32_t* e) { *b = 0; *e = (k == 255 || k == 262) ? 1000 : 2000; };
        cx::replay(2000, 263, true, range, rl, table, &p);
        bad += !(p.state[254] == cx::kAccepted && p.state[255] == cx::kCapped && p.state[261] == cx::kAccepted && p.state[262] == cx::kAccepted && p.order.size() == 262);
    }
    return bad;
}

int main(int argc, char** argv)
{
    unsigned long segments = 0, records = 0, mismatches = 0, n_acc = 0, n_cap = 0;
    for (int f = 1; f < argc; ++f) {
        FILE* in = fopen(argv[f], "r");
        if (!in) { fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
        int ns, cap;
        if (fscanf(in, "%d %d", &ns, &cap) != 2) return 2;
        for (int s = 0; s < ns; ++s) {
            long from; int size, n; unsigned long n_used, n_ov;
            if (fscanf(in, "%ld %d %d %lu %lu", &from, &size, &n, &n_used, &n_ov) != 5) return 2;
            std::vector<Rec> r((size_t)n);
            for (auto& x : r) {
                char ident[64];
                if (fscanf(in, "%ld %ld %d %d %d %d %d %d %d %63s %d", &x.soff, &x.send, &x.rl, &x.a.found, &x.a.ok, &x.a.qoff, &x.a.qend, &x.a.toff, &x.a.tend, ident, &x.state) != 11) return 2;
                x.a.ident_perc = strtod(ident, nullptr);
            }
            std::vector<unsigned long> order(n_ov);
            for (auto& k : order) if (fscanf(in, "%lu", &k) != 1) return 2;
            cx::Pass p;
            bool bad_range = false;
            cx::replay(size, (uint64_t)n, cap != 0,
                       [&](uint64_t k, int32_t* sb, int32_t* se) { if (!cx::record_range(r[k].soff, r[k].send, from, size, sb, se)) bad_range = true; },
                       [&](uint64_t k) { return r[k].rl; }, [&](uint64_t k) -> const cx::Aligned& { return r[k].a; }, &p);
            ++segments; records += (unsigned long)n;
            if (bad_range) { ++mismatches; fprintf(stderr, "%s segment %d: a record ends before the segment\n", argv[f], s); }
            for (int k = 0; k < n; ++k) {
                if (p.state[(size_t)k] != r[(size_t)k].state) { ++mismatches; fprintf(stderr, "%s segment %d record %d: state %d, the reference's %d\n", argv[f], s, k, p.state[(size_t)k], r[(size_t)k].state); }
                n_acc += p.state[(size_t)k] == cx::kAccepted; n_cap += p.state[(size_t)k] == cx::kCapped;
            }
            if (p.n_used != n_used) { ++mismatches; fprintf(stderr, "%s segment %d: n_used %lu, the reference's %lu\n", argv[f], s, (unsigned long)p.n_used, n_used); }
            if (p.order.size() != order.size()) { ++mismatches; fprintf(stderr, "%s segment %d: %zu overlaps, the reference's %zu\n", argv[f], s, p.order.size(), order.size()); }
            else for (size_t i = 0; i < order.size(); ++i) if (p.order[i] != order[i]) { ++mismatches; fprintf(stderr, "%s segment %d: overlap %zu is record %lu, the reference's %lu\n", argv[f], s, i, (unsigned long)p.order[i], order[i]); break; }
        }
        fclose(in);
    }
    const int unit = unit_checks();
    printf("segments=%lu records=%lu mismatches=%lu accepted=%lu capped=%lu unit_failures=%d\n", segments, records, mismatches, n_acc, n_cap, unit);
    return mismatches || unit ? 1 : 0;
}
