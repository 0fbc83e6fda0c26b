// check_trim.cpp - TEST ONLY.  The read trimming stage's two per-read deciders on the partition files of oc2pm4, on a machine without a GPU:
//   * necat_amd/csrc/trim_core.h, the host restatement of the reference's lcr_worker, on every read's records in the order oc2lcr holds them
//     (partition file, klib's introsort by subject id), with its classification of the reads the device hands back;
//   * the SOURCE of the device's per-read core (necat_amd/csrc/trim_kernels.h: trim_read_core) compiled with g++ behind the stand-ins for the
//     HIP built-ins (a phase runs lane 0 .. 63 one after the other), on the same records in a SHUFFLED order - the device's answer may not
//     depend on the order.
//
//   check_trim <m4 path> <num_reads> <error_cutoff> <min_ovlp_size> <min_cov> <min_size> [seed]
//
// One line per read id 1 .. num_reads on stdout:  id left right size how reason | left right size how  (host, then kernel core; final pass done).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>
#include <vector>

#define __launch_bounds__(...)
#include "../../necat_amd/csrc/trim_kernels.h"
#include "../../necat_amd/csrc/trim_io.h"

using namespace necat_host::trim;

int main(int argc, char** argv)
{
    if (argc < 7) { fprintf(stderr, "usage: check_trim m4 num_reads error_cutoff min_ovlp_size min_cov min_size [seed]\n"); return 2; }
    const char* m4_path = argv[1];
    const int num_reads = atoi(argv[2]);
    const double min_ident_perc = 100.0 - 100.0 * atof(argv[3]);
    const int min_ovlp_size = atoi(argv[4]), min_cov = atoi(argv[5]), min_size = atoi(argv[6]);
    std::mt19937_64 rng(argc > 7 ? (uint64_t)atoll(argv[7]) : 1);
    int np = 0;
    if (!load_num_partitions(m4_path, &np)) return 2;
    const int nids = num_reads + 2;
    std::vector<Clip> host((size_t)nids, Clip{0, 0, 0, kNone}), dev((size_t)nids, Clip{-1, 0, 0, kNone});
    std::vector<int> reason((size_t)nids, 0);
    auto sh = std::make_unique<necat::TrimLds>();
    for (int p = 0; p < np; ++p) {
        std::vector<M4> recs;
        std::vector<size_t> run_off;
        if (!load_records(partition_name(m4_path, p).c_str(), recs)) return 2;
        if (recs.empty()) continue;
        group_partition(recs, run_off);
        for (size_t r = 0; r + 1 < run_off.size(); ++r) {
            M4* m4v = recs.data() + run_off[r];
            const int n = (int)(run_off[r + 1] - run_off[r]), sid = m4v[0].sid;
            if (sid < 0 || sid >= nids) { fprintf(stderr, "read id %d out of range\n", sid); return 2; }
            reason[(size_t)sid] = classify(m4v, n, min_ident_perc);
            // the kernel's core, as k_trim_ranges calls it, on a shuffled copy
            std::vector<M4> sh_recs(m4v, m4v + n);
            std::shuffle(sh_recs.begin(), sh_recs.end(), rng);
            necat_clip_range out{0, 0, 0, 0};
            necat::trim_read_core(*sh, (const necat_m4*)sh_recs.data(), n > necat::kTrimCap ? necat::kTrimCap + 1 : n, min_ident_perc, min_ovlp_size, min_cov, min_size, &out);
            dev[(size_t)sid] = Clip{out.left, out.right, out.size, out.how};
            // the reference's decision, in the reference's order (permutes m4v)
            Clip c{0, 0, 0, kNone};
            bool tie = false;
            if (decide_read(m4v, n, min_ident_perc, min_ovlp_size, min_cov, &c, &tie) != kNone) host[(size_t)sid] = c;
            else host[(size_t)sid].how = kNone;
        }
    }
    for (int i = 1; i <= num_reads; ++i) {
        finish_clip(host[(size_t)i], min_size);
        printf("%d %d %d %d %d %d | %d %d %d %d\n", i, host[(size_t)i].left, host[(size_t)i].right, host[(size_t)i].size, host[(size_t)i].how, reason[(size_t)i],
               dev[(size_t)i].left, dev[(size_t)i].right, dev[(size_t)i].size, dev[(size_t)i].how);
    }
    return 0;
}
