// check_pair_jobs.cpp - the rescue pair's formulation (necat_amd/csrc/rescue_pair.h) on the contig stage's shape: the subject is a slice STRICTLY INSIDE a sequence.
// A read and a subject of different random bases lie in one word buffer between neighbours of other random bases; over slice starts at every residue mod 32, from = 0,
// from + len = the subject's size and both strands it checks that
//   * dal::seq_at over the built task gives exactly BaseWords' decode of the stretch inside [0, len) and 4 at -1 and at len (the read likewise, on its strand),
//   * (mida +- k0) / 2 are the anchor's two coordinates relative to the slice,
//   * a range on the slice as the global half's job names the same bases of the sequence, and an accepted result comes back to the slice's coordinates,
//   * the tips of a host result decode to that result, with the min_align_size rule and ident_perc.
// The positions the functions are given address the checker's own buffer: the volume's words behind kGuard words of other bits (as check_rm_spec.cpp moves them).
//   check_pair_jobs [first_base]        first_base (a number, "straddle" or "top": high_base.h): the volume's bases begin there in a buffer that really is that large
// Last line of stdout: jobs= residues= from0= to_end= inside= (behind first_base= last_base= when one was given).  Exit status 1 on any difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../necat_amd/csrc/host_bases.h"
#include "../../necat_amd/csrc/rescue_pair.h"
#include "high_base.h"

using namespace necat;

namespace {

constexpr int kGuard = 4;

[[noreturn]] void die(const char* what, i64 from, i64 len, int qdir)
{
    fprintf(stderr, "check_pair_jobs: %s (slice [%ld, %ld), strand %d)\n", what, (long)from, (long)(from + len), qdir);
    exit(1);
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937_64 rng(7);
    // neighbour, read, neighbour, subject, neighbour: no sequence begins on a word boundary, every one has other bases on both sides
    const u64 sizes[5] = {37, 301, 5, 413, 29};
    std::vector<u64> off(1, 0);
    for (u64 s : sizes) off.push_back(off.back() + s);
    std::vector<u64> vol((off.back() + 31) / 32, 0);
    for (u64 g = 0; g < off.back(); ++g) vol[g >> 5] |= (u64)(rng() & 3) << ((g & 31) * 2);
    const u64 first = high_base::first_base(argc > 1 ? argv[1] : nullptr, off.back() + 32 * kGuard);          // (the guard words in front count as bases of the layout)
    const i64 kShift = 32 * kGuard + (i64)first;          // what a position of the volume gains in the buffer
    const u64 data_words = ((u64)kShift + off.back() + 31) / 32;
    std::vector<u64> buf((size_t)data_words + kGuard, 0);
    for (int w = 0; w < kGuard; ++w) { buf[(size_t)w] = 0x5a5a5a5a5a5a5a5aULL; buf[(size_t)data_words + w] = 0xa5a5a5a5a5a5a5a5ULL; }
    for (u64 g = 0; g < off.back(); ++g) buf[(size_t)((g + (u64)kShift) >> 5)] |= ((vol[g >> 5] >> ((g & 31) * 2)) & 3) << (((g + (u64)kShift) & 31) * 2);
    necat_host::BaseWords hb; hb.w = vol.data(); hb.seq_off = off.data();
    const int qid = 1, sid = 3;
    const i64 qb = (i64)off[qid], qs = (i64)sizes[qid], sb = (i64)off[sid], ss = (i64)sizes[sid];
    const u64* bases = buf.data();

    std::set<int> residues;
    uint64_t jobs = 0, from0 = 0, to_end = 0, inside = 0;
    std::vector<u8> want, qwant;
    for (int qdir = 0; qdir < 2; ++qdir) {
        hb.strand(qid, qdir, qwant);
        for (i64 from = 0; from <= 40; ++from) {
            for (i64 len : {ss - from, (i64)97, (i64)1}) {          // to the subject's end; strictly inside (but for from = 0); one base
                if (from + len > ss) die("the test's own slice leaves the subject", from, len, qdir);
                const i64 qoff = 11 + from % 7, soff = len / 3;
                const pair::Job J{qid, qdir, sid, qb + kShift, qs, sb + kShift, from, len, qoff, soff};
                const dal::Task T = pair::task_of(J);
                ++jobs; residues.insert((int)((sb + from) & 31));
                if (from == 0) ++from0;
                if (from + len == ss) ++to_end;
                if (from > 0 && from + len < ss) ++inside;
                // ---- the slices the wave reads
                if (T.b.len != len || T.a.len != qs) die("a length", from, len, qdir);
                want.resize((size_t)len); hb.decode(sid, 0, from, from + len, want.data());
                dal::WordCache wc; wc.w = LLONG_MIN; wc.v = 0;
                for (i64 i = -1; i <= len; ++i)
                    if (dal::seq_at(bases, T.b, (int)i, wc) != (i < 0 || i >= len ? 4 : want[(size_t)i])) die("the subject slice's bases", from, len, qdir);
                wc.w = LLONG_MIN;
                for (i64 i = qs; i >= -1; --i)
                    if (dal::seq_at(bases, T.a, (int)i, wc) != (i < 0 || i >= qs ? 4 : qwant[(size_t)i])) die("the read's bases", from, len, qdir);
                // ---- the anchor
                if ((T.mida + T.k0) / 2 != qoff || (T.mida - T.k0) / 2 != soff || ((T.mida + T.k0) & 1)) die("the anchor", from, len, qdir);
                // ---- tips of a result decode to it
                rescue::DalignResult d;
                d.abpos = 3; d.aepos = (int)qs - 2; d.bbpos = (int)(len / 5); d.bepos = (int)len; d.diffs = 9;
                dal::Out f, b;
                pair::tips_of(d, &f, &b);
                if (f.flag | b.flag) die("a flag on a host result's tips", from, len, qdir);
                const int asize = d.aepos - d.abpos, bsize = d.bepos - d.bbpos;
                const int edge = asize < bsize ? asize : bsize;
                for (int min_size : {edge, edge + 1}) {          // the shorter range just long enough, and one base short
                    necat_dalign_result r;
                    memset(&r, 0, sizeof r);
                    pair::decode(f, b, min_size, &r);
                    if (r.qoff != d.abpos || r.qend != d.aepos || r.soff != d.bbpos || r.send != d.bepos || r.diffs != d.diffs) die("tips -> range", from, len, qdir);
                    if (r.ok != (min_size == edge) ||r.ident_perc != (r.ok ? 100.0 - 200.0 * d.diffs / (asize + bsize) : 0.0)) die("the accept rule", from, len, qdir);
                    // ---- the range as the global half's job: the same bases, on the sequence
                    const necat_nw_job j = pair::nw_job(qid, qdir, sid, from, r);
                    if (j.qid != qid || j.qdir != qdir || j.sid != sid || j.qfrom != r.qoff || j.qto != r.qend || j.sfrom != from + r.soff || j.sto != from + r.send ||
                        j.tolerance != r.diffs || j.sfrom < 0 || j.sto > ss) die("range -> job", from, len, qdir);
                    const nw::Seq q = pair::strand_seq(qb + kShift, qs, qdir, j.qfrom), t = pair::strand_seq(sb + kShift, ss, 0, j.sfrom);
                    for (int i = 0; i < j.qto - j.qfrom; ++i)
                        if (dal::seq_at(bases, dal::DSeq{q, j.qto - j.qfrom}, i, wc) != qwant[(size_t)(r.qoff + i)]) die("the job's query range", from, len, qdir);
                    for (int i = 0; i < j.sto - j.sfrom; ++i)
                        if (dal::seq_at(bases, dal::DSeq{t, j.sto - j.sfrom}, i, wc) != want[(size_t)(r.soff + i)]) die("the job's subject range", from, len, qdir);
                    // ---- and a result inside the job's ranges back on the slice
                    necat_nw_result nr;
                    memset(&nr, 0, sizeof nr);
                    const int cut = bsize > 2 ? 1 : 0;
                    nr.ok = 1; nr.qoff = j.qfrom + 2; nr.qend = j.qto - 1; nr.toff = j.sfrom + cut; nr.tend = j.sto - cut;
                    pair::to_slice(from, &nr);
                    if (nr.qoff != r.qoff + 2 || nr.qend != r.qend - 1 || nr.toff != r.soff + cut || nr.tend != r.send - cut) die("result -> slice", from, len, qdir);
                }
            }
        }
    }
    if (argc > 1) printf("first_base=%llu last_base=%llu ", (unsigned long long)kShift, (unsigned long long)(kShift + (i64)off.back() - 1));
    printf("jobs=%lu residues=%zu from0=%lu to_end=%lu inside=%lu\n", (unsigned long)jobs, residues.size(), (unsigned long)from0, (unsigned long)to_end, (unsigned long)inside);
    return residues.size() == 32 && from0 && to_end && inside ? 0 : 1;
}
