// trim_kernels.h - the device side of the read trimming stage (oc2pm4 + oc2lcr; reference: trim_bases/pm4_aux.c:129-196, largest_cover_range.c:290-325).
//
//   k_trim_part<MODE>   pm4_thread_func's transformation on 96-byte records + a counting sort by subject id (histogram / scan on the host of the
//                       stage / scatter): a record that passes the identity cutoff is kept under its subject as it is and, with the roles exchanged
//                       and the new subject put on the forward strand (fix_asm_m4_offsets), under its query.
//   k_trim_ranges       one WAVE64 (= one workgroup of 64 threads) per read.  The read's records (at most kTrimCap = 300, truncate_m4_list's bound)
//                       sit in LDS as columns of ints; the wave decides complete (a ballot), chimeric (a rank sort by (qid, qdir, -vscore), one
//                       lane per group head, the pairs' verdicts reduced by an ordered 64-bit maximum) or the largest covered range (three rank
//                       sorts - interval starts, interval ends, intervals by (lo, hi) - and then the sweeps of trim_sweep.h, which are serial by
//                       nature and run on lane 0 over LDS).  Why a wave and not a workgroup of several: a list has 300 records at most, the
//                       rank sorts are 300 x 300 / 64 broadcast reads per lane, and the serial sweeps (<= 600 events) set the time of a read -
//                       more waves per read would only wait for lane 0.  Integer and double arithmetic only, trim_sweep.h's code on both sides:
//                       the ranges are EQUAL to the host's.
//
// The per-read core (trim_read_core) is a header function in PHASES: TRIM_EACH_LANE(lane) { .. } runs its body once per lane - on the device as the
// lane's own code, under g++ (tests/host_core/check_trim.cpp) as a loop over the 64 lanes - and TRIM_SYNC() separates the phases.  Values that cross
// a phase live in the LDS block; the votes go through trim_vote / trim_add / trim_max64 (ballot + LDS atomics on the device, plain updates on the CPU).
#pragma once
#include "dev_common.h"
#include "trim_sweep.h"
#include "../../include/necat_hip.h"

namespace necat {

using necat_trim::Range;
constexpr int kTrimCap = necat_trim::kMaxRecs;

#if defined(__HIP_DEVICE_COMPILE__)
#define TRIM_EACH_LANE(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define TRIM_SYNC() __syncthreads()
NECAT_D void trim_vote(int* flag, bool pred)        // every lane of the wave calls it; the first lane that holds the predicate records it
{
    const unsigned long long b = __ballot(pred);
    if (b != 0ULL && (int)threadIdx.x == __ffsll(b) - 1) *flag = 1;
}
NECAT_D void trim_add(int* acc, int v) { atomicAdd(acc, v); }
NECAT_D void trim_max64(unsigned long long* acc, unsigned long long v) { atomicMax(acc, v); }
#else
#define TRIM_EACH_LANE(lane) for (int lane = 0; lane < 64; ++lane)
#define TRIM_SYNC() do { } while (0)
inline void trim_vote(int* flag, bool pred) { if (pred) *flag = 1; }
inline void trim_add(int* acc, int v) { *acc += v; }
inline void trim_max64(unsigned long long* acc, unsigned long long v) { if (v > *acc) *acc = v; }
#endif

// the LDS block of one read: 41.0 KB, so three reads are in flight per CU (160 KB) - the stage is bound by lane 0's sweeps, not by occupancy
struct TrimLds {
    int qid[kTrimCap], qdir[kTrimCap], vscore[kTrimCap], qoff[kTrimCap], qend[kTrimCap], qsize[kTrimCap], soff[kTrimCap], send[kTrimCap];
    int perm[kTrimCap];                          // record at position p of the chimera order
    int opens[kTrimCap], closes[kTrimCap];       // interval starts / ends, ascending
    Range il[kTrimCap];                          // the intervals by (lo, hi)
    Range de[2 * kTrimCap], id[2 * kTrimCap], fi[3 * kTrimCap];
    unsigned long long best;                     // (size << 32 | ~order) of the best chimeric overlap
    int low, complete, tie, nchim;
};

NECAT_HD bool trim_chimera_less(const TrimLds& sh, int a, int b)        // m4_record_chimeric_cmp, ties by slot: a total order
{
    if (sh.qid[a] != sh.qid[b]) return sh.qid[a] < sh.qid[b];
    if (sh.qdir[a] != sh.qdir[b]) return sh.qdir[a] < sh.qdir[b];
    if (sh.vscore[a] != sh.vscore[b]) return sh.vscore[a] > sh.vscore[b];
    return a < b;
}

// One read: recs[0 .. n) are its records in ANY order (all with the same sid and ssize).  Every lane of the wave calls it; lane 0 writes *out.
// how == host: the read is one of those whose answer depends on the order the reference held equal keys in, or has more than kTrimCap records
// (trim_core.h: classify) - left = -1, right = size = 0, the caller decides it with trim_core.h.
NECAT_HD void trim_read_core(TrimLds& sh, const necat_m4* __restrict__ recs, int n, double min_ident_perc, int min_ovlp_size, int min_cov, int min_size,
                             necat_clip_range* __restrict__ out)
{
    using namespace necat_trim;
    if (n <= 0 || n > kTrimCap) {
        TRIM_EACH_LANE(lane) if (lane == 0) { out->left = -1; out->right = 0; out->size = 0; out->how = n <= 0 ? kNone : kHost; }
        return;
    }
    const int ssize = (int)recs[0].ssize;
    TRIM_EACH_LANE(lane) if (lane == 0) { sh.low = 0; sh.complete = 0; sh.tie = 0; sh.nchim = 0; sh.best = 0; }
    TRIM_SYNC();
    // ---- the records into LDS; remove_low_quality_m4's test and is_complete_read's as votes
    TRIM_EACH_LANE(lane) {
        bool low = false, complete = false;
        for (int i = lane; i < n; i += 64) {
            const necat_m4 m = recs[i];
            sh.qid[i] = m.qid; sh.qdir[i] = m.qdir; sh.vscore[i] = m.vscore;
            sh.qoff[i] = (int)m.qoff; sh.qend[i] = (int)m.qend; sh.qsize[i] = (int)m.qsize;
            sh.soff[i] = (int)m.soff; sh.send[i] = (int)m.send;
            low |= m.ident_perc < min_ident_perc;
            complete |= range_is_complete((int)m.soff, (int)m.send, ssize);
        }
        trim_vote(&sh.low, low);
        trim_vote(&sh.complete, complete);
    }
    TRIM_SYNC();
    if (sh.low || sh.complete) {
        TRIM_EACH_LANE(lane) if (lane == 0) {
            if (sh.low) { out->left = -1; out->right = 0; out->size = 0; out->how = kHost; }
            else { int left = 0; final_pass(left, ssize, ssize, min_size); out->left = left; out->right = ssize; out->size = ssize; out->how = kComplete; }
        }
        return;
    }
    // ---- is_chimeric_read: the order of m4_record_chimeric_cmp by rank (every lane reads the same slot at the same time: LDS broadcasts)
    TRIM_EACH_LANE(lane) {
        for (int i = lane; i < n; i += 64) {
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += trim_chimera_less(sh, j, i) ? 1 : 0;
            sh.perm[rank] = i;
        }
    }
    TRIM_SYNC();
    // one lane per head of a qid group: the group's first record i, the first record k of its second strand, their verdict
    TRIM_EACH_LANE(lane) {
        bool tie = false;
        for (int p = lane; p < n; p += 64) {
            const int i = sh.perm[p];
            if (p > 0 && sh.qid[sh.perm[p - 1]] == sh.qid[i]) continue;
            int pk = p + 1;
            while (pk < n && sh.qid[sh.perm[pk]] == sh.qid[i] && sh.qdir[sh.perm[pk]] == sh.qdir[i]) ++pk;
            if (pk >= n || sh.qid[sh.perm[pk]] != sh.qid[i]) continue;          // one strand only
            const int k = sh.perm[pk];
            if (p + 1 < pk && sh.vscore[sh.perm[p + 1]] == sh.vscore[i]) tie = true;
            if (pk + 1 < n) { const int k2 = sh.perm[pk + 1]; if (sh.qid[k2] == sh.qid[k] && sh.qdir[k2] == sh.qdir[k] && sh.vscore[k2] == sh.vscore[k]) tie = true; }
            if (!chimera_pair(sh.qoff[i], sh.qend[i], sh.qoff[k], sh.qend[k], sh.soff[i], sh.send[i], sh.soff[k], sh.send[k], sh.qsize[i], ssize)) continue;
            trim_add(&sh.nchim, 1);
            // "first strictly larger in group order, i before k" = the largest size, and among equals the smallest order
            const int si = sh.send[i] - sh.soff[i], sk = sh.send[k] - sh.soff[k];
            if (si > 0) trim_max64(&sh.best, (unsigned long long)(u32)si << 32 | (u32)(0xffffffffu - (u32)(2 * p)));
            if (sk > 0) trim_max64(&sh.best, (unsigned long long)(u32)sk << 32 | (u32)(0xffffffffu - (u32)(2 * p + 1)));
        }
        trim_vote(&sh.tie, tie);
    }
    TRIM_SYNC();
    if (sh.tie || (sh.best != 0 && sh.nchim > 1)) {
        TRIM_EACH_LANE(lane) if (lane == 0) {
            if (sh.tie) { out->left = -1; out->right = 0; out->size = 0; out->how = kHost; }
            else {
                const u32 ord = 0xffffffffu - (u32)(sh.best & 0xffffffffu);
                const int p = (int)(ord >> 1);
                int at = sh.perm[p];
                if (ord & 1u) {
                    int pk = p + 1;
                    while (sh.qdir[sh.perm[pk]] == sh.qdir[at]) ++pk;           // the group has a second strand: the pair was evaluated
                    at = sh.perm[pk];
                }
                int left = sh.soff[at];
                const int right = sh.send[at];
                final_pass(left, right, ssize, min_size);
                out->left = left; out->right = right; out->size = ssize; out->how = kChimeric;
            }
        }
        return;
    }
    // ---- largest_cover_range: the three sorted arrays by rank ..
    TRIM_EACH_LANE(lane) {
        for (int i = lane; i < n; i += 64) {
            const int lo = sh.soff[i], hi = sh.send[i];
            int ro = 0, rc = 0, rr = 0;
            for (int j = 0; j < n; ++j) {
                const int lj = sh.soff[j], hj = sh.send[j];
                ro += (lj < lo || (lj == lo && j < i)) ? 1 : 0;
                rc += (hj < hi || (hj == hi && j < i)) ? 1 : 0;
                rr += (lj < lo || (lj == lo && (hj < hi || (hj == hi && j < i)))) ? 1 : 0;
            }
            sh.opens[ro] = lo; sh.closes[rc] = hi;
            sh.il[rr].lo = lo; sh.il[rr].hi = hi; sh.il[rr].ct = 1;
        }
    }
    TRIM_SYNC();
    // .. and the sweeps, serial as the reference's
    TRIM_EACH_LANE(lane) if (lane == 0) {
        int left = 0, right = 0;
        if (cover_range(sh.opens, sh.closes, sh.il, n, min_ovlp_size, min_cov, sh.de, sh.id, sh.fi, &left, &right)) {
            final_pass(left, right, ssize, min_size);
            out->left = left; out->right = right; out->size = ssize; out->how = kCover;
        } else { out->left = -1; out->right = 0; out->size = 0; out->how = kNone; }
    }
}

#if defined(__HIPCC__)
// pm4_aux.c:103-127 with query_is_target: the record seen from its query, the new subject on the forward strand
NECAT_D necat_m4 trim_exchanged(const necat_m4& c)
{
    necat_m4 r = c;
    r.qid = c.sid; r.qdir = c.sdir; r.qoff = c.soff; r.qend = c.send; r.qext = c.sext; r.qsize = c.ssize;
    r.sid = c.qid; r.sdir = c.qdir; r.soff = c.qoff; r.send = c.qend; r.sext = c.qext; r.ssize = c.qsize;
    if (r.sdir == 1) { r.sdir = 0; r.qdir = 1 - r.qdir; }
    return r;
}

// MODE 0: records per read id into cursor[].  MODE 1: scatter; cursor[id] runs from the read's start.  Ids outside [0, nids) go nowhere, as ids
// outside the open partitions go nowhere in the reference.  The order inside a read is free (atomics) - the ranges do not depend on it.
template <int MODE>
__global__ void __launch_bounds__(256)
k_trim_part(const necat_m4* __restrict__ recs, u64 n, int nids, double min_ident_perc, unsigned long long* __restrict__ cursor, necat_m4* __restrict__ out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const necat_m4 c = recs[i];
    if (c.ident_perc < min_ident_perc) return;
    if (c.sid >= 0 && c.sid < nids) {
        const unsigned long long at = atomicAdd(&cursor[c.sid], 1ULL);
        if (MODE == 1) out[at] = c;
    }
    if (c.qid >= 0 && c.qid < nids) {
        const unsigned long long at = atomicAdd(&cursor[c.qid], 1ULL);
        if (MODE == 1) out[at] = trim_exchanged(c);
    }
}

// exclusive scan of the per-read counts, in place, + the total behind them: ONE workgroup of 1024 walks the array in tiles (the array has one entry
// per read; the stage's records are 96 bytes each, so this is noise next to the scatter)
__global__ void __launch_bounds__(1024)
k_trim_scan(unsigned long long* __restrict__ cnt, int nids)
{
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nids; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long v = i < nids ? cnt[i] : 0ULL;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const unsigned long long a = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0ULL;
            __syncthreads();
            part[threadIdx.x] += a;
            __syncthreads();
        }
        const unsigned long long incl = part[threadIdx.x], c0 = carry;
        if (i < nids) cnt[i] = c0 + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c0 + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[nids] = carry;
}

// one wave per read id; the count of reads handed back is added up with one atomic per such read
__global__ void __launch_bounds__(64)
k_trim_ranges(const necat_m4* __restrict__ recs, const unsigned long long* __restrict__ read_off, int nids, double min_ident_perc, int min_ovlp_size, int min_cov,
              int min_size, necat_clip_range* __restrict__ out, unsigned long long* __restrict__ n_host)
{
    __shared__ TrimLds sh;
    const int id = (int)blockIdx.x;
    if (id >= nids) return;
    const unsigned long long from = read_off[id], to = read_off[id + 1];
    const unsigned long long cnt = to - from;
    const int n = cnt > (unsigned long long)kTrimCap ? kTrimCap + 1 : (int)cnt;
    trim_read_core(sh, recs + from, n, min_ident_perc, min_ovlp_size, min_cov, min_size, out + id);
    __syncthreads();
    if (threadIdx.x == 0 && out[id].how == necat_trim::kHost) atomicAdd(n_host, 1ULL);
}
#endif

}  // namespace necat
