// ctg_seed_kernels.h - the seeding of contig polishing on the device (gfx950, wave64): the kernels around the per-lane cores of ctg_seed_core.h
// (stage_ctg_seed.inl launches them; ctg_seed.h has the rule).
//   k_ctgs_index        per segment: open-addressing table key -> chain of positions over every 15-mer of the segment, one thread per position
//   k_ctgs_count        per job, one wave: the read's sampled 15-mers into a table of the job's own (key, occurrences), then per sample the product rule against
//                       the segment's chain (counted up to 21): the job's number of seeds, which sizes its share of the chunk's pool
//   k_ctgs_mems         per job, one wave: the seeds again, each extended word-wise as it is emitted; rank sort by (soff, qoff); the per-diagonal kill test and the
//                       20-base filter; rank sort of the survivors
//   k_ctgs_chain        per job, one wave: the chain DP 64 predecessors at a time (arrays in dynamic LDS up to `lds_cap` matches, in the job's scratch above), the
//                       best (f[peak], peak) among the chain ends and lane 0's walk to the root
// Nothing a kernel writes depends on the order inside the segment table's chains: the seeds are sorted before they are used, and (soff, qoff) is unique among them.
#pragma once
#include "ctg_seed_core.h"
#include "seed_kernels.h"

#if defined(__HIPCC__)
namespace necat {
namespace ctg_seed {

struct SegDev { const u32* keys; const u32* head; const u32* next; u32 cap; };

__global__ void __launch_bounds__(256)
k_ctgs_index(Seq seg, u32 cap, u32* __restrict__ keys, u32* __restrict__ head, u32* __restrict__ next)
{
    const int ne = n_entries(seg.len, 1);
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < ne; e += (i64)gridDim.x * 256) {
        const u32 key = kmer_key(seg, (int)e);
        u32 p = slot_of(key, cap);
        for (;;) {
            const u32 old = atomicCAS(&keys[p], 0u, key);
            if (old == 0u || old == key) break;
            if (++p == cap) p = 0;
        }
        next[e] = atomicExch(&head[p], (u32)e + 1u);
    }
}

// the segment's entries with this key, counted up to 21; the chain's head in *first
NECAT_D int seg_probe(const SegDev& T, u32 key, u32* first)
{
    u32 p = slot_of(key, T.cap);
    for (;;) {
        const u32 kx = T.keys[p];
        if (kx == 0u) return 0;
        if (kx == key) break;
        if (++p == T.cap) p = 0;
    }
    int c = 0;
    const u32 h0 = T.head[p];
    for (u32 x = h0; x && c <= kMaxOcc; x = T.next[x - 1]) ++c;
    *first = h0;
    return c;
}
// seeds of the read's sample e (find_kmer_match's product rule, mem_finder.c:156-157): 0, or the segment's occurrences
NECAT_D int sample_seeds(const SegDev& T, const Seq& read, const u32* qtab, u32 qcap, int e, u32* first)
{
    const u32 key = kmer_key(read, e * kReadWindow);
    const int tocc = seg_probe(T, key, first);
    if (tocc == 0 || tocc > kMaxOcc) return 0;
    u32 p = slot_of(key, qcap);
    while (__hip_atomic_load(&qtab[2 * p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != key) if (++p == qcap) p = 0;
    const u32 qocc = __hip_atomic_load(&qtab[2 * p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (u64)qocc * (u64)tocc <= (u64)kMaxOcc ? tocc : 0;
}

__global__ void __launch_bounds__(64)
k_ctgs_count(const u64* __restrict__ read_bases, SegDev T, JobDev* __restrict__ jobs, u32 n_jobs, u32* __restrict__ qtabs)
{
    const u32 w = blockIdx.x;
    if (w >= n_jobs) return;
    const int lane = threadIdx.x;
    const JobDev J = jobs[w];
    const Seq read = {read_bases, J.read_g0, J.qlen, J.qrev};
    u32* const qtab = qtabs + J.qtab_off;
    const int ns = n_entries(J.qlen, kReadWindow);
    for (int e = lane; e < ns; e += 64) {
        const u32 key = kmer_key(read, e * kReadWindow);
        u32 p = slot_of(key, J.qcap);
        for (;;) {
            const u32 old = atomicCAS(&qtab[2 * p], 0u, key);
            if (old == 0u || old == key) break;
            if (++p == J.qcap) p = 0;
        }
        atomicAdd(&qtab[2 * p + 1], 1u);
    }
    __syncthreads();
    u32 total = 0;
    for (int e = lane; e < ns; e += 64) { u32 first; total += (u32)sample_seeds(T, read, qtab, J.qcap, e, &first); }
    for (int o = 32; o > 0; o >>= 1) total += (u32)__shfl_xor((int)total, o);
    if (lane == 0) jobs[w].n_matches = total;
}

// sel: the chunk's jobs.  pool: per seed of the chunk a SeedRec in tmp and in sd, a DMem in tm and in ms.  out[job].n_mems; bad[0] counts jobs whose seeds are not the counted ones, bad[1] pairs of surviving matches that share a start (no defined order)
__global__ void __launch_bounds__(64)
k_ctgs_mems(const u64* __restrict__ read_bases, Seq seg, SegDev T, const JobDev* __restrict__ jobs, const u32* __restrict__ sel, u32 n_sel, const u32* __restrict__ qtabs,
            SeedRec* __restrict__ tmp, SeedRec* __restrict__ sds, DMem* __restrict__ tms, DMem* __restrict__ mss, DCan* __restrict__ out, u32* __restrict__ bad)
{
    if (blockIdx.x >= n_sel) return;
    const u32 w = sel[blockIdx.x];
    const int lane = threadIdx.x;
    const u64 below = (1ULL << lane) - 1ULL;
    const JobDev J = jobs[w];
    const Seq read = {read_bases, J.read_g0, J.qlen, J.qrev};
    const u32* const qtab = qtabs + J.qtab_off;
    const int ns = n_entries(J.qlen, kReadWindow);
    SeedRec* const tp = tmp + J.seed_off; SeedRec* const sd = sds + J.seed_off;
    DMem* const tm = tms + J.seed_off; DMem* const ms = mss + J.seed_off;
    u32 total = 0;
    for (int e0 = 0; e0 < ns; e0 += 64) {
        const int e = e0 + lane;
        int c = 0; u32 first = 0;
        if (e < ns) c = sample_seeds(T, read, qtab, J.qcap, e, &first);
        const int inc = wave_prefix_sum(c);
        u32 at = total + (u32)(inc - c);
        for (u32 x = first; c > 0; x = T.next[x - 1], --c, ++at) {
            if (at >= J.n_matches) { atomicAdd(bad, 1u); break; }
            tp[at] = extend_seed(seg, read, (int)x - 1, e * kReadWindow);
        }
        total += (u32)wave_read(inc, 63);
    }
    if (total != J.n_matches) { if (lane == 0) atomicAdd(bad, 1u); return; }
    __syncthreads();
    // (soff, qoff) is unique among seeds: the rank is the place
    for (u32 a = (u32)lane; a < total; a += 64) {
        const SeedRec x = tp[a];
        const u64 kx = seed_order(x);
        u32 rk = 0;
        for (u32 b = 0; b < total; ++b) rk += seed_order(tp[b]) < kx ? 1u : 0u;
        sd[rk] = x;
    }
    __syncthreads();
    u32 nm = 0;
    for (u32 a0 = 0; a0 < total; a0 += 64) {
        const u32 a = a0 + (u32)lane;
        bool keep = false;
        SeedRec s = {0, 0, 0, 0};
        if (a < total) { s = sd[a]; keep = s.qr - s.ql >= kMinMem && !seed_dropped(sd, (i64)a); }
        const u64 km = __ballot(keep);
        if (keep) tm[nm + (u32)popc64(km & below)] = mem_of(s);
        nm += (u32)popc64(km);
    }
    __syncthreads();
    for (u32 a = (u32)lane; a < nm; a += 64) {
        const DMem x = tm[a];
        const u64 kx = mem_order(x);
        u32 rk = 0;
        for (u32 b = 0; b < nm; ++b) { const u64 ky = mem_order(tm[b]); rk += (ky < kx || (ky == kx && b < a)) ? 1u : 0u; if (ky == kx && b < a) atomicAdd(bad + 1, 1u); }
        ms[rk] = x;
    }
    if (lane == 0) out[w].n_mems = (i32)nm;
}

// scratch: 4 i32 per seed of the chunk (f, p, t, v of a job whose matches outgrow lds_cap).  Dynamic LDS: lds_cap x (DMem + 4 i32)
__global__ void __launch_bounds__(64)
k_ctgs_chain(const JobDev* __restrict__ jobs, const u32* __restrict__ sel, u32 n_sel, const DMem* __restrict__ mss, i32* __restrict__ scratch, u32 lds_cap, DCan* __restrict__ out)
{
    extern __shared__ i32 l_mem[];
    if (blockIdx.x >= n_sel) return;
    const u32 w = sel[blockIdx.x];
    const int lane = threadIdx.x;
    const u64 below = (1ULL << lane) - 1ULL;
    const JobDev J = jobs[w];
    const int n = out[w].n_mems;
    if (n <= 0) return;
    const DMem* gm = mss + J.seed_off;
    const bool in_lds = (u32)n <= lds_cap;
    const DMem* m = gm;
    // (volatile: above lds_cap the arrays live in global memory, written and read by different lanes of this wave between barriers)
    volatile i32 *f, *p, *t, *v;
    if (in_lds) {
        DMem* l_m = (DMem*)(l_mem + 4 * (size_t)lds_cap);
        for (int a = lane; a < n; a += 64) l_m[a] = gm[a];
        m = l_m; f = l_mem; p = l_mem + lds_cap; t = l_mem + 2 * (size_t)lds_cap; v = l_mem + 3 * (size_t)lds_cap;
    } else {
        i32* cs = scratch + 4 * J.seed_off;
        f = cs; p = cs + n; t = cs + 2 * (size_t)n; v = cs + 3 * (size_t)n;
    }
    int sum = 0;
    for (int a = lane; a < n; a += 64) { sum += gm[a].size; f[a] = 0; p[a] = -1; t[a] = 0; v[a] = 0; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const int avg_cov = sum / n;
    __syncthreads();
    int st = 0;
    for (int i = 0; i < n; ++i) {
        const DMem mi = m[i];
        while (st < i && mi.soff > m[st].soff + kMaxDist) ++st;
        int max_f = mi.size, max_j = -1, n_skip = 0;
        for (int top = i - 1; top >= st; top -= 64) {
            const int j = top - lane;
            int sc = INT32_MIN;
            bool valid = false;
            if (j >= st) {
                valid = pair_score(mi, m[j], f[j], avg_cov, &sc);
                if (valid) { const int pj = p[j]; if (pj >= 0) t[pj] = i; }
                else sc = INT32_MIN;
            }
            __syncthreads();
            const bool marked = valid && t[j] == i;
            const int incl = wave_prefix_max(sc);
            int before = wave_from_below(incl, max_f);
            if (before < max_f) before = max_f;
            const bool newmax = valid && sc > before;
            const u64 NM = __ballot(newmax), SK = __ballot(marked && !newmax);
            u64 live = ~0ULL;
            if (SK) {
                const u64 upto = below | (1ULL << lane);
                const int S = popc64(SK & upto) - popc64(NM & upto);
                int floor_ = wave_prefix_min(S);
                if (floor_ > -n_skip) floor_ = -n_skip;
                const int W = S - floor_;
                const u64 stop = __ballot(W > kMaxSkip);
                if (stop) live = (1ULL << ctz64(stop)) - 1ULL;
                else n_skip = wave_read(W, 63);
            } else {
                n_skip -= popc64(NM); if (n_skip < 0) n_skip = 0;
            }
            const u64 best = NM & live;
            if (best) { const int lb = 63 - __clzll((long long)best); max_f = wave_read(sc, lb); max_j = top - lb; }
            if (live != ~0ULL) break;
        }
        if (lane == 0) {
            f[i] = max_f; p[i] = max_j;
            v[i] = (max_j >= 0 && v[max_j] > max_f) ? v[max_j] : max_f;
        }
        __syncthreads();
    }
    // chain ends (nobody's predecessor) whose best prefix reaches the minimum score; the largest (f[peak], peak)
    for (int a = lane; a < n; a += 64) t[a] = 0;
    __syncthreads();
    for (int a = lane; a < n; a += 64) { const int pa = p[a]; if (pa >= 0) t[pa] = 1; }
    __syncthreads();
    i64 bestk = -1;
    for (int a = lane; a < n; a += 64) {
        if (t[a] == 0 && v[a] >= kMinScore) {
            int j = a;
            while (j >= 0 && f[j] < v[j]) j = p[j];
            if (j < 0) j = a;
            const i64 key = ((i64)f[j] << 32) | (i64)(u32)j;
            if (key > bestk) bestk = key;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { const i64 x = __shfl_xor(bestk, o); if (x > bestk) bestk = x; }
    if (lane != 0) return;
    DCan c = out[w];
    c.tier = in_lds ? 0 : 1;
    if (bestk >= 0) {
        const int peak = (int)(u32)(bestk & 0xffffffffLL);
        c.found = 1; c.score = (int)(bestk >> 32);
        const DMem mp = m[peak];
        c.qend = mp.qoff + mp.size; c.send = mp.soff + mp.size;
        int max_size = 0;
        for (int j = peak; j >= 0; j = p[j]) {
            const DMem x = m[j];
            ++c.chain_len; c.qbeg = x.qoff; c.sbeg = x.soff;
            if (x.size >= max_size) { max_size = x.size; c.qoff = x.qoff + max_size / 2; c.soff = x.soff + max_size / 2; }
        }
    }
    out[w] = c;
}

}  // namespace ctg_seed
}  // namespace necat
#endif
