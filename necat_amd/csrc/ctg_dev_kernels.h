// ctg_dev_kernels.h - the consensus half of contig polishing on the device (gfx950, wave64): the kernels around the per-lane cores of ctg_dev_core.h.
// One position range of one segment per pass (stage_ctg_consensus.inl): tags of every overlap that crosses the range -> counting sort by position (k_cns_scan of
// cns_dev_kernels.h as it is, a flat scatter) + the rank sort of every position's bucket (cns_dev_kernels.h's bucket_rank_sort, ties kept in place; big buckets over the whole grid) -> nodes, links,
// coverage and per-position node offsets as compact arrays, tiled over positions.  Nothing per tag goes back to the host; the score pass runs there.
#pragma once
#include "cns_dev_kernels.h"
#include "ctg_dev_core.h"

#if defined(__HIPCC__)
namespace necat {
namespace ctg_dev {

using cns_dev::wave_incl_sum;
using cns_dev::wave_incl_max;

// ---- tags: one wave per overlap, 64 columns at a time from the column the plan names, t_pos / delta / the query index from prefix scans carried across the windows
// and across the ranges (Start).  Every slot gets a key: a column outside the range (the one column in front of it) gets the range's size as position, which is not
// counted, not scattered and not sorted.
__global__ void __launch_bounds__(256)
k_ctg_tags(const RangeOvl* __restrict__ ovs, u32 n_ov, u32 range_size, const u8* __restrict__ ops, const u64* __restrict__ words, u64* __restrict__ keys, u32* __restrict__ cnt)
{
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= n_ov) return;
    const RangeOvl o = ovs[w];
    const u8* op_bytes = ops + o.ops_off;
    ColState carry = {o.st.tcnt, o.st.qcnt, o.st.last_t};
    ColTag prev_last = {-1, 0, 0};
    auto qb = [&](i32 qi) { return cns_dev::strand_base(words, o.read_begin, o.qsize, o.qdir, max(0, min(o.qoff + qi, o.qsize - 1))); };
    for (u32 base = 0; base < o.slots; base += 64) {
        const bool valid = base + (u32)lane < o.slots;
        const i32 i = o.st.col0 + (i32)(base + (u32)lane);
        const int op = valid ? (op_bytes[i >> 2] >> ((i & 3) * 2)) & 3 : 1;
        const int is_t = valid && op != 1, is_q = valid && op != 2;
        const int t_in = wave_incl_sum(is_t, lane), q_in = wave_incl_sum(is_q, lane);
        const int l_in = wave_incl_max(max(is_t ? i : -1, carry.last_t), lane);
        int l_ex = __shfl_up(l_in, 1);
        if (lane == 0) l_ex = carry.last_t;
        const ColState before = {carry.tcnt + t_in - is_t, carry.qcnt + q_in - is_q, l_ex};
        ColTag t = {0, 0, 0};
        if (valid) t = cns_dev::col_tag(op, i, before, o.toff, qb);
        ColTag prev;
        prev.t_pos = __shfl_up(t.t_pos, 1); prev.delta = (u32)__shfl_up((int)t.delta, 1); prev.qs = (u32)__shfl_up((int)t.qs, 1);
        if (lane == 0) prev = prev_last;
        if (valid) {
            const bool in = t.t_pos >= 0 && (u32)t.t_pos < range_size;
            keys[(u64)o.slot_base + base + (u32)lane] = in ? col_key(t, prev, i == 0) : (u64)range_size << 40;
            if (in) atomicAdd(&cnt[(u32)t.t_pos], 1u);
        }
        carry.tcnt += __shfl(t_in, 63); carry.qcnt += __shfl(q_in, 63); carry.last_t = __shfl(l_in, 63);
        prev_last.t_pos = __shfl(t.t_pos, 63); prev_last.delta = (u32)__shfl((int)t.delta, 63); prev_last.qs = (u32)__shfl((int)t.qs, 63);
    }
}

// live tags into their buckets, in any order: one thread per slot
__global__ void __launch_bounds__(256)
k_ctg_scatter(const u64* __restrict__ keys, u32 n_slots, u32 range_size, u32* __restrict__ cursor, u64* __restrict__ out)
{
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n_slots; i += gridDim.x * 256u) {
        const u64 k = keys[i];
        if (key_pos(k) < range_size) out[atomicAdd(&cursor[key_pos(k)], 1u)] = k;
    }
}

// A long insertion run puts tens of thousands of tags into one position's bucket: a bucket of more than kBigBucket keys is listed by k_ctg_sort and its batches of
// 64 keys are dealt out over the waves of k_ctg_sort_big's whole grid (one wave alone would rank 65 534 keys in seconds)
__global__ void __launch_bounds__(256)
k_ctg_sort(const u32* __restrict__ off, const u32* __restrict__ cnt, u32 n_buckets, const u64* __restrict__ in, u64* __restrict__ out, u32* __restrict__ big_list)
{
    cns_dev::bucket_rank_sort<true>(off, cnt, n_buckets, in, out, kBigBucket, big_list);
}
__global__ void __launch_bounds__(256)
k_ctg_sort_big(const u32* __restrict__ off, const u32* __restrict__ cnt, const u32* __restrict__ big_list, const u64* __restrict__ in, u64* __restrict__ out)
{
    const u32 wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 n_big = big_list[0];
    for (u32 x = 0; x < n_big; ++x) {
        const u32 g = big_list[1u + x], lo = off[g], n = cnt[g];
        for (u32 a = wave * 64u; a < n; a += n_waves * 64u) cns_dev::bucket_rank_batch<true>(in, out, lo, n, a, lane);
    }
}

// ---- links, pass 1: the nodes and links that begin in every tile of kTilePositions positions (nodes in the low half of the count, links in the high half)
__global__ void __launch_bounds__(256)
k_ctg_count(const u64* __restrict__ K, const u32* __restrict__ off, u32 range_size, u64* __restrict__ tile_cnt)
{
    __shared__ u32 sn, sl;
    if (threadIdx.x == 0) { sn = 0; sl = 0; }
    __syncthreads();
    const u32 p0 = blockIdx.x * kTilePositions, p1 = min(range_size, p0 + kTilePositions);
    const u32 lo = off[p0], hi = off[p1];
    u32 nn = 0, nl = 0;
    for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
        const RunStart s = run_start(K[i], i ? K[i - 1] : 0, i == 0);
        nn += s.node; nl += s.link;
    }
    if (nn) atomicAdd(&sn, nn);
    if (nl) atomicAdd(&sl, nl);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (u64)sn | (u64)sl << 32;
}

// pass 2: exclusive scan of the tiles' counts (one workgroup); tile_base[n_tiles] = the range's nodes and links
__global__ void __launch_bounds__(256)
k_ctg_tile_scan(const u64* __restrict__ tile_cnt, u32 n_tiles, u64* __restrict__ tile_base)
{
    __shared__ u64 part[256];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (u32 base = 0; base < n_tiles; base += 256) {
        const u32 t = base + tid;
        const u64 c = t < n_tiles ? tile_cnt[t] : 0;
        part[tid] = c;
        __syncthreads();
        for (u32 d = 1; d < 256; d <<= 1) { const u64 v = tid >= d ? part[tid - d] : 0; __syncthreads(); part[tid] += v; __syncthreads(); }
        if (t < n_tiles) tile_base[t] = carry + part[tid] - c;
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
    if (tid == 0) tile_base[n_tiles] = carry;
}

struct DevLinks { u32* n_pos; u32* n_db; u32* n_link0; u32* l_pred; u32* l_tag0; u32* pos_node; i32* cov; };

// pass 3: the run boundaries of the sorted tags of a tile, numbered from the tile's base: nodes (position, delta << 3 | base, first link), links (link word, first
// tag), the first node of every position that has tags, the coverage of every position.  pos_node and cov are preset (all ones / zero).
__global__ void __launch_bounds__(256)
k_ctg_links(const u64* __restrict__ K, const u32* __restrict__ off, u32 range_size, u32 p_first, const u64* __restrict__ tile_base, DevLinks G)
{
    __shared__ u64 part[256];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x;
    const u32 p0 = blockIdx.x * kTilePositions, p1 = min(range_size, p0 + kTilePositions);
    const u32 lo = off[p0], hi = off[p1];
    if (tid == 0) carry = tile_base[blockIdx.x];
    __syncthreads();
    for (u32 base = lo; base < hi; base += 256) {
        const u32 i = base + tid;
        const bool valid = i < hi;
        const u64 k = valid ? K[i] : 0;
        RunStart s = {false, false, false};
        if (valid) s = run_start(k, i ? K[i - 1] : 0, i == 0);
        const u64 mine = (u64)s.node | (u64)s.link << 32;
        part[tid] = mine;
        __syncthreads();
        for (u32 d = 1; d < 256; d <<= 1) { const u64 v = tid >= d ? part[tid - d] : 0; __syncthreads(); part[tid] += v; __syncthreads(); }
        const u64 incl = carry + part[tid];
        if (valid) {
            const u32 node = (u32)incl - 1u, link = (u32)(incl >> 32) - 1u, pos = key_pos(k);
            if (s.node) { G.n_pos[node] = p_first + pos; G.n_db[node] = key_db(k); G.n_link0[node] = link; }
            if (s.link) { G.l_pred[link] = key_link_word(k); G.l_tag0[link] = i; }
            if (s.pos) G.pos_node[pos] = node;
            const u32 bucket_end = off[pos + 1];
            if (closes_coverage(k, i + 1 == bucket_end, i + 1 < bucket_end ? K[i + 1] : 0)) G.cov[pos] = (i32)(i - off[pos] + 1);
        }
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
}

}  // namespace ctg_dev
}  // namespace necat
#endif
