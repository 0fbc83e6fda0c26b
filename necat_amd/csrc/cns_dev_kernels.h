// cns_dev_kernels.h - the consensus proper of oc2cns on the device (gfx950, wave64): the kernels around the per-lane cores of cns_dev_core.h.
// One chunk of templates per pass (stage_cns_consensus.inl): tags of every overlap -> counting sort by target position + rank sort of every position's bucket on the
// total order -> links / nodes / coverage per template -> best path per stretch, with the certification flags.  No floating-point atomics: every sum has one order.
#pragma once
#include "cns_dev_core.h"

#if defined(__HIPCC__)
namespace necat {
namespace cns_dev {

NECAT_D u64 shfl64(u64 v, int src) { const u32 lo = (u32)__shfl((int)(u32)v, src), hi = (u32)__shfl((int)(u32)(v >> 32), src); return (u64)hi << 32 | lo; }
NECAT_D int wave_incl_sum(int v, int lane) { for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; } return v; }
NECAT_D int wave_incl_max(int v, int lane) { for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v = max(v, t); } return v; }

// ---- tags: one wave per overlap, 64 columns at a time; t_pos / delta / the query index from prefix scans carried across the windows (get_cns_tags,
// tasc/align_tags.c:22-71).  An overlap with a run of >= 255 query bases between two target bases (:38-42), and any tag outside the template, is marked with
// position `tsize`: it is not counted, not scattered and not sorted.  Also counts the live tags of every bucket.
__global__ void __launch_bounds__(256)
k_cns_tags(const DevOvl* __restrict__ ovs, u32 n_ov, const DevTmpl* __restrict__ tm, const u8* __restrict__ ops, const u64* __restrict__ words,
           u64* __restrict__ keys, u32* __restrict__ cnt)
{
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= n_ov) return;
    const DevOvl o = ovs[w];
    const DevTmpl T = tm[o.tmpl];
    const u8* op_bytes = ops + o.ops_off;
    bool dropped = false;
    {
        int last = -1;
        for (i32 base = 0; base < o.ncols; base += 64) {
            const i32 i = base + lane;
            const bool valid = i < o.ncols;
            const int op = valid ? (op_bytes[i >> 2] >> ((i & 3) * 2)) & 3 : 1;
            const int v = wave_incl_max(max(valid && op != 1 ? i : -1, last), lane);
            if (__ballot(valid && i - v >= 255) != 0ULL) dropped = true;
            last = __shfl(v, 63);
        }
    }
    ColState carry = {0, 0, -1};
    ColTag prev_last = {-1, 0, 0};
    auto qb = [&](i32 qi) { return strand_base(words, o.read_begin, o.qsize, o.qdir, max(0, min(o.qoff + qi, o.qsize - 1))); };
    for (i32 base = 0; base < o.ncols; base += 64) {
        const i32 i = base + lane;
        const bool valid = i < o.ncols;
        const int op = valid ? (op_bytes[i >> 2] >> ((i & 3) * 2)) & 3 : 1;
        const int is_t = valid && op != 1, is_q = valid && op != 2;
        const int t_in = wave_incl_sum(is_t, lane), q_in = wave_incl_sum(is_q, lane);
        const int l_in = wave_incl_max(max(is_t ? i : -1, carry.last_t), lane);
        int l_ex = __shfl_up(l_in, 1);
        if (lane == 0) l_ex = carry.last_t;
        ColState before = {carry.tcnt + t_in - is_t, carry.qcnt + q_in - is_q, l_ex};
        ColTag t = {0, 0, 0};
        if (valid) t = col_tag(op, i, before, o.toff, qb);
        ColTag prev;
        prev.t_pos = __shfl_up(t.t_pos, 1); prev.delta = (u32)__shfl_up((int)t.delta, 1); prev.qs = (u32)__shfl_up((int)t.qs, 1);
        if (lane == 0) prev = prev_last;
        if (valid) {
            const bool in = !dropped && t.t_pos >= 0 && t.t_pos < T.tsize;
            const u64 key = in ? col_key(t, prev, i == 0, o.k) : (u64)(u32)T.tsize << 40;
            keys[(u64)o.tag_base + (u32)i] = key;
            if (in) atomicAdd(&cnt[T.pos_base + (u32)t.t_pos], 1u);
        }
        carry.tcnt += __shfl(t_in, 63); carry.qcnt += __shfl(q_in, 63); carry.last_t = __shfl(l_in, 63);
        prev_last.t_pos = __shfl(t.t_pos, 63); prev_last.delta = (u32)__shfl((int)t.delta, 63); prev_last.qs = (u32)__shfl((int)t.qs, 63);
    }
}

// exclusive scan of a template's bucket counts (one workgroup per template): off[] = where each bucket's tags go, cursor[] = the same for the scatter
__global__ void __launch_bounds__(256)
k_cns_scan(const DevTmpl* __restrict__ tm, const u32* __restrict__ cnt, u32* __restrict__ off, u32* __restrict__ cursor)
{
    __shared__ u32 part[256];
    __shared__ u32 carry;
    const DevTmpl T = tm[blockIdx.x];
    const u32 nb = (u32)T.tsize + 1u, tid = threadIdx.x;
    if (tid == 0) carry = T.tag_base;
    __syncthreads();
    for (u32 base = 0; base < nb; base += 256) {
        const u32 b = base + tid;
        const u32 c = b < nb ? cnt[T.pos_base + b] : 0u;
        part[tid] = c;
        __syncthreads();
        for (u32 d = 1; d < 256; d <<= 1) { const u32 v = tid >= d ? part[tid - d] : 0u; __syncthreads(); part[tid] += v; __syncthreads(); }
        const u32 ex = carry + part[tid] - c;
        if (b < nb) { off[T.pos_base + b] = ex; cursor[T.pos_base + b] = ex; }
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
    if (tid == 0) off[T.pos_base + nb] = T.tag_base + T.ntags;       // (the next template's first entry, the same value; the last template's: the end of the chunk)
}

// live tags into their buckets, in any order (the rank sort below fixes the order)
__global__ void __launch_bounds__(256)
k_cns_scatter(const DevOvl* __restrict__ ovs, u32 n_ov, const DevTmpl* __restrict__ tm, const u64* __restrict__ keys, u32* __restrict__ cursor, u64* __restrict__ out)
{
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= n_ov) return;
    const DevOvl o = ovs[w];
    const u32 pos_base = tm[o.tmpl].pos_base, tsize = (u32)tm[o.tmpl].tsize;
    for (i32 i = (i32)(threadIdx.x & 63u); i < o.ncols; i += 64) {
        const u64 k = keys[(u64)o.tag_base + (u32)i];
        if (key_pos(k) < tsize) out[atomicAdd(&cursor[pos_base + key_pos(k)], 1u)] = k;
    }
}

// rank sort of every bucket, one wave per bucket: a key's place is the number of smaller keys.  kTies = false: the keys are distinct (the overlap index is part of
// them).  kTies = true (ctg_dev_kernels.h: keys without an overlap index): equal keys keep the order they came in, by their index in the bucket.
// Any bucket size: 64 keys at a time against 64 keys at a time.  A bucket's size is its count of live tags: a template's last bucket (`tsize`, the room its dropped
// tags leave) has none and costs nothing.
// one batch of a bucket: the 64 keys from index a on, each to its rank among the bucket's n keys
template <bool kTies>
NECAT_D void bucket_rank_batch(const u64* __restrict__ in, u64* __restrict__ out, u32 lo, u32 n, u32 a, int lane)
{
    const bool have = a + (u32)lane < n;
    const u64 mine = have ? in[lo + a + (u32)lane] : ~0ULL;
    u32 rank = 0;
    for (u32 b = 0; b < n; b += 64) {
        const u64 other = b + (u32)lane < n ? in[lo + b + (u32)lane] : ~0ULL;
        const int m = (int)min(64u, n - b);
        if (kTies) { for (int j = 0; j < m; ++j) { const u64 o = shfl64(other, j); rank += (o < mine || (o == mine && b + (u32)j < a + (u32)lane)) ? 1u : 0u; } }
        else for (int j = 0; j < m; ++j) rank += shfl64(other, j) < mine ? 1u : 0u;
    }
    if (have) out[lo + rank] = mine;
}
// big_list != nullptr: a bucket of more than big_size keys is not sorted here - its batches are a whole grid's work (ctg_dev_kernels.h: k_ctg_sort_big) - but listed:
// big_list[0] counts them, big_list[1 ..] names them
template <bool kTies>
NECAT_D void bucket_rank_sort(const u32* __restrict__ off, const u32* __restrict__ cnt, u32 n_buckets, const u64* __restrict__ in, u64* __restrict__ out,
                              u32 big_size = ~0u, u32* __restrict__ big_list = nullptr)
{
    const int lane = (int)(threadIdx.x & 63u);
    for (u32 g = blockIdx.x * 4u + (threadIdx.x >> 6); g < n_buckets; g += gridDim.x * 4u) {
        const u32 lo = off[g], n = cnt[g];
        if (big_list && n > big_size) { if (lane == 0) big_list[1u + atomicAdd(&big_list[0], 1u)] = g; continue; }
        for (u32 a = 0; a < n; a += 64) bucket_rank_batch<kTies>(in, out, lo, n, a, lane);
    }
}
__global__ void __launch_bounds__(256)
k_cns_sort(const u32* __restrict__ off, const u32* __restrict__ cnt, u32 n_buckets, const u64* __restrict__ in, u64* __restrict__ out)
{
    bucket_rank_sort<false>(off, cnt, n_buckets, in, out);
}

struct DevGraph {
    double* l_w; double* l_e; i32* l_pred;
    u32* n_lfirst; u32* n_nlink; i32* n_pos; u32* n_dc;
    double* n_score; double* n_err; i32* n_best;
    u32* node_of_tag; i32* cov; u32* t_nodes; u32* flags;
};

// ---- backbone of one template (one workgroup): run boundaries of the sorted tags give nodes and links (build_backbone, tasc/cns_aux.c:22-125)
__global__ void __launch_bounds__(256)
k_cns_backbone(const DevTmpl* __restrict__ tm, const u64* __restrict__ keys, const u32* __restrict__ off, const double* __restrict__ ovl_weight, double tol, DevGraph G)
{
    __shared__ u64 part[256];
    __shared__ u64 carry;
    const DevTmpl T = tm[blockIdx.x];
    const u32 tid = threadIdx.x, tb = T.tag_base, n = off[T.pos_base + (u32)T.tsize] - tb;      // (the tags before the bucket of dropped ones)
    const u64* K = keys + tb;
    if (tid == 0) carry = 0;
    __syncthreads();
    u32 bad = 0;
    for (u32 base = 0; base < n; base += 256) {
        const u32 i = base + tid;
        const bool valid = i < n;
        const u64 k = valid ? K[i] : 0, kp = valid && i ? K[i - 1] : 0;
        const bool new_node = valid && (i == 0 || key_node(k) != key_node(kp)), new_link = valid && (i == 0 || key_link(k) != key_link(kp));
        const u64 mine = (u64)new_node | (u64)new_link << 32;
        part[tid] = mine;
        __syncthreads();
        for (u32 d = 1; d < 256; d <<= 1) { const u64 v = tid >= d ? part[tid - d] : 0; __syncthreads(); part[tid] += v; __syncthreads(); }
        const u64 incl = carry + part[tid];
        if (valid) {
            const u32 node = tb + (u32)incl - 1u, link = tb + (u32)(incl >> 32) - 1u, pos = key_pos(k);
            const u32* boff = off + T.pos_base;
            G.node_of_tag[tb + i] = node;
            if (new_node) { G.n_lfirst[node] = link; G.n_pos[node] = (i32)pos; G.n_dc[node] = key_delta(k) << 3 | visit_code(key_qs(k)); }
            if (new_link) {
                double lw, le;
                link_sum(keys, tb + i, boff[pos + 1], ovl_weight + T.ov_base, &lw, &le);
                G.l_w[link] = lw; G.l_e[link] = le * tol;
                if (!(le <= kMaxLinkErr)) bad |= 2u; else if (!(le * tol <= kMaxLinkErr)) bad |= 4u;
                const u32 pp = key_pp(k);
                i64 pt = -1;
                if (pp) {
                    if (pp == 1 && pos == 0) bad |= 2u;
                    else {
                        const u32 ppos = pp == 2 ? pos : pos - 1;
                        pt = find_node_tag(keys, boff[ppos], boff[ppos + 1], key_pred_node(k, ppos));
                        if (pt < 0) bad |= 2u;
                    }
                }
                G.l_pred[link] = (i32)pt;          // (a tag index until the nodes are numbered: below)
            }
            if (key_delta(k) == 0 && (tb + i + 1 == boff[pos + 1] || key_delta(K[i + 1]) != 0)) G.cov[T.pos_base + pos] = (i32)(tb + i - boff[pos] + 1);
        }
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
    if (bad) atomicOr(&G.flags[blockIdx.x], bad);
    const u32 nn = (u32)carry, nl = (u32)(carry >> 32);
    if (tid == 0) G.t_nodes[blockIdx.x] = nn;
    for (u32 a = tid; a < nn; a += 256) {
        const u32 node = tb + a;
        G.n_nlink[node] = (a + 1 < nn ? G.n_lfirst[node + 1] : tb + nl) - G.n_lfirst[node];
        G.n_score[node] = 0.0; G.n_err[node] = 0.0; G.n_best[node] = -1;
    }
    for (u32 a = tid; a < nl; a += 256) { const i32 p = G.l_pred[tb + a]; if (p >= 0) G.l_pred[tb + a] = (i32)G.node_of_tag[p]; }
}

// first position >= from of cov[0 .. tsize) that is (want_ge) at least / (else) below min_cov, or tsize; the whole wave calls it
NECAT_D int cns_find_pos(const i32* cov, int from, int tsize, int min_cov, bool want_ge, int lane)
{
    for (int base = from; base < tsize; base += 64) {
        const int i = base + lane;
        const unsigned long long m = __ballot(i < tsize && ((cov[i] >= min_cov) == want_ge));
        if (m) return base + __ffsll((long long)m) - 1;
    }
    return tsize;
}

// ---- best path (consensus_backbone_segment, tasc/cns_aux.c:127-217), one wave per template, its stretches one after the other (consensus_broken /
// consensus_unbroken walk them the same way, tasc/cbcns.c:108-264).  The nodes of one (position, delta) level depend on earlier levels only: one lane per node of the
// level.  flags[t] != 0: one of the template's decisions lies inside the error bounds (1), its arrays or bounds are not what the kernels expect (2), or its scaled bounds are too
// loose to certify anything (4): the host recomputes it.
__global__ void __launch_bounds__(64)
k_cns_path(const DevTmpl* __restrict__ tm, const u32* __restrict__ off, DevGraph D, int min_cov, int min_size, u8* __restrict__ out, Seg* __restrict__ segs, u32* __restrict__ seg_n)
{
    const DevTmpl T = tm[blockIdx.x];
    const int lane = (int)threadIdx.x, tsize = T.tsize;
    const u32 tb = T.tag_base;
    const i32* cov = D.cov + T.pos_base;
    const u32* boff = off + T.pos_base;
    Graph G = {D.l_w, D.l_e, D.l_pred, D.n_lfirst, D.n_nlink, D.n_pos, D.n_dc, D.n_score, D.n_err, D.n_best};
    const u32 nn_end = tb + D.t_nodes[blockIdx.x];
    bool flagged = false;
    u32 nseg = 0;
    int i = 0;
    while (i < tsize) {
        i = cns_find_pos(cov, i, tsize, min_cov, true, lane);
        if (i >= tsize) break;
        const int j = cns_find_pos(cov, i + 1, tsize, min_cov, false, lane);
        if (j - i >= min_size * 0.85) {
            const u32 live_end = boff[tsize];
            const u32 n0 = boff[i] < live_end ? D.node_of_tag[boff[i]] : nn_end, n1 = boff[j] < live_end ? D.node_of_tag[boff[j]] : nn_end;
            double bs = -1.0, be = 0.0; u64 bvk = ~0ULL; i32 bn = -1;
            u32 n = n0;
            while (n < n1) {
                const u32 my = n + (u32)lane;
                const bool in = lane < 5 && my < n1;
                const i32 pos = in ? G.n_pos[my] : -1;
                const u32 dc = in ? G.n_dc[my] : 0u;
                const u64 lev = in ? (u64)(u32)pos << 8 | dc >> 3 : ~0ULL;
                const bool same = in && lev == shfl64(lev, 0);
                const unsigned long long mask = __ballot(same);
                if (same) {
                    if (!node_best(G, my, cov[pos])) flagged = true;
                    const double s = G.n_score[my];
                    const u64 vk = visit_key(pos, dc);
                    if (s > -1.0 && better(s, vk, bs, bvk)) { bs = s; be = G.n_err[my]; bvk = vk; bn = (i32)my; }
                }
                // the next level's lanes read what these lanes wrote to n_score / n_err / n_best: the workgroup is ONE wave (launch bounds 64, no tgsplit mode on gfx950
                // builds of this library), so the fence - the stores leave the lane before later loads issue - is all the ordering that needs
                __threadfence_block();
                n += (u32)__popcll(mask);
            }
            for (int l = 1; l < 5; ++l) {          // the five lanes' bests, by the visiting order
                const double s = __shfl(bs, l), e = __shfl(be, l); const u64 vk = shfl64(bvk, l); const i32 b = __shfl(bn, l);
                if (b != -1 && (bn == -1 || better(s, vk, bs, bvk))) { bs = s; be = e; bvk = vk; bn = b; }
            }
            bs = __shfl(bs, 0); be = __shfl(be, 0); bn = __shfl(bn, 0);
            for (u32 a = n0 + (u32)lane; a < n1; a += 64) if ((i32)a != bn && !certain(bs, be, G.n_score[a], G.n_err[a])) flagged = true;
            if (bn >= 0 && !certain(bs, be, -1.0, 0.0)) flagged = true;
            if (lane == 0 && bn >= 0) {
                Seg sg;
                sg.len = traceback(G, bn, out + n1, &sg.cns_from);
                if ((int)sg.len >= min_size) {
                    sg.left = i; sg.right = j; sg.cns_to = G.n_pos[bn] + 1; sg.off = n1 - sg.len;
                    if (nseg < T.seg_cap) segs[T.seg_base + nseg] = sg; else flagged = true;
                    ++nseg;
                }
            }
        }
        i = j;
    }
    if (__ballot(flagged) != 0ULL && lane == 0) atomicOr(&D.flags[blockIdx.x], 1u);
    if (lane == 0) seg_n[blockIdx.x] = nseg;
}

}  // namespace cns_dev
}  // namespace necat
#endif
