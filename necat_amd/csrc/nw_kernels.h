// nw_kernels.h - the __global__ shells around nw_core.h: one wave (a workgroup of 64) per task.
//   k_nw_cols    score-only banded columns of a (sub)problem, forward or with both sequences reversed (the task's Seq says which); leaves the last
//                column's values of the rows for k_nw_split, and the last row's value for the host
//   k_nw_split   NwPath::solve's split row from the two columns
//   k_nw_leaf    the same pass storing the walk's two flag words per band word and column (16 bytes), then the walk through an LDS window
//   k_nw_finish  a job's leaves joined into one path, edlib_go's end trimming, the columns packed two bits each
#pragma once
#include "nw_core.h"

namespace necat {
namespace nw {

// lane i receives v of lane i - 1 across the whole wave (GFX9 DPP wave_shr:1); lane 0 gets 0
NECAT_D int wave_from_above(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
NECAT_D int wave_sum(int v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d); return v; }

// a 32-base window of a sequence in two steps, so that the loads are in flight while the previous window is used: the two words now, the value later
struct Win { u64 lo, hi; int sh; };
NECAT_D Win win_issue(const u64* bases, const Seq s, int c)
{
    i64 g = s.g0 + (i64)s.dir * c;
    if (s.dir < 0) g -= 31;
    Win w; w.sh = (int)(g & 31) * 2; w.lo = bases[g >> 5]; w.hi = bases[(g >> 5) + 1];      // (the guard words of a volume cover the second word)
    return w;
}
NECAT_D u64 win_value(const Win w, const Seq s)      // = seq_load32 of the same position
{
    u64 x = w.sh ? (w.lo >> w.sh) | (w.hi << (64 - w.sh)) : w.lo;
    if (s.dir < 0) x = rev2(x);
    return s.comp ? ~x : x;
}

// The pass over columns [0, n_stop) of one problem, stripe after stripe.  At step s of a stripe lane l is at column c_lo + s - l of its word; the
// carry (and the column's base with it) moves down one lane per step.  Lane 0 takes the base from a 32-base window of the target and, in stripes
// after the first, the carry the previous stripe's last word left for that column.  The steps go 32 at a time: a chunk starts by taking what was
// loaded a chunk ago (window and 32 boundary carries, one per lane) and issuing the next chunk's loads: the 32 steps themselves load nothing and wait for nothing.
template <bool STORE>
__device__ void wave_pass(const u64* qbases, const u64* tbases, const Seq q, const Seq t, const int m, const int n_stop, const Band bd,
                          int* bnd, ulonglong2* flags, const int W, int* fail, int* col, int* last)
{
    const int lane = (int)(threadIdx.x & 63);
    const int nb = (m + 63) / 64, ns = (nb + kLanes - 1) / kLanes;
    for (int j = 0; j < ns; ++j) {
        const int b = j * kLanes + lane;
        Lane L;
        lane_load(L, qbases, q, m, b);
        int c_lo, c_hi;
        stripe_columns(bd, j, n_stop, &c_lo, &c_hi);
        const bool more = j + 1 < ns;
        const int* bin = bnd + (size_t)((j + 1) & 1) * (size_t)n_stop;
        int* bout = bnd + (size_t)(j & 1) * (size_t)n_stop;
        const int steps = c_hi > c_lo ? c_hi - c_lo + kLanes - 1 : 0;
        Win wn; wn.lo = wn.hi = 0; wn.sh = 0;
        int bnext = 0;
        if (steps) {
            wn = win_issue(tbases, t, c_lo);
            if (j > 0) { const int cc = c_lo + (lane & 31); bnext = cc < c_hi ? bin[cc] : 0; }
        }
        int pk = 0;
        for (int s0 = 0; s0 < steps; s0 += 32) {
            const u64 tw = win_value(wn, t);
            const int breg = bnext;
            const int nx = c_lo + s0 + 32;
            if (nx < n_stop) wn = win_issue(tbases, t, nx);
            if (j > 0) { const int cc = nx + (lane & 31); bnext = cc < c_hi ? bin[cc] : 0; }
            const int s1 = s0 + 32 < steps ? s0 + 32 : steps;
            for (int s = s0; s < s1; ++s) {
                const int ch = c_lo + s;
                int inp = wave_from_above(pk);
                const int bv = __builtin_amdgcn_readlane(breg, s & 31);
                if (lane == 0) {
                    Carry c0; c0.code = (int)((tw >> (2 * (s & 31))) & 3); c0.hout = 1; c0.botp = 0;
                    if (j > 0) { const Carry p = carry_unpack(bv); c0.hout = p.hout; c0.botp = p.botp; }
                    inp = carry_pack(c0);
                }
                const int c = ch - lane;
                Carry out; out.hout = 0; out.botp = 0; out.code = 0;
                if (c >= c_lo && c < c_hi) {
                    u64 A = 0, B = 0;
                    const bool act = lane_step<STORE>(L, bd, b, c, carry_unpack(inp), &out, &A, &B);
                    if (STORE && act) {
                        const int idx = b - band_fb(bd, c);
                        if (idx >= 0 && idx < W) flags[(size_t)c * (size_t)W + (size_t)idx] = make_ulonglong2(A, B);
                        else *fail = 1;
                    }
                    if (more && lane == kLanes - 1) bout[c] = carry_pack(out);
                }
                pk = carry_pack(out);
            }
        }
        if (64 * b < m) {
            if (col) lane_column(L, bd, b, n_stop - 1, col);
            if (b == ((m - 1) >> 6)) *last = lane_last(L, bd, b, n_stop - 1);
        }
        if (more) __threadfence();       // the next stripe's first lane reads what this stripe's last lane wrote
    }
}

__global__ __launch_bounds__(64) void k_nw_cols(const u64* qbases, const u64* tbases, const ColsTask* tasks, int* cols, int* bnd, int* last)
{
    const ColsTask T = tasks[blockIdx.x];
    int dummy = 0;
    wave_pass<false>(qbases, tbases, T.q, T.t, T.m, T.n_stop, T.bd, bnd + T.bnd_off, nullptr, 0, &dummy, T.col_off == ~0ULL ? nullptr : cols + T.col_off,
                     last + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_nw_split(const SplitTask* tasks, const int* cols, SplitOut* out)
{
    const SplitTask T = tasks[blockIdx.x];
    const int lane = (int)(threadIdx.x & 63);
    const int* Lc = cols + T.l_off;
    const int* Rc = cols + T.r_off;
    int first = -1;
    for (int base = 0; base + 1 < T.m; base += kLanes) {
        const u64 mask = __ballot(split_hit(Lc, Rc, T.m, T.best, base + lane));
        if (mask) { first = base + ctz64(mask); break; }
    }
    if (lane == 0) {
        SplitOut o;
        if (first >= 0) { o.row = first; o.ls = Lc[first]; o.rs = Rc[T.m - 2 - first]; }
        else o = split_fallback(Lc, Rc, T.m, T.best, T.lw, T.rw);
        out[blockIdx.x] = o;
    }
}

// the walk's view of the stored flags: 64 columns x 2 words around the walker in LDS; every lane of the wave walks the same path (the state is
// wave-uniform), so the reload is a plain cooperative copy and a step is one LDS read
struct TileMat {
    const ulonglong2* flags;
    ulonglong2* tile;      // [64][2]
    Band bd;
    int W, lane, c_top, b_top;
    __device__ bool rec(int c, int b, u64& A, u64& B)
    {
        const int fb = band_fb(bd, c);
        if (b < fb || b > band_lb(bd, c) || b - fb >= W) return false;
        if (c > c_top || c <= c_top - kLanes || b > b_top || b < b_top - 1) {
            __syncthreads();
            c_top = c; b_top = b;
            const int cc = c - lane;
            for (int k = 0; k < 2; ++k) {
                const int bb = b - k;
                ulonglong2 v = make_ulonglong2(0, 0);
                if (cc >= 0 && bb >= 0) {
                    const int f2 = band_fb(bd, cc);
                    if (bb >= f2 && bb <= band_lb(bd, cc) && bb - f2 < W) v = flags[(size_t)cc * (size_t)W + (size_t)(bb - f2)];
                }
                tile[lane * 2 + k] = v;
            }
            __syncthreads();
        }
        const ulonglong2 v = tile[(c_top - c) * 2 + (b_top - b)];
        A = v.x; B = v.y;
        return true;
    }
};
struct OpsSink {
    u8* end; bool store;
    __device__ void put(int i, int op) { if (store) end[-1 - (i64)i] = (u8)op; }
};

__global__ __launch_bounds__(64) void k_nw_leaf(const u64* qbases, const u64* tbases, const LeafTask* tasks, ulonglong2* flags, int* bnd, u8* ops, LeafOut* out)
{
    __shared__ ulonglong2 tile[kLanes * 2];
    const LeafTask T = tasks[blockIdx.x];
    const int lane = (int)(threadIdx.x & 63);
    LeafOut o; o.cnt = 0; o.fail = 0;
    if (T.m == 0 || T.n == 0) {          // NwPath::solve: one run of deletes / inserts
        const int len = T.m + T.n;
        for (int i = lane; i < len; i += kLanes) ops[T.ops_end - 1 - (u64)i] = T.m == 0 ? 2 : 1;
        o.cnt = len; o.fail = len != T.best ? 2 : 0;
    } else {
        int fail = 0, last = 0;
        wave_pass<true>(qbases, tbases, T.q, T.t, T.m, T.n, T.bd, bnd + T.bnd_off, flags + T.flag_off, T.W, &fail, nullptr, &last);
        __threadfence();
        __syncthreads();
        TileMat mat; mat.flags = flags + T.flag_off; mat.tile = tile; mat.bd = T.bd; mat.W = T.W; mat.lane = lane; mat.c_top = INT_MIN / 2; mat.b_top = INT_MIN / 2;
        OpsSink sink; sink.end = ops + T.ops_end; sink.store = lane == 0;
        int cost = 0;
        o.cnt = walk_leaf(T.m, T.n, mat, sink, &cost);
        // the self-check: every flag was there, the path costs what the level above said it would (and it consumed m rows and n columns by construction)
        o.fail = __ballot(fail != 0) ? 1 : (o.cnt < 0 ? 1 : (cost != T.best ? 2 : 0));
    }
    if (lane == 0) out[blockIdx.x] = o;
}

__global__ __launch_bounds__(64) void k_nw_finish(const FinTask* tasks, const LeafOut* leaf_out, const u64* leaf_end, u8* ops, u8* pack, FinOut* out)
{
    const FinTask T = tasks[blockIdx.x];
    const int lane = (int)(threadIdx.x & 63);
    FinOut o; o.ok = 0; o.pq = o.pt = o.tq = o.tt = o.asz = o.same = 0; o.fail = T.bad ? 1 : 0;
    i64 len = 0;
    for (u32 l = T.leaf_begin; l < T.leaf_end && !o.fail; ++l) { const LeafOut lo = leaf_out[l]; if (lo.fail || lo.cnt < 0) o.fail = 1; len += lo.cnt; }
    if (len != 0 && len > (i64)T.m + T.n) o.fail = 1;
    if (!o.fail) {
        u8* P = ops + T.ops_base;
        // the leaves' ops, each written right-aligned in its own stretch, moved together (towards the front: a destination never passes its source)
        i64 dst = 0;
        for (u32 l = T.leaf_begin; l < T.leaf_end; ++l) {
            const int cnt = leaf_out[l].cnt;
            const u8* src = ops + (leaf_end[l] - (u64)cnt);
            for (int i = lane; i - lane < cnt; i += kLanes) {
                const u8 v = i < cnt ? src[i] : (u8)0;
                if (i < cnt) P[dst + i] = v;
            }
            dst += cnt;
        }
        __threadfence();
        __syncthreads();
        const int ms = T.match_size;
        i64 e = -1, sb = -1;
        for (i64 base = 0; base < len; base += kLanes) {
            const u64 mask = __ballot(run_ends_at(P, len, base + lane, ms));
            if (mask) { e = base + ctz64(mask); break; }
        }
        if (e >= 0) {
            for (i64 top = len - ms; top >= 0; top -= kLanes) {
                const u64 mask = __ballot(run_starts_at(P, len, top - lane, ms));
                if (mask) { sb = top - ctz64(mask); break; }
            }
        }
        if (e >= 0 && sb >= 0) {
            const i64 from = e + 1 - ms, to = sb + ms;
            int pq = 0, pt = 0, tq = 0, tt = 0, same = 0;
            for (i64 i = lane; i < from; i += kLanes) { const int op = P[i]; pq += op != 2; pt += op != 1; }
            for (i64 i = to + lane; i < len; i += kLanes) { const int op = P[i]; tq += op != 2; tt += op != 1; }
            for (i64 i = from + lane; i < to; i += kLanes) same += P[i] == 0;
            o.ok = 1; o.pq = wave_sum(pq); o.pt = wave_sum(pt); o.tq = wave_sum(tq); o.tt = wave_sum(tt); o.same = wave_sum(same);
            o.asz = (int)(to - from);
            const i64 nbytes = (to - from + 3) / 4;
            for (i64 j = lane; j < nbytes; j += kLanes) {
                int v = 0;
                for (int k = 0; k < 4; ++k) { const i64 at = from + 4 * j + k; if (at < to) v |= (P[at] & 3) << (2 * k); }
                pack[T.pack_off + (u64)j] = (u8)v;
            }
        }
    }
    if (lane == 0) out[blockIdx.x] = o;
}

}  // namespace nw
}  // namespace necat
