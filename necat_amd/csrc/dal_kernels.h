// dal_kernels.h - the __global__ shell around dal_core.h: one wave (a workgroup of 64) per direction of a job.
//   k_dal_wave   block 2 j: the forward wave of job j, block 2 j + 1: its reverse wave - wave 0, then steps until the host loop's condition ends them; writes the
//                tip, its difference count and a flag (window above the capacity, a read of a diagonal without history, an empty window)
// The diagonals' state is in dynamic LDS (dal::Ring: two copies of R entries of T, V, M = 32 R bytes), so the capacity is a launch argument.
#pragma once
#include "dal_core.h"

namespace necat {
namespace dal {

// The best of lanes 0 .. l - 1 in lane l (worst<DIR>() in lane 0), by DPP moves as wave_scan_add (dev_common.h): Kogge-Stone inside the rows of 16 (row_shr 1, 2,
// 4, 8), lane 15 of a row into the next row (rows 1 and 3), lane 31 into rows 2 and 3, then one lane down the wave (wave_shr 1).  A lane without a source keeps
// the move's `old` operand, the identity worst<DIR>().
template <int DIR, int CTRL, int ROWS>
NECAT_D int take_best(int x)
{
    const int t = __builtin_amdgcn_update_dpp(worst<DIR>(), x, CTRL, ROWS, 0xf, false);
    return better<DIR>(t, x) ? t : x;
}
template <int DIR>
NECAT_D int wave_best_before(int v)
{
    v = take_best<DIR, 0x111, 0xf>(v);
    v = take_best<DIR, 0x112, 0xf>(v);
    v = take_best<DIR, 0x114, 0xf>(v);
    v = take_best<DIR, 0x118, 0xf>(v);
    v = take_best<DIR, 0x142, 0xa>(v);
    v = take_best<DIR, 0x143, 0xc>(v);
    return __builtin_amdgcn_update_dpp(worst<DIR>(), v, 0x138, 0xf, 0xf, false);
}

template <int DIR>
__device__ void wave_dir(const u64* abases, const u64* bbases, const Task& T, const Spec& S, const int cap, const Ring& W, Out* out)
{
    const int lane = (int)(threadIdx.x & 63);
    Fold F;
    wave0<DIR>(F, W, abases, bbases, T);          // wave-uniform: every lane stores the same point
    __syncthreads();
    if (!F.more) clip<DIR>(F, W, 0, abases, bbases, T);
    int cur = 0, flag = 0, steps = 0, max_diags = 1;
    while (goes_on<DIR>(F)) {
        const int ol = F.low, oh = F.hgh;
        flag = step_begin(F, cap, T);
        if (flag & (kFlagEmpty | kFlagStale)) break;
        const int w = F.hgh - F.low + 1;
        if (w > max_diags) max_diags = w;
        if (flag) break;
        const int nw = cur ^ 1;
        u64 stale = 0;
        for (int base = 0; base < w; base += kLanes) {
            const int k_first = DIR > 0 ? F.hgh - base : F.low + base;
            const int k = k_first - DIR * lane;
            const bool active = base + lane < w;
            LaneOut o = lane_idle<DIR>();
            if (active) { o = lane_point<DIR>(W, cur, ol, oh, k, abases, bbases, T); lane_store(W, nw, k, o); }
            int run = wave_best_before<DIR>(o.c);
            if (!better<DIR>(run, F.besta)) run = F.besta;
            const int cls = active ? lane_class<DIR>(S, o, run) : 0;
            const u64 rec = __ballot(cls & kRecord), good = __ballot(cls & kGood), trim = __ballot(cls & kTrim);
            const u64 hit_a = __ballot(o.flags & kHitA), hit_b = __ballot(o.flags & kHitB);
            stale |= __ballot(o.flags & kStale);
            fold_chunk<DIR>(F, k_first, rec, good, trim, hit_a, hit_b, [&](int l, int* c, int* y) { *c = __shfl(o.c, l); *y = __shfl(o.y, l); });
        }
        __syncthreads();
        if (stale) { flag = kFlagStale; break; }
        if (!F.more) clip<DIR>(F, W, nw, abases, bbases, T);
        if (F.hgh >= F.low) {
            int lo = INT_MAX, hi = INT_MIN;
            for (int base = F.low; base <= F.hgh; base += kLanes) {
                const int k = base + lane;
                const u64 stay = __ballot(k <= F.hgh && lane_stays<DIR>(F, W.V[W.at(nw, k)]));
                if (stay) { if (lo == INT_MAX) lo = base + ctz64(stay); hi = base + last_lane(stay); }
            }
            lag_trim(F, lo, hi);
        }
        cur = nw;
        ++steps;
    }
    if (lane == 0) {
        const Tip t = tip_of(F);
        Out o; o.a = t.a; o.y = t.y; o.d = t.d; o.flag = flag; o.steps = steps; o.max_diags = max_diags;
        *out = o;
    }
}

__global__ __launch_bounds__(64) void k_dal_wave(const u64* abases, const u64* bbases, const Task* tasks, const Spec S, const int cap, const int R, Out* out)
{
    extern __shared__ __attribute__((aligned(16))) char dal_lds[];
    Ring W; W.T = (u64*)dal_lds; W.V = (int*)(dal_lds + (size_t)16 * R); W.M = W.V + 2 * R; W.mask = R - 1;
    const Task T = tasks[blockIdx.x >> 1];
    if (blockIdx.x & 1) wave_dir<-1>(abases, bbases, T, S, cap, W, out + blockIdx.x);
    else wave_dir<+1>(abases, bbases, T, S, cap, W, out + blockIdx.x);
}

}  // namespace dal
}  // namespace necat
