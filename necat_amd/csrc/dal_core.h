// dal_core.h - DALIGNER's local alignment around an anchor (rescue::local_alignment, rescue.h:57-194; forward_wave / reverse_wave, gapped_align/align.c:382, :1043)
// for the device: the per-lane core of a wave step and the wave-uniform bookkeeping around it, written so that g++ builds the same functions for a CPU model
// that runs them lane by lane (tests/host_core/check_dalign.cpp).
//
// One WAVE owns one direction of one job.  A wave step (dif += 1) gives every diagonal k of the window [low, hgh] a new furthest point from the PREVIOUS
// step's points of k + DIR, k and k - DIR, so a lane per diagonal computes it alone (lane_point); windows wider than 64 go in chunks of 64 lanes in sweep
// order (downwards in k going forward, upwards in reverse).  The per-diagonal state (V, M, T) lives in an LDS ring addressed by k & (R - 1), once per parity
// of the step: a step reads one copy and writes the other, so no lane reads what another lane of the same step has written, and a diagonal outside the
// previous step's window is "no point" by a bounds test, never by what the ring holds.  What the host's sweep does in order - the running best (besta /
// besty), lasta, the trimmed tip, the sentinel clips - is a prefix maximum over the lanes plus "last lane of a mask" (fold_chunk); clip() and the WAVE_LAG
// trim are wave-uniform.  `org` (the diagonal a path started on) is not carried: ocda_go starts the wave on one diagonal, so it is that diagonal for every
// point - unless a step reads the history of a diagonal the direction never wrote, which needs an empty window at the head of a step; both are detected
// and flag the job for the host code (kFlagStale, kFlagEmpty).  NECAT_DAL_TRACK_ORG (the CPU model) carries org all the same, to assert exactly that.
#pragma once
#include <limits.h>

#include "nw_core.h"

namespace necat {
namespace dal {

constexpr int kLanes = 64;
constexpr int kTrimLen = 15, kPathLen = 60;                            // rescue.h:24-26
constexpr u64 kPathTop = 1ULL << kPathLen, kPathInt = kPathTop - 1;
constexpr int kTrimMask = (1 << kTrimLen) - 1, kTrimMlag = 200, kWaveLag = 30;
constexpr int kMaxDiags = 2048;                                        // NECAT_DALIGN_DIAGS at most: 2 copies x 16 bytes x 2048 = the 64 KB of LDS a workgroup may ask for
enum { kFlagOverCap = 1, kFlagStale = 2, kFlagEmpty = 4 };
enum { kHitA = 1, kHitB = 2, kStale = 4 };                             // LaneOut::flags
enum { kRecord = 1, kGood = 2, kTrim = 4 };                            // lane_class

// a sequence with its sentinels: element i in [0, len) as nw::Seq says, 4 outside
struct DSeq { nw::Seq s; int len; };
// the 32-base word a lane read last (a slide walks along one diagonal: most of its bases come from the same word)
struct WordCache { i64 w; u64 v; };
NECAT_HD int seq_at(const u64* bases, const DSeq& s, int i, WordCache& wc)
{
    if (i < 0 || i >= s.len) return 4;
    const i64 g = s.s.g0 + (i64)s.s.dir * i, w = g >> 5;
    if (w != wc.w) { wc.w = w; wc.v = bases[w]; }
    const int c = (int)((wc.v >> ((g & 31) * 2)) & 3);
    return s.s.comp ? 3 - c : c;
}

// the word of position i ahead of its use (no-op outside the sequence): a slide starts by asking for both sequences' words, so the two loads are in flight together
NECAT_HD void seq_prime(const u64* bases, const DSeq& s, int i, WordCache& wc)
{
    if (i < 0 || i >= s.len) return;
    const i64 w = (s.s.g0 + (i64)s.s.dir * i) >> 5;
    wc.w = w; wc.v = bases[w];
}

// New_Align_Spec's numbers (rescue::make_spec on the host, uploaded once per error): table / score have kTrimMask + 1 entries
struct Spec { int ave_path; const i16* table; const i16* score; };

// one direction of one job.  a: the query on its strand, b: the subject; k0 = query_start - subject_start, mida = their sum
struct Task { DSeq a, b; int k0, mida; };
struct Tip { int a, y, d; };
struct Out { int a, y, d, flag, steps, max_diags; };

// the diagonals' state, two copies of R (a power of two) entries each
struct Ring {
    int* V; int* M; u64* T; int mask;
#ifdef NECAT_DAL_TRACK_ORG
    int* O;
#endif
    NECAT_HD int at(int copy, int k) const { return copy * (mask + 1) + (k & mask); }
};
NECAT_HD size_t ring_bytes(int R) { return (size_t)R * 2 * 16; }
NECAT_HD int ring_size(int cap) { int R = 16; while (R < cap) R <<= 1; return R; }

template <int DIR> NECAT_HD bool better(int x, int y) { return DIR > 0 ? x > y : x < y; }      // x is further along than y
template <int DIR> NECAT_HD int none() { return DIR > 0 ? -1 : INT_MAX; }                     // "no point yet"
template <int DIR> NECAT_HD int worst() { return DIR > 0 ? INT_MIN : INT_MAX; }               // what an idle lane reports: never a record

// the wave-uniform state of a direction
struct Fold {
    int low, hgh, dif, more, aclip, bclip, besta, besty, lasta, morem;
    Tip trim, mor;
};
template <int DIR> NECAT_HD void clips_reset(Fold& F) { F.aclip = DIR > 0 ? INT_MAX : -INT_MAX; F.bclip = DIR > 0 ? -INT_MAX : INT_MAX; }

struct LaneOut { int c, y, m, flags; u64 b;
#ifdef NECAT_DAL_TRACK_ORG
    int o;
#endif
};

// the slide along diagonal k from (y + k, y) while the bases agree; going backwards the bases BEFORE a position are compared
template <int DIR, bool HISTORY>
NECAT_HD int slide(const u64* abases, const u64* bbases, const Task& T, int k, int& y, int& m, u64& b)
{
    const int off = DIR > 0 ? 0 : -1;
    WordCache wa, wb; wa.w = wb.w = LLONG_MIN; wa.v = wb.v = 0;
    seq_prime(bbases, T.b, y + off, wb);
    seq_prime(abases, T.a, k + y + off, wa);
    for (;;) {
        const int c = seq_at(bbases, T.b, y + off, wb);
        if (c == 4) return kHitB;
        const int d = seq_at(abases, T.a, k + y + off, wa);
        if (c != d) return d == 4 ? kHitA : 0;
        y += DIR;
        if (HISTORY) { if ((b & kPathTop) == 0) m += 1; b = (b << 1) | 1; }
    }
}

// Diagonal k's point of step F.dif from the copy `cur` of the ring, which holds the previous step's window [ol, oh] (rescue.h:141-155)
template <int DIR>
NECAT_HD LaneOut lane_point(const Ring& W, int cur, int ol, int oh, int k, const u64* abases, const u64* bbases, const Task& T)
{
    const int kNone = none<DIR>();
    const int kp = k + DIR, kn = k - DIR;
    const int prev_v = kp >= ol && kp <= oh ? W.V[W.at(cur, kp)] : kNone;
    const int ac = k >= ol && k <= oh ? W.V[W.at(cur, k)] : kNone;
    const int nxt = kn >= ol && kn <= oh ? W.V[W.at(cur, kn)] : kNone;
    LaneOut o; o.flags = 0;
    int c, s;
    const bool use_prev = better<DIR>(nxt, ac) ? better<DIR>(prev_v, nxt) : better<DIR>(prev_v, ac);
    if (use_prev) { c = prev_v + DIR; s = kp; }
    else if (better<DIR>(nxt, ac)) { c = nxt + DIR; s = kn; }
    else { c = ac + 2 * DIR; s = k; }
    if (s == k && ac == kNone) {      // the history of a diagonal this direction never wrote: the job is the host's, the lane idles
        o.c = worst<DIR>(); o.y = 0; o.m = 0; o.b = 0; o.flags = kStale;
#ifdef NECAT_DAL_TRACK_ORG
        o.o = 0;
#endif
        return o;
    }
    int m = W.M[W.at(cur, s)];
    u64 b = W.T[W.at(cur, s)];
#ifdef NECAT_DAL_TRACK_ORG
    o.o = W.O[W.at(cur, s)];
#endif
    if (b & kPathTop) m -= 1;
    b <<= 1;
    int y = (c - k) >> 1;
    o.flags |= slide<DIR, true>(abases, bbases, T, k, y, m, b);
    o.c = (y << 1) + k; o.y = y; o.m = m; o.b = b;
    return o;
}
NECAT_HD void lane_store(const Ring& W, int nxt, int k, const LaneOut& o)
{
    const int at = W.at(nxt, k);
    W.V[at] = o.c; W.M[at] = o.m; W.T[at] = o.b;
#ifdef NECAT_DAL_TRACK_ORG
    W.O[at] = o.o;
#endif
}
template <int DIR> NECAT_HD LaneOut lane_idle() { LaneOut o = LaneOut(); o.c = worst<DIR>(); return o; }

// What the sweep does with the point (rescue.h:156-162).  `run`: the best point of the lanes before this one in sweep order and of the steps before.
template <int DIR>
NECAT_HD int lane_class(const Spec& S, const LaneOut& o, int run)
{
    if (!better<DIR>(o.c, run)) return 0;
    if (o.m < S.ave_path) return kRecord;
    const int w0 = (int)(o.b & kTrimMask), w1 = (int)((o.b >> kTrimLen) & kTrimMask);
    return S.table[w0] >= 0 && S.table[w1] + S.score[w0] >= 0 ? kRecord | kGood | kTrim : kRecord | kGood;
}

NECAT_HD int last_lane(u64 mask) { return 63 - __builtin_clzll(mask); }      // mask != 0

// A chunk of 64 lanes folded into the direction's state: lane l is sweep position l of the chunk, on diagonal k_first - DIR * l.  The masks are the lanes'
// lane_class bits and hit flags; get(lane, &c, &y) reads a lane's point.  Records are in sweep order, so "the last one" is the highest lane of a mask.
template <int DIR, class Get>
NECAT_HD void fold_chunk(Fold& F, int k_first, u64 rec, u64 good, u64 trim, u64 hit_a, u64 hit_b, Get get)
{
    int c, y;
    if (rec) { get(last_lane(rec), &c, &y); F.besta = c; F.besty = y; }
    if (good) { get(last_lane(good), &c, &y); F.lasta = c; }
    if (trim) { get(last_lane(trim), &c, &y); F.trim.a = c; F.trim.y = y; F.trim.d = F.dif; }
    if (hit_a | hit_b) F.more = 0;
    if (hit_a) F.aclip = k_first - DIR * last_lane(hit_a);                       // the last one the sweep meets
    if (hit_b) {                                                                // the extreme one: the first the sweep meets
        const int k = k_first - DIR * ctz64(hit_b);
        if (DIR > 0 ? F.bclip < k : F.bclip > k) F.bclip = k;
    }
}

// rescue.h:99-111: a diagonal that ran into a sequence end leaves the wave; the best such point is remembered.  `nw`: the copy the step wrote.
template <int DIR>
NECAT_HD void clip(Fold& F, const Ring& W, int nw, const u64* abases, const u64* bbases, const Task& T)
{
    const int off = DIR > 0 ? 0 : -1;
    WordCache wa, wb; wa.w = wb.w = LLONG_MIN; wa.v = wb.v = 0;
    if (seq_at(bbases, T.b, F.besty + off, wb) != 4 && seq_at(abases, T.a, F.besta - F.besty + off, wa) != 4) F.more = 1;
    const bool a_hit = DIR > 0 ? F.hgh >= F.aclip : F.low <= F.aclip, b_hit = DIR > 0 ? F.low <= F.bclip : F.hgh >= F.bclip;
    if (a_hit) {
        if (DIR > 0) F.hgh = F.aclip - 1; else F.low = F.aclip + 1;
        const int at = W.at(nw, F.aclip);
        if (F.morem <= W.M[at]) { F.morem = W.M[at]; F.mor.a = W.V[at]; F.mor.y = (F.mor.a - F.aclip) / 2; F.mor.d = F.dif; }
    }
    if (b_hit) {
        if (DIR > 0) F.low = F.bclip + 1; else F.hgh = F.bclip - 1;
        const int at = W.at(nw, F.bclip);
        if (F.morem <= W.M[at]) { F.morem = W.M[at]; F.mor.a = W.V[at]; F.mor.y = (F.mor.a - F.bclip) / 2; F.mor.d = F.dif; }
    }
    clips_reset<DIR>(F);
}

// wave 0: the snake from the anchor on its one diagonal (rescue.h:113-122 with low == hgh); the ring's copy 0 takes the point.  Wave-uniform.
template <int DIR>
NECAT_HD void wave0(Fold& F, const Ring& W, const u64* abases, const u64* bbases, const Task& T)
{
    const int k = T.k0;
    F.low = F.hgh = k; F.dif = 0; F.more = 1; F.morem = -1;
    clips_reset<DIR>(F);
    F.besta = F.lasta = T.mida; F.besty = (T.mida - k) >> 1;
    F.trim.a = F.mor.a = T.mida; F.trim.y = F.mor.y = F.besty; F.trim.d = F.mor.d = 0;
    int y = F.besty, m = 0; u64 b = 0;
    const int hit = slide<DIR, false>(abases, bbases, T, k, y, m, b);
    if (hit) F.more = 0;
    if (hit & kHitA) F.aclip = k;
    if (hit & kHitB) F.bclip = k;
    const int c = (y << 1) + k;
    if (better<DIR>(c, F.besta)) { F.besta = F.trim.a = F.lasta = c; F.besty = F.trim.y = y; }
    LaneOut o; o.c = c; o.y = y; o.m = kPathLen; o.b = kPathInt; o.flags = 0;
#ifdef NECAT_DAL_TRACK_ORG
    o.o = k;
#endif
    lane_store(W, 0, k, o);
}

// the host loop's condition (rescue.h:124)
template <int DIR> NECAT_HD bool goes_on(const Fold& F) { return F.more && (DIR > 0 ? F.lasta >= F.besta - kTrimMlag : F.lasta <= F.besta + kTrimMlag); }

// The head of a step: the window grows by one diagonal on either side (minp / maxp are out of reach in ocda_go's call).  Returns a flag when the step
// cannot be taken here: an empty window (every read of the step would be of a diagonal without a point) or one wider than the ring holds.  Every step
// moves the best point at least one anti-diagonal on, so a direction takes at most alen + blen steps: more would be a bug, and ends the job the same way.
NECAT_HD int step_begin(Fold& F, int cap, const Task& T)
{
    if (F.hgh < F.low) return kFlagEmpty;
    if (F.dif > T.a.len + T.b.len) return kFlagStale;
    F.low -= 1; F.hgh += 1; F.dif += 1;
    return F.hgh - F.low + 1 > cap ? kFlagOverCap : 0;
}

// points more than WAVE_LAG behind the best one leave the wave (rescue.h:167-172): does diagonal k's stay?
template <int DIR> NECAT_HD bool lane_stays(const Fold& F, int v) { return !better<DIR>(F.besta - DIR * kWaveLag, v); }
// .. given the lowest and the highest diagonal that stay (lo > hi: none).  The host takes hgh down first and only then low up: with nothing left, low stays.
NECAT_HD void lag_trim(Fold& F, int lo, int hi)
{
    if (lo > hi) { F.hgh = F.low - 1; return; }
    F.low = lo; F.hgh = hi;
}

NECAT_HD Tip tip_of(const Fold& F) { return F.morem >= 0 ? F.mor : F.trim; }

}  // namespace dal
}  // namespace necat
