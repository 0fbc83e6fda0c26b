// check_item_order.cpp - TEST ONLY.  The size-class order of a round's ragged blocks (necat_amd/csrc/item_order.h) replayed on the CPU: the appends
// (ext_append_block_wg: a slot from the list's counter, the item to the staging array, the class counted once per workgroup and class) and the round-start kernel
// (k_round_ctl: class scan, slices of 256 staged items, one cursor reservation per workgroup and class, scatter) with the header's own class / slot functions, the
// workgroups' reservations in a shuffled order.  Checked per case: the lists are a permutation of what was appended, the order keys never decrease along the work
// index, list A's full front and everything between it and the ragged back are untouched, and the lane-steps a consumer issues - groups of 4, 8 and 64
// neighbouring work items, each run for its longest member's steps - exceed the steps needed by at most
//     31 x blocks + classes x group size x the longest block's steps
// (within a class blocks differ by fewer than 32 columns; one group may straddle each class boundary, and list A's first ragged group may hold full blocks).
// g++ -std=c++17 [-fsanitize=address,undefined]; no arguments.  Prints "check_item_order: ok cases=N".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "item_order.h"
using namespace necat;

namespace {

struct Item { int task, qn, tn; };                       // (task: unique per case; -1 = never written)
constexpr int kWg = 256;                                 // threads of an appending workgroup and of a k_round_ctl workgroup
constexpr int kFull = 512;

struct Rng { unsigned long long s; unsigned next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(s >> 33); } };

struct ListBuf {
    u32 cap; u32 count[3] = {0, 0, 0};                   // [0] full list-A blocks, [1] list B, [2] ragged list-A blocks
    std::vector<Item> itemsA, itemsB, stage; std::vector<u32> cls;
    explicit ListBuf(u32 cap_) : cap(cap_), itemsA(cap_, Item{-1, 0, 0}), itemsB(cap_, Item{-1, 0, 0}), stage(cap_, Item{-1, 0, 0}), cls(2 * kItemClsWords, 0u) {}
};

// one appending workgroup: its threads' blocks (list: 0 = full, 1 = list B, 2 = ragged list A, as the counters are numbered)
void append_wg(ListBuf& L, const std::vector<Item>& its)
{
    u32 tot[3] = {0, 0, 0}, ccnt[2 * kItemClasses] = {0};
    auto list_of = [](const Item& it) { return it.qn <= kFull && it.tn <= kFull ? (it.qn == kFull && it.tn == kFull ? 0 : 2) : 1; };
    for (const Item& it : its) ++tot[list_of(it)];
    u32 base[3];
    for (int l = 0; l < 3; ++l) { base[l] = L.count[l]; L.count[l] += tot[l]; }          // ONE reservation per workgroup and list
    u32 at[3] = {0, 0, 0};
    for (const Item& it : its) {
        const int l = list_of(it);
        const u32 slot = base[l] + at[l]++;
        if (l == 0) L.itemsA[slot] = it;
        else {
            L.stage[item_stage_slot(l == 1, L.cap, slot)] = it;
            ++ccnt[(l == 1 ? kItemClasses : 0) + item_order_key(it.tn)];
        }
    }
    for (int k = 0; k < 2 * kItemClasses; ++k) if (ccnt[k]) *item_cls_count(L.cls.data(), k / kItemClasses, k % kItemClasses) += ccnt[k];
}

// k_round_ctl's ordering part with `grid` workgroups; the (workgroup, slice) turns run in a shuffled order - every turn's cursor reservations at once, as one
// workgroup's atomics may fall anywhere among the others'
void round_ctl(ListBuf& L, u32 grid, Rng& rng)
{
    const u32 np = L.count[2], nB = L.count[1], total = np + nB;
    u32 base[2 * kItemClasses];
    for (int k = 0; k < 2 * kItemClasses; ++k) base[k] = item_order_base(L.cls.data(), k / kItemClasses, k % kItemClasses);
    std::vector<u32> turns;
    for (u32 wg = 0; wg < grid; ++wg) for (u32 first = wg * kWg; first < total; first += grid * kWg) turns.push_back(first);
    for (size_t i = turns.size(); i > 1; --i) std::swap(turns[i - 1], turns[rng.next() % i]);
    for (u32 first : turns) {
        u32 cnt[2 * kItemClasses] = {0}, got[2 * kItemClasses], rk[kWg]; int key[kWg];
        for (u32 t = 0; t < (u32)kWg && first + t < total; ++t) {
            const u32 i = first + t; const int list = i >= np;
            const Item& it = L.stage[item_stage_slot(list, L.cap, list ? i - np : i)];
            key[t] = list * kItemClasses + item_order_key(it.tn);
            rk[t] = cnt[key[t]]++;
        }
        for (int k = 0; k < 2 * kItemClasses; ++k) { u32* cur = item_cls_cursor(L.cls.data(), k / kItemClasses, k % kItemClasses); got[k] = *cur; *cur += cnt[k]; }
        for (u32 t = 0; t < (u32)kWg && first + t < total; ++t) {
            const u32 i = first + t; const int list = i >= np;
            const u32 j = base[key[t]] + got[key[t]] + rk[t];
            if (j >= (list ? nB : np)) { printf("ERROR: rank %u of %u\n", j, list ? nB : np); exit(1); }
            (list ? L.itemsB : L.itemsA)[item_final_slot(list, L.cap, j)] = L.stage[item_stage_slot(list, L.cap, list ? i - np : i)];
        }
    }
}

int steps_of(const Item& it) { return it.tn + (it.qn + 63) / 64 - 1; }

// issued - needed over groups of g neighbouring work items of `v` (work index of v[0] = w0; a group = the work indices of one multiple of g; `lead` = steps of the
// items before v[0] that share its group: list A's full blocks)
bool bound_holds(const std::vector<Item>& v, u32 w0, int g, const char* what, int casei)
{
    unsigned long long issued = 0, needed = 0; int longest = 0; bool seen[kItemClasses] = {false}; int classes = 0;
    for (const Item& it : v) { longest = std::max(longest, steps_of(it)); if (!seen[item_class(it.tn)]) { seen[item_class(it.tn)] = true; ++classes; } }
    if (w0 % g) longest = std::max(longest, kFull + kFull / 64 - 1);
    for (size_t i = 0; i < v.size();) {
        const u64 grp = (w0 + i) / g; size_t e = i; int mx = (i == 0 && w0 % g) ? kFull + kFull / 64 - 1 : 0;
        while (e < v.size() && (w0 + e) / g == grp) { mx = std::max(mx, steps_of(v[e])); ++e; }
        for (size_t q = i; q < e; ++q) needed += steps_of(v[q]);
        issued += (unsigned long long)(e - i) * mx;
        i = e;
    }
    const unsigned long long slack = 31ULL * v.size() + (unsigned long long)classes * g * longest;
    if (issued - needed > slack) { printf("ERROR: case %d %s groups of %d: issued %llu needed %llu, above the bound by %llu\n", casei, what, g, issued, needed, issued - needed - slack); return false; }
    return true;
}

const int kTnA[] = {1, 32, 33, 511, 512}, kTnB[] = {513, 544, 545, 794};

// pattern: 0 .. = every item the p-th size; then alternating extremes, round robin over the sizes, random sizes (any tn of the list, qn anywhere it may be)
Item make_item(int task, bool listB, int pattern, int i, Rng& rng)
{
    const int* tns = listB ? kTnB : kTnA; const int n = listB ? 4 : 5;
    int tn, qn;
    if (pattern < n) tn = tns[pattern];
    else if (pattern == n) tn = (i & 1) ? tns[n - 1] : tns[0];
    else if (pattern == n + 1) tn = tns[i % n];
    else tn = listB ? 513 + (int)(rng.next() % 282) : 1 + (int)(rng.next() % 512);
    qn = tn;
    if (pattern == n + 2 && !listB) { qn = 1 + (int)(rng.next() % 512); if (qn == kFull && tn == kFull) qn = 511; }
    if (tn == kFull && qn == kFull) qn = 511;             // (512 x 512 is a full block: the ragged one of that class is 511 x 512)
    return Item{task, qn, tn};
}

}  // namespace

int main()
{
    const u32 sizes[] = {0, 1, 15, 16, 17, 63, 64, 65, 5000};
    const u32 fulls[] = {0, 5, 16, 37};
    const u32 grids[] = {1, 3, 8};
    Rng rng{12345};
    int cases = 0;
    for (u32 np : sizes) for (u32 nB : sizes) for (int pat = 0; pat < 8; ++pat) {
        const u32 nf = fulls[cases % 4], grid = grids[cases % 3];
        const u32 cap = ((nf + np + nB + 63) & ~63u) + 64;
        ListBuf L(cap);
        // what the previous round's finishing kernel appends: the blocks in task order, dealt to workgroups of 256 threads whose reservations fall in a shuffled order
        std::vector<Item> all; int task = 0;
        for (u32 i = 0; i < nf; ++i) all.push_back(Item{task++, kFull, kFull});
        for (u32 i = 0; i < np; ++i) all.push_back(make_item(task++, false, std::min(pat, 7), (int)i, rng));
        for (u32 i = 0; i < nB; ++i) all.push_back(make_item(task++, true, std::min(pat, 6), (int)i, rng));
        for (size_t i = all.size(); i > 1; --i) std::swap(all[i - 1], all[rng.next() % i]);
        std::vector<std::vector<Item>> wgs;
        for (size_t i = 0; i < all.size(); i += kWg) wgs.emplace_back(all.begin() + i, all.begin() + std::min(all.size(), i + kWg));
        for (size_t i = wgs.size(); i > 1; --i) std::swap(wgs[i - 1], wgs[rng.next() % i]);
        for (const auto& w : wgs) append_wg(L, w);
        if (L.count[0] != nf || L.count[1] != nB || L.count[2] != np) { printf("ERROR: case %d counts\n", cases); return 1; }
        const std::vector<Item> frontA(L.itemsA.begin(), L.itemsA.begin() + nf);
        round_ctl(L, grid, rng);
        // ---- the lists: a permutation, keys in order, the rest untouched
        std::vector<char> seen(all.size(), 0);
        for (u32 i = 0; i < nf; ++i) if (L.itemsA[i].task != frontA[i].task || L.itemsA[i].tn != kFull || L.itemsA[i].qn != kFull) { printf("ERROR: case %d full front moved at %u\n", cases, i); return 1; }
        for (u32 i = nf; i < cap - np; ++i) if (L.itemsA[i].task != -1) { printf("ERROR: case %d itemsA[%u] between the front and the back written\n", cases, i); return 1; }
        for (u32 i = nB; i < cap; ++i) if (L.itemsB[i].task != -1) { printf("ERROR: case %d itemsB[%u] beyond the list written\n", cases, i); return 1; }
        std::vector<Item> ragged, listb;
        for (u32 j = 0; j < np; ++j) ragged.push_back(L.itemsA[item_final_slot(0, cap, j)]);
        for (u32 j = 0; j < nB; ++j) listb.push_back(L.itemsB[item_final_slot(1, cap, j)]);
        for (u32 i = 0; i < nf; ++i) seen[L.itemsA[i].task] = 1;
        for (const auto* v : {&ragged, &listb}) {
            int last = -1;
            for (const Item& it : *v) {
                if (it.task < 0 || (size_t)it.task >= seen.size() || seen[it.task]) { printf("ERROR: case %d item missing or twice\n", cases); return 1; }
                seen[it.task] = 1;
                const bool isB = v == &listb;
                if ((it.qn <= kFull && it.tn <= kFull) == isB) { printf("ERROR: case %d item in the wrong list\n", cases); return 1; }
                const int key = item_order_key(it.tn);
                if (key < last) { printf("ERROR: case %d class order broken\n", cases); return 1; }
                last = key;
            }
        }
        for (const Item& it : all) if (!seen[it.task]) { printf("ERROR: case %d task %d lost\n", cases, it.task); return 1; }
        // the cursors ran to the counts
        for (int k = 0; k < 2 * kItemClasses; ++k) if (*item_cls_cursor(L.cls.data(), k / kItemClasses, k % kItemClasses) != *item_cls_count(L.cls.data(), k / kItemClasses, k % kItemClasses)) { printf("ERROR: case %d cursor\n", cases); return 1; }
        // ---- the bound (the patterns whose blocks have qn = tn: a class's blocks then have one word count, as the bound assumes)
        if (pat != 7) {
            const u32 nf16 = (nf + 15) & ~15u;
            for (int g : {4, 8, 64}) if (!bound_holds(ragged, nf16, g, "list A", cases) || !bound_holds(listb, 0, g, "list B", cases)) return 1;
        }
        ++cases;
    }
    // the class function at its edges
    if (item_class(1) != 0 || item_class(32) != 0 || item_class(33) != 1 || item_class(512) != 15 || item_class(513) != 16 || item_class(794) != 24 || item_class(4000) != kItemClasses - 1 ||
        item_order_key(794) >= item_order_key(513) || item_order_key(512) >= item_order_key(1)) { printf("ERROR: class function\n"); return 1; }
    printf("check_item_order: ok cases=%d\n", cases);
    return 0;
}
