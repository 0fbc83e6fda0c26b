// item_order.h - the size-class order of a round's ragged blocks: the class of a block, the counters the appends keep per class, and where the
// round-start kernel (k_round_ctl, ext_tail.h) puts a staged item.  Host and device: tests/host_core/check_item_order.cpp replays the same functions.
//
// Every consumer of a round's lists runs a group of neighbouring work items - the 8 blocks of a ragged wave of k_myers_ck, the 4 of a wave of k_myers_ckf, the 64 of
// a walk workgroup - for as long as the group's longest block needs, and a block needs tn + nblk - 1 steps.  The non-full blocks of list A and all of list B are
// last blocks of extensions, of any size; appended as they come, a group's maximum is far above its mean.  So those items are appended to a STAGING array of their
// list buffer, the appends count them per size class, and the first kernel of the round scatters them to their final places class by class, longest class first:
// the blocks of a group then differ by fewer than kItemClassCols columns (but for the one group that may straddle each class boundary).  The order inside a class is
// whatever the atomics give - as the whole list's order was before.  A block's result does not depend on its work index.
#pragma once
#include "dev_common.h"

namespace necat {

constexpr int kItemClassCols = 32;                 // target columns per size class
constexpr int kItemClasses = 32;                   // classes per list: tn <= 794 has 25 (anything longer - no list has it - would share the longest one)
constexpr int kItemClsStride = 32;                 // u32 per class: a 128-byte line of its own (ext_kernels.h on atomics that share a line); [0] = items appended, [1] = the scatter's cursor
constexpr int kItemClsWords = kItemClasses * kItemClsStride;      // per list; a list buffer has two (list A's ragged part, then list B)
constexpr size_t kItemClsBytes = (size_t)2 * kItemClsWords * 4;   // per list buffer

// class(tn) = (tn - 1) >> 5; the order key counts from the longest class: key 0 = tn in (992, 1024], .., key 31 = tn in [1, 32]
NECAT_HD int item_class(int tn)
{
    const int c = (tn - 1) / kItemClassCols;
    return c < 0 ? 0 : c >= kItemClasses ? kItemClasses - 1 : c;
}
NECAT_HD int item_order_key(int tn) { return kItemClasses - 1 - item_class(tn); }
// the counter / cursor of order key `key` of list `list` (0 = list A's ragged part, 1 = list B) in a list buffer's class words
NECAT_HD u32* item_cls_count(u32* cls, int list, int key) { return cls + (size_t)list * kItemClsWords + (size_t)key * kItemClsStride; }
NECAT_HD u32* item_cls_cursor(u32* cls, int list, int key) { return item_cls_count(cls, list, key) + 1; }
// first rank of order key `key`: the items of the keys before it
NECAT_HD u32 item_order_base(const u32* cls, int list, int key)
{
    u32 base = 0;
    for (int k = 0; k < key; ++k) base += cls[(size_t)list * kItemClsWords + (size_t)k * kItemClsStride];
    return base;
}
// Staging: ONE array of `cap` items per list buffer - a candidate has one block at a time, so a buffer's full, ragged and list-B items together are at most cap -
// list A's ragged items from the front, list B's from the back, at the slot the list's own counter (ExtLists::count[2] / [1]) gave.
NECAT_HD u64 item_stage_slot(int list, u32 cap, u32 slot) { return list ? (u64)cap - 1 - slot : (u64)slot; }
// Final place of the item of rank j (class base + cursor): list A's ragged part fills itemsA from the back (ListView: work index nf16 + j), list B is plain
NECAT_HD u64 item_final_slot(int list, u32 cap, u32 j) { return list ? (u64)j : (u64)cap - 1 - j; }

}  // namespace necat
