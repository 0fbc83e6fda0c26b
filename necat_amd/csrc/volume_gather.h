// volume_gather.h - a subset of the reads of several volumes as one compact volume with dense ids (necat_volume_gather): the plan the host makes and the
// function that builds one destination word.  A volume holds at most 2^32 - 1 bases (oc2mkdb cuts at 2e9) and the kernels address it with that in mind; a
// project of more bases keeps one volume per file, and a stage that needs reads of several of them gathers the ones it names.  No HIP in this header: the
// kernel (volume_kernels.h: k_vol_gather) and tests/host_core/check_vol_gather.cpp run the same gather_word.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "dev_common.h"

namespace necat {
namespace vgather {

constexpr u64 kMaxVolumeBases = 1ULL << 32;       // a volume holds fewer (necat_volume_upload refuses this many)

// Per gathered sequence i (local id i of the result): the first base it takes in the result (dst_off[i]; dst_off[n] = the total: the result's seq_off), the
// volume it comes from and its first base there.
struct Plan {
    std::vector<u64> dst_off, src_off;
    std::vector<u32> src_vol;
    u64 n() const { return src_off.size(); }
    u64 nbases() const { return dst_off.empty() ? 0 : dst_off.back(); }
};

// vol_seq_off[k][0 .. vol_nseq[k]]: the sequence offsets of volume k, whose sequences have the global ids vol_start_id[k] .. + vol_nseq[k]; ids: global, strictly
// ascending.  false, with the reason in err: ids that do not ascend, an id no volume holds, volumes whose id ranges overlap, 2^32 bases or more in all.
inline bool make_plan(const u64* const* vol_seq_off, const u64* vol_nseq, const i64* vol_start_id, u64 n_vols, const i64* ids, u64 n_ids, Plan* p, char* err, size_t err_len)
{
    p->dst_off.assign(1, 0); p->src_off.clear(); p->src_vol.clear();
    std::vector<u32> order((size_t)n_vols);
    for (u64 k = 0; k < n_vols; ++k) order[k] = (u32)k;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return vol_start_id[a] != vol_start_id[b] ? vol_start_id[a] < vol_start_id[b] : a < b; });
    for (u64 j = 0; j < n_vols; ++j) {
        const u32 k = order[j];
        if (vol_start_id[k] < 0 || vol_nseq[k] >= (1ULL << 62)) { snprintf(err, err_len, "volume %u: bad first id or sequence count", k); return false; }
        if (j + 1 < n_vols && (u64)vol_start_id[k] + vol_nseq[k] > (u64)vol_start_id[order[j + 1]]) {
            snprintf(err, err_len, "the id ranges of volumes %u and %u overlap", k, order[j + 1]); return false;
        }
    }
    p->dst_off.reserve(n_ids + 1); p->src_off.reserve(n_ids); p->src_vol.reserve(n_ids);
    u64 j = 0, total = 0;          // ids ascend, so the volume (in id order) only moves forward
    for (u64 i = 0; i < n_ids; ++i) {
        if (i && ids[i] <= ids[i - 1]) { snprintf(err, err_len, "ids[%lu] = %lld does not ascend (ids[%lu] = %lld)", (unsigned long)i, (long long)ids[i], (unsigned long)(i - 1), (long long)ids[i - 1]); return false; }
        while (j < n_vols && ids[i] >= 0 && (u64)ids[i] >= (u64)vol_start_id[order[j]] + vol_nseq[order[j]]) ++j;
        if (ids[i] < 0 || j == n_vols || ids[i] < vol_start_id[order[j]]) { snprintf(err, err_len, "ids[%lu] = %lld is in no volume", (unsigned long)i, (long long)ids[i]); return false; }
        const u32 k = order[j];
        const u64 local = (u64)(ids[i] - vol_start_id[k]);
        const u64 b = vol_seq_off[k][local], e = vol_seq_off[k][local + 1];
        if (e < b || e - b >= kMaxVolumeBases) { snprintf(err, err_len, "volume %u: bad sequence offsets at %lu", k, (unsigned long)local); return false; }
        total += e - b;
        if (total >= kMaxVolumeBases) { snprintf(err, err_len, "the %lu sequences hold 2^32 bases or more: too large for one volume", (unsigned long)n_ids); return false; }
        p->src_off.push_back(b); p->src_vol.push_back(k); p->dst_off.push_back(total);
    }
    return true;
}

// Word w of the result (bases 32 w .. 32 w + 31, base g in bits 2 (g & 31)): the first sequence that reaches into it by binary search over dst_off, then every
// sequence that overlaps it - usually one or two, up to 32 of one base each - cut out of one or two words of its volume and put in place.  Bits no sequence
// covers are zero.  vol_words[k]: the words of volume k; words (b >> 5) .. ((e - 1) >> 5) of it are read for a sequence of the bases [b, e), no others.
NECAT_HD u64 gather_word(u64 w, const u64* dst_off, const u64* src_off, const u32* src_vol, u64 n, const u64* const* vol_words)
{
    const u64 b0 = w << 5, b1 = b0 + 32;
    u64 lo = 0, hi = n;                     // the first i with dst_off[i + 1] > b0
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (dst_off[mid + 1] > b0) hi = mid; else lo = mid + 1;
    }
    u64 out = 0;
    for (u64 i = lo; i < n && dst_off[i] < b1; ++i) {
        const u64 ds = dst_off[i] > b0 ? dst_off[i] : b0, de = dst_off[i + 1] < b1 ? dst_off[i + 1] : b1;
        if (de <= ds) continue;             // (a sequence of no bases)
        const u64 nb = de - ds;             // 1 .. 32 bases of sequence i go to the bits 2 (ds - b0) .. of the word
        const u64 s = src_off[i] + (ds - dst_off[i]);
        const u64* sw = vol_words[src_vol[i]] + (s >> 5);
        const u32 at = (u32)(s & 31);
        u64 bits = sw[0] >> (2 * at);
        if (at + nb > 32) bits |= sw[1] << (64 - 2 * at);          // (at >= 1 here)
        if (nb < 32) bits &= (1ULL << (2 * nb)) - 1;
        out |= bits << (2 * (ds - b0));
    }
    return out;
}

// NECAT pac bytes (first base of a byte in its top two bits) <-> the bytes of the little-endian 2-bit words: the fields of every byte in reverse order, which is
// its own inverse (k_repack, index_kernels.h, does it to eight bytes at a time)
NECAT_HD u64 swap_fields(u64 w)
{
    return ((w & 0x0303030303030303ULL) << 6) | ((w & 0x0C0C0C0C0C0C0C0CULL) << 2) | ((w >> 2) & 0x0C0C0C0C0C0C0C0CULL) | ((w >> 6) & 0x0303030303030303ULL);
}

}  // namespace vgather
}  // namespace necat
