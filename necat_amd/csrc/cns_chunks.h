// cns_chunks.h - oc2cns on a read set that is not one volume (NECAT_CNS_READS=gather): a partition's templates cut into chunks whose reads fit one gathered
// volume (necat_volume_gather), and the ids of a chunk's records rewritten to that volume's.  Host code only, no HIP: tests/host_core/check_vol_gather.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace necat_host {
namespace cns_chunks {

constexpr uint64_t kDefaultChunkBases = 1ULL << 31;       // NECAT_CNS_CHUNK_BASES
constexpr uint64_t kMaxChunkBases = 1ULL << 32;           // a volume holds fewer

struct Chunk {
    uint64_t rec_begin = 0, rec_end = 0;      // its records: Plan::order[rec_begin .. rec_end), whole templates, template ids ascending
    uint64_t n_templates = 0;
    std::vector<int64_t> ids;                 // the reads its records name (templates and queries), ascending, each once: local id i of the chunk's volume is ids[i]
    uint64_t bases = 0;                       // .. and their bases
};

struct Plan {
    std::vector<uint64_t> order;              // the partition's records by template id (records of one template in file order)
    std::vector<Chunk> chunks;
};

// rec: n records of 7 little-endian 32-bit words (PackedGappedCandidate: word 1 the template's id, word 4 the query's); read_size[id] for the nreads reads of the
// project.  Templates join a chunk, in ascending id order, until the reads its records name would hold more than `bound` bases - a read counts once per chunk,
// template and query of every record count - and a template whose reads alone exceed the bound is a chunk of its own (the caller refuses it from kMaxChunkBases on).
// false with *err: a record that names a read outside the project.
inline bool plan_chunks(const uint32_t* rec, uint64_t n, const uint64_t* read_size, uint64_t nreads, uint64_t bound, Plan* p, std::string* err)
{
    p->order.resize(n); p->chunks.clear();
    for (uint64_t i = 0; i < n; ++i) {
        if (rec[7 * i + 1] >= nreads || rec[7 * i + 4] >= nreads) { *err = "candidate record " + std::to_string(i) + " refers to a read outside the read set"; return false; }
        p->order[i] = i;
    }
    std::stable_sort(p->order.begin(), p->order.end(), [rec](uint64_t a, uint64_t b) { return rec[7 * a + 1] < rec[7 * b + 1]; });
    std::vector<uint32_t> stamp(nreads, 0);    // the last chunk (+ 1) a read was counted in
    std::vector<int64_t> fresh;
    Chunk cur;
    uint32_t mark = 1;
    auto close = [&]() { std::sort(cur.ids.begin(), cur.ids.end()); p->chunks.push_back(std::move(cur)); cur = Chunk(); cur.rec_begin = cur.rec_end = p->chunks.back().rec_end; ++mark; };
    for (uint64_t g0 = 0; g0 < n;) {
        uint64_t g1 = g0;
        const uint32_t tid = rec[7 * p->order[g0] + 1];
        while (g1 < n && rec[7 * p->order[g1] + 1] == tid) ++g1;
        for (int pass = 0; pass < 2; ++pass) {
            fresh.clear();
            uint64_t add = 0;
            auto count = [&](uint32_t id) { if (stamp[id] != mark) { stamp[id] = mark; fresh.push_back(id); add += read_size[id]; } };
            count(tid);
            for (uint64_t k = g0; k < g1; ++k) count(rec[7 * p->order[k] + 4]);
            if (pass == 0 && cur.n_templates && cur.bases + add > bound) {       // it does not fit: the chunk ends before this template, which is counted again on its own
                for (int64_t id : fresh) stamp[(size_t)id] = 0;
                close();
                continue;
            }
            cur.ids.insert(cur.ids.end(), fresh.begin(), fresh.end());
            cur.bases += add; cur.rec_end = g1; ++cur.n_templates;
            break;
        }
        g0 = g1;
    }
    if (cur.n_templates) close();
    return true;
}

// the chunk's records, in Plan::order, with both ids rewritten to the chunk's volume: dst holds 7 (rec_end - rec_begin) words
inline void chunk_records(const uint32_t* rec, const Plan& p, const Chunk& c, uint32_t* dst)
{
    auto local = [&c](uint32_t id) { return (uint32_t)(std::lower_bound(c.ids.begin(), c.ids.end(), (int64_t)id) - c.ids.begin()); };
    for (uint64_t k = c.rec_begin; k < c.rec_end; ++k, dst += 7) {
        memcpy(dst, rec + 7 * p.order[k], 28);
        dst[1] = local(dst[1]); dst[4] = local(dst[4]);
    }
}

}  // namespace cns_chunks
}  // namespace necat_host
