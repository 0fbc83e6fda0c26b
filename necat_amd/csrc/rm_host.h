// rm_host.h - host side of necat_map_reference: rm_extend_candidates / rm_extend_candidate (reference_mapping/rm_worker.c:61-196)
// replayed on one read's candidates after the device aligned every one of them block-wise against its stretch of the reference
// (rm_window, ext_core.h).  In candidate order, as the reference walks them: a candidate whose anchor lies inside a record already
// accepted for this read is skipped (map_aux.c:4-20); one whose block-wise alignment failed is dropped; one whose alignment stops
// more than 500 bp short of its chained range goes through the rescue pair (rescue.h) on its stretch and is dropped if that fails.
// The walk (rm::walk) is one body; who computes the pair is its provider: rm::Worker runs rescue::Dalign + rescue::EdlibGo on the
// decoded stretch when the walk asks, rm::TableWorker looks the candidate up in a table computed ahead of the walk (the speculative
// pass of stage_refmap.inl).  A record the pair gives changes which later candidates are contained, so a table holds an entry for
// every candidate that CAN need the pair and the walk leaves some unused.
// No HIP in this header.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/necat_hip.h"
#include "dev_common.h"
#include "ext_core.h"
#include "host_bases.h"
#include "rescue.h"

namespace necat {
namespace rm {

// rm_worker.c:82, :103-110: is the block-wise alignment (record m, REV already turned to forward coordinates) short of the chain?
inline bool needs_rescue(const necat_candidate& c, const necat_m4& m)
{
    const bool check = c.qoff >= c.qbeg && c.qoff < c.qend && c.soff >= c.sbeg && c.soff < c.send;
    if (!check) return false;
    const int64_t qb = c.qdir ? (int64_t)(m.qsize - m.qend) : (int64_t)m.qoff, qe = c.qdir ? (int64_t)(m.qsize - m.qoff) : (int64_t)m.qend;
    const int64_t lhang = qb > (int64_t)c.qbeg ? qb - (int64_t)c.qbeg : 0, rhang = qe < (int64_t)c.qend ? (int64_t)c.qend - qe : 0;
    return lhang + rhang > 500;
}

// What the rescue pair gave for one candidate - the seam between the walk and whoever computes the pair.  Coordinates are on the
// strand qdir of the read and RELATIVE TO THE CANDIDATE'S STRETCH of the reference (rm_window's `from`), as rescue::EdlibGo leaves them
// on the decoded stretch: the walk adds `from` once and turns a reverse read's range to forward coordinates.  `tried`: the pair was
// run for this candidate (a table holds an entry for every candidate that can need one; the walk may use fewer).
struct Rescue { uint8_t tried, ok; int32_t qoff, qend, toff, tend; double ident_perc; };

// rm_extend_candidates on candidates [lo, hi) = one read's, in examination order; accepted records are appended to out.
// rescue(i, cc, from, to, woff) -> Rescue: the pair for candidate i on its stretch [from, to) with the anchor at woff inside it.
// tried / rescued count what the walk consumed; missing counts answers without `tried` (a table that lacks an entry: the candidate is dropped).
template <class Provider>
inline void walk(const necat_candidate* c, const necat_m4* m4, const uint8_t* ok, uint64_t lo, uint64_t hi, std::vector<necat_m4>& out, uint64_t& tried, uint64_t& rescued,
                 uint64_t& missing, Provider&& rescue)
{
    const size_t first = out.size();
    for (uint64_t i = lo; i < hi; ++i) {
        const necat_candidate& cc = c[i];
        bool contained = false;
        for (size_t j = first; j < out.size() && !contained; ++j) {
            const necat_m4& m = out[j];
            contained = cc.qdir == m.qdir && cc.sid == m.sid && cc.qoff >= m.qoff && cc.qoff <= m.qend && cc.soff >= m.soff && cc.soff <= m.send;
        }
        if (contained || !ok[i]) continue;
        necat_m4 m = m4[i];
        if (needs_rescue(cc, m)) {
            ++tried;
            int64_t from, to, woff;
            rm_window((int64_t)cc.qoff, (int64_t)cc.qsize, (int64_t)cc.soff, (int64_t)cc.ssize, &from, &to, &woff);
            const Rescue r = rescue(i, cc, from, to, woff);
            if (!r.tried) ++missing;
            if (!r.tried || !r.ok) continue;
            ++rescued;
            m.qoff = (uint64_t)r.qoff; m.qend = (uint64_t)r.qend;
            m.soff = (uint64_t)(r.toff + from); m.send = (uint64_t)(r.tend + from);
            m.ident_perc = r.ident_perc;
            if (cc.qdir == 1) { const uint64_t qo = m.qsize - m.qend, qe = m.qsize - m.qoff; m.qoff = qo; m.qend = qe; }
        }
        out.push_back(m);
    }
}

// the host provider: rescue::Dalign + rescue::EdlibGo on the decoded stretch
struct Worker {
    rescue::Dalign dal;
    rescue::EdlibGo edl;
    std::vector<uint8_t> q, t;
    int32_t q_id = -1, q_dir = -1;
    uint64_t n_rescue_tried = 0, n_rescued = 0, n_missing = 0;
    Worker(const rescue::DalignSpec& spec, double error) : dal(spec), edl(error) {}

    void replay(const necat_candidate* c, const necat_m4* m4, const uint8_t* ok, uint64_t lo, uint64_t hi, const necat_host::BaseWords& reads, const necat_host::BaseWords& ref,
                int read_start_id, int ref_start_id, int min_align_size, std::vector<necat_m4>& out)
    {
        q_id = -1;
        walk(c, m4, ok, lo, hi, out, n_rescue_tried, n_rescued, n_missing, [&](uint64_t, const necat_candidate& cc, int64_t from, int64_t to, int64_t woff) {
            Rescue r = {1, 0, 0, 0, 0, 0, 0.0};
            if (q_id != cc.qid || q_dir != cc.qdir) { q.resize(cc.qsize); reads.decode(cc.qid - read_start_id, cc.qdir, 0, (int64_t)cc.qsize, q.data()); q_id = cc.qid; q_dir = cc.qdir; }
            t.resize((size_t)(to - from));
            ref.decode(cc.sid - ref_start_id, 0, from, to, t.data());
            if (!dal.go((const char*)q.data(), (int)cc.qoff, (int)cc.qsize, (const char*)t.data(), (int)woff, (int)(to - from), min_align_size)) return r;
            if (!edl.go((const char*)q.data(), dal.r.abpos, dal.r.aepos, (const char*)t.data(), dal.r.bbpos, dal.r.bepos, dal.r.diffs, min_align_size)) return r;
            r.ok = 1; r.qoff = edl.qoff; r.qend = edl.qend; r.toff = edl.toff; r.tend = edl.tend; r.ident_perc = edl.ident_perc;
            return r;
        });
    }
};

// the table provider: table[i] is candidate i's Rescue, computed ahead for every candidate with ok && needs_rescue (stage_refmap.inl's speculative pass)
struct TableWorker {
    const Rescue* table;
    uint64_t n_rescue_tried = 0, n_rescued = 0, n_missing = 0;
    explicit TableWorker(const Rescue* tb) : table(tb) {}

    void replay(const necat_candidate* c, const necat_m4* m4, const uint8_t* ok, uint64_t lo, uint64_t hi, std::vector<necat_m4>& out)
    {
        walk(c, m4, ok, lo, hi, out, n_rescue_tried, n_rescued, n_missing, [&](uint64_t i, const necat_candidate&, int64_t, int64_t, int64_t) { return table[i]; });
    }
};

}  // namespace rm
}  // namespace necat
