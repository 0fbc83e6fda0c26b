// check_cns_device_model.cpp - TEST ONLY.  The CPU model of the device consensus (necat_amd/csrc/cns_dev_core.h: the kernels' per-lane cores, built by g++) beside
// the host form (cns_consensus.h), both fed the add_one_align calls the ORACLE's extension loop logs, as check_consensus.cpp is.  Per template: the model's
// segments must be the host's unless the model flags the template; every link weight must lie within its error term of the host's (klib-order) weight, and in an
// unflagged template every node's score within its running bound of the host's score.  The two
// output files of oc2cns are assembled from the model's segments (the host's for flagged templates), through the shared emit code.
//
// usage: check_cns_device_model <wrk_dir> <partition file> <full log> <min_cov> <min_size> <full_consensus> <cns_out> <raw_out> <tol_scale>
// prints one line: templates= flagged= uncertain= bad= loose= links= links_differ= violations= nodes= score_violations= mismatches= max_err=
// (uncertain: flagged by a score comparison inside the bounds; bad: by a bound or an array the analysis does not cover; loose: by a scaled link bound above the cap.
// A template that is `loose` only still has its segments and scores compared with the host's: at an inflated tolerance that checks what certain() let through.)
#include <algorithm>
#include <fstream>
#include <sstream>

#include "../../necat_amd/csrc/host_io.h"
#include "../../necat_amd/csrc/cns_consensus.h"
#include "../../necat_amd/csrc/cns_dev_core.h"

using namespace necat_host;
namespace cd = necat::cns_dev;

int main(int argc, char** argv)
{
    if (argc < 10) { fprintf(stderr, "usage\n"); return 2; }
    const char* wrk = argv[1];
    const int min_cov = atoi(argv[4]), min_size = atoi(argv[5]), full = atoi(argv[6]);
    const double tol = strtod(argv[9], nullptr);
    std::string err;
    VolumesInfo vi;
    if (!load_volumes_info(wrk, &vi, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    std::vector<std::vector<uint8_t>> reads; std::vector<std::string> names;
    for (int v = 0; v < vi.num_volumes; ++v) {
        HostVolume hv;
        if (!load_volume(vi.names[v].c_str(), &hv, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
        for (uint64_t i = 0; i < hv.offset.size(); ++i) {
            std::vector<uint8_t> r(hv.size[i]);
            for (uint64_t k = 0; k < hv.size[i]; ++k) { const uint64_t g = hv.offset[i] + k; r[k] = (uint8_t)((hv.pac[g >> 2] >> ((~g & 3) << 1)) & 3); }
            reads.push_back(std::move(r)); names.emplace_back(hv.name(i));
        }
    }
    {   // the strand accessor of the tag kernel against the host's expression (cns_consensus.h: 3 - q[qsize - 1 - (qoff + i)])
        const std::vector<uint8_t>& q = reads[0];
        std::vector<uint64_t> words((q.size() + 5 + 31) / 32 + 1, 0);
        for (size_t g = 0; g < q.size(); ++g) words[(g + 5) >> 5] |= (uint64_t)q[g] << (((g + 5) & 31) * 2);
        for (int i = 0; i < (int)q.size(); ++i)
            if (cd::strand_base(words.data(), 5, (int)q.size(), 0, i) != q[(size_t)i] || cd::strand_base(words.data(), 5, (int)q.size(), 1, i) != (uint32_t)(3 - q[q.size() - 1 - (size_t)i])) {
                fprintf(stderr, "strand_base differs at %d\n", i); return 3;
            }
    }
    int min_id = 1 << 30, max_id = -1;
    {
        std::ifstream in(argv[2], std::ios::binary);
        uint32_t item[7];
        while (in.read((char*)item, 28)) { min_id = std::min(min_id, (int)item[1]); max_id = std::max(max_id, (int)item[1]); }
    }
    std::string cns_txt, raw_txt;
    std::vector<uint8_t> corrected((size_t)std::max(0, max_id + 1), 0);
    struct Ov { std::vector<uint8_t> ops, q; std::vector<uint64_t> words; int ncols, toff; double w; };
    std::vector<Ov> ovs;
    cns::Worker w;
    std::vector<cns::SegCodes> kept_host, kept_model;
    cd::ModelOut mo;
    unsigned long n_t = 0, n_flag = 0, n_unc = 0, n_bad = 0, n_loose = 0, n_links = 0, n_differ = 0, n_viol = 0, n_mis = 0, n_nodes = 0, n_sviol = 0;
    double max_err = 0;
    std::ifstream log(argv[3]);
    std::string line;
    while (std::getline(log, line)) {
        std::vector<std::string> f;
        { std::stringstream ss(line); std::string x; while (std::getline(ss, x, '\t')) f.push_back(x); }
        if (f.empty()) continue;
        if (f[0] == "A") {
            if (f.size() < 9) { fprintf(stderr, "the log must be a FULL log (gapped strings)\n"); return 2; }
            Ov o; o.toff = atoi(f[1].c_str()); o.w = strtod(f[3].c_str(), nullptr); o.ncols = atoi(f[4].c_str());
            const std::string &qa = f[7], &ta = f[8];
            o.ops.assign((size_t)(o.ncols + 3) / 4 + 1, 0);
            for (int i = 0; i < o.ncols; ++i) {
                const int op = qa[i] == '-' ? 2 : (ta[i] == '-' ? 1 : (qa[i] == ta[i] ? 0 : 3));
                o.ops[i >> 2] |= (uint8_t)(op << ((i & 3) * 2));
                if (qa[i] != '-') o.q.push_back((uint8_t)(qa[i] == 'A' ? 0 : qa[i] == 'C' ? 1 : qa[i] == 'G' ? 2 : 3));
            }
            o.words.assign(o.q.size() / 32 + 2, 0);
            for (size_t g = 0; g < o.q.size(); ++g) o.words[g >> 5] |= (uint64_t)o.q[g] << ((g & 31) * 2);
            ovs.push_back(std::move(o));
        } else if (f[0] == "T") {
            const int tid = atoi(f[1].c_str()), tsize = atoi(f[2].c_str());
            const double cutoff = strtod(f[3].c_str(), nullptr);
            const int num_can = atoi(f[4].c_str()), num_ovlps = atoi(f[5].c_str());
            std::vector<cns::OverlapIn> in;
            std::vector<cd::ModelOverlap> min_;
            for (const Ov& o : ovs) {
                cns::OverlapIn x; x.ops = o.ops.data(); x.ncols = o.ncols; x.toff = o.toff; x.weight = o.w; x.qfwd = o.q.data(); x.qsize = (int)o.q.size(); x.qoff = 0; x.qdir = 0;
                in.push_back(x);
                cd::ModelOverlap m; m.ops = o.ops.data(); m.ncols = o.ncols; m.toff = o.toff; m.weight = o.w; m.words = o.words.data(); m.read_begin = 0; m.qsize = (int)o.q.size(); m.qoff = 0; m.qdir = 0;
                min_.push_back(m);
            }
            if ((int)reads[tid].size() != tsize) { fprintf(stderr, "template %d: size mismatch\n", tid); return 2; }
            cns::template_segments(w, in.data(), in.size(), tsize, tid, min_cov, min_size, kept_host);
            cd::model_template(min_.data(), min_.size(), tsize, min_cov, min_size, tol, mo);
            ++n_t;
            max_err = std::max(max_err, mo.max_err);
            if (mo.links.size() != w.bb.links.size()) { ++n_viol; fprintf(stderr, "template %d: %zu links, the host has %zu\n", tid, mo.links.size(), w.bb.links.size()); }
            else for (size_t l = 0; l < mo.links.size(); ++l) {
                ++n_links;
                const double d = fabs(mo.links[l].weight - w.bb.links[l].weight);
                if (d != 0) ++n_differ;
                if (d > mo.links[l].err || (int)mo.links[l].count != w.bb.links[l].count) ++n_viol;
            }
            kept_model.clear();
            for (const cd::ModelSeg& s : mo.segs) { cns::SegCodes c; c.left = s.left; c.right = s.right; c.cns_from = s.cns_from; c.cns_to = s.cns_to; c.seq = s.seq; kept_model.push_back(c); }
            if (mo.uncertain) ++n_unc;
            if (mo.bad) ++n_bad;
            if (mo.loose) ++n_loose;
            if (mo.flagged) ++n_flag;
            if (!mo.uncertain && !mo.bad) {
                for (size_t n = 0; n < mo.n_score.size(); ++n) {         // the running bounds: every scored node against the host's score of the same (position, delta, base)
                    if (!mo.n_scored[n]) continue;
                    ++n_nodes;
                    const cns::BaseLinks& col = w.bb.deltas[w.bb.items[(size_t)mo.n_pos[n]].first + (mo.n_dc[n] >> 3)].links[mo.n_dc[n] & 7u];
                    if (!col.coverage || !(fabs(mo.n_score[n] - col.score) <= mo.n_err[n])) ++n_sviol;
                }
                bool same = kept_model.size() == kept_host.size();
                for (size_t s = 0; same && s < kept_host.size(); ++s) {
                    const cns::SegCodes &a = kept_model[s], &b = kept_host[s];
                    same = a.left == b.left && a.right == b.right && a.cns_from == b.cns_from && a.cns_to == b.cns_to && a.seq == b.seq;
                }
                if (!same) { ++n_mis; fprintf(stderr, "template %d: the model's segments differ from the host's\n", tid); }
            }
            const bool c = cns::emit_template(w, mo.flagged ? kept_host : kept_model, reads[tid].data(), tsize, tid, names[tid].c_str(), full != 0, num_can, num_ovlps, cutoff, cns_txt, raw_txt);
            if (c) corrected[(size_t)tid] = 1;
            ovs.clear();
        }
    }
    for (int id = min_id; id < max_id; ++id)
        if (!corrected[(size_t)id]) cns::uncorrected_record(raw_txt, reads[id].data(), (int)reads[id].size(), id, names[id].c_str());
    std::ofstream(argv[7], std::ios::binary) << cns_txt;
    std::ofstream(argv[8], std::ios::binary) << raw_txt;
    printf("templates=%lu flagged=%lu uncertain=%lu bad=%lu loose=%lu links=%lu links_differ=%lu violations=%lu nodes=%lu score_violations=%lu mismatches=%lu max_err=%.3g\n", n_t, n_flag, n_unc, n_bad, n_loose, n_links, n_differ,
           n_viol, n_nodes, n_sviol, n_mis, max_err);
    return 0;
}
