// check_cns_job.cpp - the SOURCE of necat_amd/csrc/cns_job.h (cns_run_job: oc2cns's units through two stages one unit apart) compiled with g++ against a FAKE
// library: the C-ABI entry points the job calls are defined here.  Contexts are numbered counters; a volume keeps its pac bytes and offsets;
// necat_volume_gather really gathers on the host (host_bases.h), so a wrong local id changes bytes; necat_cns_load_partition groups the records by template;
// the extension and the consensus call sleep a few milliseconds and log their context and what else ran; the consensus returns, for a template whose read length
// is no multiple of 3, one segment spanning the read with the read's bases AS THE VOLUME IT WAS HANDED HOLDS THEM, and nothing for the others (a template whose
// length is a multiple of 5 is not examined at all); the record text is the real cns_consensus.h.  Every context, volume and result block is counted when made
// and when freed.  CPU only; the volume files and candidate partitions of a project directory are read by the job as always.
//   check_cns_job <wrk-dir> <candidates> <out-prefix> <chunk-bound>
// Checks (tests/test_cns_job_model.py lists them): the same bytes in every mode; units in (partition, chunk) order, at most 2 gathered volumes and 2 result
// blocks alive; the stages overlap, each on its context; every injected failure -> 1, the error printed, nobody left waiting, nothing left alive.
#include <atomic>
#include <chrono>
#include <map>
#include <set>
#include "../../necat_amd/csrc/cns_job.h"

struct necat_ctx { int id; char err[200]; long calls; };       // calls: written by every call WITHOUT a lock - two threads on one context are a race ThreadSanitizer reports
struct necat_volume {
    std::vector<uint8_t> pac; std::vector<uint64_t> offset, size; uint64_t nbases = 0;
    std::vector<int64_t> gid;                                   // a gathered volume: the global ids it was made of (logging only)
    int64_t global(int64_t local) const { return gid.empty() ? local : gid[(size_t)local]; }
};

namespace fake {
std::mutex mu;
std::atomic<int> live_ctx{0}, live_vol{0}, live_gathered{0}, max_gathered{0}, live_blocks{0}, live_res{0}, max_res{0}, live_con{0}, created{0};
std::atomic<int> ext_running{0}, con_running{0}, overlaps{0};
std::map<std::string, std::string> knobs;
std::set<int> producer_ctx, consumer_ctx;               // the contexts of the producer-side calls (upload, gather, load, extension) / of the consensus calls
std::vector<int64_t> ext_first, con_first;              // the global id of the first template of every extension / consensus call, in call order
int n_ext, n_gather, n_load, n_con;
int fail_ext_at = -1, fail_gather_at = -1, fail_load_at = -1, fail_con_at = -1, fail_ctx_create_after = -1;      // the call of that index fails
void reset()
{
    producer_ctx.clear(); consumer_ctx.clear(); ext_first.clear(); con_first.clear();
    n_ext = n_gather = n_load = n_con = 0; max_gathered = 0; max_res = 0; overlaps = 0; created = 0;
    fail_ext_at = fail_gather_at = fail_load_at = fail_con_at = fail_ctx_create_after = -1;
}
void* block(size_t bytes) { ++live_blocks; return calloc(bytes ? bytes : 1, 1); }
void raise_max(std::atomic<int>& m, int now) { for (int v = m; now > v && !m.compare_exchange_weak(v, now);) {} }
void producer_call(necat_ctx* c) { ++c->calls; std::lock_guard<std::mutex> lk(mu); producer_ctx.insert(c->id); }
int failed(necat_ctx* c, const char* what) { snprintf(c->err, sizeof c->err, "fake: %s fails", what); return NECAT_ERR_DEVICE; }
}  // namespace fake

extern "C" {
int necat_ctx_create(int, necat_ctx** out)
{
    if (fake::fail_ctx_create_after >= 0 && fake::live_ctx >= fake::fail_ctx_create_after) { *out = nullptr; return NECAT_ERR_DEVICE; }
    necat_ctx* c = new necat_ctx(); c->id = 100 + fake::created++; c->err[0] = 0; c->calls = 0; ++fake::live_ctx; *out = c; return NECAT_OK;
}
void necat_ctx_destroy(necat_ctx* c) { if (c) { --fake::live_ctx; delete c; } }
const char* necat_last_error(const necat_ctx* c) { return c ? c->err : "fake: no context"; }
int necat_knob_get(const necat_ctx* c, const char* name, char* buf, size_t n)
{
    if (!c) return NECAT_ERR_ARG;
    auto it = fake::knobs.find(name);
    snprintf(buf, n, "%s", it == fake::knobs.end() ? "" : it->second.c_str());
    return NECAT_OK;
}
void necat_cns_default_options(necat_cns_options* o) { memset(o, 0, sizeof *o); o->min_align_size = 400; o->min_cov = 4; o->max_cov = 12; o->error = 0.5; o->mapping_ratio = 0.8; }
void necat_cns_consensus_default_options(necat_cns_consensus_options* o) { memset(o, 0, sizeof *o); o->min_cov = 4; o->min_size = 500; o->path = 1; }
int necat_volume_upload(necat_ctx* c, const uint8_t* pac, uint64_t nbases, const uint64_t* off, const uint64_t* size, uint64_t nseq, necat_volume** out)
{
    fake::producer_call(c);
    necat_volume* v = new necat_volume();
    v->pac.assign(pac, pac + (nbases + 3) / 4); v->offset.assign(off, off + nseq); v->size.assign(size, size + nseq); v->nbases = nbases;
    ++fake::live_vol; *out = v; return NECAT_OK;
}
void necat_volume_free(necat_ctx* c, necat_volume* v)
{
    if (!v) return;
    if (c) ++c->calls;
    if (!v->gid.empty()) --fake::live_gathered;
    --fake::live_vol; delete v;
}
int necat_volume_gather(necat_ctx* c, const necat_volume* const* vols, const int64_t* start, uint64_t n_vols, const int64_t* ids, uint64_t n_ids, necat_volume** out)
{
    fake::producer_call(c);
    *out = nullptr;
    if (fake::n_gather++ == fake::fail_gather_at) return fake::failed(c, "the gather");
    std::vector<uint8_t> codes, one;
    necat_volume* v = new necat_volume();
    for (uint64_t i = 0; i < n_ids; ++i) {
        uint64_t k = n_vols;
        for (uint64_t q = 0; q < n_vols; ++q) if (ids[i] >= start[q] && (uint64_t)(ids[i] - start[q]) < vols[q]->size.size()) k = q;
        if (k == n_vols || (i && ids[i] <= ids[i - 1])) { delete v; snprintf(c->err, sizeof c->err, "fake: id %ld in no volume or not ascending", (long)ids[i]); return NECAT_ERR_ARG; }
        const uint64_t r = (uint64_t)(ids[i] - start[k]);
        one.resize(vols[k]->size[r]);
        necat_host::decode_pac(vols[k]->pac.data(), vols[k]->offset[r], vols[k]->size[r], one.data());
        v->offset.push_back(codes.size()); v->size.push_back(one.size()); v->gid.push_back(ids[i]);
        codes.insert(codes.end(), one.begin(), one.end());
    }
    v->nbases = codes.size(); v->pac.assign((codes.size() + 3) / 4, 0);
    for (uint64_t g = 0; g < codes.size(); ++g) v->pac[g >> 2] |= (uint8_t)(codes[g] << ((~g & 3) << 1));
    if (v->gid.empty()) v->gid.push_back(-1);         // (an empty gathered volume still counts as one)
    ++fake::live_vol; fake::raise_max(fake::max_gathered, ++fake::live_gathered);
    *out = v; return NECAT_OK;
}
int necat_volume_gather_stats(const necat_ctx*, double* ms, uint64_t* bytes) { *ms = 0; *bytes = 0; return NECAT_OK; }
void necat_free(void* p) { if (p) { --fake::live_blocks; free(p); } }

// records of one template together, templates ascending, a template's records in file order (include/necat_hip.h documents the real order and cut)
int necat_cns_load_partition(necat_ctx* c, const necat_volume* reads, const void* packed, uint64_t n, necat_candidate** cands, uint64_t** tmpl_off, uint64_t** n_all, uint64_t* nt)
{
    fake::producer_call(c);
    *cands = nullptr; *tmpl_off = nullptr; *n_all = nullptr; *nt = 0;
    if (fake::n_load++ == fake::fail_load_at) return fake::failed(c, "the partition load");
    const uint32_t* w = (const uint32_t*)packed;
    const uint64_t nseq = reads->size.size();
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) {
        order[i] = i;
        if (w[7 * i + 1] >= nseq || w[7 * i + 4] >= nseq) { snprintf(c->err, sizeof c->err, "fake: candidate record %lu refers to a read outside the read set", (unsigned long)i); return NECAT_ERR_ARG; }
    }
    std::stable_sort(order.begin(), order.end(), [w](uint64_t a, uint64_t b) { return w[7 * a + 1] < w[7 * b + 1]; });
    necat_candidate* cd = (necat_candidate*)fake::block(n * sizeof(necat_candidate));
    std::vector<uint64_t> off;
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t* r = w + 7 * order[k];
        if (!k || r[1] != w[7 * order[k - 1] + 1]) off.push_back(k);
        necat_candidate& o = cd[k];
        o.sdir = (int)(r[0] >> 31); o.qdir = (int)(r[0] >> 30 & 1); o.score = (int)(r[0] & 0x1fffffff);
        o.sid = (int)r[1]; o.sbeg = r[2]; o.send = r[3]; o.qid = (int)r[4]; o.qbeg = r[5]; o.qend = r[6];
        o.ssize = reads->size[r[1]]; o.qsize = reads->size[r[4]]; o.qoff = o.qbeg; o.soff = o.sbeg;
    }
    off.push_back(n);
    *nt = off.size() - 1;
    *tmpl_off = (uint64_t*)fake::block(off.size() * 8); memcpy(*tmpl_off, off.data(), off.size() * 8);
    *n_all = (uint64_t*)fake::block(*nt * 8);
    for (uint64_t t = 0; t < *nt; ++t) (*n_all)[t] = off[t + 1] - off[t];
    *cands = cd;
    return NECAT_OK;
}
int necat_cns_extension_batch(necat_ctx* c, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off, const uint64_t* n_all, uint64_t nt,
                              const necat_cns_options*, necat_cns_result** out)
{
    fake::producer_call(c);
    *out = nullptr;
    ++fake::ext_running;
    if (fake::con_running) ++fake::overlaps;
    std::this_thread::sleep_for(std::chrono::milliseconds(4));
    if (fake::con_running) ++fake::overlaps;
    --fake::ext_running;
    { std::lock_guard<std::mutex> lk(fake::mu); fake::ext_first.push_back(nt ? reads->global(cands[tmpl_off[0]].sid) : -1); }
    if (fake::n_ext++ == fake::fail_ext_at) return fake::failed(c, "the extension");
    necat_cns_result* r = (necat_cns_result*)calloc(1, sizeof *r);
    r->n_templates = nt; r->templates = (necat_cns_template*)calloc(nt ? nt : 1, sizeof(necat_cns_template));
    for (uint64_t t = 0; t < nt; ++t) {
        necat_cns_template& T = r->templates[t];
        T.examined = reads->size[(size_t)cands[tmpl_off[t]].sid] % 5 != 0; T.num_can = (int)n_all[t]; T.num_ovlps = (int)(tmpl_off[t + 1] - tmpl_off[t]); T.ident_cutoff = 0.75;
    }
    fake::raise_max(fake::max_res, ++fake::live_res);
    *out = r; return NECAT_OK;
}
void necat_cns_result_free(necat_cns_result* r) { if (r) { --fake::live_res; free(r->templates); free(r); } }
int necat_cns_consensus_batch(necat_ctx* c, const necat_volume* reads, const necat_candidate* cands, const uint64_t* tmpl_off, uint64_t nt, const necat_cns_result* ext,
                              const necat_cns_consensus_options*, necat_cns_consensus** out)
{
    ++c->calls;
    *out = nullptr;
    ++fake::con_running;
    if (fake::ext_running) ++fake::overlaps;
    std::this_thread::sleep_for(std::chrono::milliseconds(6));
    --fake::con_running;
    { std::lock_guard<std::mutex> lk(fake::mu); fake::consumer_ctx.insert(c->id); fake::con_first.push_back(nt ? reads->global(cands[tmpl_off[0]].sid) : -1); }
    if (fake::n_con++ == fake::fail_con_at) return fake::failed(c, "the consensus");
    if (!ext || ext->n_templates != nt) return fake::failed(c, "the consensus (not the extension's result)");
    std::vector<uint8_t> bases;
    necat_cns_consensus* r = (necat_cns_consensus*)calloc(1, sizeof *r);
    r->n_templates = nt; r->templates = (necat_cns_consensus_template*)calloc(nt ? nt : 1, sizeof(necat_cns_consensus_template));
    r->segments = (necat_cns_segment*)calloc(nt ? nt : 1, sizeof(necat_cns_segment));
    for (uint64_t t = 0; t < nt; ++t) {
        const size_t id = (size_t)cands[tmpl_off[t]].sid;
        const uint64_t len = reads->size[id];
        r->templates[t].on_host = 1; r->templates[t].corrected = ext->templates[t].examined; r->templates[t].seg_begin = r->n_segments;
        if (ext->templates[t].examined && len % 3 != 0) {
            necat_cns_segment& s = r->segments[r->n_segments++];
            s.left = 0; s.right = (int)len; s.cns_from = 0; s.cns_to = (int)len; s.off = bases.size(); s.len = (uint32_t)len;
            bases.resize(bases.size() + len);
            necat_host::decode_pac(reads->pac.data(), reads->offset[id], len, bases.data() + s.off);
        }
        r->templates[t].seg_end = r->n_segments;
    }
    r->n_bases = bases.size(); r->bases = (uint8_t*)malloc(bases.size() + 1);
    if (!bases.empty()) memcpy(r->bases, bases.data(), bases.size());
    ++fake::live_con;
    *out = r; return NECAT_OK;
}
void necat_cns_consensus_free(necat_cns_consensus* r) { if (r) { --fake::live_con; free(r->templates); free(r->segments); free(r->bases); free(r); } }
}

using namespace necat_host;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "check_cns_job: %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static std::string slurp(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (!f) return std::string("<missing>"); std::string s; char b[4096]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) s.append(b, k); fclose(f); return s; }
static bool spit(const std::string& p, const std::string& s) { FILE* f = fopen(p.c_str(), "wb"); if (!f) return false; const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size(); return fclose(f) == 0 && ok; }
static std::multiset<std::string> records(const std::string& fasta)      // the ">..." records of a file, whatever their order
{
    std::multiset<std::string> out;
    for (size_t at = 0; at < fasta.size();) { size_t e = fasta.find("\n>", at); e = e == std::string::npos ? fasta.size() : e + 1; out.insert(fasta.substr(at, e - at)); at = e; }
    return out;
}

struct Job { std::string mode = "merged"; uint64_t bound = 0; int pipeline = 1, t = 1, s = 0, f = 0, node = 0, nodes = 1; };
struct Out { int rc; std::string cns, raw; };
static int g_run = 0;
static const char* g_wrk; static std::string g_prefix;
// one cns_run_job on the fake library; the caller sets the fake's injections AFTER fake::reset() through `inject`
template <class Inject>
static Out run_job(const Job& j, const std::string& can, Inject&& inject)
{
    fake::reset();
    fake::knobs = {{"NECAT_CNS_READS", j.mode}, {"NECAT_CNS_CHUNK_BASES", j.bound ? std::to_string(j.bound) : std::string()}, {"NECAT_CNS_DEVICE", "0"}, {"NECAT_TRACE", "0"}};
    setenv("NECAT_CNS_PIPELINE", j.pipeline ? "1" : "0", 1);
    inject();
    necat_cns_options co; necat_cns_default_options(&co);
    necat_cns_consensus_options cco; necat_cns_consensus_default_options(&cco);
    cco.host_threads = j.t; cco.full_consensus = j.f;
    const std::string base = g_prefix + "_" + std::to_string(g_run++);
    Out o;
    o.rc = cns_run_job(co, cco, j.s != 0, g_wrk, can, (base + ".cns").c_str(), (base + ".raw").c_str(), j.node, j.nodes, 0);
    o.cns = slurp(base + ".cns"); o.raw = slurp(base + ".raw");
    return o;
}
static bool nothing_alive() { return fake::live_ctx == 0 && fake::live_vol == 0 && fake::live_gathered == 0 && fake::live_blocks == 0 && fake::live_res == 0 && fake::live_con == 0; }
static bool ascending(const std::vector<int64_t>& v) { for (size_t i = 1; i < v.size(); ++i) if (v[i] <= v[i - 1]) return false; return true; }

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    g_wrk = argv[1]; g_prefix = argv[3];
    const std::string can = argv[2];
    const uint64_t bound3 = strtoull(argv[4], nullptr, 10);
    auto none = [] {};
    // what the partitions hold: the templates of each (the test wrote partition p for the template ids of one range, ranges ascending with p)
    int P = 0;
    { FILE* in = fopen((can + ".partitions").c_str(), "r"); CHECK(in && fscanf(in, "%d", &P) == 1); fclose(in); }
    std::vector<std::set<uint32_t>> tmpl((size_t)P);
    size_t n_templates = 0, n_nonempty = 0;
    for (int p = 0; p < P; ++p) {
        const std::string b = slurp(can + ".p" + std::to_string(p));
        CHECK(b != "<missing>" && b.size() % 28 == 0);
        for (size_t i = 0; i < b.size() / 28; ++i) { uint32_t w; memcpy(&w, b.data() + 28 * i + 4, 4); tmpl[(size_t)p].insert(w); }
        if (p) for (uint32_t t : tmpl[(size_t)p]) for (int q = 0; q < p; ++q) CHECK(tmpl[(size_t)q].empty() || t > *tmpl[(size_t)q].rbegin());
        n_templates += tmpl[(size_t)p].size(); n_nonempty += !tmpl[(size_t)p].empty();
    }
    CHECK(P == 3 && n_nonempty == 2);
    auto units_of = [&](int p) { size_t k = 0; for (int64_t t : fake::ext_first) k += t >= 0 && tmpl[(size_t)p].count((uint32_t)t); return k; };

    // (a) (b) (c) (e): every mode, the pipeline on and off, -t 1 and 3: the same bytes, the order, the bounds, the contexts, nothing left alive
    Out want{};
    size_t units3 = 0;
    for (int mode = 0; mode < 3; ++mode) for (int pipeline = 1; pipeline >= 0; --pipeline) for (int t : {1, 3}) {
        Job j; j.mode = mode ? "gather" : "merged"; j.bound = mode == 1 ? bound3 : mode == 2 ? 1 : 0; j.pipeline = pipeline; j.t = t;
        const Out o = run_job(j, can, none);
        CHECK(o.rc == 0);
        CHECK(nothing_alive());
        if (want.cns.empty()) { want = o; CHECK(!o.cns.empty() && !o.raw.empty() && o.cns != "<missing>" && o.raw != "<missing>"); }
        CHECK(o.cns == want.cns);
        CHECK(o.raw == want.raw);
        CHECK(fake::ext_first == fake::con_first && ascending(fake::con_first));          // units reach the consumer in (partition, chunk) order
        CHECK(fake::max_gathered <= 2 && fake::max_res <= 2);
        CHECK((mode == 0) == (fake::n_gather == 0));
        if (mode == 0) CHECK(fake::n_ext == (int)n_nonempty);
        if (mode == 1) { for (int p = 0; p < P; ++p) CHECK(tmpl[(size_t)p].empty() || units_of(p) >= 3); units3 = (size_t)fake::n_ext; }
        if (mode == 2) CHECK(fake::n_ext == (int)n_templates && fake::n_gather == (int)n_templates);          // every template is a chunk
        CHECK(fake::producer_ctx.size() == 1 && *fake::producer_ctx.begin() == 100);                       // the first context
        // (merged, the empty partition between the other two fills the one slot while the first one's consensus runs: that mode's overlap is checked with -mn below)
        if (pipeline) { CHECK(fake::created == 2 && fake::consumer_ctx == std::set<int>{101} && (fake::overlaps > 0 || mode == 0)); }
        else CHECK(fake::created == 1 && fake::consumer_ctx == std::set<int>{100} && fake::overlaps == 0);
    }
    CHECK(want.raw.find("_0_0_0.000000)") != std::string::npos);          // -s 0: reads of the id ranges nobody corrected went out whole
    CHECK(units3 >= 6);
    {   // -s 1: merged = gather, no uncorrected read; -f 1: merged = gather
        Job a; a.s = 1; Job b = a; b.mode = "gather"; b.bound = bound3;
        const Out oa = run_job(a, can, none), ob = run_job(b, can, none);
        CHECK(oa.rc == 0 && ob.rc == 0 && oa.cns == ob.cns && oa.raw == ob.raw && oa.cns == want.cns && nothing_alive());
        CHECK(oa.raw.find("_0_0_0.000000)") == std::string::npos && oa.raw.size() < want.raw.size());
        a.s = 0; a.f = 1; b.s = 0; b.f = 1; b.pipeline = 0;
        const Out fa = run_job(a, can, none), fb = run_job(b, can, none);
        CHECK(fa.rc == 0 && fb.rc == 0 && fa.cns == fb.cns && fa.raw == fb.raw && fa.raw != want.raw && nothing_alive());
    }
    for (const char* mode : {"merged", "gather"}) {   // -mn 0 2 and -mn 1 2: their partitions together are the whole run's
        Job a; a.mode = mode; a.bound = bound3; a.nodes = 2; Job b = a; b.node = 1;
        const Out oa = run_job(a, can, none);
        CHECK(fake::overlaps > 0);                 // partitions 0 and 2, one after the other: the extension of 2 beside the consensus of 0
        const Out ob = run_job(b, can, none);
        CHECK(oa.rc == 0 && ob.rc == 0 && nothing_alive());
        CHECK(records(oa.cns + ob.cns) == records(want.cns) && records(oa.raw + ob.raw) == records(want.raw) && !oa.cns.empty() && ob.cns.empty());      // (node 1's one partition is the empty one)
    }

    // (d) failures: 1, the error printed once, the call returns, nothing left alive
    int errors = 0;
    std::string bad = slurp(can + ".p" + std::to_string(P - 1));
    { const uint32_t out_of_range = 1u << 20; memcpy(&bad[28 * 2 + 16], &out_of_range, 4); }
    for (const char* which : {"missing", "bad"}) {
        CHECK(spit(g_prefix + which + ".partitions", std::to_string(P) + "\n"));
        for (int p = 0; p + 1 < P; ++p) CHECK(spit(g_prefix + which + ".p" + std::to_string(p), slurp(can + ".p" + std::to_string(p))));
    }
    CHECK(spit(g_prefix + "bad.p" + std::to_string(P - 1), bad));
    for (int pipeline = 1; pipeline >= 0; --pipeline) {
        Job g; g.mode = "gather"; g.bound = bound3; g.pipeline = pipeline; g.t = 2;
        Job m; m.pipeline = pipeline;
        auto failed = [&](const Out& o) { ++errors; return o.rc == 1 && nothing_alive(); };
        for (int at : {0, (int)units3 / 2, (int)units3 - 1}) CHECK(failed(run_job(g, can, [at] { fake::fail_ext_at = at; })));
        CHECK(failed(run_job(m, can, [&] { fake::fail_ext_at = (int)n_nonempty - 1; })));
        CHECK(failed(run_job(g, can, [] { fake::fail_gather_at = 2; })));
        CHECK(failed(run_job(g, can, [] { fake::fail_load_at = 1; })));
        CHECK(failed(run_job(m, can, [] { fake::fail_load_at = 1; })));
        CHECK(failed(run_job(g, can, [] { fake::fail_con_at = 2; })));
        CHECK(failed(run_job(m, can, [] { fake::fail_con_at = 0; })));
        CHECK(failed(run_job(g, g_prefix + "missing", none)));
        CHECK(failed(run_job(m, g_prefix + "missing", none)));
        CHECK(failed(run_job(g, g_prefix + "bad", none)));          // refused by the chunk planner
        CHECK(failed(run_job(m, g_prefix + "bad", none)));          // .. by the library's partition load
        Job x = g; x.mode = "both";
        CHECK(failed(run_job(x, can, none)));
        // the second context cannot be made: the pipelined job fails; the other one never asks for it
        const Out o = run_job(g, can, [] { fake::fail_ctx_create_after = 1; });
        if (pipeline) CHECK(failed(o)); else CHECK(o.rc == 0 && fake::created == 1 && o.cns == want.cns && o.raw == want.raw && nothing_alive());
    }
    printf("ok errors=%d\n", errors);
    return 0;
}
