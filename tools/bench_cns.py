#!/usr/bin/env python
"""Throughput of necat_cns_extension_batch on the bench workload: E. coli-size synthetic reads,
candidates from this library's own oc2pmov -j 0 path, role-swapped into one partition as oc2pcan does.

    python tools/bench_cns.py [genome_len coverage] [--consensus] [--rescue] [--long-indels FRACTION]
(the CPU port of the same loop is timed by tests/tools/cns_cpu_port.py)

--rescue runs the extension loop with rescue_long_indels = 1 (oc2cns -r 1) instead: three runs with both halves of the rescue pair on the host threads
(NECAT_DALIGN_DEVICE=0 NECAT_NW_DEVICE=0: "host"), three with the global alignment on the device (0 / 1: "device") and three with the local alignment there as
well (1 / 1: "device_device"), each in a context created under that setting, as one JSON line: candidates tried / with a range from DALIGNER / rescued, the wall
clock of the whole pair and of its two halves per run, who decided the local half, and whether the settings gave the same overlaps.  A second JSON line has
necat_dalign_stats of one necat_local_align_batch call on the anchors of the partition's first 2048 candidates (the call does not say which candidates the
loop rescues) and the histogram of wave steps per job, from one call per job.
--long-indels FRACTION gives that fraction of the reads long indels (synth.add_long_indels, as tests/util.py's make_long_indel_partition does): the bench reads
themselves need few rescues.

--consensus adds the consensus proper (necat_cns_consensus_batch) on ONE extension result: three runs of its host path (path 1, NECAT_CNS_THREADS host threads,
16 unless the environment says otherwise) and three of its device path (path 0: column upload, kernels, result download and fallback included), as a second JSON
line: wall-clock ranges, the fallback share, the kernels' times, and whether the two paths' outputs are equal.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from necat_amd import capi, synth  # noqa: E402


def consensus_leg(ctx, vol, cands, toff, res):
    import json
    out = dict(templates=int(res.templates.shape[0]), examined=int(np.count_nonzero(res.templates["examined"])), host_threads=int(ctx.knob("NECAT_CNS_THREADS")))
    snap = {}
    for path, name in ((1, "host"), (0, "device")):
        walls = []
        for it in range(3):
            t = time.time()
            r = ctx.cns_consensus_batch(vol, cands, toff, res, capi.cns_consensus_options(path=path))
            walls.append(round(time.time() - t, 3))
            if it == 2:
                key = (r.templates["corrected"].tobytes(), r.segments[["left", "right", "cns_from", "cns_to", "len"]].tobytes(), r.bases.tobytes())
                snap[name] = key
                out[name + "_segments"] = int(r.segments.shape[0])
                if path == 0:
                    out.update(n_device=int(r.n_device), n_fallback=int(r.n_fallback), n_uncertain=int(r.n_uncertain), chunks=int(r.n_chunks), device_ms=round(r.device_ms, 1),
                               fallback_host_ms=round(r.host_ms, 1), kernel_ms={k: round(v, 1) for k, v in r.kernel_ms.items()})
            r.free()
        out[name + "_wall_s"] = walls
    out["outputs_equal"] = snap["host"] == snap["device"]
    print(json.dumps(out))


def rescue_leg(vol, cands, toff, n_all):
    import json
    out, snap = {}, {}
    keys = ["cand", "qoff", "qend", "toff", "tend", "align_size", "ident_perc", "weight"]
    for dal, dev, name in ((0, 0, "host"), (0, 1, "device"), (1, 1, "device_device")):
        os.environ["NECAT_DALIGN_DEVICE"] = str(dal)
        os.environ["NECAT_NW_DEVICE"] = str(dev)
        c = capi.Context(0)          # (a context reads its knobs when it is created; the volume of another context of the device may be read)
        runs = []
        for it in range(3):
            t = time.time()
            res = c.cns_extension_batch(vol, cands, toff, n_all, capi.cns_options(rescue_long_indels=1))
            runs.append(dict(wall_s=round(time.time() - t, 4), rescue_ms=round(res.rescue_ms, 1), dalign_ms=round(res.rescue_dalign_ms, 1), nw_ms=round(res.rescue_nw_ms, 1)))
            if it == 2:
                out[name] = dict(aligned=int(res.n_aligned), overlaps=int(res.overlaps.shape[0]), tried=int(res.n_rescue_tried), with_range=int(res.n_rescue_nw),
                                 rescued=int(res.n_rescued), nw_on_device=int(res.n_rescue_nw_device), nw_handed_back=int(res.n_rescue_nw_host),
                                 dalign_on_device=int(res.n_rescue_dalign_device), dalign_handed_back=int(res.n_rescue_dalign_host))
                snap[name] = res.overlaps[keys].tobytes()
            res.free()
        out[name]["runs"] = runs
        c.close()
    out["overlaps_equal"] = snap["host"] == snap["device"] == snap["device_device"]
    print(json.dumps(out))
    dalign_leg(vol, cands)


def dalign_leg(vol, cands, n=2048):
    import json
    os.environ.pop("NECAT_DALIGN_DIAGS", None)
    c = capi.Context(0)
    n = min(n, cands.shape[0])
    jobs = np.zeros(n, dtype=capi.DALIGN_JOB_DTYPE)
    for f, g in (("qid", "qid"), ("qdir", "qdir"), ("qstart", "qoff"), ("sid", "sid"), ("sstart", "soff")):
        jobs[f] = cands[g][:n]
    walls = []
    for it in range(3):
        t = time.time()
        res, st = c.local_align_batch(vol, vol, 0, 0, jobs, error=0.5, min_align_size=400)
        walls.append(round((time.time() - t) * 1e3, 2))
    steps = np.zeros(n, dtype=np.int64)
    for i in range(n):
        steps[i] = c.local_align_batch(vol, vol, 0, 0, jobs[i:i + 1], error=0.5, min_align_size=400)[1].n_steps
    edges = [0, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 1 << 40]
    hist = {("<%d" % hi if hi < (1 << 40) else ">=%d" % lo): int(np.count_nonzero((steps >= lo) & (steps < hi))) for lo, hi in zip(edges[:-1], edges[1:])}
    print(json.dumps(dict(dalign_jobs=int(n), ok=int(np.count_nonzero(res["ok"])), wall_ms=walls, device_ms=round(st.device_ms, 2), host_ms=round(st.host_ms, 2),
                          n_device=int(st.n_device), n_host=int(st.n_host), n_selfcheck=int(st.n_selfcheck), n_over_cap=int(st.n_over_cap), n_steps=int(st.n_steps),
                          max_diags=int(st.max_diags), handed_back_share=round(st.n_host / max(1, n), 5), steps_per_job_both_directions=hist)))
    c.close()


def main():
    argv = sys.argv[1:]
    frac = 0.0
    if "--long-indels" in argv:
        i = argv.index("--long-indels")
        frac = float(argv[i + 1])
        del argv[i:i + 2]
    args = [a for a in argv if a not in ("--consensus", "--rescue")]
    consensus = "--consensus" in argv
    rescue = "--rescue" in argv
    if consensus:
        os.environ.setdefault("NECAT_CNS_THREADS", "16")          # (a context reads its knobs when it is created)
    glen = int(args[0]) if len(args) > 0 else 4_600_000
    cov = float(args[1]) if len(args) > 1 else 40.0
    import util
    rs = synth.simulate_reads(glen, cov, seed=7)
    if frac > 0:
        rs = synth.add_long_indels(rs, frac, seed=8)
    ctx = capi.Context(0)
    sizes = rs.sizes.astype(np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    vol = ctx.upload_volume(synth.pack_2bit(rs.codes), int(sizes.sum()), off, sizes)
    opt = capi.default_options(**dict(util.FAST, kmer_size=15, job=0))
    t = time.time()
    ix = ctx.build_index(vol, opt.kmer_size, opt.kmer_cnt_cutoff)
    c = ctx.find_candidates(ix, vol, vol, 0, 0, opt, True)
    ix.free()
    part = util.pcan_single_partition(capi.pack_candidates(c).tobytes())
    print("candidates: %d (%.2f s), partition records: %d" % (c.shape[0], time.time() - t, len(part) // 28), file=sys.stderr)
    t = time.time()
    cands, toff, n_all = ctx.cns_load_partition(vol, np.frombuffer(part, dtype=np.uint8))
    t_load = time.time() - t
    if rescue:
        rescue_leg(vol, cands, toff, n_all)
        return
    co = capi.cns_options()
    best = None
    for it in range(3):
        t = time.time()
        res = ctx.cns_extension_batch(vol, cands, toff, n_all, co)
        dt = time.time() - t
        ov = res.overlaps
        cols = int(ov["align_size"].sum())
        qb = int((ov["qend"] - ov["qoff"]).sum())
        line = dict(templates=int(res.templates.shape[0]), overlaps=int(ov.shape[0]), aligned=int(res.n_aligned), used=int(res.n_used),
                    rounds=int(res.n_rounds), wall_s=round(dt, 4), device_ms=round(res.device_ms, 1), host_ms=round(res.host_ms, 1),
                    accepted_columns=cols, accepted_query_bp=qb)
        if consensus and it == 2:
            consensus_leg(ctx, vol, cands, toff, res)
        res.free()
        if best is None or dt < best["wall_s"]:
            best = line
    best["load_partition_s"] = round(t_load, 3)
    best["templates_per_s"] = round(best["templates"] / best["wall_s"], 1)
    best["alignments_per_s"] = round(best["aligned"] / best["wall_s"], 1)
    import json
    print(json.dumps(best))


if __name__ == "__main__":
    main()
