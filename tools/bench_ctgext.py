#!/usr/bin/env python
"""necat_ctg_extend_batch (the aligner and the coverage cap of contig polishing) on synthetic contig segments, and the chain seeds -> extend -> consensus.

    python tools/bench_ctgext.py [--err 0.08] [--out profiles/ctg_extend_bench.json]

Input: bench_ctgseed.py's shapes and generator - one segment of 1 Mb with reads of 10 kb at 15 x, and one of 1.5 Mb at 40 x -, every read a record at its true
placement on the strand it was read from, sorted by soff as the program sorts them.  The reads carry 8 % error, not that tool's 12 %: at 12 % (thirds: mismatch,
inserted base, deleted base) an alignment's identity is 88.5 % and the accept rule turns every record down - no overlap, no cap, no consensus (--err 0.12 shows it).  Per setting a warm-up, then three runs of
    necat_ctg_seed_batch -> necat_ctg_extend_batch (that table handed in) -> necat_ctg_consensus_batch (the three arrays handed on unchanged),
each call's wall clock, the entry's four times, the records aligned ahead of the loop against those the loop reached (n_aligned / n_used), the column bytes
downloaded against those of the chosen overlaps, and the wall time of the chain: the polishing time of the segment.  It is recorded, not held to a threshold - the
reference's program is not where the GPU is.  One JSON line, also written to --out."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_input(size, coverage, seed=11, read_len=10000, err=0.12):
    """bench_ctgseed.make_input's reads (the same draws), with where each was cut from"""
    import bench_ctgseed
    contig, reads, qdirs = bench_ctgseed.make_input(size, coverage, seed, read_len, err)
    rng = np.random.default_rng(seed)
    rng.integers(0, 4, size, dtype=np.uint8)
    starts = []
    for _ in range(len(reads)):
        a = int(rng.integers(0, max(1, size - read_len + 1)))
        starts.append(a)
        u = rng.random(read_len)
        n_sub = int((u < err / 3).sum())
        rng.integers(1, 4, n_sub, dtype=np.uint8)
        n_ins = int(((u >= err / 3) & (u < 2 * err / 3)).sum())
        rng.integers(0, 4, n_ins, dtype=np.uint8)
        rng.integers(0, 2)
    return contig, reads, qdirs, starts, read_len


def one_setting(ctx, size, cov, err):
    from necat_amd import capi
    import bench_ctgseed
    t = time.time()
    contig, reads, qdirs, starts, read_len = make_input(size, cov, err=err)
    # the draws were replayed right if the reads begin with bases of their places (a 10-mer of the first 70 bases within the first 100 of the place)
    probe = list(range(0, len(reads), max(1, len(reads) // 50)))
    hits = 0
    for k in probe:
        r = (3 - reads[k])[::-1] if qdirs[k] else reads[k]
        place = contig[starts[k]:starts[k] + 100].tobytes()
        hits += any(r[i:i + 10].tobytes() in place for i in range(60))
    assert hits * 10 >= len(probe) * 9, "the placements are not the reads'"
    rv, cv = bench_ctgseed.upload(ctx, reads), bench_ctgseed.upload(ctx, [contig])
    n = len(reads)
    order = np.argsort(np.array(starts), kind="stable")
    seg = np.zeros(1, dtype=capi.CTG_SEGMENT_DTYPE)
    seg[0] = (0, size, 0, 0, n)
    jobs = np.zeros(n, dtype=capi.CTG_EXTEND_JOB_DTYPE)
    jobs["qid"] = order; jobs["qdir"] = np.array(qdirs)[order]; jobs["soff"] = np.array(starts)[order]; jobs["send"] = jobs["soff"] + read_len
    sj = np.zeros(n, dtype=capi.CTG_SEED_JOB_DTYPE)
    sj["qid"], sj["qdir"] = jobs["qid"], jobs["qdir"]
    print("input: %d bases, %d reads (%.1f s)" % (size, n, time.time() - t), file=sys.stderr)
    out = dict(segment_bases=size, coverage=cov, read_error=err, records=n, read_bases=int(sum(r.shape[0] for r in reads)))
    runs, snap = [], None
    for it in range(4):          # 0: the warm-up
        t0 = time.time()
        seeds = ctx.ctg_seed_batch(rv, 0, cv, seg, sj, capi.ctg_seed_options())
        t1 = time.time()
        ext = ctx.ctg_extend_batch(rv, 0, cv, seg, jobs, seeds, capi.ctg_extend_options())
        t2 = time.time()
        cns = ctx.ctg_consensus_batch(rv, 0, cv, ext.segments, ext.overlaps, ext.ops, capi.ctg_consensus_options())
        t3 = time.time()
        if it == 0:
            continue
        runs.append(dict(chain_s=round(t3 - t0, 4), seed_s=round(t1 - t0, 4), extend_s=round(t2 - t1, 4), consensus_s=round(t3 - t2, 4),
                         extend_ms={k: round(v, 2) for k, v in ext.ms.items()}))
        s = (ext.snapshot(), cns.snapshot())
        assert snap is None or s == snap, "two runs gave different results"
        snap = s
    st = ext.jobs["state"]
    out.update(runs=runs, chain_s_median=sorted(r["chain_s"] for r in runs)[1], n_seeded=ext.n_seeded, n_aligned=ext.n_aligned, n_used=ext.n_used,
               aligned_per_used=round(ext.n_aligned / max(1, ext.n_used), 3), overlaps=int(ext.overlaps.shape[0]),
               verdicts=dict(capped=int((st == 0).sum()), no_seed=int((st == 1).sum()), no_alignment=int((st == 2).sum()), rejected=int((st == 3).sum()), accepted=int((st == 4).sum())),
               pair_tried=ext.n_pair_tried, pair_accepted=ext.n_pair_accepted, dalign_device=ext.n_dalign_device, dalign_host=ext.n_dalign_host, nw_device=ext.n_nw_device,
               nw_host=ext.n_nw_host, cols_bytes_downloaded=ext.cols_bytes_downloaded, cols_bytes_used=ext.cols_bytes_used,
               cols_used_share=round(ext.cols_bytes_used / max(1, ext.cols_bytes_downloaded), 3),
               polished_bases=len(cns.polished[0]), consensus_upper=sum(1 for c in cns.cns[0] if c < 97), consensus_bases=len(cns.cns[0]))
    rv.free(); cv.free()
    return out


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "ctg_extend_bench.json")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    err = 0.08
    if "--err" in argv:
        i = argv.index("--err")
        err = float(argv[i + 1])
        del argv[i:i + 2]
    from necat_amd import capi
    os.environ.setdefault("NECAT_CNS_THREADS", "16")          # (a context reads its knobs when it is created)
    ctx = capi.Context(0)
    out = dict(device=ctx.device_name().strip(), host_threads=int(ctx.knob("NECAT_CNS_THREADS")), dalign_diags=int(ctx.knob("NECAT_DALIGN_DIAGS")))
    out["settings"] = [one_setting(ctx, size, cov, err) for size, cov in ((1_000_000, 15.0), (1_500_000, 40.0))]
    ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")


if __name__ == "__main__":
    main()
