#!/usr/bin/env python
"""necat_ctg_consensus_batch (the consensus half of contig polishing) on one synthetic contig segment: its host path against its device path.

    python tools/bench_ctgcns.py [segment_bases coverage] [--out profiles/ctg_consensus_bench.json]

Input: one segment of 1 Mb (the reference's kCtgSegmentSize) with 1 % substitutions against the truth, reads of 8 kb at 15 x laid over it with generated column
strings (10 % errors in thirds: mismatch, query base over '-', '-' over target base).  No reference program is needed.  Three runs of path 1 (NECAT_CNS_THREADS
host threads, 16 unless the environment says otherwise - one segment is one thread's work) and three of path 0, wall clock of the whole call, with the plan, the
kernels' event times and the host's score pass listed apart, and whether the two paths' outputs are equal; one JSON line, also written to --out."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from necat_amd import capi, synth  # noqa: E402


def make_input(size, coverage, seed=11, read_len=8000, err=0.10, sub=0.01):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, size, dtype=np.uint8)
    contig = truth.copy()
    flip = rng.random(size) < sub
    contig[flip] = (contig[flip] + rng.integers(1, 4, int(flip.sum()), dtype=np.uint8)) & 3
    n = int(size * coverage / read_len)
    reads, ovl, blobs, n_ops = [], np.zeros(n, dtype=capi.CTG_OVERLAP_DTYPE), [], 0
    for k in range(n):
        a = int(rng.integers(0, max(1, size - read_len + 1)))
        b = min(size, a + read_len)
        L = b - a
        u = rng.random(L)
        kind = np.where(u < err / 3, 1, np.where(u < 2 * err / 3, 2, np.where(u < err, 3, 0)))          # 0 as the truth, 1 another base, 2 + an inserted base, 3 deleted
        base = truth[a:b].copy()
        m = kind == 1
        base[m] = (base[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
        first = np.where(kind == 3, 2, np.where(base == contig[a:b], 0, 3)).astype(np.uint8)
        reps = np.where(kind == 2, 2, 1)
        at = np.cumsum(reps) - reps
        ops = np.ones(int(reps.sum()), dtype=np.uint8)          # (the second column of a pair: a query base over '-')
        ops[at] = first
        q = rng.integers(0, 4, ops.shape[0], dtype=np.uint8)
        q[at] = base
        q = q[ops != 2]
        qdir = int(rng.integers(0, 2))
        reads.append((3 - q)[::-1] if qdir else q)
        blob = capi.pack_columns(ops)
        blob = np.concatenate([blob, np.zeros((-blob.shape[0]) % 8, dtype=np.uint8)])
        ovl[k] = (k, qdir, 0, q.shape[0], a, b, ops.shape[0], 0, n_ops)
        blobs.append(blob)
        n_ops += blob.shape[0]
    seg = np.zeros(1, dtype=capi.CTG_SEGMENT_DTYPE)
    seg[0] = (0, size, 0, 0, n)
    return contig, reads, seg, ovl, np.concatenate(blobs + [np.zeros(8, dtype=np.uint8)])


def upload(ctx, seqs):
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    codes = np.concatenate(seqs)
    return ctx.upload_volume(synth.pack_2bit(codes), int(codes.shape[0]), off, sizes)


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "ctg_consensus_bench.json")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    size = int(argv[0]) if len(argv) > 0 else 1_000_000
    cov = float(argv[1]) if len(argv) > 1 else 15.0
    os.environ.setdefault("NECAT_CNS_THREADS", "16")          # (a context reads its knobs when it is created)
    t = time.time()
    contig, reads, seg, ovl, ops = make_input(size, cov)
    ctx = capi.Context(0)
    rv, cv = upload(ctx, reads), upload(ctx, [contig])
    print("input: %d overlaps, %d columns (%.1f s)" % (ovl.shape[0], int(ovl["align_size"].sum()), time.time() - t), file=sys.stderr)
    out = dict(segment_bases=size, coverage=cov, overlaps=int(ovl.shape[0]), columns=int(ovl["align_size"].sum()), host_threads=int(ctx.knob("NECAT_CNS_THREADS")),
               tag_budget=int(ctx.knob("NECAT_CNS_TAG_BUDGET")), device=ctx.device_name())
    snap = {}
    for path, name in ((1, "host"), (0, "device")):
        walls, parts = [], []
        for it in range(3):
            t = time.time()
            r = ctx.ctg_consensus_batch(rv, 0, cv, seg, ovl, ops, capi.ctg_consensus_options(path=path))
            walls.append(round(time.time() - t, 3))
            if path == 0:
                parts.append(dict(plan_ms=round(r.plan_ms, 1), device_ms=round(r.device_ms, 1), kernel_ms={k: round(v, 2) for k, v in r.kernel_ms.items()}, score_ms=round(r.score_ms, 1)))
            else:
                parts.append(dict(plan_ms=round(r.plan_ms, 1), host_form_ms=round(r.host_ms, 1)))
            if it == 2:
                snap[name] = r.snapshot()
                s = r.segments[0]
                out.update(tags=int(s["n_tags"]), nodes=int(s["n_nodes"]), links=int(s["n_links"]), cns_bases=int(s["cns_len"]), polished_bases=int(s["polished_len"]))
                if path == 0:
                    out.update(ranges=int(r.n_chunks), n_fallback=int(r.n_fallback))
        out[name + "_wall_s"] = walls
        out[name + "_parts"] = parts
    out["outputs_equal"] = snap["host"] == snap["device"]
    out["device_slowest_beats_host_fastest"] = max(out["device_wall_s"]) < min(out["host_wall_s"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
