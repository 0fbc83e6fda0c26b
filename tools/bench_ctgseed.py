#!/usr/bin/env python
"""necat_ctg_seed_batch (the seeding of contig polishing) on synthetic contig segments: its host path against its device path.

    python tools/bench_ctgseed.py [--out profiles/ctg_seed_bench.json]
    python tools/bench_ctgseed.py --reference-reads N [--out FILE]       (no GPU: the reference's own functions, one thread)

Input: one segment of 1 Mb with reads of 10 kb at 12 % error (thirds: mismatch, inserted base, deleted base) and 15 x, and one of 1.5 Mb at 40 x; every read is a
job on the strand it was read from.  Per setting a warm-up call of each path, then three runs of path 1 (16 host threads unless the environment says otherwise)
and three of path 0, taking turns; wall clock of the whole call, the kernels' event times, the largest seed and match lists, the share of jobs per tier, and
whether the two paths' outputs are equal.  One JSON line, also written to --out.
--reference-reads N: where the reference's sources are present, its MaximalExactMatchWorkData_Init and N calls of _FindCandidates on the first setting's input through
tests/golden/ctg_seed_ref_harness.c, on one thread - how ctgcns runs a segment; a CPU figure of the machine it runs on, not comparable run for run."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(size, coverage, seed=11, read_len=10000, err=0.12):
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size, dtype=np.uint8)
    n = int(size * coverage / read_len)
    reads, qdirs = [], []
    for _ in range(n):
        a = int(rng.integers(0, max(1, size - read_len + 1)))
        base = contig[a:a + read_len].copy()
        u = rng.random(base.shape[0])
        sub = u < err / 3
        base[sub] = (base[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
        reps = np.where(u < err / 3, 1, np.where(u < 2 * err / 3, 2, np.where(u < err, 0, 1)))
        q = np.repeat(base, reps)
        second = np.cumsum(reps)[reps == 2] - 1          # the inserted base of a pair
        q[second] = rng.integers(0, 4, second.shape[0], dtype=np.uint8)
        qdir = int(rng.integers(0, 2))
        reads.append((3 - q)[::-1].astype(np.uint8) if qdir else q)
        qdirs.append(qdir)
    return contig, reads, qdirs


def upload(ctx, seqs):
    from necat_amd import synth
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    codes = np.concatenate(seqs)
    return ctx.upload_volume(synth.pack_2bit(codes), int(codes.shape[0]), off, sizes)


def one_setting(ctx, size, cov):
    from necat_amd import capi
    t = time.time()
    contig, reads, qdirs = make_input(size, cov)
    rv, cv = upload(ctx, reads), upload(ctx, [contig])
    n = len(reads)
    seg = np.zeros(1, dtype=capi.CTG_SEGMENT_DTYPE)
    seg[0] = (0, size, 0, 0, n)
    jobs = np.zeros(n, dtype=capi.CTG_SEED_JOB_DTYPE)
    jobs["qid"] = np.arange(n); jobs["qdir"] = qdirs
    print("input: %d bases, %d reads (%.1f s)" % (size, n, time.time() - t), file=sys.stderr)
    out = dict(segment_bases=size, coverage=cov, jobs=n, read_bases=int(sum(r.shape[0] for r in reads)))
    walls, parts, snap = {0: [], 1: []}, {0: [], 1: []}, {}
    for it in range(4):          # 0: the warm-up
        for path in (1, 0):
            t = time.time()
            r = ctx.ctg_seed_batch(rv, 0, cv, seg, jobs, capi.ctg_seed_options(path=path))
            w = time.time() - t
            if it == 0:
                continue
            walls[path].append(round(w, 4))
            if path == 0:
                parts[0].append(dict(device_ms=round(r.device_ms, 2), kernel_ms={k: round(v, 2) for k, v in r.kernel_ms.items()}, fallback_ms=round(r.host_ms, 2)))
            else:
                parts[1].append(dict(host_form_ms=round(r.host_ms, 1)))
            snap[path] = r.snapshot()
            if path == 0:
                out.update(found=int(r.jobs["found"].sum()), max_matches=r.max_matches, max_mems=r.max_mems, mean_matches=round(float(r.jobs["n_matches"].mean()), 1),
                           mean_mems=round(float(r.jobs["n_mems"].mean()), 1), jobs_lds=r.n_lds, jobs_scratch=r.n_scratch, jobs_host=r.n_fallback)
    out.update(host_wall_s=walls[1], device_wall_s=walls[0], host_parts=parts[1], device_parts=parts[0], outputs_equal=snap[0] == snap[1],
               device_slowest_beats_host_fastest=max(walls[0]) < min(walls[1]))
    rv.free(); cv.free()
    return out


def reference(n_reads, size=1_000_000, cov=15.0):
    from tests import ctg_seed_cases as sc
    assert sc.have_reference(), "the reference's sources are needed"
    contig, reads, qdirs = make_input(size, cov)
    with tempfile.TemporaryDirectory() as tmp:
        exe = sc.build_harness(os.path.join(tmp, "harness"))
        times = []
        for n in (0, n_reads):
            inp = os.path.join(tmp, "in.bin")
            with open(inp, "wb") as f:
                f.write(b"S" + np.int32(size).tobytes() + contig.tobytes())
                for r, d in list(zip(reads, qdirs))[:n]:
                    s = (3 - r)[::-1].astype(np.uint8) if d else r
                    f.write(b"R" + np.int32(s.shape[0]).tobytes() + s.tobytes())
            t = time.time()
            subprocess.run([exe, inp], check=True, stdout=subprocess.DEVNULL)
            times.append(time.time() - t)
    return dict(reference_cpu_one_thread=dict(segment_bases=size, reads=n_reads, init_s=round(times[0], 3), per_read_ms=round(1e3 * (times[1] - times[0]) / n_reads, 2),
                                              note="the reference's own functions through the test harness on the build machine's CPU: another machine than the GPU host's"))


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "ctg_seed_bench.json")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    if "--reference-reads" in argv:
        out = reference(int(argv[argv.index("--reference-reads") + 1]))
    else:
        from necat_amd import capi
        os.environ.setdefault("NECAT_CNS_THREADS", "16")          # (a context reads its knobs when it is created)
        ctx = capi.Context(0)
        out = dict(device=ctx.device_name().strip(), host_threads=int(ctx.knob("NECAT_CNS_THREADS")), lds_matches=int(ctx.knob("NECAT_CTG_SEED_LDS")),
                   seed_budget=int(ctx.knob("NECAT_CTG_SEED_BUDGET")), job_max_seeds=int(ctx.knob("NECAT_CTG_SEED_JOB_MAX")))
        out["settings"] = [one_setting(ctx, size, cov) for size, cov in ((1_000_000, 15.0), (1_500_000, 40.0))]
        out["device_slowest_beats_host_fastest"] = all(s["device_slowest_beats_host_fastest"] for s in out["settings"])
        ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")


if __name__ == "__main__":
    main()
