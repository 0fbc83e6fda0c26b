#!/usr/bin/env python
"""What working oc2cns in gathered chunks costs (NECAT_CNS_READS=gather), on the bench reads of tools/bench_cns.py: the program's wall time with the
read set merged, gathered in one chunk and gathered in about eight chunks - three runs each, taking turns, after a warm-up run - and the gather kernel's time
from HIP events beside the bytes it moved (necat_volume_gather_stats after one necat_volume_gather of all reads from the project's volumes).

    python tools/bench_cns_gather.py [genome_len coverage] [--threads N] [--out profiles/cns_gather_bench.json]
    python tools/bench_cns_gather.py [genome_len coverage] --across-limit DIR [--out ...]

--across-limit DIR: the same project with filler volumes of random pac bytes (reads of 10 kb) behind its own volume until reads_info.txt totals more than 2^32
bases, the candidate partition unchanged.  One run without the fillers, one with them (auto picks gather): the two output files must be equal; a run with
NECAT_CNS_READS=merged shows what the program did before ("volume too large").  About 1.1 GB of files under DIR.
One JSON line per leg; --out also writes them to a file."""
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from necat_amd import build, capi, synth  # noqa: E402

TRACE = re.compile(r"\[oc2cns\] partition (\d+): (\d+) chunks of at most (\d+) bases, (\d+) reads and (\d+) bases gathered in ([0-9.]+) ms \(the gather kernels: ([0-9.]+) ms\)")


def make_project(tmp, glen, cov, vol_size):
    """the bench reads as a volume directory + their candidate partition (this library's own seeding, role-swapped as oc2pcan does)"""
    import util
    rs = synth.simulate_reads(glen, cov, seed=7)
    wrk = os.path.join(tmp, "wrk")
    nv = synth.write_volume_dir(wrk, rs, vol_size)
    ctx = capi.Context(0)
    sizes = rs.sizes.astype(np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    vol = ctx.upload_volume(synth.pack_2bit(rs.codes), int(sizes.sum()), off, sizes)
    opt = capi.default_options(**dict(util.FAST, kmer_size=15, job=0))
    ix = ctx.build_index(vol, opt.kmer_size, opt.kmer_cnt_cutoff)
    c = ctx.find_candidates(ix, vol, vol, 0, 0, opt, True)
    ix.free()
    vol.free()
    can = os.path.join(tmp, "cands")
    util.write_partition(can, util.pcan_single_partition(capi.pack_candidates(c).tobytes()))
    # the gather kernel alone: every read of the project from its volume files into one volume
    vols, starts, at = [], [], 0
    for path, _, _ in capi.load_volumes_info(wrk)[2]:
        vols.append(ctx.load_volume(path))
        starts.append(at)
        at += vols[-1].nseq
    runs = []
    for _ in range(4):
        g = ctx.gather_volume(vols, starts, np.arange(at))
        ms, nb = ctx.gather_stats()
        runs.append((round(ms, 4), nb))
        g.free()
    for v in vols:
        v.free()
    ctx.close()
    kern = dict(leg="gather_kernel", volumes=nv, reads=int(at), bases=int(sizes.sum()), bytes_read_and_written=runs[-1][1], kernel_ms=[r[0] for r in runs[1:]],
                gb_per_s=[round(r[1] / r[0] / 1e6, 1) for r in runs[1:]])
    return wrk, can, int(sizes.sum()), os.path.getsize(can + ".p0") // 28, kern


def run(wrk, can, tmp, tag, threads, env, check=True):
    co, ro = os.path.join(tmp, "cns_" + tag), os.path.join(tmp, "raw_" + tag)
    t = time.time()
    r = subprocess.run([build.OC2CNS, "-t", str(threads), wrk, can, co, ro], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
    dt = time.time() - t
    if check and r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest() if os.path.exists(p) else None
    return dict(wall_s=round(dt, 2), rc=r.returncode, cns_md5=md5(co), raw_md5=md5(ro), trace=[m.groups() for m in TRACE.finditer(r.stderr)], stderr_tail=r.stderr[-300:])


def count_chunks(rec, sizes, bound):
    """cns_chunks.h's planner, counted only: templates in ascending order join a chunk until the reads it names pass the bound"""
    order = np.argsort(rec[:, 1], kind="stable")
    t, q = rec[order, 1], rec[order, 4]
    cuts = np.flatnonzero(np.diff(t)) + 1
    stamp = np.zeros(sizes.shape[0], dtype=np.int64)
    chunks, cur, nt = 1, 0, 0
    for b, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [t.shape[0]]])):
        ids = np.unique(np.concatenate([t[b:b + 1], q[b:e]]))
        fresh = ids[stamp[ids] != chunks]
        add = int(sizes[fresh].sum())
        if nt and cur + add > bound:
            chunks, cur, nt = chunks + 1, 0, 0
            fresh, add = ids, int(sizes[ids].sum())
        stamp[fresh] = chunks
        cur, nt = cur + add, nt + 1
    return chunks


def bound_for(can, wrk, want):
    """the largest bound that still gives `want` chunks or more (the reads a template's candidates name lie all over the id range, so the count is steep in the bound)"""
    rec = np.frombuffer(open(can + ".p0", "rb").read(), dtype="<u4").reshape(-1, 7)
    sizes = np.concatenate([synth.read_volume(p)[2] for p, _, _ in capi.load_volumes_info(wrk)[2]]).astype(np.int64)
    lo, hi = 1, int(sizes.sum())
    while hi - lo > max(1, hi // 1000):
        mid = (lo + hi) // 2
        if count_chunks(rec, sizes, mid) >= want:
            lo = mid
        else:
            hi = mid
    return lo, count_chunks(rec, sizes, lo)


def chunk_leg(wrk, can, tmp, total, threads):
    bound, n8 = bound_for(can, wrk, 8)
    legs = (("merged", dict(NECAT_CNS_READS="merged")), ("gather_1", dict(NECAT_CNS_READS="gather", NECAT_TRACE="2")),
            ("gather_8", dict(NECAT_CNS_READS="gather", NECAT_TRACE="2", NECAT_CNS_CHUNK_BASES=str(bound))))
    print("bound for about eight chunks: %d bases of %d (%d chunks planned)" % (bound, total, n8), file=sys.stderr)
    run(wrk, can, tmp, "warm", threads, legs[0][1])
    out = {name: dict(wall_s=[], chunks=None, gathered_bases=None, gather_ms=[], gather_kernel_ms=[]) for name, _ in legs}
    files = {}
    for it in range(3):
        for name, env in legs:
            r = run(wrk, can, tmp, name, threads, env)
            o = out[name]
            o["wall_s"].append(r["wall_s"])
            if r["trace"]:
                o["chunks"] = sum(int(t[1]) for t in r["trace"])
                o["gathered_bases"] = sum(int(t[4]) for t in r["trace"])
                o["gather_ms"].append(round(sum(float(t[5]) for t in r["trace"]), 2))
                o["gather_kernel_ms"].append(round(sum(float(t[6]) for t in r["trace"]), 3))
            files.setdefault(name, (r["cns_md5"], r["raw_md5"]))
    med = lambda x: sorted(x)[len(x) // 2]
    return dict(leg="chunks", host_threads=threads, runs=out, files_equal=len(set(files.values())) == 1,
                over_merged={k: round(med(out[k]["wall_s"]) / med(out["merged"]["wall_s"]), 4) for k in out})


def across_limit_leg(wrk, can, tmp, threads, where):
    """filler volumes behind the project's own, so that no id moves"""
    rng = np.random.default_rng(5)
    os.makedirs(where, exist_ok=True)
    base = run(wrk, can, tmp, "base", threads, dict(NECAT_TRACE="2"))
    nv, nr, vols = capi.load_volumes_info(wrk)
    total = 0
    for path, _, _ in vols:
        total += int(synth.read_volume(path)[2].sum())
    lines = open(os.path.join(wrk, "volume_names.txt")).read().splitlines()[:nv]
    per = 150_000                                   # reads of 10 kb per filler volume: 1.5 Gbp, 375 MB of pac
    k = 0
    while total < (1 << 32) + 10_000_000:
        n = min(per, ((1 << 32) + 10_000_000 - total + 9_999) // 10_000)
        path = os.path.join(where, "filler%d" % k)
        total += synth.write_filler_volume(path, "f%d" % k, n, 10_000, rng)
        lines.append("%s\t%d\t%d" % (path, nr, n))
        nr += n
        k += 1
    big = os.path.join(where, "wrk_big")
    os.makedirs(big, exist_ok=True)
    open(os.path.join(big, "volume_names.txt"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(big, "reads_info.txt"), "w").write("%d\t%d\t%d\n" % (len(lines), nr, total))
    over = run(big, can, tmp, "over", threads, dict(NECAT_TRACE="2"))
    old = run(big, can, tmp, "old", threads, dict(NECAT_CNS_READS="merged"), check=False)
    return dict(leg="across_limit", total_bases=total, volumes=len(lines), reads=nr, resident_device_bytes_of_the_volume_files=(total + 3) // 4,
                without_fillers=dict(wall_s=base["wall_s"], cns_md5=base["cns_md5"], raw_md5=base["raw_md5"]),
                with_fillers=dict(wall_s=over["wall_s"], cns_md5=over["cns_md5"], raw_md5=over["raw_md5"], trace=over["trace"]),
                files_equal=(base["cns_md5"], base["raw_md5"]) == (over["cns_md5"], over["raw_md5"]),
                merged_path=dict(rc=old["rc"], says=old["stderr_tail"].strip().splitlines()[-1] if old["stderr_tail"].strip() else ""))


def main():
    argv = sys.argv[1:]

    def opt(name, default=None):
        if name in argv:
            i = argv.index(name)
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        return default
    out_path = opt("--out")
    threads = int(opt("--threads", "16"))
    where = opt("--across-limit")
    glen = int(argv[0]) if len(argv) > 0 else 4_600_000
    cov = float(argv[1]) if len(argv) > 1 else 40.0
    import tempfile
    tmp = tempfile.mkdtemp(prefix="necat_cns_gather_")
    build.build_hip()
    build.build_cli()
    wrk, can, total, nrec, kern = make_project(tmp, glen, cov, max(1, int(glen * cov) // 3))
    lines = [dict(leg="project", genome=glen, coverage=cov, bases=total, records=nrec), kern]
    lines.append(across_limit_leg(wrk, can, tmp, threads, where) if where else chunk_leg(wrk, can, tmp, total, threads))
    for ln in lines:
        print(json.dumps(ln))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
