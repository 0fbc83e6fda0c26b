#!/usr/bin/env python3
"""oc2rm_worker with the rescue pair inside the walk on the host threads (NECAT_RM_RESCUE_DEVICE=0) and ahead of the walk on the device (=1), as a program, on a
long-indel set sized like bench.py's oc2asmpm set: simulate_reads(5 Mb, 20 x, seed 71, err 0.12) with add_long_indels(0.5, lo 300, hi 1500) on half of the reads,
the reference = the genome as four contigs; oc2rm_worker's default options, -t 16.  Per setting a warm-up run and three timed ones, the settings taking turns: wall,
the md5 of the records (all runs must agree) and, from the library's NECAT_TRACE=2 line of every volume, what necat_rm_stats holds - candidates, need (jobs
speculated), tried / rescued (what the walk consumed), who decided the two halves, the widest DALIGNER window, whether the words came to the host, the milliseconds
of the two device calls and of the walk.  --program PATH also times another build of oc2rm_worker (the parent commit's, next to its own library) at the default
settings, for the baseline.  One JSON line to stdout and to profiles/rm_rescue_bench.json.

    python tools/bench_rm.py [--genome 5000000] [--coverage 20] [--threads 16] [--runs 3] [--program PATH] [--out profiles/rm_rescue_bench.json]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRACE = re.compile(r"map_reference host: ([0-9.]+) ms, (\d+) candidates, (\d+) rescue attempts, (\d+) rescued, (\d+) records(?:; (\d+) need the pair, computed (ahead on the device|inside the walk): "
                   r"local (\d+) device \+ (\d+) host \((\d+) above the cap, (\d+) flagged; widest window (\d+)\) ([0-9.]+) ms, global (\d+) jobs, (\d+) device \+ (\d+) host, ([0-9.]+) ms; "
                   r"words (fetched|not fetched); walk ([0-9.]+) ms)?")


def one_run(program, args, out, env):
    t0 = time.time()
    r = subprocess.run([program] + args + [out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, NECAT_TRACE="2", **env))
    wall = time.time() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-400:])
    res = {"wall_s": round(wall, 3), "md5": hashlib.md5(open(out, "rb").read()).hexdigest()}
    st = {}
    add = lambda k, v: st.__setitem__(k, st.get(k, 0) + v)
    for m in TRACE.finditer(r.stderr):
        add("volumes", 1); add("host_stage_ms", float(m.group(1))); add("n_candidates", int(m.group(2))); add("n_tried", int(m.group(3))); add("n_rescued", int(m.group(4)))
        add("records", int(m.group(5)))
        if m.group(6) is None:          # a build from before necat_rm_stats (the baseline)
            continue
        add("n_need", int(m.group(6))); add("speculated_volumes", 1 if m.group(7).startswith("ahead") else 0)
        for k, g in (("n_dalign_device", 8), ("n_dalign_host", 9), ("n_dalign_over_cap", 10), ("n_dalign_selfcheck", 11), ("n_nw_jobs", 14), ("n_nw_device", 15), ("n_nw_host", 16)):
            add(k, int(m.group(g)))
        st["max_diags"] = max(st.get("max_diags", 0), int(m.group(12)))
        add("dalign_ms", float(m.group(13))); add("nw_ms", float(m.group(17))); add("words_fetched", 1 if m.group(18) == "fetched" else 0); add("replay_ms", float(m.group(19)))
    res["stats"] = {k: round(v, 2) if isinstance(v, float) else v for k, v in st.items()}
    print("[bench_rm] %s %s: %.3f s" % (os.path.relpath(program, ROOT), env, wall), file=sys.stderr, flush=True)
    return res


def settings(args, out, runs, which):
    """which: name -> (program, env).  A warm-up run of each (a short-lived process pays for the device memory it maps, the first one most), then `runs` rounds
    that take the settings in turn, so that what else the machine does meets all of them alike"""
    for program, env in which.values():
        one_run(program, args, out, env)
    rs = {name: [] for name in which}
    for _ in range(runs):
        for name, (program, env) in which.items():
            rs[name].append(one_run(program, args, out, env))
    return {name: {"env": which[name][1], "walls_s": [r["wall_s"] for r in rs[name]], "md5": sorted({r["md5"] for r in rs[name]}), "stats": rs[name][-1]["stats"],
                   "host_stage_ms": [r["stats"].get("host_stage_ms") for r in rs[name]]} for name in which}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--program", default=None, help="another build of oc2rm_worker to time at the default settings (the baseline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rm_rescue_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from necat_amd import build, synth
    build.build_cli()
    tmp = tempfile.mkdtemp(prefix="necat_rm_bench_")
    G = synth.make_genome(a.genome, 71, 0.05)
    rs = synth.add_long_indels(synth.simulate_reads(coverage=a.coverage, seed=71, err=0.12, genome=G), 0.5, seed=72, lo=300, hi=1500)
    wrk = os.path.join(tmp, "vols")
    nv = synth.write_volume_dir(wrk, rs)
    cuts = [0, a.genome * 4 // 15, a.genome * 8 // 15, a.genome * 11 // 15, a.genome]
    seqs = [G[cuts[i]:cuts[i + 1]] for i in range(4)]
    ref = os.path.join(tmp, "ref.vol")
    synth.write_volume(ref, np.concatenate(seqs), [len(x) for x in seqs], ["ctg%d" % i for i in range(4)])
    out = os.path.join(tmp, "out.m4")
    args = ["-i", "0", "-t", str(a.threads), wrk, ref]
    res = {"reads": rs.nreads, "bases": rs.nbases, "volumes": nv, "reference_bases": a.genome, "contigs": 4, "threads": a.threads, "options": "-i 0", "runs": a.runs}
    which = {"host_rescue": (build.OC2RM, {"NECAT_RM_RESCUE_DEVICE": "0"}), "device_rescue": (build.OC2RM, {"NECAT_RM_RESCUE_DEVICE": "1"})}
    if a.program:
        which["baseline"] = (a.program, {})
    res.update(settings(args, out, a.runs, which))
    md5 = set()
    for k in which:
        md5 |= set(res[k]["md5"])
    res["same_records"] = len(md5) == 1
    d = res["device_rescue"]["stats"]
    res["speculation_ratio"] = round(d["n_need"] / d["n_tried"], 4) if d.get("n_tried") else None
    res["widest_window"] = d.get("max_diags")
    # the project's rule for a default: the device path's slowest run against the host path's fastest
    res["device_slowest_s"], res["host_fastest_s"] = max(res["device_rescue"]["walls_s"]), min(res["host_rescue"]["walls_s"])
    res["device_wins_by_the_rule"] = res["device_slowest_s"] < res["host_fastest_s"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res["same_records"] else 1


if __name__ == "__main__":
    sys.exit(main())
