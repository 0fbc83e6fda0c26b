#!/usr/bin/env python3
"""oc2asmpm with the end extension on the host threads (NECAT_ASM_ENDS_DEVICE=0) and on the device (=1), as a program, on bench.py's oc2asmpm set:
simulate_reads(5 Mb, 20 x, seed 71, err 0.03, repeat_frac 0.05), ASM_OVLP_OPTIONS (necat.pl:36), -t 16.  Per setting a warm-up run and three timed ones, the settings taking turns: wall and
the program's NECAT_CLI_TRACE phases (plan, aligner calls, end extension + records, output; with =1 the aligner calls contain the end extension), the md5 of the
records (all runs must agree), the device path's job counts, window histogram and tier counters, and the tier comparison: two tiers at NECAT_ASM_ENDS_DIAGS
128 / 64 / 32 against one tier (NECAT_ASM_ENDS_DIAGS = NECAT_DALIGN_DIAGS = 512).  --program PATH also times another build of oc2asmpm (the parent commit's) at the
default settings, for the baseline.  One JSON line to stdout and to profiles/asm_ends_bench.json.

    python tools/bench_asmpm.py [--genome 5000000] [--threads 16] [--runs 3] [--program PATH] [--out profiles/asm_ends_bench.json]"""
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

ARGS = "-n 100 -z 10 -b 2000 -e 0.5 -j 1 -u 0 -a 400".split()
PHASES = re.compile(r"votes \+ ranges \(device\) ([0-9.]+) s, (?:block aligner calls|aligner \+ end extension calls \(device ends\)) ([0-9.]+) s, "
                    r"(?:end extension \+ records|records) ([0-9.]+) s(?: \(\d+ host threads\))?, output ([0-9.]+) s")
VOLUME = re.compile(r"volume \d+: read ([0-9.]+) s, upload \+ index ([0-9.]+) s, one-byte codes ([0-9.]+) s")


def one_run(program, wrk, out, threads, env):
    t0 = time.time()
    r = subprocess.run([program] + ARGS + ["-t", str(threads), wrk, "0", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, NECAT_CLI_TRACE="1", **env))
    wall = time.time() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-400:])
    ph = PHASES.findall(r.stderr)
    vol = VOLUME.findall(r.stderr)
    res = {"wall_s": round(wall, 3), "md5": hashlib.md5(open(out, "rb").read()).hexdigest(),
           "plan_s": round(sum(float(p[0]) for p in ph), 3), "aligner_calls_s": round(sum(float(p[1]) for p in ph), 3),
           "ends_and_records_s": round(sum(float(p[2]) for p in ph), 3), "output_s": round(sum(float(p[3]) for p in ph), 3),
           "read_s": round(sum(float(v[0]) for v in vol), 3), "one_byte_codes_s": round(sum(float(v[2]) for v in vol), 3)}
    ends = {}
    for ln in r.stderr.splitlines():
        if "ends on the device:" in ln:
            for k, a, b in re.findall(r"(\w+)=(\d+)(?:\+(\d+))?(?= |$)", ln):
                if k == "max_diags":
                    ends[k] = max(ends.get(k, 0), int(a))
                elif b:
                    ends[k] = [x + y for x, y in zip(ends.get(k, [0, 0]), (int(a), int(b)))]
                else:
                    ends[k] = ends.get(k, 0) + int(a)
            for k, v in re.findall(r"(device_ms|host_ms)=([0-9.]+)", ln):
                ends[k] = round(ends.get(k, 0.0) + float(v), 2)
            h = re.search(r"hist=([0-9,]+)", ln)
            if h:
                ends["window_hist_log2"] = [x + y for x, y in zip(ends.get("window_hist_log2", [0] * 12), map(int, h.group(1).split(",")))]
    if ends:
        res["ends"] = ends
    return res


def summary(env, rs):
    keys = ("wall_s", "plan_s", "aligner_calls_s", "ends_and_records_s", "output_s", "read_s", "one_byte_codes_s")
    res = {"env": env, "walls_s": [r["wall_s"] for r in rs], "md5": sorted({r["md5"] for r in rs})}
    res.update({k: [r[k] for r in rs] for k in keys[1:]})
    if "ends" in rs[-1]:
        res["ends"] = rs[-1]["ends"]
        res["ends_device_ms"] = [r["ends"].get("device_ms") for r in rs]
    return res


def settings(wrk, out, threads, runs, which):
    """which: name -> (program, env).  A warm-up run of each (a short-lived process pays for the device memory it maps, the first one most), then `runs` rounds
    that take the settings in turn, so that what else the machine does meets all of them alike"""
    for program, env in which.values():
        one_run(program, wrk, out, threads, env)
    rs = {name: [] for name in which}
    for _ in range(runs):
        for name, (program, env) in which.items():
            rs[name].append(one_run(program, wrk, out, threads, env))
    return {name: summary(which[name][1], rs[name]) for name in which}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--program", default=None, help="another build of oc2asmpm to time at the default settings (the baseline)")
    ap.add_argument("--no-tiers", action="store_true", help="skip the tier comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asm_ends_bench.json"))
    args = ap.parse_args()
    from necat_amd import build, synth
    build.build_cli()
    tmp = tempfile.mkdtemp(prefix="necat_asm_bench_")
    rs = synth.simulate_reads(args.genome, 20.0, seed=71, err=0.03, repeat_frac=0.05)
    wrk = os.path.join(tmp, "vols")
    nv = synth.write_volume_dir(wrk, rs)
    out = os.path.join(tmp, "out.m4")
    res = {"reads": rs.nreads, "bases": rs.nbases, "volumes": nv, "threads": args.threads, "options": " ".join(ARGS), "runs": args.runs}
    which = {"host_ends": (build.OC2ASMPM, {"NECAT_ASM_ENDS_DEVICE": "0"}), "device_ends": (build.OC2ASMPM, {"NECAT_ASM_ENDS_DEVICE": "1"})}
    if args.program:
        which["baseline"] = (args.program, {})
    res.update(settings(wrk, out, args.threads, args.runs, which))
    if not args.no_tiers:
        tiers = {"one_tier_128": {"NECAT_ASM_ENDS_DIAGS": "128"}, "two_tiers_64": {"NECAT_ASM_ENDS_DIAGS": "64"}, "two_tiers_32": {"NECAT_ASM_ENDS_DIAGS": "32"},
                 "one_tier_512": {"NECAT_ASM_ENDS_DIAGS": "512"}}
        res["tiers"] = settings(wrk, out, args.threads, args.runs, {k: (build.OC2ASMPM, dict(v, NECAT_ASM_ENDS_DEVICE="1")) for k, v in tiers.items()})
    md5 = set(res["host_ends"]["md5"]) | set(res["device_ends"]["md5"])
    for k in ("baseline",):
        if k in res:
            md5 |= set(res[k]["md5"])
    for t in res.get("tiers", {}).values():
        md5 |= set(t["md5"])
    res["same_records"] = len(md5) == 1
    # the project's rule for a default: the device path's slowest run against the host path's fastest
    res["device_slowest_s"], res["host_fastest_s"] = max(res["device_ends"]["walls_s"]), min(res["host_ends"]["walls_s"])
    res["device_wins_by_the_rule"] = res["device_slowest_s"] < res["host_fastest_s"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if res["same_records"] else 1


if __name__ == "__main__":
    sys.exit(main())
