"""Helpers of the read trimming stage's tests (tests/test_trim.py, tests/test_gpu_trim.py): the golden cases of tests/golden/trim_f unpacked
into a work directory, the stage's programs, check_trim (tests/host_core/check_trim.cpp)."""
import gzip
import hashlib
import importlib.util
import json
import os
import subprocess

import numpy as np

from tests import util

GOLD = os.path.join(util.GOLDEN, "trim_f")
MANIFEST = json.load(open(os.path.join(util.GOLDEN, "manifest_trim.json")))
CSRC = os.path.join(util.ROOT, "necat_amd", "csrc")
PROG = {n: os.path.join(CSRC, n) for n in ("oc2pm4", "oc2lcr", "oc2etr", "oc2orderResults", "oc2asmpm", "oc2mkdb")}
CRAFT_RUNS = [(c, r) for c in sorted(MANIFEST["cases"]) for r in sorted(MANIFEST["cases"][c]["runs"])]

M4_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qoff", "<u8"), ("qend", "<u8"), ("qext", "<u8"), ("qsize", "<u8"),
                     ("sid", "<i4"), ("sdir", "<i4"), ("soff", "<u8"), ("send", "<u8"), ("sext", "<u8"), ("ssize", "<u8"),
                     ("ident_perc", "<f8"), ("vscore", "<i4"), ("_pad", "<i4")])


def generator():
    """tests/golden/make_golden_trim.py as a module (the fuzzer and the recipe that builds the reference's programs outside the repository)"""
    spec = importlib.util.spec_from_file_location("make_golden_trim", os.path.join(util.GOLDEN, "make_golden_trim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def gunzip(name, dst):
    with gzip.open(os.path.join(GOLD, name), "rb") as f:
        data = f.read()
    with open(dst, "wb") as g:
        g.write(data)
    return dst


def golden_bytes(name):
    p = os.path.join(GOLD, name)
    return gzip.open(p, "rb").read() if name.endswith(".gz") else open(p, "rb").read()


def write_reads_info(d, num_reads):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "reads_info.txt"), "w") as f:
        f.write("1\t%d\n" % num_reads)


def case_entry(case):
    return MANIFEST["natural"] if case == "nat" else MANIFEST["cases"][case]


def install_input(case, d):
    """the case's record file + reads_info.txt in d; (wrk dir, m4 path, num_reads)"""
    e = case_entry(case)
    stem = "nat.m4" if case == "nat" else "craft_%s.m4" % case
    write_reads_info(str(d), e["num_reads"])
    return str(d), gunzip(stem + ".gz", os.path.join(str(d), stem)), e["num_reads"]


def install_partitions(case, d):
    """.. + the reference's partition files (.partitions, .p<i>; the empty ones as empty files)"""
    wrk, m4, num_reads = install_input(case, d)
    e = case_entry(case)
    n = e["partition_records"]
    with open(m4 + ".partitions", "w") as f:
        f.write("%d\n" % len(n))
    for p, cnt in enumerate(n):
        if cnt:
            gunzip(os.path.basename(m4) + ".p%d.gz" % p, "%s.p%d" % (m4, p))
            assert os.path.getsize("%s.p%d" % (m4, p)) == 96 * cnt
        else:
            open("%s.p%d" % (m4, p), "wb").close()
    return wrk, m4, num_reads


def golden_ranges_text(case, run=""):
    """the reference's clipped_ranges.txt of a run, whole (a sparse golden is filled in and checked against its sha256)"""
    if case == "nat":
        return golden_bytes("nat.ranges.txt")
    r = MANIFEST["cases"][case]["runs"][run]
    data = golden_bytes(r["ranges"])
    if "sparse" not in r:
        return data
    have = {int(ln.split(b"\t")[0]): ln for ln in data.splitlines(keepends=True)}
    full = b"".join(have.get(i, b"%d\t-1\t0\t0\n" % i) for i in range(r["sparse"]["lines"]))
    assert hashlib.sha256(full).hexdigest() == r["sparse"]["sha256"]
    return full


def ranges_of_text(text):
    lines = text.decode().splitlines()
    assert lines[0] == "0\t0\t0\t0"
    return {int(a): (int(b), int(c), int(d)) for a, b, c, d in (ln.split("\t") for ln in lines[1:])}


def run_args(case, run=""):
    return (MANIFEST["natural"]["lcr_args"] if case == "nat" else MANIFEST["cases"][case]["runs"][run]["args"]).split()


def host_cap(case, run=""):
    return MANIFEST["natural"]["host_cap"] if case == "nat" else sum(MANIFEST["cases"][case]["runs"][run]["host_cap"].values())


def prog(name, args, env=None, check=True):
    r = subprocess.run([PROG[name]] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    if check:
        assert r.returncode == 0, "%s %s: exit %d\n%s" % (name, " ".join(str(a) for a in args), r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r


def build_check_trim(d):
    exe = os.path.join(str(d), "check_trim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(util.ROOT, "tests", "host_core", "check_trim.cpp")], check=True)
    return exe


def check_rows(exe, m4, num_reads, args, seed=1):
    """{read: ((left, right, size, how, reason) of trim_core.h, (left, right, size, how) of the kernel's core run lane by lane)}"""
    r = subprocess.run([exe, m4, str(num_reads)] + list(args) + [str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    rows = {}
    for ln in r.stdout.decode().splitlines():
        h, d = ln.split("|")
        h = [int(x) for x in h.split()]
        rows[h[0]] = (tuple(h[1:6]), tuple(int(x) for x in d.split()))
    return rows


def rec_rows(a):
    """records as sortable tuples of all fourteen fields"""
    return sorted(zip(*[a[n].tolist() for n in M4_DTYPE.names if n != "_pad"]))
