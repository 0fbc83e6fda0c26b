#!/usr/bin/env python
"""Golden vectors for the read trimming stage (oc2pm4, oc2lcr, oc2etr, oc2orderResults), generated from the REFERENCE ITSELF.

Run in the build container only.  The reference's four programs are compiled from /root/reference/src with plain gcc lines into a
temporary directory OUTSIDE the repository (build_reference below; the tree builds no new reference binary) and run with num_threads = 1;
oracle/_ref/oc2mkdb and oracle/_ref/oc2asmpm (`make -C oracle ref`) make the natural set's volumes and overlaps.  Committed is data only,
under tests/golden/trim_f/ (+ manifest_trim.json); binary record files and FASTA are stored gzip-compressed to stay small:

  craft_<case>.m4.gz                 crafted 96-byte records (fuzz_case below: every branch of the per-read decision is taken)
  craft_<case>.m4.p<i>.gz            the reference oc2pm4's partition files (empty ones are not stored; the manifest lists them)
  craft_<case>.ranges[.<run>].txt    the reference oc2lcr's clipped_ranges.txt, one per run (a run = one set of oc2lcr arguments); for the case with
                                     100 000 reads without a record only the lines other than "id -1 0 0" (+ the whole file's sha256 in the manifest)
  nat.reads.fasta.gz                 the natural set: corrected-read-like reads named 1..N, some chimeric, some with adapters at an end
  nat.m4.gz, nat.m4.p0.gz            reference oc2asmpm records of its volumes, the reference's partition
  nat.ranges.txt, nat.tmp_pm.m4.gz, nat.pm.m4.gz     reference oc2lcr / oc2etr / oc2orderResults outputs (text)
  (complete / uncomplete / trimReads FASTA: whole reads and substrings of nat.reads - the manifest holds their sha256 and sizes)

    python tests/golden/make_golden_trim.py

fuzz_case / build_reference / run_reference_case are also what tests/test_trim.py uses for its live comparison on fresh seeds where the
reference's sources are present.
"""
import glob
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "trim_f")
REF_SRC = "/root/reference/src"

M4_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qoff", "<u8"), ("qend", "<u8"), ("qext", "<u8"), ("qsize", "<u8"),
                     ("sid", "<i4"), ("sdir", "<i4"), ("soff", "<u8"), ("send", "<u8"), ("sext", "<u8"), ("ssize", "<u8"),
                     ("ident_perc", "<f8"), ("vscore", "<i4"), ("_pad", "<i4")])
assert M4_DTYPE.itemsize == 96

# the crafted cases: fuzz_case arguments, oc2pm4's cutoff, and the oc2lcr runs (error_cutoff min_ovlp_size min_cov min_read_size)
CASES = {
    "main": dict(seed=11, kind="main", pm4_cutoff="0.1", runs={"": "0.1 1 1 1000"}),
    "ovlp500": dict(seed=12, kind="main", scale=0.5, pm4_cutoff="0.1", runs={"": "0.1 500 1 1000", "cov2": "0.1 500 2 1000"}),
    "stale": dict(seed=13, kind="stale", scale=0.5, pm4_cutoff="0.1", runs={"": "0.05 1 1 1000"}),
    "twoparts": dict(seed=14, kind="twoparts", scale=0.35, pm4_cutoff="0.1", runs={"": "0.1 1 1 1000"}),
}
NAT = dict(genome=36_000, coverage=20.0, seed=77, asm_args="-n 100 -z 10 -b 2000 -e 0.5 -j 1 -u 1 -a 400", lcr_args="0.1 1 1 1000")
HOW = {0: "none", 1: "complete", 2: "chimeric", 3: "cover", 4: "host"}
REASON = {1: "a", 2: "b", 3: "c"}


# ---------------------------------------------------------------------------------------------------------------- the reference's programs

def build_reference(outdir):
    """the reference's oc2pm4, oc2lcr, oc2etr, oc2orderResults, compiled into outdir (outside the repository); {name: path}"""
    src = REF_SRC
    os.makedirs(outdir, exist_ok=True)
    lib = [f for f in sorted(glob.glob(os.path.join(src, "common", "*.c"))) if os.path.basename(f) != "main.c"]
    lib += [os.path.join(src, "klib", "kstring.c"), os.path.join(src, "klib", "kalloc.c")] + sorted(glob.glob(os.path.join(src, "tasc", "*.c")))
    lib += [os.path.join(src, "edlib", "edlib_wrapper.c")]
    edlib_o = os.path.join(outdir, "edlib.o")
    subprocess.run(["g++", "-O2", "-w", "-c", os.path.join(src, "edlib", "edlib.cpp"), "-o", edlib_o], check=True)
    tb = lambda *names: [os.path.join(src, "trim_bases", n + ".c") for n in names]
    progs = {
        "oc2pm4": tb("pm4_aux", "pm4_main"),
        "oc2lcr": tb("pm4_aux", "detect_chimeric_reads", "range_list", "largest_cover_range", "largest_cover_range_main"),
        "oc2etr": tb("extract_trimmed_reads", "largest_cover_range", "range_list", "detect_chimeric_reads", "pm4_aux"),
        "oc2orderResults": tb("order_results"),
    }
    out = {}
    for name, extra in progs.items():
        out[name] = os.path.join(outdir, name)
        subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-pthread", "-o", out[name]] + lib + extra + [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    return out


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(cmd), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r


def write_reads_info(d, num_reads):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "reads_info.txt"), "w") as f:
        f.write("1\t%d\n" % num_reads)


def run_reference_case(ref, wrk, m4_path, num_reads, pm4_cutoff, runs):
    """reference oc2pm4 (one thread) on m4_path, then oc2lcr once per run; {run: ranges path}"""
    write_reads_info(wrk, num_reads)
    run([ref["oc2pm4"], wrk, m4_path, pm4_cutoff, "1"])
    out = {}
    for name, args in runs.items():
        a = args.split()
        out[name] = m4_path + ".ranges" + ("." + name if name else "") + ".txt"
        run([ref["oc2lcr"], m4_path, wrk, a[0], a[1], a[2], a[3], "1", out[name]])
    return out


# ---------------------------------------------------------------------------------------------------------------- crafted records

class Craft:
    def __init__(self, seed, first_id=1):
        self.rng = np.random.default_rng(seed)
        self.rows = []
        self.size = {}
        self.next_id = first_id

    def new_read(self, lo=3000, hi=12000, size=None):
        i = self.next_id
        self.next_id += 1
        self.size[i] = int(size if size is not None else self.rng.integers(lo, hi))
        return i

    def rec(self, q, s, qdir, qoff, qend, soff, send, ident=None, vscore=None, sdir=0):
        r = self.rng
        qoff, qend = max(0, int(qoff)), min(self.size[q], int(qend))
        soff, send = max(0, int(soff)), min(self.size[s], int(send))
        if ident is None:
            ident = float(r.integers(9000, 10000)) / 100.0
        if vscore is None:
            vscore = int(r.integers(100, 100000))
        self.rows.append((q, qdir, qoff, qend, qoff, self.size[q], s, sdir, soff, send, soff, self.size[s], ident, vscore, 0))

    def array(self, shuffle=True):
        a = np.array(self.rows, dtype=M4_DTYPE)
        if shuffle:
            self.rng.shuffle(a)
        return a


def fuzz_case(seed, kind="main", scale=1.0):
    """(records, num_reads) for one crafted case.  Subjects are crafted read by read against `filler` queries, whose own lists are whatever the
    exchanged copies make them; a block of random overlaps between a third set of reads adds unplanned combinations."""
    first = 100_001 if kind == "twoparts" else 1
    c = Craft(seed, first)
    r = c.rng
    n = lambda k: max(1, int(round(k * scale)))
    low_ident = kind == "stale"
    filler = [c.new_read(1500, 9000) for _ in range(n(60))]
    fq = lambda: int(filler[int(r.integers(0, len(filler)))])
    ident = lambda: (float(r.integers(9000, 9500)) / 100.0 if (low_ident and r.random() < 0.02) else float(r.integers(9500, 10000)) / 100.0) if low_ident else None

    def interior(s, k, lo_frac=0.05, hi_frac=0.9):
        """k overlaps strictly inside the subject (never complete)"""
        L = c.size[s]
        for _ in range(k):
            a = int(r.integers(int(L * lo_frac) + 21, int(L * hi_frac)))
            b = min(L - 25, a + int(r.integers(300, max(301, L // 2))))
            if b - a < 50:
                continue
            q = fq()
            qa = int(r.integers(0, max(1, c.size[q] - 200)))
            c.rec(q, s, int(r.integers(0, 2)), qa, qa + (b - a), a, b, ident=ident(), sdir=int(r.random() < 0.1))

    # complete by one record (ends 0 .. 20 off; 21 is not complete)
    for k in range(n(26)):
        s = c.new_read()
        L = c.size[s]
        interior(s, int(r.integers(0, 8)))
        l, rr = int(r.integers(0, 21)), int(r.integers(0, 21))
        if k % 9 == 8:
            l = 21                      # one base too many: decided by the cover range instead
        q = fq()
        c.rec(q, s, int(r.integers(0, 2)), 0, L - l - rr, l, L - rr, ident=ident())
    # chimeric, case I: a query on both strands, together on >= 0.9 of the subject, sharing < 0.4 of either target range
    for k in range(n(34)):
        s = c.new_read(6000, 12000)
        L = c.size[s]
        interior(s, int(r.integers(0, 5)), 0.3, 0.6)
        pairs = 2 + int(r.integers(0, 2)) if k % 6 != 5 else 1          # one pair alone does not make a chimera
        for _ in range(pairs):
            q = c.new_read(size=int(L * 0.7))
            mid = int(L * (0.45 + 0.1 * r.random()))
            ov = int(r.integers(0, 3)) * int(r.integers(0, int(0.2 * L)))
            t1 = (int(L * 0.03) + int(r.integers(-30, 30)) + 21, mid + ov // 2)
            t2 = (mid - ov // 2, L - int(L * 0.03) - 21 + int(r.integers(-30, 30)))
            if k % 5 == 0:              # around the 0.9 threshold of the mapped target bases
                t1 = (30, mid); t2 = (mid, 30 + int(L * 0.9) + int(r.integers(-2, 3)))
            qlen = int(c.size[q] * 0.8)
            q0 = int(r.integers(0, c.size[q] - qlen))
            jit = int(r.integers(0, int(qlen * 0.12)))                  # around the 0.9 threshold of the shared query bases
            c.rec(q, s, 0, q0, q0 + qlen, t1[0], t1[1], ident=ident())
            c.rec(q, s, 1, q0 + jit, q0 + jit + qlen - int(r.integers(0, int(qlen * 0.11))), t2[0], t2[1], ident=ident())
    # chimeric, case II: most of a short query twice, on target ranges at most 1000 apart
    for k in range(n(30)):
        s = c.new_read(7000, 12000)
        L = c.size[s]
        interior(s, int(r.integers(0, 4)), 0.1, 0.3)
        for _ in range(2 + int(r.integers(0, 2))):
            q = c.new_read(size=int(r.integers(1500, 2500)))
            Q = c.size[q]
            a = int(r.integers(200, L // 3))
            gap = int(r.integers(990, 1012)) if k % 2 else int(r.integers(-400, 900))
            qa, qb = int(Q * 0.02), int(Q * (0.9 + 0.09 * r.random())) + int(r.integers(-40, 10))
            c.rec(q, s, 0, qa, qb, a, a + (qb - qa), ident=ident())
            c.rec(q, s, 1, qa + int(r.integers(0, 30)), qb, a + (qb - qa) + gap, a + 2 * (qb - qa) + gap, ident=ident())
    # cover range: gaps, containment, ranges starting at 0, abutting ranges, overlaps around 500
    for k in range(n(44)):
        s = c.new_read()
        L = c.size[s]
        m = k % 6
        if m == 0:
            interior(s, int(r.integers(2, 14)))
        elif m == 1:                    # pieces that abut or overlap by 0 .. 2 / 498 .. 502 bases, one of them from 0
            at = 0 if k % 12 == 1 else int(r.integers(30, 300))
            while at < L - 1200:
                ln = int(r.integers(600, 2500))
                q = fq()
                c.rec(q, s, int(r.integers(0, 2)), 0, ln, at, min(L - 30, at + ln), ident=ident())
                step = [0, 1, 2, 498, 499, 500, 501, 502, -1, -300][int(r.integers(0, 10))]
                at = at + ln - step
        elif m == 2:                    # containment + a far piece
            q = fq()
            c.rec(q, s, 0, 0, 3000, 100, min(L - 40, 3100), ident=ident())
            for _ in range(int(r.integers(1, 6))):
                a = int(r.integers(100, 2000))
                c.rec(fq(), s, 1, 0, 500, a, a + int(r.integers(100, 900)), ident=ident())
            if L > 5000:
                c.rec(fq(), s, 0, 0, 800, L - 1500, L - 700, ident=ident())
        elif m == 3:                    # several ranges from 0, and a zero-length one at 0
            for _ in range(int(r.integers(1, 4))):
                c.rec(fq(), s, 0, 0, 900, 0, int(r.integers(400, L - 100)), ident=ident())
            if k % 2:
                c.rec(fq(), s, 0, 0, 0, 0, 0, ident=ident())
            interior(s, int(r.integers(0, 4)))
        elif m == 4:                    # deep pile: many overlaps on one region, few elsewhere
            a = int(r.integers(100, L // 2))
            for _ in range(int(r.integers(20, 60))):
                c.rec(fq(), s, int(r.integers(0, 2)), 0, 1500, a + int(r.integers(-80, 80)), a + 1500 + int(r.integers(-80, 80)), ident=ident())
            interior(s, 3)
        else:                           # shorter than min_size: invalid in the last pass
            a = int(r.integers(100, L - 1100))
            c.rec(fq(), s, 0, 0, 900, a, a + int(r.integers(200, 1003)), ident=ident())
    # more than 300 records: the 300 best by identity, with and without a tie at the boundary
    for k in range(n(6)):
        s = c.new_read(8000, 12000)
        L = c.size[s]
        cnt = int(r.integers(301, 401))
        base = [float(x) / 100.0 for x in r.integers(9100, 10000, size=cnt)]
        if k % 2:
            srt = sorted(base, reverse=True)
            base[base.index(srt[300])] = srt[299]                        # 300th == 301st
        qs = [c.new_read(1500, 3000) for _ in range(8)]
        for i in range(cnt):
            a = int(r.integers(25, L - 2100))
            c.rec(qs[i % 8], s, int(r.integers(0, 2)), 0, 1800, a, a + int(r.integers(500, 2000)), ident=base[i])
    # equal top vscores in a group with both strands
    for k in range(n(8)):
        s = c.new_read(6000, 12000)
        L = c.size[s]
        interior(s, int(r.integers(1, 6)))
        q = c.new_read(size=int(L * 0.7))
        v = int(r.integers(1000, 50000))
        c.rec(q, s, 0, 100, 3000, 40, 2940, vscore=v, ident=ident())
        c.rec(q, s, 0, 150, 3100, 200 + int(r.integers(0, 500)), 3150, vscore=v, ident=ident())
        c.rec(q, s, 1, 120, 3000, 3000, L - 40, vscore=v - int(r.integers(0, 2)) * 7, ident=ident())
        if k % 2:
            c.rec(q, s, 1, 130, 3000, 2900, L - 60, vscore=v - 7, ident=ident())
    # reads nothing overlaps
    for _ in range(n(8)):
        c.new_read()
    # unplanned: random overlaps among a third set of reads
    pool = [c.new_read() for _ in range(n(50))]
    for _ in range(n(500)):
        q, s = int(pool[int(r.integers(0, len(pool)))]), int(pool[int(r.integers(0, len(pool)))])
        if q == s:
            continue
        ln = int(r.integers(400, 6000))
        qa, sa = int(r.integers(0, max(1, c.size[q] - 300))), int(r.integers(0, max(1, c.size[s] - 300)))
        c.rec(q, s, int(r.integers(0, 2)), qa, qa + ln, sa, sa + ln, ident=ident(), vscore=int(r.integers(100, 130)), sdir=int(r.random() < 0.1))
    if kind == "twoparts":              # a few records of reads of the first partition
        lowr = []
        for i in (5, 6, 7, 99_999):
            c.size[i] = 5000
            lowr.append(i)
        c.rec(5, 6, 0, 10, 4990, 5, 4990)
        c.rec(6, 7, 1, 100, 3000, 1000, 3900)
        c.rec(int(pool[0]), 99_999, 0, 0, 2500, 1000, 3500)
        c.rec(7, int(pool[1]), 1, 0, 2500, 50, 2550)
    return c.array(), c.next_id - 1


# ---------------------------------------------------------------------------------------------------------------- this tree's classification

def build_check_trim(outdir):
    exe = os.path.join(outdir, "check_trim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_core", "check_trim.cpp")], check=True)
    return exe


def check_rows(exe, m4_path, num_reads, args, seed=1):
    """check_trim's table: per read (host left right size how reason, kernel core left right size how)"""
    a = args.split()
    r = run([exe, m4_path, str(num_reads), a[0], a[1], a[2], a[3], str(seed)])
    rows = {}
    for ln in r.stdout.decode().splitlines():
        h, d = ln.split("|")
        h = [int(x) for x in h.split()]
        rows[h[0]] = (tuple(h[1:6]), tuple(int(x) for x in d.split()))
    return rows


def read_ranges(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        lines = f.read().splitlines()
    assert lines[0] == "0\t0\t0\t0", lines[0]
    return {int(a): (int(b), int(c), int(d)) for a, b, c, d in (ln.split("\t") for ln in lines[1:])}


def census(rows, ranges):
    """trim_core.h must reproduce the reference on every read before its classification counts; then the case's census"""
    cnt = {"complete": 0, "chimeric": 0, "cover": 0, "none": 0, "a": 0, "b": 0, "c": 0, "invalid": 0}
    for i, want in ranges.items():
        host, _ = rows[i]
        if tuple(host[:3]) != want:
            raise AssertionError("read %d: trim_core.h %r, reference %r" % (i, host[:3], want))
        if host[4]:
            cnt[REASON[host[4]]] += 1
        else:
            cnt[HOW[host[3]]] += 1
        cnt["invalid"] += want[0] < 0
    return cnt


# ---------------------------------------------------------------------------------------------------------------- the natural set

def natural_reads(genome, coverage, seed):
    """corrected-read-like reads named 1..N; 8 % joined with their own reverse complement or another read, 14 % with random bases at an end"""
    sys.path.insert(0, ROOT)
    from necat_amd import synth
    rs = synth.simulate_reads(genome, coverage, seed=seed, err=0.02, mean_len=9000, sd_len=3000)
    rng = np.random.default_rng(seed + 5)
    reads = [rs.read(i).copy() for i in range(rs.nreads)]
    out = []
    for i, x in enumerate(reads):
        u = rng.random()
        if u < 0.08:
            other = (3 - x)[::-1] if rng.random() < 0.5 else reads[int(rng.integers(0, len(reads)))]
            cut = int(rng.integers(len(other) // 3, len(other)))
            x = np.concatenate([x, other[:cut]])
        elif u < 0.22:
            junk = rng.integers(0, 4, size=int(rng.integers(30, 601))).astype(np.uint8)
            x = np.concatenate([junk, x]) if rng.random() < 0.5 else np.concatenate([x, junk])
        out.append(x)
    return out


def write_fasta(path, reads, names=None):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, x in enumerate(reads):
            f.write(b">%s\n" % (names[i].encode() if names else b"%d" % (i + 1)))
            f.write(lut[x].tobytes())
            f.write(b"\n")


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def gz_to(src, dst):
    with open(src, "rb") as f, open(dst, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as g:
            g.write(f.read())


def main():
    ref_bin = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.isdir(REF_SRC) or not os.path.exists(os.path.join(ref_bin, "oc2asmpm")):
        sys.exit("the reference's sources and oracle/_ref are needed: run in the build container after `make -C oracle ref`")
    tmp = tempfile.mkdtemp(prefix="golden_trim_")          # outside the repository: reference binaries never enter it
    ref = build_reference(os.path.join(tmp, "refbin"))
    chk = build_check_trim(tmp)
    manifest = {"cases": {}, "natural": {}}
    staged = []                                             # (source, name under trim_f) - written only when every condition holds
    total = {"complete": 0, "chimeric": 0, "cover": 0, "a": 0, "b": 0, "c": 0, "invalid": 0}
    for name, cs in CASES.items():
        recs, num_reads = fuzz_case(cs["seed"], cs["kind"], cs.get("scale", 1.0))
        wrk = os.path.join(tmp, "craft_" + name)
        os.makedirs(wrk)
        m4 = os.path.join(wrk, "craft_%s.m4" % name)
        recs.tofile(m4)
        ranges = run_reference_case(ref, wrk, m4, num_reads, cs["pm4_cutoff"], cs["runs"])
        np_ = int(open(m4 + ".partitions").read())
        entry = {"num_reads": num_reads, "records": int(recs.shape[0]), "pm4_cutoff": cs["pm4_cutoff"], "partitions": np_, "partition_records": [], "runs": {}}
        staged.append((m4, "craft_%s.m4.gz" % name))
        for p in range(np_):
            pf = "%s.p%d" % (m4, p)
            entry["partition_records"].append(os.path.getsize(pf) // 96)
            if os.path.getsize(pf):
                staged.append((pf, "craft_%s.m4.p%d.gz" % (name, p)))
        for run_name, args in cs["runs"].items():
            rows = check_rows(chk, m4, num_reads, args)
            cnt = census(rows, read_ranges(ranges[run_name]))
            for k in total:
                total[k] += cnt[k]
            leaf = "craft_%s.ranges%s.txt" % (name, "." + run_name if run_name else "")
            entry["runs"][run_name] = {"args": args, "ranges": leaf, "census": cnt, "host_cap": {k: cnt[k] for k in "abc"}}
            if os.path.getsize(ranges[run_name]) > 150_000:           # 100 000 reads without a record: only the other lines are stored
                entry["runs"][run_name]["sparse"] = {"sha256": sha(ranges[run_name]), "lines": num_reads + 1}
                sparse = ranges[run_name] + ".sparse"
                with open(sparse, "w") as f:
                    f.writelines(ln for ln in open(ranges[run_name]) if not ln.endswith("\t-1\t0\t0\n"))
                staged.append((sparse, leaf))
            else:
                staged.append((ranges[run_name], leaf))
            print("craft_%s %s: %s" % (name, run_name or "-", cnt))
        manifest["cases"][name] = entry
    main_cnt = manifest["cases"]["main"]["runs"][""]["census"]
    for k in ("complete", "chimeric", "cover"):
        assert main_cnt[k] >= 20, "craft_main: only %d reads decided as %s" % (main_cnt[k], k)
    for k in "abc":
        assert total[k] >= 5, "only %d reads of host reason (%s) over the crafted cases" % (total[k], k)
    assert main_cnt["b"] >= 5 and main_cnt["c"] >= 5 and manifest["cases"]["stale"]["runs"][""]["census"]["a"] >= 5
    assert main_cnt["invalid"] >= 10, "craft_main: only %d invalid reads" % main_cnt["invalid"]

    # ---- the natural set through the whole stage
    wrk = os.path.join(tmp, "nat")
    os.makedirs(wrk)
    reads = natural_reads(NAT["genome"], NAT["coverage"], NAT["seed"])
    fasta = os.path.join(wrk, "nat.reads.fasta")
    write_fasta(fasta, reads)
    open(os.path.join(wrk, "list.txt"), "w").write(fasta + "\n")
    vols = os.path.join(wrk, "vols")
    os.makedirs(vols)
    run([os.path.join(ref_bin, "oc2mkdb"), vols, os.path.join(wrk, "list.txt")])
    nv = len(open(os.path.join(vols, "volume_names.txt")).read().splitlines())
    m4 = os.path.join(wrk, "nat.m4")
    with open(m4, "wb") as f:
        for v in range(nv):
            o = os.path.join(wrk, "v%d.m4" % v)
            run([os.path.join(ref_bin, "oc2asmpm")] + NAT["asm_args"].split() + ["-t", "1", vols, str(v), o])
            f.write(open(o, "rb").read())
    num_reads = len(reads)
    ranges = run_reference_case(ref, vols, m4, num_reads, "0.1", {"": NAT["lcr_args"]})[""]
    comp, uncomp, tmp_pm = os.path.join(wrk, "complete.fasta"), os.path.join(wrk, "uncomplete.fasta"), os.path.join(wrk, "nat.tmp_pm.m4")
    run([ref["oc2etr"], ranges, fasta, m4, comp, uncomp, tmp_pm])
    both = os.path.join(wrk, "tmp_trimReads.fasta")
    open(both, "wb").write(open(comp, "rb").read() + open(uncomp, "rb").read())
    trimmed, pm = os.path.join(wrk, "trimReads.fasta"), os.path.join(wrk, "nat.pm.m4")
    run([ref["oc2orderResults"], both, tmp_pm, trimmed, pm])
    rows = check_rows(chk, m4, num_reads, NAT["lcr_args"])
    cnt = census(rows, read_ranges(ranges))
    n_host = cnt["a"] + cnt["b"] + cnt["c"]
    assert n_host * 10 <= num_reads, "natural set: %d of %d reads would go to the host - change the seed" % (n_host, num_reads)
    longest = max(np.bincount(np.fromfile(m4 + ".p0", dtype=M4_DTYPE)["sid"]))
    print("natural: %d reads, %d records, %s, longest list %d" % (num_reads, os.path.getsize(m4) // 96, cnt, longest))
    manifest["natural"] = {
        "num_reads": num_reads, "volumes": nv, "asm_args": NAT["asm_args"], "lcr_args": NAT["lcr_args"], "records": os.path.getsize(m4) // 96,
        "partition_records": [os.path.getsize(m4 + ".p0") // 96], "census": cnt, "host_cap": num_reads // 10, "longest_list": int(longest),
        "complete_fasta": {"sha256": sha(comp), "bytes": os.path.getsize(comp)}, "uncomplete_fasta": {"sha256": sha(uncomp), "bytes": os.path.getsize(uncomp)},
        "trimReads_fasta": {"sha256": sha(trimmed), "bytes": os.path.getsize(trimmed)},
    }
    staged += [(fasta, "nat.reads.fasta.gz"), (m4, "nat.m4.gz"), (m4 + ".p0", "nat.m4.p0.gz"), (ranges, "nat.ranges.txt"), (tmp_pm, "nat.tmp_pm.m4.gz"), (pm, "nat.pm.m4.gz")]

    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    size = 0
    for src, leaf in staged:
        dst = os.path.join(OUT, leaf)
        if leaf.endswith(".gz"):
            gz_to(src, dst)
        else:
            shutil.copy(src, dst)
        assert os.path.getsize(dst) <= 260_000, "%s: %d bytes" % (leaf, os.path.getsize(dst))
        size += os.path.getsize(dst)
    with open(os.path.join(GOLD, "manifest_trim.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d files, %d bytes" % (len(staged), size))
    assert size < 1_000_000, "the folder must stay below 1 MB"
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
