"""Cases for the consensus half of contig polishing (necat_ctg_consensus_batch; necat_amd/csrc/ctg_consensus.h, ctg_dev_core.h): the crafted generator, the case
file the CPU checker and the GPU tests read, and - where the reference's sources are present - the harness that runs the reference's own add_align_tags and
get_cns_from_align_tags (ctg_cns/fc_correct_one_read.c) on the same gapped strings.  tests/golden/make_golden_ctgcns.py writes the committed files with it.

A case is one contig segment: its raw bases (codes 0..3), its overlaps (read id, strand, the ranges on read and segment, one op per column: 0 match, 1 query base
over '-', 2 '-' over target base, 3 mismatch) and what the reference answered: cns (characters with case), t_pos and, for a case that went through the reference's
ctgcns program, the polished segment.  All cases of a file share one read set.

The case file (little endian, every block padded to 8 bytes):
  "CTGCASE1", u64 n_cases, u64 n_reads, u64 n_words; u64 seq_off[n_reads + 1]; u64 words[n_words] (base g in bits 2 (g & 31) of word g >> 5)
  (a file may hold reads alone, n_cases = 0, or cases alone, n_reads = 0: a large case is stored as such a pair)
  per case: char name[32]; u64 size, n_ov, ops_bytes, cns_len, has_polished, polished_len; n_ov x (i32 qid, qdir, qoff, qend, toff, tend, align_size, 0; u64 ops_off);
            ops (two bits per column, low bits first, every overlap 8-byte aligned); u8 contig[size]; cns[cns_len]; i32 t_pos[cns_len]; polished[polished_len]
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"
HARNESS = os.path.join(ROOT, "tests", "golden", "ctg_ref_harness.c")
OVL_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"), ("align_size", "<i4"), ("_pad", "<i4"), ("ops_off", "<u8")])
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def have_reference():
    return os.path.exists(os.path.join(REF_SRC, "ctg_cns", "fc_correct_one_read.c"))


class Case:
    def __init__(self, name, contig):
        self.name, self.contig = name, np.asarray(contig, dtype=np.uint8)
        self.ovl = []              # (qid, qdir, qoff, qend, toff, tend, ops)
        self.cns, self.t_pos, self.polished = None, None, None

    @property
    def size(self):
        return int(self.contig.shape[0])


class CaseSet:
    def __init__(self):
        self.reads, self.cases = [], []

    def add_read(self, codes):
        self.reads.append(np.asarray(codes, dtype=np.uint8))
        return len(self.reads) - 1

    def read_on_strand(self, qid, qdir):
        r = self.reads[qid]
        return (3 - r)[::-1] if qdir else r


# ---------------------------------------------------------------------------------------------------------------- crafted cases

def _columns(rng, truth, contig, toff, tend, err, force=None):
    """ops and query bases of one overlap on contig[toff, tend): the read says `truth` there, plus its own errors at rate `err` (thirds: mismatch, query base
    over '-', '-' over target base).  force: {position: list of (op, base)} replaces the columns of that position."""
    ops, q = [], []
    for p in range(toff, tend):
        if force and p in force:
            for op, b in force[p]:
                ops.append(op)
                if op != 2:
                    q.append(b)
            continue
        u = rng.random()
        if u < err / 3:
            b = int((truth[p] + 1 + rng.integers(0, 3)) % 4)
            ops.append(0 if b == contig[p] else 3)
            q.append(b)
        elif u < 2 * err / 3:
            ops.append(0 if truth[p] == contig[p] else 3)
            q.append(int(truth[p]))
            for _ in range(int(rng.integers(1, 4))):
                ops.append(1)
                q.append(int(rng.integers(0, 4)))
        elif u < err:
            ops.append(2)
        else:
            ops.append(0 if truth[p] == contig[p] else 3)
            q.append(int(truth[p]))
    return np.array(ops, dtype=np.uint8), np.array(q, dtype=np.uint8)


def _add_overlap(cs, case, rng, ops, q, toff):
    """a read around the query bases `q` (random bases at both ends), stored on a random strand"""
    qdir = int(rng.integers(0, 2))
    lo, hi = int(rng.integers(0, 40)), int(rng.integers(0, 40))
    strand = np.concatenate([rng.integers(0, 4, lo, dtype=np.uint8), q, rng.integers(0, 4, hi, dtype=np.uint8)]).astype(np.uint8)
    qid = cs.add_read((3 - strand)[::-1] if qdir else strand)
    nt = int(np.count_nonzero(ops != 1))
    case.ovl.append((qid, qdir, lo, lo + int(q.shape[0]), toff, toff + nt, ops))


def _contig(rng, size, sub=0.01):
    truth = rng.integers(0, 4, size, dtype=np.uint8)
    contig = truth.copy()
    flip = rng.random(size) < sub
    contig[flip] = (contig[flip] + 1 + rng.integers(0, 3, int(flip.sum()))) % 4
    return truth, contig


def _cover(cs, case, rng, truth, ranges, err, force_for=None):
    for k, (a, b) in enumerate(ranges):
        ops, q = _columns(rng, truth, case.contig, a, b, err, (force_for or {}).get(k))
        _add_overlap(cs, case, rng, ops, q, a)


def crafted(seed):
    """the crafted set: every case the rule treats specially, with whatever the seed makes of the rest"""
    rng = np.random.default_rng(seed)
    cs = CaseSet()

    def new(name, size, sub=0.01):
        truth, contig = _contig(rng, size, sub)
        c = Case(name, contig)
        cs.cases.append(c)
        return c, truth

    # insertion runs of 70 and 300 columns, each in two of six overlaps (the same bases: the run is a path of its own), overlaps from 0 and to `size`
    c, truth = new("ins_runs", 2500)
    run70, run300 = rng.integers(0, 4, 70), rng.integers(0, 4, 300)
    f = lambda p, run: {p: [(0 if truth[p] == c.contig[p] else 3, int(truth[p]))] + [(1, int(b)) for b in run]}
    _cover(cs, c, rng, truth, [(0, 2500), (0, 2000), (300, 2500), (0, 2500), (100, 2400), (0, 2500)], 0.06,
           {0: {**f(700, run70), **f(1500, run300)}, 3: {**f(700, run70), **f(1500, run300)}})
    # one run of 40 000 query bases: a bucket of tens of thousands of tags (the reference's allocator asserts from some 47 000 on: stop_rule_case below)
    c, truth = new("ins_40000", 400)
    _long_run(cs, c, rng, truth, 40000)
    # a deletion as an overlap's first and last column; a query base as first column behind position 0
    c, truth = new("del_ends", 600)
    _cover(cs, c, rng, truth, [(0, 600), (0, 600), (0, 600), (0, 600), (50, 550), (60, 600), (0, 540)], 0.05,
           {0: {0: [(2, 0)], 599: [(2, 0)]}, 4: {50: [(2, 0)], 549: [(2, 0)]}, 5: {60: [(1, 2), (1, 3), (0 if truth[60] == c.contig[60] else 3, int(truth[60]))]}})
    # a stretch nobody covers, a stretch three deep (lower case) on the best path (the island at 0 scores less), overlaps from 0 and to `size`
    c, truth = new("nocov_cov3", 3000)
    _cover(cs, c, rng, truth, [(0, 800)] * 5 + [(1800, 3000)] * 3 + [(2300, 3000)] * 2, 0.04)
    # upper-case runs of exactly 999 and 1000 between stretches three deep (error-free reads: one consensus base per position)
    c, truth = new("runs_999_1000", 3300, 0.02)
    _cover(cs, c, rng, truth, [(0, 3300)] * 3 + [(500, 1499)] * 2 + [(2000, 3000)] * 2, 0.0)
    # two links of equal score at one node: two overlaps that differ in the base before it
    c, truth = new("tie_links", 200)
    a, b = int((truth[100] + 1) % 4), int((truth[100] + 2) % 4)
    _cover(cs, c, rng, truth, [(10, 190), (10, 190)], 0.0, {0: {100: [(0 if a == c.contig[100] else 3, a)]}, 1: {100: [(0 if b == c.contig[100] else 3, b)]}})
    # two nodes of equal global-best score: two overlaps that differ in their last base
    c, truth = new("tie_best", 200)
    a, b = int((truth[179] + 3) % 4), int((truth[179] + 1) % 4)
    _cover(cs, c, rng, truth, [(5, 180), (5, 180)], 0.0, {0: {179: [(0 if a == c.contig[179] else 3, a)]}, 1: {179: [(0 if b == c.contig[179] else 3, b)]}})
    # whatever the seed gives: error-rich overlaps of random ranges
    c, truth = new("random", 1800)
    rg = []
    for _ in range(14):
        x = int(rng.integers(0, 1500))
        rg.append((x, min(1800, x + int(rng.integers(200, 1800)))))
    _cover(cs, c, rng, truth, rg, 0.15)
    return cs


def _long_run(cs, c, rng, truth, n):
    run = rng.integers(0, 4, n)
    _cover(cs, c, rng, truth, [(0, 400), (0, 400), (20, 380), (0, 400), (0, 400)], 0.05, {1: {150: [(0 if truth[150] == c.contig[150] else 3, int(truth[150]))] + [(1, int(b)) for b in run]}})


def stop_rule_case(seed):
    """One run of 65 540 query bases: the scan of that overlap stops for good at the column whose delta reaches 65 535.  The reference cannot answer this one -
    its block allocator holds at most 8 MB per position (ctg_cns/small_object_alloc.c:5,98) and asserts - so the case has no expected output: the paths are
    compared with each other."""
    rng = np.random.default_rng(seed)
    cs = CaseSet()
    truth, contig = _contig(rng, 400)
    c = Case("ins_65540", contig)
    cs.cases.append(c)
    _long_run(cs, c, rng, truth, 65540)
    c.cns, c.t_pos = b"", np.zeros(0, np.int32)
    return cs


# ---------------------------------------------------------------------------------------------------------------- gapped strings, the reference harness

def gapped(cs, case, k):
    qid, qdir, qoff, qend, toff, tend, ops = case.ovl[k]
    r = cs.read_on_strand(qid, qdir)
    qa = np.full(ops.shape[0], ord("-"), dtype=np.uint8)
    ta = np.full(ops.shape[0], ord("-"), dtype=np.uint8)
    qa[ops != 2] = LUT[r[qoff:qend]]
    ta[ops != 1] = LUT[case.contig[toff:tend]]
    return qa.tobytes(), ta.tobytes()


def build_harness(outdir, shim=False):
    """the reference's two functions behind our small C main (tests/golden/ctg_ref_harness.c), compiled into outdir - outside the repository"""
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "ctg_ref_harness")
    src = [os.path.join(REF_SRC, "ctg_cns", n) for n in ("fc_correct_one_read.c", "small_object_alloc.c", "kalloc.c")]
    src += [os.path.join(REF_SRC, "klib", "kstring.c"), os.path.join(REF_SRC, "common", "oc_assert.c"), os.path.join(REF_SRC, "common", "ontcns_aux.c")]
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-ffp-contract=off", "-pthread", "-I", REF_SRC, "-o", exe, HARNESS] + src + ["-lm", "-lz"], check=True)
    return exe


def write_harness_input(cs, path, min_cov=4):
    with open(path, "wb") as f:
        for c in cs.cases:
            for k, (qid, qdir, qoff, qend, toff, tend, ops) in enumerate(c.ovl):
                qa, ta = gapped(cs, c, k)
                f.write(b"O %d %d %d %d %d %d %d\n" % (qid, qdir, qoff, qend, toff, tend, ops.shape[0]))
                f.write(qa + b"\n" + ta + b"\n")
            f.write(b"S %d %d\n" % (c.size, min_cov))


def parse_answers(text):
    """[(cns bytes, t_pos array)] from the harness's `C` / `T` lines"""
    out, cns = [], None
    for ln in text.split(b"\n"):
        if ln.startswith(b"C "):
            cns = ln[2:].strip()
        elif ln.startswith(b"T "):
            out.append((cns, np.array(ln[2:].split(), dtype=np.int32)))
    return out


def run_harness(exe, cs, tmp):
    """the reference's cns / t_pos into every case of cs"""
    inp = os.path.join(tmp, "harness_in.txt")
    write_harness_input(cs, inp)
    r = subprocess.run([exe, inp], check=True, stdout=subprocess.PIPE)
    ans = parse_answers(r.stdout)
    assert len(ans) == len(cs.cases), (len(ans), len(cs.cases))
    for c, (cns, tp) in zip(cs.cases, ans):
        assert len(cns) == tp.shape[0]
        c.cns, c.t_pos = cns, tp


# ---------------------------------------------------------------------------------------------------------------- the case file

def _pad8(b):
    return b + b"\0" * ((-len(b)) % 8)


def pack_words(codes):
    n = codes.shape[0]
    c = np.zeros(((n + 31) // 32) * 32 + 32, dtype=np.uint64)
    c[:n] = codes
    return (c.reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=1, dtype=np.uint64)


def pack_ops(ops):
    n = ops.shape[0]
    p = np.zeros(((n + 3) // 4) * 4, dtype=np.uint8)
    p[:n] = ops
    q = p.reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8).tobytes()


def case_arrays(case):
    """(overlap table, ops blob) of one case as the entry point takes them"""
    tab = np.zeros(len(case.ovl), dtype=OVL_DTYPE)
    blob = b""
    for k, (qid, qdir, qoff, qend, toff, tend, ops) in enumerate(case.ovl):
        tab[k] = (qid, qdir, qoff, qend, toff, tend, ops.shape[0], 0, len(blob))
        blob += _pad8(pack_ops(ops))
    return tab, np.frombuffer(blob + b"\0" * 8, dtype=np.uint8)


def write_cases(cs, path, reads=True, cases=True):
    """reads = False: the cases alone (their reads are in another file, written with cases = False)"""
    rd = cs.reads if reads else []
    sizes = np.array([r.shape[0] for r in rd], dtype=np.uint64)
    off = np.zeros(len(rd) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)
    words = pack_words(np.concatenate(rd)) if rd else np.zeros(0, np.uint64)
    with open(path, "wb") as f:
        f.write(b"CTGCASE1" + np.array([len(cs.cases) if cases else 0, len(rd), words.shape[0]], dtype="<u8").tobytes() + off.tobytes() + words.tobytes())
        for c in cs.cases if cases else []:
            tab, blob = case_arrays(c)
            blob = blob[:-8].tobytes()
            pol = c.polished if c.polished is not None else b""
            f.write(c.name.encode()[:31].ljust(32, b"\0"))
            f.write(np.array([c.size, len(c.ovl), len(blob), len(c.cns), 0 if c.polished is None else 1, len(pol)], dtype="<u8").tobytes())
            f.write(tab.tobytes() + blob + _pad8(c.contig.tobytes()) + _pad8(c.cns) + _pad8(np.asarray(c.t_pos, dtype="<i4").tobytes()) + _pad8(pol))


def read_cases(path, reads_path=None):
    """reads_path: the file that holds the reads of a file of cases alone"""
    import gzip
    raw = (gzip.open if path.endswith(".gz") else open)(path, "rb").read()
    assert raw[:8] == b"CTGCASE1"
    nc, nr, nw = (int(x) for x in np.frombuffer(raw, "<u8", 3, 8))
    at = 32
    off = np.frombuffer(raw, "<u8", nr + 1, at); at += 8 * (nr + 1)
    words = np.frombuffer(raw, "<u8", nw, at); at += 8 * nw
    codes = ((words[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)).astype(np.uint8).reshape(-1)
    cs = CaseSet()
    cs.reads = [codes[int(off[i]):int(off[i + 1])] for i in range(nr)] if reads_path is None else read_cases(reads_path).reads
    p8 = lambda n: (n + 7) & ~7
    for _ in range(nc):
        name = raw[at:at + 32].rstrip(b"\0").decode(); at += 32
        size, n_ov, ob, cl, hp, pl = (int(x) for x in np.frombuffer(raw, "<u8", 6, at)); at += 48
        tab = np.frombuffer(raw, OVL_DTYPE, n_ov, at); at += 40 * n_ov
        blob = np.frombuffer(raw, np.uint8, ob, at); at += ob
        c = Case(name, np.frombuffer(raw, np.uint8, size, at)); at += p8(size)
        c.cns = raw[at:at + cl]; at += p8(cl)
        c.t_pos = np.frombuffer(raw, "<i4", cl, at); at += p8(4 * cl)
        c.polished = raw[at:at + pl] if hp else None; at += p8(pl)
        for o in tab:
            n = int(o["align_size"])
            b = blob[int(o["ops_off"]):int(o["ops_off"]) + (n + 3) // 4]
            ops = np.stack([b & 3, (b >> 2) & 3, (b >> 4) & 3, (b >> 6) & 3], axis=1).reshape(-1)[:n].astype(np.uint8)
            c.ovl.append((int(o["qid"]), int(o["qdir"]), int(o["qoff"]), int(o["qend"]), int(o["toff"]), int(o["tend"]), ops))
        cs.cases.append(c)
    assert at == len(raw), (at, len(raw))
    return cs


def volume_arrays(cs):
    """(pac, nbases, offsets, sizes) for capi.Context.upload_volume"""
    from necat_amd import synth
    codes = np.concatenate(cs.reads) if cs.reads else np.zeros(0, np.uint8)
    sizes = np.array([r.shape[0] for r in cs.reads], dtype=np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    return synth.pack_2bit(codes), int(codes.shape[0]), off, sizes
