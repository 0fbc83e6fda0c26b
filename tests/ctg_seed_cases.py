"""Cases for the seeding of contig polishing (necat_ctg_seed_batch; necat_amd/csrc/ctg_seed.h, ctg_seed_core.h): the crafted generator, the case file the CPU
checker and the GPU tests read, and - where the reference's sources are present - the harness that runs the reference's own MaximalExactMatchWorkData_Init /
_FindCandidates (ctg_cns/mem_finder.c, chain_dp.c) on the same segments and reads.  tests/golden/make_golden_ctgseed.py writes the committed files with it.

A case set is a volume of contigs, a volume of reads, segments (a slice of a contig and a range of jobs), jobs (read id, strand) and, per job, what the reference
answered: found + the seven numbers of can_list[0], and the sorted matches (qoff, soff, size) it chained.

The case file (little endian):
  "CTGSEED1", u64 n_contigs, n_ctg_words, n_reads, n_read_words, n_segments, n_jobs, n_mems
  u64 ctg_off[n_contigs + 1], ctg_words[]; u64 read_off[n_reads + 1], read_words[]      (base g in bits 2 (g & 31) of word g >> 5; two spare words at the end)
  per segment: char name[32]; i64 ctg_id, from, size, job_begin, job_end
  per job: i32 qid, qdir, found, qbeg, qend, sbeg, send, qoff, soff, score, n_mems, 0        then every job's matches: i32 qoff, soff, size
An answers file ("CTGSANS1", u64 n_jobs, n_mems, then the two job-wise blocks) holds the last two alone: the natural case reuses the contig and the reads of
tests/golden/ctg_g/nat*.bin.gz."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"
HARNESS = os.path.join(ROOT, "tests", "golden", "ctg_seed_ref_harness.c")
JOB_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("found", "<i4"), ("qbeg", "<i4"), ("qend", "<i4"), ("sbeg", "<i4"), ("send", "<i4"), ("qoff", "<i4"), ("soff", "<i4"),
                      ("score", "<i4"), ("n_mems", "<i4"), ("_pad", "<i4")])
CAN_FIELDS = ("found", "qbeg", "qend", "sbeg", "send", "qoff", "soff", "score")


def have_reference():
    return os.path.exists(os.path.join(REF_SRC, "ctg_cns", "mem_finder.c"))


def revcomp(codes):
    return (3 - codes)[::-1].astype(np.uint8)


class Segment:
    def __init__(self, name, ctg_id, start, size):
        self.name, self.ctg_id, self.start, self.size = name, ctg_id, int(start), int(size)
        self.jobs = []                 # (qid, qdir)
        self.answers = []              # per job: (dict of CAN_FIELDS, mems array n x 3) - the reference's


class CaseSet:
    def __init__(self):
        self.contigs, self.reads, self.segments = [], [], []

    def add_read(self, strand_codes, qdir=0):
        """a read that reads `strand_codes` on strand qdir"""
        c = np.asarray(strand_codes, dtype=np.uint8)
        self.reads.append(revcomp(c) if qdir else c.copy())
        return len(self.reads) - 1

    def read_on_strand(self, qid, qdir):
        return revcomp(self.reads[qid]) if qdir else self.reads[qid]

    def segment_codes(self, s):
        return self.contigs[s.ctg_id][s.start:s.start + s.size]

    def n_jobs(self):
        return sum(len(s.jobs) for s in self.segments)

    def by_name(self):
        return {s.name: s for s in self.segments}


# ---------------------------------------------------------------------------------------------------------------- crafted cases

def _rand(rng, n):
    """random bases without a run of four A's: no poly-A 15-mer by accident"""
    c = rng.integers(0, 4, int(n), dtype=np.uint8)
    for i in range(3, c.shape[0]):
        if c[i] == 0 and c[i - 1] == 0 and c[i - 2] == 0 and c[i - 3] == 0:
            c[i] = 1 + int(rng.integers(0, 3))
    return c


def _other(b, rng):
    return np.uint8((int(b) + 1 + int(rng.integers(0, 3))) % 4)


def _plant(rng, read, q, seg, s, n):
    """read[q : q + n] = seg[s : s + n], the bases next to it on the read made to differ from the segment's"""
    read[q:q + n] = seg[s:s + n]
    if q > 0 and s > 0:
        read[q - 1] = _other(seg[s - 1], rng)
    if q + n < read.shape[0] and s + n < seg.shape[0]:
        read[q + n] = _other(seg[s + n], rng)


def _mutate(rng, codes, err):
    out = []
    for b in codes:
        u = rng.random()
        if u < err / 3:
            out.append(_other(b, rng))
        elif u < 2 * err / 3:
            out.append(b); out.append(np.uint8(rng.integers(0, 4)))
        elif u < err:
            continue
        else:
            out.append(b)
    return np.array(out, dtype=np.uint8)


def crafted(seed):
    """the crafted set: the smallest shapes at which each rule of ctg_seed.h can go wrong, with whatever the seed makes of the rest"""
    rng = np.random.default_rng(seed)
    cs = CaseSet()
    state = {"k": 0}

    def new(name, seg, pre=None, post=None):
        """a segment on a contig of its own, `pre` bases in front (the residue of `from` modulo 32 goes round) and `post` behind"""
        k = state["k"]; state["k"] += 1
        pre = (37 + 7 * k) % 64 if pre is None else pre
        post = (k % 3) * 11 if post is None else post
        ctg = np.concatenate([_rand(rng, pre), np.asarray(seg, dtype=np.uint8), _rand(rng, post)]).astype(np.uint8)
        cs.contigs.append(ctg)
        s = Segment(name, len(cs.contigs) - 1, pre, len(seg))
        cs.segments.append(s)
        return s, ctg[pre:pre + len(seg)]

    def job(s, strand_codes, both=False):
        qdir = int(rng.integers(0, 2))
        qid = cs.add_read(strand_codes, qdir)
        s.jobs.append((qid, qdir))
        if both:
            s.jobs.append((qid, 1 - qdir))

    # reads of 14, 15, 20 and 21 bases cut out of the segment
    s, seg = new("short_reads", _rand(rng, 300))
    for n in (14, 15, 20, 21):
        job(s, seg[50:50 + n])
    # a segment of exactly 15 bases: its only entry has hash 0
    s, seg = new("seg15", _rand(rng, 15))
    job(s, np.concatenate([_rand(rng, 40), seg, _rand(rng, 40)]))
    job(s, np.concatenate([seg, _rand(rng, 40)]))
    r = _rand(rng, 60); r[15:] = 0
    job(s, r)
    # the seed (0, 0) of the two hash-less entries survives as a match whose first 15 bases differ
    s, seg = new("off0_survives", _rand(rng, 400))
    r = _rand(rng, 120)
    _plant(rng, r, 15, seg, 15, 45)
    for i in range(15):
        r[i] = _other(seg[i], rng)
    job(s, r)
    # .. and swallows the true matches of diagonal 0 behind it: the read agrees from 6 on, differs before; seeds (6, 6), (12, 12) .. die, the survivor starts at 0
    s, seg = new("off0_swallows", _rand(rng, 400))
    r = _rand(rng, 150)
    _plant(rng, r, 6, seg, 6, 74)
    for i in range(6):
        r[i] = _other(seg[i], rng)
    job(s, r)
    # poly-A: 18 A's in the segment (4 true entries + the one at offset 0), 20 A's at a sampled offset of the read (1 + the one at offset 0): product 10;
    # and 40 A's in the segment (26 + 1 entries): no seed of that group
    for name, na in (("polya_10", 18), ("polya_27", 40)):
        g = _rand(rng, 600)
        g[200:200 + na] = 0; g[199] = 1; g[200 + na] = 2
        s, seg = new(name, g)
        r = _rand(rng, 300)
        r[60:80] = 0; r[59] = 3; r[80] = 1
        _plant(rng, r, 120, seg, 400, 90)
        job(s, r, both=True)
    # products of exactly 20 and 21: 20 bases `w` t times in the segment, at r sampled offsets of the read (the 15-mer w[0:15] is r x t) and at two offsets that are
    # 1 and 2 modulo 6, where w[5:20] and w[4:19] are sampled once each (1 x t, on top) and w[0:15] is not: they do not count towards r
    for name, nr, nt in (("occ_1x20", 1, 20), ("occ_4x5", 4, 5), ("occ_3x7", 3, 7), ("occ_1x21", 1, 21)):
        w = _rand(rng, 20)
        g = _rand(rng, 60 * nt + 100)
        for t in range(nt):
            g[40 + 60 * t:40 + 60 * t + 20] = w
            g[40 + 60 * t - 1], g[40 + 60 * t + 20] = 1, 2          # (the bases next to a copy: 1 and 2 in the segment, 3 and 3 in the read - no longer match by chance)
        s, seg = new(name, g)
        r = _rand(rng, 60 * nr + 200)
        for a in range(nr):
            r[30 + 60 * a:30 + 60 * a + 20] = w
            r[30 + 60 * a - 1], r[30 + 60 * a + 20] = 3, 3
        for q in (60 * nr + 61, 60 * nr + 122):
            r[q:q + 20] = w
            r[q - 1], r[q + 20] = 3, 3
        job(s, r)
    # matches that end at each of the four ends: the read's two (the read is a piece of the segment), and the SEGMENT's two, where contig and read go on agreeing
    ctg = _rand(rng, 30 + 900 + 30)
    cs.contigs.append(ctg)
    s = Segment("four_ends", len(cs.contigs) - 1, 30, 900)
    cs.segments.append(s); state["k"] += 1
    job(s, ctg[30 + 100:30 + 400])
    job(s, ctg[0:30 + 250])
    job(s, ctg[30 + 900 - 250:])
    # matches of 19 and 20 bases; two matches of one diagonal one mismatch apart; 200 exact bases whose ~ 33 seeds are one match and a chain of 200; 199
    s, seg = new("mem_19_20", _rand(rng, 500))
    r = _rand(rng, 200)
    _plant(rng, r, 60, seg, 100, 19)
    _plant(rng, r, 120, seg, 300, 20)
    job(s, r)
    s, seg = new("one_mismatch", _rand(rng, 500))
    r = seg[200:320].copy()
    r[60] = _other(r[60], rng)
    job(s, r)
    s, seg = new("exact_200_199", _rand(rng, 900))
    for n in (200, 199):
        r = _rand(rng, 240)
        _plant(rng, r, 20, seg, 300, n)
        job(s, r, both=(n == 200))
    # every residue modulo 32 of the segment's start and of the match's start on the read, on both strands
    ctg = _rand(rng, 3000)
    cs.contigs.append(ctg)
    for m in range(32):
        s = Segment("mod32_%d" % m, len(cs.contigs) - 1, 64 + m, 1500 + 3 * m)
        cs.segments.append(s)
        tail = (1 - 300 - 2 * m) % 32 or 32          # the read is 1 modulo 32 long: the reads' own starts in the volume go through every residue too
        r = np.concatenate([_rand(rng, m), ctg[600:900 + m], _rand(rng, tail)])
        r[m + 300 + m] = _other(ctg[900 + m], rng)
        if m:
            r[m - 1] = _other(ctg[599], rng)
        job(s, r, both=True)
    state["k"] += 1
    # chain gaps of 3000 / 3001 on each axis: two matches of 120, chained (227 >= 200) or not (none)
    for name, dq, dr in (("gap_q3000", 3000, 2990), ("gap_q3001", 3001, 2991), ("gap_s3000", 2990, 3000), ("gap_s3001", 2991, 3001)):
        s, seg = new(name, _rand(rng, 4000))
        r = _rand(rng, 10 + dq + 120 + 10)
        _plant(rng, r, 10, seg, 500, 120)
        _plant(rng, r, 10 + dq, seg, 500 + dr, 120)
        job(s, r)
    # a diagonal drift of 1500 / 1501: 60 matches of 39 on one diagonal (f = 2340 at the last), then one of 2000 whose start is 1500 (1499) further on the read and 3000
    # on the segment: inside the band it joins the chain, outside it is a chain of its own
    for name, dq in (("drift_1500", 1500), ("drift_1501", 1499)):
        s, seg = new(name, _rand(rng, 9000))
        qj, sj = 12 + 59 * 40, 500 + 59 * 40
        r = _rand(rng, qj + dq + 2000 + 20)
        r[12:12 + 2400] = seg[500:2900]
        for b in range(60):
            r[12 + 40 * b + 39] = _other(seg[500 + 40 * b + 39], rng)
        r[11] = _other(seg[499], rng)
        _plant(rng, r, qj + dq, seg, sj + 3000, 2000)
        job(s, r)
    # a peak that is not the chain's end: ten matches of 39 (f = 390), then one of 25 off the diagonal that scores less than its predecessor but more than alone
    s, seg = new("peak_not_end", _rand(rng, 2000))
    r = _rand(rng, 900)
    r[12:12 + 400] = seg[500:900]
    for b in range(10):
        r[12 + 40 * b + 39] = _other(seg[500 + 40 * b + 39], rng)
    r[11] = _other(seg[499], rng)
    _plant(rng, r, 12 + 360 + 200, seg, 500 + 360 + 300, 25)
    job(s, r)
    # two chains with equal peak score (two matches of 250 more than 3000 apart): the later one is can_list[0]
    s, seg = new("equal_peaks", _rand(rng, 5000))
    r = _rand(rng, 4400)
    _plant(rng, r, 30, seg, 400, 250)
    _plant(rng, r, 30 + 3600, seg, 400 + 3600, 250)
    job(s, r)
    # two longest matches of equal size in one chain: the anchor is the middle of the first
    s, seg = new("equal_longest", _rand(rng, 2000))
    r = _rand(rng, 700)
    _plant(rng, r, 30, seg, 400, 150)
    _plant(rng, r, 330, seg, 702, 150)
    job(s, r)
    # tandem repeats: 20 units of 47 in the segment, 18 (one mismatch each) in the read: every pair of units is a match, a predecessor window holds well over
    # 128 of them and the 25-skip break falls inside, at and across the 64-entry steps of the device's scan (the checker counts where)
    trng = np.random.default_rng([seed, 47])          # (its own stream: the cases above do not move it)
    unit = _rand(trng, 47)
    g = np.concatenate([_rand(trng, 300)] + [unit] * 20 + [_rand(trng, 300)])
    s, seg = new("tandem", g)
    for k in range(4):
        ru = []
        for a in range(18 - 2 * k):
            u = unit.copy()
            x = int(trng.integers(5, 42))
            u[x] = _other(u[x], trng)
            ru.append(u)
        job(s, np.concatenate([_rand(trng, 50 + k)] + ru + [_rand(trng, 50)]), both=(k == 0))
    # whatever the seed gives: reads of a 6 kb segment at 1 to 15 % error, both strands
    s, seg = new("noisy", _rand(rng, 6000))
    for err in (0.01, 0.07, 0.12, 0.15):
        a = int(rng.integers(0, 2000))
        job(s, np.concatenate([_rand(rng, 30), _mutate(rng, seg[a:a + 3500], err), _rand(rng, 30)]), both=True)
    # the hash-less entry at offset 0 is a MEMBER of the other list's poly-A group and COUNTS towards its occ.  33 A's in the segment are 19 true entries, 20 with the
    # one at offset 0: the read's offset-0 entry (1 x 20) gives the unverified seed (0, 218), which survives as a match of 40 whose first 15 bases differ and
    # swallows the true seeds behind it.  34 A's are 20 + 1: 1 x 21, no such seed, and the true match (15, 233, 25) stands.
    prng = np.random.default_rng([seed, 48])
    for name, na in (("polya_q0_20", 33), ("polya_q0_21", 34)):
        g = _rand(prng, 500)
        g[200:200 + na] = 0; g[199] = 1; g[200 + na] = 2
        s, seg = new(name, g)
        s0 = 200 + na - 15                                     # the run's last true entry
        r = _rand(prng, 90)
        r[:15] = 1 + prng.integers(0, 3, 15)                   # no A: differs from the fifteen A's everywhere
        r[15:40] = seg[s0 + 15:s0 + 40]
        r[40] = _other(seg[s0 + 40], prng)
        job(s, r)
    # .. the mirror: the SEGMENT's offset-0 entry against sampled poly-A 15-mers of the read.  123 A's from a sampled offset are 19 samples, 20 with the read's own
    # offset-0 entry (20 x 1): the seed (q0, 0) survives as a match of 40 over the segment's first 15 bases, which are no A's; 129 A's are 20 + 1: nothing but
    # the true match (q0 + 15, 15, 25)
    for name, na in (("polya_s0_20", 123), ("polya_s0_21", 129)):
        g = _rand(prng, 400)
        g[:15] = 1 + prng.integers(0, 3, 15)
        g[15] = 1 + int(prng.integers(0, 3))
        s, seg = new(name, g)
        q0 = 60 + ((na - 15) // 6) * 6                         # the run's last sampled entry
        r = _rand(prng, 60 + na + 60)
        r[60:60 + na] = 0; r[59] = 2
        r[q0 + 15:q0 + 40] = seg[15:40]
        r[q0 + 40] = _other(seg[40], prng)
        job(s, r)
    return cs


def natural():
    """the committed contig and reads of the consensus half's natural case: every read a job on both strands of the whole contig (answers: not yet)"""
    from tests import ctg_cases as cc
    gold = os.path.join(ROOT, "tests", "golden", "ctg_g")
    src = cc.read_cases(os.path.join(gold, "nat.bin.gz"), os.path.join(gold, "nat.reads.bin.gz"))
    cs = CaseSet()
    cs.contigs = [np.array(src.cases[0].contig, dtype=np.uint8)]
    cs.reads = [np.array(r, dtype=np.uint8) for r in src.reads]
    size = cs.contigs[0].shape[0]
    whole = Segment("nat_whole", 0, 0, size)
    part = Segment("nat_part", 0, 10007, size - 10007)          # a start that is no multiple of 32, to the contig's end
    for q in range(len(cs.reads)):
        whole.jobs += [(q, 0), (q, 1)]
        if q % 4 == 0:
            part.jobs += [(q, 0), (q, 1)]
    cs.segments = [whole, part]
    return cs


# ---------------------------------------------------------------------------------------------------------------- the reference harness

def build_harness(outdir):
    """the reference's two functions behind our small C main (tests/golden/ctg_seed_ref_harness.c), compiled into outdir - outside the repository"""
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "ctg_seed_ref_harness")
    src = [os.path.join(REF_SRC, "ctg_cns", n) for n in ("mem_finder.c", "chain_dp.c")]
    src += [os.path.join(REF_SRC, "common", n) for n in ("oc_assert.c", "ontcns_aux.c", "ontcns_defs.c", "gapped_candidate.c")] + [os.path.join(REF_SRC, "klib", "kstring.c")]
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-ffp-contract=off", "-pthread", "-I", REF_SRC, "-o", exe, HARNESS] + src + ["-lm", "-lz"], check=True)
    return exe


def run_harness(exe, cs, tmp):
    """the reference's matches and candidate into every job of cs"""
    inp = os.path.join(tmp, "seed_harness_in.bin")
    with open(inp, "wb") as f:
        for s in cs.segments:
            f.write(b"S" + np.int32(s.size).tobytes() + cs.segment_codes(s).tobytes())
            for qid, qdir in s.jobs:
                r = cs.read_on_strand(qid, qdir)
                f.write(b"R" + np.int32(r.shape[0]).tobytes() + r.tobytes())
    out = subprocess.run([exe, inp], check=True, stdout=subprocess.PIPE).stdout.split(b"\n")
    at = 0
    for s in cs.segments:
        s.answers = []
        for _ in s.jobs:
            head = out[at].split(); at += 1
            assert head[0] == b"J", head
            v = [int(x) for x in head[1:]]
            mems = np.array(out[at].split(), dtype=np.int32).reshape(-1, 3); at += 1
            assert mems.shape[0] == v[0]
            s.answers.append((dict(zip(CAN_FIELDS, v[1:])), mems))
    assert not any(out[at:]), "the harness printed more than the jobs asked for"


# ---------------------------------------------------------------------------------------------------------------- the case file

def pack_words(codes):
    n = codes.shape[0]
    c = np.zeros(((n + 31) // 32) * 32 + 64, dtype=np.uint64)
    c[:n] = codes
    return (c.reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=1, dtype=np.uint64)


def _volume(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([x.shape[0] for x in seqs])
    return off, pack_words(np.concatenate(seqs) if seqs else np.zeros(0, np.uint8))


def _answer_blocks(cs):
    jobs = np.zeros(cs.n_jobs(), dtype=JOB_DTYPE)
    mems, k = [], 0
    for s in cs.segments:
        for (qid, qdir), (can, m) in zip(s.jobs, s.answers):
            jobs[k] = (qid, qdir) + tuple(can[f] for f in CAN_FIELDS) + (m.shape[0], 0)
            mems.append(m); k += 1
    return jobs, (np.concatenate(mems) if mems else np.zeros((0, 3))).astype("<i4")


def write_cases(cs, path):
    coff, cw = _volume(cs.contigs)
    roff, rw = _volume(cs.reads)
    jobs, mems = _answer_blocks(cs)
    with open(path, "wb") as f:
        f.write(b"CTGSEED1" + np.array([len(cs.contigs), cw.shape[0], len(cs.reads), rw.shape[0], len(cs.segments), jobs.shape[0], mems.shape[0]], dtype="<u8").tobytes())
        f.write(coff.tobytes() + cw.tobytes() + roff.tobytes() + rw.tobytes())
        k = 0
        for s in cs.segments:
            f.write(s.name.encode()[:31].ljust(32, b"\0") + np.array([s.ctg_id, s.start, s.size, k, k + len(s.jobs)], dtype="<i8").tobytes())
            k += len(s.jobs)
        f.write(jobs.tobytes() + mems.tobytes())


def write_answers(cs, path):
    jobs, mems = _answer_blocks(cs)
    with open(path, "wb") as f:
        f.write(b"CTGSANS1" + np.array([jobs.shape[0], mems.shape[0]], dtype="<u8").tobytes() + jobs.tobytes() + mems.tobytes())


def _open(path):
    import gzip
    return (gzip.open if path.endswith(".gz") else open)(path, "rb").read()


def _set_answers(cs, jobs, mems):
    k, at = 0, 0
    for s in cs.segments:
        s.answers = []
        for qid, qdir in s.jobs:
            j = jobs[k]; k += 1
            assert (int(j["qid"]), int(j["qdir"])) == (qid, qdir)
            n = int(j["n_mems"])
            s.answers.append(({f: int(j[f]) for f in CAN_FIELDS}, mems[at:at + n])); at += n
    assert k == jobs.shape[0] and at == mems.shape[0]


def read_answers(cs, path):
    raw = _open(path)
    assert raw[:8] == b"CTGSANS1"
    nj, nm = (int(x) for x in np.frombuffer(raw, "<u8", 2, 8))
    jobs = np.frombuffer(raw, JOB_DTYPE, nj, 24)
    _set_answers(cs, jobs, np.frombuffer(raw, "<i4", 3 * nm, 24 + 48 * nj).reshape(-1, 3))
    return cs


def read_cases(path):
    raw = _open(path)
    assert raw[:8] == b"CTGSEED1"
    nc, ncw, nr, nrw, ns, nj, nm = (int(x) for x in np.frombuffer(raw, "<u8", 7, 8))
    at = 64

    def volume(n, nw, at):
        off = np.frombuffer(raw, "<u8", n + 1, at); at += 8 * (n + 1)
        words = np.frombuffer(raw, "<u8", nw, at); at += 8 * nw
        codes = ((words[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)).astype(np.uint8).reshape(-1)
        return [codes[int(off[i]):int(off[i + 1])] for i in range(n)], at
    cs = CaseSet()
    cs.contigs, at = volume(nc, ncw, at)
    cs.reads, at = volume(nr, nrw, at)
    segs = []
    for _ in range(ns):
        name = raw[at:at + 32].rstrip(b"\0").decode(); at += 32
        cid, start, size, jb, je = (int(x) for x in np.frombuffer(raw, "<i8", 5, at)); at += 40
        segs.append((Segment(name, cid, start, size), jb, je))
    jobs = np.frombuffer(raw, JOB_DTYPE, nj, at); at += 48 * nj
    mems = np.frombuffer(raw, "<i4", 3 * nm, at).reshape(-1, 3); at += 12 * nm
    assert at == len(raw), (at, len(raw))
    for s, jb, je in segs:
        s.jobs = [(int(jobs[k]["qid"]), int(jobs[k]["qdir"])) for k in range(jb, je)]
        cs.segments.append(s)
    _set_answers(cs, jobs, mems)
    return cs


def volume_arrays(seqs):
    """(pac, nbases, offsets, sizes) for capi.Context.upload_volume"""
    from necat_amd import synth
    codes = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
    sizes = np.array([r.shape[0] for r in seqs], dtype=np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    return synth.pack_2bit(codes), int(codes.shape[0]), off, sizes
