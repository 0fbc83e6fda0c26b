"""Cases for the aligner and the coverage cap of contig polishing (necat_ctg_extend_batch; necat_amd/csrc/ctg_extend.h, stage_ctg_extend.inl): the crafted generator,
the case files the CPU checker and the GPU tests read, and - where the reference's sources are present - the harness that runs the reference's own cns_ctg_subseq and
cns_extension (ctg_cns/cns_ctg_subseq.c) on the same reads, segments and records with every aligner call logged (tests/golden/ctg_ext_ref_harness.c).
tests/golden/make_golden_ctgext.py writes the committed files with it.

A case set is a volume of contigs, a volume of reads, segments (a slice of a contig and a range of records) and records in loop order (read id, strand, soff, send
on the contig).  Per record the reference's log, as ANS_DTYPE:
  passed / order    the loop (cns_ctg_subseq): the record got past the cap (pdb_extract_sequence was called), and the rank of its add_align_tags call (-1: none)
  found             MaximalExactMatchWorkData_FindCandidates' return value
  onc_*             onc_align's return value and what it left; dal_* / edl_*: ocda_go's and edlib_go's (run = -1: not called)
  ok, qoff .. ident, align_size, ops_off      what cns_extension returned when called on the record alone (no cap), its columns two bits each at ops + ops_off
The generator asserts that the loop's log of a record equals the record-alone log, so one copy is kept.

The case file (little endian): "CTGEXT01", u64 n_contigs, n_ctg_words, n_reads, n_read_words, n_segments, n_records, n_ops_bytes;
  u64 ctg_off[n_contigs + 1], ctg_words[]; u64 read_off[n_reads + 1], read_words[]; per segment: char name[32]; i64 ctg_id, from, size, rec_begin, rec_end;
  ANS_DTYPE records[n_records]; u8 ops[n_ops_bytes]
The natural case's file holds no contig and only the reads tests/golden/ctg_g/nat.reads.bin.gz lacks (they follow its reads)."""
import gzip
import os
import subprocess

import numpy as np

from tests import ctg_seed_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"
HARNESS = os.path.join(ROOT, "tests", "golden", "ctg_ext_ref_harness.c")
GOLD = os.path.join(ROOT, "tests", "golden", "ctg_x")
WRAPS = "-Wl,--wrap=cns_ctg_subseq,--wrap=pdb_extract_sequence,--wrap=MaximalExactMatchWorkData_FindCandidates,--wrap=onc_align,--wrap=ocda_go,--wrap=edlib_go,--wrap=add_align_tags"
ANS_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("soff", "<i8"), ("send", "<i8"), ("passed", "<i4"), ("order", "<i4"), ("found", "<i4"),
                      ("onc_ret", "<i4"), ("onc_qoff", "<i4"), ("onc_qend", "<i4"), ("onc_toff", "<i4"), ("onc_tend", "<i4"), ("onc_ident", "<f8"),
                      ("dal_run", "<i4"), ("dal_qoff", "<i4"), ("dal_qend", "<i4"), ("dal_toff", "<i4"), ("dal_tend", "<i4"), ("dal_diffs", "<i4"),
                      ("edl_run", "<i4"), ("edl_qoff", "<i4"), ("edl_qend", "<i4"), ("edl_toff", "<i4"), ("edl_tend", "<i4"), ("_pad", "<i4"), ("edl_ident", "<f8"),
                      ("ok", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"), ("align_size", "<i4"), ("ident", "<f8"), ("ops_off", "<u8")])
assert ANS_DTYPE.itemsize == 160
CAPPED, NO_SEED, NO_ALIGNMENT, REJECTED, ACCEPTED = range(5)          # necat_ctg_extend_result.state
BY_NONE, BY_BLOCKS, BY_PAIR, BY_BLOCKS_KEPT = range(4)                 # .. decided
CRAFT_SEED = 20262
OWN_STREAM = {"insertion": 1, "deletion": 2, "over_start_mid": 1, "over_end_mid": 2, "over_start_end": 1}          # crafted(): streams of single cases
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def have_reference():
    return os.path.exists(os.path.join(REF_SRC, "ctg_cns", "cns_ctg_subseq.c"))


class Segment:
    def __init__(self, name, ctg_id, start, size):
        self.name, self.ctg_id, self.start, self.size = name, ctg_id, int(start), int(size)
        self.records = []              # (qid, qdir, soff, send) in loop order
        self.tags = {}                 # record index -> what it is there for (crafted set)
        self.ans = None                # ANS_DTYPE array, one per record
        self.ops = None                # per record its columns (one code each) or None


class CaseSet(sc.CaseSet):
    def n_records(self):
        return sum(len(s.records) for s in self.segments)


# ---------------------------------------------------------------------------------------------------------------- the rule, on the reference's log

def expected_decided(a):
    """which exit of cns_extension the record took, from the logged return values (cns_ctg_subseq.c:44-108)"""
    if not a["found"] or not a["ok"]:
        return BY_NONE
    if a["edl_run"] == 1:
        return BY_PAIR
    return BY_BLOCKS_KEPT if a["dal_run"] >= 0 else BY_BLOCKS


def accepted_by_rule(a, rl, size):
    """cns_ctg_subseq.c:180, the second alternative as it is written there"""
    return bool(a["ident"] >= 90.0 and (int(a["qend"]) - int(a["qoff"]) >= rl * 0.6 or int(a["toff"]) - int(a["tend"]) >= size * 0.6))


def expected_states(cs, s, cap):
    """per record of segment s: the verdict the entry must report.  cap: from the loop's log; no cap: every record by the accept rule on its own alignment"""
    out = []
    for k, a in enumerate(s.ans):
        if cap and not a["passed"]:
            out.append(CAPPED)
        elif not a["found"]:
            out.append(NO_SEED)
        elif not a["ok"]:
            out.append(NO_ALIGNMENT)
        elif cap:
            out.append(ACCEPTED if a["order"] >= 0 else REJECTED)
        else:
            out.append(ACCEPTED if accepted_by_rule(a, cs.reads[int(a["qid"])].shape[0], s.size) else REJECTED)
    return out


# ---------------------------------------------------------------------------------------------------------------- crafted cases

def _subs(rng, codes, positions):
    out = codes.copy()
    for p in positions:
        out[p] = sc._other(out[p], rng)
    return out


def _noisy(rng, codes, err, clean=40):
    """`codes` with errors at rate err, its first and last `clean` bases as they are"""
    if codes.shape[0] <= 2 * clean:
        return codes.copy()
    return np.concatenate([codes[:clean], sc._mutate(rng, codes[clean:-clean], err), codes[-clean:]]).astype(np.uint8)


def crafted(seed=CRAFT_SEED):
    """the crafted set: the smallest shapes at which each rule of ctg_extend.h can fail.  Every record that is there for a reason carries a tag; check_crafted
    asserts on the reference's log that it does what the tag says"""
    rng = np.random.default_rng(seed)
    cs = CaseSet()
    cs.contigs = [sc._rand(rng, 20000), sc._rand(rng, 60000), sc._rand(rng, 9000)]
    A, B, C, D = Segment("whole_20k", 0, 0, 20000), Segment("mid_60k", 1, 15000, 30000), Segment("end_60k", 1, 30000, 30000), Segment("whole_9k", 2, 0, 9000)
    cs.segments = [A, B, C, D]

    def own(name):
        return np.random.default_rng([seed, OWN_STREAM[name]])

    def read(strand_codes):
        qdir = int(rng.integers(0, 2))
        return cs.add_read(np.asarray(strand_codes, dtype=np.uint8), qdir), qdir

    def rec(s, r, soff, send, tag=None):
        assert not any(x[:2] == r for x in s.records), "a read twice in one segment: the log could not be told apart"
        s.records.append((r[0], r[1], int(soff), int(send)))
        if tag:
            s.tags[len(s.records) - 1] = tag

    def placed(s, a, b, err, tag=None, lo=0, hi=0, rng=rng):
        """a read of contig[a:b) at `err`, `lo` / `hi` random bases at its ends; its record is its true placement.  Where it crosses an end of the segment it has
        no error for 40 bases on either side"""
        g = cs.contigs[s.ctg_id]
        cuts = [a] + [x for x in (s.start, s.start + s.size) if a + 100 < x < b - 100] + [b]
        body = np.concatenate([_noisy(rng, g[cuts[i]:cuts[i + 1]], err) for i in range(len(cuts) - 1)])
        rec(s, read(np.concatenate([sc._rand(rng, lo), body, sc._rand(rng, hi)])), a, b, tag)

    g0, g1, g2 = cs.contigs
    # ---- the whole 20 kb contig
    for a, n, err in ((0, 1900, 0.05), (4600, 5200, 0.08), (9000, 2600, 0.12), (9500, 6000, 0.10), (12500, 4100, 0.06), (15000, 5000, 0.09), (17800, 2200, 0.07), (6500, 1500, 0.05)):
        placed(A, a, a + n, err, lo=int(rng.integers(0, 30)), hi=int(rng.integers(0, 30)))
    # one 320-base insertion / deletion between two good halves: the block-wise aligner stops there, more than 200 short of the chain; the pair goes through
    # (what the aligners make of such a read depends on its errors: these cases draw theirs from streams of their own, picked so that check_crafted holds)
    r = own("insertion")
    ins = np.concatenate([_noisy(r, g0[4500:7000], 0.02), sc._rand(r, 300), _noisy(r, g0[7000:9500], 0.02)])
    rec(A, read(ins), 4500, 9500, "insertion")
    r = own("deletion")
    dele = np.concatenate([_noisy(r, g0[11000:13500], 0.02), _noisy(r, g0[13790:16290], 0.02)])
    rec(A, read(dele), 11000, 16290, "deletion")
    # fewer than 1000 columns and no pair either: at error 0.5 DALIGNER runs through anything to an end of the read or of the segment, so its range stays below
    # 1000 bases only where the read does
    rec(A, read(_noisy(rng, g0[16000:16960], 0.05)), 16000, 16960, "too_short")
    rec(A, read(sc._rand(rng, 2500)), 3000, 5500, "no_seed")
    # identity around 90: 3000 bases with 5 substitutions per 50 (26 clean bases in between for the seeds), one fewer and one more
    for tag, delta in (("ident_above", -1), ("ident_at", 0), ("ident_below", 1)):
        pos = [50 * p + o for p in range(60) for o in (3, 8, 13, 18, 23)]
        pos = pos[:-1] if delta < 0 else pos + [50 * 30 + 30] if delta > 0 else pos
        rec(A, read(_subs(rng, g0[6000:9000], pos)), 6000, 9000, tag)
    # qe - qb at and one below rl * 0.6: an exact copy of 3000 / 2999 bases in a read of 5000
    for tag, n in (("ratio_at", 3000), ("ratio_below", 2999)):
        junk = np.tile(np.array([0, 0, 1, 1], dtype=np.uint8), 2000)[:5000 - n]
        junk[0] = sc._other(g0[16500 + n], rng)
        rec(A, read(np.concatenate([g0[16500:16500 + n], junk])), 16500, 16500 + n, tag)
    # a stack on [2000, 4500), where no other read lies: exact copies, so the counters there are known numbers.  The third record is a read the accept rule turns down; it must not count:
    # ten more are accepted, the twelfth and thirteenth record find the range full
    for k in range(13):
        if k == 2:
            placed(A, 2000, 4500, 0.16, "stack_rejected")
        else:
            rec(A, read(g0[2000:4500]), 2000, 4500, "stack_%d" % (k if k < 2 else k - 1))
    # exactly 199 / 200 positions of the record's range below 10 (the stack's counters are 10, everything behind 4500 is lower)
    open_at = 4500
    rec(A, read(_noisy(rng, g0[3000:open_at + 199], 0.03)), 3000, open_at + 199, "open_199")
    rec(A, read(_noisy(rng, g0[3000:open_at + 200], 0.03)), 3000, open_at + 200, "open_200")
    # ---- [15 000, 45 000) of the 60 kb contig: contig bases on both sides
    placed(B, 14200, 17500, 0.06, "over_start", rng=own("over_start_mid"))
    placed(B, 43000, 45800, 0.06, "over_end", rng=own("over_end_mid"))
    placed(B, 20000, 24500, 0.09)
    placed(B, 26000, 29000, 0.11)
    stack = [read(g1[36000:38500]) for _ in range(9)]
    for r in stack:
        rec(B, r, 36000, 38500)
    ra, rb = read(g1[36000:38500]), read(g1[36000:38500])
    rec(B, ra, 36000, 38500, "equal_first")
    rec(B, rb, 36000, 38500, "equal_second")
    # ---- [30 000, 60 000) of the same: the same stack, the pair of equal soff the other way round
    placed(C, 29200, 32000, 0.06, "over_start", rng=own("over_start_end"))
    placed(C, 50000, 55500, 0.08)
    placed(C, 57000, 60000, 0.05)
    for r in stack:
        rec(C, r, 36000, 38500)
    rec(C, rb, 36000, 38500, "equal_first")
    rec(C, ra, 36000, 38500, "equal_second")
    # ---- the 9 kb contig: a 16 kb read across all of it (rejected: the second alternative of the accept rule is never true), and some reads
    rec(D, read(np.concatenate([sc._rand(rng, 3500), _noisy(rng, g2, 0.05), sc._rand(rng, 3500)])), 0, 9000, "quirk")
    for a, n, err in ((0, 4000, 0.07), (2500, 5500, 0.10), (5000, 4000, 0.12), (1000, 2000, 0.05), (6800, 2200, 0.08)):
        placed(D, a, a + n, err)
    return cs


def check_crafted(cs):
    """every tagged record does in the reference's log what it is there for"""
    def counters(s, upto):
        cov = np.zeros(s.size, dtype=np.uint8)
        for k in np.argsort([a["order"] if a["order"] >= 0 else 1 << 30 for a in s.ans], kind="stable"):
            a = s.ans[k]
            if a["order"] < 0 or k >= upto:
                continue
            cov[int(a["toff"]):int(a["tend"])] += 1
        return cov

    def open_positions(s, k):
        _, _, soff, send = s.records[k]
        sb, se = max(soff - s.start, 0), min(send - s.start, s.size)
        return int((counters(s, k)[sb:se] < 10).sum())

    seen = set()
    for s in cs.segments:
        ctg = cs.contigs[s.ctg_id]
        states = expected_states(cs, s, True)
        for k, tag in s.tags.items():
            a, st = s.ans[k], states[k]
            rl = cs.reads[int(a["qid"])].shape[0]
            seen.add(tag.rstrip("0123456789"))
            if tag == "insertion" or tag == "deletion":
                assert a["onc_ret"] == 1 and a["dal_run"] == 1 and a["edl_run"] == 1 and st == ACCEPTED, (tag, a)
                assert a["qend"] - a["qoff"] > (a["onc_qend"] - a["onc_qoff"]) + 1000 and abs((a["qend"] - a["qoff"]) - (a["tend"] - a["toff"])) > 250, (tag, a)
            elif tag == "too_short":
                assert a["found"] == 1 and a["onc_ret"] == 0 and a["dal_run"] == 0 and a["ok"] == 0 and st == NO_ALIGNMENT and rl < 1000, (tag, a)
            elif tag == "no_seed":
                assert a["passed"] == 1 and a["found"] == 0 and st == NO_SEED, (tag, a)
            elif tag == "ident_above":
                assert 90.0 <= a["ident"] < 90.06 and st == ACCEPTED, (tag, a)
            elif tag == "ident_below":
                assert 89.94 < a["ident"] < 90.0 and st == REJECTED, (tag, a)
            elif tag == "ident_at":
                assert 89.94 < a["ident"] < 90.06, (tag, a)
            elif tag == "ratio_at":
                assert a["qend"] - a["qoff"] == 3000 and rl == 5000 and a["ident"] >= 90.0 and st == ACCEPTED, (tag, a)
            elif tag == "ratio_below":
                assert a["qend"] - a["qoff"] == 2999 and rl == 5000 and a["ident"] >= 90.0 and st == REJECTED, (tag, a)
            elif tag == "stack_rejected":
                assert st == REJECTED and a["ok"] == 1 and a["tend"] - a["toff"] > 2300, (tag, a)
            elif tag.startswith("stack_"):
                n = int(tag[6:])
                assert st == (ACCEPTED if n < 10 else CAPPED), (tag, a)
                assert n >= 10 or (a["toff"], a["tend"]) == (2000, 4500), (tag, a)
                assert n < 10 or open_positions(s, k) == 0
            elif tag == "open_199":
                assert open_positions(s, k) == 199 and st == CAPPED, (tag, open_positions(s, k))
            elif tag == "open_200":
                assert open_positions(s, k) == 200 and st != CAPPED, (tag, open_positions(s, k))
            elif tag == "over_start":
                assert s.start > 0 and s.records[k][2] < s.start - 500 and a["toff"] == 0 and a["qoff"] > 500 and st == ACCEPTED, (tag, a)
            elif tag == "over_end":
                assert s.start + s.size < ctg.shape[0] and s.records[k][3] > s.start + s.size + 500 and a["tend"] == s.size and rl - a["qend"] > 500 and st == ACCEPTED, (tag, a)
            elif tag == "equal_first":
                assert st == ACCEPTED and s.records[k][2] == s.records[k + 1][2], (tag, a)
            elif tag == "equal_second":
                assert st == CAPPED, (tag, a)
            elif tag == "quirk":
                assert rl > s.size / 0.6 and a["toff"] < 50 and a["tend"] > s.size - 50 and a["ident"] >= 90.0 and st == REJECTED, (tag, a)
            else:
                raise AssertionError("a tag without a check: " + tag)
    assert seen == {"insertion", "deletion", "too_short", "no_seed", "ident_above", "ident_at", "ident_below", "ratio_at", "ratio_below", "stack_rejected", "stack_",
                    "open_", "over_start", "over_end", "equal_first", "equal_second", "quirk"}, sorted(seen)
    by = cs.by_name()
    first = {n: [s.records[k][:2] for k, t in s.tags.items() if t == "equal_first"] for n, s in by.items()}
    assert first["mid_60k"] and first["end_60k"] and first["mid_60k"] != first["end_60k"]          # the pair of equal soff: each order keeps its first


# ---------------------------------------------------------------------------------------------------------------- the natural case

def natural_base():
    """contig and reads of the consensus half's natural case (tests/golden/ctg_g), one segment over the whole contig, no records yet"""
    from tests import ctg_cases as cc
    gold = os.path.join(ROOT, "tests", "golden", "ctg_g")
    src = cc.read_cases(os.path.join(gold, "nat.bin.gz"), os.path.join(gold, "nat.reads.bin.gz"))
    cs = CaseSet()
    cs.contigs = [np.array(src.cases[0].contig, dtype=np.uint8)]
    cs.reads = [np.array(r, dtype=np.uint8) for r in src.reads]
    cs.segments = [Segment("nat_whole", 0, 0, cs.contigs[0].shape[0])]
    return cs, src.cases[0]


# ---------------------------------------------------------------------------------------------------------------- the reference harness

def reference_sources():
    import glob
    lib = [f for f in sorted(glob.glob(os.path.join(REF_SRC, "common", "*.c"))) if os.path.basename(f) != "main.c"]
    lib += [os.path.join(REF_SRC, "klib", "kstring.c"), os.path.join(REF_SRC, "klib", "kalloc.c"), os.path.join(REF_SRC, "edlib", "edlib_wrapper.c")]
    lib += sorted(glob.glob(os.path.join(REF_SRC, "gapped_align", "*.c")))
    return lib, [os.path.join(REF_SRC, "ctg_cns", n + ".c") for n in ("chain_dp", "mem_finder", "cns_ctg_subseq", "fc_correct_one_read", "small_object_alloc")]


def build_harness(outdir):
    """the reference's cns_ctg_subseq and everything it calls behind our main and logging shim (tests/golden/ctg_ext_ref_harness.c), compiled into outdir - outside
    the repository"""
    os.makedirs(outdir, exist_ok=True)
    exe, edlib_o = os.path.join(outdir, "ctg_ext_ref_harness"), os.path.join(outdir, "edlib.o")
    subprocess.run(["g++", "-O2", "-w", "-c", os.path.join(REF_SRC, "edlib", "edlib.cpp"), "-o", edlib_o], check=True)
    lib, ctg = reference_sources()
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-ffp-contract=off", "-pthread", "-I", REF_SRC, WRAPS, "-o", exe, HARNESS] + lib + ctg +
                   [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    return exe


def _ops_of(qa, ta):
    qa, ta = np.frombuffer(qa, np.uint8), np.frombuffer(ta, np.uint8)
    gap = ord("-")
    return np.where(ta == gap, 1, np.where(qa == gap, 2, np.where(qa == ta, 0, 3))).astype(np.uint8)


def parse_log(lines):
    """the shim's lines as a list of blocks: ("B", from, size, records, passes) per cns_ctg_subseq call, ("J", k, events) per record alone.  events / a pass: dict
    with X (qid, strand), F, A, D, L (tuples of numbers), T or C (numbers, query line, target line)"""
    out, i, cur, in_b = [], 0, None, False
    num = lambda x: float(x) if (b"." in x or b"e" in x or b"n" in x) else int(x)
    while i < len(lines):
        ln = lines[i]; i += 1
        if not ln:
            continue
        tag, v = ln[:1], ln[2:].split()
        if tag == b"B":
            recs = []
            for _ in range(int(v[2])):
                m = lines[i].split(); i += 1
                assert m[0] == b"M"
                recs.append(tuple(int(x) for x in m[1:]))
            out.append(("B", int(v[0]), int(v[1]), recs, []))
            cur, in_b = None, True
        elif tag == b"J":
            cur = {}
            out.append(("J", int(v[0]), cur))
        elif tag == b"Z":
            cur, in_b = None, False
        elif tag == b"X":
            if in_b:
                cur = {}
                out[-1][4].append(cur)
            if cur is not None:
                cur["X"] = (int(v[0]), int(v[1]))
        elif cur is None:
            continue
        elif tag in (b"T", b"C"):
            vals = [num(x) for x in v]
            n = vals[4] if tag == b"T" else vals[6]
            if tag == b"T" or vals[0]:
                cur[tag.decode()] = (vals, lines[i], lines[i + 1])
                assert len(lines[i]) == n and len(lines[i + 1]) == n
                i += 2
            else:
                cur["C"] = (vals, b"", b"")
        else:
            cur[tag.decode()] = tuple(num(x) for x in v)
    return out


def write_harness_input(cs, path, modes=b"GE"):
    with open(path, "wb") as f:
        for r in cs.reads:
            f.write(b"R" + np.int32(r.shape[0]).tobytes() + r.tobytes())
        for s in cs.segments:
            f.write(b"S" + np.int64(s.start).tobytes() + np.int32(s.size).tobytes() + cs.segment_codes(s).tobytes())
            for m in modes:
                for qid, qdir, soff, send in s.records:
                    f.write(b"M" + np.array([qid, qdir], "<i4").tobytes() + np.array([soff, send], "<i8").tobytes())
                f.write(bytes([m]))


def _fill_alone(a, ev):
    a["found"] = ev["F"][0]
    a["dal_run"] = a["edl_run"] = -1
    if "A" in ev:
        a["onc_ret"], a["onc_qoff"], a["onc_qend"], a["onc_toff"], a["onc_tend"], a["onc_ident"] = ev["A"]
    if "D" in ev:
        a["dal_run"], a["dal_qoff"], a["dal_qend"], a["dal_toff"], a["dal_tend"], a["dal_diffs"] = ev["D"]
    if "L" in ev:
        a["edl_run"], a["edl_qoff"], a["edl_qend"], a["edl_toff"], a["edl_tend"], a["edl_ident"] = ev["L"]


def answers_from_log(cs, blocks):
    """the parsed log of write_harness_input(cs, "GE") into every segment's ans / ops; asserts that the loop's calls are the record-alone calls"""
    at = 0
    for s in cs.segments:
        n = len(s.records)
        s.ans = np.zeros(n, dtype=ANS_DTYPE)
        s.ops = [None] * n
        for k, (qid, qdir, soff, send) in enumerate(s.records):
            s.ans[k]["qid"], s.ans[k]["qdir"], s.ans[k]["soff"], s.ans[k]["send"], s.ans[k]["order"] = qid, qdir, soff, send, -1
        b = blocks[at]; at += 1
        assert b[0] == "B" and (b[1], b[2]) == (s.start, s.size) and b[3] == s.records, (s.name, b[:3])
        loop = {}
        order = 0
        for ev in b[4]:
            ks = [k for k, r in enumerate(s.records) if r[:2] == ev["X"]]
            assert len(ks) == 1
            s.ans[ks[0]]["passed"] = 1
            loop[ks[0]] = ev
            if "T" in ev:
                s.ans[ks[0]]["order"] = order; order += 1
        for k in range(n):
            j = blocks[at]; at += 1
            assert j[0] == "J" and j[1] == k
            ev, a = j[2], s.ans[k]
            _fill_alone(a, ev)
            if "C" in ev and ev["C"][0][0]:
                v, qa, ta = ev["C"]
                a["ok"], a["qoff"], a["qend"], a["toff"], a["tend"], a["ident"], a["align_size"] = v
                s.ops[k] = _ops_of(qa, ta)
            if k in loop:          # the same calls with the same answers inside the loop
                lv = loop[k]
                assert all(lv.get(t) == ev.get(t) for t in "FADL"), (s.name, k, lv, ev)
                if "T" in lv:
                    tv, qa, ta = lv["T"]
                    assert tuple(tv) == (a["qoff"], a["qend"], a["toff"], a["tend"], a["align_size"]) and (_ops_of(qa, ta) == s.ops[k]).all(), (s.name, k)
    assert at == len(blocks), (at, len(blocks))


def run_harness(exe, cs, tmp):
    inp, log = os.path.join(tmp, "ext_harness_in.bin"), os.path.join(tmp, "ext_harness.log")
    write_harness_input(cs, inp)
    subprocess.run([exe, inp], check=True, env=dict(os.environ, CTG_EXT_LOG=log), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    answers_from_log(cs, parse_log(open(log, "rb").read().split(b"\n")))


# ---------------------------------------------------------------------------------------------------------------- the case file

def write_cases(cs, path, n_base_reads=0, contigs=True):
    """n_base_reads: the first reads are another file's; contigs = False: so are the contigs"""
    coff, cw = sc._volume(cs.contigs if contigs else [])
    roff, rw = sc._volume(cs.reads[n_base_reads:])
    ans = np.concatenate([s.ans for s in cs.segments]) if cs.segments else np.zeros(0, ANS_DTYPE)
    blob, k = b"", 0
    from tests import ctg_cases as cc
    for s in cs.segments:
        for o in s.ops:
            if o is not None:
                ans[k]["ops_off"] = len(blob)
                blob += cc._pad8(cc.pack_ops(o))
            k += 1
    with open(path, "wb") as f:
        f.write(b"CTGEXT01" + np.array([len(cs.contigs) if contigs else 0, cw.shape[0], len(cs.reads) - n_base_reads, rw.shape[0], len(cs.segments), ans.shape[0], len(blob)],
                                       dtype="<u8").tobytes())
        f.write(coff.tobytes() + cw.tobytes() + roff.tobytes() + rw.tobytes())
        k = 0
        for s in cs.segments:
            f.write(s.name.encode()[:31].ljust(32, b"\0") + np.array([s.ctg_id, s.start, s.size, k, k + len(s.records)], dtype="<i8").tobytes())
            k += len(s.records)
        f.write(ans.tobytes() + blob)


def read_cases(path, base=None):
    """base: the case set whose contigs and first reads the file relies on (the natural case)"""
    raw = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
    assert raw[:8] == b"CTGEXT01"
    nc, ncw, nr, nrw, ns, nrec, nops = (int(x) for x in np.frombuffer(raw, "<u8", 7, 8))
    at = 64

    def volume(n, nw, at):
        off = np.frombuffer(raw, "<u8", n + 1, at); at += 8 * (n + 1)
        words = np.frombuffer(raw, "<u8", nw, at); at += 8 * nw
        codes = ((words[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)).astype(np.uint8).reshape(-1)
        return [codes[int(off[i]):int(off[i + 1])] for i in range(n)], at
    cs = CaseSet()
    contigs, at = volume(nc, ncw, at)
    reads, at = volume(nr, nrw, at)
    cs.contigs = contigs if base is None else base.contigs
    cs.reads = (base.reads if base is not None else []) + reads
    segs = []
    for _ in range(ns):
        name = raw[at:at + 32].rstrip(b"\0").decode(); at += 32
        cid, start, size, b, e = (int(x) for x in np.frombuffer(raw, "<i8", 5, at)); at += 40
        segs.append((Segment(name, cid, start, size), b, e))
    ans = np.frombuffer(raw, ANS_DTYPE, nrec, at); at += ANS_DTYPE.itemsize * nrec
    blob = np.frombuffer(raw, np.uint8, nops, at); at += nops
    assert at == len(raw), (at, len(raw))
    for s, b, e in segs:
        s.ans = ans[b:e]
        s.records = [(int(a["qid"]), int(a["qdir"]), int(a["soff"]), int(a["send"])) for a in s.ans]
        s.ops = []
        for a in s.ans:
            if not a["ok"]:
                s.ops.append(None)
                continue
            n = int(a["align_size"])
            p = blob[int(a["ops_off"]):int(a["ops_off"]) + (n + 3) // 4]
            s.ops.append(np.stack([p & 3, (p >> 2) & 3, (p >> 4) & 3, (p >> 6) & 3], axis=1).reshape(-1)[:n].astype(np.uint8))
        cs.segments.append(s)
    return cs


def load_crafted():
    return read_cases(os.path.join(GOLD, "craft.bin.gz"))


def load_natural():
    base, case = natural_base()
    return read_cases(os.path.join(GOLD, "nat.bin.gz"), base), case


def checker_input(cs, path, cap):
    """what tests/host_core/check_ctg_extend.cpp reads: per segment its records with the reference's per-record aligner results, and what the pass must give"""
    with open(path, "w") as f:
        f.write("%d %d\n" % (len(cs.segments), 1 if cap else 0))
        for s in cs.segments:
            states = expected_states(cs, s, cap)
            if cap:
                order = [k for k in np.argsort([a["order"] for a in s.ans], kind="stable") if s.ans[k]["order"] >= 0]
            else:
                order = [k for k, st in enumerate(states) if st == ACCEPTED]
            n_used = sum(1 for st in states if st in (NO_ALIGNMENT, REJECTED, ACCEPTED))
            f.write("%d %d %d %d %d\n" % (s.start, s.size, len(s.records), n_used, len(order)))
            for k, a in enumerate(s.ans):
                f.write("%d %d %d %d %d %d %d %d %d %s %d\n" % (a["soff"], a["send"], cs.reads[int(a["qid"])].shape[0], a["found"], a["ok"], a["qoff"], a["qend"], a["toff"], a["tend"],
                                                             float(a["ident"]).hex(), states[k]))
            f.write(" ".join(str(int(k)) for k in order) + "\n")
