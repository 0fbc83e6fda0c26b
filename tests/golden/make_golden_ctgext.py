#!/usr/bin/env python
"""Golden vectors for the aligner and the coverage cap of contig polishing (necat_ctg_extend_batch), generated from the REFERENCE ITSELF.

Run in the build container only.  The reference's objects are compiled from its sources where they lie into a temporary directory OUTSIDE the repository, behind
our main and logging shim (tests/golden/ctg_ext_ref_harness.c, -Wl,--wrap: tests/ctg_ext_cases.py has the build line, the log and the file format).  Committed is
data only, under tests/golden/ctg_x/, gzip-compressed:

  craft.bin.gz    the crafted set (ctg_ext_cases.crafted()): contigs, reads, segments, records and per record what the reference's calls answered, in the loop
                  (cns_ctg_subseq) and alone (cns_extension with no cap).  check_crafted asserts here that every case does what it is there for.
  nat.bin.gz      the natural case of tests/golden/ctg_g (make_golden_ctgcns.py's settings, the same volumes, oc2rm_worker and pm4 runs): the reference's ctgcns
                  program runs with the shim linked in, which logs the records it hands to cns_ctg_subseq in loop order and every call below; the harness's own
                  main then repeats the loop on those records (the two logs must be equal) and calls cns_extension on every record alone.  Contig, reads and the
                  148 overlaps are ctg_g's, checked to be the same here; the file adds the records, their log and the reads no overlap of ctg_g uses.

    python tests/golden/make_golden_ctgext.py"""
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from necat_amd import synth  # noqa: E402
from tests import ctg_ext_cases as xc  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_ctgcns", os.path.join(ROOT, "tests", "golden", "make_golden_ctgcns.py"))
gc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gc)

MAX_BYTES = 148642          # tests/golden/ctg_g/nat.bin.gz: no file here may be larger


def build_program(outdir):
    """the reference's pm4 and its ctgcns with the logging shim wrapped around the calls of cns_ctg_subseq, compiled into outdir (outside the repository)"""
    src = xc.REF_SRC
    os.makedirs(outdir, exist_ok=True)
    lib, _ = xc.reference_sources()
    edlib_o = os.path.join(outdir, "edlib.o")
    subprocess.run(["g++", "-O2", "-w", "-c", os.path.join(src, "edlib", "edlib.cpp"), "-o", edlib_o], check=True)
    cg = lambda *names: [os.path.join(src, "ctg_cns", n + ".c") for n in names]
    cflags = ["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-ffp-contract=off", "-pthread"]
    out = {"pm4": os.path.join(outdir, "pm4"), "ctgcns": os.path.join(outdir, "ctgcns")}
    subprocess.run(cflags + ["-o", out["pm4"]] + lib + cg("pm4", "pm4_main") + [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    subprocess.run(cflags + ["-DCTG_EXT_SHIM", "-I", src, xc.WRAPS, "-o", out["ctgcns"], xc.HARNESS] + lib +
                   cg("main", "pm4", "load_ctg_read_ids", "cns_one_ctg", "chain_dp", "mem_finder", "cns_ctg_subseq", "fc_correct_one_read", "small_object_alloc") +
                   [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    return out


def natural(ref, ref_bin, exe, tmp):
    NAT = gc.NAT
    rng = np.random.default_rng(NAT["seed"])
    truth = synth.make_genome(NAT["contig"], NAT["seed"])
    contig = synth._mutate(truth, NAT["contig_err"], rng)
    rs = synth.simulate_reads(coverage=NAT["coverage"], seed=NAT["seed"] + 1, err=NAT["read_err"], genome=truth, mean_len=NAT["mean_len"], sd_len=NAT["sd_len"], min_len=NAT["min_len"])
    reads = [rs.read(i).copy() for i in range(rs.nreads)]
    rfa, cfa = os.path.join(tmp, "reads.fasta"), os.path.join(tmp, "contigs.fasta")
    gc.write_fasta(rfa, reads, ["r%d" % i for i in range(len(reads))])
    gc.write_fasta(cfa, [contig], ["ctg0"])
    rdir, cdir = os.path.join(tmp, "reads_vols"), os.path.join(tmp, "ctg_vols")
    gc.mkdb(ref_bin, rdir, rfa)
    gc.mkdb(ref_bin, cdir, cfa)
    m4 = os.path.join(tmp, "rd2ctg.m4")
    gc.run([os.path.join(ref_bin, "oc2rm_worker")] + NAT["rm_args"].split() + [rdir, os.path.join(cdir, "vol0"), m4])
    gc.run([ref["pm4"], cdir, m4])
    log, pol = os.path.join(tmp, "program.log"), os.path.join(tmp, "polished.fasta")
    gc.run([ref["ctgcns"], rdir, cdir, "1", pol], env=dict(os.environ, CTG_EXT_LOG=log))
    prog = [b for b in xc.parse_log(open(log, "rb").read().split(b"\n")) if b[0] == "B"]
    assert len(prog) == 1, "one segment was expected"
    _, start, size, records, passes = prog[0]
    # ctg_g numbered the reads in the order of their first overlap; the others follow in the order of their first record
    base, case = xc.natural_base()
    assert (start, size) == (0, base.contigs[0].shape[0]) and (base.contigs[0] == contig).all(), "not the contig of tests/golden/ctg_g"
    ids = {}
    for ev in passes:
        if "T" in ev and ev["X"][0] not in ids:
            ids[ev["X"][0]] = len(ids)
    assert len(ids) == len(base.reads) and all((base.reads[k] == reads[q]).all() for q, k in ids.items()), "not the reads of tests/golden/ctg_g"
    cs = base
    for q, _, _, _ in records:
        if q not in ids:
            ids[q] = len(ids)
            cs.reads.append(reads[q])
    seg = cs.segments[0]
    seg.records = [(ids[q], d, a, b) for q, d, a, b in records]
    assert len(set(r[:2] for r in seg.records)) == len(seg.records), "a read twice on one strand: the log could not be told apart"
    xc.run_harness(exe, cs, tmp)
    # the harness's loop is the program's: the same records got past the cap, the same calls gave the same answers, the same overlaps in the same order
    mine = [b for b in xc.parse_log(open(os.path.join(tmp, "ext_harness.log"), "rb").read().split(b"\n")) if b[0] == "B"][0]
    assert len(mine[4]) == len(passes)
    for a, b in zip(mine[4], passes):
        assert a["X"] == (ids[b["X"][0]], b["X"][1]) and all(a.get(t) == b.get(t) for t in "FADLT"), (a.get("X"), b.get("X"))
    # .. and ctg_g's
    ov = [k for k in np.argsort([x["order"] for x in seg.ans], kind="stable") if seg.ans[k]["order"] >= 0]
    assert len(ov) == len(case.ovl)
    for k, (qid, qdir, qoff, qend, toff, tend, ops) in zip(ov, case.ovl):
        a = seg.ans[k]
        assert (qid, qdir, qoff, qend, toff, tend) == tuple(int(a[f]) for f in ("qid", "qdir", "qoff", "qend", "toff", "tend")) and (seg.ops[k] == ops).all()
    return cs, len(case.ovl)


def main():
    ref_bin = os.path.join(ROOT, "oracle", "_ref")
    if not xc.have_reference() or not os.path.exists(os.path.join(ref_bin, "oc2rm_worker")):
        sys.exit("the reference's sources and oracle/_ref are needed: run in the build container after `make -C oracle ref`")
    tmp = tempfile.mkdtemp(prefix="golden_ctgext_")          # outside the repository: reference binaries never enter it
    exe = xc.build_harness(os.path.join(tmp, "harness"))
    os.makedirs(xc.GOLD, exist_ok=True)
    craft = xc.crafted()
    xc.run_harness(exe, craft, tmp)
    xc.check_crafted(craft)
    xc.write_cases(craft, os.path.join(tmp, "craft.bin"))
    nat, n_ov = natural(build_program(os.path.join(tmp, "refbin")), ref_bin, exe, tmp)
    n_base = len(xc.natural_base()[0].reads)
    xc.write_cases(nat, os.path.join(tmp, "nat.bin"), n_base_reads=n_base, contigs=False)
    for leaf in ("craft.bin", "nat.bin"):
        dst = os.path.join(xc.GOLD, leaf + ".gz")
        gc.gz_to(os.path.join(tmp, leaf), dst)
        assert os.path.getsize(dst) <= MAX_BYTES, "%s: %d bytes" % (leaf, os.path.getsize(dst))
        print(dst, os.path.getsize(dst), "bytes")
    for name, cs in (("crafted", craft), ("natural", nat)):
        for s in cs.segments:
            st = xc.expected_states(cs, s, True)
            print(name, s.name, "records", len(s.records), "by verdict (capped, no seed, no alignment, rejected, accepted)", [st.count(v) for v in range(5)],
                  "by exit (none, block-wise, pair, block-wise kept)", [sum(1 for a in s.ans if xc.expected_decided(a) == v) for v in range(4)])
    print("natural: reads", len(nat.reads), "of which ctg_g's", n_base, "overlaps", n_ov)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
