#!/usr/bin/env python
"""Golden vectors for the consensus half of contig polishing (necat_ctg_consensus_batch), generated from the REFERENCE ITSELF.

Run in the build container only.  The reference's ctgcns and pm4 are compiled from /root/reference/src with plain gcc lines into a temporary directory OUTSIDE the
repository; oracle/_ref/oc2mkdb and oracle/_ref/oc2rm_worker (`make -C oracle ref`) make the volumes and the read-to-contig records.  Committed is data only, under
tests/golden/ctg_g/ (tests/ctg_cases.py has the format of the case files, stored gzip-compressed):

  nat.reads.bin.gz, nat.bin.gz
                  the natural case, its reads and the rest: one contig of 40 kb (1 % errors against the truth), reads of about 4 kb at 7 % error and 15 x.  ctgcns runs with our logging shim
                  (tests/golden/ctg_ref_harness.c, -DCTG_SHIM) linked in by -Wl,--wrap: every overlap the program hands to add_align_tags with the read it had
                  extracted last, the cns_seq / t_pos get_cns_from_align_tags leaves, and the program's polished contig.  Only the reads the program used are kept.
  craft.bin.gz    the crafted set (ctg_cases.crafted(CRAFT_SEED)): the reference's two functions called directly on made-up gapped strings by the harness's own main
  manifest.json   sizes and counts

    python tests/golden/make_golden_ctgcns.py
"""
import glob
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from necat_amd import synth  # noqa: E402
from tests import ctg_cases as cc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ctg_g")
REF_SRC = cc.REF_SRC
CRAFT_SEED = 1
NAT = dict(contig=40_000, contig_err=0.01, coverage=15.0, read_err=0.07, mean_len=4000.0, sd_len=800.0, min_len=2000, seed=2024, rm_args="-u 1 -z 20 -t 1")
LARGEST_FIXTURE = 181_770          # tests/golden/trim_f/nat.reads.fasta.gz: no new file may be larger


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(cmd), r.returncode, r.stderr.decode(errors="replace")[-3000:]))
    return r


def build_reference(outdir):
    """the reference's pm4 and its ctgcns with the logging shim wrapped around three of its functions, compiled into outdir (outside the repository)"""
    src = REF_SRC
    os.makedirs(outdir, exist_ok=True)
    lib = [f for f in sorted(glob.glob(os.path.join(src, "common", "*.c"))) if os.path.basename(f) != "main.c"]
    lib += [os.path.join(src, "klib", "kstring.c"), os.path.join(src, "klib", "kalloc.c"), os.path.join(src, "edlib", "edlib_wrapper.c")]
    lib += sorted(glob.glob(os.path.join(src, "gapped_align", "*.c")))
    edlib_o = os.path.join(outdir, "edlib.o")
    subprocess.run(["g++", "-O2", "-w", "-c", os.path.join(src, "edlib", "edlib.cpp"), "-o", edlib_o], check=True)
    cg = lambda *names: [os.path.join(src, "ctg_cns", n + ".c") for n in names]
    cflags = ["gcc", "-O2", "-std=gnu99", "-w", "-D_GNU_SOURCE", "-ffp-contract=off", "-pthread"]
    out = {"pm4": os.path.join(outdir, "pm4"), "ctgcns": os.path.join(outdir, "ctgcns")}
    subprocess.run(cflags + ["-o", out["pm4"]] + lib + cg("pm4", "pm4_main") + [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    wraps = "-Wl,--wrap=add_align_tags,--wrap=get_cns_from_align_tags,--wrap=pdb_extract_sequence"
    subprocess.run(cflags + ["-DCTG_SHIM", "-I", src, wraps, "-o", out["ctgcns"], cc.HARNESS] + lib +
                   cg("main", "pm4", "load_ctg_read_ids", "cns_one_ctg", "chain_dp", "mem_finder", "cns_ctg_subseq", "fc_correct_one_read", "small_object_alloc") +
                   [edlib_o, "-lm", "-lz", "-lstdc++"], check=True)
    return out


def write_fasta(path, seqs, names):
    with open(path, "wb") as f:
        for s, n in zip(seqs, names):
            f.write(b">" + n.encode() + b"\n" + cc.LUT[s].tobytes() + b"\n")


def mkdb(ref_bin, d, fasta):
    os.makedirs(d)
    lst = os.path.join(d, "list.txt")
    open(lst, "w").write(fasta + "\n")
    run([os.path.join(ref_bin, "oc2mkdb"), d, lst])


def natural(ref, ref_bin, tmp):
    rng = np.random.default_rng(NAT["seed"])
    truth = synth.make_genome(NAT["contig"], NAT["seed"])
    contig = synth._mutate(truth, NAT["contig_err"], rng)
    rs = synth.simulate_reads(coverage=NAT["coverage"], seed=NAT["seed"] + 1, err=NAT["read_err"], genome=truth, mean_len=NAT["mean_len"], sd_len=NAT["sd_len"], min_len=NAT["min_len"])
    reads = [rs.read(i).copy() for i in range(rs.nreads)]
    rfa, cfa = os.path.join(tmp, "reads.fasta"), os.path.join(tmp, "contigs.fasta")
    write_fasta(rfa, reads, ["r%d" % i for i in range(len(reads))])
    write_fasta(cfa, [contig], ["ctg0"])
    rdir, cdir = os.path.join(tmp, "reads_vols"), os.path.join(tmp, "ctg_vols")
    mkdb(ref_bin, rdir, rfa)
    mkdb(ref_bin, cdir, cfa)
    assert len(open(os.path.join(rdir, "volume_names.txt")).read().splitlines()) == 1
    m4 = os.path.join(tmp, "rd2ctg.m4")
    run([os.path.join(ref_bin, "oc2rm_worker")] + NAT["rm_args"].split() + [rdir, os.path.join(cdir, "vol0"), m4])
    run([ref["pm4"], cdir, m4])
    log, pol = os.path.join(tmp, "shim.log"), os.path.join(tmp, "polished.fasta")
    run([ref["ctgcns"], rdir, cdir, "1", pol], env=dict(os.environ, CTG_SHIM_LOG=log))
    # the log: every overlap, then the one segment's answer
    cs = cc.CaseSet()
    case = cc.Case("natural", contig)
    cs.cases.append(case)
    used = {}
    lines = open(log, "rb").read().split(b"\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith(b"O "):
            qid, qdir, qoff, qend, toff, tend, n = (int(x) for x in ln[2:].split())
            qa, ta = np.frombuffer(lines[i + 1], np.uint8), np.frombuffer(lines[i + 2], np.uint8)
            assert qa.shape[0] == n and ta.shape[0] == n
            gap = ord("-")
            ops = np.where(ta == gap, 1, np.where(qa == gap, 2, np.where(qa == ta, 0, 3))).astype(np.uint8)
            if qid not in used:
                used[qid] = cs.add_read(reads[qid])
            strand = cs.read_on_strand(used[qid], qdir)
            assert (cc.LUT[strand[qoff:qend]] == qa[qa != gap]).all() and (cc.LUT[contig[toff:tend]] == ta[ta != gap]).all(), "the logged strings are not the read's and the contig's"
            case.ovl.append((used[qid], qdir, qoff, qend, toff, tend, ops))
            i += 3
        elif ln.startswith(b"S "):
            size, min_cov = (int(x) for x in ln[2:].split())
            assert size == case.size and min_cov == 4
            (cns, tp), = cc.parse_answers(b"\n".join(lines[i + 1:i + 3]))
            case.cns, case.t_pos = cns, tp
            i += 3
        else:
            i += 1
    assert case.cns is not None, "the program made no consensus call"
    rec = open(pol, "rb").read().split(b"\n")
    assert rec[0] == b">ctg0" and len(rec) >= 2
    case.polished = rec[1]
    return cs, dict(reads=len(reads), reads_used=len(used), overlaps=len(case.ovl), columns=int(sum(o[6].shape[0] for o in case.ovl)), cns=len(case.cns),
                    lower=sum(1 for c in case.cns if c >= 97), polished=len(case.polished), contig=case.size)


def gz_to(src, dst):
    with open(src, "rb") as f, open(dst, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as g:
            g.write(f.read())


def main():
    ref_bin = os.path.join(ROOT, "oracle", "_ref")
    if not cc.have_reference() or not os.path.exists(os.path.join(ref_bin, "oc2rm_worker")):
        sys.exit("the reference's sources and oracle/_ref are needed: run in the build container after `make -C oracle ref`")
    tmp = tempfile.mkdtemp(prefix="golden_ctgcns_")          # outside the repository: reference binaries never enter it
    ref = build_reference(os.path.join(tmp, "refbin"))
    manifest = {}
    nat, manifest["natural"] = natural(ref, ref_bin, tmp)
    manifest["natural"]["settings"] = NAT
    cc.write_cases(nat, os.path.join(tmp, "nat.reads.bin"), cases=False)          # (two files: one would be larger than the largest fixture there is)
    cc.write_cases(nat, os.path.join(tmp, "nat.bin"), reads=False)
    craft = cc.crafted(CRAFT_SEED)
    cc.run_harness(cc.build_harness(os.path.join(tmp, "harness")), craft, tmp)
    cc.write_cases(craft, os.path.join(tmp, "craft.bin"))
    manifest["crafted"] = {"seed": CRAFT_SEED, "cases": {c.name: dict(size=c.size, overlaps=len(c.ovl), cns=len(c.cns), lower=sum(1 for x in c.cns if x >= 97)) for c in craft.cases}}
    os.makedirs(OUT, exist_ok=True)
    for leaf in ("nat.reads.bin", "nat.bin", "craft.bin"):
        dst = os.path.join(OUT, leaf + ".gz")
        gz_to(os.path.join(tmp, leaf), dst)
        manifest[leaf + ".gz"] = os.path.getsize(dst)
        assert os.path.getsize(dst) <= LARGEST_FIXTURE, "%s: %d bytes" % (leaf, os.path.getsize(dst))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(manifest, indent=1, sort_keys=True))
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
