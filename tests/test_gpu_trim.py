"""GPU tests of the read trimming stage: necat_trim_partition / necat_trim_ranges (necat_amd/csrc/trim_kernels.h) and the device path of
oc2lcr against files the REFERENCE's programs wrote (tests/golden/trim_f) and against the host restatement (trim_core.h through
tests/host_core/check_trim.cpp).  Reads tests/golden only."""
import hashlib
import os

import numpy as np
import pytest

from necat_amd import capi
from tests import trim_util as tu

pytestmark = pytest.mark.gpu
ALL_RUNS = tu.CRAFT_RUNS + [("nat", "")]


@pytest.fixture(scope="module")
def progs(built):
    built.build_cli()
    return tu.PROG


@pytest.fixture(scope="module")
def check_trim(tmp_path_factory):
    return tu.build_check_trim(tmp_path_factory.mktemp("check_trim"))


def cutoff(arg):
    return 100.0 - 100.0 * float(arg)          # the programs' expression


def golden_partition_records(case, d):
    wrk, m4, num_reads = tu.install_partitions(case, d)
    parts = [np.fromfile("%s.p%d" % (m4, p), dtype=tu.M4_DTYPE) for p in range(len(tu.case_entry(case)["partition_records"]))]
    return wrk, m4, num_reads, np.concatenate(parts)


def grouped(recs, num_reads):
    """records ordered by subject id + read_off[num_reads + 3]"""
    g = recs[np.argsort(recs["sid"], kind="stable")]
    off = np.zeros(num_reads + 3, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(g["sid"], minlength=num_reads + 2))
    return g, off


def by_read(recs):
    """{sid: sorted record tuples}; the 4 padding bytes of a record are not data"""
    out = {}
    names = [n for n in tu.M4_DTYPE.names if n != "_pad"]
    for row in zip(*[recs[n].tolist() for n in names]):
        out.setdefault(row[6], []).append(row)
    return {k: sorted(v) for k, v in out.items()}


@pytest.mark.parametrize("case", sorted(tu.MANIFEST["cases"]) + ["nat"])
def test_trim_partition_matches_reference_files(ctx, tmp_path, case):
    """necat_trim_partition on the case's records: per read the multiset of records of the reference oc2pm4's partition files; read_off = the run lengths"""
    wrk, m4, num_reads, want = golden_partition_records(case, tmp_path)
    recs = np.fromfile(m4, dtype=tu.M4_DTYPE)
    got, off = ctx.trim_partition(recs, num_reads, cutoff(tu.case_entry(case).get("pm4_cutoff", "0.1")))
    assert got.shape[0] == want.shape[0] == int(off[-1]) and off.shape[0] == num_reads + 3 and int(off[0]) == 0
    assert np.array_equal(np.diff(off.astype(np.int64)), np.bincount(want["sid"], minlength=num_reads + 2))
    assert np.array_equal(got["sid"], np.repeat(np.arange(num_reads + 2), np.diff(off.astype(np.int64))))
    assert by_read(got) == by_read(want)


@pytest.mark.parametrize("case,run", ALL_RUNS)
def test_trim_ranges_on_reference_partitions(ctx, check_trim, tmp_path, case, run):
    """necat_trim_ranges on the reference's partition files: (left, right, size) == the reference for every read the device decides, how == trim_core.h's
    classification, and the reads handed back are EXACTLY the ones trim_core.h marks order-dependent - the device can neither hide an answer behind
    `host` nor decide a read it must not - within the manifest's cap"""
    wrk, m4, num_reads, recs = golden_partition_records(case, tmp_path)
    a = tu.run_args(case, run)
    want = tu.ranges_of_text(tu.golden_ranges_text(case, run))
    rows = tu.check_rows(check_trim, m4, num_reads, a)
    g, off = grouped(recs, num_reads)
    out, n_host = ctx.trim_ranges(num_reads, cutoff(a[0]), int(a[1]), int(a[2]), int(a[3]), g, off)
    handed = set(np.nonzero(out["how"] == capi.TRIM_HOST)[0].tolist())
    assert handed == {i for i in rows if rows[i][0][4]} and n_host == len(handed) <= tu.host_cap(case, run)
    for i in range(1, num_reads + 1):
        got = (int(out["left"][i]), int(out["right"][i]), int(out["size"][i]))
        if i in handed:
            assert got == (-1, 0, 0)
        else:
            assert got == want[i] and int(out["how"][i]) == rows[i][0][3], "read %d: %r how %d, reference %r decided as %d" % (i, got, out["how"][i], want[i], rows[i][0][3])


@pytest.mark.parametrize("case,run", ALL_RUNS)
def test_oc2lcr_device_path_is_byte_identical(progs, tmp_path, case, run):
    wrk, m4, num_reads = tu.install_partitions(case, tmp_path)
    out = os.path.join(wrk, "clipped_ranges.txt")
    r = tu.prog("oc2lcr", [m4, wrk] + tu.run_args(case, run) + [4, out])
    assert open(out, "rb").read() == tu.golden_ranges_text(case, run)
    census = tu.case_entry(case)["census"] if case == "nat" else tu.MANIFEST["cases"][case]["runs"][run]["census"]
    assert (b" %d decided on the host\n" % (census["a"] + census["b"] + census["c"])) in r.stderr, r.stderr


@pytest.mark.parametrize("case", ["main", "twoparts", "nat"])
def test_ranges_do_not_depend_on_input_order(ctx, tmp_path, case):
    """necat_trim_partition + necat_trim_ranges on the groups it left on the device, input records as they are, reversed and shuffled: the same ranges,
    and the reference's for every read not handed back"""
    wrk, m4, num_reads = tu.install_input(case, tmp_path)
    recs = np.fromfile(m4, dtype=tu.M4_DTYPE)
    a = tu.run_args(case)
    want = tu.ranges_of_text(tu.golden_ranges_text(case))
    outs = []
    for order in (np.arange(recs.shape[0]), np.arange(recs.shape[0])[::-1], np.random.default_rng(3).permutation(recs.shape[0])):
        n = ctx.trim_partition(recs[order], num_reads, cutoff("0.1"), download=False)
        assert n == sum(tu.case_entry(case)["partition_records"])
        out, n_host = ctx.trim_ranges(num_reads, cutoff(a[0]), int(a[1]), int(a[2]), int(a[3]))
        outs.append(out)
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()
    out = outs[0]
    decided = np.nonzero(out["how"][1:num_reads + 1] != capi.TRIM_HOST)[0] + 1
    assert decided.shape[0] >= num_reads - tu.host_cap(case)
    for i in decided.tolist():
        assert (int(out["left"][i]), int(out["right"][i]), int(out["size"][i])) == want[i], "read %d" % i


def test_whole_stage_on_the_natural_set(progs, tmp_path):
    """this tree's programs chained as the pipeline chains them: oc2mkdb -> oc2asmpm -u 1 per volume -> oc2pm4 -> oc2lcr (device) -> oc2etr ->
    oc2orderResults == the reference's final trimReads.fasta (sha256) and pm.m4.  The overlap lines are compared sorted: oc2asmpm's record order is
    free.  No read of this set is handed back to the host (manifest census), so the chain does not depend on that order."""
    nat = tu.MANIFEST["natural"]
    assert nat["census"]["a"] + nat["census"]["b"] + nat["census"]["c"] == 0
    d = str(tmp_path)
    reads = tu.gunzip("nat.reads.fasta.gz", os.path.join(d, "renum_reads.fasta"))
    open(os.path.join(d, "list.txt"), "w").write(reads + "\n")
    vols = os.path.join(d, "vols")
    os.makedirs(vols)
    tu.prog("oc2mkdb", [vols, os.path.join(d, "list.txt")])
    assert len(open(os.path.join(vols, "volume_names.txt")).read().splitlines()) == nat["volumes"]
    m4 = os.path.join(d, "pm.m4")
    with open(m4, "wb") as f:
        for v in range(nat["volumes"]):
            o = os.path.join(d, "v%d.m4" % v)
            tu.prog("oc2asmpm", nat["asm_args"].split() + ["-t", "4", vols, v, o])
            f.write(open(o, "rb").read())
    assert os.path.getsize(m4) == 96 * nat["records"]
    tu.prog("oc2pm4", [vols, m4, "0.1", 4])
    ranges = os.path.join(d, "clipped_ranges.txt")
    tu.prog("oc2lcr", [m4, vols] + nat["lcr_args"].split() + [4, ranges])
    assert open(ranges, "rb").read() == tu.golden_ranges_text("nat")
    comp, uncomp, tmp_pm = (os.path.join(d, n) for n in ("complete.fasta", "uncomplete.fasta", "tmp_pm.m4"))
    tu.prog("oc2etr", [ranges, reads, m4, comp, uncomp, tmp_pm])
    both = os.path.join(d, "tmp_trimReads.fasta")
    open(both, "wb").write(open(comp, "rb").read() + open(uncomp, "rb").read())
    trimmed, pm = os.path.join(d, "trimReads.fasta"), os.path.join(d, "final_pm.m4")
    tu.prog("oc2orderResults", [both, tmp_pm, trimmed, pm])
    assert hashlib.sha256(open(trimmed, "rb").read()).hexdigest() == nat["trimReads_fasta"]["sha256"]
    assert sorted(open(pm, "rb").read().splitlines()) == sorted(tu.golden_bytes("nat.pm.m4.gz").splitlines())


def synthetic_records(n_reads, n_recs, seed):
    """overlaps between neighbouring reads (so that a read meets the same query several times, on both strands, with few distinct scores), a share of
    them spanning their subject, identities on both sides of the 90 % cutoff"""
    rng = np.random.default_rng(seed)
    size = rng.integers(3000, 12000, size=n_reads + 1)
    sid = rng.integers(1, n_reads + 1, size=n_recs)
    qid = np.clip(sid + rng.integers(-4, 5, size=n_recs), 1, n_reads)
    qid = np.where(qid == sid, np.where(sid > 1, sid - 1, sid + 1), qid)
    r = np.zeros(n_recs, dtype=tu.M4_DTYPE)
    r["qid"], r["sid"] = qid, sid
    r["qdir"] = rng.integers(0, 2, size=n_recs)
    r["qsize"], r["ssize"] = size[qid], size[sid]
    span = rng.random(n_recs) < 0.05
    soff = (rng.random(n_recs) * 0.7 * size[sid]).astype(np.int64)
    send = np.minimum(size[sid] - 21, soff + 200 + (rng.random(n_recs) * 0.6 * size[sid]).astype(np.int64))
    r["soff"] = np.where(span, rng.integers(0, 25, size=n_recs), soff)
    r["send"] = np.where(span, size[sid] - rng.integers(0, 25, size=n_recs), np.maximum(send, soff + 1))
    qoff = (rng.random(n_recs) * 0.5 * size[qid]).astype(np.int64)
    r["qoff"] = qoff
    r["qend"] = np.minimum(size[qid], qoff + (r["send"] - r["soff"]).astype(np.int64))
    r["qext"], r["sext"] = r["qoff"], r["soff"]
    r["ident_perc"] = rng.integers(8800, 10000, size=n_recs) / 100.0
    r["vscore"] = rng.integers(100, 140, size=n_recs)
    return r


def test_scale_two_million_records(ctx, check_trim, tmp_path):
    """2 M synthetic records over 200 k reads (two partitions): the device's ranges == trim_core.h for every read it decides, and it hands back exactly
    the reads trim_core.h marks order-dependent"""
    num_reads, a = 200_000, "0.1 1 1 1000".split()
    recs = synthetic_records(num_reads, 2_000_000, 9)
    g, off = ctx.trim_partition(recs, num_reads, cutoff("0.1"))
    assert int(off[-1]) == g.shape[0] > 3_000_000
    out, n_host = ctx.trim_ranges(num_reads, cutoff(a[0]), int(a[1]), int(a[2]), int(a[3]))
    m4 = os.path.join(str(tmp_path), "s.m4")
    open(m4 + ".partitions", "w").write("2\n")
    cut = int(off[100_000])
    g[:cut].tofile(m4 + ".p0")
    g[cut:].tofile(m4 + ".p1")
    rows = tu.check_rows(check_trim, m4, num_reads, a)
    how = np.array([rows[i][0][3] for i in range(1, num_reads + 1)])
    reason = np.array([rows[i][0][4] for i in range(1, num_reads + 1)])
    host = np.array([rows[i][0][:3] for i in range(1, num_reads + 1)])
    o = out[1:num_reads + 1]
    handed = o["how"] == capi.TRIM_HOST
    assert np.array_equal(handed, reason != 0) and n_host == int(handed.sum())
    d = ~handed
    got = np.stack([o["left"], o["right"], o["size"]], axis=1)
    bad = np.nonzero(d & ((got != host).any(axis=1) | (o["how"] != how)))[0]
    assert bad.shape[0] == 0, "reads %r: device %r, trim_core.h %r" % ((bad[:5] + 1).tolist(), got[bad[:5]].tolist(), host[bad[:5]].tolist())
    assert {1, 2, 3} <= set(o["how"][d].tolist()) or {1, 3} <= set(o["how"][d].tolist())
    print("scale: %d reads, %d grouped records, handed back %d, how counts %r" % (num_reads, g.shape[0], n_host, np.bincount(o["how"], minlength=5).tolist()))
