"""CPU tests of the read trimming stage: the host restatement (necat_amd/csrc/trim_core.h), the device kernel's per-read core compiled
with g++ and run lane by lane (trim_kernels.h through tests/host_core/check_trim.cpp), and the four programs oc2pm4, oc2lcr (NECAT_TRIM_HOST=1),
oc2etr, oc2orderResults - against files the REFERENCE's programs wrote (tests/golden/trim_f, tests/golden/make_golden_trim.py)."""
import hashlib
import os
import shutil

import numpy as np
import pytest

from tests import trim_util as tu

HOST = {"NECAT_TRIM_HOST": "1"}
ALL_RUNS = tu.CRAFT_RUNS + [("nat", "")]


@pytest.fixture(scope="module")
def progs(built):
    built.build_cli()
    return tu.PROG


@pytest.fixture(scope="module")
def check_trim(tmp_path_factory):
    return tu.build_check_trim(tmp_path_factory.mktemp("check_trim"))


@pytest.mark.parametrize("case,run", ALL_RUNS)
def test_host_core_and_kernel_core_match_reference(check_trim, tmp_path, case, run):
    """trim_core.h == the reference's range on every read; the kernel's core, on the read's records in a shuffled order, == the same on every
    read it decides, its `how` == trim_core.h's classification, and it hands back exactly the reads trim_core.h marks order-dependent"""
    wrk, m4, num_reads = tu.install_partitions(case, tmp_path)
    want = tu.ranges_of_text(tu.golden_ranges_text(case, run))
    rows = tu.check_rows(check_trim, m4, num_reads, tu.run_args(case, run), seed=5)
    assert len(want) == num_reads == len(rows)
    n_host = 0
    for i in range(1, num_reads + 1):
        host, dev = rows[i]
        assert host[:3] == want[i], "trim_core.h, read %d: %r, reference %r" % (i, host[:3], want[i])
        if host[4]:                                  # order-dependent: not the device's to decide
            assert dev == (-1, 0, 0, 4), "read %d (reason %d) must be handed back, the core said %r" % (i, host[4], dev)
            n_host += 1
        else:
            assert dev[:3] == want[i] and dev[3] == host[3], "kernel core, read %d: %r, reference %r decided as %d" % (i, dev, want[i], host[3])
    assert n_host <= tu.host_cap(case, run)
    census = tu.case_entry(case)["census"] if case == "nat" else tu.MANIFEST["cases"][case]["runs"][run]["census"]
    assert n_host == census["a"] + census["b"] + census["c"]


@pytest.mark.parametrize("case", sorted(tu.MANIFEST["cases"]) + ["nat"])
def test_oc2pm4_one_thread_is_byte_identical(progs, tmp_path, case):
    """the partition files at one thread: the same records in the same order as the reference's.  Crafted cases: byte for byte.  The natural set's
    records come from the reference's oc2asmpm, which leaves the struct's 4 padding bytes (92 .. 95 of a record) uninitialised, and the reference's
    oc2pm4 copies records field by field in places, so what its files hold there is indeterminate stack content: those 4 bytes are masked, the other
    92 of every record are compared byte for byte."""
    wrk, m4, num_reads = tu.install_input(case, tmp_path / "ours")
    tu.prog("oc2pm4", [wrk, m4, tu.case_entry(case).get("pm4_cutoff", "0.1"), 1])
    rw, rm4, _ = tu.install_partitions(case, tmp_path / "ref")
    assert open(m4 + ".partitions", "rb").read() == open(rm4 + ".partitions", "rb").read()
    for p in range(len(tu.case_entry(case)["partition_records"])):
        a, b = np.fromfile("%s.p%d" % (m4, p), dtype=tu.M4_DTYPE), np.fromfile("%s.p%d" % (rm4, p), dtype=tu.M4_DTYPE)
        if case == "nat":
            a["_pad"] = 0
            b["_pad"] = 0
        assert a.tobytes() == b.tobytes(), "partition %d" % p
    assert not [f for f in os.listdir(wrk) if f.endswith(".part")]


@pytest.mark.parametrize("case", ["main", "twoparts"])
def test_oc2pm4_four_threads_same_multiset(progs, tmp_path, case):
    """several chunks (NECAT_PM4_CHUNK: 700 records) taken by four threads: every partition file holds the records the reference's holds"""
    wrk, m4, num_reads = tu.install_input(case, tmp_path / "ours")
    tu.prog("oc2pm4", [wrk, m4, "0.1", 4], env={"NECAT_PM4_CHUNK": "700"})
    rw, rm4, _ = tu.install_partitions(case, tmp_path / "ref")
    for p in range(len(tu.case_entry(case)["partition_records"])):
        a, b = np.fromfile("%s.p%d" % (m4, p), dtype=tu.M4_DTYPE), np.fromfile("%s.p%d" % (rm4, p), dtype=tu.M4_DTYPE)
        assert tu.rec_rows(a) == tu.rec_rows(b), "partition %d" % p


@pytest.mark.parametrize("case,run", ALL_RUNS)
def test_oc2lcr_host_path_is_byte_identical(progs, tmp_path, case, run):
    wrk, m4, num_reads = tu.install_partitions(case, tmp_path)
    out = os.path.join(wrk, "clipped_ranges.txt")
    a = tu.run_args(case, run)
    r = tu.prog("oc2lcr", [m4, wrk] + a + [2, out], env=HOST)
    assert open(out, "rb").read() == tu.golden_ranges_text(case, run)
    assert b"decided on the host" in r.stderr and not os.path.exists(out + ".part")


def _natural_stage(tmp_path):
    wrk, m4, num_reads = tu.install_partitions("nat", tmp_path)
    reads = tu.gunzip("nat.reads.fasta.gz", os.path.join(wrk, "renum_reads.fasta"))
    ranges = os.path.join(wrk, "clipped_ranges.txt")
    open(ranges, "wb").write(tu.golden_ranges_text("nat"))
    return wrk, m4, reads, ranges


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("gz", [False, True])
def test_oc2etr_and_oc2orderResults_are_byte_identical(progs, tmp_path, gz):
    """the rest of the stage on the natural set, from the reference's ranges: complete / trimmed reads (sha256 of the reference's files), the
    overlaps of complete reads and the renumbered overlaps (text, byte for byte); plain and gzip input"""
    wrk, m4, reads, ranges = _natural_stage(tmp_path)
    nat = tu.MANIFEST["natural"]
    if gz:
        import gzip
        with open(reads, "rb") as f, gzip.open(reads + ".gz", "wb") as g:
            g.write(f.read())
        reads += ".gz"
    comp, uncomp, tmp_pm = (os.path.join(wrk, n) for n in ("complete.fasta", "uncomplete.fasta", "tmp_pm.m4"))
    tu.prog("oc2etr", [ranges, reads, m4, comp, uncomp, tmp_pm])
    assert (_sha(comp), os.path.getsize(comp)) == (nat["complete_fasta"]["sha256"], nat["complete_fasta"]["bytes"])
    assert (_sha(uncomp), os.path.getsize(uncomp)) == (nat["uncomplete_fasta"]["sha256"], nat["uncomplete_fasta"]["bytes"])
    assert nat["uncomplete_fasta"]["bytes"] > 0
    assert open(tmp_pm, "rb").read() == tu.golden_bytes("nat.tmp_pm.m4.gz")
    both = os.path.join(wrk, "tmp_trimReads.fasta")
    open(both, "wb").write(open(comp, "rb").read() + open(uncomp, "rb").read())
    trimmed, pm = os.path.join(wrk, "trimReads.fasta"), os.path.join(wrk, "pm.m4")
    tu.prog("oc2orderResults", [both, tmp_pm, trimmed, pm])
    assert (_sha(trimmed), os.path.getsize(trimmed)) == (nat["trimReads_fasta"]["sha256"], nat["trimReads_fasta"]["bytes"])
    assert open(pm, "rb").read() == tu.golden_bytes("nat.pm.m4.gz")
    assert not [f for f in os.listdir(wrk) if f.endswith(".part")]


@pytest.mark.parametrize("name,nargs,stream", [("oc2pm4", 4, "stderr"), ("oc2lcr", 8, "stdout"), ("oc2etr", 6, "stderr"), ("oc2orderResults", 4, "stderr")])
def test_usage_and_exit_status(progs, name, nargs, stream):
    """a wrong argument count: the reference's usage text (oc2lcr prints its on stdout) and exit status 1"""
    for n in (0, nargs - 1, nargs + 1):
        r = tu.prog(name, ["x"] * n, check=False)
        assert r.returncode == 1
        text = getattr(r, stream).decode()
        assert text.startswith("USAGE:\n" + tu.PROG[name] + " ") and text.count("\n") == 2


def test_truncated_and_missing_inputs_leave_nothing(progs, tmp_path):
    """a record file cut inside a record, a missing file: exit status 1, a line on stderr, no output file and no .part file"""
    wrk, m4, num_reads = tu.install_partitions("main", tmp_path)
    before = set(os.listdir(wrk))
    cut = os.path.join(wrk, "cut.m4")
    open(cut, "wb").write(open(m4, "rb").read()[:96 * 40 + 17])
    r = tu.prog("oc2pm4", [wrk, cut, "0.1", 1], check=False)
    assert r.returncode == 1 and b"truncated" in r.stderr
    r = tu.prog("oc2pm4", [wrk, os.path.join(wrk, "absent.m4"), "0.1", 1], check=False)
    assert r.returncode == 1 and r.stderr
    assert set(os.listdir(wrk)) == before | {"cut.m4"}
    # oc2lcr: a partition file cut short
    with open(m4 + ".p0", "r+b") as f:
        f.truncate(96 * 100 + 50)
    out = os.path.join(wrk, "ranges.txt")
    r = tu.prog("oc2lcr", [m4, wrk] + tu.run_args("main") + [1, out], env=HOST, check=False)
    assert r.returncode == 1 and b"truncated" in r.stderr and not os.path.exists(out) and not os.path.exists(out + ".part")
    # oc2etr / oc2orderResults
    wrk2, m4n, reads, ranges = _natural_stage(tmp_path / "nat")
    open(cut, "wb").write(open(m4n, "rb").read()[:96 * 10 + 1])
    outs = [os.path.join(wrk2, n) for n in ("c.fasta", "u.fasta", "t.m4")]
    r = tu.prog("oc2etr", [ranges, reads, cut] + outs, check=False)
    assert r.returncode == 1 and b"truncated" in r.stderr
    r = tu.prog("oc2etr", [ranges, os.path.join(wrk2, "absent.fasta"), m4n] + outs, check=False)
    assert r.returncode == 1 and r.stderr
    r = tu.prog("oc2orderResults", [reads, os.path.join(wrk2, "absent.m4")] + outs[:2], check=False)
    assert r.returncode == 1 and r.stderr
    assert not [f for f in os.listdir(wrk2) if f.endswith(".part") or os.path.join(wrk2, f) in outs]


@pytest.fixture(scope="module")
def reference_programs(tmp_path_factory):
    """the reference's four programs, built by the golden generator's recipe into pytest's temporary directory (never into the repository)"""
    out = tmp_path_factory.mktemp("refbin")
    assert not str(out).startswith(tu.util.ROOT + os.sep)
    return tu.generator().build_reference(str(out))


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/trim_bases"), reason="the reference's sources are not on this machine")
@pytest.mark.parametrize("seed,kind,args", [(101, "main", "0.1 1 1 1000"), (102, "main", "0.1 500 2 1000"), (103, "stale", "0.04 1 1 1000")])
def test_fresh_fuzz_cases_against_the_reference_live(progs, check_trim, reference_programs, tmp_path_factory, seed, kind, args):
    """three more seeds of the golden generator's fuzzer through the reference's programs (built outside the repository by the generator's recipe)
    and through ours: partition files byte for byte, ranges byte for byte, trim_core.h and the kernel's core read for read"""
    gen = tu.generator()
    out = tmp_path_factory.mktemp("live")
    ref = reference_programs
    recs, num_reads = gen.fuzz_case(seed, kind, 0.6)
    rdir, odir = os.path.join(str(out), "ref"), os.path.join(str(out), "ours")
    os.makedirs(rdir); os.makedirs(odir)
    rm4, om4 = os.path.join(rdir, "f.m4"), os.path.join(odir, "f.m4")
    recs.tofile(rm4)
    shutil.copy(rm4, om4)
    ref_ranges = gen.run_reference_case(ref, rdir, rm4, num_reads, "0.1", {"": args})[""]
    tu.write_reads_info(odir, num_reads)
    tu.prog("oc2pm4", [odir, om4, "0.1", 1])
    assert open(om4 + ".p0", "rb").read() == open(rm4 + ".p0", "rb").read()       # crafted records: the padding is zero on both sides
    ours = os.path.join(odir, "ranges.txt")
    tu.prog("oc2lcr", [om4, odir] + args.split() + [1, ours], env=HOST)
    assert open(ours, "rb").read() == open(ref_ranges, "rb").read()
    want = tu.ranges_of_text(open(ref_ranges, "rb").read())
    rows = tu.check_rows(check_trim, om4, num_reads, args.split(), seed=seed)
    hows = set()
    for i in range(1, num_reads + 1):
        host, dev = rows[i]
        assert host[:3] == want[i]
        assert dev == ((-1, 0, 0, 4) if host[4] else want[i] + (host[3],)), "read %d" % i
        hows.add(4 if host[4] else host[3])
    assert hows >= {0, 1, 2, 3, 4}
