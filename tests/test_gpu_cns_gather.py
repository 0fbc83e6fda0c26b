"""oc2cns on a read set kept as one volume per file (NECAT_CNS_READS=gather): the project of the existing oc2cns program test, cut into three volumes, run in
chunks of templates whose reads are gathered on the device - against the same program with the read set merged (today's path) and against the golden files of
tests/golden/cns_c (what the reference's oc2cns wrote).  Both output files must be the same bytes; the trace line of the gather path says how many chunks a
partition took, which is also what fails without the feature."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from necat_amd import build, capi, synth
from oracle import oracle_api as ora
from tests import util

pytestmark = pytest.mark.gpu

MAN = json.load(open(os.path.join(util.GOLDEN, "cns_c", "manifest.json")))
CHUNK_BASES = 805_000          # of the project's 807 132 bases: the planner makes 13 chunks of the golden partition's 98 templates (every template names most reads)
TRACE = re.compile(r"\[oc2cns\] partition (\d+): (\d+) chunks of at most (\d+) bases, (\d+) reads and (\d+) bases gathered in ([0-9.]+) ms")


@pytest.fixture(scope="module")
def project(built, tmp_path_factory):
    """the golden reads through this repository's oc2mkdb at a volume size that gives three volumes; the golden candidate partition beside them"""
    built.build_cli()
    tmp = str(tmp_path_factory.mktemp("cns_gather"))
    src = util.install_golden_volumes("vols_c", os.path.join(tmp, "src"))
    fa = os.path.join(tmp, "reads.fasta")
    with open(fa, "w") as f:
        for path, _, _ in capi.load_volumes_info(src)[2]:
            pac, off, sz, names = synth.read_volume(path)
            codes = synth.unpack_2bit(pac, int(sz.sum()))
            for i, nm in enumerate(names):
                f.write(">%s\n%s\n" % (nm, bytes(b"ACGT"[c] for c in codes[int(off[i]):int(off[i] + sz[i])]).decode()))
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write(fa + "\n")
    wrk = os.path.join(tmp, "wrk")
    r = subprocess.run([build.OC2MKDB, wrk, lst], env=dict(os.environ, NECAT_MKDB_VOLSIZE="300000"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    nv, nr, _ = capi.load_volumes_info(wrk)
    assert (nv, nr) == (3, 98)
    can = os.path.join(tmp, "cands")
    for fn in ("cands.p0", "cands.partitions"):
        shutil.copy(os.path.join(util.GOLDEN, "cns_c", fn), os.path.join(tmp, fn))
    return wrk, can, tmp


def _oc2cns(argv, wrk, can, tmp, tag, mn=None, **env):
    co, ro = os.path.join(tmp, "cns_" + tag), os.path.join(tmp, "raw_" + tag)
    cmd = [build.OC2CNS] + argv + [wrk, can, co, ro] + (["-mn", str(mn[0]), str(mn[1])] if mn else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return open(co, "rb").read(), open(ro, "rb").read(), r.stderr


def _gather(argv, wrk, can, tmp, tag, chunk=CHUNK_BASES, **kw):
    env = dict(NECAT_CNS_READS="gather", NECAT_TRACE="2")
    if chunk is not None:
        env["NECAT_CNS_CHUNK_BASES"] = str(chunk)
    env.update(kw.pop("env", {}))
    cns, raw, err = _oc2cns(argv, wrk, can, tmp, tag, **kw, **env)
    return cns, raw, [tuple(int(x) for x in m.groups()[:5]) for m in TRACE.finditer(err)]


def _golden(name, cns, raw):
    m = MAN["oc2cns"][name]
    assert (len(cns), cns.count(b">")) == (m["cns_bytes"], m["cns_records"]) and hashlib.md5(cns).hexdigest() == m["cns_md5"]
    assert (len(raw), raw.count(b">")) == (m["raw_bytes"], m["raw_records"]) and hashlib.md5(raw).hexdigest() == m["raw_md5"]


@pytest.mark.parametrize("name", ["default", "x9_l3000"])
def test_gather_in_chunks_writes_the_merged_and_the_golden_files(project, name):
    wrk, can, tmp = project
    m = MAN["oc2cns"][name]
    argv = ora.cns_argv(ora.cns_options(**m["options"])) + m["extra_argv"] + ["-t", "3"]
    cns_m, raw_m, err_m = _oc2cns(argv, wrk, can, tmp, name + "_m", NECAT_CNS_READS="merged", NECAT_TRACE="2")
    assert not TRACE.search(err_m)
    cns_g, raw_g, lines = _gather(argv, wrk, can, tmp, name + "_g")
    assert len(lines) == 1 and lines[0][0] == 0 and lines[0][1] >= 3 and lines[0][2] == CHUNK_BASES, lines
    assert lines[0][3] >= 98 and lines[0][4] > 807_132           # reads are gathered for more than one chunk
    assert cns_g == cns_m and raw_g == raw_m
    _golden(name, cns_g, raw_g)


def _x9_argv():
    m = MAN["oc2cns"]["x9_l3000"]
    return ora.cns_argv(ora.cns_options(**m["options"])) + m["extra_argv"] + ["-t", "2"]


def test_one_chunk_at_the_default_bound_and_auto(project):
    """the default bound makes one chunk of this project; auto takes the merged path below 2^32 bases"""
    wrk, can, tmp = project
    cns_g, raw_g, lines = _gather(_x9_argv(), wrk, can, tmp, "one", chunk=None)
    assert [ln[1] for ln in lines] == [1] and lines[0][2] == 1 << 31 and lines[0][3:] == (98, 807_132)
    _golden("x9_l3000", cns_g, raw_g)
    cns_a, raw_a, err_a = _oc2cns(_x9_argv(), wrk, can, tmp, "auto", NECAT_TRACE="2")
    assert not TRACE.search(err_a)
    _golden("x9_l3000", cns_a, raw_a)


def test_small_memory_option(project):
    """-s 1 changes what is written (no uncorrected reads at a partition's end), not what is loaded: merged and gather agree"""
    wrk, can, tmp = project
    cns_s, raw_s, _ = _oc2cns(_x9_argv() + ["-s", "1"], wrk, can, tmp, "s1_m", NECAT_CNS_READS="merged")
    cns_g, raw_g, lines = _gather(_x9_argv() + ["-s", "1"], wrk, can, tmp, "s1_g")
    assert lines[0][1] >= 3 and (cns_g, raw_g) == (cns_s, raw_s)
    assert hashlib.md5(cns_g).hexdigest() == MAN["oc2cns"]["x9_l3000"]["cns_md5"]


def test_node_split(project):
    """-mn: node 0 of 2 has the one partition, node 1 writes nothing"""
    wrk, can, tmp = project
    cns_0, raw_0, lines = _gather(_x9_argv(), wrk, can, tmp, "n0", mn=(0, 2))
    assert lines[0][1] >= 3
    _golden("x9_l3000", cns_0, raw_0)
    cns_1, raw_1, lines = _gather(_x9_argv(), wrk, can, tmp, "n1", mn=(1, 2))
    assert lines == [] and cns_1 == b"" and raw_1 == b""


def test_two_sparse_partitions_and_the_uncorrected_reads(project):
    """the golden records thinned out and split into two partitions by template: templates without records inside a partition's id range are written whole to
    raw_out after the partition's last chunk (-s 0), a template whose reads alone pass the bound is a chunk of its own, and an empty partition is passed over -
    merged, gather through the pipeline and gather with NECAT_CNS_PIPELINE=0 write the same two files"""
    wrk, _, tmp = project
    rec = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype="<u4").reshape(-1, 7)
    keep = rec[(rec[:, 1] % 5 != 2) & ((rec[:, 1] + rec[:, 4]) % 3 != 0) & (rec[:, 1] < 40)]       # 32 templates; 2, 7 .. 37 have no records of their own
    can = os.path.join(tmp, "sparse")
    keep[keep[:, 1] < 20].tofile(can + ".p0")
    open(can + ".p1", "wb").close()
    keep[keep[:, 1] >= 20].tofile(can + ".p2")
    open(can + ".partitions", "w").write("3\n")
    argv = ora.cns_argv(ora.cns_options(min_cov=3)) + ["-t", "3"]
    cns_m, raw_m, _ = _oc2cns(argv, wrk, can, tmp, "sp_m", NECAT_CNS_READS="merged")
    assert cns_m.count(b">") > 20 and raw_m.count(b">") >= 8
    cns_g, raw_g, lines = _gather(argv, wrk, can, tmp, "sp_g", chunk=600_000)
    assert [ln[0] for ln in lines] == [0, 2] and all(ln[1] >= 3 for ln in lines), lines
    assert (cns_g, raw_g) == (cns_m, raw_m)
    cns_1, raw_1, lines = _gather(argv, wrk, can, tmp, "sp_1", chunk=1, env=dict(NECAT_CNS_PIPELINE="0"))          # every template a chunk of its own
    assert [ln[0] for ln in lines] == [0, 2] and sum(ln[1] for ln in lines) == np.unique(keep[:, 1]).shape[0]
    assert (cns_1, raw_1) == (cns_m, raw_m)


def test_gather_refuses_a_chunk_of_a_bad_record(project):
    """a record that names a read the project does not have stops the program with a message, as it does on the merged path"""
    wrk, _, tmp = project
    rec = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype="<u4").reshape(-1, 7)[:50].copy()
    rec[7, 4] = 10 ** 6
    can = os.path.join(tmp, "bad")
    rec.tofile(can + ".p0")
    open(can + ".partitions", "w").write("1\n")
    r = subprocess.run([build.OC2CNS, wrk, can, os.path.join(tmp, "bad_c"), os.path.join(tmp, "bad_r")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, NECAT_CNS_READS="gather"))
    assert r.returncode == 1 and "outside the read set" in r.stderr
    r = subprocess.run([build.OC2CNS, wrk, can, os.path.join(tmp, "bad_c"), os.path.join(tmp, "bad_r")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, NECAT_CNS_READS="neither"))
    assert r.returncode == 1 and "NECAT_CNS_READS" in r.stderr
