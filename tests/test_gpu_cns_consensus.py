"""GPU tests of necat_cns_consensus_batch (the consensus proper of oc2cns: tags -> backbone -> best path) through capi: its device path (path 0: kernels of
cns_dev_kernels.h, every score with an error bound, templates with a comparison inside the bounds recomputed by the host code) against its host path (path 1:
cns_consensus.h, which the CPU and program tests pin to the reference) of the same call - segments, `corrected` and base blobs must be equal.  In every case but
the forced fallback at most 10 % of the examined templates may come from the host, so no case passes on the host path alone."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from necat_amd import capi
from oracle import oracle_api as ora
from tests import util

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(util.GOLDEN, "cns_c", "manifest.json")))


def _opt(argv, flag, default):
    return int(argv[argv.index(flag) + 1]) if flag in argv else default


def _both(c, vol, cands, off, ext, min_cov, min_size, full=0, cap=True):
    """path 0 against path 1; returns path 0's result (freed by the caller) and the examined count"""
    dev = c.cns_consensus_batch(vol, cands, off, ext, capi.cns_consensus_options(min_cov=min_cov, min_size=min_size, full_consensus=full, path=0))
    host = c.cns_consensus_batch(vol, cands, off, ext, capi.cns_consensus_options(min_cov=min_cov, min_size=min_size, full_consensus=full, path=1))
    examined = int(np.count_nonzero(ext.templates["examined"]))
    try:
        assert host.n_device == 0 and host.n_fallback == 0
        assert host.templates["on_host"].sum() == examined
        assert dev.n_device + dev.n_fallback == examined and int(dev.templates["on_host"].sum()) == dev.n_fallback
        a, b = dev.snapshot(), host.snapshot()
        assert len(a) == len(b) == ext.templates.shape[0]
        for t, (x, y) in enumerate(zip(a, b)):
            assert x == y, "template %d: device %r, host %r" % (t, [(s[:4], len(s[4])) for s in x[1]], [(s[:4], len(s[4])) for s in y[1]])
        print("examined %d, device %d, fallback %d, chunks %d, segments %d, kernels %s" % (examined, dev.n_device, dev.n_fallback, dev.n_chunks, dev.segments.shape[0], dev.kernel_ms))
        if cap:
            assert dev.n_fallback <= 0.1 * examined
    finally:
        host.free()
    return dev, examined


# ---- the golden partition (98 templates, about 2 200 overlaps) after cns_extension_batch

@pytest.fixture(scope="module")
def golden(ctx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gcc")
    wrk = util.install_golden_volumes(MANIFEST["volumes"], tmp)
    part = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype=np.uint8)
    vol = ctx.load_merged_volumes(wrk)
    cands, off, n_all = ctx.cns_load_partition(vol, part)
    ext = {}

    def get(name):
        okw = MANIFEST["oc2cns"][name]["options"]
        key = json.dumps(okw, sort_keys=True)
        if key not in ext:
            ext[key] = ctx.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(**okw))
        return ext[key]
    yield vol, cands, off, get
    for r in ext.values():
        r.free()
    vol.free()


@pytest.mark.parametrize("name", sorted(MANIFEST["oc2cns"]))
def test_golden_device_equals_host(ctx, golden, name):
    vol, cands, off, get = golden
    m = MANIFEST["oc2cns"][name]
    min_cov = m["options"].get("min_cov", 4)
    dev, examined = _both(ctx, vol, cands, off, get(name), min_cov, _opt(m["extra_argv"], "-l", 500), _opt(m["extra_argv"], "-f", 0))
    assert examined >= 90 and dev.segments.shape[0] > 0
    dev.free()


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = capi.Context(0)          # knobs are read when a context is created
        try:
            return fn(c)
        finally:
            c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_golden_in_several_chunks(golden):
    vol, cands, off, get = golden

    def run(c):
        assert c.knob("NECAT_CNS_TAG_BUDGET") == "1500000"
        dev, examined = _both(c, vol, cands, off, get("default"), 4, 500)
        assert dev.n_chunks >= 3
        dev.free()
    _with_env({"NECAT_CNS_TAG_BUDGET": "1500000"}, run)


def test_forced_fallback_gives_the_same_output(golden):
    vol, cands, off, get = golden

    def run(c):
        dev, examined = _both(c, vol, cands, off, get("default"), 4, 500, cap=False)
        assert dev.n_fallback == examined >= 90 and dev.n_device == 0
        assert dev.n_uncertain > 0          # (comparisons inside the bounds among the reasons, not the cap on the scaled bound alone)
        dev.free()
    _with_env({"NECAT_CNS_TOL_SCALE": "10000000"}, run)


def test_intermediate_tolerance_flags_some_templates_through_comparisons(golden):
    """certain() on the device: at a scale of 1e6 the score comparisons of some templates fall inside the bounds and those of others do not (the CPU model on the
    oracle's log of this partition: 58 of 98; tests/test_cns_device_model.py has the argument).  n_uncertain counts the templates a comparison flagged, whatever else
    sent them to the host - at this scale the cap on the scaled link bound sends all of them."""
    vol, cands, off, get = golden

    def run(c):
        dev, examined = _both(c, vol, cands, off, get("default"), 4, 500, cap=False)
        print("uncertain", dev.n_uncertain)
        assert examined >= 90 and 0 < dev.n_uncertain < examined and dev.n_uncertain <= dev.n_fallback
        dev.free()
    _with_env({"NECAT_CNS_TOL_SCALE": "1000000"}, run)


def _handed_back_share(vol, cands, ext, on_host):
    """the bases of the reads the overlaps of the templates in on_host name, and the volume's"""
    qids = set()
    for t in np.flatnonzero(on_host):
        T = ext.templates[t]
        qids.update(int(q) for q in cands["qid"][ext.overlaps["cand"][int(T["ovlp_begin"]):int(T["ovlp_end"])]])
    return sum(int(vol.sizes[q]) for q in qids), int(vol.nbases)


# ---- fresh data sets

def _fresh(ctx, tmp_path, genome, coverage, seed, err, vol_size, okw, min_size):
    wrk, rs, nv = util.make_dataset(tmp_path, genome=genome, coverage=coverage, seed=seed, err=err, vol_size=vol_size)
    o = ora.options(**dict(util.FAST, job=0, binary_output=1, num_threads=4))
    rec = b""
    for v in range(nv):
        out = os.path.join(str(tmp_path), "pm_%d" % v)
        ora.pm_main(o, v, wrk, out)
        rec += open(out, "rb").read()
    part = util.pcan_single_partition(rec)
    vol = ctx.load_merged_volumes(wrk)
    cands, off, n_all = ctx.cns_load_partition(vol, np.frombuffer(part, dtype=np.uint8))
    ext = ctx.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(**okw))
    dev, examined = _both(ctx, vol, cands, off, ext, okw.get("min_cov", 4), min_size)
    n_seg = dev.segments.shape[0]
    dev.free()
    ext.free()
    vol.free()
    return examined, n_seg


def test_fresh_deep_coverage(ctx, tmp_path):
    examined, n_seg = _fresh(ctx, tmp_path, 40_000, 35.0, 91, 0.13, 500_000, {}, 500)
    assert examined > 100 and n_seg > 100


def test_fresh_sparse_coverage(ctx, tmp_path):
    """7x coverage: templates below min_cov, uncovered stretches, stretches that are too short"""
    examined, n_seg = _fresh(ctx, tmp_path, 80_000, 7.0, 77, 0.12, 300_000, dict(min_cov=3), 500)
    assert examined > 40 and n_seg > 40


# ---- crafted overlaps (capi.CraftedCnsResult)

class Craft:
    """reads, and overlaps of them with templates, made column by column"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.tmpl = [], []          # reads: code arrays; tmpl: (read id, examined, [overlap dicts])

    def template(self, size, examined=1):
        self.reads.append(self.rng.integers(0, 4, size, dtype=np.uint8))
        self.tmpl.append((len(self.reads) - 1, examined, []))
        return len(self.tmpl) - 1

    def overlap(self, t, toff, tend, err=0.1, weight=None, qdir=0, ins_at=None, shared_ins=(), mismatch_at=None, flank=7):
        """an overlap of template t's [toff, tend): random errors at rate err, plus a run of ins_at = (position, length) query bases after that target position, one
        inserted 'A' after every position of shared_ins, a mismatch at mismatch_at"""
        rng, T = self.rng, self.reads[self.tmpl[t][0]]
        cols, q = [], []
        for p in range(toff, tend):
            r = rng.random()
            if mismatch_at == p:
                cols.append(3); q.append((int(T[p]) + 1) & 3)
            elif r < err / 3 and p > toff:
                cols.append(2)
            elif r < 2 * err / 3:
                cols.append(3); q.append((int(T[p]) + 1 + int(rng.integers(0, 3))) & 3)
            else:
                cols.append(0); q.append(int(T[p]))
                if r > 1 - err / 3 and p + 1 < tend:
                    cols.append(1); q.append(int(rng.integers(0, 4)))
            if p in shared_ins:
                cols.append(1); q.append(0)
            if ins_at and ins_at[0] == p:
                cols += [1] * ins_at[1]
                q += [int(x) for x in rng.integers(0, 4, ins_at[1])]
        q = np.array(q, dtype=np.uint8)
        left, right = rng.integers(0, 4, flank, dtype=np.uint8), rng.integers(0, 4, flank + 3, dtype=np.uint8)
        strand = np.concatenate([left, q, right])
        self.reads.append(strand if not qdir else (3 - strand[::-1]).astype(np.uint8))
        self.tmpl[t][2].append(dict(qid=len(self.reads) - 1, qdir=qdir, qoff=flank, qend=flank + q.shape[0], toff=toff, tend=tend, cols=np.array(cols, dtype=np.uint8),
                                    weight=float(rng.uniform(0.7, 1.0)) if weight is None else weight))

    def build(self, ctx):
        sizes = np.array([r.shape[0] for r in self.reads], dtype=np.int64)
        offs = np.zeros(len(self.reads), dtype=np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        from necat_amd.synth import pack_2bit
        vol = ctx.upload_volume(pack_2bit(np.concatenate(self.reads)), int(sizes.sum()), offs, sizes)
        cands, ovs, cols, tm, off = [], [], [], [], [0]
        for rid, examined, ol in self.tmpl:
            b = len(ovs)
            for o in ol or [None]:          # (a template without overlaps still has a candidate: its read)
                qid = o["qid"] if o else rid
                c = np.zeros(1, dtype=capi.CANDIDATE_DTYPE)[0]
                c["qid"], c["sid"], c["qdir"], c["qsize"], c["ssize"] = qid, rid, o["qdir"] if o else 0, sizes[qid], sizes[rid]
                if o:
                    v = np.zeros(1, dtype=capi.CNS_OVERLAP_DTYPE)[0]
                    v["cand"], v["qoff"], v["qend"], v["toff"], v["tend"], v["weight"], v["ident_perc"] = len(cands), o["qoff"], o["qend"], o["toff"], o["tend"], o["weight"], 90.0
                    ovs.append(v); cols.append(o["cols"])
                cands.append(c)
            t = np.zeros(1, dtype=capi.CNS_TEMPLATE_DTYPE)[0]
            t["examined"], t["num_can"], t["num_ovlps"], t["ovlp_begin"], t["ovlp_end"] = examined, len(ol), len(ol), b, len(ovs)
            tm.append(t); off.append(len(cands))
        ext = capi.CraftedCnsResult(np.array(tm, dtype=capi.CNS_TEMPLATE_DTYPE), np.array(ovs, dtype=capi.CNS_OVERLAP_DTYPE) if ovs else np.zeros(0, capi.CNS_OVERLAP_DTYPE), cols)
        return vol, np.array(cands, dtype=capi.CANDIDATE_DTYPE), np.array(off, dtype=np.uint64), ext


def test_crafted_overlaps(ctx):
    k = Craft(5)
    # 0: insertion runs of 254 (kept) and 255 (the whole overlap is dropped), both strands, overlaps from base 0 to the last base
    t = k.template(1500)
    for i in range(7):
        k.overlap(t, 0, 1500, qdir=i & 1, ins_at=(500, 254) if i == 0 else (900, 255) if i == 1 else None)
    # 1: 70 overlaps on one template and one 200-base insertion: buckets of more than 64 and of more than 256 tags
    t = k.template(600)
    for i in range(70):
        k.overlap(t, 0, 600, qdir=i & 1, ins_at=(300, 200) if i == 3 else None)
    # 2 - 4: min_size 200, 0.85 min_size = 170.  Exact overlaps of one stretch of length L with s shared insertions give a consensus of L - 1 + s bases:
    # 170 + 30 -> 199 (not kept), 170 + 31 -> 200 (kept), 169 + 40 -> the stretch is too short to be scored
    for L, s in ((170, 30), (170, 31), (169, 40)):
        t = k.template(1000)
        for i in range(5):
            k.overlap(t, 400, 400 + L, err=0.0, weight=1.0, qdir=i & 1, shared_ins=set(range(410, 410 + s)))
    # 5: not examined; 6: examined, no overlaps; 7: ragged starts and ends, 3 000 bases
    t = k.template(800, examined=0)
    for i in range(5):
        k.overlap(t, 0, 800)
    k.template(700)
    t = k.template(3000)
    for i in range(14):
        a = int(k.rng.integers(0, 1200))
        k.overlap(t, a, int(k.rng.integers(a + 900, 3001)), qdir=i & 1)
    vol, cands, off, ext = k.build(ctx)
    dev, examined = _both(ctx, vol, cands, off, ext, 4, 200)
    snap = dev.snapshot()
    assert examined == 7 and dev.n_fallback == 0
    assert [len(s[1]) for s in snap[2:5]] == [0, 1, 0] and len(snap[3][1][0][4]) == 200 and snap[3][1][0][:2] == (400, 570)
    assert snap[5] == (0, []) and snap[6] == (1, []) and len(snap[0][1]) >= 1 and len(snap[1][1]) == 1 and len(snap[7][1]) >= 1
    dev.free()
    vol.free()


def test_crafted_exact_tie_goes_to_the_first_in_visiting_order(ctx):
    """two overlaps of equal weight that disagree at one base: equal scores with bound 0 - decided on the device, as the host decides"""
    k = Craft(9)
    t = k.template(900)
    k.overlap(t, 0, 900, err=0.0, weight=1.0, mismatch_at=450)
    k.overlap(t, 0, 900, err=0.0, weight=1.0)
    vol, cands, off, ext = k.build(ctx)
    dev, examined = _both(ctx, vol, cands, off, ext, 2, 300)
    assert examined == 1 and dev.n_fallback == 0 and int(dev.templates["on_host"][0]) == 0
    (corrected, segs), = dev.snapshot()
    assert corrected == 1 and len(segs) == 1 and len(segs[0][4]) == 899
    T = k.reads[0]
    got = np.frombuffer(segs[0][4], dtype=np.uint8)
    assert (got[:449] == T[1:450]).all() and (got[450:] == T[451:]).all()
    assert int(got[449]) == min(int(T[450]), (int(T[450]) + 1) & 3)          # A C G T order: the smaller base code is visited first
    dev.free()
    vol.free()


def test_minority_handed_back_reads_come_down_read_by_read():
    """The host form fetches the reads its templates name read by read when they are less than a quarter of the volume, and the whole volume otherwise.  On the
    golden partition no tolerance scale reaches the first branch: the first template a growing scale flags (at 4 800, on the device as in the CPU model of
    tests/test_cns_device_model.py) names 399 759 of the volume's 807 132 bases by itself.  So: crafted templates.  A link of at most two tags has the bound 0
    (link_sum, cns_dev_core.h), which no scale changes, so exact templates of two overlaps stay on the device at a scale of 1e7, where the cap on the scaled bound
    hands back every template that has a link of three tags - the two noisy templates of four overlaps.  The test states the branch condition itself, from on_host
    and the overlaps, so it cannot pass through the whole-volume branch; the output must be path 1's."""
    k = Craft(17)
    for i in range(20):
        t = k.template(900)
        k.overlap(t, 0, 900, err=0.0, weight=1.0, qdir=i & 1)
        k.overlap(t, 0, 900, err=0.0, weight=1.0, mismatch_at=300 + i)
    noisy = []
    for i in range(2):
        noisy.append(k.template(900))
        for j in range(4):
            k.overlap(noisy[-1], 0, 900, qdir=j & 1)

    def run(c):
        vol, cands, off, ext = k.build(c)
        dev, examined = _both(c, vol, cands, off, ext, 2, 300, cap=False)
        need, nbases = _handed_back_share(vol, cands, ext, dev.templates["on_host"])
        print("handed back %d of %d, their reads %d of %d bases" % (dev.n_fallback, examined, need, nbases))
        assert examined == 22 and 0 < dev.n_fallback < examined
        assert np.flatnonzero(dev.templates["on_host"]).tolist() == noisy
        assert 0 < need and need * 4 < nbases
        assert dev.segments.shape[0] >= 20          # (every exact template gives its stretch)
        dev.free()
        vol.free()
    _with_env({"NECAT_CNS_TOL_SCALE": "10000000"}, run)


# ---- the program

def _oc2cns(built, env, argv, wrk, can, tmp, tag):
    built.build_cli()
    co, ro = os.path.join(tmp, "cns_" + tag), os.path.join(tmp, "raw_" + tag)
    r = subprocess.run([built.OC2CNS] + argv + [wrk, can, co, ro], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return open(co, "rb").read(), open(ro, "rb").read(), r.stderr


@pytest.mark.parametrize("device", ["1", "0"])
def test_oc2cns_program_on_either_path(built, tmp_path, device):
    m = MANIFEST["oc2cns"]["default"]
    wrk = util.install_golden_volumes("vols_c", tmp_path)
    can = os.path.join(str(tmp_path), "cands")
    for fn in ("cands.p0", "cands.partitions"):
        shutil.copy(os.path.join(util.GOLDEN, "cns_c", fn), os.path.join(str(tmp_path), fn))
    cns, raw, err = _oc2cns(built, {"NECAT_CNS_DEVICE": device, "NECAT_TRACE": "2"}, ora.cns_argv(ora.cns_options(**m["options"])) + m["extra_argv"] + ["-t", "3"], wrk, can,
                            str(tmp_path), "d" + device)
    assert hashlib.md5(cns).hexdigest() == m["cns_md5"] and hashlib.md5(raw).hexdigest() == m["raw_md5"]
    line = re.search(r"\[oc2cns\] partition 0: consensus proper of (\d+) templates on the device, (\d+) on the host", err)
    assert line, err
    n_dev, n_host = int(line.group(1)), int(line.group(2))
    assert (n_dev >= 88 and n_host <= 9) if device == "1" else (n_dev == 0 and n_host >= 90)


def test_oc2cns_program_device_path_beside_the_producer(built, tmp_path):
    """two partitions, so the partition pipeline runs: the consensus proper on a context of its own, on a volume uploaded through the producer's context, while the
    producer runs the next partition's extension loop.  Device path and host path must write the same two files, and the corrected reads are the manifest's."""
    m = MANIFEST["oc2cns"]["default"]
    wrk = util.install_golden_volumes("vols_c", tmp_path)
    can = os.path.join(str(tmp_path), "cands")
    rec = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype=np.uint32).reshape(-1, 7)
    cut = int(rec[:, 1].max()) // 2 + 1          # (records are in template order; a partition is a range of template ids)
    rec[rec[:, 1] < cut].tofile(can + ".p0")
    rec[rec[:, 1] >= cut].tofile(can + ".p1")
    open(can + ".partitions", "w").write("2\n")
    argv = ora.cns_argv(ora.cns_options(**m["options"])) + m["extra_argv"] + ["-t", "3"]
    out = {}
    for device in ("1", "0"):
        cns, raw, err = _oc2cns(built, {"NECAT_CNS_DEVICE": device, "NECAT_TRACE": "2"}, argv, wrk, can, str(tmp_path), "p" + device)
        lines = re.findall(r"\[oc2cns\] partition (\d): consensus proper of (\d+) templates on the device, (\d+) on the host", err)
        assert [l[0] for l in lines] == ["0", "1"], err
        n_dev, n_host = sum(int(l[1]) for l in lines), sum(int(l[2]) for l in lines)
        assert (n_dev >= 88 and n_host <= 9) if device == "1" else (n_dev == 0 and n_host >= 90)
        out[device] = (cns, raw)
    assert out["1"] == out["0"]
    assert hashlib.md5(out["1"][0]).hexdigest() == m["cns_md5"]
