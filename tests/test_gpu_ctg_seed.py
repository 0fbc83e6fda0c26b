"""GPU tests of necat_ctg_seed_batch (the seeding of contig polishing) through capi: its device path (path 0: kernels of necat_amd/csrc/ctg_seed_kernels.h)
against the reference's own output in tests/golden/ctg_s/ and against its host path (path 1: necat_amd/csrc/ctg_seed.h, which tests/test_ctg_seed.py pins to the
same files) - sorted matches and candidates must be equal numbers; at the default knobs no job of the committed cases goes back to the host."""
import os

import numpy as np
import pytest

from necat_amd import capi
from tests import ctg_seed_cases as sc
from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.GOLDEN, "ctg_s")


def _upload(c, cs):
    """the case set's reads and contigs as volumes, and the call's arrays"""
    reads = c.upload_volume(*sc.volume_arrays(cs.reads))
    ctg = c.upload_volume(*sc.volume_arrays(cs.contigs))
    seg = np.zeros(len(cs.segments), dtype=capi.CTG_SEGMENT_DTYPE)
    jobs = np.zeros(cs.n_jobs(), dtype=capi.CTG_SEED_JOB_DTYPE)
    k = 0
    for i, s in enumerate(cs.segments):
        seg[i] = (s.ctg_id, s.size, s.start, k, k + len(s.jobs))
        for qid, qdir in s.jobs:
            jobs[k] = (qid, qdir); k += 1
    return reads, ctg, seg, jobs


def _both(c, reads, ctg, seg, jobs, fallback=False):
    """path 0 and path 1, with the matches and without: equal; returns path 0's result with the matches"""
    dev = c.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=0, keep_mems=1))
    host = c.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=1, keep_mems=1))
    assert host.n_fallback == 0 and (host.jobs["how"] == 2).all() and (fallback or dev.n_fallback == 0)
    assert dev.n_lds + dev.n_scratch + dev.n_fallback == jobs.shape[0] and int((dev.jobs["how"] == 2).sum()) == dev.n_fallback
    for k in range(jobs.shape[0]):
        a, b = dev.jobs[k], host.jobs[k]
        assert all(a[f] == b[f] for f in capi.CtgSeed.CANDIDATE), "job %d: device %s, host %s" % (k, a, b)
        assert (dev.mems(k) == host.mems(k)).all(), "job %d" % k
    assert dev.snapshot() == host.snapshot()
    for path in (0, 1):
        bare = c.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=path))
        assert not bare.have_mems and bare.snapshot()[:-1] == dev.snapshot()[:-1]
    print("jobs %d: %d in LDS, %d in scratch, %d on the host; largest seed list %d, match list %d; kernels %s ms, device %.2f ms, host path %.2f ms" % (
        jobs.shape[0], dev.n_lds, dev.n_scratch, dev.n_fallback, dev.max_matches, dev.max_mems, {k: round(v, 3) for k, v in dev.kernel_ms.items()}, dev.device_ms, host.host_ms))
    return dev


def _against_golden(cs, dev):
    k = 0
    for s in cs.segments:
        for can, mems in s.answers:
            j = dev.jobs[k]
            assert int(j["found"]) == can["found"], (s.name, k)
            if can["found"]:
                assert {f: int(j[f]) for f in sc.CAN_FIELDS} == can, (s.name, k)
            assert dev.mems(k).tolist() == mems.tolist(), (s.name, k)
            k += 1
    assert k == dev.jobs.shape[0]


def test_natural_case(ctx):
    cs = sc.read_answers(sc.natural(), os.path.join(GOLD, "nat.ans.bin.gz"))
    reads, ctg, seg, jobs = _upload(ctx, cs)
    assert seg["from"][1] % 32 != 0 and seg["from"][1] + seg["size"][1] == cs.contigs[0].shape[0]
    dev = _both(ctx, reads, ctg, seg, jobs)
    _against_golden(cs, dev)
    assert jobs.shape[0] == 370 and 150 <= int(dev.jobs["found"].sum()) < 300
    reads.free(); ctg.free()


def test_crafted_set(ctx):
    cs = sc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    reads, ctg, seg, jobs = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, jobs)
    _against_golden(cs, dev)
    assert jobs.shape[0] == 115 and dev.max_mems > 128
    reads.free(); ctg.free()


def _one_contig(seed):
    """several segments of one contig in one call: starts that are no multiple of 32, overlapping ranges, the last one to the contig's end"""
    rng = np.random.default_rng(seed)
    cs = sc.CaseSet()
    n = 20011
    cs.contigs = [sc._rand(rng, n)]
    for name, start, size in (("a", 33, 7000), ("b", 5001, 6100), ("c", 12345, n - 12345)):
        s = sc.Segment(name, 0, start, size)
        cs.segments.append(s)
        for err in (0.02, 0.1, 0.14):
            a = start + int(rng.integers(0, size - 3000))
            r = np.concatenate([sc._rand(rng, 17), sc._mutate(rng, cs.contigs[0][a:a + 2800], err), sc._rand(rng, 9)])
            qdir = int(rng.integers(0, 2))
            qid = cs.add_read(r, qdir)
            s.jobs += [(qid, qdir), (qid, 1 - qdir)]
        # a read that runs over the segment's end into the rest of the contig
        r = cs.contigs[0][max(0, start - 500):start + 900].copy()
        s.jobs.append((cs.add_read(r, 0), 0))
    return cs


def test_several_segments_of_one_contig(ctx):
    cs = _one_contig(5)
    reads, ctg, seg, jobs = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, jobs)
    found = dev.jobs["found"]
    assert jobs.shape[0] == 21 and int(found.sum()) >= 12
    for i, s in enumerate(cs.segments):          # the read over the segment's start: its match begins at the segment's first base, not at the contig's
        j = dev.jobs[int(seg["ovlp_end"][i]) - 1]
        assert j["found"] and j["sbeg"] == 0 and j["qbeg"] == min(500, s.start) and j["send"] == 900
    reads.free(); ctg.free()


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


def test_tiers(ctx):
    cs = sc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    reads, ctg, seg, jobs = _upload(ctx, cs)
    base = ctx.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=0, keep_mems=1))
    assert base.n_fallback == 0 and base.n_scratch == 0
    with_mems = int((base.jobs["n_mems"] > 0).sum())

    def small_lds(c):
        assert c.knob("NECAT_CTG_SEED_LDS") == "0"
        r, g, _, _ = _upload(c, cs)
        dev = _both(c, r, g, seg, jobs)
        assert dev.n_scratch == with_mems > 60 and dev.snapshot() == base.snapshot()
        r.free(); g.free()
    _with_env({"NECAT_CTG_SEED_LDS": "0"}, small_lds)

    def small_budget(c):
        r, g, _, _ = _upload(c, cs)
        dev = _both(c, r, g, seg, jobs, fallback=True)
        over = base.jobs["n_matches"] > 100
        assert dev.n_fallback == int(over.sum()) > 0 and ((dev.jobs["how"] == 2) == over).all() and dev.snapshot() == base.snapshot()
        r.free(); g.free()
    _with_env({"NECAT_CTG_SEED_BUDGET": "100"}, small_budget)
    _with_env({"NECAT_CTG_SEED_JOB_MAX": "100"}, small_budget)          # the cap on one job's seeds sends the same jobs back
    reads.free(); ctg.free()


def test_the_same_call_twice_gives_equal_bytes(ctx):
    cs = sc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    reads, ctg, seg, jobs = _upload(ctx, cs)
    a = ctx.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=0, keep_mems=1))
    b = ctx.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options(path=0, keep_mems=1))
    assert a.jobs.tobytes() == b.jobs.tobytes() and a.all_mems.tobytes() == b.all_mems.tobytes() and a.all_mems.shape[0] > 1000
    reads.free(); ctg.free()


def test_bad_arguments_are_refused(ctx):
    cs = _one_contig(6)
    reads, ctg, seg, jobs = _upload(ctx, cs)
    good = ctx.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options()).snapshot()

    def refused(seg_, jobs_, text, reads_=reads, contigs_=ctg):
        with pytest.raises(capi.NecatError) as e:
            ctx.ctg_seed_batch(reads_, 0, contigs_, seg_, jobs_, capi.ctg_seed_options())
        assert text in str(e.value), str(e.value)

    s = seg.copy(); s["size"][1] = 1 << 24
    refused(s, jobs, "2^24")
    s = seg.copy(); s["size"][1] = 14
    refused(s, jobs, "fewer than 15")
    s = seg.copy(); s["size"][2] += 1
    refused(s, jobs, "leaves its contig")
    s = seg.copy(); s["ctg_id"][0] = 1
    refused(s, jobs, "leaves its contig")
    j = jobs.copy(); j["qid"][3] = len(cs.reads)
    refused(seg, j, "names no read")
    j = jobs.copy(); j["qid"][3] = -1
    refused(seg, j, "names no read")
    j = jobs.copy(); j["qdir"][3] = 2
    refused(seg, j, "strand")
    refused(seg, jobs, "needs the contigs", contigs_=None)
    # a read of 2^30 bases (all A: the packed bytes are zero)
    n = 1 << 30
    big = ctx.upload_volume(np.zeros(n // 4, dtype=np.uint8), n, np.zeros(1, dtype=np.int64), np.array([n], dtype=np.int64))
    refused(seg[:1], np.zeros(int(seg["ovlp_end"][0]), dtype=capi.CTG_SEED_JOB_DTYPE), "2^30", reads_=big)
    big.free()
    assert ctx.ctg_seed_batch(reads, 0, ctg, seg, jobs, capi.ctg_seed_options()).snapshot() == good
    reads.free(); ctg.free()
