"""GPU tests of necat_ctg_consensus_batch (the consensus half of contig polishing) through capi: its device path (path 0: kernels of
necat_amd/csrc/ctg_dev_kernels.h, the score pass on the host) against the reference's own output in tests/golden/ctg_g/ and against its host path (path 1:
necat_amd/csrc/ctg_consensus.h, which tests/test_ctg_consensus.py pins to the same files) - cns, t_pos and the polished segment must be equal bytes, and the
device path has no fallback: n_fallback is 0 everywhere."""
import os

import numpy as np
import pytest

from necat_amd import capi
from tests import ctg_cases as cc
from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.GOLDEN, "ctg_g")


def _upload(ctx, cs, contigs=True):
    """the case set's reads as a volume, its cases' raw segments as a volume of contigs, and the call's arrays: every case one segment"""
    reads = ctx.upload_volume(*cc.volume_arrays(cs))
    ctg = None
    if contigs:
        from necat_amd import synth
        sizes = np.array([c.size for c in cs.cases], dtype=np.int64)
        off = np.zeros(sizes.shape[0], dtype=np.int64)
        off[1:] = np.cumsum(sizes)[:-1]
        codes = np.concatenate([c.contig for c in cs.cases])
        ctg = ctx.upload_volume(synth.pack_2bit(codes), int(codes.shape[0]), off, sizes)
    seg = np.zeros(len(cs.cases), dtype=capi.CTG_SEGMENT_DTYPE)
    tabs, blobs, n_ov, n_ops = [], [], 0, 0
    for i, c in enumerate(cs.cases):
        tab, blob = cc.case_arrays(c)
        tab = tab.copy()
        tab["ops_off"] += n_ops
        seg[i] = (i, c.size, 0, n_ov, n_ov + tab.shape[0])
        tabs.append(tab); blobs.append(blob)
        n_ov += tab.shape[0]; n_ops += blob.shape[0]
    ovl = np.concatenate(tabs).astype(capi.CTG_OVERLAP_DTYPE) if n_ov else np.zeros(0, capi.CTG_OVERLAP_DTYPE)
    return reads, ctg, seg, ovl, np.concatenate(blobs)


def _both(c, reads, ctg, seg, ovl, ops, **kw):
    dev = c.ctg_consensus_batch(reads, 0, ctg, seg, ovl, ops, capi.ctg_consensus_options(path=0, **kw))
    host = c.ctg_consensus_batch(reads, 0, ctg, seg, ovl, ops, capi.ctg_consensus_options(path=1, **kw))
    assert dev.n_fallback == 0 and host.n_fallback == 0 and host.n_chunks == 0
    a, b = dev.snapshot(), host.snapshot()
    assert len(a) == len(b) == seg.shape[0]
    for s, (x, y) in enumerate(zip(a, b)):
        assert x == y, "segment %d: device cns %d bases, host %d" % (s, len(x[0]), len(y[0]))
    for k in ("n_tags", "n_nodes", "n_links"):
        assert (dev.segments[k] == host.segments[k]).all(), k
    print("segments %d, ranges %d, tags %d, nodes %d, links %d, plan %.2f ms, device %.2f ms %s, score %.2f ms, host path %.2f ms" % (
        seg.shape[0], dev.n_chunks, int(dev.segments["n_tags"].sum()), int(dev.segments["n_nodes"].sum()), int(dev.segments["n_links"].sum()), dev.plan_ms, dev.device_ms,
        dev.kernel_ms, dev.score_ms, host.host_ms))
    return dev


def _against_golden(cs, dev):
    for i, c in enumerate(cs.cases):
        assert dev.cns[i] == c.cns, c.name
        assert (dev.t_pos[i] == c.t_pos).all(), c.name
        if c.polished is not None:
            assert dev.polished[i] == c.polished, c.name


def test_natural_case(ctx):
    cs = cc.read_cases(os.path.join(GOLD, "nat.bin.gz"), os.path.join(GOLD, "nat.reads.bin.gz"))
    reads, ctg, seg, ovl, ops = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, ovl, ops)
    _against_golden(cs, dev)
    assert cs.cases[0].polished is not None and int(dev.segments["n_tags"][0]) > 500_000
    reads.free(); ctg.free()


def test_crafted_set(ctx):
    cs = cc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    reads, ctg, seg, ovl, ops = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, ovl, ops)
    _against_golden(cs, dev)
    assert len(cs.cases) == 8
    reads.free(); ctg.free()


def test_stop_rule_run_of_65540(ctx):
    """one run of 65 540 query bases: a bucket of 65 534 tags, and the overlap's later columns give none.  The reference cannot answer it (ctg_cases.stop_rule_case):
    the two paths against each other"""
    cs = cc.stop_rule_case(5)
    reads, ctg, seg, ovl, ops = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, ovl, ops)
    cols = int(ovl["align_size"].sum())
    assert 65534 <= int(dev.segments["n_tags"][0]) < cols - 200
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


def _sized_cases(seed):
    """segments of 1, 63, 64, 65 and 3000 bases in one call, the one of 64 without overlaps"""
    rng = np.random.default_rng(seed)
    cs = cc.CaseSet()
    for size in (1, 63, 64, 65, 3000):
        truth, contig = cc._contig(rng, size)
        c = cc.Case("size_%d" % size, contig)
        cs.cases.append(c)
        if size == 64:
            continue
        rg = [(0, size)] * 4 + [(int(rng.integers(0, size)), size) for _ in range(3)] + ([(100, 2900), (0, 1500), (1400, 3000)] if size == 3000 else [])
        cc._cover(cs, c, rng, truth, [r for r in rg if r[1] > r[0]], 0.1 if size > 1 else 0.0)
    return cs


def test_several_segments_and_a_small_budget(ctx):
    cs = _sized_cases(77)
    reads, ctg, seg, ovl, ops = _upload(ctx, cs)
    dev = _both(ctx, reads, ctg, seg, ovl, ops, min_run=200)
    assert [int(x) for x in dev.segments["n_chunks"]] == [1, 1, 0, 1, 1] and dev.cns[2] == b"" and len(dev.polished[2]) == 64
    assert len(dev.cns[4]) > 2500 and dev.polished[4] != cc.LUT[cs.cases[4].contig].tobytes()
    budget = int(dev.segments["n_tags"][4]) // 6

    def run(c):
        assert c.knob("NECAT_CNS_TAG_BUDGET") == str(budget)
        small = _both(c, reads, ctg, seg, ovl, ops, min_run=200)
        assert int(small.segments["n_chunks"][4]) >= 4
        assert small.snapshot() == dev.snapshot()
    _with_env({"NECAT_CNS_TAG_BUDGET": str(budget)}, run)
    reads.free(); ctg.free()


def test_bad_arguments_are_refused(ctx):
    cs = _sized_cases(78)
    reads, ctg, seg, ovl, ops = _upload(ctx, cs)
    good = ctx.ctg_consensus_batch(reads, 0, ctg, seg, ovl, ops, capi.ctg_consensus_options()).snapshot()

    def refused(seg_, ovl_, ops_, text):
        with pytest.raises(capi.NecatError) as e:
            ctx.ctg_consensus_batch(reads, 0, ctg, seg_, ovl_, ops_, capi.ctg_consensus_options())
        assert text in str(e.value), str(e.value)

    k = int(seg["ovlp_begin"][4])
    o = ovl.copy(); o["tend"][k] -= 1
    refused(seg, o, ops, "do not add up")
    o = ovl.copy(); o["qend"][k] -= 1
    refused(seg, o, ops, "do not add up")
    o = ovl.copy(); o["toff"][k] += 1; o["tend"][k] += 1          # (the overlap reaches the segment's end: now past it)
    refused(seg, o, ops, "leaves its segment")
    o = ovl.copy(); o["qoff"][k] -= 10_000; o["qend"][k] -= 10_000
    refused(seg, o, ops, "leaves its read")
    o = ovl.copy(); o["qend"][k] += 100_000
    refused(seg, o, ops, "leaves its read")
    # a query base in front of the segment's first base: the first column of an overlap from 0 (a match or a mismatch) made a query base over '-'
    k0 = next(x for x in range(k, int(seg["ovlp_end"][4])) if ovl["toff"][x] == 0 and (int(ops[int(ovl["ops_off"][x])]) & 3) in (0, 3))
    p = ops.copy(); p[int(ovl["ops_off"][k0])] = (p[int(ovl["ops_off"][k0])] & 0xfc) | 1
    o = ovl.copy(); o["tend"][k0] -= 1
    refused(seg, o, p, "leaves its segment")
    s = seg.copy(); s["size"][4] = 1 << 24
    refused(s, ovl, ops, "2^24")
    again = ctx.ctg_consensus_batch(reads, 0, ctg, seg, ovl, ops, capi.ctg_consensus_options()).snapshot()
    assert again == good
    reads.free(); ctg.free()
