"""GPU tests of necat_ctg_extend_batch (the aligner and the coverage cap of contig polishing) through capi, against the reference's own log in tests/golden/ctg_x
(tests/ctg_ext_cases.py; tests/test_ctg_extend.py pins the serial pass to the same files on the CPU): per record the verdict, who decided, coordinates, align_size
and ident_perc as equal numbers, the overlaps in loop order with equal columns; the rescue pair on the device and on the host threads; the seeds given and made by
the entry; the chain seeds -> extend -> consensus against the reference program's polished contig."""
import ctypes as C
import os

import numpy as np
import pytest

from necat_amd import capi
from tests import ctg_ext_cases as xc
from tests import ctg_seed_cases as sc

pytestmark = pytest.mark.gpu

FIELDS = ("qoff", "qend", "toff", "tend", "align_size")


@pytest.fixture(scope="module")
def crafted():
    cs = xc.load_crafted()
    for s, g in zip(cs.segments, xc.crafted().segments):          # (what each record is there for lives in the generator)
        assert s.records == g.records
        s.tags = g.tags
    return cs


@pytest.fixture(scope="module")
def natural():
    return xc.load_natural()


def _arrays(cs, segments=None):
    """the call's arrays for `segments` of cs (default: all, in order), every segment with jobs of its own; (seg, jobs, seed jobs, [(segment, first job)])"""
    segments = list(cs.segments) if segments is None else segments
    seg = np.zeros(len(segments), dtype=capi.CTG_SEGMENT_DTYPE)
    jobs = np.zeros(sum(len(s.records) for s in segments), dtype=capi.CTG_EXTEND_JOB_DTYPE)
    k, where = 0, []
    for i, s in enumerate(segments):
        seg[i] = (s.ctg_id, s.size, s.start, k, k + len(s.records))
        where.append((s, k))
        for r in s.records:
            jobs[k] = r; k += 1
    sj = np.zeros(jobs.shape[0], dtype=capi.CTG_SEED_JOB_DTYPE)
    sj["qid"], sj["qdir"] = jobs["qid"], jobs["qdir"]
    return seg, jobs, sj, where


def _upload(c, cs):
    return c.upload_volume(*sc.volume_arrays(cs.reads)), c.upload_volume(*sc.volume_arrays(cs.contigs))


def _strings(cs, s, a, ops):
    """the gapped strings the reference logged for an alignment of segment s, from the golden's columns and the bases"""
    q, t = cs.read_on_strand(int(a["qid"]), int(a["qdir"])), cs.segment_codes(s)
    qa = np.full(ops.shape[0], ord("-"), dtype=np.uint8)
    ta = np.full(ops.shape[0], ord("-"), dtype=np.uint8)
    qa[ops != 2] = xc.LUT[q[int(a["qoff"]):int(a["qend"])]]
    ta[ops != 1] = xc.LUT[t[int(a["toff"]):int(a["tend"])]]
    return qa.tobytes(), ta.tobytes()


def _against_golden(cs, res, where, cap):
    """every job and every overlap of `res` against the reference's log"""
    n_ov = 0
    for i, (s, k0) in enumerate(where):
        states = xc.expected_states(cs, s, cap)
        want_order = [k for k in np.argsort([a["order"] for a in s.ans], kind="stable") if s.ans[k]["order"] >= 0] if cap else [k for k, st in enumerate(states) if st == xc.ACCEPTED]
        lo, hi = int(res.segments["ovlp_begin"][i]), int(res.segments["ovlp_end"][i])
        assert lo == n_ov and hi - lo == len(want_order), (s.name, lo, hi, len(want_order))
        assert tuple(res.segments[i][f] for f in ("ctg_id", "size", "from")) == (s.ctg_id, s.size, s.start)
        for k, a in enumerate(s.ans):
            j = res.jobs[k0 + k]
            assert int(j["state"]) == states[k], (s.name, k, s.tags.get(k), j, a)
            if states[k] in (xc.CAPPED, xc.NO_SEED, xc.NO_ALIGNMENT):
                assert all(int(j[f]) == 0 for f in FIELDS) and j["ident_perc"] == 0.0 and j["overlap"] == -1 and (states[k] == xc.NO_ALIGNMENT or j["decided"] == 0), (s.name, k, j)
                continue
            assert {f: int(j[f]) for f in FIELDS} == {f: int(a[f]) for f in FIELDS}, (s.name, k, j, a)
            assert float(j["ident_perc"]) == float(a["ident"]), (s.name, k, float(j["ident_perc"]), float(a["ident"]))          # equal as doubles
            assert int(j["decided"]) == xc.expected_decided(a), (s.name, k, j)
            assert (int(j["overlap"]) >= 0) == (states[k] == xc.ACCEPTED)
        for x, k in enumerate(want_order):
            a, o = s.ans[k], res.overlaps[lo + x]
            assert int(res.jobs[k0 + k]["overlap"]) == lo + x
            assert (int(o["qid"]), int(o["qdir"])) + tuple(int(o[f]) for f in FIELDS) == (int(a["qid"]), int(a["qdir"])) + tuple(int(a[f]) for f in FIELDS), (s.name, k)
            cols = res.columns(lo + x)
            assert cols.shape == s.ops[k].shape and (cols == s.ops[k]).all(), (s.name, k)
            assert int(o["ops_off"]) % 8 == 0
        n_ov = hi
    assert n_ov == res.overlaps.shape[0]


def _counters(cs, where, cap):
    n_used = sum(st in (xc.NO_ALIGNMENT, xc.REJECTED, xc.ACCEPTED) for s, _ in where for st in xc.expected_states(cs, s, cap))
    seeded = sum(int(a["found"]) for s, _ in where for a in s.ans)
    tried = sum(int(a["dal_run"]) >= 0 for s, _ in where for a in s.ans)
    won = sum(int(a["edl_run"]) == 1 for s, _ in where for a in s.ans)
    return n_used, seeded, tried, won


@pytest.mark.parametrize("rescue_path", [0, 1])
@pytest.mark.parametrize("given", [True, False], ids=["seeds_given", "seeds_made"])
def test_crafted_set(ctx, crafted, rescue_path, given):
    cs = crafted
    reads, ctg = _upload(ctx, cs)
    seg, jobs, sj, where = _arrays(cs)
    seeds = ctx.ctg_seed_batch(reads, 0, ctg, seg, sj, capi.ctg_seed_options()) if given else None
    res = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, seeds, capi.ctg_extend_options(rescue_path=rescue_path))
    _against_golden(cs, res, where, True)
    n_used, seeded, tried, won = _counters(cs, where, True)
    assert (res.n_used, res.n_seeded, res.n_aligned, res.n_pair_tried, res.n_pair_accepted) == (n_used, seeded, seeded, tried, won) and won == 2 and tried == 3
    assert (res.ms["seed"] == 0.0) == given and res.cols_bytes_used <= res.cols_bytes_downloaded and res.cols_bytes_used == int(((res.overlaps["align_size"] + 3) // 4).sum())
    # columns through necat_gapped_strings are the strings the reference handed to add_align_tags (the golden keeps them as columns: the same expansion of those)
    by, tags, k0 = cs.by_name()["whole_20k"], cs.by_name()["whole_20k"].tags, where[0][1]
    for k in [k for k, t in tags.items() if t in ("insertion", "ident_above", "open_200")]:
        a, ov = by.ans[k], res.overlaps[int(res.jobs[k0 + k]["overlap"])]
        n = int(ov["align_size"])
        got = capi.gapped_strings(res.ops[int(ov["ops_off"]):int(ov["ops_off"]) + (n + 3) // 4], n, cs.read_on_strand(int(a["qid"]), int(a["qdir"])), int(ov["qoff"]),
                                  cs.segment_codes(by), int(ov["toff"]))
        assert got == _strings(cs, by, a, by.ops[k]) and len(got[0]) == n and got[0].count(b"-") + int(a["qend"] - a["qoff"]) == n
    if rescue_path == 0:
        # the pair is not vacuous: the insertion and the deletion case were decided by the kernels, none went back to the host code
        assert res.n_dalign_device == tried and res.n_dalign_host == 0 and res.n_dalign_selfcheck == 0 and res.n_dalign_over_cap == 0
        assert res.n_nw_jobs == won and res.n_nw_device == won and res.n_nw_host == 0
        for tag in ("insertion", "deletion"):
            k = next(k for k, t in tags.items() if t == tag)
            assert int(res.jobs[where[0][1] + k]["decided"]) == capi.CTG_EXT_BY_PAIR
    else:
        assert res.n_dalign_device == 0 and res.n_dalign_host == tried and res.n_nw_host == won
    reads.free(); ctg.free()


@pytest.mark.parametrize("rescue_path", [0, 1])
def test_natural_case(ctx, natural, rescue_path):
    cs, case = natural
    reads, ctg = _upload(ctx, cs)
    seg, jobs, sj, where = _arrays(cs)
    res = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options(rescue_path=rescue_path))
    _against_golden(cs, res, where, True)
    assert res.overlaps.shape[0] == 148 and res.n_used == 148 and res.n_aligned == 149 and int((res.jobs["state"] == capi.CTG_EXT_CAPPED).sum()) == 1
    a, o = cs.segments[0].ans, res.overlaps
    k = int(np.flatnonzero(res.jobs["overlap"] == 5)[0])
    n = int(o[5]["align_size"])
    got = capi.gapped_strings(res.ops[int(o[5]["ops_off"]):int(o[5]["ops_off"]) + (n + 3) // 4], n, cs.read_on_strand(int(a[k]["qid"]), int(a[k]["qdir"])), int(o[5]["qoff"]),
                              cs.contigs[0], int(o[5]["toff"]))
    assert got == _strings(cs, cs.segments[0], a[k], cs.segments[0].ops[k])
    reads.free(); ctg.free()


@pytest.mark.parametrize("which", ["crafted", "natural"])
def test_without_the_cap_every_record_is_reported(ctx, crafted, natural, which):
    cs = crafted if which == "crafted" else natural[0]
    reads, ctg = _upload(ctx, cs)
    seg, jobs, sj, where = _arrays(cs)
    res = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options(cap=0))
    _against_golden(cs, res, where, False)
    n_used, seeded, _, _ = _counters(cs, where, False)
    assert res.n_used == n_used == seeded == res.n_aligned and not (res.jobs["state"] == capi.CTG_EXT_CAPPED).any()
    assert res.overlaps.shape[0] == (149 if which == "natural" else 59)
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


def test_pair_fallback_tier_at_the_smallest_capacity(crafted):
    """NECAT_DALIGN_DIAGS=4, the knob's minimum: the pair's windows outgrow it, those jobs are recomputed by the host code on the segment's slice of the contig and
    come back as tips; the global half stays on the device and every record is still the reference's"""
    cs = crafted
    seg, jobs, sj, where = _arrays(cs)

    def small(c):
        assert c.knob("NECAT_DALIGN_DIAGS") == "4"
        reads, ctg = _upload(c, cs)
        res = c.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options(rescue_path=0))
        _against_golden(cs, res, where, True)
        assert res.n_dalign_over_cap > 0
        assert res.n_dalign_device + res.n_dalign_host == res.n_pair_tried
        assert res.n_nw_host == 0
        assert res.n_pair_accepted == 2
        reads.free(); ctg.free()
    _with_env({"NECAT_DALIGN_DIAGS": "4"}, small)


def test_extension_in_several_batches_gives_the_same(ctx, crafted, natural):
    """the block-wise aligner's call cut into batches of 64 candidates (NECAT_BATCH): the crafted set in two, the natural case in three - equal bytes"""
    for cs in (crafted, natural[0]):
        reads, ctg = _upload(ctx, cs)
        seg, jobs, sj, where = _arrays(cs)
        base = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options())
        reads.free(); ctg.free()

        def small(c):
            assert c.knob("NECAT_BATCH") == "64" and base.n_aligned > 64
            r, g = _upload(c, cs)
            got = c.ctg_extend_batch(r, 0, g, seg, jobs, None, capi.ctg_extend_options())
            _against_golden(cs, got, where, True)
            assert got.snapshot() == base.snapshot()
            r.free(); g.free()
        _with_env({"NECAT_BATCH": "64"}, small)


def test_the_chain_gives_the_reference_programs_polished_contig(ctx, natural):
    """seeds -> extend -> consensus, the three arrays handed on unchanged: cns, t_pos and the polished contig of the reference's ctgcns (tests/golden/ctg_g)"""
    cs, case = natural
    reads, ctg = _upload(ctx, cs)
    seg, jobs, sj, where = _arrays(cs)
    seeds = ctx.ctg_seed_batch(reads, 0, ctg, seg, sj, capi.ctg_seed_options())
    ext = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, seeds, capi.ctg_extend_options())
    for path in (0, 1):
        cns = ctx.ctg_consensus_batch(reads, 0, ctg, ext.segments, ext.overlaps, ext.ops, capi.ctg_consensus_options(path=path))
        assert cns.cns[0] == case.cns and (cns.t_pos[0] == case.t_pos).all() and cns.polished[0] == case.polished and len(case.polished) == 40019
    reads.free(); ctg.free()


def test_segments_twice_and_in_reverse_order(ctx, crafted):
    """overlapping and repeated segments in any order in one call: each copy's result is the single call's"""
    cs = crafted
    reads, ctg = _upload(ctx, cs)
    single = {}
    for s in cs.segments:
        seg, jobs, sj, where = _arrays(cs, [s])
        single[s.name] = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options())
    order = list(reversed(cs.segments)) + list(cs.segments)
    seg, jobs, sj, where = _arrays(cs, order)
    res = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options())
    _against_golden(cs, res, where, True)
    for i, (s, k0) in enumerate(where):
        one = single[s.name]
        lo, hi = int(res.segments["ovlp_begin"][i]), int(res.segments["ovlp_end"][i])
        j = res.jobs[k0:k0 + len(s.records)].copy()
        j["overlap"] = np.where(j["overlap"] >= 0, j["overlap"] - lo, -1)
        assert j.tobytes() == one.jobs.tobytes() and hi - lo == one.overlaps.shape[0]
        for x in range(hi - lo):
            assert (res.columns(lo + x) == one.columns(x)).all()
            assert all(res.overlaps[lo + x][f] == one.overlaps[x][f] for f in capi.CTG_OVERLAP_DTYPE.names if f != "ops_off")
    reads.free(); ctg.free()


def test_bad_arguments_are_refused(ctx, crafted):
    cs = crafted
    reads, ctg = _upload(ctx, cs)
    seg, jobs, sj, where = _arrays(cs)
    seeds = ctx.ctg_seed_batch(reads, 0, ctg, seg, sj, capi.ctg_seed_options())
    good = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, seeds, capi.ctg_extend_options()).snapshot()

    def refused(seg_, jobs_, text, seeds_=None, contigs_=ctg, **kw):
        with pytest.raises(capi.NecatError) as e:
            ctx.ctg_extend_batch(reads, 0, contigs_, seg_, jobs_, seeds_, capi.ctg_extend_options(**kw))
        assert text in str(e.value), str(e.value)

    k1 = int(seg["ovlp_begin"][1])          # a job of [15 000, 45 000)
    j = jobs.copy(); j["send"][k1] = 15000
    refused(seg, j, "ends at or before its segment's start")
    j = jobs.copy(); j["send"][k1] = 15001; j["soff"][k1] = 10
    assert ctx.ctg_extend_batch(reads, 0, ctg, seg, j, None, capi.ctg_extend_options()).jobs.shape[0] == jobs.shape[0]          # one base inside is a record
    j = jobs.copy(); j["qid"][3] = len(cs.reads)
    refused(seg, j, "names no read")
    j = jobs.copy(); j["qid"][3] = -1
    refused(seg, j, "names no read")
    j = jobs.copy(); j["qdir"][3] = 2
    refused(seg, j, "strand")
    s = seg.copy(); s["size"][1] = 45001
    refused(s, jobs, "leaves its contig")
    s = seg.copy(); s["ctg_id"][0] = 3
    refused(s, jobs, "leaves its contig")
    s = seg.copy(); s["size"][1] = 1 << 24
    refused(s, jobs, "2^24")
    s = seg.copy(); s["size"][3] = 14
    refused(s, jobs, "fewer than 15")
    refused(seg[:2], jobs, "the seed table holds", seeds_=seeds)          # a table over other jobs
    s = seg.copy(); s["ovlp_end"][1] += 1          # the first job of [30 000, 60 000) lies in [15 000, 45 000) too
    refused(s, jobs, "is named by segments 1 and 2")
    refused(seg, jobs, "needs the contigs", contigs_=None)
    refused(seg, jobs, "options out of range", cap=2)
    refused(seg, jobs, "options out of range", rescue_path=2)
    # *out stays NULL
    out = C.POINTER(capi._CtgExtend)()
    j = jobs.copy(); j["send"][k1] = 15000
    o = capi.ctg_extend_options()
    rc = ctx.lib.necat_ctg_extend_batch(ctx.h, reads.h, 0, ctg.h, seg.ctypes.data, seg.shape[0], j.ctypes.data, None, C.byref(o), C.byref(out))
    assert rc == -1 and not out
    assert ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, seeds, capi.ctg_extend_options()).snapshot() == good
    reads.free(); ctg.free()
