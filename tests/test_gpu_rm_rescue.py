"""GPU parity of necat_map_reference's speculative rescue pass (NECAT_RM_RESCUE_DEVICE=1: the rescue pair ahead of the walk through the kernels of
necat_local_align_batch and necat_nw_path_batch, the walk on the host threads reading a table; stage_refmap.inl): the oc2rm_worker program under the knob against the
committed vectors and the REFERENCE's own oc2rm_worker -t 1 (oracle/_ref), necat_map_reference through the C ABI against a context made with the knob at 0, what
necat_get_rm_stats_sized reports, the fallback tier at a small DALIGNER capacity, and the -mn volume split."""
import json
import os
import subprocess

import numpy as np
import pytest

from necat_amd import build, capi
from oracle import oracle_api as ora
from tests import util

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not os.path.exists(ora.REF_RM), reason="needs oracle/_ref/oc2rm_worker")
KNOB = "NECAT_RM_RESCUE_DEVICE"


def _under(knobs, fn):
    """fn() with the environment extended by `knobs` (a context made inside reads them)"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ref(args, wrk, ref, out):
    subprocess.run([ora.REF_RM] + args + ["-t", "1", wrk, ref, out], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return open(out, "rb").read()


def _mine(built, args, wrk, ref, out, mn=None, knobs=None):
    built.build_cli()
    r = subprocess.run([build.OC2RM] + args + ["-t", "4", wrk, ref, out] + (["-mn", str(mn[0]), str(mn[1])] if mn else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **({KNOB: "1"} if knobs is None else knobs)))
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """util.make_rm_dataset, every (seed, repeat_frac) made once"""
    made = {}

    def get(seed, repeat):
        if (seed, repeat) not in made:
            made[(seed, repeat)] = util.make_rm_dataset(tmp_path_factory.mktemp("rm_%d" % seed), seed=seed, repeat_frac=repeat)
        return made[(seed, repeat)]
    return get


def test_program_golden_under_the_knob(built, tmp_path):
    """the committed vectors: tests/golden/rm_e/ref.m4 = what the reference's oc2rm_worker wrote for tests/golden/vols_e against rm_e/ref.vol"""
    m = json.load(open(os.path.join(util.GOLDEN, "manifest_asm_rm.json")))["rm_e"]
    wrk = util.install_golden_volumes(m["volumes"], tmp_path)
    got = _mine(built, m["args"].split(), wrk, os.path.join(util.GOLDEN, "rm_e", "ref.vol"), os.path.join(str(tmp_path), "mine.m4"))
    assert got == open(os.path.join(util.GOLDEN, "rm_e", "ref.m4"), "rb").read()


@needs_ref
@pytest.mark.parametrize("seed,repeat,args", [
    (13, 0.6, "-k 13 -i 0"),
    (12, 0.4, "-k 12 -z 10 -n 8 -a 1000"),          # names as ids (the default)
    (17, 0.2, "-k 13 -b 2000 -e 0.3 -u 1"),         # binary records
])
def test_program_reproduces_reference_under_the_knob(built, dataset, tmp_path, seed, repeat, args):
    wrk, ref, nv = dataset(seed, repeat)
    want = _ref(args.split(), wrk, ref, os.path.join(str(tmp_path), "ref.m4"))
    got = _mine(built, args.split(), wrk, ref, os.path.join(str(tmp_path), "mine.m4"))
    assert len(want) > 5000
    if "-u 1" in args:          # 96-byte records: the reference writes whatever its stack held into the 4 padding bytes
        a, b = np.frombuffer(got, dtype=capi.M4_DTYPE), np.frombuffer(want, dtype=capi.M4_DTYPE)
        assert a.shape == b.shape
        for f in capi.M4_DTYPE.names:
            if not f.startswith("_"):
                assert (a[f] == b[f]).all(), f
    else:
        assert got == want


@pytest.fixture(scope="module")
def abi(built, dataset):
    """necat_map_reference volume by volume on the seed-21 set in a context made under `knobs`: (records per volume as bytes, rescued per volume, RmStats per volume); every
    set of knobs runs once"""
    done = {}

    def run(**knobs):
        key = tuple(sorted(knobs.items()))
        if key in done:
            return done[key]
        wrk, ref, nv = dataset(21, 0.5)
        assert nv >= 3
        c = _under(knobs, lambda: capi.Context(0))
        try:
            for k, v in knobs.items():
                assert c.knob(k) == v
            nvol, nreads, vols = capi.load_volumes_info(wrk)
            opt = capi.default_options(kmer_size=13, scan_window=5, kmer_cnt_cutoff=500, block_size=1000, block_score_cutoff=3, num_candidates=20,
                                       align_size_cutoff=400, ddfs_cutoff=0.25, error=0.5, num_output=20, job=1)
            rv = c.load_volume(ref)
            ix = c.build_index(rv, 13, 500)
            recs, rescued, stats = [], [], []
            for path, start, _ in vols:
                v = c.load_volume(path)
                m4, ncand, nresc = c.map_reference(ix, rv, v, int(start), 0, opt)
                st = c.rm_stats()
                assert st.n_candidates == ncand and st.n_rescued == nresc
                recs.append(m4.tobytes()); rescued.append(nresc); stats.append(st)
                v.free()
            ix.free()
            rv.free()
        finally:
            c.close()
        done[key] = (recs, rescued, stats)
        return done[key]
    return run


def _sum(stats, field):
    return sum(getattr(s, field) for s in stats)


def test_abi_parity_and_stats(abi):
    recs0, resc0, st0 = abi(**{KNOB: "0"})
    recs1, resc1, st1 = abi(**{KNOB: "1"})
    assert recs1 == recs0 and sum(len(r) for r in recs0) > 96 * 1000
    assert sum(resc1) == sum(resc0) > 5
    for s0, s1 in zip(st0, st1):
        print({f: getattr(s1, f) for f, _ in capi.RmStats._fields_})
        assert (s1.n_candidates, s1.n_need, s1.n_tried, s1.n_rescued) == (s0.n_candidates, s0.n_need, s0.n_tried, s0.n_rescued)
        assert s1.words_fetched == 0
        assert s1.n_dalign_device + s1.n_dalign_host == s1.n_need
        assert s1.n_dalign_host == s1.n_dalign_over_cap + s1.n_dalign_selfcheck
        assert s1.n_nw_device + s1.n_nw_host == s1.n_nw_jobs <= s1.n_need
        assert s1.n_nw_host == 0          # a self-check failure is a bug indicator
        assert 0 < s1.n_tried <= s1.n_need <= 1.25 * s1.n_tried          # (the reference's own walk: at most 1.07; the cap only catches a job list that forgot a filter)
        assert s1.n_rescued <= s1.n_nw_jobs
        assert s1.max_diags <= 512 and (s1.max_diags >= 1) == (s1.n_need > 0)
        # the knob at 0: nothing on the device, the words come to the host whenever a pair can be needed
        assert s0.n_dalign_device == s0.n_dalign_host == s0.n_nw_jobs == s0.n_nw_device == s0.n_nw_host == 0 and s0.max_diags == 0 and s0.dalign_ms == 0 and s0.nw_ms == 0
        assert s0.words_fetched == (1 if s0.n_need else 0)
    assert (_sum(st1, "n_need"), _sum(st1, "n_tried")) == (90, 87)          # what rm_host.h's sequential walk gives on this set (tests/test_rm_rescue_model.py)


def test_fallback_tier_at_a_small_capacity(abi):
    """16 diagonals: the jobs whose window outgrows them are recomputed by the host code on the slices, for which the words are fetched; the records do not change"""
    recs0, resc0, st0 = abi(**{KNOB: "0"})
    recs1, resc1, st1 = abi(**{KNOB: "1", "NECAT_DALIGN_DIAGS": "16"})
    assert recs1 == recs0 and sum(resc1) == sum(resc0)
    assert _sum(st1, "n_dalign_over_cap") > 0 and _sum(st1, "n_nw_host") == 0
    for s, s0 in zip(st1, st0):
        assert (s.n_candidates, s.n_need, s.n_tried, s.n_rescued) == (s0.n_candidates, s0.n_need, s0.n_tried, s0.n_rescued)
        assert s.words_fetched == (1 if s.n_dalign_host else 0)
        assert s.n_dalign_device + s.n_dalign_host == s.n_need and s.max_diags <= 18
        assert s.n_dalign_host == s.n_dalign_over_cap + s.n_dalign_selfcheck
        assert s.n_nw_device + s.n_nw_host == s.n_nw_jobs <= s.n_need and s.n_nw_host == 0
        assert 0 < s.n_tried <= s.n_need <= 1.25 * s.n_tried
    assert any(s.words_fetched for s in st1)


def test_node_split_under_the_knob(built, dataset, tmp_path):
    wrk, ref, nv = dataset(21, 0.5)
    args = "-k 13 -i 0".split()
    parts = [_mine(built, args, wrk, ref, os.path.join(str(tmp_path), "mine_%d.m4" % node), mn=(node, 2)) for node in range(2)]
    whole = _mine(built, args, wrk, ref, os.path.join(str(tmp_path), "mine_all.m4"))
    assert all(len(p) > 1000 for p in parts)
    assert sorted((parts[0] + parts[1]).splitlines()) == sorted(whole.splitlines())
    assert whole == _mine(built, args, wrk, ref, os.path.join(str(tmp_path), "mine_host.m4"), knobs={KNOB: "0"})
