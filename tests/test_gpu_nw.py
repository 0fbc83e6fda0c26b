"""GPU tests of necat_nw_path_batch (edlib_go, the rescue pair's global alignment with its path, on the device) through the C ABI: every field and
every column EQUAL to what the reference returned (tests/golden/nw_cases.json on the shapes of tests/nw_cases.py, tests/golden/rescue_cases.json on
its 60 read pairs) and, on random read pairs outside the goldens, to rescue::EdlibGo through tests/host_core/rescue_capi.cpp; no job handed to the
host code, no self-check failure."""
import json
import os
import subprocess
import ctypes as C

import numpy as np
import pytest

from necat_amd import capi
from oracle import oracle_api as ora
from tests import nw_cases, util

pytestmark = pytest.mark.gpu

READ0, REF0 = nw_cases.READ0, nw_cases.REF0          # the volumes' first global ids
pack, run_cases, hashed, golden_of = nw_cases.pack, nw_cases.run_cases, nw_cases.hashed, nw_cases.golden_of          # (shared with tests/test_gpu_high_offsets.py)


@pytest.fixture(scope="module")
def mine_lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("nw_host")), "librescue_mine.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "host_core", "rescue_capi.cpp")], check=True)
    return C.CDLL(so)


def test_shapes_equal_the_reference(ctx):
    """word and stripe boundaries of rows and columns, the leaf limit from both sides, a split with one word of rows, every reject rule on either
    side of its threshold, unrelated sequences, no run of 4 matches, the read's reverse strand - one batch per (error, min_size)"""
    cases = nw_cases.shape_cases()
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "nw_cases.json")))["cases"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = run_cases(ctx, cases)
    for c, r in zip(cases, got):
        assert ora.fnv64(bytes(c["read"])) == g[c["name"]]["read_fnv"] and ora.fnv64(bytes(c["tmpl"])) == g[c["name"]]["tmpl_fnv"], c["name"]
        assert hashed(r) == golden_of(g[c["name"]]), c["name"]
    assert sum(st.n_splits for st in stats) >= 5 and sum(st.n_leaves for st in stats) > len(cases)


def test_rescue_golden_equal_the_reference_in_one_batch(ctx):
    """the 60 read pairs of tests/golden/rescue_cases.json (3 - 9 kb every fourth: nested splits, tolerances up to 0.6 x the span) and the ten
    edge cases of tests/test_rescue.py, mixed in one call per (error, min_size)"""
    cases = nw_cases.golden_rescue_cases()
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["edlib_go"]}
    edges = nw_cases.edge_cases()
    got, stats = run_cases(ctx, cases + edges)
    n_ok = 0
    for c, r in zip(cases, got):
        assert hashed(r) == golden_of(g[c["name"]]), c["name"]
        n_ok += r[0]
    assert n_ok > 15
    assert [r[0] for r in got[len(cases):]] == [1, 1, 0, 1, 1, 0, 1, 1, 0, 1]
    assert max(st.n_levels for st in stats) >= 3 and sum(st.n_splits for st in stats) > 20


def test_random_pairs_equal_the_host_code(ctx, mine_lib):
    cases = nw_cases.seed_cases(range(7000, 7080)) + nw_cases.edge_cases()
    got, _ = run_cases(ctx, cases)
    n_ok = 0
    for c, r in zip(cases, got):
        assert r == nw_cases.host_result(mine_lib, c), c["name"]
        n_ok += r[0]
    assert n_ok > 30


def test_smallest_pool_runs_the_leaves_in_chunks(mine_lib):
    """NECAT_NW_POOL_MB=1: the leaves' flags go through a 1 MB arena in several launches - the same answers"""
    cases = [c for c in nw_cases.shape_cases() if c["name"] in ("split_1784", "qdir1_split", "two_stripes", "leaf_1783")] + nw_cases.seed_cases(range(7003, 7012)) + \
        nw_cases.golden_rescue_cases()[3:28:4]
    old = os.environ.get("NECAT_NW_POOL_MB")
    os.environ["NECAT_NW_POOL_MB"] = "1"
    try:
        c1 = capi.Context(0)          # knobs are read when a context is created
        got, stats = run_cases(c1, cases)
        c1.close()
    finally:
        if old is None:
            os.environ.pop("NECAT_NW_POOL_MB", None)
        else:
            os.environ["NECAT_NW_POOL_MB"] = old
    assert max(st.n_leaf_chunks for st in stats) >= 3 and all(st.n_leaf_chunks >= 1 for st in stats)
    for c, r in zip(cases, got):
        assert r == nw_cases.host_result(mine_lib, c), c["name"]


def test_argument_errors(ctx):
    cases = nw_cases.shape_cases()[:2]
    reads, ref = pack(ctx, [c["read"] for c in cases]), pack(ctx, [c["tmpl"] for c in cases])
    ok = (READ0, 0, 0, 1, REF0, 0, 300, 400)
    for bad in ((READ0 + 2, 0, 0, 1, REF0, 0, 300, 400), (READ0, 2, 0, 1, REF0, 0, 300, 400), (READ0, 0, 0, 2, REF0, 0, 300, 400), (READ0, 0, 0, 1, REF0, 5, 301, 400)):
        with pytest.raises(capi.NecatError):
            ctx.nw_path_batch(ref, reads, READ0, REF0, np.array([ok, bad], dtype=capi.NW_JOB_DTYPE), error=0.5, min_align_size=100)
    with pytest.raises(capi.NecatError):
        ctx.nw_path_batch(ref, reads, READ0, REF0, np.array([ok], dtype=capi.NW_JOB_DTYPE), match_size=0)
    res, ops, off, st = ctx.nw_path_batch(ref, reads, READ0, REF0, np.zeros(0, dtype=capi.NW_JOB_DTYPE))
    assert res.shape[0] == 0 and off.tolist() == [0] and st.n_device == 0
    reads.free(); ref.free()


# ---- oc2cns -r 1: the device path behind NECAT_NW_DEVICE ----

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


def test_cns_rescue_device_equals_host(built, tmp_path):
    """the long-indel partition through necat_cns_extension_batch with rescue_long_indels = 1, once with the global half of the rescue pair on the
    device (NECAT_NW_DEVICE=1) and once on the host threads (=0): the same log text - and the reference driver's -r 1 log where oracle/_ref is there -
    more than 150 rescued alignments in both, every DALIGNER survivor decided on the device in the first and none in the second; then the oc2cns
    program with -r 1 writes the same two files under both settings"""
    wrk, can, part = util.make_long_indel_partition(tmp_path)

    def run():
        c = capi.Context(0)
        vol = c.load_merged_volumes(wrk)
        cands, off, n_all = c.cns_load_partition(vol, np.frombuffer(part, dtype=np.uint8))
        res = c.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(rescue_long_indels=1))
        roff = np.zeros(len(vol.names) + 1, dtype=np.int64)
        roff[1:] = np.cumsum(vol.sizes)
        txt = util.cns_log_text(res, cands, off, vol.codes, roff, ora.fnv64, full=True)
        counts = dict(tried=res.n_rescue_tried, rescued=res.n_rescued, nw=res.n_rescue_nw, dev=res.n_rescue_nw_device, back=res.n_rescue_nw_host)
        res.free(); vol.free(); c.close()
        return txt, counts

    txt1, n1 = _under({"NECAT_NW_DEVICE": "1"}, run)
    txt0, n0 = _under({"NECAT_NW_DEVICE": "0"}, run)
    assert n1["rescued"] > 150 and n0["rescued"] > 150
    assert n1["dev"] == n1["nw"] and n1["nw"] >= n1["rescued"] and n1["back"] == 0
    assert n0["dev"] == 0 and n0["back"] == 0 and (n0["tried"], n0["nw"], n0["rescued"]) == (n1["tried"], n1["nw"], n1["rescued"])
    assert txt1 == txt0
    if ora.have_ref_cns():
        want = os.path.join(str(tmp_path), "ref_r1.txt")
        subprocess.run([ora.REF_CNS] + ora.cns_argv(ora.cns_options()) + ["-r", "1", wrk, can, want, "full"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert txt1 == open(want).read()
    built.build_cli()
    files = {}
    for dev in ("1", "0"):
        oc, orw = os.path.join(str(tmp_path), "cns_" + dev), os.path.join(str(tmp_path), "raw_" + dev)
        r = subprocess.run([built.OC2CNS] + ora.cns_argv(ora.cns_options()) + ["-r", "1", "-t", "3", wrk, can, oc, orw], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(os.environ, NECAT_NW_DEVICE=dev))
        assert r.returncode == 0, r.stdout.decode()
        files[dev] = (open(oc, "rb").read(), open(orw, "rb").read())
    assert files["1"] == files["0"] and files["1"][0].count(b">") > 40
