"""GPU tests of necat_local_align_batch (ocda_go, the rescue pair's local alignment around the anchor, on the device) through the C ABI: every field EQUAL
to what the reference returned (tests/golden/dalign_cases.json on the shapes of tests/dalign_cases.py, tests/golden/rescue_cases.json on its 60 read
pairs) and, on random read pairs outside the goldens, to rescue::Dalign through tests/host_core/rescue_capi.cpp; no job handed to the host code at the
default capacity, the wide ones - and only those - at a capacity of 64 diagonals; then oc2cns -r 1 with the local half on the device."""
import json
import os
import subprocess
import ctypes as C

import numpy as np
import pytest

from necat_amd import capi
from oracle import oracle_api as ora
from tests import dalign_cases, nw_cases, util

pytestmark = pytest.mark.gpu

READ0, REF0 = nw_cases.READ0, nw_cases.REF0          # the volumes' first global ids
pack, run_cases, all_on_device = nw_cases.pack, dalign_cases.run_cases, dalign_cases.all_on_device          # (shared with tests/test_gpu_high_offsets.py)


@pytest.fixture(scope="module")
def mine_lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("dalign_host")), "librescue_mine.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "host_core", "rescue_capi.cpp")], check=True)
    return C.CDLL(so)


def test_shapes_equal_the_reference(ctx):
    """anchors on the sequences' ends and on the 2-bit words' boundaries, unrelated sequences, long indels (windows above 64 diagonals: several chunks of
    lanes), sizes around min_align_size, reached ends, the trim, equal diagonals, the read's reverse strand - one batch per (error, min_size)"""
    cases = dalign_cases.shape_cases()
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "dalign_cases.json")))["cases"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = run_cases(ctx, cases)
    assert all_on_device(got, stats) and sum(st.n_device for st in stats) == len(cases)
    for c, r in zip(cases, got):
        assert ora.fnv64(bytes(c["read"])) == g[c["name"]]["read_fnv"] and ora.fnv64(bytes(c["tmpl"])) == g[c["name"]]["tmpl_fnv"], c["name"]
        assert r[:3] == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert max(st.max_diags for st in stats) > 128 and sum(st.n_steps for st in stats) > 5000


def test_rescue_golden_equal_the_reference_in_one_batch(ctx):
    """the 60 read pairs of tests/golden/rescue_cases.json's ocda_go, one call per error"""
    cases = dalign_cases.golden_rescue_cases()
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["ocda_go"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = run_cases(ctx, cases)
    assert all_on_device(got, stats)
    for c, r in zip(cases, got):
        assert r[:3] == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert sum(r[0] for r in got) > 20


def test_random_pairs_equal_the_host_code(ctx, mine_lib):
    cases = dalign_cases.seed_cases(range(9000, 9080))
    assert sum(c["qdir"] for c in cases) >= 15
    got, stats = run_cases(ctx, cases)
    assert all_on_device(got, stats)
    for c, r in zip(cases, got):
        assert r[:3] == dalign_cases.host_result(mine_lib, c), c["name"]
    assert sum(r[0] for r in got) > 30


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


def test_small_capacity_hands_the_wide_windows_back(mine_lib):
    """NECAT_DALIGN_DIAGS=64: a job whose window outgrows 64 diagonals is recomputed by the host code inside the call (how = 1) - exactly those,
    the same answers everywhere"""
    cases = dalign_cases.shape_cases() + dalign_cases.seed_cases(range(9000, 9012))

    def run():
        c1 = capi.Context(0)          # knobs are read when a context is created
        try:
            return run_cases(c1, cases)
        finally:
            c1.close()

    got, stats = _under({"NECAT_DALIGN_DIAGS": "64"}, run)
    assert sum(st.n_over_cap for st in stats) > 0 and sum(st.n_device for st in stats) > 0 and sum(st.n_selfcheck for st in stats) == 0
    assert sum(r[3] for r in got) == sum(st.n_over_cap for st in stats) == sum(st.n_host for st in stats)
    assert 64 < max(st.max_diags for st in stats) <= 66     # a job stops at the step that outgrew the capacity (a step widens the window by two)
    by = {c["name"]: r for c, r in zip(cases, got)}
    assert all(by[n][3] == 0 for n in by if n.startswith("word")) and by["deletion600"][3] == 1 and by["insertion600"][3] == 1 and by["unrelated"][3] == 1
    for c, r in zip(cases, got):
        assert r[:3] == dalign_cases.host_result(mine_lib, c), c["name"]


def test_argument_errors(ctx):
    cases = dalign_cases.shape_cases()[:2]
    reads, ref = pack(ctx, [c["read"] for c in cases]), pack(ctx, [c["tmpl"] for c in cases])
    ok = (READ0, 0, 350, REF0, 350)
    for bad in ((READ0 + 2, 0, 350, REF0, 350), (READ0 - 1, 0, 350, REF0, 350), (READ0, 0, 350, REF0 + 2, 350), (READ0, 2, 350, REF0, 350), (READ0, 0, 701, REF0, 350),
                (READ0, 0, -1, REF0, 350), (READ0, 0, 350, REF0, 701)):
        with pytest.raises(capi.NecatError):
            ctx.local_align_batch(ref, reads, READ0, REF0, np.array([ok, bad], dtype=capi.DALIGN_JOB_DTYPE), error=0.5, min_align_size=100)
    for error in (0.0, -0.5, 1.5):
        with pytest.raises(capi.NecatError):
            ctx.local_align_batch(ref, reads, READ0, REF0, np.array([ok], dtype=capi.DALIGN_JOB_DTYPE), error=error, min_align_size=100)
    res, st = ctx.local_align_batch(ref, reads, READ0, REF0, np.zeros(0, dtype=capi.DALIGN_JOB_DTYPE))
    assert res.shape[0] == 0 and st.n_device == 0 and st.n_host == 0
    res, st = ctx.local_align_batch(ref, reads, READ0, REF0, np.array([ok], dtype=capi.DALIGN_JOB_DTYPE), error=1.0, min_align_size=100)
    assert res.shape[0] == 1 and res[0]["ok"] == 1
    reads.free(); ref.free()


# ---- oc2cns -r 1: the device path behind NECAT_DALIGN_DEVICE ----

def test_cns_rescue_local_half_on_device_equals_host(built, tmp_path):
    """the long-indel partition through necat_cns_extension_batch with rescue_long_indels = 1 under NECAT_DALIGN_DEVICE x NECAT_NW_DEVICE in {1, 0} x {1, 0}:
    one log text for all four - and the reference driver's -r 1 log where oracle/_ref is there - more than 150 rescued alignments, every candidate's
    local half decided on the device when it is asked to; then the oc2cns program with -r 1 writes the same two files with both halves on the device as
    with both on the host threads"""
    wrk, can, part = util.make_long_indel_partition(tmp_path)

    def run():
        c = capi.Context(0)
        vol = c.load_merged_volumes(wrk)
        cands, off, n_all = c.cns_load_partition(vol, np.frombuffer(part, dtype=np.uint8))
        res = c.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(rescue_long_indels=1))
        roff = np.zeros(len(vol.names) + 1, dtype=np.int64)
        roff[1:] = np.cumsum(vol.sizes)
        txt = util.cns_log_text(res, cands, off, vol.codes, roff, ora.fnv64, full=True)
        counts = dict(tried=res.n_rescue_tried, rescued=res.n_rescued, nw=res.n_rescue_nw, dal_dev=res.n_rescue_dalign_device, dal_host=res.n_rescue_dalign_host)
        res.free(); vol.free(); c.close()
        return txt, counts

    runs = {(d, g): _under({"NECAT_DALIGN_DEVICE": d, "NECAT_NW_DEVICE": g}, run) for d in ("1", "0") for g in ("1", "0")}
    txt0, n0 = runs[("0", "0")]
    assert n0["rescued"] > 150 and n0["dal_dev"] == 0 and n0["dal_host"] == 0
    for (d, g), (txt, n) in runs.items():
        assert txt == txt0, (d, g)
        assert (n["tried"], n["nw"], n["rescued"]) == (n0["tried"], n0["nw"], n0["rescued"]), (d, g)
        assert (n["dal_dev"], n["dal_host"]) == ((n["tried"], 0) if d == "1" else (0, 0)), (d, g)
    if ora.have_ref_cns():
        want = os.path.join(str(tmp_path), "ref_r1.txt")
        subprocess.run([ora.REF_CNS] + ora.cns_argv(ora.cns_options()) + ["-r", "1", wrk, can, want, "full"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert txt0 == open(want).read()
    built.build_cli()
    files = {}
    for dev in ("1", "0"):
        oc, orw = os.path.join(str(tmp_path), "cns_" + dev), os.path.join(str(tmp_path), "raw_" + dev)
        r = subprocess.run([built.OC2CNS] + ora.cns_argv(ora.cns_options()) + ["-r", "1", "-t", "3", wrk, can, oc, orw], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(os.environ, NECAT_DALIGN_DEVICE=dev, NECAT_NW_DEVICE=dev))
        assert r.returncode == 0, r.stdout.decode()
        files[dev] = (open(oc, "rb").read(), open(orw, "rb").read())
    assert files["1"] == files["0"] and files["1"][0].count(b">") > 40
