"""CPU tests of the DEVICE form of edlib_go (necat_amd/csrc/nw_core.h: the per-lane cores of the kernels in nw_kernels.h and the host orchestration of
the recursion levels, built here by g++ as a model of the device path).  tests/host_core/check_nw.cpp runs the model lane by lane and compares it
with rescue::EdlibGo::go for EQUALITY of ok, coordinates, distance, identity and both gapped strings; this file feeds it
  * the 60 edlib_go cases of tests/golden/rescue_cases.json (the model's output is also held against the reference's values there),
  * the ten edge cases of tests/test_rescue.py::test_edlib_go_edges,
  * the shapes of tests/nw_cases.py (held against tests/golden/nw_cases.json, the reference's values, as well),
  * a few hundred random read pairs on both sides of the leaf limit, a fifth of them on the read's reverse strand,
and runs the shapes once more with a flag pool of 1 MB, so that the leaves go through in several chunks."""
import json
import os
import subprocess

import pytest

from tests import nw_cases, util
from oracle import oracle_api as ora

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_nw.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("nw")), "check_nw")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC], check=True)
    return exe


def write_cases(path, cases):
    with open(path, "w") as f:
        for c in cases:
            f.write("%d %d %d %d %d %d %d %.17g\n" % (c["qdir"], c["qf"], c["qt"], c["tf"], c["tt"], c["tol"], c["min_size"], c["error"]))
            f.write("".join("ACGT"[x] for x in c["read"]) + "\n")
            f.write("".join("ACGT"[x] for x in c["tmpl"]) + "\n")


def run_model(exe, tmp, cases, tag, pool=None, high=None):
    """the model's results, one per case: (0,) or (1, [qoff qend toff tend dist n], ident, qaln, taln); the checker itself compares with the host code.  high:
    "straddle" or "top" - the cases' bases around base 2^31 of a buffer that large, or ending at base 2^32 - 2 (tests/host_core/high_base.h)"""
    inp, out = os.path.join(tmp, "cases_" + tag), os.path.join(tmp, "out_" + tag)
    write_cases(inp, cases)
    r = subprocess.run([exe, inp, out] + ([str(pool or 64 << 20)] if pool or high else []) + ([high] if high else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = dict(kv.split("=") for kv in r.stdout.split())
    assert int(stats["selfcheck"]) == 0 and int(stats["cases"]) == len(cases)
    if high:
        first, last = int(stats["first_base"]), int(stats["last_base"])
        assert (first < 1 << 31 < last) if high == "straddle" else (first > 1 << 31 and last == (1 << 32) - 2)
    res = []
    for ln in open(out):
        f = ln.split()
        res.append((0,) if f[0] == "0" else (1, [int(x) for x in f[1:7]], float(f[7]), f[8].encode(), f[9].encode()))
    assert len(res) == len(cases)
    return res, stats


def against_golden(res, cases, golden):
    g = {c["name"]: c for c in golden}
    n_ok = 0
    for r, c in zip(res, cases):
        want = g[c["name"]]
        assert r[0] == want["ret"], c["name"]
        if r[0]:
            assert (r[1], r[2], ora.fnv64(r[3]), ora.fnv64(r[4])) == (want["out"], want["ident"], want["qaln"], want["taln"]), c["name"]
            n_ok += 1
    return n_ok


def test_model_on_rescue_golden(checker, tmp_path):
    cases = nw_cases.golden_rescue_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "golden")
    g = json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["edlib_go"]
    assert against_golden(res, cases, [dict(c, name="seed%d" % c["seed"]) for c in g]) > 15
    assert int(stats["splits"]) > 20          # the big cases nest their splits


def test_model_on_edges(checker, tmp_path):
    res, _ = run_model(checker, str(tmp_path), nw_cases.edge_cases(), "edges")
    assert [r[0] for r in res] == [1, 1, 0, 1, 1, 0, 1, 1, 0, 1]


def test_model_on_shapes(checker, tmp_path):
    cases = nw_cases.shape_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "shapes")
    g = json.load(open(os.path.join(util.GOLDEN, "nw_cases.json")))["cases"]
    assert against_golden(res, cases, g) >= 12
    by = {c["name"]: r for c, r in zip(cases, res)}
    # either side of every reject rule
    for gone, kept in (("tol_below_diff", "tol_at_diff"), ("best_above_tol", "best_at_tol"), ("len_below_min", "len_at_min"), ("error_above", "error_at")):
        assert by[gone][0] == 0 and by[kept][0] == 1, (gone, kept)
    assert by["no_run"][0] == 0 and by["unrelated"][0] == 1
    # the same cases with the smallest flag pool: several chunks of leaves, the same answers
    res1, stats1 = run_model(checker, str(tmp_path), cases, "shapes_pool", pool=1 << 20)
    assert res1 == res and int(stats1["leaf_chunks"]) > int(stats["leaf_chunks"])


@pytest.mark.parametrize("high", ["straddle", "top"])
def test_model_at_high_positions(checker, tmp_path, high):
    """the shapes and the golden rescue pairs once more with their bases around base 2^31, and ending at base 2^32 - 2: the expectations of the tests above, unchanged"""
    cases = nw_cases.shape_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "shapes_" + high, high=high)
    assert against_golden(res, cases, json.load(open(os.path.join(util.GOLDEN, "nw_cases.json")))["cases"]) >= 12
    cases = nw_cases.golden_rescue_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "golden_" + high, high=high)
    g = json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["edlib_go"]
    assert against_golden(res, cases, [dict(c, name="seed%d" % c["seed"]) for c in g]) > 15
    assert int(stats["splits"]) > 20


def test_leaf_limit_branches(checker, tmp_path):
    """1800 rows against 1783 columns is one leaf, against 1784 one split into two; 41 rows against 40 000 columns splits with one word of rows"""
    by = {c["name"]: c for c in nw_cases.shape_cases()}
    for name, splits, leaves in (("leaf_1783", 0, 1), ("split_1784", 1, 2)):
        _, stats = run_model(checker, str(tmp_path), [by[name]], name)
        assert (int(stats["splits"]), int(stats["leaves"])) == (splits, leaves), name
    _, stats = run_model(checker, str(tmp_path), [by["split_m41"]], "m41")
    assert int(stats["splits"]) >= 1


def test_model_on_random_pairs(checker, tmp_path):
    cases = nw_cases.seed_cases(range(5000, 5240))
    res, stats = run_model(checker, str(tmp_path), cases, "seeds")
    assert len(cases) > 200 and sum(r[0] for r in res) > 80
    assert int(stats["splits"]) > 50 and int(stats["leaves"]) > len(cases) // 2
