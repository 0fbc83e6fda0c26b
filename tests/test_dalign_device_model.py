"""CPU tests of the DEVICE form of ocda_go (necat_amd/csrc/dal_core.h: the per-lane core of k_dal_wave and the wave-uniform bookkeeping around it, built
here by g++ as a model of the device path).  tests/host_core/check_dalign.cpp runs the model lane by lane, the two directions of a job as separate jobs,
and compares it with rescue::Dalign::go for EQUALITY of ok, the four coordinates, diffs and ident_perc; it also carries every point's `org` and fails if
a record's is not the anchor's diagonal.  This file feeds it
  * the shapes of tests/dalign_cases.py (held against tests/golden/dalign_cases.json, the reference's values, as well),
  * the 60 ocda_go cases of tests/golden/rescue_cases.json (also held against the reference's values there),
  * ocda_inputs of seeds 0 - 399, a fifth of them on the read's reverse strand,
requires that no job read a diagonal without history, met an empty window or outgrew the default capacity, runs the shapes once more with a capacity
of 64 diagonals (some jobs go back to the host code, not all; the answers do not change), and once more built with -fsanitize=address,undefined."""
import json
import os
import subprocess

import pytest

from tests import dalign_cases, util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_dalign.cpp")


def build(tmp, name, extra=()):
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("dalign")), "check_dalign")


def write_cases(path, cases):
    with open(path, "w") as f:
        for c in cases:
            f.write("%d %d %d %d %.17g\n" % (c["qdir"], c["qs"], c["ts"], c["min_size"], c["error"]))
            f.write("".join("ACGT"[x] for x in c["read"]) + "\n")
            f.write("".join("ACGT"[x] for x in c["tmpl"]) + "\n")


def run_model(exe, tmp, cases, tag, cap=None, high=None):
    """the model's results, one per case: (ok, [abpos aepos bbpos bepos diffs], ident, how); the checker itself compares with the host code.  high: "straddle" or
    "top" - every case's bases around base 2^31 of a buffer that large, or ending at base 2^32 - 2 (tests/host_core/high_base.h)"""
    inp, out = os.path.join(tmp, "cases_" + tag), os.path.join(tmp, "out_" + tag)
    write_cases(inp, cases)
    r = subprocess.run([exe, inp, out] + ([str(cap or 512)] if cap or high else []) + ([high] if high else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert stats["cases"] == len(cases) and stats["org_bad"] == 0
    if high:
        assert (stats["first_base"] < 1 << 31 < stats["last_base"]) if high == "straddle" else (stats["first_base"] > 1 << 31 and stats["last_base"] == (1 << 32) - 2)
    res = []
    for ln in open(out):
        f = ln.split()
        res.append((int(f[0]), [int(x) for x in f[1:6]], float(f[6]), int(f[7])))
    assert len(res) == len(cases)
    return res, stats


def clean(stats):
    """no read of a diagonal without history, no empty window, nothing above the capacity"""
    return stats["stale"] == 0 and stats["empty"] == 0 and stats["over_cap"] == 0


def test_model_on_shapes(checker, tmp_path):
    cases = dalign_cases.shape_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "shapes")
    assert clean(stats), stats
    assert not any(r[3] for r in res)
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "dalign_cases.json")))["cases"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    for c, r in zip(cases, res):
        assert (r[0], r[1], r[2]) == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    by = {c["name"]: r for c, r in zip(cases, res)}
    qlen = len(cases[[c["name"] for c in cases].index("noisy_e50")]["read"])
    assert by["same100"][0] == 1 and by["same99"][0] == 0 and by["same99"][1][:4] == [0, 99, 0, 99]
    assert by["noisy_e50"][1][:4] == [0, qlen, 0, 2000]                  # end to end
    e20 = by["noisy_e20"]
    assert e20[0] == 1 and e20[1][0] > 300 and e20[1][1] < qlen - 300    # a local result short of both ends
    assert 64 < stats["max_diags"] <= 512
    # capacity 64: the wide windows go back to the host code, the narrow ones stay; the answers are the same
    res64, stats64 = run_model(checker, str(tmp_path), cases, "shapes64", cap=64)
    assert 0 < stats64["over_cap"] < len(cases) and stats64["stale"] == 0 and stats64["empty"] == 0
    assert [r[:3] for r in res64] == [r[:3] for r in res]
    assert sum(r[3] for r in res64) == stats64["over_cap"]
    assert all(by64[3] == 0 for c, by64 in zip(cases, res64) if c["name"].startswith("word")) and res64[[c["name"] for c in cases].index("deletion600")][3] == 1


def test_model_on_rescue_golden(checker, tmp_path):
    cases = dalign_cases.golden_rescue_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "golden")
    assert clean(stats), stats
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["ocda_go"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    for c, r in zip(cases, res):
        assert (r[0], r[1], r[2]) == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert sum(r[0] for r in res) > 20


@pytest.mark.parametrize("high", ["straddle", "top"])
def test_model_at_high_positions(checker, tmp_path, high):
    """the shapes and the golden pairs once more with every case's bases around base 2^31, and ending at base 2^32 - 2: the expectations of the two tests above,
    unchanged"""
    cases = dalign_cases.shape_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "shapes_" + high, high=high)
    assert clean(stats) and not any(r[3] for r in res) and 64 < stats["max_diags"] <= 512
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "dalign_cases.json")))["cases"]}
    for c, r in zip(cases, res):
        assert (r[0], r[1], r[2]) == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    cases = dalign_cases.golden_rescue_cases()
    res, stats = run_model(checker, str(tmp_path), cases, "golden_" + high, high=high)
    assert clean(stats), stats
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["ocda_go"]}
    for c, r in zip(cases, res):
        assert (r[0], r[1], r[2]) == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert sum(r[0] for r in res) > 20


def test_model_on_random_pairs(checker, tmp_path):
    cases = dalign_cases.seed_cases(range(0, 400))
    res, stats = run_model(checker, str(tmp_path), cases, "seeds")
    assert clean(stats), stats
    assert len(cases) > 380 and sum(c["qdir"] for c in cases) > 70 and sum(r[0] for r in res) > 200
    assert stats["max_diags"] > 128 and stats["steps"] > 100000


def test_model_under_sanitizers(tmp_path):
    """the stand-alone checker built with the address and undefined-behaviour sanitizers exits clean on the shapes (at both capacities)"""
    exe = build(str(tmp_path), "check_dalign_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    cases = dalign_cases.shape_cases()
    _, stats = run_model(exe, str(tmp_path), cases, "san")
    assert clean(stats)
    run_model(exe, str(tmp_path), cases, "san64", cap=64)
    _, stats = run_model(exe, str(tmp_path), cases, "san_straddle", high="straddle")          # a buffer of 2^26 words and more, every case around base 2^31
    assert clean(stats)
