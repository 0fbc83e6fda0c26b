"""CPU tests of the DEVICE form of oc2asmpm's end extension (necat_amd/csrc/asm_ends_core.h: plan_ends and finish_ends, the per-anchor cores of k_asm_ends_plan and
k_asm_ends_finish, with dal_core.h's wave for the DALIGNER jobs), built here by g++ as a model of the device path.  tests/host_core/check_asm_ends.cpp runs the model
lane by lane on the aligner's own stream layout (left stream reversed, two bits per column) and compares every alignment with asm_core.h's Extender::ends (gapped
strings) and Extender::ends_packed (packed columns) for EQUALITY of the coordinates, the identity and which ends were extended.  This file feeds it
  * the alignments of the oracle's block aligner on tests/golden/vols_d with the asm_d arguments (as tests/host_core/check_asmpm.cpp walks them) and holds the branch
    counts against what the host code gives on that set,
  * crafted ends: unrelated prefixes / suffixes of 20 - 299 bases at the anchor, related ones, hangs of 0 and above 300, cores below 400 columns and below the identity
    cut, column streams without a run of 8 and with from >= to; ends that the host code tries and declines (low-complexity ends found by search: unrelated random ends
    are always extended); and made-up tips for each acceptance test,
  * the crafted ends once more at capacities of 4 and 16 diagonals (jobs in all three tiers, the answers unchanged),
and builds the checker once more as a stand-alone program with -fsanitize=address,undefined."""
import json
import os
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_asm_ends.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]


def build(tmp, name, extra=(), oracle=False):
    exe = os.path.join(tmp, name)
    objs = []
    if oracle:
        obj = os.path.join(tmp, "necat_oracle.o")
        subprocess.run(["gcc", "-O2", "-std=gnu99", "-c", os.path.join(util.ROOT, "oracle", "necat_oracle.c"), "-o", obj], check=True)
        objs = ["-DCHECK_ASM_ENDS_ORACLE", obj, "-lm", "-lpthread"]
    subprocess.run(["g++"] + FLAGS + list(extra) + ["-o", exe, SRC] + objs, check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("asm_ends")), "check_asm_ends", oracle=True)


def run(exe, args):
    """the checker's counters; it compares the model with the host code itself and exits 1 on any difference"""
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert n["bad"] == 0
    for side in "lr":       # the model's branch counts are the host code's
        for k in ("tried", "extended", "hang0", "hang_long", "no_run", "declined"):
            assert n["%s_%s" % (k, side)] == n["h_%s_%s" % (k, side)], (k, side, n)
    assert n["both"] == n["h_both"] and n["jobs"] == n["tier1"] + n["tier2"] + n["host"]
    return n


def test_model_on_golden(checker, tmp_path):
    """tests/golden/vols_d, the asm_d arguments: 465 alignments with a record; the host code's branch counts on that set"""
    m = json.load(open(os.path.join(util.GOLDEN, "manifest_asm_rm.json")))["asm_d"]
    wrk = util.install_golden_volumes(m["volumes"], tmp_path)
    tot = {}
    for v in range(m["n_volumes"]):
        for k, x in run(checker, ["golden", 128, 512] + m["args"].split() + [wrk, v]).items():
            tot[k] = max(tot.get(k, 0), x) if k == "max_diags" else tot.get(k, 0) + x
    assert tot["ok"] - tot["low_ident"] == 465
    assert (tot["tried_l"], tot["extended_l"], tot["hang0_l"], tot["hang_long_l"], tot["no_run_l"], tot["declined_l"]) == (238, 238, 133, 94, 0, 0)
    assert (tot["tried_r"], tot["extended_r"], tot["hang0_r"], tot["hang_long_r"], tot["no_run_r"], tot["declined_r"]) == (288, 288, 105, 72, 0, 0)
    assert tot["both"] == 136
    assert tot["jobs"] == 238 + 288 == tot["tier1"] and tot["max_diags"] <= 128          # every job inside the first capacity


def test_model_on_crafted_ends(checker):
    n = run(checker, ["crafted", 128, 512, 11, 400])
    assert n["cases"] == 400 + 12 and n["host"] == 0
    for side in "lr":
        assert n["extended_" + side] >= 200 and n["hang0_" + side] >= 20 and n["hang_long_" + side] >= 20
        # tried, not extended: the streams without a run of 8, and the ends DALIGNER declines (an identity below 0)
        assert n["no_run_" + side] >= 20 and n["declined_" + side] >= 3 and n["tried_" + side] - n["extended_" + side] == n["no_run_" + side] + n["declined_" + side]
    assert n["from_ge_to"] >= 10 and n["low_ident"] >= 20 and n["cases"] - n["ok"] >= 20 and n["both"] >= 100
    # the same at 4 and 16 diagonals: the tiers change, the answers (compared inside the checker) and the branch counts do not
    s = run(checker, ["crafted", 4, 16, 11, 400])
    assert s["tier1"] > 0 and s["tier2"] > 0 and s["host"] > 0
    skip = ("tier1", "tier2", "host", "steps", "max_diags")
    assert {k: v for k, v in s.items() if k not in skip} == {k: v for k, v in n.items() if k not in skip}
    # one tier only (the first capacity is the second)
    one = run(checker, ["crafted", 16, 16, 11, 400])
    assert one["tier2"] == 0 and one["host"] > 0 and one["tier1"] == s["tier1"] + s["tier2"]


def test_model_under_sanitizers(tmp_path):
    """the stand-alone checker built with the address and undefined-behaviour sanitizers exits clean on the crafted ends (at both pairs of capacities)"""
    exe = build(str(tmp_path), "check_asm_ends_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    run(exe, ["crafted", 128, 512, 11, 200])
    run(exe, ["crafted", 4, 16, 11, 200])
