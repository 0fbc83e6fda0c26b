"""CPU tests of the consensus half of contig polishing: the host form (necat_amd/csrc/ctg_consensus.h, path 1 of necat_ctg_consensus_batch) and the CPU model of the
device cores (necat_amd/csrc/ctg_dev_core.h) through tests/host_core/check_ctg_consensus.cpp, a stand-alone program built by g++ once plainly and once with
-fsanitize=address,undefined:
  * against the reference's own output, byte for byte: the natural case (tests/golden/ctg_g/nat*.bin.gz: what the reference's ctgcns handed to add_align_tags, what
    get_cns_from_align_tags left, and the program's polished contig) and the crafted set (craft.bin.gz: the reference's two functions on made-up gapped strings),
    the model at the default tag budget and at one that cuts a segment into at least 4 position ranges;
  * against each other on the case the reference cannot answer (one run of 65 540 query bases: the stop rule) and on 300 seeded random cases;
  * where the reference's sources are present: three fresh seeds of the crafted generator through the live harness."""
import gzip
import os
import re
import subprocess

import pytest

from tests import ctg_cases as cc
from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_ctg_consensus.cpp")
GOLD = os.path.join(util.GOLDEN, "ctg_g")


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + list(flags) + ["-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(os.path.join(str(tmp_path_factory.mktemp("ctg")), "check_ctg_consensus"), "-O2")


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    """the committed case files unpacked, and the stop-rule case: {name: path}"""
    tmp = str(tmp_path_factory.mktemp("ctg_cases"))
    out = {}
    for leaf in ("nat.reads.bin", "nat.bin", "craft.bin"):
        out[leaf] = os.path.join(tmp, leaf)
        open(out[leaf], "wb").write(gzip.open(os.path.join(GOLD, leaf + ".gz"), "rb").read())
    out["stop.bin"] = os.path.join(tmp, "stop.bin")
    cc.write_cases(cc.stop_rule_case(5), out["stop.bin"])
    return out


def _run(exe, n_random, seed, files):
    r = subprocess.run([exe, str(n_random), str(seed)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}


def test_natural_case_matches_the_reference(checker, case_files):
    st = _run(checker, 0, 1, [case_files["nat.reads.bin"], case_files["nat.bin"]])
    print(st)
    assert st["cases"] == 1 and st["mismatches"] == 0 and st["tags"] > 500_000 and st["min_ranges"] >= 4


def test_crafted_set_matches_the_reference(checker, case_files):
    st = _run(checker, 0, 1, [case_files["craft.bin"]])
    print(st)
    assert st["cases"] == 8 and st["mismatches"] == 0 and st["min_ranges"] >= 4


def test_crafted_set_holds_what_it_is_for():
    """the committed crafted cases still show the properties they were made for"""
    cs = cc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    by = {c.name: c for c in cs.cases}
    assert max(int((o[6] == 1).sum()) for o in by["ins_40000"].ovl) >= 40000 and len(by["ins_40000"].cns) > 40000          # the long run is on the best path
    assert any(o[6][0] == 2 and o[6][-1] == 2 for o in by["del_ends"].ovl) and any(o[6][0] == 1 for o in by["del_ends"].ovl)
    assert any(o[4] == 0 for o in by["ins_runs"].ovl) and any(o[5] == by["ins_runs"].size for o in by["ins_runs"].ovl)
    low = by["nocov_cov3"].cns
    assert any(97 <= x for x in low) and any(x < 97 for x in low) and int(by["nocov_cov3"].t_pos.min()) >= 1800              # the uncovered stretch cuts the path
    runs = [len(m) for m in re.findall(rb"[A-Z]+", by["runs_999_1000"].cns)]
    assert runs == [999, 1000]
    assert len(by["tie_links"].cns) > 0 and len(by["tie_best"].cns) > 0


def test_stop_rule_and_random_cases_agree(checker, case_files):
    st = _run(checker, 300, 20261, [case_files["stop.bin"]])
    print(st)
    assert st["cases"] == 1 and st["stopped"] >= 1 and st["random"] == 300 and st["mismatches"] == 0 and st["random_mismatches"] == 0


def test_checker_is_clean_under_sanitizers(case_files, tmp_path):
    """the stand-alone checker with -fsanitize=address,undefined (host code only): the crafted set, the stop rule and 40 random cases"""
    exe = _build(os.path.join(str(tmp_path), "check_asan"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    st = _run(exe, 40, 3, [case_files["craft.bin"], case_files["stop.bin"]])
    assert st["mismatches"] == 0 and st["random_mismatches"] == 0 and st["cases"] == 9


@pytest.mark.skipif(not cc.have_reference(), reason="the reference's sources are not on this machine")
@pytest.mark.parametrize("seed", [101, 102, 103])
def test_fresh_seeds_through_the_live_reference(checker, tmp_path, seed):
    tmp = str(tmp_path)
    exe = cc.build_harness(os.path.join(tmp, "harness"))
    cs = cc.crafted(seed)
    cc.run_harness(exe, cs, tmp)
    path = os.path.join(tmp, "fresh.bin")
    cc.write_cases(cs, path)
    st = _run(checker, 0, 1, [path])
    assert st["cases"] == 8 and st["mismatches"] == 0
