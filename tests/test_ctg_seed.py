"""CPU tests of the seeding of contig polishing: the host form (necat_amd/csrc/ctg_seed.h, path 1 of necat_ctg_seed_batch) and the CPU model of the device cores
(necat_amd/csrc/ctg_seed_core.h) through tests/host_core/check_ctg_seed.cpp, a stand-alone program built by g++ once plainly and once with
-fsanitize=address,undefined:
  * against the reference's own output, number for number: the natural case (the contig and reads of tests/golden/ctg_g/nat*.bin.gz, every read on both strands;
    answers in tests/golden/ctg_s/nat.ans.bin.gz) and the crafted set (ctg_s/craft.bin.gz) - sorted matches and candidate, the model with the segment's table filled
    in two orders and the chain's arrays at the default capacity and at 8, the candidate also by the literal loop of chaining_find_candidates;
  * against each other on 300 seeded random cases;
  * where the reference's sources are present: three fresh seeds of the crafted generator through the live harness."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ctg_seed_cases as sc
from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_ctg_seed.cpp")
GOLD = os.path.join(util.GOLDEN, "ctg_s")
N_CRAFTED_JOBS = 115


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + list(flags) + ["-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(os.path.join(str(tmp_path_factory.mktemp("ctgseed")), "check_ctg_seed"), "-O2")


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    """the committed cases as the checker reads them: {name: path}"""
    tmp = str(tmp_path_factory.mktemp("ctgseed_cases"))
    out = {"craft": os.path.join(tmp, "craft.bin"), "nat": os.path.join(tmp, "nat.bin")}
    open(out["craft"], "wb").write(gzip.open(os.path.join(GOLD, "craft.bin.gz"), "rb").read())
    sc.write_cases(sc.read_answers(sc.natural(), os.path.join(GOLD, "nat.ans.bin.gz")), out["nat"])
    return out


def _run(exe, n_random, seed, files):
    r = subprocess.run([exe, str(n_random), str(seed)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}


def test_natural_case_matches_the_reference(checker, case_files):
    st = _run(checker, 0, 1, [case_files["nat"]])
    print(st)
    assert st["jobs"] == 370 and st["mismatches"] == 0 and 150 <= st["found"] < 300 and st["max_mems"] <= 512          # the default LDS capacity holds every job


def test_crafted_set_matches_the_reference(checker, case_files):
    st = _run(checker, 0, 1, [case_files["craft"]])
    print(st)
    assert st["jobs"] == N_CRAFTED_JOBS and st["mismatches"] == 0 and st["max_mems"] <= 512
    # the tandem case: the 25-skip break inside a 64-entry step of the scan, at its last entry and in a later step; the capacity of 8 sends jobs to the scratch tier
    assert st["breaks_inside"] > 0 and st["breaks_at_63"] > 0 and st["breaks_later_step"] > 0 and st["global_jobs"] > 0


def test_crafted_set_holds_what_it_is_for():
    """the committed crafted cases still show the properties they were made for"""
    cs = sc.read_cases(os.path.join(GOLD, "craft.bin.gz"))
    by = cs.by_name()

    def ans(name, k=0):
        return by[name].answers[k]

    def bases(name, k=0):
        s = by[name]
        return cs.read_on_strand(*s.jobs[k]), cs.segment_codes(s)

    assert [cs.reads[q].shape[0] for q, _ in by["short_reads"].jobs] == [14, 15, 20, 21] and [a[1].shape[0] for a in by["short_reads"].answers] == [0, 0, 0, 1]
    assert by["seg15"].size == 15 and all(not a[0]["found"] for a in by["seg15"].answers)
    # a match from (0, 0) whose first 15 bases differ everywhere / whose first 6 differ while the true match begins at 6
    for name, n_bad, size in (("off0_survives", 15, 60), ("off0_swallows", 6, 80)):
        r, g = bases(name)
        m = ans(name)[1]
        assert m.tolist() == [[0, 0, size]] and (r[:n_bad] != g[:n_bad]).all() and (r[n_bad:size] == g[n_bad:size]).all()
    assert (cs.segment_codes(by["polya_10"])[200:218] == 0).all() and (cs.segment_codes(by["polya_27"])[200:240] == 0).all()
    # the entry at offset 0 is a member of the other list's poly-A group and counts towards its occ: with 19 true entries (1 x 20) the read's offset-0 entry gives
    # a match from read offset 0 over fifteen A's it does not have; with 20 (1 x 21) only the true match is left.  The mirror on the segment's offset-0 entry
    r, g = bases("polya_q0_20")
    assert ans("polya_q0_20")[1].tolist() == [[0, 218, 40]] and (g[200:233] == 0).all() and g[233] != 0 and (r[:15] != 0).all() and (r[15:40] == g[233:258]).all()
    assert ans("polya_q0_21")[1].tolist() == [[15, 234, 25]] and (cs.segment_codes(by["polya_q0_21"])[200:234] == 0).all()
    r, g = bases("polya_s0_20")
    assert ans("polya_s0_20")[1].tolist() == [[168, 0, 40]] and (r[60:183] == 0).all() and r[183] != 0 and (g[:15] != 0).all() and (r[183:208] == g[15:40]).all()
    r, g = bases("polya_s0_21")
    assert ans("polya_s0_21")[1].tolist() == [[189, 15, 25]] and (r[60:189] == 0).all() and r[189] != 0
    # products: 1 x 20 and 4 x 5 give their 20 matches, 3 x 7 and 1 x 21 none; the two copies off the sampling grid give t more each (w[5:20], w[4:19]: 1 x t)
    n20 = lambda name: int((ans(name)[1][:, 2] >= 20).sum())
    assert n20("occ_1x20") == 20 + 2 * 20 and n20("occ_4x5") == 20 + 2 * 5 and n20("occ_3x7") == 2 * 7
    assert n20("occ_1x21") == 0
    # the four ends: the read's two, the segment's first base (the read goes on agreeing with the contig in front of it) and its last
    s = by["four_ends"]
    assert ans("four_ends", 0)[1].tolist() == [[0, 100, 300]] and ans("four_ends", 1)[1].tolist() == [[30, 0, 250]] and ans("four_ends", 2)[1].tolist() == [[0, 650, 250]]
    ctg, r1 = cs.contigs[s.ctg_id], cs.read_on_strand(*s.jobs[1])
    assert s.start == 30 and (r1[:30] == ctg[:30]).all() and s.start + s.size + 30 == ctg.shape[0]
    assert ans("mem_19_20")[1].tolist() == [[120, 300, 20]]
    assert ans("one_mismatch")[1].tolist() == [[0, 200, 60], [61, 261, 59]]
    a200, a199 = ans("exact_200_199", 0), ans("exact_200_199", 2)
    assert a200[1].tolist() == [[20, 300, 200]] and a200[0]["found"] == 1 and a200[0]["score"] == 200
    assert a199[1].tolist() == [[20, 300, 199]] and a199[0]["found"] == 0 and not ans("exact_200_199", 1)[0]["found"]
    mod = [by["mod32_%d" % m] for m in range(32)]
    assert sorted(s.start % 32 for s in mod) == list(range(32)) and sorted(s.answers[0][1][0, 0] % 32 for s in mod) == list(range(32))
    assert all(s.answers[0][0]["found"] and not s.answers[1][0]["found"] for s in mod) and {s.jobs[0][1] for s in mod} == {0, 1}
    assert len({int(np.concatenate(cs.reads[:q]).shape[0]) % 32 for s in mod for q, _ in s.jobs[:1]}) == 32          # the reads' own starts in the volume
    for name, found in (("gap_q3000", 1), ("gap_q3001", 0), ("gap_s3000", 1), ("gap_s3001", 0)):
        c, m = ans(name)
        assert c["found"] == found and m.shape[0] == 2 and (not found or c["score"] == 227)
    assert {(int(m[1, 0] - m[0, 0]), int(m[1, 1] - m[0, 1])) for m in (ans(n)[1] for n in ("gap_q3000", "gap_q3001", "gap_s3000", "gap_s3001"))} == \
        {(3000, 2990), (3001, 2991), (2990, 3000), (2991, 3001)}
    c0, c1 = ans("drift_1500")[0], ans("drift_1501")[0]
    assert c0["qend"] - c0["qbeg"] > 5000 and c0["score"] == 2770 and c1["score"] == 2340 and c1["qend"] - c1["qbeg"] < 2500
    c, m = ans("peak_not_end")
    assert m.shape[0] == 11 and c["score"] == 390 and c["qend"] == 411 and int(m[-1, 0]) > 411          # the chain's last match lies behind the peak's end
    c, m = ans("equal_peaks")
    assert m[:, 2].tolist() == [250, 250] and c["score"] == 250 and c["sbeg"] == int(m[1, 1])
    c, m = ans("equal_longest")
    assert m[:, 2].tolist() == [150, 150] and c["qbeg"] == 30 and c["qend"] == 480 and c["qoff"] == 30 + 75
    assert max(a[1].shape[0] for a in by["tandem"].answers) > 128
    assert all(a[0]["found"] for a in by["noisy"].answers[0::2]) and not any(a[0]["found"] for a in by["noisy"].answers[1::2])


def test_random_cases_agree(checker):
    st = _run(checker, 300, 20261, [])
    print(st)
    assert st["random"] == 300 and st["random_mismatches"] == 0 and st["found"] > 300 and st["global_jobs"] > 0


def test_checker_is_clean_under_sanitizers(case_files, tmp_path):
    """the stand-alone checker with -fsanitize=address,undefined (host code only): the crafted set and 40 random cases"""
    exe = _build(os.path.join(str(tmp_path), "check_asan"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    st = _run(exe, 40, 3, [case_files["craft"]])
    assert st["mismatches"] == 0 and st["random_mismatches"] == 0 and st["jobs"] == N_CRAFTED_JOBS


@pytest.mark.skipif(not sc.have_reference(), reason="the reference's sources are not on this machine")
@pytest.mark.parametrize("seed", [101, 102, 103])
def test_fresh_seeds_through_the_live_reference(checker, tmp_path, seed):
    tmp = str(tmp_path)
    exe = sc.build_harness(os.path.join(tmp, "harness"))
    cs = sc.crafted(seed)
    sc.run_harness(exe, cs, tmp)
    path = os.path.join(tmp, "fresh.bin")
    sc.write_cases(cs, path)
    st = _run(checker, 0, 1, [path])
    assert st["jobs"] == N_CRAFTED_JOBS and st["mismatches"] == 0
