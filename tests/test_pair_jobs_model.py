"""CPU test of the rescue pair's formulation (necat_amd/csrc/rescue_pair.h: the functions stage_dalign.inl, stage_nw.inl, stage_refmap.inl, stage_ctg_extend.inl and
stage_cns.inl build their jobs with) on the contig stage's shape, a subject slice strictly inside a sequence.  tests/host_core/check_pair_jobs.cpp lays a read and a
subject out in one word buffer between other bases and checks, over slice starts at every residue mod 32, from = 0, from + len = the subject's size and both strands:
the bases dal::seq_at reads over the built task against BaseWords' decode (4 at -1 and at len), the anchor from k0 / mida, range -> job -> result -> slice as the
identity on coordinates, and result -> tips -> decode as the identity with the accept rule.  Built plain and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_pair_jobs.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("extra", [[], SAN], ids=["plain", "sanitizers"])
def test_pair_jobs(tmp_path, extra):
    exe = os.path.join(str(tmp_path), "check_pair_jobs")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert n["residues"] == 32 and n["from0"] >= 2 and n["to_end"] >= 2 and n["inside"] >= 64 and n["jobs"] == 2 * 41 * 3
    # once more with the volume's bases around base 2^31 of a buffer that large and - plain only: a buffer of 1 GB - ending at base 2^32 - 2; the same counts
    for high in ["straddle"] + ([] if extra else ["top"]):
        r = subprocess.run([exe, high], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        h = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
        assert (h["first_base"] < 1 << 31 < h["last_base"]) if high == "straddle" else (h["first_base"] > 1 << 31 and h["last_base"] == (1 << 32) - 2)
        assert {k: h[k] for k in n if k != "residues"} == {k: n[k] for k in n if k != "residues"} and h["residues"] == 32
