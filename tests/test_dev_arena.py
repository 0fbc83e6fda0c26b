"""CPU test of the layout half of the batch stages' device arena (necat_amd/csrc/arena_layout.h, stage_arenas.h) through tests/host_core/check_dev_arena.cpp, a stand-alone
program built by g++ once plainly and once with -fsanitize=address,undefined: slots of 1, 2, 4, 8, 12, 16 and 24-byte elements at counts 0, 1, 63, 64, 65 and a
sequence past 2^32 bytes begin at multiples of 256, ascend in take order, do not reach into each other or past bytes(); take(0) leaves the cursor; bytes() is
the sum of the rounded sizes.  The stages' five arena structs obey the same rules at the smallest shapes (one template with one overlap of one column, one
range of one position, one job with zero seeds, one anchor) and at a larger odd one, have the slot order and counts their kernels and clears rely on, and are as
many bytes as the expressions the stages carved with before."""
import os
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_dev_arena.cpp")


def _build(out, *flags):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + list(flags) + ["-I", os.path.join(util.ROOT, "necat_amd", "csrc"), "-o", out, SRC],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "check_dev_arena: ok" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]


def test_layout_rules(tmp_path):
    exe = os.path.join(str(tmp_path), "check_dev_arena")
    c = _build(exe, "-O2")
    assert c.returncode == 0 and "warning" not in c.stdout, c.stdout[-3000:]
    _run(exe)


def test_layout_rules_under_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined (host code only, a program of its own); whether g++ has the sanitizers' runtimes here is decided by a
    one-line probe program"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = os.path.join(str(tmp_path), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17"] + san + ["-o", os.path.join(str(tmp_path), "probe"), probe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + p.stdout[-200:])
    exe = os.path.join(str(tmp_path), "check_dev_arena_asan")
    c = _build(exe, *san)
    assert c.returncode == 0, c.stdout[-3000:]
    _run(exe)
