"""CPU test of the size-class order of a round's ragged blocks (necat_amd/csrc/item_order.h) through tests/host_core/check_item_order.cpp, a
stand-alone program built by g++ once plainly and once with -fsanitize=address,undefined.  The program replays the appends (staging slot, class counters per
workgroup) and k_round_ctl's class scan and scatter with the header's own functions - list sizes 0, 1, 15, 16, 17, 63, 64, 65 and 5000 for list A's ragged part and
for list B, target lengths at the class edges (1, 32, 33, 511, 512; 513, 544, 545, 794), all items in one class, alternating extremes, several workgroups whose
reservations fall in a shuffled order - and checks that the lists are a permutation of what was appended, that the classes never grow along the work index, that
the full front of list A and everything outside the lists are untouched, and the bound on the lane-steps issued beyond those needed for groups of 4, 8 and 64."""
import os
import re
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_item_order.cpp")


def _build(out, *flags):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + list(flags) + ["-I", os.path.join(util.ROOT, "necat_amd", "csrc"), "-o", out, SRC],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    m = re.search(r"check_item_order: ok cases=(\d+)", r.stdout)
    assert m and int(m.group(1)) == 9 * 9 * 8, r.stdout[-3000:]


def test_append_scan_scatter_replay(tmp_path):
    exe = os.path.join(str(tmp_path), "check_item_order")
    c = _build(exe, "-O2")
    assert c.returncode == 0 and "warning" not in c.stdout, c.stdout[-3000:]
    _run(exe)


def test_append_scan_scatter_replay_under_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined (host code only, a program of its own): the item arrays, the staging array and the class words are held
    without slack, so a slot outside them is caught here; whether g++ has the sanitizers' runtimes is decided by a one-line probe program"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = os.path.join(str(tmp_path), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17"] + san + ["-o", os.path.join(str(tmp_path), "probe"), probe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + p.stdout[-200:])
    exe = os.path.join(str(tmp_path), "check_item_order_asan")
    c = _build(exe, *san)
    assert c.returncode == 0, c.stdout[-3000:]
    _run(exe)


def test_binding_header_and_knob_agree():
    """the getter of the waste counters is declared, bound and listed; the struct is the header's; the knob is in the table with default 1"""
    from necat_amd import capi
    hdr = open(os.path.join(util.ROOT, "include", "necat_hip.h")).read()
    assert "necat_get_item_order_stats" in capi.EXPORTED_SYMBOLS and re.search(r"\bnecat_get_item_order_stats\(", hdr)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} necat_item_order_stats;", hdr).group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in capi.ItemOrderStats._fields_] and hasattr(capi.Context, "item_order_stats")
    knobs = open(os.path.join(util.ROOT, "necat_amd", "csrc", "knobs.h")).read()
    assert re.search(r'NUM\(item_sort,\s*u32,\s*"NECAT_ITEM_SORT",\s*1,', knobs)
