"""CPU test of necat_volume_gather's plan and word function (necat_amd/csrc/volume_gather.h) and of oc2cns's chunk planner (cns_chunks.h) through
tests/host_core/check_vol_gather.cpp, a stand-alone program built by g++ once plainly and once with -fsanitize=address,undefined.  The word function is the one
k_vol_gather runs per destination word: every destination word of every case is compared against a base-by-base merge - three volumes of 1 003, 4 097 and 64
bases tiled with reads of 1 .. 1 000 bases until all 32 x 32 (source offset mod 32, destination offset mod 32) pairs occurred with a read >= 65 and with a read
< 32, ten one-base reads in one word, first and last reads, a last read ending in mid-word, the empty list - and every refusal is checked on the plan (2^32
bases with sizes only).  The planner: a template alone above the bound, a read shared by two chunks, bounds that give 1, 3 and n chunks."""
import os
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_vol_gather.cpp")


def _build(out, *flags):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + list(flags) + ["-I", os.path.join(util.ROOT, "necat_amd", "csrc"), "-o", out, SRC],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "check_vol_gather: ok" in r.stdout and "pairs: all 32 x 32" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]


def _run_high(exe, high):
    """the high form: a source volume whose test reads lie around base 2^31 ("straddle") or end at base 2^32 - 2 ("top"); the destination passes word 2^26"""
    r = subprocess.run([exe, high], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "check_vol_gather: ok" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout and r.stdout.count("destination words from word") == 3, r.stdout[-3000:]
    st = dict(kv.split("=") for kv in r.stdout.splitlines()[-2].split())
    first, last = int(st["first_base"]), int(st["last_base"])
    assert (first < 1 << 31 < last and first % 32 == 13) if high == "straddle" else (first > 1 << 31 and last == (1 << 32) - 2)


def test_word_function_plan_and_chunks(tmp_path):
    exe = os.path.join(str(tmp_path), "check_vol_gather")
    c = _build(exe, "-O2")
    assert c.returncode == 0 and "warning" not in c.stdout, c.stdout[-3000:]
    _run(exe)
    _run_high(exe, "straddle")
    _run_high(exe, "top")


def test_word_function_plan_and_chunks_under_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined (host code only, a program of its own): the source words are held without slack, so a word read
    outside a sequence's own is caught here; whether g++ has the sanitizers' runtimes is decided by a one-line probe program"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = os.path.join(str(tmp_path), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17"] + san + ["-o", os.path.join(str(tmp_path), "probe"), probe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + p.stdout[-200:])
    exe = os.path.join(str(tmp_path), "check_vol_gather_asan")
    c = _build(exe, *san)
    assert c.returncode == 0, c.stdout[-3000:]
    _run(exe)
    _run_high(exe, "straddle")


def test_binding_and_header_agree():
    """the three entry points are declared, bound and listed; the binding's ABI version is the header's; necat_timings is still what the binding copies"""
    import re
    from necat_amd import capi
    hdr = open(os.path.join(util.ROOT, "include", "necat_hip.h")).read()
    assert int(re.search(r"#define NECAT_ABI_VERSION\s+(\d+)", hdr).group(1)) == capi.ABI_VERSION
    for sym in ("necat_volume_gather", "necat_volume_gather_stats", "necat_volume_download"):
        assert sym in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)
    assert hasattr(capi.Context, "gather_volume") and hasattr(capi.Context, "gather_stats") and hasattr(capi.Volume, "download")
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} necat_timings;", hdr).group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in capi.Timings._fields_]
