"""CPU tests of the aligner and coverage cap of contig polishing (necat_ctg_extend_batch): the serial pass of necat_amd/csrc/ctg_extend.h through
tests/host_core/check_ctg_extend.cpp, a stand-alone program built by g++ on that header alone, once plainly and once with -fsanitize=address,undefined:
  * fed with the reference's own per-record aligner results (tests/golden/ctg_x: the crafted set and the natural case), the pass gives the reference's verdicts,
    overlap order and count of extended records, number for number - with the cap (the reference's loop) and without (every record by the accept rule);
  * the committed crafted set still does in the reference's log what each of its cases is there for;
  * where the reference's sources are present: the committed files are what the generator writes today.
And what of the entry needs no device: the binding's structs against the header, the exported symbols, the ABI number."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ctg_ext_cases as xc
from tests import util

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_ctg_extend.cpp")
N_CRAFTED, N_NATURAL = 67, 149


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + list(flags) + ["-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(os.path.join(str(tmp_path_factory.mktemp("ctgext")), "check_ctg_extend"), "-O2")


@pytest.fixture(scope="module")
def sets():
    return {"craft": xc.load_crafted(), "nat": xc.load_natural()[0]}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, sets):
    tmp = str(tmp_path_factory.mktemp("ctgext_in"))
    out = {}
    for name, cs in sets.items():
        for cap in (1, 0):
            out[name, cap] = os.path.join(tmp, "%s_%d.txt" % (name, cap))
            xc.checker_input(cs, out[name, cap], cap)
    return out


def _run(exe, files):
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}


@pytest.mark.parametrize("cap", [1, 0])
def test_the_pass_gives_the_references_loop_on_the_crafted_set(checker, inputs, cap):
    st = _run(checker, [inputs["craft", cap]])
    print(st)
    assert st["segments"] == 4 and st["records"] == N_CRAFTED and st["mismatches"] == 0 and st["unit_failures"] == 0
    assert (st["capped"] == 5 and st["accepted"] == 54) if cap else (st["capped"] == 0 and st["accepted"] == 59)


@pytest.mark.parametrize("cap", [1, 0])
def test_the_pass_gives_the_references_loop_on_the_natural_case(checker, inputs, cap):
    st = _run(checker, [inputs["nat", cap]])
    print(st)
    assert st["segments"] == 1 and st["records"] == N_NATURAL and st["mismatches"] == 0
    assert (st["capped"], st["accepted"]) == ((1, 148) if cap else (0, 149))


def test_a_wrong_table_is_noticed(checker, inputs, tmp_path):
    """the checker is not vacuous: one alignment made one base shorter in the table moves the reference's verdict away from the pass's"""
    lines = open(inputs["craft", 1]).read().split("\n")
    k = next(i for i, ln in enumerate(lines) if len(ln.split()) == 11 and ln.split()[2] == "5000" and int(ln.split()[6]) - int(ln.split()[5]) == 3000)
    f = lines[k].split()
    f[6] = str(int(f[6]) - 1)
    lines[k] = " ".join(f)
    bad = os.path.join(str(tmp_path), "bad.txt")
    open(bad, "w").write("\n".join(lines))
    r = subprocess.run([checker, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "mismatches=0" not in r.stdout


def test_checker_is_clean_under_sanitizers(inputs, tmp_path):
    """the stand-alone checker with -fsanitize=address,undefined (host code only): both sets, both modes"""
    exe = _build(os.path.join(str(tmp_path), "check_asan"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    st = _run(exe, sorted(inputs.values()))
    assert st["mismatches"] == 0 and st["unit_failures"] == 0 and st["records"] == 2 * (N_CRAFTED + N_NATURAL)


def test_crafted_set_holds_what_it_is_for(sets):
    cs = sets["craft"]
    cs2 = xc.crafted()          # the tags live in the generator; the committed file is its output
    assert [s.records for s in cs.segments] == [s.records for s in cs2.segments] and all((a == b).all() for a, b in zip(cs.reads, cs2.reads))
    for s, s2 in zip(cs.segments, cs2.segments):
        s.tags = s2.tags
    xc.check_crafted(cs)
    assert [s.size for s in cs.segments] == [20000, 30000, 30000, 9000] and [s.start for s in cs.segments] == [0, 15000, 30000, 0]
    assert [c.shape[0] for c in cs.contigs] == [20000, 60000, 9000]
    assert sum(xc.expected_decided(a) == xc.BY_PAIR for s in cs.segments for a in s.ans) == 2
    for s in cs.segments:          # every logged alignment's columns add up to its coordinates
        for a, ops in zip(s.ans, s.ops):
            if a["ok"]:
                assert ops.shape[0] == a["align_size"] and int((ops != 2).sum()) == a["qend"] - a["qoff"] and int((ops != 1).sum()) == a["tend"] - a["toff"]


def test_natural_case_is_the_consensus_halfs(sets):
    """the natural case's accepted alignments, in loop order, are the 148 overlaps tests/golden/ctg_g holds - what the chain test hands on"""
    cs, case = xc.load_natural()
    s = cs.segments[0]
    ov = [k for k in np.argsort([a["order"] for a in s.ans], kind="stable") if s.ans[k]["order"] >= 0]
    assert len(ov) == len(case.ovl) == 148 and len(s.records) == N_NATURAL
    for k, o in zip(ov, case.ovl):
        a = s.ans[k]
        assert tuple(int(a[f]) for f in ("qid", "qdir", "qoff", "qend", "toff", "tend")) == o[:6] and (s.ops[k] == o[6]).all()
    assert sorted(r[2] for r in s.records) == [r[2] for r in s.records]          # the program's order: by soff


def test_binding_matches_the_header():
    from necat_amd import capi
    hdr = open(os.path.join(util.ROOT, "include", "necat_hip.h")).read()
    assert "#define NECAT_ABI_VERSION   16" in hdr and capi.ABI_VERSION == 16
    for sym in ("necat_ctg_extend_batch", "necat_ctg_extend_free", "necat_ctg_extend_default_options"):
        assert sym in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)
    # the result struct, field by field in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} necat_ctg_extend;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in capi._CtgExtend._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} necat_ctg_extend_result;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(capi.CTG_EXTEND_RESULT_DTYPE.names)
    assert (capi.CTG_EXT_CAPPED, capi.CTG_EXT_NO_SEED, capi.CTG_EXT_NO_ALIGNMENT, capi.CTG_EXT_REJECTED, capi.CTG_EXT_ACCEPTED) == (xc.CAPPED, xc.NO_SEED, xc.NO_ALIGNMENT, xc.REJECTED, xc.ACCEPTED)
    for k, name in enumerate(("CAPPED", "NO_SEED", "NO_ALIGNMENT", "REJECTED", "ACCEPTED")):
        assert re.search(r"#define NECAT_CTG_EXT_%s\s+%d\b" % (name, k), hdr)


def test_library_has_the_entry_and_its_defaults():
    """no device needed: the built library exports the three symbols and its defaults are the loop with the pair on the device"""
    from necat_amd import capi
    lib = capi.load_library()
    o = capi.ctg_extend_options()
    assert (o.cap, o.rescue_path, o.host_threads) == (1, 0, 0)
    assert capi.ctg_extend_options(cap=0, rescue_path=1).rescue_path == 1
    with pytest.raises(KeyError):
        capi.ctg_extend_options(path=1)
    lib.necat_ctg_extend_free(None)
    # without a context nothing is touched: NECAT_ERR_ARG
    import ctypes as C
    out = C.POINTER(capi._CtgExtend)()
    assert lib.necat_ctg_extend_batch(None, None, 0, None, None, 0, None, None, C.byref(o), C.byref(out)) == -1 and not out


@pytest.mark.skipif(not xc.have_reference(), reason="the reference's sources are not on this machine")
def test_committed_files_are_what_the_reference_gives_today(tmp_path, sets):
    """the crafted set through the live harness: the committed per-record log, bit for bit"""
    tmp = str(tmp_path)
    exe = xc.build_harness(os.path.join(tmp, "harness"))
    cs = xc.crafted()
    xc.run_harness(exe, cs, tmp)
    xc.check_crafted(cs)
    path = os.path.join(tmp, "craft.bin")
    xc.write_cases(cs, path)
    assert open(path, "rb").read() == gzip.open(os.path.join(xc.GOLD, "craft.bin.gz"), "rb").read()
    # the natural case: the committed records through the live harness give the committed log
    nat = sets["nat"]
    live, _ = xc.load_natural()
    for s in live.segments:
        s.ans, s.ops = None, None
    xc.run_harness(exe, live, tmp)
    assert all(a.ans.tobytes()[:0] == b"" for a in live.segments)
    for a, b in zip(live.segments, nat.segments):
        drop = lambda x: [tuple(r[f] for f in xc.ANS_DTYPE.names if f != "ops_off") for r in x]
        assert drop(a.ans) == drop(b.ans) and all((x is None and y is None) or (x == y).all() for x, y in zip(a.ops, b.ops))
