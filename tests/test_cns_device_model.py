"""CPU tests of the DEVICE form of oc2cns's consensus proper (necat_amd/csrc/cns_dev_core.h: the per-lane cores of the kernels in cns_dev_kernels.h, built here by
g++ as a model of the device path).  tests/host_core/check_cns_device_model.cpp feeds the model and the host form (cns_consensus.h) the add_one_align calls the oracle's
extension loop logs for the committed partition (tests/golden/cns_c):
  * every template the model does not flag has the host's segments, and the two output files assembled from the model's segments have the manifest's md5s;
  * no link weight (summed in overlap-index order) lies further from the host's (klib-order) weight than its error term;
  * at most 10 % of the templates are flagged (the GPU tests' cap on the fallback, checked on the same input);
  * in every unflagged template every node's score lies within its running bound of the host's score of that node;
  * with the tolerance scaled by 1e7 every template is flagged - and the output, then the host's, is still the manifest's;
  * with it scaled by 1e6 the score comparisons (certain()) flag some templates and not others, and those they let through still have the host's segments."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

from tests import util
from oracle import oracle_api as ora

MANIFEST = json.load(open(os.path.join(util.GOLDEN, "cns_c", "manifest.json")))
SRC = os.path.join(util.ROOT, "tests", "host_core", "check_cns_device_model.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory, built):
    exe = os.path.join(str(tmp_path_factory.mktemp("hdm")), "check_cns_device_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    """the oracle's full log of the golden partition, once per option set"""
    tmp = str(tmp_path_factory.mktemp("hdm_logs"))
    wrk = util.install_golden_volumes("vols_c", tmp)
    can = os.path.join(tmp, "cands")
    for fn in ("cands.p0", "cands.partitions"):
        shutil.copy(os.path.join(util.GOLDEN, "cns_c", fn), os.path.join(tmp, fn))
    done = {}

    def get(name):
        if name not in done:
            m = MANIFEST["oc2cns"][name]
            o = ora.cns_options(**m["options"])
            log = os.path.join(tmp, "log_" + name)
            ora.cns_run(o, wrk, can, log, full=True)
            done[name] = (wrk, can, o, m["extra_argv"], log)
        return done[name]
    return get


def _opt(argv, flag, default):
    return argv[argv.index(flag) + 1] if flag in argv else default


def _run(exe, case, tmp, tol, tag=""):
    wrk, can, o, extra, log = case
    mc, mr = os.path.join(tmp, "cns" + tag), os.path.join(tmp, "raw" + tag)
    r = subprocess.run([exe, wrk, can + ".p0", log, str(o.min_cov), _opt(extra, "-l", "500"), _opt(extra, "-f", "0"), mc, mr, tol], check=True, stdout=subprocess.PIPE, text=True)
    st = {k: float(v) for k, v in re.findall(r"(\w+)=(\S+)", r.stdout)}
    return st, open(mc, "rb").read(), open(mr, "rb").read()


@pytest.mark.parametrize("name", sorted(MANIFEST["oc2cns"]))
def test_model_reproduces_reference_outputs(checker, logs, tmp_path, name):
    m = MANIFEST["oc2cns"][name]
    st, cns, raw = _run(checker, logs(name), str(tmp_path), "1")
    print(name, st)
    assert st["templates"] >= 90 and st["links"] > 100000
    assert st["mismatches"] == 0 and st["violations"] == 0
    assert st["nodes"] > 100000 and st["score_violations"] == 0
    assert st["flagged"] <= 0.1 * st["templates"]
    assert (len(cns), cns.count(b">")) == (m["cns_bytes"], m["cns_records"]) and hashlib.md5(cns).hexdigest() == m["cns_md5"]
    assert (len(raw), raw.count(b">")) == (m["raw_bytes"], m["raw_records"]) and hashlib.md5(raw).hexdigest() == m["raw_md5"]


def test_inflated_tolerance_flags_every_template(checker, logs, tmp_path):
    name = sorted(MANIFEST["oc2cns"])[0]
    m = MANIFEST["oc2cns"][name]
    st, cns, raw = _run(checker, logs(name), str(tmp_path), "10000000", "_tol")
    print(st)
    assert st["flagged"] == st["templates"] >= 90 and st["violations"] == 0
    assert st["uncertain"] > 0 and st["bad"] == 0          # (comparisons inside the bounds among the reasons, not the cap on the scaled bound alone)
    assert hashlib.md5(cns).hexdigest() == m["cns_md5"] and hashlib.md5(raw).hexdigest() == m["raw_md5"]


def test_intermediate_tolerance_flags_some_templates_through_comparisons(checker, logs, tmp_path):
    """The certification itself: certain(), err_add() and the winner-against-the-others checks.  The bounds at scale 1 are some 1e-13 and the margins between scores
    some 1e-1 or exact ties, so a scale of 1e6 puts the comparisons of SOME templates inside the bounds (the issue's prototype: 20 % at 1e4, 100 % at 1e7, on deeper
    templates).  `uncertain` counts the templates a comparison flagged, whatever else flagged them; a certain() that always said yes would give 0, one that always said
    no every template.  The templates the comparisons let through are compared with the host form, segments and per-node scores (mismatches, score_violations)."""
    m = MANIFEST["oc2cns"]["default"]
    st, cns, raw = _run(checker, logs("default"), str(tmp_path), "1000000", "_mid")
    print(st)
    assert st["templates"] >= 90 and st["bad"] == 0
    assert 0 < st["uncertain"] < st["templates"]
    assert st["nodes"] > 10000 and st["score_violations"] == 0 and st["mismatches"] == 0 and st["violations"] == 0
    assert hashlib.md5(cns).hexdigest() == m["cns_md5"] and hashlib.md5(raw).hexdigest() == m["raw_md5"]


def test_checker_is_clean_under_sanitizers(logs, tmp_path):
    """the stand-alone checker once with -fsanitize=address,undefined (host code only)"""
    exe = os.path.join(str(tmp_path), "check_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    name = sorted(MANIFEST["oc2cns"])[0]
    st, _, _ = _run(exe, logs(name), str(tmp_path), "1", "_asan")
    assert st["mismatches"] == 0 and st["violations"] == 0


@pytest.mark.parametrize("shape", [dict(genome=40_000, coverage=35.0, seed=91, err=0.13, vol_size=500_000, min_cov=4),
                                   dict(genome=80_000, coverage=7.0, seed=77, err=0.12, vol_size=300_000, min_cov=3)], ids=["deep", "sparse"])
def test_fresh_inputs_of_the_gpu_tests_stay_under_the_fallback_cap(checker, tmp_path, shape):
    """the two fresh data sets of tests/test_gpu_cns_consensus.py through the model: at most 10 % of their templates flagged (the GPU tests' cap), the rest with the
    host's segments, every link weight and node score inside its bound"""
    shape = dict(shape)
    min_cov = shape.pop("min_cov")
    wrk, rs, nv = util.make_dataset(tmp_path, **shape)
    o = ora.options(**dict(util.FAST, job=0, binary_output=1, num_threads=4))
    rec = b""
    for v in range(nv):
        out = os.path.join(str(tmp_path), "pm_%d" % v)
        ora.pm_main(o, v, wrk, out)
        rec += open(out, "rb").read()
    can = os.path.join(str(tmp_path), "cands")
    open(can + ".p0", "wb").write(util.pcan_single_partition(rec))
    open(can + ".partitions", "w").write("1\n")
    co = ora.cns_options(min_cov=min_cov)
    log = os.path.join(str(tmp_path), "log")
    ora.cns_run(co, wrk, can, log, full=True)
    st, _, _ = _run(checker, (wrk, can, co, [], log), str(tmp_path), "1")
    print(st)
    assert st["templates"] > 40 and st["links"] > 100000
    assert st["flagged"] <= 0.1 * st["templates"]
    assert st["mismatches"] == 0 and st["violations"] == 0 and st["score_violations"] == 0
