"""CPU test of oc2cns's job (necat_amd/csrc/cns_job.h: the read set, the units, their source, the hand-off one unit ahead, the consumer) through
tests/host_core/check_cns_job.cpp: the SOURCE of that header compiled with g++ against a fake C ABI, a stand-alone program built plainly, with
-fsanitize=thread and with -fsanitize=address,undefined.  The fake gathers for real on the host, groups records by template, sleeps in the extension and the
consensus call and logs contexts and concurrency; the consensus returns the read's own bases from the volume it was handed for every template whose length is no
multiple of 3, and the record text is the real cns_consensus.h - so a wrong local id, a wrong volume or a wrong order changes bytes.

The project: 40 reads of 200 .. 2000 bases in 3 volumes; 3 partitions of crafted 28-byte records - partition 0 has templates with no records of their own inside
its id range (they go out uncorrected with -s 0), partition 1 is empty, partition 2 has a template whose reads alone pass the chunk bound.  The checker asserts:
  (a) both files are the same bytes merged, gathered with a bound that gives >= 3 chunks per partition and with bound 1 (every template a chunk), each with the
      pipeline on and off and -t 1 / 3; -s 1: merged = gather and no uncorrected read; -mn 0 2 + -mn 1 2 hold the whole run's records;
  (b) units reach the consumer in (partition, chunk) order; never more than 2 gathered volumes nor more than 2 units' result blocks alive;
  (c) pipeline on: an extension call overlaps a consensus call, producer-side calls on the first context, consensus calls on the second; off: one context;
  (d) a failing extension (first, middle, last unit), gather, partition load, consensus call, a missing .p<i>, a record naming a read outside the project, a bad
      mode, each with the pipeline on and off, and a second context that cannot be made: 1, the error printed once, the call returns (the subprocess has a
      timeout: a lost wake-up fails), nothing left alive.  With the pipeline off no second context is asked for, so that injection must leave the run intact;
  (e) after every run every counter of live contexts, volumes and blocks is zero."""
import os
import subprocess

import numpy as np
import pytest

from tests import util
from necat_amd import synth

SRC = os.path.join(util.ROOT, "tests", "host_core", "check_cns_job.cpp")
BOUND = 6000            # chunk bound of the ">= 3 chunks" legs, in bases
N_ERRORS = 2 * 14 + 1   # injected failures per pipeline setting + the second context (pipeline on only): each printed once


def _project(tmp):
    rng = np.random.default_rng(11)
    sizes = rng.integers(200, 2001, 40).astype(np.int64)
    sizes[2], sizes[4], sizes[31] = 1000, 1998, 1500          # not examined (x 5) / examined without a segment, one raw interval (x 3) / both
    sizes[1], sizes[28] = 1001, 1801                          # one segment spanning the read
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    rs = synth.ReadSet(rng.integers(0, 4, int(sizes.sum())).astype(np.uint8), offsets, sizes, ["read_%d/x" % i for i in range(40)])
    d = os.path.join(tmp, "vols")
    assert synth.write_volume_dir(d, rs, vol_size=int(sizes.sum()) // 3 + 1) == 3

    def rec(sid, qid, score):
        qe, se = int(sizes[qid]), int(sizes[sid])
        return [(int(rng.integers(0, 2)) << 30) | score, sid, se // 10, se - se // 10, qid, qe // 8, qe - qe // 8]

    # partition p: the templates of [14 p, 14 p + 14) (oc2pcan's rule), records in no particular order, queries from all volumes
    parts = [[], [], []]
    for sid in (1, 2, 4, 5, 8, 9, 12):                        # 3, 6, 7, 10, 11 lie inside the id range without records of their own
        parts[0] += [rec(sid, int(q), 100 + k) for k, q in enumerate(rng.choice([i for i in range(40) if i != sid], 3, replace=False))]
    for sid in (28, 30, 31, 35, 37, 38):
        parts[2] += [rec(sid, int(q), 200 + k) for k, q in enumerate(rng.choice([i for i in range(40) if i != sid], 3, replace=False))]
    big = [int(q) for q in rng.choice([i for i in range(40) if i != 33], 15, replace=False)]
    parts[2] += [rec(33, q, 300 + k) for k, q in enumerate(big)]
    assert sizes[33] + sum(int(sizes[q]) for q in big) > BOUND          # template 33's reads alone pass the bound
    can = os.path.join(tmp, "candidates")
    with open(can + ".partitions", "w") as f:
        f.write("3\n")
    for p, recs in enumerate(parts):
        a = np.array(recs, dtype="<u4").reshape(-1, 7)
        rng.shuffle(a, axis=0)
        a.tofile("%s.p%d" % (can, p))
    return d, can


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    return _project(str(tmp_path_factory.mktemp("cns_job")))


@pytest.mark.parametrize("san", ["plain", "thread", "address,undefined"])
def test_cns_job_with_a_fake_library(project, tmp_path, san):
    d, can = project
    flags = [] if san == "plain" else ["-fsanitize=" + san, "-fno-omit-frame-pointer"] + (["-fno-sanitize-recover=undefined"] if "undefined" in san else [])
    exe = os.path.join(str(tmp_path), "check_cns_job")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exe, SRC, "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if san != "plain" and r.returncode != 0 and ("tsan" in r.stdout.lower() or "asan" in r.stdout.lower() or "ubsan" in r.stdout.lower()):
        pytest.skip("no %s sanitizer runtime in this toolchain" % san)
    assert r.returncode == 0, r.stdout[-3000:]
    run = lambda **env: subprocess.run([exe, d, can, os.path.join(str(tmp_path), "out"), str(BOUND)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", **env))
    r = run()
    if "LeakSanitizer has encountered a fatal error" in r.stderr:          # where the leak checker itself cannot run (no ptrace): the fake's counters still count every object
        r = run(ASAN_OPTIONS="detect_leaks=0")
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("ok errors=%d" % N_ERRORS)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stderr.count("[oc2cns] ERROR: ") == N_ERRORS
