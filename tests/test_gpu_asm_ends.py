"""necat_asm_map_batch (oc2asmpm from the anchor to the record on the device: block aligner, DALIGNER's end extension of hbn_map_extend, fix_ident_perc, the record)
against the host code: the alignments of necat_asm_align_batch on the same context (pinned to the oracle by tests/test_gpu_zz_asm_align.py) put through
asm_core.h's Extender::ends (tests/host_core/asm_ends_capi.cpp, built here with g++) and assembled into records in Python.  Then the program: oc2asmpm with
NECAT_ASM_ENDS_DEVICE=1 against the committed golden records and against the reference's own oc2asmpm."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from necat_amd import build, capi, synth
from necat_amd.synth import _mutate, pack_2bit
from oracle import oracle_api as ora
from tests import util

REF_ASMPM = os.path.join(os.path.dirname(ora.REF_PMOV), "oc2asmpm")
pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not os.path.exists(REF_ASMPM), reason="needs oracle/_ref/oc2asmpm")

SIDES = ("left", "right")

# Ends that the host code tries and DECLINES: (read, subject) prefixes that end in a run of 8 equal bases, and suffixes that begin with one, found by a hill climb
# on rescue::Dalign's identity (the unrelated parts are of low complexity on nearly disjoint letters: the wave meets a sequence end on a path of more differences
# than half its bases, so daligner.c's identity is below 0).  Random unrelated ends never do that.
DECLINED_LEFT = [
    ("TTCCTTAAATTTAATTTTTTATTTAGATCGTAAGT", "CGGGACGGGAGAAGGGCGGCGCGCGCGCGGCGCCCTCGTAAGT"),
    ("TGGCAACGAAAAAAAAAAAAAAAAAACAAAAGACCGTATCA", "TTCAGCCGGGTCTCTTTTCCCCTCCTGTGGTCCCCGTATCA"),
    ("TAAAAAAATAAAAAACCCCCCCAGCCCTCAACAAA", "AACCCGACAATCCCTCATTTCCGGGCGGGGGGGGGGTATTTCAACAAA"),
    ("CCTTCATAGGCCAAAAGGCAAACGGAAAAAGGAGGGCGCGATAGTTGCA", "CTTTTTTTTCCTTTTTTTTTAATATAACTAGTTGCA"),
    ("TCGCGCCACCTTCGGATTGGCCGGGGGGGGGGCGTGGGGGGGGTGTCCCAGTGG", "TAAAAATAAAAAACAACAACACAACCCAGTGG"),
]
DECLINED_RIGHT = [
    ("CCAGAGAATTGGTGGGGTGGGTGGGGGAGAGGGTATCC", "CCAGAGAACACCAAACCAACAAACACCCCCTCTC"),
    ("TAAACCTCAGCAACAAACCCCACCACACACTT", "TAAACCTCTTTGGTGTGGTGGGGGCGGGGCGGCAGCACCGATAG"),
    ("TAGACGCTCCAACAAAAAAAACAACAAAGAATATTCTTAGAGAC", "TAGACGCTAGGTTTGTGTTTTGGTTGGTTGGCCG"),
    ("AGTAATCAAATTTTGGGGTGTTGTTGTTTGGCTGTTGGTGTTGCCG", "AGTAATCAGCGCGCCCCCCCCCCCCCCCCCCA"),
    ("CGGGCGAAAGTTTGGGGTTTTTTTTTTTTTTTCCTTA", "CGGGCGAACACCAACAAAGCAGCGCACGAGGCTGCGCGGGTGGCG"),
]


def make_pairs():
    """About 100 pairs of 1.5 - 12 kb, three anchors each, the subject on either strand: (sequences as the volume stores them, rows, plans).
    rows[i] = (q, t on its strand, sdir) of plans[i].  Kinds: the same stretch twice (the aligner stops a few bases short of both ends: small hangs), overlap-shaped and
    contained pairs (no hang where a sequence ends), unrelated prefixes / suffixes of 20 - 299 bases at one or both ends, of 301 - 900 bases, unrelated pairs,
    pairs of low identity, entries without a chain (qoff < 0), and ten pairs with an end of DECLINED_LEFT / DECLINED_RIGHT."""
    rng = np.random.default_rng(20251)
    junk = lambda lo, hi: rng.integers(0, 4, int(rng.integers(lo, hi + 1)), dtype=np.uint8)
    seqs, rows, plans = [], [], []
    for it in range(104):
        g = rng.integers(0, 4, int(rng.integers(1500, 12000)), dtype=np.uint8)
        e = float(rng.uniform(0.005, 0.06))
        kind = it % 13
        a, b = g, g
        if kind in (1, 2):          # overlap-shaped: the read's tail on the subject's head (1), the other way round (2)
            cut = int(g.shape[0] * rng.uniform(0.2, 0.5))
            a, b = (g[cut:], g[:g.shape[0] - cut // 2]) if kind == 1 else (g[:g.shape[0] - cut // 2], g[cut:])
        if kind == 3:               # contained
            a = g[g.shape[0] // 4: g.shape[0] - g.shape[0] // 5]
        q, t = _mutate(a, e, rng), _mutate(b, e, rng)
        qa0 = ta0 = 0               # where the related part starts
        if kind in (4, 5, 6, 7, 8):     # unrelated ends of 20 - 299 bases: both sides (4 - 6), left only (7), right only (8)
            if kind != 8:
                jq, jt = junk(20, 299), junk(20, 299)
                q, t, qa0, ta0 = np.concatenate([jq, q]), np.concatenate([jt, t]), jq.shape[0], jt.shape[0]
            if kind != 7:
                q, t = np.concatenate([q, junk(20, 299)]), np.concatenate([t, junk(20, 299)])
        if kind == 9:               # overhangs above 300
            jq, jt = junk(301, 900), junk(301, 900)
            q, t, qa0, ta0 = np.concatenate([jq, q, junk(301, 900)]), np.concatenate([jt, t, junk(301, 900)]), jq.shape[0], jt.shape[0]
        if kind == 10:              # unrelated
            t = rng.integers(0, 4, t.shape[0], dtype=np.uint8)
        if kind == 11:              # far apart: few equal columns
            q, t = _mutate(a, 0.30, rng), _mutate(b, 0.30, rng)
        sdir = it & 1
        stored_t = (3 - t[::-1]).astype(np.uint8) if sdir else t       # the volume holds the forward strand; the alignment sees strand sdir = t
        qid, sid = len(seqs), len(seqs) + 1
        seqs += [q, stored_t]
        related_q, related_t = q.shape[0] - qa0, t.shape[0] - ta0
        for j in range(3):
            frac = float(rng.uniform(0.1, 0.9))
            if kind in (1, 2, 3):   # (an anchor inside the part the two share)
                qoff, soff = int(frac * (q.shape[0] - 1)), int(frac * (t.shape[0] - 1))
                if kind == 1:
                    qoff = int(frac * 0.3 * q.shape[0]); soff = min(t.shape[0] - 1, cut + qoff)
                if kind == 2:
                    soff = int(frac * 0.3 * t.shape[0]); qoff = min(q.shape[0] - 1, cut + soff)
                if kind == 3:
                    soff = min(t.shape[0] - 1, g.shape[0] // 4 + qoff)
            else:
                span = min(related_q, related_t) - (600 if kind in (4, 5, 6, 8, 9) else 0)
                qoff, soff = qa0 + int(frac * max(1, span)), ta0 + int(frac * max(1, span))
            if kind == 12 and j == 1:
                qoff, soff = -1, -1         # no chain: the entry is skipped
            plans.append((qid, sid, sdir, qoff, soff, 100 + it * 3 + j, t.shape[0]))
            rows.append((q, t, sdir))
    # the declined ends: the literal end on both sequences, 20 bases copied exactly next to its run of 8 (the alignment ends at that run), then the related rest
    codes = lambda text: np.array(["ACGT".index(c) for c in text], dtype=np.uint8)
    for it, (side, (eq, et)) in enumerate([(0, e) for e in DECLINED_LEFT] + [(1, e) for e in DECLINED_RIGHT]):
        g = rng.integers(0, 4, int(rng.integers(1500, 4000)), dtype=np.uint8)
        exact = rng.integers(0, 4, 20, dtype=np.uint8)
        rq, rt = _mutate(g, 0.03, rng), _mutate(g, 0.03, rng)
        if side == 0:
            q, t = np.concatenate([codes(eq), exact, rq]), np.concatenate([codes(et), exact, rt])
        else:
            q, t = np.concatenate([rq, exact, codes(eq)]), np.concatenate([rt, exact, codes(et)])
        sdir = it & 1
        qid, sid = len(seqs), len(seqs) + 1
        seqs += [q, (3 - t[::-1]).astype(np.uint8) if sdir else t]
        for j in range(3):
            at = int((0.2 + 0.3 * j) * g.shape[0])
            qoff, soff = (len(eq) + 20 + at, len(et) + 20 + at) if side == 0 else (at, at)
            plans.append((qid, sid, sdir, qoff, soff, 500 + it * 3 + j, t.shape[0]))
            rows.append((q, t, sdir))
    return seqs, rows, np.array(plans, dtype=capi.ASM_PLAN_DTYPE)


@pytest.fixture(scope="module")
def ends_lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("asm_ends")), "asm_ends_capi.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(util.ROOT, "tests", "host_core", "asm_ends_capi.cpp")], check=True)
    lib = C.CDLL(so)
    lib.mine_asm_ends.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.mine_asm_ends.restype = None
    return lib


def host_records(lib, rows, plans, aligned):
    """The records and the branch counts of the host code.  aligned(k) for the k-th entry with an anchor: (ok, qoff, qend, toff, tend, ident, qaln, taln)."""
    recs = np.zeros(plans.shape[0], dtype=capi.M4_DTYPE)
    kept = np.zeros(plans.shape[0], dtype=np.uint8)
    n = dict(anchors=0, ok=0, low_ident=0, both=0, strands=set(), tried=[0, 0], extended=[0, 0], hang0=[0, 0], hang_long=[0, 0])
    for i, ((q, t, sdir), p) in enumerate(zip(rows, plans)):
        if p["qoff"] < 0:
            continue
        ok, a0, a1, b0, b1, ident, qa, ta = aligned(n["anchors"])
        n["anchors"] += 1
        if not ok:
            continue
        n["ok"] += 1
        if not ident >= 65.0:
            n["low_ident"] += 1
            continue
        for side, hang in enumerate((min(a0, b0), min(q.shape[0] - a1, t.shape[0] - b1))):
            n["hang0"][side] += hang == 0
            n["hang_long"][side] += hang > 300
            n["tried"][side] += 0 < hang <= 300
        io = (C.c_int * 6)(a0, a1, b0, b1, 0, 0)
        idp = C.c_double(ident)
        qc, tc = np.ascontiguousarray(q), np.ascontiguousarray(t)
        lib.mine_asm_ends(qc.ctypes.data, qc.shape[0], tc.ctypes.data, tc.shape[0], qa, ta, len(qa), io, C.byref(idp))
        n["extended"][0] += io[4]
        n["extended"][1] += io[5]
        n["both"] += io[4] and io[5]
        if io[4] or io[5]:
            n["strands"].add(sdir)
        soff, send = (io[2], io[3]) if not sdir else (t.shape[0] - io[3], t.shape[0] - io[2])
        recs[i] = (p["qid"], 0, io[0], io[1], p["qoff"], q.shape[0], p["sid"], sdir, soff, send, p["soff"], t.shape[0], idp.value, p["score"], 0)
        kept[i] = 1
    return recs, kept, n


def upload(ctx, seqs):
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return ctx.upload_volume(pack_2bit(np.concatenate(seqs)), int(sizes.sum()), offs, sizes)


@pytest.fixture(scope="module")
def case(ctx, ends_lib):
    """the pairs and what the host code makes of them: the alignments of necat_asm_align_batch through Extender::ends, once for all tests"""
    seqs, rows, plans = make_pairs()
    vol = upload(ctx, seqs)
    with_anchor = plans[plans["qoff"] >= 0]
    anchors = np.zeros(with_anchor.shape[0], dtype=capi.ASM_ANCHOR_DTYPE)
    for f in capi.ASM_ANCHOR_DTYPE.names:
        anchors[f] = with_anchor[f]
    aln, ops, off = ctx.asm_align_batch(vol, vol, 0, 0, anchors, 0.5, 400)
    live = [r for r, p in zip(rows, plans) if p["qoff"] >= 0]

    def aligned(k):
        a, (q, t, _) = aln[k], live[k]
        qa, ta = capi.gapped_strings(ops[int(off[k]):int(off[k + 1])], int(a["align_size"]), q, int(a["qoff"]), t, int(a["toff"]))
        return bool(a["ok"]), int(a["qoff"]), int(a["qend"]), int(a["toff"]), int(a["tend"]), float(a["ident_perc"]), qa, ta

    recs, kept, counts = host_records(ends_lib, rows, plans, aligned)
    vol.free()
    return seqs, plans, recs, kept, counts


def check_coverage(plans, counts):
    """what the data reaches, counted by the host code alone"""
    assert (plans["qoff"] < 0).sum() >= 5
    for side in range(2):
        assert counts["extended"][side] >= 20, (SIDES[side], counts)
        assert counts["hang0"][side] >= 5 and counts["hang_long"][side] >= 5, (SIDES[side], counts)
    assert counts["both"] >= 10 and counts["strands"] == {0, 1}, counts
    assert counts["low_ident"] >= 1 and counts["anchors"] - counts["ok"] >= 5, counts


def same_records(got, kept, want, want_kept):
    assert np.array_equal(kept, want_kept)
    for f in capi.M4_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f


def check_stats(st, counts):
    assert (st.n_anchors, st.n_ok, st.n_low_ident) == (counts["anchors"], counts["ok"], counts["low_ident"])
    for side in range(2):
        assert (st.n_tried[side], st.n_extended[side], st.n_hang0[side], st.n_hang_long[side]) == \
               (counts["tried"][side], counts["extended"][side], counts["hang0"][side], counts["hang_long"][side]), SIDES[side]
    # (the block aligner trims every alignment to a run of 8 equal columns at both ends: a tried end always has its job)
    assert st.n_no_run[0] == 0 and st.n_no_run[1] == 0
    assert st.n_jobs == counts["tried"][0] + counts["tried"][1] == st.n_tier1 + st.n_tier2 + st.n_host
    assert sum(st.diag_hist) == st.n_jobs and st.n_steps > 0 and st.max_diags >= 1


def test_records_against_host_code(ctx, case):
    seqs, plans, want, want_kept, counts = case
    check_coverage(plans, counts)
    vol = upload(ctx, seqs)
    recs, kept, st = ctx.asm_map_batch(vol, vol, 0, 0, plans, 0.5, 400, 65.0)
    vol.free()
    same_records(recs, kept, want, want_kept)
    check_stats(st, counts)
    assert st.n_host == 0                                   # at the default capacities
    assert st.max_diags <= int(ctx.knob("NECAT_DALIGN_DIAGS"))
    print("asm ends: jobs %d, tier 1 %d, tier 2 %d, widest window %d, histogram %s" % (st.n_jobs, st.n_tier1, st.n_tier2, st.max_diags, list(st.diag_hist)))


def test_pairs_reach_a_declined_end(case):
    """At least 3 ends per side that are tried and NOT extended, counted by the host code: the pairs of DECLINED_LEFT / DECLINED_RIGHT.  (Unrelated random ends do
    not get there: 0 of 312 on the other pairs here, 0 of 526 on tests/golden/vols_d, 0 of 612 000 searched random, repetitive and edited-copy ends - behind a run of
    8 equal bases DALIGNER declines only when a path of more differences than half its bases meets a sequence end.)"""
    counts = case[4]
    for side in range(2):
        assert counts["tried"][side] - counts["extended"][side] >= 3, (SIDES[side], counts)


def test_small_capacities(case, monkeypatch):
    """4 diagonals, then 16, then the host code: the same bytes (tests/host_core/check_asm_ends.cpp runs its crafted ends at these two capacities and finds jobs in all
    three tiers, with the same answers)"""
    seqs, plans, want, want_kept, counts = case
    monkeypatch.setenv("NECAT_ASM_ENDS_DIAGS", "4")
    monkeypatch.setenv("NECAT_DALIGN_DIAGS", "16")
    small = capi.Context(0)          # knobs are read when a context is created
    assert int(small.knob("NECAT_ASM_ENDS_DIAGS")) == 4 and int(small.knob("NECAT_DALIGN_DIAGS")) == 16
    vol = upload(small, seqs)
    recs, kept, st = small.asm_map_batch(vol, vol, 0, 0, plans, 0.5, 400, 65.0)
    vol.free()
    small.close()
    same_records(recs, kept, want, want_kept)
    check_stats(st, counts)
    assert st.n_tier1 > 0 and st.n_tier2 > 0 and st.n_host > 0, (st.n_tier1, st.n_tier2, st.n_host)


def test_arguments(ctx, case):
    seqs, plans = case[0], case[1]
    vol = upload(ctx, seqs)
    live = plans[plans["qoff"] >= 0]
    bad = live[:1].copy()
    bad["sdir"] = 2
    with pytest.raises(capi.NecatError):
        ctx.asm_map_batch(vol, vol, 0, 0, bad)
    bad = live[:1].copy()
    bad["qoff"] = 10 ** 8
    with pytest.raises(capi.NecatError):
        ctx.asm_map_batch(vol, vol, 0, 0, bad)
    bad = live[:1].copy()
    bad["sid"] = len(seqs)
    with pytest.raises(capi.NecatError):
        ctx.asm_map_batch(vol, vol, 0, 0, bad)
    with pytest.raises(capi.NecatError):
        ctx.asm_map_batch(vol, vol, 0, 0, live[:1], error=0.0)
    recs, kept, st = ctx.asm_map_batch(vol, vol, 0, 0, plans[:0])
    assert recs.shape[0] == 0 and kept.shape[0] == 0 and st.n_anchors == 0 and st.n_jobs == 0
    skipped = live[:2].copy()
    skipped["qoff"] = -1            # nothing but skipped entries: no record, no kernel
    recs, kept, st = ctx.asm_map_batch(vol, vol, 0, 0, skipped)
    assert kept.tolist() == [0, 0] and not recs.tobytes().strip(b"\0") and st.n_anchors == 0
    vol.free()


def trace_of(stderr):
    """the counters of the program's "ends on the device" lines, summed over the volume pairs"""
    tot = {}
    for ln in stderr.splitlines():
        if "ends on the device:" in ln:
            for k, v in re.findall(r"(\w+)=(\d+)(?=[ +])", ln):
                tot[k] = tot.get(k, 0) + int(v)
    return tot


def test_program_golden(built, tmp_path):
    """oc2asmpm with NECAT_ASM_ENDS_DEVICE=1 on tests/golden/vols_d: the committed bytes (what the reference's oc2asmpm wrote)"""
    built.build_cli()
    m = json.load(open(os.path.join(util.GOLDEN, "manifest_asm_rm.json")))["asm_d"]
    wrk = util.install_golden_volumes(m["volumes"], tmp_path)
    seen = {}
    for v in range(m["n_volumes"]):
        got = os.path.join(str(tmp_path), "mine_%d.m4" % v)
        r = subprocess.run([build.OC2ASMPM] + m["args"].split() + ["-t", "3", wrk, str(v), got], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, NECAT_ASM_ENDS_DEVICE="1", NECAT_CLI_TRACE="1"))
        assert r.returncode == 0, r.stderr
        assert open(got, "rb").read() == open(os.path.join(util.GOLDEN, "asm_d", "ref_v%d.m4" % v), "rb").read(), v
        for k, n in trace_of(r.stderr).items():
            seen[k] = seen.get(k, 0) + n
    assert seen.get("calls", 0) >= m["n_volumes"] and seen["jobs"] > 400 and seen["host"] == 0 and seen["jobs"] == seen["tier1"] + seen["tier2"], seen


@needs_ref
@pytest.mark.parametrize("seed,err,repeat,indels,args", [
    (61, 0.03, 0.3, False, "-n 100 -z 10 -b 2000 -e 0.5 -j 1 -u 0 -a 400 -k 13"),      # necat.pl:36 (ASM_OVLP_OPTIONS)
    (62, 0.06, 0.4, True, "-z 5 -k 12 -n 20 -u 1"),                                     # TRIM_OVLP_OPTIONS write binary records (-u 1)
])
def test_program_reproduces_reference(built, tmp_path, seed, err, repeat, indels, args):
    """the two synthetic sets of tests/test_gpu_asmpm.py with the ends decided on the device, against the reference's own oc2asmpm -t 1"""
    built.build_cli()
    rs = synth.simulate_reads(40_000, 10.0, seed=seed, err=err, repeat_frac=repeat)
    if indels:
        rs = synth.add_long_indels(rs, 0.3, seed=seed + 1)
    wrk = os.path.join(str(tmp_path), "vols")
    nv = synth.write_volume_dir(wrk, rs, 200_000)
    assert nv >= 2
    total = jobs = 0
    for v in range(nv):
        want, got = os.path.join(str(tmp_path), "ref_%d.m4" % v), os.path.join(str(tmp_path), "mine_%d.m4" % v)
        subprocess.run([REF_ASMPM] + args.split() + ["-t", "1", wrk, str(v), want], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        env = dict(os.environ, NECAT_ASM_ENDS_DEVICE="1", NECAT_CLI_TRACE="1")
        if v == 0 and seed == 62:
            env["NECAT_ASM_CALL_ANCHORS"] = "70"            # once with many small calls
        r = subprocess.run([build.OC2ASMPM] + args.split() + ["-t", "4", wrk, str(v), got], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        assert r.returncode == 0, r.stderr
        tr = trace_of(r.stderr)
        assert tr.get("calls", 0) >= nv - v and "end extension + records" not in r.stderr, r.stderr      # the device path decided the ends
        if "NECAT_ASM_CALL_ANCHORS" in env:
            assert tr["calls"] > 2 * (nv - v)
        jobs += tr["jobs"]
        a, b = open(want, "rb").read(), open(got, "rb").read()
        if "-u 1" in args:          # the reference leaves the records' 4 padding bytes uninitialised
            x, y = np.frombuffer(b, dtype=capi.M4_DTYPE), np.frombuffer(a, dtype=capi.M4_DTYPE)
            assert x.shape == y.shape
            for f in capi.M4_DTYPE.names:
                if not f.startswith("_"):
                    assert (x[f] == y[f]).all(), (v, f)
            total += x.shape[0]
        else:
            assert a == b, v
            total += len(a.splitlines())
    assert total > 300 and jobs > 100
