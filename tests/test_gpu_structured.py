"""GPU parity on structured input (tests/structured.py): low-complexity, tie-heavy and threshold-edge sequence through the block kernels one by one, the
round launcher and the whole pipeline, everything bit-exact against the oracle (ident_perc is an exactly reproducible IEEE quotient, compared with ==).
tests/test_structured.py holds the conditions on the generators; the counts that keep a case from passing without its edge cases are asserted here too."""
import os

import numpy as np
import pytest

from tests import structured, util
from oracle import oracle_api as ora

pytestmark = pytest.mark.gpu

PATH_KNOBS = {
    "band": {},                                                                                 # k_myers_coop (8 / 16 lanes per block, unbanded) + band records + walk
    "band_lanes": {"NECAT_COOP_THRESHOLD": "0"},                                                # k_myers (a lane per block, the reference's banding) + the same walk
    "recompute": {"NECAT_BATCH_RC": "1", "NECAT_RC_WW": "2"},                                   # k_myers_ckg + k_rcwalk3, 32 diagonals
    "recompute_16": {"NECAT_BATCH_RC": "1", "NECAT_RC_WW": "2", "NECAT_RC3_BAND": "16"},         # .. 16 diagonals
    "recompute_rows": {"NECAT_BATCH_RC": "1", "NECAT_RC_WW": "1"},                               # k_myers_ckg + k_rcwalk2w
    "recompute_fast": {"NECAT_BATCH_RC": "2", "NECAT_RC_WW": "1"},                               # k_myers_ckf (fast_shw_ckr, unrolled windows) + k_rcwalk2w
    "recompute_fast_rolled": {"NECAT_BATCH_RC": "2", "NECAT_RC_WW": "1", "NECAT_CKR_FAST": "0"},
    "recompute_fast_chunks": {"NECAT_BATCH_RC": "2", "NECAT_RC_WW": "1", "NECAT_BATCH_CHUNK": "128"},
}


@pytest.fixture(scope="module")
def blocks(built):
    b = structured.concat_blocks(structured.structured_blocks(np.random.default_rng(structured.BLOCK_SEED)),
                                 structured.threshold_blocks(np.random.default_rng(structured.THRESHOLD_SEED)))
    return b, structured.reference_results(b, 0.5)


@pytest.mark.parametrize("path", list(PATH_KNOBS))
def test_structured_blocks_match_oracle(ctx, blocks, monkeypatch, path):
    """The block kernels in isolation (necat_edlib_align_batch, as test_edlib_blocks_match_oracle runs them) on homopolymers, tandem repeats, two-letter and mixed
    sequence, every boundary size, long single indels and blocks with d = k - 1 .. k + 2: refused iff the oracle refuses; distance, end row, end column and
    every op equal.  recompute_fast_chunks: the hook in chunks of 128 blocks (NECAT_BATCH_CHUNK), its per-chunk bookkeeping with base > 0."""
    for name, val in PATH_KNOBS[path].items():
        monkeypatch.setenv(name, val)
    b, ref = blocks
    seqs, qo, ql, to, tl, tag = b
    dist, qend, tend, ops, ops_off = ctx.edlib_align_batch(seqs, qo, ql, to, tl, 0.5)
    ran = ctx._xc if ctx._xc is not None else ctx            # the context the hook ran on
    for name, val in PATH_KNOBS[path].items():
        assert ran.knob(name) == val
    accepted = {off: 0 for off in structured.THRESHOLD_OFFSETS}
    refused = dict(accepted)
    for i, (ok, d, qe, te, oops) in enumerate(ref):
        off = structured.threshold_offset(tag[i])
        if not ok:
            assert dist[i] == -1, "%s: the oracle refuses the block (d > k), the kernel gives distance %d" % (tag[i], dist[i])
            if off is not None:
                refused[off] += 1
            continue
        assert dist[i] != -1, "%s: the oracle aligns the block at distance %d, the kernel refuses it" % (tag[i], d)
        assert (int(dist[i]), int(qend[i]), int(tend[i])) == (d, qe, te), "%s: (distance, qend, tend)" % tag[i]
        mine = ops[ops_off[i]:ops_off[i + 1]]
        assert np.array_equal(mine, oops), "%s: ops differ (first at %d of %d / %d)" % (
            tag[i], int(np.argmax(mine[:min(len(mine), len(oops))] != oops[:min(len(mine), len(oops))])), len(mine), len(oops))
        if off is not None:
            accepted[off] += 1
    assert accepted[-1] >= 10 and accepted[0] >= 10 and accepted[1] == accepted[2] == 0, accepted
    assert refused[1] >= 10 and refused[2] >= 10 and refused[-1] == refused[0] == 0, refused
    tm = ran.timings()
    assert ran.xcheck and tm.myers_word_updates > 0 and tm.myers_blocks == len(tag)
    nA = sum(1 for i in range(len(tag)) if ql[i] == 512 and tl[i] == 512)
    chunk = int(PATH_KNOBS[path].get("NECAT_BATCH_CHUNK", 65536))
    assert tm.myers_launches == -(-nA // chunk) + -(-(len(tag) - nA) // chunk)          # one per chunk of either shape
    if path == "recompute_fast_chunks":
        assert tm.myers_launches > 2 and nA > 2 * chunk and len(tag) - nA > 2 * chunk


# ---- the product library through the round launcher

ONC_KNOBS = ["", "NECAT_RCWALK=1 NECAT_TAIL_FUSED=0", "NECAT_RC_WW=2 NECAT_RCWALK=1 NECAT_TAIL_FUSED=0", "NECAT_FRAG_FUSE=0 NECAT_RCWALK=1 NECAT_TAIL_FUSED=0",
             "NECAT_CK_POST=0 NECAT_RCWALK=1 NECAT_TAIL_FUSED=0"]


@pytest.fixture(scope="module")
def onc_pairs(built):
    """the pairs, their candidate records and the oracle's onc_align of every anchor at tail-match lengths 4 and 1"""
    from necat_amd import capi
    pairs = structured.anchored_pairs(np.random.default_rng(4321), 40)
    seqs, rows = [], []
    for q, t, qdir, anchors in pairs:
        qid = len(seqs)
        seqs += [(3 - q[::-1]).astype(np.uint8) if qdir else q, t]          # the volume holds the forward strand
        rows += [(qid, qid + 1, qdir, qoff, toff, q, t) for qoff, toff in anchors]
    cands = np.zeros(len(rows), dtype=capi.CANDIDATE_DTYPE)
    for i, (qid, sid, qdir, qoff, toff, q, t) in enumerate(rows):
        cands[i]["qid"], cands[i]["sid"], cands[i]["qdir"] = qid, sid, qdir
        cands[i]["qsize"], cands[i]["ssize"], cands[i]["qoff"], cands[i]["soff"] = q.shape[0], t.shape[0], qoff, toff
    al = ora.Aligner(0.5)
    want = {tail: [al.align(q, qoff, t, toff, 500, tail) for (_, _, _, qoff, toff, q, t) in rows] for tail in (4, 1)}
    al.close()
    n_ok = sum(w[0] for ws in want.values() for w in ws)
    n_empty = sum(len(w[6]) == 0 for ws in want.values() for w in ws)
    assert n_ok > 100 and n_empty > 5, (n_ok, n_empty)
    return seqs, rows, cands, want


@pytest.mark.parametrize("knobs", ONC_KNOBS, ids=[k.replace(" ", ",") or "default" for k in ONC_KNOBS])
def test_onc_align_on_low_complexity(onc_pairs, monkeypatch, knobs):
    """necat_onc_align_batch of the PRODUCT library on pairs full of runs, anchors inside a run, at random places and at the ends, a run of the target longer or
    shorter than the query's: the default (every round of so short a list through k_tail_fused), and every round through k_myers_ck + the recomputing walk
    (k_rcwalk2w; NECAT_RC_WW=2: k_rcwalk3) with fragment fusion and the post-pass minimum on and off - (ok, coordinates, align_size, ident_perc) and both gapped strings"""
    from necat_amd import capi
    from necat_amd.synth import pack_2bit
    seqs, rows, cands, want = onc_pairs
    for kv in knobs.split():
        monkeypatch.setenv(*kv.split("="))
    assert not capi.needs_xcheck()
    c = capi.Context(0)          # knobs are read when a context is created
    try:
        assert not c.xcheck and all(c.knob(kv.split("=")[0]) == kv.split("=")[1] for kv in knobs.split())
        sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        vol = c.upload_volume(pack_2bit(np.concatenate(seqs)), int(sizes.sum()), offs, sizes)
        opt = capi.default_options(**dict(util.FAST, job=1, align_size_cutoff=500))
        for tail in (4, 1):
            aln, ops, off = c.onc_align_batch(vol, vol, 0, 0, cands, opt, tail)
            tm = c.timings()
            print("knobs [%s] tail %d: rounds %d, fused_blocks %d, rc_blocks %d, myers_word_updates %d" % (knobs, tail, tm.rounds, tm.fused_blocks, tm.rc_blocks, tm.myers_word_updates))
            assert tm.rounds >= 3 and tm.myers_word_updates > 0
            assert (tm.rc_blocks > 0) == bool(knobs) and (tm.fused_blocks > 0) == (not knobs)          # which kernels the rounds went through
            for i, (qid, sid, qdir, qoff, toff, q, t) in enumerate(rows):
                ok, a0, a1, b0, b1, ident, qa, ta = want[tail][i]
                a = aln[i]
                where = "pair %d anchor %d (%d, %d) of %d x %d, tail %d" % (i // 3, i % 3, qoff, toff, q.shape[0], t.shape[0], tail)
                assert (bool(a["ok"]), int(a["qoff"]), int(a["qend"]), int(a["toff"]), int(a["tend"]), int(a["align_size"]),
                        float(a["ident_perc"])) == (ok, a0, a1, b0, b1, len(qa), ident), where
                assert capi.gapped_strings(ops[int(off[i]):int(off[i + 1])], int(a["align_size"]), q, a0, t, b0) == (qa, ta), where
        vol.free()
    finally:
        c.close()


# ---- the whole pipeline

@pytest.fixture(scope="module")
def lowc_reads(tmp_path_factory, built):
    from necat_amd import synth
    G = structured.low_complexity_genome(60_000, 2, 0.6)
    rs = synth.simulate_reads(coverage=14.0, seed=2, err=0.15, genome=G)
    d = os.path.join(str(tmp_path_factory.mktemp("lowc")), "vols")
    assert synth.write_volume_dir(d, rs, 2_000_000) == 1
    return d, {}


PIPELINE = {
    "job0": (dict(util.FAST), 0, ""),
    "job1": (dict(util.FAST), 1, ""),
    "job0_k11_q50": (dict(util.FAST, kmer_size=11, kmer_cnt_cutoff=50), 0, ""),          # run k-mers on both sides of the -q cutoff
    "job1_k11_q50": (dict(util.FAST, kmer_size=11, kmer_cnt_cutoff=50), 1, ""),
    "job1_rcwalk": (dict(util.FAST), 1, "NECAT_RCWALK=1 NECAT_TAIL_FUSED=0"),           # every round through k_myers_ck + the recomputing walk
}


@pytest.mark.parametrize("job", list(PIPELINE))
def test_pipeline_on_low_complexity_reads(lowc_reads, tmp_path, monkeypatch, job):
    """pm_main on reads from a genome with homopolymer / repeat / two-letter runs of 20 - 400 bases: the 28-byte candidate records (job 0) and the M4 rows (job 1)
    equal the oracle's - seeding with low-complexity k-mers, tied DDF votes and full blocks of 40 seeds, extension through runs"""
    from necat_amd import capi
    d, cache = lowc_reads
    kw, jb, knobs = PIPELINE[job]
    key = (tuple(sorted(kw.items())), jb)
    if key not in cache:          # (the oracle's records once per option set)
        o = ora.options(**dict(kw, job=jb, binary_output=1))
        out = os.path.join(str(tmp_path), "oracle.out")
        st = ora.pm_main(o, 0, d, out)
        cache[key] = (ora.sorted_records(out, 28) if jb == 0 else np.frombuffer(open(out, "rb").read(), dtype=capi.M4_DTYPE), st.n_records)
    want, n_records = cache[key]
    for kv in knobs.split():
        monkeypatch.setenv(*kv.split("="))
    assert not capi.needs_xcheck()
    c = capi.Context(0)          # knobs are read when a context is created
    try:
        cands, m4 = capi.pm_main(c, capi.default_options(**dict(kw, job=jb, binary_output=1)), 0, d)
        tm = c.timings()
    finally:
        c.close()
    assert cands.shape[0] > 500
    if jb == 0:
        mine = sorted(bytes(r) for r in capi.pack_candidates(cands).astype("<u4"))
        assert len(mine) == n_records
        assert mine == want
    else:
        assert m4.shape[0] == want.shape[0] == n_records
        assert util.m4_key_rows(m4) == util.m4_key_rows(want)
        assert tm.rounds >= 3 and tm.myers_word_updates > 0 and (not knobs or tm.rc_blocks > 0)
