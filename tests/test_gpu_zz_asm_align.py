"""necat_asm_align_batch through the C ABI against the oracle's onc_align at block size 2048 / tail match length 8 (= asm_pm/blockwise_edlib.c, which
tests/test_asmpm.py pins to the reference's own oc2asmpm): anchors anywhere in the overlap, at the sequence ends, on unrelated sequences, subjects on
both strands, reads of corrected and of raw quality."""
import numpy as np
import pytest

from necat_amd import capi
from necat_amd.synth import _mutate, pack_2bit
from oracle import oracle_api as ora

pytestmark = pytest.mark.gpu


def arbitrary_anchor_pairs():
    """60 read pairs with three anchors each: (sequences as the volume holds them, rows of (qid, sid, sdir, qoff, soff, query, subject strand))"""
    rng = np.random.default_rng(654)
    seqs, rows = [], []
    for it in range(60):
        g = rng.integers(0, 4, int(rng.integers(1500, 12000)), dtype=np.uint8)
        e = float(rng.uniform(0.005, 0.06)) if it % 4 else float(rng.uniform(0.10, 0.16))
        q = _mutate(g, e, rng)
        t = _mutate(g, e, rng)
        if it % 9 == 4:
            t = rng.integers(0, 4, t.shape[0], dtype=np.uint8)
        sdir = it & 1
        stored_t = (3 - t[::-1]).astype(np.uint8) if sdir else t       # the volume holds the forward strand; the alignment sees strand sdir = t
        qid, sid = len(seqs), len(seqs) + 1
        seqs += [q, stored_t]
        for _ in range(3):
            frac = float(rng.uniform(0.0, 1.0)) if it % 5 else float(rng.integers(0, 2))
            rows.append((qid, sid, sdir, int(frac * (q.shape[0] - 1)), int(frac * (t.shape[0] - 1)), q, t))
    return seqs, rows


@pytest.mark.parametrize("impl", ["cooperative", "band", "lane"])
def test_asm_align_arbitrary_anchors(ctx, monkeypatch, impl):
    """cooperative: the default path (asm_coop.h - the extension stage's round structure at the 2048-bp geometry, blocks through the
    checkpoint pass + recomputing walk of ext_rcwalk.h); band: the same rounds through the two-pass kernel + band records + wave walk
    (NECAT_ASM_RC=0); lane: the lane-per-alignment kernel they replaced, kept as a further implementation (NECAT_ASM_LANE=1)"""
    own = None
    if impl != "cooperative":
        monkeypatch.setenv("NECAT_ASM_LANE" if impl == "lane" else "NECAT_ASM_RC", "1" if impl == "lane" else "0")
        own = ctx = capi.Context(0)          # knobs are read when a context is created
    seqs, rows = arbitrary_anchor_pairs()
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    vol = ctx.upload_volume(pack_2bit(np.concatenate(seqs)), int(sizes.sum()), offs, sizes)
    anchors = np.zeros(len(rows), dtype=capi.ASM_ANCHOR_DTYPE)
    for i, (qid, sid, sdir, qoff, soff, q, t) in enumerate(rows):
        anchors[i] = (qid, sid, sdir, qoff, soff)
    aln, ops, off = ctx.asm_align_batch(vol, vol, 0, 0, anchors, 0.5, 400)
    al = ora.Aligner(0.5)
    n_ok = n_empty = 0
    for i, (qid, sid, sdir, qoff, soff, q, t) in enumerate(rows):
        ok, a0, a1, b0, b1, ident, qa, ta = al.align(q, qoff, t, soff, 400, 8, block_size=2048)
        a = aln[i]
        got = (bool(a["ok"]), int(a["qoff"]), int(a["qend"]), int(a["toff"]), int(a["tend"]), int(a["align_size"]), float(a["ident_perc"]))
        assert got == (ok, a0, a1, b0, b1, len(qa), ident), i
        assert capi.gapped_strings(ops[int(off[i]):int(off[i + 1])], int(a["align_size"]), q, a0, t, b0) == (qa, ta), i
        n_ok += ok
        n_empty += len(qa) == 0
    al.close()
    assert n_ok > 100 and n_empty > 5
    # arguments: a strand that is neither 0 nor 1, an anchor outside its read, no anchors at all
    bad = anchors[:1].copy()
    bad["sdir"] = 2
    with pytest.raises(capi.NecatError):
        ctx.asm_align_batch(vol, vol, 0, 0, bad)
    bad = anchors[:1].copy()
    bad["qoff"] = 10 ** 8
    with pytest.raises(capi.NecatError):
        ctx.asm_align_batch(vol, vol, 0, 0, bad)
    aln, ops, off = ctx.asm_align_batch(vol, vol, 0, 0, anchors[:0])
    assert aln.shape[0] == 0 and off.shape[0] == 1
    if impl != "lane":
        tm = ctx.timings()
        assert tm.rounds >= 1 or len(rows) == 0          # (the empty call above ran no round; the counters are the last non-empty call's only if > 0)
    vol.free()
    if own is not None:
        own.close()


def test_asm_align_through_several_checkpoint_chunks(ctx, monkeypatch):
    """The cooperative path with list A of round 0 longer than its checkpoint pool holds: NECAT_ASM_RC_POOL_MB=256 (the knob's minimum) is
    (256 MB / 81 920 B per 2048 x 2048 block) & ~63 = 3 264 work indices per launch of the pass + walk.  The pairs of the test above with 64 anchors each;
    a task's first block extends to the LEFT of its anchor (ext_init: ext_q = qoff, ext_t = soff) and is a full 2048 x 2048 block when at least
    2048 + 100 bases lie there in both sequences (ext_plan<2048>), so the anchors of every pair long enough are placed that far in: more than 3 264 full blocks in
    round 0, two chunks.  Per anchor the oracle's result, and the same bytes as a context at the default pool (one chunk)."""
    full_left, per_chunk = 2048 + 100, ((256 << 20) // 81920) & ~63
    rng = np.random.default_rng(654)
    seqs, rows = [], []
    for it in range(60):
        g = rng.integers(0, 4, int(rng.integers(1500, 12000)), dtype=np.uint8)
        e = float(rng.uniform(0.005, 0.06)) if it % 4 else float(rng.uniform(0.10, 0.16))
        q = _mutate(g, e, rng)
        t = _mutate(g, e, rng)
        if it % 9 == 4:
            t = rng.integers(0, 4, t.shape[0], dtype=np.uint8)
        sdir = it & 1
        stored_t = (3 - t[::-1]).astype(np.uint8) if sdir else t
        qid, sid = len(seqs), len(seqs) + 1
        seqs += [q, stored_t]
        short = min(q.shape[0], t.shape[0]) - 1
        fmin = (full_left + 2) / short if short >= full_left + 150 else 0.0      # (a pair too short for a full block keeps anchors anywhere)
        for j in range(64):
            frac = 1.0 if (it % 5 == 0 and j == 0) else float(rng.uniform(fmin, 1.0))
            rows.append((qid, sid, sdir, int(frac * (q.shape[0] - 1)), int(frac * (t.shape[0] - 1)), q, t))
    n_full = sum(1 for r in rows if min(r[3], r[4]) >= full_left)
    assert len(rows) == 3840 and n_full >= 3400 and n_full > per_chunk == 3264
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    anchors = np.zeros(len(rows), dtype=capi.ASM_ANCHOR_DTYPE)
    for i, (qid, sid, sdir, qoff, soff, q, t) in enumerate(rows):
        anchors[i] = (qid, sid, sdir, qoff, soff)
    monkeypatch.setenv("NECAT_ASM_RC_POOL_MB", "256")
    small = capi.Context(0)          # knobs are read when a context is created
    assert int(small.knob("NECAT_ASM_RC_POOL_MB")) == 256 << 20 < int(ctx.knob("NECAT_ASM_RC_POOL_MB"))      # (bytes in the field)
    out = []
    for c in (small, ctx):
        vol = c.upload_volume(pack_2bit(np.concatenate(seqs)), int(sizes.sum()), offs, sizes)
        out.append(c.asm_align_batch(vol, vol, 0, 0, anchors, 0.5, 400))
        vol.free()
    small.close()
    (aln, ops, off), (aln1, ops1, off1) = out
    assert aln.tobytes() == aln1.tobytes() and np.array_equal(off, off1) and np.array_equal(ops, ops1)
    al = ora.Aligner(0.5)
    for i, (qid, sid, sdir, qoff, soff, q, t) in enumerate(rows):
        ok, a0, a1, b0, b1, ident, qa, ta = al.align(q, qoff, t, soff, 400, 8, block_size=2048)
        a = aln[i]
        got = (bool(a["ok"]), int(a["qoff"]), int(a["qend"]), int(a["toff"]), int(a["tend"]), int(a["align_size"]), float(a["ident_perc"]))
        assert got == (ok, a0, a1, b0, b1, len(qa), ident), i
        assert capi.gapped_strings(ops[int(off[i]):int(off[i + 1])], int(a["align_size"]), q, a0, t, b0) == (qa, ta), i
    al.close()
