"""Conditions on the generators of tests/structured.py, with the oracle alone: the GPU cases built on them (tests/test_gpu_structured.py) keep their
edge cases only while these hold - enough aligned blocks of every family, blocks on both sides of the acceptance threshold d <= k."""
import collections

import numpy as np
import pytest

from tests import structured

@pytest.fixture(scope="module")
def blocks(built):
    b = structured.structured_blocks(np.random.default_rng(structured.BLOCK_SEED))
    return b, structured.reference_results(b, 0.5)


def test_low_complexity_kinds():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 7, 64, 513):
        for kind in structured.KINDS:
            s = structured.low_complexity(n, kind, rng)
            assert s.dtype == np.uint8 and s.shape == (n,) and (n == 0 or int(s.max()) < 4)
    assert len(set(structured.low_complexity(300, "homo", rng).tolist())) == 1
    d = structured.low_complexity(300, "di", rng)
    assert len(set(d.tolist())) == 2 and np.array_equal(d[2:], d[:-2]) and d[0] != d[1]
    assert len(set(structured.low_complexity(300, "two", rng).tolist())) == 2
    t = structured.low_complexity(300, "tandem", rng)
    assert any(np.array_equal(t[u:], t[:-u]) for u in range(3, 9))
    g, runs = structured.genome_with_runs(60_000, np.random.default_rng(2), 0.6)
    assert np.array_equal(g, structured.low_complexity_genome(60_000, 2, 0.6))
    lens = [L for _, L, _ in runs]
    assert len(runs) > 50 and min(lens) >= 20 and max(lens) > 300 and {k for _, _, k in runs} == set(structured.PURE_KINDS)
    assert 0.1 < sum(lens) / 60_000 < 0.5


def test_structured_blocks_cover_their_families(blocks):
    """each kind x {ragged, full} has at least 20 blocks the oracle aligns; every boundary size is there, as query and as target, on both kinds of sequence;
    at least half of the long-indel blocks are aligned, and at every length, as insertion and as deletion"""
    b, ref = blocks
    seqs, qo, ql, to, tl, tag = b
    aligned = collections.Counter()
    total = collections.Counter()
    for i, tg in enumerate(tag):
        f = tg.split()[0].split("/")
        fam = f[0] if f[0] == "indel" else "/".join(f[:2])
        total[fam] += 1
        aligned[fam] += ref[i][0]
        if f[0] == "full":
            assert (ql[i], tl[i]) == (512, 512)
        if f[0] == "indel":
            aligned["/".join(["indel", f[2].split("@")[0]])] += ref[i][0]
    for kind in structured.KINDS:
        for shape in ("ragged", "full"):
            assert aligned["%s/%s" % (shape, kind)] >= 20, (shape, kind)
    for kind in ("mixed", "uniform"):
        sizes = [(ql[i], tl[i]) for i, tg in enumerate(tag) if tg.startswith("size/" + kind)]
        assert {q for q, _ in sizes} == set(structured.BOUNDARY_SIZES) == {t for _, t in sizes}
        assert all((s, s) in sizes for s in structured.BOUNDARY_SIZES) and (513, 512) in sizes and (512, 513) in sizes and (64, 65) in sizes
        assert aligned["size/" + kind] >= 30
    assert total["indel"] == 2 * len(structured.INDEL_LENGTHS) * 2 * 3 * 2 and 2 * aligned["indel"] >= total["indel"]
    for L in structured.INDEL_LENGTHS:
        assert aligned["indel/ins%d" % L] >= 6 and aligned["indel/del%d" % L] >= 6, L
    nfail = sum(not r[0] for r in ref)
    assert 0 < nfail < len(tag) // 4


def test_threshold_blocks_sit_on_both_sides_of_k(built):
    """at least 10 blocks at each of d - k = -1, 0, +1, +2, at least 5 of them 512 x 512 and at least 5 ragged with qn > 512; the oracle accepts exactly d <= k
    (threshold_blocks asserts that while it builds the chains; here once more from the tags, on the finished blocks)"""
    b = structured.threshold_blocks(np.random.default_rng(structured.THRESHOLD_SEED))
    ref = structured.reference_results(b, 0.5)
    seqs, qo, ql, to, tl, tag = b
    n = collections.Counter()
    for i, tg in enumerate(tag):
        off = structured.threshold_offset(tg)
        assert off in structured.THRESHOLD_OFFSETS
        k = int(min(ql[i], tl[i]) * 0.5 * 1.1)
        assert ref[i][0] == (off <= 0) and (not ref[i][0] or ref[i][1] == k + off), tg
        n[off, "all"] += 1
        n[off, "full"] += (ql[i], tl[i]) == (512, 512)
        n[off, "long"] += ql[i] > 512
    for off in structured.THRESHOLD_OFFSETS:
        assert n[off, "all"] >= 10 and n[off, "full"] >= 5 and n[off, "long"] >= 5, (off, n)
    assert all(structured.threshold_offset(tg) is None for tg in structured.structured_blocks(np.random.default_rng(3), per_kind=1)[5])
