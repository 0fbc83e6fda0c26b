"""The unsharded LDS-slice index build keeps every slice (4096 table entries) at the index of its first record: what the occurrence cutoff drops leaves a hole
at the slice's end, in the offset list and in the compact table.  Lookups go through an entry's own start and count and never see the holes; the two downloads
close them and return the reference layout.  Everything here is compared with the oracle, or with the build that counts first (NECAT_INDEX_DENSE_BASES=1)."""
import os

import numpy as np
import pytest

from tests import util
from oracle import oracle_api as ora
from necat_amd import synth

pytestmark = pytest.mark.gpu

SLICE_BITS = 12          # table entries per slice (kSliceBits, index_kernels.h)
LOW_Q = 3                # an occurrence cutoff that drops k-mers in many slices at 6 x coverage
NO_CUTOFF = 1 << 30


@pytest.fixture(scope="module")
def holes(tmp_path_factory):
    """about 300 kb x 6 with a repeat family (5 kb unit over a tenth of the genome), and a smaller volume for the second build of a context"""
    d, rs, nv = util.make_dataset(tmp_path_factory.mktemp("holes"), genome=300_000, coverage=6.0, seed=31, repeat_frac=0.10)
    d2, rs2, nv2 = util.make_dataset(tmp_path_factory.mktemp("holes_small"), genome=60_000, coverage=5.0, seed=32, repeat_frac=0.10)
    assert nv == 1 and nv2 == 1
    return d, d2


_ORACLE = {}


def oracle_index(vol_path, k, q):
    """the oracle's (kmer_stats, offset_list); at the cutoff several tests share, computed once per (volume, k) and never written to"""
    key = (vol_path, k, q)
    if key in _ORACLE:
        return _ORACLE[key]
    stats, offs = ora.build_index(vol_path, k, q)
    stats.setflags(write=False); offs.setflags(write=False)
    if q == LOW_Q:
        _ORACLE[key] = (stats, offs)
    return stats, offs


def slice_losses(vol_path, k, q):
    """(non-empty slices, those that lose a k-mer to the cutoff, those that lose all of them) from the oracle's tables with and without the cutoff"""
    key = (vol_path, k, q, "losses")
    if key in _ORACLE:
        return _ORACLE[key]
    kept = oracle_index(vol_path, k, q)[0] != 0
    there = ora.build_index(vol_path, k, NO_CUTOFF)[0] != 0
    n = kept.shape[0] >> SLICE_BITS
    there_s = there.reshape(n, -1).sum(axis=1)
    kept_s = kept.reshape(n, -1).sum(axis=1)
    _ORACLE[key] = int((there_s > 0).sum()), int((kept_s < there_s).sum()), int(((there_s > 0) & (kept_s == 0)).sum())
    return _ORACLE[key]


def knob_context(monkeypatch, **env):
    """a context of its own: the knob table is read once, when a context is created"""
    from necat_amd import capi
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    c = capi.Context(0)
    for name, v in env.items():
        assert c.knob(name) == v
    return c


def check_against_oracle(c, vol, vol_path, k, q):
    """one build, both downloads, against the oracle; returns what was downloaded"""
    from necat_amd import shard
    ostats, ooffs = oracle_index(vol_path, k, q)
    ix = c.build_index(vol, k, q)
    try:
        assert ix.sizes() == (ostats.shape[0], ooffs.shape[0])
        stats, offs = ix.download()
        assert np.array_equal(stats, ostats)
        assert np.array_equal(offs, ooffs)
        sp = ix.download_sparse()
        assert sp is not None
        bits, base, compact, soffs = sp
        present = np.flatnonzero(ostats)
        assert ix.sparse_sizes() == (ostats.shape[0] // 64, present.shape[0])
        assert np.array_equal(soffs, ooffs)
        assert np.array_equal(compact, ostats[present])          # the non-zero entries in hash order, starts in the dense offset list
        pop = np.unpackbits(bits.view(np.uint8)).reshape(-1, 64).sum(axis=1).astype(np.uint64)
        assert np.array_equal(base, np.concatenate([[0], np.cumsum(pop)[:-1]]).astype(np.uint64))
        h = np.concatenate([present[:5000], np.random.default_rng(k).integers(0, ostats.shape[0], 5000)]).astype(np.uint64)
        assert np.array_equal(shard.sparse_lookup(bits, base, compact, h), ostats[h.astype(np.int64)])
        return stats, offs, bits, base, compact, ix.sizes(), ix.sparse_sizes()
    finally:
        ix.free()


@pytest.mark.parametrize("emit_big", ["0", "1"])
@pytest.mark.parametrize("k", [11, 13])
def test_index_with_holes_equals_oracle(built, holes, monkeypatch, k, emit_big):
    """both instances of k_slice_emit; at least a tenth of the non-empty slices lose a k-mer (an input without holes proves nothing)"""
    vol_path = os.path.join(holes[0], "vol0")
    nonempty, losing, _ = slice_losses(vol_path, k, LOW_Q)
    assert nonempty > 0 and losing * 10 >= nonempty, (nonempty, losing)
    c = knob_context(monkeypatch, NECAT_INDEX_EMIT_BIG=emit_big)
    try:
        assert c.knob("NECAT_INDEX_DENSE_BASES") == "0"
        vol = c.load_volume(vol_path)
        check_against_oracle(c, vol, vol_path, k, LOW_Q)
        check_against_oracle(c, vol, vol_path, k, 1)              # kmer_cnt_cutoff = 1: every repeated k-mer goes
        vol.free()
    finally:
        c.close()


def _write_one_volume(d, reads):
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "vol0")
    synth.write_volume(path, np.concatenate(reads).astype(np.uint8), [r.shape[0] for r in reads], ["r%d" % i for i in range(len(reads))])
    return path


@pytest.mark.parametrize("emit_big", ["0", "1"])
def test_edges_empty_slices_and_no_records(built, tmp_path, monkeypatch, emit_big):
    rng = np.random.default_rng(77)
    # a read twice, and a third one: at cutoff 1 every k-mer of the doubled read is dropped - the slices only it reaches keep nothing of their records
    a, b = rng.integers(0, 4, 400, dtype=np.uint8), rng.integers(0, 4, 3000, dtype=np.uint8)
    doubled = _write_one_volume(str(tmp_path / "doubled"), [a, a.copy(), b])
    nonempty, losing, emptied = slice_losses(doubled, 12, 1)
    assert emptied > 0 and losing >= emptied, (nonempty, losing, emptied)
    # one read shorter than k: bases, but no record at all
    short = _write_one_volume(str(tmp_path / "short"), [rng.integers(0, 4, 9, dtype=np.uint8)])
    c = knob_context(monkeypatch, NECAT_INDEX_EMIT_BIG=emit_big)
    try:
        vol = c.load_volume(doubled)
        for k in (11, 12):
            check_against_oracle(c, vol, doubled, k, 1)
        vol.free()
        vol = c.load_volume(short)
        for k in (11, 12):
            stats, offs = check_against_oracle(c, vol, short, k, 500)[:2]
            assert offs.shape[0] == 0 and not stats.any()
        vol.free()
    finally:
        c.close()


@pytest.mark.parametrize("q", [LOW_Q, 500])
def test_candidates_through_the_holes(ctx, holes, tmp_path, q):
    """find_candidates of the volume against itself (-j 0) reads the table and the offset list with their holes in place"""
    from necat_amd import capi
    assert ctx.knob("NECAT_INDEX_DENSE_BASES") == "0"
    d = holes[0]
    kw = dict(util.FAST, kmer_cnt_cutoff=q)
    out = os.path.join(str(tmp_path), "oracle_%d.out" % q)
    st = ora.pm_main(ora.options(**dict(kw, job=0, binary_output=1)), 0, d, out)
    cands, _ = capi.pm_main(ctx, capi.default_options(**dict(kw, job=0, binary_output=1)), 0, d)
    mine = sorted(bytes(r) for r in capi.pack_candidates(cands).astype("<u4"))
    assert len(mine) == st.n_records and len(mine) > 100
    assert mine == ora.sorted_records(out, 28)


def test_record_space_build_equals_the_counting_build(built, holes, monkeypatch):
    """the fallback (NECAT_INDEX_DENSE_BASES=1: count, scan, pack without holes) and the default give the same downloads and the same sizes"""
    vol_path = os.path.join(holes[0], "vol0")
    got = {}
    for dense in ("1", "0"):
        c = knob_context(monkeypatch, NECAT_INDEX_DENSE_BASES=dense)
        try:
            vol = c.load_volume(vol_path)
            got[dense] = [check_against_oracle(c, vol, vol_path, k, LOW_Q) for k in (11, 13)]
            vol.free()
        finally:
            c.close()
    for old, new in zip(got["1"], got["0"]):
        for x, y in zip(old[:5], new[:5]):
            assert np.array_equal(x, y)
        assert old[5:] == new[5:]


def test_back_to_back_builds_reuse_the_cached_arrays(built, holes, monkeypatch):
    """the second build of a context, of a smaller volume, takes the table and the offset list the first one released (sized by the first one's
    capacity, not by its counts); stale entries of the first build lie in the second one's holes"""
    big, small = os.path.join(holes[0], "vol0"), os.path.join(holes[1], "vol0")
    c = knob_context(monkeypatch, NECAT_INDEX_DENSE_BASES="0")
    try:
        for path in (big, small, big):
            vol = c.load_volume(path)
            check_against_oracle(c, vol, path, 13, LOW_Q)
            vol.free()
    finally:
        c.close()
