"""necat_volume_gather / necat_volume_download on the GPU (k_vol_gather, k_unpack_words): the cases of tests/host_core/check_vol_gather.cpp through the C ABI.
A gathered volume, downloaded, must be the pac of the subset merged on the host, byte for byte (the unused bits of the last byte zero); every refusal is
NECAT_ERR_ARG with its message; and the consensus stage's extension loop on a gathered subset of the cns golden reads gives what it gives on the set
uploaded whole, ids mapped."""
import json
import os

import numpy as np
import pytest

from necat_amd import capi, synth
from oracle import oracle_api as ora
from tests import util

pytestmark = pytest.mark.gpu

LENS = np.array([1, 2, 31, 32, 33, 63, 64, 65, 97, 1000])
VOL_BASES = (1003, 4097, 64)


def _tiling(rng, nbases):
    """reads of the lengths above that tile nbases (1 always fits)"""
    sizes, left = [], nbases
    while left:
        # a third of the picks from the reads below 32, a third from 65 and 97, a third from all ten: the two classes the 32 x 32 pairs are counted in come up
        # equally often, so the pairs fill up in some hundreds of tilings
        pool = (LENS[:3], LENS[7:9], LENS)[int(rng.integers(3))]
        n = int(pool[int(rng.integers(pool.shape[0]))])
        if n <= left:
            sizes.append(n)
            left -= n
    return np.array(sizes, dtype=np.int64)


def _upload(ctx, codes, sizes):
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    if sizes.shape[0]:
        off[1:] = np.cumsum(sizes)[:-1]
    return ctx.upload_volume(synth.pack_2bit(codes), int(codes.shape[0]), off, sizes)


def _gather_and_compare(ctx, vol_codes, vol_sizes, starts, ids):
    """gather `ids` from volumes made of (codes, sizes), download, compare with the host merge; returns (source offsets, destination offsets) of the gathered reads"""
    vols = [_upload(ctx, c, s) for c, s in zip(vol_codes, vol_sizes)]
    g = ctx.gather_volume(vols, starts, ids)
    offs = [np.concatenate([[0], np.cumsum(s)]) for s in vol_sizes]
    want, src, dst, lens, at = [], [], [], [], 0
    for i in ids:
        k = max((j for j in range(len(vols)) if starts[j] <= i), key=lambda j: starts[j])          # the volume whose id range holds i
        b, e = int(offs[k][i - starts[k]]), int(offs[k][i - starts[k] + 1])
        want.append(vol_codes[k][b:e])
        src.append(b)
        dst.append(at)
        lens.append(e - b)
        at += e - b
    want = np.concatenate(want) if want else np.zeros(0, np.uint8)
    assert g.nbases == want.shape[0] and g.nseq == len(ids) and g.sizes.tolist() == lens
    got = g.download()
    assert got.shape[0] == (want.shape[0] + 3) // 4
    assert np.array_equal(got, synth.pack_2bit(want))
    g.free()
    for v in vols:
        v.free()
    return src, dst, lens


def test_gather_all_offset_pairs(ctx):
    """three volumes of 1 003, 4 097 and 64 bases tiled with reads of 1 .. 1 000 bases, a random half gathered, tiling after tiling until every (source offset
    mod 32, destination offset mod 32) pair occurred with a read >= 65 and with a read < 32 (asserted); every gather is compared byte for byte"""
    rng = np.random.default_rng(2024)
    seen = np.zeros((2, 32, 32), dtype=bool)
    rounds = 0
    while not seen.all() and rounds < 4000:
        rounds += 1
        vol_sizes = [_tiling(rng, n) for n in VOL_BASES]
        vol_codes = [rng.integers(0, 4, n, dtype=np.uint8) for n in VOL_BASES]
        starts, at = [], int(rng.integers(5))
        for s in vol_sizes:
            starts.append(at)
            at += s.shape[0] + int(rng.integers(3))
        ids = [starts[k] + i for k in range(3) for i in range(vol_sizes[k].shape[0]) if rng.integers(2)]
        src, dst, lens = (np.array(x, dtype=np.int64) for x in _gather_and_compare(ctx, vol_codes, vol_sizes, starts, ids))
        seen[0, src[lens >= 65] & 31, dst[lens >= 65] & 31] = True
        seen[1, src[lens < 32] & 31, dst[lens < 32] & 31] = True
    assert seen.all(), "%d of the 2 x 32 x 32 offset cases never came up in %d tilings" % (int((~seen).sum()), rounds)


def test_gather_edges(ctx):
    rng = np.random.default_rng(7)
    codes = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    a = np.array
    # ten one-base reads in one word, between two longer reads
    sizes = a([40] + [1] * 10 + [50])
    c = codes(100)
    _gather_and_compare(ctx, [c], [sizes], [0], list(range(1, 11)))
    _gather_and_compare(ctx, [c], [sizes], [0], list(range(12)))
    _gather_and_compare(ctx, [c], [sizes], [7], [8, 10, 12, 14, 16, 18])
    # the first and the last read of every volume; a last read that ends in mid-word; one base; volumes given out of id order
    vc, vs = [codes(1003), codes(4097), codes(64)], [a([500, 3, 500]), a([1, 4095, 1]), a([32, 32])]
    _gather_and_compare(ctx, vc, vs, [0, 3, 6], [0, 2, 3, 5, 6, 7])
    _gather_and_compare(ctx, vc, vs, [0, 3, 6], [2])
    _gather_and_compare(ctx, vc, vs, [0, 3, 6], [5])
    _gather_and_compare(ctx, vc, vs, [0, 3, 6], list(range(8)))
    _gather_and_compare(ctx, [vc[2], vc[0], vc[1]], [vs[2], vs[0], vs[1]], [6, 0, 3], [0, 2, 3, 5, 6, 7])
    # reads of no bases; the empty list
    _gather_and_compare(ctx, [codes(70)], [a([33, 0, 0, 37])], [0], [0, 1, 2, 3])
    _gather_and_compare(ctx, [codes(70)], [a([33, 0, 0, 37])], [0], [1, 2])
    _gather_and_compare(ctx, [codes(64)], [a([64])], [0], [])
    # more than one block of the kernel's grid, source and destination out of step: 700 reads of 997 bases, every one but each seventh
    n = 700
    big = codes(997 * n)
    _gather_and_compare(ctx, [big], [np.full(n, 997)], [0], [i for i in range(n) if i % 7])


def test_download_is_the_inverse_of_upload(ctx):
    rng = np.random.default_rng(11)
    for n in (1, 3, 4, 31, 32, 33, 64, 1003, 100_001):
        c = rng.integers(0, 4, n, dtype=np.uint8)
        pac = synth.pack_2bit(c)
        v = ctx.upload_volume(pac, n, np.zeros(1, np.int64), np.array([n]))
        assert np.array_equal(v.download(), pac), n
        v.free()
    v = ctx.upload_volume(np.zeros(0, np.uint8), 0, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert v.download().shape[0] == 0
    v.free()


def test_gather_refusals(ctx):
    """ids that do not ascend, an id in no volume, overlapping id ranges and 2^32 bases are NECAT_ERR_ARG (-1) with a message; nothing is returned"""
    rng = np.random.default_rng(3)
    v0 = _upload(ctx, rng.integers(0, 4, 30, dtype=np.uint8), np.array([10, 10, 10]))
    v1 = _upload(ctx, rng.integers(0, 4, 9, dtype=np.uint8), np.array([5, 4]))
    for starts, ids, word in (([0, 5], [1, 1], "ascend"), ([0, 5], [2, 1], "ascend"), ([0, 5], [0, 6, 5], "ascend"), ([0, 5], [3], "in no volume"),
                              ([0, 5], [0, 7], "in no volume"), ([0, 5], [-1, 0], "in no volume"), ([0, 2], [0], "overlap"), ([5, 5], [], "overlap")):
        with pytest.raises(capi.NecatError, match=r"\(-1\).*" + word):
            ctx.gather_volume([v0, v1], starts, ids)
    g = ctx.gather_volume([v1, v0], [3, 0], [0, 1, 2, 4])            # adjacent ranges, out of order: fine
    assert g.nbases == 34 and g.sizes.tolist() == [10, 10, 10, 4]
    g.free()
    v0.free()
    v1.free()
    # 2^32 bases: nine volumes of 2^29 bases (one read each; zeros, 128 MB apiece on the device) - eight of them are 2^32, seven and a small one fit the limit's side
    n = 1 << 29
    pac = np.zeros(n // 4, dtype=np.uint8)
    big = [ctx.upload_volume(pac, n, np.zeros(1, np.int64), np.array([n])) for _ in range(8)]
    with pytest.raises(capi.NecatError, match=r"\(-1\).*2\^32"):
        ctx.gather_volume(big, list(range(8)), list(range(8)))
    for v in big:
        v.free()


def test_extension_loop_on_a_gathered_subset(ctx, tmp_path):
    """the consensus stage's extension loop on half of the cns golden reads: once on the set uploaded whole with the records among those reads, once on the
    subset gathered from the same reads cut into three volumes with the records' ids rewritten - the same candidates, decisions and alignments, ids mapped"""
    man = json.load(open(os.path.join(util.GOLDEN, "cns_c", "manifest.json")))
    wrk = util.install_golden_volumes(man["volumes"], tmp_path)
    whole = ctx.load_merged_volumes(wrk)
    n = whole.nseq
    sub = np.array([i for i in range(n) if i % 2 == 0], dtype=np.int64)
    assert 24 <= sub.shape[0] <= 60
    rec = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype="<u4").reshape(-1, 7)
    rec = rec[np.isin(rec[:, 1], sub) & np.isin(rec[:, 4], sub)].copy()
    assert rec.shape[0] > 500
    roff = np.zeros(n + 1, dtype=np.int64)
    roff[1:] = np.cumsum(whole.sizes)

    def loop(vol, records, back):
        cands, off, n_all = ctx.cns_load_partition(vol, records.view(np.uint8).reshape(-1))
        res = ctx.cns_extension_batch(vol, cands, off, n_all, capi.cns_options())
        cg = cands.copy()
        cg["sid"], cg["qid"] = back[cands["sid"]], back[cands["qid"]]
        txt = util.cns_log_text(res, cg, off, whole.codes, roff, ora.fnv64, full=True)
        res.free()
        return cg, off, n_all, txt

    want = loop(whole, rec, np.arange(n))
    cuts = [0, n // 3 + 1, 2 * n // 3, n]                            # three volumes of the same reads
    parts = [_upload(ctx, whole.codes[roff[cuts[k]]:roff[cuts[k + 1]]], whole.sizes[cuts[k]:cuts[k + 1]]) for k in range(3)]
    g = ctx.gather_volume(parts, cuts[:3], sub)
    assert np.array_equal(g.download(), synth.pack_2bit(np.concatenate([whole.codes[roff[i]:roff[i + 1]] for i in sub])))
    local = rec.copy()
    local[:, 1], local[:, 4] = np.searchsorted(sub, rec[:, 1]), np.searchsorted(sub, rec[:, 4])
    got = loop(g, local, sub)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert want[3].count("\nT\t") >= 20 and got[3] == want[3]
    assert ctx.gather_stats()[1] == 2 * 8 * ((g.nbases + 31) // 32) and ctx.gather_stats()[0] > 0
    g.free()
    for v in parts + [whole]:
        v.free()
