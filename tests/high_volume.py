"""Test sequences placed high in a volume: behind filler sequences of zero bases, so that the sequences a job names begin around base 2^31 of the volume
("straddle") or end at its last base with the volume as large as necat_volume_upload takes, 2^32 - 1 bases ("top").  What an entry computes on them must
be what it computes on the same sequences at the front of a small volume: tests/test_gpu_high_offsets.py runs the suite's reference-pinned cases this way.
A filler holds at most 2^29 bases, so no per-sequence limit (2^30, 2^31) comes into play."""
import numpy as np

from necat_amd import synth

PLACEMENTS = ("straddle", "top")
HALF = 1 << 31                       # the base an i32 position cannot name
TOP_BASES = (1 << 32) - 1            # the largest volume necat_volume_upload accepts
FILLER_MAX = 1 << 29

_zero_pac = None                     # (TOP_BASES + 3) // 4 zero bytes, made once; a placement pokes its packed tail in and takes it out again


def _pac(nbytes):
    global _zero_pac
    if _zero_pac is None:
        _zero_pac = np.zeros((TOP_BASES + 3) // 4, dtype=np.uint8)
    return _zero_pac[:nbytes]


def layout(lens, where, straddle=None):
    """(prefix bases, filler sizes, index of the straddling sequence or None) for test sequences of the lengths `lens`"""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    assert lens.shape[0] and total < FILLER_MAX
    s = None
    if where == "straddle":
        if straddle is None:
            # the longest sequence that has a neighbour on either side
            assert lens.shape[0] >= 3, "a sequence on both sides of the straddling one"
            straddle = 1 + int(np.argmax(lens[1:-1]))
        s = int(straddle)
        assert 0 < s < lens.shape[0] - 1 and lens[s] >= 2
        before = int(lens[:s].sum())
        prefix = HALF - before - int(lens[s]) // 2          # base 2^31 in the middle of sequence s ...
        prefix -= (prefix - 13) % 32                        # ... and the prefix = 13 (mod 32): at most 31 bases earlier (place() asserts begin < 2^31 < end)
        assert prefix % 32 == 13
    elif where == "top":
        prefix = TOP_BASES - total
    else:
        raise ValueError(where)
    k = -(-prefix // FILLER_MAX)
    fill = np.full(k, FILLER_MAX, dtype=np.int64)
    fill[-1] = prefix - (k - 1) * FILLER_MAX
    assert int(fill.sum()) == prefix and 0 < fill.min() and fill.max() <= FILLER_MAX
    return prefix, fill, s


def place(ctx, seqs, where, straddle=None):
    """a capi.Volume of k fillers followed by `seqs` (arrays of base codes 0..3), and k: local id i of `seqs` is id k + i of the volume.  .first_base is where
    seqs[0] begins, .placed = (begin, end) of the straddling sequence ("straddle") or of the last one ("top")"""
    seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    lens = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    prefix, fill, s = layout(lens, where, straddle)
    k = int(fill.shape[0])
    sizes = np.concatenate([fill, lens])
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    nbases = int(sizes.sum())
    if where == "straddle":
        begin, end = int(off[k + s]), int(off[k + s] + sizes[k + s])
        assert begin < HALF < end, (begin, end)
        assert k + s > k and k + s < sizes.shape[0] - 1
    else:
        assert nbases == TOP_BASES
        begin, end = int(off[-1]), nbases
    pac = _pac((nbases + 3) // 4)
    tail = synth.pack_2bit(np.concatenate([np.zeros(prefix % 4, dtype=np.uint8)] + seqs))
    at = prefix // 4
    assert at + tail.shape[0] == pac.shape[0]
    pac[at:] = tail
    try:
        vol = ctx.upload_volume(pac, nbases, off, sizes)
    finally:
        pac[at:] = 0
    vol.first_base, vol.placed = prefix, (begin, end)
    return vol, k


def small(ctx, seqs):
    """the same sequences as a volume of their own: the other side of a two-volume entry"""
    seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    sizes = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    off = np.zeros(sizes.shape[0], dtype=np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    return ctx.upload_volume(synth.pack_2bit(np.concatenate(seqs)), int(sizes.sum()), off, sizes)
