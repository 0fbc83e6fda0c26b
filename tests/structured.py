"""Structured test input: low-complexity sequence, tie-heavy blocks, blocks at the acceptance threshold.

The other generators of the suite (necat_amd/synth.py, tests/util.py) draw i.i.d. uniform ACGT with i.i.d. errors.  On such input a cell of
the edit matrix rarely has more than one optimal predecessor for long, the bottom row has one clear minimum, and a block's distance sits far
from k = (int)(min(qn, tn) * error * 1.1).  Here: homopolymers, tandem repeats and two-letter sequence (every cell ties, for hundreds of steps;
the bottom row is a plateau of equal minima), every block size at which a kernel changes words, long single indels, and chains of blocks whose
distance walks through k - 1 .. k + 2.  Plain numpy, seeded; everything is checked against the oracle at run time (no goldens)."""
import re

import numpy as np

from necat_amd.synth import _mutate

KINDS = ("homo", "di", "tandem", "two", "mixed")
PURE_KINDS = KINDS[:4]
MAX_BLOCK = 794            # the longest fragment a block takes (a last block of 512 + 282)
BOUNDARY_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 793, 794)
INDEL_LENGTHS = (40, 64, 65, 100, 128, 129, 200)
THRESHOLD_OFFSETS = (-1, 0, 1, 2)
BLOCK_SEED, THRESHOLD_SEED = 20261, 20262          # the seeds at which tests/test_structured.py asserts its conditions and tests/test_gpu_structured.py draws its blocks


def _two_letters(rng):
    a = int(rng.integers(0, 4))
    return a, (a + int(rng.integers(1, 4))) & 3


def low_complexity(n, kind, rng):
    """n bases of one kind: homo = one base; di = a 2-mer of two different bases repeated; tandem = a random unit of 3 - 8 bases repeated;
    two = i.i.d. over two letters; mixed = random stretches of 5 - 60 bases alternating with runs of one base of 5 - 120."""
    n = int(n)
    if kind == "homo":
        return np.full(n, int(rng.integers(0, 4)), dtype=np.uint8)
    if kind == "di":
        return np.tile(np.array(_two_letters(rng), dtype=np.uint8), n // 2 + 1)[:n]
    if kind == "tandem":
        u = rng.integers(0, 4, int(rng.integers(3, 9)), dtype=np.uint8)
        return np.tile(u, n // u.shape[0] + 1)[:n]
    if kind == "two":
        return np.array(_two_letters(rng), dtype=np.uint8)[rng.integers(0, 2, n)]
    if kind == "mixed":
        out, have, run = [], 0, bool(rng.integers(0, 2))
        while have < n:
            if run:
                out.append(np.full(int(rng.integers(5, 121)), int(rng.integers(0, 4)), dtype=np.uint8))
            else:
                out.append(rng.integers(0, 4, int(rng.integers(5, 61)), dtype=np.uint8))
            have += out[-1].shape[0]
            run = not run
        return np.concatenate(out)[:n] if out else np.zeros(0, dtype=np.uint8)
    if kind == "uniform":
        return rng.integers(0, 4, n, dtype=np.uint8)
    raise ValueError("unknown kind %r" % (kind,))


def genome_with_runs(n, rng, frac):
    """(genome, runs): a uniform genome in which, every 100 .. 600 / frac bases, a stretch of 20 - 400 bases is overwritten with one of the four
    pure kinds - runs longer than one 64-row word and, at 400, most of a 512-base block; runs = [(start, length, kind)]."""
    n = int(n)
    g = rng.integers(0, 4, n, dtype=np.uint8)
    runs = []
    p = 0
    while True:
        p += int(rng.integers(100, int(600 / frac) + 1))
        L = int(rng.integers(20, 401))
        if p + L > n:
            break
        kind = PURE_KINDS[int(rng.integers(0, 4))]
        g[p:p + L] = low_complexity(L, kind, rng)
        runs.append((p, L, kind))
        p += L
    return g, runs


def low_complexity_genome(n, seed, frac):
    return genome_with_runs(n, np.random.default_rng(seed), frac)[0]


class _Blocks:
    """blocks in the layout edlib_align_batch takes: one array of bases, per block the offsets and lengths of query and target, and a tag"""

    def __init__(self):
        self.parts, self.pos = [], 0
        self.q_off, self.q_len, self.t_off, self.t_len, self.tag = [], [], [], [], []

    def add(self, q, t, tag):
        assert 1 <= q.shape[0] <= MAX_BLOCK and 1 <= t.shape[0] <= MAX_BLOCK, tag
        for s, off, ln in ((q, self.q_off, self.q_len), (t, self.t_off, self.t_len)):
            self.parts.append(np.ascontiguousarray(s, dtype=np.uint8))
            off.append(self.pos); ln.append(int(s.shape[0])); self.pos += int(s.shape[0])
        self.tag.append("%s %dx%d" % (tag, q.shape[0], t.shape[0]))

    def result(self):
        return np.concatenate(self.parts), self.q_off, self.q_len, self.t_off, self.t_len, self.tag


def concat_blocks(*sets):
    """several block sets as one"""
    seqs, out, base = [], ([], [], [], [], []), 0
    for s, qo, ql, to, tl, tag in sets:
        seqs.append(s)
        out[0].extend(int(o) + base for o in qo); out[1].extend(ql)
        out[2].extend(int(o) + base for o in to); out[3].extend(tl); out[4].extend(tag)
        base += int(s.shape[0])
    return (np.concatenate(seqs),) + out


def block_pair(blocks, i):
    seqs, qo, ql, to, tl, _ = blocks
    return seqs[qo[i]:qo[i] + ql[i]], seqs[to[i]:to[i] + tl[i]]


def _cut_pair(kind, qn, tn, err, rng):
    """q and t of exactly qn and tn bases, two independently mutated copies of one sequence of `kind`"""
    base = low_complexity(int(max(qn, tn) * 1.3) + 24, kind, rng)
    q, t = _mutate(base, err, rng), _mutate(base, err, rng)
    assert q.shape[0] >= qn and t.shape[0] >= tn
    return q[:qn], t[:tn]


def structured_blocks(rng, per_kind=30):
    """(seqs, q_off, q_len, t_off, t_len, tag).  Families (the first word of a tag):
    ragged/<kind>   t = low_complexity(n), n in 1 .. 794, q = t with 15 % errors, cut at 794
    full/<kind>     exact 512 x 512 blocks cut from a 700-base pair at 13 %
    size/<kind>     qn in BOUNDARY_SIZES against tn of the same and of the neighbouring size, on mixed and on uniform sequence, both 10 % off a common ancestor
    indel/<kind>/<ins|del><L>@<at>/<full|ragged>   q = t at 5 % with one stretch of L bases put in / taken out at row 0, at 60 or in the middle; L < k"""
    b = _Blocks()
    for kind in KINDS:
        for _ in range(per_kind):
            t = low_complexity(int(rng.integers(1, MAX_BLOCK + 1)), kind, rng)
            q = _mutate(t, 0.15, rng)[:MAX_BLOCK]
            if q.shape[0] == 0:
                q = t[:1].copy()
            b.add(q, t, "ragged/" + kind)
        n = 0
        while n < per_kind:
            t = low_complexity(700, kind, rng)
            q = _mutate(t, 0.13, rng)
            if q.shape[0] >= 512:
                b.add(q[:512], t[:512], "full/" + kind)
                n += 1
    for kind in ("mixed", "uniform"):
        for i, qn in enumerate(BOUNDARY_SIZES):
            for tn in BOUNDARY_SIZES[max(i - 1, 0):i + 2]:
                q, t = _cut_pair(kind, qn, tn, 0.10, rng)
                b.add(q, t, "size/" + kind)
    for kind in ("uniform", "mixed"):
        for L in INDEL_LENGTHS:
            for what in ("ins", "del"):
                for at in ("0", "60", "mid"):
                    for shape in ("full", "ragged"):
                        t = low_complexity(1100, kind, rng)
                        q = _mutate(t, 0.05, rng)
                        p = {"0": 0, "60": 60}.get(at, 256 if shape == "full" else 330)
                        if what == "ins":
                            q = np.concatenate([q[:p], low_complexity(L, kind, rng), q[p:]])
                        else:
                            q = np.concatenate([q[:p], q[p + L:]])
                        qn, tn = (512, 512) if shape == "full" else (int(rng.integers(520, MAX_BLOCK + 1)), int(rng.integers(520, MAX_BLOCK + 1)))
                        assert L < int(min(qn, tn) * 0.5 * 1.1)
                        b.add(q[:qn], t[:tn], "indel/%s/%s%d@%s/%s" % (kind, what, L, at, shape))
    return b.result()


def reference_results(blocks, error=0.5):
    """the oracle's Edlib_align of every block: [(ok, dist, qend, tend, ops)]"""
    from oracle import oracle_api as ora
    return [ora.edlib_align(*block_pair(blocks, i), error) for i in range(len(blocks[5]))]


def threshold_offset(tag):
    """d - k of a threshold block, from its tag (None for every other block)"""
    m = re.search(r"d-k=([+-]?\d+)", tag)
    return int(m.group(1)) if m else None


def threshold_blocks(rng, error=0.5, chains=(16, 24)):
    """Blocks whose distance d is k - 1, k, k + 1 and k + 2, k = (int)(min(qn, tn) * error * 1.1): Edlib_align accepts the first two and refuses the others.
    Chains: a pair far below k, then one base of q changed at a time (a change moves d by at most one, so no offset is jumped over); d after every change from
    the oracle at error = 0.95, where no block fails below d ~ min(qn, tn); the block is kept the first time d - k is each of -1, 0, +1, +2.
    chains[0] chains of 512 x 512 blocks: t i.i.d. over two letters, q cut from a copy at 13 %; a change writes one of the OTHER two letters (substitutions inside one alphabet
    saturate near 0.3 n, and uniform ACGT near 0.51 n = 261 < k = 281); chains[1] ragged chains: tn in 200 .. 600, q = t + up to 0.5 tn random bases, cut at 794.
    Asserts the reference alone first: ora.edlib_align(q, t, error) succeeds iff d <= k, and with the same d.  Tags: threshold/<two512|ragged> QxT d-k=<offset>."""
    from oracle import oracle_api as ora
    b = _Blocks()
    for c in range(chains[0] + chains[1]):
        full = c < chains[0]
        if full:
            a0, a1 = _two_letters(rng)
            t = np.array([a0, a1], dtype=np.uint8)[rng.integers(0, 2, 700)]
            q = _mutate(t, 0.13, rng)[:512].copy()
            t = t[:512]
            assert q.shape[0] == 512
            others = np.array([x for x in range(4) if x not in (a0, a1)], dtype=np.uint8)
        else:
            tn = int(rng.integers(200, 601))
            t = rng.integers(0, 4, tn, dtype=np.uint8)
            q = np.concatenate([t, rng.integers(0, 4, int(rng.integers(0, int(0.5 * tn) + 1)), dtype=np.uint8)])[:MAX_BLOCK]
        qn, tn = int(q.shape[0]), int(t.shape[0])
        k = int(min(qn, tn) * error * 1.1)
        order = rng.permutation(qn)
        done, kept = 0, set()
        while True:
            ok95, d, _, _, _ = ora.edlib_align(q, t, 0.95)
            assert ok95, (qn, tn, d)
            off = d - k
            if off in THRESHOLD_OFFSETS and off not in kept:
                ok, d2, _, _, _ = ora.edlib_align(q, t, error)
                assert ok == (d <= k) and (not ok or d2 == d), (qn, tn, d, k, ok, d2)
                kept.add(off)
                b.add(q.copy(), t, "threshold/%s d-k=%+d" % ("two512" if full else "ragged", off))
            if off > 2 or len(kept) == 4:
                break
            step = max(1, (k - 1) - d)          # d rises by at most one per change: never past k - 1 unseen
            if done + step > qn:
                break
            for p in order[done:done + step]:
                q[p] = others[int(rng.integers(0, 2))] if full else (int(q[p]) + 1 + int(rng.integers(0, 3))) & 3
            done += step
    return b.result()


def anchored_pairs(rng, npairs=40):
    """Pairs for the whole block-wise aligner (onc_align), as tests/test_gpu_parity.py::test_onc_align_arbitrary_anchors builds them, on sequence with runs:
    [(q, t, qdir, [(qoff, toff)] * 3)], q in the orientation it is aligned in.  Ancestor of 1 200 - 6 000 bases from genome_with_runs at frac 0.3 - 0.6 plus one
    planted run of 100 - 250 bases; q and t are copies at 3 - 16 % errors.  Every fourth pair: the target's planted run is 30 - 200 bases longer, or shorter (by
    at most half the run).  Every seventh: an unrelated target (the extension fails).  Anchors: one inside the planted run, a quarter into it, exact on both
    sequences (the copies are mutated piece by piece around it); one at a random fraction; one at an end of both sequences or at another random fraction."""
    out = []
    for it in range(npairs):
        n = int(rng.integers(1200, 6001))
        g, _ = genome_with_runs(n, rng, float(rng.uniform(0.3, 0.6)))
        R, kind = int(rng.integers(100, 251)), PURE_KINDS[int(rng.integers(0, 4))]
        run = low_complexity(R + 200, kind, rng)
        at = int(rng.integers(0, n - R + 1))
        g[at:at + R] = run[:R]
        gt = g
        if it % 4 == 3:
            delta = int(rng.integers(30, 201))
            if rng.integers(0, 2):
                gt = np.concatenate([g[:at], run[:R + delta], g[at + R:]])
            else:
                gt = np.concatenate([g[:at + R - min(delta, R // 2)], g[at + R:]])
        p = at + R // 4
        eq, et = float(rng.uniform(0.03, 0.16)), float(rng.uniform(0.03, 0.16))
        qa, qb = _mutate(g[:p], eq, rng), _mutate(g[p:], eq, rng)
        ta, tb = _mutate(gt[:p], et, rng), _mutate(gt[p:], et, rng)
        q, t = np.concatenate([qa, qb]), np.concatenate([ta, tb])
        anchors = [(int(qa.shape[0]), int(ta.shape[0]))]
        if it % 7 == 3:
            t = rng.integers(0, 4, t.shape[0], dtype=np.uint8)
        for j in (1, 2):
            frac = float(rng.integers(0, 2)) if (j == 2 and it % 2) else float(rng.uniform(0.0, 1.0))
            anchors.append((int(frac * (q.shape[0] - 1)), int(frac * (t.shape[0] - 1))))
        out.append((q, t, it & 1, anchors))
    return out
