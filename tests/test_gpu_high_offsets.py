"""The batch entries on sequences that lie above base 2^31 of their volume (tests/high_volume.py): around it ("straddle": a sequence a job names begins
below 2^31 and ends above it, behind a prefix that is 13 modulo 32) and at the end of a volume of 2^32 - 1 bases ("top", the largest necat_volume_upload
takes).  A project of 2.1 to 4.2 Gbp is one such volume for oc2cns, so this is where its reads are.  Every expectation is one the suite already pins to
the reference or to the oracle at the front of a small volume - the goldens, the oracle's aligner - and the ids are mapped; nothing here is compared with
a low-offset run of the same kernel alone.  An entry that takes two volumes runs with either of them high and the other small."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from necat_amd import build, capi, synth
from oracle import oracle_api as ora
from tests import ctg_cases as cc
from tests import ctg_ext_cases as xc
from tests import ctg_seed_cases as sc
from tests import dalign_cases, nw_cases, util
from tests import high_volume as hv

pytestmark = pytest.mark.gpu

WHERE = pytest.mark.parametrize("where", hv.PLACEMENTS)
SIDE = pytest.mark.parametrize("side", ["reads_high", "ref_high"])
MAN = json.load(open(os.path.join(util.GOLDEN, "cns_c", "manifest.json")))


def _check_placement(vol, where):
    """what the helper promises, seen from the volume it returned"""
    assert vol.first_base % 32 == 13 or where == "top"
    if where == "straddle":
        assert vol.placed[0] < hv.HALF < vol.placed[1] and hv.HALF < vol.nbases < hv.HALF + hv.FILLER_MAX
    else:
        assert vol.nbases == hv.TOP_BASES == vol.placed[1] and vol.first_base > hv.HALF


def _two_volumes(where, side):
    """a volume builder for nw_cases.run_cases / dalign_cases.run_cases: the side named high, the other one small"""
    def build_volumes(ctx, reads, tmpls):
        if side == "reads_high":
            rv, k = hv.place(ctx, reads, where)
            _check_placement(rv, where)
            return rv, hv.small(ctx, tmpls), nw_cases.READ0 + k, nw_cases.REF0
        tv, k = hv.place(ctx, tmpls, where)
        _check_placement(tv, where)
        return hv.small(ctx, reads), tv, nw_cases.READ0, nw_cases.REF0 + k
    return build_volumes


# ---- necat_volume_gather, necat_volume_download

@WHERE
def test_gather_and_download(ctx, where):
    """the test reads gathered out of the high volume, then every sequence, fillers included (the destination passes word 2^26), then the volume itself
    downloaded: pack_2bit of the concatenation, or the uploaded pac, byte for byte"""
    rng = np.random.default_rng(31)
    lens = [1, 31, 32, 33, 63, 64, 65, 97, 1000, 4097, 2, 129]
    seqs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    vol, k = hv.place(ctx, seqs, where, straddle=lens.index(4097) if where == "straddle" else None)
    _check_placement(vol, where)
    ids = [k + i for i in range(len(seqs)) if i != 3]
    g = ctx.gather_volume([vol], [0], ids)
    want = np.concatenate([s for i, s in enumerate(seqs) if i != 3])
    assert g.nbases == want.shape[0] and g.sizes.tolist() == [n for i, n in enumerate(lens) if i != 3]
    assert np.array_equal(g.download(), synth.pack_2bit(want))
    g.free()
    # all ids: the gathered volume is the volume
    tail = synth.pack_2bit(np.concatenate([np.zeros(vol.first_base % 4, dtype=np.uint8)] + seqs))
    at = vol.first_base // 4

    def is_the_upload(pac):
        assert pac.shape[0] == (vol.nbases + 3) // 4 == at + tail.shape[0]
        assert np.array_equal(pac[at:], tail) and not pac[:at].any()
    g = ctx.gather_volume([vol], [0], np.arange(vol.nseq))
    assert g.nbases == vol.nbases and (g.nbases + 31) // 32 > 1 << 26
    is_the_upload(g.download())
    g.free()
    is_the_upload(vol.download())
    vol.free()


# ---- necat_nw_path_batch, necat_local_align_batch

@WHERE
@SIDE
def test_nw_path_batch(ctx, where, side):
    """tests/test_gpu_nw.py's shapes and the 60 golden rescue pairs against tests/golden/nw_cases.json and rescue_cases.json; run_cases asserts
    n_host == 0 and n_selfcheck == 0 on every call"""
    cases = nw_cases.shape_cases()
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "nw_cases.json")))["cases"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = nw_cases.run_cases(ctx, cases, _two_volumes(where, side))
    for c, r in zip(cases, got):
        assert nw_cases.hashed(r) == nw_cases.golden_of(g[c["name"]]), c["name"]
    assert sum(st.n_splits for st in stats) >= 5
    cases = nw_cases.golden_rescue_cases()
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["edlib_go"]}
    got, stats = nw_cases.run_cases(ctx, cases, _two_volumes(where, side))
    for c, r in zip(cases, got):
        assert nw_cases.hashed(r) == nw_cases.golden_of(g[c["name"]]), c["name"]
    assert sum(r[0] for r in got) > 15 and max(st.n_levels for st in stats) >= 3


@WHERE
@SIDE
def test_local_align_batch(ctx, where, side):
    """tests/test_gpu_dalign.py's shapes and the 60 golden pairs against tests/golden/dalign_cases.json and rescue_cases.json, every job decided on the device"""
    cases = dalign_cases.shape_cases()
    g = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "dalign_cases.json")))["cases"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = dalign_cases.run_cases(ctx, cases, _two_volumes(where, side))
    assert dalign_cases.all_on_device(got, stats) and sum(st.n_device for st in stats) == len(cases)
    for c, r in zip(cases, got):
        assert r[:3] == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert max(st.max_diags for st in stats) > 128
    cases = dalign_cases.golden_rescue_cases()
    g = {"seed%d" % c["seed"]: c for c in json.load(open(os.path.join(util.GOLDEN, "rescue_cases.json")))["ocda_go"]}
    assert sorted(g) == sorted(c["name"] for c in cases)
    got, stats = dalign_cases.run_cases(ctx, cases, _two_volumes(where, side))
    assert dalign_cases.all_on_device(got, stats)
    for c, r in zip(cases, got):
        assert r[:3] == (g[c["name"]]["ret"], g[c["name"]]["out"], g[c["name"]]["ident"]), c["name"]
    assert sum(r[0] for r in got) > 20


# ---- necat_onc_align_batch, necat_asm_align_batch: both sequences of a pair come from one list; one volume holds it high, the other small

def _pair_volumes(ctx, seqs, where, side):
    """(ref, reads, what to add to a query id, what to add to a subject id)"""
    high, k = hv.place(ctx, seqs, where)
    _check_placement(high, where)
    low = hv.small(ctx, seqs)
    return (low, high, k, 0) if side == "reads_high" else (high, low, 0, k)


@WHERE
@SIDE
def test_onc_align_batch(ctx, where, side):
    """the candidates of tests/golden/onc_align_a.json: what the reference's own onc_align returned (value, coordinates, identity, md5 of both gapped strings),
    at tail_match_len 4 and 1 - the fields tests/test_oracle_golden.py compares for the oracle"""
    gold = json.load(open(os.path.join(util.GOLDEN, "onc_align_a.json")))
    pac, offs, sizes, _ = synth.read_volume(os.path.join(util.GOLDEN, "vols_a", "vol0"))
    codes = synth.unpack_2bit(pac, int(sizes.sum()))
    keys = [tuple(g["cand"]) for g in gold if g["tail"] == 4]
    assert len(gold) == 2 * len(keys) and [tuple(g["cand"]) for g in gold if g["tail"] == 1] == keys
    used = sorted({i for key in keys for i in key[:2]})
    local = {i: n for n, i in enumerate(used)}
    seqs = [codes[int(offs[i]):int(offs[i] + sizes[i])] for i in used]
    ref, reads, dq, ds = _pair_volumes(ctx, seqs, where, side)
    cands = np.zeros(len(keys), dtype=capi.CANDIDATE_DTYPE)
    for n, (qid, sid, qdir, qoff, soff) in enumerate(keys):
        cands[n]["qid"], cands[n]["sid"], cands[n]["qdir"] = local[qid] + dq, local[sid] + ds, qdir
        cands[n]["qsize"], cands[n]["ssize"], cands[n]["qoff"], cands[n]["soff"] = sizes[qid], sizes[sid], qoff, soff
    opt = capi.default_options(**dict(util.FAST, job=1, align_size_cutoff=1000))
    n_ok = 0
    for tail in (4, 1):
        aln, ops, off = ctx.onc_align_batch(ref, reads, 0, 0, cands, opt, tail)
        want = [g for g in gold if g["tail"] == tail]
        for n, (key, g) in enumerate(zip(keys, want)):
            a = aln[n]
            q = seqs[local[key[0]]]
            if key[2] == 1:
                q = (3 - q[::-1]).astype(np.uint8)
            qa, ta = capi.gapped_strings(ops[int(off[n]):int(off[n + 1])], int(a["align_size"]), q, int(a["qoff"]), seqs[local[key[1]]], int(a["toff"]))
            got = dict(cand=list(key), tail=tail, ok=int(a["ok"]), qoff=int(a["qoff"]), qend=int(a["qend"]), toff=int(a["toff"]), tend=int(a["tend"]),
                       ident="%.17g" % float(a["ident_perc"]), columns=len(qa), query_align_md5=hashlib.md5(qa).hexdigest(), target_align_md5=hashlib.md5(ta).hexdigest())
            assert got == g, (n, tail)
            n_ok += g["ok"]
    assert n_ok > 100
    ref.free(); reads.free()


@WHERE
@SIDE
def test_asm_align_batch(ctx, where, side):
    """the 60 pairs of tests/test_gpu_zz_asm_align.py::test_asm_align_arbitrary_anchors on the default path, against the oracle's aligner at block size 2048"""
    from tests import test_gpu_zz_asm_align as asm_t
    seqs, rows = asm_t.arbitrary_anchor_pairs()
    ref, reads, dq, ds = _pair_volumes(ctx, seqs, where, side)
    anchors = np.zeros(len(rows), dtype=capi.ASM_ANCHOR_DTYPE)
    for i, (qid, sid, sdir, qoff, soff, q, t) in enumerate(rows):
        anchors[i] = (qid + dq, sid + ds, sdir, qoff, soff)
    aln, ops, off = ctx.asm_align_batch(ref, reads, 0, 0, anchors, 0.5, 400)
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
    ref.free(); reads.free()


# ---- the consensus stage: necat_cns_load_partition, necat_cns_extension_batch, necat_cns_consensus_batch on the golden reads of tests/golden/cns_c

def _golden_reads(tmp):
    """(per-read code arrays, all codes, read offsets [n + 1]) of the golden project's volumes"""
    wrk = util.install_golden_volumes(MAN["volumes"], tmp)
    codes, sizes = [], []
    for path, _, _ in capi.load_volumes_info(wrk)[2]:
        pac, off, sz, _ = synth.read_volume(path)
        codes.append(synth.unpack_2bit(pac, int(sz.sum())))
        sizes.append(sz)
    codes, sizes = np.concatenate(codes), np.concatenate(sizes).astype(np.int64)
    roff = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    roff[1:] = np.cumsum(sizes)
    return [codes[roff[i]:roff[i + 1]] for i in range(sizes.shape[0])], codes, roff


def _shifted_records(part, k):
    """a candidate partition's records with every read id + k"""
    rec = np.frombuffer(part, dtype="<u4").reshape(-1, 7).copy()
    rec[:, 1] += k
    rec[:, 4] += k
    return rec.view(np.uint8).reshape(-1)


@pytest.fixture(scope="module", params=hv.PLACEMENTS)
def cns_high(request, ctx, tmp_path_factory):
    """the golden reads high in a volume, the golden partition loaded on it and the extension loop's result at the default options"""
    where = request.param
    reads, codes, roff = _golden_reads(tmp_path_factory.mktemp("cns_high"))
    vol, k = hv.place(ctx, reads, where)
    _check_placement(vol, where)
    part = open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read()
    cands, off, n_all = ctx.cns_load_partition(vol, _shifted_records(part, k))
    ext = ctx.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(**MAN["cases"]["default"]["options"]))
    yield where, vol, k, cands, off, ext, reads, codes, roff
    ext.free()
    vol.free()


def test_cns_partition_and_extension_loop(cns_high):
    """the golden log text of test_cns_loop_golden's `default` case (what the reference's consensus driver logged), the ids mapped back"""
    where, vol, k, cands, off, ext, reads, codes, roff = cns_high
    back = cands.copy()
    back["qid"] -= k
    back["sid"] -= k
    assert back["sid"].min() >= 0 and back["qid"].min() >= 0
    txt = util.cns_log_text(ext, back, off, codes, roff, ora.fnv64)
    assert txt.count("\nT\t") + txt.startswith("T\t") == MAN["cases"]["default"]["templates"]
    assert txt == open(os.path.join(util.GOLDEN, "cns_c", "ref_default.txt")).read()


def test_cns_consensus_batch(ctx, cns_high):
    """device path == host path on the high volume (tests/test_gpu_cns_consensus.py's comparison, with its cap on the fallback), and both == the host path on the
    same reads as a small volume - the path the CPU and program tests pin to the manifest's md5s; the templates handed to the host are the same set as there"""
    from tests import test_gpu_cns_consensus as cns_t
    where, vol, k, cands, off, ext, reads, codes, roff = cns_high
    m = MAN["oc2cns"]["default"]
    assert m["options"] == MAN["cases"]["default"]["options"]
    min_cov, min_size = m["options"].get("min_cov", 4), cns_t._opt(m["extra_argv"], "-l", 500)
    dev, examined = cns_t._both(ctx, vol, cands, off, ext, min_cov, min_size)
    low = hv.small(ctx, reads)
    part = np.frombuffer(open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read(), dtype=np.uint8)
    lc, lo, ln = ctx.cns_load_partition(low, part)
    assert np.array_equal(lo, off)
    lext = ctx.cns_extension_batch(low, lc, lo, ln, capi.cns_options(**m["options"]))
    ldev, lexamined = cns_t._both(ctx, low, lc, lo, lext, min_cov, min_size)
    lhost = ctx.cns_consensus_batch(low, lc, lo, lext, capi.cns_consensus_options(min_cov=min_cov, min_size=min_size, full_consensus=0, path=1))
    assert examined == lexamined >= 90 and dev.snapshot() == lhost.snapshot() and dev.segments.shape[0] > 0
    assert np.array_equal(dev.templates["on_host"], ldev.templates["on_host"])
    for r in (dev, ldev, lhost, lext):
        r.free()
    low.free()


# ---- oc2cns -r 1 with both halves of the rescue pair on the device

@pytest.fixture(scope="module")
def long_indels(built, tmp_path_factory):
    """the reads of test_cns_rescue_long_indels_vs_reference, their partition and the log of the reference's consensus driver run with -r 1"""
    tmp = tmp_path_factory.mktemp("high_r1")
    wrk, can, part = util.make_long_indel_partition(tmp)
    want = os.path.join(str(tmp), "ref_r1.txt")
    subprocess.run([ora.REF_CNS] + ora.cns_argv(ora.cns_options()) + ["-r", "1", wrk, can, want, "full"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    codes, sizes = [], []
    for path, _, _ in capi.load_volumes_info(wrk)[2]:
        pac, off, sz, _ = synth.read_volume(path)
        codes.append(synth.unpack_2bit(pac, int(sz.sum())))
        sizes.append(sz)
    codes, sizes = np.concatenate(codes), np.concatenate(sizes).astype(np.int64)
    roff = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    roff[1:] = np.cumsum(sizes)
    return part, open(want).read(), codes, roff


@pytest.mark.skipif(not ora.have_ref_cns(), reason="needs oracle/_ref (the reference's consensus driver; it travels to the GPU box), as test_cns_rescue_long_indels_vs_reference does")
@WHERE
def test_cns_rescue_pair_on_the_device(long_indels, where, monkeypatch):
    """reads with long indels, rescue_long_indels = 1, NECAT_NW_DEVICE=1 and NECAT_DALIGN_DEVICE=1: the log of the reference's consensus driver run with -r 1,
    every candidate's local half and every survivor's global half decided on the device"""
    part, want, codes, roff = long_indels
    monkeypatch.setenv("NECAT_NW_DEVICE", "1")
    monkeypatch.setenv("NECAT_DALIGN_DEVICE", "1")
    c = capi.Context(0)          # knobs are read when a context is created
    try:
        vol, k = hv.place(c, [codes[roff[i]:roff[i + 1]] for i in range(roff.shape[0] - 1)], where)
        _check_placement(vol, where)
        cands, off, n_all = c.cns_load_partition(vol, _shifted_records(part, k))
        res = c.cns_extension_batch(vol, cands, off, n_all, capi.cns_options(rescue_long_indels=1))
        back = cands.copy()
        back["qid"] -= k
        back["sid"] -= k
        txt = util.cns_log_text(res, back, off, codes, roff, ora.fnv64, full=True)
        assert res.n_rescued > 150 and res.n_rescue_tried >= res.n_rescued
        assert res.n_rescue_nw_device == res.n_rescue_nw >= res.n_rescued and res.n_rescue_nw_host == 0
        assert (res.n_rescue_dalign_device, res.n_rescue_dalign_host) == (res.n_rescue_tried, 0)
        res.free()
        vol.free()
    finally:
        c.close()
    assert txt == want


# ---- contig polishing: the crafted goldens of tests/golden/ctg_s, ctg_x and ctg_g, the contigs high and the reads small, then the other way round

def _ctg_volumes(ctx, reads, contigs, where, side):
    """(reads volume, contigs volume, what to add to a read id, what to add to a contig id)"""
    if side == "reads_high":
        rv, k = hv.place(ctx, reads, where)
        _check_placement(rv, where)
        return rv, hv.small(ctx, contigs), k, 0
    cv, k = hv.place(ctx, contigs, where)
    _check_placement(cv, where)
    return hv.small(ctx, reads), cv, 0, k


@WHERE
@SIDE
def test_ctg_seed_batch(ctx, where, side):
    """tests/golden/ctg_s/craft.bin.gz: the reference's matches and candidate per job, on the device path and on the host path"""
    from tests import test_gpu_ctg_seed as seed_t
    cs = sc.read_cases(os.path.join(util.GOLDEN, "ctg_s", "craft.bin.gz"))
    reads, ctg, dq, dc = _ctg_volumes(ctx, cs.reads, cs.contigs, where, side)
    seg = np.zeros(len(cs.segments), dtype=capi.CTG_SEGMENT_DTYPE)
    jobs = np.zeros(cs.n_jobs(), dtype=capi.CTG_SEED_JOB_DTYPE)
    n = 0
    for i, s in enumerate(cs.segments):
        seg[i] = (s.ctg_id + dc, s.size, s.start, n, n + len(s.jobs))
        for qid, qdir in s.jobs:
            jobs[n] = (qid + dq, qdir); n += 1
    dev = seed_t._both(ctx, reads, ctg, seg, jobs)          # path 0 == path 1, no job back to the host
    seed_t._against_golden(cs, dev)
    assert jobs.shape[0] == 115 and dev.max_mems > 128
    reads.free(); ctg.free()


@WHERE
@SIDE
@pytest.mark.parametrize("rescue_path", [0, 1])
def test_ctg_extend_batch(ctx, where, side, rescue_path):
    """tests/golden/ctg_x/craft.bin.gz: per record the reference's verdict, coordinates and columns, the rescue pair on the device and on the host threads"""
    from tests import test_gpu_ctg_extend as ext_t
    cs = xc.load_crafted()
    for s, g in zip(cs.segments, xc.crafted().segments):
        s.tags = g.tags
    reads, ctg, dq, dc = _ctg_volumes(ctx, cs.reads, cs.contigs, where, side)
    seg, jobs, sj, where_of = ext_t._arrays(cs)
    seg["ctg_id"] += dc
    jobs["qid"] += dq
    res = ctx.ctg_extend_batch(reads, 0, ctg, seg, jobs, None, capi.ctg_extend_options(rescue_path=rescue_path))
    res.segments["ctg_id"] -= dc
    res.overlaps["qid"] -= dq
    ext_t._against_golden(cs, res, where_of, True)
    n_used, seeded, tried, won = ext_t._counters(cs, where_of, True)
    assert (res.n_used, res.n_seeded, res.n_aligned, res.n_pair_tried, res.n_pair_accepted) == (n_used, seeded, seeded, tried, won) and won == 2 and tried == 3
    if rescue_path == 0:
        assert res.n_dalign_device == tried and res.n_dalign_host == 0 and res.n_dalign_selfcheck == 0 and res.n_dalign_over_cap == 0
        assert res.n_nw_jobs == won and res.n_nw_device == won and res.n_nw_host == 0
    else:
        assert res.n_dalign_device == 0 and res.n_dalign_host == tried and res.n_nw_host == won
    reads.free(); ctg.free()


@WHERE
@SIDE
def test_ctg_consensus_batch(ctx, where, side):
    """tests/golden/ctg_g/craft.bin.gz: the reference's cns, t_pos and polished segment, on the device path and on the host path"""
    from tests import test_gpu_ctg_consensus as cns_t
    cs = cc.read_cases(os.path.join(util.GOLDEN, "ctg_g", "craft.bin.gz"))
    low_reads, _, seg, ovl, ops = cns_t._upload(ctx, cs, contigs=False)
    low_reads.free()
    reads, ctg, dq, dc = _ctg_volumes(ctx, cs.reads, [c.contig for c in cs.cases], where, side)
    seg["ctg_id"] += dc
    ovl["qid"] += dq
    dev = cns_t._both(ctx, reads, ctg, seg, ovl, ops)          # path 0 == path 1, no fallback
    cns_t._against_golden(cs, dev)
    assert len(cs.cases) == 8
    reads.free(); ctg.free()


# ---- the oc2cns program behind filler volumes

FILLER_READ = 10_000
GATHER_TRACE = re.compile(r"\[oc2cns\] partition (\d+): (\d+) chunks of at most (\d+) bases")


def test_oc2cns_program_behind_filler_volumes(built, tmp_path):
    """the project of tests/test_gpu_cns_gather.py (the golden reads in three volumes) behind sparse filler files of 2^31 + 13 000 bases and more: `auto` takes the
    merged path - one volume of more than 2^31 bases, no gather trace line - and NECAT_CNS_READS=gather writes the same two files: the golden files with
    every ontsa_id_N read as N + fillers (compared after taking the fillers off again: the manifest keeps the golden files' md5s)"""
    built.build_cli()
    tmp = str(tmp_path)
    src = util.install_golden_volumes("vols_c", os.path.join(tmp, "src"))
    fa = os.path.join(tmp, "reads.fasta")
    with open(fa, "w") as f:
        for path, _, _ in capi.load_volumes_info(src)[2]:
            pac, off, sz, names = synth.read_volume(path)
            codes = synth.unpack_2bit(pac, int(sz.sum()))
            for i, nm in enumerate(names):
                f.write(">%s\n%s\n" % (nm, bytes(b"ACGT"[c] for c in codes[int(off[i]):int(off[i] + sz[i])]).decode()))
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write(fa + "\n")
    own = os.path.join(tmp, "own")
    r = subprocess.run([build.OC2MKDB, own, lst], env=dict(os.environ, NECAT_MKDB_VOLSIZE="300000"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    nv, nr, vols = capi.load_volumes_info(own)
    assert (nv, nr) == (3, 98)
    # fillers in front: two files, reads of 10 kb, 2^31 + 13 000 bases - the project's first read begins above 2^31
    per = [110_000, (hv.HALF + 13_000 + FILLER_READ - 1) // FILLER_READ - 110_000]
    wrk = os.path.join(tmp, "wrk")
    os.makedirs(wrk)
    lines, fillers = [], 0
    for n, count in enumerate(per):
        path = os.path.join(wrk, "filler%d" % n)
        assert synth.write_filler_volume(path, "f%d" % n, count, FILLER_READ) == count * FILLER_READ
        lines.append("%s\t%d\t%d\n" % (path, fillers, count))
        fillers += count
    assert hv.HALF < fillers * FILLER_READ and fillers * FILLER_READ + 807_132 < 1 << 32
    for path, first, count in vols:
        lines.append("%s\t%d\t%d\n" % (path, first + fillers, count))
    open(os.path.join(wrk, "volume_names.txt"), "w").writelines(lines)
    open(os.path.join(wrk, "reads_info.txt"), "w").write("%d\t%d\n" % (len(lines), nr + fillers))
    can = os.path.join(tmp, "cands")
    part = open(os.path.join(util.GOLDEN, "cns_c", "cands.p0"), "rb").read()
    open(can + ".p0", "wb").write(_shifted_records(part, fillers).tobytes())
    open(can + ".partitions", "w").write("1\n")
    m = MAN["oc2cns"]["default"]
    argv = ora.cns_argv(ora.cns_options(**m["options"])) + m["extra_argv"] + ["-t", "3"]
    out = {}
    for mode in ("auto", "gather"):
        co, ro = os.path.join(tmp, "cns_" + mode), os.path.join(tmp, "raw_" + mode)
        r = subprocess.run([build.OC2CNS] + argv + [wrk, can, co, ro], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, NECAT_TRACE="2", **({"NECAT_CNS_READS": "gather"} if mode == "gather" else {})))
        assert r.returncode == 0, r.stderr[-3000:]
        assert bool(GATHER_TRACE.search(r.stderr)) == (mode == "gather"), r.stderr[-3000:]
        out[mode] = (open(co, "rb").read(), open(ro, "rb").read())
    assert out["auto"] == out["gather"]
    ids = [int(x) for x in re.findall(rb"ontsa_id_(\d+)", out["auto"][0] + out["auto"][1])]
    assert ids and min(ids) >= fillers
    cns, raw = (re.sub(rb"ontsa_id_(\d+)", lambda x: b"ontsa_id_%d" % (int(x.group(1)) - fillers), b) for b in out["auto"])
    assert (len(cns), cns.count(b">")) == (m["cns_bytes"], m["cns_records"]) and hashlib.md5(cns).hexdigest() == m["cns_md5"]
    assert (len(raw), raw.count(b">")) == (m["raw_bytes"], m["raw_records"]) and hashlib.md5(raw).hexdigest() == m["raw_md5"]


# ---- what is refused below 2^32

def test_refusals_below_2_32(ctx):
    """necat_asm_plan_batch keeps offsets in 32 bits and says so on a volume of 2^31 bases; necat_ctg_extend_batch with the pair on the device refuses a segment
    that ends 2^31 bases into its contig (and takes it with the pair on the host threads)"""
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, 4, n, dtype=np.uint8) for n in (500, 3000, 700)]
    big, k = hv.place(ctx, seqs, "straddle")
    assert big.nbases >= 1 << 31
    tiny = hv.small(ctx, seqs)
    opt = capi.default_options(**dict(util.FAST, job=1))
    ix = ctx.build_index(tiny, opt.kmer_size, opt.kmer_cnt_cutoff)
    for ref, reads in ((big, tiny), (tiny, big)):
        plan, first = C.c_void_p(), C.c_void_p()
        rc = ctx.lib.necat_asm_plan_batch(ctx.h, ix.h, ref.h, reads.h, 0, 0, C.byref(opt), C.byref(plan), C.byref(first))
        assert rc == -1 and not plan and not first
        assert "32-bit offsets" in ctx.lib.necat_last_error(ctx.h).decode()
    ix.free()
    big.free()
    # one contig of 2^31 bases (zeros), a segment over its last 3 000 bases with one job
    n = 1 << 31
    contig = ctx.upload_volume(hv._pac(n // 4), n, np.zeros(1, np.int64), np.array([n], dtype=np.int64))
    seg = np.zeros(1, dtype=capi.CTG_SEGMENT_DTYPE)
    seg[0] = (0, 3000, n - 3000, 0, 1)
    jobs = np.zeros(1, dtype=capi.CTG_EXTEND_JOB_DTYPE)
    jobs["qid"], jobs["soff"], jobs["send"] = 1, n - 3000, n
    with pytest.raises(capi.NecatError, match=r"\(-1\).*ends 2\^31 bases or more into its contig"):
        ctx.ctg_extend_batch(tiny, 0, contig, seg, jobs, None, capi.ctg_extend_options(rescue_path=0))
    seg["from"] -= 1          # ends one base earlier: taken
    res = ctx.ctg_extend_batch(tiny, 0, contig, seg, jobs, None, capi.ctg_extend_options(rescue_path=0))
    assert res.jobs.shape[0] == 1
    contig.free(); tiny.free()
