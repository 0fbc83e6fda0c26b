"""The shapes the device form of ocda_go (DALIGNER's local alignment around an anchor) is tested on - tests/test_dalign_device_model.py on the CPU model,
tests/test_gpu_dalign.py on the GPU, tests/tools/make_golden_dalign.py for what the reference returns on them: the smallest inputs at which each rule of
rescue::local_alignment can go wrong.  A case: name, read (the query's read on its forward strand), tmpl, qdir, qs, ts (the anchor: query start on the
query's strand, subject start), error, min_size."""
import numpy as np

from tests import test_rescue as T


def revcomp(a):
    return (3 - a[::-1]).astype(np.uint8)


def _case(name, q, t, qs, ts, error=0.5, min_size=100, qdir=0):
    q = np.ascontiguousarray(q, dtype=np.uint8)
    return dict(name=name, read=revcomp(q) if qdir else q, tmpl=np.ascontiguousarray(t, dtype=np.uint8), qdir=qdir, qs=int(qs), ts=int(ts), error=float(error),
                min_size=int(min_size))


def query_of(c):
    """the query strand the host code is handed"""
    return revcomp(c["read"]) if c["qdir"] else c["read"]


def shape_cases():
    rng = np.random.default_rng(411)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)      # noqa: E731
    out = []
    # identical sequences: the anchor in the middle and on either end (wave 0 alone reaches both ends)
    t7 = rnd(700)
    for a in (350, 0, 699):
        out.append(_case("same700_at%d" % a, t7, t7, a, a))
    # the anchor on either side of the 2-bit words' boundaries (32 bases a word), the subject one base on
    t15 = rnd(1500)
    q15 = T.mutate(t15, rng, 0.15)
    for a in (31, 32, 33, 63, 64, 65):
        out.append(_case("word%d" % a, q15, t15, a, a + 1))
    # unrelated sequences: at error 0.5 the wave runs on, more than 64 diagonals wide
    out.append(_case("unrelated", rnd(1500), rnd(1500), 750, 750))
    # a long deletion and its transpose: the window has to reach the other side's diagonal
    t3 = rnd(3000)
    q3 = T.mutate(t3, rng, 0.12, (1500, 600))
    out.append(_case("deletion600", q3, t3, 300, 300))
    out.append(_case("insertion600", t3, q3, 300, 300))
    # sizes around min_align_size
    t150 = rnd(150)
    out.append(_case("pair150", T.mutate(t150, rng, 0.1), t150, 70, 70))
    out.append(_case("same100", t7[:100], t7[:100], 50, 50))
    out.append(_case("same99", t7[:99], t7[:99], 50, 50))
    # the query inside the target and the transpose: an a-end and a b-end are reached
    t2 = rnd(2000)
    q2 = T.mutate(t2[600:1400], rng, 0.1)
    out.append(_case("inside", q2, t2, 400, 1000))
    out.append(_case("around", t2, q2, 1000, 400))
    # a noisy pair that the loose setting follows to both ends and the strict one trims to a local result
    t35 = rnd(2000)
    left, mid, right = T.mutate(t35[:650], rng, 0.35), T.mutate(t35[650:1350], rng, 0.08), T.mutate(t35[1350:], rng, 0.35)
    q35 = np.concatenate([left, mid, right])
    out.append(_case("noisy_e50", q35, t35, len(left) + 350, 1000, error=0.5))
    out.append(_case("noisy_e20", q35, t35, len(left) + 350, 1000, error=0.2))
    # equal diagonals: a period-7 tandem repeat with the anchor one base off, a homopolymer with the anchor 20 off
    unit = np.array([0, 1, 2, 3, 1, 0, 2], dtype=np.uint8)
    rep = np.tile(unit, 120)
    out.append(_case("tandem7", rep, rep, 400, 401))
    out.append(_case("homopolymer", np.zeros(600, dtype=np.uint8), np.zeros(600, dtype=np.uint8), 300, 320))
    # unrelated flanks of 300 bp on both sides of either sequence
    core = rnd(900)
    out.append(_case("flanks", np.concatenate([rnd(300), T.mutate(core, rng, 0.1), rnd(300)]), np.concatenate([rnd(300), core, rnd(300)]), 700, 700))
    # the anchor 30 bp off the true diagonal
    t12 = rnd(1200)
    out.append(_case("off30", T.mutate(t12, rng, 0.05), t12, 600, 630))
    # every third once more from the read's reverse strand
    for c in list(out[::3]):
        out.append(_case(c["name"] + "_rc", c["read"], c["tmpl"], c["qs"], c["ts"], error=c["error"], min_size=c["min_size"], qdir=1))
    return out


def golden_rescue_cases():
    """the 60 ocda_go cases of tests/golden/rescue_cases.json as cases (name = "seed<N>")"""
    return seed_cases(range(2000, 2060), qdir_every=0)


def seed_cases(seeds, qdir_every=5):
    """random read pairs as tests/test_rescue.py::ocda_inputs draws them, every qdir_every-th from the read's reverse strand (0: none)"""
    out = []
    for seed in seeds:
        c = T.ocda_inputs(seed)
        if c is None:
            continue
        q, t, qs, ts, e = c
        out.append(_case("seed%d" % seed, q, t, qs, ts, error=e, qdir=1 if qdir_every and seed % qdir_every == 0 else 0))
    return out


def host_result(mine_lib, c):
    """rescue::Dalign::go through tests/host_core/rescue_capi.cpp: (ret, [abpos aepos bbpos bepos diffs], ident) - the coordinates also when ret is 0"""
    import ctypes as C
    q = np.ascontiguousarray(query_of(c))
    o, ident = (C.c_int * 6)(), C.c_double()
    r = mine_lib.mine_ocda_go(T.ptr(q), c["qs"], len(q), T.ptr(c["tmpl"]), c["ts"], len(c["tmpl"]), C.c_double(c["error"]), c["min_size"], o, C.byref(ident))
    return (r, list(o)[:5], ident.value if r else 0.0)


# ---- the cases through necat_local_align_batch (tests/test_gpu_dalign.py at the front of small volumes, tests/test_gpu_high_offsets.py high in a large one) ----

def run_cases(ctx, cases, volumes=None):
    """the cases through necat_local_align_batch, one call per (error, min_size) among them: per case (ok, [qoff qend soff send diffs], ident, how) as
    host_result gives the first three, and the calls' stats.  `volumes(ctx, reads, tmpls)` builds the two volumes and says which global ids their first test
    sequences have (tests.nw_cases.packed_volumes by default)"""
    from necat_amd import capi
    from tests import nw_cases
    reads, ref, read0, ref0 = (volumes or nw_cases.packed_volumes)(ctx, [c["read"] for c in cases], [c["tmpl"] for c in cases])
    out, stats = [None] * len(cases), []
    for key in sorted({(c["error"], c["min_size"]) for c in cases}):
        idx = [i for i, c in enumerate(cases) if (c["error"], c["min_size"]) == key]
        jobs = np.zeros(len(idx), dtype=capi.DALIGN_JOB_DTYPE)
        for k, i in enumerate(idx):
            c = cases[i]
            jobs[k] = (read0 + i, c["qdir"], c["qs"], ref0 + i, c["ts"])
        res, st = ctx.local_align_batch(ref, reads, nw_cases.READ0, nw_cases.REF0, jobs, error=key[0], min_align_size=key[1])
        assert res.shape[0] == len(idx) and st.n_device + st.n_host == len(idx) and st.n_host == st.n_selfcheck + st.n_over_cap
        stats.append(st)
        for k, i in enumerate(idx):
            r = res[k]
            out[i] = (int(r["ok"]), [int(r[f]) for f in ("qoff", "qend", "soff", "send", "diffs")], float(r["ident_perc"]), int(r["how"]))
    reads.free(); ref.free()
    return out, stats


def all_on_device(got, stats):
    return not any(r[3] for r in got) and all(st.n_host == 0 and st.n_selfcheck == 0 and st.n_over_cap == 0 for st in stats)
