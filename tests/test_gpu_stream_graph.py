"""The stream graph of a context (NECAT_STREAM_GRAPH, knobs.h): 1 = list A's chain on the context's own stream, list B's streams made when the context is made, the stream of
the un-merged ragged chain only where the knobs select a path that launches on it; 0 = the graph until then (five streams, four of them made by the first extension call).
A dependency lost between two streams shows up as a race and wrong records, not as a hang, so every case compares records: both graphs with each other and the oracle,
contexts on host threads with a context that ran alone, a call cut into batches on two lanes, and the launcher variants that need the streams the default path does not."""
import os
import threading

import numpy as np
import pytest

from tests import util
from oracle import oracle_api as ora

pytestmark = pytest.mark.gpu


def _context(env):
    """a context that read `env` (knobs are read when a context is made); the environment is left as it was"""
    from necat_amd import capi
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = capi.Context(0)
        for k, v in env.items():
            assert c.knob(k) == v, (k, c.knob(k))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return c


def _sorted(m4):
    return np.sort(m4.copy(), order=list(m4.dtype.names))


@pytest.fixture(scope="module")
def small(tmp_path_factory, ctx):
    """the 150-kb set of test_gpu_parity.py, its M4 records by the oracle and by the session's context (default knobs), computed once"""
    from necat_amd import capi
    tmp = tmp_path_factory.mktemp("stream_graph")
    d, rs, nv = util.make_dataset(tmp, genome=150_000, coverage=18.0, seed=5)
    out = os.path.join(str(tmp), "oracle.m4")
    ora.pm_main(ora.options(**dict(util.FAST, job=1, binary_output=1)), 0, d, out)
    ref = np.frombuffer(open(out, "rb").read(), dtype=capi.M4_DTYPE)
    opt = capi.default_options(**dict(util.FAST, job=1))
    _, base = capi.pm_main(ctx, opt, 0, d)
    assert base.shape[0] > 500 and util.m4_key_rows(base) == util.m4_key_rows(ref)
    return d, opt, ref, _sorted(base)


def test_the_default_is_the_new_graph(ctx):
    assert ctx.knob("NECAT_STREAM_GRAPH") == "1"


def test_one_context_both_graphs(small):
    """NECAT_STREAM_GRAPH=0 and =1: the M4 records are equal as sorted arrays, and equal to the oracle's"""
    from necat_amd import capi
    d, opt, ref, base = small
    got = {}
    for g in ("0", "1"):
        c = _context({"NECAT_STREAM_GRAPH": g})
        try:
            _, m4 = capi.pm_main(c, opt, 0, d)
            _, again = capi.pm_main(c, opt, 0, d)          # (the second call of a context finds its streams and events used)
        finally:
            c.close()
        got[g] = _sorted(m4)
        assert np.array_equal(got[g], _sorted(again))
        assert util.m4_key_rows(m4) == util.m4_key_rows(ref)
    assert np.array_equal(got["0"], got["1"]) and np.array_equal(got["1"], base)


def test_contexts_on_threads(ctx):
    """four contexts on four host threads, two steps each (index build + map_pair) over ONE resident volume, under the new graph: every step's records are those of a
    context that ran alone (the 300-kb set of test_gpu_cli_golden.py)"""
    from necat_amd import capi, synth
    rs = synth.simulate_reads(300_000, 20.0, seed=5)
    pac = synth.pack_2bit(rs.codes)
    kw = dict(kmer_size=13, scan_window=10, kmer_cnt_cutoff=500, block_size=2000, block_score_cutoff=3, num_candidates=500, align_size_cutoff=1000, error=0.5, use_hdr_as_id=0)
    opt = capi.default_options(**dict(kw, job=1))
    ctxs = [_context({"NECAT_STREAM_GRAPH": "1"}) for _ in range(4)]
    vol = ctxs[0].upload_volume(pac, rs.nbases, rs.offsets, rs.sizes)

    def one(c):
        ix = c.build_index(vol, opt.kmer_size, opt.kmer_cnt_cutoff)
        m4, nc = c.map_pair(ix, vol, vol, 0, 0, opt, True, 1)
        ix.free()
        return nc, _sorted(m4)
    try:
        nc0, want = one(ctxs[0])
        assert want.shape[0] > 1000
        got, errs = {}, []

        def work(i):
            try:
                for rep in range(2):
                    got[(i, rep)] = one(ctxs[i])
            except BaseException as e:
                errs.append(e)
        th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        assert len(got) == 8
        for nc, m4 in got.values():
            assert nc == nc0 and np.array_equal(m4, want)
    finally:
        vol.free()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_several_batches_on_two_lanes(small, graph):
    """a call cut into batches of 320 candidates (NECAT_BATCH): batch i + 1 runs on lane 1's streams beside batch i on lane 0's - same records under both graphs"""
    from necat_amd import capi
    d, opt, ref, base = small
    c = _context({"NECAT_STREAM_GRAPH": graph, "NECAT_BATCH": "320"})
    try:
        assert c.knob("NECAT_EXT_LANES") == "2" and c.knob("NECAT_EXT_OVERLAP") == "1"
        cands, m4 = capi.pm_main(c, opt, 0, d)
    finally:
        c.close()
    assert cands.shape[0] > 2 * 320          # more than two batches: both lanes ran, and lane 0 took a second batch
    assert np.array_equal(_sorted(m4), base)


@pytest.mark.parametrize("knobs", ["NECAT_TAIL_FUSED=0", "NECAT_RC_MERGE=0", "NECAT_RC_MERGE=0 NECAT_RCWALK=1 NECAT_TAIL_FUSED=0", "NECAT_LISTB_STREAMS=1", "NECAT_LISTB_PRIO=1",
                                   "NECAT_LISTB_PRIO=2 NECAT_BATCH=320"])
def test_launcher_variants(small, knobs):
    """under the new graph: no round through the one-launch tail kernel; the ragged blocks of a big round on a chain of their own (NECAT_RC_MERGE=0 - the path that launches
    on stream d, which a context makes only when its knobs ask for such a path), also in every round; one list-B stream; list B's streams in another priority pool"""
    from necat_amd import capi
    d, opt, ref, base = small
    c = _context(dict({"NECAT_STREAM_GRAPH": "1"}, **dict(kv.split("=") for kv in knobs.split())))
    try:
        _, m4 = capi.pm_main(c, opt, 0, d)
    finally:
        c.close()
    assert np.array_equal(_sorted(m4), base)
