"""GPU tests of the size-class order of a round's ragged blocks (NECAT_ITEM_SORT, necat_amd/csrc/item_order.h).  A block's result does not depend on
its work index, so the order may change nothing: the -j 1 M4 records and the alignments of necat_onc_align_batch are the same with the order on and off - under
the default round and under every alternative round launcher - and are the oracle's.  The device's own counters (necat_get_item_order_stats) then show what the
order is for: the lane-steps the checkpoint passes issue stay within the bound of tests/host_core/check_item_order.cpp of those their blocks need."""
import os

import numpy as np
import pytest

from tests import util
from oracle import oracle_api as ora

pytestmark = pytest.mark.gpu

TAIL = 4
N_ORACLE_ALIGN = 300          # alignments compared with the oracle's one by one (every k-th candidate; the two orders are compared on all of them)


@pytest.fixture(scope="module")
def ref(ctx, tmp_path_factory):
    """the 150-kb-genome read set of the parity tests; computed once: the oracle's M4 records, the candidates, the oracle's alignments of a sample of them"""
    from necat_amd import capi
    tmp = tmp_path_factory.mktemp("item_order")
    d, rs, nv = util.make_dataset(tmp, genome=150_000, coverage=18.0, seed=5)
    out = os.path.join(str(tmp), "oracle_m4.out")
    st = ora.pm_main(ora.options(**dict(util.FAST, job=1, binary_output=1)), 0, d, out)
    m4 = np.frombuffer(open(out, "rb").read(), dtype=capi.M4_DTYPE)
    assert m4.shape[0] == st.n_records > 500
    o0 = capi.default_options(**dict(util.FAST, job=0))
    cands, _ = capi.pm_main(ctx, o0, 0, d)
    assert cands.shape[0] > 1000          # (more than NECAT_TAIL_FUSED / NECAT_RCWALK's 512 blocks a round: the first rounds go through the checkpoint pass)
    al = ora.Aligner(o0.error)
    sample = {}
    for i in range(0, cands.shape[0], max(1, cands.shape[0] // N_ORACLE_ALIGN)):
        c = cands[i]
        q = rs.codes[rs.offsets[c["qid"]]: rs.offsets[c["qid"]] + rs.sizes[c["qid"]]]
        if c["qdir"] == 1:
            q = (3 - q[::-1]).astype(np.uint8)
        t = rs.codes[rs.offsets[c["sid"]]: rs.offsets[c["sid"]] + rs.sizes[c["sid"]]]
        sample[i] = (q, t, al.align(q, int(c["qoff"]), t, int(c["soff"]), o0.align_size_cutoff, TAIL))
    al.close()
    return {"d": d, "m4": util.m4_key_rows(m4), "cands": cands, "sample": sample}


def _run(ref, monkeypatch, env):
    """-j 1 records, alignments and the counters of the -j 1 call from a fresh context made under `env`"""
    from necat_amd import capi
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(0)          # knobs are read when a context is created
    try:
        assert not c.xcheck and all(c.knob(k) == v for k, v in env.items() if not k.endswith("_MB"))
        o1 = capi.default_options(**dict(util.FAST, job=1))
        _, m4 = capi.pm_main(c, o1, 0, ref["d"])
        st, rounds = c.item_order_stats(), int(c.timings().rounds)
        _, _, vols = capi.load_volumes_info(ref["d"])
        vol = c.load_volume(vols[0][0])
        aln, ops, off = c.onc_align_batch(vol, vol, 0, 0, ref["cands"], o1, TAIL)
        vol.free()
    finally:
        c.close()
        monkeypatch.undo()
    return util.m4_key_rows(m4), (aln, ops, off), st, rounds


def _check_against_oracle(ref, m4, al):
    from necat_amd import capi
    assert m4 == ref["m4"]
    aln, ops, off = al
    assert aln.shape[0] == ref["cands"].shape[0]
    n_ok = 0
    for i, (q, t, (ok, qoff, qend, toff, tend, ident, qa, ta)) in ref["sample"].items():
        a = aln[i]
        assert (bool(a["ok"]), int(a["qoff"]), int(a["qend"]), int(a["toff"]), int(a["tend"]), int(a["align_size"])) == (ok, qoff, qend, toff, tend, len(qa)), i
        assert float(a["ident_perc"]) == ident, i
        assert capi.gapped_strings(ops[int(off[i]):int(off[i + 1])], int(a["align_size"]), q, qoff, t, toff) == (qa, ta), i
        n_ok += ok
    assert n_ok > len(ref["sample"]) // 3


def _waste_bound(blocks, rounds, classes, group, longest):
    """check_item_order.cpp's bound for the lists of `rounds` rounds: within a class blocks differ by fewer than 32 steps; per list at most one group straddles each
    class boundary (list A: the first ragged group may hold full blocks)"""
    return 31 * blocks + rounds * classes * group * longest


KNOBS = [
    "",                                                                  # (a) the default round
    "NECAT_RC_POOL_MB=1",
    "NECAT_RC_PIPE=3 NECAT_RC_PIPE_MIN=64",
    "NECAT_RC_MERGE=0",
    "NECAT_FRAG_FUSE=0",
    "NECAT_TAIL_FUSED=0 NECAT_RCWALK=1",
    "NECAT_BATCH=1024 NECAT_EXT_LANES=2",
    "NECAT_BATCH=1024 NECAT_EXT_LANES=3",
]


@pytest.mark.parametrize("knob", KNOBS)
def test_same_records_with_and_without_the_order(ref, monkeypatch, knob):
    """(a), (b): M4 records and alignments with NECAT_ITEM_SORT=1 and =0 are the same and the oracle's, under the default round and each alternative launcher;
    (c) under the default round the counters of the ordered run keep the bound, those of the other run are printed"""
    env = dict(kv.split("=") for kv in knob.split())
    m_on, a_on, st_on, rounds_on = _run(ref, monkeypatch, dict(env, NECAT_ITEM_SORT="1"))
    m_off, a_off, st_off, rounds_off = _run(ref, monkeypatch, dict(env, NECAT_ITEM_SORT="0"))
    assert m_on == m_off
    for x, y in zip(a_on, a_off):
        assert x.tobytes() == y.tobytes()
    _check_against_oracle(ref, m_on, a_on)
    for tag, st, rounds in (("order on ", st_on, rounds_on), ("order off", st_off, rounds_off)):
        print("%s [%s]: rounds %d | list A ragged waves: blocks %d issued %d needed %d | list B waves: blocks %d issued %d needed %d"
              % (tag, knob, rounds, st.a_blocks, st.a_issued, st.a_needed, st.b_blocks, st.b_issued, st.b_needed))
    if not knob:
        assert st_on.a_blocks > 0 and st_on.a_needed > 0 and st_on.a_issued >= st_on.a_needed
        assert st_on.b_issued >= st_on.b_needed
        assert st_on.a_issued - st_on.a_needed <= _waste_bound(st_on.a_blocks, rounds_on, 16, 8, 512 + 8 - 1)
        assert st_on.b_issued - st_on.b_needed <= _waste_bound(st_on.b_blocks, rounds_on, 9, 4, 794 + 13 - 1)
        # the blocks are the same whatever their order (list A's ragged waves may hold full blocks too, which ones follows the order)
        assert st_on.b_needed == st_off.b_needed and st_on.b_blocks == st_off.b_blocks
