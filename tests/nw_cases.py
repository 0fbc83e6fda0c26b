"""The shapes the device form of edlib_go is tested on (tests/test_nw_device_model.py on the CPU model, tests/test_gpu_nw.py on the GPU,
tests/golden/make_golden_nw.py for what the reference returns on them): the smallest inputs at which each rule of rescue::EdlibGo::go and
NwPath::solve can go wrong.  A case: name, read (the query's read on its forward strand), tmpl, qdir, qf, qt, tf, tt, error, tol, min_size."""
import numpy as np

from tests import test_rescue as T


def revcomp(a):
    return (3 - a[::-1]).astype(np.uint8)


def edit_distance(q, t):
    """global edit distance, a row at a time"""
    n = len(t)
    idx = np.arange(n + 1)
    prev = idx.copy()
    for i in range(1, len(q) + 1):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (t != q[i - 1]), prev[1:] + 1)
        cur = np.minimum.accumulate(cur - idx) + idx
        prev = cur
    return int(prev[n])


def _case(name, q, t, qf, qt, tf, tt, error, tol, min_size=100, qdir=0):
    q = np.ascontiguousarray(q, dtype=np.uint8)
    return dict(name=name, read=revcomp(q) if qdir else q, tmpl=np.ascontiguousarray(t, dtype=np.uint8), qdir=qdir, qf=int(qf), qt=int(qt), tf=int(tf), tt=int(tt),
                error=float(error), tol=int(tol), min_size=int(min_size))


def query_of(c):
    """the query strand the host code is handed"""
    return revcomp(c["read"]) if c["qdir"] else c["read"]


def _fit(q, rng, n):
    return q[:n] if len(q) >= n else np.concatenate([q, rng.integers(0, 4, n - len(q), dtype=np.uint8)])


def shape_cases():
    rng = np.random.default_rng(77)
    out = []
    t300 = rng.integers(0, 4, 300, dtype=np.uint8)
    q300 = T.mutate(t300, rng, 0.1)
    for L in (1, 63, 64, 65, 128):
        # a word boundary of rows, then of columns
        out.append(_case("rows%d" % L, t300[100:100 + L], t300, 0, L, 0, 300, 1e9, 400))
        out.append(_case("cols%d" % L, q300, t300[100:100 + L], 0, len(q300), 0, L, 1e9, 400, min_size=0))
    t48 = rng.integers(0, 4, 5000, dtype=np.uint8)
    out.append(_case("one_word_4800", t48, t48, 0, 64, 0, 4800, 1e9, 5000))
    out.append(_case("4800_one_word", t48, t48, 0, 4800, 0, 64, 1e9, 5000, min_size=0))
    # the leaf limit from both sides with the same sequences: 29 words of rows, 20 * 29 * n + 8 * n against 2^20
    t18 = rng.integers(0, 4, 1784, dtype=np.uint8)
    q18 = _fit(T.mutate(t18, rng, 0.15), rng, 1800)
    out.append(_case("leaf_1783", q18, t18, 0, 1800, 0, 1783, 0.5, 900))
    out.append(_case("split_1784", q18, t18, 0, 1800, 0, 1784, 0.5, 900))
    # a split with one word of rows: the "row -1" / "row m - 1" fallbacks
    t40k = rng.integers(0, 4, 40000, dtype=np.uint8)
    out.append(_case("split_m41", t40k[20000:20041], t40k, 0, 41, 0, 40000, 1e9, 40000))
    out.append(_case("split_m41_front", t40k[3:44], t40k, 0, 41, 0, 40000, 1e9, 40000))
    # the reject rules on either side of their thresholds
    t6 = rng.integers(0, 4, 600, dtype=np.uint8)
    out.append(_case("tol_below_diff", t6[:570], t6, 0, 570, 0, 600, 0.5, 29))
    out.append(_case("tol_at_diff", t6[:570], t6, 0, 570, 0, 600, 0.5, 30))
    q6 = T.mutate(t6, rng, 0.1)
    best = edit_distance(q6, t6)
    out.append(_case("best_at_tol", q6, t6, 0, len(q6), 0, 600, 0.5, best))
    out.append(_case("best_above_tol", q6, t6, 0, len(q6), 0, 600, 0.5, best - 1))
    out.append(_case("len_at_min", q6, t6, 0, len(q6), 0, 600, 0.5, 300, min_size=599))
    out.append(_case("len_below_min", q6, t6, 0, len(q6), 0, 600, 0.5, 300, min_size=600))
    e0 = best / 599.0
    out.append(_case("error_at", q6, t6, 0, len(q6), 0, 600, e0, 300))
    out.append(_case("error_above", q6, t6, 0, len(q6), 0, 600, float(np.nextafter(e0, 0.0)), 300))
    # unrelated sequences (trimming by chance runs of 4 only), and a pair without any run of 4 matches
    out.append(_case("unrelated", rng.integers(0, 4, 1500, dtype=np.uint8), rng.integers(0, 4, 1500, dtype=np.uint8), 0, 1500, 0, 1500, 1e9, 1500))
    out.append(_case("no_run", np.zeros(600, dtype=np.uint8), np.ones(600, dtype=np.uint8), 0, 600, 0, 600, 1e9, 600))
    # the reverse strand of the read, ranges inside both sequences, a split
    t9 = rng.integers(0, 4, 5200, dtype=np.uint8)
    q9 = T.mutate(t9[100:5100], rng, 0.15, (2000, 300))
    out.append(_case("qdir1_split", q9, t9, 20, len(q9) - 15, 110, 5090, 0.5, int(0.4 * len(q9)), qdir=1))
    out.append(_case("qdir1_leaf", q300, t300, 3, len(q300) - 2, 1, 299, 0.5, 120, qdir=1))
    # more than one stripe of 64 words (rows beyond 4096) with a band wider than a stripe
    t7 = rng.integers(0, 4, 9000, dtype=np.uint8)
    q7 = T.mutate(t7, rng, 0.25, (4000, 500))
    out.append(_case("two_stripes", q7, t7, 0, len(q7), 0, 9000, 0.5, int(0.6 * len(q7))))
    return out


def golden_rescue_cases():
    """the 60 edlib_go cases of tests/golden/rescue_cases.json as cases (name = "seed<N>")"""
    out = []
    for seed in range(3000, 3060):
        c = T.edlib_inputs(seed, seed % 4 == 3)
        if c is None:
            continue
        q, t, qf, qt, tf, tt, error, tol = c
        out.append(_case("seed%d" % seed, q, t, qf, qt, tf, tt, error, tol))
    return out


def edge_cases():
    """the ten cases of tests/test_rescue.py::test_edlib_go_edges"""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, 5000, dtype=np.uint8)
    q = t.copy()
    cases = [(q, t, 0, 5000, 0, 5000, 0.5, 100), (q, t, 0, 5000, 0, 5000, 0.5, 0), (q, t, 0, 4000, 0, 5000, 0.5, 999), (q, t, 0, 4000, 0, 5000, 0.5, 1000),
             (q, t, 100, 4100, 0, 5000, 0.5, 2000), (q, t, 0, 120, 0, 90, 0.5, 60), (q, t, 0, 64, 0, 4800, 1e9, 5000), (q, t, 0, 4800, 0, 130, 1e9, 5000)]
    q2 = T.mutate(t, rng, 0.4)
    cases.append((q2, t, 0, len(q2), 0, 5000, 0.2, 4000))
    q3 = rng.integers(0, 4, 5000, dtype=np.uint8)
    cases.append((q3, t, 0, 5000, 0, 5000, 1e9, 5000))
    return [_case("edge%d" % i, *c) for i, c in enumerate(cases)]


def seed_cases(seeds, qdir_every=5):
    """random read pairs as test_edlib_go_matches_reference draws them: small ones (a leaf) and, every fourth, big ones (nested splits)"""
    out = []
    for seed in seeds:
        c = T.edlib_inputs(seed, seed % 4 == 3)
        if c is None:
            continue
        q, t, qf, qt, tf, tt, error, tol = c
        out.append(_case("seed%d" % seed, q, t, qf, qt, tf, tt, error, tol, qdir=1 if seed % qdir_every == 0 else 0))
    return out


def host_result(mine_lib, c):
    """rescue::EdlibGo::go through tests/host_core/rescue_capi.cpp: (ret,) or (ret, [qoff qend toff tend dist n], ident, qaln, taln)"""
    import ctypes as C
    q = np.ascontiguousarray(query_of(c))
    cap = (c["qt"] - c["qf"]) + (c["tt"] - c["tf"]) + 16
    o, ident = (C.c_int * 6)(), C.c_double()
    qa, ta = C.create_string_buffer(cap), C.create_string_buffer(cap)
    r = mine_lib.mine_edlib_go(T.ptr(q), c["qf"], c["qt"], T.ptr(c["tmpl"]), c["tf"], c["tt"], C.c_double(c["error"]), c["tol"], c["min_size"], o, C.byref(ident), qa, ta, cap)
    return (r,) if not r else (r, list(o), ident.value, qa.value, ta.value)


# ---- the cases through necat_nw_path_batch (tests/test_gpu_nw.py at the front of small volumes, tests/test_gpu_high_offsets.py high in a large one) ----

READ0, REF0 = 7, 3          # the volumes' first global ids


def pack(ctx, seqs):
    """the sequences as a volume of their own through necat_volume_pack"""
    import ctypes as C
    from necat_amd import capi
    sizes = np.array([len(s) for s in seqs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    text = bytes(b"ACGT"[c] for c in np.concatenate(seqs))
    vol = C.c_void_p()
    rc = ctx.lib.necat_volume_pack(ctx.h, text, len(text), offs.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p), len(sizes), None, C.byref(vol))
    assert rc == 0, ctx.lib.necat_last_error(ctx.h).decode()
    return capi.Volume(ctx, vol, len(text), offs.astype(np.int64), sizes.astype(np.int64))


def packed_volumes(ctx, reads, tmpls):
    """the default volume builder of run_cases: (reads volume, ref volume, global id of reads[0], global id of tmpls[0])"""
    return pack(ctx, reads), pack(ctx, tmpls), READ0, REF0


def run_cases(ctx, cases, volumes=packed_volumes):
    """the cases through necat_nw_path_batch, one call per (error, min_size) among them: results as host_result gives them, and the calls' stats.
    `volumes(ctx, reads, tmpls)` builds the two volumes and says which global ids their first test sequences have"""
    from necat_amd import capi
    reads, ref, read0, ref0 = volumes(ctx, [c["read"] for c in cases], [c["tmpl"] for c in cases])
    out, stats = [None] * len(cases), []
    for key in sorted({(c["error"], c["min_size"]) for c in cases}):
        idx = [i for i, c in enumerate(cases) if (c["error"], c["min_size"]) == key]
        jobs = np.zeros(len(idx), dtype=capi.NW_JOB_DTYPE)
        for k, i in enumerate(idx):
            c = cases[i]
            jobs[k] = (read0 + i, c["qdir"], c["qf"], c["qt"], ref0 + i, c["tf"], c["tt"], c["tol"])
        res, ops, off, st = ctx.nw_path_batch(ref, reads, READ0, REF0, jobs, error=key[0], min_align_size=key[1])
        assert off.shape[0] == len(idx) + 1 and not (off % 8).any()
        assert st.n_host == 0 and st.n_selfcheck == 0 and st.n_device == len(idx)
        assert not res["how"].any()
        stats.append(st)
        for k, i in enumerate(idx):
            r, c = res[k], cases[i]
            if not r["ok"]:
                assert off[k + 1] == off[k]
                out[i] = (0,)
                continue
            n = int(r["align_size"])
            assert off[k + 1] - off[k] == ((n + 3) // 4 + 7) // 8 * 8
            qa, ta = capi.gapped_strings(ops[int(off[k]):int(off[k + 1])], n, query_of(c), int(r["qoff"]), c["tmpl"], int(r["toff"]))
            out[i] = (1, [int(r["qoff"]), int(r["qend"]), int(r["toff"]), int(r["tend"]), int(r["dist"]), n], float(r["ident_perc"]), bytes(qa), bytes(ta))
    reads.free(); ref.free()
    return out, stats


def hashed(r):
    from oracle import oracle_api as ora
    return r if not r[0] else (r[0], r[1], r[2], ora.fnv64(r[3]), ora.fnv64(r[4]))


def golden_of(g):
    return (g["ret"],) if not g["ret"] else (g["ret"], g["out"], g["ident"], g["qaln"], g["taln"])
