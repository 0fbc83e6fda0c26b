"""ctypes binding of libnecat_hip.so (include/necat_hip.h) + a Python mirror of pm_main.

The product is the C ABI and the oc2pmov program on top of it; this module only lets tests and
bench.py drive the same entry points.  No computation happens in Python, and there is no CPU
fallback: if the library or a GPU is missing every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import List, Optional, Tuple

import numpy as np

from . import build as _build
from .synth import read_volume


class MapOptions(C.Structure):
    """common/map_options.h:10-25"""
    _fields_ = [("kmer_size", C.c_int), ("scan_window", C.c_int), ("kmer_cnt_cutoff", C.c_int),
                ("block_size", C.c_int), ("block_score_cutoff", C.c_int), ("num_candidates", C.c_int),
                ("align_size_cutoff", C.c_int), ("ddfs_cutoff", C.c_double), ("error", C.c_double),
                ("num_output", C.c_int), ("num_threads", C.c_int), ("job", C.c_int),
                ("binary_output", C.c_int), ("use_hdr_as_id", C.c_int)]


class Timings(C.Structure):
    _fields_ = [("index_ms", C.c_double), ("seed_ms", C.c_double), ("extend_ms", C.c_double),
                ("myers_ms", C.c_double), ("traceback_ms", C.c_double), ("myers_launches", C.c_uint64),
                ("myers_blocks", C.c_uint64), ("myers_word_updates", C.c_uint64),
                ("myers_cells_bases", C.c_uint64), ("rounds", C.c_uint64),
                ("myersA_ms", C.c_double), ("myersA_launches", C.c_uint64), ("myersA_blocks", C.c_uint64),
                ("tracebackA_ms", C.c_double), ("myersA_big_ms", C.c_double), ("myersA_big_blocks", C.c_uint64),
                ("myers_band_words", C.c_uint64),
                ("fused_ms", C.c_double), ("fused_launches", C.c_uint64), ("fused_blocks", C.c_uint64),
                ("rc_ms", C.c_double), ("rc_launches", C.c_uint64), ("rc_blocks", C.c_uint64), ("rc_words", C.c_uint64),
                ("rc_ck_ms", C.c_double),
                ("seed_bases", C.c_uint64), ("seed_lookups", C.c_uint64), ("seed_hits", C.c_uint64), ("seed_cands", C.c_uint64)]


class ShardTimings(C.Structure):
    """necat_shard_timings"""
    _fields_ = [("index_local_ms", C.c_double), ("index_exchange_ms", C.c_double), ("index_exchange_bytes", C.c_uint64),
                ("gather_ms", C.c_double), ("gather_bytes", C.c_uint64), ("reads_local", C.c_uint64),
                ("index_sharded", C.c_uint64), ("index_plan_replicate_ms", C.c_double), ("index_plan_shard_ms", C.c_double)]


class IndexPlan(C.Structure):
    """necat_index_plan_t"""
    _fields_ = [("shard", C.c_int32), ("_pad", C.c_int32), ("replicate_ms", C.c_double), ("shard_ms", C.c_double), ("exchange_ms", C.c_double),
                ("exchange_bytes", C.c_uint64)]


HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)

CANDIDATE_DTYPE = np.dtype([("qid", "<i4"), ("sid", "<i4"), ("qdir", "<i4"), ("sdir", "<i4"), ("score", "<i4"),
                            ("_pad", "<i4"), ("qbeg", "<u8"), ("qend", "<u8"), ("qsize", "<u8"),
                            ("sbeg", "<u8"), ("send", "<u8"), ("ssize", "<u8"), ("qoff", "<u8"), ("soff", "<u8")])
M4_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qoff", "<u8"), ("qend", "<u8"), ("qext", "<u8"),
                     ("qsize", "<u8"), ("sid", "<i4"), ("sdir", "<i4"), ("soff", "<u8"), ("send", "<u8"),
                     ("sext", "<u8"), ("ssize", "<u8"), ("ident_perc", "<f8"), ("vscore", "<i4"), ("_pad", "<i4")])
ALIGNMENT_DTYPE = np.dtype([("ok", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"),
                            ("align_size", "<i4"), ("ident_perc", "<f8")])
ASM_ANCHOR_DTYPE = np.dtype([("qid", "<i4"), ("sid", "<i4"), ("sdir", "<i4"), ("qoff", "<i4"), ("soff", "<i4")])      # necat_asm_anchor
CLIP_RANGE_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("size", "<i4"), ("how", "<i4")])     # necat_clip_range
TRIM_NONE, TRIM_COMPLETE, TRIM_CHIMERIC, TRIM_COVER, TRIM_HOST = 0, 1, 2, 3, 4                      # necat_clip_range.how
assert CANDIDATE_DTYPE.itemsize == 88 and M4_DTYPE.itemsize == 96 and ALIGNMENT_DTYPE.itemsize == 32 and CLIP_RANGE_DTYPE.itemsize == 16
CNS_OVERLAP_DTYPE = np.dtype([("cand", "<u8"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"),
                              ("align_size", "<i4"), ("ops_block", "<u4"), ("ops_off", "<u8"), ("ident_perc", "<f8"),
                              ("weight", "<f8")])
CNS_TEMPLATE_DTYPE = np.dtype([("examined", "<i4"), ("num_can", "<i4"), ("num_ovlps", "<i4"), ("_pad", "<i4"),
                               ("ident_cutoff", "<f8"), ("ovlp_begin", "<u8"), ("ovlp_end", "<u8"),
                               ("range_begin", "<u8"), ("range_end", "<u8")])
assert CNS_OVERLAP_DTYPE.itemsize == 56 and CNS_TEMPLATE_DTYPE.itemsize == 56
CNS_CONSENSUS_TEMPLATE_DTYPE = np.dtype([("corrected", "<i4"), ("on_host", "<i4"), ("seg_begin", "<u8"), ("seg_end", "<u8")])
CNS_SEGMENT_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("cns_from", "<i4"), ("cns_to", "<i4"), ("off", "<u8"), ("len", "<u4"), ("_pad", "<u4")])
assert CNS_CONSENSUS_TEMPLATE_DTYPE.itemsize == 24 and CNS_SEGMENT_DTYPE.itemsize == 32


class CnsOptions(C.Structure):
    """necat_cns_options (include/necat_hip.h) = the CnsOptions fields the extension loop reads"""
    _fields_ = [("min_align_size", C.c_int), ("min_cov", C.c_int), ("max_cov", C.c_int), ("error", C.c_double),
                ("mapping_ratio", C.c_double), ("use_fixed_ident_cutoff", C.c_int), ("rescue_long_indels", C.c_int)]


class CnsConsensusOptions(C.Structure):
    """necat_cns_consensus_options: -x, -l, -f of oc2cns, the path (0 = device with certified fallback, 1 = host only) and the host threads (0: NECAT_CNS_THREADS)"""
    _fields_ = [("min_cov", C.c_int), ("min_size", C.c_int), ("full_consensus", C.c_int), ("path", C.c_int), ("host_threads", C.c_int)]


class _CnsConsensus(C.Structure):
    _fields_ = [("n_templates", C.c_uint64), ("templates", C.c_void_p), ("n_segments", C.c_uint64), ("segments", C.c_void_p), ("n_bases", C.c_uint64),
                ("bases", C.c_void_p), ("n_device", C.c_uint64), ("n_fallback", C.c_uint64), ("device_ms", C.c_double), ("host_ms", C.c_double),
                ("tags_ms", C.c_double), ("sort_ms", C.c_double), ("backbone_ms", C.c_double), ("path_ms", C.c_double), ("n_chunks", C.c_uint32), ("_pad", C.c_uint32), ("n_uncertain", C.c_uint64)]


CTG_SEGMENT_DTYPE = np.dtype([("ctg_id", "<i4"), ("size", "<i4"), ("from", "<i8"), ("ovlp_begin", "<u8"), ("ovlp_end", "<u8")])      # necat_ctg_segment
CTG_OVERLAP_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"), ("align_size", "<i4"), ("_pad", "<i4"),
                              ("ops_off", "<u8")])      # necat_ctg_overlap
CTG_CONSENSUS_SEGMENT_DTYPE = np.dtype([("cns_off", "<u8"), ("cns_len", "<u8"), ("polished_off", "<u8"), ("polished_len", "<u8"), ("n_tags", "<u8"), ("n_nodes", "<u8"),
                                        ("n_links", "<u8"), ("n_chunks", "<u4"), ("_pad", "<u4")])
assert CTG_SEGMENT_DTYPE.itemsize == 32 and CTG_OVERLAP_DTYPE.itemsize == 40 and CTG_CONSENSUS_SEGMENT_DTYPE.itemsize == 64


class CtgConsensusOptions(C.Structure):
    """necat_ctg_consensus_options: the coverage below which a consensus base is lower case, the shortest upper-case run the splice takes, the path (0 = device,
    1 = host) and the host threads (0: NECAT_CNS_THREADS)"""
    _fields_ = [("min_cov", C.c_int), ("min_run", C.c_int), ("path", C.c_int), ("host_threads", C.c_int)]


class _CtgConsensus(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("segments", C.c_void_p), ("n_cns", C.c_uint64), ("cns", C.c_void_p), ("t_pos", C.c_void_p), ("n_polished", C.c_uint64),
                ("polished", C.c_void_p), ("n_fallback", C.c_uint64), ("n_chunks", C.c_uint32), ("_pad", C.c_uint32), ("device_ms", C.c_double), ("tags_ms", C.c_double),
                ("sort_ms", C.c_double), ("links_ms", C.c_double), ("plan_ms", C.c_double), ("score_ms", C.c_double), ("host_ms", C.c_double)]


CTG_SEED_JOB_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4")])      # necat_ctg_seed_job
CTG_SEED_MEM_DTYPE = np.dtype([("qoff", "<i4"), ("soff", "<i4"), ("size", "<i4")])      # necat_ctg_seed_mem
CTG_SEED_RESULT_DTYPE = np.dtype([("found", "<i4"), ("qbeg", "<i4"), ("qend", "<i4"), ("sbeg", "<i4"), ("send", "<i4"), ("qoff", "<i4"), ("soff", "<i4"), ("score", "<i4"),
                                  ("n_matches", "<u4"), ("n_mems", "<u4"), ("chain_len", "<i4"), ("how", "<i4"), ("mems_off", "<u8")])      # necat_ctg_seed_result
assert CTG_SEED_JOB_DTYPE.itemsize == 8 and CTG_SEED_MEM_DTYPE.itemsize == 12 and CTG_SEED_RESULT_DTYPE.itemsize == 56


class CtgSeedOptions(C.Structure):
    """necat_ctg_seed_options: the path (0 = device, 1 = host), the host threads (0: NECAT_CNS_THREADS), and whether the result holds every job's sorted matches"""
    _fields_ = [("path", C.c_int), ("host_threads", C.c_int), ("keep_mems", C.c_int), ("_pad", C.c_int)]


class _CtgSeed(C.Structure):
    _fields_ = [("n_jobs", C.c_uint64), ("jobs", C.c_void_p), ("n_mems", C.c_uint64), ("mems", C.c_void_p), ("n_fallback", C.c_uint64), ("n_lds", C.c_uint64),
                ("n_scratch", C.c_uint64), ("max_matches", C.c_uint32), ("max_mems", C.c_uint32), ("index_ms", C.c_double), ("match_ms", C.c_double),
                ("chain_ms", C.c_double), ("device_ms", C.c_double), ("host_ms", C.c_double)]


CTG_EXTEND_JOB_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("soff", "<i8"), ("send", "<i8")])      # necat_ctg_extend_job
CTG_EXTEND_RESULT_DTYPE = np.dtype([("state", "<i4"), ("decided", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"), ("align_size", "<i4"), ("_pad", "<i4"),
                                    ("ident_perc", "<f8"), ("overlap", "<i8")])      # necat_ctg_extend_result
assert CTG_EXTEND_JOB_DTYPE.itemsize == 24 and CTG_EXTEND_RESULT_DTYPE.itemsize == 48
CTG_EXT_CAPPED, CTG_EXT_NO_SEED, CTG_EXT_NO_ALIGNMENT, CTG_EXT_REJECTED, CTG_EXT_ACCEPTED = range(5)      # necat_ctg_extend_result.state
CTG_EXT_BY_NONE, CTG_EXT_BY_BLOCKS, CTG_EXT_BY_PAIR, CTG_EXT_BY_BLOCKS_KEPT = range(4)                     # .. decided


class CtgExtendOptions(C.Structure):
    """necat_ctg_extend_options: the loop with its coverage cap (1) or every job (0), the rescue pair on the device (0) or on the host threads (1), the host
    threads (0: NECAT_CNS_THREADS)"""
    _fields_ = [("cap", C.c_int), ("rescue_path", C.c_int), ("host_threads", C.c_int), ("_pad", C.c_int)]


class _CtgExtend(C.Structure):
    _COUNTERS = ("n_seeded", "n_aligned", "n_used", "n_pair_tried", "n_pair_accepted", "n_dalign_device", "n_dalign_host", "n_dalign_over_cap", "n_dalign_selfcheck",
                 "n_nw_jobs", "n_nw_device", "n_nw_host", "cols_bytes_downloaded", "cols_bytes_used")
    _TIMES = ("seed_ms", "align_ms", "rescue_ms", "replay_ms")
    _fields_ = [("n_jobs", C.c_uint64), ("jobs", C.c_void_p), ("n_segments", C.c_uint64), ("segments", C.c_void_p), ("n_overlaps", C.c_uint64), ("overlaps", C.c_void_p),
                ("n_ops", C.c_uint64), ("ops", C.c_void_p)] + [(f, C.c_uint64) for f in _COUNTERS] + [(f, C.c_double) for f in _TIMES]


class _CnsResult(C.Structure):
    _fields_ = [("n_templates", C.c_uint64), ("templates", C.c_void_p), ("n_overlaps", C.c_uint64), ("overlaps", C.c_void_p),
                ("n_ranges", C.c_uint64), ("ranges", C.c_void_p), ("n_ops_blocks", C.c_uint32), ("ops", C.POINTER(C.c_void_p)),
                ("n_aligned", C.c_uint64), ("n_used", C.c_uint64), ("n_rounds", C.c_uint32), ("device_ms", C.c_double),
                ("host_ms", C.c_double), ("n_rescue_tried", C.c_uint64), ("n_rescued", C.c_uint64), ("rescue_ms", C.c_double),
                ("rescue_dalign_ms", C.c_double), ("rescue_nw_ms", C.c_double), ("n_rescue_nw", C.c_uint64), ("n_rescue_nw_device", C.c_uint64),
                ("n_rescue_nw_host", C.c_uint64), ("n_rescue_dalign_device", C.c_uint64), ("n_rescue_dalign_host", C.c_uint64)]


class NwStats(C.Structure):
    """necat_nw_stats"""
    _fields_ = [("n_device", C.c_uint64), ("n_host", C.c_uint64), ("n_selfcheck", C.c_uint64), ("n_levels", C.c_uint32), ("n_leaf_chunks", C.c_uint32),
                ("n_passes", C.c_uint64), ("n_splits", C.c_uint64), ("n_leaves", C.c_uint64), ("device_ms", C.c_double), ("cols_ms", C.c_double),
                ("split_ms", C.c_double), ("leaf_ms", C.c_double), ("finish_ms", C.c_double), ("host_ms", C.c_double)]


NW_JOB_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qfrom", "<i4"), ("qto", "<i4"), ("sid", "<i4"), ("sfrom", "<i4"), ("sto", "<i4"), ("tolerance", "<i4")])
NW_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("how", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("toff", "<i4"), ("tend", "<i4"), ("align_size", "<i4"), ("dist", "<i4"),
                            ("ident_perc", "<f8")])

class DalignStats(C.Structure):
    """necat_dalign_stats"""
    _fields_ = [("n_device", C.c_uint64), ("n_host", C.c_uint64), ("n_selfcheck", C.c_uint64), ("n_over_cap", C.c_uint64), ("n_steps", C.c_uint64),
                ("max_diags", C.c_uint32), ("device_ms", C.c_double), ("host_ms", C.c_double)]


DALIGN_JOB_DTYPE = np.dtype([("qid", "<i4"), ("qdir", "<i4"), ("qstart", "<i4"), ("sid", "<i4"), ("sstart", "<i4")])
DALIGN_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("how", "<i4"), ("qoff", "<i4"), ("qend", "<i4"), ("soff", "<i4"), ("send", "<i4"), ("diffs", "<i4"), ("_pad", "<i4"),
                                ("ident_perc", "<f8")])

ASM_PLAN_DTYPE = np.dtype([("qid", "<i4"), ("sid", "<i4"), ("sdir", "<i4"), ("qoff", "<i4"), ("soff", "<i4"), ("score", "<i4"), ("ssize", "<i4")])      # necat_asm_plan


class AsmMapStats(C.Structure):
    """necat_asm_map_stats ([0] the left end, [1] the right end)"""
    _fields_ = [("n_anchors", C.c_uint64), ("n_ok", C.c_uint64), ("n_low_ident", C.c_uint64), ("n_tried", C.c_uint64 * 2), ("n_extended", C.c_uint64 * 2),
                ("n_hang0", C.c_uint64 * 2), ("n_hang_long", C.c_uint64 * 2), ("n_no_run", C.c_uint64 * 2), ("n_jobs", C.c_uint64), ("n_tier1", C.c_uint64),
                ("n_tier2", C.c_uint64), ("n_host", C.c_uint64), ("n_steps", C.c_uint64), ("diag_hist", C.c_uint64 * 12), ("max_diags", C.c_uint32), ("_pad", C.c_uint32),
                ("device_ms", C.c_double), ("host_ms", C.c_double)]


class RmStats(C.Structure):
    """necat_rm_stats: what the context's last necat_map_reference did with the rescue pair"""
    _fields_ = [("n_candidates", C.c_uint64), ("n_need", C.c_uint64), ("n_tried", C.c_uint64), ("n_rescued", C.c_uint64), ("n_dalign_device", C.c_uint64),
                ("n_dalign_host", C.c_uint64), ("n_dalign_over_cap", C.c_uint64), ("n_dalign_selfcheck", C.c_uint64), ("n_nw_jobs", C.c_uint64),
                ("n_nw_device", C.c_uint64), ("n_nw_host", C.c_uint64), ("max_diags", C.c_uint32), ("words_fetched", C.c_uint32), ("dalign_ms", C.c_double),
                ("nw_ms", C.c_double), ("replay_ms", C.c_double)]


class ItemOrderStats(C.Structure):
    """necat_item_order_stats: lane-steps the checkpoint passes of the context's last extension call issued / needed (list A's ragged waves, list B's waves)"""
    _fields_ = [("a_issued", C.c_uint64), ("a_needed", C.c_uint64), ("a_blocks", C.c_uint64), ("b_issued", C.c_uint64), ("b_needed", C.c_uint64), ("b_blocks", C.c_uint64)]


ABI_VERSION = 16         # include/necat_hip.h: NECAT_ABI_VERSION

EXPORTED_SYMBOLS = [
    "necat_default_options", "necat_ctx_create", "necat_ctx_destroy", "necat_ctx_trim", "necat_last_error", "necat_device_name",
    "necat_volume_upload", "necat_volume_pack", "necat_volume_gather", "necat_volume_gather_stats", "necat_volume_download", "necat_volume_free", "necat_index_build", "necat_index_size", "necat_index_download",
    "necat_index_free", "necat_index_sparse_size", "necat_index_download_sparse", "necat_find_candidates", "necat_extend", "necat_map_pair", "necat_map_reference", "necat_onc_align_batch", "necat_asm_align_batch", "necat_asm_plan_batch", "necat_asm_map_batch",
    "necat_nw_path_batch", "necat_local_align_batch",
    "necat_gapped_strings", "necat_cns_default_options", "necat_cns_load_partition", "necat_cns_extension_batch",
    "necat_cns_result_free", "necat_cns_consensus_default_options", "necat_cns_consensus_batch", "necat_cns_consensus_free",
    "necat_ctg_consensus_default_options", "necat_ctg_consensus_batch", "necat_ctg_consensus_free",
    "necat_ctg_seed_default_options", "necat_ctg_seed_batch", "necat_ctg_seed_free",
    "necat_ctg_extend_default_options", "necat_ctg_extend_batch", "necat_ctg_extend_free",
    "necat_edlib_align_batch", "necat_get_timings", "necat_get_timings_sized", "necat_get_rm_stats_sized", "necat_get_item_order_stats", "necat_get_shard_timings_sized", "necat_abi_version", "necat_knob_get", "necat_free", "necat_pcan_partition", "necat_trim_partition", "necat_trim_ranges",
    "necat_comm_create", "necat_comm_destroy", "necat_comm_transport", "necat_get_shard_timings", "necat_comm_selftest_rccl", "necat_comm_selftest_rccl2",
    "necat_index_build_sharded", "necat_index_plan", "necat_find_candidates_sharded", "necat_map_pair_sharded",
    "necat_pair_schedule", "necat_pair_chunk_reads", "necat_find_candidates_part", "necat_map_pair_part",
]

_lib = None
_lib_xcheck = None


# the defaults needs_xcheck has to know: restated from the table in necat_amd/csrc/knobs.h, the one declaration of every knob (tests/test_knobs.py compares the two)
XCHECK_DEFAULTS = {"NECAT_RCWALK": 512, "NECAT_TAIL_FUSED": 512, "NECAT_RC_CARRY": 1, "NECAT_RC_RAGGED": 1, "NECAT_RC_WW": 1, "NECAT_FAST": 1, "NECAT_COOP_FILTER": 1,
                   "NECAT_RC_LISTB": 1, "NECAT_RC_MAXDIST": 1 << 20, "NECAT_SEED_WAVE": 1, "NECAT_ASM_LANE": 0, "NECAT_ASM_RC": 1}


def needs_xcheck(env=None) -> bool:
    """True when the kernel-path knobs in `env` (default: os.environ) select a path of the CROSS-CHECK build - a kernel family the default paths replaced, kept as an
    independent implementation for the parity tests (necat_hip.hip, NECAT_BUILD_CROSSCHECK; libnecat_hip_xcheck.so).  The product library refuses such a knob with
    NECAT_ERR_ARG (never another path), so a wrong answer here fails a test loudly."""
    env = os.environ if env is None else env
    num = lambda k: int(env.get(k, XCHECK_DEFAULTS[k]))
    rcwalk, tail = num("NECAT_RCWALK"), num("NECAT_TAIL_FUSED")
    all_fused = tail >= 1 << 26                      # every list through k_tail_fused
    if not all_fused and (rcwalk == 0 or rcwalk > max(tail, 15)):      # list sizes no default path covers (a round's bound is >= 16)
        return True
    if num("NECAT_RC_CARRY") == 0 or num("NECAT_RC_RAGGED") == 0 or num("NECAT_RC_WW") == 0 or num("NECAT_FAST") != 1 or num("NECAT_COOP_FILTER") == 0:
        return True
    if (num("NECAT_RC_LISTB") == 0 and not all_fused) or "NECAT_COOP_THRESHOLD" in env or num("NECAT_RC_MAXDIST") < 300:
        return True
    return num("NECAT_SEED_WAVE") == 0 or num("NECAT_ASM_LANE") != 0 or num("NECAT_ASM_RC") == 0


def load_library(path: Optional[str] = None, xcheck: bool = False) -> C.CDLL:
    """dlopen the in-tree library (xcheck: the tests' cross-check build of the same sources); never falls back to anything else."""
    global _lib, _lib_xcheck
    if xcheck:
        if _lib_xcheck is not None:
            return _lib_xcheck
    elif _lib is not None:
        return _lib
    if xcheck:
        p = path or _build.LIB_XCHECK
        if not os.path.exists(p):
            raise RuntimeError("libnecat_hip_xcheck.so is not built (%s): run `python -m necat_amd.build` (build_xcheck)" % p)
    else:
        p = path or os.environ.get("NECAT_HIP_LIB") or _build.LIB       # NECAT_HIP_LIB: an instrumented build of the same sources (tools/seed_prof.sh)
        if not os.path.exists(p):
            raise RuntimeError("libnecat_hip.so is not built (%s): run `python -m necat_amd.build`" % p)
    # (the host program's job since round 6 - the library no longer sets it when it is loaded; read by the HIP runtime at its first call)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(p)
    lib.necat_abi_version.restype = C.c_int
    if lib.necat_abi_version() != ABI_VERSION:
        raise RuntimeError("%s has ABI version %d, this binding was written for %d (include/necat_hip.h: NECAT_ABI_VERSION)" % (p, lib.necat_abi_version(), ABI_VERSION))
    vp, u64p, i32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.necat_get_timings_sized.argtypes = [vp, vp, C.c_size_t]
    lib.necat_get_rm_stats_sized.argtypes = [vp, vp, C.c_size_t]
    lib.necat_get_item_order_stats.argtypes = [vp, C.POINTER(ItemOrderStats)]
    lib.necat_knob_get.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.necat_get_shard_timings_sized.argtypes = [vp, vp, C.c_size_t]
    lib.necat_default_options.argtypes = [C.POINTER(MapOptions)]
    lib.necat_default_options.restype = None
    lib.necat_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.necat_ctx_destroy.argtypes = [vp]
    lib.necat_ctx_destroy.restype = None
    lib.necat_ctx_trim.argtypes = [vp]
    lib.necat_ctx_trim.restype = None
    lib.necat_pcan_partition.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
    lib.necat_trim_partition.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_double, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    lib.necat_trim_ranges.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_uint64)]
    lib.necat_comm_selftest_rccl.argtypes = [vp, C.c_uint64]
    lib.necat_comm_selftest_rccl2.argtypes = [vp, C.c_uint64]
    lib.necat_last_error.argtypes = [vp]
    lib.necat_last_error.restype = C.c_char_p
    lib.necat_device_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.necat_volume_upload.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(vp)]
    lib.necat_volume_free.argtypes = [vp, vp]
    lib.necat_volume_pack.argtypes = [vp, C.c_char_p, C.c_uint64, vp, vp, C.c_uint64, vp, C.POINTER(vp)]
    lib.necat_volume_free.restype = None
    lib.necat_volume_gather.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(vp)]
    lib.necat_volume_download.argtypes = [vp, vp, vp]
    lib.necat_volume_gather_stats.argtypes = [vp, C.POINTER(C.c_double), u64p]
    lib.necat_index_build.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.necat_index_size.argtypes = [vp, u64p, u64p]
    lib.necat_index_download.argtypes = [vp, vp, vp, vp]
    lib.necat_index_free.argtypes = [vp, vp]
    lib.necat_index_sparse_size.argtypes = [vp, u64p, u64p]
    lib.necat_index_download_sparse.argtypes = [vp, vp, vp, vp, vp]
    lib.necat_index_free.restype = None
    lib.necat_find_candidates.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions),
                                          C.POINTER(vp), u64p]
    lib.necat_extend.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.POINTER(MapOptions), C.c_int,
                                 C.POINTER(vp), u64p]
    lib.necat_map_pair.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions), C.c_int,
                                   C.POINTER(vp), u64p, u64p]
    lib.necat_map_reference.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(MapOptions), C.POINTER(vp), u64p, u64p, u64p]
    lib.necat_onc_align_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.POINTER(MapOptions), C.c_int,
                                          C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.necat_asm_align_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.c_double, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.necat_asm_plan_batch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.necat_asm_map_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.c_double, C.c_int, C.c_double, C.POINTER(vp), C.POINTER(vp), C.POINTER(AsmMapStats)]
    lib.necat_nw_path_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.c_double, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(NwStats)]
    lib.necat_local_align_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint64, C.c_double, C.c_int, C.POINTER(vp), C.POINTER(DalignStats)]
    lib.necat_gapped_strings.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, vp]
    lib.necat_cns_default_options.argtypes = [C.POINTER(CnsOptions)]
    lib.necat_cns_default_options.restype = None
    lib.necat_cns_load_partition.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u64p]
    lib.necat_cns_extension_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(CnsOptions),
                                              C.POINTER(C.POINTER(_CnsResult))]
    lib.necat_cns_result_free.argtypes = [C.POINTER(_CnsResult)]
    lib.necat_cns_result_free.restype = None
    lib.necat_cns_consensus_default_options.argtypes = [C.POINTER(CnsConsensusOptions)]
    lib.necat_cns_consensus_default_options.restype = None
    lib.necat_cns_consensus_batch.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(_CnsResult), C.POINTER(CnsConsensusOptions), C.POINTER(C.POINTER(_CnsConsensus))]
    lib.necat_cns_consensus_free.argtypes = [C.POINTER(_CnsConsensus)]
    lib.necat_cns_consensus_free.restype = None
    lib.necat_ctg_consensus_default_options.argtypes = [C.POINTER(CtgConsensusOptions)]
    lib.necat_ctg_consensus_default_options.restype = None
    lib.necat_ctg_consensus_batch.argtypes = [vp, vp, C.c_int, vp, vp, C.c_uint64, vp, vp, C.POINTER(CtgConsensusOptions), C.POINTER(C.POINTER(_CtgConsensus))]
    lib.necat_ctg_consensus_free.argtypes = [C.POINTER(_CtgConsensus)]
    lib.necat_ctg_consensus_free.restype = None
    lib.necat_ctg_seed_default_options.argtypes = [C.POINTER(CtgSeedOptions)]
    lib.necat_ctg_seed_default_options.restype = None
    lib.necat_ctg_seed_batch.argtypes = [vp, vp, C.c_int, vp, vp, C.c_uint64, vp, C.POINTER(CtgSeedOptions), C.POINTER(C.POINTER(_CtgSeed))]
    lib.necat_ctg_seed_free.argtypes = [C.POINTER(_CtgSeed)]
    lib.necat_ctg_seed_free.restype = None
    lib.necat_ctg_extend_default_options.argtypes = [C.POINTER(CtgExtendOptions)]
    lib.necat_ctg_extend_default_options.restype = None
    lib.necat_ctg_extend_batch.argtypes = [vp, vp, C.c_int, vp, vp, C.c_uint64, vp, C.POINTER(_CtgSeed), C.POINTER(CtgExtendOptions), C.POINTER(C.POINTER(_CtgExtend))]
    lib.necat_ctg_extend_free.argtypes = [C.POINTER(_CtgExtend)]
    lib.necat_ctg_extend_free.restype = None
    lib.necat_edlib_align_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, C.c_double,
                                            vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.necat_get_timings.argtypes = [vp, C.POINTER(Timings)]
    lib.necat_comm_create.argtypes = [vp, C.c_int, C.c_int, HOST_ALLGATHER_FN, vp, C.c_char_p, C.POINTER(vp)]
    lib.necat_comm_destroy.argtypes = [vp]
    lib.necat_comm_destroy.restype = None
    lib.necat_comm_transport.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.necat_get_shard_timings.argtypes = [vp, C.POINTER(ShardTimings)]
    lib.necat_index_build_sharded.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.necat_index_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_double, C.POINTER(IndexPlan)]
    lib.necat_find_candidates_sharded.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions), C.c_int, C.c_int,
                                                  C.POINTER(vp), u64p, u64p]
    lib.necat_map_pair_sharded.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions), C.c_int, C.c_int, C.c_int,
                                           C.POINTER(vp), u64p, u64p, u64p]
    lib.necat_pair_chunk_reads.argtypes = [C.c_uint64, C.c_int]
    lib.necat_pair_schedule.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.necat_find_candidates_part.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions), C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(vp), u64p]
    lib.necat_map_pair_part.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MapOptions), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(vp), u64p, u64p]
    lib.necat_free.argtypes = [vp]
    lib.necat_free.restype = None
    for name in EXPORTED_SYMBOLS:
        getattr(lib, name)
    if xcheck:
        _lib_xcheck = lib
    else:
        _lib = lib
    return lib


def index_plan(nbases: int, k: int, nranks: int, link_gbs: float = 0.0) -> IndexPlan:
    """necat_index_plan: what a `nranks`-rank build of a volume's index costs either way (no device needed)"""
    p = IndexPlan()
    rc = load_library().necat_index_plan(nbases, k, nranks, link_gbs, C.byref(p))
    if rc:
        raise NecatError("necat_index_plan: %d" % rc)
    return p


def default_options(**kw) -> MapOptions:
    o = MapOptions()
    load_library().necat_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


class NecatError(RuntimeError):
    pass


class Context:
    """necat_ctx + RAII wrappers of volumes and indexes."""

    def __init__(self, device: int = 0, xcheck: Optional[bool] = None):
        # xcheck None: the cross-check build exactly when the environment's knobs select one of its paths (needs_xcheck) - the product library otherwise
        self.xcheck = needs_xcheck() if xcheck is None else bool(xcheck)
        self.device = device
        self._xc, self._xc_key = None, None
        self.lib = load_library(xcheck=self.xcheck)
        h = C.c_void_p()
        rc = self.lib.necat_ctx_create(device, C.byref(h))
        if rc != 0:
            raise NecatError("necat_ctx_create(device=%d) failed with %d: no usable gfx950 GPU "
                             "(this library has no CPU fallback)" % (device, rc))
        self.h = h

    def close(self):
        if getattr(self, "_xc", None) is not None:
            self._xc.close()
            self._xc = None
        if getattr(self, "h", None):
            self.lib.necat_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise NecatError("%s failed (%d): %s" % (what, rc, self.lib.necat_last_error(self.h).decode()))

    def device_name(self) -> str:
        b = C.create_string_buffer(256)
        self.lib.necat_device_name(self.h, b, 256)
        return b.value.decode()

    def knob(self, name: str) -> str:
        """the value this context read for a knob of knobs.h's table when it was created, as text ("" = a set-at-all knob that was not set)"""
        b = C.create_string_buffer(4096)
        self._check(self.lib.necat_knob_get(self.h, name.encode(), b, 4096), "necat_knob_get(%s)" % name)
        return b.value.decode()

    def timings(self) -> Timings:
        t = Timings()
        self.lib.necat_get_timings(self.h, C.byref(t))
        return t

    # ---- one volume on several GPUs (include/necat_hip.h, "one reference volume on several GPUs")
    def shard_timings(self) -> ShardTimings:
        t = ShardTimings()
        self.lib.necat_get_shard_timings(self.h, C.byref(t))
        return t

    def comm(self, rank: int, nranks: int, allgather, transport: str = "auto") -> "Comm":
        """allgather(send: bytes) -> list of nranks bytes objects (rank order): the host-side exchange of the job's launcher
        (necat_amd.dist.torch_allgather for torch.distributed)"""
        return Comm(self, rank, nranks, allgather, transport)

    def build_index_sharded(self, comm: "Comm", ref: "Volume", k: int, max_occ: int) -> "Index":
        h = C.c_void_p()
        self._check(self.lib.necat_index_build_sharded(self.h, comm.h, ref.h, k, max_occ, C.byref(h)), "necat_index_build_sharded")
        return Index(self, h, k)

    def find_candidates_sharded(self, comm: "Comm", ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int,
                                opt: MapOptions, pairwise: bool = True, chunk_reads: int = 64, root: int = 0):
        """(records - all ranks' on the root, this rank's elsewhere -, this rank's own count)"""
        p = C.c_void_p()
        n, nl = C.c_uint64(), C.c_uint64()
        self._check(self.lib.necat_find_candidates_sharded(self.h, comm.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, 1 if pairwise else 0,
                                                           C.byref(opt), chunk_reads, root, C.byref(p), C.byref(n), C.byref(nl)),
                    "necat_find_candidates_sharded")
        return self._take(p, n.value, CANDIDATE_DTYPE), int(nl.value)

    def map_pair_sharded(self, comm: "Comm", ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, opt: MapOptions,
                         pairwise: bool = True, tail_match_len: int = 1, chunk_reads: int = 64, root: int = 0):
        """(M4 records - all ranks' on the root -, this rank's own record count, this rank's candidates)"""
        p = C.c_void_p()
        n, nl, nc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.necat_map_pair_sharded(self.h, comm.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, 1 if pairwise else 0,
                                                    C.byref(opt), tail_match_len, chunk_reads, root, C.byref(p), C.byref(n), C.byref(nl), C.byref(nc)),
                    "necat_map_pair_sharded")
        return self._take(p, n.value, M4_DTYPE), int(nl.value), int(nc.value)

    # ---- volumes
    def upload_volume(self, pac: np.ndarray, nbases: int, offsets: np.ndarray, sizes: np.ndarray) -> "Volume":
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        h = C.c_void_p()
        self._check(self.lib.necat_volume_upload(self.h, pac.ctypes.data, nbases, off.ctypes.data, sz.ctypes.data,
                                                 off.shape[0], C.byref(h)), "necat_volume_upload")
        return Volume(self, h, nbases, off.astype(np.int64), sz.astype(np.int64))

    def gather_volume(self, vols, vol_start_ids, ids) -> "Volume":
        """necat_volume_gather: the sequences `ids` (global, strictly ascending) of the resident volumes `vols` - vols[k] holds the ids vol_start_ids[k] .. + its
        nseq - as one compact volume whose local id i is ids[i]; names follow where every source volume has them"""
        vols = list(vols)
        start = np.ascontiguousarray(vol_start_ids, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if start.shape[0] != len(vols):
            raise ValueError("one first id per volume")
        hs = (C.c_void_p * max(1, len(vols)))(*[v.h.value for v in vols])
        h = C.c_void_p()
        self._check(self.lib.necat_volume_gather(self.h, hs, start.ctypes.data, len(vols), ids.ctypes.data, ids.shape[0], C.byref(h)), "necat_volume_gather")
        order = np.argsort(start, kind="stable")
        which = np.searchsorted(start[order], ids, side="right") - 1
        sizes = np.array([vols[order[k]].sizes[i - start[order[k]]] for k, i in zip(which, ids)], dtype=np.int64)
        off = np.zeros(sizes.shape[0], dtype=np.int64)
        if sizes.shape[0]:
            off[1:] = np.cumsum(sizes)[:-1]
        v = Volume(self, h, int(sizes.sum()), off, sizes)
        if all(len(s.names) == s.nseq for s in vols):
            v.names = [vols[order[k]].names[i - start[order[k]]] for k, i in zip(which, ids)]
        return v

    def gather_stats(self):
        """(kernel ms from HIP events, bytes read and written) of this context's last gather_volume"""
        ms, nb = C.c_double(), C.c_uint64()
        self._check(self.lib.necat_volume_gather_stats(self.h, C.byref(ms), C.byref(nb)), "necat_volume_gather_stats")
        return ms.value, int(nb.value)

    def load_volume(self, path: str) -> "Volume":
        pac, off, sz, names = read_volume(path)
        v = self.upload_volume(pac, int(sz.sum()), off, sz)
        v.names = names
        return v

    def load_merged_volumes(self, wrk_dir: str) -> "Volume":
        """all volumes of a work directory as ONE read set with global ids (merge_volumes, common/makedb_aux.c:137-153) -
        what the consensus stage works on; .codes keeps the byte-coded bases for the callers' gapped strings"""
        from .synth import pack_2bit, unpack_2bit
        _, _, vols = load_volumes_info(wrk_dir)
        codes, sizes, names = [], [], []
        for path, _, _ in vols:
            pac, off, sz, nm = read_volume(path)
            codes.append(unpack_2bit(pac, int(sz.sum())))
            sizes.append(sz)
            names += nm
        codes = np.concatenate(codes) if codes else np.zeros(0, np.uint8)
        sizes = np.concatenate(sizes).astype(np.int64) if sizes else np.zeros(0, np.int64)
        off = np.zeros(sizes.shape[0], dtype=np.int64)
        if sizes.shape[0]:
            off[1:] = np.cumsum(sizes)[:-1]
        v = self.upload_volume(pack_2bit(codes), int(sizes.sum()), off, sizes)
        v.names, v.codes = names, codes
        return v

    def build_index(self, ref: "Volume", k: int, max_occ: int) -> "Index":
        h = C.c_void_p()
        self._check(self.lib.necat_index_build(self.h, ref.h, k, max_occ, C.byref(h)), "necat_index_build")
        return Index(self, h, k)

    def find_candidates(self, ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int,
                        opt: MapOptions, pairwise: bool = True) -> np.ndarray:
        p = C.c_void_p()
        n = C.c_uint64()
        self._check(self.lib.necat_find_candidates(self.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id,
                                                   1 if pairwise else 0, C.byref(opt), C.byref(p), C.byref(n)),
                    "necat_find_candidates")
        return self._take(p, n.value, CANDIDATE_DTYPE)

    def extend(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, cands: np.ndarray,
               opt: MapOptions, tail_match_len: int = 1) -> np.ndarray:
        cands = np.ascontiguousarray(cands, dtype=CANDIDATE_DTYPE)
        p = C.c_void_p()
        n = C.c_uint64()
        self._check(self.lib.necat_extend(self.h, ref.h, reads.h, read_start_id, ref_start_id, cands.ctypes.data,
                                          cands.shape[0], C.byref(opt), tail_match_len, C.byref(p), C.byref(n)),
                    "necat_extend")
        return self._take(p, n.value, M4_DTYPE)

    def map_pair(self, ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, opt: MapOptions,
                 pairwise: bool = True, tail_match_len: int = 1):
        """find_candidates + extend with the candidates kept on the device: (M4 records, number of candidates)."""
        p = C.c_void_p()
        n, nc = C.c_uint64(), C.c_uint64()
        self._check(self.lib.necat_map_pair(self.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, 1 if pairwise else 0,
                                            C.byref(opt), tail_match_len, C.byref(p), C.byref(n), C.byref(nc)), "necat_map_pair")
        return self._take(p, n.value, M4_DTYPE), int(nc.value)

    def find_candidates_part(self, ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, opt: MapOptions,
                             chunk_reads: int, slot_lo: int, slot_hi: int, slots: int, pairwise: bool = True) -> np.ndarray:
        """necat_find_candidates for the query chunks c with slot_lo <= c % slots < slot_hi (one unit of the pair scheduler)"""
        p = C.c_void_p()
        n = C.c_uint64()
        self._check(self.lib.necat_find_candidates_part(self.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, 1 if pairwise else 0, C.byref(opt),
                                                        chunk_reads, slot_lo, slot_hi, slots, C.byref(p), C.byref(n)), "necat_find_candidates_part")
        return self._take(p, n.value, CANDIDATE_DTYPE)

    def map_pair_part(self, ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, opt: MapOptions,
                      chunk_reads: int, slot_lo: int, slot_hi: int, slots: int, pairwise: bool = True, tail_match_len: int = 1):
        """necat_map_pair for one unit of the pair scheduler: (M4 records, number of candidates)"""
        p = C.c_void_p()
        n, nc = C.c_uint64(), C.c_uint64()
        self._check(self.lib.necat_map_pair_part(self.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, 1 if pairwise else 0, C.byref(opt), tail_match_len,
                                                 chunk_reads, slot_lo, slot_hi, slots, C.byref(p), C.byref(n), C.byref(nc)), "necat_map_pair_part")
        return self._take(p, n.value, M4_DTYPE), int(nc.value)

    def map_reference(self, ix: "Index", ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, opt: MapOptions):
        """rm_search_one_volume for every read of `reads`: (M4 records, number of candidates, records from the rescue pair)."""
        p = C.c_void_p()
        n, nc, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.necat_map_reference(self.h, ix.h, ref.h, reads.h, read_start_id, ref_start_id, C.byref(opt), C.byref(p), C.byref(n),
                                                 C.byref(nc), C.byref(nr)), "necat_map_reference")
        return self._take(p, n.value, M4_DTYPE), int(nc.value), int(nr.value)

    def rm_stats(self) -> RmStats:
        """what this context's last map_reference did with the rescue pair (necat_get_rm_stats_sized)"""
        t = RmStats()
        self._check(self.lib.necat_get_rm_stats_sized(self.h, C.byref(t), C.sizeof(t)), "necat_get_rm_stats_sized")
        return t

    def item_order_stats(self) -> ItemOrderStats:
        """what the checkpoint passes of this context's last extension call issued against what their blocks needed (necat_get_item_order_stats)"""
        t = ItemOrderStats()
        self._check(self.lib.necat_get_item_order_stats(self.h, C.byref(t)), "necat_get_item_order_stats")
        return t

    def onc_align_batch(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, cands: np.ndarray,
                        opt: MapOptions, tail_match_len: int = 4):
        """onc_align with the alignment itself for every candidate (the consensus stage's call):
        (alignments[ALIGNMENT_DTYPE], ops[uint8: 2 bits per column], ops_off[uint64, n + 1: byte offsets])."""
        cands = np.ascontiguousarray(cands, dtype=CANDIDATE_DTYPE)
        n = cands.shape[0]
        a, o, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.necat_onc_align_batch(self.h, ref.h, reads.h, read_start_id, ref_start_id, cands.ctypes.data, n,
                                                   C.byref(opt), tail_match_len, C.byref(a), C.byref(o), C.byref(f)),
                    "necat_onc_align_batch")
        off = self._take(f, n + 1, np.dtype("<u8"))
        return self._take(a, n, ALIGNMENT_DTYPE), self._take(o, int(off[-1]), np.dtype("u1")), off

    def nw_path_batch(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, jobs: np.ndarray, error: float = 0.5,
                      min_align_size: int = 400, match_size: int = 4):
        """edlib_go (the rescue pair's global alignment with its path) for every job (NW_JOB_DTYPE):
        (results[NW_RESULT_DTYPE], ops[uint8: 2 bits per column], ops_off[uint64, n + 1: byte offsets], NwStats)."""
        jobs = np.ascontiguousarray(jobs, dtype=NW_JOB_DTYPE)
        n = jobs.shape[0]
        a, o, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = NwStats()
        self._check(self.lib.necat_nw_path_batch(self.h, ref.h, reads.h, read_start_id, ref_start_id, jobs.ctypes.data, n, error, min_align_size, match_size,
                                                 C.byref(a), C.byref(o), C.byref(f), C.byref(st)), "necat_nw_path_batch")
        off = self._take(f, n + 1, np.dtype("<u8"))
        return self._take(a, n, NW_RESULT_DTYPE), self._take(o, int(off[-1]), np.dtype("u1")), off, st

    def local_align_batch(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, jobs: np.ndarray, error: float = 0.5, min_align_size: int = 400):
        """ocda_go (the rescue pair's local alignment around the anchor) for every job (DALIGN_JOB_DTYPE): (results[DALIGN_RESULT_DTYPE], DalignStats)."""
        jobs = np.ascontiguousarray(jobs, dtype=DALIGN_JOB_DTYPE)
        n = jobs.shape[0]
        a = C.c_void_p()
        st = DalignStats()
        self._check(self.lib.necat_local_align_batch(self.h, ref.h, reads.h, read_start_id, ref_start_id, jobs.ctypes.data, n, error, min_align_size, C.byref(a), C.byref(st)),
                    "necat_local_align_batch")
        return self._take(a, n, DALIGN_RESULT_DTYPE), st

    def asm_align_batch(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, anchors: np.ndarray, error: float = 0.5,
                        min_align_size: int = 400):
        """blockwise_edlib_align (oc2asmpm's block aligner: 2048-bp blocks, tail match length 8) for every anchor; returns as onc_align_batch"""
        anchors = np.ascontiguousarray(anchors, dtype=ASM_ANCHOR_DTYPE)
        n = anchors.shape[0]
        a, o, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.necat_asm_align_batch(self.h, ref.h, reads.h, read_start_id, ref_start_id, anchors.ctypes.data, n, error, min_align_size,
                                                   C.byref(a), C.byref(o), C.byref(f)), "necat_asm_align_batch")
        off = self._take(f, n + 1, np.dtype("<u8"))
        return self._take(a, n, ALIGNMENT_DTYPE), self._take(o, max(8, int(off[-1])), np.dtype("u1")), off

    def asm_map_batch(self, ref: "Volume", reads: "Volume", read_start_id: int, ref_start_id: int, plans: np.ndarray, error: float = 0.5,
                      min_align_size: int = 400, min_ident_perc: float = 65.0):
        """hbn_map_extend (oc2asmpm from the anchor to the record: block aligner, DALIGNER's end extension, fix_ident_perc) for every planned anchor
        (ASM_PLAN_DTYPE, qoff < 0: skipped): (records[M4_DTYPE], kept[uint8], AsmMapStats), both arrays in plan order"""
        plans = np.ascontiguousarray(plans, dtype=ASM_PLAN_DTYPE)
        n = plans.shape[0]
        r, k = C.c_void_p(), C.c_void_p()
        st = AsmMapStats()
        self._check(self.lib.necat_asm_map_batch(self.h, ref.h, reads.h, read_start_id, ref_start_id, plans.ctypes.data, n, error, min_align_size, min_ident_perc,
                                                 C.byref(r), C.byref(k), C.byref(st)), "necat_asm_map_batch")
        return self._take(r, max(1, n), M4_DTYPE)[:n], self._take(k, max(1, n), np.dtype("u1"))[:n], st

    def cns_load_partition(self, reads: "Volume", packed: np.ndarray):
        """order and cut of one candidate partition as oc2cns does it: (cands, tmpl_off, n_all)"""
        packed = np.ascontiguousarray(packed).view(np.uint8).reshape(-1)
        n = packed.shape[0] // 28
        c, o, a, nt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self.lib.necat_cns_load_partition(self.h, reads.h, packed.ctypes.data, n, C.byref(c), C.byref(o), C.byref(a),
                                                      C.byref(nt)), "necat_cns_load_partition")
        off = self._take(o, nt.value + 1, np.dtype("<u8"))
        return self._take(c, int(off[-1]), CANDIDATE_DTYPE), off, self._take(a, nt.value, np.dtype("<u8"))

    def cns_extension_batch(self, reads: "Volume", cands: np.ndarray, tmpl_off: np.ndarray, n_all, opt: CnsOptions) -> "CnsResult":
        """the consensus stage's extension loop for all templates of the call (include/necat_hip.h)"""
        cands = np.ascontiguousarray(cands, dtype=CANDIDATE_DTYPE)
        tmpl_off = np.ascontiguousarray(tmpl_off, dtype=np.uint64)
        na = None if n_all is None else np.ascontiguousarray(n_all, dtype=np.uint64)
        r = C.POINTER(_CnsResult)()
        self._check(self.lib.necat_cns_extension_batch(self.h, reads.h, cands.ctypes.data, tmpl_off.ctypes.data,
                                                       None if na is None else na.ctypes.data, tmpl_off.shape[0] - 1,
                                                       C.byref(opt), C.byref(r)), "necat_cns_extension_batch")
        return CnsResult(self.lib, r)

    def cns_consensus_batch(self, reads: "Volume", cands: np.ndarray, tmpl_off: np.ndarray, ext, opt: CnsConsensusOptions) -> "CnsConsensus":
        """necat_cns_consensus_batch: the consensus proper of every template of `ext` (a CnsResult, or a CraftedCnsResult made from numpy arrays); cands / tmpl_off as
        given to cns_extension_batch"""
        cands = np.ascontiguousarray(cands, dtype=CANDIDATE_DTYPE)
        tmpl_off = np.ascontiguousarray(tmpl_off, dtype=np.uint64)
        r = C.POINTER(_CnsConsensus)()
        self._check(self.lib.necat_cns_consensus_batch(self.h, reads.h, cands.ctypes.data, tmpl_off.ctypes.data, tmpl_off.shape[0] - 1, ext.r, C.byref(opt), C.byref(r)),
                    "necat_cns_consensus_batch")
        return CnsConsensus(self.lib, r)

    def ctg_consensus_batch(self, reads: "Volume", read_start_id: int, contigs: Optional["Volume"], segments: np.ndarray, overlaps: np.ndarray, ops: np.ndarray,
                            opt: CtgConsensusOptions) -> "CtgConsensus":
        """necat_ctg_consensus_batch: the consensus half of contig polishing for every segment (CTG_SEGMENT_DTYPE) with its overlaps (CTG_OVERLAP_DTYPE; columns two
        bits each in `ops`, pack_columns); contigs = None: no polished strings"""
        segments = np.ascontiguousarray(segments, dtype=CTG_SEGMENT_DTYPE)
        overlaps = np.ascontiguousarray(overlaps, dtype=CTG_OVERLAP_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.uint8)
        if overlaps.shape[0] and int((overlaps["ops_off"] + (overlaps["align_size"].clip(0).astype(np.uint64) + np.uint64(3)) // np.uint64(4)).max()) > ops.shape[0]:
            raise ValueError("an overlap's columns lie outside `ops`")
        if segments.shape[0] and int(segments["ovlp_end"].max()) > overlaps.shape[0]:
            raise ValueError("a segment's overlaps lie outside `overlaps`")
        r = C.POINTER(_CtgConsensus)()
        self._check(self.lib.necat_ctg_consensus_batch(self.h, reads.h, read_start_id, contigs.h if contigs is not None else None, segments.ctypes.data, segments.shape[0],
                                                       overlaps.ctypes.data if overlaps.shape[0] else None, ops.ctypes.data if ops.shape[0] else None, C.byref(opt), C.byref(r)),
                    "necat_ctg_consensus_batch")
        return CtgConsensus(self.lib, r)

    def ctg_seed_batch(self, reads: "Volume", read_start_id: int, contigs: "Volume", segments: np.ndarray, jobs: np.ndarray, opt: CtgSeedOptions) -> "CtgSeed":
        """necat_ctg_seed_batch: the seeding of contig polishing for every job (CTG_SEED_JOB_DTYPE: read id, strand) of every segment (CTG_SEGMENT_DTYPE, whose
        ovlp_begin .. ovlp_end index `jobs`): can_list[0] of the reference's MaximalExactMatchWorkData_FindCandidates, or none"""
        segments = np.ascontiguousarray(segments, dtype=CTG_SEGMENT_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=CTG_SEED_JOB_DTYPE)
        if segments.shape[0] and int(segments["ovlp_end"].max()) > jobs.shape[0]:
            raise ValueError("a segment's jobs lie outside `jobs`")
        r = C.POINTER(_CtgSeed)()
        self._check(self.lib.necat_ctg_seed_batch(self.h, reads.h, read_start_id, contigs.h if contigs is not None else None, segments.ctypes.data, segments.shape[0],
                                                  jobs.ctypes.data if jobs.shape[0] else None, C.byref(opt), C.byref(r)), "necat_ctg_seed_batch")
        return CtgSeed(self.lib, r)

    def ctg_extend_batch(self, reads: "Volume", read_start_id: int, contigs: "Volume", segments: np.ndarray, jobs: np.ndarray, seeds: Optional["CtgSeed"],
                         opt: CtgExtendOptions) -> "CtgExtend":
        """necat_ctg_extend_batch: the aligner and the coverage cap of contig polishing for every job (CTG_EXTEND_JOB_DTYPE: read id, strand, the record's range on the
        contig) of every segment (CTG_SEGMENT_DTYPE, whose ovlp_begin .. ovlp_end index `jobs`); seeds: a ctg_seed_batch result over the same segments and jobs, or
        None - the entry then seeds itself"""
        segments = np.ascontiguousarray(segments, dtype=CTG_SEGMENT_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=CTG_EXTEND_JOB_DTYPE)
        if segments.shape[0] and int(segments["ovlp_end"].max()) > jobs.shape[0]:
            raise ValueError("a segment's jobs lie outside `jobs`")
        table, sj = None, None
        if seeds is not None:
            sj = np.ascontiguousarray(seeds.jobs, dtype=CTG_SEED_RESULT_DTYPE)
            table = _CtgSeed(n_jobs=sj.shape[0], jobs=sj.ctypes.data if sj.shape[0] else None)
        r = C.POINTER(_CtgExtend)()
        self._check(self.lib.necat_ctg_extend_batch(self.h, reads.h, read_start_id, contigs.h if contigs is not None else None, segments.ctypes.data, segments.shape[0],
                                                    jobs.ctypes.data if jobs.shape[0] else None, C.byref(table) if table is not None else None, C.byref(opt), C.byref(r)),
                    "necat_ctg_extend_batch")
        return CtgExtend(self.lib, r)

    def edlib_align_batch(self, seqs: np.ndarray, q_off, q_len, t_off, t_len, error: float = 0.5, want_ops: bool = True):
        """necat_edlib_align_batch, the block-by-block hook of the parity tests: it exists in the cross-check build only, so a product context hands the call to a
        cross-check context of its own (made on first use, with the knobs of the environment at that moment)"""
        if not self.xcheck:
            # (a context reads its knobs when it is made: a cross-check context per knob environment, so that a test's NECAT_* settings choose the kernels they name)
            key = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("NECAT_")))
            if self._xc is None or self._xc_key != key:
                if self._xc is not None:
                    self._xc.close()
                self._xc, self._xc_key = Context(self.device, xcheck=True), key
            return self._xc.edlib_align_batch(seqs, q_off, q_len, t_off, t_len, error, want_ops)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.int32)
        t_len = np.ascontiguousarray(t_len, dtype=np.int32)
        n = q_off.shape[0]
        dist = np.zeros(n, dtype=np.int32)
        qend = np.zeros(n, dtype=np.int32)
        tend = np.zeros(n, dtype=np.int32)
        ops = C.c_void_p()
        ops_off = C.c_void_p()
        self._check(self.lib.necat_edlib_align_batch(self.h, seqs.ctypes.data, seqs.shape[0], q_off.ctypes.data,
                                                     q_len.ctypes.data, t_off.ctypes.data, t_len.ctypes.data, n, error,
                                                     dist.ctypes.data, qend.ctypes.data, tend.ctypes.data,
                                                     C.byref(ops) if want_ops else None,
                                                     C.byref(ops_off) if want_ops else None), "necat_edlib_align_batch")
        o = oo = None
        if want_ops and n:
            oo = self._take(ops_off, n + 1, np.dtype("<u8"))
            o = self._take(ops, int(oo[-1]), np.dtype("u1"))
        return dist, qend, tend, o, oo

    def trim_partition(self, recs: np.ndarray, num_reads: int, min_ident_perc: float, download: bool = True):
        """necat_trim_partition (oc2pm4 on records in memory): the records that reach min_ident_perc, each under its subject and - exchanged - under
        its query, grouped by read id.  The groups stay on the device for trim_ranges().  Returns (grouped records, read_off[num_reads + 3]), or the
        number of grouped records when download is False."""
        recs = np.ascontiguousarray(recs, dtype=M4_DTYPE)
        g, off, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self.lib.necat_trim_partition(self.h, recs.ctypes.data, recs.shape[0], num_reads, float(min_ident_perc),
                                                  C.byref(g) if download else None, C.byref(off) if download else None, C.byref(n)), "necat_trim_partition")
        if not download:
            return int(n.value)
        return self._take(g, n.value, M4_DTYPE), self._take(off, num_reads + 3, np.dtype("<u8"))

    def trim_ranges(self, num_reads: int, min_ident_perc: float, min_ovlp_size: int, min_cov: int, min_size: int, grouped: Optional[np.ndarray] = None,
                    read_off: Optional[np.ndarray] = None):
        """necat_trim_ranges (oc2lcr's per-read decision, final pass included): (ranges[num_reads + 2] as CLIP_RANGE_DTYPE, number of reads handed back
        as how == TRIM_HOST).  grouped / read_off: records grouped by subject id; both None = what the last trim_partition() left on the device."""
        out = np.zeros(num_reads + 2, dtype=CLIP_RANGE_DTYPE)
        nh = C.c_uint64()
        gp = op = None
        if grouped is not None:
            grouped = np.ascontiguousarray(grouped, dtype=M4_DTYPE)
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
            if read_off.shape[0] != num_reads + 3 or int(read_off[-1]) != grouped.shape[0]:
                raise ValueError("read_off must have num_reads + 3 entries and end at the number of records")
            gp, op = grouped.ctypes.data, read_off.ctypes.data
        self._check(self.lib.necat_trim_ranges(self.h, gp, op, num_reads, float(min_ident_perc), min_ovlp_size, min_cov, min_size, out.ctypes.data, C.byref(nh)),
                    "necat_trim_ranges")
        return out, int(nh.value)

    def _take(self, p: C.c_void_p, n: int, dtype: np.dtype) -> np.ndarray:
        """Wrap a library-malloc'ed result array without copying; necat_free runs when the array dies."""
        if not p.value:
            return np.zeros(0, dtype=dtype)
        if n == 0:
            self.lib.necat_free(p)
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * dtype.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=n)
        weakref.finalize(buf, self.lib.necat_free, C.c_void_p(p.value))   # arr keeps buf alive through .base
        return arr


class Comm:
    """necat_comm: the rank-to-rank data path (RCCL or HIP IPC) + the caller's host all-gather as a C callback"""

    def __init__(self, ctx: Context, rank: int, nranks: int, allgather, transport: str = "auto"):
        self.ctx, self.rank, self.nranks = ctx, rank, nranks

        def cb(_user, send, recv, nbytes):
            try:
                parts = allgather(C.string_at(send, nbytes))
                if len(parts) != nranks or any(len(x) != nbytes for x in parts):
                    return 2
                C.memmove(recv, b"".join(parts), nbytes * nranks)
                return 0
            except Exception:      # an exception must not cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._cb = HOST_ALLGATHER_FN(cb)          # kept alive as long as the communicator
        h = C.c_void_p()
        ctx._check(ctx.lib.necat_comm_create(ctx.h, rank, nranks, self._cb, None, transport.encode(), C.byref(h)), "necat_comm_create")
        self.h = h

    def transport(self) -> str:
        b = C.create_string_buffer(16)
        self.ctx.lib.necat_comm_transport(self.h, b, 16)
        return b.value.decode()

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.necat_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CnsResult:
    """necat_cns_result: templates / overlaps / ranges are numpy views, valid until free()"""

    def __init__(self, lib, r):
        self.lib, self.r = lib, r
        c = r.contents
        self.templates = self._view(c.templates, c.n_templates, CNS_TEMPLATE_DTYPE)
        self.overlaps = self._view(c.overlaps, c.n_overlaps, CNS_OVERLAP_DTYPE)
        self.ranges = self._view(c.ranges, 2 * c.n_ranges, np.dtype("<i4")).reshape(-1, 2)
        self.n_aligned, self.n_used, self.n_rounds = c.n_aligned, c.n_used, c.n_rounds
        self.device_ms, self.host_ms = c.device_ms, c.host_ms
        self.n_rescue_tried, self.n_rescued, self.rescue_ms = c.n_rescue_tried, c.n_rescued, c.rescue_ms
        self.rescue_dalign_ms, self.rescue_nw_ms = c.rescue_dalign_ms, c.rescue_nw_ms
        self.n_rescue_nw, self.n_rescue_nw_device, self.n_rescue_nw_host = c.n_rescue_nw, c.n_rescue_nw_device, c.n_rescue_nw_host
        self.n_rescue_dalign_device, self.n_rescue_dalign_host = c.n_rescue_dalign_device, c.n_rescue_dalign_host

    @staticmethod
    def _view(p, n, dtype):
        if not p or n == 0:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(p), dtype=dtype, count=n)

    def ops(self, ov) -> np.ndarray:
        """the packed alignment columns (2 bits each) of one overlap record"""
        n = (int(ov["align_size"]) + 3) // 4
        base = self.r.contents.ops[int(ov["ops_block"])]
        return np.frombuffer((C.c_char * n).from_address(base + int(ov["ops_off"])), dtype=np.uint8, count=n) if n else np.zeros(0, np.uint8)

    def free(self):
        if self.r:
            self.templates = self.overlaps = self.ranges = None
            self.lib.necat_cns_result_free(self.r)
            self.r = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CraftedCnsResult:
    """a necat_cns_result built from numpy arrays (tests hand-craft overlaps with it): templates (CNS_TEMPLATE_DTYPE: examined, num_can, ident_cutoff and
    ovlp_begin / ovlp_end matter), overlaps (CNS_OVERLAP_DTYPE: cand, qoff, qend, toff, tend, weight; align_size / ops_block / ops_off are filled in here) and one array
    of column codes (0 match, 1 query base over '-', 2 '-' over target base, 3 mismatch) per overlap.  The arrays belong to this object: nothing is freed by the library."""

    def __init__(self, templates: np.ndarray, overlaps: np.ndarray, columns):
        self.templates = np.ascontiguousarray(templates, dtype=CNS_TEMPLATE_DTYPE).copy()
        self.overlaps = np.ascontiguousarray(overlaps, dtype=CNS_OVERLAP_DTYPE).copy()
        assert len(columns) == self.overlaps.shape[0]
        packed, at = [], 0
        for i, col in enumerate(columns):
            p = pack_columns(np.ascontiguousarray(col, dtype=np.uint8))
            p = np.concatenate([p, np.zeros((-p.shape[0]) % 8 + 8, np.uint8)])
            self.overlaps[i]["align_size"], self.overlaps[i]["ops_block"], self.overlaps[i]["ops_off"] = len(col), 0, at
            packed.append(p)
            at += p.shape[0]
        self._ops = np.concatenate(packed) if packed else np.zeros(8, np.uint8)
        self._blocks = (C.c_void_p * 1)(self._ops.ctypes.data)
        self._ranges = np.zeros(2, np.int32)
        self._s = _CnsResult(n_templates=self.templates.shape[0], templates=self.templates.ctypes.data, n_overlaps=self.overlaps.shape[0],
                             overlaps=self.overlaps.ctypes.data, n_ranges=0, ranges=self._ranges.ctypes.data, n_ops_blocks=1, ops=self._blocks)
        self.r = C.pointer(self._s)


class CnsConsensus:
    """necat_cns_consensus: templates / segments / bases are numpy views, valid until free()"""

    def __init__(self, lib, r):
        self.lib, self.r = lib, r
        c = r.contents
        self.templates = CnsResult._view(c.templates, c.n_templates, CNS_CONSENSUS_TEMPLATE_DTYPE)
        self.segments = CnsResult._view(c.segments, c.n_segments, CNS_SEGMENT_DTYPE)
        self.bases = CnsResult._view(c.bases, c.n_bases, np.dtype(np.uint8))
        self.n_device, self.n_fallback, self.n_chunks, self.n_uncertain = c.n_device, c.n_fallback, c.n_chunks, c.n_uncertain
        self.device_ms, self.host_ms = c.device_ms, c.host_ms
        self.kernel_ms = dict(tags=c.tags_ms, sort=c.sort_ms, backbone=c.backbone_ms, path=c.path_ms)

    def snapshot(self):
        """what two paths must agree on, as plain Python data: per template (corrected, [(left, right, cns_from, cns_to, bases)])"""
        out = []
        for t in self.templates:
            segs = [(int(s["left"]), int(s["right"]), int(s["cns_from"]), int(s["cns_to"]), self.bases[int(s["off"]):int(s["off"]) + int(s["len"])].tobytes())
                    for s in self.segments[int(t["seg_begin"]):int(t["seg_end"])]]
            out.append((int(t["corrected"]), segs))
        return out

    def free(self):
        if self.r:
            self.templates = self.segments = self.bases = None
            self.lib.necat_cns_consensus_free(self.r)
            self.r = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CtgConsensus:
    """necat_ctg_consensus as plain Python data (copied; the result is released at once): per segment cns (bytes with case), t_pos, polished (bytes; b"" without
    contigs) and the counters, plus the call's times"""

    def __init__(self, lib, r):
        c = r.contents
        seg = CnsResult._view(c.segments, c.n_segments, CTG_CONSENSUS_SEGMENT_DTYPE).copy()
        cns = CnsResult._view(c.cns, c.n_cns, np.dtype(np.uint8)).tobytes()
        t_pos = CnsResult._view(c.t_pos, c.n_cns, np.dtype("<i4")).copy()
        pol = CnsResult._view(c.polished, c.n_polished, np.dtype(np.uint8)).tobytes()
        self.segments = seg
        self.cns = [cns[int(s["cns_off"]):int(s["cns_off"] + s["cns_len"])] for s in seg]
        self.t_pos = [t_pos[int(s["cns_off"]):int(s["cns_off"] + s["cns_len"])] for s in seg]
        self.polished = [pol[int(s["polished_off"]):int(s["polished_off"] + s["polished_len"])] for s in seg]
        self.n_fallback, self.n_chunks = int(c.n_fallback), int(c.n_chunks)
        self.device_ms, self.host_ms, self.plan_ms, self.score_ms = c.device_ms, c.host_ms, c.plan_ms, c.score_ms
        self.kernel_ms = dict(tags=c.tags_ms, sort=c.sort_ms, links=c.links_ms)
        lib.necat_ctg_consensus_free(r)

    def snapshot(self):
        """what two paths must agree on"""
        return [(a, b.tobytes(), c) for a, b, c in zip(self.cns, self.t_pos, self.polished)]


class CtgSeed:
    """necat_ctg_seed as plain Python data (copied; the result is released at once): jobs (CTG_SEED_RESULT_DTYPE), per job its sorted matches (keep_mems; an
    n x 3 array of qoff, soff, size), the counters and the call's times"""

    CANDIDATE = ("found", "qbeg", "qend", "sbeg", "send", "qoff", "soff", "score", "n_matches", "n_mems", "chain_len")

    def __init__(self, lib, r):
        c = r.contents
        self.jobs = CnsResult._view(c.jobs, c.n_jobs, CTG_SEED_RESULT_DTYPE).copy()
        self.all_mems = CnsResult._view(c.mems, c.n_mems, CTG_SEED_MEM_DTYPE).copy()
        self.have_mems = int(c.n_mems) > 0
        self.n_fallback, self.n_lds, self.n_scratch = int(c.n_fallback), int(c.n_lds), int(c.n_scratch)
        self.max_matches, self.max_mems = int(c.max_matches), int(c.max_mems)
        self.device_ms, self.host_ms = c.device_ms, c.host_ms
        self.kernel_ms = dict(index=c.index_ms, match=c.match_ms, chain=c.chain_ms)
        lib.necat_ctg_seed_free(r)

    def mems(self, k):
        """job k's sorted matches as an n x 3 array (keep_mems)"""
        j = self.jobs[k]
        m = self.all_mems[int(j["mems_off"]):int(j["mems_off"]) + int(j["n_mems"])]
        return np.stack([m["qoff"], m["soff"], m["size"]], axis=1).astype(np.int32) if m.shape[0] else np.zeros((0, 3), np.int32)

    def snapshot(self):
        """what two paths, or two calls, must agree on: everything but who decided"""
        return tuple(self.jobs[f].tobytes() for f in self.CANDIDATE) + (self.all_mems.tobytes(),)


class CtgExtend:
    """necat_ctg_extend as plain Python data (copied; the result is released at once): jobs (CTG_EXTEND_RESULT_DTYPE), and what necat_ctg_consensus_batch takes
    unchanged - segments (CTG_SEGMENT_DTYPE, indexing overlaps), overlaps (CTG_OVERLAP_DTYPE, loop order) and ops (their packed columns) -, the counters as
    attributes and the four times in `ms`"""

    def __init__(self, lib, r):
        c = r.contents
        self.jobs = CnsResult._view(c.jobs, c.n_jobs, CTG_EXTEND_RESULT_DTYPE).copy()
        self.segments = CnsResult._view(c.segments, c.n_segments, CTG_SEGMENT_DTYPE).copy()
        self.overlaps = CnsResult._view(c.overlaps, c.n_overlaps, CTG_OVERLAP_DTYPE).copy()
        self.ops = CnsResult._view(c.ops, c.n_ops, np.dtype(np.uint8)).copy()
        for f in _CtgExtend._COUNTERS:
            setattr(self, f, int(getattr(c, f)))
        self.ms = {f[:-3]: float(getattr(c, f)) for f in _CtgExtend._TIMES}
        lib.necat_ctg_extend_free(r)

    def columns(self, k):
        """overlap k's columns, one code per column (0 match, 1 query base against a gap, 2 gap against a segment base, 3 mismatch)"""
        o = self.overlaps[k]
        n, at = int(o["align_size"]), int(o["ops_off"])
        b = self.ops[at:at + (n + 3) // 4]
        return ((b[:, None] >> (np.arange(4, dtype=np.uint8) * 2)) & 3).reshape(-1)[:n].astype(np.uint8)

    def snapshot(self):
        """what two paths, or two calls, must agree on: verdicts, alignments, overlaps and their columns"""
        return (self.jobs.tobytes(), self.segments.tobytes(), self.overlaps.tobytes(), self.ops.tobytes(), self.n_seeded, self.n_aligned, self.n_used)


def ctg_extend_options(**kw) -> CtgExtendOptions:
    o = CtgExtendOptions()
    load_library().necat_ctg_extend_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def ctg_seed_options(**kw) -> CtgSeedOptions:
    o = CtgSeedOptions()
    load_library().necat_ctg_seed_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def ctg_consensus_options(**kw) -> CtgConsensusOptions:
    o = CtgConsensusOptions()
    load_library().necat_ctg_consensus_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def cns_consensus_options(**kw) -> CnsConsensusOptions:
    o = CnsConsensusOptions()
    load_library().necat_cns_consensus_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def cns_options(**kw) -> CnsOptions:
    o = CnsOptions()
    load_library().necat_cns_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


class Volume:
    def __init__(self, ctx: Context, h, nbases: int, offsets: np.ndarray, sizes: np.ndarray):
        self.ctx, self.h, self.nbases, self.offsets, self.sizes = ctx, h, nbases, offsets, sizes
        self.names: List[str] = []

    @property
    def nseq(self) -> int:
        return int(self.sizes.shape[0])

    def download(self) -> np.ndarray:
        """necat_volume_download: the resident bases as pac bytes, (nbases + 3) // 4 of them - what upload_volume took"""
        pac = np.zeros((self.nbases + 3) // 4, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.necat_volume_download(self.ctx.h, self.h, pac.ctypes.data if pac.shape[0] else None), "necat_volume_download")
        return pac

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.necat_volume_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    def __init__(self, ctx: Context, h, k: int):
        self.ctx, self.h, self.k = ctx, h, k

    def sizes(self) -> Tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx.lib.necat_index_size(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def download(self, want_stats: bool = True) -> Tuple[Optional[np.ndarray], np.ndarray]:
        T, n = self.sizes()
        stats = np.empty(T, dtype=np.uint64) if want_stats else None
        offs = np.empty(n, dtype=np.uint64)
        self.ctx._check(self.ctx.lib.necat_index_download(self.ctx.h, self.h, stats.ctypes.data if want_stats else None,
                                                          offs.ctypes.data if n else None), "necat_index_download")
        return stats, offs

    def sparse_sizes(self) -> Tuple[int, int]:
        """(pairs of (bits, base) words, non-zero table entries) of an index in the sparse layout; (0, 0) for a dense one"""
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx.lib.necat_index_sparse_size(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def download_sparse(self):
        """(bits[T / 64], base[T / 64], compact, offset_list) of an index held in the sparse layout (IndexView, dev_common.h); None for a dense one"""
        npairs, ncomp = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx.lib.necat_index_sparse_size(self.h, C.byref(npairs), C.byref(ncomp)), "necat_index_sparse_size")
        if npairs.value == 0:
            return None
        _, n_off = self.sizes()
        pairs = np.empty(2 * npairs.value, dtype=np.uint64)
        comp = np.empty(max(1, ncomp.value), dtype=np.uint64)
        offs = np.empty(max(1, n_off), dtype=np.uint64)
        self.ctx._check(self.ctx.lib.necat_index_download_sparse(self.ctx.h, self.h, pairs.ctypes.data, comp.ctypes.data, offs.ctypes.data), "necat_index_download_sparse")
        return pairs[0::2].copy(), pairs[1::2].copy(), comp[:ncomp.value], offs[:n_off]

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.necat_index_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# --------------------------------------------------------------------------------------------------
# Python mirror of pm_main (pm_one_volume/pm_worker.c:338-400) for tests / bench: volume `vid`
# against every volume >= vid, records returned instead of written.
# --------------------------------------------------------------------------------------------------

def load_volumes_info(wrk_dir: str):
    """common/makedb_aux.c:78-118"""
    base = wrk_dir if wrk_dir.endswith("/") else wrk_dir + "/"
    with open(base + "reads_info.txt") as f:
        nv, nr = [int(x) for x in f.read().split()[:2]]
    vols = []
    with open(base + "volume_names.txt") as f:
        for _ in range(nv):
            parts = f.readline().split()
            vols.append((parts[0], int(parts[1]), int(parts[2])))
    return nv, nr, vols


def pack_columns(ops: np.ndarray) -> np.ndarray:
    """one op code (0..3) per column -> the library's packed form: 2 bits per column, 4 per byte, low bits first"""
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    n = ops.shape[0]
    pad = np.zeros(((n + 3) // 4) * 4, dtype=np.uint8)
    pad[:n] = ops & 3
    q = pad.reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)


def unpack_columns(packed: np.ndarray, n: int) -> np.ndarray:
    p = np.ascontiguousarray(packed, dtype=np.uint8)[:(n + 3) // 4]
    return np.stack([p & 3, (p >> 2) & 3, (p >> 4) & 3, (p >> 6) & 3], axis=1).reshape(-1)[:n].astype(np.uint8)


def gapped_strings(ops: np.ndarray, n: int, qseq: np.ndarray, qoff: int, tseq: np.ndarray, toff: int):
    """necat_gapped_strings: `n` packed columns (2 bits each) -> (query_align, target_align) as bytes ("ACGT-")."""
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    if ops.shape[0] * 4 < n:
        raise ValueError("%d columns need %d bytes, got %d" % (n, (n + 3) // 4, ops.shape[0]))
    q = np.ascontiguousarray(qseq, dtype=np.uint8)
    t = np.ascontiguousarray(tseq, dtype=np.uint8)
    qa = C.create_string_buffer(max(1, n))
    ta = C.create_string_buffer(max(1, n))
    rc = load_library().necat_gapped_strings(ops.ctypes.data, n, q.ctypes.data, q.shape[0], qoff, t.ctypes.data, t.shape[0], toff, qa, ta)
    if rc != 0:
        raise NecatError("necat_gapped_strings failed with %d" % rc)
    return qa.raw[:n], ta.raw[:n]


def pcan_single_partition(packed: bytes) -> bytes:
    """oc2pcan (partition_candidates/pcan.c:39-103) when all reads fall in ONE partition: every record is kept
    and followed by its role-swapped twin (change_pcan_roles, common/gapped_candidate.c:54-69: the subject
    becomes the query, strands swap with them).  Record order inside a partition file is free."""
    a = np.frombuffer(packed, dtype="<u4").reshape(-1, 7)
    b = np.empty_like(a)
    w0 = a[:, 0]
    b[:, 0] = (w0 & np.uint32((1 << 30) - 1)) | ((w0 >> 31) << 30) | (((w0 >> 30) & 1) << 31)
    b[:, 1:4] = a[:, 4:7]
    b[:, 4:7] = a[:, 1:4]
    return np.concatenate([a, b]).tobytes()


def pack_candidates(c: np.ndarray) -> np.ndarray:
    """pack_candidate (common/gapped_candidate.c:13-30): 7 x u32 records."""
    out = np.zeros((c.shape[0], 7), dtype=np.uint32)
    item0 = np.minimum(c["score"], 1000000).astype(np.uint32)
    item0 |= (c["sdir"] == 1).astype(np.uint32) << 31
    item0 |= (c["qdir"] == 1).astype(np.uint32) << 30
    item0 |= (c["qoff"] == c["qbeg"]).astype(np.uint32) << 29
    out[:, 0] = item0
    out[:, 1] = c["sid"].astype(np.uint32)
    out[:, 2] = c["sbeg"].astype(np.uint32)
    out[:, 3] = c["send"].astype(np.uint32)
    out[:, 4] = c["qid"].astype(np.uint32)
    out[:, 5] = c["qbeg"].astype(np.uint32)
    out[:, 6] = c["qend"].astype(np.uint32)
    return out


def m4_text_lines(m: np.ndarray) -> List[bytes]:
    """DUMP_ASM_M4 (common/m4_record.h:72-97), numeric ids."""
    return [b"%d\t%d\t%.2f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" %
            (r["qid"], r["sid"], r["ident_perc"], r["vscore"], r["qdir"], r["qoff"], r["qend"], r["qsize"],
             r["sdir"], r["soff"], r["send"], r["ssize"]) for r in m]


def candidate_text_lines(c: np.ndarray) -> List[bytes]:
    """DUMP_GAPPED_CANDIDATE (common/gapped_candidate.h:26-42)."""
    return [b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" %
            (r["qid"], r["sid"], r["score"], r["qdir"], r["qbeg"], r["qend"], r["qoff"], r["qsize"], r["sdir"],
             r["sbeg"], r["send"], r["soff"], r["ssize"]) for r in c]


PAIR_UNIT_DTYPE = np.dtype([("ref_vol", "<i4"), ("query_vol", "<i4"), ("slot_lo", "<i4"), ("slot_hi", "<i4")])


def pair_chunk_reads(query_reads: int, slots: int = 64) -> int:
    return int(load_library().necat_pair_chunk_reads(int(query_reads), slots))


def pair_schedule(vol_bases, nranks: int, slots: int = 64):
    """necat_pair_schedule (host arithmetic only, no device): (units[PAIR_UNIT_DTYPE], rank_off[nranks + 1], team[V, 2]) - rank g
    owns units[rank_off[g]:rank_off[g + 1]]; ranks team[v, 0] .. team[v, 1] (inclusive) work on reference volume v."""
    lib = load_library()
    vb = np.ascontiguousarray(vol_bases, dtype=np.uint64)
    V = int(vb.shape[0])
    pu, po, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.necat_pair_schedule(vb.ctypes.data, V, nranks, slots, C.byref(pu), C.byref(po), C.byref(pt))
    if rc:
        raise NecatError("necat_pair_schedule failed (%d)" % rc)
    off = np.frombuffer((C.c_char * (8 * (nranks + 1))).from_address(po.value), dtype=np.uint64).copy()
    n = int(off[nranks])
    units = np.frombuffer((C.c_char * (16 * max(n, 1))).from_address(pu.value), dtype=PAIR_UNIT_DTYPE)[:n].copy()
    team = np.frombuffer((C.c_char * (8 * V)).from_address(pt.value), dtype=np.int32).reshape(V, 2).copy()
    for q in (pu, po, pt):
        lib.necat_free(q)
    return units, off.astype(np.int64), team


def pm_main(ctx: Context, opt: MapOptions, vid: int, wrk_dir: str):
    """Returns (candidates, m4) over all volume pairs (vid, i >= vid); m4 is None for job 0."""
    nv, _, vols = load_volumes_info(wrk_dir)
    ref = ctx.load_volume(vols[vid][0])
    ix = ctx.build_index(ref, opt.kmer_size, opt.kmer_cnt_cutoff)
    cands, m4s = [], []
    for i in range(vid, nv):
        reads = ref if i == vid else ctx.load_volume(vols[i][0])
        c = ctx.find_candidates(ix, ref, reads, vols[i][1], vols[vid][1], opt, True)
        cands.append(c)
        if opt.job == 1:
            m4s.append(ctx.extend(ref, reads, vols[i][1], vols[vid][1], c, opt, 1))
        if reads is not ref:
            reads.free()
    ix.free()
    ref.free()
    return np.concatenate(cands), (np.concatenate(m4s) if opt.job == 1 else None)
