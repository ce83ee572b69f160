"""deciphon-old_amd -- MI355X-native profile-HMM scan engine (host binding).

Thin ctypes layer over the C-ABI of ``include/dcp_gpu.h`` (``libdcp_hip.so``,
built from ``csrc/`` by hipcc for gfx950).  It mirrors the reference's interface
for the scan hot path so tests read like the reference's own:

=====================================  =========================================
reference (deciphon-old)               here
=====================================  =========================================
protein_profile_init + _sample         ``ProteinProfile.sample(seed, core_size, cfg)``
protein_profile_init + _absorb(model)  ``ProteinProfile.from_params(...)``
protein_profile_setup(prof, L, ...)    ``xtrans(L, multi_hits, hmmer3_compat)`` (EINVAL on L=0)
profile_reader_setup/rewind/next       ``Scanner.upload_db(profiles)`` (resident, once)
imm_seq + imm_task_setup               ``Scanner.upload_seqs(seqs)``
thread_run (per (seq, profile) pair)   ``Scanner.scan(multi_hits, hmmer3_compat, lrt_threshold)``
xmath_lrt                              ``lrt(null, alt)``
=====================================  =========================================

There is NO CPU fallback: importing works without a GPU (so the host logic and
the symbol table can be tested), but creating a ``Scanner`` without a HIP device
raises, and a missing ``libdcp_hip.so`` raises at import.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libdcp_hip.so")
CSRC = os.path.join(_HERE, "csrc")

# enum rc (include/deciphon/core/rc.h:4-15)
RC_OK, RC_END, RC_EFAIL, RC_EINVAL, RC_EIO, RC_ENOMEM, RC_EPARSE, RC_EAPI, RC_EHTTP = range(9)
RC_NAMES = ["RC_OK", "RC_END", "RC_EFAIL", "RC_EINVAL", "RC_EIO", "RC_ENOMEM", "RC_EPARSE",
            "RC_EAPI", "RC_EHTTP"]
# enum entry_dist (include/deciphon/model/entry_dist.h)
ENTRY_DIST_NULL, ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY = 0, 1, 2
NCODES = 1364
NDIST = 129
NXTRANS = 13
CORE_SIZE_MAX = 4096
NUM_THREADS = 64

# every symbol include/dcp_gpu.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "dcp_profile_new", "dcp_profile_sample", "dcp_profile_del", "dcp_profile_core_size",
    "dcp_profile_from_parts", "dcp_profile_entry_dist", "dcp_profile_epsilon", "dcp_rnd_seed", "dcp_rnd_next",
    "dcp_dist_unique_id", "dcp_dist_init", "dcp_dist_init_from_file", "dcp_dist_free", "dcp_dist_rank",
    "dcp_dist_nranks", "dcp_dist_last_error", "dcp_dist_shard", "dcp_dist_gather_hits", "dcp_dist_free_hits",
    "dcp_dist_merge_hits", "dcp_dist_gather_scan_hits", "dcp_dist_gather_plan", "dcp_dist_init_from_file_run",
    "dcp_dist_comm_count", "dcp_dist_last_gather_ms", "dcp_plan_query_slots",
    "dcp_lprob_normalize", "dcp_h3reader_open_fp", "dcp_h3reader_next_params", "dcp_gpu_seqs_set_xtrans",
    "dcp_profile_accession", "dcp_profile_trans8", "dcp_profile_null_dist",
    "dcp_profile_insert_dist", "dcp_profile_match_dist", "dcp_frame_table_host", "dcp_xtrans",
    "dcp_lrt", "dcp_partition_by_count", "dcp_partition_by_cells", "dcp_gpu_device_count",
    "dcp_gpu_ctx_new", "dcp_gpu_ctx_del", "dcp_gpu_last_error", "dcp_gpu_stream",
    "dcp_gpu_db_upload", "dcp_gpu_db_nprofiles", "dcp_gpu_db_fetch_match_table",
    "dcp_gpu_db_one_layout", "dcp_gpu_db_table_bytes",
    "dcp_gpu_seqs_upload", "dcp_gpu_seqs_upload_text", "dcp_gpu_nseqs", "dcp_gpu_scan",
    "dcp_gpu_sync", "dcp_gpu_last_scan_kernel", "dcp_gpu_hit_buffer", "dcp_gpu_last_scan_redo_pairs", "dcp_gpu_last_scan_ms", "dcp_gpu_last_scan_launches", "dcp_gpu_fetch_scores",
    "dcp_gpu_fetch_hits", "dcp_gpu_scan_range", "dcp_gpu_set_hit_buffer",
    "dcp_gpu_last_scan_launch_info", "dcp_gpu_scan_cells", "dcp_gpu_scan_algorithmic_bytes",
    "dcp_gpu_trace_paths", "dcp_state_name", "dcp_profile_decode", "dcp_gc_decode",
    "dcp_prod_format_row", "dcp_prod_header", "dcp_h3reader_open", "dcp_h3reader_next",
    "dcp_h3reader_error", "dcp_h3reader_close", "dcp_swissprot_null_lprobs", "dcp_profile_consensus",
    "dcp_db_write", "dcp_db_open", "dcp_db_close", "dcp_db_nprofiles", "dcp_db_entry_dist", "dcp_db_epsilon",
    "dcp_db_profile_sizes", "dcp_db_partitions", "dcp_db_read",
    # the double build
    "dcp_profile_new64", "dcp_profile_sample64", "dcp_profile_precision", "dcp_profile_epsilon64",
    "dcp_profile_trans8_64", "dcp_profile_null_dist64", "dcp_profile_insert_dist64", "dcp_profile_match_dist64",
    "dcp_xtrans64", "dcp_gpu_db_upload64", "dcp_gpu_db_precision", "dcp_gpu_set_lrt_threshold64", "dcp_gpu_fetch_scores64", "dcp_gpu_fetch_hits64",
    "dcp_gpu_db_fetch_match_table64", "dcp_gpu_db_fetch_insert_null64", "dcp_gpu_trace_paths64",
    "dcp_gpu_seqs_set_xtrans64", "dcp_profile_from_parts64", "dcp_lprob_normalize64",
    "dcp_gpu_last_scan_query_plan",
    # the double build across GPUs: the caller's hit buffer and the gather of struct dcp_hit64 records
    "dcp_gpu_set_hit_buffer64", "dcp_gpu_hit_buffer64", "dcp_dist_gather_scan_hits64", "dcp_dist_gather_hits64",
    "dcp_dist_merge_hits64", "dcp_dist_free_hits64",
    # both strands: the reverse complement of the resident batch
    "dcp_gpu_seqs_add_revcomp", "dcp_gpu_seqs_strands", "dcp_gpu_seqs_fetch", "dcp_seq_revcomp",
    # windows: the resident batch cut into overlapping windows
    "dcp_seq_window_count", "dcp_seq_window_start", "dcp_seq_window_plan", "dcp_gpu_seqs_cut_windows",
    "dcp_gpu_seqs_windows", "dcp_gpu_seqs_window_map",
    # the decode of paths on the device
    "dcp_gpu_db_keep_dists", "dcp_gpu_db_has_dists", "dcp_gpu_decode_paths", "dcp_profile_codon_joint",
    "dcp_prod_format_row_codes",
    # domains: hit paths split at B .. E on the device, located on their sources, merged
    "dcp_gpu_path_domains", "dcp_gpu_path_domains64", "dcp_gpu_path_domains_kernel_ms", "dcp_domains_locate",
    "dcp_gpu_domains_locate", "dcp_domains_merge",
    # rescoring: located domains joined into regions, regions cut out of the resident batch, a pair list scored
    "dcp_domains_regions", "dcp_domains_locate_regions", "dcp_gpu_seqs_cut_regions", "dcp_gpu_seqs_regions",
    "dcp_gpu_seqs_region_map", "dcp_gpu_scan_pairs",
    # calibration: a random batch and one Gumbel fit per profile on the device, their host twins, E-values
    "dcp_seq_random_thresholds", "dcp_seq_random", "dcp_gpu_seqs_random", "dcp_gumbel_fit", "dcp_gpu_fit_gumbel",
    "dcp_gpu_db_calibrate", "dcp_gpu_calib_kernel_ms", "dcp_gumbel_sf", "dcp_hits_evalues", "dcp_hits_evalues64",
    # the tail fit: the k-th largest score per profile, a censored Gumbel fit over the scores from it up
    "dcp_gumbel_fit_tail", "dcp_gpu_fit_gumbel_tail", "dcp_gpu_db_calibrate_tail", "dcp_gpu_calib_tail_kernel_ms",
    # Forward scores of a pair list: a log-sum-exp sweep on the device, and its host twin
    "dcp_forward_tables", "dcp_gpu_forward_pairs", "dcp_gpu_forward_kernel_ms",
    # Backward sweep and posterior decoding of a pair list, the host twin, envelopes from the core row
    "dcp_posterior_tables", "dcp_posterior_envelopes", "dcp_gpu_posterior_pairs", "dcp_gpu_posterior_kernel_ms",
    # the posterior-decoded alignment of a pair list: a max-plus sweep over word posteriors, and its host twins
    "dcp_mea_tables", "dcp_mea_path_gain", "dcp_gpu_mea_pairs", "dcp_gpu_mea_kernel_ms",
    # Forward E-values: the dense Forward scan, the exponential tail fit per profile, E-values of score arrays
    "dcp_gpu_forward_dense", "dcp_gpu_fetch_forward_scores", "dcp_gpu_forward_dense_kernel_ms", "dcp_exp_tail_fit",
    "dcp_gpu_fit_exp_tail", "dcp_gpu_exp_tail_kernel_ms", "dcp_gpu_db_calibrate_forward", "dcp_exp_sf",
    "dcp_scores_evalues",
    # the scaled probability-space Forward sweep: pair lists and the dense scan, the host twin, the float factor rule
    "dcp_fwd_factor_f32", "dcp_forward_scaled_tables", "dcp_forward_scaled_tables_band", "dcp_gpu_forward_pairs_scaled",
    "dcp_gpu_forward_scaled_redo_pairs", "dcp_gpu_forward_scaled_kernel_ms", "dcp_gpu_forward_dense_scaled",
    "dcp_gpu_forward_dense_is_scaled",
    # the scaled Backward sweep and posterior rows of a pair list, and the host twin
    "dcp_posterior_scaled_tables", "dcp_posterior_scaled_tables_band", "dcp_gpu_posterior_pairs_scaled",
    "dcp_gpu_posterior_scaled_redo_pairs", "dcp_gpu_posterior_scaled_kernel_ms",
    # posterior envelopes of a pair list found on the device, the host twin, envelopes as regions to cut
    "dcp_posterior_envelope_records", "dcp_gpu_envelope_pairs", "dcp_gpu_envelope_kernel_ms", "dcp_envelopes_regions",
]


class DcpError(RuntimeError):
    def __init__(self, rc, msg=""):
        self.rc = rc
        name = RC_NAMES[rc] if 0 <= rc < len(RC_NAMES) else str(rc)
        super().__init__(f"{name}: {msg}" if msg else name)


def build(verbose=False):
    """Compile csrc/ for gfx950 into libdcp_hip.so (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC] + ([] if verbose else ["-s"]))
    return LIB_PATH


class ScanParams(C.Structure):
    _fields_ = [("multi_hits", C.c_int), ("hmmer3_compat", C.c_int),
                ("lrt_threshold", C.c_float), ("keep_scores", C.c_int), ("kernel", C.c_int)]


KERNEL_AUTO, KERNEL_ROWSWEEP, KERNEL_QLANE, KERNEL_QLANE2 = 0, 1, 2, 3
KERNEL_QLANE64 = 4  # double DBs only: the f64 query-lane kernel
DB_EXPAND_ON_HOST, DB_ONE_LAYOUT = 1, 2  # dcp_gpu_db_upload flags (include/dcp_gpu.h)


class Hit(C.Structure):
    _fields_ = [("seq_idx", C.c_uint32), ("profile_idx", C.c_uint32),
                ("null_loglik", C.c_float), ("alt_loglik", C.c_float)]


class Hit64(C.Structure):
    _fields_ = [("seq_idx", C.c_uint32), ("profile_idx", C.c_uint32),
                ("null_loglik", C.c_double), ("alt_loglik", C.c_double)]


class LaunchInfo(C.Structure):
    _fields_ = [("nodes_per_lane", C.c_int), ("waves_per_pair", C.c_int), ("nprofiles", C.c_uint),
                ("ms", C.c_float), ("cells", C.c_uint64), ("algorithmic_bytes", C.c_uint64)]


CODE_MUTE = 0xFF  # DCP_CODE_MUTE: the code of a step that emits nothing (Scanner.decode_paths)
STEP_DTYPE = np.dtype([("state_id", np.uint16), ("seqlen", np.uint8), ("reserved", np.uint8)])
HIT_DTYPE = np.dtype([("seq_idx", np.uint32), ("profile_idx", np.uint32),
                      ("null_loglik", np.float32), ("alt_loglik", np.float32)])
HIT64_DTYPE = np.dtype([("seq_idx", np.uint32), ("profile_idx", np.uint32),
                        ("null_loglik", np.float64), ("alt_loglik", np.float64)])
# struct dcp_domain: one B .. E stretch of an alt path (Scanner.path_domains)
DOMAIN_DTYPE = np.dtype([(f, np.uint32) for f in ("path", "step_begin", "step_end", "seq_begin", "seq_end", "node_first",
                                                   "node_last", "n_match", "n_insert", "n_delete", "n_shift", "reserved")])
# struct dcp_envelope (48 bytes): a posterior envelope of pair `pair` of a list, bases [begin, end) of its sequence
ENVELOPE_DTYPE = np.dtype([("pair", np.uint32), ("begin", np.uint32), ("end", np.uint32), ("peak", np.uint32),
                           ("core_max", np.float64), ("core_sum", np.float64), ("begin_sum", np.float64),
                           ("end_sum", np.float64)])


def _load(path=None, hooks=False):
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C deciphon-old_amd/csrc` (there is no CPU fallback)")
    lib = C.CDLL(path)
    P, F, U, I = C.c_void_p, C.c_float, C.c_uint, C.c_int
    sig = {
        "dcp_profile_new": (P, [C.c_char_p, U, I, F, P, P, P, C.c_char_p, C.POINTER(I)]),
        "dcp_profile_sample": (P, [C.c_char_p, U, U, I, F, C.POINTER(I)]),
        "dcp_profile_del": (None, [P]),
        "dcp_profile_core_size": (U, [P]),
        "dcp_profile_accession": (C.c_char_p, [P]),
        "dcp_profile_trans8": (P, [P]),
        "dcp_profile_null_dist": (P, [P]),
        "dcp_profile_insert_dist": (P, [P]),
        "dcp_profile_match_dist": (P, [P]),
        "dcp_frame_table_host": (None, [P, F, P]),
        "dcp_xtrans": (I, [U, I, I, P]),
        "dcp_lrt": (F, [F, F]),
        "dcp_partition_by_count": (U, [U, U, P]),
        "dcp_partition_by_cells": (None, [P, U, U, P]),
        "dcp_gpu_device_count": (I, []),
        "dcp_gpu_ctx_new": (P, [I]),
        "dcp_gpu_ctx_del": (None, [P]),
        "dcp_gpu_last_error": (C.c_char_p, [P]),
        "dcp_gpu_stream": (P, [P]),
        "dcp_gpu_db_upload": (I, [P, P, U, I]),
        "dcp_gpu_db_nprofiles": (U, [P]),
        "dcp_gpu_db_one_layout": (I, [P]),
        "dcp_gpu_db_table_bytes": (C.c_uint64, [P]),
        "dcp_gpu_db_fetch_match_table": (I, [P, U, P]),
        "dcp_gpu_seqs_upload": (I, [P, P, P, U]),
        "dcp_gpu_seqs_upload_text": (I, [P, C.c_char_p, P, U]),
        "dcp_gpu_nseqs": (U, [P]),
        "dcp_gpu_seqs_set_xtrans": (I, [P, P, U]),
        "dcp_gpu_scan": (I, [P, C.POINTER(ScanParams)]),
        "dcp_gpu_sync": (I, [P]),
        "dcp_gpu_last_scan_redo_pairs": (I, [P, C.POINTER(U)]),
        "dcp_gpu_last_scan_query_plan": (I, [P, C.POINTER(U), C.POINTER(C.c_ulonglong), C.POINTER(U), C.POINTER(U)]),
        "dcp_gpu_last_scan_ms": (F, [P]),
        "dcp_gpu_last_scan_launches": (U, [P]),
        "dcp_gpu_last_scan_kernel": (I, [P]),
        "dcp_gpu_fetch_scores": (I, [P, P, P]),
        "dcp_gpu_fetch_hits": (I, [P, P, U, C.POINTER(U)]),
        "dcp_gpu_scan_range": (I, [P, C.POINTER(ScanParams), U, U]),
        "dcp_gpu_set_hit_buffer": (I, [P, P, U, P]),
        "dcp_gpu_hit_buffer": (I, [P, C.POINTER(P), C.POINTER(P), C.POINTER(U)]),
        "dcp_gpu_set_hit_buffer64": (I, [P, P, U, P]),
        "dcp_gpu_hit_buffer64": (I, [P, C.POINTER(P), C.POINTER(P), C.POINTER(U)]),
        "dcp_gpu_last_scan_launch_info": (I, [P, U, C.POINTER(LaunchInfo)]),
        "dcp_gpu_trace_paths": (I, [P, P, U, I, I, I, P, U, P, P]),
        "dcp_state_name": (U, [U, C.c_char_p]),
        "dcp_profile_decode": (I, [P, P, U, U, P]),
        "dcp_gc_decode": (C.c_char, [P]),
        "dcp_prod_format_row": (C.c_long, [C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_char_p, C.c_char_p,
                                           C.c_double, C.c_double, C.c_char_p, C.c_char_p, P, P, U, P, U]),
        "dcp_prod_header": (C.c_char_p, []),
        "dcp_h3reader_open": (P, [C.c_char_p, I, F]),
        "dcp_h3reader_next": (I, [P, C.POINTER(P)]),
        "dcp_h3reader_error": (C.c_char_p, [P]),
        "dcp_h3reader_close": (None, [P]),
        "dcp_swissprot_null_lprobs": (None, [P]),
        "dcp_profile_consensus": (C.c_char_p, [P]),
        "dcp_db_write": (I, [C.c_char_p, P, U]),
        "dcp_db_open": (P, [C.c_char_p, C.POINTER(I)]),
        "dcp_db_close": (None, [P]),
        "dcp_db_nprofiles": (U, [P]),
        "dcp_db_entry_dist": (I, [P]),
        "dcp_db_epsilon": (F, [P]),
        "dcp_db_profile_sizes": (C.POINTER(C.c_uint32), [P]),
        "dcp_db_partitions": (U, [P, U, P, P]),
        "dcp_db_read": (I, [P, U, U, P]),
        "dcp_gpu_scan_cells": (C.c_uint64, [P]),
        "dcp_gpu_scan_algorithmic_bytes": (C.c_uint64, [P]),
        "dcp_profile_new64": (P, [C.c_char_p, U, I, C.c_double, P, P, P, C.c_char_p, C.POINTER(I)]),
        "dcp_profile_sample64": (P, [C.c_char_p, U, U, I, C.c_double, C.POINTER(I)]),
        "dcp_profile_precision": (I, [P]),
        "dcp_profile_epsilon64": (C.c_double, [P]),
        "dcp_profile_trans8_64": (P, [P]),
        "dcp_profile_null_dist64": (P, [P]),
        "dcp_profile_insert_dist64": (P, [P]),
        "dcp_profile_match_dist64": (P, [P]),
        "dcp_xtrans64": (I, [U, I, I, P]),
        "dcp_gpu_db_upload64": (I, [P, P, U]),
        "dcp_gpu_db_precision": (I, [P]),
        "dcp_gpu_set_lrt_threshold64": (I, [P, C.c_double]),
        "dcp_gpu_fetch_scores64": (I, [P, P, P]),
        "dcp_gpu_fetch_hits64": (I, [P, P, U, C.POINTER(U)]),
        "dcp_gpu_db_fetch_match_table64": (I, [P, U, P]),
        "dcp_gpu_db_fetch_insert_null64": (I, [P, U, P, P]),
        "dcp_gpu_trace_paths64": (I, [P, P, U, I, I, I, P, U, P, P]),
        "dcp_gpu_seqs_set_xtrans64": (I, [P, P, U]),
        "dcp_lprob_normalize64": (None, [U, P]),
        "dcp_profile_from_parts64": (P, [C.c_char_p, U, I, C.c_double, C.c_char_p, P, P, P, P, C.POINTER(I)]),
        "dcp_gpu_seqs_add_revcomp": (I, [P]),
        "dcp_gpu_seqs_strands": (U, [P]),
        "dcp_gpu_seqs_fetch": (I, [P, U, P, U, C.POINTER(U)]),
        "dcp_seq_revcomp": (None, [P, U, P]),
        "dcp_seq_window_count": (U, [U, U, U]),
        "dcp_seq_window_start": (U, [U, U, U, U]),
        "dcp_seq_window_plan": (I, [P, U, U, U, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "dcp_gpu_seqs_cut_windows": (I, [P, U, U]),
        "dcp_gpu_seqs_windows": (I, [P, C.POINTER(U), C.POINTER(U)]),
        "dcp_gpu_seqs_window_map": (I, [P, P, P, U]),
        "dcp_gpu_db_keep_dists": (I, [P, I]),
        "dcp_gpu_db_has_dists": (I, [P]),
        "dcp_gpu_decode_paths": (I, [P, P, P, U, P, P, P]),
        "dcp_profile_codon_joint": (I, [P, P, U, U, P, C.POINTER(C.c_double)]),
        "dcp_prod_format_row_codes": (C.c_long, [C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_char_p, C.c_char_p,
                                                 C.c_double, C.c_double, C.c_char_p, C.c_char_p, P, P, U, P, U, P]),
        "dcp_gpu_path_domains": (I, [P, P, P, U, P, P, I, I, P, U, P, P, P, P]),
        "dcp_gpu_path_domains64": (I, [P, P, P, U, P, P, I, I, P, U, P, P, P, P]),
        "dcp_gpu_path_domains_kernel_ms": (F, [P]),
        "dcp_domains_locate": (I, [P, P, U, P, U, U, P, P, P, P, P, P]),
        "dcp_gpu_domains_locate": (I, [P, P, P, U, P, P, P, P]),
        "dcp_domains_merge": (I, [P, P, P, P, P, P, U, P, C.POINTER(U)]),
        "dcp_domains_regions": (I, [P, P, P, P, P, U, P, U, C.c_uint64, C.c_uint32, P, P, P, P, P, P, P, U, C.POINTER(U)]),
        "dcp_domains_locate_regions": (I, [P, P, U, P, U, P, P, P, P, P, P, P]),
        "dcp_gpu_seqs_cut_regions": (I, [P, P, P, P, P, U]),
        "dcp_gpu_seqs_regions": (U, [P]),
        "dcp_gpu_seqs_region_map": (I, [P, P, P, P, U]),
        "dcp_gpu_scan_pairs": (I, [P, C.POINTER(ScanParams), P, P, U]),
        "dcp_seq_random_thresholds": (I, [P, P]),
        "dcp_seq_random": (None, [C.c_uint64, C.c_uint32, U, P, P]),
        "dcp_gpu_seqs_random": (I, [P, U, U, C.c_uint64, P]),
        "dcp_gumbel_fit": (I, [P, U, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dcp_gpu_fit_gumbel": (I, [P, P, P, P]),
        "dcp_gpu_db_calibrate": (I, [P, U, U, C.c_uint64, P, I, I, I, P, P, P]),
        "dcp_gpu_calib_kernel_ms": (F, [P, I]),
        "dcp_gumbel_fit_tail": (I, [P, U, C.c_size_t, U, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_uint)]),
        "dcp_gpu_fit_gumbel_tail": (I, [P, U, P, P, P, P, P]),
        "dcp_gpu_db_calibrate_tail": (I, [P, U, U, C.c_uint64, P, I, I, I, U, P, P, P, P, P]),
        "dcp_gpu_calib_tail_kernel_ms": (F, [P, I]),
        "dcp_gumbel_sf": (C.c_double, [C.c_double, C.c_double, C.c_double]),
        "dcp_hits_evalues": (I, [P, U, P, P, P, U, C.c_double, P]),
        "dcp_hits_evalues64": (I, [P, U, P, P, P, U, C.c_double, P]),
        "dcp_forward_tables": (I, [U, U, P, P, P, P, P, P, U, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dcp_gpu_forward_pairs": (I, [P, I, I, P, P, U, P, P]),
        "dcp_gpu_forward_kernel_ms": (F, [P]),
        "dcp_posterior_tables": (I, [U, U, P, P, P, P, P, P, U, P, P, P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dcp_posterior_envelopes": (I, [P, U, C.c_double, U, P, P, U, C.POINTER(U)]),
        "dcp_posterior_envelope_records": (I, [P, P, P, U, C.c_double, C.c_double, U, P, U, C.POINTER(U)]),
        "dcp_gpu_envelope_pairs": (I, [P, I, I, I, P, P, U, C.c_double, C.c_double, U, P, C.c_uint64, P, P, P]),
        "dcp_gpu_envelope_kernel_ms": (F, [P]),
        "dcp_envelopes_regions": (I, [P, C.c_uint64, P, U, P, U, U, P, P, P, P]),
        "dcp_gpu_posterior_pairs": (I, [P, I, I, P, P, U, P, P, P, P, C.c_uint64, P, P]),
        "dcp_gpu_posterior_kernel_ms": (F, [P]),
        "dcp_mea_tables": (I, [U, U, P, P, P, P, P, P, U, P, U, C.POINTER(U), P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dcp_mea_path_gain": (I, [U, U, P, P, P, P, P, P, U, P, U, C.POINTER(C.c_double), P]),
        "dcp_gpu_mea_pairs": (I, [P, I, I, P, P, U, P, U, P, P, P, P]),
        "dcp_gpu_mea_kernel_ms": (F, [P]),
        "dcp_gpu_forward_dense": (I, [P, I, I]),
        "dcp_fwd_factor_f32": (C.c_double, [C.c_float]),
        "dcp_forward_scaled_tables": (I, [U, U, P, P, P, P, P, P, U, I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(I)]),
        "dcp_forward_scaled_tables_band": (I, [U, U, P, P, P, P, P, P, U, I, I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(I)]),
        "dcp_gpu_forward_pairs_scaled": (I, [P, I, I, P, P, U, P, P]),
        "dcp_gpu_forward_scaled_redo_pairs": (U, [P]),
        "dcp_gpu_forward_scaled_kernel_ms": (F, [P]),
        "dcp_gpu_forward_dense_scaled": (I, [P, I, I]),
        "dcp_gpu_forward_dense_is_scaled": (I, [P]),
        "dcp_posterior_scaled_tables": (I, [U, U, P, P, P, P, P, P, U, I, P, P, P, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int)]),
        "dcp_posterior_scaled_tables_band": (I, [U, U, P, P, P, P, P, P, U, I, I, P, P, P, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "dcp_gpu_posterior_pairs_scaled": (I, [P, I, I, P, P, U, P, P, P, P, C.c_uint64, P, P]),
        "dcp_gpu_posterior_scaled_redo_pairs": (U, [P]),
        "dcp_gpu_posterior_scaled_kernel_ms": (F, [P]),
        "dcp_gpu_fetch_forward_scores": (I, [P, P, P]),
        "dcp_gpu_forward_dense_kernel_ms": (F, [P]),
        "dcp_exp_tail_fit": (I, [P, U, C.c_size_t, U, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_uint)]),
        "dcp_gpu_fit_exp_tail": (I, [P, I, U, P, P, P, P, P]),
        "dcp_gpu_exp_tail_kernel_ms": (F, [P, I]),
        "dcp_gpu_db_calibrate_forward": (I, [P, U, U, C.c_uint64, P, I, I, U, P, P, P, P, P]),
        "dcp_exp_sf": (C.c_double, [C.c_double, C.c_double, C.c_double]),
        "dcp_scores_evalues": (I, [P, P, P, U, P, P, P, U, C.c_double, I, P]),
    }
    if hooks:
        sig["dcp_gpu_test_set_redo_cap"] = (I, [P, U])
        sig["dcp_gpu_test_set_rowsweep_variant"] = (I, [P, I, U])
        sig["dcp_gpu_test_set_ring_stall"] = (I, [P, I])
        sig["dcp_gpu_test_set_seg_col_bytes"] = (I, [P, C.c_ulonglong])
        sig["dcp_gpu_test_set_trace_mode"] = (I, [P, I, C.c_ulonglong])
        sig["dcp_gpu_test_fetch_table_span"] = (I, [P, U, P, C.c_ulonglong, C.POINTER(U), C.POINTER(U), C.POINTER(U)])
        sig["dcp_gpu_test_fetch_seq_words"] = (I, [P, U, P, U, C.POINTER(U)])
        sig["dcp_gpu_test_last_rowsweep_plan"] = (I, [P, P, U, C.POINTER(U)])
        sig["dcp_gpu_test_last_pair_launches"] = (I, [P, P, U, C.POINTER(U)])
        sig["dcp_gpu_test_set_forward_waves"] = (I, [P, U])
        sig["dcp_gpu_test_set_dense_round"] = (I, [P, U])
        sig["dcp_gpu_test_set_forward_scale_band"] = (I, [P, U])
        sig["dcp_gpu_test_set_posterior_budget"] = (I, [P, C.c_ulonglong])
        sig["dcp_gpu_test_set_mea_budget"] = (I, [P, C.c_ulonglong])
        sig["dcp_gpu_test_envelope_records_kernel_ms"] = (F, [P])
        sig["dcp_gpu_test_envelopes_of_rows"] = (I, [P, P, P, P, P, U, C.c_double, C.c_double, U, P, C.c_uint64, P])
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
TESTHOOKS_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libdcp_hip_testhooks.so")


def load_testhooks():
    """TESTS ONLY: the -DDCP_TEST_HOOKS build of the same sources (csrc/Makefile), which adds
    dcp_gpu_test_set_redo_cap.  `Scanner(device, lib=load_testhooks())` runs a context of that build."""
    return _load(TESTHOOKS_LIB_PATH, hooks=True)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class ProteinCfg:
    """struct protein_cfg {entry_dist, epsilon} (include/deciphon/model/protein_cfg.h)."""

    def __init__(self, entry_dist=ENTRY_DIST_OCCUPANCY, epsilon=0.01):
        if not (0.0 <= epsilon <= 1.0):  # assert in protein_cfg():18
            raise DcpError(RC_EINVAL, "epsilon out of [0, 1]")
        self.entry_dist = entry_dist
        self.epsilon = float(np.float32(epsilon))
        self.epsilon64 = float(epsilon)  # what the double build takes (dcp_profile_sample64 / new64)


PROTEIN_CFG_DEFAULT = ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)  # protein_cfg.h:22-23


class ProteinProfile:
    """The scan-time profile object (struct protein_profile, protein_profile.h:12-43) in its
    compact device-facing form: 8 transition rows + one 129-float nuclt_dist per node."""

    def __init__(self, handle):
        if not handle:
            raise DcpError(RC_EINVAL, "profile construction failed")
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.dcp_profile_del(h)

    @classmethod
    def sample(cls, seed, core_size, cfg=PROTEIN_CFG_DEFAULT, accession="accession", precision=32):
        """protein_profile_sample (src/model/protein_profile.c:259-304).  precision=64: the reference's
        IMM_DOUBLE_PRECISION build (dcp_profile_sample64), whose epsilon is cfg's value in double."""
        rc = C.c_int(0)
        if precision == 64:
            h = lib.dcp_profile_sample64(accession.encode(), seed, core_size, cfg.entry_dist,
                                         cfg.epsilon64, C.byref(rc))
        elif precision == 32:
            h = lib.dcp_profile_sample(accession.encode(), seed, core_size, cfg.entry_dist,
                                       cfg.epsilon, C.byref(rc))
        else:
            raise DcpError(RC_EINVAL, "precision is 32 or 64")
        if not h:
            raise DcpError(rc.value, "protein_profile_sample")
        return cls(h)

    @classmethod
    def from_params(cls, null_lprobs, match_lprobs, trans, cfg=PROTEIN_CFG_DEFAULT,
                    accession="accession", consensus=None, precision=32):
        """protein_model_init/setup/add_node/add_trans + protein_profile_absorb.  precision=64: built in
        double from double parameters (dcp_profile_new64)."""
        if precision not in (32, 64):
            raise DcpError(RC_EINVAL, "precision is 32 or 64")
        cv = _f64 if precision == 64 else _f32
        nl, ml, tr = cv(null_lprobs), cv(match_lprobs), cv(trans)
        M = ml.shape[0] if ml.ndim == 2 else 0
        if nl.shape != (20,) or ml.shape != (M, 20) or tr.shape != (M + 1, 7):
            raise DcpError(RC_EINVAL, "bad parameter shapes")
        rc = C.c_int(0)
        cons = consensus.encode() if consensus else None
        new, eps = (lib.dcp_profile_new64, cfg.epsilon64) if precision == 64 else (lib.dcp_profile_new, cfg.epsilon)
        h = new(accession.encode(), M, cfg.entry_dist, eps, nl.ctypes.data, ml.ctypes.data, tr.ctypes.data, cons,
                C.byref(rc))
        if not h:
            raise DcpError(rc.value, "protein_model_setup")
        return cls(h)

    @property
    def core_size(self):
        return lib.dcp_profile_core_size(self._h)

    @property
    def precision(self):
        """64 for a profile of the double build, else 32."""
        return lib.dcp_profile_precision(self._h)

    def decode(self, frag, state_id):
        """protein_profile_decode (src/model/protein_profile.c:306-331): most likely codon of a
        1..5-nt fragment emitted by `state_id`, as an ACGT string. RC_EINVAL for mute states."""
        f = encode_seq(frag) if isinstance(frag, str) else np.ascontiguousarray(frag, np.uint8)
        out = np.zeros(3, np.uint8)
        rc = lib.dcp_profile_decode(self._h, f.ctypes.data, len(f), int(state_id), out.ctypes.data)
        if rc:
            raise DcpError(rc, "failed to decode sequence")
        return "".join("ACGT"[b] for b in out)

    def codon_joint(self, frag, state_id, codon):
        """p(fragment, codon) of ONE codon (dcp_profile_codon_joint): the quantity decode() maximises over the 64
        codons, by the same arithmetic.  codon: an ACGT string, three ids, or its code 16a + 4b + c."""
        f = encode_seq(frag) if isinstance(frag, str) else np.ascontiguousarray(frag, np.uint8)
        if isinstance(codon, str):
            cd = encode_seq(codon)
        elif np.ndim(codon) == 0:
            cd = np.array([int(codon) >> 4, (int(codon) >> 2) & 3, int(codon) & 3], np.uint8)
        else:
            cd = np.ascontiguousarray(codon, np.uint8)
        if len(cd) != 3:
            raise DcpError(RC_EINVAL, "a codon has three bases")
        out = C.c_double(0.0)
        rc = lib.dcp_profile_codon_joint(self._h, f.ctypes.data, len(f), int(state_id), cd.ctypes.data, C.byref(out))
        if rc:
            raise DcpError(rc, "no joint for this fragment, state and codon")
        return out.value

    def prod_row(self, seq, steps, scan_id=0, seq_id=0, alt_loglik=0.0, null_loglik=0.0,
                 abc_name="dna", profile_typeid="protein", version="0.0.0", profile_name=None, codes=None):
        """One product TSV row as prod_fwrite + protein_match_write_func write it
        (src/server/prod.c:153-181, src/server/protein_match.c:21-56).  codes: one code per step as
        Scanner.decode_paths returns them (dcp_prod_format_row_codes) instead of decoding here."""
        s = encode_seq(seq) if isinstance(seq, str) else np.ascontiguousarray(seq, np.uint8)
        st = np.ascontiguousarray(steps, STEP_DTYPE)
        cap = 256 + 64 * (len(st) + 1) + 2 * len(s)
        buf = C.create_string_buffer(cap)
        args = (buf, cap, scan_id, seq_id, (profile_name or self.accession).encode(),
                abc_name.encode(), float(alt_loglik), float(null_loglik),
                profile_typeid.encode(), version.encode(), self._h, s.ctypes.data,
                len(s), st.ctypes.data, len(st))
        if codes is None:
            n = lib.dcp_prod_format_row(*args)
        else:
            cd = np.ascontiguousarray(codes, np.uint8)
            # a wrong number of codes fails like any other row that cannot be written
            n = lib.dcp_prod_format_row_codes(*args, cd.ctypes.data) if cd.shape == (len(st),) else -1
        if n < 0:
            raise DcpError(RC_EFAIL, "failed to write prod")
        return buf.raw[:n].decode()

    @property
    def accession(self):
        return lib.dcp_profile_accession(self._h).decode()

    def _view(self, ptr, shape, ctype=C.c_float):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).reshape(shape).copy()

    def parts64(self):
        """The double build's scan-time parts (trans8 [8, M], null [129], insert [129], match [M, 129]) in
        float64; RC_EINVAL for a float profile."""
        if self.precision != 64:
            raise DcpError(RC_EINVAL, "a float profile has no double parts")
        M, d = self.core_size, C.c_double
        return (self._view(lib.dcp_profile_trans8_64(self._h), (8, M), d),
                self._view(lib.dcp_profile_null_dist64(self._h), (NDIST,), d),
                self._view(lib.dcp_profile_insert_dist64(self._h), (NDIST,), d),
                self._view(lib.dcp_profile_match_dist64(self._h), (M, NDIST), d))

    @classmethod
    def from_parts64(cls, trans8, null_dist, insert_dist, match_dist, cfg=PROTEIN_CFG_DEFAULT,
                     accession="accession", consensus=None):
        """A double profile from stored double parts (dcp_profile_from_parts64): what parts64() returns."""
        t8, nd, idist, md = _f64(trans8), _f64(null_dist), _f64(insert_dist), _f64(match_dist)
        M = t8.shape[1] if t8.ndim == 2 else 0
        if t8.shape != (8, M) or nd.shape != (NDIST,) or idist.shape != (NDIST,) or md.shape != (M, NDIST):
            raise DcpError(RC_EINVAL, "bad part shapes")
        rc = C.c_int(0)
        h = lib.dcp_profile_from_parts64(accession.encode(), M, cfg.entry_dist, cfg.epsilon64,
                                         consensus.encode() if consensus else None, t8.ctypes.data, nd.ctypes.data,
                                         idist.ctypes.data, md.ctypes.data, C.byref(rc))
        if not h:
            raise DcpError(rc.value, "dcp_profile_from_parts64")
        return cls(h)

    @property
    def epsilon64(self):
        return lib.dcp_profile_epsilon64(self._h)

    @property
    def consensus(self):
        return lib.dcp_profile_consensus(self._h).decode()

    @property
    def trans8(self):
        return self._view(lib.dcp_profile_trans8(self._h), (8, self.core_size))

    @property
    def null_dist(self):
        return self._view(lib.dcp_profile_null_dist(self._h), (NDIST,))

    @property
    def insert_dist(self):
        return self._view(lib.dcp_profile_insert_dist(self._h), (NDIST,))

    @property
    def match_dist(self):
        return self._view(lib.dcp_profile_match_dist(self._h), (self.core_size, NDIST))


def state_name(state_id):
    """protein_state_name (src/model/protein_state.c:5-39)."""
    b = C.create_string_buffer(8)
    lib.dcp_state_name(int(state_id), b)
    return b.value.decode()


def gc_decode(codon):
    """imm_gc_decode(1, codon): amino acid letter of an ACGT codon string."""
    c = encode_seq(codon)
    return lib.dcp_gc_decode(c.ctypes.data).decode()


PROD_HEADER = lib.dcp_prod_header().decode()


def swissprot_null_lprobs():
    """Swiss-Prot 50.8 background (src/model/protein_h3reader.c:79-103), log-probabilities."""
    out = np.zeros(20, np.float32)
    lib.dcp_swissprot_null_lprobs(out.ctypes.data)
    return out


def read_hmmer3(path, cfg=PROTEIN_CFG_DEFAULT):
    """All profiles of a HMMER3 ASCII file: protein_h3reader_next + protein_profile_absorb per
    profile, as hmm_press does (src/server/hmm.c:120-178)."""
    r = lib.dcp_h3reader_open(str(path).encode(), cfg.entry_dist, cfg.epsilon)
    if not r:
        raise DcpError(RC_EIO, f"failed to open {path}")
    out = []
    try:
        while True:
            h = C.c_void_p()
            rc = lib.dcp_h3reader_next(r, C.byref(h))
            if rc == RC_END:
                return out
            if rc:
                raise DcpError(rc, lib.dcp_h3reader_error(r).decode())
            out.append(ProteinProfile(h.value))
    finally:
        lib.dcp_h3reader_close(r)


def write_db(path, profiles):
    """Write a dcpx profile DB (the press output: protein_db_writer_pack_profile per profile)."""
    arr = (C.c_void_p * len(profiles))(*[p._h for p in profiles])
    rc = lib.dcp_db_write(str(path).encode(), arr, len(profiles))
    if rc:
        raise DcpError(rc, f"failed to write {path}")


class ProfileDB:
    """protein_db_reader + profile_reader over a dcpx file: header fields, per-profile byte sizes,
    the reference's partition table, and reading a range of profiles."""

    def __init__(self, path):
        rc = C.c_int(0)
        self._h = lib.dcp_db_open(str(path).encode(), C.byref(rc))
        if not self._h:
            raise DcpError(rc.value, f"failed to open {path}")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.dcp_db_close(h)

    __del__ = close

    @property
    def nprofiles(self):
        return lib.dcp_db_nprofiles(self._h)

    @property
    def cfg(self):
        return ProteinCfg(lib.dcp_db_entry_dist(self._h), lib.dcp_db_epsilon(self._h))

    @property
    def profile_sizes(self):
        return np.ctypeslib.as_array(lib.dcp_db_profile_sizes(self._h), shape=(self.nprofiles,)).copy()

    def partitions(self, npartitions):
        """(partition_size[npart], partition_offset[npart + 1]) as profile_reader_setup computes them."""
        sizes = np.zeros(NUM_THREADS, np.uint32)
        offs = np.zeros(NUM_THREADS + 1, np.int64)
        n = lib.dcp_db_partitions(self._h, npartitions, sizes.ctypes.data, offs.ctypes.data)
        if n == 0:
            raise DcpError(RC_EINVAL, "can't have zero partitions / too many partitions")
        return sizes[:n].tolist(), offs[:n + 1].tolist()

    def read(self, begin=0, end=None):
        end = self.nprofiles if end is None else end
        out = (C.c_void_p * max(end - begin, 1))()
        rc = lib.dcp_db_read(self._h, begin, end, out)
        profs = [ProteinProfile(h) for h in out[:end - begin] if h]
        if rc:
            raise DcpError(rc, "failed to read profiles")
        return profs


def frame_table_host(dist, epsilon):
    d = _f32(dist)
    out = np.zeros(NCODES, np.float32)
    lib.dcp_frame_table_host(d.ctypes.data, float(np.float32(epsilon)), out.ctypes.data)
    return out


def xtrans(seq_size, multi_hits=True, hmmer3_compat=False):
    """protein_profile_setup's 13 special transitions (protein_profile.c:155-216).
    Raises RC_EINVAL for an empty sequence, as the reference returns."""
    out = np.zeros(NXTRANS, np.float32)
    rc = lib.dcp_xtrans(seq_size, int(multi_hits), int(hmmer3_compat), out.ctypes.data)
    if rc:
        raise DcpError(rc, "sequence cannot be empty")
    return out


def xtrans64(seq_size, multi_hits=True, hmmer3_compat=False):
    """The same 13 special transitions in double (dcp_xtrans64)."""
    out = np.zeros(NXTRANS, np.float64)
    rc = lib.dcp_xtrans64(seq_size, int(multi_hits), int(hmmer3_compat), out.ctypes.data)
    if rc:
        raise DcpError(rc, "sequence cannot be empty")
    return out


def forward_tables(t8, em, ei, en, xt, seq):
    """(null, alt) Forward scores of one sequence against one profile on the host (dcp_forward_tables): the scan's
    recursion with every max replaced by log-sum-exp, in double.  t8 [8, ldk], em [1364, ldk], ei [1364], en [1364],
    xt [13], seq base ids 0..3; the arrays are converted to float64, so float tables go in as they are."""
    t8, em, ei, en, xt = _f64(t8), _f64(em), _f64(ei), _f64(en), _f64(xt)
    seq = np.ascontiguousarray(seq, np.uint8)
    if t8.ndim != 2 or em.ndim != 2 or t8.shape != (8, em.shape[1]) or em.shape[0] != NCODES or \
            ei.shape != (NCODES,) or en.shape != (NCODES,) or xt.shape != (NXTRANS,) or seq.ndim != 1:
        raise DcpError(RC_EINVAL, "tables of shapes [8, ldk], [1364, ldk], [1364], [1364], [13]")
    null, alt = C.c_double(0.0), C.c_double(0.0)
    rc = lib.dcp_forward_tables(em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data,
                                xt.ctypes.data, seq.ctypes.data, len(seq), C.byref(null), C.byref(alt))
    if rc:
        raise DcpError(rc, "dcp_forward_tables")
    return null.value, alt.value


def fwd_factor_f32(t):
    """exp(t) of the float32 t as the scaled Forward sweeps form it on a float DB (dcp_fwd_factor_f32): float
    arithmetic alone, the same bits on host and device.  0 below -708 and for -inf, +inf above 708."""
    return lib.dcp_fwd_factor_f32(float(np.float32(t)))


def forward_scaled_tables(t8, em, ei, en, xt, seq, float_factors=False, band=None):
    """(null, alt, out_of_range) of one sequence against one profile by the scaled probability-space Forward on the
    host (dcp_forward_scaled_tables): forward_tables' arguments; float_factors applies the float DB's factor rule to
    float32(t) of every table value, else exp(t) in double.  out_of_range: a value left the double range and the two
    scores are None.  band (tests): the rescaling rule's band in bits, which the scores do not depend on."""
    t8, em, ei, en, xt = _f64(t8), _f64(em), _f64(ei), _f64(en), _f64(xt)
    seq = np.ascontiguousarray(seq, np.uint8)
    if t8.ndim != 2 or em.ndim != 2 or t8.shape != (8, em.shape[1]) or em.shape[0] != NCODES or \
            ei.shape != (NCODES,) or en.shape != (NCODES,) or xt.shape != (NXTRANS,) or seq.ndim != 1:
        raise DcpError(RC_EINVAL, "tables of shapes [8, ldk], [1364, ldk], [1364], [1364], [13]")
    null, alt, oor = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    args = (em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data, xt.ctypes.data,
            seq.ctypes.data, len(seq), int(bool(float_factors)))
    outs = (C.byref(null), C.byref(alt), C.byref(oor))
    rc = lib.dcp_forward_scaled_tables(*args, *outs) if band is None else lib.dcp_forward_scaled_tables_band(*args, int(band), *outs)
    if rc:
        raise DcpError(rc, "dcp_forward_scaled_tables")
    if oor.value:
        return None, None, True
    return null.value, alt.value, False


def posterior_tables(t8, em, ei, en, xt, seq):
    """(begin, end, core, alt_fwd, alt_bwd) of one sequence against one profile on the host (dcp_posterior_tables):
    three float64 rows of len(seq) + 1 -- the posteriors that a domain begins at row j, that one ends there, and that
    base j - 1 is emitted by a core state -- and the alt score by the Forward and by the Backward sweep.  The tables
    are forward_tables' ones."""
    t8, em, ei, en, xt = _f64(t8), _f64(em), _f64(ei), _f64(en), _f64(xt)
    seq = np.ascontiguousarray(seq, np.uint8)
    if t8.ndim != 2 or em.ndim != 2 or t8.shape != (8, em.shape[1]) or em.shape[0] != NCODES or \
            ei.shape != (NCODES,) or en.shape != (NCODES,) or xt.shape != (NXTRANS,) or seq.ndim != 1:
        raise DcpError(RC_EINVAL, "tables of shapes [8, ldk], [1364, ldk], [1364], [1364], [13]")
    begin, end, core = (np.zeros(len(seq) + 1, np.float64) for _ in range(3))
    fwd, bwd = C.c_double(0.0), C.c_double(0.0)
    rc = lib.dcp_posterior_tables(em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data,
                                  xt.ctypes.data, seq.ctypes.data, len(seq), begin.ctypes.data, end.ctypes.data,
                                  core.ctypes.data, C.byref(fwd), C.byref(bwd))
    if rc:
        raise DcpError(rc, "dcp_posterior_tables")
    return begin, end, core, fwd.value, bwd.value


def posterior_scaled_tables(t8, em, ei, en, xt, seq, float_factors=False, band=None):
    """(begin, end, core, alt_fwd, alt_bwd, out_of_range) of one sequence against one profile by the scaled
    probability-space sweeps on the host (dcp_posterior_scaled_tables): posterior_tables' arguments and rows;
    float_factors as forward_scaled_tables.  out_of_range: a value left the double range, or a row's records may have
    lost a term that matters to underflow, and the five results are None.  band (tests): the rescaling rule's band in
    bits, which the results of a pair in range do not depend on."""
    t8, em, ei, en, xt = _f64(t8), _f64(em), _f64(ei), _f64(en), _f64(xt)
    seq = np.ascontiguousarray(seq, np.uint8)
    if t8.ndim != 2 or em.ndim != 2 or t8.shape != (8, em.shape[1]) or em.shape[0] != NCODES or \
            ei.shape != (NCODES,) or en.shape != (NCODES,) or xt.shape != (NXTRANS,) or seq.ndim != 1:
        raise DcpError(RC_EINVAL, "tables of shapes [8, ldk], [1364, ldk], [1364], [1364], [13]")
    begin, end, core = (np.zeros(len(seq) + 1, np.float64) for _ in range(3))
    fwd, bwd, oor = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    args = (em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data, xt.ctypes.data,
            seq.ctypes.data, len(seq), int(bool(float_factors)))
    outs = (begin.ctypes.data, end.ctypes.data, core.ctypes.data, C.byref(fwd), C.byref(bwd), C.byref(oor))
    rc = lib.dcp_posterior_scaled_tables(*args, *outs) if band is None else \
        lib.dcp_posterior_scaled_tables_band(*args, int(band), *outs)
    if rc:
        raise DcpError(rc, "dcp_posterior_scaled_tables")
    if oor.value:
        return None, None, None, None, None, True
    return begin, end, core, fwd.value, bwd.value, False


def _mea_tables_args(t8, em, ei, en, xt, seq):
    t8, em, ei, en, xt = _f64(t8), _f64(em), _f64(ei), _f64(en), _f64(xt)
    seq = np.ascontiguousarray(seq, np.uint8)
    if t8.ndim != 2 or em.ndim != 2 or t8.shape != (8, em.shape[1]) or em.shape[0] != NCODES or \
            ei.shape != (NCODES,) or en.shape != (NCODES,) or xt.shape != (NXTRANS,) or seq.ndim != 1:
        raise DcpError(RC_EINVAL, "tables of shapes [8, ldk], [1364, ldk], [1364], [1364], [13]")
    return t8, em, ei, en, xt, seq


def mea_tables(t8, em, ei, en, xt, seq):
    """(steps, post, gain, alt_fwd) of one sequence against one profile on the host (dcp_mea_tables): the
    posterior-decoded path -- the S .. T path over finite transitions and emissions that emits len(seq) bases and has
    the largest sum of seqlen x word posterior over its emitting steps -- as a STEP_DTYPE array in trace_paths' format,
    the word posterior of every step (-1 for a step that emits nothing), that sum, and the Forward alt score.  No path
    at all (alt_fwd = -inf): zero steps and gain -inf.  The tables are forward_tables' ones."""
    t8, em, ei, en, xt, seq = _mea_tables_args(t8, em, ei, en, xt, seq)
    n, gain, fwd = C.c_uint(0), C.c_double(0.0), C.c_double(0.0)
    cap = 2 * len(seq) + 2 * em.shape[1] + 16
    for _ in range(2):  # a longer path is walked once more at its exact count
        steps, post = np.zeros(max(cap, 1), STEP_DTYPE), np.zeros(max(cap, 1), np.float64)
        rc = lib.dcp_mea_tables(em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data,
                                xt.ctypes.data, seq.ctypes.data, len(seq), steps.ctypes.data, cap, C.byref(n),
                                post.ctypes.data, C.byref(gain), C.byref(fwd))
        if rc != RC_ENOMEM or n.value <= cap:
            break
        cap = n.value
    if rc:
        raise DcpError(rc, "dcp_mea_tables")
    return steps[:n.value].copy(), post[:n.value].copy(), gain.value, fwd.value


def mea_path_gain(t8, em, ei, en, xt, seq, steps):
    """(gain, post) of a given alt path of one sequence against one profile on the host (dcp_mea_path_gain): the sum
    of seqlen x word posterior over its emitting steps under mea_tables' own sweeps, and every step's word posterior
    (-1 for a step that emits nothing).  DcpError(EINVAL): the path is not S .. T, uses an edge that is not in the
    graph or a transition or emission that is -inf, names a node outside 1 .. M, or does not emit len(seq) bases."""
    t8, em, ei, en, xt, seq = _mea_tables_args(t8, em, ei, en, xt, seq)
    st = np.ascontiguousarray(steps, STEP_DTYPE)
    if st.ndim != 1:
        raise DcpError(RC_EINVAL, "one array of steps")
    gain, post = C.c_double(0.0), np.zeros(max(len(st), 1), np.float64)
    rc = lib.dcp_mea_path_gain(em.shape[1], em.shape[1], t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data,
                               xt.ctypes.data, seq.ctypes.data, len(seq), st.ctypes.data if len(st) else None, len(st),
                               C.byref(gain), post.ctypes.data)
    if rc:
        raise DcpError(rc, "dcp_mea_path_gain")
    return gain.value, post[:len(st)]


def posterior_envelopes(core, threshold=0.5, min_len=1):
    """[(begin, end), ..]: the maximal runs of bases whose core posterior is at least `threshold` and that are at least
    min_len bases long, as half-open base intervals in order (dcp_posterior_envelopes).  core is a row of
    posterior_tables / Scanner.posterior_pairs: len(seq) + 1 values, base i at core[i + 1]."""
    core = _f64(core)
    if core.ndim != 1 or len(core) == 0 or not 0 <= min_len < 2 ** 32:
        raise DcpError(RC_EINVAL, "a core row of L + 1 values; min_len in 32 bits")
    L, n = len(core) - 1, C.c_uint(0)
    rc = lib.dcp_posterior_envelopes(core.ctypes.data, L, float(threshold), int(min_len), None, None, 0, C.byref(n))
    if rc:
        raise DcpError(rc, "dcp_posterior_envelopes")
    b, e = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
    rc = lib.dcp_posterior_envelopes(core.ctypes.data, L, float(threshold), int(min_len), b.ctypes.data, e.ctypes.data,
                                     n.value, C.byref(n))
    if rc:
        raise DcpError(rc, "dcp_posterior_envelopes")
    return [(int(x), int(y)) for x, y in zip(b, e)]


def posterior_envelope_records(begin, end, core, hi=0.5, lo=None, min_len=1):
    """The envelopes of one pair's posterior rows as ENVELOPE_DTYPE records, in order (dcp_posterior_envelope_records,
    the host twin of Scanner.envelope_pairs): the maximal runs of bases with core >= lo (lo=None: hi) that are at least
    min_len bases long and reach hi somewhere; per run its interval, the first base where core is largest and that
    value, and the sums of core, begin and end over it -- the expected numbers of core-emitted bases, domain starts and
    domain ends.  begin, end, core are rows of posterior_tables / posterior_pairs (L + 1 values, base i at core[i + 1]);
    pair is 0."""
    begin, end, core = _f64(begin), _f64(end), _f64(core)
    if not len(begin) == len(end) == len(core):
        raise DcpError(RC_EINVAL, "rows of one length")
    L = max(len(core) - 1, 0)
    lo = hi if lo is None else lo
    n = C.c_uint(0)
    rc = lib.dcp_posterior_envelope_records(begin.ctypes.data, end.ctypes.data, core.ctypes.data, L, float(hi), float(lo),
                                            int(min_len), None, 0, C.byref(n))
    if rc != RC_OK:
        raise DcpError(rc, "dcp_posterior_envelope_records")
    out = np.zeros(n.value, ENVELOPE_DTYPE)
    rc = lib.dcp_posterior_envelope_records(begin.ctypes.data, end.ctypes.data, core.ctypes.data, L, float(hi), float(lo),
                                            int(min_len), out.ctypes.data, n.value, C.byref(n))
    if rc != RC_OK:
        raise DcpError(rc, "dcp_posterior_envelope_records")
    return out


def envelopes_regions(env, seq_idx, seq_len, flank=0):
    """(src, begin, length, profile_pair) for Scanner.cut_regions from ENVELOPE_DTYPE records (dcp_envelopes_regions):
    envelope k becomes the stretch [max(begin - flank, 0), min(end + flank, L)) of resident sequence
    seq_idx[env[k].pair], L = seq_len[that sequence]; profile_pair[k] = env[k].pair names the list entry whose profile
    the region is to be scored against.  seq_idx is the list envelope_pairs was given, seq_len the resident
    sequences' lengths."""
    env = np.ascontiguousarray(env, ENVELOPE_DTYPE)
    sq = np.ascontiguousarray(np.atleast_1d(seq_idx), np.uint32)
    sl = np.ascontiguousarray(np.atleast_1d(seq_len), np.uint32)
    n = len(env)
    src, begin, length, pair = (np.zeros(n, np.uint32) for _ in range(4))
    rc = lib.dcp_envelopes_regions(env.ctypes.data, n, sq.ctypes.data, len(sq), sl.ctypes.data, len(sl), int(flank),
                                   src.ctypes.data, begin.ctypes.data, length.ctypes.data, pair.ctypes.data)
    if rc != RC_OK:
        raise DcpError(rc, "dcp_envelopes_regions")
    return src, begin, length, pair


def lrt(null_loglik, alt_loglik):
    """xmath_lrt_f32 (include/deciphon/core/xmath.h:32-35)."""
    return lib.dcp_lrt(float(null_loglik), float(alt_loglik))


def partition_by_count(nprofiles, npartitions):
    """profile_reader partition sizes (src/db/profile_reader.c:54-72)."""
    sizes = np.zeros(NUM_THREADS, np.uint32)
    n = lib.dcp_partition_by_count(nprofiles, npartitions, sizes.ctypes.data)
    if n == 0:
        raise DcpError(RC_EINVAL, "can't have zero partitions / too many partitions")
    return sizes[:n].tolist()


def partition_by_cells(core_sizes, npartitions):
    """Contiguous shards balanced by sum of core sizes: one per GPU."""
    cs = np.ascontiguousarray(core_sizes, np.uint32)
    out = np.zeros(npartitions + 1, np.uint32)
    lib.dcp_partition_by_cells(cs.ctypes.data, len(cs), npartitions, out.ctypes.data)
    return out.tolist()


def encode_seq(text):
    """ACGT text -> symbol ids (imm_dna_iupac order); anything else -> 255."""
    lut = np.full(256, 255, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    return lut[np.frombuffer(text.encode() if isinstance(text, str) else text, np.uint8)]


def revcomp(ids):
    """The reverse complement of symbol ids 0..3 (A C G T): out[i] = 3 - ids[n - 1 - i] (dcp_seq_revcomp), the map
    Scanner.add_reverse_strand applies on the device."""
    ids = np.frombuffer(ids, np.uint8) if isinstance(ids, (bytes, bytearray)) else np.ascontiguousarray(ids, np.uint8)
    out = np.empty_like(ids)
    lib.dcp_seq_revcomp(ids.ctypes.data, len(ids), out.ctypes.data)
    return out


def _window_rule(window, step):
    if not (1 <= window < 2 ** 32 and 1 <= step <= window):
        raise DcpError(RC_EINVAL, f"bad window rule (window {window}, step {step}): window >= 1 and 1 <= step <= window")


def window_count(L, window, step):
    """Windows of a sequence of L bases (dcp_seq_window_count): 1 if L <= window, else 1 + ceil((L - window) / step)."""
    _window_rule(window, step)
    return lib.dcp_seq_window_count(L, window, step)


def window_starts(L, window, step):
    """First bases of the windows Scanner.cut_windows(window, step) cuts a sequence of L bases into
    (dcp_seq_window_start): i * step, the last one anchored at L - window; [0] if L <= window.  A uint32 array."""
    n = window_count(L, window, step)
    return np.array([lib.dcp_seq_window_start(L, window, step, i) for i in range(n)], np.uint32)


def window_plan(lens, window, step):
    """(windows, words) of a batch with these lengths, cut by the rule (dcp_seq_window_plan): the totals as Python
    ints; DcpError(RC_EINVAL) for a bad rule or when either passes 2^32 - 1 -- the refusal of Scanner.cut_windows."""
    lens = np.ascontiguousarray(lens, np.uint32)
    nwin, nwords = C.c_uint64(0), C.c_uint64(0)
    rc = lib.dcp_seq_window_plan(lens.ctypes.data, len(lens), min(window, 2 ** 32 - 1) if window >= 0 else 0,
                                 min(step, 2 ** 32 - 1) if step >= 0 else 0, C.byref(nwin), C.byref(nwords))
    if rc:
        raise DcpError(rc, f"window plan refused: {nwin.value} windows, {nwords.value} words")
    return nwin.value, nwords.value


def _locate_outputs(n):
    return np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)


def locate_domains(res_idx, domains, res_len, per_strand, strands=1, win_src=None, win_off=None):
    """Where domains lie on their sources (dcp_domains_locate): (src uint32, begin uint64, end uint64, minus uint8).
    res_idx[j]: the resident sequence domain j was found on (its hit's seq_idx); res_len: the resident lengths, strands
    x per_strand of them; win_src / win_off: the window map of a cut batch (Scanner.window_map), None if uncut.  On the
    minus strand [seq_begin, seq_end) becomes [len - seq_end, len - seq_begin) before the window's offset is added."""
    res = np.ascontiguousarray(res_idx, np.uint32)
    dom = np.ascontiguousarray(domains, DOMAIN_DTYPE)
    if len(res) != len(dom):
        raise DcpError(RC_EINVAL, "one resident index per domain")
    lens = np.ascontiguousarray(res_len, np.uint32)
    if len(lens) != per_strand * strands:
        raise DcpError(RC_EINVAL, "res_len holds strands x per_strand lengths")
    ws = wo = None
    if win_src is not None:
        ws, wo = np.ascontiguousarray(win_src, np.uint32), np.ascontiguousarray(win_off, np.uint32)
        if len(ws) != per_strand or len(wo) != per_strand:
            raise DcpError(RC_EINVAL, "the window map holds per_strand entries")
    src, begin, end, minus = _locate_outputs(len(dom))
    rc = lib.dcp_domains_locate(res.ctypes.data, dom.ctypes.data, len(dom), lens.ctypes.data, per_strand, strands,
                                ws.ctypes.data if ws is not None else None, wo.ctypes.data if wo is not None else None,
                                src.ctypes.data, begin.ctypes.data, end.ctypes.data, minus.ctypes.data)
    if rc:
        raise DcpError(rc, "a domain lies outside its resident sequence, or a bad batch shape")
    return src, begin, end, minus


def merge_domains(src, minus, profile, begin, end, odds):
    """One representative per duplicated domain (dcp_domains_merge): a bool array, True for the domains kept.  Within
    each (src, minus, profile) group the candidates go by odds = core - null descending (then longer first, then lower
    index first), and one is dropped if a kept one overlaps it by more than half the shorter of the two.  The rank is
    the odds, not the core score: core is a log-likelihood that falls with length, so a stump cut by a window's edge
    would outrank the whole gene."""
    src, profile = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(profile, np.uint32)
    minus = np.ascontiguousarray(minus, np.uint8)
    begin, end = np.ascontiguousarray(begin, np.uint64), np.ascontiguousarray(end, np.uint64)
    odds = np.ascontiguousarray(odds, np.float64)
    n = len(src)
    if not all(len(a) == n for a in (minus, profile, begin, end, odds)):
        raise DcpError(RC_EINVAL, "arrays of one length")
    keep, nkept = np.zeros(n, np.uint8), C.c_uint(0)
    rc = lib.dcp_domains_merge(src.ctypes.data, minus.ctypes.data, profile.ctypes.data, begin.ctypes.data,
                               end.ctypes.data, odds.ctypes.data, n, keep.ctypes.data, C.byref(nkept))
    if rc:
        raise DcpError(rc, "a NaN in odds, or an empty interval")
    assert int(keep.sum()) == nkept.value
    return keep.astype(bool)


# one region of domain_regions: what Scanner.cut_regions cuts and Scanner.scan_pairs scores against `profile`
REGION_DTYPE = np.dtype([("src", np.uint32), ("minus", np.uint8), ("profile", np.uint32), ("begin", np.uint32),
                         ("len", np.uint32), ("nparts", np.uint32)])


def domain_regions(src, minus, profile, begin, end, src_len, max_gap=0, flank=0):
    """Located domains (locate_domains' output, BEFORE any merge) joined into the regions to score again
    (dcp_domains_regions): (reg_of uint32 [n], regions REGION_DTYPE).  Within each (src, minus, profile) group a domain
    joins the open cluster while it begins at most max_gap behind the cluster's largest end; a cluster [lo, hi) gives
    the region [lo - flank, hi + flank) clipped to its source.  Regions come ordered by (src, minus, profile, begin);
    reg_of[j] is domain j's region, nparts the domains of a region."""
    src, profile = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(profile, np.uint32)
    minus = np.ascontiguousarray(minus, np.uint8)
    begin, end = np.ascontiguousarray(begin, np.uint64), np.ascontiguousarray(end, np.uint64)
    lens = np.ascontiguousarray(src_len, np.uint32)
    n = len(src)
    if not all(len(a) == n for a in (minus, profile, begin, end)):
        raise DcpError(RC_EINVAL, "arrays of one length")
    if not (0 <= max_gap < 2 ** 64 and 0 <= flank < 2 ** 32):
        raise DcpError(RC_EINVAL, f"max_gap {max_gap} / flank {flank} out of range")
    reg_of, nreg = np.zeros(n, np.uint32), C.c_uint(0)
    cap = 0
    for _ in range(2):  # count, then fill
        cols = [np.zeros(cap, t) for t in (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)]
        rc = lib.dcp_domains_regions(src.ctypes.data, minus.ctypes.data, profile.ctypes.data, begin.ctypes.data,
                                     end.ctypes.data, n, lens.ctypes.data, len(lens), int(max_gap), int(flank),
                                     reg_of.ctypes.data, *[a.ctypes.data if cap else None for a in cols], cap, C.byref(nreg))
        if rc != RC_ENOMEM:
            break
        cap = nreg.value
    if rc:
        raise DcpError(rc, "an empty interval, a domain outside its source, or a source that is not in src_len")
    regions = np.zeros(nreg.value, REGION_DTYPE)
    for name, a in zip(("src", "minus", "profile", "begin", "len", "nparts"), cols):
        regions[name] = a[:nreg.value]
    return reg_of, regions


def locate_domains_regions(res_idx, domains, res_len, reg_src, reg_begin, reg_minus):
    """locate_domains for a batch of regions (dcp_domains_locate_regions): resident r is the res_len[r] bases from
    reg_begin[r] of source reg_src[r], reverse-complemented where reg_minus[r]."""
    res = np.ascontiguousarray(res_idx, np.uint32)
    dom = np.ascontiguousarray(domains, DOMAIN_DTYPE)
    lens = np.ascontiguousarray(res_len, np.uint32)
    rs, rb = np.ascontiguousarray(reg_src, np.uint32), np.ascontiguousarray(reg_begin, np.uint32)
    rm = np.ascontiguousarray(reg_minus, np.uint8)
    if len(res) != len(dom) or not len(lens) == len(rs) == len(rb) == len(rm):
        raise DcpError(RC_EINVAL, "one resident index per domain, one map entry per region")
    src, begin, end, minus = _locate_outputs(len(dom))
    rc = lib.dcp_domains_locate_regions(res.ctypes.data, dom.ctypes.data, len(dom), lens.ctypes.data, len(lens),
                                        rs.ctypes.data, rb.ctypes.data, rm.ctypes.data, src.ctypes.data,
                                        begin.ctypes.data, end.ctypes.data, minus.ctypes.data)
    if rc:
        raise DcpError(rc, "a domain lies outside its region")
    return src, begin, end, minus


# enum dcp_fit_status (include/dcp_gpu.h): what a Gumbel fit can end with
FIT_OK, FIT_FLAT, FIT_NONFINITE, FIT_DIVERGED = 0, 16, 17, 18


def _probs(probs):
    """None (uniform), or the four base probabilities as a float64 array for the C side to judge."""
    if probs is None:
        return None
    probs = np.ascontiguousarray(probs, np.float64)
    if probs.shape != (4,):
        raise DcpError(RC_EINVAL, "base probabilities: four values, A C G T")
    return probs


def random_thresholds(probs=None):
    """The generator's three thresholds in 0 .. 65 536 for base probabilities (A, C, G, T); None is uniform
    (dcp_seq_random_thresholds).  c[k] = floor(65536 (p_0 + .. + p_k) + 0.5).  A uint32 array."""
    probs = _probs(probs)
    out = np.zeros(3, np.uint32)
    rc = lib.dcp_seq_random_thresholds(None if probs is None else probs.ctypes.data, out.ctypes.data)
    if rc:
        raise DcpError(rc, "bad base probabilities: four finite values >= 0 that sum to 1")
    return out


def random_seq(seed, q, length, probs=None):
    """Random sequence q of `length` bases under seed, as symbol ids (dcp_seq_random): what Scanner.random_seqs makes
    resident as sequence q.  Integer arithmetic, the same bits on host and device."""
    if not (0 <= seed < 2 ** 64 and 0 <= q < 2 ** 32 and 0 <= length < 2 ** 32):
        raise DcpError(RC_EINVAL, "seed in 64 bits, q and length in 32")
    c = random_thresholds(probs)
    out = np.zeros(length, np.uint8)
    lib.dcp_seq_random(seed, q, length, c.ctypes.data, out.ctypes.data)
    return out


def gumbel_fit(x):
    """(mu, lambda, status) of the maximum-likelihood Gumbel fit of a 1-d sample (dcp_gumbel_fit; a strided view is
    fitted in place).  status is FIT_OK, FIT_FLAT, FIT_NONFINITE or FIT_DIVERGED; mu and lambda are NaN unless FIT_OK.
    Fewer than 2 values: DcpError(RC_EINVAL)."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or (len(x) > 1 and (x.strides[0] <= 0 or x.strides[0] % 8)):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
    stride = x.strides[0] // 8 if len(x) > 1 else 1
    mu, lam = C.c_double(0), C.c_double(0)
    rc = lib.dcp_gumbel_fit(x.ctypes.data, len(x), stride, C.byref(mu), C.byref(lam))
    if rc == RC_EINVAL:
        raise DcpError(rc, "a fit needs at least 2 values")
    return mu.value, lam.value, rc


def gumbel_fit_tail(x, k):
    """(mu, lambda, status, tau, k_eff) of the censored Gumbel fit of a 1-d sample (dcp_gumbel_fit_tail; a strided view
    is fitted in place): tau is the k-th largest value, the k_eff >= k values >= tau enter with their values, the
    others only as "below tau".  k = len(x) is gumbel_fit in bits.  tau is NaN and k_eff 0 with FIT_NONFINITE.  Fewer
    than 2 values, k < 2 or k > len(x): DcpError(RC_EINVAL).  The law holds for scores >= tau only."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or (len(x) > 1 and (x.strides[0] <= 0 or x.strides[0] % 8)):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
    stride = x.strides[0] // 8 if len(x) > 1 else 1
    if not 0 <= k < 2 ** 32:
        raise DcpError(RC_EINVAL, "the tail count: 2 .. len(x)")
    mu, lam, tau, k_eff = C.c_double(0), C.c_double(0), C.c_double(0), C.c_uint(0)
    rc = lib.dcp_gumbel_fit_tail(x.ctypes.data, len(x), stride, int(k), C.byref(mu), C.byref(lam), C.byref(tau), C.byref(k_eff))
    if rc == RC_EINVAL:
        raise DcpError(rc, "a tail fit needs at least 2 values and a tail count in 2 .. len(x)")
    return mu.value, lam.value, rc, tau.value, k_eff.value


def gumbel_sf(mu, lam, s):
    """P(X > s) under a Gumbel fit: -expm1(-exp(-lam (s - mu))) (dcp_gumbel_sf)."""
    return lib.dcp_gumbel_sf(float(mu), float(lam), float(s))


def hit_evalues(hits, mu, lam, status, nsearched):
    """E-values of hit records (HIT_DTYPE or HIT64_DTYPE) under a calibration (mu, lam, status) of the resident DB:
    nsearched * P(score >= alt - null) per hit, the number of sequences among nsearched random ones expected to score as
    high against the hit's profile; NaN where the profile's fit is not FIT_OK (dcp_hits_evalues / ...64)."""
    hits = np.ascontiguousarray(hits)
    if hits.dtype not in (HIT_DTYPE, HIT64_DTYPE) or hits.ndim != 1:
        raise DcpError(RC_EINVAL, "hit records: a 1-d array of HIT_DTYPE or HIT64_DTYPE")
    mu, lam = _f64(mu), _f64(lam)
    status = np.ascontiguousarray(status, np.uint8)
    if not (mu.ndim == 1 and mu.shape == lam.shape == status.shape):
        raise DcpError(RC_EINVAL, "mu, lam and status: one entry per profile")
    out = np.zeros(len(hits), np.float64)
    fn = lib.dcp_hits_evalues64 if hits.dtype == HIT64_DTYPE else lib.dcp_hits_evalues
    rc = fn(hits.ctypes.data, len(hits), mu.ctypes.data, lam.ctypes.data, status.ctypes.data, len(mu), float(nsearched),
            out.ctypes.data)
    if rc:
        raise DcpError(rc, "a profile index outside the calibration, or nsearched not finite or negative")
    return out


# which law an E-value is taken under (score_evalues), and which dense matrices a device fit reads (Scanner.fit_exp_tail)
LAW_GUMBEL, LAW_EXP = 0, 1
SCORES_SCAN, SCORES_FORWARD = 0, 1


def exp_tail_fit(x, k):
    """(mu, lambda, status, tau, k_eff) of the exponential tail fit of a 1-d sample (dcp_exp_tail_fit; a strided view is
    fitted in place): tau is the k-th largest value, lambda = k_eff / sum(x - tau over the k_eff values >= tau) and mu =
    tau + log(k_eff / n) / lambda, so that P(X >= s) = exp(-lambda (s - mu)) is k_eff / n at tau.  Closed-form: status is
    FIT_OK, FIT_FLAT (every value >= tau equals tau) or FIT_NONFINITE (tau NaN, k_eff 0); mu and lambda are NaN unless
    FIT_OK.  Fewer than 2 values, k < 2 or k > len(x): DcpError(RC_EINVAL).  The law holds for scores >= tau only."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or (len(x) > 1 and (x.strides[0] <= 0 or x.strides[0] % 8)):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
    stride = x.strides[0] // 8 if len(x) > 1 else 1
    if not 0 <= k < 2 ** 32:
        raise DcpError(RC_EINVAL, "the tail count: 2 .. len(x)")
    mu, lam, tau, k_eff = C.c_double(0), C.c_double(0), C.c_double(0), C.c_uint(0)
    rc = lib.dcp_exp_tail_fit(x.ctypes.data, len(x), stride, int(k), C.byref(mu), C.byref(lam), C.byref(tau), C.byref(k_eff))
    if rc == RC_EINVAL:
        raise DcpError(rc, "a tail fit needs at least 2 values and a tail count in 2 .. len(x)")
    return mu.value, lam.value, rc, tau.value, k_eff.value


def exp_sf(mu, lam, s):
    """P(X >= s) under an exponential tail fit: 1 for s <= mu, else exp(-lam (s - mu)) (dcp_exp_sf)."""
    return lib.dcp_exp_sf(float(mu), float(lam), float(s))


def score_evalues(profile_idx, null, alt, mu, lam, status, nsearched, law):
    """E-values of scores that are not hit records -- the arrays forward_pairs and scan_pairs return -- under a
    calibration (mu, lam, status) of the resident DB: nsearched * P(score >= alt - null) per entry under LAW_GUMBEL
    (gumbel_sf: hit_evalues' numbers) or LAW_EXP (exp_sf: a calibrate_forward calibration); NaN where the profile's fit
    is not FIT_OK (dcp_scores_evalues)."""
    profile_idx = np.ascontiguousarray(profile_idx)
    if profile_idx.ndim != 1 or profile_idx.dtype.kind not in "iu" or (len(profile_idx) and
                                                                        (profile_idx.min() < 0 or profile_idx.max() >= 2 ** 32)):
        raise DcpError(RC_EINVAL, "profile indices: a 1-d array of integers in 32 bits")
    profile_idx = np.ascontiguousarray(profile_idx, np.uint32)
    null, alt, mu, lam = _f64(null), _f64(alt), _f64(mu), _f64(lam)
    status = np.ascontiguousarray(status, np.uint8)
    if not (null.shape == alt.shape == profile_idx.shape):
        raise DcpError(RC_EINVAL, "profile_idx, null and alt: one entry per score")
    if not (mu.ndim == 1 and mu.shape == lam.shape == status.shape):
        raise DcpError(RC_EINVAL, "mu, lam and status: one entry per profile")
    out = np.zeros(len(profile_idx), np.float64)
    rc = lib.dcp_scores_evalues(profile_idx.ctypes.data, null.ctypes.data, alt.ctypes.data, len(profile_idx), mu.ctypes.data,
                                lam.ctypes.data, status.ctypes.data, len(mu), float(nsearched), int(law), out.ctypes.data)
    if rc:
        raise DcpError(rc, "a profile index outside the calibration, nsearched not finite or negative, or an unknown law")
    return out


def device_count():
    return lib.dcp_gpu_device_count()


def _pair_list(seq_idx, profile_idx):
    """A pair list's two index arrays as contiguous uint32, one profile index per sequence index."""
    sq = np.ascontiguousarray(seq_idx, np.uint32)
    pr = np.ascontiguousarray(profile_idx, np.uint32)
    if sq.ndim != 1 or sq.shape != pr.shape:
        raise DcpError(RC_EINVAL, "one profile index per sequence index")
    return sq, pr


class Scanner:
    """One device context = one reference "partition" (thread_run's unit, scan.c:239-249):
    holds a profile shard resident in HBM and scans sequence batches against it."""

    def __init__(self, device=0, lib=None):
        self._lib = lib or globals()["lib"]
        self._c = self._lib.dcp_gpu_ctx_new(device)
        if not self._c:
            raise DcpError(RC_EFAIL, f"no HIP device {device}: this engine has no CPU fallback")
        self._profiles = None
        self._seq_lens = np.zeros(0, np.int64)  # of the resident batch

    def close(self):
        c, self._c = getattr(self, "_c", None), None
        if c:
            self._lib.dcp_gpu_ctx_del(c)

    __del__ = close

    def _check(self, rc):
        if rc:
            raise DcpError(rc, self._lib.dcp_gpu_last_error(self._c).decode())

    @property
    def stream(self):
        return self._lib.dcp_gpu_stream(self._c)

    def upload_db(self, profiles, expand_on_host=False, one_layout=False):
        """one_layout: DCP_DB_ONE_LAYOUT (include/dcp_gpu.h) -- no tile images, the query-lane kernels gather them.
        Profiles of the double build (precision=64) go to dcp_gpu_db_upload64: a double DB, scanned in double
        (the flags do not apply to it).  A list mixing both precisions is refused."""
        precs = {p.precision for p in profiles}
        if len(precs) > 1:
            raise DcpError(RC_EINVAL, "a DB holds profiles of one precision: this list mixes float and double")
        arr = (C.c_void_p * len(profiles))(*[p._h for p in profiles])
        if precs == {64}:
            if expand_on_host or one_layout:
                raise DcpError(RC_EINVAL, "a double DB has one layout, expanded on the device")
            self._check(self._lib.dcp_gpu_db_upload64(self._c, arr, len(profiles)))
        else:
            flags = (DB_EXPAND_ON_HOST if expand_on_host else 0) | (DB_ONE_LAYOUT if one_layout else 0)
            self._check(self._lib.dcp_gpu_db_upload(self._c, arr, len(profiles), flags))
        self._profiles = list(profiles)

    @property
    def precision(self):
        """32 or 64: the precision of the resident DB (0 without one)."""
        return self._lib.dcp_gpu_db_precision(self._c)

    @property
    def one_layout(self):
        return bool(self._lib.dcp_gpu_db_one_layout(self._c))

    @property
    def table_bytes(self):
        return int(self._lib.dcp_gpu_db_table_bytes(self._c))

    @property
    def nprofiles(self):
        return self._lib.dcp_gpu_db_nprofiles(self._c)

    @property
    def nseqs(self):
        return self._lib.dcp_gpu_nseqs(self._c)

    def match_table(self, p):
        """Profile p's match table [1364, core_size] as the device holds it: float64 on a double DB."""
        M = self._profiles[p].core_size
        if self.precision == 64:
            out = np.zeros((NCODES, M), np.float64)
            self._check(self._lib.dcp_gpu_db_fetch_match_table64(self._c, p, out.ctypes.data))
        else:
            out = np.zeros((NCODES, M), np.float32)
            self._check(self._lib.dcp_gpu_db_fetch_match_table(self._c, p, out.ctypes.data))
        return out

    def insert_null_tables64(self, p):
        """(insert [1364], null [1364]) of profile p on a double DB, in float64 (dcp_gpu_db_fetch_insert_null64)."""
        ins, nul = np.zeros(NCODES, np.float64), np.zeros(NCODES, np.float64)
        self._check(self._lib.dcp_gpu_db_fetch_insert_null64(self._c, p, ins.ctypes.data, nul.ctypes.data))
        return ins, nul

    def upload_seqs(self, seqs):
        """seqs: list of ACGT strings, or of uint8 arrays / bytes of symbol ids 0..3."""
        if len(seqs) and isinstance(seqs[0], str):
            seqs = [encode_seq(s) for s in seqs]
        arrs = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else
                np.ascontiguousarray(s, np.uint8) for s in seqs]
        off = np.zeros(len(arrs) + 1, np.uint32)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        cat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(0, np.uint8)
        self.upload_seqs_flat(cat, off)

    def upload_seqs_flat(self, cat, off):
        cat = np.ascontiguousarray(cat, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        self._check(self._lib.dcp_gpu_seqs_upload(self._c, cat.ctypes.data, off.ctypes.data, len(off) - 1))
        self._seq_lens = np.diff(off.astype(np.int64))

    def random_seqs(self, n, length, seed, probs=None):
        """A random batch (dcp_gpu_seqs_random): the resident batch is replaced by n sequences of `length` bases,
        sequence q the bases of random_seq(seed, q, length, probs), generated on the device.  Afterwards the context is
        as after an upload: one strand, uncut; add_reverse_strand, cut_windows and cut_regions may follow."""
        if not (0 <= n < 2 ** 32 and 0 <= length < 2 ** 32 and 0 <= seed < 2 ** 64):
            raise DcpError(RC_EINVAL, "n and length in 32 bits, seed in 64")
        probs = _probs(probs)
        self._check(self._lib.dcp_gpu_seqs_random(self._c, n, length, seed, None if probs is None else probs.ctypes.data))
        self._seq_lens = np.full(n, length, np.int64)

    def _fit_outputs(self):
        n = self.nprofiles
        return np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint8)

    def fit_gumbel(self):
        """(mu, lam, status), one entry per resident profile: the Gumbel fit of alt - null over the dense scores of the
        last scan, which must have covered the whole batch with keep_scores (dcp_gpu_fit_gumbel; one lane per profile
        on the device).  status: FIT_OK, FIT_FLAT, FIT_NONFINITE, FIT_DIVERGED; mu and lam are NaN unless FIT_OK."""
        mu, lam, status = self._fit_outputs()
        self._check(self._lib.dcp_gpu_fit_gumbel(self._c, mu.ctypes.data, lam.ctypes.data, status.ctypes.data))
        return mu, lam, status

    def calibrate(self, n, length, seed, probs=None, multi_hits=True, hmmer3_compat=False, kernel=KERNEL_AUTO):
        """random_seqs(n, length, seed, probs), one scan with these flags that keeps the dense scores and reports no
        hits, fit_gumbel(): (mu, lam, status) for hit_evalues (dcp_gpu_db_calibrate).  The random batch and that scan
        STAY resident: upload the real batch afterwards.  The fit holds for this length, these flags and this base
        composition -- calibrate at the window length that cut_windows will cut."""
        if not (0 <= n < 2 ** 32 and 0 <= length < 2 ** 32 and 0 <= seed < 2 ** 64):
            raise DcpError(RC_EINVAL, "n and length in 32 bits, seed in 64")
        probs = _probs(probs)
        mu, lam, status = self._fit_outputs()
        self._check(self._lib.dcp_gpu_db_calibrate(self._c, n, length, seed, None if probs is None else probs.ctypes.data,
                                                   int(multi_hits), int(hmmer3_compat), int(kernel), mu.ctypes.data,
                                                   lam.ctypes.data, status.ctypes.data))
        self._seq_lens = np.full(n, length, np.int64)
        return mu, lam, status

    def fit_gumbel_tail(self, k):
        """(mu, lam, status, tau, k_eff), one entry per resident profile: the censored Gumbel fit of alt - null over the
        dense scores of the last scan, as fit_gumbel (dcp_gpu_fit_gumbel_tail; two launches: the k-th largest score tau
        per profile by comparisons alone, then the fit over the k_eff scores >= tau).  k in 2 .. nseqs.  The law holds
        for scores >= tau[p]: below it a hit's E-value is at least about nsearched k_eff / nseqs, and not calibrated."""
        if not 0 <= k < 2 ** 32:
            raise DcpError(RC_EINVAL, "the tail count: 2 .. nseqs")
        mu, lam, status = self._fit_outputs()
        tau, k_eff = np.zeros(len(mu), np.float64), np.zeros(len(mu), np.uint32)
        self._check(self._lib.dcp_gpu_fit_gumbel_tail(self._c, int(k), mu.ctypes.data, lam.ctypes.data, status.ctypes.data,
                                                      tau.ctypes.data, k_eff.ctypes.data))
        return mu, lam, status, tau, k_eff

    def calibrate_tail(self, n, length, seed, k, probs=None, multi_hits=True, hmmer3_compat=False, kernel=KERNEL_AUTO):
        """calibrate() with fit_gumbel_tail(k) as its third step: (mu, lam, status, tau, k_eff)
        (dcp_gpu_db_calibrate_tail).  A k outside 2 .. n is refused before the batch is replaced."""
        if not (0 <= n < 2 ** 32 and 0 <= length < 2 ** 32 and 0 <= seed < 2 ** 64 and 0 <= k < 2 ** 32):
            raise DcpError(RC_EINVAL, "n, length and k in 32 bits, seed in 64")
        probs = _probs(probs)
        mu, lam, status = self._fit_outputs()
        tau, k_eff = np.zeros(len(mu), np.float64), np.zeros(len(mu), np.uint32)
        self._check(self._lib.dcp_gpu_db_calibrate_tail(self._c, n, length, seed, None if probs is None else probs.ctypes.data,
                                                        int(multi_hits), int(hmmer3_compat), int(kernel), int(k),
                                                        mu.ctypes.data, lam.ctypes.data, status.ctypes.data, tau.ctypes.data,
                                                        k_eff.ctypes.data))
        self._seq_lens = np.full(n, length, np.int64)
        return mu, lam, status, tau, k_eff

    def calib_tail_kernel_ms(self, which):
        """Milliseconds of the last tail selection kernel (which = 0) or tail fit kernel (1) alone, by HIP events;
        negative if none has run."""
        return self._lib.dcp_gpu_calib_tail_kernel_ms(self._c, which)

    def calib_kernel_ms(self, which):
        """Milliseconds of the last generator kernel (which = 0) or fit kernel (1) alone, by HIP events; negative if
        none has run."""
        return self._lib.dcp_gpu_calib_kernel_ms(self._c, which)

    def add_reverse_strand(self):
        """Both strands (dcp_gpu_seqs_add_revcomp): the resident batch of n sequences becomes 2n, sequence n + q the
        reverse complement of q, written on the device.  Scans, hits, scores and traces then carry indices 0 .. 2n - 1;
        scan(q_range=(n, 2 * n)) is the minus strand alone.  Until the next upload_seqs."""
        self._check(self._lib.dcp_gpu_seqs_add_revcomp(self._c))
        self._seq_lens = np.concatenate([self._seq_lens, self._seq_lens])

    def cut_windows(self, window, step):
        """Windows (dcp_gpu_seqs_cut_windows): the resident batch is replaced by its windows of `window` bases every
        `step` bases (window_starts), in source order, then offset order, written on the device.  Scans, hits, scores and
        traces then carry window indices; window_map() names each window's source and offset.  add_reverse_strand()
        may follow (not precede) it.  Until the next upload_seqs."""
        if not (0 <= window < 2 ** 32 and 0 <= step < 2 ** 32):
            raise DcpError(RC_EINVAL, f"bad window rule (window {window}, step {step})")
        self._check(self._lib.dcp_gpu_seqs_cut_windows(self._c, window, step))
        self._seq_lens = np.concatenate([np.full(len(window_starts(int(L), window, step)), min(int(L), window), np.int64)
                                         for L in self._seq_lens])

    @property
    def windows(self):
        """None, or (window, step) while the resident batch is cut into windows."""
        w, s = C.c_uint(0), C.c_uint(0)
        return (w.value, s.value) if self._lib.dcp_gpu_seqs_windows(self._c, C.byref(w), C.byref(s)) else None

    def window_map(self):
        """(src, off), two uint32 arrays with one entry per window: its source's index in the uploaded batch and its
        first base there (dcp_gpu_seqs_window_map).  After add_reverse_strand resident W + i is window i's reverse
        complement; the map keeps W entries."""
        n = self.nseqs // max(self.strands, 1)
        src, off = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._check(self._lib.dcp_gpu_seqs_window_map(self._c, src.ctypes.data, off.ctypes.data, n))
        return src, off

    def cut_regions(self, src, begin, length, minus):
        """Regions (dcp_gpu_seqs_cut_regions): the resident batch is replaced by the stretches [begin[i], begin[i] +
        length[i]) of its sequences src[i], reverse-complemented where minus[i], written on the device.  Regions may
        overlap, repeat and come in any order.  Scans, hits and traces then carry region indices; region_map() names
        each region's source, first base and strand, and locate_domains() maps through it.  Neither add_reverse_strand
        nor cut_windows may follow.  Until the next upload_seqs."""
        cols = [np.atleast_1d(np.asarray(a)) for a in (src, begin, length)]
        if any(a.size and (a.min() < 0 or a.max() >= 2 ** 32) for a in cols):
            raise DcpError(RC_EINVAL, "a region's source, first base or length does not fit 32 bits")
        src, begin, length = (np.ascontiguousarray(a, np.uint32) for a in cols)
        minus = np.ascontiguousarray(np.atleast_1d(np.asarray(minus)) != 0, np.uint8)
        if not len(src) == len(begin) == len(length) == len(minus):
            raise DcpError(RC_EINVAL, "arrays of one length")
        self._check(self._lib.dcp_gpu_seqs_cut_regions(self._c, src.ctypes.data, begin.ctypes.data, length.ctypes.data,
                                                       minus.ctypes.data, len(src)))
        self._seq_lens = length.astype(np.int64)

    @property
    def regions(self):
        """The number of regions while the resident batch is one of regions (cut_regions), else 0."""
        return self._lib.dcp_gpu_seqs_regions(self._c)

    def region_map(self):
        """(src uint32, begin uint32, minus uint8), one entry per region: its source's index in the uploaded batch, its
        first base there in plus-strand coordinates, its strand (dcp_gpu_seqs_region_map)."""
        n = self.regions
        src, begin, minus = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._check(self._lib.dcp_gpu_seqs_region_map(self._c, src.ctypes.data, begin.ctypes.data, minus.ctypes.data, n))
        return src, begin, minus

    @property
    def strands(self):
        """0 (no batch resident), 1, or 2 after add_reverse_strand."""
        return self._lib.dcp_gpu_seqs_strands(self._c)

    def fetch_seq(self, q):
        """Resident sequence q as a uint8 array of symbol ids, unpacked from the device's words (dcp_gpu_seqs_fetch)."""
        n = C.c_uint(0)
        out = np.zeros(int(self._seq_lens[q]) if 0 <= q < self.nseqs else 1, np.uint8)
        self._check(self._lib.dcp_gpu_seqs_fetch(self._c, q, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def test_seq_words(self, q):
        """TEST-ONLY (test-hooks build): the raw L // 16 + 3 words of resident sequence q (uint32)."""
        n = C.c_uint(0)
        rc = self._lib.dcp_gpu_test_fetch_seq_words(self._c, q, None, 0, C.byref(n))
        if rc != RC_ENOMEM:
            self._check(rc or RC_EFAIL)
        out = np.zeros(n.value, np.uint32)
        self._check(self._lib.dcp_gpu_test_fetch_seq_words(self._c, q, out.ctypes.data, len(out), C.byref(n)))
        return out

    def set_xtrans(self, xt):
        """Explicit special transitions [nseqs, 13] for the resident sequences (dcp_gpu_seqs_set_xtrans):
        what imm_dp_viterbi uses for a profile whose transitions were not set from the sequence length.
        A float64 array on a double DB goes to dcp_gpu_seqs_set_xtrans64 (see set_xtrans64); anything else is
        taken as float, which a scan of a double DB refuses."""
        if self.precision == 64 and np.asarray(xt).dtype == np.float64:
            return self.set_xtrans64(xt)
        xt = np.ascontiguousarray(xt, np.float32).reshape(-1, NXTRANS)
        self._check(self._lib.dcp_gpu_seqs_set_xtrans(self._c, xt.ctypes.data, len(xt)))

    def set_xtrans64(self, xt):
        """Explicit special transitions [nseqs, 13] in double, in xtrans64 order (dcp_gpu_seqs_set_xtrans64): the
        scans and traces of a double DB use them until the next upload_seqs; a float DB refuses them."""
        xt = np.ascontiguousarray(xt, np.float64).reshape(-1, NXTRANS)
        self._check(self._lib.dcp_gpu_seqs_set_xtrans64(self._c, xt.ctypes.data, len(xt)))

    def scan(self, multi_hits=True, hmmer3_compat=False, lrt_threshold=10.0, keep_scores=True,
             sync=True, q_range=None, kernel=KERNEL_AUTO):
        """Scan the resident sequences (or q_range of them) against the resident DB.  kernel: KERNEL_AUTO, or one of
        KERNEL_ROWSWEEP (either DB), KERNEL_QLANE / KERNEL_QLANE2 (float DB), KERNEL_QLANE64 (double DB: the f64
        query-lane kernel, the row sweep's bits at several times its rate from a few hundred queries on; on a
        double DB KERNEL_AUTO is the row sweep).  A kernel that does not fit the DB's precision is RC_EINVAL."""
        prm = ScanParams(int(multi_hits), int(hmmer3_compat), float(lrt_threshold), int(keep_scores),
                         int(kernel))
        # a double DB filters with the threshold in double (dcp_gpu_set_lrt_threshold64)
        self._check(self._lib.dcp_gpu_set_lrt_threshold64(self._c, float(lrt_threshold)))
        if q_range is None:
            self._check(self._lib.dcp_gpu_scan(self._c, C.byref(prm)))
        else:
            self._check(self._lib.dcp_gpu_scan_range(self._c, C.byref(prm), q_range[0], q_range[1]))
        if sync:
            self.sync()

    def scan_pairs(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False, lrt_threshold=10.0, sync=True):
        """Score exactly the pairs (resident sequence seq_idx[i], resident profile profile_idx[i]) with the row-sweep
        kernels over the list (dcp_gpu_scan_pairs), on a float or a double DB: hits() then holds the listed pairs that
        pass the LRT filter, with the bits of a KERNEL_ROWSWEEP scan; lrt_threshold=-inf reports every pair whose scores
        are finite.  A pair listed twice is reported twice.  No dense scores are kept: scores() fails afterwards."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        prm = ScanParams(int(multi_hits), int(hmmer3_compat), float(lrt_threshold), 0, KERNEL_AUTO)
        self._check(self._lib.dcp_gpu_set_lrt_threshold64(self._c, float(lrt_threshold)))
        self._check(self._lib.dcp_gpu_scan_pairs(self._c, C.byref(prm), sq.ctypes.data, pr.ctypes.data, len(sq)))
        if sync:
            self.sync()

    def forward_pairs(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False):
        """(null, alt) Forward scores, float64 arrays in list order, of the pairs (resident sequence seq_idx[i],
        resident profile profile_idx[i]) on a float or a double DB (dcp_gpu_forward_pairs): the log of the summed
        weight of all paths, where a scan's score is the weight of the best one.  Returns synchronised; the last scan's
        results stay what they were.  A pair listed twice is scored twice."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        null, alt = np.zeros(len(sq), np.float64), np.zeros(len(sq), np.float64)
        self._check(self._lib.dcp_gpu_forward_pairs(self._c, int(multi_hits), int(hmmer3_compat), sq.ctypes.data,
                                                    pr.ctypes.data, len(sq), null.ctypes.data, alt.ctypes.data))
        return null, alt

    @property
    def forward_kernel_ms(self):
        """Milliseconds of the last forward_pairs call's kernel launches, by HIP events; negative before any."""
        return self._lib.dcp_gpu_forward_kernel_ms(self._c)

    def forward_pairs_scaled(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False):
        """forward_pairs by the scaled probability-space sweep (dcp_gpu_forward_pairs_scaled): no log and one exp per
        table value in the loop.  The same lists, batches and refusals; scores within 2^-32 (|x| + 1) of forward_pairs'
        on a double DB and within DESIGN 24's looser allowance on a float DB.  Pairs whose values leave the double range
        are rerun by forward_pairs' kernels in the same call (last_forward_scaled_redo_pairs) and have its bits."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        null, alt = np.zeros(len(sq), np.float64), np.zeros(len(sq), np.float64)
        self._check(self._lib.dcp_gpu_forward_pairs_scaled(self._c, int(multi_hits), int(hmmer3_compat), sq.ctypes.data,
                                                           pr.ctypes.data, len(sq), null.ctypes.data, alt.ctypes.data))
        return null, alt

    @property
    def last_forward_scaled_redo_pairs(self):
        """How many pairs the last forward_pairs_scaled or forward_dense_scaled reran in log space."""
        return self._lib.dcp_gpu_forward_scaled_redo_pairs(self._c)

    @property
    def forward_scaled_kernel_ms(self):
        """Milliseconds of the last forward_pairs_scaled call's launches, the rerun's included; negative before any."""
        return self._lib.dcp_gpu_forward_scaled_kernel_ms(self._c)

    def forward_dense_scaled(self, multi_hits=True, hmmer3_compat=False):
        """forward_dense by the scaled sweep (dcp_gpu_forward_dense_scaled): forward_pairs_scaled's bits in the same
        matrices, for forward_scores and fit_exp_tail unchanged."""
        self._check(self._lib.dcp_gpu_forward_dense_scaled(self._c, int(multi_hits), int(hmmer3_compat)))

    @property
    def forward_dense_is_scaled(self):
        """Whether the dense Forward matrices were filled by forward_dense_scaled."""
        return bool(self._lib.dcp_gpu_forward_dense_is_scaled(self._c))

    def test_set_forward_scale_band(self, bits):
        """TEST-ONLY (test-hooks build): the band of the scaled sweeps' rescaling rule in bits (0: the default, 64)."""
        self._check(self._lib.dcp_gpu_test_set_forward_scale_band(self._c, int(bits)))

    def test_set_forward_waves(self, nwaves):
        """TEST-ONLY (test-hooks build): cap the wavefronts of the following forward_pairs launches (0: default)."""
        self._check(self._lib.dcp_gpu_test_set_forward_waves(self._c, int(nwaves)))

    def forward_dense(self, multi_hits=True, hmmer3_compat=False):
        """The dense Forward scan (dcp_gpu_forward_dense): every resident sequence against every resident profile with
        forward_pairs' kernels and bits, the pair lists written on the device.  The two [n, P] matrices stay on the
        device (forward_scores, fit_exp_tail) until the DB, the batch or the explicit transitions change; scans and
        pair-list calls leave them alone, and this call leaves the last scan's results alone.  Returns synchronised."""
        self._check(self._lib.dcp_gpu_forward_dense(self._c, int(multi_hits), int(hmmer3_compat)))

    def forward_scores(self):
        """(null, alt), two [n, P] float64 arrays: the matrices of the last forward_dense
        (dcp_gpu_fetch_forward_scores).  DcpError(RC_EINVAL) while there are none, or they are void."""
        null = np.zeros((self.nseqs, self.nprofiles), np.float64)
        alt = np.zeros_like(null)
        self._check(self._lib.dcp_gpu_fetch_forward_scores(self._c, null.ctypes.data, alt.ctypes.data))
        return null, alt

    def forward_dense_kernel_ms(self):
        """Milliseconds of the last forward_dense call's launches, by HIP events; negative before any."""
        return self._lib.dcp_gpu_forward_dense_kernel_ms(self._c)

    def fit_exp_tail(self, k, source="forward"):
        """(mu, lam, status, tau, k_eff), one entry per resident profile: the exponential tail fit of alt - null
        (dcp_gpu_fit_exp_tail; two launches: fit_gumbel_tail's selection of the k-th largest score tau, then the
        closed-form fit over the k_eff scores >= tau) over the matrices of the last forward_dense (source "forward") or
        the dense scores of the last scan (source "scan", fit_gumbel_tail's preconditions).  k in 2 .. nseqs.  tau,
        k_eff, status and lam are exp_tail_fit's bits on the same scores.  The law -- exp_sf, score_evalues(LAW_EXP) --
        holds for scores >= tau[p]: below it the survival is at least k_eff / nseqs, and not calibrated."""
        if source not in ("forward", "scan"):
            raise DcpError(RC_EINVAL, 'source: "forward" or "scan"')
        if not 0 <= k < 2 ** 32:
            raise DcpError(RC_EINVAL, "the tail count: 2 .. nseqs")
        mu, lam, status = self._fit_outputs()
        tau, k_eff = np.zeros(len(mu), np.float64), np.zeros(len(mu), np.uint32)
        self._check(self._lib.dcp_gpu_fit_exp_tail(self._c, SCORES_FORWARD if source == "forward" else SCORES_SCAN, int(k),
                                                   mu.ctypes.data, lam.ctypes.data, status.ctypes.data, tau.ctypes.data,
                                                   k_eff.ctypes.data))
        return mu, lam, status, tau, k_eff

    def exp_tail_kernel_ms(self, which):
        """Milliseconds of the last fit_exp_tail's selection kernel (which = 0) or fit kernel (1) alone, by HIP events;
        negative if none has run."""
        return self._lib.dcp_gpu_exp_tail_kernel_ms(self._c, which)

    def calibrate_forward(self, n, length, seed, k, probs=None, multi_hits=True, hmmer3_compat=False):
        """random_seqs(n, length, seed, probs), forward_dense(multi_hits, hmmer3_compat), fit_exp_tail(k): (mu, lam,
        status, tau, k_eff) for score_evalues(..., LAW_EXP) (dcp_gpu_db_calibrate_forward).  A k outside 2 .. n is refused
        before the batch is replaced.  The random batch and the matrices STAY resident: upload the real batch
        afterwards.  The fit holds for this length, these flags and this base composition."""
        if not (0 <= n < 2 ** 32 and 0 <= length < 2 ** 32 and 0 <= seed < 2 ** 64 and 0 <= k < 2 ** 32):
            raise DcpError(RC_EINVAL, "n, length and k in 32 bits, seed in 64")
        probs = _probs(probs)
        mu, lam, status = self._fit_outputs()
        tau, k_eff = np.zeros(len(mu), np.float64), np.zeros(len(mu), np.uint32)
        self._check(self._lib.dcp_gpu_db_calibrate_forward(self._c, n, length, seed, None if probs is None else probs.ctypes.data,
                                                           int(multi_hits), int(hmmer3_compat), int(k), mu.ctypes.data,
                                                           lam.ctypes.data, status.ctypes.data, tau.ctypes.data,
                                                           k_eff.ctypes.data))
        self._seq_lens = np.full(n, length, np.int64)
        return mu, lam, status, tau, k_eff

    def test_set_dense_round(self, npairs):
        """TEST-ONLY (test-hooks build): bound the pairs of a round of the following forward_dense calls (0: default)."""
        self._check(self._lib.dcp_gpu_test_set_dense_round(self._c, int(npairs)))

    def posterior_pairs(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False):
        """(row_off, begin, end, core, alt_fwd, alt_bwd) of the pairs (resident sequence seq_idx[i], resident profile
        profile_idx[i]) on a float or a double DB (dcp_gpu_posterior_pairs): pair i's rows are
        [row_off[i], row_off[i + 1]) of the three float64 arrays, one per row j = 0 .. L_i -- the posteriors that a
        domain begins at row j, that one ends there, and that base j - 1 is emitted by a core state -- and the alt score
        by the Forward sweep (forward_pairs' bits) and by the Backward sweep.  Returns synchronised; the last scan's
        results stay what they were."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        lens = getattr(self, "_seq_lens", np.zeros(0, np.int64))
        ok = sq < len(lens)  # an index out of range is the call's to refuse, with its message
        cap = int(np.sum(lens[sq[ok]] + 1)) if len(sq) else 0
        row_off = np.zeros(len(sq) + 1, np.uint64)
        begin, end, core = (np.zeros(cap, np.float64) for _ in range(3))
        fwd, bwd = np.zeros(len(sq), np.float64), np.zeros(len(sq), np.float64)
        self._check(self._lib.dcp_gpu_posterior_pairs(self._c, int(multi_hits), int(hmmer3_compat), sq.ctypes.data,
                                                      pr.ctypes.data, len(sq), row_off.ctypes.data, begin.ctypes.data,
                                                      end.ctypes.data, core.ctypes.data, cap, fwd.ctypes.data,
                                                      bwd.ctypes.data))
        return row_off, begin, end, core, fwd, bwd

    def posterior_pairs_scaled(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False):
        """posterior_pairs by the scaled probability-space sweeps (dcp_gpu_posterior_pairs_scaled): the same six
        results, no log-space cell, five logs per row.  Pairs that leave the double range, or whose records may have
        lost a term that matters to underflow, are rerun by posterior_pairs' kernels in the same call
        (last_posterior_scaled_redo_pairs) and have its bits."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        lens = getattr(self, "_seq_lens", np.zeros(0, np.int64))
        ok = sq < len(lens)  # an index out of range is the call's to refuse, with its message
        cap = int(np.sum(lens[sq[ok]] + 1)) if len(sq) else 0
        row_off = np.zeros(len(sq) + 1, np.uint64)
        begin, end, core = (np.zeros(cap, np.float64) for _ in range(3))
        fwd, bwd = np.zeros(len(sq), np.float64), np.zeros(len(sq), np.float64)
        self._check(self._lib.dcp_gpu_posterior_pairs_scaled(self._c, int(multi_hits), int(hmmer3_compat), sq.ctypes.data,
                                                             pr.ctypes.data, len(sq), row_off.ctypes.data,
                                                             begin.ctypes.data, end.ctypes.data, core.ctypes.data, cap,
                                                             fwd.ctypes.data, bwd.ctypes.data))
        return row_off, begin, end, core, fwd, bwd

    @property
    def last_posterior_scaled_redo_pairs(self):
        """How many pairs the last posterior_pairs_scaled reran in log space."""
        return self._lib.dcp_gpu_posterior_scaled_redo_pairs(self._c)

    @property
    def posterior_scaled_kernel_ms(self):
        """Milliseconds of the last posterior_pairs_scaled call's launches, the reruns included; negative before any."""
        return self._lib.dcp_gpu_posterior_scaled_kernel_ms(self._c)

    @property
    def posterior_kernel_ms(self):
        """Milliseconds of the last posterior_pairs call's kernel launches, by HIP events; negative before any."""
        return self._lib.dcp_gpu_posterior_kernel_ms(self._c)

    def test_set_posterior_budget(self, nbytes):
        """TEST-ONLY (test-hooks build): the device memory the following posterior_pairs calls give their row records
        (0: the default, 1 GiB)."""
        self._check(self._lib.dcp_gpu_test_set_posterior_budget(self._c, int(nbytes)))

    def envelope_pairs(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False, hi=0.5, lo=None, min_len=1,
                       scaled=True):
        """(env_off, env, alt_fwd, alt_bwd) of the pairs (resident sequence seq_idx[i], resident profile profile_idx[i])
        on a float or a double DB (dcp_gpu_envelope_pairs): the posterior envelopes of every pair, found on the device
        from the rows posterior_pairs_scaled (scaled=True) or posterior_pairs (scaled=False) would return, without those
        rows leaving it.  env is an ENVELOPE_DTYPE array, pair i's records env[env_off[i]:env_off[i + 1]] in order of
        begin: the maximal runs of bases with core >= lo (lo=None: hi), at least min_len bases long, that reach hi
        (posterior_envelope_records is the host twin).  alt_fwd / alt_bwd have the posterior call's bits.  The array
        is sized by a first guess of four envelopes a pair; if the list has more, the call names the count
        (DCP_ENOMEM's env_off) and runs once more.  Returns synchronised; the last scan's results stay what they were."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        n = len(sq)
        lo = hi if lo is None else lo
        cap = 4 * n + 64
        off = np.zeros(n + 1, np.uint64)
        fwd, bwd = np.zeros(n, np.float64), np.zeros(n, np.float64)
        for _ in range(2):
            env = np.zeros(cap, ENVELOPE_DTYPE)
            rc = self._lib.dcp_gpu_envelope_pairs(self._c, int(multi_hits), int(hmmer3_compat), int(bool(scaled)),
                                                  sq.ctypes.data, pr.ctypes.data, n, float(hi), float(lo), int(min_len),
                                                  env.ctypes.data, cap, off.ctypes.data, fwd.ctypes.data, bwd.ctypes.data)
            if rc != RC_ENOMEM or int(off[n]) <= cap:
                break
            cap = int(off[n])
        self._check(rc)
        return off, env[:int(off[n])].copy(), fwd, bwd

    @property
    def envelope_kernel_ms(self):
        """Milliseconds of the last envelope_pairs call's launches -- sweeps, reruns, combining and envelope kernels, all
        rounds -- by HIP events; negative before any."""
        return self._lib.dcp_gpu_envelope_kernel_ms(self._c)

    @property
    def test_envelope_records_kernel_ms(self):
        """TEST-ONLY (test-hooks build): the envelope kernels' own part of envelope_kernel_ms."""
        return self._lib.dcp_gpu_test_envelope_records_kernel_ms(self._c)

    def test_envelopes_of_rows(self, row_off, begin, end, core, hi=0.5, lo=None, min_len=1):
        """TEST-ONLY (test-hooks build): (env_off, env) of caller-made rows by the envelope kernels alone
        (dcp_gpu_test_envelopes_of_rows): pair i's rows are [row_off[i], row_off[i + 1]) of the three arrays."""
        row_off = np.ascontiguousarray(row_off, np.uint64)
        begin, end, core = _f64(begin), _f64(end), _f64(core)
        n = len(row_off) - 1
        lo = hi if lo is None else lo
        off = np.zeros(n + 1, np.uint64)
        cap = int(row_off[-1] - row_off[0])  # no more runs than rows
        env = np.zeros(max(cap, 1), ENVELOPE_DTYPE)
        self._check(self._lib.dcp_gpu_test_envelopes_of_rows(self._c, row_off.ctypes.data, begin.ctypes.data, end.ctypes.data,
                                                             core.ctypes.data, n, float(hi), float(lo), int(min_len),
                                                             env.ctypes.data, cap, off.ctypes.data))
        return off, env[:int(off[n])].copy()

    def mea_pairs(self, seq_idx, profile_idx, multi_hits=True, hmmer3_compat=False):
        """(paths, posts, gain, alt_fwd) of the pairs (resident sequence seq_idx[i], resident profile profile_idx[i])
        on a float or a double DB (dcp_gpu_mea_pairs): the posterior-decoded path of every pair -- a list of
        STEP_DTYPE arrays that decode_paths and path_domains take as they are -- the word posterior of every step
        (-1 for a step that emits nothing), the path's gain (the sum of seqlen x posterior) and the Forward alt score
        (forward_pairs' bits).  A pair with no path at all has zero steps and gain -inf.  Returns synchronised; the
        last scan's results stay what they were."""
        sq, pr = _pair_list(seq_idx, profile_idx)
        n = len(sq)
        # the driver's own first estimate, L + M + 16 steps a pair; the call names the true count if that is short.  An
        # index out of range, a missing DB or batch are the call's to refuse, with its message
        lens = self._seq_lens
        sizes = np.array([p.core_size for p in self._profiles or []], np.int64)
        ok = (sq < len(lens)) & (pr < len(sizes))
        cap = int(np.sum(lens[sq[ok]] + sizes[pr[ok]] + 16))
        off = np.zeros(n + 1, np.uint32)
        gain, fwd = np.zeros(n, np.float64), np.zeros(n, np.float64)
        for _ in range(2):
            steps, post = np.zeros(max(cap, 1), STEP_DTYPE), np.zeros(max(cap, 1), np.float64)
            rc = self._lib.dcp_gpu_mea_pairs(self._c, int(multi_hits), int(hmmer3_compat), sq.ctypes.data, pr.ctypes.data, n,
                                             steps.ctypes.data, cap, off.ctypes.data, post.ctypes.data, gain.ctypes.data,
                                             fwd.ctypes.data)
            if rc != RC_ENOMEM or int(off[n]) <= cap:
                break
            cap = int(off[n])
        self._check(rc)
        paths = [steps[int(off[i]):int(off[i + 1])].copy() for i in range(n)]
        posts = [post[int(off[i]):int(off[i + 1])].copy() for i in range(n)]
        return paths, posts, gain, fwd

    @property
    def mea_kernel_ms(self):
        """Milliseconds of the last mea_pairs call's kernel launches, by HIP events; negative before any."""
        return self._lib.dcp_gpu_mea_kernel_ms(self._c)

    def test_set_mea_budget(self, nbytes):
        """TEST-ONLY (test-hooks build): the device memory the following mea_pairs calls give their matrices and
        choices (0: the default, 8 GiB)."""
        self._check(self._lib.dcp_gpu_test_set_mea_budget(self._c, int(nbytes)))

    def set_hit_buffer(self, hits_dev_ptr, cap, nhits_dev_ptr):
        """Route hit records into caller-owned device memory (e.g. a torch tensor for RCCL)."""
        self._check(self._lib.dcp_gpu_set_hit_buffer(self._c, hits_dev_ptr, cap, nhits_dev_ptr))

    def set_hit_buffer64(self, hits_dev_ptr, cap, nhits_dev_ptr):
        """The same for the scans of a double DB (dcp_gpu_set_hit_buffer64): cap records of HIT64_DTYPE -- 6 int32
        words each -- and one counter in caller-owned device memory; (None, 0, None) restores the context's own
        buffer.  Independent of set_hit_buffer: a scan writes to the registration of its DB's precision."""
        self._check(self._lib.dcp_gpu_set_hit_buffer64(self._c, hits_dev_ptr, cap, nhits_dev_ptr))

    def hit_buffer64(self):
        """(records pointer, counter pointer, capacity) of the device memory the last scan of a double DB wrote its
        hits to (dcp_gpu_hit_buffer64): the context's own or the caller's.  RC_EINVAL before any scan and after a
        scan of a float DB."""
        h, n, cap = C.c_void_p(), C.c_void_p(), C.c_uint(0)
        self._check(self._lib.dcp_gpu_hit_buffer64(self._c, C.byref(h), C.byref(n), C.byref(cap)))
        return h.value, n.value, cap.value

    def launch_infos(self):
        out = []
        for i in range(self.last_scan_launches):
            li = LaunchInfo()
            self._check(self._lib.dcp_gpu_last_scan_launch_info(self._c, i, C.byref(li)))
            out.append(dict(R=li.nodes_per_lane, W=li.waves_per_pair, nprofiles=li.nprofiles,
                            ms=li.ms, cells=li.cells, algorithmic_bytes=li.algorithmic_bytes))
        return out

    def sync(self):
        self._check(self._lib.dcp_gpu_sync(self._c))

    def test_set_redo_cap(self, cap):
        """TEST-ONLY, and only on a Scanner of the test-hooks build (load_testhooks): shrink the redo lists
        (0 restores 2^26) to reach the overflow path."""
        self._check(self._lib.dcp_gpu_test_set_redo_cap(self._c, int(cap)))

    def test_set_ring_stall(self, on):
        """TEST-ONLY (test-hooks build): the next two-stage query-lane scans stall one stage of the first task, so its
        partner runs into the ring hand-shake's poll bound (the scan must fail with RC_EFAIL, not hang)."""
        self._check(self._lib.dcp_gpu_test_set_ring_stall(self._c, int(bool(on))))

    def test_set_seg_col_bytes(self, nbytes):
        """TEST-ONLY (test-hooks build): cap on a size class's boundary columns in the segmented row sweep (0: default)."""
        self._check(self._lib.dcp_gpu_test_set_seg_col_bytes(self._c, int(nbytes)))

    def test_set_trace_mode(self, own_forward, budget_floats=0):
        """TEST-ONLY (test-hooks build): trace_paths' forward pass by the trace kernel's own loop (1) or the row-sweep
        kernels (0, the default); budget_floats: work area per round of launches (0: default)."""
        self._check(self._lib.dcp_gpu_test_set_trace_mode(self._c, int(bool(own_forward)), int(budget_floats)))

    def test_table_span(self, p):
        """TEST-ONLY (test-hooks build): profile p's raw column span of the match tables, padding included
        (dcp_gpu_test_fetch_table_span): ([1364, span] in the DB's precision, the device's row stride)."""
        span, ldk, eb = C.c_uint(0), C.c_uint(0), C.c_uint(0)
        self._check(self._lib.dcp_gpu_test_fetch_table_span(self._c, p, None, 0, C.byref(span), C.byref(ldk),
                                                            C.byref(eb)))
        out = np.zeros((NCODES, span.value), np.float64 if eb.value == 8 else np.float32)
        self._check(self._lib.dcp_gpu_test_fetch_table_span(self._c, p, out.ctypes.data, out.nbytes, C.byref(span),
                                                            C.byref(ldk), C.byref(eb)))
        return out, ldk.value

    def test_rowsweep_plan(self):
        """TEST-ONLY (test-hooks build, read-only): how the last float row-sweep scan ran each size class
        (dcp_gpu_test_last_rowsweep_plan): {"forked": bool, "classes": {(R, W): {"path": "plain" | "mp" | "segmented",
        "stage", "waves", "prefetch" (plain), "chunk", "seg_redo" (segmented), "flagged_rest" (mp)}}}; empty classes
        are left out."""
        n = C.c_uint(0)
        rc = self._lib.dcp_gpu_test_last_rowsweep_plan(self._c, None, 0, C.byref(n))
        if rc != RC_ENOMEM:
            self._check(rc or RC_EFAIL)
        w = np.zeros(n.value, np.uint32)
        self._check(self._lib.dcp_gpu_test_last_rowsweep_plan(self._c, w.ctypes.data, len(w), C.byref(n)))
        per = (len(w) - 2) // int(w[1])
        classes = {}
        for k in range(int(w[1])):
            R, W, path, stage, waves, pf, chunk, redo, rest = (int(v) for v in w[2 + per * k:2 + per * k + 9])
            if path:
                classes[(R, W)] = dict(path=("plain", "mp", "segmented")[path - 1], stage=stage, waves=waves, prefetch=pf,
                                       chunk=chunk, seg_redo=redo, flagged_rest=bool(rest))
        return dict(forked=bool(w[0]), classes=classes)

    def test_pair_launches(self):
        """TEST-ONLY (test-hooks build, read-only): the pair-mode launches of the last scan or scan_pairs call, in launch
        order (dcp_gpu_test_last_pair_launches): a list of {"kind": "scan_pairs" | "qlane_redo" | "seg_redo",
        "precision": 32 | 64, "cls": (R, W) of the float size class, or "group": 0 .. 3 of the double launch group and
        "R" its nodes per lane, "units": blocks (float) or wavefronts (double) launched, "tpb": tasks per block,
        "cap": the list capacity the kernel was given}.  Waits for the stream and completes nothing: after a scan
        whose redo lists overflowed, ask before anything that repeats it (hits, scores, last_scan_redo_pairs)."""
        n = C.c_uint(0)
        rc = self._lib.dcp_gpu_test_last_pair_launches(self._c, None, 0, C.byref(n))
        if rc != RC_ENOMEM:
            self._check(rc or RC_EFAIL)
        w = np.zeros(n.value, np.uint32)
        self._check(self._lib.dcp_gpu_test_last_pair_launches(self._c, w.ctypes.data, len(w), C.byref(n)))
        out = []
        for i in range(int(w[0])):
            kind, prec, a, b, units, tpb, cap = (int(v) for v in w[1 + 7 * i:8 + 7 * i])
            rec = dict(kind=("scan_pairs", "qlane_redo", "seg_redo")[kind - 1], precision=prec, units=units, tpb=tpb, cap=cap)
            rec.update(dict(cls=(a, b)) if prec == 32 else dict(group=a, R=b))
            out.append(rec)
        return out

    def test_set_rowsweep_variant(self, stage_rows, block_waves=0):
        """TEST-ONLY (test-hooks build): force the grid-mode row-sweep kernel variant; stage_rows < 0: automatic."""
        self._check(self._lib.dcp_gpu_test_set_rowsweep_variant(self._c, int(stage_rows), int(block_waves)))

    @property
    def last_scan_ms(self):
        return self._lib.dcp_gpu_last_scan_ms(self._c)

    @property
    def last_scan_kernel(self):
        """KERNEL_ROWSWEEP / KERNEL_QLANE / KERNEL_QLANE2 / KERNEL_QLANE64: what the last scan ran with
        (KERNEL_ROWSWEEP after a query-lane scan whose redo list overflowed and was repeated)."""
        return self._lib.dcp_gpu_last_scan_kernel(self._c)

    @property
    def last_scan_launches(self):
        return self._lib.dcp_gpu_last_scan_launches(self._c)

    @property
    def last_scan_query_plan(self):
        """The batch plan the last scan ran with, if it ran KERNEL_QLANE64 (synchronises): a dict of the plan's
        blocks, the rows a tile costs summed over the blocks, the rows of a block's planes and the most groups any
        wavefront slot holds.  DcpError (RC_EINVAL) after any other scan -- an overflowed kernel-4 scan that was
        repeated with the row sweep included -- and before the first."""
        nb, rows, prow, mg = C.c_uint(0), C.c_ulonglong(0), C.c_uint(0), C.c_uint(0)
        self._check(self._lib.dcp_gpu_last_scan_query_plan(self._c, C.byref(nb), C.byref(rows), C.byref(prow),
                                                           C.byref(mg)))
        return dict(nblocks=nb.value, sum_block_rows=rows.value, plane_rows=prow.value,
                    max_groups_per_slot=mg.value)

    @property
    def last_scan_redo_pairs(self):
        """Pairs of the last query-lane scan that the row-sweep kernel re-scored (synchronises)."""
        n = C.c_uint(0)
        self._check(self._lib.dcp_gpu_last_scan_redo_pairs(self._c, C.byref(n)))
        return n.value

    @property
    def cells(self):
        return self._lib.dcp_gpu_scan_cells(self._c)

    @property
    def algorithmic_bytes(self):
        return self._lib.dcp_gpu_scan_algorithmic_bytes(self._c)

    def scores(self):
        """(null[nseqs, nprofiles], alt[nseqs, nprofiles]) of the last scan: float64 after a scan of a double DB."""
        f64 = self.precision == 64
        nl = np.zeros((self.nseqs, self.nprofiles), np.float64 if f64 else np.float32)
        al = np.zeros_like(nl)
        fetch = self._lib.dcp_gpu_fetch_scores64 if f64 else self._lib.dcp_gpu_fetch_scores
        self._check(fetch(self._c, nl.ctypes.data, al.ctypes.data))
        return nl, al

    def trace_paths(self, hits, multi_hits=True, hmmer3_compat=False, null_model=False):
        """Viterbi paths (alt model, or null model if null_model) of the given hit records, computed
        on the device: a list of STEP_DTYPE arrays, plus the log-likelihoods the trace recomputed.
        On a double DB the records are HIT64_DTYPE and the log-likelihoods float64 (dcp_gpu_trace_paths64)."""
        f64 = self.precision == 64
        h = np.ascontiguousarray(hits, HIT64_DTYPE if f64 else HIT_DTYPE)
        trace = self._lib.dcp_gpu_trace_paths64 if f64 else self._lib.dcp_gpu_trace_paths
        n = len(h)
        off = np.zeros(n + 1, np.uint32)
        alt = np.zeros(n, np.float64 if f64 else np.float32)
        cap = int(sum(2 * int(self._seq_lens[q]) + 2 * self._profiles[p].core_size + 16
                      for q, p in zip(h["seq_idx"], h["profile_idx"]))) if n else 0
        steps = np.zeros(max(cap, 1), STEP_DTYPE)
        rc = trace(self._c, h.ctypes.data, n, int(multi_hits), int(hmmer3_compat), int(null_model),
                   steps.ctypes.data, cap, off.ctypes.data, alt.ctypes.data)
        if rc == RC_ENOMEM and off[n] > cap:  # the estimate is short of a long multi-domain path: the true total
            cap = int(off[n])
            steps = np.zeros(cap, STEP_DTYPE)
            rc = trace(self._c, h.ctypes.data, n, int(multi_hits), int(hmmer3_compat), int(null_model),
                       steps.ctypes.data, cap, off.ctypes.data, alt.ctypes.data)
        self._check(rc)
        return [steps[off[i]:off[i + 1]].copy() for i in range(n)], alt

    def keep_dists(self, on=True):
        """dcp_gpu_db_keep_dists: later uploads keep the profiles' compact distributions resident for decode_paths
        (516 B per node of a float DB, 1 032 B of a double DB).  Default off."""
        self._check(self._lib.dcp_gpu_db_keep_dists(self._c, int(bool(on))))

    @property
    def has_dists(self):
        """True if the resident DB can decode (dcp_gpu_db_has_dists)."""
        return bool(self._lib.dcp_gpu_db_has_dists(self._c))

    def decode_paths(self, hits, paths):
        """The codon of every step of the given paths, decoded on the device (dcp_gpu_decode_paths): a list of uint8
        arrays, one per path, code 16a + 4b + c of the codon ProteinProfile.decode returns for the step, CODE_MUTE for
        a step that emits nothing.  hits: any structured array with seq_idx / profile_idx (HIT_DTYPE, HIT64_DTYPE);
        paths: what trace_paths returns (its list of STEP_DTYPE arrays, or the (list, logliks) pair itself)."""
        if isinstance(paths, tuple):
            paths = paths[0]
        n = len(paths)
        if len(hits) != n:
            raise DcpError(RC_EINVAL, "one path per hit")
        sq = np.ascontiguousarray(hits["seq_idx"], np.uint32)
        pr = np.ascontiguousarray(hits["profile_idx"], np.uint32)
        off = np.zeros(n + 1, np.uint32)
        if n:
            off[1:] = np.cumsum([len(p) for p in paths])
        steps = np.ascontiguousarray(np.concatenate(paths), STEP_DTYPE) if n and off[n] else np.zeros(1, STEP_DTYPE)
        codes = np.zeros(max(int(off[n]), 1), np.uint8)
        self._check(self._lib.dcp_gpu_decode_paths(self._c, sq.ctypes.data, pr.ctypes.data, n, steps.ctypes.data,
                                                   off.ctypes.data, codes.ctypes.data))
        return [codes[off[i]:off[i + 1]].copy() for i in range(n)]

    def path_domains(self, hits, paths, multi_hits=True, hmmer3_compat=False):
        """The domains of the given paths -- one per B .. E stretch of an alt path -- split and scored on the device
        (dcp_gpu_path_domains / ...64): (domains DOMAIN_DTYPE, dom_off uint32 [n + 1], core, null, total).  Path i's
        domains are domains[dom_off[i]:dom_off[i + 1]] (none for a null path); core[d] is the domain's score from B to
        E on the resident tables, null[d] the null emissions of the same fragments, total[i] the whole path's score, all
        in the DB's precision and in step order.  hits, paths: as for decode_paths; the flags as for trace_paths.
        Like hits(), it retries once at the true count when the first capacity is too small."""
        if isinstance(paths, tuple):
            paths = paths[0]
        n = len(paths)
        if len(hits) != n:
            raise DcpError(RC_EINVAL, "one path per hit")
        f64 = self.precision == 64
        real = np.float64 if f64 else np.float32
        call = self._lib.dcp_gpu_path_domains64 if f64 else self._lib.dcp_gpu_path_domains
        sq = np.ascontiguousarray(hits["seq_idx"], np.uint32)
        pr = np.ascontiguousarray(hits["profile_idx"], np.uint32)
        off = np.zeros(n + 1, np.uint32)
        if n:
            off[1:] = np.cumsum([len(p) for p in paths])
        steps = np.ascontiguousarray(np.concatenate(paths), STEP_DTYPE) if n and off[n] else np.zeros(1, STEP_DTYPE)
        dom_off = np.zeros(n + 1, np.uint32)
        total = np.zeros(n, real)
        cap = max(2 * n, 1)
        for _ in range(2):
            dom = np.zeros(cap, DOMAIN_DTYPE)
            core, null = np.zeros(cap, real), np.zeros(cap, real)
            rc = call(self._c, sq.ctypes.data, pr.ctypes.data, n, steps.ctypes.data, off.ctypes.data, int(multi_hits),
                      int(hmmer3_compat), dom.ctypes.data, cap, dom_off.ctypes.data, core.ctypes.data, null.ctypes.data,
                      total.ctypes.data)
            if rc != RC_ENOMEM or dom_off[n] <= cap:
                break
            cap = int(dom_off[n])
        self._check(rc)
        nd = int(dom_off[n])
        return dom[:nd], dom_off, core[:nd], null[:nd], total

    @property
    def path_domains_kernel_ms(self):
        """Milliseconds the kernel of the last path_domains call ran (dcp_gpu_path_domains_kernel_ms)."""
        return self._lib.dcp_gpu_path_domains_kernel_ms(self._c)

    def locate_domains(self, hits, domains):
        """Where the domains of path_domains(hits, ...) lie on the uploaded sequences (dcp_gpu_domains_locate), through
        the context's own strand and window maps: (src uint32, begin uint64, end uint64, minus uint8), the interval in
        the source's plus-strand coordinates."""
        dom = np.ascontiguousarray(domains, DOMAIN_DTYPE)
        res = np.ascontiguousarray(np.asarray(hits["seq_idx"], np.uint32)[dom["path"]] if len(dom) else [], np.uint32)
        src, begin, end, minus = _locate_outputs(len(dom))
        self._check(self._lib.dcp_gpu_domains_locate(self._c, res.ctypes.data, dom.ctypes.data, len(dom), src.ctypes.data,
                                                     begin.ctypes.data, end.ctypes.data, minus.ctypes.data))
        return src, begin, end, minus

    def hits(self, cap=1 << 20):
        """Hit records of the last scan, sorted by (seq_idx, profile_idx): HIT64_DTYPE after a scan of a double DB."""
        f64 = self.precision == 64
        buf = np.zeros(cap, HIT64_DTYPE if f64 else HIT_DTYPE)
        n = C.c_uint(0)
        fetch = self._lib.dcp_gpu_fetch_hits64 if f64 else self._lib.dcp_gpu_fetch_hits
        rc = fetch(self._c, buf.ctypes.data, cap, C.byref(n))
        if rc == RC_ENOMEM and n.value > cap:
            return self.hits(n.value)
        self._check(rc)
        return buf[:n.value]
