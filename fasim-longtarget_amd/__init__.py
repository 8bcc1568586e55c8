"""fasim-longtarget_amd: ctypes binding of libfasim_hip.so (include/fasim_hip.h).

The package directory name contains a hyphen (it is fixed by the project layout), so import it with

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("fasim_longtarget_amd", ".../fasim-longtarget_amd/__init__.py")
    mod = importlib.util.module_from_spec(spec); sys.modules[spec.name] = mod; spec.loader.exec_module(mod)

or use the `load()` helper in `__graft_entry__.py`.

Names mirror the reference's interface for this path: `calc_score_once` (stats.h:879), `ssw_pre_align`
(ssw.h:128), `ssw_align` (ssw.h:118), `pick_candidates` (Aligner::preAlign, ssw_cpp.cpp:427-572), `scan`
(= the body of LongTarget(), Fasim-LongTarget.cpp:379-598) and `tfosorted` (printResult(), :797-829).

There is no CPU fallback: if the shared library is missing or no HIP device is usable, construction of
`Engine` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

# the scan keeps ~10 batches in flight on separate HIP streams; give them more than the runtime's default of four
# hardware queues (must be in the environment before HIP initialises, i.e. before torch touches the GPU)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfasim_hip.so")


class FasimError(RuntimeError):
    """`code` is the FASIM_E_* value of the failing call (None where the binding itself raised)."""

    def __init__(self, msg="", code=None):
        super().__init__(msg)
        self.code = code


E_ARG = -2              # FASIM_E_ARG
E_UNSUPPORTED = -5      # FASIM_E_UNSUPPORTED


class Params(C.Structure):
    """struct fasim_params -- defaults of initEnv() (Fasim-LongTarget.cpp:284-303)."""
    _fields_ = [("rule", C.c_int32), ("cutLength", C.c_int32), ("strand", C.c_int32), ("overlapLength", C.c_int32),
                ("ntMin", C.c_int32), ("ntMax", C.c_int32), ("scoreMin", C.c_float), ("minIdentity", C.c_float),
                ("minStability", C.c_float), ("penaltyT", C.c_int32), ("penaltyC", C.c_int32), ("cDistance", C.c_int32),
                ("cLength", C.c_int32), ("classicSim", C.c_int32)]


class Alignment(C.Structure):
    _fields_ = [("sw_score", C.c_int32), ("ref_begin", C.c_int32), ("ref_end", C.c_int32), ("query_begin", C.c_int32),
                ("query_end", C.c_int32), ("cigar_len", C.c_int32), ("cigar", C.c_uint32 * 256)]

    def cigar_string(self) -> str:
        ops = "MIDNSHP=X"
        return "".join(f"{c >> 4}{'M' if (c & 15) > 8 else ops[c & 15]}" for c in self.cigar[: max(0, self.cigar_len)])


class Triplex(C.Structure):
    _fields_ = [("stari", C.c_int32), ("endi", C.c_int32), ("starj", C.c_int32), ("endj", C.c_int32), ("strand", C.c_int32),
                ("reverse", C.c_int32), ("rule", C.c_int32), ("nt", C.c_int32), ("score", C.c_float), ("identity", C.c_float),
                ("tri_score", C.c_float), ("seg", C.c_int32), ("enc", C.c_int32), ("genome_shift", C.c_int32),
                ("tfo_off", C.c_int64), ("tts_off", C.c_int64)]


class ScanStats(C.Structure):
    _fields_ = [("segments", C.c_int64), ("segments_skipped", C.c_int64), ("units", C.c_int64), ("candidates", C.c_int64),
                ("align_calls", C.c_int64), ("align_word_reruns", C.c_int64), ("stage2_overflow_units", C.c_int64),
                ("stage1_word_reruns", C.c_int64), ("logical_cells", C.c_int64), ("t_total_s", C.c_double),
                ("t_stage1_s", C.c_double), ("t_stage2_s", C.c_double), ("t_stage3_s", C.c_double), ("t_host_s", C.c_double),
                ("kernel_ms", C.c_double * 10), ("kernel_launches", C.c_int64 * 10), ("cells_stage1", C.c_int64),
                ("cells_stage2", C.c_int64), ("cells_stage3", C.c_int64), ("hazard_units", C.c_int64), ("rev_exact", C.c_int64),
                ("exact_replays", C.c_int64), ("tries_skipped", C.c_int64), ("band_tries", C.c_int64), ("band_proven", C.c_int64),
                ("band_cells", C.c_int64), ("rev_bound_passes", C.c_int64), ("striped_window_probs", C.c_int64),
                ("striped_window_ms", C.c_double), ("dp_f16_reruns", C.c_int64),
                ("finish_lds16", C.c_int64), ("finish_lds64", C.c_int64), ("finish_glob16k", C.c_int64), ("finish_glob1m", C.c_int64),
                ("sim_resweep_lds", C.c_int64), ("sim_resweep_l2", C.c_int64), ("sim_suspended", C.c_int64), ("sim_handover", C.c_int64),
                ("finish_skipped", C.c_int64), ("finish_skip_violations", C.c_int64)]


class SimNode(C.Structure):
    """struct fasim_sim_node: one entry of SIM's node list (vertex, sim.h:47-58)."""
    _fields_ = [(k, C.c_int64) for k in ("score", "stari", "starj", "endi", "endj", "top", "bot", "left", "right")]

    def astuple(self):
        return tuple(getattr(self, k) for k, _ in self._fields_)


SIM_K = 50
# FASIM_MAX_QUERY (include/fasim_hip.h): longest query of the fastSIM entry points (the reference's 16-bit stage-1 workspace)
MAX_QUERY = 92256
# FASIM_MAX_OLIGO (include/fasim_hip.h): longest oligo of a panel (Engine.scan_oligos)
MAX_OLIGO = 112
# FASIM_MAX_ALLELE / FASIM_MAX_FLANK (include/fasim_hip.h): longest allele and widest flank of a scored variant (Engine.score_variants)
MAX_ALLELE = 1024
MAX_FLANK = 2048
# FASIM_MAX_DELETION_LENGTHS (include/fasim_hip.h): deletion lengths of one Engine.score_deletions() call
MAX_DELETION_LENGTHS = 16


class _Region(C.Structure):
    _fields_ = [("line", C.c_int64), ("start", C.c_int64), ("end", C.c_int64), ("chrom", C.c_char_p), ("name", C.c_char_p)]


class _Variant(C.Structure):
    _fields_ = [("line", C.c_int64), ("pos", C.c_int64), ("rec", C.c_int32), ("ref_len", C.c_int32), ("alt_len", C.c_int32),
                ("chrom", C.c_char_p), ("id", C.c_char_p), ("ref", C.c_char_p), ("alt", C.c_char_p)]


class _VariantScore(C.Structure):
    _fields_ = [("value", (C.c_int32 * 4) * 2), ("enc", (C.c_int32 * 4) * 2), ("flags", C.c_int32), ("reserved", C.c_int32)]


class _VariantWindow(C.Structure):
    _fields_ = [("pre", C.c_int32), ("post", C.c_int32), ("edge", C.c_int32), ("reserved", C.c_int32)]


class _Genotype(C.Structure):
    _fields_ = [("hap", C.c_int8 * 2), ("phased", C.c_uint8), ("pad", C.c_uint8)]


class _HapScore(C.Structure):
    _fields_ = [("hap", _VariantScore * 2), ("carried", C.c_int32 * 2), ("applied", C.c_int32 * 2), ("flags", C.c_int32 * 2)]


class _VariantStats(C.Structure):
    _fields_ = [("problems", C.c_int64), ("cells", C.c_int64), ("kernel_s", C.c_double), ("total_s", C.c_double)]


class _Interval(C.Structure):
    _fields_ = [("rec", C.c_int32), ("reserved", C.c_int32), ("start", C.c_int64), ("end", C.c_int64)]


class _MutScore(C.Structure):
    _fields_ = [("value", (C.c_int32 * 4) * 4), ("enc", (C.c_int8 * 4) * 4), ("ref", C.c_int8), ("clipped", C.c_uint8 * 4),
                ("reserved", C.c_uint8 * 3)]


class _MutagenesisStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("intervals", "positions", "prefix_problems", "problems", "launches", "prefix_cols", "cont_cols",
                                         "cont_cols_bound")] + [(k, C.c_double) for k in ("prefix_s", "cont_s", "total_s")]


class _DelScore(C.Structure):
    _fields_ = [("value", (C.c_int32 * 4) * 2), ("enc", (C.c_int8 * 4) * 2), ("clipped", C.c_uint8 * 2), ("valid", C.c_uint8),
                ("clean", C.c_uint8), ("reserved", C.c_uint8 * 4)]


class _DeletionStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("intervals", "positions", "deletions", "launches", "prefix_problems", "prefix_cols", "own_problems",
                                         "alt_problems", "cont_cols", "cont_cols_bound")] + [(k, C.c_double) for k in ("prefix_s", "cont_s", "total_s")]


class _Result(C.Structure):
    _fields_ = [("recs", C.POINTER(Triplex)), ("count", C.c_int64), ("pool", C.POINTER(C.c_char)), ("pool_len", C.c_int64),
                ("stats", ScanStats)]


class _Track(C.Structure):
    _fields_ = [("nbins", C.c_int64), ("bin", C.c_int32), ("v", C.POINTER(C.c_uint16) * 4), ("units", C.c_int64),
                ("saturated_units", C.c_int64)]


class _TfoProfile(C.Structure):
    _fields_ = [("m", C.c_int32), ("v", C.POINTER(C.c_uint16) * 4), ("units", C.c_int64), ("saturated_units", C.c_int64)]


class _Peak(C.Structure):
    _fields_ = [("value", C.c_int32), ("enc", C.c_int32), ("pos", C.c_int64)]


class _Site(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("pos", C.c_int64), ("value", C.c_int32), ("enc", C.c_int32),
                ("cls", C.c_int32), ("reserved", C.c_int32)]


class _Sites(C.Structure):
    _fields_ = [("n", C.c_int64), ("s", C.POINTER(_Site)), ("units", C.c_int64), ("saturated_units", C.c_int64),
                ("raw_runs", C.c_int64), ("min_value", C.c_int32), ("max_gap", C.c_int32)]


class _SiteHits(C.Structure):
    _fields_ = [("n", C.c_int64), ("t", C.POINTER(Triplex)), ("q_begin", C.POINTER(C.c_int32)), ("q_end", C.POINTER(C.c_int32)),
                ("t_begin", C.POINTER(C.c_int32)), ("t_end", C.POINTER(C.c_int32)), ("cigar_off", C.POINTER(C.c_int64)),
                ("cigar_len", C.POINTER(C.c_int32)), ("cigar", C.POINTER(C.c_uint32)), ("pool", C.POINTER(C.c_char)),
                ("pool_len", C.c_int64), ("unaligned", C.c_int64)]


class _HistEdge(C.Structure):
    _fields_ = [("record", C.c_int32), ("side", C.c_int32), ("boundary", C.c_int64), ("len", C.c_int32), ("reserved", C.c_int32),
                ("v", C.POINTER(C.c_uint16))]


class _Hist(C.Structure):
    _fields_ = [("n", C.POINTER(C.c_int64) * 4), ("positions", C.c_int64), ("units", C.c_int64), ("saturated_units", C.c_int64),
                ("npending", C.c_int64), ("pending", C.POINTER(_HistEdge))]


class _SiteCountsEdge(C.Structure):
    _fields_ = [("record", C.c_int32), ("side", C.c_int32), ("boundary", C.c_int64), ("len", C.c_int32), ("link", C.c_int32),
                ("nb", C.c_uint16 * 4), ("v", C.POINTER(C.c_uint16))]


class _SiteCounts(C.Structure):
    _fields_ = [("n", C.POINTER(C.c_int64) * 4), ("pairs", C.POINTER(C.c_int64) * 4), ("positions", C.c_int64), ("npairs", C.c_int64),
                ("units", C.c_int64), ("saturated_units", C.c_int64), ("npending", C.c_int64), ("pending", C.POINTER(_SiteCountsEdge))]


# FASIM_HIST_BINS (include/fasim_hip.h): values of a potential histogram; HIST_LDS_BINS (csrc/kernels.h): values below it are counted
# in k_hist's workgroup histogram first, HIST_PAIR_LDS_BINS the same for the two histograms of k_hist_pairs
HIST_BINS = 16384
HIST_LDS_BINS = 1024
HIST_PAIR_LDS_BINS = 512

TRACK_CLASSES = ("ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus")

EXPORTS = ["fasim_params_default", "fasim_engine_create", "fasim_engine_create_ex", "fasim_engine_destroy", "fasim_last_error", "fasim_set_option", "fasim_set_query",
           "fasim_calc_score_once", "fasim_ssw_pre_align", "fasim_ssw_colmax_word", "fasim_pick_candidates", "fasim_ssw_align", "fasim_pre_align_batch",
           "fasim_align_batch", "fasim_align_batch_ex", "fasim_encode_unit", "fasim_sim_forward_batch", "fasim_sim_finish_unit", "fasim_scan", "fasim_scan_queries", "fasim_scan_records", "fasim_merge_results", "fasim_rebase_offsets", "fasim_load_dna", "fasim_result_free", "fasim_segment_count",
           "fasim_tfosorted", "fasim_tfoclass", "fasim_tfosorted_ex", "fasim_tfoclass_ex", "fasim_tail_outputs", "fasim_upper_case", "fasim_free",
           "fasim_synth_dna", "fasim_selfcheck_records", "fasim_read_bed", "fasim_maximum3_f16",
           "fasim_scan_track", "fasim_track_merge", "fasim_track_bedgraph", "fasim_track_free",
           "fasim_scan_records_track", "fasim_peaks_merge", "fasim_screen_tsv",
           "fasim_scan_tfo_profile", "fasim_tfo_profile_merge", "fasim_tfo_profile_tsv", "fasim_tfo_profile_free",
           "fasim_scan_records_sites", "fasim_sites_merge", "fasim_sites_bed", "fasim_sites_free",
           "fasim_scan_records_sites_aligned", "fasim_site_hits_merge", "fasim_site_hits_tsv", "fasim_site_hits_free",
           "fasim_scan_oligos", "fasim_oligo_panel_tsv", "fasim_scan_oligos_aligned", "fasim_scan_oligos_profile", "fasim_scan_oligos_peaks",
           "fasim_scan_records_hist", "fasim_scan_oligos_hist", "fasim_hist_merge", "fasim_hist_free", "fasim_shuffle_query",
           "fasim_hist_threshold", "fasim_hist_tsv",
           "fasim_scan_records_site_counts", "fasim_scan_oligos_site_counts", "fasim_site_counts_merge", "fasim_site_counts_free",
           "fasim_shuffle_query_dinuc", "fasim_site_counts_threshold", "fasim_site_counts_tsv",
           "fasim_read_vcf", "fasim_score_variants", "fasim_variants_tsv",
           "fasim_score_variants_aligned", "fasim_variant_hit_span", "fasim_variant_hits_tsv",
           "fasim_read_vcf_sample", "fasim_haplotype_window", "fasim_haplotype_info", "fasim_score_haplotypes", "fasim_haplotypes_tsv",
           "fasim_score_mutagenesis", "fasim_mutagenesis_tsv", "fasim_score_deletions", "fasim_deletions_tsv",
           # the reference's own ssw.h ABI (include/ssw.h)
           "ssw_init", "init_destroy", "ssw_pre_align", "ssw_align", "align_destroy", "encoded_ops"]

_lib = None
_EMPTY_POOL = C.create_string_buffer(1)


def lib():
    """Load libfasim_hip.so (fails loudly when it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FasimError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    L.fasim_last_error.restype = C.c_char_p
    L.fasim_last_error.argtypes = [C.c_void_p]
    L.fasim_engine_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.fasim_engine_destroy.argtypes = [C.c_void_p]
    L.fasim_engine_destroy.restype = None
    L.fasim_params_default.argtypes = [C.POINTER(Params)]
    L.fasim_params_default.restype = None
    L.fasim_set_query.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.fasim_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.fasim_calc_score_once.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fasim_ssw_pre_align.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fasim_pick_candidates.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_int32, C.POINTER(C.c_int32)]
    L.fasim_ssw_align.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(Alignment)]
    L.fasim_pre_align_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.fasim_align_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
                                    C.POINTER(Alignment)]
    L.fasim_align_batch_ex.argtypes = L.fasim_align_batch.argtypes + [C.POINTER(C.c_int32)]
    L.fasim_encode_unit.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p]
    L.fasim_sim_finish_unit.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                        C.POINTER(SimNode), C.c_int32, C.POINTER(C.POINTER(_Result))]
    L.fasim_sim_forward_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
                                          C.POINTER(C.c_int64), C.POINTER(SimNode), C.POINTER(C.c_int32)]
    L.fasim_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(Params),
                             C.POINTER(C.POINTER(_Result))]
    L.fasim_load_dna.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.fasim_scan_queries.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p, C.c_int64,
                                     C.c_int64, C.c_int64, C.POINTER(Params), C.POINTER(C.POINTER(_Result))]
    L.fasim_scan_records.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                     C.POINTER(C.POINTER(_Result)), C.POINTER(ScanStats)]
    L.fasim_merge_results.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                      C.c_int32, C.POINTER(C.POINTER(_Result))]
    L.fasim_rebase_offsets.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.fasim_ssw_colmax_word.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fasim_result_free.argtypes = [C.POINTER(_Result)]
    L.fasim_result_free.restype = None
    L.fasim_segment_count.argtypes = [C.c_int64, C.POINTER(Params)]
    L.fasim_segment_count.restype = C.c_int64
    L.fasim_tfosorted.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.POINTER(Params),
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_tfoclass.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p,
                                 C.POINTER(Params), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_tfosorted_ex.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.POINTER(Params),
                                     C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_tfoclass_ex.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p,
                                    C.POINTER(Params), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_tail_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p,
                                     C.POINTER(Params), C.c_int32] + [C.POINTER(C.c_void_p), C.POINTER(C.c_int64)] * 3
    L.fasim_upper_case.argtypes = [C.c_void_p, C.c_int64]
    L.fasim_upper_case.restype = None
    L.fasim_free.argtypes = [C.c_void_p]
    L.fasim_free.restype = None
    L.fasim_synth_dna.argtypes = [C.c_char_p, C.c_int64, C.c_uint64]
    L.fasim_synth_dna.restype = None
    L.fasim_maximum3_f16.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64]
    L.fasim_read_bed.argtypes = [C.c_char_p, C.POINTER(C.POINTER(_Region)), C.POINTER(C.c_int64)]
    L.fasim_scan_track.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p, C.c_int64,
                                   C.c_int64, C.c_int64, C.POINTER(Params), C.c_int32, C.POINTER(C.POINTER(_Result)),
                                   C.POINTER(C.POINTER(_Track))]
    L.fasim_track_merge.argtypes = [C.POINTER(C.POINTER(_Track)), C.c_int32, C.POINTER(C.POINTER(_Track))]
    L.fasim_track_bedgraph.argtypes = [C.POINTER(_Track), C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int32,
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_track_free.argtypes = [C.POINTER(_Track)]
    L.fasim_track_free.restype = None
    L.fasim_scan_records_track.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                           C.POINTER(Params), C.c_int32, C.POINTER(C.POINTER(_Result)),
                                           C.POINTER(C.POINTER(_Track)), C.POINTER(_Peak), C.POINTER(ScanStats)]
    L.fasim_peaks_merge.argtypes = [C.POINTER(C.POINTER(_Peak)), C.c_int32, C.c_int64, C.POINTER(_Peak)]
    L.fasim_screen_tsv.argtypes = [C.POINTER(_Region), C.POINTER(C.c_int64), C.POINTER(_Peak), C.c_int64, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int64)]
    L.fasim_scan_tfo_profile.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                         C.POINTER(Params), C.c_int32, C.POINTER(C.POINTER(_Result)),
                                         C.POINTER(C.POINTER(_TfoProfile)), C.POINTER(ScanStats)]
    L.fasim_tfo_profile_merge.argtypes = [C.POINTER(C.POINTER(_TfoProfile)), C.c_int32, C.POINTER(C.POINTER(_TfoProfile))]
    L.fasim_tfo_profile_tsv.argtypes = [C.POINTER(_TfoProfile), C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_tfo_profile_free.argtypes = [C.POINTER(_TfoProfile)]
    L.fasim_tfo_profile_free.restype = None
    L.fasim_scan_records_sites.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                           C.POINTER(Params), C.c_int32, C.c_int32, C.POINTER(C.POINTER(_Result)),
                                           C.POINTER(C.POINTER(_Sites)), C.POINTER(ScanStats)]
    L.fasim_sites_merge.argtypes = [C.POINTER(C.POINTER(_Sites)), C.c_int32, C.POINTER(C.POINTER(_Sites))]
    L.fasim_sites_bed.argtypes = [C.POINTER(_Sites), C.c_char_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int32,
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_sites_free.argtypes = [C.POINTER(_Sites)]
    L.fasim_sites_free.restype = None
    L.fasim_scan_records_sites_aligned.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                                   C.POINTER(Params), C.c_int32, C.c_int32, C.POINTER(C.POINTER(_Result)),
                                                   C.POINTER(C.POINTER(_Sites)), C.POINTER(C.POINTER(_SiteHits)), C.POINTER(ScanStats)]
    L.fasim_site_hits_merge.argtypes = [C.POINTER(C.POINTER(_Sites)), C.POINTER(C.POINTER(_SiteHits)), C.c_int32,
                                        C.POINTER(C.POINTER(_Sites)), C.POINTER(C.POINTER(_SiteHits))]
    L.fasim_site_hits_tsv.argtypes = [C.POINTER(_Sites), C.POINTER(_SiteHits), C.c_char_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int32,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_site_hits_free.argtypes = [C.POINTER(_SiteHits)]
    L.fasim_site_hits_free.restype = None
    L.fasim_scan_oligos.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                    C.c_int32, C.c_int32, C.POINTER(C.POINTER(_Sites)), C.c_int32, C.POINTER(C.POINTER(_Track)),
                                    C.POINTER(ScanStats)]
    L.fasim_scan_oligos_aligned.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                            C.c_int32, C.c_int32, C.POINTER(C.POINTER(_Sites)), C.POINTER(C.POINTER(_SiteHits)),
                                            C.POINTER(ScanStats)]
    L.fasim_scan_oligos_profile.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                            C.c_int32, C.POINTER(C.POINTER(_TfoProfile)), C.POINTER(ScanStats)]
    L.fasim_scan_oligos_peaks.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Params),
                                          C.c_int32, C.POINTER(C.POINTER(_Track)), C.POINTER(_Peak), C.POINTER(ScanStats)]
    L.fasim_oligo_panel_tsv.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.POINTER(_Sites)), C.c_int32,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_scan_records_hist.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                          C.POINTER(Params), C.POINTER(C.POINTER(_Result)), C.POINTER(C.POINTER(_Hist)),
                                          C.POINTER(ScanStats)]
    L.fasim_scan_oligos_hist.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                         C.POINTER(Params), C.POINTER(C.POINTER(_Hist)), C.POINTER(ScanStats)]
    L.fasim_hist_merge.argtypes = [C.POINTER(C.POINTER(_Hist)), C.c_int32, C.POINTER(C.POINTER(_Hist))]
    L.fasim_hist_free.argtypes = [C.POINTER(_Hist)]
    L.fasim_hist_free.restype = None
    L.fasim_shuffle_query.argtypes = [C.c_char_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p]
    L.fasim_hist_threshold.argtypes = [C.POINTER(_Hist), C.POINTER(C.POINTER(_Hist)), C.c_int32, C.c_double]
    L.fasim_hist_threshold.restype = C.c_int32
    L.fasim_hist_tsv.argtypes = [C.POINTER(_Hist), C.POINTER(C.POINTER(_Hist)), C.c_int32, C.c_uint64, C.c_double, C.c_char_p,
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_scan_records_site_counts.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                                 C.POINTER(Params), C.POINTER(C.POINTER(_Result)), C.POINTER(C.POINTER(_SiteCounts)),
                                                 C.POINTER(ScanStats)]
    L.fasim_scan_oligos_site_counts.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                                C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int64, C.c_int64,
                                                C.POINTER(Params), C.POINTER(C.POINTER(_SiteCounts)), C.POINTER(ScanStats)]
    L.fasim_site_counts_merge.argtypes = [C.POINTER(C.POINTER(_SiteCounts)), C.c_int32, C.POINTER(C.POINTER(_SiteCounts))]
    L.fasim_site_counts_free.argtypes = [C.POINTER(_SiteCounts)]
    L.fasim_site_counts_free.restype = None
    L.fasim_shuffle_query_dinuc.argtypes = [C.c_char_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p]
    L.fasim_site_counts_threshold.argtypes = [C.POINTER(_SiteCounts), C.POINTER(C.POINTER(_SiteCounts)), C.c_int32, C.c_double]
    L.fasim_site_counts_threshold.restype = C.c_int32
    L.fasim_site_counts_tsv.argtypes = [C.POINTER(_SiteCounts), C.POINTER(C.POINTER(_SiteCounts)), C.c_int32, C.c_uint64, C.c_int32,
                                        C.c_double, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_read_vcf.argtypes = [C.c_char_p, C.POINTER(C.POINTER(_Variant)), C.POINTER(C.c_int64)]
    L.fasim_score_variants.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(_Variant), C.c_int64, C.c_int32,
                                       C.POINTER(Params), C.POINTER(_VariantScore), C.POINTER(_VariantStats)]
    L.fasim_score_variants_aligned.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(_Variant), C.c_int64,
                                               C.c_int32, C.POINTER(Params), C.POINTER(_VariantScore), C.POINTER(_VariantStats),
                                               C.POINTER(_VariantWindow), C.POINTER(C.POINTER(_SiteHits))]
    L.fasim_variant_hit_span.argtypes = [C.POINTER(_Variant), C.POINTER(_VariantWindow), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.fasim_variant_hits_tsv.argtypes = [C.POINTER(_Variant), C.POINTER(_VariantScore), C.POINTER(_VariantWindow), C.POINTER(_SiteHits),
                                         C.c_int64, C.c_int32, C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64)]
    L.fasim_variants_tsv.argtypes = [C.POINTER(_Variant), C.POINTER(_VariantScore), C.c_int64, C.c_int32, C.c_char_p,
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_read_vcf_sample.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(_Variant)), C.POINTER(C.c_int64),
                                        C.POINTER(C.POINTER(_Genotype))]
    L.fasim_haplotype_window.argtypes = [C.POINTER(_Variant), C.POINTER(_Genotype), C.c_int64, C.POINTER(C.c_uint8), C.c_int64, C.c_char_p,
                                         C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.fasim_haplotype_info.argtypes = [C.POINTER(_Variant), C.POINTER(_Genotype), C.c_int64, C.POINTER(C.c_uint8), C.c_int64, C.c_char_p,
                                       C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.fasim_score_haplotypes.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(_Variant), C.POINTER(_Genotype),
                                         C.POINTER(C.c_uint8), C.c_int64, C.c_int32, C.POINTER(Params), C.POINTER(_HapScore),
                                         C.POINTER(_VariantStats)]
    L.fasim_haplotypes_tsv.argtypes = [C.POINTER(_Variant), C.POINTER(_Genotype), C.POINTER(_HapScore), C.c_int64, C.c_int32, C.c_char_p,
                                       C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_score_mutagenesis.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(_Interval), C.c_int64, C.c_int32,
                                          C.POINTER(Params), C.POINTER(_MutScore), C.POINTER(_MutagenesisStats)]
    L.fasim_mutagenesis_tsv.argtypes = [C.POINTER(_Region), C.POINTER(C.c_int64), C.c_int64, C.POINTER(_MutScore), C.c_int32, C.c_char_p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.fasim_score_deletions.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_char_p,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(_Interval), C.c_int64, C.c_int32,
                                        C.POINTER(C.c_int32), C.c_int32, C.POINTER(Params), C.POINTER(_DelScore), C.POINTER(_DeletionStats)]
    L.fasim_deletions_tsv.argtypes = [C.POINTER(_Region), C.POINTER(C.c_int64), C.c_int64, C.POINTER(_DelScore), C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    _lib = L
    return L


def default_params(**kw) -> Params:
    p = Params()
    lib().fasim_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class _Native:
    """What the objects over a structure of the library share.  `_native`: a POINTER the library made, released with the class's
    `_free` when the object dies; otherwise `_keep` holds the structure made in Python (at index 1) and the arrays it points into.
    `_keep` set beside `_native` (SiteHits): a structure of the caller's, which the library must not free."""
    _free = None              # name of the library's free function
    _native = None
    _keep = None

    def __del__(self):
        try:
            if self._native is not None and self._keep is None:
                getattr(lib(), self._free)(self._native)
                self._native = None
        except Exception:
            pass

    def pointer(self):
        """POINTER(struct) for the C-ABI; valid while this object lives."""
        return self._native if self._native is not None else C.pointer(self._keep[1])

    @property
    def _t(self):
        return self._native.contents if self._native is not None else self._keep[1]


def _text_call(fn, *args, name=None, code=True):
    """A library function whose last two parameters are (char** text, int64_t* text_len): its text as bytes."""
    L = lib()
    text = C.c_void_p()
    n = C.c_int64()
    rc = fn(*args, C.byref(text), C.byref(n))
    if rc != 0:
        msg = f"{name or fn.__name__} failed ({rc}): {L.fasim_last_error(None).decode()}"
        raise FasimError(msg, rc) if code else FasimError(msg)
    try:
        return C.string_at(text, n.value)
    finally:
        L.fasim_free(text)


def _pack_records(dnas, rec_lens=None, resident_ok=False):
    """The record set of a call as (blob, offs, lens, nrec): `dnas` a list of records or one bytes object (a set of one record).
    dnas None: the resident buffer -- cut into records of rec_lens, or (resident_ok) whole, as the one record the engine knows."""
    if isinstance(dnas, (bytes, bytearray)):
        dnas = [bytes(dnas)]
    if dnas is None and rec_lens is None:
        if not resident_ok:
            raise FasimError("this call needs its records: dnas is None", E_ARG)
        return None, None, None, 1
    lens_l = [len(d) for d in dnas] if dnas is not None else [int(x) for x in rec_lens]
    nrec = len(lens_l)
    offs = (C.c_int64 * max(1, nrec))()
    lens = (C.c_int64 * max(1, nrec))()
    o = 0
    for i, n in enumerate(lens_l):
        offs[i], lens[i] = o, n
        o += n
    return (b"".join(dnas) if dnas is not None else None), offs, lens, nrec


def _pack_spans(seq, spans, who):
    """0-based half-open (start, end) spans of `seq` (None: of the resident buffer) as the records (offs, lens, nrec) of a call."""
    spans = [(int(s), int(e)) for s, e in spans]
    nrec = len(spans)
    if nrec == 0:
        raise FasimError(f"{who} needs at least one span", E_ARG)
    for k, (s, e) in enumerate(spans):
        if s < 0 or e <= s or (seq is not None and e > len(seq)):
            raise FasimError(f"span {k}: ({s}, {e}) is not a non-empty slice of the sequence", E_ARG)
    return (C.c_int64 * nrec)(*[s for s, _ in spans]), (C.c_int64 * nrec)(*[e - s for s, e in spans]), nrec


def _pack_queries(rnas):
    """The queries of a call as (arr, qlens, nq, nqo): rnas None is the engine's own query (nq 0); nqo = max(1, nq) outputs."""
    rnas = list(rnas or [])
    nq = len(rnas)
    nqo = max(1, nq)
    return (C.c_char_p * nqo)(*rnas), (C.c_int32 * nqo)(*[len(r) for r in rnas]), nq, nqo


def _grid(cls, ptrs, nq, nrec):
    """ptrs[q * nrec + r] as objects of `cls`: a list per query of lists per record."""
    return [[cls(_native=ptrs[q * nrec + r]) for r in range(nrec)] for q in range(nq)]


class ScanResult:
    """Records of one scan (or of one shard, or of a merge).  Either a view of a native `fasim_result` (what scan() and
    merge_results() return: nothing is copied) or two Python byte strings (`ScanResult(recs, pool, stats)`)."""

    def __init__(self, recs: bytes | None = b"", pool: bytes | None = b"", stats: dict | None = None, _native=None, _ext=None):
        self.stats = stats if stats is not None else {}
        self._native = _native            # POINTER(_Result) owned by this object
        self._ext = _ext                  # (recs address, count, pool address, pool_len, owner of that memory)
        lazy = _native is not None or _ext is not None
        self._recs = None if lazy else (recs or b"")
        self._pool = None if lazy else (pool or b"")

    def __del__(self):
        try:
            if self._native is not None:
                lib().fasim_result_free(self._native)
                self._native = None
        except Exception:
            pass

    @property
    def count(self) -> int:
        if self._native is not None or self._ext is not None:
            return self.pointers()[1]
        return len(self._recs) // C.sizeof(Triplex)

    @property
    def pool_len(self) -> int:
        return self.pointers()[3] if (self._native is not None or self._ext is not None) else len(self._pool)

    @property
    def recs(self) -> bytes:
        if self._recs is None:
            rp, cnt, _, _ = self.pointers()
            self._recs = C.string_at(rp, cnt * C.sizeof(Triplex)) if cnt else b""
        return self._recs

    @property
    def pool(self) -> bytes:
        if self._pool is None:
            _, _, pp, plen = self.pointers()
            self._pool = C.string_at(pp, plen) if plen else b""
        return self._pool

    def pointers(self):
        """(recs address, count, pool address, pool_len) for the C-ABI; valid while this object lives."""
        if self._ext is not None:
            return self._ext[:4]
        if self._native is not None:
            r = self._native.contents
            return C.cast(r.recs, C.c_void_p).value or 0, int(r.count), C.cast(r.pool, C.c_void_p).value or 0, int(r.pool_len)
        if getattr(self, "_keep", None) is None:      # created once: earlier pointers must stay valid
            self._keep = (C.create_string_buffer(self._recs, max(1, len(self._recs))), C.create_string_buffer(self._pool, max(1, len(self._pool))))
        return C.addressof(self._keep[0]), self.count, C.addressof(self._keep[1]), len(self._pool)

    def triplexes(self):
        recs, pool = self.recs, self.pool
        arr = (Triplex * self.count).from_buffer_copy(recs)
        out = []
        for t in arr:
            tfo = pool[t.tfo_off:pool.index(b"\0", t.tfo_off)]
            tts = pool[t.tts_off:pool.index(b"\0", t.tts_off)]
            out.append((t.stari, t.endi, t.starj, t.endj, t.strand, t.reverse, t.rule, t.nt, int(t.score),
                        C.c_uint32.from_buffer_copy(C.c_float(t.identity)).value,
                        C.c_uint32.from_buffer_copy(C.c_float(t.tri_score)).value, tfo, tts, t.seg, t.enc))
        return out


class Track(_Native):
    """Per-base triplex potential of one record and one lncRNA (struct fasim_track): per strand class (TRACK_CLASSES) and bin
    of `bin` bases the best local alignment score of the lncRNA that ends in the bin, without the candidate threshold.
    Either a native track (what scan_track() and merge_tracks() return) or one made from a (4, nbins) array:
    `Track(values, bin, units=0, saturated_units=0)`."""

    _free = "fasim_track_free"

    def __init__(self, values=None, bin: int = 1, units: int = 0, saturated_units: int = 0, _native=None):
        self._native = _native
        self._keep = None
        if _native is None:
            import numpy as np
            a = np.ascontiguousarray(values, dtype=np.uint16)
            if a.ndim != 2 or a.shape[0] != 4:
                raise FasimError("a track is a (4, nbins) array", E_ARG)
            t = _Track()
            t.nbins, t.bin, t.units, t.saturated_units = a.shape[1], bin, units, saturated_units
            for c in range(4):
                t.v[c] = C.cast(a[c].ctypes.data, C.POINTER(C.c_uint16))
            self._keep = (a, t)

    @property
    def bin(self) -> int:
        return int(self._t.bin)

    @property
    def nbins(self) -> int:
        return int(self._t.nbins)

    @property
    def units(self) -> int:
        return int(self._t.units)

    @property
    def saturated_units(self) -> int:
        return int(self._t.saturated_units)

    def array(self):
        """(4, nbins) numpy uint16 array (a copy), rows in TRACK_CLASSES order."""
        import numpy as np
        t, n = self._t, self.nbins
        out = np.zeros((4, n), dtype=np.uint16)
        for c in range(4):
            if n:
                C.memmove(out[c].ctypes.data, t.v[c], 2 * n)
        return out


def merge_tracks(parts) -> Track:
    """Element-wise maximum of the tracks of one record (fasim_track_merge): shards of a segment range, devices."""
    L = lib()
    parts = list(parts)
    arr = (C.POINTER(_Track) * max(1, len(parts)))(*[t.pointer() for t in parts])
    out = C.POINTER(_Track)()
    rc = L.fasim_track_merge(arr, len(parts), C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_track_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return Track(_native=out)


def track_bedgraph(track: Track, chr_name: str, start_genome: int, dna_len: int, rna_name: str, min_value: int = 1) -> bytes:
    """bedGraph bytes of a potential track (fasim_track_bedgraph): one block per strand class, runs of equal bins joined, bins
    below `min_value` left out; what `fasim --track BIN` writes as <stem>-TFOpotential-<BIN>."""
    L = lib()
    return _text_call(L.fasim_track_bedgraph, track.pointer(), chr_name.encode(), start_genome, dna_len, rna_name.encode(),
                      min_value)


class Hist(_Native):
    """Histogram of the per-base potential of one lncRNA (or oligo, or shuffled control) over a record set (struct fasim_hist):
    per strand class (TRACK_CLASSES) and value v in [0, 16383] the number of covered positions whose potential is v.  Either a
    native histogram (what scan_hist(), scan_oligos_hist() and merge_hists() return) or one made from a (4, 16384) array:
    `Hist(counts, positions=None, units=0, saturated_units=0, pending=())`, positions defaulting to the sum of class 0 and
    `pending` a list of (record, boundary, side, values) with values a (4, len) array."""

    _free = "fasim_hist_free"

    def __init__(self, counts=None, positions=None, units: int = 0, saturated_units: int = 0, pending=(), _native=None):
        self._native = _native
        self._keep = None
        if _native is None:
            import numpy as np
            a = np.ascontiguousarray(counts, dtype=np.int64)
            if a.shape != (4, HIST_BINS):
                raise FasimError(f"a histogram is a (4, {HIST_BINS}) array", E_ARG)
            t = _Hist()
            t.positions = int(a[0].sum()) if positions is None else positions
            t.units, t.saturated_units = units, saturated_units
            for c in range(4):
                t.n[c] = C.cast(a[c].ctypes.data, C.POINTER(C.c_int64))
            pend = sorted(((int(r), int(b), int(sd), np.ascontiguousarray(v, dtype=np.uint16)) for r, b, sd, v in pending),
                          key=lambda e: e[:3])
            edges = (_HistEdge * max(1, len(pend)))()
            for k, (r, b, sd, v) in enumerate(pend):
                if v.ndim != 2 or v.shape[0] != 4:
                    raise FasimError("the values of a pending edge are a (4, len) array", E_ARG)
                edges[k].record, edges[k].boundary, edges[k].side, edges[k].len = r, b, sd, v.shape[1]
                edges[k].v = C.cast(v.ctypes.data, C.POINTER(C.c_uint16))
            t.npending, t.pending = len(pend), C.cast(edges, C.POINTER(_HistEdge))
            self._keep = (a, t, pend, edges)

    @property
    def positions(self) -> int:
        return int(self._t.positions)

    @property
    def units(self) -> int:
        return int(self._t.units)

    @property
    def saturated_units(self) -> int:
        return int(self._t.saturated_units)

    @property
    def pending(self):
        """[(record, boundary, side, values)]: the boundaries whose other segment lay outside the call's range, ordered; values is
        a (4, len) uint16 array (a copy) of the potential of this range at the positions of the overlap."""
        import numpy as np
        t = self._t
        out = []
        for k in range(int(t.npending)):
            e = t.pending[k]
            v = np.zeros((4, e.len), dtype=np.uint16)
            if e.len:
                C.memmove(v.ctypes.data, e.v, 2 * 4 * e.len)
            out.append((int(e.record), int(e.boundary), int(e.side), v))
        return out

    def array(self):
        """(4, 16384) numpy int64 array (a copy), rows in TRACK_CLASSES order."""
        import numpy as np
        out = np.zeros((4, HIST_BINS), dtype=np.int64)
        for c in range(4):
            C.memmove(out[c].ctypes.data, self._t.n[c], 8 * HIST_BINS)
        return out


def merge_hists(parts) -> Hist:
    """The histogram of a record set from those of its shards (fasim_hist_merge): counts are summed, and where both sides of a
    boundary are pending the positions of the overlap are counted once with the maximum of the two."""
    L = lib()
    parts = list(parts)
    arr = (C.POINTER(_Hist) * max(1, len(parts)))(*[t.pointer() for t in parts])
    out = C.POINTER(_Hist)()
    rc = L.fasim_hist_merge(arr, len(parts), C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_hist_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return Hist(_native=out)


def shuffle_query(rna: bytes, seed: int, k: int) -> bytes:
    """Control k (1-based) of a query under `seed` (fasim_shuffle_query): a Fisher-Yates shuffle of its bytes, splitmix64."""
    L = lib()
    rna = bytes(rna)
    out = C.create_string_buffer(max(1, len(rna)))
    rc = L.fasim_shuffle_query(rna, len(rna), seed & 0xFFFFFFFFFFFFFFFF, k, out)
    if rc != 0:
        raise FasimError(f"fasim_shuffle_query failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return out.raw[:len(rna)]


def _hist_ptrs(controls):
    controls = list(controls)
    return controls, (C.POINTER(_Hist) * max(1, len(controls)))(*[t.pointer() for t in controls])


def hist_threshold(real: Hist, controls=(), fdr: float = 0.05) -> int:
    """The smallest potential from which on the controls reach at most `fdr` times what the query reaches, per control
    (fasim_hist_threshold); 0 when there is none.  What `fasim --potential-hist` reports as min_value."""
    L = lib()
    controls, arr = _hist_ptrs(controls)
    v = L.fasim_hist_threshold(real.pointer(), arr, len(controls), fdr)
    if v < 0:
        raise FasimError(f"fasim_hist_threshold failed ({v}): {L.fasim_last_error(None).decode()}", v)
    return int(v)


def hist_tsv(real: Hist, rna_name: str, controls=(), seed: int = 0, fdr: float = 0.05) -> bytes:
    """The table of `fasim --potential-hist` (fasim_hist_tsv): per value the counts and the counts at or above it per class and,
    with controls, those of the controls and the false discovery rate."""
    L = lib()
    controls, arr = _hist_ptrs(controls)
    return _text_call(L.fasim_hist_tsv, real.pointer(), arr, len(controls), seed & 0xFFFFFFFFFFFFFFFF, fdr, rna_name.encode())


class SiteCounts(_Native):
    """Positions and pairs of neighbouring positions per strand class and potential of one lncRNA (or oligo, or control) over a
    record set (struct fasim_site_counts): n is Hist's, pairs[c][w] the number of pairs (x - 1, x) of one record with
    min(P[x - 1], P[x]) == w, and sites()[c][v] the number of sites `scan_sites(min_value=v, max_gap=0)` reports for class c.  Either
    native (what scan_site_counts(), scan_oligos_site_counts() and merge_site_counts() return) or made from a (2, 4, 16384) array:
    `SiteCounts(counts, positions=None, npairs=None, units=0, saturated_units=0, pending=())`, positions and npairs defaulting to
    the sums of class 0 and `pending` a list of (record, boundary, side, values, nb, link): values a (4, len) array, nb the four
    values of the position next to the zone and link 0 / 1 / 2 (fasim_site_counts_edge)."""

    _free = "fasim_site_counts_free"

    def __init__(self, counts=None, positions=None, npairs=None, units: int = 0, saturated_units: int = 0, pending=(), _native=None):
        self._native = _native
        self._keep = None
        if _native is None:
            import numpy as np
            a = np.ascontiguousarray(counts, dtype=np.int64)
            if a.shape != (2, 4, HIST_BINS):
                raise FasimError(f"site counts are a (2, 4, {HIST_BINS}) array", E_ARG)
            t = _SiteCounts()
            t.positions = int(a[0, 0].sum()) if positions is None else positions
            t.npairs = int(a[1, 0].sum()) if npairs is None else npairs
            t.units, t.saturated_units = units, saturated_units
            for c in range(4):
                t.n[c] = C.cast(a[0, c].ctypes.data, C.POINTER(C.c_int64))
                t.pairs[c] = C.cast(a[1, c].ctypes.data, C.POINTER(C.c_int64))
            pend = sorted(((int(r), int(b), int(sd), np.ascontiguousarray(v, dtype=np.uint16), [int(x) for x in nb], int(link))
                           for r, b, sd, v, nb, link in pending), key=lambda e: e[:3])
            edges = (_SiteCountsEdge * max(1, len(pend)))()
            for k, (r, b, sd, v, nb, link) in enumerate(pend):
                if v.ndim != 2 or v.shape[0] != 4 or len(nb) != 4:
                    raise FasimError("the values of a pending edge are a (4, len) array and four neighbour values", E_ARG)
                edges[k].record, edges[k].boundary, edges[k].side, edges[k].len, edges[k].link = r, b, sd, v.shape[1], link
                for c in range(4):
                    edges[k].nb[c] = nb[c]
                edges[k].v = C.cast(v.ctypes.data, C.POINTER(C.c_uint16))
            t.npending, t.pending = len(pend), C.cast(edges, C.POINTER(_SiteCountsEdge))
            self._keep = (a, t, pend, edges)

    positions = property(lambda self: int(self._t.positions))
    npairs = property(lambda self: int(self._t.npairs))
    units = property(lambda self: int(self._t.units))
    saturated_units = property(lambda self: int(self._t.saturated_units))

    @property
    def pending(self):
        """[(record, boundary, side, values, nb, link)]: the boundaries whose other segment lay outside the call's range, ordered."""
        import numpy as np
        t = self._t
        out = []
        for k in range(int(t.npending)):
            e = t.pending[k]
            v = np.zeros((4, e.len), dtype=np.uint16)
            if e.len:
                C.memmove(v.ctypes.data, e.v, 2 * 4 * e.len)
            out.append((int(e.record), int(e.boundary), int(e.side), v, [int(e.nb[c]) for c in range(4)], int(e.link)))
        return out

    def array(self):
        """(2, 4, 16384) numpy int64 array (a copy): [0] the positions (Hist.array()), [1] the pairs; rows in TRACK_CLASSES order."""
        import numpy as np
        out = np.zeros((2, 4, HIST_BINS), dtype=np.int64)
        for c in range(4):
            C.memmove(out[0, c].ctypes.data, self._t.n[c], 8 * HIST_BINS)
            C.memmove(out[1, c].ctypes.data, self._t.pairs[c], 8 * HIST_BINS)
        return out

    def sites(self):
        """(4, 16384) int64: sites()[c][v] = the sum over w >= v of n[c][w] - pairs[c][w], the sites of class c at threshold v >= 1
        with max_gap 0 (column 0 counts the records' covered stretches)."""
        import numpy as np
        a = self.array()
        return np.cumsum((a[0] - a[1])[:, ::-1], axis=1)[:, ::-1].copy()


def merge_site_counts(parts) -> SiteCounts:
    """The site counts of a record set from those of its shards (fasim_site_counts_merge): as merge_hists(), with the pairs inside
    and across the borders of every overlap whose two sides are there."""
    L = lib()
    parts = list(parts)
    arr = (C.POINTER(_SiteCounts) * max(1, len(parts)))(*[t.pointer() for t in parts])
    out = C.POINTER(_SiteCounts)()
    rc = L.fasim_site_counts_merge(arr, len(parts), C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_site_counts_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return SiteCounts(_native=out)


def shuffle_query_dinuc(rna: bytes, seed: int, k: int) -> bytes:
    """Control k (1-based) of a query under `seed` that keeps every dinucleotide count and both end bytes
    (fasim_shuffle_query_dinuc): a random Euler path, splitmix64 as shuffle_query()."""
    L = lib()
    rna = bytes(rna)
    out = C.create_string_buffer(max(1, len(rna)))
    rc = L.fasim_shuffle_query_dinuc(rna, len(rna), seed & 0xFFFFFFFFFFFFFFFF, k, out)
    if rc != 0:
        raise FasimError(f"fasim_shuffle_query_dinuc failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return out.raw[:len(rna)]


def _site_counts_ptrs(controls):
    controls = list(controls)
    return controls, (C.POINTER(_SiteCounts) * max(1, len(controls)))(*[t.pointer() for t in controls])


def site_counts_threshold(real: SiteCounts, controls=(), fdr: float = 0.05) -> int:
    """hist_threshold() on sites instead of positions (fasim_site_counts_threshold); 0 when there is none."""
    L = lib()
    controls, arr = _site_counts_ptrs(controls)
    v = L.fasim_site_counts_threshold(real.pointer(), arr, len(controls), fdr)
    if v < 0:
        raise FasimError(f"fasim_site_counts_threshold failed ({v}): {L.fasim_last_error(None).decode()}", v)
    return int(v)


def site_counts_tsv(real: SiteCounts, rna_name: str, controls=(), seed: int = 0, fdr: float = 0.05, shuffle: str = "mono") -> bytes:
    """The table of `fasim --potential-hist --hist-sites` (fasim_site_counts_tsv): per value the sites per class and, with controls,
    those of the controls and the false discovery rate per site."""
    L = lib()
    if shuffle not in ("mono", "di"):
        raise FasimError(f"site_counts_tsv: shuffle = {shuffle!r} is neither 'mono' nor 'di'", E_ARG)
    controls, arr = _site_counts_ptrs(controls)
    return _text_call(L.fasim_site_counts_tsv, real.pointer(), arr, len(controls), seed & 0xFFFFFFFFFFFFFFFF, int(shuffle == "di"), fdr,
                      rna_name.encode())


class TfoProfile(_Native):
    """Per-base profile of one lncRNA (struct fasim_tfo_profile): per strand class (TRACK_CLASSES) and base of the lncRNA the best
    local alignment score that ends on that base, over the scanned records.  Either a native profile (what scan_tfo_profile()
    and merge_tfo_profiles() return) or one made from a (4, m) array: `TfoProfile(values, units=0, saturated_units=0)`."""

    _free = "fasim_tfo_profile_free"

    def __init__(self, values=None, units: int = 0, saturated_units: int = 0, _native=None):
        self._native = _native
        self._keep = None
        if _native is None:
            import numpy as np
            a = np.ascontiguousarray(values, dtype=np.uint16)
            if a.ndim != 2 or a.shape[0] != 4:
                raise FasimError("a profile is a (4, m) array", E_ARG)
            t = _TfoProfile()
            t.m, t.units, t.saturated_units = a.shape[1], units, saturated_units
            for c in range(4):
                t.v[c] = C.cast(a[c].ctypes.data, C.POINTER(C.c_uint16))
            self._keep = (a, t)

    @property
    def m(self) -> int:
        return int(self._t.m)

    @property
    def units(self) -> int:
        return int(self._t.units)

    @property
    def saturated_units(self) -> int:
        return int(self._t.saturated_units)

    def array(self):
        """(4, m) numpy uint16 array (a copy), rows in TRACK_CLASSES order."""
        import numpy as np
        t, n = self._t, self.m
        out = np.zeros((4, n), dtype=np.uint16)
        for c in range(4):
            if n:
                C.memmove(out[c].ctypes.data, t.v[c], 2 * n)
        return out


def merge_tfo_profiles(parts) -> TfoProfile:
    """Element-wise maximum of the profiles of one lncRNA (fasim_tfo_profile_merge): shards of a segment range, devices."""
    L = lib()
    parts = list(parts)
    arr = (C.POINTER(_TfoProfile) * max(1, len(parts)))(*[t.pointer() for t in parts])
    out = C.POINTER(_TfoProfile)()
    rc = L.fasim_tfo_profile_merge(arr, len(parts), C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_tfo_profile_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return TfoProfile(_native=out)


def tfo_profile_tsv(profile: TfoProfile, rna: bytes, rna_name: str = "") -> bytes:
    """The table `fasim --tfo-profile` writes (fasim_tfo_profile_tsv): header `pos base ParaPlus ParaMinus AntiMinus AntiPlus`,
    then one tab-separated line per base of the lncRNA."""
    L = lib()
    if len(rna) != profile.m:
        raise FasimError(f"the lncRNA has {len(rna)} bases, the profile {profile.m}", E_ARG)
    return _text_call(L.fasim_tfo_profile_tsv, profile.pointer(), rna, rna_name.encode())


class Sites(_Native):
    """Sites of one record and one lncRNA above a fixed potential (struct fasim_sites): the ranges of positions whose potential
    in one strand class reaches `min_value`, ranges at most `max_gap` apart joined, each with its peak.  Either a native list
    (what scan_sites() and merge_sites() return) or one made from an (n, 6) array of (cls, start, end, value, pos, enc) rows:
    `Sites(rows, min_value, max_gap=0, units=0, saturated_units=0, raw_runs=0)`."""

    _free = "fasim_sites_free"

    def __init__(self, rows=None, min_value: int = 1, max_gap: int = 0, units: int = 0, saturated_units: int = 0, raw_runs: int = 0,
                 _native=None):
        self._native = _native
        self._keep = None
        if _native is None:
            import numpy as np
            a = np.asarray(rows if rows is not None else [], dtype=np.int64).reshape(-1, 6)
            arr = (_Site * max(1, len(a)))()
            for i, (c, s, e, v, pos, enc) in enumerate(a.tolist()):
                arr[i].cls, arr[i].start, arr[i].end, arr[i].value, arr[i].pos, arr[i].enc = c, s, e, v, pos, enc
            t = _Sites()
            t.n, t.s = len(a), C.cast(arr, C.POINTER(_Site))
            t.units, t.saturated_units, t.raw_runs, t.min_value, t.max_gap = units, saturated_units, raw_runs, min_value, max_gap
            self._keep = (arr, t)

    @property
    def n(self) -> int:
        return int(self._t.n)

    def __len__(self) -> int:
        return self.n

    @property
    def units(self) -> int:
        return int(self._t.units)

    @property
    def saturated_units(self) -> int:
        return int(self._t.saturated_units)

    @property
    def raw_runs(self) -> int:
        return int(self._t.raw_runs)

    @property
    def min_value(self) -> int:
        return int(self._t.min_value)

    @property
    def max_gap(self) -> int:
        return int(self._t.max_gap)

    def array(self):
        """(n, 6) numpy int64 array (a copy) of (cls, start, end, value, pos, enc), ordered by (start, cls)."""
        import numpy as np
        t, n = self._t, self.n
        out = np.zeros((n, 6), dtype=np.int64)
        if n:
            raw = np.frombuffer(C.string_at(t.s, n * C.sizeof(_Site)), dtype=np.dtype(
                [("start", "<i8"), ("end", "<i8"), ("pos", "<i8"), ("value", "<i4"), ("enc", "<i4"), ("cls", "<i4"), ("reserved", "<i4")]))
            for k, f in enumerate(("cls", "start", "end", "value", "pos", "enc")):
                out[:, k] = raw[f]
        return out


def merge_sites(parts) -> Sites:
    """The site list of one record from those of its shards (fasim_sites_merge): union of the intervals per class, joined by
    max_gap again; units, saturated_units and raw_runs summed."""
    L = lib()
    parts = list(parts)
    arr = (C.POINTER(_Sites) * max(1, len(parts)))(*[t.pointer() for t in parts])
    out = C.POINTER(_Sites)()
    rc = L.fasim_sites_merge(arr, len(parts), C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_sites_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return Sites(_native=out)


def sites_bed(sites: Sites, chr_name: str, start_genome: int, rna_name: str, record_name: str | None = None, header: bool = True) -> bytes:
    """BED bytes of a site list (fasim_sites_bed): chrom, start, end, class, value, strand, peak, rule and, where record_name is
    given, the record's name; what `fasim --sites V` writes."""
    L = lib()
    return _text_call(L.fasim_sites_bed, sites.pointer(), chr_name.encode(), start_genome, rna_name.encode(),
                      record_name.encode() if record_name is not None else None, 1 if header else 0)


def oligo_panel_tsv(names, oligos, sites) -> bytes:
    """The panel table of Engine.scan_oligos() (fasim_oligo_panel_tsv): per oligo its name, length, number of sites and covered
    bases over all records and classes, and per strand class the number of sites and the largest value (0 without a site).
    `sites`: the list per oligo of lists per record that scan_oligos() returns; what `fasim --oligos --sites V` writes."""
    L = lib()
    names, oligos, sites = list(names), list(oligos), [list(row) for row in sites]
    nq = len(names)
    if len(oligos) != nq or len(sites) != nq:
        raise FasimError("oligo_panel_tsv: names, oligos and sites differ in length", E_ARG)
    nrec = len(sites[0]) if nq else 1
    if any(len(row) != nrec for row in sites):
        raise FasimError("oligo_panel_tsv: every oligo needs one site list per record", E_ARG)
    flat = [t for row in sites for t in row]
    arr = (C.POINTER(_Sites) * max(1, len(flat)))(*[t.pointer() for t in flat])
    nm = (C.c_char_p * max(1, nq))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
    lens = (C.c_int32 * max(1, nq))(*[len(o) for o in oligos])
    return _text_call(L.fasim_oligo_panel_tsv, nm, lens, nq, arr, nrec)


class SiteHits(_Native):
    """The hits of the sites of one record and one lncRNA (struct fasim_site_hits): hit k is the alignment behind the peak of site
    k of the Sites object of the same call.  What scan_sites_aligned() and merge_site_hits() return."""

    _free = "fasim_site_hits_free"

    def __init__(self, _native, _keep=None):
        self._native = _native
        self._keep = _keep               # not None: a structure made by the caller, which the library must not free

    @property
    def n(self) -> int:
        return int(self._t.n)

    def __len__(self) -> int:
        return self.n

    @property
    def unaligned(self) -> int:
        return int(self._t.unaligned)

    def array(self):
        """(n, 8) numpy int64 array (a copy) of (seg, enc, i0, i1, j0, j1, nt, cigar_len); i0 .. j1 are the unit-relative cells of
        the hit's first and last pair, cigar_len -1 marks an unaligned hit."""
        import numpy as np
        t, n = self._t, self.n
        out = np.zeros((n, 8), dtype=np.int64)
        for k in range(n):
            r = t.t[k]
            out[k] = (r.seg, r.enc, t.q_begin[k], t.q_end[k], t.t_begin[k], t.t_end[k], r.nt, t.cigar_len[k])
        return out

    def cigars(self):
        """One CIGAR string per hit ("40M2I40M"; I = a lncRNA base against a gap, D = a DNA base against a gap), "" when unaligned."""
        t = self._t
        out = []
        for k in range(self.n):
            n, o = int(t.cigar_len[k]), int(t.cigar_off[k])
            out.append("".join(f"{t.cigar[o + i] >> 4}{'MID'[t.cigar[o + i] & 15]}" for i in range(max(0, n))))
        return out

    def triplexes(self):
        """One dict per hit with the fields of a ScanResult record (stari ... tri_score, seg, enc, tfo, tts)."""
        t = self._t
        out = []
        for k in range(self.n):
            r = t.t[k]
            d = {f: getattr(r, f) for f, _ in Triplex._fields_ if f not in ("tfo_off", "tts_off", "genome_shift")}
            d["tfo"] = C.string_at(C.addressof(t.pool.contents) + r.tfo_off).decode()
            d["tts"] = C.string_at(C.addressof(t.pool.contents) + r.tts_off).decode()
            out.append(d)
        return out


def merge_site_hits(sites_parts, hits_parts):
    """Shards of one record (fasim_site_hits_merge): `(Sites, SiteHits)` of the unsharded call from the shards' site lists and
    hits.  Where intervals unite, the part whose site wins supplies the hit; on a full tie the hit of the smaller segment."""
    L = lib()
    sites_parts, hits_parts = list(sites_parts), list(hits_parts)
    if len(sites_parts) != len(hits_parts):
        raise FasimError("merge_site_hits: as many hit lists as site lists are needed", E_ARG)
    n = len(sites_parts)
    sa = (C.POINTER(_Sites) * max(1, n))(*[t.pointer() for t in sites_parts])
    ha = (C.POINTER(_SiteHits) * max(1, n))(*[t.pointer() for t in hits_parts])
    so, ho = C.POINTER(_Sites)(), C.POINTER(_SiteHits)()
    rc = L.fasim_site_hits_merge(sa, ha, n, C.byref(so), C.byref(ho))
    if rc != 0:
        raise FasimError(f"fasim_site_hits_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return Sites(_native=so), SiteHits(ho)


def site_hits_tsv(sites: Sites, hits: SiteHits, chr_name: str, start_genome: int, rna_name: str, record_name: str | None = None,
                  header: bool = True) -> bytes:
    """The table of `fasim --sites V --sites-align` (fasim_site_hits_tsv): one line per site with its hit."""
    L = lib()
    return _text_call(L.fasim_site_hits_tsv, sites.pointer(), hits.pointer(), chr_name.encode(), start_genome,
                      rna_name.encode(), record_name.encode() if record_name is not None else None, 1 if header else 0)


def _peaks_to_c(peaks):
    """(..., 3) integer array of (value, pos, enc) -> ctypes array of fasim_peak."""
    import numpy as np
    a = np.ascontiguousarray(peaks, dtype=np.int64).reshape(-1, 3)
    arr = (_Peak * max(1, len(a)))()
    for k, (v, pos, enc) in enumerate(a.tolist()):
        arr[k].value, arr[k].pos, arr[k].enc = v, pos, enc
    return arr, len(a)


def _peaks_from_c(arr, n):
    import numpy as np
    out = np.empty((n, 3), dtype=np.int64)
    for k in range(n):
        out[k] = (arr[k].value, arr[k].pos, arr[k].enc)
    return out


def merge_peaks(parts):
    """Entry-wise merge of peak arrays of one record set (fasim_peaks_merge; shards of a segment range, devices): the larger
    value wins, then the lower pos, then the lower enc.  Arrays of (value, pos, enc) rows of one shape; returns that shape."""
    import numpy as np
    L = lib()
    parts = [np.asarray(x, dtype=np.int64) for x in parts]
    if parts and any(x.shape != parts[0].shape for x in parts):
        raise FasimError("merge_peaks: the parts differ in shape", E_ARG)
    cs = [_peaks_to_c(x) for x in parts]
    n = cs[0][1] if cs else 0
    ptrs = (C.POINTER(_Peak) * max(1, len(cs)))(*[C.cast(a, C.POINTER(_Peak)) for a, _ in cs])
    out = (_Peak * max(1, n))()
    rc = L.fasim_peaks_merge(ptrs, len(cs), n, out)
    if rc != 0:
        raise FasimError(f"fasim_peaks_merge failed ({rc}): {L.fasim_last_error(None).decode()}", rc)
    return _peaks_from_c(out, n).reshape(parts[0].shape)


def screen_tsv(regions, segments, peaks) -> bytes:
    """The bytes of `fasim --screen`'s table (fasim_screen_tsv): `regions` are Region tuples (line, chrom, start, end, name),
    segments[k] the interval's segment count (negative: not scanned, NA line), peaks a (len(regions), 4, 3) array of
    (value, pos within the interval, enc)."""
    L = lib()
    n = len(regions)
    reg = (_Region * max(1, n))()
    for k, g in enumerate(regions):
        reg[k].line, reg[k].start, reg[k].end = g.line, g.start, g.end
        reg[k].chrom, reg[k].name = g.chrom.encode(), g.name.encode()
    segs = (C.c_int64 * max(1, n))(*[int(x) for x in segments])
    pk, npk = _peaks_to_c(peaks)
    if npk != 4 * n:
        raise FasimError("screen_tsv: peaks must hold four (value, pos, enc) rows per interval", E_ARG)
    return _text_call(L.fasim_screen_tsv, reg, segs, pk, n)


def _merge_pointers(ptrs):
    """ptrs: list of (recs address, count, pool address, pool_len) -> native-backed ScanResult (fasim_merge_results)."""
    L = lib()
    n = len(ptrs)
    recs = (C.c_void_p * n)(*[p[0] or None for p in ptrs])
    counts = (C.c_int64 * n)(*[p[1] for p in ptrs])
    pools = (C.c_void_p * n)(*[p[2] or None for p in ptrs])
    plens = (C.c_int64 * n)(*[p[3] for p in ptrs])
    out = C.POINTER(_Result)()
    rc = L.fasim_merge_results(recs, counts, pools, plens, n, C.byref(out))
    if rc != 0:
        raise FasimError(f"fasim_merge_results failed ({rc}): {L.fasim_last_error(None).decode()}")
    return ScanResult(stats={}, _native=out)


def merge_results(parts):
    """Concatenate shard results in rank order (shards are contiguous segment ranges, so this IS the canonical
    (segment, encoding, rank) order); pool offsets are rebased.  Native: fasim_merge_results, one pass per shard."""
    parts = list(parts)
    return _merge_pointers([r.pointers() for r in parts])      # `parts` keeps the source buffers alive during the call


def shard_segments(nseg: int, rank: int, world: int):
    """Contiguous block of segment indices for `rank` (blocks differ by at most one segment)."""
    base, rem = divmod(nseg, world)
    first = rank * base + min(rank, rem)
    return first, base + (1 if rank < rem else 0)


GATHER_CHUNK = 256 << 20      # bytes rank 0 stages on the device per transfer (two such buffers)


def _pieces(sizes, rsz, tot_r):
    """Transfer plan of gather_results: for every source rank k > 0 its records and its pool cut into pieces of at most
    GATHER_CHUNK bytes: (k, offset in the sender's staging buffer, offset in the merged buffer, length)."""
    out, roff, poff = [], 0, 0
    for k, (a, b) in enumerate(sizes):
        if k > 0:
            for src0, dst0, n in ((0, roff, a), (a, tot_r + poff, b)):
                o = 0
                while o < n:
                    ln = min(GATHER_CHUNK, n - o)
                    out.append((k, src0 + o, dst0 + o, ln))
                    o += ln
        roff += a
        poff += b
    return out


def gather_results(res: ScanResult, dist, rank: int, world: int, device: str = "cuda"):
    """The path's only exchange step: every rank contributes the records of its segment shard, rank 0 gets them
    merged in rank order (= canonical (segment, encoding, rank) order because shards are contiguous).
    One all_gather of (records bytes, pool bytes), then point-to-point transfers (RCCL send/recv over xGMI; gloo in
    the CPU tests) that put every shard's records and pool at their final positions of ONE pinned host buffer on rank 0;
    the pool offsets are then rebased in place (fasim_rebase_offsets).  No per-record work in Python and no second copy
    of the merged records.  On the GPU path rank 0 never stages more than 2 x GATHER_CHUNK bytes on its device: piece i + 1
    is received into one staging buffer while piece i leaves the other one for the host (at hg38 scale the merged records
    are 4-5 GB)."""
    import torch
    if world == 1:
        return res
    L = lib()
    rp, cnt, pp, plen = res.pointers()
    rsz = C.sizeof(Triplex)
    nr = cnt * rsz
    gathered = [torch.zeros(2, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(gathered, torch.tensor([nr, plen], dtype=torch.int64, device=device))
    sizes = [(int(s[0]), int(s[1])) for s in gathered]
    tot_r = sum(a for a, _ in sizes)
    tot_p = sum(b for _, b in sizes)
    plan = _pieces(sizes, rsz, tot_r)
    gpu = device != "cpu"
    if rank != 0:
        stage = torch.empty(max(1, nr + plen), dtype=torch.uint8, pin_memory=gpu)
        if nr:
            C.memmove(stage.data_ptr(), rp, nr)
        if plen:
            C.memmove(stage.data_ptr() + nr, pp, plen)
        mine = stage.to(device, non_blocking=True) if gpu else stage
        for k, src, _dst, ln in plan:
            if k == rank:
                dist.send(mine[src:src + ln], 0)
        return None
    host = torch.empty(max(1, tot_r + tot_p), dtype=torch.uint8, pin_memory=gpu)       # [records of all shards][pools of all shards]
    base = host.data_ptr()
    if nr:
        C.memmove(base, rp, nr)                      # rank 0's own shard: host to host
    if plen:
        C.memmove(base + tot_r, pp, plen)
    if not gpu:
        for k, _src, dst, ln in plan:
            dist.recv(host[dst:dst + ln], k)
    elif plan:
        bufs = [torch.empty(min(GATHER_CHUNK, max(ln for _, _, _, ln in plan)), dtype=torch.uint8, device=device) for _ in range(2)]
        copy_stream = torch.cuda.Stream()
        freed = [None, None]                         # event: the buffer's previous piece has left for the host
        for i, (k, _src, dst, ln) in enumerate(plan):
            b = i & 1
            if freed[b] is not None:
                freed[b].synchronize()
            dist.recv(bufs[b][:ln], k)               # (RCCL recv is ordered on the current stream)
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ready)
                host[dst:dst + ln].copy_(bufs[b][:ln], non_blocking=True)
                freed[b] = torch.cuda.Event()
                freed[b].record()
        copy_stream.synchronize()
    roff = poff = 0
    for a, b in sizes:
        if a and poff:
            L.fasim_rebase_offsets(base + roff, a // rsz, poff)
        roff += a
        poff += b
    return ScanResult(stats={}, _ext=(base, tot_r // rsz, base + tot_r, tot_p, host))


class Engine:
    """One engine per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.fasim_engine_create(device, C.byref(h))
        if rc != 0:
            raise FasimError(f"fasim_engine_create({device}) failed ({rc}): {self._L.fasim_last_error(None).decode()}")
        self._h = h
        self.m = 0
        self.rna = None                   # the query as last given to set_query() (scan_hist() shuffles it for its controls)

    def close(self):
        if getattr(self, "_h", None):
            self._L.fasim_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise FasimError(f"libfasim_hip error {rc}: {self._L.fasim_last_error(self._h).decode()}", rc)

    def set_option(self, key: str, value: int):
        self._check(self._L.fasim_set_option(self._h, key.encode(), value))

    def set_query(self, rna: bytes):
        self._check(self._L.fasim_set_query(self._h, rna, len(rna)))
        self.m = len(rna)
        self.rna = bytes(rna)

    def maximum3_f16(self, a, b, c):
        """v_pk_maximum3_f16 on numpy uint32 arrays of packed f16 pairs: (maximum3(a, b, c), maximum3(a, b, +0))."""
        import numpy as np
        a, b, c = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, b, c))
        out3, out0 = np.empty_like(a), np.empty_like(a)
        self._check(self._L.fasim_maximum3_f16(self._h, a.ctypes.data, b.ctypes.data, c.ctypes.data, out3.ctypes.data,
                                               out0.ctypes.data, a.size))
        return out3, out0

    # --- single-problem drop-ins ------------------------------------------------------------------
    def calc_score_once(self, target: bytes) -> int:
        s = C.c_int32()
        self._check(self._L.fasim_calc_score_once(self._h, target, len(target), C.byref(s)))
        return s.value

    def ssw_pre_align(self, target: bytes):
        out = (C.c_int32 * len(target))()
        self._check(self._L.fasim_ssw_pre_align(self._h, target, len(target), out))
        return list(out)

    def ssw_align(self, window: bytes) -> Alignment:
        a = Alignment()
        self._check(self._L.fasim_ssw_align(self._h, window, len(window), C.byref(a)))
        return a

    # --- batched ----------------------------------------------------------------------------------
    @staticmethod
    def _pack(seqs):
        blob = b"".join(seqs)
        n = len(seqs)
        offs = (C.c_int64 * n)()
        lens = (C.c_int32 * n)()
        o = 0
        for i, s in enumerate(seqs):
            offs[i] = o
            lens[i] = len(s)
            o += len(s)
        return blob, offs, lens

    def pre_align_batch(self, targets, want_cols=True, want_stage1=True):
        blob, offs, lens = self._pack(targets)
        cols = (C.c_int32 * len(blob))() if want_cols else None
        s1 = (C.c_int32 * len(targets))() if want_stage1 else None
        self._check(self._L.fasim_pre_align_batch(self._h, blob, offs, lens, len(targets), cols, s1))
        out_cols = None
        if want_cols:
            out_cols, o = [], 0
            for t in targets:
                out_cols.append(list(cols[o:o + len(t)]))
                o += len(t)
        return out_cols, (list(s1) if want_stage1 else None)

    def align_batch(self, windows, paths=False):
        """ssw_align of every window.  paths=True: also, per window, what produced its alignment (fasim_align_batch_ex): 0 nothing
        aligned, 1 ... 4 the finish tier (16 KB LDS, 64 KB LDS, 16 KB and 1 MB of global scratch), 5 the stripe-faithful replay."""
        blob, offs, lens = self._pack(windows)
        out = (Alignment * len(windows))()
        if not paths:
            self._check(self._L.fasim_align_batch(self._h, blob, offs, lens, len(windows), out))
            return list(out)
        how = (C.c_int32 * len(windows))()
        self._check(self._L.fasim_align_batch_ex(self._h, blob, offs, lens, len(windows), out, how))
        return list(out), list(how)

    def sim_forward(self, targets, min_scores):
        """Forward sweep of classic SIM (-F, sim.h:506-571) for a batch of targets: per target the node list it leaves, as
        tuples (score x10, stari, starj, endi, endj, top, bot, left, right) in list order."""
        blob, offs, lens = self._pack(targets)
        n = len(targets)
        mins = (C.c_int64 * n)(*min_scores)
        nodes = (SimNode * (n * SIM_K))()
        counts = (C.c_int32 * n)()
        self._check(self._L.fasim_sim_forward_batch(self._h, blob, offs, lens, n, mins, nodes, counts))
        return [[nodes[k * SIM_K + x].astuple() for x in range(counts[k])] for k in range(n)]

    # --- the LongTarget() body ----------------------------------------------------------------------
    def resident_len(self) -> int:
        """Length of the record set last given to load_dna() (0: none)."""
        return getattr(self, "_resident_len", 0)

    def load_dna(self, dna: bytes):
        """Upload one DNA record and keep it resident in HBM; scan(None, ...) then scans it without H2D copies."""
        self._check(self._L.fasim_load_dna(self._h, dna, len(dna)))
        self._resident_len = len(dna)

    @staticmethod
    def _stats_dict(st) -> dict:
        stats = {}
        for k, _ in ScanStats._fields_:
            v = getattr(st, k)
            stats[k] = list(v) if hasattr(v, "__len__") else v
        return stats

    def _wrap_results(self, outs, nqo, nrec):
        """outs[q * nrec + r] as ScanResults that own them: a list per query of lists per record."""
        return [[ScanResult(stats=self._stats_dict(outs[q * nrec + r].contents.stats), _native=outs[q * nrec + r]) for r in range(nrec)]
                for q in range(nqo)]

    def _totals(self, totals, nq):
        """The call's totals, one stats dict per query, into `self.last_totals`."""
        self.last_totals = [self._stats_dict(totals[q]) for q in range(nq)]

    def scan(self, dna: bytes | None, params: Params | None = None, seg_first: int = 0, seg_count: int = -1) -> ScanResult:
        p = params or default_params()
        res = C.POINTER(_Result)()
        self._check(self._L.fasim_scan(self._h, dna, len(dna) if dna is not None else 0, seg_first, seg_count, C.byref(p),
                                       C.byref(res)))
        return ScanResult(stats=self._stats_dict(res.contents.stats), _native=res)

    def scan_queries(self, rnas, dna: bytes | None, params: Params | None = None, seg_first: int = 0, seg_count: int = -1):
        """Multi-lncRNA batch (fasim_scan_queries): one ScanResult per lncRNA, each identical to what scan() returns for
        that lncRNA alone; the DNA record stays resident and the lncRNAs share one work queue."""
        p = params or default_params()
        arr, lens, n, _ = _pack_queries(rnas)
        outs = (C.POINTER(_Result) * n)()
        self._check(self._L.fasim_scan_queries(self._h, arr, lens, n, dna, len(dna) if dna is not None else 0, seg_first,
                                               seg_count, C.byref(p), outs))
        self.m = len(rnas[-1])
        return [ScanResult(stats=self._stats_dict(outs[k].contents.stats), _native=outs[k]) for k in range(n)]

    def scan_track(self, dna: bytes | None, params: Params | None = None, rnas=None, bin: int = 1, records: bool = True,
                   seg_first: int = 0, seg_count: int = -1):
        """Potential tracks (fasim_scan_track): `(results or None, tracks)`.  rnas None: the engine's query, one ScanResult (the
        same as scan()) and one Track; otherwise lists, one entry per lncRNA, as scan_queries().  records False: track only, stage 3
        is not run and the first element is None.  With a segment range the tracks still span the whole record: merge the
        shards' tracks with merge_tracks()."""
        p = params or default_params()
        arr, qlens, nq, nqo = _pack_queries(rnas)
        outs = (C.POINTER(_Result) * nqo)() if records else None
        trks = (C.POINTER(_Track) * nqo)()
        self._check(self._L.fasim_scan_track(self._h, arr, qlens, nq, dna, len(dna) if dna is not None else 0, seg_first,
                                             seg_count, C.byref(p), bin, outs, trks))
        if nq:
            self.m = len(rnas[-1])
        tracks = [Track(_native=trks[k]) for k in range(nqo)]
        res = [ScanResult(stats=self._stats_dict(outs[k].contents.stats), _native=outs[k]) for k in range(nqo)] if records else None
        if rnas is None:
            return (res[0] if records else None), tracks[0]
        return res, tracks

    def scan_records(self, dnas, params: Params | None = None, rnas=None, seg_first: int = 0, seg_count: int = -1, rec_lens=None):
        """Record set (fasim_scan_records): many DNA records (peaks, promoter windows) scanned in shared batches.
        `dnas`: list of bytes, one per record; None together with `rec_lens` scans the buffer made resident by load_dna() of the
        records' concatenation.  Segments are numbered globally, record after record; seg_first / seg_count select a range.
        rnas None: one ScanResult per record, each identical to scan() of that record alone (the engine's query).  Otherwise a
        list per lncRNA of per-record lists, like scan_queries().  The call's totals (one stats dict per query) are left in
        `self.last_totals`."""
        p = params or default_params()
        if dnas is None and rec_lens is None:
            raise FasimError("scan_records(None, ...) needs rec_lens (the records of the resident buffer)", E_ARG)
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens)
        arr, qlens, nq, nqo = _pack_queries(rnas)
        outs = (C.POINTER(_Result) * (nqo * max(1, nrec)))()
        totals = (ScanStats * nqo)()
        self._check(self._L.fasim_scan_records(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                               outs, totals))
        if nq:
            self.m = len(rnas[-1])
        self._totals(totals, nqo)
        res = self._wrap_results(outs, nqo, nrec)
        return res[0] if rnas is None else res

    def scan_tfo_profile(self, dnas, params: Params | None = None, rnas=None, per_record: bool = False, records: bool = True,
                         seg_first: int = 0, seg_count: int = -1):
        """Per-base profile of the lncRNA (fasim_scan_tfo_profile): `(results | None, profiles)`.  `dnas`: a list of records, or
        one `bytes` (a single record).  rnas None: the engine's query; results is what scan_records() returns (one ScanResult
        per record) and profiles one TfoProfile over the whole set, or with per_record a list, one per record, each what that
        record scanned alone gives.  rnas given: lists per lncRNA of those.  records False: no stage 3, results is None.
        Shards of a segment range merge with merge_tfo_profiles().  Totals: `self.last_totals`."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas)
        arr, qlens, nq, nqo = _pack_queries(rnas)
        nout = nqo * max(1, nrec)
        nprof = nout if per_record else nqo
        outs = (C.POINTER(_Result) * nout)() if records else None
        profs = (C.POINTER(_TfoProfile) * nprof)()
        totals = (ScanStats * nqo)()
        self._check(self._L.fasim_scan_tfo_profile(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                   1 if per_record else 0, outs, profs, totals))
        if nq:
            self.m = len(rnas[-1])
        self._totals(totals, nqo)
        res = None
        if records:
            res = self._wrap_results(outs, nqo, nrec)
        if per_record:
            prof = _grid(TfoProfile, profs, nqo, nrec)
        else:
            prof = [TfoProfile(_native=profs[q]) for q in range(nqo)]
        if rnas is None:
            return (res[0] if res else None), prof[0]
        return res, prof

    def _sites_call(self, aligned, dnas, params, min_value, max_gap, records, rnas, seg_first, seg_count):
        """Argument marshalling and result wrapping shared by scan_sites() and scan_sites_aligned()."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, nqo = _pack_queries(rnas)
        nout = nqo * max(1, nrec)
        outs = (C.POINTER(_Result) * nout)() if records else None
        sts = (C.POINTER(_Sites) * nout)()
        totals = (ScanStats * nqo)()
        if aligned:
            hts = (C.POINTER(_SiteHits) * nout)()
            self._check(self._L.fasim_scan_records_sites_aligned(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count,
                                                                 C.byref(p), min_value, max_gap, outs, sts, hts, totals))
        else:
            self._check(self._L.fasim_scan_records_sites(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                         min_value, max_gap, outs, sts, totals))
        if nq:
            self.m = len(rnas[-1])
        self._totals(totals, nqo)
        res = None
        if records:
            res = self._wrap_results(outs, nqo, nrec)
        out = [res, _grid(Sites, sts, nqo, nrec)]
        if aligned:
            out.append(_grid(SiteHits, hts, nqo, nrec))
        if rnas is None:
            return tuple([(res[0] if res else None)] + [x[0] for x in out[1:]])
        return tuple(out)

    def scan_sites(self, dnas, params: Params | None = None, min_value: int = 1, max_gap: int = 0, records: bool = True, rnas=None,
                   seg_first: int = 0, seg_count: int = -1):
        """Sites above a fixed potential (fasim_scan_records_sites): `(results | None, sites)`.  `dnas`: a list of records, one
        `bytes` (a set of one record) or None (the record made resident by load_dna()).  rnas None: the engine's query; results is
        what scan_records() returns (one ScanResult per record) and sites one Sites per record.  rnas given: lists per lncRNA of
        those.  records False: no stage 3, results is None.  Shards of a segment range merge with merge_sites().  Totals:
        `self.last_totals`."""
        return self._sites_call(False, dnas, params, min_value, max_gap, records, rnas, seg_first, seg_count)

    def scan_sites_aligned(self, dnas, params: Params | None = None, min_value: int = 1, max_gap: int = 0, records: bool = True,
                           rnas=None, seg_first: int = 0, seg_count: int = -1):
        """scan_sites() and the hit of every site (fasim_scan_records_sites_aligned): `(results | None, sites, hits)`.  The first
        two are exactly what scan_sites() returns; hits has the shape of sites, one SiteHits per record (per lncRNA and record
        with rnas given).  Shards of a segment range merge with merge_site_hits()."""
        return self._sites_call(True, dnas, params, min_value, max_gap, records, rnas, seg_first, seg_count)

    def scan_oligos(self, oligos, dnas, params: Params | None = None, min_value: int = 1, max_gap: int = 0, track_bin: int = 0,
                    seg_first: int = 0, seg_count: int = -1):
        """Sites, and with track_bin >= 1 potential tracks, of a panel of short oligos of 1 .. MAX_OLIGO nt (fasim_scan_oligos):
        `sites`, or `(sites, tracks)`, lists per oligo of lists per record of Sites / Track objects -- what scan_sites() and
        scan_records_track() would give for a lncRNA, with the oligo in its place.  `dnas` as for scan_sites().  The engine's own
        query is not touched.  Shards of a segment range merge with merge_sites() / merge_tracks(); the panel table is
        oligo_panel_tsv().  Totals per oligo: `self.last_totals`."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        nout = max(1, nq) * max(1, nrec)
        sts = (C.POINTER(_Sites) * nout)()
        trks = (C.POINTER(_Track) * nout)() if track_bin != 0 else None
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                              min_value, max_gap, sts, track_bin, trks, totals))
        self._totals(totals, nq)
        sites = _grid(Sites, sts, nq, nrec)
        if trks is None:
            return sites
        return sites, _grid(Track, trks, nq, nrec)

    def scan_oligos_aligned(self, oligos, dnas, params: Params | None = None, min_value: int = 1, max_gap: int = 0,
                            seg_first: int = 0, seg_count: int = -1):
        """The sites of a panel of short oligos and the hit of every site (fasim_scan_oligos_aligned): `(sites, hits)`, lists per
        oligo of lists per record of Sites and SiteHits.  sites is exactly what scan_oligos() returns; a hit is what
        scan_sites_aligned() would give for a lncRNA, with the oligo in its place.  `dnas` as for scan_oligos().  Shards of a
        segment range merge with merge_site_hits().  Option site_short = 0 runs the hits on the lncRNAs' kernel (same results)."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        nout = max(1, nq) * max(1, nrec)
        sts = (C.POINTER(_Sites) * nout)()
        hts = (C.POINTER(_SiteHits) * nout)()
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos_aligned(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                      min_value, max_gap, sts, hts, totals))
        self._totals(totals, nq)
        return _grid(Sites, sts, nq, nrec), _grid(SiteHits, hts, nq, nrec)

    def scan_oligos_profile(self, oligos, dnas, params: Params | None = None, per_record: bool = False, seg_first: int = 0,
                            seg_count: int = -1):
        """The per-base profile of every oligo of a panel (fasim_scan_oligos_profile): a list per oligo of TfoProfile -- what
        scan_tfo_profile() would give for a lncRNA, with the oligo in its place -- over the whole record set, or with per_record
        lists per record, each what that record scanned alone gives.  `dnas` as for scan_oligos().  The engine's own query is not
        touched.  Shards of a segment range merge with merge_tfo_profiles(); the table is tfo_profile_tsv().  Totals per oligo:
        `self.last_totals`."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        nprof = max(1, nq) * (max(1, nrec) if per_record else 1)
        profs = (C.POINTER(_TfoProfile) * nprof)()
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos_profile(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                      1 if per_record else 0, profs, totals))
        self._totals(totals, nq)
        if per_record:
            return _grid(TfoProfile, profs, nq, nrec)
        return [TfoProfile(_native=profs[q]) for q in range(nq)]

    def scan_oligos_peaks(self, oligos, dnas, params: Params | None = None, bin: int = 0, seg_first: int = 0, seg_count: int = -1):
        """The screen of a panel (fasim_scan_oligos_peaks): an (nq, nrec, 4, 3) int64 array of (value, pos, enc) per oligo, record and
        strand class (TRACK_CLASSES) -- what scan_records_track() gives for a lncRNA, from the oligo's potential -- (0, -1, -1)
        where the potential is zero.  bin >= 1: `(tracks, peaks)`, tracks being scan_oligos()' tracks of that width.  `dnas` as for
        scan_oligos().  Shards of a segment range merge with merge_peaks() / merge_tracks(); the table is screen_tsv().  Totals per
        oligo: `self.last_totals`."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        nout = max(1, nq) * max(1, nrec)
        trks = (C.POINTER(_Track) * nout)() if bin != 0 else None
        peaks = (_Peak * (nout * 4))()
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos_peaks(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                    bin, trks, peaks, totals))
        self._totals(totals, nq)
        pk = _peaks_from_c(peaks, nout * 4).reshape(nq, nrec, 4, 3)
        if trks is None:
            return pk
        return _grid(Track, trks, nq, nrec), pk

    def scan_hist(self, dnas, params: Params | None = None, controls: int = 0, seed: int = 0, records: bool = False, seg_first: int = 0,
                  seg_count: int = -1, rnas=None):
        """Histogram of the potential over a record set, with shuffled controls (fasim_scan_records_hist): `(results | None, hist,
        control_hists)`.  `dnas` as for scan_sites().  rnas None: the query last given to set_query(); hist is one
        Hist over the whole set and control_hists the Hists of shuffle_query(rna, seed, k), k = 1 .. controls, scanned as plain
        queries of the same call.  rnas given: lists per lncRNA of those.  records True: stage 3 runs and results is what
        scan_records() returns for the lncRNA (not for its controls).  Shards of a segment range merge with merge_hists()."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        if controls < 0:
            raise FasimError(f"scan_hist: controls = {controls} is negative", E_ARG)
        if rnas is None and getattr(self, "rna", None) is None:
            raise FasimError("scan_hist: no query set: call set_query() first", E_ARG)
        base = [self.rna] if rnas is None else [bytes(r) for r in rnas]
        nb = len(base)
        ctl = [shuffle_query(r, seed, k + 1) for r in base for k in range(controls)]

        def call(qs, want_records):
            arr, qlens, nq, _ = _pack_queries(qs)
            outs = (C.POINTER(_Result) * (max(1, nq) * max(1, nrec)))() if want_records else None
            hs = (C.POINTER(_Hist) * max(1, nq))()
            totals = (ScanStats * max(1, nq))()
            self._check(self._L.fasim_scan_records_hist(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                        outs, hs, totals))
            res = None
            if want_records:
                res = self._wrap_results(outs, nq, nrec)
            return res, [Hist(_native=hs[q]) for q in range(nq)], [self._stats_dict(totals[q]) for q in range(nq)]

        if records:
            # stage 3 for the lncRNAs only: their controls go in a histogram-only call of their own
            res, hists, totals = call(base, True)
            chists = call(ctl, False)[1] if ctl else []
        else:
            res, allh, totals = call(base + ctl, False)
            hists, chists, totals = allh[:nb], allh[nb:], totals[:nb]
        if ctl:
            self._check(self._L.fasim_set_query(self._h, base[-1], len(base[-1])))      # (a call leaves the engine on its last query)
        self.rna, self.m = base[-1], len(base[-1])
        self.last_totals = totals
        chists = [chists[q * controls:(q + 1) * controls] for q in range(nb)]
        if rnas is None:
            return (res[0] if res else None), hists[0], chists[0]
        return res, hists, chists

    def scan_oligos_hist(self, oligos, dnas, params: Params | None = None, seg_first: int = 0, seg_count: int = -1):
        """Histograms of the potential of a panel of short oligos (fasim_scan_oligos_hist): one Hist per oligo over the record set,
        what scan_hist() would give for a lncRNA with the oligo in its place.  `dnas` as for scan_oligos()."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        hs = (C.POINTER(_Hist) * max(1, nq))()
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos_hist(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                   hs, totals))
        self._totals(totals, nq)
        return [Hist(_native=hs[q]) for q in range(nq)]

    def scan_site_counts(self, dnas, params: Params | None = None, controls: int = 0, seed: int = 0, shuffle: str = "mono",
                         records: bool = False, seg_first: int = 0, seg_count: int = -1, rnas=None):
        """Sites per threshold over a record set, with shuffled controls (fasim_scan_records_site_counts): `(results | None, counts,
        control_counts)`, everything as scan_hist() with SiteCounts in the place of the Hists.  shuffle "mono": the controls are
        shuffle_query(rna, seed, k); "di": shuffle_query_dinuc(rna, seed, k), which keep the dinucleotide counts.  Shards of a
        segment range merge with merge_site_counts()."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        if controls < 0:
            raise FasimError(f"scan_site_counts: controls = {controls} is negative", E_ARG)
        if shuffle not in ("mono", "di"):
            raise FasimError(f"scan_site_counts: shuffle = {shuffle!r} is neither 'mono' nor 'di'", E_ARG)
        if rnas is None and getattr(self, "rna", None) is None:
            raise FasimError("scan_site_counts: no query set: call set_query() first", E_ARG)
        base = [self.rna] if rnas is None else [bytes(r) for r in rnas]
        nb = len(base)
        shuf = shuffle_query_dinuc if shuffle == "di" else shuffle_query
        ctl = [shuf(r, seed, k + 1) for r in base for k in range(controls)]

        def call(qs, want_records):
            arr, qlens, nq, _ = _pack_queries(qs)
            outs = (C.POINTER(_Result) * (max(1, nq) * max(1, nrec)))() if want_records else None
            cs = (C.POINTER(_SiteCounts) * max(1, nq))()
            totals = (ScanStats * max(1, nq))()
            self._check(self._L.fasim_scan_records_site_counts(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count,
                                                               C.byref(p), outs, cs, totals))
            res = self._wrap_results(outs, nq, nrec) if want_records else None
            return res, [SiteCounts(_native=cs[q]) for q in range(nq)], [self._stats_dict(totals[q]) for q in range(nq)]

        if records:
            # stage 3 for the lncRNAs only: their controls go in a counts-only call of their own
            res, counts, totals = call(base, True)
            ccounts = call(ctl, False)[1] if ctl else []
        else:
            res, allc, totals = call(base + ctl, False)
            counts, ccounts, totals = allc[:nb], allc[nb:], totals[:nb]
        if ctl:
            self._check(self._L.fasim_set_query(self._h, base[-1], len(base[-1])))      # (a call leaves the engine on its last query)
        self.rna, self.m = base[-1], len(base[-1])
        self.last_totals = totals
        ccounts = [ccounts[q * controls:(q + 1) * controls] for q in range(nb)]
        if rnas is None:
            return (res[0] if res else None), counts[0], ccounts[0]
        return res, counts, ccounts

    def scan_oligos_site_counts(self, oligos, dnas, params: Params | None = None, seg_first: int = 0, seg_count: int = -1):
        """Sites per threshold of a panel of short oligos (fasim_scan_oligos_site_counts): one SiteCounts per oligo over the record
        set.  `dnas` as for scan_oligos()."""
        p = params or default_params()
        blob, offs, lens, nrec = _pack_records(dnas, resident_ok=True)
        arr, qlens, nq, _ = _pack_queries([bytes(x) for x in oligos])
        cs = (C.POINTER(_SiteCounts) * max(1, nq))()
        totals = (ScanStats * max(1, nq))()
        self._check(self._L.fasim_scan_oligos_site_counts(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count,
                                                          C.byref(p), cs, totals))
        self._totals(totals, nq)
        return [SiteCounts(_native=cs[q]) for q in range(nq)]

    def score_variants(self, variants, dnas, p: Params | None = None, flank: int = 300, queries=None, _aligned: bool = False):
        """The triplex potential through variants (fasim_score_variants): `(values, encs, flags)`, int32 arrays of shape
        (nq, nvar, 2, 4), the same, and (nq, nvar): per query, variant, allele (0 REF, 1 ALT) and strand class (TRACK_CLASSES) the best
        score of a local alignment through the allele within `flank` bases of it, the smallest encoding that attains it (-1: value 0),
        and bit 0 `clipped` (an alignment of the variant's largest value may continue past the flank).  `variants`: Variant tuples
        (read_vcf()), pos 0-based within record `rec` of `dnas` (a list of records, one bytes object, or None with the whole resident
        buffer as record 0); an unusable variant gets zeros and -1.  queries None: the lncRNA last given to set_query() -- the
        engine's own query is neither used nor changed by the call.  REF is not compared with the record.  Counters of the call:
        `self.last_variant_stats`."""
        import numpy as np
        p = p or default_params()
        if queries is None:
            if self.rna is None:
                raise FasimError("score_variants: no queries given and no query set", E_ARG)
            queries = [self.rna]
        queries = [bytes(x) for x in queries]
        # (dnas None: the whole resident buffer as record 0)
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens=[self.resident_len()] if dnas is None else None)
        arr, qlens, nq, _ = _pack_queries(queries)
        vs, _keep = _variants_to_c(variants)
        nvar = len(variants)
        out = (_VariantScore * max(1, nq * nvar))()
        st = _VariantStats()
        if _aligned:
            win = (_VariantWindow * max(1, nvar))()
            hts = (C.POINTER(_SiteHits) * max(1, nq))()
            self._check(self._L.fasim_score_variants_aligned(self._h, arr, qlens, nq, blob, offs, lens, nrec, vs, nvar, flank, C.byref(p), out,
                                                             C.byref(st), win, hts))
        else:
            self._check(self._L.fasim_score_variants(self._h, arr, qlens, nq, blob, offs, lens, nrec, vs, nvar, flank, C.byref(p), out, C.byref(st)))
        self.last_variant_stats = dict(problems=st.problems, cells=st.cells, kernel_s=st.kernel_s, total_s=st.total_s)
        flat = np.frombuffer(out, dtype=np.int32).reshape(max(1, nq * nvar), 18)[:nq * nvar]
        values = flat[:, 0:8].reshape(nq, nvar, 2, 4).copy()
        encs = flat[:, 8:16].reshape(nq, nvar, 2, 4).copy()
        flags = flat[:, 16].reshape(nq, nvar).copy()
        if _aligned:
            windows = np.frombuffer(win, dtype=np.int32).reshape(max(1, nvar), 4)[:nvar, :3].copy()
            return values, encs, flags, windows, [SiteHits(hts[q]) for q in range(nq)]
        return values, encs, flags

    def score_haplotypes(self, variants, genotypes, dnas, p: Params | None = None, flank: int = 300, queries=None, matched=None):
        """Variants scored on a sample's two haplotypes (fasim_score_haplotypes): `(values, encs, info)`.  values and encs are int32
        arrays of shape (nq, nvar, 2, 2, 4): per query, entry, haplotype, allele (0 REF, 1 ALT) and strand class what score_variants()
        gives for the entry in a record that carries the haplotype's other variants (`genotypes`: (nvar, 3) rows of hap[0], hap[1],
        phased, as read_vcf(path, sample) returns them).  info (nq, nvar, 2, 3): per haplotype `carried` (1 this ALT, 0 REF, 2 another
        ALT of the line, -1 missing), `applied` (neighbours with a letter in the windows) and `flags` (bit 0 clipped, bit 1 an
        unphased heterozygote in reach was left out, bit 2 an entry in reach was rejected for overlap, bit 3 both haplotypes have
        the same windows).  matched[k] false keeps entry k from being applied as a neighbour.  `dnas` and `queries` as for
        score_variants().  Counters of the call: `self.last_variant_stats`."""
        import numpy as np
        p = p or default_params()
        if queries is None:
            if self.rna is None:
                raise FasimError("score_haplotypes: no queries given and no query set", E_ARG)
            queries = [self.rna]
        queries = [bytes(x) for x in queries]
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens=[self.resident_len()] if dnas is None else None)
        arr, qlens, nq, _ = _pack_queries(queries)
        vs, _keep = _variants_to_c(variants)
        nvar = len(variants)
        gs = _genotypes_to_c(genotypes, nvar)
        mt = None if matched is None else (C.c_uint8 * max(1, nvar))(*[1 if x else 0 for x in matched])
        out = (_HapScore * max(1, nq * nvar))()
        st = _VariantStats()
        self._check(self._L.fasim_score_haplotypes(self._h, arr, qlens, nq, blob, offs, lens, nrec, vs, gs, mt, nvar, flank, C.byref(p), out,
                                                   C.byref(st)))
        self.last_variant_stats = dict(problems=st.problems, cells=st.cells, kernel_s=st.kernel_s, total_s=st.total_s)
        flat = np.frombuffer(out, dtype=np.int32).reshape(max(1, nq * nvar), 42)[:nq * nvar]
        per = flat[:, :36].reshape(nq, nvar, 2, 18)
        values = per[..., 0:8].reshape(nq, nvar, 2, 2, 4).copy()
        encs = per[..., 8:16].reshape(nq, nvar, 2, 2, 4).copy()
        info = np.stack([flat[:, 36:38], flat[:, 38:40], flat[:, 40:42]], axis=-1).reshape(nq, nvar, 2, 3).copy()
        return values, encs, info

    def score_variants_aligned(self, variants, dnas, p: Params | None = None, flank: int = 300, queries=None):
        """score_variants() and the alignment behind every score (fasim_score_variants_aligned): `(values, encs, flags, windows,
        hits)`.  The first three are exactly what score_variants() returns.  windows: (nvar, 3) int32 rows of (pre, post, edge) --
        the record's letters before and after REF inside the flank, edge bit 0 / 1: the lower / upper end of the window was cut by
        the flank.  hits: one SiteHits per query with 8 * nvar hits, hit variant_hit_index(v, allele, cls): the cells i0, i1, j0, j1
        of the path through the touching matrix in the unit of encs[q, v, allele, cls], its CIGAR and its triplex record (seg = v);
        a slot without a value has cigar_len 0, an unaligned one (more than 2^26 cells) -1."""
        return self.score_variants(variants, dnas, p, flank, queries, _aligned=True)

    def score_mutagenesis(self, intervals, dnas, p: Params | None = None, flank: int = 300, queries=None):
        """Every substitution at every position of intervals, from one shared pass per interval (fasim_score_mutagenesis):
        `(values, encs, ref, clipped, offsets)`.  `intervals`: (rec, start, end) triples, 0-based half-open stretches of record `rec`
        of `dnas` (as for score_variants()), at most 5 120 - 2 * flank positions each.  values and encs (nq, npos, 4, 4): per query,
        position, letter of ACGT and strand class the value of the position with that letter in it -- what score_variants() defines
        for the window [start - flank, end + flank) of the record, the same for every position of the interval -- and the smallest
        encoding that attains it (-1: value 0).  ref (npos,): the index in ACGT of the record's own byte, -1 for any other byte.
        clipped (nq, npos, 4): bit 0 of the letter's largest 2 * value + bit.  offsets (nint + 1,): the positions of interval k are
        [offsets[k], offsets[k + 1]), ascending.  queries as for score_variants().  Counters of the call:
        `self.last_mutagenesis_stats`."""
        import numpy as np
        p = p or default_params()
        if queries is None:
            if self.rna is None:
                raise FasimError("score_mutagenesis: no queries given and no query set", E_ARG)
            queries = [self.rna]
        queries = [bytes(x) for x in queries]
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens=[self.resident_len()] if dnas is None else None)
        arr, qlens, nq, _ = _pack_queries(queries)
        ivs, offsets = _intervals_to_c(intervals)
        nint, npos = len(intervals), int(offsets[-1])
        out = (_MutScore * max(1, nq * npos))()
        st = _MutagenesisStats()
        self._check(self._L.fasim_score_mutagenesis(self._h, arr, qlens, nq, blob, offs, lens, nrec, ivs, nint, flank, C.byref(p), out, C.byref(st)))
        self.last_mutagenesis_stats = {k: getattr(st, k) for k, _ in _MutagenesisStats._fields_}
        flat = np.frombuffer(out, dtype=_mut_dtype())[:nq * npos].reshape(nq, npos)
        ref = flat["ref"][0].copy() if nq else np.zeros(npos, dtype=np.int8)
        return flat["value"].copy(), flat["enc"].copy(), ref, flat["clipped"].copy(), offsets

    def score_deletions(self, intervals, dnas, p: Params | None = None, flank: int = 300, lengths=(1,), queries=None):
        """Every deletion inside intervals, from the shared pass of score_mutagenesis() (fasim_score_deletions): `(values, encs,
        clipped, valid, clean, offsets)`.  intervals, dnas, flank, queries and offsets as for score_mutagenesis(); `lengths`: 1 to
        MAX_DELETION_LENGTHS strictly ascending integers in [1, MAX_ALLELE - 1].  The deletion (x, d) keeps base x, the anchor of its
        VCF line, and takes out the d bases behind it; it exists where x + d < end.  values and encs (nq, npos, nlen, 2, 4): per
        query, position, length, allele (0 REF, 1 ALT) and strand class what score_variants() defines for pos = x, REF =
        record[x:x + d + 1], ALT = record[x] in the window [start - flank, end + flank), and the smallest encoding that attains it
        (-1: value 0).  clipped (nq, npos, nlen, 2): bit 0 of the allele's largest 2 * value + bit.  valid (npos, nlen): the pair is
        a deletion (else zeros).  clean (npos, nlen): it is one and its d + 1 bytes are upper-case ACGT.  Counters of the call:
        `self.last_deletion_stats`."""
        import numpy as np
        p = p or default_params()
        if queries is None:
            if self.rna is None:
                raise FasimError("score_deletions: no queries given and no query set", E_ARG)
            queries = [self.rna]
        queries = [bytes(x) for x in queries]
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens=[self.resident_len()] if dnas is None else None)
        arr, qlens, nq, _ = _pack_queries(queries)
        ivs, offsets = _intervals_to_c(intervals)
        nint, npos = len(intervals), int(offsets[-1])
        lengths = [int(d) for d in lengths]
        nlen = len(lengths)
        ln = (C.c_int32 * max(1, nlen))(*lengths)
        out = (_DelScore * max(1, nq * npos * nlen))()
        st = _DeletionStats()
        self._check(self._L.fasim_score_deletions(self._h, arr, qlens, nq, blob, offs, lens, nrec, ivs, nint, flank, ln, nlen, C.byref(p), out, C.byref(st)))
        self.last_deletion_stats = {k: getattr(st, k) for k, _ in _DeletionStats._fields_}
        flat = np.frombuffer(out, dtype=_del_dtype())[:nq * npos * nlen].reshape(nq, npos, nlen)
        valid = flat["valid"][0].copy() if nq else np.zeros((npos, nlen), dtype=np.uint8)
        clean = flat["clean"][0].copy() if nq else np.zeros((npos, nlen), dtype=np.uint8)
        return flat["value"].copy(), flat["enc"].copy(), flat["clipped"].copy(), valid, clean, offsets

    def _records_track(self, blob, offs, lens, nrec, p, rnas, bin, records, seg_first, seg_count):
        arr, qlens, nq, nqo = _pack_queries(rnas)
        nout = nqo * max(1, nrec)
        outs = (C.POINTER(_Result) * nout)() if records else None
        trks = (C.POINTER(_Track) * nout)() if bin != 0 else None
        peaks = (_Peak * (nout * 4))()
        totals = (ScanStats * nqo)()
        self._check(self._L.fasim_scan_records_track(self._h, arr, qlens, nq, blob, offs, lens, nrec, seg_first, seg_count, C.byref(p),
                                                     bin, outs, trks, peaks, totals))
        if nq:
            self.m = len(rnas[-1])
        self._totals(totals, nqo)
        res = trk = None
        if records:
            res = self._wrap_results(outs, nqo, nrec)
        if trks is not None:
            trk = _grid(Track, trks, nqo, nrec)
        pk = _peaks_from_c(peaks, nout * 4).reshape(nqo, nrec, 4, 3)
        if rnas is None:
            return (res[0] if res else None), (trk[0] if trk else None), pk[0]
        return res, trk, pk

    def scan_records_track(self, dnas, params: Params | None = None, rnas=None, bin: int = 0, records: bool = True,
                           seg_first: int = 0, seg_count: int = -1, rec_lens=None):
        """Record set with its potential (fasim_scan_records_track): `(results | None, tracks | None, peaks)`.  Arguments as
        scan_records(); bin 0: peaks only (tracks is None), bin >= 1: one Track per record, what scan_track() gives for that
        record alone.  records False: no stage 3, results is None.  peaks: (nrec, 4, 3) int64 array of (value, pos, enc) per
        record and strand class (TRACK_CLASSES), (0, -1, -1) where the potential is zero.  rnas given: lists per lncRNA and a
        (nq, nrec, 4, 3) array.  Shards of a segment range merge with merge_tracks() / merge_peaks().  Totals: `self.last_totals`."""
        p = params or default_params()
        if dnas is None and rec_lens is None:
            raise FasimError("scan_records_track(None, ...) needs rec_lens (the records of the resident buffer)", E_ARG)
        blob, offs, lens, nrec = _pack_records(dnas, rec_lens)
        return self._records_track(blob, offs, lens, nrec, p, rnas, bin, records, seg_first, seg_count)

    def scan_regions_track(self, seq: bytes | None, spans, params: Params | None = None, rnas=None, bin: int = 0,
                           records: bool = True, seg_first: int = 0, seg_count: int = -1):
        """scan_records_track() for BED-style spans of one sequence (see scan_regions()): positions of the peaks and the tracks'
        bins are relative to each span's start."""
        p = params or default_params()
        offs, lens, nrec = _pack_spans(seq, spans, "scan_regions_track")
        return self._records_track(seq, offs, lens, nrec, p, rnas, bin, records, seg_first, seg_count)

    def scan_regions(self, seq: bytes | None, spans, params: Params | None = None, rnas=None):
        """BED-style regions of one sequence (fasim_scan_records with explicit offsets): `spans` are 0-based half-open
        (start, end) pairs into `seq`, or into the buffer made resident by load_dna() when `seq` is None.  Spans may overlap,
        nest, repeat and come in any order.  Returns what scan_records() returns, and result k is identical to
        scan_records([seq[s:e]]) of span k.  The call's totals are left in `self.last_totals`."""
        p = params or default_params()
        offs, lens, nrec = _pack_spans(seq, spans, "scan_regions")
        arr, qlens, nq, nqo = _pack_queries(rnas)
        outs = (C.POINTER(_Result) * (nqo * nrec))()
        totals = (ScanStats * nqo)()
        self._check(self._L.fasim_scan_records(self._h, arr, qlens, nq, seq, offs, lens, nrec, 0, -1, C.byref(p), outs, totals))
        if nq:
            self.m = len(rnas[-1])
        self._totals(totals, nqo)
        res = self._wrap_results(outs, nqo, nrec)
        return res[0] if rnas is None else res


def sim_finish_unit(rna: bytes, seg: bytes, enc: int, dna_start: int, min_score: int, nodes, params: Params | None = None) -> "ScanResult":
    """Host half of the -F path for one unit (fasim_sim_finish_unit): `nodes` = 9-tuples of the forward sweep's node list."""
    L = lib()
    p = params or default_params()
    arr = (SimNode * max(1, len(nodes)))()
    for k, t in enumerate(nodes):
        for (name, _), v in zip(SimNode._fields_, t):
            setattr(arr[k], name, v)
    res = C.POINTER(_Result)()
    rc = L.fasim_sim_finish_unit(rna, len(rna), seg, len(seg), enc, dna_start, min_score, C.byref(p), arr, len(nodes), C.byref(res))
    if rc != 0:
        raise FasimError(f"fasim_sim_finish_unit failed ({rc}): {L.fasim_last_error(None).decode()}")
    return ScanResult(stats={}, _native=res)


def pick_candidates(cols, threshold):
    L = lib()
    n = len(cols)
    arr = (C.c_int32 * n)(*cols)
    s = (C.c_int32 * (n + 1))()
    p = (C.c_int32 * (n + 1))()
    k = C.c_int32()
    rc = L.fasim_pick_candidates(arr, n, threshold, s, p, n + 1, C.byref(k))
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode())
    return [(s[i], p[i]) for i in range(k.value)]


def encode_unit(seg: bytes, enc: int):
    L = lib()
    t = C.create_string_buffer(len(seg) + 1)
    s = C.create_string_buffer(len(seg) + 1)
    rc = L.fasim_encode_unit(seg, len(seg), enc, t, s)
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode())
    return t.raw[:len(seg)], s.raw[:len(seg)].rstrip(b"\0")


def segment_count(dna_len: int, params: Params | None = None) -> int:
    p = params or default_params()
    return lib().fasim_segment_count(dna_len, C.byref(p))


TAIL_CLAMP_CLUSTER = 1


def tfosorted(result: ScanResult, chr_name: str, start_genome: int, params: Params | None = None, flags: int = 0) -> bytes:
    """-TFOsorted bytes for the (merged) records; host-side tail of the path."""
    L = lib()
    p = params or default_params()
    rp, cnt, pp, plen = result.pointers()
    return _text_call(L.fasim_tfosorted_ex, rp or None, cnt, pp or C.addressof(_EMPTY_POOL), max(1, plen), chr_name.encode(),
                      start_genome, C.byref(p), flags, name="fasim_tfosorted", code=False)


def tfoclass(result: ScanResult, level: int, chr_name: str, start_genome: int, dna_len: int, rna_name: str,
             params: Params | None = None, flags: int = 0) -> bytes:
    """-TFOclass<level>-<ds>-<lg> bedGraph bytes (print_cluster, Fasim-LongTarget.cpp:694) for the merged records."""
    L = lib()
    p = params or default_params()
    rp, cnt, _, _ = result.pointers()
    return _text_call(L.fasim_tfoclass_ex, rp or None, cnt, level, chr_name.encode(), start_genome, dna_len, rna_name.encode(),
                      C.byref(p), flags, name="fasim_tfoclass", code=False)


def tail_outputs(result: ScanResult, chr_name: str, start_genome: int, dna_len: int, rna_name: str, params: Params | None = None,
                 flags: int = 0):
    """(-TFOsorted, -TFOclass1, -TFOclass2) bytes from one clustering of the records (fasim_tail_outputs)."""
    L = lib()
    p = params or default_params()
    texts = [C.c_void_p() for _ in range(3)]
    lens = [C.c_int64() for _ in range(3)]
    rp, cnt, pp, plen = result.pointers()
    args = []
    for t, n in zip(texts, lens):
        args += [C.byref(t), C.byref(n)]
    rc = L.fasim_tail_outputs(rp or None, cnt, pp or C.addressof(_EMPTY_POOL), max(1, plen), chr_name.encode(), start_genome, dna_len,
                              rna_name.encode(), C.byref(p), flags, *args)
    if rc != 0:
        raise FasimError(f"fasim_tail_outputs failed ({rc}): {L.fasim_last_error(None).decode()}")
    try:
        return tuple(C.string_at(t, n.value) for t, n in zip(texts, lens))
    finally:
        for t in texts:
            L.fasim_free(t)


class Region(NamedTuple):
    """One BED interval (fasim_read_bed): 1-based line, chrom, 0-based half-open [start, end), name (column 4, else
    <chrom>_<start+1>_<end>; a repeated (name, chrom) pair gets _<line> appended)."""
    line: int
    chrom: str
    start: int
    end: int
    name: str


def read_bed(path) -> list:
    """The intervals of a BED file as `fasim --regions` reads them; a refused file raises FasimError with code E_ARG and the
    line number in the message."""
    L = lib()
    out = C.POINTER(_Region)()
    n = C.c_int64()
    rc = L.fasim_read_bed(os.fsencode(path), C.byref(out), C.byref(n))
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode(), rc)
    try:
        return [Region(out[k].line, out[k].chrom.decode(), out[k].start, out[k].end, out[k].name.decode()) for k in range(n.value)]
    finally:
        L.fasim_free(out)


class Variant(NamedTuple):
    """One (VCF line, ALT allele) pair (fasim_read_vcf): 1-based line, chrom, 0-based pos of REF's first letter, id, ref, alt
    (upper case), the record it lies in (read_vcf: 0) and whether its alleles can be scored (1 .. MAX_ALLELE letters of ACGTN)."""
    line: int
    chrom: str
    pos: int
    id: str
    ref: str
    alt: str
    rec: int = 0
    usable: bool = True


def read_vcf(path, sample=None):
    """The variants of a VCF file as `fasim --variants` reads them, one Variant per ALT allele; a refused file raises FasimError
    with code E_ARG and the line number in the message.  With `sample` (a name of the #CHROM line; fasim_read_vcf_sample):
    `(variants, genotypes)`, genotypes an (n, 3) int8 array of hap[0], hap[1] (1 the entry's ALT, 0 not, -1 missing) and phased."""
    L = lib()
    out = C.POINTER(_Variant)()
    gts = C.POINTER(_Genotype)()
    n = C.c_int64()
    if sample is None:
        rc = L.fasim_read_vcf(os.fsencode(path), C.byref(out), C.byref(n))
    else:
        rc = L.fasim_read_vcf_sample(os.fsencode(path), sample.encode() if isinstance(sample, str) else bytes(sample), C.byref(out),
                                     C.byref(n), C.byref(gts))
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode(), rc)
    try:
        variants = [Variant(out[k].line, out[k].chrom.decode(), out[k].pos, out[k].id.decode(), out[k].ref.decode(), out[k].alt.decode(),
                            out[k].rec, out[k].alt_len >= 0) for k in range(n.value)]
        if sample is None:
            return variants
        import numpy as np
        g = np.array([[gts[k].hap[0], gts[k].hap[1], gts[k].phased] for k in range(n.value)], dtype=np.int8).reshape(n.value, 3)
        return variants, g
    finally:
        L.fasim_free(out)
        if sample is not None:
            L.fasim_free(gts)


def _variants_to_c(variants):
    n = len(variants)
    vs = (_Variant * max(1, n))()
    keep = []
    for k, v in enumerate(variants):
        strs = [x.encode() if isinstance(x, str) else bytes(x) for x in (v.chrom, v.id, v.ref, v.alt)]
        keep.append(strs)
        vs[k].line, vs[k].pos, vs[k].rec = v.line, v.pos, v.rec
        vs[k].ref_len, vs[k].alt_len = len(strs[2]), (len(strs[3]) if v.usable else -1)
        vs[k].chrom, vs[k].id, vs[k].ref, vs[k].alt = strs
    return vs, keep


def _genotypes_to_c(genotypes, n):
    import numpy as np
    g = np.asarray(genotypes, dtype=np.int8).reshape(n, 3)
    gs = (_Genotype * max(1, n))()
    for k in range(n):
        gs[k].hap[0], gs[k].hap[1], gs[k].phased = int(g[k, 0]), int(g[k, 1]), 1 if g[k, 2] else 0
    return gs


def haplotype_window(variants, genotypes, dna: bytes, v: int, hap: int, allele: int, flank: int, matched=None):
    """`(letters, v0, edge)`: the window of entry v on haplotype `hap` for `allele` (0 REF, 1 ALT) in haplotype letters, as the
    planner of Engine.score_haplotypes() builds it (fasim_haplotype_window, pure host code); `dna` is the record of variants[v].  The
    allele's letters start at v0; edge bit 0 / 1: the lower / upper end was cut by the flank."""
    L = lib()
    n = len(variants)
    vs, _keep = _variants_to_c(variants)
    gs = _genotypes_to_c(genotypes, n)
    mt = None if matched is None else (C.c_uint8 * max(1, n))(*[1 if x else 0 for x in matched])
    text = C.c_void_p()
    ln, v0, edge = C.c_int32(), C.c_int32(), C.c_int32()
    dna = bytes(dna)
    rc = L.fasim_haplotype_window(vs, gs, n, mt, len(dna), dna, v, hap, allele, flank, C.byref(text), C.byref(ln), C.byref(v0), C.byref(edge))
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode(), rc)
    try:
        return C.string_at(text, ln.value), v0.value, edge.value
    finally:
        L.fasim_free(text)


def haplotype_info(variants, genotypes, dna: bytes, v: int, flank: int, matched=None):
    """A (2, 3) int32 array: per haplotype carried, applied and flags (without bit 0, clipped) of entry v as Engine.score_haplotypes()
    reports them in `info` -- the part of the result that the host planner decides (fasim_haplotype_info, pure host code)."""
    import numpy as np
    L = lib()
    n = len(variants)
    vs, _keep = _variants_to_c(variants)
    gs = _genotypes_to_c(genotypes, n)
    mt = None if matched is None else (C.c_uint8 * max(1, n))(*[1 if x else 0 for x in matched])
    c, a, f = (C.c_int32 * 2)(), (C.c_int32 * 2)(), (C.c_int32 * 2)()
    dna = bytes(dna)
    rc = L.fasim_haplotype_info(vs, gs, n, mt, len(dna), dna, v, flank, c, a, f)
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode(), rc)
    return np.array([[c[h], a[h], f[h]] for h in range(2)], dtype=np.int32)


def haplotypes_tsv(variants, genotypes, values, encs, info, flank: int, rna_name: str, sample: str, matched=None) -> bytes:
    """The bytes of `fasim --variants --sample`'s table for one query (fasim_haplotypes_tsv): values and encs (nvar, 2, 2, 4), info
    (nvar, 2, 3) as Engine.score_haplotypes() returns them per query."""
    import numpy as np
    L = lib()
    n = len(variants)
    vs, _keep = _variants_to_c(variants)
    gs = _genotypes_to_c(genotypes, n)
    sc = (_HapScore * max(1, n))()
    flat = np.frombuffer(sc, dtype=np.int32).reshape(max(1, n), 42)
    info = np.asarray(info, dtype=np.int32).reshape(n, 2, 3)
    per = flat[:n, :36].reshape(n, 2, 18)
    per[..., 0:8] = np.asarray(values, dtype=np.int32).reshape(n, 2, 8)
    per[..., 8:16] = np.asarray(encs, dtype=np.int32).reshape(n, 2, 8)
    per[..., 16] = info[..., 2] & 1
    flat[:n, 36:38], flat[:n, 38:40], flat[:n, 40:42] = info[..., 0], info[..., 1], info[..., 2]
    mt = None if matched is None else (C.c_uint8 * max(1, n))(*[1 if x else 0 for x in matched])
    return _text_call(L.fasim_haplotypes_tsv, vs, gs, sc, n, flank, rna_name.encode(), sample.encode(), mt)


def variants_tsv(variants, values, encs, flags, flank: int, rna_name: str, matched=None) -> bytes:
    """The bytes of `fasim --variants`' table for one query (fasim_variants_tsv): values and encs (nvar, 2, 4), flags (nvar) as
    Engine.score_variants() returns them per query; matched[k] false (or an unusable variant): an NA line."""
    import numpy as np
    L = lib()
    n = len(variants)
    vs, _keep = _variants_to_c(variants)
    values = np.asarray(values, dtype=np.int32).reshape(n, 8)
    encs = np.asarray(encs, dtype=np.int32).reshape(n, 8)
    flags = np.asarray(flags, dtype=np.int32).reshape(n)
    sc = (_VariantScore * max(1, n))()
    flat = np.frombuffer(sc, dtype=np.int32).reshape(max(1, n), 18)
    flat[:n, 0:8], flat[:n, 8:16], flat[:n, 16] = values, encs, flags
    mt = None if matched is None else (C.c_uint8 * max(1, n))(*[1 if x else 0 for x in matched])
    return _text_call(L.fasim_variants_tsv, vs, sc, n, flank, rna_name.encode(), mt)


def _mut_dtype():
    """fasim_mut_score as a numpy record."""
    import numpy as np
    return np.dtype([("value", "<i4", (4, 4)), ("enc", "i1", (4, 4)), ("ref", "i1"), ("clipped", "u1", (4,)), ("reserved", "u1", (3,))])


def _intervals_to_c(intervals):
    """(rec, start, end) triples as fasim_interval[] and the positions' offsets (nint + 1,)."""
    import numpy as np
    n = len(intervals)
    ivs = (_Interval * max(1, n))()
    offsets = np.zeros(n + 1, dtype=np.int64)
    for k, (rec, start, end) in enumerate(intervals):
        ivs[k].rec, ivs[k].start, ivs[k].end = int(rec), int(start), int(end)
        offsets[k + 1] = offsets[k] + max(0, int(end) - int(start))
    return ivs, offsets


def mutagenesis_variants(intervals, dnas) -> list:
    """The SNVs that Engine.score_mutagenesis() scores for `intervals` ((rec, start, end) triples of the records `dnas`), as Variants
    in its order -- per position the three letters of ACGT that differ from the record's, none where the record's byte is not one
    of the four (ref -1) -- with line = the interval's index + 1, chrom = "rec<rec>" and id ".".  Any of them can go to
    Engine.score_variants_aligned() for the alignment behind its value."""
    if isinstance(dnas, (bytes, bytearray)):
        dnas = [bytes(dnas)]
    out = []
    for k, (rec, start, end) in enumerate(intervals):
        for x in range(start, end):
            r = chr(dnas[rec][x])
            if r not in "ACGT":
                continue
            out.extend(Variant(k + 1, f"rec{rec}", x, ".", r, b, rec) for b in "ACGT" if b != r)
    return out


def mutagenesis_tsv(regions, values, encs, ref, clipped, offsets, flank: int, rna_name: str) -> bytes:
    """The bytes of `fasim --mutagenesis`' table for one query (fasim_mutagenesis_tsv): `regions` the intervals as Region tuples
    (read_bed()), values and encs (npos, 4, 4), ref (npos,), clipped (npos, 4) and offsets (len(regions) + 1,) as
    Engine.score_mutagenesis() returns them per query; an interval without positions in offsets gets no lines."""
    import numpy as np
    L = lib()
    n = len(regions)
    rg = (_Region * max(1, n))()
    keep = []
    for k, r in enumerate(regions):
        keep.append((r.chrom.encode(), r.name.encode()))
        rg[k].line, rg[k].start, rg[k].end, rg[k].chrom, rg[k].name = r.line, r.start, r.end, keep[-1][0], keep[-1][1]
    offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(n + 1)
    npos = int(offs[-1])
    sc = (_MutScore * max(1, npos))()
    flat = np.frombuffer(sc, dtype=_mut_dtype())
    flat["value"][:npos] = np.asarray(values, dtype=np.int32).reshape(npos, 4, 4)
    flat["enc"][:npos] = np.asarray(encs, dtype=np.int8).reshape(npos, 4, 4)
    flat["ref"][:npos] = np.asarray(ref, dtype=np.int8).reshape(npos)
    flat["clipped"][:npos] = np.asarray(clipped, dtype=np.uint8).reshape(npos, 4)
    return _text_call(L.fasim_mutagenesis_tsv, rg, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, sc, flank, rna_name.encode())


def _del_dtype():
    """fasim_del_score as a numpy record."""
    import numpy as np
    return np.dtype([("value", "<i4", (2, 4)), ("enc", "i1", (2, 4)), ("clipped", "u1", (2,)), ("valid", "u1"), ("clean", "u1"),
                     ("reserved", "u1", (4,))])


def deletion_variants(intervals, dnas, lengths) -> list:
    """The clean deletions that Engine.score_deletions() scores for `intervals` and `lengths`, as Variants in the order of its table
    -- intervals, positions ascending, lengths in their order; REF the d + 1 letters from the anchor on, ALT the anchor -- with line =
    the interval's index + 1, chrom = "rec<rec>" and id ".".  Any of them can go to Engine.score_variants_aligned() for the
    alignment behind its value."""
    if isinstance(dnas, (bytes, bytearray)):
        dnas = [bytes(dnas)]
    out = []
    for k, (rec, start, end) in enumerate(intervals):
        for x in range(start, end):
            for d in lengths:
                ref = bytes(dnas[rec][x:x + d + 1]).decode("latin-1")
                if x + d < end and all(c in "ACGT" for c in ref):
                    out.append(Variant(k + 1, f"rec{rec}", x, ".", ref, ref[0], rec))
    return out


def deletions_tsv(regions, values, encs, clipped, valid, clean, offsets, seqs, lengths, flank: int, rna_name: str) -> bytes:
    """The bytes of `fasim --mutagenesis --deletions`' table for one query (fasim_deletions_tsv): `regions` the intervals as Region
    tuples (read_bed()); values and encs (npos, nlen, 2, 4), clipped (npos, nlen, 2), valid and clean (npos, nlen) and offsets
    (len(regions) + 1,) as Engine.score_deletions() returns them per query; seqs[k] the end - start letters of interval k (None for
    an interval without positions in offsets, which gets no lines); lengths as in the call."""
    import numpy as np
    L = lib()
    n = len(regions)
    rg = (_Region * max(1, n))()
    keep = []
    for k, r in enumerate(regions):
        keep.append((r.chrom.encode(), r.name.encode()))
        rg[k].line, rg[k].start, rg[k].end, rg[k].chrom, rg[k].name = r.line, r.start, r.end, keep[-1][0], keep[-1][1]
    sq = (C.c_char_p * max(1, n))(*[None if x is None else bytes(x) for x in seqs])
    lengths = [int(d) for d in lengths]
    nlen = len(lengths)
    ln = (C.c_int32 * max(1, nlen))(*lengths)
    offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(n + 1)
    npair = int(offs[-1]) * nlen
    sc = (_DelScore * max(1, npair))()
    flat = np.frombuffer(sc, dtype=_del_dtype())
    flat["value"][:npair] = np.asarray(values, dtype=np.int32).reshape(npair, 2, 4)
    flat["enc"][:npair] = np.asarray(encs, dtype=np.int8).reshape(npair, 2, 4)
    flat["clipped"][:npair] = np.asarray(clipped, dtype=np.uint8).reshape(npair, 2)
    flat["valid"][:npair] = np.asarray(valid, dtype=np.uint8).reshape(npair)
    flat["clean"][:npair] = np.asarray(clean, dtype=np.uint8).reshape(npair)
    return _text_call(L.fasim_deletions_tsv, rg, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, sc, sq, ln, nlen, flank, rna_name.encode())


def variant_hit_index(v: int, allele: int, cls: int) -> int:
    """Index of the hit of variant v, allele (0 REF, 1 ALT) and strand class cls in the SiteHits of score_variants_aligned()."""
    return (v * 2 + allele) * 4 + cls


def _variant_hit_span(variant, window, allele: int, enc: int, j0: int, j1: int):
    L = lib()
    vs, _keep = _variants_to_c([variant])
    w = _VariantWindow(int(window[0]), int(window[1]), int(window[2]), 0)
    a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
    rc = L.fasim_variant_hit_span(vs, C.byref(w), allele, enc, j0, j1, C.byref(a), C.byref(b), C.byref(c))
    if rc != 0:
        raise FasimError(L.fasim_last_error(None).decode(), rc)
    return a.value, b.value, bool(c.value)


def variant_hit_span(variant, window, allele: int, enc: int, j0: int, j1: int):
    """The reference bases `(start, end)`, 0-based half-open in the coordinates of variant.pos, that the unit columns [j0, j1] of a
    hit of `allele` under `enc` cover (fasim_variant_hit_span); window: (pre, post, edge) of score_variants_aligned().  Letters of
    the allele map to REF's range, letters behind it are shifted by the difference of the alleles' lengths."""
    return _variant_hit_span(variant, window, allele, enc, j0, j1)[:2]


def variant_hit_clipped(variant, window, allele: int, enc: int, j0: int, j1: int) -> bool:
    """The path of a hit lies in the unit's first or last column and that end of the window was cut by the flank."""
    return _variant_hit_span(variant, window, allele, enc, j0, j1)[2]


def variant_hits_tsv(variants, values, encs, windows, hits, flank: int, rna_name: str, matched=None) -> bytes:
    """The bytes of `fasim --variants --variant-hits`' second table for one query (fasim_variant_hits_tsv): values and encs
    (nvar, 2, 4), windows (nvar, 3) and hits (one SiteHits) as Engine.score_variants_aligned() returns them per query."""
    import numpy as np
    L = lib()
    n = len(variants)
    vs, _keep = _variants_to_c(variants)
    sc = (_VariantScore * max(1, n))()
    flat = np.frombuffer(sc, dtype=np.int32).reshape(max(1, n), 18)
    flat[:n, 0:8] = np.asarray(values, dtype=np.int32).reshape(n, 8)
    flat[:n, 8:16] = np.asarray(encs, dtype=np.int32).reshape(n, 8)
    win = (_VariantWindow * max(1, n))()
    wflat = np.frombuffer(win, dtype=np.int32).reshape(max(1, n), 4)
    wflat[:n, 0:3] = np.asarray(windows, dtype=np.int32).reshape(n, 3)
    mt = None if matched is None else (C.c_uint8 * max(1, n))(*[1 if x else 0 for x in matched])
    return _text_call(L.fasim_variant_hits_tsv, vs, sc, win, hits.pointer(), n, flank, rna_name.encode(), mt)


def empty_variant_hits(nvar: int) -> SiteHits:
    """8 * nvar hits without a value (cigar_len 0, cells -1, empty strings): what score_variants_aligned() returns where nothing
    scores; a structure of the caller's."""
    n = 8 * nvar
    k = max(1, n)
    keep = dict(t=(Triplex * k)(), qb=(C.c_int32 * k)(*[-1] * k), qe=(C.c_int32 * k)(*[-1] * k), tb=(C.c_int32 * k)(*[-1] * k),
                te=(C.c_int32 * k)(*[-1] * k), coff=(C.c_int64 * k)(), clen=(C.c_int32 * k)(), cig=(C.c_uint32 * 1)(),
                pool=C.create_string_buffer(1))
    for i in range(n):
        keep["t"][i].seg, keep["t"][i].enc = i // 8, -1
    h = _SiteHits(n, keep["t"], keep["qb"], keep["qe"], keep["tb"], keep["te"], keep["coff"], keep["clen"], keep["cig"],
                  C.cast(keep["pool"], C.POINTER(C.c_char)), 1, 0)
    return SiteHits(C.pointer(h), _keep=(h, keep))


def synth_dna(n: int, seed: int) -> bytes:
    buf = C.create_string_buffer(n)
    lib().fasim_synth_dna(buf, n, seed)
    return buf.raw[:n]


def parse_dna_header(header: str):
    """'>species|chr|start-end' -> (species, chr, start) like readDna() (Fasim-LongTarget.cpp:226-255)."""
    species = chro = start = ""
    tmp, j = "", 0
    for c in header.lstrip(">"):
        if c == "|" and j == 0:
            species, tmp, j = tmp, "", 1
        elif c == "|" and j == 1:
            chro, tmp, j = tmp, "", 2
        elif c == "-" and j == 2:
            start, tmp = tmp, ""
        else:
            tmp += c
    digits = ""
    for c in start.strip():
        if c.isdigit() or (c in "+-" and not digits):
            digits += c
        else:
            break
    try:
        st = int(digits)
    except ValueError:
        st = 0
    return species, chro, st
