"""finito_amd -- MI355X-native search-fmin k-mer localization (host binding over the C ABI).

Thin ctypes plumbing over libfinito_amd.so (include/finito_amd.h).  The class and function names mirror the
reference's interface for this path: FinimizerIndex.{search, load, serialize, size_in_bytes}
(include/FinimizerIndex.hh:26-259) and run_fmin_queries_streaming (include/search_fmin.hh:33-84).

There is no CPU search path in this package: if the HIP library is missing or no device is present the query
calls raise.  The CPU oracle under oracle/ is test infrastructure and is never imported from here.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, "libfinito_amd.so")
_LIB = None

FIN_FWD, FIN_MERGED = 0, 1
FIN_OK, FIN_EINVAL, FIN_EIO, FIN_ENODEV, FIN_ENOMEM, FIN_ELIMIT = 0, -1, -2, -3, -4, -5   # include/finito_amd.h
X_C, X_PLANE_A, X_LCS, X_FMIN, X_USTART, X_GOFF, X_ENDS, X_CONCAT = 0, 1, 5, 6, 7, 8, 9, 10
DT_PTAB, DT_JTAB, DT_FILT, DT_SAFE, DT_RCWIN, DT_CBF, DT_FBF = range(7)   # fin_index_debug_table


class AbundanceInfo(C.Structure):
    """fin_abundance_info of include/finito_amd.h"""
    _fields_ = [("n_classes", C.c_uint64), ("n_reads", C.c_uint64), ("n_unaligned", C.c_uint64), ("iters", C.c_uint32), ("converged", C.c_uint32),
                ("loglik", C.c_double), ("max_change", C.c_double)]


class FinitoError(RuntimeError):
    """std::runtime_error of the reference (caught in src/main.cpp:51-57)."""

    def __init__(self, code, msg):
        super().__init__("%s (code %d)" % (msg, code))
        self.code = code


def host_threads():
    """Usable host cores: affinity mask capped by the cgroup CPU quota (a GPU box hands each GPU a share of its cores)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    n = min(n, max(1, q // int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())))
            break
        except Exception:
            continue
    return max(1, min(n, int(os.environ.get("FINITO_THREADS", "64"))))


def build_native(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    cmd = ["make", "-s", "-C", src, "all"]
    if force:
        cmd.insert(1, "-B")
    subprocess.check_call(cmd)
    return _LIBPATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIBPATH):
            raise FinitoError(-3, "libfinito_amd.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                                  "there is no fallback path")
        L = C.CDLL(_LIBPATH)
        vp, i64, u64, cp = C.c_void_p, C.c_int64, C.c_uint64, C.c_char_p
        u64p, i64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        L.fin_version.restype = cp
        L.fin_host_threads.restype = C.c_int
        L.fin_index_build.argtypes = [cp, u64p, u64, C.c_int, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_index_save.argtypes = [vp, cp, cp, C.c_size_t]
        L.fin_index_load.argtypes = [cp, C.POINTER(vp), cp, C.c_size_t]
        L.fin_index_free.argtypes = [vp]
        L.fin_index_save_reference_layout.argtypes = [vp, cp, cp, C.c_size_t]
        L.fin_index_load_reference_layout.argtypes = [cp, C.POINTER(vp), cp, C.c_size_t]
        L.fin_index_save_sbwt.argtypes = [vp, cp, cp, C.c_size_t]
        L.fin_sbwt_file_info.argtypes = [cp, i64p, i64p, i64p, cp, C.c_size_t]
        L.fin_index_check_against_files.argtypes = [vp, cp, cp, cp, C.c_size_t]
        for f in ("fin_index_k", "fin_index_n_nodes", "fin_index_n_kmers", "fin_index_n_unitigs", "fin_index_n_finimizers",
                  "fin_index_total_len", "fin_index_size_in_bytes"):
            getattr(L, f).restype = i64
            getattr(L, f).argtypes = [vp]
        L.fin_index_export_size.restype = i64
        L.fin_index_export_size.argtypes = [vp, C.c_int]
        L.fin_index_export.argtypes = [vp, C.c_int, vp, u64, cp, C.c_size_t]
        L.fin_index_to_device.argtypes = [vp, C.c_int, cp, C.c_size_t]
        L.fin_index_prefix_table_depth.argtypes = [vp, C.c_int]
        L.fin_index_jump_table_depth.argtypes = [vp, C.c_int]
        L.fin_index_filter_depth.argtypes = [vp, C.c_int]
        L.fin_index_seed_table_bytes.argtypes = [vp, C.c_int]
        L.fin_index_seed_table_bytes.restype = C.c_int64
        L.fin_index_is_disjoint.argtypes = [vp]
        L.fin_index_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.fin_index_clear_option.argtypes = [vp, C.c_char_p]
        L.fin_index_kmer_table_bytes.argtypes = [vp, C.c_int]
        L.fin_index_kmer_table_bytes.restype = C.c_int64
        L.fin_index_string_filter_bytes.argtypes = [vp, C.c_int]
        L.fin_index_string_filter_bytes.restype = C.c_int64
        L.fin_index_replica_table_bytes.argtypes = [vp, C.c_int]
        L.fin_index_replica_table_bytes.restype = C.c_int64
        L.fin_index_rc_pairs.argtypes = [vp, C.c_int]
        L.fin_index_rc_pairs.restype = C.c_int64
        L.fin_index_unsafe_places.argtypes = [vp, C.c_int]
        L.fin_index_unsafe_places.restype = C.c_int64
        L.fin_index_anchor_build_ms.argtypes = [vp, C.c_int]
        L.fin_index_anchor_build_ms.restype = C.c_double
        L.fin_index_debug_seed_table.argtypes = [vp, C.c_int, vp, cp, C.c_size_t]
        L.fin_index_debug_table_bytes.argtypes = [vp, C.c_int, C.c_int]
        L.fin_index_debug_table_bytes.restype = C.c_int64
        L.fin_index_debug_table.argtypes = [vp, C.c_int, C.c_int, vp, u64, cp, C.c_size_t]
        L.fin_index_string_filter_geometry.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.fin_index_finimizer_stats.argtypes = [vp, cp, u64p, u64, C.c_int, i64, i64p, i64p, i64p, cp, C.c_size_t]
        L.fin_search.argtypes = [vp, cp, i64, i64p, i64p, cp, C.c_size_t]
        L.fin_search_batch.argtypes = [vp, cp, u64p, u64, C.c_int, i32p, u64p, cp, C.c_size_t]
        L.fin_batch_create.argtypes = [vp, cp, u64p, u64, C.POINTER(vp), cp, C.c_size_t]
        L.fin_batch_create_on.argtypes = [vp, C.c_int, cp, u64p, u64, C.POINTER(vp), cp, C.c_size_t]
        L.fin_search_batch_multi.argtypes = [vp, C.POINTER(C.c_int), C.c_int, cp, u64p, u64, C.c_int, i32p, u64p, cp, C.c_size_t]
        L.fin_device_count.restype = C.c_int
        L.fin_host_alloc.restype = vp
        L.fin_host_alloc.argtypes = [C.c_size_t]
        L.fin_host_free.argtypes = [vp]
        L.fin_batch_run.argtypes = [vp, C.c_int, vp, cp, C.c_size_t]
        L.fin_batch_reload.argtypes = [vp, cp, u64p, u64, cp, C.c_size_t]
        L.fin_batch_n_kmers.restype = u64
        L.fin_batch_n_kmers.argtypes = [vp]
        L.fin_batch_n_base_strands.restype = u64
        L.fin_batch_n_base_strands.argtypes = [vp]
        L.fin_batch_set_pairs.argtypes = [vp, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
        L.fin_batch_set_records.argtypes = [vp, vp, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
        L.fin_batch_records.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_batch_download_records.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_batch_device_pairs.restype = vp
        L.fin_batch_device_pairs.argtypes = [vp]
        L.fin_batch_download.argtypes = [vp, i32p, u64p, cp, C.c_size_t]
        L.fin_batch_kernel_time.argtypes = [vp, C.POINTER(C.c_double), u64p]
        L.fin_batch_format_text.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_batch_download_text.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_text_mode.argtypes = [vp, C.c_int]
        L.fin_text_create.restype = vp
        L.fin_text_free.argtypes = [vp]
        L.fin_text_data.restype = vp
        L.fin_text_data.argtypes = [vp]
        L.fin_text_size.restype = u64
        L.fin_text_size.argtypes = [vp]
        L.fin_search_batch_text.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u64p, cp, C.c_size_t]
        L.fin_batch_download_range.argtypes = [vp, u64, u64, i32p, cp, C.c_size_t]
        L.fin_batch_step_time.argtypes = [vp, u64, C.POINTER(C.c_double), u64p]
        L.fin_batch_free.argtypes = [vp]
        L.fin_batch_overflow_reads.restype = i64
        L.fin_batch_overflow_reads.argtypes = [vp]
        L.fin_format_pairs.restype = i64
        L.fin_format_pairs.argtypes = [i32p, i64, cp]
        L.fin_hits_create.argtypes = [vp, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_hits_reset.argtypes = [vp, vp]
        L.fin_batch_add_hits.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_hits_device_counts.restype = vp
        L.fin_hits_device_counts.argtypes = [vp]
        L.fin_hits_download.argtypes = [vp, u64p, u64p, cp, C.c_size_t]
        L.fin_hits_free.argtypes = [vp]
        L.fin_search_batch_unitig_counts.argtypes = [vp, cp, u64p, u64, C.c_int, u64p, u64p, cp, C.c_size_t]
        L.fin_search_batch_add_hits.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_records_unitig_counts.argtypes = [vp, u64, vp, u64, C.c_int, u64, u64p, C.c_int]
        L.fin_cover_create.argtypes = [vp, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_cover_reset.argtypes = [vp, vp]
        L.fin_batch_add_cover.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_cover_device_bits.restype = vp
        L.fin_cover_device_bits.argtypes = [vp]
        L.fin_cover_download.argtypes = [vp, u64p, u64p, u64p, cp, C.c_size_t]
        L.fin_cover_free.argtypes = [vp]
        L.fin_search_batch_add_cover.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_search_batch_unitig_coverage.argtypes = [vp, cp, u64p, u64, C.c_int, u64p, u64p, cp, C.c_size_t]
        L.fin_records_cover.argtypes = [vp, u64, vp, u64, C.c_int, i64p, u64, u64p, C.c_int]
        L.fin_depth_create.argtypes = [vp, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_depth_reset.argtypes = [vp, vp]
        L.fin_batch_add_depth.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_depth_device_diff.restype = vp
        L.fin_depth_device_diff.argtypes = [vp]
        L.fin_depth_download.argtypes = [vp, C.c_uint32, vp, vp, u64p, cp, C.c_size_t]
        L.fin_depth_free.argtypes = [vp]
        L.fin_search_batch_add_depth.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_search_batch_unitig_depth.argtypes = [vp, cp, u64p, u64, C.c_int, C.c_uint32, vp, u64p, cp, C.c_size_t]
        L.fin_records_depth.argtypes = [vp, u64, vp, u64, C.c_int, i64p, u64, vp, C.c_int]
        L.fin_pileup_create.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(vp), cp, C.c_size_t]
        L.fin_pileup_reset.argtypes = [vp, vp]
        L.fin_batch_add_pileup.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_pileup_device_alt.restype = vp
        L.fin_pileup_device_alt.argtypes = [vp]
        L.fin_pileup_device_cover_diff.restype = vp
        L.fin_pileup_device_cover_diff.argtypes = [vp]
        L.fin_pileup_download.argtypes = [vp, vp, vp, u64p, cp, C.c_size_t]
        L.fin_pileup_call.argtypes = [vp, C.c_uint32, C.c_uint32, vp, u64, u64p, cp, C.c_size_t]
        L.fin_pileup_free.argtypes = [vp]
        L.fin_search_batch_add_pileup.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_records_pileup.argtypes = [vp, u64, vp, u64, C.c_int, cp, u64p, i64p, u64, vp, C.c_uint32, vp, vp, u64p, C.c_int]
        L.fin_batch_segments.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_batch_device_segments.argtypes = [vp]
        L.fin_batch_device_segments.restype = vp
        L.fin_batch_device_segment_offsets.argtypes = [vp]
        L.fin_batch_device_segment_offsets.restype = vp
        L.fin_batch_download_segments.argtypes = [vp, u64p, vp, cp, C.c_size_t]
        L.fin_search_batch_segments.argtypes = [vp, cp, u64p, u64, C.c_int, u64p, vp, u64, u64p, u64p, cp, C.c_size_t]
        L.fin_expand_segments.argtypes = [u64p, vp, u64, vp, vp, u64p, C.c_int]
        L.fin_records_segments.argtypes = [vp, u64, vp, u64, C.c_int, u64p, vp, u64, u64p, C.c_int]
        L.fin_batch_read_summaries.argtypes = [vp, cp, C.c_size_t]
        L.fin_batch_device_read_summaries.argtypes = [vp]
        L.fin_batch_device_read_summaries.restype = vp
        L.fin_batch_download_read_summaries.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_screen.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, u64p, cp, C.c_size_t]
        L.fin_batch_device_screen_ids.argtypes = [vp]
        L.fin_batch_device_screen_ids.restype = vp
        L.fin_batch_device_screen_bits.argtypes = [vp]
        L.fin_batch_device_screen_bits.restype = vp
        L.fin_batch_download_screen.argtypes = [vp, vp, u64p, cp, C.c_size_t]
        L.fin_search_batch_read_summaries.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u64p, cp, C.c_size_t]
        L.fin_search_batch_screen.argtypes = [vp, cp, u64p, u64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, u64p, u64p, cp, C.c_size_t]
        L.fin_records_read_summaries.argtypes = [vp, u64, vp, u64, C.c_int, vp, C.c_int]
        u32 = C.c_uint32
        L.fin_labels_create.argtypes = [vp, C.c_int, vp, u32, C.POINTER(vp), cp, C.c_size_t]
        L.fin_labels_reset.argtypes = [vp, vp]
        L.fin_labels_device_labels.argtypes = [vp]
        L.fin_labels_device_labels.restype = vp
        L.fin_labels_device_reads.argtypes = [vp]
        L.fin_labels_device_reads.restype = vp
        L.fin_labels_download.argtypes = [vp, u64p, u64p, cp, C.c_size_t]
        L.fin_labels_free.argtypes = [vp]
        L.fin_labels_free.restype = None
        L.fin_batch_classify.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_device_read_classes.argtypes = [vp]
        L.fin_batch_device_read_classes.restype = vp
        L.fin_batch_download_read_classes.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_add_classes.argtypes = [vp, vp, u32, u32, u32, vp, cp, C.c_size_t]
        L.fin_search_batch_classify.argtypes = [vp, cp, u64p, u64, C.c_int, vp, vp, u64p, cp, C.c_size_t]
        L.fin_search_batch_add_classes.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, u32, cp, C.c_size_t]
        L.fin_records_read_classes.argtypes = [vp, u64, vp, u64, C.c_int, vp, u64, vp, C.c_int]
        L.fin_index_unitig_numbers.argtypes = [vp, cp, u64p, u64, vp, cp, C.c_size_t]
        L.fin_taxonomy_create.argtypes = [vp, C.c_int, vp, u64, vp, C.POINTER(vp), cp, C.c_size_t]
        L.fin_taxonomy_create_from_colors.argtypes = [vp, vp, u64, vp, C.POINTER(vp), cp, C.c_size_t]
        L.fin_taxonomy_device_labels.argtypes = [vp]
        L.fin_taxonomy_device_labels.restype = vp
        L.fin_taxonomy_download_labels.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_taxonomy_reset.argtypes = [vp, vp]
        L.fin_taxonomy_download.argtypes = [vp, u64p, u64p, u64p, cp, C.c_size_t]
        L.fin_taxonomy_free.argtypes = [vp]
        L.fin_taxonomy_free.restype = None
        L.fin_batch_taxa.argtypes = [vp, vp, u32, u32, cp, C.c_size_t]
        L.fin_batch_device_read_taxa.argtypes = [vp]
        L.fin_batch_device_read_taxa.restype = vp
        L.fin_batch_download_read_taxa.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_add_taxa.argtypes = [vp, vp, u32, u32, vp, cp, C.c_size_t]
        L.fin_search_batch_taxa.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, vp, u64p, cp, C.c_size_t]
        L.fin_search_batch_add_taxa.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, cp, C.c_size_t]
        L.fin_unitig_lca_labels.argtypes = [u64p, u64, u32, vp, u64, vp, vp, C.c_int]
        L.fin_records_read_taxa.argtypes = [vp, u64, vp, u64, C.c_int, vp, u64, vp, u64, u32, u32, vp, C.c_int]
        L.fin_taxa_clade_reads.argtypes = [u64p, vp, u64, u64p]
        L.fin_colors_create.argtypes = [vp, C.c_int, u32, C.POINTER(vp), cp, C.c_size_t]
        L.fin_colors_upload.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_colors_reset.argtypes = [vp, vp]
        L.fin_colors_device_bits.argtypes = [vp]
        L.fin_colors_device_bits.restype = vp
        L.fin_colors_n_colors.argtypes = [vp]
        L.fin_colors_n_colors.restype = u32
        L.fin_colors_words.argtypes = [vp]
        L.fin_colors_words.restype = u32
        L.fin_colors_download.argtypes = [vp, u64p, u64p, cp, C.c_size_t]
        L.fin_colors_free.argtypes = [vp]
        L.fin_colors_free.restype = None
        u32p = C.POINTER(C.c_uint32)
        L.fin_colors_compact.argtypes = [vp, u64, vp, cp, C.c_size_t]
        L.fin_colors_expand.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_colors_is_compact.argtypes = [vp]
        L.fin_colors_n_sets.argtypes = [vp]
        L.fin_colors_n_sets.restype = u64
        L.fin_colors_device_set_of.argtypes = [vp]
        L.fin_colors_device_set_of.restype = vp
        L.fin_colors_device_sets.argtypes = [vp]
        L.fin_colors_device_sets.restype = vp
        L.fin_colors_download_sets.argtypes = [vp, u32p, u64p, u64, u64p, cp, C.c_size_t]
        L.fin_colors_upload_sets.argtypes = [vp, u32p, u64p, u64, cp, C.c_size_t]
        L.fin_colors_compact_stats.argtypes = [vp, u64p]
        L.fin_unitig_color_sets.argtypes = [u64p, u64, u32, u32p, u64p, u64, u64p, C.c_int]
        L.fin_color_sets_expand.argtypes = [u32p, u64p, u64, u64, u32, u64p, C.c_int]
        L.fin_batch_add_colors.argtypes = [vp, vp, u32, vp, cp, C.c_size_t]
        L.fin_search_batch_add_colors.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, cp, C.c_size_t]
        L.fin_batch_pseudoalign.argtypes = [vp, vp, u32, cp, C.c_size_t]
        L.fin_batch_device_pseudo_rows.argtypes = [vp]
        L.fin_batch_device_pseudo_rows.restype = vp
        L.fin_batch_device_pseudo_heads.argtypes = [vp]
        L.fin_batch_device_pseudo_heads.restype = vp
        L.fin_batch_download_pseudo.argtypes = [vp, u64p, vp, cp, C.c_size_t]
        L.fin_search_batch_pseudoalign.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u64p, vp, u64p, cp, C.c_size_t]
        L.fin_records_pseudoalign.argtypes = [vp, u64, vp, u64, C.c_int, u64p, u64, u32, u32, u64p, vp, C.c_int]
        L.fin_batch_pseudoalign_paired.argtypes = [vp, vp, u32, u32, cp, C.c_size_t]
        L.fin_batch_device_pair_rows.argtypes = [vp]
        L.fin_batch_device_pair_rows.restype = vp
        L.fin_batch_device_pair_heads.argtypes = [vp]
        L.fin_batch_device_pair_heads.restype = vp
        L.fin_batch_download_pair_pseudo.argtypes = [vp, u64p, vp, cp, C.c_size_t]
        L.fin_batch_add_eqclasses_paired.argtypes = [vp, vp, u32, u32, vp, cp, C.c_size_t]
        L.fin_search_batch_pseudoalign_paired.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, u64p, vp, u64p, cp, C.c_size_t]
        L.fin_search_batch_add_eqclasses_paired.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, cp, C.c_size_t]
        L.fin_records_pseudoalign_paired.argtypes = [vp, u64, vp, u64, C.c_int, u64p, u64, u32, u32, u32, u64p, vp, C.c_int]
        L.fin_fragments_create.argtypes = [vp, C.c_int, u32, u32, C.POINTER(vp), cp, C.c_size_t]
        L.fin_fragments_reset.argtypes = [vp, vp]
        L.fin_fragments_free.argtypes = [vp]
        L.fin_fragments_free.restype = None
        L.fin_batch_add_fragments.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_fragments_download.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_fragments_device_hist.argtypes = [vp]
        L.fin_fragments_device_hist.restype = vp
        L.fin_batch_fragments.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_batch_download_fragments.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_batch_device_fragments.argtypes = [vp]
        L.fin_batch_device_fragments.restype = vp
        L.fin_search_batch_add_fragments.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_search_batch_fragments.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_records_fragments.argtypes = [vp, u64, vp, u64, C.c_int, i64p, u64, u32, u32, vp, vp, vp, C.c_int]
        L.fin_link_hash.argtypes = [u64]
        L.fin_link_hash.restype = u64
        L.fin_links_create.argtypes = [vp, C.c_int, u64, C.POINTER(vp), cp, C.c_size_t]
        L.fin_links_reset.argtypes = [vp, vp]
        L.fin_links_free.argtypes = [vp]
        L.fin_links_free.restype = None
        L.fin_batch_add_links.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_links_download.argtypes = [vp, u64, vp, u64, u64p, vp, cp, C.c_size_t]
        L.fin_links_device_table.argtypes = [vp]
        L.fin_links_device_table.restype = vp
        L.fin_links_capacity.argtypes = [vp]
        L.fin_links_capacity.restype = u64
        L.fin_search_batch_add_links.argtypes = [vp, cp, u64p, u64, C.c_int, vp, cp, C.c_size_t]
        L.fin_records_links.argtypes = [vp, u64, vp, u64, C.c_int, i64p, u64, u64, vp, u64, u64p, vp, C.c_int]
        L.fin_refpaths_create.argtypes = [vp, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_refpaths_reset.argtypes = [vp, vp]
        L.fin_refpaths_free.argtypes = [vp]
        L.fin_refpaths_free.restype = None
        for f in ("n_seqs", "n_segments", "n_slots"):
            getattr(L, "fin_refpaths_" + f).argtypes = [vp]
            getattr(L, "fin_refpaths_" + f).restype = u64
        L.fin_refpaths_download.argtypes = [vp, vp, vp, vp, cp, C.c_size_t]
        L.fin_refpaths_upload.argtypes = [vp, vp, vp, vp, u64, cp, C.c_size_t]
        L.fin_refpaths_device_segments.argtypes = [vp]
        L.fin_refpaths_device_segments.restype = vp
        L.fin_refpaths_device_segment_offsets.argtypes = [vp]
        L.fin_refpaths_device_segment_offsets.restype = vp
        L.fin_batch_add_refpaths.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_search_batch_add_refpaths.argtypes = [vp, cp, u64p, u64, vp, cp, C.c_size_t]
        L.fin_refpaths_depth.argtypes = [vp, vp, u32, u32, vp, vp, u64, u64p, cp, C.c_size_t]
        L.fin_refpaths_lift_variants.argtypes = [vp, vp, u64, vp, u64, u64p, cp, C.c_size_t]
        L.fin_segments_check.argtypes = [vp, vp, vp, u64, C.c_int, i64p, u64, cp, C.c_size_t]
        L.fin_segments_window_depth.argtypes = [vp, vp, vp, u64, C.c_int, i64p, u64, vp, u32, u32, vp, vp, u64, u64p, C.c_int, cp, C.c_size_t]
        L.fin_segments_lift_variants.argtypes = [vp, vp, vp, u64, C.c_int, i64p, u64, vp, u64, vp, u64, u64p, C.c_int, cp, C.c_size_t]
        L.fin_effective_lengths.argtypes = [vp, u32, u32, vp, u64, vp]
        L.fin_eqclasses_create.argtypes = [vp, u64, C.POINTER(vp), cp, C.c_size_t]
        L.fin_eqclasses_reset.argtypes = [vp, vp]
        L.fin_eqclasses_free.argtypes = [vp]
        L.fin_eqclasses_free.restype = None
        L.fin_eqclasses_add_rows.argtypes = [vp, vp, u64, vp, cp, C.c_size_t]
        L.fin_eqclasses_add_classes.argtypes = [vp, vp, vp, u64, u64, vp, cp, C.c_size_t]
        L.fin_eqclasses_add_classes_host.argtypes = [vp, u64p, u64p, u64, u64, cp, C.c_size_t]
        L.fin_eqclasses_merge.argtypes = [vp, vp, vp, cp, C.c_size_t]
        L.fin_classes_merge.argtypes = [u64p, u64p, u64, u64p, u64p, u64, u32, u64p, u64p, u64, u64p]
        L.fin_batch_add_eqclasses.argtypes = [vp, vp, u32, vp, cp, C.c_size_t]
        L.fin_search_batch_add_eqclasses.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, cp, C.c_size_t]
        L.fin_eqclasses_download.argtypes = [vp, u64p, u64p, u64, u64p, u64p, cp, C.c_size_t]
        L.fin_eqclasses_stats.argtypes = [vp, u64p, cp, C.c_size_t]
        L.fin_rows_eqclasses.argtypes = [u64p, u64, u32, u64p, u64p, u64, u64p, u64p]
        L.fin_eqclasses_color_tally.argtypes = [u64p, u64p, u64, u32, u64p, u64p]
        f64p = C.POINTER(C.c_double)
        L.fin_eqclasses_abundance.argtypes = [vp, f64p, u32, C.c_double, f64p, f64p, C.POINTER(AbundanceInfo), cp, C.c_size_t]
        L.fin_classes_abundance.argtypes = [u64p, u64p, u64, u32, f64p, u32, C.c_double, f64p, f64p, C.POINTER(AbundanceInfo), C.c_int]
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        L.fin_bootstrap_check.argtypes = [u64, u32, cp, C.c_size_t]
        L.fin_eqclasses_bootstrap.argtypes = [vp, f64p, u32, C.c_double, u32, u64, f64p, C.POINTER(AbundanceInfo), f64p, u64p, u32p, u8p, cp, C.c_size_t]
        L.fin_classes_resample.argtypes = [u64p, u64p, u64, u32, u64, u32, u64p, C.c_int]
        L.fin_classes_bootstrap.argtypes = [u64p, u64p, u64, u32, f64p, u32, C.c_double, u32, u64, f64p, C.POINTER(AbundanceInfo), f64p, u64p, u32p, u8p, C.c_int]
        L.fin_assign_create.argtypes = [vp, f64p, f64p, C.POINTER(vp), cp, C.c_size_t]
        L.fin_assign_reset.argtypes = [vp, vp]
        L.fin_assign_free.argtypes = [vp]
        L.fin_assign_free.restype = None
        L.fin_assign_set.argtypes = [vp, f64p, f64p, vp, cp, C.c_size_t]
        L.fin_assign_rows.argtypes = [vp, vp, u64, vp, vp, vp, cp, C.c_size_t]
        L.fin_assign_download.argtypes = [vp, u64p, u64p, u64p, cp, C.c_size_t]
        L.fin_batch_assign.argtypes = [vp, vp, u32, u32, vp, cp, C.c_size_t]
        L.fin_batch_device_assign_rows.restype = vp
        L.fin_batch_device_assign_rows.argtypes = [vp]
        L.fin_batch_device_assign_heads.restype = vp
        L.fin_batch_device_assign_heads.argtypes = [vp]
        L.fin_batch_download_assign.argtypes = [vp, u64p, vp, cp, C.c_size_t]
        L.fin_batch_assign_bin.argtypes = [vp, u32, u64p, cp, C.c_size_t]
        L.fin_batch_device_bin_ids.restype = vp
        L.fin_batch_device_bin_ids.argtypes = [vp]
        L.fin_batch_download_bin.argtypes = [vp, u32p, cp, C.c_size_t]
        L.fin_search_batch_assign.argtypes = [vp, cp, u64p, u64, C.c_int, vp, u32, u32, u64p, vp, cp, C.c_size_t]
        L.fin_rows_assign.argtypes = [u64p, u64, u32, f64p, f64p, u64p, vp, u64p, u64p, u64p, C.c_int]
        L.fin_colors_coverage.argtypes = [vp, vp, vp, u32, vp, vp, cp, C.c_size_t]
        L.fin_unitig_color_coverage.argtypes = [u64p, u64, u32, u64p, u64p, vp, vp, vp, C.c_int]
        L.fin_colors_shared.argtypes = [vp, vp, vp, vp, cp, C.c_size_t]
        L.fin_unitig_color_shared.argtypes = [u64p, u64, u32, u64p, u64p, C.c_int]
        L.fin_depth_histogram.argtypes = [vp, u32, u32, vp, cp, C.c_size_t]
        L.fin_colors_depth_histogram.argtypes = [vp, vp, u32, u32, vp, vp, cp, C.c_size_t]
        L.fin_depth_positions_histogram.argtypes = [vp, vp, u64, C.c_int, u32, u32, vp, C.c_int]
        L.fin_unitig_color_depth_histogram.argtypes = [vp, vp, u64, C.c_int, vp, u32, u32, u32, vp, vp, C.c_int]
        _LIB = L
    return _LIB


def sbwt_file_info(path):
    """(k, nodes, k-mers) of an SBWT file written by `sbwt build` (plain-matrix variant)"""
    k, n, m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    err = C.create_string_buffer(512)
    _check(lib().fin_sbwt_file_info(str(path).encode(), C.byref(k), C.byref(n), C.byref(m), err, 512), err)
    return int(k.value), int(n.value), int(m.value)


def _check(rc, errbuf):
    if rc != 0:
        raise FinitoError(rc, errbuf.value.decode(errors="replace") or "finito_amd call failed")


def flatten(seqs):
    """list of str/bytes -> (uint8 bases, uint64 offsets[n+1]); (bases, offsets) arrays pass through."""
    if isinstance(seqs, tuple) and len(seqs) == 2 and isinstance(seqs[0], np.ndarray):
        return np.ascontiguousarray(seqs[0], dtype=np.uint8), np.ascontiguousarray(seqs[1], dtype=np.uint64)
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    joined = b"".join(bs)
    bases = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    return bases, offsets


class PinnedArray:
    """numpy view of page-locked host memory (fin_host_alloc): PCIe copies to/from it run at link speed."""

    def __init__(self, shape, dtype):
        self.L = lib()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self.L.fin_host_alloc(max(n, 1))
        if not self.ptr:
            raise FinitoError(-4, "fin_host_alloc failed (no HIP device or out of pinned memory)")
        buf = (C.c_char * max(n, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.L.fin_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QueryResult:
    """FinimizerIndex::QueryResult (FinimizerIndex.hh:30-33)."""

    def __init__(self, local_offsets, n_found):
        self.local_offsets = local_offsets
        self.n_found = n_found


class Batch:
    """Reads resident in HBM with their output buffer (fin_batch_* of the C ABI)."""

    def __init__(self, index, reads):
        self.index = index
        self.L = lib()
        bases, offsets = flatten(reads)
        self._keep = (bases, offsets)
        self.n_reads = len(offsets) - 1
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_create(index.h, *_reads_args((bases, offsets)), C.byref(h), err, 512), err)
        self.h = h
        self._keep = None   # the reads live in HBM now

    def reload(self, reads):
        """Replace the reads of this batch, keeping its device buffers (fin_batch_reload)."""
        bases, offsets = flatten(reads)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_reload(self.h, *_reads_args((bases, offsets)), err, 512), err)
        self.n_reads = len(offsets) - 1

    @property
    def n_kmers(self):
        return int(self.L.fin_batch_n_kmers(self.h))

    @property
    def n_base_strands(self):
        return int(self.L.fin_batch_n_base_strands(self.h))

    def run(self, strands=FIN_MERGED, stream=None):
        """Enqueue the search on a HIP stream (int handle, e.g. torch.cuda.current_stream().cuda_stream); no sync."""
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_run(self.h, strands, C.c_void_p(stream or 0), err, 512), err)

    def download(self, want_pairs=True, want_positive=True):
        n = self.n_kmers
        out = np.empty((max(n, 1), 2), dtype=np.int32) if want_pairs else None
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_download(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)) if want_pairs else None,
                                         C.byref(npos) if want_positive else None, err, 512), err)
        return (out[:n] if want_pairs else None), int(npos.value)

    def text(self):
        """the reference's output text of this batch's pairs, formatted on the device (fin_batch_format_text): bytes"""
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_format_text(self.h, C.byref(n), err, 512), err)
        buf = C.create_string_buffer(max(int(n.value), 1))
        _check(self.L.fin_batch_download_text(self.h, buf, err, 512), err)
        return buf.raw[:int(n.value)]

    def text_mode(self, mode):
        """0: pairs (default); 1: pairs + the fast path's per-read records (the text is made from them); 2: text only (fin_batch_text_mode)"""
        if self.L.fin_batch_text_mode(self.h, int(mode)) != 0:
            raise FinitoError("fin_batch_text_mode(%r)" % (mode,))

    def format_text(self):
        """format the reference's output text of this batch's pairs on the device and leave it there (fin_batch_format_text): bytes
        of text.  Runs on the stream of the last run(); returns after the text is complete."""
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_format_text(self.h, C.byref(n), err, 512), err)
        return int(n.value)

    def download_range(self, first_pair, n_pairs):
        """int32 pairs [first_pair, first_pair + n_pairs) of the output (fin_batch_download_range)"""
        out = np.empty((max(n_pairs, 1), 2), dtype=np.int32)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_download_range(self.h, int(first_pair), int(n_pairs), out.ctypes.data_as(C.POINTER(C.c_int32)), err, 512), err)
        return out[:n_pairs]

    def set_pairs(self, pairs):
        """diagnostic: overwrite the batch's pairs in HBM (fin_batch_set_pairs) -- for tests of the text formatter"""
        a = np.ascontiguousarray(pairs, dtype=np.int32)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_set_pairs(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)), err, 512), err)

    def set_records(self, recs, pairs=None):
        """diagnostic: overwrite the records the most recent run left -- and, with `pairs`, the batch's pairs -- in HBM (fin_batch_set_records) -- for tests of
        the record consumers.  Refused unless that run left records and every record passes the host-side checks of include/finito_amd.h"""
        r = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        if len(r) != self.n_reads:
            raise FinitoError(FIN_EINVAL, "set_records: %d records for %d reads" % (len(r), self.n_reads))
        a = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        if a is not None and a.size != 2 * self.n_kmers:
            raise FinitoError(FIN_EINVAL, "set_records: %d pair words for %d k-mers" % (a.size, self.n_kmers))
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_set_records(self.h, r.ctypes.data_as(C.c_void_p), None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)), err, 512), err)

    def records(self):
        """the most recent run's results as records + stream (fin_batch_records + fin_batch_download_records): (recs RECORD_DTYPE[n_reads], int32 stream [n, 2] --
        the pairs of the kind-0 reads in read order)"""
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_records(self.h, C.byref(n), err, 512), err)
        recs = np.zeros(max(self.n_reads, 1), dtype=RECORD_DTYPE)
        stream = np.zeros((max(int(n.value), 1), 2), dtype=np.int32)
        _check(self.L.fin_batch_download_records(self.h, recs.ctypes.data_as(C.c_void_p), stream.ctypes.data_as(C.c_void_p), err, 512), err)
        return recs[: self.n_reads], stream[: int(n.value)]

    def device_pairs_ptr(self):
        return int(self.L.fin_batch_device_pairs(self.h) or 0)

    def segments(self):
        """the most recent run's results as segments, made on the device (fin_batch_segments + fin_batch_download_segments): (seg_offs uint64[n_reads + 1],
        segs SEGMENT_DTYPE[n_segments]) -- read r's segments are segs[seg_offs[r]:seg_offs[r + 1]]"""
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_segments(self.h, C.byref(n), err, 512), err)
        seg_offs = np.zeros(self.n_reads + 1, dtype=np.uint64)
        segs = np.zeros(max(int(n.value), 1), dtype=SEGMENT_DTYPE)
        _check(self.L.fin_batch_download_segments(self.h, seg_offs.ctypes.data_as(C.POINTER(C.c_uint64)), segs.ctypes.data_as(C.c_void_p), err, 512), err)
        return seg_offs, segs[: int(n.value)]

    def device_segments_ptr(self):
        """(segments, seg_offs) device pointers, 0 before segments()"""
        return int(self.L.fin_batch_device_segments(self.h) or 0), int(self.L.fin_batch_device_segment_offsets(self.h) or 0)

    def read_summaries(self):
        """the most recent run's results as one summary per read, made on the device (fin_batch_read_summaries + fin_batch_download_read_summaries):
        READ_SUMMARY_DTYPE[n_reads] -- n_found, n_segments, longest, span over the read's output slots"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_read_summaries(self.h, err, 512), err)
        out = np.zeros(max(self.n_reads, 1), dtype=READ_SUMMARY_DTYPE)
        _check(self.L.fin_batch_download_read_summaries(self.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[: self.n_reads]

    def device_read_summaries_ptr(self):
        """the summaries' device pointer, 0 before read_summaries() / screen()"""
        return int(self.L.fin_batch_device_read_summaries(self.h) or 0)

    def screen(self, min_found=1, min_permille=0, invert=False):
        """the reads that pass (n_found >= min_found and 1000 * n_found >= min_permille * nk) != invert, decided on the device (fin_batch_screen +
        fin_batch_download_screen): (ids uint32[n_pass] ascending, bits uint64[(n_reads + 63) // 64] -- bit r & 63 of word r >> 6 is read r's)"""
        if not (0 <= int(min_found) <= 0xFFFFFFFF and 0 <= int(min_permille) <= 0xFFFFFFFF):
            raise FinitoError(FIN_EINVAL, "screen: min_found and min_permille are unsigned 32-bit numbers")
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_screen(self.h, int(min_found), int(min_permille), 1 if invert else 0, C.byref(n), err, 512), err)
        ids = np.zeros(max(int(n.value), 1), dtype=np.uint32)
        bits = np.zeros(max((self.n_reads + 63) // 64, 1), dtype=np.uint64)
        _check(self.L.fin_batch_download_screen(self.h, ids.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.POINTER(C.c_uint64)), err, 512), err)
        return ids[: int(n.value)], bits[: (self.n_reads + 63) // 64]

    def device_screen_ptr(self):
        """(ids, bits) device pointers, 0 before screen()"""
        return int(self.L.fin_batch_device_screen_ids(self.h) or 0), int(self.L.fin_batch_device_screen_bits(self.h) or 0)

    def classify(self, labels):
        """the most recent run's results as one class per read under a labelling (Labels), made on the device (fin_batch_classify +
        fin_batch_download_read_classes): READ_CLASS_DTYPE[n_reads] -- label (FIN_NO_LABEL: none), n_best, n_second, n_labelled"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_classify(self.h, labels.h, err, 512), err)
        out = np.zeros(max(self.n_reads, 1), dtype=READ_CLASS_DTYPE)
        _check(self.L.fin_batch_download_read_classes(self.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[: self.n_reads]

    def taxa(self, tax, min_found=1, confidence=0):
        """the most recent run's results as one taxon per read under a Taxonomy, by Kraken's root-to-leaf rule, made on the device (fin_batch_taxa +
        fin_batch_download_read_taxa): READ_TAXON_DTYPE[n_reads] -- taxon (FIN_NO_LABEL: unclassified), score, clade, n_labelled.  confidence is in thousandths
        of the read's k-mers, 0 .. 1000"""
        t = _taxa_thresholds("Batch.taxa", min_found, confidence)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_taxa(self.h, tax.h, *t, err, 512), err)
        out = np.zeros(max(self.n_reads, 1), dtype=READ_TAXON_DTYPE)
        _check(self.L.fin_batch_download_read_taxa(self.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[: self.n_reads]

    def device_read_taxa_ptr(self):
        """the read taxa's device pointer, 0 before taxa() / Taxonomy.add()"""
        return int(self.L.fin_batch_device_read_taxa(self.h) or 0)

    def device_read_classes_ptr(self):
        """the classes' device pointer, 0 before classify() / Labels.add()"""
        return int(self.L.fin_batch_device_read_classes(self.h) or 0)

    def pseudoalign(self, colors, permille=1000):
        """the most recent run's results as one colour row per read under a colour matrix (Colors), made on the device (fin_batch_pseudoalign +
        fin_batch_download_pseudo): (rows uint64[n_reads, W], heads READ_PSEUDO_DTYPE[n_reads]) -- colour c is in a read's row iff at least permille thousandths
        of its coloured k-mers have it; 1000: the intersection, 0: the union"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_pseudoalign(self.h, colors.h, _permille("Batch.pseudoalign", permille), err, 512), err)
        rows = np.zeros((max(self.n_reads, 1), colors.words), dtype=np.uint64)
        heads = np.zeros(max(self.n_reads, 1), dtype=READ_PSEUDO_DTYPE)
        _check(self.L.fin_batch_download_pseudo(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), heads.ctypes.data_as(C.c_void_p), err, 512), err)
        return rows[: self.n_reads], heads[: self.n_reads]

    def device_pseudo_ptrs(self):
        """(rows, heads) device pointers, 0 before pseudoalign()"""
        return int(self.L.fin_batch_device_pseudo_rows(self.h) or 0), int(self.L.fin_batch_device_pseudo_heads(self.h) or 0)

    def pseudoalign_pairs(self, colors, permille=1000, both=False):
        """the most recent run's reads as interleaved mates -- fragment f is reads 2f and 2f + 1 --, one colour row per FRAGMENT under a colour matrix, made on
        the device (fin_batch_pseudoalign_paired + fin_batch_download_pair_pseudo): (rows uint64[F, W], heads PAIR_PSEUDO_DTYPE[F]).  The definition of
        pseudoalign() over both mates' slots together; at 1000 the AND of the mates' rows where both have coloured k-mers, else the row of the one that has; at 0
        the OR.  both: the row is empty unless both mates have a coloured k-mer (FIN_PAIR_BOTH).  The per-read rows of pseudoalign() are left alone"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_pseudoalign_paired(self.h, colors.h, _permille("Batch.pseudoalign_pairs", permille), FIN_PAIR_BOTH if both else FIN_PAIR_ANY, err, 512), err)
        nf = self.n_reads // 2
        rows = np.zeros((max(nf, 1), colors.words), dtype=np.uint64)
        heads = np.zeros(max(nf, 1), dtype=PAIR_PSEUDO_DTYPE)
        _check(self.L.fin_batch_download_pair_pseudo(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), heads.ctypes.data_as(C.c_void_p), err, 512), err)
        return rows[:nf], heads[:nf]

    def device_pair_ptrs(self):
        """(rows, heads) device pointers of the fragments' rows, 0 before pseudoalign_pairs()"""
        return int(self.L.fin_batch_device_pair_rows(self.h) or 0), int(self.L.fin_batch_device_pair_heads(self.h) or 0)

    def fragments(self):
        """the most recent run's reads as interleaved mates, one FRAGMENT_DTYPE entry per fragment, made on the device (fin_batch_fragments +
        fin_batch_download_fragments; include/finito_amd.h: FRAGMENT GEOMETRY): where the mates lie, which way they face, the class and the length"""
        err = C.create_string_buffer(512)
        nf = C.c_uint64(0)
        _check(self.L.fin_batch_fragments(self.h, C.byref(nf), err, 512), err)
        out = np.zeros(max(int(nf.value), 1), dtype=FRAGMENT_DTYPE)
        _check(self.L.fin_batch_download_fragments(self.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[: int(nf.value)]

    def device_fragments_ptr(self):
        """the fragments' device pointer, 0 before fragments()"""
        return int(self.L.fin_batch_device_fragments(self.h) or 0)

    def assign(self, assigner, permille=1000, pairs=False, both=False, stream=None):
        """the most recent run's reads (pairs: its fragments) assigned to references under an Assign's weights and thresholds, made and counted on the device
        (fin_batch_assign + fin_batch_download_assign): (assigned rows uint64[F, W], heads READ_ASSIGN_DTYPE[F]).  Pseudoaligns first, at `permille`; the
        pseudo rows survive"""
        assigner.add(self, permille, pairs, both, stream)
        n = self.n_reads // 2 if pairs else self.n_reads
        rows = np.zeros((max(n, 1), assigner.words), dtype=np.uint64)
        heads = np.zeros(max(n, 1), dtype=READ_ASSIGN_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_download_assign(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), heads.ctypes.data_as(C.c_void_p), err, 512), err)
        return rows[:n], heads[:n]

    def assign_bin(self, colour):
        """the ascending numbers (uint32) of the reads or fragments of the last assign() that have `colour` assigned, compacted on the device
        (fin_batch_assign_bin + fin_batch_download_bin); device_bin_ptr() is the list in HBM"""
        if not 0 <= int(colour) <= 0xFFFFFFFF:
            raise FinitoError(FIN_EINVAL, "Batch.assign_bin: colour is an unsigned 32-bit number")
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_batch_assign_bin(self.h, int(colour), C.byref(n), err, 512), err)
        ids = np.zeros(max(int(n.value), 1), dtype=np.uint32)
        _check(self.L.fin_batch_download_bin(self.h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), err, 512), err)
        return ids[: int(n.value)]

    def device_assign_ptrs(self):
        """(assigned rows, heads) device pointers, 0 before assign()"""
        return int(self.L.fin_batch_device_assign_rows(self.h) or 0), int(self.L.fin_batch_device_assign_heads(self.h) or 0)

    def device_bin_ptr(self):
        """the bin's ids in HBM, 0 before assign_bin()"""
        return int(self.L.fin_batch_device_bin_ids(self.h) or 0)

    def pipeline_counts(self, n=64):
        """kernel 4's queue counters of the last run (fin_batch_pipeline_counts)"""
        out = (C.c_uint32 * n)()
        self.L.fin_batch_pipeline_counts(self.h, out, n)
        return list(out)

    def overflow_reads(self):
        return int(self.L.fin_batch_overflow_reads(self.h))

    def run_info(self):
        """what the most recent run decided (fin_batch_run_info): {'kernel', 'no_prefill', 'deferred', 'fast_path'}"""
        out = (C.c_uint32 * 4)()
        self.L.fin_batch_run_info(self.h, out)
        return {"kernel": int(out[0]), "no_prefill": bool(out[1]), "deferred": bool(out[2]), "fast_path": bool(out[3])}

    def debug_ingest(self, n_chunks=0):
        """the most recent run's ingest (fin_batch_debug_ingest): (fused, its first n_chunks packed chunks as uint32 words [n, 4], the pre-pass verdicts [n_reads, 2])"""
        fused = C.c_uint32(0)
        ch = np.zeros((n_chunks, 4), dtype=np.uint32)
        pv = np.zeros((self.n_reads, 2), dtype=np.uint32)
        rc = self.L.fin_batch_debug_ingest(self.h, C.byref(fused), ch.ctypes.data_as(C.c_void_p), C.c_uint64(n_chunks), pv.ctypes.data_as(C.c_void_p),
                                           C.c_uint64(2 * self.n_reads))
        if rc != 0:
            raise FinitoError(rc, "fin_batch_debug_ingest")
        return bool(fused.value), ch, pv

    def debug_side_stream(self):
        """diagnostic: the side stream of option "overlap_prefill" as an int handle (fin_batch_debug_side_stream)"""
        self.L.fin_batch_debug_side_stream.restype = C.c_void_p
        self.L.fin_batch_debug_side_stream.argtypes = [C.c_void_p]
        h = self.L.fin_batch_debug_side_stream(self.h)
        if not h:
            raise FinitoError(FIN_ENODEV, "fin_batch_debug_side_stream")
        return int(h)

    def kernel_time_ms(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        self.L.fin_batch_kernel_time(self.h, C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def step_time_ms(self, skip_first=0):
        """({'ingest_prefill', 'probe_prepass', 'search', 'overflow_tail', 'step'} -> ms averaged over the runs after the first
        `skip_first`, number of runs): device time of a step from HIP events on the launch stream (fin_batch_step_time)"""
        p, n = (C.c_double * 5)(), C.c_uint64(0)
        self.L.fin_batch_step_time(self.h, int(skip_first), p, C.byref(n))
        return dict(zip(("ingest_prefill", "probe_prepass", "search", "overflow_tail", "step"), (float(x) for x in p))), int(n.value)

    def close(self):
        if getattr(self, "h", None):
            self.L.fin_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _reads_args(reads):
    """(bases pointer, offsets pointer, n_reads): a read set as the C ABI takes it, `reads` as flatten takes them; the pointers keep their arrays alive"""
    bases, offsets = flatten(reads)
    return bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(offsets) - 1


def _acc_add(acc, fn, batch, stream, *args):
    """the plumbing of every accumulator's add: the batch's most recent run into `acc` by the C function `fn`, on a HIP stream"""
    err = C.create_string_buffer(512)
    _check(getattr(acc.L, fn)(batch.h, acc.h, *args, C.c_void_p(stream or 0), err, 512), err)
    return acc


def _acc_add_reads(acc, fn, reads, strands, *args):
    """... and of every add_reads: a read set from host buffers through the pipeline of acc.index, into `acc` (anything with index, h and L: the C side checks
    that they belong together)"""
    err = C.create_string_buffer(512)
    _check(getattr(acc.L, fn)(acc.index.h, *_reads_args(reads), int(strands), acc.h, *args, err, 512), err)
    return acc


class _Accumulator:
    """what the device accumulators share: the handle's life and reset.  A subclass names its C functions; self.index is the index it lives beside"""
    _FREE = _RESET = None

    def _create(self, fn, *args):
        self.L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(getattr(self.L, fn)(*args, C.byref(h), err, 512), err)
        self.h = h

    def reset(self, stream=None):
        """zero what was accumulated (a labelling itself stays), on a HIP stream, behind the adds issued so far"""
        rc = getattr(self.L, self._RESET)(self.h, C.c_void_p(stream or 0))
        if rc != 0:
            raise FinitoError(rc, self._RESET)
        return self

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._FREE)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Hits(_Accumulator):
    """uint64 found-k-mer counts per unitig, resident in HBM beside one replica of the index (fin_hits_* of the C ABI): the profile of
    everything that was added, however many reads that was.  Unitig numbers are the index's own, the numbers the pairs carry."""
    _FREE, _RESET = "fin_hits_free", "fin_hits_reset"

    def __init__(self, index, device=0):
        self.index = index
        self.n_unitigs = index.n_unitigs
        self._create("fin_hits_create", index.h, int(device))

    def add(self, batch, stream=None):
        """counts += the hits of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_hits).  Adding the
        same run twice counts it twice."""
        return _acc_add(self, "fin_batch_add_hits", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and add its hits; nothing comes back (fin_search_batch_add_hits)"""
        return _acc_add_reads(self, "fin_search_batch_add_hits", reads, strands)

    def download(self):
        """(uint64 counts[n_unitigs], their sum = the k-mers found); waits for the adds (fin_hits_download)"""
        out = np.zeros(max(self.n_unitigs, 1), dtype=np.uint64)
        tot = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_hits_download(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tot), err, 512), err)
        return out[: self.n_unitigs], int(tot.value)

    def device_ptr(self):
        return int(self.L.fin_hits_device_counts(self.h) or 0)


def _class_thresholds(what, min_found, min_permille, min_margin):
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in (min_found, min_permille, min_margin)):
        raise FinitoError(FIN_EINVAL, what + ": min_found, min_permille and min_margin are unsigned 32-bit numbers")
    return int(min_found), int(min_permille), int(min_margin)


class Labels(_Accumulator):
    """a labelling of the index's unitigs (uint32 per unitig: a label below n_labels, or FIN_NO_LABEL) resident in HBM beside one replica, with the tally of the
    reads assigned to each label (fin_labels_* of the C ABI).  Unitig numbers are the index's own (FinimizerIndex.unitig_numbers maps an input order to them)."""
    _FREE, _RESET = "fin_labels_free", "fin_labels_reset"

    def __init__(self, index, unitig_labels, n_labels=None, device=0):
        self.index = index
        lab = np.asarray(unitig_labels)
        if lab.ndim != 1 or len(lab) != index.n_unitigs:
            raise FinitoError(FIN_EINVAL, "labels: one label per unitig of the index (%d), got %s" % (index.n_unitigs, lab.shape))
        if len(lab) and (lab.dtype.kind not in "iu" or int(lab.min()) < 0 or int(lab.max()) > FIN_NO_LABEL):
            raise FinitoError(FIN_EINVAL, "labels: unsigned 32-bit numbers, FIN_NO_LABEL for none")
        lab = np.ascontiguousarray(lab, dtype=np.uint32)
        if n_labels is None:
            named = lab[lab != FIN_NO_LABEL]
            n_labels = int(named.max()) + 1 if len(named) else 1
        if not 0 <= int(n_labels) <= 0xFFFFFFFF:
            raise FinitoError(FIN_EINVAL, "labels: n_labels is 1 .. 2^31")
        self.n_labels = int(n_labels)
        self._create("fin_labels_create", index.h, int(device), lab.ctypes.data_as(C.c_void_p), self.n_labels)

    def add(self, batch, min_found=1, min_permille=0, min_margin=0, stream=None):
        """tally += the reads of the batch's most recent run: a read goes to its class's label when n_best >= max(min_found, 1), 1000 * n_best >= min_permille * nk
        and n_best >= n_second + min_margin, else to `unassigned`; on a HIP stream, behind that run, no sync (fin_batch_add_classes).  Adding twice counts twice."""
        t = _class_thresholds("Labels.add", min_found, min_permille, min_margin)
        return _acc_add(self, "fin_batch_add_classes", batch, stream, *t)

    def add_reads(self, reads, min_found=1, min_permille=0, min_margin=0, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and tally its reads; nothing comes back (fin_search_batch_add_classes)"""
        t = _class_thresholds("Labels.add_reads", min_found, min_permille, min_margin)
        return _acc_add_reads(self, "fin_search_batch_add_classes", reads, strands, *t)

    def download(self):
        """(uint64 reads[n_labels + 1] -- the reads assigned to each label, then the unassigned ones --, their sum = the reads added); waits for the adds
        (fin_labels_download)"""
        out = np.zeros(self.n_labels + 1, dtype=np.uint64)
        tot = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_labels_download(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tot), err, 512), err)
        return out, int(tot.value)

    def device_ptrs(self):
        """(labels uint32[n_unitigs], reads uint64[n_labels + 1]) device pointers"""
        return int(self.L.fin_labels_device_labels(self.h) or 0), int(self.L.fin_labels_device_reads(self.h) or 0)


def _taxa_thresholds(what, min_found, confidence):
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in (min_found, confidence)):
        raise FinitoError(FIN_EINVAL, what + ": min_found and confidence are unsigned 32-bit numbers")
    return int(min_found), int(confidence)


def _taxa_parent(what, parent):
    p = np.asarray(parent)
    if p.ndim != 1 or len(p) == 0 or p.dtype.kind not in "iu" or int(p.min()) < 0 or int(p.max()) > 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, what + ": parent is one unsigned 32-bit number per taxon, taxon 0 the root")
    return np.ascontiguousarray(p, dtype=np.uint32)


class Taxonomy(_Accumulator):
    """a tree over taxa (parent[n_taxa] in topological numbering: parent[0] == 0, parent[t] < t; taxonomy_order makes it from arbitrary ids) with a taxon per
    unitig of the index, resident in HBM beside one replica, and the tally of the reads called at each taxon (fin_taxonomy_* of the C ABI).
    Made by FinimizerIndex.taxonomy from labels of the caller's, or by Colors.taxonomy from the colour matrix: a unitig's taxon is the LCA of its colours' taxa."""
    _FREE, _RESET = "fin_taxonomy_free", "fin_taxonomy_reset"

    def __init__(self, index, parent, unitig_labels=None, device=0, colors=None, color_taxon=None):
        self.index = index
        self.parent = _taxa_parent("taxonomy", parent)
        self.n_taxa = len(self.parent)
        self.color_taxon = None
        if colors is not None:
            ct = np.asarray(color_taxon)
            if ct.shape != (colors.n_colors,) or ct.dtype.kind not in "iu" or (len(ct) and (int(ct.min()) < 0 or int(ct.max()) > 0xFFFFFFFF)):
                raise FinitoError(FIN_EINVAL, "taxonomy: one taxon per colour (%d), got %s" % (colors.n_colors, ct.shape))
            ct = np.ascontiguousarray(ct, dtype=np.uint32)
            self.device = colors.device
            self._create("fin_taxonomy_create_from_colors", colors.h, self.parent.ctypes.data_as(C.c_void_p), self.n_taxa, ct.ctypes.data_as(C.c_void_p))
            self.color_taxon = ct   # (accepted: each is below n_taxa)
            return
        lab = np.asarray(unitig_labels)
        if lab.ndim != 1 or len(lab) != index.n_unitigs:
            raise FinitoError(FIN_EINVAL, "taxonomy: one label per unitig of the index (%d), got %s" % (index.n_unitigs, lab.shape))
        if len(lab) and (lab.dtype.kind not in "iu" or int(lab.min()) < 0 or int(lab.max()) > FIN_NO_LABEL):
            raise FinitoError(FIN_EINVAL, "taxonomy: labels are unsigned 32-bit numbers, FIN_NO_LABEL for none")
        lab = np.ascontiguousarray(lab, dtype=np.uint32)
        self.device = int(device)
        self._create("fin_taxonomy_create", index.h, self.device, self.parent.ctypes.data_as(C.c_void_p), self.n_taxa, lab.ctypes.data_as(C.c_void_p))

    def labels(self):
        """uint32 label[n_unitigs]: every unitig's taxon, FIN_NO_LABEL for none (fin_taxonomy_download_labels)"""
        out = np.zeros(max(self.index.n_unitigs, 1), dtype=np.uint32)
        err = C.create_string_buffer(512)
        _check(self.L.fin_taxonomy_download_labels(self.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[: self.index.n_unitigs]

    def as_labels(self):
        """the same labelling as a Labels with n_labels = n_taxa: the majority vote (Batch.classify) runs on it as it is.  A copy through the host: the labels
        are downloaded and uploaded again into the new Labels (4 bytes per unitig each way, once)"""
        return Labels(self.index, self.labels(), self.n_taxa, self.device)

    def add(self, batch, min_found=1, confidence=0, stream=None):
        """tally += the reads of the batch's most recent run, each at the taxon Batch.taxa gives it under these thresholds, unclassified ones apart; on a HIP
        stream, behind that run (fin_batch_add_taxa).  Adding twice counts twice."""
        return _acc_add(self, "fin_batch_add_taxa", batch, stream, *_taxa_thresholds("Taxonomy.add", min_found, confidence))

    def add_reads(self, reads, min_found=1, confidence=0, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and tally its reads; nothing comes back (fin_search_batch_add_taxa)"""
        return _acc_add_reads(self, "fin_search_batch_add_taxa", reads, strands, *_taxa_thresholds("Taxonomy.add_reads", min_found, confidence))

    def download(self):
        """(direct uint64[n_taxa] -- the reads called at each taxon --, clade uint64[n_taxa] -- the reads called at or below it, rolled up on the device --,
        unclassified); clade[0] + unclassified = the reads added.  Waits for the adds (fin_taxonomy_download)"""
        direct = np.zeros(self.n_taxa + 1, dtype=np.uint64)
        clade = np.zeros(self.n_taxa, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_taxonomy_download(self.h, direct.ctypes.data_as(C.POINTER(C.c_uint64)), clade.ctypes.data_as(C.POINTER(C.c_uint64)), None, err, 512), err)
        return direct[: self.n_taxa], clade, int(direct[self.n_taxa])

    def rollup(self, values_per_colour):
        """host only, float64: out[t] = the sum of values_per_colour[c] over the colours c whose taxon is t or below it -- Abundance.alpha summed into clades.
        A fixed order: the colours ascending into their taxa, then the taxa descending into their parents.  For a taxonomy made from colours"""
        v = np.asarray(values_per_colour, dtype=np.float64)
        ct = self.color_taxon
        if ct is None or v.shape != ct.shape:
            raise FinitoError(FIN_EINVAL, "Taxonomy.rollup: one value per colour of the colour matrix this taxonomy was made from")
        out = np.zeros(self.n_taxa, dtype=np.float64)
        for c in range(len(v)):
            out[int(ct[c])] += v[c]
        for t in range(self.n_taxa - 1, 0, -1):
            out[int(self.parent[t])] += out[t]
        return out

    def device_labels_ptr(self):
        return int(self.L.fin_taxonomy_device_labels(self.h) or 0)


def _permille(what, permille):
    if not 0 <= int(permille) <= 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, what + ": permille is an unsigned 32-bit number")
    return int(permille)


class Colors(_Accumulator):
    """the colour set of every unitig of the index -- which of n_colors references it occurs in -- as a bit matrix uint64[n_unitigs, W], W = ceil(n_colors / 64),
    resident in HBM beside one replica (fin_colors_* of the C ABI): colour c of unitig u is bit c & 63 of bits[u, c >> 6].  1 <= n_colors <= 4096.  Unitig numbers
    are the index's own."""
    _FREE, _RESET = "fin_colors_free", "fin_colors_reset"

    def __init__(self, index, n_colors, device=0):
        self.index = index
        self.n_unitigs = index.n_unitigs
        if not 0 <= int(n_colors) <= 0xFFFFFFFF:
            raise FinitoError(FIN_ELIMIT, "colors: n_colors is 1 .. 4096")
        self.n_colors = int(n_colors)
        self.words = (self.n_colors + 63) // 64
        self.device = int(device)
        self._create("fin_colors_create", index.h, self.device, self.n_colors)

    def upload(self, bits):
        """replace the matrix: uint64[n_unitigs, W]; a set bit at or above n_colors is refused (fin_colors_upload)"""
        a = np.asarray(bits)
        if a.shape != (self.n_unitigs, self.words) or a.dtype.kind not in "iu":
            raise FinitoError(FIN_EINVAL, "colors: a matrix of shape (%d, %d), got %s" % (self.n_unitigs, self.words, a.shape))
        a = np.ascontiguousarray(a, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_upload(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64)), err, 512), err)
        return self

    def add(self, batch, color, stream=None):
        """every unitig in which the batch's most recent run found a k-mer gets `color`, on a HIP stream, behind that run; no sync (fin_batch_add_colors).
        Adding twice changes nothing."""
        return _acc_add(self, "fin_batch_add_colors", batch, stream, self._color(color))

    def add_reads(self, reads, color, strands=FIN_MERGED):
        """search a sequence set (a reference genome's) from host buffers, sub-batches pipelined as in search_reads, and give `color` to every unitig it is
        found in; nothing comes back (fin_search_batch_add_colors)"""
        bases_offsets = flatten(reads)
        return _acc_add_reads(self, "fin_search_batch_add_colors", bases_offsets, strands, self._color(color))

    def _color(self, color):
        if not 0 <= int(color) < self.n_colors:
            raise FinitoError(FIN_EINVAL, "colors: colour %r is not in 0 .. %d" % (color, self.n_colors - 1))
        return int(color)

    def download(self):
        """(uint64 bits[n_unitigs, W], the number of set bits); waits for the adds (fin_colors_download)"""
        out = np.zeros((max(self.n_unitigs, 1), self.words), dtype=np.uint64)
        n = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_download(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), err, 512), err)
        return out[: self.n_unitigs], int(n.value)

    def device_ptr(self):
        """the dense matrix in HBM; 0 while compact"""
        return int(self.L.fin_colors_device_bits(self.h) or 0)

    # ---- the compact state: every distinct row once (fin_colors_compact) ----
    def compact(self, max_sets=0, stream=None):
        """deduplicate the rows on the device, behind every add so far, and free the dense matrix: set_of[n_unitigs] and sets[n_sets + 1, W] take its place.
        max_sets 0: min(n_unitigs, 2^26).  FIN_ELIMIT -- the object unchanged and still dense -- for more distinct non-empty rows than max_sets or a flagged
        matrix.  pseudoalign and all behind it work unchanged; add / add_reads / coverage / shared / taxonomy want expand() first.  A no-op when compact"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_compact(self.h, _u64("Colors.compact", "max_sets", max_sets), C.c_void_p(int(stream or 0)), err, 512), err)
        return self

    def expand(self, stream=None):
        """back to the dense matrix, gathered on the device (fin_colors_expand); a no-op when dense"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_expand(self.h, C.c_void_p(int(stream or 0)), err, 512), err)
        return self

    @property
    def is_compact(self):
        return bool(self.L.fin_colors_is_compact(self.h))

    @property
    def n_sets(self):
        """the number of sets beside the empty one; 0 while dense"""
        return int(self.L.fin_colors_n_sets(self.h))

    def device_set_of_ptr(self):
        return int(self.L.fin_colors_device_set_of(self.h) or 0)

    def device_sets_ptr(self):
        return int(self.L.fin_colors_device_sets(self.h) or 0)

    def download_sets(self):
        """(set_of uint32[n_unitigs], sets uint64[n_sets + 1, W]) of a compact object: sets[0] is empty, sets[set_of[u]] is unitig u's row; the order of the ids
        the device made is unspecified (fin_colors_download_sets)"""
        n = self.n_sets
        set_of = np.zeros(max(self.n_unitigs, 1), dtype=np.uint32)
        sets = np.zeros((n + 1, self.words), dtype=np.uint64)
        got = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_download_sets(self.h, set_of.ctypes.data_as(C.POINTER(C.c_uint32)), sets.ctypes.data_as(C.POINTER(C.c_uint64)), n + 1, C.byref(got),
                                               err, 512), err)
        return set_of[: self.n_unitigs], sets

    def upload_sets(self, set_of, sets):
        """make the object compact from host arrays (fin_colors_upload_sets): set_of[n_unitigs], sets[n_sets + 1, W] with sets[0] empty.  Duplicate rows and
        unused sets are legal"""
        so = np.asarray(set_of)
        a = np.asarray(sets)
        if so.shape != (self.n_unitigs,) or so.dtype.kind not in "iu" or (so.size and (int(so.min()) < 0 or int(so.max()) > 0xFFFFFFFF)):
            raise FinitoError(FIN_EINVAL, "colors: set_of is %d unsigned 32-bit set ids, got shape %s" % (self.n_unitigs, so.shape))
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != self.words or a.dtype.kind not in "iu":
            raise FinitoError(FIN_EINVAL, "colors: sets has shape (n_sets + 1, %d), got %s" % (self.words, a.shape))
        so = np.ascontiguousarray(so, dtype=np.uint32)
        if self.n_unitigs == 0:
            so = np.zeros(1, dtype=np.uint32)
        a = np.ascontiguousarray(a, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_upload_sets(self.h, so.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint64)), a.shape[0] - 1, err, 512), err)
        return self

    def compact_stats(self):
        """what the most recent compact() met: (n_sets, rows that met a foreign row under their tag, the longest probe, slots) -- fin_colors_compact_stats"""
        out = np.zeros(4, dtype=np.uint64)
        self.L.fin_colors_compact_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return tuple(int(v) for v in out)

    def eqclasses(self, max_classes=1 << 20):
        """an accumulator of equivalence classes beside this matrix (EqClasses)"""
        return EqClasses(self, max_classes)

    def taxonomy(self, parent, color_taxon):
        """a Taxonomy beside this matrix whose unitig labels are the LCA of their colours' taxa, made on the device (fin_taxonomy_create_from_colors): parent in
        topological numbering, color_taxon one taxon per colour.  Waits for the adds to the matrix; later adds do not change the labels"""
        return Taxonomy(self.index, parent, colors=self, color_taxon=color_taxon)

    def assigner(self, weights, thresholds=0.5):
        """an accumulator that assigns reads to references beside this matrix (Assign): weights one per colour, usually Abundance.weights(); thresholds one per
        colour or a scalar for all -- thresholds=ab.theta is the mGEMS rule"""
        return Assign(self, weights, thresholds)

    def coverage(self, cover=None, depth=None, min_depth=1):
        """the per-unitig coverage numbers projected through this matrix, on the device (fin_colors_coverage): a ColorCoverage.  cover: a Cover,
        depth: a Depth of the same index and device, either may be None (its sums are 0; both None: kmers / kmers_only alone, the references' sizes in the graph);
        n_at_least of the depth is counted against min_depth.  Waits for the adds to all three; changes none of them"""
        if not 0 <= int(min_depth) <= 0xFFFFFFFF:
            raise FinitoError(FIN_EINVAL, "Colors.coverage: min_depth is an unsigned 32-bit number")
        out = np.zeros(self.n_colors + 1, dtype=COLOR_COVERAGE_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_coverage(self.h, cover.h if cover is not None else None, depth.h if depth is not None else None, int(min_depth),
                                          out.ctypes.data_as(C.c_void_p), out[self.n_colors:].ctypes.data_as(C.c_void_p), err, 512), err)
        return ColorCoverage(out[: self.n_colors], out[self.n_colors])

    def shared(self, cover=None, weights=None):
        """the k-mers every pair of references shares: this matrix times itself under a weight per unitig, on the device (fin_colors_shared) -- a
        ColorShared.  Neither given: the unitigs' k-mers, the references' overlap in the graph; cover: a Cover of the same index and device, the k-mers that bitmap
        found; weights: uint64[n_unitigs] of the caller's (sums are mod 2^64).  Not both.  Waits for the adds to the matrix and the bitmap; changes neither"""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.uint64)
            if w.shape != (self.n_unitigs,):
                raise FinitoError(FIN_EINVAL, "Colors.shared: weights has shape %s, the index has %d unitigs" % (w.shape, self.n_unitigs))
            if self.n_unitigs == 0:
                w = np.zeros(1, dtype=np.uint64)
        out = np.zeros((self.n_colors, self.n_colors), dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_shared(self.h, cover.h if cover is not None else None, w.ctypes.data_as(C.c_void_p) if w is not None else None,
                                        out.ctypes.data_as(C.c_void_p), err, 512), err)
        return ColorShared(out)

    def depth_histogram(self, depth, n_bins=256, bin_width=1):
        """the histogram of every reference's k-mer depths, on the device (fin_colors_depth_histogram): a ColorDepthHistogram -- what medians and
        quartiles are read from.  depth: a Depth of the same index and device; bin(d) = min(d // bin_width, n_bins - 1), n_bins 1 .. 1024.  Waits for the adds to
        both; changes neither"""
        nb, bw = _hist_args("Colors.depth_histogram", n_bins, bin_width)
        if depth is None:
            raise FinitoError(FIN_EINVAL, "Colors.depth_histogram: a Depth is needed")
        out = np.zeros((self.n_colors * 2 + 1, nb), dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_colors_depth_histogram(self.h, depth.h, nb, bw, out.ctypes.data_as(C.c_void_p), out[self.n_colors * 2:].ctypes.data_as(C.c_void_p), err, 512), err)
        return ColorDepthHistogram(out[: self.n_colors * 2].reshape(self.n_colors, 2, nb), out[self.n_colors * 2], bw)


class EqClasses(_Accumulator):
    """the equivalence classes of pseudoaligned reads -- the distinct colour rows the added runs produced and how many reads have each --, accumulated in HBM
    beside a colour matrix (fin_eqclasses_* of the C ABI).  An all-zero row is an unaligned read and belongs to no class.  At most max_classes (1 .. 2^26)
    distinct rows; free it before the colours."""
    _FREE, _RESET = "fin_eqclasses_free", "fin_eqclasses_reset"

    def __init__(self, colors, max_classes=1 << 20):
        self.colors = colors
        self.index = colors.index
        self.n_colors = colors.n_colors
        self.words = colors.words
        if not 0 <= int(max_classes) <= 0xFFFFFFFFFFFFFFFF:
            raise FinitoError(FIN_ELIMIT, "eqclasses: max_classes is 1 .. 2^26")
        self.max_classes = int(max_classes)
        self._create("fin_eqclasses_create", colors.h, self.max_classes)

    def add(self, batch, permille=1000, stream=None):
        """the batch's most recent run, pseudoaligned against the colours at `permille` and added, on a HIP stream; no sync (fin_batch_add_eqclasses).  Adding
        twice counts twice."""
        return _acc_add(self, "fin_batch_add_eqclasses", batch, stream, _permille("EqClasses.add", permille))

    def add_pairs(self, batch, permille=1000, both=False, stream=None):
        """the batch's most recent run as interleaved mates: one row per FRAGMENT, made by Batch.pseudoalign_pairs' kernel and added, on a HIP stream; no sync
        (fin_batch_add_eqclasses_paired).  A fragment is one "read" of its class"""
        return _acc_add(self, "fin_batch_add_eqclasses_paired", batch, stream, _permille("EqClasses.add_pairs", permille), FIN_PAIR_BOTH if both else FIN_PAIR_ANY)

    def add_rows(self, ptr, n_rows, stream=None):
        """rows any producer left in HBM: a device pointer to uint64[n_rows, W], valid until the add has finished (fin_eqclasses_add_rows)"""
        if not 0 <= int(n_rows) <= 0xFFFFFFFFFFFFFFFF:
            raise FinitoError(FIN_EINVAL, "EqClasses.add_rows: n_rows is an unsigned 64-bit number")
        err = C.create_string_buffer(512)
        _check(self.L.fin_eqclasses_add_rows(self.h, C.c_void_p(int(ptr) or 0), int(n_rows), C.c_void_p(stream or 0), err, 512), err)
        return self

    def add_classes(self, class_rows, class_reads, n_unaligned=0):
        """classes {row, reads} from host arrays -- a download, another rank's classes --, added as if row r had been added class_reads[r] times, and n_unaligned
        empty rows besides; exact, in integers.  A row with a bit at or above n_colors is refused before anything is added; returns when the add has run
        (fin_eqclasses_add_classes_host)"""
        a, r = _classes("EqClasses.add_classes", class_rows, class_reads, self.n_colors)
        un = _u64("EqClasses.add_classes", "n_unaligned", n_unaligned)
        u64p = C.POINTER(C.c_uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_eqclasses_add_classes_host(self.h, a.ctypes.data_as(u64p), r.ctypes.data_as(u64p), len(a), un, err, 512), err)
        return self

    def add_classes_device(self, rows_ptr, reads_ptr, n_classes, n_unaligned=0, stream=None):
        """the same from device pointers: uint64[n_classes, W] and uint64[n_classes] in HBM, valid until the add has finished; on a HIP stream, no sync
        (fin_eqclasses_add_classes)"""
        n = _u64("EqClasses.add_classes_device", "n_classes", n_classes)
        un = _u64("EqClasses.add_classes_device", "n_unaligned", n_unaligned)
        err = C.create_string_buffer(512)
        _check(self.L.fin_eqclasses_add_classes(self.h, C.c_void_p(int(rows_ptr) or 0), C.c_void_p(int(reads_ptr) or 0), n, un, C.c_void_p(stream or 0), err, 512), err)
        return self

    def merge(self, other, stream=None):
        """this accumulator gains what `other` holds (its classes and its unaligned count), on the device; `other` is left as it was found.  Waits for `other`'s
        adds, not for its own; `other` must be another accumulator on the same device with the same n_colors, and not flagged (fin_eqclasses_merge).
        Accumulators on different devices: add_classes(*other.download())"""
        if not isinstance(other, EqClasses) or not getattr(other, "h", None):
            raise FinitoError(FIN_EINVAL, "EqClasses.merge: another EqClasses")
        err = C.create_string_buffer(512)
        _check(self.L.fin_eqclasses_merge(self.h, other.h, C.c_void_p(stream or 0), err, 512), err)
        return self

    def add_reads(self, reads, permille=1000, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and add every read's row; nothing comes back
        (fin_search_batch_add_eqclasses)"""
        bases_offsets = flatten(reads)
        return _acc_add_reads(self, "fin_search_batch_add_eqclasses", bases_offsets, strands, _permille("EqClasses.add_reads", permille))

    def add_read_pairs(self, reads, permille=1000, both=False, strands=FIN_MERGED):
        """add_reads for interleaved mates: every fragment's row is added; no sub-batch splits a pair (fin_search_batch_add_eqclasses_paired)"""
        bases_offsets = flatten(reads)
        return _acc_add_reads(self, "fin_search_batch_add_eqclasses_paired", bases_offsets, strands, _permille("EqClasses.add_read_pairs", permille),
                              FIN_PAIR_BOTH if both else FIN_PAIR_ANY)

    def download(self):
        """(rows uint64[n, W], reads uint64[n], n_unaligned) in canonical order -- np.unique(rows, axis=0)'s; waits for the adds (fin_eqclasses_download)"""
        u64p = C.POINTER(C.c_uint64)
        n, un = C.c_uint64(0), C.c_uint64(0)
        err = C.create_string_buffer(512)
        cap = 0
        rows = np.zeros((1, self.words), dtype=np.uint64)
        reads = np.zeros(1, dtype=np.uint64)
        while True:   # the first call learns the number of classes
            rc = self.L.fin_eqclasses_download(self.h, rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), cap, C.byref(n), C.byref(un), err, 512)
            if rc == FIN_ELIMIT and int(n.value) > cap:
                cap = int(n.value)
                rows = np.zeros((cap, self.words), dtype=np.uint64)
                reads = np.zeros(cap, dtype=np.uint64)
                n.value = 0
                continue
            _check(rc, err)
            return rows[: int(n.value)], reads[: int(n.value)], int(un.value)

    def tally(self):
        """(reads_with uint64[n_colors], reads_only uint64[n_colors], n_unaligned): per colour, the reads whose class contains it and the reads whose class
        is that colour alone -- derived from the classes (fin_eqclasses_color_tally)"""
        rows, reads, un = self.download()
        w, o = eqclasses_color_tally(rows, reads, self.n_colors)
        return w, o, un

    def abundance(self, lengths=None, max_iters=1000, tol=1e-6, trace=False):
        """expected reads per colour by EM over the classes, on the device: an Abundance; waits for the adds and leaves the accumulator as it found it
        (fin_eqclasses_abundance).  lengths: one finite positive number per colour (None: all 1); trace: keep the log-likelihood of every iteration -- an
        array given here is written in place, entries behind `iters` left alone.  References with the same column of the colour matrix
        (Colors.shared().identical_groups()) are not identifiable: the EM splits their reads by its starting point, only the group's sum means something"""
        lens, mi, tol = _abundance_args("EqClasses.abundance", self.n_colors, lengths, max_iters, tol)
        alpha = np.zeros(self.n_colors, dtype=np.float64)
        tr = _abundance_trace("EqClasses.abundance", trace, mi)
        info = AbundanceInfo()
        err = C.create_string_buffer(512)
        f64p = C.POINTER(C.c_double)
        _check(self.L.fin_eqclasses_abundance(self.h, lens.ctypes.data_as(f64p) if lens is not None else None, mi, tol, alpha.ctypes.data_as(f64p),
                                              tr.ctypes.data_as(f64p) if tr is not None else None, C.byref(info), err, 512), err)
        return Abundance(alpha, lens, info, tr)

    def bootstrap(self, n_boot, seed=0, lengths=None, max_iters=1000, tol=1e-6):
        """the estimate of abundance() and n_boot (1 .. 4096) bootstrap replicates of it, the class counts of each resampled on the device: a Bootstrap
        (fin_eqclasses_bootstrap).  A Poisson bootstrap keyed by the class's row: the replicates are a function of the classes, seed and the
        replicate's number alone.  Waits for the adds and leaves the accumulator as it found it"""
        lens, mi, tol = _abundance_args("EqClasses.bootstrap", self.n_colors, lengths, max_iters, tol)
        nb, seed = _bootstrap_args("EqClasses.bootstrap", n_boot, seed)
        out = _BootOut(nb, self.n_colors)
        err = C.create_string_buffer(512)
        f64p = C.POINTER(C.c_double)
        _check(self.L.fin_eqclasses_bootstrap(self.h, lens.ctypes.data_as(f64p) if lens is not None else None, mi, tol, nb, seed, *out.args(), err, 512), err)
        return out.result(lens, seed)

    def stats(self):
        """[rows added, unaligned, classes, rows that went through the serial pass]; waits (fin_eqclasses_stats)"""
        out = np.zeros(4, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_eqclasses_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), err, 512), err)
        return [int(v) for v in out]


class ColorCoverage:
    """breadth and depth of coverage per reference (Colors.coverage, unitig_color_coverage): the eight uint64[n_colors] arrays kmers, kmers_only, covered,
    covered_only, depth_sum, depth_sum_only, solid, solid_only -- the unitigs' k-mers, distinct found k-mers, summed depth and positions at or above min_depth,
    summed over the unitigs that carry colour c and (_only) over those that carry c alone -- and `uncolored`, a dict of the four sums over the unitigs without a
    colour.  table: the COLOR_COVERAGE_DTYPE array they are views of.  The ratios are derived here, in float64; the library stays in integers"""
    FIELDS = ("kmers", "kmers_only", "covered", "covered_only", "depth_sum", "depth_sum_only", "solid", "solid_only")

    def __init__(self, table, uncolored):
        self.table = table
        for f in self.FIELDS:
            setattr(self, f, table[f])
        self.uncolored = {f: int(uncolored[f]) for f in ("kmers", "covered", "depth_sum", "solid")}

    @staticmethod
    def _ratio(num, den):
        out = np.full(len(num), np.nan)
        np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
        return out

    @property
    def breadth(self):
        """covered / kmers: the share of the reference's k-mers that were found; nan for a reference without k-mers in the graph"""
        return self._ratio(self.covered, self.kmers)

    @property
    def breadth_only(self):
        """covered_only / kmers_only: the same over the k-mers of unitigs that carry this colour alone; nan where there are none"""
        return self._ratio(self.covered_only, self.kmers_only)

    @property
    def mean_depth(self):
        """depth_sum / covered: the mean depth of the found k-mers; nan where none was found"""
        return self._ratio(self.depth_sum, self.covered)


FIN_DEPTH_HIST_MAX_BINS = 1024


def _hist_args(what, n_bins, bin_width):
    nb, bw = int(n_bins), int(bin_width)
    if not 1 <= nb <= FIN_DEPTH_HIST_MAX_BINS:
        raise FinitoError(FIN_EINVAL, "%s: n_bins is 1 .. %d" % (what, FIN_DEPTH_HIST_MAX_BINS))
    if not 1 <= bw <= 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: bin_width is 1 .. 2^32 - 1" % what)
    return nb, bw


def histogram_quantile(hist, permille, bin_width=1):
    """the quantile rule of include/finito_amd.h (DEPTH HISTOGRAMS AND QUANTILES) for one histogram, in Python integers: with N = sum(hist) and
    t = max(1, ceil(permille * N / 1000)), the smallest bin b whose cumulative count reaches t -- (b * bin_width, saturated), saturated when b is the last of
    more than one bin ("this much or more"); None when the histogram is empty"""
    p, bw = int(permille), int(bin_width)
    if not 0 <= p <= 1000:
        raise FinitoError(FIN_EINVAL, "histogram_quantile: permille is 0 .. 1000")
    if bw < 1:
        raise FinitoError(FIN_EINVAL, "histogram_quantile: bin_width is at least 1")
    h = [int(x) for x in hist]
    n = sum(h)
    if n == 0:
        return None
    t = max(1, (p * n + 999) // 1000)
    acc = 0
    for b, x in enumerate(h):
        acc += x
        if acc >= t:
            return b * bw, (b == len(h) - 1 and len(h) > 1)
    raise AssertionError("unreachable: t <= N")


class ColorDepthHistogram:
    """the histogram of every reference's k-mer depths (Colors.depth_histogram, unitig_color_depth_histogram): table uint64[n_colors, 2, n_bins] -- [c, 0] over the
    unitigs that carry colour c, [c, 1] over those that carry c alone --, uncolored uint64[n_bins] over the unitigs without a colour, n_bins, bin_width; kmers and
    kmers_only are the row sums.  Bin b holds the k-mer positions whose depth d has min(d // bin_width, n_bins - 1) == b.  Quantiles follow histogram_quantile"""

    def __init__(self, table, uncolored, bin_width):
        self.table, self.uncolored = table, uncolored
        self.n_colors, _, self.n_bins = table.shape
        self.bin_width = int(bin_width)
        self.kmers = table[:, 0, :].sum(axis=1, dtype=np.uint64)
        self.kmers_only = table[:, 1, :].sum(axis=1, dtype=np.uint64)

    def quantile(self, permille, only=False):
        """(values int64[n_colors], saturated bool[n_colors]): every colour's quantile in thousandths as a depth (the bin's lower edge); -1 where the colour has
        no k-mers"""
        values, sat = np.full(self.n_colors, -1, dtype=np.int64), np.zeros(self.n_colors, dtype=bool)
        for c in range(self.n_colors):
            q = histogram_quantile(self.table[c, 1 if only else 0], permille, self.bin_width)
            if q is not None:
                values[c], sat[c] = q
        return values, sat

    def median(self, only=False):
        return self.quantile(500, only)

    def iqr(self, only=False):
        """(q750 - q250 int64[n_colors], saturated where either quartile is): -1 where the colour has no k-mers"""
        (lo, s_lo), (hi, s_hi) = self.quantile(250, only), self.quantile(750, only)
        return np.where(lo < 0, -1, hi - lo), s_lo | s_hi

    def breadth(self, only=False):
        """1 - table[:, ., 0] / kmers: the share of the k-mers found at least bin_width times; nan for a colour without k-mers"""
        j = 1 if only else 0
        den = self.kmers_only if only else self.kmers
        out = np.full(self.n_colors, np.nan)
        np.divide(self.table[:, j, 0].astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
        return np.where(den != 0, 1.0 - out, np.nan)


class ColorShared:
    """what every pair of references shares (Colors.shared, unitig_color_shared): table uint64[n_colors, n_colors], table[i, j] = the sum of the unitigs' weights
    over the unitigs that carry colour i and colour j -- symmetric; sizes is its diagonal.  With the default weights on a graph coloured by search, table[i, j] is
    the number of distinct k-mers references i and j have in common.  The ratios are derived here, in float64; the groups and pairs from the integers, exactly"""

    def __init__(self, table):
        self.table = table
        self.sizes = np.ascontiguousarray(np.diagonal(table))

    @property
    def jaccard(self):
        """s_ij / (s_ii + s_jj - s_ij), float64[n_colors, n_colors]; nan where both references are empty"""
        s, d = self.table.astype(np.float64), self.sizes.astype(np.float64)
        den = d[:, None] + d[None, :] - s
        out = np.full(s.shape, np.nan)
        np.divide(s, den, out=out, where=den != 0)
        return out

    @property
    def containment(self):
        """[i, j] = s_ij / s_ii, the share of reference i that reference j has, float64[n_colors, n_colors]; row i is nan for an empty reference i"""
        s, d = self.table.astype(np.float64), self.sizes.astype(np.float64)
        out = np.full(s.shape, np.nan)
        np.divide(s, d[:, None], out=out, where=(d != 0)[:, None])
        return out

    def identical_groups(self):
        """the lists of two or more colours with s_ij == s_ii == s_jj > 0 -- the same column of the matrix, as far as the weights can see: no estimate downstream
        can tell their members apart --, each ascending, each group once, by its first member"""
        d, groups, seen = self.sizes, [], np.zeros(len(self.sizes), dtype=bool)
        for i in range(len(d)):
            if seen[i] or d[i] == 0:
                continue
            members = np.nonzero((self.table[i] == d[i]) & (d == d[i]))[0]
            seen[members] = True
            if len(members) >= 2:
                groups.append([int(c) for c in members])
        return groups

    def contained(self):
        """the pairs (i, j), i != j, with s_ij == s_ii > 0 and s_jj > s_ii: reference i lies in reference j and j has more; ascending"""
        d = self.sizes
        i, j = np.nonzero((self.table == d[:, None]) & (d[:, None] > 0) & (d[None, :] > d[:, None]))
        return [(int(a), int(b)) for a, b in zip(i, j)]


def _assign_args(what, n_colors, weights, thresholds):
    """the checks of fin_assign_create, fin_assign_set and fin_rows_assign, made here so that the message can say what was wrong; a scalar threshold is broadcast"""
    nc = int(n_colors)
    if not 1 <= nc <= 4096:
        raise FinitoError(FIN_ELIMIT, "%s: n_colors is 1 .. 4096" % what)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != nc:
        raise FinitoError(FIN_EINVAL, "%s: %d weights for %d colours" % (what, len(w), nc))
    t = np.asarray(thresholds, dtype=np.float64)
    t = np.full(nc, float(t), dtype=np.float64) if t.ndim == 0 else np.ascontiguousarray(t).reshape(-1)
    if len(t) != nc:
        raise FinitoError(FIN_EINVAL, "%s: %d thresholds for %d colours" % (what, len(t), nc))
    bad = np.nonzero(~(np.isfinite(w) & (w >= 0)))[0]
    if len(bad):
        raise FinitoError(FIN_EINVAL, "%s: the weight of colour %d is not a finite number >= 0" % (what, int(bad[0])))
    bad = np.nonzero(~((t >= 0) & (t <= 1)))[0]
    if len(bad):
        raise FinitoError(FIN_EINVAL, "%s: the threshold of colour %d is not a number in 0 .. 1" % (what, int(bad[0])))
    return w, t


def _assign_unit(pairs, both):
    return (2 if both else 1) if pairs else 0


class Assign(_Accumulator):
    """reads assigned to references from per-colour weights, on the device beside a colour matrix (fin_assign_* of the C ABI): colour c of a row
    is assigned iff x[c] > 0, d > 0 and x[c] >= thr[c] * d, d being the sum of the row's weights in the EM's order.  Accumulates assigned[c], sole[c] and the
    counters {rows, unaligned, unassigned, multi}; free it before the colours."""
    _FREE, _RESET = "fin_assign_free", "fin_assign_reset"

    def __init__(self, colors, weights, thresholds=0.5):
        self.colors = colors
        self.index = colors.index
        self.n_colors = colors.n_colors
        self.words = colors.words
        w, t = _assign_args("Assign", self.n_colors, weights, thresholds)
        f64p = C.POINTER(C.c_double)
        self._create("fin_assign_create", colors.h, w.ctypes.data_as(f64p), t.ctypes.data_as(f64p))

    def set(self, weights, thresholds=0.5, stream=None):
        """new weights and thresholds, behind the adds issued so far; the counts stay (fin_assign_set)"""
        w, t = _assign_args("Assign.set", self.n_colors, weights, thresholds)
        f64p = C.POINTER(C.c_double)
        err = C.create_string_buffer(512)
        _check(self.L.fin_assign_set(self.h, w.ctypes.data_as(f64p), t.ctypes.data_as(f64p), C.c_void_p(stream or 0), err, 512), err)
        return self

    def add(self, batch, permille=1000, pairs=False, both=False, stream=None):
        """the batch's most recent run, pseudoaligned at `permille` per read (pairs: per fragment; both: FIN_PAIR_BOTH), assigned and counted on a HIP stream;
        no sync (fin_batch_assign).  Batch.assign() also brings the rows and heads back"""
        return _acc_add(self, "fin_batch_assign", batch, stream, _permille("Assign.add", permille), _assign_unit(pairs, both))

    def add_rows(self, ptr, n_rows, out_rows_ptr=0, heads_ptr=0, stream=None):
        """rows any producer left in HBM: a device pointer to uint64[n_rows, W]; the assigned rows and READ_ASSIGN_DTYPE heads go to the device pointers given
        (0: not wanted).  All valid until the add has finished; no sync (fin_assign_rows)"""
        if not 0 <= int(n_rows) <= 0xFFFFFFFFFFFFFFFF:
            raise FinitoError(FIN_EINVAL, "Assign.add_rows: n_rows is an unsigned 64-bit number")
        err = C.create_string_buffer(512)
        _check(self.L.fin_assign_rows(self.h, C.c_void_p(int(ptr) or 0), int(n_rows), C.c_void_p(int(out_rows_ptr) or 0), C.c_void_p(int(heads_ptr) or 0),
                                      C.c_void_p(stream or 0), err, 512), err)
        return self

    def add_reads(self, reads, permille=1000, pairs=False, both=False, strands=FIN_MERGED, want_rows=True):
        """(assigned rows uint64[F, W] or None, heads READ_ASSIGN_DTYPE[F]): a read set from host buffers, sub-batches pipelined and cut between pairs only,
        pseudoaligned, assigned and counted (fin_search_batch_assign)"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        nf = n // 2 if pairs else n
        rows = np.zeros((max(nf, 1), self.words), dtype=np.uint64) if want_rows else None
        heads = np.zeros(max(nf, 1), dtype=READ_ASSIGN_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_assign(self.index.h, *_reads_args((bases, offsets)), int(strands), self.h, _permille("Assign.add_reads", permille),
                                              _assign_unit(pairs, both), rows.ctypes.data_as(C.POINTER(C.c_uint64)) if want_rows else None,
                                              heads.ctypes.data_as(C.c_void_p), err, 512), err)
        return (rows[:nf] if want_rows else None), heads[:nf]

    def download(self):
        """(assigned uint64[n_colors], sole uint64[n_colors], counters uint64[4] = rows, unaligned, unassigned, multi); waits for the adds (fin_assign_download)"""
        u64p = C.POINTER(C.c_uint64)
        assigned, sole = np.zeros(self.n_colors, dtype=np.uint64), np.zeros(self.n_colors, dtype=np.uint64)
        counters = np.zeros(4, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_assign_download(self.h, assigned.ctypes.data_as(u64p), sole.ctypes.data_as(u64p), counters.ctypes.data_as(u64p), err, 512), err)
        return assigned, sole, counters


class Abundance:
    """the result of an abundance estimate: alpha = expected reads per colour, theta = alpha / N, rho = (alpha / len) / sum(alpha / len) -- the
    share of the sample's copies; iters, converged, loglik (of the last iteration), max_change (max |delta alpha| / max(alpha, 1) of the last iteration),
    n_reads (N, the aligned reads), n_unaligned, n_classes; trace = the log-likelihood of iterations 0 .. iters - 1 when asked for, else None"""

    def __init__(self, alpha, lengths, info, trace):
        self.alpha = alpha
        self.n_reads, self.n_unaligned, self.n_classes = int(info.n_reads), int(info.n_unaligned), int(info.n_classes)
        self.iters, self.converged = int(info.iters), bool(info.converged)
        self.loglik, self.max_change = float(info.loglik), float(info.max_change)
        self.theta = alpha / self.n_reads if self.n_reads else np.zeros_like(alpha)
        per_len = alpha / lengths if lengths is not None else alpha
        self.rho = per_len / per_len.sum() if per_len.sum() > 0 else np.zeros_like(alpha)
        self.trace = trace[: self.iters] if trace is not None else None
        self.lengths = lengths

    def weights(self):
        """alpha / lengths: the per-colour weights of Colors.assigner"""
        return self.alpha / self.lengths if self.lengths is not None else self.alpha.copy()


class Bootstrap:
    """the result of a bootstrap: point = the Abundance of the classes as they are; per replicate b alpha[b] (expected reads per colour),
    n_reads[b] (N_b, the replicate's reads), iters[b], converged[b]; theta = alpha / n_reads (0 where N_b = 0); mean and sd of alpha over the replicates
    (ddof = 1; sd is 0 for one replicate), made on the host; seed"""

    def __init__(self, point, alpha, n_reads, iters, converged, seed):
        self.point, self.alpha, self.n_reads, self.iters, self.converged, self.seed = point, alpha, n_reads, iters, converged, seed
        nz = n_reads > 0
        self.theta = np.zeros_like(alpha)
        self.theta[nz] = alpha[nz] / n_reads[nz].astype(np.float64)[:, None]
        self.mean = alpha.mean(axis=0)
        self.sd = alpha.std(axis=0, ddof=1) if len(alpha) > 1 else np.zeros(alpha.shape[1])


class _BootOut:
    """the output arrays of fin_eqclasses_bootstrap and fin_classes_bootstrap"""

    def __init__(self, n_boot, n_colors):
        self.point, self.info = np.zeros(n_colors, dtype=np.float64), AbundanceInfo()
        self.alpha = np.zeros((n_boot, n_colors), dtype=np.float64)
        self.n_reads, self.iters, self.conv = np.zeros(n_boot, dtype=np.uint64), np.zeros(n_boot, dtype=np.uint32), np.zeros(n_boot, dtype=np.uint8)

    def args(self):
        f64p = C.POINTER(C.c_double)
        return (self.point.ctypes.data_as(f64p), C.byref(self.info), self.alpha.ctypes.data_as(f64p), self.n_reads.ctypes.data_as(C.POINTER(C.c_uint64)),
                self.iters.ctypes.data_as(C.POINTER(C.c_uint32)), self.conv.ctypes.data_as(C.POINTER(C.c_uint8)))

    def result(self, lens, seed):
        return Bootstrap(Abundance(self.point, lens, self.info, None), self.alpha, self.n_reads, self.iters, self.conv.astype(bool), seed)


def _bootstrap_args(what, n_boot, seed):
    nb, seed = int(n_boot), int(seed)
    if nb < 1:
        raise FinitoError(FIN_EINVAL, "%s: n_boot is 1 .. 4096" % what)
    if nb > 4096:
        raise FinitoError(FIN_ELIMIT, "%s: n_boot is 1 .. 4096" % what)
    if not 0 <= seed <= 0xFFFFFFFFFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: seed is an unsigned 64-bit number" % what)
    return nb, seed


def _abundance_args(what, n_colors, lengths, max_iters, tol):
    """the checks of fin_eqclasses_abundance and fin_classes_abundance, made here so that the message can say what was wrong"""
    if not 1 <= int(n_colors) <= 4096:
        raise FinitoError(FIN_ELIMIT, "%s: n_colors is 1 .. 4096" % what)
    mi = int(max_iters)
    if mi < 1:
        raise FinitoError(FIN_EINVAL, "%s: max_iters is 1 .. 100000" % what)
    if mi > 100000:
        raise FinitoError(FIN_ELIMIT, "%s: max_iters is 1 .. 100000" % what)
    tol = float(tol)
    if not tol >= 0.0:
        raise FinitoError(FIN_EINVAL, "%s: tol is a number >= 0" % what)
    lens = None
    if lengths is not None:
        lens = np.ascontiguousarray(lengths, dtype=np.float64).reshape(-1)
        if len(lens) != int(n_colors):
            raise FinitoError(FIN_EINVAL, "%s: %d lengths for %d colours" % (what, len(lens), int(n_colors)))
        bad = np.nonzero(~(np.isfinite(lens) & (lens > 0)))[0]
        if len(bad):
            raise FinitoError(FIN_EINVAL, "%s: the length of colour %d is not a finite positive number" % (what, int(bad[0])))
    return lens, mi, tol


def _abundance_trace(what, trace, max_iters):
    if trace is None or trace is False:
        return None
    if trace is True:
        return np.zeros(max_iters, dtype=np.float64)
    if not (isinstance(trace, np.ndarray) and trace.dtype == np.float64 and trace.ndim == 1 and trace.flags.c_contiguous and len(trace) >= max_iters):
        raise FinitoError(FIN_EINVAL, "%s: trace is a bool or a contiguous float64 array of at least max_iters entries" % what)
    return trace


class Cover(_Accumulator):
    """one bit per base of the concatenated unitig text, resident in HBM beside one replica of the index (fin_cover_* of the C ABI): bit start(u) + off is set
    iff a found pair (u, off) was added -- which k-mers of each unitig were seen, where Hits says how often the unitig was hit."""
    _FREE, _RESET = "fin_cover_free", "fin_cover_reset"

    def __init__(self, index, device=0):
        self.index = index
        self.n_unitigs = index.n_unitigs
        self.n_words = (index.total_len + 63) // 64
        self._create("fin_cover_create", index.h, int(device))

    def add(self, batch, stream=None):
        """bits |= the found places of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_cover).  Adding the same run
        twice changes nothing."""
        return _acc_add(self, "fin_batch_add_cover", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and set its places; nothing comes back (fin_search_batch_add_cover)"""
        return _acc_add_reads(self, "fin_search_batch_add_cover", reads, strands)

    def download(self):
        """(uint64 bits[(total_len + 63) // 64], uint64 covered[n_unitigs], their sum = the distinct k-mers found); waits for the adds (fin_cover_download)"""
        bits = np.zeros(max(self.n_words, 1), dtype=np.uint64)
        cov = np.zeros(max(self.n_unitigs, 1), dtype=np.uint64)
        tot = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_cover_download(self.h, bits.ctypes.data_as(C.POINTER(C.c_uint64)), cov.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tot), err, 512), err)
        return bits[: self.n_words], cov[: self.n_unitigs], int(tot.value)

    def device_ptr(self):
        return int(self.L.fin_cover_device_bits(self.h) or 0)


class Depth(_Accumulator):
    """how many times each position of the concatenated unitig text was found, resident in HBM beside one replica of the index as a difference array
    (fin_depth_* of the C ABI): between Hits (the depth summed over a unitig) and Cover (where it is above zero)."""
    _FREE, _RESET = "fin_depth_free", "fin_depth_reset"

    def __init__(self, index, device=0):
        self.index = index
        self.n_unitigs = index.n_unitigs
        self.total_len = index.total_len
        self._create("fin_depth_create", index.h, int(device))

    def add(self, batch, stream=None):
        """depth += the found places of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_depth).  Adding the same run
        twice counts it twice."""
        return _acc_add(self, "fin_batch_add_depth", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and add its places; nothing comes back (fin_search_batch_add_depth)"""
        return _acc_add_reads(self, "fin_search_batch_add_depth", reads, strands)

    def download(self, min_depth=1, want_positions=True):
        """(uint32 depth[total_len] -- None without want_positions --, DEPTH_STAT_DTYPE stats[n_unitigs] with n_at_least counted against min_depth, the sum over
        all positions = the k-mers found); waits for the adds, runs the prefix sum on the device and leaves the accumulator as it is (fin_depth_download)"""
        depth = np.zeros(max(self.total_len, 1), dtype=np.uint32) if want_positions else None
        stats = np.zeros(max(self.n_unitigs, 1), dtype=DEPTH_STAT_DTYPE)
        tot = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_depth_download(self.h, int(min_depth), depth.ctypes.data_as(C.c_void_p) if want_positions else None, stats.ctypes.data_as(C.c_void_p),
                                         C.byref(tot), err, 512), err)
        return (depth[: self.total_len] if want_positions else None), stats[: self.n_unitigs], int(tot.value)

    def histogram(self, n_bins=256, bin_width=1):
        """the k-mer spectrum of the run, made on the device (fin_depth_histogram): uint64[n_bins], entry b the k-mer positions of the text whose
        depth d has min(d // bin_width, n_bins - 1) == b.  Waits for the adds; leaves the accumulator as it is"""
        nb, bw = _hist_args("Depth.histogram", n_bins, bin_width)
        out = np.zeros(nb, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_depth_histogram(self.h, nb, bw, out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out

    def device_ptr(self):
        return int(self.L.fin_depth_device_diff(self.h) or 0)


class Pileup(_Accumulator):
    """which base was seen at each position of the concatenated unitig text, resident in HBM beside one replica of the index (fin_pileup_* of the C ABI;
    DESIGN.md 4.19): cover[g] = the placed reads that span g, alt[g][b] = how many of them show base b where the text has another.  A read counts when its found
    k-mers lie on one diagonal of one unitig, the whole read lies inside that unitig and it has at most max_mismatch mismatches."""
    _FREE, _RESET = "fin_pileup_free", "fin_pileup_reset"

    def __init__(self, index, device=0, max_mismatch=8):
        self.index = index
        self.n_unitigs = index.n_unitigs
        self.total_len = index.total_len
        self.max_mismatch = int(max_mismatch)
        if not 0 <= self.max_mismatch <= 255:
            raise FinitoError(FIN_EINVAL, "Pileup: max_mismatch is 0 .. 255")
        self._create("fin_pileup_create", index.h, int(device), self.max_mismatch)

    def add(self, batch, stream=None):
        """pileup += the reads of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_pileup).  Adding the same run twice
        counts it twice."""
        return _acc_add(self, "fin_batch_add_pileup", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and add its reads; nothing comes back (fin_search_batch_add_pileup)"""
        return _acc_add_reads(self, "fin_search_batch_add_pileup", reads, strands)

    def download(self):
        """(uint32 cover[total_len], uint32 alt[total_len, 4], uint64 counters[4] = reads kept, not straight, off their unitig, with too many mismatches); waits
        for the adds, runs cover's prefix sum on the device and leaves the accumulator as it is (fin_pileup_download)"""
        cover = np.zeros(max(self.total_len, 1), dtype=np.uint32)
        alt = np.zeros((max(self.total_len, 1), 4), dtype=np.uint32)
        counters = np.zeros(4, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_pileup_download(self.h, cover.ctypes.data_as(C.c_void_p), alt.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          err, 512), err)
        return cover[: self.total_len], alt[: self.total_len], counters

    def call(self, min_alt=2, min_permille=200, cap=None):
        """the candidate positions as a VARIANT_DTYPE array, ascending: those whose greatest alt count m has m >= max(min_alt, 1) and
        1000 m >= min_permille * cover (fin_pileup_call).  cap: room for so many -- FinitoError FIN_ELIMIT beyond; None: as many as there are"""
        err = C.create_string_buffer(512)
        n = C.c_uint64(0)
        room = 1024 if cap is None else int(cap)
        while True:
            out = np.zeros(max(room, 1), dtype=VARIANT_DTYPE)
            rc = self.L.fin_pileup_call(self.h, int(min_alt), int(min_permille), out.ctypes.data_as(C.c_void_p), room, C.byref(n), err, 512)
            if rc == FIN_ELIMIT and cap is None and int(n.value) > room:
                room = int(n.value)
                continue
            _check(rc, err)
            return out[: int(n.value)]

    def device_ptrs(self):
        """(alt uint32[total_len][4], cover's difference array int32[total_len + 1]) in HBM"""
        return int(self.L.fin_pileup_device_alt(self.h) or 0), int(self.L.fin_pileup_device_cover_diff(self.h) or 0)


FIN_FRAG_NONE, FIN_FRAG_ONE, FIN_FRAG_SPLIT, FIN_FRAG_TANDEM, FIN_FRAG_OUTWARD, FIN_FRAG_INWARD = range(6)
FIN_FRAG_MAX_BINS = 4096
FRAGMENT_CLASS_NAMES = ("none", "one", "split", "tandem", "outward", "inward")


def _frag_hist_args(what, n_bins, bin_width):
    nb, bw = int(n_bins), int(bin_width)
    if not 1 <= nb <= FIN_FRAG_MAX_BINS:
        raise FinitoError(FIN_EINVAL, "%s: n_bins is 1 .. %d" % (what, FIN_FRAG_MAX_BINS))
    if not 1 <= bw <= 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: bin_width is 1 .. 2^32 - 1" % what)
    return nb, bw


def effective_lengths(hist, ref_lengths, bin_width=1):
    """host: float64[n], the effective length of references of ref_lengths[n] bases under the fragment-length histogram `hist` (fin_effective_lengths;
    include/finito_amd.h): the length minus the mean of the fragment lengths that fit, plus one; the last bin, "this much or more", is left out.  bin_width must
    be 1"""
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    rl = np.ascontiguousarray(ref_lengths, dtype=np.uint64).reshape(-1)
    if int(bin_width) != 1:
        raise FinitoError(FIN_EINVAL, "effective_lengths: bin_width must be 1 (it is %d): effective lengths are read from a histogram of single lengths" % int(bin_width))
    if not 1 <= len(h) <= FIN_FRAG_MAX_BINS:
        raise FinitoError(FIN_EINVAL, "effective_lengths: the histogram must have 1 .. %d bins (it has %d)" % (FIN_FRAG_MAX_BINS, len(h)))
    out = np.zeros(max(len(rl), 1), dtype=np.float64)
    rc = lib().fin_effective_lengths(h.ctypes.data_as(C.c_void_p), len(h), int(bin_width), rl.ctypes.data_as(C.c_void_p), len(rl), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise FinitoError(rc, "fin_effective_lengths refused its arguments")
    return out[: len(rl)]


class FragmentStats:
    """what Fragments.download() returns: hist uint64[n_bins] of the inward fragments' lengths (bin b: min(length // bin_width, n_bins - 1) == b), counters
    uint64[7] = the six classes and len_sum; the classes by name (none, one, split, tandem, outward, inward), n_fragments their sum"""

    def __init__(self, hist, counters, bin_width):
        self.hist, self.counters, self.bin_width = hist, counters, int(bin_width)
        self.n_bins = len(hist)
        for i, name in enumerate(FRAGMENT_CLASS_NAMES):
            setattr(self, name, int(counters[i]))
        self.len_sum = int(counters[6])
        self.n_fragments = sum(int(c) for c in counters[:6])

    @property
    def mean(self):
        """the mean length of the inward fragments, None without one"""
        return self.len_sum / self.inward if self.inward else None

    def quantile(self, permille):
        """(length, saturated) of the inward fragments under histogram_quantile's rule, None without one"""
        return histogram_quantile(self.hist, permille, self.bin_width)

    def effective_lengths(self, ref_lengths):
        """float64[n]: effective_lengths() under this histogram (bin_width must be 1)"""
        return effective_lengths(self.hist, ref_lengths, self.bin_width)


class Fragments(_Accumulator):
    """the insert-size histogram and the class counters of a run's fragments -- interleaved mates, fragment f = reads 2f and 2f + 1 --, resident in HBM beside one
    replica of the index (fin_fragments_* of the C ABI; include/finito_amd.h: FRAGMENT GEOMETRY)"""
    _FREE, _RESET = "fin_fragments_free", "fin_fragments_reset"

    def __init__(self, index, device=0, n_bins=1024, bin_width=1):
        self.index = index
        self.n_bins, self.bin_width = _frag_hist_args("Fragments", n_bins, bin_width)
        self._create("fin_fragments_create", index.h, int(device), self.n_bins, self.bin_width)

    def add(self, batch, stream=None):
        """accumulator += the fragments of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_fragments).  Adding the same run
        twice counts it twice."""
        return _acc_add(self, "fin_batch_add_fragments", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search interleaved mates from host buffers, sub-batches pipelined and cut between pairs only, and add their fragments; nothing comes back
        (fin_search_batch_add_fragments)"""
        return _acc_add_reads(self, "fin_search_batch_add_fragments", reads, strands)

    def download(self):
        """FragmentStats; waits for the adds and leaves the accumulator as it is (fin_fragments_download)"""
        hist = np.zeros(self.n_bins, dtype=np.uint64)
        counters = np.zeros(7, dtype=np.uint64)
        err = C.create_string_buffer(512)
        _check(self.L.fin_fragments_download(self.h, hist.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p), err, 512), err)
        return FragmentStats(hist, counters, self.bin_width)

    def device_ptr(self):
        """uint64 hist[n_bins], then the seven counters, in HBM"""
        return int(self.L.fin_fragments_device_hist(self.h) or 0)


FIN_LINKS_MAX = 1 << 28
LINK_DTYPE = np.dtype([("u_a", np.uint32), ("off_a", np.uint32), ("u_b", np.uint32), ("off_b", np.uint32), ("count", np.uint64)])   # fin_link
LINK_EDGE_DTYPE = np.dtype([("u_a", np.uint32), ("end_a", "S1"), ("u_b", np.uint32), ("end_b", "S1"), ("count", np.uint64)])
_M64 = (1 << 64) - 1


def link_hash(key):
    """the link table's hash (fin_link_hash of the C ABI, restated here): a key's home slot is link_hash(key) & (cap - 1)"""
    x = int(key) & _M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _links_canonical(links):
    """LINK_DTYPE in the canonical order: ascending by (g_a, g_b), which is ascending by (u_a, off_a, u_b, off_b)"""
    links = np.ascontiguousarray(links, dtype=LINK_DTYPE).reshape(-1)
    return links[np.lexsort((links["off_b"], links["u_b"], links["off_a"], links["u_a"]))]


class UnitigEdges:
    """LinkTable.unitig_edges' result: `edges`, LINK_EDGE_DTYPE ascending by (u_a, end_a, u_b, end_b) with the counts summed; n_edge, the transitions along edges
    of the graph (both ends S, E or B); n_jump, those with an interior end"""
    def __init__(self, edges, n_edge, n_jump):
        self.edges, self.n_edge, self.n_jump = edges, int(n_edge), int(n_jump)


class LinkTable:
    """a downloaded link table (include/finito_amd.h: LINKS): `links`, LINK_DTYPE in the canonical order -- the a end is the lower place --; `transitions`, how many
    were counted; `n_distinct`, the distinct links of the whole table; `n_self`, those of them whose two places are equal"""
    def __init__(self, links, transitions, n_distinct, n_self):
        self.links, self.transitions, self.n_distinct, self.n_self = links, int(transitions), int(n_distinct), int(n_self)

    def unitig_edges(self, ends, k):
        """host: every end of every link classed by where it lies in its unitig -- S: offset 0, E: the last k-mer, B: both (a unitig of one k-mer), I: the
        interior -- and the counts summed per (u_a, end_a, u_b, end_b).  A link between S / E / B ends walks an edge of the graph; one with an I end is a jump
        that the indexed sequences do not make there.  UnitigEdges"""
        e = np.ascontiguousarray(ends, dtype=np.int64).reshape(-1)
        last = np.diff(np.concatenate([[0], e])) - int(k)   # the offset of a unitig's last k-mer
        lk = self.links

        def cls(u, off):
            o, l = off.astype(np.int64), last[u]
            c = np.full(len(u), b"I", dtype="S1")
            c[o == 0] = b"S"
            c[o == l] = b"E"
            c[(o == 0) & (l == 0)] = b"B"
            return c
        if len(lk) and int(max(lk["u_a"].max(), lk["u_b"].max())) >= len(e):
            raise FinitoError(FIN_EINVAL, "unitig_edges: a link names a unitig beyond `ends`")
        ca, cb = cls(lk["u_a"], lk["off_a"]), cls(lk["u_b"], lk["off_b"])
        sums = {}
        for ua, a, ub, b, c in zip(lk["u_a"].tolist(), ca.tolist(), lk["u_b"].tolist(), cb.tolist(), lk["count"].tolist()):
            sums[(ua, a, ub, b)] = sums.get((ua, a, ub, b), 0) + c
        edges = np.zeros(len(sums), dtype=LINK_EDGE_DTYPE)
        for i, key in enumerate(sorted(sums)):
            edges[i] = key + (sums[key],)
        jump = (edges["end_a"] == b"I") | (edges["end_b"] == b"I")
        return UnitigEdges(edges, edges["count"][~jump].sum(), edges["count"][jump].sum())


def links_merge(a, b):
    """host: two downloaded LinkTables added -- same keys, counts summed, canonical order.  How the tables of several ranks or runs combine.  n_distinct and n_self
    are those of the merged rows: exact when both tables were downloaded with min_count 1"""
    la, lb = _links_canonical(a.links), _links_canonical(b.links)
    both = np.concatenate([la, lb])
    keys = np.stack([both["u_a"], both["off_a"], both["u_b"], both["off_b"]], axis=1).astype(np.uint32)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True) if len(keys) else (keys, np.zeros(0, dtype=np.int64))
    out = np.zeros(len(uniq), dtype=LINK_DTYPE)
    if len(uniq):
        out["u_a"], out["off_a"], out["u_b"], out["off_b"] = uniq[:, 0], uniq[:, 1], uniq[:, 2], uniq[:, 3]
        np.add.at(out["count"], np.asarray(inv).reshape(-1), both["count"])
    out = _links_canonical(out)
    n_self = int(((out["u_a"] == out["u_b"]) & (out["off_a"] == out["off_b"])).sum())
    return LinkTable(out, a.transitions + b.transitions, len(out), n_self)


class Links(_Accumulator):
    """the junctions reads cross, counted in a hash table resident in HBM beside one replica of the index: which edges of the unitig graph a sample walked, and
    how often (fin_links_* of the C ABI; include/finito_amd.h: LINKS).  The table holds up to max_links distinct links and does not grow"""
    _FREE, _RESET = "fin_links_free", "fin_links_reset"

    def __init__(self, index, device=0, max_links=1 << 20):
        self.index = index
        self.max_links = int(max_links)
        if not 0 <= self.max_links < (1 << 64):
            raise FinitoError(FIN_ELIMIT, "Links: max_links is 1 .. 2^28")
        self._create("fin_links_create", index.h, int(device), self.max_links)
        self.capacity = int(self.L.fin_links_capacity(self.h))

    def add(self, batch, stream=None):
        """table += the transitions of the batch's most recent run, on a HIP stream, behind that run; no sync (fin_batch_add_links).  Adding the same run twice
        counts it twice."""
        return _acc_add(self, "fin_batch_add_links", batch, stream)

    def add_reads(self, reads, strands=FIN_MERGED):
        """search a read set from host buffers, sub-batches pipelined as in search_reads, and add its transitions; nothing comes back (fin_search_batch_add_links)"""
        return _acc_add_reads(self, "fin_search_batch_add_links", reads, strands)

    def download(self, min_count=1):
        """LinkTable of the links with count >= max(min_count, 1), filtered, compacted and decoded on the device; waits for the adds and leaves the accumulator as
        it is (fin_links_download)"""
        mc = int(min_count)
        if not 0 <= mc < (1 << 64):
            raise FinitoError(FIN_EINVAL, "Links.download: min_count is an unsigned 64-bit number")
        n, err = C.c_uint64(0), C.create_string_buffer(512)
        _check(self.L.fin_links_download(self.h, mc, None, 0, C.byref(n), None, err, 512), err)
        links = np.zeros(max(int(n.value), 1), dtype=LINK_DTYPE)
        counters = np.zeros(4, dtype=np.uint64)
        _check(self.L.fin_links_download(self.h, mc, links.ctypes.data_as(C.c_void_p), len(links), C.byref(n), counters.ctypes.data_as(C.c_void_p), err, 512), err)
        return LinkTable(links[: int(n.value)], counters[0], counters[1], counters[3])

    def device_ptr(self):
        """`capacity` slots of {uint64 key, uint64 count}, then uint64 n_distinct, in HBM"""
        return int(self.L.fin_links_device_table(self.h) or 0)


def _window_args(what, window, min_depth):
    w, md = int(window), int(min_depth)
    if not 1 <= w <= 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: window is 1 .. 2^32 - 1" % what)
    if not 0 <= md <= 0xFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: min_depth is an unsigned 32-bit number" % what)
    return w, md


def _path_set(what, seq_nk, seg_offs, segs):
    nk = np.ascontiguousarray(seq_nk, dtype=np.uint32).reshape(-1)
    so = np.ascontiguousarray(seg_offs, dtype=np.uint64).reshape(-1)
    sg = np.ascontiguousarray(segs, dtype=SEGMENT_DTYPE).reshape(-1)
    if len(so) != len(nk) + 1 or int(so[-1]) > len(sg):
        raise FinitoError(FIN_EINVAL, "%s: seg_offs has one entry more than seq_nk and its last entry is the number of segments" % what)
    return nk, so, sg


class RefDepth:
    """what depth_windows returns: win_offs uint64[n_seqs + 1] and windows REF_WINDOW_DTYPE[n_windows] -- sequence s owns windows win_offs[s] .. win_offs[s + 1] - 1,
    window w of it the slots [w * window, (w + 1) * window); mean_depth = depth_sum / in_graph and breadth = covered / in_graph per window, float64, nan where
    no slot of the window lies in the graph"""

    def __init__(self, win_offs, windows, window, min_depth):
        self.win_offs, self.windows, self.window, self.min_depth = win_offs, windows, int(window), int(min_depth)

    def of(self, seq):
        """the windows of sequence `seq`"""
        return self.windows[int(self.win_offs[seq]):int(self.win_offs[seq + 1])]

    @staticmethod
    def _ratio(num, den):
        out = np.full(len(den), np.nan, dtype=np.float64)
        np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
        return out

    @property
    def mean_depth(self):
        return self._ratio(self.windows["depth_sum"], self.windows["in_graph"])

    @property
    def breadth(self):
        return self._ratio(self.windows["covered"], self.windows["in_graph"])


class RefPaths(_Accumulator):
    """the paths of sequences -- reference records searched as reads -- through the unitig set, as segments in HBM beside one replica of the index (fin_refpaths_* of
    the C ABI; include/finito_amd.h: REFERENCE COORDINATES): what lifts depth and variant candidates from unitig coordinates onto the sequences"""
    _FREE, _RESET = "fin_refpaths_free", "fin_refpaths_reset"

    def __init__(self, index, device=0):
        self.index = index
        self._create("fin_refpaths_create", index.h, int(device))

    def add(self, batch, stream=None):
        """append the reads of the batch's most recent run as sequences, device to device on a HIP stream behind that run (fin_batch_add_refpaths)"""
        return _acc_add(self, "fin_batch_add_refpaths", batch, stream)

    def add_reads(self, seqs):
        """search sequences from host buffers, sub-batches pipelined and cut between sequences only, and append their paths (fin_search_batch_add_refpaths)"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_add_refpaths(self.index.h, *_reads_args(seqs), self.h, err, 512), err)
        return self

    @property
    def n_seqs(self): return int(self.L.fin_refpaths_n_seqs(self.h))
    @property
    def n_segments(self): return int(self.L.fin_refpaths_n_segments(self.h))
    @property
    def n_slots(self): return int(self.L.fin_refpaths_n_slots(self.h))

    def upload(self, seq_nk, seg_offs, segs):
        """replace the path set by host arrays; FinitoError FIN_EINVAL names the first segment that is not valid against the index (fin_refpaths_upload)"""
        nk, so, sg = _path_set("RefPaths.upload", seq_nk, seg_offs, segs)
        err = C.create_string_buffer(512)
        _check(self.L.fin_refpaths_upload(self.h, nk.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), len(nk), err, 512), err)
        return self

    def download(self):
        """(seq_nk uint32[n_seqs], seg_offs uint64[n_seqs + 1], segs SEGMENT_DTYPE[n_segments]); waits for the appends (fin_refpaths_download)"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_refpaths_download(self.h, None, None, None, err, 512), err)
        ns, ng = self.n_seqs, self.n_segments
        nk = np.zeros(max(ns, 1), dtype=np.uint32); so = np.zeros(ns + 1, dtype=np.uint64); sg = np.zeros(max(ng, 1), dtype=SEGMENT_DTYPE)
        _check(self.L.fin_refpaths_download(self.h, nk.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), err, 512), err)
        return nk[:ns], so, sg[:ng]

    def depth_windows(self, depth, window=1000, min_depth=1):
        """RefDepth: a Depth accumulator lifted onto the sequences in windows of `window` slots, on the device; only the windows come back (fin_refpaths_depth)"""
        w, md = _window_args("RefPaths.depth_windows", window, min_depth)
        err = C.create_string_buffer(512)
        n = C.c_uint64(0)
        rc = self.L.fin_refpaths_depth(self.h, depth.h, w, md, None, None, 0, C.byref(n), err, 512)
        if rc != FIN_ELIMIT:
            _check(rc, err)
        wo = np.zeros(self.n_seqs + 1, dtype=np.uint64)
        out = np.zeros(max(int(n.value), 1), dtype=REF_WINDOW_DTYPE)
        _check(self.L.fin_refpaths_depth(self.h, depth.h, w, md, wo.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(n.value), C.byref(n), err, 512), err)
        return RefDepth(wo, out[: int(n.value)], w, md)

    def lift_variants(self, variants):
        """REF_VARIANT_DTYPE[n]: Pileup.call's candidates under every sequence that crosses them -- seq, pos (the sequence base, 0-based), var (the index into
        `variants`), flags (bit 0: the sequence runs against the text there, bases are to be complemented); by segment, then by pos (fin_refpaths_lift_variants)"""
        v = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE).reshape(-1)
        err = C.create_string_buffer(512)
        n = C.c_uint64(0)
        room = max(1024, 4 * len(v))   # (a candidate usually lies under a few sequences: one call; beyond that the refusal says how many there are)
        while True:
            out = np.zeros(room, dtype=REF_VARIANT_DTYPE)
            rc = self.L.fin_refpaths_lift_variants(self.h, v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p), room, C.byref(n), err, 512)
            if rc == FIN_ELIMIT and int(n.value) > room:
                room = int(n.value)
                continue
            _check(rc, err)
            return out[: int(n.value)]

    def device_ptrs(self):
        """(segments, seg_offs) in HBM"""
        return int(self.L.fin_refpaths_device_segments(self.h) or 0), int(self.L.fin_refpaths_device_segment_offsets(self.h) or 0)


def ref_variant_bases(lifted, variants):
    """(ref uint32[n], alt uint32[n, 4]) of lifted records in the SEQUENCE's orientation: the text's base code and the four alt counts (A, C, G, T) of
    variants[lifted["var"]], complemented -- code b becomes 3 - b -- where bit 0 of flags is set"""
    v = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE).reshape(-1)
    l = np.ascontiguousarray(lifted, dtype=REF_VARIANT_DTYPE).reshape(-1)
    rev = (l["flags"] & 1) != 0
    ref = v["ref"][l["var"]].astype(np.uint32)
    alt = v["alt"][l["var"]].reshape(-1, 4).astype(np.uint32)
    return np.where(rev, 3 - ref, ref).astype(np.uint32), np.where(rev[:, None], alt[:, ::-1], alt)


class FinimizerIndex:
    """Mirror of the reference class (FinimizerIndex.hh:26-259) backed by the HIP path."""

    def __init__(self, handle=None):
        self.L = lib()
        self.h = handle

    # -- construction / persistence ---------------------------------------------------------------------------
    @classmethod
    def build(cls, unitigs, k, n_threads=0):
        """FinimizerIndexBuilder (FinimizerIndex.hh:262-395) + `sbwt build` + LCS, in one call."""
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(L.fin_index_build(*_reads_args(unitigs), int(k), int(n_threads) if n_threads > 0 else host_threads(), C.byref(h), err, 512), err)
        return cls(h)

    @classmethod
    def build_on_device(cls, unitigs, k, device=0):
        """the same index built on a HIP device (fin_index_build_device; every k <= 255): bit-identical to build()'s.  The stages' device
        times in milliseconds are left in .build_phase_ms"""
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        ph = (C.c_double * 8)()
        L.fin_index_build_device.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
        _check(L.fin_index_build_device(*_reads_args(unitigs), int(k), int(device),
                                        C.byref(h), ph, err, 512), err)
        x = cls(h)
        x.build_phase_ms = dict(zip(("upload_kmers", "sort_unique", "dummies", "sbwt", "unitigs", "finimizers", "dictionaries", "copy_back"), (float(v) for v in ph)))
        return x

    def load(self, index_prefix):
        """FinimizerIndex::load (FinimizerIndex.hh:209-241)."""
        self.close()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_load(str(index_prefix).encode(), C.byref(h), err, 512), err)
        self.h = h
        return self

    def serialize(self, index_prefix):
        """FinimizerIndex::serialize (FinimizerIndex.hh:187-207)."""
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_save(self.h, str(index_prefix).encode(), err, 512), err)

    def serialize_reference_layout(self, index_prefix):
        """FinimizerIndex::serialize in the reference's own seven-file layout (FinimizerIndex.hh:187-207); parity unpinned."""
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_save_reference_layout(self.h, str(index_prefix).encode(), err, 512), err)

    def load_reference_layout(self, index_prefix):
        self.close()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_load_reference_layout(str(index_prefix).encode(), C.byref(h), err, 512), err)
        self.h = h
        return self

    def save_sbwt(self, path):
        """the SBWT as `sbwt build` writes it (what build-fmin -i reads)"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_save_sbwt(self.h, str(path).encode(), err, 512), err)

    def check_against_files(self, sbwt_path=None, lcs_path=None):
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_check_against_files(self.h, str(sbwt_path).encode() if sbwt_path else None,
                                                    str(lcs_path).encode() if lcs_path else None, err, 512), err)

    def size_in_bytes(self):
        return int(self.L.fin_index_size_in_bytes(self.h))

    def finimizer_stats(self, seqs, kind="shortest", t=1):
        """build-fmin --type shortest / verify (build_fmin.hh:95-214): (distinct finimizers, sum of frequencies, sum of lengths)."""
        n, sf, sl = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_finimizer_stats(self.h, *_reads_args(seqs), 1 if kind == "shortest" else 2, int(t), C.byref(n), C.byref(sf), C.byref(sl), err, 512), err)
        return int(n.value), int(sf.value), int(sl.value)

    def prefix_table_depth(self, device=0):
        """T of the 4^T-entry prefix table the device replica carries for the kernel's probe mode (0: none)."""
        return int(self.L.fin_index_prefix_table_depth(self.h, int(device)))

    def is_disjoint(self):
        """every k-mer of the index has exactly one place in the unitigs (fin_index_is_disjoint)"""
        return bool(self.L.fin_index_is_disjoint(self.h))

    def seed_table(self, device=0):
        """the device replica's anchor table as a numpy array [n_nodes, 2] of u32: [:, 0] = the reference's answer for the node's k-mer
        (offset of its last base in the concatenated unitigs; 0xFFFFFFFF: none; 0xFFFFFF00 | d: a dummy node), [:, 1] = the entry's
        unitig with the top bit set when the text at that place does not spell the k-mer (unverified).  None when that replica has no
        table (option seed_anchors 0 at upload)"""
        import numpy as np
        out = np.empty((self.n_nodes, 2), dtype=np.uint32)
        err = C.create_string_buffer(512)
        rc = self.L.fin_index_debug_seed_table(self.h, int(device), out.ctypes.data_as(C.c_void_p), err, 512)
        return out if rc == 0 else None

    def debug_table(self, what, device=0):
        """fin_index_debug_table: a derived table of the device replica as it lies in HBM (DT_*), or None when that replica carries none: DT_PTAB / DT_JTAB
        uint32 [4^T, 2] (l, r), DT_FILT uint32 words, DT_SAFE uint64 words (bit g & 63 of word g >> 6), DT_RCWIN uint8 (a byte per 512 text positions),
        DT_CBF / DT_FBF uint32 [blocks, 4]"""
        nbytes = int(self.L.fin_index_debug_table_bytes(self.h, int(device), int(what)))
        if nbytes < 0:
            raise FinitoError(FIN_EINVAL, "debug_table: no replica on device %d, or no table %r" % (device, what))
        if nbytes == 0:
            return None
        dt = {DT_SAFE: np.uint64, DT_RCWIN: np.uint8}.get(what, np.uint32)
        out = np.zeros(nbytes // np.dtype(dt).itemsize, dtype=dt)
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_debug_table(self.h, int(device), int(what), out.ctypes.data_as(C.c_void_p), out.nbytes, err, 512), err)
        return out.reshape(-1, 2) if what in (DT_PTAB, DT_JTAB) else out.reshape(-1, 4) if what in (DT_CBF, DT_FBF) else out

    def string_filter_geometry(self, device=0):
        """(cbf_m, cbf_log2) of the device replica's string filters: the length of their strings and log2 of their number of 128-bit blocks; (0, 0): none"""
        m, lg = C.c_uint32(0), C.c_uint32(0)
        rc = self.L.fin_index_string_filter_geometry(self.h, int(device), C.byref(m), C.byref(lg))
        if rc != 0:
            raise FinitoError(rc, "string_filter_geometry: no replica on device %d" % device)
        return int(m.value), int(lg.value)

    def kmer_table_query(self, kmers, device=0):
        """fin_index_debug_kmer_table: what the compact k-mer table claims about each k-mer (strings over ACGT of length k): (g, flags) arrays"""
        k = self.k
        code = {"A": 0, "C": 1, "G": 2, "T": 3}
        k0 = np.zeros(len(kmers), dtype=np.uint64); k1 = np.zeros(len(kmers), dtype=np.uint64)
        for i, s in enumerate(kmers):
            a = b = 0
            for j, ch in enumerate(s):
                if j < 32: a |= code[ch] << (2 * j)
                else: b |= code[ch] << (2 * (j - 32))
            k0[i] = a; k1[i] = b
        out = np.zeros((len(kmers), 2), dtype=np.uint32)
        err = C.create_string_buffer(512)
        self.L.fin_index_debug_kmer_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]
        _check(self.L.fin_index_debug_kmer_table(self.h, int(device), k0.ctypes.data_as(C.c_void_p), k1.ctypes.data_as(C.c_void_p), len(kmers), out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[:, 0].copy(), out[:, 1].copy()

    def seed_table_bytes(self, device=0):
        """bytes of the anchor table the device replica carries (0: none -- option seed_anchors 0 at upload)"""
        return int(self.L.fin_index_seed_table_bytes(self.h, int(device)))

    def set_option(self, name, value):
        """fin_index_set_option: this handle's own value of a tuning switch (None: follow the process-wide value again)"""
        nm = name.encode() if isinstance(name, str) else name
        rc = self.L.fin_index_clear_option(self.h, nm) if value is None else self.L.fin_index_set_option(self.h, nm, int(value))
        if rc != 0:
            raise FinitoError(rc, "bad option %r = %r" % (name, value))
        return self

    def kmer_table_bytes(self, device=0):
        """bytes of the k-mer table (text k-mer -> SBWT node) the device replica carries (0: none -- k > 31, or option kmer_table 0 at upload)"""
        return int(self.L.fin_index_kmer_table_bytes(self.h, int(device)))

    def string_filter_bytes(self, device=0):
        """bytes of the canonical string filter the device replica carries (round 4: the fast path's absence proofs; 0: none)"""
        return int(self.L.fin_index_string_filter_bytes(self.h, int(device)))

    def replica_table_bytes(self, device=0):
        """HBM the device replica occupies beyond the index arrays: every derived table, filter and bitmap (fin_index_replica_table_bytes)"""
        return int(self.L.fin_index_replica_table_bytes(self.h, int(device)))

    def unsafe_places(self, device=0):
        """k-mer positions of the unitig text that are not the place the reference reports for their k-mer (0 on disjoint unitigs;
        -1: not computed) -- fin_index_unsafe_places"""
        return int(self.L.fin_index_unsafe_places(self.h, int(device)))

    def unverified_kmers(self, device=0):
        """k-mer places whose k-mer's answer is a place that does not spell it (kept whole in the k-mer table's exact side table); -1: no anchor pass"""
        self.L.fin_index_unverified_kmers.restype = C.c_int64
        self.L.fin_index_unverified_kmers.argtypes = [C.c_void_p, C.c_int]
        return int(self.L.fin_index_unverified_kmers(self.h, device))

    def rc_pairs(self, device=0):
        """k-mers of the unitig text whose reverse complement is in the index too (fin_index_rc_pairs; -1: not counted)"""
        return int(self.L.fin_index_rc_pairs(self.h, int(device)))

    def defers_second_strand(self, device=0):
        """kernel 4 may search a read's second strand only where the first left slots open on this replica (option defer_strand aside)"""
        return self.rc_pairs(device) >= 0 and (self.seed_table_bytes(device) > 0 or self.lean_tables(device))

    def lean_tables(self, device=0):
        """the replica was uploaded with "lean_tables" (k <= 31, the default): k-mer table + string filters, no prefix table, no anchor table"""
        return self.seed_table_bytes(device) == 0 and self.kmer_table_bytes(device) > 0 and self.string_filter_bytes(device) > 0 and self.prefix_table_depth(device) == 0

    def anchor_build_ms(self, device=0):
        return float(self.L.fin_index_anchor_build_ms(self.h, int(device)))

    def filter_depth(self, device=0):
        """F of the 4^F-bit absence filter the device replica carries for the pre-pass (0: none)."""
        return int(self.L.fin_index_filter_depth(self.h, int(device)))

    def jump_table_depth(self, device=0):
        """J of the 4^J-entry jump table the device replica carries for (re)started streaming searches (0: none)."""
        return int(self.L.fin_index_jump_table_depth(self.h, int(device)))

    def to_device(self, device=0):
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_to_device(self.h, int(device), err, 512), err)
        return self

    # -- scalar members -----------------------------------------------------------------------------------------
    @property
    def k(self): return int(self.L.fin_index_k(self.h))
    @property
    def n_nodes(self): return int(self.L.fin_index_n_nodes(self.h))
    @property
    def n_kmers(self): return int(self.L.fin_index_n_kmers(self.h))
    @property
    def n_unitigs(self): return int(self.L.fin_index_n_unitigs(self.h))
    @property
    def n_finimizers(self): return int(self.L.fin_index_n_finimizers(self.h))
    @property
    def total_len(self): return int(self.L.fin_index_total_len(self.h))

    def export(self, what):
        """Decoded view of a public member of the reference class (FinimizerIndex.hh:108-115)."""
        nbytes = int(self.L.fin_index_export_size(self.h, what))
        dt = {X_C: np.int64, X_LCS: np.uint8, X_GOFF: np.int64, X_ENDS: np.int64, X_CONCAT: np.uint8}.get(what, np.uint64)
        out = np.zeros(max(nbytes // np.dtype(dt).itemsize, 1), dtype=dt)
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_export(self.h, what, out.ctypes.data_as(C.c_void_p), out.nbytes, err, 512), err)
        return out[: nbytes // np.dtype(dt).itemsize]

    def components(self):
        """Everything the oracle needs to assemble the same index (tests / cpu_baseline at large sizes)."""
        return {"n_nodes": self.n_nodes, "planes": [self.export(X_PLANE_A + c) for c in range(4)], "lcs": self.export(X_LCS),
                "fmin": self.export(X_FMIN), "ustart": self.export(X_USTART), "goff": self.export(X_GOFF),
                "n_fmin": self.n_finimizers, "concat": self.export(X_CONCAT), "ends": self.export(X_ENDS)}

    # -- queries ------------------------------------------------------------------------------------------------
    def search(self, query):
        """FinimizerIndex::search(const std::string&) (FinimizerIndex.hh:119): one strand of one read."""
        qb = query.encode() if isinstance(query, str) else bytes(query)
        nk = max(0, len(qb) - self.k + 1)
        out = np.zeros(2 * nk + 2, dtype=np.int64)
        nf = C.c_int64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search(self.h, qb, len(qb), out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nf), err, 512), err)
        return QueryResult([(int(out[2 * i]), int(out[2 * i + 1])) for i in range(nk)], int(nf.value))

    def search_reads(self, reads, strands=FIN_MERGED, out=None):
        """run_fmin_queries_streaming (search_fmin.hh:33-84) over host buffers (fin_search_batch): (int32 pairs [n_kmers, 2],
        total_positive).  `out` may be a preallocated (e.g. PinnedArray(...).array) int32 [>= n_kmers, 2] buffer."""
        bases, offsets = flatten(reads)
        lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
        nk = int(np.maximum(lens - self.k + 1, 0).sum())
        if out is None:
            out = np.empty((max(nk, 1), 2), dtype=np.int32)
        assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and out.shape[0] >= max(nk, 1)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch(self.h, *_reads_args((bases, offsets)), int(strands), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(npos), err, 512), err)
        return out[:nk], int(npos.value)

    def search_reads_records(self, reads):
        """fin_search_batch_records: (records, stream) -- a 32-byte record per read (structured array: u, off0, meta, nk, Es, Es2) and the pairs of the
        reads whose record says "nk pairs follow" (kind 0), back to back"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        nk = int(np.maximum(np.diff(offsets.astype(np.int64)) - self.k + 1, 0).sum())
        recs = np.zeros(n, dtype=RECORD_DTYPE)
        stream = np.empty((max(nk, 1), 2), dtype=np.int32)
        got = C.c_uint64(0)
        err = C.create_string_buffer(512)
        self.L.fin_search_batch_records.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        _check(self.L.fin_search_batch_records(self.h, *_reads_args((bases, offsets)),
                                               recs.ctypes.data_as(C.c_void_p), stream.ctypes.data_as(C.c_void_p), nk, C.byref(got), err, 512), err)
        return recs, stream[: int(got.value)]

    def search_reads_segments(self, reads, strands=FIN_MERGED):
        """fin_search_batch_segments: (seg_offs uint64[n_reads + 1], segs SEGMENT_DTYPE[n_segments], n_positive) -- every read's found stretches inside a
        unitig, made on the device; nothing per k-mer comes back"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        nk = int(np.maximum(np.diff(offsets.astype(np.int64)) - self.k + 1, 0).sum())
        seg_offs = np.zeros(n + 1, dtype=np.uint64)
        segs = np.zeros(max(nk, 1), dtype=SEGMENT_DTYPE)
        got, npos = C.c_uint64(0), C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_segments(self.h, *_reads_args((bases, offsets)), int(strands),
                                                seg_offs.ctypes.data_as(C.POINTER(C.c_uint64)), segs.ctypes.data_as(C.c_void_p), nk, C.byref(got), C.byref(npos), err, 512), err)
        return seg_offs, segs[: int(got.value)].copy(), int(npos.value)

    def search_reads_summaries(self, reads, strands=FIN_MERGED):
        """fin_search_batch_read_summaries: (READ_SUMMARY_DTYPE[n_reads], n_positive) -- 16 bytes per read come back, nothing per k-mer"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=READ_SUMMARY_DTYPE)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_read_summaries(self.h, *_reads_args((bases, offsets)), int(strands),
                                                      out.ctypes.data_as(C.c_void_p), C.byref(npos), err, 512), err)
        return out[:n], int(npos.value)

    def screen_reads(self, reads, min_found=1, min_permille=0, invert=False, strands=FIN_MERGED):
        """fin_search_batch_screen: a bool per read -- it passes (n_found >= min_found and 1000 * n_found >= min_permille * nk) != invert; one bit per read
        comes back"""
        if not (0 <= int(min_found) <= 0xFFFFFFFF and 0 <= int(min_permille) <= 0xFFFFFFFF):
            raise FinitoError(FIN_EINVAL, "screen_reads: min_found and min_permille are unsigned 32-bit numbers")
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        bits = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        n_pass = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_screen(self.h, *_reads_args((bases, offsets)), int(strands),
                                              int(min_found), int(min_permille), 1 if invert else 0, bits.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              C.byref(n_pass), err, 512), err)
        out = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
        if int(out.sum()) != int(n_pass.value):
            raise FinitoError(FIN_EINVAL, "screen_reads: the bitmap holds %d reads, the device counted %d" % (int(out.sum()), int(n_pass.value)))
        return out

    def labels(self, unitig_labels, n_labels=None, device=0):
        """a labelling of this index's unitigs beside the replica on `device`, with a zeroed tally (Labels); n_labels defaults to the largest label + 1"""
        return Labels(self, unitig_labels, n_labels, device)

    def classify_reads(self, reads, labels, strands=FIN_MERGED):
        """fin_search_batch_classify: READ_CLASS_DTYPE[n_reads] from host buffers -- 16 bytes per read come back, nothing per k-mer"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=READ_CLASS_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_classify(self.h, *_reads_args((bases, offsets)), int(strands), labels.h,
                                                out.ctypes.data_as(C.c_void_p), None, err, 512), err)
        return out[:n]

    def taxonomy(self, parent, unitig_labels, device=0):
        """a Taxonomy of this index beside the replica on `device` from a labelling the caller brings: a taxon (or FIN_NO_LABEL) per unitig"""
        return Taxonomy(self, parent, unitig_labels, device)

    def taxa_reads(self, reads, tax, min_found=1, confidence=0, strands=FIN_MERGED):
        """fin_search_batch_taxa: READ_TAXON_DTYPE[n_reads] from host buffers -- 16 bytes per read come back, nothing per k-mer"""
        t = _taxa_thresholds("taxa_reads", min_found, confidence)
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=READ_TAXON_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_taxa(self.h, *_reads_args((bases, offsets)), int(strands), tax.h, *t, out.ctypes.data_as(C.c_void_p), None, err, 512), err)
        return out[:n]

    def colors(self, n_colors, bits=None, device=0, set_of=None, sets=None):
        """a colour matrix of this index on `device` (Colors), zeroed or holding `bits`; or compact from the start, from set_of and sets (both or neither;
        Colors.upload_sets)"""
        if (set_of is None) != (sets is None) or (bits is not None and sets is not None):
            raise FinitoError(FIN_EINVAL, "colors: set_of and sets go together, and not beside bits")
        c = Colors(self, n_colors, device)
        if sets is not None:
            return c.upload_sets(set_of, sets)
        return c if bits is None else c.upload(bits)

    def pseudoalign_reads(self, reads, colors, permille=1000, strands=FIN_MERGED, want_rows=True):
        """(rows uint64[n_reads, W] or None, heads READ_PSEUDO_DTYPE[n_reads], the coloured k-mers found): a read set pseudoaligned from host buffers, sub-batches
        pipelined (fin_search_batch_pseudoalign)"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        rows = np.zeros((max(n, 1), colors.words), dtype=np.uint64) if want_rows else None
        heads = np.zeros(max(n, 1), dtype=READ_PSEUDO_DTYPE)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_pseudoalign(self.h, *_reads_args((bases, offsets)), int(strands), colors.h,
                                                   _permille("pseudoalign_reads", permille), rows.ctypes.data_as(C.POINTER(C.c_uint64)) if want_rows else None,
                                                   heads.ctypes.data_as(C.c_void_p), C.byref(npos), err, 512), err)
        return (rows[:n] if want_rows else None), heads[:n], int(npos.value)

    def pseudoalign_pairs(self, reads, colors, permille=1000, both=False, strands=FIN_MERGED, want_rows=True):
        """(rows uint64[F, W] or None, heads PAIR_PSEUDO_DTYPE[F], the coloured k-mers found): interleaved mates pseudoaligned as fragments from host buffers,
        sub-batches pipelined and cut between pairs only (fin_search_batch_pseudoalign_paired)"""
        bases, offsets = flatten(reads)
        n = len(offsets) - 1
        nf = n // 2
        rows = np.zeros((max(nf, 1), colors.words), dtype=np.uint64) if want_rows else None
        heads = np.zeros(max(nf, 1), dtype=PAIR_PSEUDO_DTYPE)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_pseudoalign_paired(self.h, *_reads_args((bases, offsets)), int(strands),
                                                          colors.h, _permille("pseudoalign_pairs", permille), FIN_PAIR_BOTH if both else FIN_PAIR_ANY,
                                                          rows.ctypes.data_as(C.POINTER(C.c_uint64)) if want_rows else None, heads.ctypes.data_as(C.c_void_p),
                                                          C.byref(npos), err, 512), err)
        return (rows[:nf] if want_rows else None), heads[:nf], int(npos.value)

    def fragments(self, n_bins=1024, bin_width=1, device=0):
        """a zeroed fragment-length histogram with its class counters beside the replica on `device` (Fragments)"""
        return Fragments(self, device, n_bins, bin_width)

    def links(self, max_links=1 << 20, device=0):
        """an empty link table for up to max_links distinct links beside the replica on `device` (Links)"""
        return Links(self, device, max_links)

    def ref_paths(self, device=0):
        """an empty path set beside the replica on `device` (RefPaths)"""
        return RefPaths(self, device)

    def fragments_reads(self, reads, strands=FIN_MERGED):
        """FRAGMENT_DTYPE[F]: interleaved mates from host buffers as fragments, sub-batches pipelined and cut between pairs only (fin_search_batch_fragments)"""
        bases, offsets = flatten(reads)
        nf = (len(offsets) - 1) // 2
        out = np.zeros(max(nf, 1), dtype=FRAGMENT_DTYPE)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_fragments(self.h, *_reads_args((bases, offsets)), int(strands), out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[:nf]

    def unitig_numbers(self, unitigs):
        """fin_index_unitig_numbers: uint32[len(unitigs)] -- the index's number of each given unitig sequence (the index renumbers its input); raises for a
        sequence that is not a unitig of this index"""
        bases, offsets = flatten(unitigs)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=np.uint32)
        err = C.create_string_buffer(512)
        _check(self.L.fin_index_unitig_numbers(self.h, *_reads_args((bases, offsets)),
                                               out.ctypes.data_as(C.c_void_p), err, 512), err)
        return out[:n]

    def hits(self, device=0):
        """a zeroed per-unitig accumulator beside the replica on `device` (Hits)"""
        return Hits(self, device)

    def unitig_counts(self, reads, strands=FIN_MERGED):
        """the profile of a read set over host buffers (fin_search_batch_unitig_counts): (uint64 counts[n_unitigs], total_positive) -- how many of the
        reads' k-mers were found in each unitig; only the counts come back from the device"""
        out = np.zeros(max(self.n_unitigs, 1), dtype=np.uint64)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_unitig_counts(self.h, *_reads_args(reads),
                                                     int(strands), out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(npos), err, 512), err)
        return out[: self.n_unitigs], int(npos.value)

    def cover(self, device=0):
        """a zeroed coverage bitmap beside the replica on `device` (Cover)"""
        return Cover(self, device)

    def unitig_coverage(self, reads, strands=FIN_MERGED):
        """the breadth of a read set over host buffers (fin_search_batch_unitig_coverage): (uint64 covered[n_unitigs], total_positive) -- how many DISTINCT
        k-mers of each unitig were found, and the k-mers found as search_reads reports them; only the covered numbers come back from the device"""
        out = np.zeros(max(self.n_unitigs, 1), dtype=np.uint64)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_unitig_coverage(self.h, *_reads_args(reads),
                                                       int(strands), out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(npos), err, 512), err)
        return out[: self.n_unitigs], int(npos.value)

    def depth(self, device=0):
        """a zeroed per-position depth accumulator beside the replica on `device` (Depth)"""
        return Depth(self, device)

    def color_coverage(self, reads, colors, min_depth=1, strands=FIN_MERGED):
        """breadth and depth of a read set per reference of `colors` (a Colors of this index): a fresh Cover and Depth beside the colours, the reads searched
        into each, then Colors.coverage -- a ColorCoverage"""
        cov, dep = Cover(self, colors.device), Depth(self, colors.device)
        try:
            reads = flatten(reads)
            cov.add_reads(reads, strands)
            dep.add_reads(reads, strands)
            return colors.coverage(cov, dep, min_depth)
        finally:
            cov.close(); dep.close()

    def color_depth_histogram(self, reads, colors, n_bins=256, bin_width=1, strands=FIN_MERGED):
        """the depth histogram of a read set per reference of `colors` (a Colors of this index): a fresh Depth beside the colours, the reads searched into it,
        then Colors.depth_histogram -- a ColorDepthHistogram"""
        dep = Depth(self, colors.device)
        try:
            dep.add_reads(flatten(reads), strands)
            return colors.depth_histogram(dep, n_bins, bin_width)
        finally:
            dep.close()

    def pileup(self, max_mismatch=8, device=0):
        """a zeroed base pileup beside the replica on `device` (Pileup)"""
        return Pileup(self, device, max_mismatch)

    def unitig_depth(self, reads, strands=FIN_MERGED, min_depth=1):
        """the depth of a read set over host buffers, per unitig (fin_search_batch_unitig_depth): (DEPTH_STAT_DTYPE stats[n_unitigs], total_positive) -- each
        unitig's summed and greatest depth and how many of its positions were found at least min_depth times; only the statistics come back from the device"""
        out = np.zeros(max(self.n_unitigs, 1), dtype=DEPTH_STAT_DTYPE)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_search_batch_unitig_depth(self.h, *_reads_args(reads),
                                                    int(strands), int(min_depth), out.ctypes.data_as(C.c_void_p), C.byref(npos), err, 512), err)
        return out[: self.n_unitigs], int(npos.value)

    def search_reads_text(self, reads, strands=FIN_MERGED):
        """run_fmin_queries_streaming with its printed text as the result (fin_search_batch_text): (bytes, total_positive)"""
        t = self.L.fin_text_create()
        try:
            npos = C.c_uint64(0)
            err = C.create_string_buffer(512)
            _check(self.L.fin_search_batch_text(self.h, *_reads_args(reads), int(strands), t, C.byref(npos), err, 512), err)
            n = int(self.L.fin_text_size(t))
            return C.string_at(self.L.fin_text_data(t), n) if n else b"", int(npos.value)
        finally:
            self.L.fin_text_free(t)

    def search_reads_multi(self, reads, devices, strands=FIN_MERGED):
        """fin_search_batch_multi: the same loop with the reads sharded by record over several GPUs (index replicated)."""
        bases, offsets = flatten(reads)
        lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
        nk = int(np.maximum(lens - self.k + 1, 0).sum())
        out = np.empty((max(nk, 1), 2), dtype=np.int32)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        devs = (C.c_int * len(devices))(*devices)
        _check(self.L.fin_search_batch_multi(self.h, devs, len(devices), *_reads_args((bases, offsets)), int(strands),
                                             out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(npos), err, 512), err)
        return out[:nk], int(npos.value)

    def batch(self, reads):
        return Batch(self, reads)

    def close(self):
        if getattr(self, "h", None):
            self.L.fin_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RECORD_DTYPE = np.dtype([("u", np.uint32), ("off0", np.uint32), ("meta", np.uint32), ("nk", np.uint32), ("Es", np.uint64), ("Es2", np.uint64)])
SEGMENT_DTYPE = np.dtype([("u", np.int32), ("off", np.int32), ("slot", np.uint32), ("len", np.int32)])   # fin_segment
READ_SUMMARY_DTYPE = np.dtype([("n_found", np.uint32), ("n_segments", np.uint32), ("longest", np.uint32), ("span", np.uint32)])   # fin_read_summary
READ_CLASS_DTYPE = np.dtype([("label", np.uint32), ("n_best", np.uint32), ("n_second", np.uint32), ("n_labelled", np.uint32)])   # fin_read_class
FIN_NO_LABEL = 0xFFFFFFFF
READ_TAXON_DTYPE = np.dtype([("taxon", np.uint32), ("score", np.uint32), ("clade", np.uint32), ("n_labelled", np.uint32)])   # fin_read_taxon
READ_PSEUDO_DTYPE = np.dtype([("n_found", np.uint32), ("n_colored", np.uint32), ("n_colors", np.uint32), ("reserved", np.uint32)])   # fin_read_pseudo
PAIR_PSEUDO_DTYPE = np.dtype([("n_found", np.uint32), ("n_colored", np.uint32), ("n_colors", np.uint32), ("n_colored_first", np.uint32)])   # fin_pair_pseudo
FIN_PAIR_ANY, FIN_PAIR_BOTH = 0, 1
FRAGMENT_DTYPE = np.dtype([("u", np.uint32), ("start", np.uint32), ("length", np.uint32), ("cls", np.uint32)])   # fin_fragment
FIN_MAX_COLORS = 4096
READ_ASSIGN_DTYPE = np.dtype([("n_assigned", np.uint32), ("best", np.uint32)])   # fin_read_assign
FIN_NO_COLOR = 0xFFFFFFFF
DEPTH_STAT_DTYPE = np.dtype([("sum", np.uint64), ("max", np.uint32), ("n_at_least", np.uint32)])            # fin_depth_stat
COLOR_COVERAGE_DTYPE = np.dtype([(f, np.uint64) for f in ColorCoverage.FIELDS])   # fin_color_coverage
VARIANT_DTYPE = np.dtype([("u", np.uint32), ("off", np.uint32), ("cover", np.uint32), ("ref", np.uint32), ("alt", np.uint32, (4,))])   # fin_variant
REF_WINDOW_DTYPE = np.dtype([("depth_sum", np.uint64), ("in_graph", np.uint32), ("covered", np.uint32)])   # fin_ref_window
REF_VARIANT_DTYPE = np.dtype([("seq", np.uint32), ("pos", np.uint32), ("var", np.uint32), ("flags", np.uint32)])   # fin_ref_variant


class PartitionedBatch:
    """A read set resident on the device of a PartitionedIndex (fin_pbatch_*): run() = every part's step and its merge.  The batch holds its own
    reference on the C side's set (include/finito_amd.h: the free-order contract), not on the Python object: it stays usable after the index is
    closed or collected, until it is closed itself."""

    def __init__(self, pindex, reads):
        self.L = lib(); self.h = C.c_void_p()
        err = C.create_string_buffer(512)
        _check(self.L.fin_pbatch_create(pindex.h, *_reads_args(reads),
                                        C.byref(self.h), err, 512), err)
        self.n_kmers = int(self.L.fin_pbatch_n_kmers(self.h))

    def run(self, stream=None):
        err = C.create_string_buffer(512)
        _check(self.L.fin_pbatch_run(self.h, C.c_void_p(stream or 0), err, 512), err)

    def download(self, want_pairs=True):
        out = np.empty((max(self.n_kmers, 1), 2), dtype=np.int32) if want_pairs else None
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_pbatch_download(self.h, out.ctypes.data_as(C.c_void_p) if want_pairs else None, C.byref(npos), err, 512), err)
        return (out[: self.n_kmers] if want_pairs else None), int(npos.value)

    def step_time_ms(self, skip_first=0):
        ms = C.c_double(0); n = C.c_uint64(0)
        self.L.fin_pbatch_step_time(self.h, int(skip_first), C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def close(self):
        if self.h:
            self.L.fin_pbatch_free(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PartitionedIndex:
    """A unitig set beyond 2^32 nodes as parts of at most max_part_bases bases (fin_pindex_*; include/finito_amd.h): an ordinary index and device
    replica of each part, every read searched in every part, results those of ONE FinimizerIndex (FinimizerIndex.hh:26-259) of all the unitigs --
    for the input the reference requires, a disjoint spectrum-preserving string set (README.md:79-80), which verify=True checks on the device."""

    def __init__(self, unitigs, k, device=0, max_part_bases=0, verify=True, _load_prefix=None):
        self.L = L = lib(); self._h = C.c_void_p()
        vp, cp = C.c_void_p, C.c_char_p
        L.fin_pindex_save.argtypes = [vp, cp, cp, C.c_size_t]
        L.fin_pindex_load.argtypes = [cp, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_pindex_exists.argtypes = [cp]
        L.fin_pbatch_reload.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.c_uint64, cp, C.c_size_t]
        L.fin_pindex_build_device.argtypes = [cp, C.POINTER(C.c_uint64), C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(vp), cp, C.c_size_t]
        L.fin_pindex_free.argtypes = [vp]
        L.fin_pindex_parts.argtypes = [vp]; L.fin_pindex_parts.restype = C.c_uint32
        for f in ("k", "n_nodes", "n_kmers", "n_unitigs", "total_len", "size_in_bytes", "replica_table_bytes", "shared_kmers"):
            getattr(L, "fin_pindex_" + f).argtypes = [vp]; getattr(L, "fin_pindex_" + f).restype = C.c_int64
        L.fin_pindex_verify_seconds.argtypes = [vp]; L.fin_pindex_verify_seconds.restype = C.c_double
        L.fin_pindex_part.argtypes = [vp, C.c_uint32]; L.fin_pindex_part.restype = vp
        L.fin_pindex_unitig_ids.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
        L.fin_pindex_search_batch.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.c_uint64, vp, C.POINTER(C.c_uint64), cp, C.c_size_t]
        L.fin_pbatch_create.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(vp), cp, C.c_size_t]
        L.fin_pbatch_run.argtypes = [vp, vp, cp, C.c_size_t]
        L.fin_pbatch_n_kmers.argtypes = [vp]; L.fin_pbatch_n_kmers.restype = C.c_uint64
        L.fin_pbatch_device_pairs.argtypes = [vp]; L.fin_pbatch_device_pairs.restype = vp
        L.fin_pbatch_download.argtypes = [vp, vp, C.POINTER(C.c_uint64), cp, C.c_size_t]
        L.fin_pbatch_step_time.argtypes = [vp, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.fin_pbatch_free.argtypes = [vp]
        err = C.create_string_buffer(1024)
        self.device = int(device)
        if _load_prefix is not None:
            _check(L.fin_pindex_load(str(_load_prefix).encode(), int(device), C.byref(self._h), err, 1024), err)
            return
        _check(L.fin_pindex_build_device(*_reads_args(unitigs), int(k), int(device),
                                         int(max_part_bases), 1 if verify else 0, C.byref(self._h), err, 1024), err)

    @classmethod
    def load(cls, index_prefix, device=0):
        """fin_pindex_load: the parts written by serialize() (<prefix>.finparts, .p<i>.finamd, .p<i>.gid), their replicas uploaded to `device`"""
        return cls(None, 0, device=device, _load_prefix=index_prefix)

    @staticmethod
    def exists(index_prefix):
        lib().fin_pindex_exists.argtypes = [C.c_char_p]
        return bool(lib().fin_pindex_exists(str(index_prefix).encode()))

    def serialize(self, index_prefix):
        """fin_pindex_save (FinimizerIndex::serialize of every part + the manifest)"""
        err = C.create_string_buffer(512)
        _check(self.L.fin_pindex_save(self.h, str(index_prefix).encode(), err, 512), err)

    n_parts = property(lambda self: int(self.L.fin_pindex_parts(self.h)))
    k = property(lambda self: int(self.L.fin_pindex_k(self.h)))
    n_nodes = property(lambda self: int(self.L.fin_pindex_n_nodes(self.h)))
    n_kmers = property(lambda self: int(self.L.fin_pindex_n_kmers(self.h)))
    n_unitigs = property(lambda self: int(self.L.fin_pindex_n_unitigs(self.h)))
    total_len = property(lambda self: int(self.L.fin_pindex_total_len(self.h)))
    shared_kmers = property(lambda self: int(self.L.fin_pindex_shared_kmers(self.h)))
    verify_seconds = property(lambda self: float(self.L.fin_pindex_verify_seconds(self.h)))

    def size_in_bytes(self):
        return int(self.L.fin_pindex_size_in_bytes(self.h))

    def replica_table_bytes(self):
        return int(self.L.fin_pindex_replica_table_bytes(self.h))

    def part_nodes(self):
        """n_nodes of every part (each below 2^32)"""
        self.L.fin_index_n_nodes.argtypes = [C.c_void_p]
        return [int(self.L.fin_index_n_nodes(self.L.fin_pindex_part(self.h, p))) for p in range(self.n_parts)]

    def unitig_ids(self, part):
        """the set's number of each of the part's unitigs (permute_unitigs over the whole set, PackedStrings.hh:105-135)"""
        self.L.fin_index_n_unitigs.argtypes = [C.c_void_p]
        n = int(self.L.fin_index_n_unitigs(self.L.fin_pindex_part(self.h, part)))
        out = np.empty(n, dtype=np.uint32)
        if self.L.fin_pindex_unitig_ids(self.h, part, out.ctypes.data_as(C.c_void_p), n) != 0:
            raise FinitoError(FIN_EINVAL, "fin_pindex_unitig_ids")
        return out

    def search_reads(self, reads):
        """merged search of a read set in every part (fin_pindex_search_batch): (int32 pairs [n_kmers, 2], total_positive)"""
        bases, offsets = flatten(reads)
        k = self.k
        lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
        nk = int(np.maximum(lens - k + 1, 0).sum())
        out = np.empty((max(nk, 1), 2), dtype=np.int32)
        npos = C.c_uint64(0)
        err = C.create_string_buffer(512)
        _check(self.L.fin_pindex_search_batch(self.h, *_reads_args((bases, offsets)),
                                              out.ctypes.data_as(C.c_void_p), C.byref(npos), err, 512), err)
        return out[:nk], int(npos.value)

    def batch(self, reads):
        return PartitionedBatch(self, reads)

    @property
    def h(self):
        """the fin_pindex handle; a closed index has none, and whatever asks for it is refused here, before the C side sees a null or a dangling pointer"""
        if not self._h:
            raise FinitoError(FIN_EINVAL, "the PartitionedIndex is closed")
        return self._h

    def close(self):
        """fin_pindex_free: the owner's reference.  Batches made by batch() hold their own and stay usable until they are closed themselves"""
        if self._h:
            self.L.fin_pindex_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def expand_records(recs, stream, k, n_threads=0):
    """fin_expand_records (host): the pairs fin_search_batch delivers, from records + stream; returns (pairs, n_positive)"""
    L = lib()
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    nk = int(recs["nk"].astype(np.int64).sum())
    out = np.empty((max(nk, 1), 2), dtype=np.int32)
    pos = C.c_uint64(0)
    L.fin_expand_records.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    rc = L.fin_expand_records(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                              out.ctypes.data_as(C.c_void_p), C.byref(pos), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_expand_records: records and stream do not belong together")
    return out[:nk], int(pos.value)


def records_unitig_counts(recs, stream, k, n_unitigs, n_threads=0):
    """fin_records_unitig_counts (host): uint64 counts[n_unitigs] of the found k-mers per unitig, from records + stream, without making the pairs"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    out = np.zeros(max(int(n_unitigs), 1), dtype=np.uint64)
    rc = lib().fin_records_unitig_counts(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                         int(n_unitigs), out.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_unitig_counts: a unitig number outside [0, n_unitigs), or records and stream do not belong together")
    return out[: int(n_unitigs)]


def records_cover(recs, stream, k, ends, n_threads=0):
    """fin_records_cover (host): the coverage bitmap uint64[(ends[-1] + 63) // 64] from records + stream, without making the pairs; `ends` as export(X_ENDS)"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    ends = np.ascontiguousarray(ends, dtype=np.int64)
    n_words = (int(ends[-1]) + 63) // 64 if len(ends) else 0
    out = np.zeros(max(n_words, 1), dtype=np.uint64)
    rc = lib().fin_records_cover(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                 ends.ctypes.data_as(C.POINTER(C.c_int64)), len(ends), out.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_cover: a unitig number outside the index, a k-mer that does not lie inside its unitig, or records and stream do not belong together")
    return out[:n_words]


def records_depth(recs, stream, k, ends, n_threads=0):
    """fin_records_depth (host): the per-position depth uint32[ends[-1]] from records + stream, without making the pairs; `ends` as export(X_ENDS)"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    ends = np.ascontiguousarray(ends, dtype=np.int64)
    total_len = int(ends[-1]) if len(ends) else 0
    out = np.zeros(max(total_len, 1), dtype=np.uint32)
    rc = lib().fin_records_depth(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                 ends.ctypes.data_as(C.POINTER(C.c_int64)), len(ends), out.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_depth: a unitig number outside the index, a k-mer that does not lie inside its unitig, or records and stream do not belong together")
    return out[:total_len]


def records_pileup(recs, stream, k, reads, ends, concat, max_mismatch=8, n_threads=0):
    """fin_records_pileup (host): (cover uint32[ends[-1]], alt uint32[ends[-1], 4], counters uint64[4]) from records + stream and the reads themselves (as
    flatten takes them), every placed read compared with the text whole; `ends` as export(X_ENDS), `concat` as export(X_CONCAT)"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    ends = np.ascontiguousarray(ends, dtype=np.int64); concat = np.ascontiguousarray(concat, dtype=np.uint8)
    total_len = int(ends[-1]) if len(ends) else 0
    bases, offsets, n_reads = _reads_args(reads)
    if n_reads != len(recs) or len(concat) < total_len:
        raise FinitoError(FIN_EINVAL, "records_pileup: %d reads for %d records, or a text shorter than the unitigs' ends" % (n_reads, len(recs)))
    cover = np.zeros(max(total_len, 1), dtype=np.uint32)
    alt = np.zeros((max(total_len, 1), 4), dtype=np.uint32)
    counters = np.zeros(4, dtype=np.uint64)
    rc = lib().fin_records_pileup(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k), bases, offsets,
                                  ends.ctypes.data_as(C.POINTER(C.c_int64)), len(ends), concat.ctypes.data_as(C.c_void_p), int(max_mismatch),
                                  cover.ctypes.data_as(C.c_void_p), alt.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_pileup: a unitig number outside the index, a k-mer that does not lie inside its unitig, records and stream or reads that do "
                              "not belong together, or max_mismatch above 255")
    return cover[:total_len], alt[:total_len], counters


def expand_segments(seg_offs, segs, nk_per_read, n_threads=0):
    """fin_expand_segments (host): the pairs fin_search_batch delivers, from segments; nk_per_read[r] = max(0, length of read r - k + 1); returns (pairs, n_positive)"""
    seg_offs = np.ascontiguousarray(seg_offs, dtype=np.uint64); segs = np.ascontiguousarray(segs, dtype=SEGMENT_DTYPE)
    nks = np.ascontiguousarray(nk_per_read, dtype=np.uint32)
    if len(seg_offs) != len(nks) + 1 or (len(seg_offs) and int(seg_offs[-1]) > len(segs)):
        raise FinitoError(FIN_EINVAL, "expand_segments: seg_offs does not fit the reads or the segments")
    nk = int(nks.astype(np.int64).sum())
    out = np.empty((max(nk, 1), 2), dtype=np.int32)
    pos = C.c_uint64(0)
    rc = lib().fin_expand_segments(seg_offs.ctypes.data_as(C.POINTER(C.c_uint64)), segs.ctypes.data_as(C.c_void_p), len(nks), nks.ctypes.data_as(C.c_void_p),
                                   out.ctypes.data_as(C.c_void_p), C.byref(pos), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_expand_segments: a segment outside its read, overlapping or unsorted segments, a segment of length 0 or with a negative offset")
    return out[:nk], int(pos.value)


def records_segments(recs, stream, k, seg_cap=None, n_threads=0):
    """fin_records_segments (host): the canonical segments (seg_offs, segs) from records + stream, without making the pairs; seg_cap: room for that many
    segments (default: the record set's number of k-mers, which always suffices)"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    cap = int(recs["nk"].astype(np.int64).sum()) if seg_cap is None else int(seg_cap)
    seg_offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    segs = np.zeros(max(cap, 1), dtype=SEGMENT_DTYPE)
    n = C.c_uint64(0)
    rc = lib().fin_records_segments(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                    seg_offs.ctypes.data_as(C.POINTER(C.c_uint64)), segs.ctypes.data_as(C.c_void_p), cap, C.byref(n), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_segments: %s" % ("room for %d segments, %d needed" % (cap, n.value) if rc == FIN_ELIMIT else
                                                            "records and stream do not belong together, or a pair that is neither found nor (-1,-1)"))
    return seg_offs, segs[: int(n.value)].copy()


def records_read_summaries(recs, stream, k, n_threads=0):
    """fin_records_read_summaries (host): READ_SUMMARY_DTYPE[n_reads] from records + stream, without making the pairs"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    out = np.zeros(max(len(recs), 1), dtype=READ_SUMMARY_DTYPE)
    rc = lib().fin_records_read_summaries(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                          out.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_read_summaries: records and stream do not belong together, or a pair that is neither found nor (-1,-1)")
    return out[: len(recs)]


def records_read_classes(recs, stream, k, unitig_labels, n_threads=0):
    """fin_records_read_classes (host): READ_CLASS_DTYPE[n_reads] from records + stream under unitig_labels (uint32 per unitig), without making the pairs"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    lab = np.ascontiguousarray(unitig_labels, dtype=np.uint32)
    out = np.zeros(max(len(recs), 1), dtype=READ_CLASS_DTYPE)
    rc = lib().fin_records_read_classes(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                        lab.ctypes.data_as(C.c_void_p), len(lab), out.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_read_classes: a unitig number outside the labelling, records and stream that do not belong together, or a pair that is "
                              "neither found nor (-1,-1)")
    return out[: len(recs)]


def unitig_lca_labels(bits, n_colors, parent, color_taxon, n_threads=0):
    """fin_unitig_lca_labels (host): uint32 label[n_unitigs] from the colour matrix bits[n_unitigs, W] -- the LCA of the taxa of each row's colours, FIN_NO_LABEL
    for an empty row -- the CPU statement of Colors.taxonomy"""
    W = (int(n_colors) + 63) // 64 if 0 < int(n_colors) <= FIN_MAX_COLORS else 1
    b = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, W)
    p = _taxa_parent("unitig_lca_labels", parent)
    ct = np.ascontiguousarray(color_taxon, dtype=np.uint32)
    if len(ct) != int(n_colors):
        raise FinitoError(FIN_EINVAL, "unitig_lca_labels: one taxon per colour")
    out = np.zeros(max(len(b), 1), dtype=np.uint32)
    rc = lib().fin_unitig_lca_labels(b.ctypes.data_as(C.POINTER(C.c_uint64)), len(b), int(n_colors), p.ctypes.data_as(C.c_void_p), len(p),
                                     ct.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_unitig_lca_labels: a parent that breaks the topological numbering, a colour's taxon outside the tree, a bit at or above "
                              "n_colors, or n_colors outside 1 .. 4096")
    return out[: len(b)]


def records_read_taxa(recs, stream, k, unitig_labels, parent, min_found=1, confidence=0, n_threads=0):
    """fin_records_read_taxa (host): READ_TAXON_DTYPE[n_reads] from records + stream under unitig_labels and the tree `parent`, written from the definitions -- the
    CPU statement of Batch.taxa"""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); stream = np.ascontiguousarray(stream, dtype=np.int32)
    lab = np.ascontiguousarray(unitig_labels, dtype=np.uint32)
    p = _taxa_parent("records_read_taxa", parent)
    t = _taxa_thresholds("records_read_taxa", min_found, confidence)
    out = np.zeros(max(len(recs), 1), dtype=READ_TAXON_DTYPE)
    rc = lib().fin_records_read_taxa(recs.ctypes.data_as(C.c_void_p), len(recs), stream.ctypes.data_as(C.c_void_p), len(stream.reshape(-1, 2)), int(k),
                                     lab.ctypes.data_as(C.c_void_p), len(lab), p.ctypes.data_as(C.c_void_p), len(p), *t, out.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_read_taxa: a bad taxonomy, label or confidence, a unitig number outside the labelling, records and stream that do not "
                              "belong together, or a pair that is neither found nor (-1,-1)")
    return out[: len(recs)]


def taxa_clade_reads(direct, parent):
    """fin_taxa_clade_reads (host): uint64 clade[n_taxa] -- direct[t] summed over every taxon's subtree -- the CPU statement of Taxonomy.download's roll-up"""
    p = _taxa_parent("taxa_clade_reads", parent)
    d = np.ascontiguousarray(direct, dtype=np.uint64)
    if len(d) < len(p):
        raise FinitoError(FIN_EINVAL, "taxa_clade_reads: one count per taxon")
    out = np.zeros(len(p), dtype=np.uint64)
    rc = lib().fin_taxa_clade_reads(d.ctypes.data_as(C.POINTER(C.c_uint64)), p.ctypes.data_as(C.c_void_p), len(p), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise FinitoError(rc, "fin_taxa_clade_reads: a parent that breaks the topological numbering")
    return out


def taxonomy_order(ids, parent_ids):
    """arbitrary integer taxon ids (NCBI nodes.dmp's first two columns, say) into the topological numbering a Taxonomy takes: (order, parent) with order[i] = the
    new number of ids[i] and parent uint32[n] in the new numbers -- the root is 0 and its own parent, every other parent is below its child.  The root is the one
    node that is its own parent.  Children are numbered breadth-first, siblings in input order.  ValueError for a repeated id, an unknown parent, no root or more
    than one, and a cycle (nodes the root does not reach)"""
    ids = [int(x) for x in ids]
    pids = [int(x) for x in parent_ids]
    if len(ids) != len(pids) or not ids:
        raise ValueError("taxonomy_order: one parent id per id, at least one")
    at = {}
    for i, x in enumerate(ids):
        if x in at:
            raise ValueError("taxonomy_order: id %d is given twice (entries %d and %d)" % (x, at[x], i))
        at[x] = i
    kids = [[] for _ in ids]
    roots = []
    for i, (x, p) in enumerate(zip(ids, pids)):
        if p == x:
            roots.append(i)
        elif p not in at:
            raise ValueError("taxonomy_order: entry %d: id %d has the unknown parent %d" % (i, x, p))
        else:
            kids[at[p]].append(i)
    if len(roots) != 1:
        raise ValueError("taxonomy_order: %s" % ("no root (a node that is its own parent)" if not roots else
                                                 "more than one root: ids %d and %d are their own parents" % (ids[roots[0]], ids[roots[1]])))
    order = np.full(len(ids), -1, dtype=np.int64)
    parent = np.zeros(len(ids), dtype=np.uint32)
    queue = [roots[0]]
    order[roots[0]] = 0
    n = 1
    for i in queue:   # (grows while it is walked)
        for c in kids[i]:
            order[c] = n
            parent[n] = order[i]
            n += 1
            queue.append(c)
    if n != len(ids):
        bad = int(np.flatnonzero(order < 0)[0])
        raise ValueError("taxonomy_order: a cycle: id %d (entry %d) never reaches the root" % (ids[bad], bad))
    return order, parent


def records_pseudoalign(recs, stream, k, bits, n_colors, permille=1000, n_threads=0):
    """host: (rows uint64[n_reads, W], heads READ_PSEUDO_DTYPE[n_reads]) from records + stream under the colour matrix bits[n_unitigs, W]
    (fin_records_pseudoalign) -- the CPU statement of Batch.pseudoalign"""
    r = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    st = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1, 2)
    W = (int(n_colors) + 63) // 64 if 0 <= int(n_colors) <= 0xFFFFFFFF else 0
    b = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, max(W, 1))
    if not (0 <= int(n_colors) <= 0xFFFFFFFF and 0 <= int(permille) <= 0xFFFFFFFF):
        raise FinitoError(FIN_EINVAL, "records_pseudoalign: n_colors and permille are unsigned 32-bit numbers")
    rows = np.zeros((max(len(r), 1), max(W, 1)), dtype=np.uint64)
    heads = np.zeros(max(len(r), 1), dtype=READ_PSEUDO_DTYPE)
    rc = lib().fin_records_pseudoalign(r.ctypes.data_as(C.c_void_p), len(r), st.ctypes.data_as(C.c_void_p), len(st), int(k), b.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       len(b), int(n_colors), int(permille), rows.ctypes.data_as(C.POINTER(C.c_uint64)), heads.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_pseudoalign: n_colors outside 1 .. 4096, permille above 1000, a bit at or above n_colors, a unitig number outside the "
                              "matrix, or records and stream that do not belong together")
    return rows[: len(r)], heads[: len(r)]


def records_pseudoalign_pairs(recs, stream, k, bits, n_colors, permille=1000, both=False, n_threads=0, mode=None):
    """host: (rows uint64[F, W], heads PAIR_PSEUDO_DTYPE[F]) from the records + stream of interleaved mates (fin_records_pseudoalign_paired) -- the CPU statement
    of Batch.pseudoalign_pairs.  mode (FIN_PAIR_ANY / FIN_PAIR_BOTH) overrides `both`"""
    r = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    st = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1, 2)
    W = (int(n_colors) + 63) // 64 if 0 <= int(n_colors) <= 0xFFFFFFFF else 0
    b = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, max(W, 1))
    m = (FIN_PAIR_BOTH if both else FIN_PAIR_ANY) if mode is None else int(mode)
    if not (0 <= int(n_colors) <= 0xFFFFFFFF and 0 <= int(permille) <= 0xFFFFFFFF and 0 <= m <= 0xFFFFFFFF):
        raise FinitoError(FIN_EINVAL, "records_pseudoalign_pairs: n_colors, permille and mode are unsigned 32-bit numbers")
    nf = len(r) // 2
    rows = np.zeros((max(nf, 1), max(W, 1)), dtype=np.uint64)
    heads = np.zeros(max(nf, 1), dtype=PAIR_PSEUDO_DTYPE)
    rc = lib().fin_records_pseudoalign_paired(r.ctypes.data_as(C.c_void_p), len(r), st.ctypes.data_as(C.c_void_p), len(st), int(k), b.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              len(b), int(n_colors), int(permille), m, rows.ctypes.data_as(C.POINTER(C.c_uint64)), heads.ctypes.data_as(C.c_void_p),
                                              int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_pseudoalign_paired: an odd number of reads, a mode that is neither FIN_PAIR_ANY nor FIN_PAIR_BOTH, n_colors outside 1 .. 4096, "
                              "permille above 1000, a bit at or above n_colors, a unitig number outside the matrix, or records and stream that do not belong together")
    return rows[:nf], heads[:nf]


def records_fragments(recs, stream, k, ends, n_bins=1024, bin_width=1, n_threads=0):
    """host: (frags FRAGMENT_DTYPE[F], hist uint64[n_bins], counters uint64[7]) from the records + stream of interleaved mates (fin_records_fragments) -- the CPU
    statement of Batch.fragments and Fragments, read off every read's expanded slots"""
    r = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    st = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1, 2)
    e = np.ascontiguousarray(ends, dtype=np.int64)
    if not (0 <= int(n_bins) <= 0xFFFFFFFF and 0 <= int(bin_width) <= 0xFFFFFFFF):
        raise FinitoError(FIN_EINVAL, "records_fragments: n_bins and bin_width are unsigned 32-bit numbers")
    nf = len(r) // 2
    frags = np.zeros(max(nf, 1), dtype=FRAGMENT_DTYPE)
    hist = np.zeros(max(min(int(n_bins), FIN_FRAG_MAX_BINS), 1), dtype=np.uint64)
    counters = np.zeros(7, dtype=np.uint64)
    rc = lib().fin_records_fragments(r.ctypes.data_as(C.c_void_p), len(r), st.ctypes.data_as(C.c_void_p), len(st), int(k), e.ctypes.data_as(C.POINTER(C.c_int64)), len(e),
                                     int(n_bins), int(bin_width), frags.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p),
                                     int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_fragments: an odd number of reads, n_bins outside 1 .. %d, bin_width 0, a unitig number outside the index, a k-mer that does "
                              "not lie inside its unitig, or records and stream that do not belong together" % FIN_FRAG_MAX_BINS)
    return frags[:nf], hist, counters


def records_links(recs, stream, k, ends, min_count=1, n_threads=0):
    """host: the LinkTable of records + stream (fin_records_links) -- the CPU statement of Links, read off every read's expanded slots"""
    r = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    st = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1, 2)
    e = np.ascontiguousarray(ends, dtype=np.int64).reshape(-1)
    mc = int(min_count)
    if not 0 <= mc < (1 << 64):
        raise FinitoError(FIN_EINVAL, "records_links: min_count is an unsigned 64-bit number")
    n = C.c_uint64(0)
    counters = np.zeros(4, dtype=np.uint64)
    args = (r.ctypes.data_as(C.c_void_p), len(r), st.ctypes.data_as(C.c_void_p), len(st), int(k), e.ctypes.data_as(C.POINTER(C.c_int64)), len(e), mc)
    rc = lib().fin_records_links(*args, None, 0, C.byref(n), None, int(n_threads))
    links = np.zeros(max(int(n.value), 1), dtype=LINK_DTYPE)
    if rc == 0:
        rc = lib().fin_records_links(*args, links.ctypes.data_as(C.c_void_p), len(links), C.byref(n), counters.ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_records_links: a transition with an end outside the index, a record kind above 2, unitig ends that descend or reach 2^32, or "
                              "records and stream that do not belong together")
    return LinkTable(links[: int(n.value)], counters[0], counters[1], counters[3])


def _twin_ends(ends):
    e = np.ascontiguousarray(ends, dtype=np.int64).reshape(-1)
    return e, e.ctypes.data_as(C.POINTER(C.c_int64)), len(e)


def segments_check(seq_nk, seg_offs, segs, k, ends):
    """host: FinitoError FIN_EINVAL naming the first segment of a path set that is not valid, and the clause (fin_segments_check)"""
    nk, so, sg = _path_set("segments_check", seq_nk, seg_offs, segs)
    e, ep, ne = _twin_ends(ends)
    err = C.create_string_buffer(512)
    _check(lib().fin_segments_check(nk.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), len(nk), int(k), ep, ne, err, 512), err)


def segments_window_depth(seq_nk, seg_offs, segs, k, ends, depth, window=1000, min_depth=1, n_threads=0, cap=None):
    """host: RefDepth of a path set over depth uint32[total_len] (fin_segments_window_depth) -- the CPU statement of RefPaths.depth_windows.  cap: room for so many
    windows, FinitoError FIN_ELIMIT beyond (its n_windows attribute the true count); None: as many as there are"""
    nk, so, sg = _path_set("segments_window_depth", seq_nk, seg_offs, segs)
    e, ep, ne = _twin_ends(ends)
    d = np.ascontiguousarray(depth, dtype=np.uint32).reshape(-1)
    w, md = _window_args("segments_window_depth", window, min_depth)
    room = int(sum(-(-int(x) // w) for x in nk)) if cap is None else int(cap)
    wo = np.zeros(len(nk) + 1, dtype=np.uint64)
    out = np.zeros(max(room, 1), dtype=REF_WINDOW_DTYPE)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = lib().fin_segments_window_depth(nk.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), len(nk), int(k), ep, ne,
                                         d.ctypes.data_as(C.c_void_p), w, md, wo.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), room, C.byref(n),
                                         int(n_threads), err, 512)
    if rc != 0:
        ex = FinitoError(rc, "fin_segments_window_depth: " + err.value.decode())
        ex.n_windows = int(n.value)
        raise ex
    return RefDepth(wo, out[: int(n.value)], w, md)


def segments_lift_variants(seq_nk, seg_offs, segs, k, ends, variants, n_threads=0, cap=None):
    """host: REF_VARIANT_DTYPE[n] of a path set and Pileup.call's candidates (fin_segments_lift_variants) -- the CPU statement of RefPaths.lift_variants.  cap: room
    for so many records, FinitoError FIN_ELIMIT beyond (its n_out attribute the true count); None: as many as there are"""
    nk, so, sg = _path_set("segments_lift_variants", seq_nk, seg_offs, segs)
    e, ep, ne = _twin_ends(ends)
    v = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE).reshape(-1)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    room = 1024 if cap is None else int(cap)
    while True:
        out = np.zeros(max(room, 1), dtype=REF_VARIANT_DTYPE)
        rc = lib().fin_segments_lift_variants(nk.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), len(nk), int(k), ep, ne,
                                              v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p), room, C.byref(n), int(n_threads), err, 512)
        if rc == FIN_ELIMIT and cap is None and int(n.value) > room:
            room = int(n.value)
            continue
        if rc != 0:
            ex = FinitoError(rc, "fin_segments_lift_variants: " + err.value.decode())
            ex.n_out = int(n.value)
            raise ex
        return out[: int(n.value)]


def rows_eqclasses(rows, n_colors):
    """host: (class rows uint64[n, W], reads uint64[n], n_unaligned) of rows uint64[n_rows, W] in canonical order (fin_rows_eqclasses) -- the CPU statement of
    EqClasses"""
    if not 1 <= int(n_colors) <= 4096:
        raise FinitoError(FIN_ELIMIT, "rows_eqclasses: n_colors is 1 .. 4096")
    W = max((int(n_colors) + 63) // 64, 1)
    a = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, W)
    u64p = C.POINTER(C.c_uint64)
    cap = max(len(a), 1)
    out = np.zeros((cap, W), dtype=np.uint64)
    reads = np.zeros(cap, dtype=np.uint64)
    n, un = C.c_uint64(0), C.c_uint64(0)
    rc = lib().fin_rows_eqclasses(a.ctypes.data_as(u64p), len(a), int(n_colors), out.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), cap, C.byref(n), C.byref(un))
    if rc != 0:
        raise FinitoError(rc, "fin_rows_eqclasses: n_colors outside 1 .. 4096, or a row with a bit at or above n_colors")
    return out[: int(n.value)], reads[: int(n.value)], int(un.value)


def rows_assign(rows, n_colors, weights, thresholds=0.5, n_threads=0):
    """host: (assigned rows uint64[n, W], heads READ_ASSIGN_DTYPE[n], assigned uint64[n_colors], sole uint64[n_colors], counters uint64[4]) of rows
    uint64[n, W] under weights and thresholds (fin_rows_assign) -- the CPU statement of Assign, in its order; the result does not depend on n_threads"""
    w, t = _assign_args("rows_assign", n_colors, weights, thresholds)
    nc = int(n_colors)
    W = (nc + 63) // 64
    a = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, W)
    n = len(a)
    out = np.zeros((max(n, 1), W), dtype=np.uint64)
    heads = np.zeros(max(n, 1), dtype=READ_ASSIGN_DTYPE)
    assigned, sole, counters = np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    rc = lib().fin_rows_assign(a.ctypes.data_as(u64p), n, nc, w.ctypes.data_as(f64p), t.ctypes.data_as(f64p), out.ctypes.data_as(u64p), heads.ctypes.data_as(C.c_void_p),
                               assigned.ctypes.data_as(u64p), sole.ctypes.data_as(u64p), counters.ctypes.data_as(u64p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_rows_assign: a row with a bit at or above n_colors")
    return out[:n], heads[:n], assigned, sole, counters


def unitig_color_coverage(bits, n_colors, nk, covered=None, stats=None, n_threads=0):
    """host: the ColorCoverage of a colour matrix uint64[n_unitigs, W] over per-unitig numbers -- nk uint64[n_unitigs], covered uint64[n_unitigs] or None,
    stats DEPTH_STAT_DTYPE[n_unitigs] or None (fin_unitig_color_coverage) -- the CPU statement of Colors.coverage; the result does not depend on n_threads"""
    nc = int(n_colors)
    if not 1 <= nc <= FIN_MAX_COLORS:
        raise FinitoError(FIN_ELIMIT, "unitig_color_coverage: n_colors is 1 .. 4096")
    W = (nc + 63) // 64
    a = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, W)
    n = len(a)
    u64p = C.POINTER(C.c_uint64)

    def per_unitig(what, v, dtype):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=dtype)
        if v.shape != (n,):
            raise FinitoError(FIN_EINVAL, "unitig_color_coverage: %s has shape %s, the matrix has %d unitigs" % (what, v.shape, n))
        return v
    nk_, cov_, st_ = per_unitig("nk", nk, np.uint64), per_unitig("covered", covered, np.uint64), per_unitig("stats", stats, DEPTH_STAT_DTYPE)
    if nk_ is None:
        raise FinitoError(FIN_EINVAL, "unitig_color_coverage: nk is needed")
    out = np.zeros(nc + 1, dtype=COLOR_COVERAGE_DTYPE)
    rc = lib().fin_unitig_color_coverage(a.ctypes.data_as(u64p), n, nc, nk_.ctypes.data_as(u64p), cov_.ctypes.data_as(u64p) if cov_ is not None else None,
                                         st_.ctypes.data_as(C.c_void_p) if st_ is not None else None, out.ctypes.data_as(C.c_void_p),
                                         out[nc:].ctypes.data_as(C.c_void_p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_unitig_color_coverage: a row with a bit at or above n_colors")
    return ColorCoverage(out[:nc], out[nc])


def unitig_color_shared(bits, n_colors, v, n_threads=0):
    """host: the ColorShared of a colour matrix uint64[n_unitigs, W] under the weights v uint64[n_unitigs] (fin_unitig_color_shared) -- the CPU statement of
    Colors.shared; sums are mod 2^64 and the result does not depend on n_threads"""
    nc = int(n_colors)
    if not 1 <= nc <= FIN_MAX_COLORS:
        raise FinitoError(FIN_ELIMIT, "unitig_color_shared: n_colors is 1 .. 4096")
    W = (nc + 63) // 64
    a = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, W)
    n = len(a)
    if v is None:
        raise FinitoError(FIN_EINVAL, "unitig_color_shared: v is needed")
    v_ = np.ascontiguousarray(v, dtype=np.uint64)
    if v_.shape != (n,):
        raise FinitoError(FIN_EINVAL, "unitig_color_shared: v has shape %s, the matrix has %d unitigs" % (v_.shape, n))
    out = np.zeros((nc, nc), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    rc = lib().fin_unitig_color_shared(a.ctypes.data_as(u64p), n, nc, v_.ctypes.data_as(u64p), out.ctypes.data_as(u64p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_unitig_color_shared: a row with a bit at or above n_colors")
    return ColorShared(out)


def _hist_inputs(what, depth, ends, k):
    e = np.ascontiguousarray(ends, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(depth, dtype=np.uint32).reshape(-1)
    total = int(e[-1]) if len(e) else 0
    if len(d) < total:
        raise FinitoError(FIN_EINVAL, "%s: depth has %d entries, the unitigs end at %d" % (what, len(d), total))
    if len(d) == 0:
        d = np.zeros(1, dtype=np.uint32)
    if int(k) < 1:
        raise FinitoError(FIN_EINVAL, "%s: k is at least 1" % what)
    if len(e) and (e[0] < 0 or (np.diff(e) < 0).any()):
        raise FinitoError(FIN_EINVAL, "%s: the unitig ends decrease" % what)
    return d, e


def depth_positions_histogram(depth, ends, k, n_bins=256, bin_width=1, n_threads=0):
    """host: the k-mer spectrum uint64[n_bins] of per-position depths uint32[total_len] over unitigs ending at ends (X_ENDS) -- the CPU statement of
    Depth.histogram (fin_depth_positions_histogram); the result does not depend on n_threads"""
    nb, bw = _hist_args("depth_positions_histogram", n_bins, bin_width)
    d, e = _hist_inputs("depth_positions_histogram", depth, ends, k)
    out = np.zeros(nb, dtype=np.uint64)
    vp = C.c_void_p
    rc = lib().fin_depth_positions_histogram(d.ctypes.data_as(vp), e.ctypes.data_as(vp) if len(e) else None, len(e), int(k), nb, bw, out.ctypes.data_as(vp), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_depth_positions_histogram: refused with code %d" % rc)   # (every refusal it has is caught above)
    return out


def unitig_color_depth_histogram(depth, ends, k, bits, n_colors, n_bins=256, bin_width=1, n_threads=0):
    """host: the ColorDepthHistogram of per-position depths under a colour matrix uint64[n_unitigs, W] -- the CPU statement of Colors.depth_histogram
    (fin_unitig_color_depth_histogram); the result does not depend on n_threads"""
    nc = int(n_colors)
    if not 1 <= nc <= FIN_MAX_COLORS:
        raise FinitoError(FIN_ELIMIT, "unitig_color_depth_histogram: n_colors is 1 .. 4096")
    nb, bw = _hist_args("unitig_color_depth_histogram", n_bins, bin_width)
    d, e = _hist_inputs("unitig_color_depth_histogram", depth, ends, k)
    W = (nc + 63) // 64
    a = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, W)
    if len(a) != len(e):
        raise FinitoError(FIN_EINVAL, "unitig_color_depth_histogram: the matrix has %d rows, there are %d unitigs" % (len(a), len(e)))
    out = np.zeros((nc * 2 + 1, nb), dtype=np.uint64)
    vp = C.c_void_p
    rc = lib().fin_unitig_color_depth_histogram(d.ctypes.data_as(vp), e.ctypes.data_as(vp) if len(e) else None, len(e), int(k), a.ctypes.data_as(vp) if len(e) else None,
                                                nc, nb, bw, out.ctypes.data_as(vp), out[nc * 2:].ctypes.data_as(vp), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_unitig_color_depth_histogram: a row with a bit at or above n_colors")   # (the other refusals are caught above)
    return ColorDepthHistogram(out[: nc * 2].reshape(nc, 2, nb), out[nc * 2], bw)


def unitig_color_sets(bits, n_colors, n_threads=0):
    """host: (set_of uint32[n_unitigs], sets uint64[n_sets + 1, W]) of a colour matrix uint64[n_unitigs, W] in CANONICAL form (fin_unitig_color_sets) -- the CPU
    statement of Colors.compact: sets[0] empty, sets[1:] = np.unique(axis=0) of the non-empty rows, sets[set_of] == bits"""
    nc = int(n_colors)
    if not 1 <= nc <= FIN_MAX_COLORS:
        raise FinitoError(FIN_ELIMIT, "unitig_color_sets: n_colors is 1 .. 4096")
    W = (nc + 63) // 64
    a = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, W)
    n = len(a)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    if n >= 1 << 31:
        raise FinitoError(FIN_ELIMIT, "unitig_color_sets: more than 2^31-1 unitigs")
    got = C.c_uint64(0)
    src = a if n else np.zeros((1, W), dtype=np.uint64)
    set_of = np.zeros(max(n, 1), dtype=np.uint32)
    sets = np.zeros((n + 1, W), dtype=np.uint64)     # room for every row being a set of its own: one call
    rc = lib().fin_unitig_color_sets(src.ctypes.data_as(u64p), n, nc, set_of.ctypes.data_as(u32p), sets.ctypes.data_as(u64p), n + 1, C.byref(got), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_unitig_color_sets: a row with a bit at or above n_colors")
    return set_of[:n], sets[: int(got.value) + 1].copy()


def color_sets_expand(set_of, sets, n_colors=None, n_threads=0):
    """host: the dense matrix uint64[n_unitigs, W] back from (set_of, sets) (fin_color_sets_expand).  n_colors None: all 64 W bits of a row may be used"""
    a = np.ascontiguousarray(sets, dtype=np.uint64)
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= 64:
        raise FinitoError(FIN_EINVAL, "color_sets_expand: sets has shape (n_sets + 1, W), W in 1 .. 64")
    W = a.shape[1]
    nc = 64 * W if n_colors is None else int(n_colors)
    if not 1 <= nc <= FIN_MAX_COLORS or (nc + 63) // 64 != W:
        raise FinitoError(FIN_ELIMIT, "color_sets_expand: n_colors does not go with W = %d" % W)
    so = np.ascontiguousarray(set_of, dtype=np.uint32).reshape(-1)
    n = len(so)
    out = np.zeros((max(n, 1), W), dtype=np.uint64)
    src = so if n else np.zeros(1, dtype=np.uint32)
    rc = lib().fin_color_sets_expand(src.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint64)), n, a.shape[0] - 1, nc,
                                     out.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_color_sets_expand: a set id above n_sets, a non-empty set 0 or a bit at or above n_colors")
    return out[:n]


def _u64(what, name, v):
    if not 0 <= int(v) <= 0xFFFFFFFFFFFFFFFF:
        raise FinitoError(FIN_EINVAL, "%s: %s is an unsigned 64-bit number" % (what, name))
    return int(v)


def classes_merge(rows_a, reads_a, rows_b, reads_b, n_colors):
    """host: (class rows uint64[n, W], reads uint64[n]) of the union of two class lists, in canonical order (fin_classes_merge) -- the CPU statement of
    EqClasses.merge and add_classes.  Either list may be unsorted and hold duplicate rows; classes of 0 reads and all-zero rows are dropped"""
    if not 1 <= int(n_colors) <= 4096:
        raise FinitoError(FIN_ELIMIT, "classes_merge: n_colors is 1 .. 4096")
    a, ra = _classes("classes_merge", rows_a, reads_a, n_colors)
    b, rb = _classes("classes_merge", rows_b, reads_b, n_colors)
    u64p = C.POINTER(C.c_uint64)
    cap = max(len(a) + len(b), 1)
    out = np.zeros((cap, a.shape[1]), dtype=np.uint64)
    reads = np.zeros(cap, dtype=np.uint64)
    n = C.c_uint64(0)
    rc = lib().fin_classes_merge(a.ctypes.data_as(u64p), ra.ctypes.data_as(u64p), len(a), b.ctypes.data_as(u64p), rb.ctypes.data_as(u64p), len(b), int(n_colors),
                                 out.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), cap, C.byref(n))
    if rc != 0:
        raise FinitoError(rc, "fin_classes_merge: n_colors outside 1 .. 4096, or a class with a bit at or above n_colors")
    return out[: int(n.value)], reads[: int(n.value)]


def classes_abundance(class_rows, class_reads, n_colors, lengths=None, max_iters=1000, tol=1e-6, trace=False, n_threads=0):
    """host: the estimate of EqClasses.abundance from classes {row, reads} in the order given: an Abundance with n_unaligned = 0 (fin_classes_abundance)"""
    lens, mi, tol = _abundance_args("classes_abundance", n_colors, lengths, max_iters, tol)
    W = (int(n_colors) + 63) // 64
    a = np.ascontiguousarray(class_rows, dtype=np.uint64).reshape(-1, W)
    r = np.ascontiguousarray(class_reads, dtype=np.uint64).reshape(-1)
    if len(a) != len(r):
        raise FinitoError(FIN_EINVAL, "classes_abundance: %d rows and %d counts" % (len(a), len(r)))
    alpha = np.zeros(int(n_colors), dtype=np.float64)
    tr = _abundance_trace("classes_abundance", trace, mi)
    info = AbundanceInfo()
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    rc = lib().fin_classes_abundance(a.ctypes.data_as(u64p), r.ctypes.data_as(u64p), len(a), int(n_colors), lens.ctypes.data_as(f64p) if lens is not None else None, mi, tol,
                                     alpha.ctypes.data_as(f64p), tr.ctypes.data_as(f64p) if tr is not None else None, C.byref(info), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_classes_abundance: more than 2^26 classes" if rc == FIN_ELIMIT else
                          "fin_classes_abundance: a class with a bit at or above n_colors, an empty row or a class of 0 reads")
    return Abundance(alpha, lens, info, tr)


def _classes(what, class_rows, class_reads, n_colors):
    W = (int(n_colors) + 63) // 64
    a = np.ascontiguousarray(class_rows, dtype=np.uint64).reshape(-1, W)
    r = np.ascontiguousarray(class_reads, dtype=np.uint64).reshape(-1)
    if len(a) != len(r):
        raise FinitoError(FIN_EINVAL, "%s: %d rows and %d counts" % (what, len(a), len(r)))
    return a, r


def classes_resample(class_rows, class_reads, n_colors, seed=0, b=0, n_threads=0):
    """host: the class counts uint64[n] of bootstrap replicate b under `seed`, for classes {row, reads} in the order given -- the order does not matter
    (fin_classes_resample)"""
    if not 1 <= int(n_colors) <= 4096:
        raise FinitoError(FIN_ELIMIT, "classes_resample: n_colors is 1 .. 4096")
    _, seed = _bootstrap_args("classes_resample", 1, seed)
    if not 0 <= int(b) < 4096:
        raise FinitoError(FIN_ELIMIT, "classes_resample: b is 0 .. 4095")
    a, r = _classes("classes_resample", class_rows, class_reads, n_colors)
    out = np.zeros(len(a), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    rc = lib().fin_classes_resample(a.ctypes.data_as(u64p), r.ctypes.data_as(u64p), len(a), int(n_colors), seed, int(b), out.ctypes.data_as(u64p), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_classes_resample: more than 2^26 classes, or a class of 2^40 reads or more")
    return out


def classes_bootstrap(class_rows, class_reads, n_colors, n_boot, seed=0, lengths=None, max_iters=1000, tol=1e-6, n_threads=0):
    """host: EqClasses.bootstrap from classes {row, reads} in the order given: a Bootstrap whose replicates are classes_abundance over their non-zero classes
    (fin_classes_bootstrap)"""
    lens, mi, tol = _abundance_args("classes_bootstrap", n_colors, lengths, max_iters, tol)
    nb, seed = _bootstrap_args("classes_bootstrap", n_boot, seed)
    a, r = _classes("classes_bootstrap", class_rows, class_reads, n_colors)
    out = _BootOut(nb, int(n_colors))
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    rc = lib().fin_classes_bootstrap(a.ctypes.data_as(u64p), r.ctypes.data_as(u64p), len(a), int(n_colors), lens.ctypes.data_as(f64p) if lens is not None else None, mi, tol,
                                     nb, seed, *out.args(), int(n_threads))
    if rc != 0:
        raise FinitoError(rc, "fin_classes_bootstrap: more than 2^26 classes, or N x n_boot above 2^38" if rc == FIN_ELIMIT else
                          "fin_classes_bootstrap: a class with a bit at or above n_colors, an empty row or a class of 0 reads")
    return out.result(lens, seed)


def eqclasses_color_tally(class_rows, class_reads, n_colors):
    """host: (reads_with uint64[n_colors], reads_only uint64[n_colors]) of classes {row, reads} (fin_eqclasses_color_tally)"""
    if not 1 <= int(n_colors) <= 4096:
        raise FinitoError(FIN_ELIMIT, "eqclasses_color_tally: n_colors is 1 .. 4096")
    W = max((int(n_colors) + 63) // 64, 1)
    a = np.ascontiguousarray(class_rows, dtype=np.uint64).reshape(-1, W)
    r = np.ascontiguousarray(class_reads, dtype=np.uint64).reshape(-1)
    if len(a) != len(r):
        raise FinitoError(FIN_EINVAL, "eqclasses_color_tally: %d rows and %d counts" % (len(a), len(r)))
    u64p = C.POINTER(C.c_uint64)
    w = np.zeros(max(int(n_colors), 1), dtype=np.uint64)
    o = np.zeros(max(int(n_colors), 1), dtype=np.uint64)
    rc = lib().fin_eqclasses_color_tally(a.ctypes.data_as(u64p), r.ctypes.data_as(u64p), len(a), int(n_colors), w.ctypes.data_as(u64p), o.ctypes.data_as(u64p))
    if rc != 0:
        raise FinitoError(rc, "fin_eqclasses_color_tally: n_colors outside 1 .. 4096, or a class with a bit at or above n_colors")
    return w[: int(n_colors)], o[: int(n_colors)]


def format_pairs(pairs):
    """The reference's output line for one read: '(u,p) (u,p) ...\\n' (search_fmin.hh:62-65)."""
    p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    buf = C.create_string_buffer(24 * len(p) + 2)
    n = lib().fin_format_pairs(p.ctypes.data_as(C.POINTER(C.c_int32)), len(p), buf)
    return buf.raw[:n].decode()
