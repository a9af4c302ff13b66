"""ctypes binding of libhvs.so (C ABI: include/hvs.h)."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_HERE)
_CSRC = os.path.join(_HERE, "csrc")
_LIB = os.path.join(_CSRC, "libhvs.so")
_HDR = os.path.join(_REPO, "include", "hvs.h")

ENGINE_AUTO, ENGINE_EXACT_SCAN, ENGINE_MFMA_FILTER, ENGINE_MFMA_I8, ENGINE_MFMA_F16 = 0, 1, 2, 3, 4
K, DCOLS, QCOLS = 100, 102, 104
NDIM = 100  # floats of a vector (a query row: 4 attribute floats + NDIM)

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"]


class HvsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hvs error {code}: {msg}")
        self.code = code


class Timing(C.Structure):
    _fields_ = [("query_ms", C.c_double), ("main_kernel_ms", C.c_double), ("main_kernel_launches", C.c_uint32),
                ("nq", C.c_uint32), ("pairs", C.c_uint64), ("scanned_pairs", C.c_uint64), ("load_ms", C.c_double),
                ("engine", C.c_uint32), ("fallback_queries", C.c_uint32), ("rescored_pairs", C.c_uint64),
                ("n_gpus", C.c_uint32), ("untimed_launches", C.c_uint32), ("host_ms", C.c_double),
                ("retry_queries", C.c_uint32), ("flags", C.c_uint32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class MaskInfo(C.Structure):
    """hvs_mask_info (include/hvs.h)."""
    _fields_ = [("n_live", C.c_uint32), ("n_dead", C.c_uint32), ("tiles_patched", C.c_uint64), ("dead_survivors", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class AppendInfo(C.Structure):
    """hvs_append_info (include/hvs.h)."""
    _fields_ = [("n_indexed", C.c_uint32), ("n_tail", C.c_uint32), ("tail_limit", C.c_uint32), ("reindexes", C.c_uint32),
                ("tail_pairs", C.c_uint64), ("tail_admitted", C.c_uint64), ("reindex_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class UpdateInfo(C.Structure):
    """hvs_update_info (include/hvs.h)."""
    _fields_ = [("n_stale", C.c_uint32), ("limit", C.c_uint32), ("stale_pairs", C.c_uint64), ("stale_admitted", C.c_uint64),
                ("stale_survivors", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class CompactInfo(C.Structure):
    """hvs_compact_info (include/hvs.h)."""
    _fields_ = [("compactions", C.c_uint32), ("n_before", C.c_uint32), ("n_after", C.c_uint32), ("first_moved", C.c_uint32),
                ("chunks", C.c_uint32), ("rows_moved", C.c_uint64), ("move_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PartitionInfo(C.Structure):
    """hvs_partition_info (include/hvs.h)."""
    _fields_ = [("n_parts", C.c_uint32), ("row0", C.c_uint32 * 17), ("padded_queries", C.c_uint32), ("exchanged_bytes", C.c_uint64),
                ("exchange_ms", C.c_double), ("merge_ms", C.c_double)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["row0"] = list(self.row0[:self.n_parts + 1])
        return d


class WithinInfo(C.Structure):
    """hvs_within_info (include/hvs.h)."""
    _fields_ = [("capped_queries", C.c_uint32), ("underfull_queries", C.c_uint32), ("within_slots", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class AfterInfo(C.Structure):
    """hvs_after_info (include/hvs.h)."""
    _fields_ = [("cursor_queries", C.c_uint32), ("exhausted_queries", C.c_uint32), ("underfull_queries", C.c_uint32),
                ("after_slots", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class InInfo(C.Structure):
    """hvs_in_info (include/hvs.h)."""
    _fields_ = [("set_queries", C.c_uint32), ("sub_queries", C.c_uint32), ("max_set", C.c_uint32), ("underfull_queries", C.c_uint32),
                ("merged_keys", C.c_uint64), ("expand_ms", C.c_double), ("merge_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ExcludeInfo(C.Structure):
    """hvs_exclude_info (include/hvs.h)."""
    _fields_ = [("excluding_queries", C.c_uint32), ("underfull_queries", C.c_uint32), ("kept_slots", C.c_uint64),
                ("refused_keys", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class VectorsInfo(C.Structure):
    """hvs_vectors_info (include/hvs.h)."""
    _fields_ = [("multi_queries", C.c_uint32), ("sub_queries", C.c_uint32), ("max_vectors", C.c_uint32), ("underfull_queries", C.c_uint32),
                ("merged_keys", C.c_uint64), ("duplicate_keys", C.c_uint64), ("expand_ms", C.c_double), ("merge_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ClausesInfo(C.Structure):
    """hvs_clauses_info (include/hvs.h)."""
    _fields_ = [("clause_queries", C.c_uint32), ("sub_queries", C.c_uint32), ("max_clauses", C.c_uint32), ("underfull_queries", C.c_uint32),
                ("read_keys", C.c_uint64), ("duplicate_keys", C.c_uint64), ("bounded_keys", C.c_uint64), ("skipped_chunks", C.c_uint64),
                ("expand_ms", C.c_double), ("merge_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class CandidatesInfo(C.Structure):
    """hvs_candidates_info (include/hvs.h)."""
    _fields_ = [("listed_queries", C.c_uint32), ("underfull_queries", C.c_uint32), ("scanned_ids", C.c_uint64),
                ("passing_ids", C.c_uint64), ("kept_slots", C.c_uint64), ("scan_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class RowSetsInfo(C.Structure):
    """hvs_row_sets_info (include/hvs.h)."""
    _fields_ = [("n_sets", C.c_uint32), ("words_per_set", C.c_uint32), ("bytes", C.c_uint64), ("restricted_queries", C.c_uint32),
                ("underfull_queries", C.c_uint32), ("refused_keys", C.c_uint64), ("kept_slots", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


IN_MAX_VALUES = 64
EXCLUDE_MAX = 1024
CANDIDATES_MAX = 8192
ROW_SETS_MAX = 256
VECTORS_MAX_EXTRA = 63
CLAUSES_MAX_EXTRA = 255


def library_path():
    return _LIB


def sources():
    return [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".hip", ".h", ".cpp"))] + [
        _HDR, os.path.join(_REPO, "include", "hvs_gen.h"), os.path.join(_REPO, "include", "hvs_vec_query.hpp"),
        os.path.join(_REPO, "tests", "seam_main.cpp")]


def build_library(force=False, verbose=False):
    """Compile csrc/hvs.hip for gfx950 into csrc/libhvs.so (hipcc cross-compiles without a GPU)."""
    if (not force and os.path.exists(_LIB) and os.path.exists(cli_path()) and os.path.exists(seam_path())
            and all(os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in sources())):
        return _LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + HIPCC_FLAGS + [os.path.join(_CSRC, "hvs.hip"), "-o", _LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=_CSRC)
    build_cli(verbose)
    build_seam(verbose)
    return _LIB


def cli_path():
    return os.path.join(_CSRC, "hvs_search.out")


def build_cli(verbose=False):
    """The reference-compatible command-line driver (csrc/hvs_main.cpp, argv contract of src/test.cpp)."""
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(_CSRC, "hvs_main.cpp"), "-L" + _CSRC, "-lhvs",
           "-Wl,-rpath,$ORIGIN", "-o", cli_path()]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=_CSRC)
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(_CSRC, "hvs_compare.cpp"), "-o", compare_path()]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=_CSRC)
    return cli_path()


def seam_path():
    """tests/seam_main.cpp: the reference's src/test.cpp with include/hvs_vec_query.hpp as its engine header."""
    return os.path.join(_REPO, "tests", "seam_main.out")


def build_seam(verbose=False):
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(_REPO, "include"), os.path.join(_REPO, "tests", "seam_main.cpp"),
           "-L" + _CSRC, "-lhvs", "-Wl,-rpath," + _CSRC, "-o", seam_path()]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return seam_path()


def compare_path():
    """The reference-compatible result checker (csrc/hvs_compare.cpp, CLI of src/compare_data.cpp)."""
    return os.path.join(_CSRC, "hvs_compare.out")


def exported_symbols():
    """Names declared in include/hvs.h (every one must be exported by libhvs.so)."""
    txt = open(_HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hvs_[a-z_0-9]+)\s*\(", txt)))


_lib = None
_f32p, _u32p, _u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def library():
    """Load libhvs.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("HVS_LIB", _LIB)   # A/B experiments load an alternative build of the same ABI
    if not os.path.exists(path):
        raise HvsError(-100, f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    vp = C.c_void_p
    sig = {
        "hvs_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "hvs_create_multi": (C.c_int, [C.POINTER(vp), C.c_int]),
        "hvs_create_on_devices": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]),
        "hvs_num_gpus": (C.c_int, [vp]),
        "hvs_device_count": (C.c_int, []),
        "hvs_set_gather": (C.c_int, [vp, C.c_int]),
        "hvs_reserve": (C.c_int, [vp, C.c_uint32]),
        "hvs_destroy": (None, [vp]),
        "hvs_last_error": (C.c_char_p, [vp]),
        "hvs_last_global_error": (C.c_char_p, []),
        "hvs_set_engine": (C.c_int, [vp, C.c_int]),
        "hvs_set_distance_order": (C.c_int, [vp, C.c_int]),
        "hvs_set_padding": (C.c_int, [vp, C.c_int]),
        "hvs_set_k": (C.c_int, [vp, C.c_uint32]),
        "hvs_get_k": (C.c_uint32, [vp]),
        "hvs_load_data": (C.c_int, [vp, _f32p, C.c_uint32]),
        "hvs_gen_data": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32]),
        "hvs_download_data": (C.c_int, [vp, C.c_uint32, C.c_uint32, _f32p]),
        "hvs_num_rows": (C.c_uint32, [vp]),
        "hvs_query": (C.c_int, [vp, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_upload_queries": (C.c_int, [vp, _f32p, C.c_uint32]),
        "hvs_gen_queries": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.c_uint64]),
        "hvs_download_queries": (C.c_int, [vp, C.c_uint32, C.c_uint32, _f32p]),
        "hvs_query_resident": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_float]),
        "hvs_sync": (C.c_int, [vp]),
        "hvs_download_results": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, _f32p]),
        "hvs_export_results_device": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp]),
        "hvs_stream_wait": (C.c_int, [vp, vp]),
        "hvs_merge_shards_device": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(C.c_uint64), C.c_uint32, vp, vp, vp]),
        "hvs_last_timing": (C.c_int, [vp, C.POINTER(Timing)]),
        "hvs_last_reruns": (C.c_int, [vp, C.c_int, _u32p, C.c_uint32]),
        "hvs_version": (C.c_char_p, []),
        "hvs_plan_guess_m": (C.c_uint32, [C.c_uint32, C.c_double, C.c_uint32]),
        "hvs_plan_batches": (C.c_uint32, [C.c_uint32, C.c_int, _u32p, C.c_uint32]),
        "hvs_delete_rows": (C.c_int, [vp, _u32p, C.c_uint32]),
        "hvs_set_row_mask": (C.c_int, [vp, _u64p]),
        "hvs_get_row_mask": (C.c_int, [vp, _u64p]),
        "hvs_num_live_rows": (C.c_uint32, [vp]),
        "hvs_mask_stats": (C.c_int, [vp, C.POINTER(MaskInfo)]),
        "hvs_mask_plan": (None, [_u64p, C.c_uint32, C.c_uint32, C.c_float, _u32p, _u32p, _u32p]),
        "hvs_append_rows": (C.c_int, [vp, _f32p, C.c_uint32, _u32p]),
        "hvs_reserve_rows": (C.c_int, [vp, C.c_uint32]),
        "hvs_reindex": (C.c_int, [vp]),
        "hvs_set_tail_limit": (C.c_int, [vp, C.c_uint32]),
        "hvs_append_stats": (C.c_int, [vp, C.POINTER(AppendInfo)]),
        "hvs_append_plan": (None, [C.c_uint32, C.c_uint32, C.c_float, _u32p, _u32p, _u32p]),
        "hvs_update_rows": (C.c_int, [vp, _u32p, _f32p, C.c_uint32]),
        "hvs_update_stats": (C.c_int, [vp, C.POINTER(UpdateInfo)]),
        "hvs_update_plan": (C.c_uint32, [_u32p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.POINTER(C.c_uint8)]),
        "hvs_compact": (C.c_int, [vp, _u32p]),
        "hvs_compact_stats": (C.c_int, [vp, C.POINTER(CompactInfo)]),
        "hvs_trim_rows": (C.c_int, [vp]),
        "hvs_compact_plan": (None, [_u64p, C.c_uint32, _u32p, _u32p, _u32p]),
        "hvs_create_partitioned": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]),
        "hvs_partition_stats": (C.c_int, [vp, C.POINTER(PartitionInfo)]),
        "hvs_partition_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _u32p, _u32p, _u32p]),
        "hvs_set_queries_device": (C.c_int, [vp, vp, C.c_uint32, vp]),
        "hvs_load_data_device": (C.c_int, [vp, vp, C.c_uint32, vp]),
        "hvs_set_queries_from_rows": (C.c_int, [vp, _u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_float]),
        "hvs_row_query": (None, [_f32p, C.c_int, C.c_float, _f32p]),
        "hvs_set_max_dist2": (C.c_int, [vp, _f32p, C.c_uint32]),
        "hvs_set_max_dist2_device": (C.c_int, [vp, vp, C.c_uint32, vp]),
        "hvs_query_within": (C.c_int, [vp, _f32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_within_stats": (C.c_int, [vp, C.POINTER(WithinInfo)]),
        "hvs_within_plan": (None, [_u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p, C.c_int, _u32p, _f32p, _u32p]),
        "hvs_set_after": (C.c_int, [vp, _f32p, _u32p, C.c_uint32]),
        "hvs_set_after_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "hvs_set_after_from_results": (C.c_int, [vp]),
        "hvs_query_after": (C.c_int, [vp, _f32p, _f32p, _u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_after_stats": (C.c_int, [vp, C.POINTER(AfterInfo)]),
        "hvs_after_plan": (None, [_u32p, _f32p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, _u32p, _f32p, C.c_int, _u32p, _f32p, _u32p]),
        "hvs_set_category_sets": (C.c_int, [vp, _u32p, _f32p, C.c_uint32]),
        "hvs_query_in": (C.c_int, [vp, _f32p, _u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_in_stats": (C.c_int, [vp, C.POINTER(InInfo)]),
        "hvs_in_plan": (C.c_uint32, [_f32p, _u32p, _f32p, C.c_uint32, _u32p, _u32p, _f32p]),
        "hvs_set_category_sets_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "hvs_download_in_plan": (C.c_int, [vp, _u32p, _u32p, _f32p, C.c_uint32]),
        "hvs_set_exclude_ids": (C.c_int, [vp, _u32p, _u32p, C.c_uint32]),
        "hvs_set_exclude_ids_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "hvs_query_excluding": (C.c_int, [vp, _f32p, _u32p, _u32p, _f32p, _u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_exclude_stats": (C.c_int, [vp, C.POINTER(ExcludeInfo)]),
        "hvs_download_exclude_plan": (C.c_int, [vp, _u32p, _u32p, _u32p, C.c_uint32]),
        "hvs_exclude_plan": (C.c_uint32, [_u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]),
        "hvs_set_candidate_ids": (C.c_int, [vp, _u32p, _u32p, C.c_uint32]),
        "hvs_set_candidate_ids_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "hvs_query_among": (C.c_int, [vp, _f32p, _u32p, _u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_candidates_stats": (C.c_int, [vp, C.POINTER(CandidatesInfo)]),
        "hvs_download_candidates_plan": (C.c_int, [vp, _u32p, _u32p, _u32p, C.c_uint32]),
        "hvs_candidates_plan": (C.c_uint32, [_u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]),
        "hvs_set_row_sets": (C.c_int, [vp, _u64p, C.c_uint32]),
        "hvs_set_row_sets_device": (C.c_int, [vp, vp, C.c_uint32, vp]),
        "hvs_assign_row_sets": (C.c_int, [vp, C.c_uint32, _u32p, C.c_uint32, C.c_int]),
        "hvs_get_row_sets": (C.c_int, [vp, _u64p]),
        "hvs_set_query_row_sets": (C.c_int, [vp, _u32p, C.c_uint32]),
        "hvs_set_query_row_sets_device": (C.c_int, [vp, vp, C.c_uint32, vp]),
        "hvs_query_in_row_sets": (C.c_int, [vp, _f32p, _u32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_row_sets_stats": (C.c_int, [vp, C.POINTER(RowSetsInfo)]),
        "hvs_row_sets_compact_plan": (None, [_u64p, _u64p, C.c_uint32, C.c_uint32, _u64p]),
        "hvs_set_query_vectors": (C.c_int, [vp, _u32p, _f32p, C.c_uint32]),
        "hvs_set_query_vectors_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "hvs_query_vectors": (C.c_int, [vp, _f32p, _u32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_vectors_stats": (C.c_int, [vp, C.POINTER(VectorsInfo)]),
        "hvs_vectors_plan": (C.c_uint32, [_u32p, _f32p, C.c_uint32, C.c_uint32, _u32p, _f32p, C.c_int, _u32p, _f32p, _u32p]),
        "hvs_vectors_check": (C.c_uint32, [_u32p, C.c_uint32]),
        "hvs_set_query_clauses": (C.c_int, [vp, _u32p, _f32p, _f32p, C.c_uint32]),
        "hvs_set_query_clauses_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp]),
        "hvs_query_clauses": (C.c_int, [vp, _f32p, _u32p, _f32p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p]),
        "hvs_clauses_stats": (C.c_int, [vp, C.POINTER(ClausesInfo)]),
        "hvs_clauses_check": (C.c_uint32, [_u32p, C.c_uint32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _fp(a):
    return a.ctypes.data_as(_f32p)


def _up(a):
    return a.ctypes.data_as(_u32p)


def pack_row_mask(live):
    """bool array of n rows -> the ceil(n / 64) uint64 words of hvs_set_row_mask (bit i & 63 of word i >> 6 = row i)."""
    live = np.ascontiguousarray(live, dtype=bool).ravel()
    bits = np.zeros(((live.size + 63) // 64) * 64, np.uint8)
    bits[:live.size] = live
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64))


def unpack_row_mask(words, n):
    """The inverse of pack_row_mask."""
    words = np.ascontiguousarray(words, "<u8")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def pack_row_sets(sets):
    """bool array [n_sets][n] -> (n_sets, n, the n_sets x ceil(n / 64) uint64 words of hvs_set_row_sets)."""
    sets = np.ascontiguousarray(sets, dtype=bool)
    if sets.ndim != 2:
        raise HvsError(-1, "row sets must be a bool array [n_sets][n]")
    words = np.zeros((sets.shape[0], (sets.shape[1] + 63) // 64), np.uint64)
    for s in range(sets.shape[0]):
        words[s] = pack_row_mask(sets[s])
    return sets.shape[0], sets.shape[1], words


def row_sets_compact_plan(sets, live):
    """hvs_row_sets_compact_plan: the sets (bool [n_sets][n]) as they must be after a compaction under the mask `live` (bool [n],
    or None = every row live): a bool array [n_sets][live rows]."""
    n_sets, n, words = pack_row_sets(sets)
    lw = None
    n_live = n
    if live is not None:
        live = np.ascontiguousarray(live, dtype=bool).ravel()
        if live.size != n:
            raise HvsError(-1, "live must hold one bool per row")
        lw = pack_row_mask(live)
        n_live = int(live.sum())
    out = np.full_like(words, np.uint64(0xA5A5A5A5A5A5A5A5))
    library().hvs_row_sets_compact_plan(words.ctypes.data_as(_u64p), lw.ctypes.data_as(_u64p) if lw is not None else None, n, n_sets,
                                        out.ctypes.data_as(_u64p))
    full = np.stack([unpack_row_mask(out[s], out.shape[1] * 64) for s in range(n_sets)]) if n_sets else np.zeros((0, 0), bool)
    if n_sets and full[:, n_live:].any():
        raise HvsError(-1, "hvs_row_sets_compact_plan left bits at or past the live rows")
    return full[:, :n_live]


def mask_plan(live, k, sample_proportion):
    """hvs_mask_plan on a bool array (or None = all live, then `live` must be the row count): (n_live, cut, pad_ids)."""
    if isinstance(live, (int, np.integer)):
        n, words = int(live), None
    else:
        live = np.asarray(live, dtype=bool).ravel()
        n, words = live.size, pack_row_mask(live)
    n_live, cut = C.c_uint32(0), C.c_uint32(0)
    pad = np.empty(int(k), np.uint32)
    library().hvs_mask_plan(words.ctypes.data_as(_u64p) if words is not None else None, n, int(k), float(sample_proportion),
                            C.byref(n_live), C.byref(cut), _up(pad))
    return int(n_live.value), int(cut.value), pad


def append_plan(n_indexed, n_total, sample_proportion):
    """hvs_append_plan: (sn, tail_lo, tail_hi) for an index over n_indexed of n_total rows."""
    sn, lo, hi = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    library().hvs_append_plan(int(n_indexed), int(n_total), float(sample_proportion), C.byref(sn), C.byref(lo), C.byref(hi))
    return int(sn.value), int(lo.value), int(hi.value)


def update_plan(stale, ids, n_indexed, n_total, want_last=True):
    """hvs_update_plan: fold one call's `ids` into the ascending stale list `stale`.  Returns (new stale list, last) with
    last[i] = True where occurrence i is the last of its id (None when want_last is False), or (None, None) when an id is
    >= n_total (nothing written)."""
    stale = np.ascontiguousarray(stale, np.uint32).ravel()
    ids = np.ascontiguousarray(ids, np.uint32).ravel()
    out = np.full(stale.size + ids.size + 1, 0xFFFFFFFF, np.uint32)
    last = np.full(ids.size + 1, 0xFF, np.uint8)
    m = library().hvs_update_plan(_up(stale), stale.size, _up(ids), ids.size, int(n_indexed), int(n_total), _up(out),
                                  last.ctypes.data_as(C.POINTER(C.c_uint8)) if want_last else None)
    if m == 0xFFFFFFFF:
        if (out != 0xFFFFFFFF).any() or (last != 0xFF).any():
            raise HvsError(-1, "hvs_update_plan wrote its outputs although it refused the ids")
        return None, None
    return out[:m].copy(), (last[:ids.size].astype(bool) if want_last else None)


def compact_plan(live, want_map=True):
    """hvs_compact_plan on a bool array (or None = all live, then `live` must be the row count): (n_live, first_dead,
    new_to_old) -- new_to_old is None when want_map is False."""
    if isinstance(live, (int, np.integer)):
        n, words = int(live), None
    else:
        live = np.asarray(live, dtype=bool).ravel()
        n, words = live.size, pack_row_mask(live)
    n_live, first_dead = C.c_uint32(0), C.c_uint32(0)
    out = np.full(n + 1, 0xFFFFFFFF, np.uint32) if want_map else None
    library().hvs_compact_plan(words.ctypes.data_as(_u64p) if words is not None else None, n, C.byref(n_live), C.byref(first_dead),
                               _up(out) if want_map else None)
    if want_map and (out[int(n_live.value):] != 0xFFFFFFFF).any():
        raise HvsError(-1, "hvs_compact_plan wrote past n_live entries")
    return int(n_live.value), int(first_dead.value), (out[:int(n_live.value)].copy() if want_map else None)


def partition_plan(n, n_parts, k, sample_proportion):
    """hvs_partition_plan: (row0[n_parts + 1], sn, local_sn[n_parts]) of a row-partitioned context over n rows, or None
    when the plan is refused (n_parts outside 1..16, or a part with fewer than k rows; nothing is written then)."""
    m = max(0, min(int(n_parts), 16))
    row0 = np.full(m + 2, 0xFFFFFFFF, np.uint32)
    local = np.full(m + 1, 0xFFFFFFFF, np.uint32)
    sn = C.c_uint32(0xFFFFFFFF)
    rc = library().hvs_partition_plan(int(n), int(n_parts), int(k), float(sample_proportion), _up(row0), C.byref(sn), _up(local))
    if rc != 0:
        if (row0 != 0xFFFFFFFF).any() or (local != 0xFFFFFFFF).any() or sn.value != 0xFFFFFFFF:
            raise HvsError(-1, "hvs_partition_plan wrote its outputs although it refused the plan")
        return None
    if row0[m + 1] != 0xFFFFFFFF or local[m] != 0xFFFFFFFF:
        raise HvsError(-1, "hvs_partition_plan wrote past its outputs")
    return row0[:m + 1].copy(), int(sn.value), local[:m].copy()


ROWQ_KNN, ROWQ_SAME_C, ROWQ_T_WINDOW, ROWQ_BOTH = 0, 1, 2, 3


def row_query(row, type, dt):
    """hvs_row_query: the query hvs_set_queries_from_rows builds from one data row (102 float32) -- [type, v, l, r] by `type`
    (0: k-NN, 1: same category, 2: T within +-dt, 3: both) and the row's 100 vector floats, as 104 float32."""
    row = np.ascontiguousarray(row, np.float32).ravel()
    if row.size != DCOLS or int(type) not in (0, 1, 2, 3):
        raise HvsError(-1, "row_query takes one row of 102 float32 and a type in 0..3")
    out = np.empty(QCOLS, np.float32)
    library().hvs_row_query(_fp(row), int(type), float(dt), _fp(out))
    return out


def within_plan(ids, dists, max_d2, pad_ids=None, pad_dists=None, padding=True):
    """hvs_within_plan: one uncapped, unpadded answer row (k ids, k distances; empty slots 0xFFFFFFFF / +inf) and a cap ->
    (ids, dists, n_within) of the capped row, padded from pad_ids / pad_dists (the first k padding rows) when `padding`."""
    ids = np.ascontiguousarray(ids, np.uint32).ravel()
    dists = np.ascontiguousarray(dists, np.float32).ravel()
    k = ids.size
    if dists.size != k:
        raise HvsError(-1, "within_plan: ids and dists must have k entries each")
    if padding:
        pad_ids = np.ascontiguousarray(pad_ids, np.uint32).ravel()
        pad_dists = np.ascontiguousarray(pad_dists, np.float32).ravel()
        if pad_ids.size < k or pad_dists.size < k:
            raise HvsError(-1, "within_plan: padding needs k pad ids and k pad distances")
    out_ids, out_d, n_in = np.empty(k, np.uint32), np.empty(k, np.float32), C.c_uint32(0)
    library().hvs_within_plan(_up(ids), _fp(dists), k, C.c_float(max_d2), _up(pad_ids) if padding else None,
                              _fp(pad_dists) if padding else None, int(bool(padding)), _up(out_ids), _fp(out_d), C.byref(n_in))
    return out_ids, out_d, int(n_in.value)


def _exclude_csr(lists):
    """Exclusion lists as a CSR pair of uint32 arrays: a LIST of per-query id sequences, or an (offsets, ids) TUPLE."""
    if isinstance(lists, tuple) and len(lists) == 2:
        off = np.ascontiguousarray(lists[0], np.uint32).ravel()
        ids = np.ascontiguousarray(lists[1], np.uint32).ravel()
    else:
        rows = [np.asarray(r, np.uint32).ravel() for r in lists]
        off = np.zeros(len(rows) + 1, np.uint32)
        if rows:
            off[1:] = np.cumsum([r.size for r in rows])
        ids = np.ascontiguousarray(np.concatenate(rows) if rows else np.empty(0, np.uint32), np.uint32)
    if off.size == 0:
        raise HvsError(-1, "exclusion lists: the offsets need nq + 1 entries")
    if ids.size == 0:
        ids = np.zeros(1, np.uint32)  # (a valid pointer for an empty id array)
    return off, ids


def exclude_plan(lists, row0=0, n_rows=0xFFFFFFFF):
    """hvs_exclude_plan: exclusion lists (a list of per-query id sequences, or an (offsets, ids) pair) normalised for rows
    [row0, row0 + n_rows) -> (kept, begin, count, ids), or None when the offsets are refused (nothing is written then)."""
    off, ids = _exclude_csr(lists)
    nq = off.size - 1
    begin, count = np.full(nq + 1, 0xFFFFFFFF, np.uint32), np.full(nq + 1, 0xFFFFFFFF, np.uint32)
    total = int(off[-1]) if nq and off[-1] >= off[0] and off[-1] <= ids.size else 0
    out = np.full(total + 1, 0xFFFFFFFF, np.uint32)
    kept = library().hvs_exclude_plan(_up(off), _up(ids), nq, int(row0), int(n_rows), _up(begin), _up(count), _up(out))
    if kept == 0xFFFFFFFF:
        if (begin != 0xFFFFFFFF).any() or (count != 0xFFFFFFFF).any() or (out != 0xFFFFFFFF).any():
            raise HvsError(-1, "hvs_exclude_plan wrote its outputs although it refused the lists")
        return None
    return int(kept), begin[:nq].copy(), count[:nq].copy(), out[:total].copy()


def candidates_plan(lists, row0=0, n_rows=0xFFFFFFFF):
    """hvs_candidates_plan: candidate lists (a list of per-query id sequences, or an (offsets, ids) pair) normalised for rows
    [row0, row0 + n_rows) -> (kept, begin, count, ids), or None when the offsets are refused (nothing is written then)."""
    off, ids = _exclude_csr(lists)
    nq = off.size - 1
    begin, count = np.full(nq + 1, 0xFFFFFFFF, np.uint32), np.full(nq + 1, 0xFFFFFFFF, np.uint32)
    total = int(off[-1]) if nq and off[-1] >= off[0] and off[-1] <= ids.size else 0
    out = np.full(total + 1, 0xFFFFFFFF, np.uint32)
    kept = library().hvs_candidates_plan(_up(off), _up(ids), nq, int(row0), int(n_rows), _up(begin), _up(count), _up(out))
    if kept == 0xFFFFFFFF:
        if (begin != 0xFFFFFFFF).any() or (count != 0xFFFFFFFF).any() or (out != 0xFFFFFFFF).any():
            raise HvsError(-1, "hvs_candidates_plan wrote its outputs although it refused the lists")
        return None
    return int(kept), begin[:nq].copy(), count[:nq].copy(), out[:total].copy()


def after_plan(ids, dists, k, after_dist, after_id, pad_ids=None, pad_dists=None, padding=True):
    """hvs_after_plan: a query's matched keys in key order (m ids, m distances) and a cursor -> (ids, dists, n_after) of the
    page of k slots behind the cursor, padded from pad_ids / pad_dists (the first k padding rows) when `padding`."""
    ids = np.ascontiguousarray(ids, np.uint32).ravel()
    dists = np.ascontiguousarray(dists, np.float32).ravel()
    m, k = ids.size, int(k)
    if dists.size != m:
        raise HvsError(-1, "after_plan: ids and dists must have the same number of entries")
    if padding:
        pad_ids = np.ascontiguousarray(pad_ids, np.uint32).ravel()
        pad_dists = np.ascontiguousarray(pad_dists, np.float32).ravel()
        if pad_ids.size < k or pad_dists.size < k:
            raise HvsError(-1, "after_plan: padding needs k pad ids and k pad distances")
    out_ids, out_d, n_after = np.empty(k, np.uint32), np.empty(k, np.float32), C.c_uint32(0)
    library().hvs_after_plan(_up(ids) if m else None, _fp(dists) if m else None, m, k, C.c_float(after_dist), int(after_id) & 0xFFFFFFFF,
                             _up(pad_ids) if padding else None, _fp(pad_dists) if padding else None, int(bool(padding)), _up(out_ids),
                             _fp(out_d), C.byref(n_after))
    return out_ids, out_d, int(n_after.value)


def _sets_csr(sets):
    """Category sets as (offsets uint32[nq + 1], values float32): from a LIST of per-query sequences, or a TUPLE (offsets,
    values) of an integer numpy array and the values, passed through as it is (so that a malformed CSR reaches the library)."""
    if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray) and sets[0].dtype.kind in "iu":
        off = np.ascontiguousarray(sets[0], np.uint32).ravel()
        vals = np.ascontiguousarray(sets[1], np.float32).ravel()
        return off, vals
    lens = [len(s) for s in sets]
    off = np.zeros(len(lens) + 1, np.uint32)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    vals = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).ravel() for s in sets]) if lens else [], np.float32)
    return off, vals


def in_plan(q_rows, sets, want=True):
    """hvs_in_plan: (nsub, sub_offsets, parent, value) of the expansion of `sets` (see _sets_csr) over `q_rows` (nq x 104, or
    None = every query of type 1); the three arrays are None when `want` is False, and the whole result is None when the plan
    is refused (malformed offsets, a set of more than 64 distinct categories; nothing is written then)."""
    off, vals = _sets_csr(sets)
    nq = max(off.size, 1) - 1
    q = None
    if q_rows is not None:
        q = np.ascontiguousarray(q_rows, np.float32)
        if q.ndim != 2 or q.shape != (nq, QCOLS):
            raise HvsError(-1, "in_plan: query rows must be nq x 104 float32, one per set")
    lib = library()
    args = (_fp(q) if q is not None else None, _up(off) if off.size else None, _fp(vals) if vals.size else None, nq)
    nsub = lib.hvs_in_plan(*args, None, None, None)
    if nsub == 0xFFFFFFFF:
        return None
    if not want:
        return int(nsub), None, None, None
    sub = np.full(nq + 2, 0xFFFFFFFF, np.uint32)
    parent = np.full(nsub + 1, 0xFFFFFFFF, np.uint32)
    value = np.full(nsub + 1, -12345.0, np.float32)
    if lib.hvs_in_plan(*args, _up(sub), _up(parent), _fp(value)) != nsub or sub[nq + 1] != 0xFFFFFFFF or parent[nsub] != 0xFFFFFFFF \
            or value[nsub] != np.float32(-12345.0):
        raise HvsError(-1, "hvs_in_plan wrote past its outputs")
    return int(nsub), sub[:nq + 1].copy(), parent[:nsub].copy(), value[:nsub].copy()


def _vectors_csr(vectors):
    """Extra query vectors as (offsets uint32[nq + 1], vecs float32[total, 100]): from a LIST of per-query [m_i, 100] arrays
    (an empty one leaves the query plain), or a TUPLE (offsets, vecs) passed through as it is (so that a malformed CSR reaches
    the library)."""
    if isinstance(vectors, tuple) and len(vectors) == 2:
        off = np.ascontiguousarray(vectors[0], np.uint32).ravel()
        vecs = np.ascontiguousarray(vectors[1], np.float32).reshape(-1, NDIM)
        return off, vecs
    rows = [np.asarray(v, np.float32).reshape(-1, NDIM) for v in vectors]
    off = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        off[1:] = np.cumsum([r.shape[0] for r in rows], dtype=np.uint64)
    vecs = np.ascontiguousarray(np.concatenate(rows) if rows else np.empty((0, NDIM)), np.float32)
    return off, vecs


def vectors_check(offsets):
    """hvs_vectors_check: the sub-queries nsub = offsets[nq] + nq of vector offsets (nq + 1 entries), or None when they are refused
    (offsets[0] != 0, a descending pair, more than VECTORS_MAX_EXTRA extras on a query, too many sub-queries)."""
    off = np.ascontiguousarray(offsets, np.uint32).ravel()
    if off.size == 0:
        raise HvsError(-1, "vectors_check: the offsets need nq + 1 entries")
    nsub = library().hvs_vectors_check(_up(off), off.size - 1)
    return None if nsub == 0xFFFFFFFF else int(nsub)


def vectors_plan(ids, dists, pad_ids=None, pad_dists=None, padding=True):
    """hvs_vectors_plan: the unpadded answer rows of ONE query's vectors (m x k ids and distances; empty slots 0xFFFFFFFF / +inf)
    -> (ids, dists, n_rows, n_duplicates) of the merged row: per id the smallest key, the first k, padded from pad_ids /
    pad_dists (the first k padding rows, the distances already the minimum over the vectors) when `padding`."""
    ids = np.ascontiguousarray(ids, np.uint32)
    dists = np.ascontiguousarray(dists, np.float32)
    if ids.ndim != 2 or dists.shape != ids.shape:
        raise HvsError(-1, "vectors_plan: ids and dists must be m x k each")
    m, k = ids.shape
    if padding:
        pad_ids = np.ascontiguousarray(pad_ids, np.uint32).ravel()
        pad_dists = np.ascontiguousarray(pad_dists, np.float32).ravel()
        if pad_ids.size < k or pad_dists.size < k:
            raise HvsError(-1, "vectors_plan: padding needs k pad ids and k pad distances")
    out_ids, out_d, dup = np.empty(k, np.uint32), np.empty(k, np.float32), C.c_uint32(0)
    kept = library().hvs_vectors_plan(_up(ids) if m else None, _fp(dists) if m else None, m, k, _up(pad_ids) if padding else None,
                                      _fp(pad_dists) if padding else None, int(bool(padding)), _up(out_ids), _fp(out_d), C.byref(dup))
    return out_ids, out_d, int(kept), int(dup.value)


def _clauses_csr(clauses, vectors=None):
    """Extra clauses as (offsets uint32[nq + 1], attrs float32[total, 4], vecs float32[total, 100] or None): `clauses` a LIST of
    per-query lists of [type, v, l, r] (an empty one leaves the query plain) with `vectors` None (predicate-only clauses) or a
    list of per-query [m_i, 100] arrays, one vector per clause; or a TUPLE (offsets, attrs) -- `vectors` then the vector array
    or None -- passed through as it is (so that a malformed CSR reaches the library)."""
    if isinstance(clauses, tuple) and len(clauses) == 2:
        off = np.ascontiguousarray(clauses[0], np.uint32).ravel()
        attrs = np.ascontiguousarray(clauses[1], np.float32).reshape(-1, 4)
        vecs = None if vectors is None else np.ascontiguousarray(vectors, np.float32).reshape(-1, NDIM)
        return off, attrs, vecs
    rows = [np.asarray(a, np.float32).reshape(-1, 4) for a in clauses]
    off = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        off[1:] = np.cumsum([r.shape[0] for r in rows], dtype=np.uint64)
    attrs = np.ascontiguousarray(np.concatenate(rows) if rows else np.empty((0, 4)), np.float32)
    vecs = None
    if vectors is not None:
        vr = [np.asarray(v, np.float32).reshape(-1, NDIM) for v in vectors]
        if [v.shape[0] for v in vr] != [r.shape[0] for r in rows]:
            raise HvsError(-1, "clauses: one vector per clause, or vectors=None")
        vecs = np.ascontiguousarray(np.concatenate(vr) if vr else np.empty((0, NDIM)), np.float32)
    return off, attrs, vecs


def clauses_check(offsets):
    """hvs_clauses_check: the sub-queries nsub = offsets[nq] + nq of clause offsets (nq + 1 entries), or None when they are refused
    (offsets[0] != 0, a descending pair, more than CLAUSES_MAX_EXTRA extras on a query, too many sub-queries)."""
    off = np.ascontiguousarray(offsets, np.uint32).ravel()
    if off.size == 0:
        raise HvsError(-1, "clauses_check: the offsets need nq + 1 entries")
    nsub = library().hvs_clauses_check(_up(off), off.size - 1)
    return None if nsub == 0xFFFFFFFF else int(nsub)


def product_clauses(q_rows, sets, vectors=None):
    """The cross product of category sets and extra vectors as clauses, built on the host: (q_out, offsets, attrs, vecs) for
    Engine.query_clauses(q_out, (offsets, attrs), vecs).  `sets` as for in_plan, `vectors` as for set_query_vectors (a list of
    per-query [m_i, 100] arrays, or None: no extras).  A query of type 1 / 3 with a non-empty set of c distinct categories
    (normalised and ordered as in_plan does) and m extras gets the c (1 + m) clauses [type, category, l, r] x vector, category by
    category, the query's own vector first; the first of them takes the place of clause 0, so q_out's own v is the first
    category.  A query that does not test C, or whose set is empty, gets its 1 + m vector clauses.  vecs is None when no query
    has an extra vector (predicate-only clauses: cursors stay allowed).  More than 1 + CLAUSES_MAX_EXTRA clauses on a query: an
    HvsError."""
    q = np.ascontiguousarray(q_rows, np.float32)
    if q.ndim != 2 or q.shape[1] != QCOLS:
        raise HvsError(-1, "product_clauses: query rows must be nq x 104 float32")
    nq = q.shape[0]
    plan = in_plan(q, sets)
    if plan is None:
        raise HvsError(-1, "product_clauses: the category sets are refused (see in_plan)")
    _, sub_off, _, value = plan
    set_off = _sets_csr(sets)[0]
    extras = [np.empty((0, NDIM), np.float32)] * nq if vectors is None else [np.asarray(v, np.float32).reshape(-1, NDIM) for v in vectors]
    if len(extras) != nq:
        raise HvsError(-1, "product_clauses: one vector list per query")
    with_vecs = any(v.shape[0] for v in extras)
    q_out = q.copy()
    attrs, vecs, off = [], [], np.zeros(nq + 1, np.uint32)
    for p in range(nq):
        t = q[p, 0]
        tests_c = bool(t > -1.0 and t < 4.0 and int(t) in (1, 3)) and set_off[p + 1] > set_off[p]
        cats = value[sub_off[p]:sub_off[p + 1]] if tests_c else q[p, 1:2]
        own = np.concatenate([q[p:p + 1, 4:], extras[p]])
        if len(cats) * own.shape[0] > 1 + CLAUSES_MAX_EXTRA:
            raise HvsError(-1, f"product_clauses: query {p} would have {len(cats) * own.shape[0]} clauses, more than {1 + CLAUSES_MAX_EXTRA}")
        first = True
        for cat in cats:
            for v in own:
                if first:
                    q_out[p, 1] = cat
                    first = False
                    continue
                attrs.append([q[p, 0], cat, q[p, 2], q[p, 3]])
                vecs.append(v)
        off[p + 1] = len(attrs)
    attrs = np.ascontiguousarray(np.asarray(attrs, np.float32).reshape(-1, 4))
    vecs = np.ascontiguousarray(np.asarray(vecs, np.float32).reshape(-1, NDIM)) if with_vecs else None
    return q_out, off, attrs, vecs


def _device_u32(x, what):
    """(pointer, entries) of a GPU tensor of 32-bit integers (torch.uint32 or torch.int32: the bits are the ids)."""
    import torch
    ok = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
    if not isinstance(x, torch.Tensor) or x.dtype not in ok or not x.is_cuda or not x.is_contiguous():
        raise HvsError(-1, f"{what}: the id tensor must be int32 / uint32, contiguous and on a GPU")
    return int(x.data_ptr()), x.numel()


def _device_rows(x, count, cols, what):
    """(pointer, rows) of a device buffer given as a raw pointer plus a row count, or as an object with data_ptr() and shape
    (a torch tensor): float32, contiguous, on a GPU, rows of `cols` floats."""
    if not (hasattr(x, "data_ptr") and hasattr(x, "shape")):
        if count is None:
            raise HvsError(-1, f"{what}: a raw pointer needs its row count")
        return int(x), int(count)
    import torch  # (only here: the package imports without it)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise HvsError(-1, f"{what}: the tensor must be float32, contiguous and on a GPU")
    if x.numel() % cols or (x.dim() == 2 and x.shape[1] != cols) or x.dim() > 2:
        raise HvsError(-1, f"{what}: the tensor must hold rows of {cols} float32")
    rows = x.numel() // cols
    if count is not None and int(count) > rows:
        raise HvsError(-1, f"{what}: the tensor holds {rows} rows, fewer than the {int(count)} asked for")
    return int(x.data_ptr()), rows if count is None else int(count)


def _stream_ptr(stream):
    """A hipStream_t from None (the null stream), a raw handle, or an object with `cuda_stream` (a torch stream)."""
    if stream is None:
        return None
    h = int(getattr(stream, "cuda_stream", stream))
    return C.c_void_p(h) if h else None


class Engine:
    """One hvs_ctx.  Engine(device): one GPU.  Engine(n_gpus=N) (0 = all visible) or Engine(devices=[...]): the
    multi-GPU context of hvs_create_multi / hvs_create_on_devices -- D replicated, the queries of a call partitioned,
    every GPU writing its slice of the result (a device index may repeat: virtual ranks on one GPU).
    Engine(devices=[...], partition=True): the row-partitioned context of hvs_create_partitioned -- D cut into one row range per
    entry of `devices`, every part answering all queries, the partial answers merged (same answers as one GPU)."""

    def __init__(self, device=-1, n_gpus=None, devices=None, partition=False):
        self._lib = library()
        h = C.c_void_p()
        if partition:
            if devices is None:
                raise HvsError(-1, "partition=True needs devices=[...]")
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._lib.hvs_create_partitioned(C.byref(h), arr, len(devices))
        elif devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._lib.hvs_create_on_devices(C.byref(h), arr, len(devices))
        elif n_gpus is not None:
            rc = self._lib.hvs_create_multi(C.byref(h), int(n_gpus))
        else:
            rc = self._lib.hvs_create(C.byref(h), device)
        if rc != 0:
            raise HvsError(rc, self._lib.hvs_last_global_error().decode())
        self._h = h
        self._padding = True  # (what set_padding last asked for: query_pages restores it)

    @property
    def num_gpus(self):
        return int(self._lib.hvs_num_gpus(self._h))

    def set_gather(self, mode):
        """0 = every GPU copies its block into its slice of the caller's array, 1 = peer gather to GPU 0 first."""
        self._ck(self._lib.hvs_set_gather(self._h, int(mode)))

    def partition_stats(self):
        """hvs_partition_stats: the row plan and the exchange / merge figures of the last call (partitioned contexts only)."""
        p = PartitionInfo()
        self._ck(self._lib.hvs_partition_stats(self._h, C.byref(p)))
        return p

    def reserve(self, nq):
        """Allocate query/result buffers and the batch workspace for calls of up to nq queries now."""
        self._ck(self._lib.hvs_reserve(self._h, int(nq)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hvs_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise HvsError(rc, self._lib.hvs_last_error(self._h).decode())

    def set_engine(self, engine):
        self._ck(self._lib.hvs_set_engine(self._h, engine))

    def set_distance_order(self, order):
        """0 = the hot path's SIMD order (default), 1 = the baseline engine's sequential order."""
        self._ck(self._lib.hvs_set_distance_order(self._h, order))

    def set_k(self, k):
        """Neighbours per query (the reference's compile-time KNN_LIMIT): 8..256, default 100."""
        self._ck(self._lib.hvs_set_k(self._h, int(k)))

    @property
    def k(self):
        return int(self._lib.hvs_get_k(self._h))

    def set_padding(self, enabled):
        """Off: answers of a data shard keep id 0xFFFFFFFF / distance +inf in unmatched slots."""
        self._ck(self._lib.hvs_set_padding(self._h, int(bool(enabled))))
        self._padding = bool(enabled)

    # --- data
    def load_data(self, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != DCOLS:
            raise HvsError(-1, "data rows must be n x 102 float32")
        self._ck(self._lib.hvs_load_data(self._h, _fp(rows), rows.shape[0]))

    def gen_data(self, n, seed, profile=1, ncat=100):
        self._ck(self._lib.hvs_gen_data(self._h, n, seed, profile, ncat))

    def download_data(self, row0, nrows):
        out = np.empty((nrows, DCOLS), np.float32)
        self._ck(self._lib.hvs_download_data(self._h, row0, nrows, _fp(out)))
        return out

    @property
    def n(self):
        return int(self._lib.hvs_num_rows(self._h))

    # --- row deletion (the live-row mask; include/hvs.h "row deletion")
    def delete_rows(self, ids):
        """Mark rows as deleted: later answers are those of the data set without them, ids unchanged."""
        ids = np.ascontiguousarray(np.asarray(ids).ravel(), np.uint32)
        self._ck(self._lib.hvs_delete_rows(self._h, _up(ids), ids.size))

    def set_row_mask(self, live):
        """Replace the whole mask: `live` is a bool array of n rows (True = live) or None for "all rows live"."""
        if live is None:
            self._ck(self._lib.hvs_set_row_mask(self._h, None))
            return
        live = np.asarray(live, dtype=bool).ravel()
        if live.size != self.n:
            raise HvsError(-1, "the row mask must have one entry per row")
        words = pack_row_mask(live)
        self._ck(self._lib.hvs_set_row_mask(self._h, words.ctypes.data_as(_u64p)))

    def row_mask(self):
        """The current mask as a bool array of n rows."""
        n = self.n
        words = np.zeros((n + 63) // 64, np.uint64)
        self._ck(self._lib.hvs_get_row_mask(self._h, words.ctypes.data_as(_u64p)))
        return unpack_row_mask(words, n)

    @property
    def n_live(self):
        return int(self._lib.hvs_num_live_rows(self._h))

    def mask_stats(self):
        m = MaskInfo()
        self._ck(self._lib.hvs_mask_stats(self._h, C.byref(m)))
        return m

    # --- row append (include/hvs.h "row append")
    def append_rows(self, rows):
        """Append rows (count x 102 float32): searchable by the next call; returns the id of the first of them."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != DCOLS:
            raise HvsError(-1, "data rows must be count x 102 float32")
        first = C.c_uint32(self.n)
        self._ck(self._lib.hvs_append_rows(self._h, _fp(rows), rows.shape[0], C.byref(first)))
        return int(first.value)

    def reserve_rows(self, n_capacity):
        """Room for the data set to grow to n_capacity rows without a device-to-device move."""
        self._ck(self._lib.hvs_reserve_rows(self._h, int(n_capacity)))

    def reindex(self):
        """Fold the appended rows into the index now."""
        self._ck(self._lib.hvs_reindex(self._h))

    def set_tail_limit(self, rows):
        """Appended rows the index may lag behind before an append rebuilds it (0: the default rule)."""
        self._ck(self._lib.hvs_set_tail_limit(self._h, int(rows)))

    def append_stats(self):
        a = AppendInfo()
        self._ck(self._lib.hvs_append_stats(self._h, C.byref(a)))
        return a

    # --- row update (include/hvs.h "row update in place")
    def update_rows(self, ids, rows):
        """Replace rows `ids` (uint32) by `rows` (count x 102 float32) in place: searchable by the next call, ids kept."""
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != DCOLS or rows.shape[0] != ids.size:
            raise HvsError(-1, "update rows must be len(ids) x 102 float32")
        self._ck(self._lib.hvs_update_rows(self._h, _up(ids), _fp(rows), ids.size))

    def update_stats(self):
        u = UpdateInfo()
        self._ck(self._lib.hvs_update_stats(self._h, C.byref(u)))
        return u

    # --- row compaction (include/hvs.h "row compaction")
    def compact(self):
        """Drop the deleted rows from the data set and renumber the live ones in order: afterwards the context is that of
        a fresh load of the live rows.  Returns new_to_old: the old id of every new id."""
        new_to_old = np.empty(self.n_live, np.uint32)
        self._ck(self._lib.hvs_compact(self._h, _up(new_to_old)))
        return new_to_old

    def compact_stats(self):
        s = CompactInfo()
        self._ck(self._lib.hvs_compact_stats(self._h, C.byref(s)))
        return s

    def trim_rows(self):
        """Give back the spare room of the data set's buffer (re-allocates it to exactly n rows)."""
        self._ck(self._lib.hvs_trim_rows(self._h))

    # --- the vec_query seam
    def query(self, q_rows, sample_proportion=1.0, want_dists=True, out_ids=None, out_dists=None, max_dist2=None, after=None, exclude=None,
              among=None, row_set=None):
        """hvs_query: host rows in, host ids (and distances) out.  `out_ids` / `out_dists`: caller-provided arrays
        (e.g. views of pinned memory) to be filled instead of fresh ones.  `max_dist2`: one squared-distance cap per query
        (hvs_query_within: the k nearest rows within it); None = no caps.  `after`: (dists, ids), one result cursor per query
        (hvs_query_after: the k nearest rows after that key); None = no cursors.  `exclude`: one exclusion list per query, a
        list of id sequences or an (offsets, ids) pair (hvs_query_excluding: the k nearest rows not in it); None = no lists.
        `among`: one candidate list per query in the same forms (hvs_query_among: the k nearest rows among it; with max_dist2
        only); None = no lists.  `row_set`: one set index per query, 0xFFFFFFFF = no restriction (hvs_query_in_row_sets: the k
        nearest rows inside that shared row set; on its own in one call); None = no indices."""
        q = np.ascontiguousarray(q_rows, np.float32)
        if q.ndim != 2 or q.shape[1] != QCOLS:
            raise HvsError(-1, "query rows must be nq x 104 float32")
        nq, K = q.shape[0], self.k
        ids = out_ids if out_ids is not None else np.empty((nq, K), np.uint32)
        d = out_dists if out_dists is not None else (np.empty((nq, K), np.float32) if want_dists else None)
        if ids.shape != (nq, K) or ids.dtype != np.uint32 or not ids.flags.c_contiguous:
            raise HvsError(-1, "out_ids must be a C-contiguous nq x k uint32 array")
        if d is not None and (d.shape != (nq, K) or d.dtype != np.float32 or not d.flags.c_contiguous):
            raise HvsError(-1, "out_dists must be a C-contiguous nq x k float32 array")
        caps = None
        if max_dist2 is not None:
            caps = np.ascontiguousarray(max_dist2, np.float32).ravel()
            if caps.size != nq:
                raise HvsError(-1, "max_dist2 must hold one float32 per query")
        ad = ai = None
        if after is not None:
            ad = np.ascontiguousarray(after[0], np.float32).ravel()
            ai = np.ascontiguousarray(after[1], np.uint32).ravel()
            if ad.size != nq or ai.size != nq:
                raise HvsError(-1, "after must be (dists, ids) with one entry per query each")
        if row_set is not None:
            if after is not None or exclude is not None or among is not None or caps is not None:
                raise HvsError(-1, "row_set stands alone in one call: attach caps, cursors or lists to the resident queries")
            idx = np.ascontiguousarray(row_set, np.uint32).ravel()
            if idx.size != nq:
                raise HvsError(-1, "row_set must hold one set index per query")
            self._ck(self._lib.hvs_query_in_row_sets(self._h, _fp(q), _up(idx), nq, sample_proportion, _up(ids),
                                                     _fp(d) if d is not None else None))
        elif among is not None:
            if after is not None or exclude is not None:
                raise HvsError(-1, "among composes with max_dist2 only in one call: attach cursors or exclusion lists to the resident queries")
            co, ci = _exclude_csr(among)
            if co.size != nq + 1:
                raise HvsError(-1, "among must hold one list per query")
            self._ck(self._lib.hvs_query_among(self._h, _fp(q), _up(co), _up(ci), _fp(caps) if caps is not None else None, nq,
                                               sample_proportion, _up(ids), _fp(d) if d is not None else None))
            self._cand_nq = nq
        elif exclude is not None:
            eo, ei = _exclude_csr(exclude)
            if eo.size != nq + 1:
                raise HvsError(-1, "exclude must hold one list per query")
            self._ck(self._lib.hvs_query_excluding(self._h, _fp(q), _up(eo), _up(ei), _fp(ad) if ad is not None else None,
                                                   _up(ai) if ai is not None else None, _fp(caps) if caps is not None else None, nq,
                                                   sample_proportion, _up(ids), _fp(d) if d is not None else None))
            self._excl_nq = nq
        elif after is not None:
            self._ck(self._lib.hvs_query_after(self._h, _fp(q), _fp(ad), _up(ai), _fp(caps) if caps is not None else None, nq,
                                               sample_proportion, _up(ids), _fp(d) if d is not None else None))
        elif caps is None:
            self._ck(self._lib.hvs_query(self._h, _fp(q), nq, sample_proportion, _up(ids), _fp(d) if d is not None else None))
        else:
            self._ck(self._lib.hvs_query_within(self._h, _fp(q), _fp(caps), nq, sample_proportion, _up(ids),
                                                _fp(d) if d is not None else None))
        return (ids, d) if d is not None else ids

    # --- per-query distance caps (include/hvs.h "per-query distance caps")
    def set_max_dist2(self, caps, stream=None):
        """Attach one squared-distance cap per resident query: a float32 array (hvs_set_max_dist2), a float32 GPU tensor
        (hvs_set_max_dist2_device; `stream` as for set_queries_device), or None to remove the caps.  Any call that replaces the
        resident queries removes them too."""
        if caps is None:
            self._ck(self._lib.hvs_set_max_dist2(self._h, None, 0))
        elif hasattr(caps, "data_ptr") and hasattr(caps, "shape"):
            ptr, n = _device_rows(caps, None, 1, "set_max_dist2")
            self._ck(self._lib.hvs_set_max_dist2_device(self._h, C.c_void_p(ptr) if ptr else None, n, _stream_ptr(stream)))
        else:
            caps = np.ascontiguousarray(caps, np.float32).ravel()
            self._ck(self._lib.hvs_set_max_dist2(self._h, _fp(caps), caps.size))

    def within_stats(self):
        """hvs_within_stats: capped / under-full queries and non-pad slots of the last call."""
        w = WithinInfo()
        self._ck(self._lib.hvs_within_stats(self._h, C.byref(w)))
        return w

    # --- per-query result cursors (include/hvs.h "per-query result cursors")
    def set_after(self, dists, ids, stream=None):
        """Attach one result cursor (after_dist, after_id) per resident query: two host arrays (hvs_set_after), two GPU tensors
        (hvs_set_after_device: float32 distances, int32 / uint32 ids; `stream` as for set_queries_device), or None, None to
        remove the cursors.  Any call that replaces the resident queries removes them too."""
        if dists is None and ids is None:
            self._ck(self._lib.hvs_set_after(self._h, None, None, 0))
        elif dists is None or ids is None:
            raise HvsError(-1, "set_after: give both dists and ids, or None for both")
        elif hasattr(dists, "data_ptr") and hasattr(ids, "data_ptr"):
            pd, n = _device_rows(dists, None, 1, "set_after")
            pi, ni = _device_u32(ids, "set_after")
            if ni != n:
                raise HvsError(-1, "set_after: dists and ids must have one entry per query each")
            self._ck(self._lib.hvs_set_after_device(self._h, C.c_void_p(pd) if pd else None, C.c_void_p(pi) if pi else None, n,
                                                    _stream_ptr(stream)))
        else:
            ad = np.ascontiguousarray(dists, np.float32).ravel()
            ai = np.ascontiguousarray(ids, np.uint32).ravel()
            if ad.size != ai.size:
                raise HvsError(-1, "set_after: dists and ids must have one entry per query each")
            self._ck(self._lib.hvs_set_after(self._h, _fp(ad), _up(ai), ad.size))

    def set_after_from_results(self):
        """hvs_set_after_from_results: every resident query's cursor becomes the last slot of its current result row, on the
        device (padding must be off, results of all resident queries must exist)."""
        self._ck(self._lib.hvs_set_after_from_results(self._h))

    def after_stats(self):
        """hvs_after_stats: queries with a cursor, exhausted and under-full ones, and non-pad slots of the last call."""
        a = AfterInfo()
        self._ck(self._lib.hvs_after_stats(self._h, C.byref(a)))
        return a

    def query_pages(self, q_rows, pages, sample_proportion=1.0, max_dist2=None):
        """The pages * k nearest rows of every query, k at a time: page 1 by query(), pages 2.. by set_after_from_results +
        query_resident.  Padding is off for the call (and restored): unpadded [nq][pages * k] ids and distances, empty slots
        0xFFFFFFFF / +inf behind a query's last match."""
        pages = int(pages)
        if pages < 1:
            raise HvsError(-1, "query_pages: pages must be at least 1")
        was = self._padding
        self.set_padding(False)
        try:
            ids, d = self.query(q_rows, sample_proportion, max_dist2=max_dist2)
            nq, K = ids.shape
            out_i = np.empty((nq, pages * K), np.uint32)
            out_d = np.empty((nq, pages * K), np.float32)
            out_i[:, :K], out_d[:, :K] = ids, d
            for p in range(1, pages):
                self.set_after_from_results()
                self.query_resident(0, nq, sample_proportion)
                pi, pd = self.download_results(0, nq)
                out_i[:, p * K:(p + 1) * K], out_d[:, p * K:(p + 1) * K] = pi, pd
            return out_i, out_d
        finally:
            self.set_padding(was)

    # --- per-query exclusion lists (include/hvs.h "per-query exclusion lists")
    def set_exclude_ids(self, lists, stream=None):
        """Attach one exclusion list per resident query: a list of per-query id sequences or an (offsets, ids) pair of host
        arrays (hvs_set_exclude_ids), an (offsets, ids) pair of GPU tensors (hvs_set_exclude_ids_device: int32 / uint32,
        contiguous, offsets with nq + 1 entries; `stream` as for set_queries_device), or None to remove the lists.  Any call
        that replaces the resident queries, and attaching or removing category sets, removes them too."""
        if lists is None:
            self._ck(self._lib.hvs_set_exclude_ids(self._h, None, None, 0))
        elif isinstance(lists, tuple) and len(lists) == 2 and all(hasattr(x, "data_ptr") and hasattr(x, "shape") for x in lists):
            po, n = _device_u32(lists[0], "set_exclude_ids")
            pi, _ = _device_u32(lists[1], "set_exclude_ids")
            self.set_exclude_ids_device(po, pi, max(n, 1) - 1, stream=stream)
        else:
            off, ids = _exclude_csr(lists)
            self._ck(self._lib.hvs_set_exclude_ids(self._h, _up(off), _up(ids), off.size - 1))
            self._excl_nq = off.size - 1

    def set_exclude_ids_device(self, offsets_ptr, ids_ptr, nq, stream=None):
        """hvs_set_exclude_ids_device from two raw pointers (0 / None = NULL) and the number of queries."""
        po, pi = int(offsets_ptr or 0), int(ids_ptr or 0)
        self._ck(self._lib.hvs_set_exclude_ids_device(self._h, C.c_void_p(po) if po else None, C.c_void_p(pi) if pi else None, int(nq),
                                                      _stream_ptr(stream)))
        self._excl_nq = int(nq)

    def exclude_stats(self):
        """hvs_exclude_stats: queries run under lists, under-full ones, non-pad slots and refused keys of the last call."""
        e = ExcludeInfo()
        self._ck(self._lib.hvs_exclude_stats(self._h, C.byref(e)))
        return e

    def exclude_plan_device(self, nq=None):
        """hvs_download_exclude_plan: (total, begin, count, ids) of the normalised lists of the resident queries as they lie
        on the device, whichever way they were attached (one-GPU contexts).  `nq`: the number of resident queries (None: that
        of the last set_exclude_ids / query(exclude=) of this object)."""
        nq = getattr(self, "_excl_nq", 0) if nq is None else nq
        total = self._lib.hvs_download_exclude_plan(self._h, None, None, None, 0)
        self._ck(min(total, 0))
        begin, count, ids = np.empty(int(nq), np.uint32), np.empty(int(nq), np.uint32), np.empty(max(total, 1), np.uint32)
        self._ck(min(self._lib.hvs_download_exclude_plan(self._h, _up(begin), _up(count), _up(ids), total), 0))
        return int(total), begin, count, ids[:total].copy()

    # --- shared row sets (include/hvs.h "shared row sets")
    def set_row_sets(self, sets, stream=None):
        """Load the context's row sets: a bool array [n_sets][n], a uint64 array [n_sets][ceil(n / 64)] of packed words
        (hvs_set_row_sets), a GPU tensor of packed words, int64 [n_sets][ceil(n / 64)] (hvs_set_row_sets_device; `stream` as for
        set_queries_device), or None to remove the sets.  The queries' set indices go with the sets they named."""
        if sets is None:
            self._ck(self._lib.hvs_set_row_sets(self._h, None, 0))
        elif hasattr(sets, "data_ptr") and hasattr(sets, "shape"):
            import torch
            if not isinstance(sets, torch.Tensor) or sets.dtype != torch.int64 or not sets.is_cuda or not sets.is_contiguous() or sets.dim() != 2:
                raise HvsError(-1, "set_row_sets: the tensor must be int64 [n_sets][ceil(n / 64)], contiguous and on a GPU")
            if sets.shape[1] != (self.n + 63) // 64:
                raise HvsError(-1, "set_row_sets: every set needs ceil(n / 64) words")
            self._ck(self._lib.hvs_set_row_sets_device(self._h, C.c_void_p(int(sets.data_ptr())), int(sets.shape[0]), _stream_ptr(stream)))
        else:
            a = np.asarray(sets)
            if a.dtype == np.uint64:
                words = np.ascontiguousarray(a)
                if words.ndim != 2 or words.shape[1] != (self.n + 63) // 64:
                    raise HvsError(-1, "set_row_sets: packed sets must be uint64 [n_sets][ceil(n / 64)]")
                n_sets = words.shape[0]
            else:
                n_sets, n, words = pack_row_sets(a)
                if n != self.n:
                    raise HvsError(-1, "set_row_sets: every set needs one bool per row")
            self._ck(self._lib.hvs_set_row_sets(self._h, words.ctypes.data_as(_u64p), n_sets))

    def assign_row_sets(self, set, ids, member=True):
        """hvs_assign_row_sets: put the rows `ids` into set `set` (member=False: take them out); ids >= n are ignored."""
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        self._ck(self._lib.hvs_assign_row_sets(self._h, int(set), _up(ids), ids.size, 1 if member else 0))

    def row_sets(self):
        """hvs_get_row_sets: the sets as a bool array [n_sets][n]."""
        st, n = self.row_sets_stats(), self.n
        words = np.zeros((st.n_sets, st.words_per_set), np.uint64)
        self._ck(self._lib.hvs_get_row_sets(self._h, words.ctypes.data_as(_u64p)))
        return np.stack([unpack_row_mask(words[s], n) for s in range(st.n_sets)])

    def set_query_row_sets(self, idx, stream=None):
        """Attach one set index per resident query (0xFFFFFFFF = no restriction): a host array (hvs_set_query_row_sets), an
        int32 / uint32 GPU tensor (hvs_set_query_row_sets_device), or None to remove the indices."""
        if idx is None:
            self._ck(self._lib.hvs_set_query_row_sets(self._h, None, 0))
        elif hasattr(idx, "data_ptr") and hasattr(idx, "shape"):
            ptr, n = _device_u32(idx, "set_query_row_sets")
            self._ck(self._lib.hvs_set_query_row_sets_device(self._h, C.c_void_p(ptr) if ptr else None, n, _stream_ptr(stream)))
        else:
            idx = np.ascontiguousarray(idx, np.uint32).ravel()
            self._ck(self._lib.hvs_set_query_row_sets(self._h, _up(idx), idx.size))

    def row_sets_stats(self):
        """hvs_row_sets_stats: the sets loaded, and restricted / under-full queries, refused keys and non-pad slots of the last call."""
        e = RowSetsInfo()
        self._ck(self._lib.hvs_row_sets_stats(self._h, C.byref(e)))
        return e

    # --- per-query candidate lists (include/hvs.h "per-query candidate lists")
    def set_candidate_ids(self, lists, stream=None):
        """Attach one candidate list per resident query: a list of per-query id sequences or an (offsets, ids) pair of host
        arrays (hvs_set_candidate_ids), an (offsets, ids) pair of GPU tensors (hvs_set_candidate_ids_device: int32 / uint32,
        contiguous, offsets with nq + 1 entries; `stream` as for set_queries_device), or None to remove the lists.  Any call
        that replaces the resident queries, and attaching or removing category sets, query vectors or clauses, removes them too."""
        if lists is None:
            self._ck(self._lib.hvs_set_candidate_ids(self._h, None, None, 0))
        elif isinstance(lists, tuple) and len(lists) == 2 and all(hasattr(x, "data_ptr") and hasattr(x, "shape") for x in lists):
            po, n = _device_u32(lists[0], "set_candidate_ids")
            pi, _ = _device_u32(lists[1], "set_candidate_ids")
            self.set_candidate_ids_device(po, pi, max(n, 1) - 1, stream=stream)
        else:
            off, ids = _exclude_csr(lists)
            self._ck(self._lib.hvs_set_candidate_ids(self._h, _up(off), _up(ids), off.size - 1))
            self._cand_nq = off.size - 1

    def set_candidate_ids_device(self, offsets_ptr, ids_ptr, nq, stream=None):
        """hvs_set_candidate_ids_device from two raw pointers (0 / None = NULL) and the number of queries."""
        po, pi = int(offsets_ptr or 0), int(ids_ptr or 0)
        self._ck(self._lib.hvs_set_candidate_ids_device(self._h, C.c_void_p(po) if po else None, C.c_void_p(pi) if pi else None, int(nq),
                                                        _stream_ptr(stream)))
        self._cand_nq = int(nq)

    def candidates_stats(self):
        """hvs_candidates_stats: queries run under lists, under-full ones, scanned and passing ids, non-pad slots and the scan's
        device time of the last call."""
        e = CandidatesInfo()
        self._ck(self._lib.hvs_candidates_stats(self._h, C.byref(e)))
        return e

    def candidates_plan_device(self, nq=None):
        """hvs_download_candidates_plan: (total, begin, count, ids) of the normalised lists of the resident queries as they lie
        on the device, whichever way they were attached (one-GPU contexts).  `nq`: the number of resident queries (None: that
        of the last set_candidate_ids / query(among=) of this object)."""
        nq = getattr(self, "_cand_nq", 0) if nq is None else nq
        total = self._lib.hvs_download_candidates_plan(self._h, None, None, None, 0)
        self._ck(min(total, 0))
        begin, count, ids = np.empty(int(nq), np.uint32), np.empty(int(nq), np.uint32), np.empty(max(total, 1), np.uint32)
        self._ck(min(self._lib.hvs_download_candidates_plan(self._h, _up(begin), _up(count), _up(ids), total), 0))
        return int(total), begin, count, ids[:total].copy()

    # --- category sets (include/hvs.h "category sets")
    def set_category_sets(self, sets, stream=None):
        """Attach one category set per resident query -- a list of per-query sequences of category values (an empty one leaves
        the query as it is), or an (offsets, values) CSR pair -- or None to remove the sets.  A query of type 1 or 3 with a
        non-empty set then matches the rows whose C is any of its values.  Caps and cursors are attached afterwards.
        A pair of GPU tensors -- offsets int32 / uint32 with nq + 1 entries, values float32 or None, both contiguous -- goes
        to hvs_set_category_sets_device: the plan is made on the GPU and the values never reach the host (`stream` as for
        set_queries_device)."""
        if sets is None:
            self._ck(self._lib.hvs_set_category_sets(self._h, None, None, 0))
            return
        if isinstance(sets, tuple) and len(sets) == 2 and any(hasattr(x, "data_ptr") and hasattr(x, "shape") for x in sets):
            self.set_category_sets_device(sets[0], sets[1], stream=stream)
            return
        off, vals = _sets_csr(sets)
        self._ck(self._lib.hvs_set_category_sets(self._h, _up(off) if off.size else None, _fp(vals) if vals.size else None,
                                                 max(off.size, 1) - 1))

    def set_category_sets_device(self, offsets, values, nq=None, stream=None):
        """hvs_set_category_sets_device: the CSR from device memory -- two GPU tensors (see set_category_sets), or two raw
        pointers (0 / None = NULL) with `nq`."""
        if hasattr(offsets, "data_ptr") or hasattr(values, "data_ptr"):
            po, n = _device_u32(offsets, "set_category_sets")
            pv = 0 if values is None else _device_rows(values, None, 1, "set_category_sets")[0]
            nq = max(n, 1) - 1 if nq is None else int(nq)
        else:
            if nq is None:
                raise HvsError(-1, "set_category_sets: raw pointers need the number of queries")
            po, pv, nq = int(offsets or 0), int(values or 0), int(nq)
        self._ck(self._lib.hvs_set_category_sets_device(self._h, C.c_void_p(po) if po else None, C.c_void_p(pv) if pv else None, nq,
                                                        _stream_ptr(stream)))

    def in_plan_device(self):
        """hvs_download_in_plan: (nsub, sub_offsets, parent, value) of the plan as it lies on the device, whichever way the
        sets were attached (one-GPU contexts)."""
        nsub = self._lib.hvs_download_in_plan(self._h, None, None, None, 0)
        self._ck(min(nsub, 0))
        # every user query has a sub-query, so nsub + 1 entries hold sub_offsets whatever nq is; the last parent names the last query
        sub, parent, value = np.zeros(nsub + 1, np.uint32), np.empty(nsub, np.uint32), np.empty(nsub, np.float32)
        self._ck(min(self._lib.hvs_download_in_plan(self._h, _up(sub), _up(parent), _fp(value), nsub), 0))
        nq = int(parent[-1]) + 1 if nsub else 0
        return int(nsub), sub[:nq + 1].copy(), parent, value

    def query_in(self, q_rows, sets, sample_proportion=1.0, want_dists=True):
        """hvs_query_in: host rows and their category sets in, host ids (and distances) out; sets = None is query()."""
        q = np.ascontiguousarray(q_rows, np.float32)
        if q.ndim != 2 or q.shape[1] != QCOLS:
            raise HvsError(-1, "query rows must be nq x 104 float32")
        nq, K = q.shape[0], self.k
        ids = np.empty((nq, K), np.uint32)
        d = np.empty((nq, K), np.float32) if want_dists else None
        off, vals = (None, None) if sets is None else _sets_csr(sets)
        if off is not None and off.size != nq + 1:
            raise HvsError(-1, "query_in: one set per query")
        self._ck(self._lib.hvs_query_in(self._h, _fp(q), _up(off) if off is not None else None,
                                        _fp(vals) if vals is not None and vals.size else None, nq, sample_proportion, _up(ids),
                                        _fp(d) if want_dists else None))
        return (ids, d) if want_dists else ids

    def in_stats(self):
        """hvs_in_stats: queries answered through their sets, sub-queries, under-full queries, merge time of the last call."""
        s = InInfo()
        self._ck(self._lib.hvs_in_stats(self._h, C.byref(s)))
        return s

    # --- multi-vector queries (include/hvs.h "multi-vector queries")
    def set_query_vectors(self, vectors, stream=None):
        """Attach extra vectors to the resident queries -- a list of per-query [m_i, 100] arrays (an empty one leaves the query
        plain) or an (offsets, vecs) CSR pair of host arrays --, or None to remove them.  A query then asks for the k rows
        nearest to ANY of its vectors (its own and the extras), each row once.  Caps and exclusion lists are attached
        afterwards; cursors are refused meanwhile.  A pair of GPU tensors -- offsets int32 / uint32 with nq + 1 entries, vecs
        float32 [total, 100] or None, both contiguous -- goes to hvs_set_query_vectors_device: the vectors never reach the host
        (`stream` as for set_queries_device)."""
        if vectors is None:
            self._ck(self._lib.hvs_set_query_vectors(self._h, None, None, 0))
            return
        if isinstance(vectors, tuple) and len(vectors) == 2 and any(hasattr(x, "data_ptr") and hasattr(x, "shape") for x in vectors):
            po, n = _device_u32(vectors[0], "set_query_vectors")
            pv = 0 if vectors[1] is None else _device_rows(vectors[1], None, NDIM, "set_query_vectors")[0]
            self.set_query_vectors_device(po, pv, max(n, 1) - 1, stream=stream)
            return
        off, vecs = _vectors_csr(vectors)
        self._ck(self._lib.hvs_set_query_vectors(self._h, _up(off) if off.size else None, _fp(vecs) if vecs.size else None,
                                                 max(off.size, 1) - 1))

    def set_query_vectors_device(self, offsets_ptr, vecs_ptr, nq, stream=None):
        """hvs_set_query_vectors_device from two raw pointers (0 / None = NULL) and the number of queries."""
        po, pv = int(offsets_ptr or 0), int(vecs_ptr or 0)
        self._ck(self._lib.hvs_set_query_vectors_device(self._h, C.c_void_p(po) if po else None, C.c_void_p(pv) if pv else None, int(nq),
                                                        _stream_ptr(stream)))

    def query_vectors(self, q_rows, vectors, sample_proportion=1.0, want_dists=True):
        """hvs_query_vectors: host rows and their extra vectors in, host ids (and distances) out; vectors = None is query()."""
        q = np.ascontiguousarray(q_rows, np.float32)
        if q.ndim != 2 or q.shape[1] != QCOLS:
            raise HvsError(-1, "query rows must be nq x 104 float32")
        nq, K = q.shape[0], self.k
        ids = np.empty((nq, K), np.uint32)
        d = np.empty((nq, K), np.float32) if want_dists else None
        off, vecs = (None, None) if vectors is None else _vectors_csr(vectors)
        if off is not None and off.size != nq + 1:
            raise HvsError(-1, "query_vectors: one vector list per query")
        self._ck(self._lib.hvs_query_vectors(self._h, _fp(q), _up(off) if off is not None else None,
                                             _fp(vecs) if vecs is not None and vecs.size else None, nq, sample_proportion, _up(ids),
                                             _fp(d) if want_dists else None))
        return (ids, d) if want_dists else ids

    def vector_stats(self):
        """hvs_vectors_stats: multi-vector queries, sub-queries, under-full queries, merged and duplicate keys, merge time of the
        last call."""
        s = VectorsInfo()
        self._ck(self._lib.hvs_vectors_stats(self._h, C.byref(s)))
        return s

    # --- query clauses (include/hvs.h "query clauses")
    def set_query_clauses(self, clauses, vectors=None, stream=None):
        """Attach extra clauses to the resident queries -- per query a list of [type, v, l, r] (an empty one leaves the query
        plain), or an (offsets, attrs) CSR pair of host arrays; `vectors` None (predicate-only clauses: every clause searches the
        query's own vector, cursors stay allowed) or one vector per clause --, or None to remove them.  A query then asks for the
        k rows with the smallest minimum key over the clauses they pass, each row once.  Caps, cursors and exclusion lists are
        attached afterwards.  A pair of GPU tensors (offsets int32 / uint32 with nq + 1 entries, attrs float32 [total, 4]) and
        `vectors` None or a GPU tensor float32 [total, 100] go to hvs_set_query_clauses_device: attributes and vectors never
        reach the host (`stream` as for set_queries_device)."""
        if clauses is None:
            self._ck(self._lib.hvs_set_query_clauses(self._h, None, None, None, 0))
            return
        if isinstance(clauses, tuple) and len(clauses) == 2 and any(hasattr(x, "data_ptr") and hasattr(x, "shape") for x in clauses):
            po, n = _device_u32(clauses[0], "set_query_clauses")
            pa = 0 if clauses[1] is None else _device_rows(clauses[1], None, 4, "set_query_clauses")[0]
            pv = 0 if vectors is None else _device_rows(vectors, None, NDIM, "set_query_clauses")[0]
            self.set_query_clauses_device(po, pa, pv, max(n, 1) - 1, stream=stream)
            return
        off, attrs, vecs = _clauses_csr(clauses, vectors)
        self._ck(self._lib.hvs_set_query_clauses(self._h, _up(off) if off.size else None, _fp(attrs) if attrs.size else None,
                                                 _fp(vecs) if vecs is not None and vecs.size else None, max(off.size, 1) - 1))

    def set_query_clauses_device(self, offsets_ptr, attrs_ptr, vecs_ptr, nq, stream=None):
        """hvs_set_query_clauses_device from three raw pointers (0 / None = NULL) and the number of queries."""
        po, pa, pv = int(offsets_ptr or 0), int(attrs_ptr or 0), int(vecs_ptr or 0)
        self._ck(self._lib.hvs_set_query_clauses_device(self._h, C.c_void_p(po) if po else None, C.c_void_p(pa) if pa else None,
                                                        C.c_void_p(pv) if pv else None, int(nq), _stream_ptr(stream)))

    def query_clauses(self, q_rows, clauses, vectors=None, sample_proportion=1.0, want_dists=True):
        """hvs_query_clauses: host rows and their extra clauses in, host ids (and distances) out; clauses = None is query()."""
        q = np.ascontiguousarray(q_rows, np.float32)
        if q.ndim != 2 or q.shape[1] != QCOLS:
            raise HvsError(-1, "query rows must be nq x 104 float32")
        nq, K = q.shape[0], self.k
        ids = np.empty((nq, K), np.uint32)
        d = np.empty((nq, K), np.float32) if want_dists else None
        off, attrs, vecs = (None, None, None) if clauses is None else _clauses_csr(clauses, vectors)
        if off is not None and off.size != nq + 1:
            raise HvsError(-1, "query_clauses: one clause list per query")
        self._ck(self._lib.hvs_query_clauses(self._h, _fp(q), _up(off) if off is not None else None,
                                             _fp(attrs) if attrs is not None and attrs.size else None,
                                             _fp(vecs) if vecs is not None and vecs.size else None, nq, sample_proportion, _up(ids),
                                             _fp(d) if want_dists else None))
        return (ids, d) if want_dists else ids

    def clause_stats(self):
        """hvs_clauses_stats: clause queries, sub-queries, under-full queries, the merge's four key counters and its time, of the
        last call."""
        s = ClausesInfo()
        self._ck(self._lib.hvs_clauses_stats(self._h, C.byref(s)))
        return s

    # --- resident variant
    def upload_queries(self, q_rows):
        q = np.ascontiguousarray(q_rows, np.float32)
        self._ck(self._lib.hvs_upload_queries(self._h, _fp(q), q.shape[0]))

    # --- inputs that are on the GPU already (include/hvs.h "device-resident inputs")
    def set_queries_device(self, ptr_or_tensor, nq=None, stream=None):
        """hvs_set_queries_device: resident queries from device memory (nq x 104 float32) of any visible GPU -- a raw pointer
        with `nq`, or a torch tensor.  `stream`: the stream that produced the buffer (a raw hipStream_t or a torch stream;
        None = the null stream).  Blocks until the copy is done."""
        ptr, nq = _device_rows(ptr_or_tensor, nq, QCOLS, "set_queries_device")
        self._ck(self._lib.hvs_set_queries_device(self._h, C.c_void_p(ptr) if ptr else None, nq, _stream_ptr(stream)))

    def load_data_device(self, ptr_or_tensor, n=None, stream=None):
        """hvs_load_data_device: the data set from device memory (n x 102 float32) of any visible GPU; arguments as for
        set_queries_device.  The context is that of load_data of the same rows."""
        ptr, n = _device_rows(ptr_or_tensor, n, DCOLS, "load_data_device")
        self._ck(self._lib.hvs_load_data_device(self._h, C.c_void_p(ptr) if ptr else None, n, _stream_ptr(stream)))

    def set_queries_from_rows(self, ids=None, first_id=0, nq=None, type=0, dt=0.0):
        """hvs_set_queries_from_rows: resident query i built on the device from stored row ids[i] (or, without ids, row
        first_id + i for i < nq) as D holds it now; `type` 0..3 and `dt` as in row_query."""
        if ids is not None:
            ids = np.ascontiguousarray(np.asarray(ids).ravel(), np.uint32)
            if nq is not None and int(nq) != ids.size:
                raise HvsError(-1, "set_queries_from_rows: nq does not match len(ids)")
            nq = ids.size
        elif nq is None:
            raise HvsError(-1, "set_queries_from_rows needs ids, or first_id and nq")
        self._ck(self._lib.hvs_set_queries_from_rows(self._h, _up(ids) if ids is not None else None, int(first_id), int(nq),
                                                     int(type), float(dt)))

    def gen_queries(self, nq, seed, profile=1, ncat=100, force_type=-1, first_row=0):
        self._ck(self._lib.hvs_gen_queries(self._h, nq, seed, profile, ncat, force_type, first_row))

    def download_queries(self, q0, nq):
        out = np.empty((nq, QCOLS), np.float32)
        self._ck(self._lib.hvs_download_queries(self._h, q0, nq, _fp(out)))
        return out

    def query_resident(self, q0, nq, sample_proportion=1.0):
        self._ck(self._lib.hvs_query_resident(self._h, q0, nq, sample_proportion))

    def sync(self):
        self._ck(self._lib.hvs_sync(self._h))

    def download_results(self, q0, nq, want_dists=True):
        K = self.k
        ids = np.empty((nq, K), np.uint32)
        d = np.empty((nq, K), np.float32) if want_dists else None
        self._ck(self._lib.hvs_download_results(self._h, q0, nq, _up(ids), _fp(d) if want_dists else None))
        return (ids, d) if want_dists else ids

    def export_results_device(self, q0, nq, ids_ptr, dists_ptr=None):
        """Copy results into device buffers given as raw pointers (e.g. torch tensor.data_ptr())."""
        self._ck(self._lib.hvs_export_results_device(self._h, q0, nq, C.c_void_p(ids_ptr),
                                                     C.c_void_p(dists_ptr) if dists_ptr else None))

    def stream_wait(self, stream_ptr):
        """Work enqueued on the given hipStream_t (raw pointer, e.g. torch.cuda.current_stream().cuda_stream) from now on
        waits for everything this context has enqueued so far -- a stream-ordered hand-off, no host wait for the kernels."""
        self._ck(self._lib.hvs_stream_wait(self._h, C.c_void_p(stream_ptr)))

    def merge_shards_device(self, ids_all_ptr, dists_all_ptr, shard_row0, nq, n_total, pad_dists_ptr, out_ids_ptr,
                            out_dists_ptr=None):
        """D-sharded mode: merge [nshards][nq][100] partial answers (device pointers, e.g. the output of an
        all_gather) into the whole-set answer on the device; see hvs_merge_shards_device in include/hvs.h."""
        rows = (C.c_uint64 * len(shard_row0))(*[int(r) for r in shard_row0])
        self._ck(self._lib.hvs_merge_shards_device(self._h, len(shard_row0), nq, C.c_void_p(ids_all_ptr),
                                                   C.c_void_p(dists_all_ptr), rows, n_total, C.c_void_p(pad_dists_ptr),
                                                   C.c_void_p(out_ids_ptr),
                                                   C.c_void_p(out_dists_ptr) if out_dists_ptr else None))

    def last_reruns(self, which):
        """Query indices of the last call answered a second time: which = 0 the exact engine's list, 1 the retry list."""
        n = self._lib.hvs_last_reruns(self._h, int(which), None, 0)
        if n < 0:
            self._ck(n)
        out = np.empty(n, np.uint32)
        if n:
            self._ck(min(0, self._lib.hvs_last_reruns(self._h, int(which), _up(out), n)))
        return out

    def last_timing(self):
        t = Timing()
        self._ck(self._lib.hvs_last_timing(self._h, C.byref(t)))
        return t
