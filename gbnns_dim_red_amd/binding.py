"""ctypes binding of include/gbnns.h.

Host buffers are numpy arrays; device buffers are torch CUDA(ROCm) tensors (torch is used only
as the owner of device memory and streams -- no torch op is on the search path).
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libgbnns_hip.so")

METRIC_L2, METRIC_NEG_DOT = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
MODE_NET, MODE_LOWQ, MODE_PLAIN = 0, 1, 2
FLAG_NO_FUSED_RERANK = 2
FLAG_AUX_GRAPH = 4
FLAG_LLF = 8
FLAG_WIDE_INDEX = 16
FLAG_BITMAP_PASS = 32
FLAG_SERIAL = 64
FLAG_DEFER_JOIN = 128
FLAG_MFMA_PROJECTION = 256
FLAG_HALF_ROWS = 512
FLAG_TAG_BRIDGE = 1024   # gbnns_search_tagged only: disallowed neighbours are looked through (bridge_graph)
FLAG_SCAN_GATHER = 4096  # search_auto only: scan-routed queries are served by the gathered exact scan (Index.exact_knn(gather=True)); every output unchanged
FLAG_BYTE_WALK = 2048    # MODE_PLAIN on a byte handle (Index(db=<uint8>)): walk the uint8 rows; the float handle's answers over db.astype(float32), bit for bit
FLAG_HALF_WALK = 8192    # MODE_PLAIN on a half-base handle (Index(db=<float16>)): walk the binary16 rows; the float handle's answers over db.astype(float32), bit for bit

# every symbol include/gbnns.h declares (tests check the library exports all of them)
SYMBOLS = [
    "gbnns_index_create", "gbnns_index_destroy", "gbnns_index_set_aux_graph", "gbnns_search_ex", "gbnns_search_batch", "gbnns_index_join", "gbnns_index_wait", "gbnns_host_pin", "gbnns_host_unpin",
    "gbnns_project", "gbnns_rerank", "gbnns_rerank_topk", "gbnns_search_topk", "gbnns_debug_knob", "gbnns_debug_walk_plan", "gbnns_debug_net_lds", "gbnns_index_knob", "gbnns_index_knob_get", "gbnns_profile_enable", "gbnns_profile_read", "gbnns_build_graph_gd", "gbnns_build_graph_gd_device",
    "gbnns_free", "gbnns_exact_knn", "gbnns_device_count", "gbnns_version", "gbnns_last_error",
    "gbnns_index_n", "gbnns_index_d", "gbnns_index_d_low", "gbnns_index_device",
    "gbnns_multi_create", "gbnns_multi_destroy", "gbnns_multi_size", "gbnns_multi_replica", "gbnns_multi_device_of",
    "gbnns_multi_stream", "gbnns_multi_set_aux_graph", "gbnns_shard_bounds", "gbnns_multi_search_ex",
    "gbnns_multi_search_device", "gbnns_multi_synchronize", "gbnns_multi_last_error",
    "gbnns_multi_rccl_single_rank", "gbnns_multi_rccl_version",
    "gbnns_round_to_half", "gbnns_index_enable_half_rows", "gbnns_index_low_rows",
    "gbnns_index_set_tags", "gbnns_search_tagged", "gbnns_debug_tag_plan", "gbnns_debug_bridge_plan",
    "gbnns_index_create_bytes", "gbnns_index_is_bytes", "gbnns_debug_byte_plan", "gbnns_debug_byte_walk_plan",
    "gbnns_exact_knn_bytes", "gbnns_debug_knn_bytes_plan", "gbnns_debug_knn_slab",
    "gbnns_search_byte_queries", "gbnns_debug_byte_query_plan",
    "gbnns_exact_knn_tagged", "gbnns_exact_knn_bytes_tagged", "gbnns_index_exact_knn",
    "gbnns_index_tag_census", "gbnns_search_tagged_auto",
    "gbnns_debug_knn_plan", "gbnns_debug_census_slot",
    "gbnns_index_exact_knn_gather", "gbnns_debug_gather_plan", "gbnns_debug_gather_schedule",
    "gbnns_debug_project_plan", "gbnns_index_project_last",
    "gbnns_index_order_last", "gbnns_debug_query_order",
    "gbnns_debug_rerank_plan",
    "gbnns_index_create_half_base", "gbnns_index_is_half_base", "gbnns_debug_half_base_plan",
    "gbnns_debug_half_walk_plan",
]


class GbnnsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gbnns status {code}: {msg}")
        self.code = code


class _IndexDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("metric", C.c_int32),
        ("mem_kind", C.c_int32), ("n", C.c_uint64), ("d", C.c_uint32), ("d_low", C.c_uint32),
        ("d_hidden", C.c_uint32), ("reserved0", C.c_uint32), ("db", C.c_void_p),
        ("db_low", C.c_void_p), ("graph_offsets", C.c_void_p), ("graph_nbrs", C.c_void_p),
        ("net_l1", C.c_void_p), ("net_l2", C.c_void_p), ("net_l3", C.c_void_p),
    ]


class _SearchArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_int32), ("ef", C.c_int32), ("k", C.c_int32),
        ("mem_kind", C.c_int32), ("hash_capacity", C.c_int32), ("n_q", C.c_uint64),
        ("queries", C.c_void_p), ("queries_low", C.c_void_p), ("entry_ids", C.c_void_p),
        ("out_ids", C.c_void_p), ("out_hops", C.c_void_p), ("out_dist_calc", C.c_void_p),
        ("out_cand", C.c_void_p), ("out_cand_dist", C.c_void_p), ("out_q_low", C.c_void_p),
        ("out_edges", C.c_void_p), ("stream", C.c_void_p), ("flags", C.c_uint32),
        ("hops_bound", C.c_uint32), ("n_entries", C.c_uint32), ("defer_depth", C.c_uint32),
    ]


class Profile(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("calls", C.c_uint32), ("project_ms", C.c_double),
        ("walk_ms", C.c_double), ("walk_general_ms", C.c_double), ("rerank_ms", C.c_double),
        ("total_ms", C.c_double), ("queries", C.c_uint64), ("general_queries", C.c_uint64),
        ("walk_kernel", C.c_char * 96), ("project_kernel", C.c_char * 32),
        ("retry_kernel", C.c_char * 96), ("retry_queries", C.c_uint64), ("retry_general_queries", C.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}
        d["walk_kernel"] = d["walk_kernel"].decode("ascii", "replace")
        d["project_kernel"] = d["project_kernel"].decode("ascii", "replace")
        d["retry_kernel"] = d["retry_kernel"].decode("ascii", "replace")
        return d


_lib = None


def lib_path():
    return _LIB_PATH


def load_library():
    """Load libgbnns_hip.so.  Fails loudly when it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc, gfx950).  gbnns_dim_red_amd has no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    lib.gbnns_last_error.restype = C.c_char_p
    lib.gbnns_index_create.argtypes = [C.POINTER(_IndexDesc), C.POINTER(C.c_void_p)]
    lib.gbnns_index_destroy.argtypes = [C.c_void_p]
    lib.gbnns_index_set_aux_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gbnns_search_ex.argtypes = [C.c_void_p, C.POINTER(_SearchArgs)]
    lib.gbnns_index_join.argtypes = [C.c_void_p]
    lib.gbnns_index_wait.argtypes = [C.c_void_p, C.c_uint32]
    lib.gbnns_host_pin.argtypes = [C.c_void_p, C.c_size_t]
    lib.gbnns_host_unpin.argtypes = [C.c_void_p]
    lib.gbnns_search_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gbnns_project.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                                  C.c_void_p]
    lib.gbnns_rerank.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_rerank_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_search_topk.argtypes = [C.c_void_p, C.POINTER(_SearchArgs), C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "gbnns_debug_knob"):  # (absent from the rounds 1-3 libraries that tools/ab4.sh may put in place of this one)
        lib.gbnns_debug_knob.argtypes = [C.c_char_p, C.c_int]
    if hasattr(lib, "gbnns_debug_walk_plan"):
        lib.gbnns_debug_walk_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    if hasattr(lib, "gbnns_debug_net_lds"):
        lib.gbnns_debug_net_lds.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    if hasattr(lib, "gbnns_index_knob"):
        lib.gbnns_index_knob.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.gbnns_index_knob_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.gbnns_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.gbnns_profile_read.argtypes = [C.c_void_p, C.POINTER(Profile), C.c_int]
    lib.gbnns_build_graph_gd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.gbnns_free.argtypes = [C.c_void_p]
    lib.gbnns_build_graph_gd_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_uint64)]
    lib.gbnns_exact_knn.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_exact_knn_bytes.argtypes = lib.gbnns_exact_knn.argtypes
    lib.gbnns_exact_knn_tagged.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_exact_knn_bytes_tagged.argtypes = lib.gbnns_exact_knn_tagged.argtypes
    lib.gbnns_index_exact_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p]
    lib.gbnns_index_exact_knn_gather.argtypes = lib.gbnns_index_exact_knn.argtypes
    lib.gbnns_debug_gather_plan.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.gbnns_debug_gather_schedule.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.gbnns_index_tag_census.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_search_tagged_auto.argtypes = [C.c_void_p, C.POINTER(_SearchArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    lib.gbnns_debug_knn_bytes_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    lib.gbnns_debug_knn_slab.argtypes = [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    lib.gbnns_debug_knn_plan.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_uint32,
                                         C.POINTER(C.c_int)]
    lib.gbnns_debug_census_slot.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(lib, "gbnns_debug_project_plan"):  # (as above: absent from an older library put in this one's place for an A/B run)
        lib.gbnns_debug_project_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_char_p, C.c_uint32]
        lib.gbnns_index_project_last.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
    if hasattr(lib, "gbnns_index_order_last"):
        lib.gbnns_index_order_last.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.gbnns_debug_query_order.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p]
    lib.gbnns_multi_last_error.restype = C.c_char_p
    lib.gbnns_multi_create.argtypes = [C.POINTER(_IndexDesc), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.gbnns_multi_destroy.argtypes = [C.c_void_p]
    lib.gbnns_multi_size.argtypes = [C.c_void_p]
    lib.gbnns_multi_replica.argtypes = [C.c_void_p, C.c_int32]
    lib.gbnns_multi_replica.restype = C.c_void_p
    lib.gbnns_multi_stream.argtypes = [C.c_void_p, C.c_int32]
    lib.gbnns_multi_stream.restype = C.c_void_p
    lib.gbnns_multi_device_of.argtypes = [C.c_void_p, C.c_int32]
    lib.gbnns_multi_set_aux_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gbnns_multi_search_ex.argtypes = [C.c_void_p, C.POINTER(_SearchArgs)]
    lib.gbnns_multi_search_device.argtypes = [C.c_void_p, C.POINTER(_SearchArgs), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gbnns_multi_synchronize.argtypes = [C.c_void_p]
    lib.gbnns_multi_rccl_single_rank.argtypes = [C.c_void_p, C.c_int]
    lib.gbnns_multi_rccl_version.argtypes = [C.c_void_p]
    lib.gbnns_shard_bounds.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.gbnns_shard_bounds.restype = None
    lib.gbnns_round_to_half.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.gbnns_index_enable_half_rows.argtypes = [C.c_void_p]
    lib.gbnns_index_low_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gbnns_index_set_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    lib.gbnns_search_tagged.argtypes = [C.c_void_p, C.POINTER(_SearchArgs), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gbnns_debug_tag_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int,
                                         C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.gbnns_debug_bridge_plan.argtypes = lib.gbnns_debug_tag_plan.argtypes
    lib.gbnns_index_create_bytes.argtypes = [C.POINTER(_IndexDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gbnns_index_is_bytes.argtypes = [C.c_void_p]
    lib.gbnns_debug_byte_walk_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                              C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.gbnns_debug_byte_query_plan.argtypes = lib.gbnns_debug_byte_walk_plan.argtypes
    lib.gbnns_debug_half_walk_plan.argtypes = lib.gbnns_debug_byte_walk_plan.argtypes
    lib.gbnns_search_byte_queries.argtypes = [C.c_void_p, C.POINTER(_SearchArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gbnns_debug_byte_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]
    lib.gbnns_debug_rerank_plan.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.gbnns_index_create_half_base.argtypes = [C.POINTER(_IndexDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gbnns_index_is_half_base.argtypes = [C.c_void_p]
    lib.gbnns_debug_half_base_plan.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.gbnns_index_d_low.argtypes = [C.c_void_p]
    lib.gbnns_index_d_low.restype = C.c_uint32
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise GbnnsError(rc, load_library().gbnns_last_error().decode(errors="replace"))


def version():
    return load_library().gbnns_version()


def device_count():
    return load_library().gbnns_device_count()


def _is_dev(x):
    return hasattr(x, "data_ptr")


def round_to_half(a):
    """gbnns_round_to_half (host code): (bits uint16, widened float32), both of a's shape -- a rounded to IEEE binary16, nearest even.
    GbnnsError when a value is not finite or rounds out of the binary16 range.  widened is the table R that
    FLAG_HALF_ROWS searches walk when a is db_low."""
    a = _host(a, np.float32)
    bits = np.empty(a.shape, np.uint16)
    wide = np.empty(a.shape, np.float32)
    _check(load_library().gbnns_round_to_half(a.ctypes.data, a.size, bits.ctypes.data, wide.ctypes.data))
    return bits, wide


def cut_graph(off, nbr, allowed):
    """G' of a tagged search, by NumPy: the CSR graph (off [n + 1], nbr) with every adjacency row keeping only the neighbours j with
    allowed[j] (a boolean mask over the n rows), in their original order -> (offsets uint64, nbrs uint32).  A tagged search of a query
    whose allowed rows are `allowed` is the reference's search on this graph: allowed = (tags & q_tag) != 0."""
    off = np.asarray(off, np.uint64)
    nbr = np.asarray(nbr, np.uint32)
    allowed = np.asarray(allowed, bool)
    n = len(off) - 1
    if allowed.shape != (n,):
        raise ValueError("allowed must have one entry per row")
    keep = allowed[nbr]
    owner = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    new_off = np.zeros(n + 1, np.uint64)
    new_off[1:] = np.cumsum(np.bincount(owner[keep], minlength=n))
    return new_off, np.ascontiguousarray(nbr[keep])


def bridge_graph(off, nbr, allowed):
    """G'' of a bridged tagged search (FLAG_TAG_BRIDGE), by NumPy: row u of the CSR graph (off [n + 1], nbr) rebuilt from its slots in order --
    an allowed neighbour v (allowed[v], a boolean mask over the n rows) stands for itself, a disallowed v is replaced by the allowed entries
    of v's own row in their order (one level: a disallowed entry of v's row is dropped).  A plain concatenation: a row may hold u itself and
    the same id more than once.  -> (offsets uint64, nbrs uint32).  A bridged tagged search of a query whose allowed rows are `allowed` is the
    reference's search on this graph: allowed = (tags & q_tag) != 0."""
    off = np.asarray(off, np.uint64)
    nbr = np.asarray(nbr, np.uint32)
    allowed = np.asarray(allowed, bool)
    n = len(off) - 1
    if allowed.shape != (n,):
        raise ValueError("allowed must have one entry per row")
    o = off.astype(np.int64)
    cut_off, cut_nbr = cut_graph(off, nbr, allowed)
    cut_o = cut_off.astype(np.int64)
    cut_deg = np.diff(cut_o)
    # what every slot contributes: itself, or the cut row of the neighbour it names
    width = np.where(allowed[nbr], 1, cut_deg[nbr]) if len(nbr) else np.zeros(0, np.int64)
    start = np.zeros(len(nbr) + 1, np.int64)
    start[1:] = np.cumsum(width)
    total = int(start[-1])
    src = np.repeat(np.arange(len(nbr)), width)            # the slot every output entry comes from
    k = np.arange(total) - start[src]                      # its index inside that slot's contribution
    v = nbr[src]
    from_cut = cut_nbr[np.minimum(cut_o[v] + k, max(len(cut_nbr) - 1, 0))] if len(cut_nbr) else np.zeros(total, np.uint32)
    out = np.where(allowed[v], v, from_cut).astype(np.uint32)
    new_off = start[o].astype(np.uint64)
    return new_off, np.ascontiguousarray(out)


def tag_census(T, Q):
    """gbnns_index_tag_census by NumPy (no device needed): for the row tags T [n] and the query words Q [nq], (allowed uint32 [nq], first uint32
    [nq]) -- allowed[i] = the number of rows j with (T[j] & Q[i]) != 0, first[i] = the lowest such j, 0xFFFFFFFF when there is none.  One pass
    over T per distinct word of Q."""
    T = np.ascontiguousarray(T, np.uint32).reshape(-1)
    Q = np.ascontiguousarray(Q, np.uint32).reshape(-1)
    allowed = np.zeros(len(Q), np.uint32)
    first = np.full(len(Q), 0xFFFFFFFF, np.uint32)
    for w in np.unique(Q):
        rows = np.flatnonzero(T & w)
        sel = Q == w
        allowed[sel] = len(rows)
        if len(rows):
            first[sel] = rows[0]
    return allowed, first


def tag_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, rr_reserve=0):
    """gbnns_debug_tag_plan (no device needed): name of the first-pass kernel a tagged search of that shape gets."""
    name = C.create_string_buffer(128)
    lds = C.c_uint64(0)
    _check(load_library().gbnns_debug_tag_plan(metric, dim, (dim + 3) // 4 * 4, n, ell_stride, aux_stride, ef, n_entries, int(wide), rr_reserve,
                                               name, 128, C.byref(lds)))
    return name.value.decode()


def bridge_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, rr_reserve=0, with_lds=False):
    """gbnns_debug_bridge_plan (no device needed): name of the first-pass kernel a tagged search with FLAG_TAG_BRIDGE of that shape gets;
    with_lds: (name, LDS bytes of that instance per wavefront without the visited set)."""
    name = C.create_string_buffer(128)
    lds = C.c_uint64(0)
    _check(load_library().gbnns_debug_bridge_plan(metric, dim, (dim + 3) // 4 * 4, n, ell_stride, aux_stride, ef, n_entries, int(wide), rr_reserve,
                                                  name, 128, C.byref(lds)))
    return (name.value.decode(), int(lds.value)) if with_lds else name.value.decode()


def byte_walk_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, tagged=False):
    """gbnns_debug_byte_walk_plan (no device needed): name of the first-pass kernel a MODE_PLAIN search with FLAG_BYTE_WALK of that shape gets
    on a byte handle (dim: the original dimension); "walk_general_kernel": the general kernel's byte-walk instance takes the whole batch."""
    name = C.create_string_buffer(128)
    lds = C.c_uint64(0)
    _check(load_library().gbnns_debug_byte_walk_plan(metric, dim, n, ell_stride, aux_stride, ef, n_entries, int(wide), int(tagged), name, 128,
                                                     C.byref(lds)))
    return name.value.decode()


def half_walk_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, tagged=False):
    """gbnns_debug_half_walk_plan (no device needed): name of the first-pass kernel a MODE_PLAIN search with FLAG_HALF_WALK of that shape gets
    on a half-base handle (dim: the original dimension; knob "half_walk_fast" = 2: every first-pass instance the library has, also of a class the default, 1, leaves to the general instance); "walk_general_kernel": the general kernel's half-walk
    instance takes the whole batch."""
    name = C.create_string_buffer(128)
    lds = C.c_uint64(0)
    _check(load_library().gbnns_debug_half_walk_plan(metric, dim, n, ell_stride, aux_stride, ef, n_entries, int(wide), int(tagged), name, 128,
                                                     C.byref(lds)))
    return name.value.decode()


def byte_query_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, tagged=False):
    """gbnns_debug_byte_query_plan (no device needed): byte_walk_plan for a call whose queries are uint8 too (Index.search(queries=<uint8>)) with
    the knob "byte_query_int" = 7 -- an integer instance ("beam_u8_kernel<...>" / "beam_u8_big_kernel<...>") inside the byte-walk first pass's
    domain, "walk_general_kernel" outside it."""
    name = C.create_string_buffer(128)
    lds = C.c_uint64(0)
    _check(load_library().gbnns_debug_byte_query_plan(metric, dim, n, ell_stride, aux_stride, ef, n_entries, int(wide), int(tagged), name, 128,
                                                      C.byref(lds)))
    return name.value.decode()


def byte_plan(metric, dim, n, ell_stride, ef, aux_stride=0, n_entries=1, wide=False, coop=False, late_rows=False, spec_rows=False, pass_no=0,
              rr_reserve=0):
    """gbnns_debug_byte_plan (no device needed): (name, fused) -- the first-pass kernel an untagged search of that walked shape gets on a byte
    handle (Index(db=<uint8>)) whose original dimension is a multiple of 16, and whether that kernel re-ranks its own query over the byte
    rows; fused False: the name is gbnns_debug_walk_plan's and the stand-alone byte re-rank kernel follows."""
    name = C.create_string_buffer(128)
    fused = C.c_int(0)
    _check(load_library().gbnns_debug_byte_plan(metric, dim, (dim + 3) // 4 * 4, n, ell_stride, aux_stride, ef, n_entries, int(wide), int(coop),
                                                int(late_rows), int(spec_rows), pass_no, rr_reserve, name, 128, C.byref(fused)))
    return name.value.decode(), bool(fused.value)


def rerank_plan(metric, d, bytes=False):
    """gbnns_debug_rerank_plan (no device needed): (name, deep, fused) -- the kernel Index.rerank launches on rows of d coordinates (bytes=True:
    the uint8 rows of a byte handle), the 16-byte row loads a lane of it has in flight in the first loop of its ladder (24 / 8 the float pair
    form, 4 the byte chunk-pair form, 0 a lane per row), and whether a MODE_NET / MODE_LOWQ search may fuse the re-rank of such rows into its
    walk kernels."""
    name = C.create_string_buffer(128)
    deep, fused = C.c_int(0), C.c_int(0)
    _check(load_library().gbnns_debug_rerank_plan(metric, d, int(bool(bytes)), name, 128, C.byref(deep), C.byref(fused)))
    return name.value.decode(), int(deep.value), bool(fused.value)


def half_base_plan(metric, d):
    """gbnns_debug_half_base_plan (no device needed): (name, deep, fused) -- the kernel Index.rerank launches on the binary16 rows of a half-base
    handle (Index(db=<float16>)) of d coordinates, the 16-byte row loads a lane of it has in flight in the first loop of its ladder (0: a lane
    per row), and fused, which is always False: no walk kernel re-ranks half rows, a re-rank launch follows every first pass."""
    name = C.create_string_buffer(128)
    deep, fused = C.c_int(0), C.c_int(0)
    _check(load_library().gbnns_debug_half_base_plan(metric, d, name, 128, C.byref(deep), C.byref(fused)))
    return name.value.decode(), int(deep.value), bool(fused.value)


def knn_bytes_plan(n, n_q, d, k):
    """gbnns_debug_knn_bytes_plan (no device needed): what exact_knn does with uint8 inputs of that shape under the current knn_chunk /
    knn_pool_min_k / knn_slab knobs -- dict(dp, cap, first_rows, max_chunk, pool, slab); slab: knn_slab(n_q, k, bytes=True)."""
    dp, cap, first, chunk, pool = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    _check(load_library().gbnns_debug_knn_bytes_plan(n, n_q, d, k, C.byref(dp), C.byref(cap), C.byref(first), C.byref(chunk), C.byref(pool)))
    return {"dp": int(dp.value), "cap": int(cap.value), "first_rows": int(first.value), "max_chunk": int(chunk.value), "pool": bool(pool.value),
            "slab": knn_slab(n_q, k, bytes=True)}


def knn_slab(n_q, k, bytes=False):
    """gbnns_debug_knn_slab (no device needed): the queries exact_knn serves at a time under the current knn_slab knob -- uint8 inputs
    (bytes=True), or float inputs on the pool path; n_q, or a multiple of 128."""
    slab = C.c_uint32(0)
    _check(load_library().gbnns_debug_knn_slab(int(bool(bytes)), n_q, k, C.byref(slab)))
    return int(slab.value)


def knn_plan(bytes, metric, n, n_q, d, k, tagged=False):
    """gbnns_debug_knn_plan (no device needed): (name, pool) -- the kernel that sweeps the rows of an exact_knn call of that shape under the
    current knn_filter / knn_pool_min_k knobs ("knn_filter_kernel<...>", "knn_scan_kernel<...>", "knn_scan_wide_kernel<...>"; bytes=True:
    "knn_bytes_sweep_kernel<...>"), taken from the table the launch reads, and whether the lists are pools (True) or heaps."""
    name = C.create_string_buffer(128)
    pool = C.c_int(0)
    _check(load_library().gbnns_debug_knn_plan(int(bool(bytes)), metric, n, n_q, d, k, int(bool(tagged)), name, 128, C.byref(pool)))
    return name.value.decode(), bool(pool.value)


def project_plan(d, d_hidden, d_low, n_q, cus=256, in_flight=False, mfma=False, mlp_net=1, mlp_slab=1, mlp_small=4096):
    """gbnns_debug_project_plan (no device needed): the names of the kernel instances the projection of an n_q-query batch through the net
    d -> d_hidden -> d_hidden -> d_low launches on a device of `cus` compute units, in launch order, template arguments as in the source;
    in_flight: a FLAG_DEFER_JOIN call, mfma: FLAG_MFMA_PROJECTION, mlp_*: the handle knobs of those names (defaults: the library's)."""
    names = C.create_string_buffer(512)
    _check(load_library().gbnns_debug_project_plan(d, d_hidden, d_low, n_q, cus, int(bool(in_flight)), int(bool(mfma)), mlp_net, mlp_slab,
                                                   mlp_small, names, 512))
    return tuple(names.value.decode().split("\n")) if names.value else ()


def gather_plan(bytes, metric, d, k):
    """gbnns_debug_gather_plan (no device needed): (name, W) -- the kernel that serves Index.exact_knn(gather=True) on a float (bytes=False) or
    byte handle of that metric and dimension, "knn_gather_kernel<...>", and the queries W one of its workgroups serves; for a shape the
    gathered kernel does not cover (d > 128, k > 4 096) the existing scan's tagged instance and W = 0: the call falls back to it."""
    name = C.create_string_buffer(128)
    w = C.c_uint32(0)
    _check(load_library().gbnns_debug_gather_plan(int(bool(bytes)), metric, d, k, name, 128, C.byref(w)))
    return name.value.decode(), int(w.value)


GATHER_BUDGET = 1 << 26   # default of the handle knob "gather_budget": list entries a round of the gathered scan may hold


def gather_schedule(words, allowed, n, budget=None, W=128):
    """gbnns_debug_gather_schedule (no device needed): the schedule Index.exact_knn(gather=True) builds from the queries' tag words [nq] and
    their census counts allowed [nq] (tag_census) over n rows -- dict(order, round_of, list_offset_of, rounds, workgroups); include/gbnns.h
    defines each.  budget None: the call's default, max(GATHER_BUDGET, n); W: queries per workgroup (gather_plan)."""
    words, allowed = _host(words, np.uint32).reshape(-1), _host(allowed, np.uint32).reshape(-1)
    nq = int(words.shape[0])
    if int(allowed.shape[0]) != nq:
        raise ValueError("words and allowed must have the same length")
    order, round_of, off = np.empty(nq, np.uint32), np.empty(nq, np.uint32), np.empty(nq, np.uint64)
    rounds, wgs = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().gbnns_debug_gather_schedule(words.ctypes.data, allowed.ctypes.data, nq, n, max(GATHER_BUDGET, n) if budget is None else budget,
                                                      W, order.ctypes.data, round_of.ctypes.data, off.ctypes.data, C.byref(rounds), C.byref(wgs)))
    return {"order": order, "round_of": round_of, "list_offset_of": off, "rounds": int(rounds.value), "workgroups": int(wgs.value)}


def knob_default(name):
    """gbnns_index_knob_get without a handle (no device needed): the process-wide default of "order_min" / "order_bits", what a handle
    created now would start from."""
    v = C.c_int(0)
    _check(load_library().gbnns_index_knob_get(None, name.encode() if isinstance(name, str) else name, C.byref(v)))
    return v.value


def query_order(queries, bits=12, dim=None):
    """gbnns_debug_query_order: the locality order of host queries [nq x qstride] (float32, C order) on the sign bits of their first `bits`
    coordinates (clamped to 10 .. 16), sorted on the current device; dim: the coordinates a row holds (default: all of them, qstride = dim).
    A permutation of 0 .. nq-1 with non-decreasing keys."""
    queries = _host(queries, np.float32)
    nq, qstride = int(queries.shape[0]), int(queries.shape[1])
    order = np.empty(nq, np.uint32)
    _check(load_library().gbnns_debug_query_order(queries.ctypes.data, qstride, qstride if dim is None else int(dim), nq, int(bits), order.ctypes.data))
    return order


def census_slot(word, n_q):
    """gbnns_debug_census_slot (no device needed): (slot, cap) -- the slot a query word's probe sequence starts at in the dedupe table of a
    tag census over n_q queries, and the table's slots (a power of two >= 2 n_q)."""
    slot, cap = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().gbnns_debug_census_slot(int(word) & 0xFFFFFFFF, n_q, C.byref(slot), C.byref(cap)))
    return int(slot.value), int(cap.value)


def _is_u8(x):
    if _is_dev(x):
        import torch
        return x.dtype == torch.uint8
    return isinstance(x, np.ndarray) and x.dtype == np.uint8


def _is_f16(x):
    if _is_dev(x):
        import torch
        return x.dtype == torch.float16
    return isinstance(x, np.ndarray) and x.dtype == np.float16


def _float32_queries(ix, queries):
    """float16 queries on a half-base handle: TypeError (the handle's kind alone is read, before anything touches the library)."""
    if _is_f16(queries) and getattr(ix, "is_half_base", False):
        raise TypeError("float16 queries: a half-base handle (Index(db=<float16>)) takes float32 queries -- the query is never rounded")


def _ptr(x):
    if x is None:
        return None
    if _is_dev(x):
        return x.data_ptr()
    return x.ctypes.data


def _host(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _prep(x, dtype, torch_dtype_name):
    """numpy -> contiguous numpy of dtype; torch tensor -> contiguous tensor (dtype checked)."""
    if x is None:
        return None
    if _is_dev(x):
        import torch
        want = getattr(torch, torch_dtype_name)
        if x.dtype != want:
            raise TypeError(f"expected torch.{torch_dtype_name}, got {x.dtype}")
        if not x.is_cuda and not x.is_pinned():
            raise TypeError("torch buffers must be CUDA/ROCm tensors (device buffers) or pinned CPU tensors "
                            "(page-locked host buffers); pass numpy arrays for pageable host memory")
        return x.contiguous()
    return _host(x, dtype)


def build_graph_gd(knn_offsets, knn_nbrs, ds, M, metric=METRIC_L2, reverse=True, threads=0):
    """hnswlikeGD + reverse edges (support_func.h:521-575, 402-445) on host arrays -> CSR."""
    lib = load_library()
    koff, knbr, ds = _host(knn_offsets, np.uint64), _host(knn_nbrs, np.uint32), _host(ds, np.float32)
    n, d = ds.shape
    po, pn = C.c_void_p(), C.c_void_p()
    _check(lib.gbnns_build_graph_gd(koff.ctypes.data, knbr.ctypes.data, ds.ctypes.data, n, d, M,
                                    metric, int(reverse), threads, C.byref(po), C.byref(pn)))
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        total = int(off[n])
        nbr = (np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint32)), shape=(max(total, 1),))
               [:total].copy())
    finally:
        lib.gbnns_free(po)
        lib.gbnns_free(pn)
    return off, nbr


def build_graph_gd_device(knn_offsets, knn_nbrs, ds, M, metric=METRIC_L2, reverse=True, threads=0, device=0):
    """gbnns_build_graph_gd_device: per-node pruning on the device (ties finished on the host), same result as
    build_graph_gd.  Returns (offsets, nbrs, nodes_finished_on_host)."""
    lib = load_library()
    koff, knbr, ds = _host(knn_offsets, np.uint64), _host(knn_nbrs, np.uint32), _host(ds, np.float32)
    n, d = ds.shape
    po, pn, hn = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    _check(lib.gbnns_build_graph_gd_device(device, koff.ctypes.data, knbr.ctypes.data, ds.ctypes.data, n, d, M,
                                           metric, int(reverse), threads, C.byref(po), C.byref(pn), C.byref(hn)))
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        total = int(off[n])
        nbr = (np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint32)), shape=(max(total, 1),))
               [:total].copy())
    finally:
        lib.gbnns_free(po)
        lib.gbnns_free(pn)
    return off, nbr, int(hn.value)


def _prep_tags(tags, dev, count, what):
    """A tag array beside host (numpy uint32) or device (CUDA/ROCm int32 tensor) inputs, one word per row / query."""
    if dev:
        if not (_is_dev(tags) and tags.is_cuda):
            raise TypeError(f"{what}: a CUDA/ROCm int32 tensor beside device inputs")
        tags = _prep(tags, np.uint32, "int32")
    else:
        if _is_dev(tags):
            raise TypeError(f"{what}: a numpy uint32 array beside host inputs")
        tags = _host(tags, np.uint32)
    if tags.ndim != 1 or int(tags.shape[0]) != count:
        raise ValueError(f"{what} must have {count} words")
    return tags


def exact_knn(base, queries, k, metric=METRIC_L2, self_offset=-1, want_dist=False, device=0, stream=None, row_tags=None, query_tags=None):
    """gbnns_exact_knn: ids [n_q x k] (and distances) of the k nearest base rows of every query, in the
    reference's distance arithmetic, ascending (distance, id).  numpy in -> numpy out; torch CUDA in -> torch
    out.  self_offset >= 0: query i is base row i + self_offset (excluded from its own list).
    Both arguments uint8 (numpy or torch): gbnns_exact_knn_bytes -- the same answer as over the widened arrays, bit for
    bit, on the int8 matrix cores and without a float copy (d <= 256, k <= 4096).
    row_tags [n] and query_tags [n_q] (both or neither; numpy uint32, or int32 tensors beside device inputs): gbnns_exact_knn_tagged /
    gbnns_exact_knn_bytes_tagged -- the same lists over the rows j with (row_tags[j] & query_tags[i]) != 0 only, under their original ids;
    0xFFFFFFFF / +inf where fewer than k rows are allowed."""
    lib = load_library()
    dev = _is_dev(base)
    if _is_dev(queries) != dev:
        raise TypeError("base and queries must live in the same memory kind")
    u8 = _is_u8(base)
    if _is_u8(queries) != u8:
        raise TypeError("base and queries must both be uint8 (gbnns_exact_knn_bytes: byte rows against byte queries) or both be float "
                        "(gbnns_exact_knn); for float queries against a byte table widen the table with .astype(float32)")
    tagged = row_tags is not None
    if (query_tags is not None) != tagged:
        raise TypeError("row_tags and query_tags: both or neither")
    if tagged:
        fn = lib.gbnns_exact_knn_bytes_tagged if u8 else lib.gbnns_exact_knn_tagged
    else:
        fn = lib.gbnns_exact_knn_bytes if u8 else lib.gbnns_exact_knn
    base = _prep(base, np.uint8, "uint8") if u8 else _prep(base, np.float32, "float32")
    queries = _prep(queries, np.uint8, "uint8") if u8 else _prep(queries, np.float32, "float32")
    n, d = int(base.shape[0]), int(base.shape[1])
    nq = int(queries.shape[0])
    if int(queries.shape[1]) != d:
        raise ValueError("dimension mismatch")
    if tagged:
        row_tags, query_tags = _prep_tags(row_tags, dev, n, "row_tags"), _prep_tags(query_tags, dev, nq, "query_tags")
    if dev:
        import torch
        ids = torch.empty((nq, k), dtype=torch.int32, device=base.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=base.device) if want_dist else None
        if stream is None:
            stream = torch.cuda.current_stream(base.device)
        sptr = stream.cuda_stream
        device = base.device.index or 0
    else:
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float32) if want_dist else None
        sptr = None
    tag_args = (_ptr(row_tags), _ptr(query_tags)) if tagged else ()
    _check(fn(device, _ptr(base), n, _ptr(queries), nq, d, k, metric, self_offset, *tag_args, _ptr(ids),
              _ptr(dist), MEM_DEVICE if dev else MEM_HOST, sptr))
    return (ids, dist) if want_dist else ids


def _check_multi(rc):
    if rc != 0:
        raise GbnnsError(rc, load_library().gbnns_multi_last_error().decode(errors="replace"))


class MultiIndex:
    """gbnns_multi: one replica of the index per entry of `devices` (host arrays in), a batch is cut into contiguous
    blocks, one per replica, each on its own host thread and HIP stream."""

    def __init__(self, db, graph_offsets, graph_nbrs, db_low=None, net=None, metric=METRIC_L2, devices=None):
        lib = load_library()
        self._lib = lib
        self._h = C.c_void_p()
        db = _host(db, np.float32)
        db_low = None if db_low is None else _host(db_low, np.float32)
        net = None if net is None else tuple(_host(x, np.float32) for x in net)
        off, nbr = _host(graph_offsets, np.uint64), _host(graph_nbrs, np.uint32)
        self.n, self.d = int(db.shape[0]), int(db.shape[1])
        self.d_low = int(db_low.shape[1]) if db_low is not None else 0
        self.d_hidden = int(net[0].shape[0]) if net is not None else 0
        desc = _IndexDesc(
            struct_size=C.sizeof(_IndexDesc), device=0, metric=metric, mem_kind=MEM_HOST, n=self.n, d=self.d,
            d_low=self.d_low, d_hidden=self.d_hidden, db=_ptr(db), db_low=_ptr(db_low), graph_offsets=_ptr(off),
            graph_nbrs=_ptr(nbr), net_l1=_ptr(net[0]) if net else None, net_l2=_ptr(net[1]) if net else None,
            net_l3=_ptr(net[2]) if net else None)
        devs = None if devices is None else np.ascontiguousarray(devices, np.int32)
        _check_multi(lib.gbnns_multi_create(C.byref(desc), _ptr(devs), 0 if devs is None else len(devs), C.byref(self._h)))
        self.size = lib.gbnns_multi_size(self._h)
        self.devices = [lib.gbnns_multi_device_of(self._h, i) for i in range(self.size)]

    def close(self):
        if self._h:
            self._lib.gbnns_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard_bounds(self, n_q, part):
        lo, hi = C.c_uint64(), C.c_uint64()
        self._lib.gbnns_shard_bounds(n_q, self.size, part, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def set_aux_graph(self, offsets, nbrs):
        off = None if offsets is None else _host(offsets, np.uint64)
        nbr = None if nbrs is None else _host(nbrs, np.uint32)
        _check_multi(self._lib.gbnns_multi_set_aux_graph(self._h, _ptr(off), _ptr(nbr)))

    def search(self, queries, ef, mode=MODE_NET, k=1, queries_low=None, entry_ids=None, want=("hops", "dist_calc"),
               flags=0, hops_bound=0):
        """gbnns_multi_search_ex: host arrays holding the whole batch in, numpy results out."""
        q = _host(queries, np.float32)
        ql = None if queries_low is None else _host(queries_low, np.float32)
        ent = None if entry_ids is None else _host(entry_ids, np.uint32)
        nq = q.shape[0]
        kk = ef if mode != MODE_PLAIN else max(1, min(k, ef))
        res = {"ids": np.empty(nq, np.uint32)}
        a = _SearchArgs(struct_size=C.sizeof(_SearchArgs), mode=mode, ef=ef, k=kk, mem_kind=MEM_HOST, n_q=nq,
                        queries=_ptr(q), queries_low=_ptr(ql), entry_ids=_ptr(ent), out_ids=_ptr(res["ids"]),
                        flags=flags, hops_bound=hops_bound,
                        n_entries=int(ent.shape[1]) if ent is not None and ent.ndim == 2 else 0)
        if "hops" in want:
            res["hops"] = np.empty(nq, np.int32); a.out_hops = _ptr(res["hops"])
        if "dist_calc" in want:
            res["dist_calc"] = np.empty(nq, np.int32); a.out_dist_calc = _ptr(res["dist_calc"])
        if "cand" in want:
            res["cand"] = np.empty((nq, kk), np.uint32); a.out_cand = _ptr(res["cand"])
        if "cand_dist" in want:
            res["cand_dist"] = np.empty((nq, kk), np.float32); a.out_cand_dist = _ptr(res["cand_dist"])
        if "q_low" in want:
            res["q_low"] = np.empty((nq, self.d_low), np.float32); a.out_q_low = _ptr(res["q_low"])
        _check_multi(self._lib.gbnns_multi_search_ex(self._h, C.byref(a)))
        return res

    def search_device(self, query_blocks, ef, n_q, mode=MODE_NET, entry_blocks=None, flags=0):
        """gbnns_multi_search_device: query_blocks[r] = torch tensor on replica r's device; returns one [n_q] int32
        tensor per replica (every one holds all answers once synchronize() has returned)."""
        import torch
        outs = [torch.empty(n_q, dtype=torch.int32, device=b.device) for b in query_blocks]
        qp = (C.c_void_p * self.size)(*[b.data_ptr() for b in query_blocks])
        op = (C.c_void_p * self.size)(*[o.data_ptr() for o in outs])
        ep = None if entry_blocks is None else (C.c_void_p * self.size)(*[e.data_ptr() for e in entry_blocks])
        a = _SearchArgs(struct_size=C.sizeof(_SearchArgs), mode=mode, ef=ef, k=1, flags=flags)
        _check_multi(self._lib.gbnns_multi_search_device(self._h, C.byref(a), n_q, qp, ep, op))
        self._keep = (query_blocks, entry_blocks, outs)
        return outs

    def synchronize(self):
        _check_multi(self._lib.gbnns_multi_synchronize(self._h))

    def rccl_single_rank(self, on=True):
        """One replica: run the exchange leg all the same (one-rank communicator, ncclAllGather of the single block)."""
        _check_multi(self._lib.gbnns_multi_rccl_single_rank(self._h, int(on)))

    def rccl_version(self):
        """ncclGetVersion() of the librccl this handle has loaded, 0 while it has not loaded one."""
        return int(self._lib.gbnns_multi_rccl_version(self._h))


class Index:
    """One dataset resident in HBM (gbnns_index).  db / db_low / net may be numpy arrays (copied
    to the device) or torch CUDA tensors (borrowed; kept alive by this object).
    db of dtype uint8 (numpy or torch): a byte handle (gbnns_index_create_bytes) -- the original-space table stays uint8 on the device and
    every search, rerank and rerank_topk returns what the index over db.astype(float32) returns, bit for bit; needs db_low, no MODE_PLAIN.
    db of dtype float16 (numpy or torch): a half-base handle (gbnns_index_create_half_base) -- the original-space table stays IEEE binary16 on
    the device, half the bytes of the float32 table, and every search, rerank and rerank_topk returns what the index over db.astype(float32)
    returns, bit for bit; needs db_low (the library's error without it), no MODE_PLAIN, no exact_knn / search_auto, float32 queries only.  The
    library rounds nothing itself: float32 data is rounded by the caller -- round_to_half(a)[0].view(np.float16) is that table."""

    def __init__(self, db, graph_offsets, graph_nbrs, db_low=None, net=None, metric=METRIC_L2,
                 device=0):
        lib = load_library()
        self._lib = lib
        self._h = C.c_void_p()
        dev = _is_dev(db)
        is_bytes, is_half = _is_u8(db), _is_f16(db)
        db = _prep(db, np.uint8, "uint8") if is_bytes else (_prep(db, np.float16, "float16") if is_half else _prep(db, np.float32, "float32"))
        db_low = _prep(db_low, np.float32, "float32")
        if db_low is not None and _is_dev(db_low) != dev:
            raise TypeError("db and db_low must live in the same memory kind")
        if net is not None:
            net = tuple(_prep(x, np.float32, "float32") for x in net)
            if any(_is_dev(x) != dev for x in net):
                raise TypeError("net layers must live in the same memory kind as db")
        off = _host(graph_offsets, np.uint64)
        nbr = _host(graph_nbrs, np.uint32)
        self.n, self.d = int(db.shape[0]), int(db.shape[1])
        self.d_low = int(db_low.shape[1]) if db_low is not None else 0
        self.d_hidden = int(net[0].shape[0]) if net is not None else 0
        if off.shape[0] != self.n + 1:
            raise ValueError("graph_offsets must have n+1 entries")
        if net is not None:
            shapes = [tuple(x.shape) for x in net]
            want = [(self.d_hidden, self.d + 1), (self.d_hidden, self.d_hidden + 1),
                    (self.d_low, self.d_hidden + 1)]
            if shapes != want:
                raise ValueError(f"net layer shapes {shapes} != {want}")
        desc = _IndexDesc(
            struct_size=C.sizeof(_IndexDesc), device=device, metric=metric,
            mem_kind=MEM_DEVICE if dev else MEM_HOST, n=self.n, d=self.d, d_low=self.d_low,
            d_hidden=self.d_hidden, db=None if is_bytes or is_half else _ptr(db), db_low=_ptr(db_low), graph_offsets=_ptr(off),
            graph_nbrs=_ptr(nbr), net_l1=_ptr(net[0]) if net else None,
            net_l2=_ptr(net[1]) if net else None, net_l3=_ptr(net[2]) if net else None)
        if is_bytes:
            _check(lib.gbnns_index_create_bytes(C.byref(desc), _ptr(db), C.byref(self._h)))
        elif is_half:
            _check(lib.gbnns_index_create_half_base(C.byref(desc), _ptr(db), C.byref(self._h)))
        else:
            _check(lib.gbnns_index_create(C.byref(desc), C.byref(self._h)))
        self._in_flight = collections.deque(maxlen=8)  # (inputs, outputs) of the deferred calls not yet joined
        self._last = None
        self._keep = (db, db_low, net) if dev else None
        self.metric = metric
        self.device = device

    @property
    def is_bytes(self):
        """gbnns_index_is_bytes: the original-space table is uint8 on the device (created from a uint8 db)."""
        return bool(self._lib.gbnns_index_is_bytes(self._h))

    @property
    def is_half_base(self):
        """gbnns_index_is_half_base: the original-space table is binary16 on the device (created from a float16 db)."""
        return bool(self._lib.gbnns_index_is_half_base(self._h))


    def set_aux_graph(self, offsets, nbrs):
        """The reference's auxiliary_graph (host CSR); None, None removes it."""
        if offsets is None:
            _check(self._lib.gbnns_index_set_aux_graph(self._h, None, None))
            return
        off = _host(offsets, np.uint64)
        nbr = _host(nbrs, np.uint32)
        if off.shape[0] != self.n + 1:
            raise ValueError("auxiliary graph offsets must have n+1 entries")
        _check(self._lib.gbnns_index_set_aux_graph(self._h, _ptr(off), _ptr(nbr)))

    def enable_half_rows(self):
        """gbnns_index_enable_half_rows: builds the binary16 table (and its float32 copy) that FLAG_HALF_ROWS searches walk."""
        _check(self._lib.gbnns_index_enable_half_rows(self._h))

    def low_rows(self, device=False):
        """gbnns_index_low_rows: R = float32(float16(db_low)) [n x d_low] as a numpy array, or (device=True) a torch tensor on the
        index's device (enqueued on the current stream)."""
        if device:
            import torch
            out = torch.empty((self.n, self.d_low), dtype=torch.float32, device=torch.device("cuda", self.device))
            _check(self._lib.gbnns_index_low_rows(self._h, out.data_ptr(), MEM_DEVICE, torch.cuda.current_stream(out.device).cuda_stream))
            return out
        out = np.empty((self.n, self.d_low), np.float32)
        _check(self._lib.gbnns_index_low_rows(self._h, out.ctypes.data, MEM_HOST, None))
        return out

    def set_tags(self, tags, first=0):
        """gbnns_index_set_tags: rows [first, first + len(tags)) get these 32-bit tag words (numpy: synchronous; torch CUDA int32 tensor:
        enqueued on the current stream).  The table starts out all ones."""
        if _is_dev(tags):
            import torch
            tags = _prep(tags, np.uint32, "int32")
            if not tags.is_cuda:
                raise TypeError("tags: a numpy array or a CUDA/ROCm int32 tensor")
            _check(self._lib.gbnns_index_set_tags(self._h, tags.data_ptr(), first, tags.numel(), MEM_DEVICE,
                                                  torch.cuda.current_stream(tags.device).cuda_stream))
            self._tags_keep = tags
            return
        tags = _host(tags, np.uint32)
        src = tags if tags.size else np.zeros(1, np.uint32)   # (an empty range still names a buffer: NULL with count 0 drops the table)
        _check(self._lib.gbnns_index_set_tags(self._h, src.ctypes.data, first, tags.size, MEM_HOST, None))

    def clear_tags(self):
        """Drops the tag table (gbnns_index_set_tags(NULL, 0, 0)): tagged searches are refused until set_tags is called again."""
        _check(self._lib.gbnns_index_set_tags(self._h, None, 0, 0, MEM_HOST, None))

    def close(self):
        if self._h:
            self._lib.gbnns_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- search ------------------------------------------------------------------------------
    def search(self, queries, ef, mode=MODE_NET, k=1, queries_low=None, entry_ids=None,
               want=("hops", "dist_calc"), hash_capacity=0, stream=None, out=None, flags=0,
               aux=False, llf=False, hops_bound=50, defer_depth=0, top_k=0, query_tags=None):
        """Runs one batch.  numpy queries -> synchronous call, numpy results.  torch CUDA queries
        -> enqueued on `stream` (torch stream or None = current), torch results, no sync.  Pinned torch CPU queries ->
        HOST buffers in page-locked memory, pinned torch results: synchronous, or with FLAG_DEFER_JOIN a host batch in
        flight (copy in, kernels and ids out on a lane's stream; wait() / join() + stream.synchronize() to read them).
        `want` may also name "cand", "cand_dist", "q_low", "edges".  Returns a dict with "ids" + wanted.
        aux / llf / hops_bound: the reference's use_second_graph walk over set_aux_graph()'s graph.
        top_k > 0 (NET / LOWQ): gbnns_search_topk -- also "top_ids" / "top_dist" [nq x top_k], the top_k best of each query's ef
        candidates in ascending (original-space distance, pop index); top_ids[:, 0] == ids.
        query_tags [nq] (uint32 numpy / int32 torch, like entry_ids): gbnns_search_tagged -- query i walks only the rows j with
        (tags[j] & query_tags[i]) != 0 (set_tags), i.e. the graph cut_graph gives; combines with top_k.  With flags=FLAG_TAG_BRIDGE a disallowed neighbour is looked
        through instead of dropped: the graph bridge_graph gives.
        uint8 queries (numpy uint8 / torch.uint8) on a byte handle (Index(db=<uint8>)): gbnns_search_byte_queries -- every result is, bit for
        bit, that of the same call with queries.astype(float32); same keywords.  On a float handle they raise TypeError (exact_knn's mixed-pair
        rule)."""
        top_k = top_k or 0
        _float32_queries(self, queries)
        u8 = _is_u8(queries)
        if u8 and not self.is_bytes:
            raise TypeError("uint8 queries need a byte handle (Index(db=<uint8>)); widen them for a float handle")
        if aux:
            flags |= FLAG_AUX_GRAPH | (FLAG_LLF if llf else 0)
        dev = _is_dev(queries) and queries.is_cuda
        pinned = _is_dev(queries) and not queries.is_cuda
        queries = _prep(queries, np.uint8, "uint8") if u8 else _prep(queries, np.float32, "float32")
        queries_low = _prep(queries_low, np.float32, "float32")
        nq = int(queries.shape[0])
        if queries.shape[1] != self.d:
            raise ValueError("query dimension mismatch")
        kk = ef if mode != MODE_PLAIN else max(1, min(k, ef))
        res = {} if out is None else out
        if dev:
            import torch
            tdev = queries.device
            entry_ids = None if entry_ids is None else entry_ids.to(torch.int32).contiguous() \
                if entry_ids.dtype != torch.int32 else entry_ids.contiguous()
            query_tags = _prep(query_tags, np.uint32, "int32")

            def alloc(name, shape, dtype):
                if name not in res:
                    res[name] = torch.empty(shape, dtype=dtype, device=tdev)
                return res[name]
            i32, f32 = torch.int32, torch.float32
            if stream is None:
                stream = torch.cuda.current_stream(tdev)
            sptr = stream.cuda_stream
        elif pinned:
            import torch
            if entry_ids is not None and not (_is_dev(entry_ids) and entry_ids.dtype == torch.int32 and entry_ids.is_pinned()):
                raise TypeError("entry_ids must be a pinned int32 tensor beside pinned queries")
            if query_tags is not None and not (_is_dev(query_tags) and query_tags.dtype == torch.int32 and query_tags.is_pinned()):
                raise TypeError("query_tags must be a pinned int32 tensor beside pinned queries")

            def alloc(name, shape, dtype):
                if name not in res:
                    res[name] = torch.empty(shape, dtype=dtype, pin_memory=True)
                return res[name]
            i32, f32 = torch.int32, torch.float32
            if stream is None:
                stream = torch.cuda.current_stream(self.device)  # (the index's device, whatever the current one is)
            sptr = stream.cuda_stream
        else:
            entry_ids = None if entry_ids is None else _host(entry_ids, np.uint32)
            query_tags = None if query_tags is None else _host(query_tags, np.uint32)

            def alloc(name, shape, dtype):
                if name not in res:
                    res[name] = np.empty(shape, dtype=dtype)
                return res[name]
            i32, f32 = np.int32, np.float32
            sptr = None
        n_entries = 0
        if entry_ids is not None and len(entry_ids.shape) == 2:
            n_entries = int(entry_ids.shape[1])   # several entry points per query (row-major)
        ids = alloc("ids", (nq,), i32 if (dev or pinned) else np.uint32)
        a = _SearchArgs(struct_size=C.sizeof(_SearchArgs), mode=mode, ef=ef, k=kk,
                        mem_kind=MEM_DEVICE if dev else MEM_HOST, hash_capacity=hash_capacity,
                        n_q=nq, queries=None if u8 else _ptr(queries), queries_low=_ptr(queries_low),
                        entry_ids=_ptr(entry_ids), out_ids=_ptr(ids), stream=sptr, flags=flags,
                        hops_bound=hops_bound if aux else 0, n_entries=n_entries, defer_depth=defer_depth)
        if "hops" in want:
            a.out_hops = _ptr(alloc("hops", (nq,), i32))
        if "dist_calc" in want:
            a.out_dist_calc = _ptr(alloc("dist_calc", (nq,), i32))
        if "cand" in want:
            a.out_cand = _ptr(alloc("cand", (nq, kk), i32 if (dev or pinned) else np.uint32))
        if "cand_dist" in want:
            a.out_cand_dist = _ptr(alloc("cand_dist", (nq, kk), f32))
        if "q_low" in want:
            a.out_q_low = _ptr(alloc("q_low", (nq, self.d_low), f32))
        if "edges" in want:
            a.out_edges = _ptr(alloc("edges", (nq,), i32))
        if query_tags is not None and int(query_tags.shape[0]) != nq:
            raise ValueError("query_tags must have one word per query")
        if top_k > 0:
            top_ids = alloc("top_ids", (nq, top_k), i32 if (dev or pinned) else np.uint32)
            top_dist = alloc("top_dist", (nq, top_k), f32)
        if u8:
            tk = (top_k, _ptr(top_ids), _ptr(top_dist)) if top_k > 0 else (0, None, None)
            _check(self._lib.gbnns_search_byte_queries(self._h, C.byref(a), _ptr(queries), _ptr(query_tags), *tk))
        elif top_k > 0:
            if query_tags is not None:
                _check(self._lib.gbnns_search_tagged(self._h, C.byref(a), _ptr(query_tags), top_k, _ptr(top_ids), _ptr(top_dist)))
            else:
                _check(self._lib.gbnns_search_topk(self._h, C.byref(a), top_k, _ptr(top_ids), _ptr(top_dist)))
        elif query_tags is not None:
            _check(self._lib.gbnns_search_tagged(self._h, C.byref(a), _ptr(query_tags), 0, None, None))
        else:
            _check(self._lib.gbnns_search_ex(self._h, C.byref(a)))
        # Inputs (and the result buffers handed out) stay referenced while a lane stream may still read / write them: torch's
        # caching allocators do not know the library's internal streams.  A plain call: until the next call; deferred
        # calls: the last four (= the most lanes a handle has), until wait() / join() / a plain call joins them.
        held = (queries, queries_low, entry_ids, query_tags, res)
        if flags & FLAG_DEFER_JOIN:
            self._in_flight.append(held)
        else:
            self._in_flight.clear()
        self._last = held
        return res

    def wait(self, keep=0):
        """gbnns_index_wait: blocks until every FLAG_DEFER_JOIN batch but the `keep` most recent has finished."""
        _check(self._lib.gbnns_index_wait(self._h, keep))
        while len(self._in_flight) > keep:
            self._in_flight.popleft()

    def join(self):
        """gbnns_index_join: the stream of the last FLAG_DEFER_JOIN call waits for that call's pieces."""
        _check(self._lib.gbnns_index_join(self._h))
        self._in_flight.clear()  # (the caller's stream now waits for the lanes: stream-ordered reuse of the buffers is safe)

    def search_batch(self, queries, ef, entry_ids=None, want_cand=False):
        """The plain 9-argument C entry point (NET mode, host buffers)."""
        q = _host(queries, np.float32)
        nq = q.shape[0]
        ids = np.empty(nq, np.uint32)
        hops = np.empty(nq, np.int32)
        dc = np.empty(nq, np.int32)
        cand = np.empty((nq, ef), np.uint32) if want_cand else None
        ent = None if entry_ids is None else _host(entry_ids, np.uint32)
        _check(self._lib.gbnns_search_batch(self._h, q.ctypes.data, nq, ef, _ptr(ent),
                                            ids.ctypes.data, hops.ctypes.data, dc.ctypes.data,
                                            _ptr(cand)))
        r = dict(ids=ids, hops=hops, dist_calc=dc)
        if want_cand:
            r["cand"] = cand
        return r

    def project(self, x, stream=None):
        """GetLowQueryFromNet over the rows of x -> [rows x d_low]."""
        dev = _is_dev(x)
        x = _prep(x, np.float32, "float32")
        if dev:
            import torch
            out = torch.empty((x.shape[0], self.d_low), dtype=torch.float32, device=x.device)
            if stream is None:
                stream = torch.cuda.current_stream(x.device)
            sptr = stream.cuda_stream
        else:
            out = np.empty((x.shape[0], self.d_low), np.float32)
            sptr = None
        _check(self._lib.gbnns_project(self._h, _ptr(x), x.shape[0], _ptr(out),
                                       MEM_DEVICE if dev else MEM_HOST, sptr))
        return out

    def rerank(self, queries, cand, count=None):
        """getRealNearest over a batch (host buffers): cand [nq x stride] in pop order."""
        _float32_queries(self, queries)
        q = _host(queries, np.float32)
        cand = _host(cand, np.uint32)
        count = None if count is None else _host(count, np.int32)
        out = np.empty(q.shape[0], np.uint32)
        _check(self._lib.gbnns_rerank(self._h, q.ctypes.data, q.shape[0], cand.ctypes.data,
                                      cand.shape[1], _ptr(count), out.ctypes.data, MEM_HOST, None))
        return out

    def rerank_topk(self, queries, cand, k, count=None, want_dist=True):
        """gbnns_rerank_topk (host buffers): the k best of each row of cand [nq x stride] (pop order) -> (ids, dist) [nq x k],
        ascending (distance, pop index); 0xFFFFFFFF / +inf from column count on.  ids[:, 0] == rerank(queries, cand, count)."""
        _float32_queries(self, queries)
        q = _host(queries, np.float32)
        cand = _host(cand, np.uint32)
        count = None if count is None else _host(count, np.int32)
        ids = np.empty((q.shape[0], k), np.uint32)
        dist = np.empty((q.shape[0], k), np.float32) if want_dist else None
        _check(self._lib.gbnns_rerank_topk(self._h, q.ctypes.data, q.shape[0], cand.ctypes.data, cand.shape[1], _ptr(count), k,
                                           ids.ctypes.data, _ptr(dist), MEM_HOST, None))
        return ids, dist

    def exact_knn(self, queries, k, query_tags=None, self_offset=-1, want_dist=False, gather=False):
        """gbnns_index_exact_knn: exact_knn(db, queries, k, metric=<the handle's>, ...) over the handle's resident table, read in place --
        nothing of the table is uploaded.  query_tags [nq]: the tagged answer over set_tags()'s table (exact_knn's row_tags / query_tags
        form, the ground truth of search(query_tags=...)); None: the untagged answer.  A float handle takes float queries (uint8 ones raise
        TypeError), a byte handle uint8 queries (float ones: GbnnsError, code 5 -- there is no mixed-pair scan).  numpy queries -> numpy
        results; torch CUDA queries -> torch results, on the current stream.  Returns ids, or (ids, dist) with want_dist.
        gather=True: gbnns_index_exact_knn_gather -- the same bytes, computed from distances to the rows each query's word allows only (the
        queries of a word scan that word's row list); needs query_tags (None: ValueError).  Opt-in; gather_plan() names its kernel."""
        if gather and query_tags is None:
            raise ValueError("exact_knn(gather=True) needs query_tags: an untagged call has nothing to gather")
        u8 = _is_u8(queries)
        if u8 and not self.is_bytes:
            raise TypeError("uint8 queries need a byte handle (Index(db=<uint8>)); widen them for a float handle")
        dev = _is_dev(queries)
        if dev and not queries.is_cuda:
            raise TypeError("queries: a numpy array or a CUDA/ROCm tensor")
        queries = _prep(queries, np.uint8, "uint8") if u8 else _prep(queries, np.float32, "float32")
        nq = int(queries.shape[0])
        if queries.ndim != 2 or int(queries.shape[1]) != self.d:
            raise ValueError("query dimension mismatch")
        if query_tags is not None:
            query_tags = _prep_tags(query_tags, dev, nq, "query_tags")
        if dev:
            import torch
            ids = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
            dist = torch.empty((nq, k), dtype=torch.float32, device=queries.device) if want_dist else None
            sptr = torch.cuda.current_stream(queries.device).cuda_stream
        else:
            ids = np.empty((nq, k), np.uint32)
            dist = np.empty((nq, k), np.float32) if want_dist else None
            sptr = None
        fn = self._lib.gbnns_index_exact_knn_gather if gather else self._lib.gbnns_index_exact_knn
        _check(fn(self._h, None if u8 else _ptr(queries), _ptr(queries) if u8 else None, nq, _ptr(query_tags), k, self_offset, _ptr(ids), _ptr(dist),
                  MEM_DEVICE if dev else MEM_HOST, sptr))
        return (ids, dist) if want_dist else ids

    def tag_census(self, query_tags):
        """gbnns_index_tag_census over set_tags()'s table: (allowed, first) [nq] -- the number of rows query word i allows and the lowest of
        them (0xFFFFFFFF: none); the module-level tag_census(T, Q) by the device.  numpy uint32 in -> numpy uint32 out (synchronous); a
        CUDA/ROCm int32 tensor in -> int32 tensors out, enqueued on the current stream."""
        dev = _is_dev(query_tags)
        nq = int(query_tags.shape[0]) if dev else int(np.asarray(query_tags).reshape(-1).shape[0])
        query_tags = _prep_tags(query_tags if dev else np.asarray(query_tags).reshape(-1), dev, nq, "query_tags")
        if dev:
            import torch
            allowed = torch.empty(nq, dtype=torch.int32, device=query_tags.device)
            first = torch.empty(nq, dtype=torch.int32, device=query_tags.device)
            sptr = torch.cuda.current_stream(query_tags.device).cuda_stream
        else:
            allowed, first = np.empty(nq, np.uint32), np.empty(nq, np.uint32)
            sptr = None
        _check(self._lib.gbnns_index_tag_census(self._h, _ptr(query_tags) if nq else None, nq, _ptr(allowed), _ptr(first),
                                                MEM_DEVICE if dev else MEM_HOST, sptr))
        return allowed, first

    def search_auto(self, queries, ef, top_k, query_tags, *, scan_below, mode=MODE_NET, queries_low=None, entry_ids=None,
                    want=("hops", "dist_calc"), flags=0, aux=False, llf=False, hops_bound=50, hash_capacity=0):
        """gbnns_search_tagged_auto: a tagged search that routes itself.  The census of set_tags()'s table gives every query the number of rows
        its word allows; query i takes the exact scan (exact_knn(query_tags=...)'s row) when that number is <= scan_below -- a required
        keyword: 0 sends only the queries that may see nothing to the scan, 2**64 - 1 every query -- and else the tagged walk
        (search(query_tags=..., top_k=...)'s row; flags=FLAG_TAG_BRIDGE: the bridged walk; flags=FLAG_SCAN_GATHER: the scan is exact_knn(gather=True)'s, same rows), entered at the lowest row it may see unless
        entry_ids are given.  Returns search()'s dict plus "top_ids" / "top_dist" [nq x top_k], "allowed" [nq] (the census) and "route" [nq]
        uint8 (0 = walk, 1 = scan); a scan-routed query's "ids" is top_ids[:, 0] and its walk-only outputs are the bad-entry row.  numpy
        in -> numpy out; CUDA/ROCm tensors in -> tensors out, on the current stream; either way the call returns when the work has finished.
        uint8 queries go to the byte form (a byte handle; on a float handle: TypeError)."""
        u8 = _is_u8(queries)
        if u8 and not self.is_bytes:
            raise TypeError("uint8 queries need a byte handle (Index(db=<uint8>)); widen them for a float handle")
        if aux:
            flags |= FLAG_AUX_GRAPH | (FLAG_LLF if llf else 0)
        dev = _is_dev(queries)
        if dev and not queries.is_cuda:
            raise TypeError("queries: a numpy array or a CUDA/ROCm tensor")
        queries = _prep(queries, np.uint8, "uint8") if u8 else _prep(queries, np.float32, "float32")
        if queries_low is not None and _is_dev(queries_low) != dev:
            raise TypeError("queries and queries_low must live in the same memory kind")
        queries_low = _prep(queries_low, np.float32, "float32")
        nq = int(queries.shape[0])
        if queries.ndim != 2 or int(queries.shape[1]) != self.d:
            raise ValueError("query dimension mismatch")
        if query_tags is None:
            raise TypeError("search_auto needs query_tags")
        query_tags = _prep_tags(query_tags, dev, nq, "query_tags")
        res = {}
        if dev:
            import torch
            tdev = queries.device
            if entry_ids is not None:
                entry_ids = _prep(entry_ids, np.uint32, "int32")
            alloc = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=tdev)
            u32, i32, f32, u8t = torch.int32, torch.int32, torch.float32, torch.uint8
            sptr = torch.cuda.current_stream(tdev).cuda_stream
        else:
            entry_ids = None if entry_ids is None else _host(entry_ids, np.uint32)
            alloc = lambda shape, dtype: np.empty(shape, dtype=dtype)
            u32, i32, f32, u8t = np.uint32, np.int32, np.float32, np.uint8
            sptr = None
        n_entries = int(entry_ids.shape[1]) if entry_ids is not None and len(entry_ids.shape) == 2 else 0
        res["ids"] = alloc((nq,), u32)
        a = _SearchArgs(struct_size=C.sizeof(_SearchArgs), mode=mode, ef=ef, k=ef, mem_kind=MEM_DEVICE if dev else MEM_HOST,
                        hash_capacity=hash_capacity, n_q=nq, queries=None if u8 else _ptr(queries), queries_low=_ptr(queries_low),
                        entry_ids=_ptr(entry_ids), out_ids=_ptr(res["ids"]), stream=sptr, flags=flags, hops_bound=hops_bound if aux else 0,
                        n_entries=n_entries)
        kk = max(int(ef), 1)
        for name, field, shape, dtype in (("hops", "out_hops", (nq,), i32), ("dist_calc", "out_dist_calc", (nq,), i32),
                                          ("cand", "out_cand", (nq, kk), u32), ("cand_dist", "out_cand_dist", (nq, kk), f32),
                                          ("q_low", "out_q_low", (nq, self.d_low), f32), ("edges", "out_edges", (nq,), i32)):
            if name in want:
                res[name] = alloc(shape, dtype)
                setattr(a, field, _ptr(res[name]))
        kt = max(int(top_k), 1)   # (a k the call refuses still gets buffers: the refusal is the library's)
        res["top_ids"], res["top_dist"] = alloc((nq, kt), u32), alloc((nq, kt), f32)
        res["allowed"], res["route"] = alloc((nq,), u32), alloc((nq,), u8t)
        _check(self._lib.gbnns_search_tagged_auto(self._h, C.byref(a), _ptr(queries) if u8 else None, _ptr(query_tags), int(top_k), int(scan_below),
                                                  _ptr(res["top_ids"]), _ptr(res["top_dist"]), _ptr(res["allowed"]), _ptr(res["route"])))
        self._in_flight.clear()
        self._last = (queries, queries_low, entry_ids, query_tags, res)
        return res

    # -- profiling -----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        _check(self._lib.gbnns_profile_enable(self._h, int(on)))

    def knob(self, name, value):
        """A diagnostic knob of THIS handle (gbnns_index_knob; include/gbnns.h lists them).  Results never depend on it."""
        _check(self._lib.gbnns_index_knob(self._h, name.encode() if isinstance(name, str) else name, int(value)))

    def knob_get(self, name):
        v = C.c_int(0)
        _check(self._lib.gbnns_index_knob_get(self._h, name.encode() if isinstance(name, str) else name, C.byref(v)))
        return v.value

    def project_last(self):
        """gbnns_index_project_last: the names of the kernel instances this handle's last projection launched, in launch order
        (project_plan's format; () before the first one)."""
        names = C.create_string_buffer(512)
        _check(self._lib.gbnns_index_project_last(self._h, names, 512))
        return tuple(names.value.decode().split("\n")) if names.value else ()

    def order_last(self):
        """gbnns_index_order_last: the permutation the handle's last ordered search call walked its batch in (knobs "order_min" /
        "order_bits"; knob_get("order_last") tells whether the very last call was one), read once the device's work has completed."""
        n = C.c_uint64(0)
        rc = self._lib.gbnns_index_order_last(self._h, None, 0, C.byref(n))   # (the size first: refused, with n set)
        if n.value == 0:
            _check(rc)   # no ordered call yet
        order = np.empty(n.value, np.uint32)
        _check(self._lib.gbnns_index_order_last(self._h, order.ctypes.data, order.shape[0], C.byref(n)))
        return order

    def profile_read(self, reset=True):
        p = Profile()
        p.struct_size = C.sizeof(Profile)   # the callee writes no more than this
        _check(self._lib.gbnns_profile_read(self._h, C.byref(p), int(reset)))
        return p.as_dict()
