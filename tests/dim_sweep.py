"""The row-length sweep: one table of lengths (DIMS) at which every distance routine of the library runs bit for bit against the oracle,
and, per distance form, a small `trace` function that says how often each rung of that form's ladder -- unrolled main loop, shorter
loops, remainder loop, tail rule -- runs at a length.  A plain module: tests/test_dim_sweep_cpu.py proves on the CPU that DIMS puts 0, 1
and >= 2 trips on every rung and a length on each side of every switch between forms; tests/test_gpu_dim_sweep.py runs every entry point
at every length on the device.

The traces restate LOOP BOUNDS only (the `for` headers of walk_common.h, walk_lists.h and knn.hip), no arithmetic.  WHICH form a length
takes is never restated here: the library's plan functions say (gbnns_debug_rerank_plan, gbnns_debug_walk_plan, gbnns_debug_knn_plan) and
the *_form helpers below only read the names they return.  Two switches sit inside device code and have no plan function: the four-lanes-
per-row distance of the run-time-length L2 walk instances (walk_generic.h kQuadRowsMinDim) and the device builder's d <= 128 guard
(graph_api.cpp); their values are named here once and tests/test_dim_sweep_cpu.py reads them back from the sources.
"""
import ctypes
import functools
import re

import numpy as np

import datagen

# 1 .. 40: the lengths at which tests/golden/kats.npz pins the oracle to the compiled reference; then the edges of the ladders
DIMS = tuple(range(1, 41)) + (44, 45, 48, 52, 56, 60, 63, 64, 65, 66, 67, 68, 72, 80, 96, 100, 112, 120, 124, 127, 128, 129, 130, 131, 132, 136, 144, 156,
                              160, 164, 176, 188, 192, 196, 200, 224, 256, 257, 260, 288, 300, 320, 352, 376, 380, 384, 388, 392, 408, 416, 440, 448, 504, 508,
                              512, 576, 640, 960)

N, NQ = 2048, 64                                   # rows and queries of every device test
CAND_STRIDE = 70
COUNTS = (0, 1, 31, 32, 33, 64, 65, 70)            # candidate counts, cycling over the queries: around the 32- and 64-candidate passes
QUAD_ROWS_MIN_DIM = 128                            # walk_generic.h kQuadRowsMinDim
GD_DEVICE_MAX_DIM = 128                            # graph_api.cpp: gd_prune_kernel stages the node's vector in pi_s[132]
GD_DIMS = tuple(range(1, 9)) + tuple(range(124, 133))
NONE = 0xFFFFFFFF


# ---- trip counts of the ladders ----------------------------------------------------------------------------------------------------
def trace_l2_pairs(d, deep):
    """rerank_pairs_core<0, DEEP> (walk_common.h): `pairs` 32-byte steps shared by two lanes -- the DEEP = 24 loop, the 8-loop, the 4-loop,
    the remainder loop's whole pairs, and the even lane's lone 16-byte step at d % 8 == 4."""
    pairs = d >> 3
    deep24 = pairs // 24 if deep == 24 else 0
    k = 24 * deep24
    eight = (pairs - k) // 8
    k += 8 * eight
    four = (pairs - k) // 4
    k += 4 * four
    return {"deep24": deep24, "eight": eight, "four": four, "rest": pairs - k, "odd_step": (d >> 2) & 1}


def trace_dot_pairs(d):
    """rerank_pairs_core<1>: the 8-loop and the remainder loop over the pairs (d % 8 == 0: nothing else)."""
    pairs = d >> 3
    return {"eight": pairs // 8, "rest": pairs % 8}


def trace_l2_lane(d):
    """l2_ordered: 16-byte steps four at a time, then one at a time; `tail` coordinates are never read."""
    steps = d >> 2
    return {"four": steps // 4, "rest": steps % 4, "tail": d % 4}


def trace_dot_lane(d):
    """negdot_ordered: 32-byte iterations, the optional 4-wide step, the masked step and the coordinates it holds."""
    rem = d & 7
    return {"eight": d >> 3, "four_wide": int(rem >= 4), "masked": int(rem % 4 > 0), "masked_lanes": rem % 4}


def trace_byte_pairs(d):
    """rerank_bytes_core: `chunks` 16-byte chunks, pairs of them four at a time, the leftover pairs, the even lane's lone chunk."""
    chunks = d >> 4
    cpairs = chunks >> 1
    return {"four": cpairs // 4, "rest": cpairs % 4, "odd_chunk": chunks & 1}


def trace_quad(d):
    """l2_quad_rows: sixteen steps per round trip, what is left as one masked batch of `masked` steps (0: no batch); `tail` ignored."""
    steps = d >> 2
    return {"sixteen": steps // 16, "masked": steps % 16, "tail": d % 4}


def trace_scan(d, name):
    """The exact scan under the instance `name` (gbnns_debug_knn_plan).  knn_scan_kernel<M, S, QPT, TAG>: S unrolled steps of which `steps`
    hold the row, the other `zero_steps` zeros.  knn_scan_wide_kernel: chunks of eight steps, the last one zero filled by `pad` steps."""
    steps = d >> 2
    m = re.fullmatch(r"knn_scan_kernel<(\d), (\d+), (\d), (true|false)>", name)
    if m:
        S = int(m.group(2))
        assert steps <= S, (d, name)
        return {"kernel": "scan", "S": S, "steps": steps, "zero_steps": S - steps, "tail": d % 4}
    assert re.fullmatch(r"knn_scan_wide_kernel<(\d), (\d+), (true|false)>", name), name
    steps8 = (steps + 7) & ~7
    return {"kernel": "wide", "chunks": steps8 // 8, "pad": steps8 - steps, "tail": d % 4}


# ---- which form a length takes: the library's answer ---------------------------------------------------------------------------------
def rerank_form(g, metric, d, bytes=False):
    """(form, deep, fused) of the stand-alone re-rank: form "pairs" / "chunk_pairs" / "lane", read off gbnns_debug_rerank_plan's kernel name."""
    name, deep, fused = g.rerank_plan(metric, d, bytes)
    form = {"rerank_pair_kernel": "pairs", "rerank_bytes_pair_kernel": "chunk_pairs", "rerank_kernel": "lane", "rerank_bytes_kernel": "lane"}[name.split("<")[0]]
    return form, deep, fused


def rerank_trace(g, metric, d, bytes=False):
    """(form, trace) of the re-rank's distance at a length."""
    form, deep, _ = rerank_form(g, metric, d, bytes)
    if form == "pairs":
        return form, (trace_dot_pairs(d) if metric else trace_l2_pairs(d, deep))
    if form == "chunk_pairs":
        return form, trace_byte_pairs(d)
    return form, (trace_dot_lane(d) if metric else trace_l2_lane(d))


def walk_plan(g, metric, d, n, ell_stride, ef, n_entries=1):
    """gbnns_debug_walk_plan for a PLAIN walk (first pass, the handle knobs "coop" / "late_rows" / speculative rows off, no re-rank room)."""
    name, lds = ctypes.create_string_buffer(128), ctypes.c_uint64()
    rc = g.load_library().gbnns_debug_walk_plan(metric, d, (d + 3) // 4 * 4, n, ell_stride, 0, ef, n_entries, 0, 0, 0, 0, 0, 0, name, 128, ctypes.byref(lds))
    assert rc == 0, (metric, d, n, ell_stride, ef, n_entries, rc)
    return name.value.decode()


def walk_form(metric, d, name):
    """The distance form of a walk instance, from its planned name: "general" (walk_general_kernel: metric_dist at the run-time length),
    "fixed<STEPS>" (a compile-time row length: no ladder), or the run-time-length instances' "lane" / "quad"."""
    if name == "walk_general_kernel":
        return "general"
    m = re.fullmatch(r"(walk_reg_kernel|walk_reg_big_kernel|walk_fast_kernel|walk_bitmap_kernel|walk_bitmap_big_kernel)<(\d), (\d+), .*>", name)
    if m is None:                               # the hot and wide-row families: compile-time lengths only
        m2 = re.fullmatch(r"walk_(reg_wide|coop)_kernel<(\d+), .*>", name)
        assert m2 or name.startswith("walk_hot"), name
        return "fixed%d" % (int(m2.group(2)) if m2 else 8)
    steps = int(m.group(3))
    if steps:
        return "fixed%d" % steps
    return "quad" if metric == 0 and d >= QUAD_ROWS_MIN_DIM else "lane"


def walk_trace(metric, d, form):
    if form == "quad":
        return trace_quad(d)
    if form in ("lane", "general"):
        return trace_dot_lane(d) if metric else trace_l2_lane(d)
    return {"steps": int(form[5:])}


def knn_filter_allowed(g, metric, d, k):
    """Whether the library's shape rule lets the matrix-core filter take a call of the sweep's shape (asked under "knn_filter" = 2)."""
    return g.knn_plan(False, metric, N, NQ, d, k)[0].startswith("knn_filter_kernel")


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def rng_of(*key):
    return np.random.Generator(np.random.PCG64(list((9100,) + key)))


@functools.lru_cache(maxsize=None)
def vectors(d):
    """Full-mantissa rows [N x d], queries [NQ x d], random entry ids (two per query, the first column for one-entry walks).  Read-only."""
    rng = rng_of(d)
    return dict(base=datagen.full_mantissa(rng, N, d), queries=datagen.full_mantissa(rng, NQ, d),
                ent=rng.integers(0, N, size=(NQ, 2)).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def byte_vectors(d):
    """uint8 rows [N x d] (every value, clustered so that distances differ), full-mantissa queries scaled into the rows' range."""
    rng = rng_of(d, 8)
    centres = rng.integers(40, 216, size=(16, d))
    base = np.clip(centres[rng.integers(0, 16, size=N)] + rng.integers(-40, 41, size=(N, d)), 0, 255).astype(np.uint8)
    queries = (datagen.full_mantissa(rng, NQ, d) * np.float32(256.0) + np.float32(128.0)).astype(np.float32)
    return dict(base=base, queries=queries)


@functools.lru_cache(maxsize=None)
def graph(n=N):
    """One random graph over n rows for every length (degrees 2 .. 30: adjacency stride 32)."""
    return datagen.random_graph(rng_of(0, 1, n), n, 2, 30)


ELL_STRIDE = 32


@functools.lru_cache(maxsize=None)
def candidates(lo=0, hi=N, seed=0):
    """cand [NQ x CAND_STRIDE] random rows of [lo, hi) (drawn with replacement), 0xFFFFFFFF beyond count; count cycling through COUNTS."""
    rng = rng_of(1, seed)
    count = np.array([COUNTS[i % len(COUNTS)] for i in range(NQ)], np.int32)
    cand = rng.integers(lo, hi, size=(NQ, CAND_STRIDE)).astype(np.uint32)
    cand[np.arange(CAND_STRIDE)[None, :] >= count[:, None]] = NONE
    return cand, count


def contest_candidates(per, groups, seed):
    """The same lists for a contest table of `groups` groups of `per` rows: query i belongs to group (i // len(COUNTS)) % groups -- every
    group meets every count -- and its candidates are distinct rows of that group -> (cand, count, group of every query)."""
    rng = rng_of(2, seed)
    count = np.array([COUNTS[i % len(COUNTS)] for i in range(NQ)], np.int32)
    qg = (np.arange(NQ) // len(COUNTS)) % groups
    cand = np.full((NQ, CAND_STRIDE), NONE, np.uint32)
    for i in range(NQ):
        cand[i, :count[i]] = qg[i] * per + rng.permutation(per)[:count[i]]
    return cand, count, qg


@functools.lru_cache(maxsize=None)
def byte_contest(d, groups=8, per=128):
    """The equal-distance contest over uint8 rows: the rows of a group are permutations of one vector of bytes and every query is
    c * (1, ..., 1) with c = 11184811 / 2^16 (170.66..., a full mantissa), so in real arithmetic a group's rows are equidistant from its
    query under both metrics and in float32 the distances are a few values apart -- decided by the order of the roundings alone.
    Returns base uint8 [groups * per x d] (group-major) and queries [groups x d]."""
    rng = rng_of(9, d)
    base = np.empty((groups * per, d), np.uint8)
    for grp in range(groups):
        v = rng.integers(0, 256, size=d).astype(np.uint8)
        for r in range(per):
            base[grp * per + r] = v[rng.permutation(d)]
    queries = np.full((groups, d), np.float32(11184811) / np.float32(1 << 16), np.float32)
    return base, queries
