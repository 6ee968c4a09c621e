"""The census of the exact-scan kernel instances: one static table of exact-kNN calls that, between them, launch every instance of
knn_bytes_sweep_kernel (16), knn_filter_kernel (16), knn_scan_kernel (12) and knn_scan_wide_kernel (10), and the data those calls run
on.  A plain module: tests/test_knn_instances_cpu.py proves on the CPU, through gbnns_debug_knn_plan, that every case takes the instance
it names, that the names cover the 54 instances exactly and that no tagged case is vacuous; tests/test_gpu_knn_instances.py runs every
case on the device, ids and distance bits of every query against the CPU oracle.

A case is what a caller can set -- row type, metric, d, n, n_q, k, tagged or not, the process-wide knobs -- plus the name that must come
out and whether the lists are pools.  The classes below restate the launch tables of knn.hip / knn_bytes.hip by hand: that is the point.

Shapes, the smallest at which an instance can still go wrong:
  n = 1 037     33 blocks of 32 rows, the last of 13; with "knn_chunk" = 64 five chunks and more, none of them the set's length
  n_q           128 QB + 37 for the instance's QB (QPT for the scan kernels): a second workgroup, in it one full block of 32 queries
                and one of 5, and whole blocks of lanes without a query
  d             per K step count the narrowest row (most of the last K step is padding) and the full one; byte L2 also 32 K - 1,
                where d % 4 != 0 and the distance leaves the last three columns out
  k             1 and 10 on heaps; 64, or "knn_pool_min_k" = 1, on pools
Tagged cases take k >= 10 only: their words allow some rows but not all, and the word of rows 0 .. 6 allows fewer than k.
"""
import collections
import functools

import numpy as np

import datagen
import knn_bytes_util as ku
import knn_tagged_util as kt

N = 1037
CHUNK = 64
L2, NEG_DOT = 0, 1

# KSTEPS -> QB: query blocks of 32 a wavefront holds (knn_bytes.hip: K steps of 32 bytes; knn.hip: K steps of 16 floats)
BYTE_QB = {1: 4, 2: 4, 3: 4, 4: 4, 5: 2, 6: 2, 7: 2, 8: 2}
FILTER_QB = {1: 4, 2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}
# knn_scan_kernel<METRIC, S, QPT, TAG>: (S, QPT, narrowest d by metric, widest d)
SCAN_CLASSES = ((8, 2, (4, 8), 32), (16, 2, (36, 40), 64), (32, 1, (68, 72), 128))
# knn_scan_wide_kernel<METRIC, R, TAG>: (metric, R, narrowest d, widest d untagged, widest d tagged) -- R rows of ((d / 4 + 7) & ~7) * 16
# bytes fit 160 KB of LDS, less 64 bytes in a tagged instance
WIDE_CLASSES = ((L2, 16, 132, 2560, 2528), (L2, 8, 2564, 5120, 5088), (L2, 4, 5124, 8192, 8192),
                (NEG_DOT, 8, 136, 5120, 5088), (NEG_DOT, 4, 5128, 8192, 8192))
# every word of knn_tagged_util.query_words that allows some rows of tag_table but not all: bits 1 .. 7 (a share of 2^-b), "the last 40
# rows" and "rows 0 .. 6"
TAG_WORDS = tuple(w for w in kt.QUERY_WORDS if w in [1 << b for b in range(1, 10)])


class Case(collections.namedtuple("Case", "bytes metric d n nq k tagged knobs name pool")):
    __slots__ = ()

    @property
    def id(self):
        return "%s_m%d_d%d_nq%d_k%d%s%s" % (self.name[4:self.name.index("_kernel")], self.metric, self.d, self.nq, self.k,
                                             "_tag" if self.tagged else "", "_pool" if self.pool else "")

    @property
    def knob_dict(self):
        return dict(self.knobs)


def _bool(b):
    return "true" if b else "false"


def _table():
    t = []
    heap, pool1 = (("knn_chunk", CHUNK),), (("knn_chunk", CHUNK), ("knn_pool_min_k", 1))
    # ---- knn_bytes_sweep_kernel<KSTEPS, QB, TAG> ----
    for ks, qb in BYTE_QB.items():
        nq, narrow, full = 128 * qb + 37, 32 * (ks - 1) + 8, 32 * ks
        for tagged in (False, True):
            name = "knn_bytes_sweep_kernel<%d, %d, %s>" % (ks, qb, _bool(tagged))
            t.append(Case(True, L2, narrow, N, nq, 10, tagged, heap, name, False))
            t.append(Case(True, L2, full, N, nq, 64, tagged, heap, name, True))
            t.append(Case(True, L2, full - 1, N, nq, 10 if tagged else 1, tagged, heap, name, False))
            t.append(Case(True, NEG_DOT, full, N, nq, 10, tagged, pool1, name, True))
            if not tagged:
                t.append(Case(True, NEG_DOT, narrow, N, nq, 1, tagged, heap, name, False))
    # ---- knn_filter_kernel<KSTEPS, QB, TAG>: "knn_filter" = 2 ----
    fheap, fpool1 = heap + (("knn_filter", 2),), pool1 + (("knn_filter", 2),)
    for ks, qb in FILTER_QB.items():
        nq, narrow, full = 128 * qb + 37, 16 * (ks - 1) + 4, 16 * ks
        for tagged in (False, True):
            name = "knn_filter_kernel<%d, %d, %s>" % (ks, qb, _bool(tagged))
            t.append(Case(False, L2, narrow, N, nq, 10, tagged, fheap, name, False))
            t.append(Case(False, L2, full, N, nq, 10 if tagged else 1, tagged, fheap, name, False))
            t.append(Case(False, L2, narrow, N, nq, 64, tagged, fheap, name, True))
            if ks in (2, 4, 8):
                t.append(Case(False, L2, full, N, nq, 10, tagged, fpool1, name, True))
    # ---- knn_scan_kernel<METRIC, S, QPT, TAG> ----
    for s, qpt, narrow, full in SCAN_CLASSES:
        nq = 128 * qpt + 37
        for metric in (L2, NEG_DOT):
            for tagged in (False, True):
                name = "knn_scan_kernel<%d, %d, %d, %s>" % (metric, s, qpt, _bool(tagged))
                t.append(Case(False, metric, narrow[metric], N, nq, 10, tagged, (), name, False))
                t.append(Case(False, metric, full, N, nq, 64 if tagged else 1, tagged, (), name, False))
                if metric == L2:   # d % 4 != 0: rows not 16-byte aligned, the distance leaves the last columns out
                    t.append(Case(False, metric, full - 2, N, nq, 10, tagged, (), name, False))
    # ---- knn_scan_wide_kernel<METRIC, R, TAG> ----
    for metric, r, narrow, full, full_tagged in WIDE_CLASSES:
        for tagged in (False, True):
            name = "knn_scan_wide_kernel<%d, %d, %s>" % (metric, r, _bool(tagged))
            t.append(Case(False, metric, narrow, N, 128 + 37, 10, tagged, (), name, False))
            t.append(Case(False, metric, full_tagged if tagged else full, N, 128 + 37, 10 if tagged else 1, tagged, (), name, False))
    return tuple(t)


CASES = _table()


def instance_names():
    """The 54 names the table must cover, by family."""
    return {
        "bytes": {"knn_bytes_sweep_kernel<%d, %d, %s>" % (ks, qb, _bool(t)) for ks, qb in BYTE_QB.items() for t in (0, 1)},
        "filter": {"knn_filter_kernel<%d, %d, %s>" % (ks, qb, _bool(t)) for ks, qb in FILTER_QB.items() for t in (0, 1)},
        "scan": {"knn_scan_kernel<%d, %d, %d, %s>" % (m, s, qpt, _bool(t)) for s, qpt, _, _ in SCAN_CLASSES for m in (0, 1) for t in (0, 1)},
        "wide": {"knn_scan_wide_kernel<%d, %d, %s>" % (m, r, _bool(t)) for m, r, _, _, _ in WIDE_CLASSES for t in (0, 1)},
    }


def queries_per_workgroup(name):
    """128 QB (QPT) of the instance a name stands for."""
    args = name[name.index("<") + 1:-1].split(", ")
    if name.startswith("knn_scan_wide_kernel"):
        return 128
    return 128 * int(args[2] if name.startswith("knn_scan_kernel") else args[1])


@functools.lru_cache(maxsize=4)
def data(bytes, d, nq):
    """(base [N x d], queries [nq x d]): knn_bytes_util.random_bytes (asymmetric: rows 0 / 1 all 0 / all 255), or datagen.Case's float rows."""
    if bytes:
        return ku.random_bytes(7100 + d, N, d), ku.random_bytes(7400 + d + nq, nq, d)
    c = datagen.Case("knn_instances", 7700 + d, N, nq, d, 4, 8)
    return c.base, c.queries


def tags(case):
    """(T [N], Q [nq]): knn_tagged_util.tag_table and, cycling, its query words that allow some rows but not all."""
    return kt.tag_table(7900, case.n), np.array([TAG_WORDS[i % len(TAG_WORDS)] for i in range(case.nq)], np.uint32)


def expected(orc, case):
    """(ids, dist) [nq x k] from the CPU oracle over the widened arrays."""
    base, q = data(case.bytes, case.d, case.nq)
    if case.tagged:
        T, Q = tags(case)
        return kt.expected(orc, base, q, T, Q, case.k, case.metric)
    return orc.exact_knn(ku.widen(base), ku.widen(q), case.k, case.metric, threads=8)
