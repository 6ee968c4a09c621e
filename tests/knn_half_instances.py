"""The census of the half-row exact-kNN kernel instances: one static table of gbnns_exact_knn_half calls that, between them, launch every
instance of knn_half_sweep_kernel (16) and every binary16 instance of knn_scan_kernel (12) and knn_scan_wide_kernel (10), and the data
those calls run on.  A plain module, the half-row twin of tests/knn_instances.py: tests/test_knn_half_instances_cpu.py proves on the CPU,
through gbnns_debug_knn_half_plan, that every case takes the instance it names on the path and from the table (in place / a copy) it
states, that the names cover the 38 instances exactly and that no tagged case is vacuous; tests/test_gpu_knn_half_instances.py runs every
case on the device, ids and distance bits against the plain reference of tests/knn_half_util.py.

The classes below restate the launch tables of knn_half.hip (knn_half_sweep_pick) and knn_scan_kernels.h (knn_scan_pick<uint16_t>) by
hand: that is the point.  Shapes are those of tests/knn_instances.py, for its reasons: n = 1 037 with "knn_chunk" = 64, n_q = 128 QB + 37
(QPT for the scans, 128 + 37 for the wide scans), k = 1 and 10 on heaps, 64 or "knn_pool_min_k" = 1 on pools, tagged cases k >= 10.

Row lengths of the sweep, per K step count K ("knn_filter" = 2: the sweep wherever the shape allows):
  16 K - 12   a caller's array with d % 8 == 4: rows that are no whole 16-byte chunks, so a copy is swept (packed)
  16 K - 8    in place, an odd chunk count: lane half h = 1 of the last K step is clamped to the row's last chunk
  16 K        in place, full
One of the three runs on rows x 2^-20 (mostly subnormal halves) and one on rows x 2^13, so every instance meets subnormal operands.
Row lengths of the scans: per class the narrowest and the widest d, for L2 also widest - 2 (d % 4 != 0: the distance leaves the last
columns out and the rows are not 8-byte aligned).  The scan shapes are scans under the default knobs (sets this small are not swept).
"""
import collections
import functools

import numpy as np

import knn_bytes_util as ku
import knn_half_util as hu
import knn_tagged_util as kt

N = 1037
CHUNK = 64
L2, NEG_DOT = 0, 1

# KSTEPS -> QB: query blocks of 32 a wavefront holds (knn_half.hip: K steps of 16 halves)
SWEEP_QB = {1: 4, 2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}
# knn_scan_kernel<METRIC, S, QPT, TAG, half>: (S, QPT, narrowest d by metric, widest d)
SCAN_CLASSES = ((8, 2, (4, 8), 32), (16, 2, (36, 40), 64), (32, 1, (68, 72), 128))
# knn_scan_wide_kernel<METRIC, R, TAG, half>: (metric, R, narrowest d, widest d untagged, widest d tagged) -- the LDS tile holds the rows
# WIDENED, R rows of ((d / 4 + 7) & ~7) * 16 bytes within 160 KB, less 64 bytes in a tagged instance: the float instances' bounds
WIDE_CLASSES = ((L2, 16, 132, 2560, 2528), (L2, 8, 2564, 5120, 5088), (L2, 4, 5124, 8192, 8192),
                (NEG_DOT, 8, 136, 5120, 5088), (NEG_DOT, 4, 5128, 8192, 8192))
# every word of knn_tagged_util.query_words that allows some rows of tag_table but not all
TAG_WORDS = tuple(w for w in kt.QUERY_WORDS if w in [1 << b for b in range(1, 10)])
# queries 0 .. 3 are rows 12 .. 15; rows 14 and 15 are equal (every eighth row duplicates the row before it)
QUERY_ROWS = (12, 13, 14, 15)
DUPLICATE_QUERY = 2


class Case(collections.namedtuple("Case", "metric d n nq k tagged knobs name path packed cls")):
    """path: "filter" (sweep in front of heaps), "pool" (in front of pools) or "scan"; packed: the sweep reads a copy; cls: the magnitude
    class of knn_half_util.SCALE."""
    __slots__ = ()

    @property
    def id(self):
        return "%s_m%d_d%d_nq%d_k%d_%s%s%s" % (self.name[4:self.name.index("_kernel")], self.metric, self.d, self.nq, self.k, self.cls,
                                               "_tag" if self.tagged else "", "_pool" if self.path == "pool" else "")

    @property
    def knob_dict(self):
        return dict(self.knobs)


def _bool(b):
    return "true" if b else "false"


def _table():
    t = []
    heap = (("knn_chunk", CHUNK), ("knn_filter", 2))
    pool1 = heap + (("knn_pool_min_k", 1),)
    # ---- knn_half_sweep_kernel<KSTEPS, QB, TAG> ----
    for ks, qb in SWEEP_QB.items():
        nq, copied, clamped, full = 128 * qb + 37, 16 * ks - 12, 16 * ks - 8, 16 * ks
        for tagged in (False, True):
            name = "knn_half_sweep_kernel<%d, %d, %s>" % (ks, qb, _bool(tagged))
            t.append(Case(L2, copied, N, nq, 10, tagged, heap, name, "filter", True, "subnormal"))
            t.append(Case(L2, clamped, N, nq, 64, tagged, heap, name, "pool", False, "large"))
            t.append(Case(L2, full, N, nq, 10 if tagged else 1, tagged, heap, name, "filter", False, "unit"))
            t.append(Case(L2, copied, N, nq, 10, tagged, pool1, name, "pool", True, "unit"))
    # ---- knn_scan_kernel<METRIC, S, QPT, TAG, half> ----
    for s, qpt, narrow, full in SCAN_CLASSES:
        nq = 128 * qpt + 37
        for metric in (L2, NEG_DOT):
            for tagged in (False, True):
                name = "knn_scan_kernel<%d, %d, %d, %s, half>" % (metric, s, qpt, _bool(tagged))
                t.append(Case(metric, narrow[metric], N, nq, 10, tagged, (), name, "scan", False, "unit"))
                t.append(Case(metric, full, N, nq, 64 if tagged else 1, tagged, (), name, "scan", False, "subnormal"))
                if metric == L2:
                    t.append(Case(metric, full - 2, N, nq, 10, tagged, (), name, "scan", False, "large"))
    # ---- knn_scan_wide_kernel<METRIC, R, TAG, half> ----
    for metric, r, narrow, full, full_tagged in WIDE_CLASSES:
        for tagged in (False, True):
            name = "knn_scan_wide_kernel<%d, %d, %s, half>" % (metric, r, _bool(tagged))
            t.append(Case(metric, narrow, N, 128 + 37, 10, tagged, (), name, "scan", False, "unit"))
            t.append(Case(metric, full_tagged if tagged else full, N, 128 + 37, 10 if tagged else 1, tagged, (), name, "scan", False, "unit"))
    return tuple(t)


CASES = _table()


def instance_names():
    """The 38 names the table must cover, by family."""
    return {
        "sweep": {"knn_half_sweep_kernel<%d, %d, %s>" % (ks, qb, _bool(t)) for ks, qb in SWEEP_QB.items() for t in (0, 1)},
        "scan": {"knn_scan_kernel<%d, %d, %d, %s, half>" % (m, s, qpt, _bool(t)) for s, qpt, _, _ in SCAN_CLASSES for m in (0, 1) for t in (0, 1)},
        "wide": {"knn_scan_wide_kernel<%d, %d, %s, half>" % (m, r, _bool(t)) for m, r, _, _, _ in WIDE_CLASSES for t in (0, 1)},
    }


def queries_per_workgroup(name):
    """128 QB (QPT) of the instance a name stands for."""
    args = name[name.index("<") + 1:-1].split(", ")
    if name.startswith("knn_scan_wide_kernel"):
        return 128
    return 128 * int(args[2] if name.startswith("knn_scan_kernel") else args[1])


@functools.lru_cache(maxsize=4)
def data(d, nq, cls):
    """(rows [N x d] float16, queries [nq x d] float32): knn_half_util.half_rows and standard_normal queries at the rows' scale, the first
    four of them rows themselves (QUERY_ROWS)."""
    rng = np.random.default_rng(8100 + 16 * d + hu.SCALE[cls])
    rows = hu.half_rows(rng, N, d, cls)
    q = rng.standard_normal((nq, d)).astype(hu.F32) * hu.F32(2.0 ** hu.SCALE[cls])
    q[:4] = rows[list(QUERY_ROWS)].astype(hu.F32)
    return rows, q


def tags(case):
    """(T [N], Q [nq]): knn_tagged_util.tag_table and, cycling, its query words that allow some rows but not all."""
    return kt.tag_table(7900, case.n), np.array([TAG_WORDS[i % len(TAG_WORDS)] for i in range(case.nq)], np.uint32)


def named_queries(nq):
    """The queries of a d > 128 case that go against the plain reference: the first four (rows themselves, DUPLICATE_QUERY a duplicated
    one), both sides of the workgroup boundary at query 128, and the last two."""
    return np.array([0, 1, 2, 3, 127, 128, nq - 2, nq - 1])


def expected(case, queries=None):
    """(ids, dist) of the plain reference (knn_half_util): ordered float32 sums on the widened rows, lexsort of (distance, id), tagged cases
    filtered by (T & Q) != 0; queries: a sample of the case's queries, default all."""
    rows, q = data(case.d, case.nq, case.cls)
    sel = np.arange(case.nq) if queries is None else queries
    allowed = None
    if case.tagged:
        T, Q = tags(case)
        allowed = (T[None, :] & Q[sel, None]) != 0
    return hu.knn_of(hu.ordered_dist(rows, np.ascontiguousarray(q[sel]), case.metric), case.k, allowed=allowed)


def expected_oracle(orc, case):
    """(ids, dist) [nq x k] from the CPU oracle over the widened rows (d > 128: every query)."""
    rows, q = data(case.d, case.nq, case.cls)
    if case.tagged:
        T, Q = tags(case)
        return kt.expected(orc, ku.widen(rows), q, T, Q, case.k, case.metric)
    return orc.exact_knn(ku.widen(rows), q, case.k, case.metric, threads=8)
