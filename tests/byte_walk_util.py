"""What tests/test_byte_walk_cpu.py and tests/test_gpu_byte_walk.py share: the fixtures and expected values of the byte-row PLAIN walk
(MODE_PLAIN with FLAG_BYTE_WALK on a byte handle).

The contract under test: every output equals, bit for bit, what the same call without the flag returns on the handle created with
db = float32(db_bytes).  Every expected value is therefore the CPU oracle's walk over `bu.wide(base)` in the original space -- the unchanged
oracle decides everything, nothing takes a tolerance -- and every GPU case is compared byte for byte with the float handle as well.

Two kinds of fixture, all of 2 048 rows and 96 queries:
  * the byte contest (byte_rows_util.index_data): its rows, original-space queries, disconnected 256-row groups and entry points as they
    are.  In real arithmetic every row of a group is equidistant from the group's query; only the order of the roundings separates them,
    and between the exact copies nothing does (the integer form ties every row of a group: the id decides);
  * random bytes: rows drawn from 0 .. 255 (every row holds 0, 127, 128 and 255 in its first four columns, in an order that rotates with
    the row), each query a base row plus N(0, 20) noise plus a k / 2^14 jitter, clipped to [0, 255]; a one-pass graph
    (random_graph(rng, n, 2, 30)) and a two-pass graph (random_graph(rng, n, 34, 60)); random entry points, query 0 entering at row n - 1 so
    that nothing behind the last row's padding can enter a sum.  Walks differ per query and every list holds distinct distances.
"""
import functools

import numpy as np

import byte_rows_util as bu
import datagen
import oracle as orc_mod
import topk_util as tu

N, NQ, NONE = bu.N, 96, bu.NONE
MARKS = bu.MARKS
BEAMS = (8, 64, 100, 200)
# (metric, d, integer) of the contest fixtures the tests use
CONTESTS = [(0, 128, False), (0, 128, True), (0, 48, False), (0, 100, False), (1, 45, False), (1, 128, False)]
RANDOM_DIMS = (128, 48, 100)
WANT = ("hops", "dist_calc", "cand", "cand_dist", "edges")


def contest(metric, d, integer=False):
    return bu.index_data(metric, d, 32, integer=integer)


@functools.lru_cache(maxsize=None)
def random_bytes(d):
    """dict: base uint8 [N x d], wide, queries [NQ x d] float32, graphs {1: (off, nbr) one-pass, 2: two-pass}, ent [NQ], db_low (any: a byte
    handle needs one; the PLAIN walk never reads it)."""
    rng = tu.rng_of(777 + d)
    base = rng.integers(0, 256, size=(N, d)).astype(np.uint8)
    for j in range(4):
        base[:, j] = np.array(MARKS, np.uint8)[(np.arange(N) + j) % 4]
    pick = rng.integers(0, N, size=NQ)
    noise = rng.normal(0.0, 20.0, size=(NQ, d))
    jitter = rng.integers(0, 1 << 14, size=(NQ, d)) / float(1 << 14)
    queries = np.clip(base[pick].astype(np.float64) + noise + jitter, 0.0, 255.0).astype(np.float32)
    graphs = {1: datagen.random_graph(rng, N, 2, 30), 2: datagen.random_graph(rng, N, 34, 60)}
    ent = rng.integers(0, N, size=NQ).astype(np.uint32)
    ent[0] = N - 1
    db_low = datagen.full_mantissa(rng, N, 32)
    return dict(base=base, wide=bu.wide(base), queries=np.ascontiguousarray(queries), graphs=graphs, ent=ent, db_low=db_low)


_WALKS = {}


def expected(orc, key, queries, wide, off, nbr, ef, k, ent, metric=0, **kw):
    """The contract's outputs of a PLAIN search: the oracle's walk over the widened table (ids [nq x k] pop order, dists, count, hops,
    dist_calc) plus `want`, the answer -- the k-th best, i.e. the first id popped (0xFFFFFFFF for an empty list).  Computed once per key."""
    kk = (key, ef, k, metric, tuple(sorted((n, str(v)) for n, v in kw.items() if n != "aux")), "aux" in kw)
    if kk not in _WALKS:
        w = orc.walk(queries, wide, off, nbr, ef, k=k, entries=ent, metric=metric, threads=8, **kw)
        w["want"] = np.where(w["count"] > 0, w["ids"][:, 0], NONE).astype(np.uint32)
        if np.asarray(ent).ndim == 1:  # (Oracle.search_batch takes one entry point per query: there the reference's own PLAIN answer decides)
            s = orc.search_batch(orc_mod.MODE_PLAIN, queries, wide, off, nbr, ef, k=k, entries=ent, metric=metric, threads=8, **kw)
            assert np.array_equal(s["ids"], w["want"]) and np.array_equal(s["hops"], w["hops"]) and np.array_equal(s["dist_calc"], w["dist_calc"])
        for v in w.values():
            v.setflags(write=False)
        _WALKS[kk] = w
    return _WALKS[kk]


def against(r, w):
    """What differs between a search result and the expected values ([] = nothing)."""
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % bu.rows_that_differ(r["cand"], w["ids"]))
    got, exp = np.ascontiguousarray(r["cand_dist"], np.float32).view(np.uint32), np.ascontiguousarray(w["dists"], np.float32).view(np.uint32)
    if not np.array_equal(got, exp):
        bad.append("distance bits (%d differ)" % int((got != exp).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc")
    if not np.array_equal(r["ids"], w["want"]):
        bad.append("answers (%d differ)" % int((np.asarray(r["ids"]) != w["want"]).sum()))
    return bad


def same_bytes(a, b, names=("ids",) + WANT):
    """Names of the outputs that are not byte-identical."""
    return [n for n in names if np.asarray(a[n]).tobytes() != np.asarray(b[n]).tobytes()]


def l2_bits_lanes_never_meet(rows, q):
    """[len(rows)] uint32: float32 L2 bit patterns of `rows` (float32 [m x d]) from q in an order the kernels must NOT use -- the two lanes of
    a pair never exchange sums: the even 16-coordinate chunks go into one set of four running sums, the odd chunks into another, the two sets
    are added at the end and closed as ((s0 + s1) + s2) + s3.  The d % 4 tail is ignored, as in the reference."""
    rows, q = np.asarray(rows, np.float32), np.asarray(q, np.float32)
    steps = rows.shape[1] // 4
    s = np.zeros((2, len(rows), 4), np.float32)
    for t in range(steps):
        e = (rows[:, 4 * t:4 * t + 4] - q[None, 4 * t:4 * t + 4]).astype(np.float32)
        which = (t // 4) % 2
        s[which] = (s[which] + (e * e).astype(np.float32)).astype(np.float32)
    m = (s[0] + s[1]).astype(np.float32)
    return ((((m[:, 0] + m[:, 1]).astype(np.float32) + m[:, 2]).astype(np.float32) + m[:, 3]).astype(np.float32)).view(np.uint32)


def oracle_l2_bits(orc, wide, q):
    return np.array([np.float32(orc.l2(wide[j], q)).view(np.uint32) for j in range(len(wide))], np.uint32)
