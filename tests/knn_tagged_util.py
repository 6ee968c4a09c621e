"""Shared by tests/test_knn_tagged_cpu.py and tests/test_gpu_knn_tagged.py: the tag fixtures of gbnns_exact_knn_tagged /
gbnns_exact_knn_bytes_tagged / gbnns_index_exact_knn and their expected values.  Row j is allowed for query i when (T[j] & Q[i]) != 0; the
expected answer of a case is the unchanged CPU oracle's exact_knn over the allowed rows of each distinct query word, mapped back to the
original ids.  Nothing here has a tolerance."""
import numpy as np

import datagen
import knn_bytes_util as ku

NONE_ID = ku.NONE_ID
ALL = 0xFFFFFFFF
NS, NQS = (5, 1037, 6000), (1, 70, 300)
N_MAX, NQ_MAX, K_MAX = 6000, 300, 200
FRACTION_BITS = range(8)   # bit b of T[j] is set with probability 2^-b
LATE_BIT, FEW_BIT = 8, 9   # the last 40 rows only / rows 0 .. 6 only
QUERY_WORDS = [1 << b for b in range(10)] + [0, ALL, 0x3]


def tag_table(seed, n):
    """T [n] uint32: bit b = 0 .. 7 set with probability 2^-b (bit 0: every row); bit 8 on the last 40 rows only -- a query of that word
    finds nothing until the last chunk, so its threshold stays at "everything passes" until then; bit 9 on rows 0 .. 6 only -- fewer than
    k rows allowed, hence padding."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, np.uint32)
    for b in FRACTION_BITS:
        t |= (rng.random(n) < 2.0 ** -b).astype(np.uint32) << np.uint32(b)
    t[max(0, n - 40):] |= np.uint32(1 << LATE_BIT)
    t[:7] |= np.uint32(1 << FEW_BIT)
    return t


def query_words(nq):
    """Q [nq]: cycles through 1 << b for the ten bits, 0 (nothing allowed), all ones (everything) and 0x3."""
    return np.array([QUERY_WORDS[i % len(QUERY_WORDS)] for i in range(nq)], np.uint32)


def lane_map_tags(n, nq):
    """T[j] = 1 << (j % 32), Q[i] = 1 << (i % 32): exactly one row of every block of 32 is allowed, at a position that differs per query --
    a wrong row <-> register map in a sweep kernel's tag test gives a wrong id."""
    return (np.uint32(1) << (np.arange(n, dtype=np.uint32) % 32)).astype(np.uint32), \
           (np.uint32(1) << (np.arange(nq, dtype=np.uint32) % 32)).astype(np.uint32)


def expected(orc, base, queries, T, Q, k, metric, self_offset=-1):
    """(ids uint32, dist float32) [nq x k] from the oracle: per distinct word w of Q the oracle's (k + 1)-lists of the queries with that
    word over base[nonzero(T & w)], ids mapped back through the row list, the self row (i + self_offset, allowed or not) dropped, cut to
    k, padded with 0xFFFFFFFF / +inf.  base / queries: float32, or uint8 (widened: the byte call's promise is the float answer)."""
    base, queries = ku.widen(base), ku.widen(queries)
    nq = queries.shape[0]
    ids = np.full((nq, k), NONE_ID, np.uint32)
    dist = np.full((nq, k), np.inf, np.float32)
    for w in np.unique(Q):
        rows = np.nonzero(T & w)[0]
        qs = np.nonzero(Q == w)[0]
        if rows.size == 0:
            continue
        oi, od = orc.exact_knn(np.ascontiguousarray(base[rows]), np.ascontiguousarray(queries[qs]), k + 1, metric, threads=8)
        found = oi != NONE_ID
        mapped = np.where(found, rows[np.where(found, oi, 0)], NONE_ID).astype(np.uint32)
        for j, i in enumerate(qs):
            keep = found[j]
            if self_offset >= 0:
                keep = keep & (mapped[j] != i + self_offset)
            m, dd = mapped[j][keep][:k], od[j][keep][:k]
            ids[i, :m.size] = m
            dist[i, :m.size] = dd
    return ids, dist


def expected_int(base, queries, T, Q, k, metric, self_offset=-1):
    """The same from plain numpy on bytes: np.lexsort((id, distance)) over the int64 distances of the allowed rows of each query."""
    d = ku.int_dist(base, queries, metric)
    nq, n = d.shape
    ids = np.full((nq, k), NONE_ID, np.uint32)
    dist = np.full((nq, k), np.inf, np.float32)
    rows = np.arange(n)
    for i in range(nq):
        ok = (T & Q[i]) != 0
        if self_offset >= 0 and i + self_offset < n:
            ok[i + self_offset] = False
        cand = rows[ok]
        order = cand[np.lexsort((cand, d[i, cand]))][:k]
        ids[i, :order.size] = order
        dist[i, :order.size] = d[i, order].astype(np.float32) + np.float32(0.0)
    return ids, dist


def byte_case(metric, d):
    """The shape fixture of the byte tests: knn_bytes_util.random_bytes base [6 000 x d] and queries [300 x d] (queries 0 / 1 all 255 / all 0)."""
    base, q = ku.random_bytes(300 + d + metric, N_MAX, d), ku.random_bytes(400 + d + metric, NQ_MAX, d)
    q[0], q[1] = 255, 0
    return base, q


def float_case(metric, d):
    """The shape fixture of the float tests: datagen.full_mantissa rows (about 22 significant bits a coordinate: every partial sum rounds)."""
    rng = np.random.default_rng(500 + d + metric)
    return datagen.full_mantissa(rng, N_MAX, d), datagen.full_mantissa(rng, NQ_MAX, d)


def tie_case():
    """test_gpu_knn_bytes.test_ties' data -- bytes in {0, 1, 2}, every row three times, 1 020 rows, the first 200 as queries -- and tags that
    disallow the LOWEST id of every triple of equal rows (tag word 2; the others 1; every query asks for 1): at every rank the allowed row
    reported has a disallowed twin of the same distance and a lower id."""
    d = 16
    rows = np.random.default_rng(7).integers(0, 3, (340, d), dtype=np.uint8)
    perm = np.random.default_rng(8).permutation(1020)
    base = np.ascontiguousarray(np.repeat(rows, 3, axis=0)[perm])
    group = (np.arange(1020) // 3)[perm]   # which of the 340 rows base row j is a copy of
    first = np.full(340, 1020, np.int64)
    np.minimum.at(first, group, np.arange(1020))
    T = np.ones(1020, np.uint32)
    T[first] = 2
    q = base[:200].copy()
    return base, q, T, np.ones(200, np.uint32), group


def overflow_case(k):
    """test_gpu_knn_bytes.test_overflowing_chunks_are_swept_again's data (rows sorted farthest first from query 0, the centre: every row of
    every chunk is a hit for it) with bit 1 of tag_table -- half the rows -- as every query's filter."""
    d, n, nq = 32, 12000, 40
    rng = np.random.default_rng(k)
    centre = np.full(d, 128, np.uint8)
    base = rng.integers(0, 256, (n, d), dtype=np.uint8)
    dist = ((base.astype(np.int64) - 128) ** 2).sum(1)
    base = np.ascontiguousarray(base[np.lexsort((np.arange(n), -dist))])
    q = np.tile(centre, (nq, 1))
    q[1:, 0] += rng.integers(0, 2, nq - 1).astype(np.uint8)
    return base, q, tag_table(600 + k, n), np.full(nq, 1 << 1, np.uint32)


def same(got, want, what):
    gi, gd = got
    wi, wd = want
    gi, gd = np.asarray(gi).view(np.uint32), np.asarray(gd)
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.nonzero((gi != wi).any(1) | (ku.bits(gd) != ku.bits(wd)).any(1))[0]
    assert bad.size == 0, (what, "queries that differ:", bad[:8], gi[bad[0]][:8], wi[bad[0]][:8], gd[bad[0]][:8], wd[bad[0]][:8])
