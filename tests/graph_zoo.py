"""The graph as a test axis: seeded topologies that hold what datagen.random_graph excludes by construction -- rows without
neighbours, full adjacency rows (no padding slot), ids that repeat inside a row, self loops, components smaller than the beam, hops that
find nothing fresh and paths on which every hop finds exactly one id -- and a sixth, small components with repeated ids.  A plain
module: tests/test_graph_zoo_cpu.py proves on the CPU that every graph holds what it claims and that the oracle is a valid expectation on
it (the compiled reference agrees byte for byte); tests/test_gpu_graph_zoo.py runs the census of tests/walk_instances.py and the feature
instances over it on a device.

`cap` (32, 64, 96) is the largest raw row length of the CSR.  The padded adjacency's stride is round_up(cap, 16), the stride
walk_instances.ELL_STRIDE expects of the degree classes 30 / 60 / 90: the planned kernel name of every census case is the zoo's too.
Every result is cached per key and shared: treat as read-only.
"""
import functools

import numpy as np

import walk_instances as wi

NQ = wi.NQ
TOPOLOGIES = ("ragged", "path", "islands", "star", "funnel", "knots")
CAPS = (32, 64, 96)
DEG_OF_CAP = {cap: deg for deg, cap in wi.ELL_STRIDE.items()}   # 32 -> 30, 64 -> 60, 96 -> 90: the census's degree class of a cap
DEAD_ENTRIES = 8         # queries 1 .. 8 enter at a row without neighbours where the topology has such rows
NONE = 0xFFFFFFFF


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list((7200,) + tuple(int(k) for k in key))))


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    nbr = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(nbr, np.uint32)


def rows(off, nbr):
    """The adjacency rows of a CSR as a list of arrays (views)."""
    o = np.asarray(off).astype(np.int64)
    return [nbr[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _distinct(rng, n, k, avoid):
    """k distinct ids of 0 .. n-1 other than `avoid`, in random order."""
    c = rng.permutation(n)[:k + 1]
    return c[c != avoid][:k].astype(np.uint32)


def _ragged(rng, n, cap):
    lists = []
    kind = rng.integers(0, 5, size=n)
    for i in range(n):
        k = (0, 1, cap - 1, cap, int(rng.integers(0, cap + 1)))[int(kind[i])]
        if i == n - 1:
            k = cap                                   # (row n - 1, where query 0 enters, is a full row of distinct ids whatever the draw)
        row = _distinct(rng, n, k, i)
        if i % 7 == 0 and k > 0:
            row[int(rng.integers(0, k))] = i          # a self loop at a random slot
        if i % 5 == 0 and k >= 4:
            row[k // 2] = row[0]                      # cap 32: inside the 32-slot pass; a 64-slot row: slot 0 against slot 32
            row[k - 1] = row[1]                       # rows beyond 32 slots: across passes
        lists.append(row)
    return lists


def _path(rng, n, cap):
    lists = [np.array([(i + 1) % n], np.uint32) for i in range(n)]
    lists[n - 1] = _distinct(rng, n, cap, n - 1)
    return lists


def island_sizes(cap):
    return (1, 2, 5, 33, 65, cap + 1)


def island_of(n, cap):
    """(start, size) of the island every row belongs to, as two [n] arrays: cliques of island_sizes(cap) in rotation, the last one cut at n."""
    start, size = np.empty(n, np.int64), np.empty(n, np.int64)
    s, t, sizes = 0, 0, island_sizes(cap)
    while s < n:
        e = min(n, s + sizes[t % len(sizes)])
        start[s:e], size[s:e] = s, e - s
        s, t = e, t + 1
    return start, size


def _islands(rng, n, cap):
    start, size = island_of(n, cap)
    lists = []
    for i in range(n):
        m = np.arange(start[i], start[i] + size[i])
        lists.append(m[m != i][:cap].astype(np.uint32))
    return lists


def _knots(rng, n, cap):
    lists = []
    for r in _islands(rng, n, cap):
        lists.append(np.concatenate([r[:cap - 1], r[:1]]).astype(np.uint32) if len(r) >= 3 else r)
    return lists


def _star(rng, n, cap):
    lists = []
    for i in range(n):
        hub, j = i - i % (cap + 1), i % (cap + 1)
        if j == 0:
            lists.append(np.arange(hub + 1, min(hub + cap + 1, n), dtype=np.uint32))
        else:
            lists.append(np.array([hub] if j % 2 else [], np.uint32))
    return lists


def _funnel(rng, n, cap):
    row = rng.permutation(n)[:cap].astype(np.uint32)
    return [row] * n


_BUILD = {"ragged": _ragged, "path": _path, "islands": _islands, "star": _star, "funnel": _funnel, "knots": _knots}


@functools.lru_cache(maxsize=None)
def zoo(topology, n, cap, seed_key=()):
    """(off, nbr) of the topology over n rows whose longest raw row has `cap` entries.
    ragged   row lengths drawn from {0, 1, cap - 1, cap, uniform 0 .. cap}; every seventh non-empty row holds its own id at a random slot;
             every fifth row of at least 4 entries repeats its first id in the middle and its second id in the last slot; row n - 1 is
             a full row of distinct ids.
    path     row i = [i + 1 mod n]; row n - 1 holds cap distinct random ids (it alone fixes the stride class).
    islands  disjoint cliques of 1, 2, 5, 33, 65, cap + 1 rows in rotation; a member's row is the other members in id order, cut to cap.
    star     a hub every cap + 1 rows, its row the cap leaves behind it; a leaf with an odd place points back to the hub, one with an
             even place has an empty row.
    funnel   every row is the same cap distinct ids.
    knots    (beyond the five the census was asked on) islands whose rows of three or more entries are cut to cap - 1 and end with their
             first id again: small components AND repeated ids, so that a short list's out_edges tells raw degrees from kept ones."""
    assert topology in TOPOLOGIES and cap in CAPS and n > 2 * (cap + 1)
    return _csr(_BUILD[topology](_rng(TOPOLOGIES.index(topology), n, cap, *seed_key), n, cap))


def dedup(off, nbr):
    """build_ell's de-duplication restated: every row keeps the first occurrence of each id, in order."""
    out = []
    for r in rows(off, nbr):
        _, first = np.unique(r, return_index=True)
        out.append(r[np.sort(first)])
    return _csr(out)


@functools.lru_cache(maxsize=None)
def zoo_dedup(topology, n, cap, seed_key=()):
    return dedup(*zoo(topology, n, cap, seed_key))


def aux_overlapping(off, nbr, rng=None):
    """An auxiliary graph that repeats ids of the main one: an odd row holds the first three ids of its main row reversed, then two random
    ids; even rows are empty.  At most 5 entries a row: walk_instances.AUX_STRIDE slots."""
    rng = _rng(len(off), len(nbr)) if rng is None else rng
    n = len(off) - 1
    out = []
    for i, r in enumerate(rows(off, nbr)):
        extra = rng.integers(0, n, size=2).astype(np.uint32)
        out.append(np.concatenate([r[:3][::-1], extra]).astype(np.uint32) if i % 2 else np.zeros(0, np.uint32))
    return _csr(out)


@functools.lru_cache(maxsize=None)
def zoo_aux(topology, n, cap, seed_key=()):
    return aux_overlapping(*zoo(topology, n, cap, seed_key), rng=_rng(99, TOPOLOGIES.index(topology), n, cap, *seed_key))


@functools.lru_cache(maxsize=None)
def entries(topology, n, cap, seed_key=(), nq=NQ):
    """One entry id per query: random rows; query 0 enters at row n - 1; queries 1 .. DEAD_ENTRIES enter at rows without neighbours where
    the topology has any (ragged, islands, star, knots)."""
    rng = _rng(98, TOPOLOGIES.index(topology), n, cap, *seed_key)
    ent = rng.integers(0, n, size=nq).astype(np.uint32)
    off, _ = zoo(topology, n, cap, seed_key)
    empty = np.flatnonzero(np.diff(off.astype(np.int64)) == 0)
    if len(empty):
        ent[1:1 + DEAD_ENTRIES] = rng.choice(empty, DEAD_ENTRIES, replace=False)
    ent[0] = n - 1
    return ent


def seed_of(case):
    """The zoo's seed key of a census case: one graph per (metric, walked dimension), as in walk_instances.graph."""
    return (case.metric, case.dim)


def case_graph(case, topology):
    """(off, nbr, entries) a census case walks on this topology."""
    cap = wi.ELL_STRIDE[case.deg]
    return zoo(topology, case.n, cap, seed_of(case)) + (entries(topology, case.n, cap, seed_of(case)),)


_WALKS = {}


def oracle_walk(orc, case, topology):
    """walk_instances.oracle_walk on the zoo: (walk, re-ranked answers) of the oracle over the case's vectors, the topology's graph and
    entry ids and -- a case with an auxiliary graph -- zoo_aux, computed once per (data, graph, auxiliary graph, beam, topology)."""
    key = case.graph_key + (case.aux, case.ef, topology)
    if key not in _WALKS:
        v = wi.vectors(case.metric, case.dim, case.n)
        off, nbr, ent = case_graph(case, topology)
        kw = dict(aux=zoo_aux(topology, case.n, wi.ELL_STRIDE[case.deg], seed_of(case)), llf=True, hops_bound=50) if case.aux else {}
        w = orc.walk(v["q_low"], v["db_low"], off, nbr, case.ef, entries=ent, metric=case.metric, threads=8, **kw)
        _WALKS[key] = (w, orc.rerank(v["queries"], w["ids"], w["count"], v["base"], metric=case.metric, threads=8))
    return _WALKS[key]


def over(orc, case, topology="ragged"):
    """Queries of a census case with a small visited set whose oracle walk computes more distances than that set holds: whatever the
    kernel, the first pass hands at least these over (a set of hash_capacity entries cannot hold more ids)."""
    assert case.hash_capacity
    return int((oracle_walk(orc, case, topology)[0]["dist_calc"] > case.hash_capacity).sum())


def expected_edges(topology, n, cap, seed_key, ent, hops, aux=False):
    """(edges [nq] int64, mask [nq] bool): where every node a query can expand has the same degree, out_edges = degree x hops, from the
    oracle's hops alone.  Covered: funnel (every row has cap ids); islands (a walk never leaves its island, whose rows all hold
    min(size - 1, cap) ids); path queries that never expand row n - 1 (a walk from e expands e, e + 1, ... in turn, one id a row: row
    n - 1 stays unexpanded when e + hops < n).  None of these rows repeats an id, so raw and de-duplicated degrees are the same.  A walk
    that also expands auxiliary rows (aux) is not covered: those rows have other lengths and lead off the path."""
    ent, hops = np.asarray(ent).astype(np.int64), np.asarray(hops).astype(np.int64)
    if aux:
        return np.zeros(len(ent), np.int64), np.zeros(len(ent), bool)
    if topology == "funnel":
        return cap * hops, np.ones(len(ent), bool)
    if topology == "islands":
        _, size = island_of(n, cap)
        return np.minimum(size[ent] - 1, cap) * hops, np.ones(len(ent), bool)
    if topology == "path":
        return hops.copy(), ent + hops < n
    return np.zeros(len(ent), np.int64), np.zeros(len(ent), bool)


@functools.lru_cache(maxsize=None)
def kept_degrees(topology, n, cap, seed_key=(), aux=False):
    """[n] int64: the entries every row keeps in the padded adjacency (repeats inside a row dropped); aux: plus those of zoo_aux's row."""
    deg = np.diff(zoo_dedup(topology, n, cap, seed_key)[0].astype(np.int64))
    return deg + np.diff(dedup(*zoo_aux(topology, n, cap, seed_key))[0].astype(np.int64)) if aux else deg


def short_list_edges(deg, w, ef, hops_bound=None):
    """(edges [nq] int64, mask [nq] bool) from a single-entry oracle walk w on any graph: a list that never fills (count < ef) evicts
    nothing and every candidate passes the stop test, so the walk expands every id it returns exactly once (hops == count) and out_edges
    is the sum of their degrees deg [n] -- kept_degrees: the DE-DUPLICATED rows are what the padded adjacency holds.  With an auxiliary
    graph walked without LLF (deg: both rows' entries) only the queries whose every hop reads it are covered: hops <= hops_bound."""
    count, hops = np.asarray(w["count"]).astype(np.int64), np.asarray(w["hops"]).astype(np.int64)
    mask = count < ef
    if hops_bound is not None:
        mask &= hops <= hops_bound
    assert (hops[mask] == count[mask]).all()
    edges = np.array([deg[w["ids"][i, :count[i]].astype(np.int64)].sum() for i in range(len(count))], np.int64)
    return edges, mask


@functools.lru_cache(maxsize=None)
def byte_vectors(n, d=128):
    """The byte handle's original space: rows uint8 [n x d], float queries [NQ x d] (a row plus noise and a k / 2^14 jitter, clipped to
    0 .. 255) and the same queries rounded to bytes."""
    rng = _rng(96, n, d)
    base = rng.integers(0, 256, size=(n, d)).astype(np.uint8)
    q = base[rng.integers(0, n, size=NQ)].astype(np.float64) + rng.normal(0.0, 20.0, size=(NQ, d)) + rng.integers(0, 1 << 14, size=(NQ, d)) / float(1 << 14)
    queries = np.ascontiguousarray(np.clip(q, 0.0, 255.0).astype(np.float32))
    queries_u8 = np.ascontiguousarray(np.clip(np.rint(queries), 0, 255).astype(np.uint8))
    return dict(base=base, wide=np.ascontiguousarray(base.astype(np.float32)), queries=queries, queries_u8=queries_u8,
                queries_u8_wide=np.ascontiguousarray(queries_u8.astype(np.float32)))


DISALLOWED = (10, 40)    # queries of a tagged batch (both carry the word 0x01) that enter at a row their word does not allow


def tagged_entries(ent, T, Q):
    """entries() moved for a tagged batch: query i enters at the first row from ent[i] on (cyclically) that its word allows -- a third of
    the batch carries the word that allows every row and keeps its entry, dead ends included --, the DISALLOWED queries at the first row
    their word does NOT allow."""
    n, out = len(T), np.asarray(ent, np.uint32).copy()
    for i in range(len(out)):
        ok = (T & Q[i]) != 0
        if i in DISALLOWED:
            ok = ~ok
        ring = (int(out[i]) + np.arange(n)) % n
        out[i] = ring[np.flatnonzero(ok[ring])[0]]
    return out


ENTRY_KINDS = ("same", "first", "dead")
# (auxiliary graph, LLF, hops_bound) of the two-entry searches: alone, zoo_aux under AUX_GRAPH | LLF, and hops_bound 3 without LLF; the
# last run (every hop reads both rows) is there for the edge count of the single-entry searches
ENTRY_RUNS = ((False, False, 50), (True, True, 50), (True, False, 3), (True, False, 50))


@functools.lru_cache(maxsize=None)
def two_entries(topology, n, cap, seed_key=(), kind="same"):
    """[NQ x 2] entry ids over entries()'s e: "same" [e, e]; "first" [e, the first id of e's row] (e again where the row is empty);
    "dead" [a row without neighbours, e] (ragged, islands, star)."""
    e = entries(topology, n, cap, seed_key)
    off, nbr = zoo(topology, n, cap, seed_key)
    o = off.astype(np.int64)
    if kind == "same":
        other = e.copy()
    elif kind == "first":
        other = np.where(o[e.astype(np.int64) + 1] > o[e], nbr[np.minimum(o[e], len(nbr) - 1)], e).astype(np.uint32)
    else:
        empty = np.flatnonzero(np.diff(o) == 0)
        dead = _rng(97, TOPOLOGIES.index(topology), n, cap, *seed_key).choice(empty, len(e)).astype(np.uint32)
        return np.ascontiguousarray(np.stack([dead, e], axis=1))
    return np.ascontiguousarray(np.stack([e, other], axis=1))
