"""What tests/test_tags_cpu.py and tests/test_gpu_tags.py share: the tag words, the fixtures, the expected values and the expected kernel
names of gbnns_search_tagged.

The contract under test: row j is allowed for query i when (T[j] & Q[i]) != 0, and a tagged search of query i is the reference's search
on G'(i) -- the graph whose adjacency rows keep the allowed neighbours only, in their order (gbnns_dim_red_amd.cut_graph).  Every expected
value is the CPU oracle's on that CSR, one oracle call per distinct value of Q; a query whose entry row it may not see (or whose entry id
is outside the index) gets the bad-entry row.  Nothing takes a tolerance.
"""
import functools

import numpy as np

import datagen
import half_rows_util as hu
import topk_util as tu
from gbnns_dim_red_amd import cut_graph

NQ = hu.NQ
N = tu.GROUPS * tu.PER                       # 2 048 rows in every fixture
SHAPES = hu.SHAPES                           # (metric, d, d_low): the contest indexes (one-pass adjacency rows)
TWO_PASS_SHAPES = hu.TWO_PASS_SHAPES         # (metric, d_low) over datagen.random_graph(rng, 2048, 33, 48)
BEAMS = hu.BEAMS                             # 8, 64 one list register; 100 two; 200 the two-list kernel
NONE = tu.NONE
ALL = 0xFFFFFFFF
Q_VALUES = (0x0F, 0x01, 0xFF)                # about 1/2, 1/8 and all rows


def row_tags(n=N):
    """T[j] = 1 << (hash(j) % 8): every row carries one of eight tags."""
    j = np.arange(n, dtype=np.uint64)
    h = ((j * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)
    return (np.uint32(1) << (h % np.uint64(8)).astype(np.uint32)).astype(np.uint32)


def query_tags(nq=NQ):
    """Three distinct values of Q in one batch, interleaved."""
    return np.array([Q_VALUES[i % 3] for i in range(nq)], np.uint32)


def allowed_entries(rng, T, Q, pools):
    """One entry per query, drawn from the rows of pools[i] (an index array) that query i may see."""
    ent = np.empty(len(Q), np.uint32)
    for i, q in enumerate(Q):
        ok = pools[i][(T[pools[i]] & q) != 0]
        ent[i] = ok[rng.integers(0, len(ok))]
    return ent


@functools.lru_cache(maxsize=None)
def contest(metric, d, dlow):
    """tu.contest_index_data plus T, Q and an allowed entry point per query inside the query's component."""
    c = dict(tu.contest_index_data(metric, d, dlow))
    rng = tu.rng_of(9100 + 7 * d + 3 * dlow + metric)
    c["T"], c["Q"] = row_tags(), query_tags(len(c["qg"]))
    pools = [np.arange(g * tu.PER, (g + 1) * tu.PER) for g in c["qg"]]
    c["ent"] = allowed_entries(rng, c["T"], c["Q"], pools)
    return c


@functools.lru_cache(maxsize=None)
def two_pass(metric, dlow):
    """hu.two_pass's recipe (adjacency rows of 33 .. 48 slots) plus T, Q and allowed entry points."""
    c = dict(hu.two_pass(metric, dlow))
    rng = tu.rng_of(9200 + 10 * dlow + metric)
    c["T"], c["Q"] = row_tags(), query_tags(NQ)
    c["ent"] = allowed_entries(rng, c["T"], c["Q"], [np.arange(N)] * NQ)
    return c


@functools.lru_cache(maxsize=None)
def odd_first(slots, dlow=32):
    """A hand-built graph over 2 048 nodes: every adjacency row holds `slots` - 8 odd ids first (32: one 32-slot chunk of the pair form; 64: two
    of them, one chunk of the general kernel), then 8 even ids.  T allows the even rows only, every query enters at an even row: the walk on
    G' goes through the 8 even neighbours, a kernel that takes a chunk of disallowed neighbours for the end of the row returns the entry
    alone."""
    rng = tu.rng_of(9300 + slots + dlow)
    odd, even = np.arange(1, N, 2), np.arange(0, N, 2)
    lists = []
    for i in range(N):
        ev = even[even != i]
        lists.append(np.concatenate([rng.choice(odd[odd != i], slots - 8, replace=False), rng.choice(ev, 8, replace=False)]).astype(np.uint32))
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    T = np.where(np.arange(N) % 2 == 0, 1, 2).astype(np.uint32)
    return dict(base=datagen.full_mantissa(rng, N, hu.D_ORIG), queries=datagen.full_mantissa(rng, NQ, hu.D_ORIG),
                db_low=datagen.full_mantissa(rng, N, dlow), q_low=datagen.full_mantissa(rng, NQ, dlow), off=off, nbr=np.concatenate(lists),
                T=T, Q=np.ones(NQ, np.uint32), ent=(2 * rng.integers(0, N // 2, size=NQ)).astype(np.uint32))


def entry_ok(T, Q, ent):
    """[nq] bool: every entry point of the query is a row of the index that the query may see."""
    ent = np.asarray(ent, np.uint32).reshape(len(Q), -1)
    inside = ent < len(T)
    return (inside & ((T[np.where(inside, ent, 0)] & Q[:, None]) != 0)).all(axis=1)


def expected(orc, c, ef, metric, T=None, Q=None, ent=None, q_low=None, aux=None, **kw):
    """The contract's outputs of a tagged NET / LOWQ search over c: dict(ids [nq x ef] pop order, dists, count, hops, dist_calc, want = the
    re-ranked answers), from Oracle.walk on cut_graph's CSR (the auxiliary graph cut the same way), one call per distinct value of Q."""
    T = c["T"] if T is None else T
    Q = c["Q"] if Q is None else Q
    ent = c["ent"] if ent is None else ent
    q_low = c["q_low"] if q_low is None else q_low
    nq = len(Q)
    w = dict(ids=np.full((nq, ef), NONE, np.uint32), dists=np.full((nq, ef), np.inf, np.float32), count=np.zeros(nq, np.int32),
             hops=np.zeros(nq, np.int32), dist_calc=np.zeros(nq, np.int32), want=np.full(nq, NONE, np.uint32))
    ok = entry_ok(T, Q, ent)
    for qv in np.unique(Q[ok]):
        sel = np.flatnonzero(ok & (Q == qv))
        allowed = (T & qv) != 0
        off, nbr = cut_graph(c["off"], c["nbr"], allowed)
        part = orc.walk(q_low[sel], c["db_low"], off, nbr, ef, entries=ent[sel], metric=metric, threads=8,
                        aux=None if aux is None else cut_graph(aux[0], aux[1], allowed), **kw)
        for name in ("ids", "dists", "count", "hops", "dist_calc"):
            w[name][sel] = part[name]
        w["want"][sel] = orc.rerank(c["queries"][sel], part["ids"], part["count"], c["base"], metric=metric, threads=8)
    return w


def tag_kernel(metric, dlow, ef, one_pass, late=False):
    """The first-pass kernel a tagged search of a compact index launches (one entry point, no auxiliary graph): by the domain of the tag
    instances -- rows of 32 / 48 / 64 floats with L2 and of 32 floats with the negative dot in the one- / two-register-list and two-list
    kernels, rows of 144 floats with L2 in the two-list kernel -- else the general kernel takes the batch."""
    steps, one = dlow // 4, "true" if one_pass else "false"
    if dlow == 144 and ef <= 128:
        return "walk_general_kernel"
    if ef <= 64:
        return "walk_reg_tag_kernel<%d, %d, 1, %s>" % (metric, steps, one)
    if ef <= 128:
        return "walk_reg_tag_kernel<%d, %d, 2, false>" % (metric, steps)
    return "walk_reg_big_tag_kernel<%d, %d, %s, %s>" % (metric, steps, one, "true" if late else "false")


def rows_that_differ(a, b):
    return int((a != b).any(axis=1).sum())


def untagged(orc, c, ef, metric, **kw):
    """The oracle's walk of the same queries from the same entry points on the FULL graph, with its re-ranked answers."""
    w = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8, **kw)
    w["want"] = orc.rerank(c["queries"], w["ids"], w["count"], c["base"], metric=metric, threads=8)
    return w


def restricted_queries_that_differ(exp, full, Q):
    """(queries with Q != all whose answer or hop count on G' differs from the full graph's, queries with Q != all)."""
    sel = (Q & 0xFF) != 0xFF
    return int(((exp["want"] != full["want"]) | (exp["hops"] != full["hops"]))[sel].sum()), int(sel.sum())
