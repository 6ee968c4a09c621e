"""What tests/test_bridge_cpu.py and tests/test_gpu_bridge.py share: the expected values, the hand-built fixtures and the expected kernel names
of gbnns_search_tagged with GBNNS_FLAG_TAG_BRIDGE.

The contract under test: a bridged tagged search of query i is the reference's search on G''(i) -- the row of node u is u's adjacency row in
order, an allowed neighbour standing for itself, a disallowed one replaced by the allowed entries of its own row (one level;
gbnns_dim_red_amd.bridge_graph).  Every expected value is the CPU oracle's on that CSR, one oracle call per distinct value of Q.  Nothing takes
a tolerance.  Tags, query words, entry points and the fixtures of the contest / two-pass shapes are tag_util's.
"""
import functools

import numpy as np

import datagen
import half_rows_util as hu
import tag_util as tg
import topk_util as tu
from gbnns_dim_red_amd import bridge_graph

N, NQ, NONE = tg.N, tg.NQ, tg.NONE


def bridge_graph_loops(off, nbr, allowed):
    """bridge_graph restated with plain loops: the definition, slot by slot."""
    off = [int(x) for x in off]
    new_off, out = [0], []
    for u in range(len(off) - 1):
        for v in nbr[off[u]:off[u + 1]]:
            if allowed[v]:
                out.append(int(v))
            else:
                out.extend(int(w) for w in nbr[off[v]:off[v + 1]] if allowed[w])
        new_off.append(len(out))
    return np.array(new_off, np.uint64), np.array(out, np.uint32)


def expected(orc, c, ef, metric, T=None, Q=None, ent=None, q_low=None, aux=None, db=None, rerank=True, **kw):
    """The contract's outputs of a bridged tagged search over c: tag_util.expected with bridge_graph in the place of cut_graph (the auxiliary
    graph bridged through itself).  db: the walked table (default c["db_low"]; a PLAIN walk: c["base"], q_low = the queries, rerank=False)."""
    T = c["T"] if T is None else T
    Q = c["Q"] if Q is None else Q
    ent = c["ent"] if ent is None else ent
    q_low = c["q_low"] if q_low is None else q_low
    db = c["db_low"] if db is None else db
    nq = len(Q)
    w = dict(ids=np.full((nq, ef), NONE, np.uint32), dists=np.full((nq, ef), np.inf, np.float32), count=np.zeros(nq, np.int32),
             hops=np.zeros(nq, np.int32), dist_calc=np.zeros(nq, np.int32), want=np.full(nq, NONE, np.uint32))
    ok = tg.entry_ok(T, Q, ent)
    for qv in np.unique(Q[ok]):
        sel = np.flatnonzero(ok & (Q == qv))
        allowed = (T & qv) != 0
        off, nbr = bridge_graph(c["off"], c["nbr"], allowed)
        part = orc.walk(q_low[sel], db, off, nbr, ef, entries=ent[sel], metric=metric, threads=8,
                        aux=None if aux is None else bridge_graph(aux[0], aux[1], allowed), **kw)
        for name in ("ids", "dists", "count", "hops", "dist_calc"):
            w[name][sel] = part[name]
        if rerank:
            w["want"][sel] = orc.rerank(c["queries"][sel], part["ids"], part["count"], c["base"], metric=metric, threads=8)
    return w


def bridge_kernel(metric, dlow, ef):
    """The first-pass kernel a bridged search of a compact index launches (one entry point, no auxiliary graph): a bridge instance over rows
    of 32 / 48 / 64 floats with L2 and 32 floats with the negative dot at beams up to 128, else the general kernel takes the batch."""
    if ef > 128 or dlow not in ((32,) if metric else (32, 48, 64)):
        return "walk_general_kernel"
    return "walk_bridge_kernel<%d, %d, %d>" % (metric, dlow // 4, 1 if ef <= 64 else 2)


def queries_that_differ(a, b, sel):
    """Queries of `sel` whose answer or hop count differs between two expectations."""
    return int(((a["want"] != b["want"]) | (a["hops"] != b["hops"]))[sel].sum())


def _fixture(rng, lists, T, ent, dlow=32):
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return dict(base=datagen.full_mantissa(rng, N, hu.D_ORIG), queries=datagen.full_mantissa(rng, NQ, hu.D_ORIG),
                db_low=datagen.full_mantissa(rng, N, dlow), q_low=datagen.full_mantissa(rng, NQ, dlow), off=off,
                nbr=np.concatenate(lists).astype(np.uint32), T=T, Q=np.ones(NQ, np.uint32), ent=ent.astype(np.uint32))


@functools.lru_cache(maxsize=None)
def parity():
    """Fixtures (a) and (d): every neighbour of an even row is odd, every odd row lists even ids, T allows the even rows only.  The cut walk
    returns the entry alone; the bridged walk goes on through the odd rows.  Every odd row v holds 16 even ids; the row of an even u lists the
    odd rows that hold u first (so a looked-through row contains u itself), then further odd ids, 16 in all."""
    rng = tu.rng_of(9700)
    odd, even = np.arange(1, N, 2), np.arange(0, N, 2)
    lists = [None] * N
    for v in odd:
        lists[v] = rng.choice(even, 16, replace=False)
    holders = {int(u): [] for u in even}
    for v in odd:
        for u in lists[v]:
            holders[int(u)].append(int(v))
    for u in even:
        first = np.array(holders[int(u)][:8], np.int64)
        rest = rng.choice(np.setdiff1d(odd, first), 16 - len(first), replace=False)
        lists[u] = np.concatenate([first, rest])
    T = np.where(np.arange(N) % 2 == 0, 1, 2).astype(np.uint32)
    return _fixture(rng, lists, T, 2 * rng.integers(0, N // 2, size=NQ))


@functools.lru_cache(maxsize=None)
def twins():
    """Fixture (b): the odd rows are disallowed and come in pairs (4k + 1, 4k + 3) with IDENTICAL rows of 12 even ids; an even row lists 4 even
    ids, the two rows of one pair side by side, 4 more even ids.  The bridged row is 4 + 12 + 12 + 4 ids with every looked-through id twice,
    inside one 32-slot chunk of the pair form and one 64-slot chunk of the general kernel."""
    rng = tu.rng_of(9701)
    even = np.arange(0, N, 2)
    lists = [None] * N
    for k in range(N // 4):
        lists[4 * k + 1] = lists[4 * k + 3] = rng.choice(even, 12, replace=False)
    for u in even:
        k = int(rng.integers(0, N // 4))
        ev = rng.choice(even[even != u], 8, replace=False)
        lists[u] = np.concatenate([ev[:4], [4 * k + 1, 4 * k + 3], ev[4:]])
    T = np.where(np.arange(N) % 2 == 0, 1, 2).astype(np.uint32)
    return _fixture(rng, lists, T, 2 * rng.integers(0, N // 2, size=NQ))
