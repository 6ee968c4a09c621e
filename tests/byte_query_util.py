"""What tests/test_byte_query_cpu.py and tests/test_gpu_byte_query.py share: the fixtures and expected values of byte queries on a byte handle
(Index.search(queries=<uint8>), gbnns_search_byte_queries).

The contract under test: every output equals, bit for bit, what the corresponding float-query call returns on the same handle with
queries.astype(float32).  Every expected value is the unchanged CPU oracle's on `bu.wide(base)` with `queries.astype(float32)`; nothing takes a
tolerance.  Shapes are tests/byte_walk_util.py's: 2 048 rows of d = 128, 96 queries, beams (8, 64, 100, 200).

Three fixtures, each dict(base uint8, wide, queries_u8, queries = queries_u8.astype(float32), graphs {1: one-pass, 2: two-pass}, ent, db_low):
  * random   -- byte_walk_util.random_bytes(128): its rows, graphs and entry points; its queries rint-ed and clipped to uint8, with the marker
                columns of the rows (0, 127, 128, 255, rotating with the index) in the queries' first four columns as well;
  * extremes -- the same rows and queries with eight EXTREME rows (four all 255, four all 0) that form a component of their own in both
                graphs (nothing else points to them), queries 0 .. 3 all 0 entering at an all-255 row and queries 4 .. 7 all 255 entering at
                an all-0 row -- their lists hold 128 * 255^2 = 8 323 200 exactly, next to 0 --, and queries 8 .. 11 all 0 / 12 .. 15 all 255
                walking the main component from ordinary entry points;
  * ties     -- the integer byte contest (byte_rows_util.index_data(0, 128, 32, integer=True)): its queries are c * (1, ..., 1) with an
                integer c, cast to bytes; every row of a group ties and the id decides.  Graph 1 is the contest's own (one pass), graph 2 a
                two-pass contest graph over the same groups (contest_graph(rng, 8, 256, 34, 60)).
"""
import functools

import numpy as np

import byte_rows_util as bu
import byte_walk_util as bw
import datagen
import topk_util as tu

N, NQ, NONE = bw.N, bw.NQ, bw.NONE
BEAMS = bw.BEAMS
MARKS = bw.MARKS
WANT = bw.WANT
FIXTURES = ("random", "extremes", "ties")
EXTREME_255 = (3, 700, 1500, N - 1)
EXTREME_0 = (5, 900, 1600, 2000)
FAR = 128 * 255 * 255  # 8 323 200: an all-0 vector against an all-255 one


def _bytes_of(q):
    return np.clip(np.rint(q), 0, 255).astype(np.uint8)


def _pack(base, queries_u8, graphs, ent, db_low):
    base, queries_u8 = np.ascontiguousarray(base), np.ascontiguousarray(queries_u8)
    c = dict(base=base, wide=bu.wide(base), queries_u8=queries_u8, queries=np.ascontiguousarray(queries_u8.astype(np.float32)), graphs=graphs,
             ent=np.ascontiguousarray(ent, np.uint32), db_low=db_low)
    for v in (c["wide"], c["queries_u8"], c["queries"]):  # (made here; base / ent may be another module's cached arrays)
        v.setflags(write=False)
    return c


def _isolate(off, nbr, members):
    """The CSR graph with `members` made a component of their own: each member's row lists the other members, and no other row keeps one."""
    off = off.astype(np.int64)
    inside = np.zeros(len(off) - 1, bool)
    inside[list(members)] = True
    rows = []
    for i in range(len(off) - 1):
        if inside[i]:
            rows.append(np.array([m for m in members if m != i], np.uint32))
        else:
            r = nbr[off[i]:off[i + 1]]
            rows.append(r[~inside[r]].astype(np.uint32))
    new_off = np.zeros(len(off), np.uint64)
    new_off[1:] = np.cumsum([len(r) for r in rows])
    return new_off, np.ascontiguousarray(np.concatenate(rows), np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name == "ties":
        t = bw.contest(0, 128, True)
        q8 = _bytes_of(t["queries"])
        assert np.array_equal(q8.astype(np.float32), t["queries"])  # (integer queries: the cast rounds nothing)
        two_pass = datagen.contest_graph(tu.rng_of(7801), bu.GROUPS, bu.PER, 34, 60)
        return _pack(t["base"], q8, {1: (t["off"], t["nbr"]), 2: two_pass}, t["ent"], t["db_low"])
    r = bw.random_bytes(128)
    q8 = _bytes_of(r["queries"])
    for j in range(4):
        q8[:, j] = np.array(MARKS, np.uint8)[(np.arange(NQ) + j) % 4]
    if name == "random":
        return _pack(r["base"], q8, r["graphs"], r["ent"], r["db_low"])
    assert name == "extremes"
    base, ent = r["base"].copy(), r["ent"].copy()
    base[list(EXTREME_255)] = 255
    base[list(EXTREME_0)] = 0
    members = EXTREME_255 + EXTREME_0
    graphs = {k: _isolate(off, nbr, members) for k, (off, nbr) in r["graphs"].items()}
    q8[[0, 1, 2, 3, 8, 9, 10, 11]] = 0
    q8[[4, 5, 6, 7, 12, 13, 14, 15]] = 255
    ent[0:4] = EXTREME_255          # (query 0 still enters at row N - 1)
    ent[4:8] = EXTREME_0
    for i in range(8, NQ):          # everybody else starts, and stays, in the main component
        while int(ent[i]) in members:
            ent[i] = (int(ent[i]) + 1) % N
    return _pack(base, q8, graphs, ent, r["db_low"])


def stride(off):
    return max(16, (int(np.diff(off.astype(np.int64)).max()) + 15) // 16 * 16)


def expected(orc, name, graph, ef, k, **kw):
    """The oracle's PLAIN walk of fixture `name` over graph 1 / 2 (byte_walk_util.expected: computed once, read-only)."""
    c = fixture(name)
    off, nbr = c["graphs"][graph]
    return bw.expected(orc, ("byte query", name, graph), c["queries"], c["wide"], off, nbr, ef, k, c["ent"], **kw)


def int_l2_bits(base, q8):
    """[len(base)] uint32: float32(sum q^2 + sum x^2 - 2 sum q x) in uint32 wrap-around arithmetic, as bit patterns -- the integer kernels' distance."""
    x, q = np.asarray(base).astype(np.uint32), np.asarray(q8).astype(np.uint32)
    with np.errstate(over="ignore"):
        qq = (q * q).sum(dtype=np.uint32)
        xx = (x * x).sum(axis=1, dtype=np.uint32)
        qx = (x * q[None, :]).sum(axis=1, dtype=np.uint32)
        s = (qq + xx - np.uint32(2) * qx).astype(np.uint32)
    return s.astype(np.float32).view(np.uint32)


# ---- three wrong distances, each restated as a walk the unchanged oracle can run -------------------------------------------------------
def _swap_chunk_pairs(a):
    d = a.shape[1]
    return np.ascontiguousarray(a.reshape(len(a), d // 32, 2, 16)[:, :, ::-1, :].reshape(len(a), d))


def wrong_walk(orc, variant, name, graph, ef):
    """Candidate ids [NQ x ef] in pop order of the walk with a wrong distance:
      "int8"     every byte, of rows and queries, read as int8 (a signed dot instruction);
      "partner"  a lane consumes its partner's chunks of the ROW (16-byte chunks swapped within pairs) against its own chunks of the query,
                 and chunk c weighs 1 (c even) or 4 (c odd) -- the weight keeps the swap visible where the query is constant (ties);
      "no_row"   the row term sum x^2 left out: sum q^2 - 2 sum q x, which orders the rows as the negative dot does (a monotone map of it;
                 every value is an integer below 2^24, so ties stay ties)."""
    c = fixture(name)
    off, nbr = c["graphs"][graph]
    q, x, metric = c["queries"], c["wide"], 0
    if variant == "int8":
        q, x = c["queries_u8"].view(np.int8).astype(np.float32), c["base"].view(np.int8).astype(np.float32)
    elif variant == "partner":
        s = np.repeat(np.tile(np.array([1.0, 2.0], np.float32), c["base"].shape[1] // 32), 16)  # sqrt of the chunk's weight, per column
        q, x = q * s[None, :], _swap_chunk_pairs(c["wide"]) * s[None, :]
    else:
        assert variant == "no_row"
        metric = 1
    w = orc.walk(np.ascontiguousarray(q, np.float32), np.ascontiguousarray(x, np.float32), off, nbr, ef, k=ef, entries=c["ent"], metric=metric, threads=8)
    return w["ids"]


def against(r, w):
    return bw.against(r, w)


def same_bytes(a, b, names=("ids",) + WANT):
    return bw.same_bytes(a, b, names)
