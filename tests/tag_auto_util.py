"""What tests/test_tag_auto_cpu.py and tests/test_gpu_tag_auto.py share: the fixture and the expected values of gbnns_index_tag_census and
gbnns_search_tagged_auto.

The contract under test: the census counts, per query word, the rows the word allows and names the lowest of them; query i takes the exact
scan when allowed[i] <= scan_below and the tagged walk otherwise, and every row of the call is bit for bit a row of one of the two existing
calls.  So the expectation is COMPOSED from the existing ones: tag_util.expected / bridge_util.expected (the CPU oracle on the cut / bridged
graph) with topk_util.expected_topk for walk rows -- scan-routed queries walk under word 0 and get the bad-entry row --, and
knn_tagged_util.expected (the CPU oracle's exact lists over the allowed rows) for scan rows.  Nothing takes a tolerance.
"""
import functools

import numpy as np

import bridge_util as bu
import knn_tagged_util as kt
import tag_util as tg
import topk_util as tu
from gbnns_dim_red_amd import tag_census

NONE = tg.NONE
DLOW = 32
WORDS = (0x0F, 0x01, 0xFF, 0x02, 0xF0, 0x100, 0)
# tag_util.row_tags() under those words: rows allowed, lowest allowed row
CENSUS = {0x0F: (1024, 0), 0x01: (256, 0), 0xFF: (2048, 0), 0x02: (255, 11), 0xF0: (1024, 2), 0x100: (0, NONE), 0: (0, NONE)}
# 0: only the empty queries scan; 300: the small words; 1023 / 1024: words 0x0F and 0xF0 (1 024 rows) on the two sides of the boundary; all
SCAN_BELOW = (0, 300, 1023, 1024, 2 ** 64 - 1)
EFS, KS = (8, 64, 200), (1, 10)
# (metric, ef, k, bridged) of the routing tests: every beam class, both k (k <= ef), both metrics, both walks.  Not the cross product: a configuration
# is listed only where the fixture makes a wrong route visible (tests/test_tag_auto_cpu.py asserts it for every entry: the walk's k-answer
# row differs from the exact row for at least three quarters of the queries of every non-empty word).  That leaves out k = 1 at ef 200 --
# a walk that keeps 200 of at most 256 allowed rows finds the exact nearest neighbour of most queries (CPU oracle: 2 of 14 queries of word
# 0x01 differ, 4 .. 5 of 14 of word 0x02) --, k = 1 at ef 64 with L2 (8 of 14 of word 0x02) and the cut walk at ef 200 with the negative dot
# (10 of 14 of word 0x01, k = 10).
CONFIGS = (
    (0, 8, 1, False), (0, 8, 1, True), (0, 64, 10, False), (0, 64, 10, True), (0, 200, 10, False), (0, 200, 10, True),
    (1, 8, 1, True), (1, 8, 1, False), (1, 64, 1, False), (1, 64, 10, True), (1, 200, 10, True),
)


def scan_below_of(ef):
    """Every scan_below at ef 64, 300 at every beam."""
    return SCAN_BELOW if ef == 64 else (300,)


def query_words(nq=tg.NQ):
    return np.array([WORDS[i % len(WORDS)] for i in range(nq)], np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(metric):
    """tag_util.two_pass(metric, 32) -- 2 048 rows, 96 queries, adjacency rows of 33 .. 48 slots, db_low independent of base -- with the seven
    words interleaved as Q."""
    c = dict(tg.two_pass(metric, DLOW))
    c["Q"] = query_words(len(c["q_low"]))
    return c


def census_loops(T, Q):
    """The census by a double loop: the definition."""
    allowed, first = np.zeros(len(Q), np.uint32), np.full(len(Q), NONE, np.uint32)
    for i, q in enumerate(Q):
        for j, t in enumerate(T):
            if int(t) & int(q):
                if allowed[i] == 0:
                    first[i] = j
                allowed[i] += 1
    return allowed, first


def routes(allowed, scan_below):
    """[nq] bool: True = scan.  (scan_below may be 2^64 - 1: Python integers.)"""
    return np.array([int(a) <= scan_below for a in allowed], bool)


_WALKS, _SCANS, _MEMO = {}, {}, {}


def _walk(orc, key, c, ef, metric, Q, ent, bridge, q_low):
    k = (key, ef, Q.tobytes(), ent.tobytes(), bridge, None if q_low is None else q_low.tobytes())
    if k not in _WALKS:
        _WALKS[k] = (bu if bridge else tg).expected(orc, c, ef, metric, Q=Q, ent=ent, q_low=q_low)
    return _WALKS[k]


def _scan(orc, key, c, k, metric, Q):
    kk = (key, k, Q.tobytes())
    if kk not in _SCANS:
        _SCANS[kk] = kt.expected(orc, c["base"], c["queries"], c["T"], Q, k, metric)
    return _SCANS[kk]


def expected(orc, key, c, ef, k, metric, scan_below, Q=None, ent=None, bridge=False, q_low=None):
    """Every output of search_auto over c: dict(allowed, first, route, ids, top_ids, top_dist, cand, cand_dist, hops, dist_calc).  `key` names
    c (the caches are shared by the tests); ent None: the walk enters at `first`."""
    Q = c["Q"] if Q is None else Q
    allowed, first = tag_census(c["T"], Q)
    scan = routes(allowed, scan_below)
    walk_q = np.where(scan, 0, Q).astype(np.uint32)
    w = _walk(orc, key, c, ef, metric, walk_q, first if ent is None else np.asarray(ent, np.uint32), bridge, q_low)
    memo = _MEMO.setdefault(key, {})
    dist = tu.list_distances(orc, c["base"], c["queries"], w["ids"], w["count"], metric, memo)
    top_ids, top_dist = tu.expected_topk(dist, w["ids"], w["count"], k)
    ids = w["want"].copy()
    if scan.any():
        s_ids, s_dist = _scan(orc, key, c, k, metric, Q)
        top_ids[scan], top_dist[scan] = s_ids[scan], s_dist[scan]
        ids[scan] = s_ids[scan, 0]
    return dict(allowed=allowed, first=first, route=scan.astype(np.uint8), ids=ids, top_ids=top_ids, top_dist=top_dist, cand=w["ids"],
                cand_dist=w["dists"], hops=w["hops"], dist_calc=w["dist_calc"], want=w["want"])


def both_routes(orc, key, c, ef, k, metric, bridge=False):
    """(walk rows, scan rows) of every query: the call's top-k rows with every query walked (scan_below below every count but the empty
    queries') and with every query scanned."""
    w = expected(orc, key, c, ef, k, metric, 0, bridge=bridge)
    s = expected(orc, key, c, ef, k, metric, 2 ** 64 - 1, bridge=bridge)
    return w["top_ids"], s["top_ids"]


def quantised(c):
    """The fixture's original-space rows and queries as bytes (their [-0.35, 0.35] range mapped into 0 .. 255)."""
    q8 = lambda a: np.ascontiguousarray(np.clip(np.rint((a + np.float32(0.4)) * np.float32(300)), 0, 255).astype(np.uint8))
    return q8(c["base"]), q8(c["queries"])


def differences(r, e, names=("ids", "top_ids", "top_dist", "cand", "cand_dist", "hops", "dist_calc", "allowed", "route")):
    """Names of the outputs of r (search_auto's dict) that differ from the expectation e; floats by their bits."""
    bad = []
    for name in names:
        got, want = np.asarray(r[name]), np.asarray(e[name])
        if got.dtype.kind == "f":
            got, want = got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
        elif got.dtype != want.dtype:
            got = got.view(want.dtype) if got.dtype.itemsize == want.dtype.itemsize else got.astype(want.dtype)
        if got.shape != want.shape or not np.array_equal(got, want):
            rows = np.flatnonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(axis=1)) if got.shape == want.shape else []
            bad.append((name, list(rows[:8])))
    return bad
