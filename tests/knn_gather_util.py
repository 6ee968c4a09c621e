"""Shared by tests/test_knn_gather_cpu.py and tests/test_gpu_knn_gather.py: the tag fixtures of gbnns_index_exact_knn_gather -- those of
tests/knn_tagged_util.py extended by two words whose lists are exactly one and exactly two tiles of the gathered kernel long -- and a numpy
restatement of its schedule.  Nothing here has a tolerance."""
import numpy as np

import knn_tagged_util as tu

TILE_BIT, TWO_TILE_BIT = 10, 11   # on exactly 64 / exactly 128 rows, spread over the table (every row of a table shorter than that)
QUERY_WORDS = tu.QUERY_WORDS + [1 << TILE_BIT, 1 << TWO_TILE_BIT]
N_ROUNDS, NQ_ROUNDS = 6000, 300   # the shape of the rounds tests


def tag_table(seed, n):
    """knn_tagged_util.tag_table(seed, n) with bit 10 on min(n, 64) rows and bit 11 on min(n, 128) rows, evenly spaced from row 0."""
    t = tu.tag_table(seed, n)
    for bit, count in ((TILE_BIT, 64), (TWO_TILE_BIT, 128)):
        rows = np.unique((np.arange(min(n, count), dtype=np.int64) * n) // min(n, count))
        assert rows.size == min(n, count)
        t[rows] |= np.uint32(1 << bit)
    return t


def query_words(nq):
    """Q [nq]: knn_tagged_util.query_words' cycle (the ten bits, 0, all ones, 0x3) extended by the two words above: 15 distinct words."""
    return np.array([QUERY_WORDS[i % len(QUERY_WORDS)] for i in range(nq)], np.uint32)


def census(T, Q):
    """allowed [nq] uint32 by numpy: rows of T that share a bit with Q[i]."""
    return np.array([np.count_nonzero(T & w) for w in Q], np.uint32)


def schedule(words, allowed, budget, W):
    """The schedule of include/gbnns.h (gbnns_debug_gather_schedule) by numpy: dict(order, round_of, list_offset_of, rounds, workgroups, groups)
    -- groups: [(word, list length, queries, round, offset)] in ascending word order."""
    words, allowed = np.asarray(words, np.uint32), np.asarray(allowed, np.uint32)
    nq = words.size
    live = np.nonzero(allowed > 0)[0]
    order = np.concatenate([live[np.argsort(words[live], kind="stable")], np.nonzero(allowed == 0)[0]]).astype(np.uint32)
    round_of = np.full(nq, 0xFFFFFFFF, np.uint32)
    offset_of = np.zeros(nq, np.uint64)
    groups, rnd, filled, wgs = [], 0, 0, 0
    for w in np.unique(words[live]):
        qs = np.nonzero((words == w) & (allowed > 0))[0]
        length = int(allowed[qs[0]])
        assert (allowed[qs] == length).all()
        if filled and filled + length > budget:
            rnd, filled = rnd + 1, 0
        round_of[qs], offset_of[qs] = rnd, filled
        groups.append((int(w), length, qs, rnd, filled))
        filled += length
        wgs += -(-qs.size // W)
    return {"order": order, "round_of": round_of, "list_offset_of": offset_of, "rounds": rnd + 1 if groups else 0, "workgroups": wgs, "groups": groups}
