"""Shared by tests/test_knn_instances_cpu.py and tests/test_gpu_census_edges.py: the batches and tag tables that put census_dedupe_kernel and
census_rows_kernel (tag_census.hip) on their edges, each with the precondition it rests on as an assertion.  The reference is always
gbnns_dim_red_amd.tag_census (NumPy).

Geometry the fixtures are built around: a wavefront of the dedupe kernel is 64 consecutive queries; the rows kernel runs the batch's distinct
words in chunks of 256, 64 to a register; a workgroup of it holds a tile of 1 024 rows, 256 to a wavefront, lane l the rows 4 l .. 4 l + 3 of
that share.
"""
import numpy as np

import knn_tagged_util as kt
from gbnns_dim_red_amd import census_slot

N = 1037
DISTINCT = (63, 64, 65, 255, 256, 257, 512, 513)   # U at the lane and chunk edges of the word loop
TILE_NS = (1023, 1024, 1025, 2048)                 # n at the tile's edges
PLACE_N = 2049
WRAP_NQ, WRAP_CAP = 40, 128


def distinct_words(u):
    """u distinct random 32-bit words, none of them 0."""
    w = np.random.default_rng(8000 + u).choice(2 ** 32 - 1, u, replace=False) + 1
    return w.astype(np.uint32)


def repeated(words):
    """Every word twice and five of them a third time, 2 U + 5 queries in a shuffled order."""
    rng = np.random.default_rng(8100 + len(words))
    q = np.concatenate([words, words, words[:5]])
    return np.ascontiguousarray(q[rng.permutation(len(q))])


def one_word_batch():
    """(T [N], Q [1 000]): one word in 1 000 queries -- whole wavefronts take the dedupe kernel's leader shortcut -- that allows 35 rows, the
    lowest of them row 517."""
    T = np.zeros(N, np.uint32)
    T[:] = 0x0F
    rows = np.arange(517, N, 15)
    T[rows] |= np.uint32(0x4000)
    Q = np.full(1000, 0x4000, np.uint32)
    assert len(rows) == 35 and rows[0] == 517
    return T, Q


def half_shared_batch():
    """Q [645] over kt.tag_table: every wavefront of 64 queries starts with a word that half of its lanes share (the even lanes; another word
    per wavefront), the odd lanes carry words of their own.  The last wavefront is a partial one of 5 queries."""
    nq = 10 * 64 + 5
    own = distinct_words(nq)
    lead = np.array([1 << (w % 10) for w in range(11)], np.uint32)   # a word of tag_table per wavefront
    Q = own.copy()
    for w in range(11):
        Q[64 * w:64 * (w + 1):2] = lead[w]
    for w in range(11):
        wave = Q[64 * w:64 * (w + 1)]
        assert wave[0] == lead[w] and (wave == wave[0]).sum() == (len(wave) + 1) // 2
    return np.ascontiguousarray(Q)


def placement():
    """(T [2 049], rows [32], Q): bit b of the tag words is set on exactly one row, rows[b]; the rows are the ends of the table, of a tile and
    of a wavefront's share -- lane 63, element 3 of each of the four wavefronts of tiles 0 and 1 among them.  Q: 1 << b for every bit (allowed
    1, first rows[b]), then pairs of bits (allowed 2, first the lower row)."""
    n = PLACE_N
    rows = [0, 3, 255, 256, 1023, 1024, n - 1]
    rows += [1024 * t + 256 * v + 4 * 63 + 3 for t in (0, 1) for v in range(4)]        # 255, 511, 767, 1023, 1279, ...
    rows += [1024 * t + 256 * v + 4 * 63 for t in (0, 1) for v in range(4)]            # lane 63, element 0
    rows += [1024 * t + 256 * v for t in (0, 1) for v in range(1, 4)]                  # lane 0, element 0 of the other wavefronts
    rows += [1, 2, 4, 252, 253, 254, 257, 1022, 1025, 2044, 2046, 2047]
    rows = list(dict.fromkeys(rows))[:32]
    assert len(rows) == 32 and len(set(rows)) == 32 and max(rows) == n - 1
    for r in (0, 3, 255, 256, 1023, 1024, n - 1, 511, 767, 1279, 1535, 1791, 2047):
        assert r in rows, r
    rows = np.array(rows, np.int64)
    rows = rows[np.random.default_rng(8200).permutation(32)]   # which bit sits where is not ordered by row
    T = np.zeros(n, np.uint32)
    T[rows] = np.uint32(1) << np.arange(32, dtype=np.uint32)
    single = (np.uint32(1) << np.arange(32, dtype=np.uint32)).astype(np.uint32)
    rng = np.random.default_rng(8201)
    pairs = np.array([(1 << int(a)) | (1 << int(b)) for a, b in (rng.choice(32, 2, replace=False) for _ in range(48))], np.uint32)
    return T, rows, np.concatenate([single, pairs]).astype(np.uint32)


def wrap_words():
    """40 distinct words whose home slots in the 128-slot dedupe table of a 40-query census are the last three (by census_slot): their probe
    sequences run past the end of the table and go on from slot 0."""
    words, w = [], 1
    while len(words) < WRAP_NQ:
        slot, cap = census_slot(w, WRAP_NQ)
        assert cap == WRAP_CAP
        if slot >= cap - 3:
            words.append(w)
        w += 1
    words = np.array(words, np.uint32)
    slots = np.array([census_slot(int(x), WRAP_NQ)[0] for x in words])
    assert len(np.unique(words)) == WRAP_NQ and set(slots.tolist()) == {125, 126, 127}
    return words


def table(n=N):
    return kt.tag_table(8300 + n, n)
