"""What tests/test_half_walk_cpu.py and tests/test_gpu_half_walk.py share: the fixtures and expected values of the half-row PLAIN walk
(MODE_PLAIN with FLAG_HALF_WALK on a half-base handle).

The contract under test: every output equals, bit for bit, what the same call without the flag returns on the handle created with
db = float32(db_half).  Every expected value is therefore the CPU oracle's walk over `hb.wide(base)` in the original space -- the unchanged
oracle decides everything, nothing takes a tolerance -- and every GPU case is compared byte for byte with the float handle as well.

Two kinds of fixture, all of 2 048 rows and 96 queries:
  * the half contest (half_base_util.index_data): its rows, original-space queries, disconnected 256-row groups and entry points as they
    are.  In real arithmetic every row of a group is equidistant from the group's query; only the order of the roundings separates them,
    and between the exact copies nothing does.  Every group holds -0, both subnormal ends and a value >= 2^14; an L2 tail holds arbitrary
    16-bit patterns;
  * random halves: rows of finite binary16 values whose 11 significand bits are all in use (an odd mantissa field), magnitudes 1 .. 16, either
    sign; each query a base row plus N(0, 0.5) noise with every float32 mantissa bit in use; a one-pass graph (random_graph(rng, n, 2, 30))
    and a two-pass graph (random_graph(rng, n, 34, 60)); random entry points, query 0 entering at row n - 1 so that nothing behind the last
    row's padding can enter a sum.  Walks differ per query and every list holds distinct distances (but for a bit-equal pair in a few of
    the lists of 100 and 200: a tie the id breaks).
"""
import functools

import numpy as np

import byte_walk_util as bw
import datagen
import half_base_util as hb
import topk_util as tu

N, NQ, NONE = hb.N, 96, hb.NONE
GROUPS, PER = hb.GROUPS, hb.PER
BEAMS = (8, 64, 100, 200)
WANT = bw.WANT
# (metric, d) of the contest fixtures the tests use: the 24-step pair form; the long rows (16 and 120 chunks); the general instance -- 45 the
# tail ignored, 40 five chunks, 8 one, 12 the half-padded one, the negative dot without and with its masked tail
FAST_CONTESTS = [(0, 96), (0, 128), (0, 960)]
GENERAL_CONTESTS = [(0, 45), (0, 40), (0, 8), (0, 12), (1, 128), (1, 45)]
# random halves: 96 the pair form; 300 rows of 304 halves, 38 chunks (19 a lane = 8 + 8 + 3 in the masked batch, the last half padding);
# 404 rows of 408 halves, 51 chunks (25 a lane = 8 + 8 + 8 + 1, then the even lane's lone, half-padded one)
RANDOM_DIMS = (96, 300, 404)
# dimensions at which the order of the sums must be visible, and the wrong order the instance of that dimension could take
PAIR_DIMS, LONG_DIMS = (96,), (128, 300, 404, 960)

expected, against, same_bytes = bw.expected, bw.against, bw.same_bytes


def contest(metric, d):
    return hb.index_data(metric, d, 32)


@functools.lru_cache(maxsize=None)
def random_halves(d):
    """dict: base float16 [N x d], wide, queries [NQ x d] float32, graphs {1: (off, nbr) one-pass, 2: two-pass}, ent [NQ], db_low (any: a
    half-base handle needs one; the PLAIN walk never reads it)."""
    rng = tu.rng_of(8800 + d)
    bits = (rng.integers(0, 2, size=(N, d)).astype(np.uint16) << 15) | (rng.integers(15, 19, size=(N, d)).astype(np.uint16) << 10) | \
           (2 * rng.integers(0, 512, size=(N, d)) + 1).astype(np.uint16)
    base = np.ascontiguousarray(bits.view(np.float16))
    pick = rng.integers(0, N, size=NQ)
    noise = rng.normal(0.0, 0.5, size=(NQ, d))
    queries = (base[pick].astype(np.float64) + noise).astype(np.float32)
    queries = (queries.view(np.uint32) | np.uint32(1)).view(np.float32)   # every mantissa bit in use
    graphs = {1: datagen.random_graph(rng, N, 2, 30), 2: datagen.random_graph(rng, N, 34, 60)}
    ent = rng.integers(0, N, size=NQ).astype(np.uint32)
    ent[0] = N - 1
    db_low = datagen.full_mantissa(rng, N, 32)
    return dict(base=base, wide=hb.wide(base), queries=np.ascontiguousarray(queries), graphs=graphs, ent=ent, db_low=db_low)


@functools.lru_cache(maxsize=None)
def three_pass_graph():
    """(off, nbr) over the N rows with 66 .. 90 neighbours a row: adjacency rows of 96 slots, two passes of the run-time-length instances'
    64-slot pass loop (the graphs of random_halves end at 60 neighbours, one such pass)."""
    return datagen.random_graph(tu.rng_of(8899), N, 66, 90)


# ---- the order of the sums, restated in NumPy ----------------------------------------------------------------------------------------
def _squares(rows, q):
    """[steps x m x 4] float32: (row - q)^2 of every 4-wide step, each operation rounded to float32; the d % 4 tail is ignored."""
    rows, q = np.asarray(rows, np.float32), np.asarray(q, np.float32)
    steps = rows.shape[1] // 4
    e = (rows[:, :4 * steps] - q[None, :4 * steps]).astype(np.float32)
    return np.moveaxis((e * e).astype(np.float32).reshape(len(rows), steps, 4), 1, 0)


def _close(s):
    return ((((s[:, 0] + s[:, 1]).astype(np.float32) + s[:, 2]).astype(np.float32) + s[:, 3]).astype(np.float32)).view(np.uint32)


def l2_bits_reference_order(rows, q):
    """The reference's order: four running sums over the steps in row order, closed as ((s0 + s1) + s2) + s3 -- the oracle's bits."""
    sq = _squares(rows, q)
    s = np.zeros(sq.shape[1:], np.float32)
    for t in range(len(sq)):
        s = (s + sq[t]).astype(np.float32)
    return _close(s)


def l2_bits_summed_apart(rows, q, part_of_step):
    """An order the kernels must NOT use: the steps of part 0 and of part 1 (part_of_step(t, steps)) go into two sets of four running
    sums that never meet until the end, where they are added and closed."""
    sq = _squares(rows, q)
    s = np.zeros((2,) + sq.shape[1:], np.float32)
    for t in range(len(sq)):
        w = part_of_step(t, len(sq))
        s[w] = (s[w] + sq[t]).astype(np.float32)
    return _close((s[0] + s[1]).astype(np.float32))


def lane_halves(t, steps):
    """d = 96, the pair form: the even lane holds the first half of the row's steps, the odd lane the second."""
    return 0 if t < steps // 2 else 1


def alternate_chunks(t, steps):
    """the long rows: a 16-byte chunk of halves is two steps; the even lane takes the chunks 0, 2, 4, ..., the odd lane 1, 3, 5, ..."""
    return (t // 2) % 2


def oracle_l2_bits(orc, wide, q):
    return np.array([np.float32(orc.l2(wide[j], q)).view(np.uint32) for j in range(len(wide))], np.uint32)
