"""What tests/test_half_base_cpu.py and tests/test_gpu_half_base.py share: the fixtures of the half-base handle (Index(db=<float16>)).

The contract under test: every call on a half-base handle returns what the same call returns on the handle over db.astype(float32), bit
for bit.  Every expected value is therefore the CPU oracle's on `wide(base)` -- the unchanged oracle decides everything, nothing takes a
tolerance.

The half contest (the byte contest's recipe with binary16 values): group g has one vector v_g of finite binary16 values whose 11
significand bits are all in use (an odd mantissa field), positive and negative, of magnitudes 32 .. 512 around the query's constant; it
contains the bit patterns 0x8000 (-0), 0x0001 and 0x03FF (the smallest and the largest subnormal) and one value of magnitude >= 2^14.  The
group's 256 rows are v_g under a fresh permutation of the coordinates the metric reads (4 * floor(d / 4) for L2, all d for the negative
dot; an L2 tail holds arbitrary 16-bit patterns -- infinities and NaNs among them -- that must not matter), three of them exact copies of
other rows of the group, tail included.  The group's query is c_g * (1, ..., 1) with c_g a full-mantissa float32 near 100: in real
arithmetic every row of a group is equidistant from its query, in float32 only the order of the roundings separates them -- and between
the copies nothing does, so the pop index decides.
"""
import functools

import numpy as np

import datagen
import topk_util as tu

GROUPS, PER, NONE = tu.GROUPS, tu.PER, tu.NONE
N = GROUPS * PER
DUPLICATES = 3
MARKS = (0x8000, 0x0001, 0x03FF)   # and one value of magnitude >= 2^14 (BIG_EXPONENTS)
BIG_EXPONENTS = (29, 30)           # biased: 2^14 .. 65 504
# (d, metric) of the stand-alone kernels.  L2, the chunk-pair form: 128 and 96 even chunk counts (the four-loads loop; 96: two single chunks
# behind it), 40 five chunks (the last the even lane's alone), 8 one chunk, 12 and 300 d % 8 == 4 (the half-padded last chunk at its
# shortest and at glove's length), 960 the deep ladder (its first loop only: 60 chunks a lane = 3 x 20), 404 the shortest d whose deep
# instance enters its other two loops, the four-loads loop and the single chunks (51 chunks: 25 a lane = 20 + 4 + 1, then the even lane's
# lone, half-padded one).  45: a lane per row, the tail ignored.  The negative dot with and without its masked tail.
RERANK_SHAPES = [(128, 0), (96, 0), (40, 0), (8, 0), (12, 0), (300, 0), (960, 0), (404, 0), (45, 0), (128, 1), (45, 1)]
BEAMS = (8, 64, 100, 200)
INDEX_SHAPES = [(0, 96, 48), (1, 128, 32)]   # (metric, d, d_low): the contest index and the negative-dot one


def wide(a):
    """The float table of the contract: binary16 -> binary32 is exact."""
    a = np.asarray(a)
    assert a.dtype == np.float16
    return np.ascontiguousarray(a.astype(np.float32))


def bits_of(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint16)


def _half_groups(rng, d, metric):
    width = d if metric else 4 * (d // 4)
    base = np.empty((N, d), np.uint16)
    for g in range(GROUPS):
        sign = rng.integers(0, 2, size=d).astype(np.uint16) << 15
        v = sign | (rng.integers(20, 24, size=d).astype(np.uint16) << 10) | (2 * rng.integers(0, 512, size=d) + 1).astype(np.uint16)
        at = rng.permutation(width)[:len(MARKS) + 1]
        v[at[:len(MARKS)]] = MARKS
        v[at[-1]] = (int(rng.integers(0, 2)) << 15) | (int(rng.choice(BIG_EXPONENTS)) << 10) | (2 * int(rng.integers(0, 512)) + 1)
        rows = datagen._permuted_rows(rng, v, PER, width)
        rows[:, width:] = rng.integers(0, 1 << 16, size=(PER, d - width)).astype(np.uint16)
        pick = rng.permutation(PER)[:2 * DUPLICATES]
        rows[pick[DUPLICATES:]] = rows[pick[:DUPLICATES]]   # exact copies, tail included
        base[g * PER:(g + 1) * PER] = rows
    return np.ascontiguousarray(base.view(np.float16))


def _group_queries(rng, d):
    """c_g * (1, ..., 1): c_g = 100 + k / 2^17 with k odd (float32 has steps of 2^-17 there: every mantissa bit is in use)."""
    k = 2 * rng.integers(-(1 << 18), 1 << 18, size=GROUPS) + 1
    c = (np.float32(100.0) + k.astype(np.float32) / np.float32(1 << 17)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(c[:, None], d, axis=1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rerank_contest(d, metric):
    """dict: base float16 [N x d], wide its float32 table, gq [GROUPS x d] the groups' queries, queries [nq x d], cand [nq x 200] (the
    query's own group's rows in random order, 0xFFFFFFFF beyond count), count: twelve queries per entry of tu.RERANK_COUNTS.  The first list
    that holds more than one candidate starts with the table's last row."""
    rng = tu.rng_of(10800 + 2 * d + metric)
    base = _half_groups(rng, d, metric)
    gq = _group_queries(rng, d)
    count = np.repeat(np.array(tu.RERANK_COUNTS, np.int32), 12)
    qg = rng.integers(0, GROUPS, size=len(count))
    cand = np.full((len(count), max(tu.RERANK_COUNTS)), NONE, np.uint32)
    for i, (c, grp) in enumerate(zip(count, qg)):
        cand[i, :c] = grp * PER + rng.permutation(PER)[:c]
    first = int(np.flatnonzero(count > 1)[0])
    cand[first, 0] = N - 1   # the last row: whatever lies behind its padding must not be read into the sums
    return dict(base=base, wide=wide(base), gq=gq, queries=np.ascontiguousarray(gq[qg]), cand=cand, count=count)


@functools.lru_cache(maxsize=None)
def index_data(metric, d, dlow):
    """A contest index over half rows (tu.contest_index_data's recipe): the half contest as the original-space table, independent
    full-mantissa low-dimensional rows and queries, the groups disconnected components of contest_graph(rng, 8, 256, 2, 30), twelve queries
    per group (96) that share the group's original-space query and differ in their low-dimensional query and entry point, a full-mantissa net."""
    rng = tu.rng_of(10900 + 7 * d + 3 * dlow + metric)
    base = _half_groups(rng, d, metric)
    gq = _group_queries(rng, d)
    db_low = datagen.full_mantissa(rng, N, dlow)
    off, nbr = datagen.contest_graph(rng, GROUPS, PER, 2, 30)
    qg = np.repeat(np.arange(GROUPS), 12)
    q_low = datagen.full_mantissa(rng, len(qg), dlow)
    ent = (qg * PER + rng.integers(0, PER, size=len(qg))).astype(np.uint32)
    net = datagen.net_layers_full(rng, d, 64, dlow)
    return dict(base=base, wide=wide(base), gq=gq, db_low=db_low, off=off, nbr=nbr, qg=qg, queries=np.ascontiguousarray(gq[qg]), q_low=q_low,
                ent=ent, net=net)


def group_distance_bits(orc, base, gq, metric):
    """[GROUPS x PER] uint32: the bit pattern of the oracle's distance of every row of a group from the group's query, on the widened table."""
    f = orc.negdot if metric else orc.l2
    w = wide(base)
    out = np.empty((GROUPS, PER), np.uint32)
    for g in range(GROUPS):
        for r in range(PER):
            out[g, r] = np.float32(f(w[g * PER + r], gq[g])).view(np.uint32)
    return out


def marks_present(base, d, metric):
    """Per group: -0, both subnormals and a value of magnitude >= 2^14 among the coordinates the metric reads."""
    width = d if metric else 4 * (d // 4)
    b = bits_of(base)[:, :width]
    out = []
    for g in range(GROUPS):
        rows = b[g * PER:(g + 1) * PER]
        big = ((rows & 0x7FFF) >= (BIG_EXPONENTS[0] << 10)) & ((rows & 0x7C00) != 0x7C00)
        out.append(all((rows == m).any() for m in MARKS) and bool(big.any()))
    return out


# ---- widening is exact: one-hot rows ---------------------------------------------------------------------------------------------
ONE_HOT_MARKS = (0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x8000)
ONE_HOT_D = 32   # four chunks: two of the even lane's, two of the odd lane's


def one_hot_table():
    """float16 [6 * 32 x 32]: row (m, p) holds mark m at coordinate p and +0 elsewhere; p sweeps the eight places of all four chunks -- chunks
    0 and 2 are the even lane's, 1 and 3 the odd lane's."""
    t = np.zeros((len(ONE_HOT_MARKS) * ONE_HOT_D, ONE_HOT_D), np.uint16)
    for i, m in enumerate(ONE_HOT_MARKS):
        for p in range(ONE_HOT_D):
            t[i * ONE_HOT_D + p, p] = m
    return np.ascontiguousarray(t.view(np.float16))


def rows_that_differ(a, b):
    return int((a != b).any(axis=1).sum())
