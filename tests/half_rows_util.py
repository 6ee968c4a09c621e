"""What tests/test_half_rows_cpu.py and tests/test_gpu_half_rows.py share: the shapes, the fixtures and the expected kernel names of
GBNNS_FLAG_HALF_ROWS.

The contract under test: a search with half rows is the reference's search on R = float32(float16(db_low)), so every expected value is
the oracle's on `rounded(db_low)` -- NumPy's own binary16 round trip, which gbnns_round_to_half is tested against.
"""
import functools

import numpy as np

import datagen
import topk_util as tu

NQ = 96
SHAPES = [(0, 128, 32), (0, 96, 48), (0, 960, 64), (0, 300, 144), (1, 200, 32)]   # (metric, d, d_low): the contest indexes
BEAMS = (8, 64, 100, 200)
# adjacency rows of 33 .. 48 slots (two passes of the pair form): every walked width that has half instances
TWO_PASS_SHAPES = [(0, 32), (1, 32), (0, 48), (0, 64), (0, 144)]               # (metric, d_low)
D_ORIG = 40                                                                    # their original space (d % 8 == 0: the re-rank is fused)

# float32 values around every rounding decision of binary16, each with the value it rounds to
EDGES = [
    (0.0, 0.0), (-0.0, -0.0),
    (1.0 + 2.0 ** -11, 1.0), (1.0 + 3 * 2.0 ** -11, 1.001953125),             # ties to even, down and up
    (2.0 ** -24, 2.0 ** -24), (2.0 ** -25, 0.0), (1.5 * 2.0 ** -25, 2.0 ** -24), (-(2.0 ** -25), -0.0),   # the smallest subnormal, the tie below it
    (2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -14),                              # the largest subnormal's upper neighbour rounds to the smallest normal
    (65504.0, 65504.0), (65519.99, 65504.0), (-65519.99, -65504.0),
]
OUT_OF_RANGE = [65520.0, np.inf, np.nan, -65520.0, -np.inf]


def rounded(a):
    """R of the contract, by NumPy: round to nearest-even binary16, widen back."""
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16).astype(np.float32))


def edge_values():
    return np.array([e[0] for e in EDGES], np.float32), np.array([e[1] for e in EDGES], np.float32)


def contest(metric, d, dlow):
    """tu.contest_index_data plus R (read-only, shared)."""
    return _contest(metric, d, dlow)


@functools.lru_cache(maxsize=None)
def _contest(metric, d, dlow):
    c = dict(tu.contest_index_data(metric, d, dlow))
    c["R"] = rounded(c["db_low"])
    return c


@functools.lru_cache(maxsize=None)
def two_pass(metric, dlow):
    """Full-mantissa walked rows and queries over datagen.random_graph(rng, 2048, 33, 48): adjacency rows of two 32-slot passes."""
    rng = tu.rng_of(8800 + 10 * dlow + metric)
    n = 2048
    off, nbr = datagen.random_graph(rng, n, 33, 48)
    db_low = datagen.full_mantissa(rng, n, dlow)
    return dict(base=datagen.full_mantissa(rng, n, D_ORIG), queries=datagen.full_mantissa(rng, NQ, D_ORIG), db_low=db_low, R=rounded(db_low),
                q_low=datagen.full_mantissa(rng, NQ, dlow), ent=rng.integers(0, n, size=NQ).astype(np.uint32), off=off, nbr=nbr)


@functools.lru_cache(maxsize=None)
def clustered_index(dlow=32):
    """A contest index whose walked rows are datagen.clustered's multiples of 1 / 256 (|k| <= 88): exactly representable in binary16, so
    R == db_low, and full of equal distances."""
    c = dict(tu.contest_index_data(0, 128, dlow))
    rng = tu.rng_of(8900 + dlow)
    c["db_low"] = datagen.clustered(rng, len(c["base"]), dlow)
    c["q_low"] = datagen.clustered(rng, len(c["qg"]), dlow)
    c["R"] = rounded(c["db_low"])
    return c


SUB_GROUP = 3   # the contest group whose walked rows are binary16 subnormals


@functools.lru_cache(maxsize=None)
def subnormal_index():
    """The (0, 128, 32) contest index with one component (group SUB_GROUP) whose walked rows are k * 2^-24, |k| <= 1 000: binary16
    subnormals (below 2^-14), exactly representable, and a query batch of the same scale entering that group.  A device that flushed
    binary16 subnormals would see every one of those rows as zero."""
    c = dict(tu.contest_index_data(0, 128, 32))
    rng = tu.rng_of(8950)
    lo, hi = SUB_GROUP * tu.PER, (SUB_GROUP + 1) * tu.PER
    db_low = c["db_low"].copy()
    db_low[lo:hi] = (rng.integers(-1000, 1001, size=(tu.PER, 32)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    q_low = c["q_low"].copy()
    sub = np.flatnonzero(c["qg"] == SUB_GROUP)
    q_low[sub] = (rng.integers(-1000, 1001, size=(len(sub), 32)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    c["db_low"], c["q_low"], c["sub_queries"] = db_low, q_low, sub
    c["R"] = rounded(db_low)
    flushed = c["R"].copy()
    flushed[np.abs(flushed) < np.float32(2.0 ** -14)] = 0.0
    c["R_flushed"] = flushed
    return c


def half_kernel(metric, dlow, ef, one_pass, late=False):
    """The first-pass kernel a flagged search of a compact index launches (one entry point, no auxiliary graph, no two-wavefront walk, no
    bitmap pass): by the domain of the half instances -- rows of 32 / 48 / 64 floats with L2 and of 32 floats with the negative dot in
    the one- / two-register-list and two-list kernels, rows of 144 floats with L2 in the two-list kernel -- else the float32 instance."""
    steps, one = dlow // 4, "true" if one_pass else "false"
    if dlow == 144 and ef <= 128:  # the run-time-length float32 instances (one pass: up to 64 slots a lane per row)
        return "walk_reg_kernel<0, 0, true, false, %d, %s, false>" % ((1, "true") if ef <= 64 else (2, "false"))
    if ef <= 64:
        return "walk_reg_half_kernel<%d, %d, 1, %s>" % (metric, steps, one)
    if ef <= 128:
        return "walk_reg_half_kernel<%d, %d, 2, false>" % (metric, steps)
    return "walk_reg_big_half_kernel<%d, %d, %s, %s>" % (metric, steps, one, "true" if late else "false")


def rows_that_differ(a, b):
    return int((a != b).any(axis=1).sum())
