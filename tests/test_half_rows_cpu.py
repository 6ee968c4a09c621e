"""GBNNS_FLAG_HALF_ROWS without a device: gbnns_round_to_half -- the definition of the walked table R = float32(float16(db_low)) --
against NumPy's binary16 round trip, argument validation of the handle calls, and the preconditions that keep
tests/test_gpu_half_rows.py from passing vacuously: on every fixture the oracle's walk over R differs from its walk over db_low, so a
kernel that walked the wrong table cannot equal the expected values, and the exactly representable table equals its own R.
"""
import ctypes as C
import re

import numpy as np
import pytest

import golden_util as gu
import half_rows_util as hu
import topk_util as tu


@pytest.fixture(scope="module")
def lib():
    import gbnns_dim_red_amd as g
    return g.load_library()


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _round(lib, a, want_bits=True, want_wide=True):
    a = np.ascontiguousarray(a, np.float32)
    bits = np.full(a.shape, 0xDEAD, np.uint16)
    wide = np.full(a.shape, 123.0, np.float32)
    rc = lib.gbnns_round_to_half(a.ctypes.data, a.size, bits.ctypes.data if want_bits else None, wide.ctypes.data if want_wide else None)
    return rc, bits, wide


def test_round_to_half_equals_numpy(lib, g):
    """10^5 full-mantissa values over the whole binary16 range (subnormal results included) plus the edge list: the bits equal
    NumPy's float16 conversion, the widened values its round trip, bit for bit (the sign of zero included); each output alone too."""
    rng = tu.rng_of(8700)
    mant = rng.integers(1 << 23, 1 << 24, size=100000).astype(np.float32) / np.float32(1 << 23)          # [1, 2), 24 bits
    vals = (mant * np.exp2(rng.integers(-28, 16, size=mant.size)).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=mant.size)).astype(np.float32)
    vals = vals[np.abs(vals) < 65520.0]
    edge_in, edge_out = hu.edge_values()
    a = np.concatenate([vals, edge_in])
    want_bits = a.astype(np.float16).view(np.uint16)
    want_wide = a.astype(np.float16).astype(np.float32)
    assert (np.abs(want_wide[:len(vals)]) < 2.0 ** -14).sum() > 5000 and (want_wide[:len(vals)] == 0).sum() > 1000   # subnormal and zero results occur
    assert np.array_equal(gu.bits(want_wide[len(vals):]), gu.bits(edge_out)), "the edge list's expected values are NumPy's"
    rc, bits, wide = _round(lib, a)
    assert rc == 0
    assert np.array_equal(bits, want_bits), np.flatnonzero(bits != want_bits)[:8]
    assert np.array_equal(gu.bits(wide), gu.bits(want_wide))
    rc, bits, wide = _round(lib, a, want_wide=False)
    assert rc == 0 and np.array_equal(bits, want_bits) and (wide == 123.0).all()
    rc, bits, wide = _round(lib, a, want_bits=False)
    assert rc == 0 and np.array_equal(gu.bits(wide), gu.bits(want_wide)) and (bits == 0xDEAD).all()
    # the binding's form
    b2, w2 = g.round_to_half(a.reshape(-1, 1))
    assert b2.shape == (a.size, 1) and np.array_equal(b2.ravel(), want_bits) and np.array_equal(gu.bits(w2.ravel()), gu.bits(want_wide))
    assert lib.gbnns_round_to_half(None, 0, None, None) == 0


@pytest.mark.parametrize("bad", hu.OUT_OF_RANGE, ids=[str(v) for v in hu.OUT_OF_RANGE])
def test_round_to_half_refuses_what_leaves_the_range(lib, g, bad):
    """A value that is not finite, or rounds to 2^16 (|x| >= 65 520), is GBNNS_ERR_UNSUPPORTED and the message names its index."""
    a = np.array([1.0, -2.5, 65519.99, bad, np.inf], np.float32)
    rc, bits, wide = _round(lib, a)
    assert rc == 5
    msg = lib.gbnns_last_error().decode()
    assert re.findall(r"\d+", msg.split(":", 1)[1])[0] == "3", msg   # the first offending value, not the infinity behind it
    assert np.array_equal(bits[:3], a[:3].astype(np.float16).view(np.uint16))
    with pytest.raises(g.GbnnsError) as e:
        g.round_to_half(a)
    assert e.value.code == 5


def test_handle_calls_refuse_a_null_handle(lib):
    out = np.zeros(4, np.float32)
    assert lib.gbnns_index_enable_half_rows(None) == 1
    assert lib.gbnns_index_low_rows(None, out.ctypes.data, 0, None) == 1
    assert lib.gbnns_round_to_half(None, 3, None, None) == 1


def test_flag_and_symbols(g):
    from gbnns_dim_red_amd import binding
    assert g.FLAG_HALF_ROWS == 512 and binding.FLAG_HALF_ROWS == 512
    for name in ("gbnns_round_to_half", "gbnns_index_enable_half_rows", "gbnns_index_low_rows"):
        assert name in binding.SYMBOLS and hasattr(g.load_library(), name)
    assert g.version() == 100


@pytest.mark.parametrize("metric,d,dlow", hu.SHAPES, ids=["m%d_d%d_low%d" % s for s in hu.SHAPES])
def test_rounding_changes_the_walks_of_the_contest_indexes(orc, metric, d, dlow):
    """Non-vacuity: rounding changes nearly every coordinate, every row of distance bits, and at ef 64 the candidate ids of at least 24
    of the 96 queries (measured: 33 .. 45)."""
    c = hu.contest(metric, d, dlow)
    assert (c["R"] != c["db_low"]).mean() > 0.95
    a = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], 64, entries=c["ent"], metric=metric, threads=8)
    b = orc.walk(c["q_low"], c["R"], c["off"], c["nbr"], 64, entries=c["ent"], metric=metric, threads=8)
    differ = hu.rows_that_differ(a["ids"], b["ids"])
    print("half rows: contest", (metric, d, dlow), "ef 64: candidate rows that differ", differ)
    assert differ >= 24, differ
    assert hu.rows_that_differ(gu.bits(a["dists"]), gu.bits(b["dists"])) == len(c["q_low"])


@pytest.mark.parametrize("metric,dlow", hu.TWO_PASS_SHAPES, ids=["m%d_low%d" % s for s in hu.TWO_PASS_SHAPES])
def test_rounding_changes_the_walks_of_the_two_pass_graphs(orc, metric, dlow):
    c = hu.two_pass(metric, dlow)
    assert int(np.diff(c["off"].astype(np.int64)).max()) > 32 and int(np.diff(c["off"].astype(np.int64)).max()) <= 48   # two passes of 32 slots
    a = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], 64, entries=c["ent"], metric=metric, threads=8)
    b = orc.walk(c["q_low"], c["R"], c["off"], c["nbr"], 64, entries=c["ent"], metric=metric, threads=8)
    differ = hu.rows_that_differ(a["ids"], b["ids"])
    print("half rows: two-pass", (metric, dlow), "ef 64: candidate rows that differ", differ)
    assert differ >= 24, differ


def test_exactly_representable_table_equals_its_own_r(orc):
    """datagen.clustered's multiples of 1 / 256 are binary16 values: the table is its own R.  Such data holds equal distances: at ef 200
    at least 20 of the 96 candidate lists contain some (measured: 37), so the identical-bytes test on the device covers tie handling."""
    c = hu.clustered_index()
    assert np.array_equal(gu.bits(c["R"]), gu.bits(c["db_low"]))
    w = orc.walk(c["q_low"], c["R"], c["off"], c["nbr"], 200, entries=c["ent"], metric=0, threads=8)
    assert sum(len(np.unique(row)) < len(row) for row in w["dists"]) >= 20


def test_subnormal_component_is_decided_by_its_subnormals(orc):
    """The rows of one component are binary16 subnormals, exactly representable (R keeps them); with those values flushed to zero the
    oracle returns other candidate rows for every query that enters the component."""
    c = hu.subnormal_index()
    lo, hi = hu.SUB_GROUP * tu.PER, (hu.SUB_GROUP + 1) * tu.PER
    assert np.array_equal(gu.bits(c["R"][lo:hi]), gu.bits(c["db_low"][lo:hi]))
    assert (np.abs(c["R"][lo:hi]) < 2.0 ** -14).all() and (c["R"][lo:hi] != 0).mean() > 0.99 and (c["R_flushed"][lo:hi] == 0).all()
    sub = c["sub_queries"]
    assert len(sub) == 12
    for ef in (8, 64):
        a = orc.walk(c["q_low"][sub], c["R"], c["off"], c["nbr"], ef, entries=c["ent"][sub], metric=0, threads=4)
        b = orc.walk(c["q_low"][sub], c["R_flushed"], c["off"], c["nbr"], ef, entries=c["ent"][sub], metric=0, threads=4)
        assert hu.rows_that_differ(a["ids"], b["ids"]) == len(sub), ef
