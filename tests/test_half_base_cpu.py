"""The half-base handle (gbnns_index_create_half_base, Index(db=<float16>)) without a device: the exports, gbnns_debug_half_base_plan -- which
stand-alone kernel re-ranks binary16 rows of a given length --, the refusals that need no device, and the preconditions that keep
tests/test_gpu_half_base.py from passing vacuously: by the oracle on the widened table every group of every fixture holds distances that
differ in their bits (a kernel that added in another order cannot return the expected rows), a pair that is bit-equal (the pop index
decides), and the marks -0, 0x0001, 0x03FF and a value of magnitude >= 2^14.
"""
import ctypes as C

import numpy as np
import pytest

import half_base_util as hb


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_library_exports_the_half_base_entry_points(g):
    lib = g.load_library()
    for sym in ("gbnns_index_create_half_base", "gbnns_index_is_half_base", "gbnns_debug_half_base_plan"):
        assert hasattr(lib, sym), sym
        assert sym in g.binding.SYMBOLS, sym
    assert lib.gbnns_index_is_half_base(None) == 0


@pytest.mark.parametrize("d,metric", hb.RERANK_SHAPES + [(96, 1), (384, 0), (380, 0), (383, 0), (1, 0), (4, 0)], ids=lambda v: str(v))
def test_half_base_plan_names_the_kernel(g, d, metric):
    """Chunk pairs for L2 with d % 4 == 0, a lane per row otherwise; never fused; the loads in flight: the ladder's depth from d = 384 on (at
    least the four of the short rows), 4 below, 0 a lane per row."""
    name, deep, fused = g.half_base_plan(metric, d)
    assert fused is False
    if metric == 0 and d % 4 == 0:
        assert name == "rerank_half_pair_kernel"
        assert deep == 4 if d < 384 else deep >= 4
    else:
        assert name == "rerank_half_kernel<%d>" % metric and deep == 0
    # one depth for every long row
    assert g.half_base_plan(0, 384)[1] == g.half_base_plan(0, 960)[1]


def test_half_base_plan_refusals(g):
    lib = g.load_library()
    name, deep, fused = C.create_string_buffer(128), C.c_int(0), C.c_int(0)
    ok = (0, 96)
    assert lib.gbnns_debug_half_base_plan(*ok, name, 128, C.byref(deep), C.byref(fused)) == 0
    assert lib.gbnns_debug_half_base_plan(0, 0, name, 128, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(2, 96, name, 128, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(-1, 96, name, 128, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(*ok, None, 128, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(*ok, name, 0, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(*ok, name, 128, None, C.byref(fused)) == 1
    assert lib.gbnns_debug_half_base_plan(*ok, name, 128, C.byref(deep), None) == 1
    with pytest.raises(g.GbnnsError) as e:
        g.half_base_plan(0, 0)
    assert e.value.code == 1


def test_rerank_plan_is_unchanged_beside_it(g):
    """gbnns_debug_rerank_plan keeps its two row types: the half rows have a function of their own."""
    assert g.rerank_plan(0, 960) == ("rerank_pair_kernel<0>", 24, True)
    assert g.rerank_plan(0, 128, bytes=True) == ("rerank_bytes_pair_kernel", 4, True)


def _tiny(dtype):
    rng = np.random.Generator(np.random.PCG64(3))
    n, d = 8, 16
    db = rng.standard_normal((n, d)).astype(dtype)
    off = np.arange(n + 1, dtype=np.uint64)
    nbr = ((np.arange(n) + 1) % n).astype(np.uint32)
    return db, off, nbr, rng.standard_normal((n, 4)).astype(np.float32)


def test_create_reaches_the_library(g):
    """Index(db=<float16>) goes to gbnns_index_create_half_base: without a device that is the library's "no device" error (code 2), and without
    db_low the library's GBNNS_ERR_INVALID, which needs no device -- never a Python exception from the dtype path."""
    db, off, nbr, db_low = _tiny(np.float16)
    with pytest.raises(g.GbnnsError) as e:
        g.Index(db, off, nbr)
    assert e.value.code == 1 and "gbnns_index_create_half_base" in str(e.value), str(e.value)
    if g.device_count() == 0:
        with pytest.raises(g.GbnnsError) as e:
            g.Index(db, off, nbr, db_low=db_low)
        assert e.value.code == 2, str(e.value)
    lib = g.load_library()
    out = C.c_void_p()
    assert lib.gbnns_index_create_half_base(None, db.ctypes.data, C.byref(out)) == 1


def test_type_errors(g):
    """float16 queries are a TypeError on a half-base handle (queries are float32 there: the query is never rounded); a float16 table in
    another memory kind than db_low is the usual one."""
    torch = pytest.importorskip("torch")
    db, off, nbr, db_low = _tiny(np.float16)
    with pytest.raises(TypeError):
        g.Index(torch.from_numpy(db), off, nbr, db_low=db_low)   # (a pageable CPU tensor is neither a device nor a pinned buffer)

    class HalfBaseHandle:  # (what Index.search / rerank / rerank_topk look at before they touch the library)
        is_half_base = True
        is_bytes = False
        d = 16
    q16 = np.zeros((2, 16), np.float16)
    cand = np.zeros((2, 4), np.uint32)
    with pytest.raises(TypeError):
        g.Index.search(HalfBaseHandle(), q16, 8)
    with pytest.raises(TypeError):
        g.Index.search(HalfBaseHandle(), torch.zeros((2, 16), dtype=torch.float16), 8)
    with pytest.raises(TypeError):
        g.Index.rerank(HalfBaseHandle(), q16, cand)
    with pytest.raises(TypeError):
        g.Index.rerank_topk(HalfBaseHandle(), q16, cand, 2)


def _sound(bits, base, d, metric):
    assert all(hb.marks_present(base, d, metric)), hb.marks_present(base, d, metric)
    for grp in range(hb.GROUPS):
        b = bits[grp]
        assert len(np.unique(b)) >= 2, ("one distance only", grp)
        assert len(np.unique(b)) < len(b), ("no bit-equal pair", grp)
    assert np.isfinite(hb.wide(base)[:, :d if metric else 4 * (d // 4)]).all()


@pytest.mark.parametrize("d,metric", hb.RERANK_SHAPES, ids=["d%d_m%d" % s for s in hb.RERANK_SHAPES])
def test_rerank_fixture_is_sound(orc, d, metric):
    c = hb.rerank_contest(d, metric)
    assert c["base"].dtype == np.float16 and c["cand"][c["count"] > 0, 0].max() == hb.N - 1
    bits = hb.group_distance_bits(orc, c["base"], c["gq"], metric)
    print("half contest d %d metric %d: distinct distances per group" % (d, metric), [len(np.unique(b)) for b in bits])
    _sound(bits, c["base"], d, metric)


@pytest.mark.parametrize("metric,d,dlow", hb.INDEX_SHAPES, ids=["m%d_d%d_l%d" % s for s in hb.INDEX_SHAPES])
def test_index_fixture_is_sound(orc, metric, d, dlow):
    c = hb.index_data(metric, d, dlow)
    bits = hb.group_distance_bits(orc, c["base"], c["gq"], metric)
    _sound(bits, c["base"], d, metric)
    # the copies: three pairs of identical rows in every group
    for grp in range(hb.GROUPS):
        rows = hb.bits_of(c["base"])[grp * hb.PER:(grp + 1) * hb.PER]
        assert len(np.unique(rows, axis=0)) <= hb.PER - hb.DUPLICATES, grp


def test_one_hot_table_holds_every_mark_at_every_place():
    t = hb.bits_of(hb.one_hot_table())
    assert t.shape == (len(hb.ONE_HOT_MARKS) * hb.ONE_HOT_D, hb.ONE_HOT_D)
    for i, m in enumerate(hb.ONE_HOT_MARKS):
        block = t[i * hb.ONE_HOT_D:(i + 1) * hb.ONE_HOT_D]
        assert np.array_equal(block, np.eye(hb.ONE_HOT_D, dtype=np.uint16) * np.uint16(m))
    # widening the marks: subnormals stay, the zero keeps its sign
    w = hb.wide(hb.one_hot_table())
    assert w[0, 0] == np.float32(2.0 ** -24) and w[hb.ONE_HOT_D, 0] == np.float32(1023 * 2.0 ** -24)
    assert np.signbit(w[5 * hb.ONE_HOT_D, 0]) and w[5 * hb.ONE_HOT_D, 0] == 0
