"""gbnns_index_tag_census and gbnns_search_tagged_auto on an MI355X (run with -m gpu).  The census equals NumPy's; every row of the routed
search is, bit for bit, a row of one of the two existing calls -- the tagged (or bridged) walk's, or the exact tagged scan's -- and the
expectation is composed from their CPU-oracle expectations (tests/tag_auto_util.py).  tests/test_tag_auto_cpu.py proves that on every
configuration run here a query sent down the wrong route gets a different row.  Nothing takes a tolerance.
"""
import ctypes as C

import numpy as np
import pytest

import knn_tagged_util as kt
import locality_order_util as lo
import tag_auto_util as au
import tag_util as tg

pytestmark = pytest.mark.gpu

WANT = ("hops", "dist_calc", "cand", "cand_dist", "edges")
CENSUS_NS = (5, 63, 64, 65, 1037, 6000)


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _np(r):
    """search_auto's / tag_census's tensors as the numpy arrays the HOST call returns."""
    import torch
    torch.cuda.synchronize()
    out = {}
    for name, v in r.items():
        v = v.cpu().numpy()
        out[name] = v.view(np.uint32) if v.dtype == np.int32 and name in ("ids", "cand", "top_ids", "allowed", "first") else v
    return out


def _tiny_index(g, n):
    """n rows on a ring: the census needs a handle and a tag table, nothing of the search."""
    rng = np.random.default_rng(n)
    off = np.arange(n + 1, dtype=np.uint64)
    nbr = ((np.arange(n) + 1) % n).astype(np.uint32)
    return g.Index(rng.standard_normal((n, 8)).astype(np.float32), off, nbr)


def _index(g, c, metric, db=None, net=None):
    ix = g.Index(c["base"] if db is None else db, c["off"], c["nbr"], db_low=c["db_low"], net=net, metric=metric)
    ix.set_tags(c["T"])
    return ix


def _auto(g, ix, c, ef, k, sb, Q=None, ent=None, flags=0, queries=None, device=False, mode=None, want=WANT):
    Q = c["Q"] if Q is None else Q
    queries = c["queries"] if queries is None else queries
    mode = g.MODE_LOWQ if mode is None else mode
    q_low = c["q_low"] if mode == g.MODE_LOWQ else None
    if device:
        r = ix.search_auto(_dev(queries), ef, k, _dev(Q), scan_below=sb, mode=mode, queries_low=None if q_low is None else _dev(q_low),
                           entry_ids=None if ent is None else _dev(ent), want=want, flags=flags)
        return _np(r)
    return ix.search_auto(queries, ef, k, Q, scan_below=sb, mode=mode, queries_low=q_low, entry_ids=ent, want=want, flags=flags)


def _same_census(got, T, Q, what):
    import gbnns_dim_red_amd as g
    want = g.tag_census(T, Q)
    assert np.array_equal(np.asarray(got[0]).view(np.uint32), want[0]), (what, "allowed")
    assert np.array_equal(np.asarray(got[1]).view(np.uint32), want[1]), (what, "first")


# ---- 1. the census, every shape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CENSUS_NS)
def test_census_equals_numpy(g, n):
    """Rows below, at and above a wavefront's share, a tile and a half, several tiles -- n is no multiple of anything; 13 distinct words in
    300 (0, all ones, "last 40 rows only", "rows 0 .. 6 only" among them), 300 distinct words (the dedupe table takes collisions), the lane
    map, one query; HOST and DEVICE buffers; either output NULL."""
    ix = _tiny_index(g, n)
    T = kt.tag_table(n, n)
    ix.set_tags(T)
    few = kt.query_words(300)
    assert len(np.unique(few)) == 13
    many = np.random.default_rng(100 + n).choice(2 ** 32, 300, replace=False).astype(np.uint32)
    for what, Q in (("13 words", few), ("300 words", many), ("one query", few[9:10]), ("one query, word 0", few[10:11])):
        _same_census(ix.tag_census(Q), T, Q, (n, what, "host"))
        a, f = ix.tag_census(_dev(Q))
        r = _np(dict(allowed=a, first=f))
        _same_census((r["allowed"], r["first"]), T, Q, (n, what, "device"))
    # either output NULL, through the C ABI
    want = g.tag_census(T, few)
    for which in (0, 1):
        out = np.full(300, 0x5A5A5A5A, np.uint32)
        args = [None, None]
        args[which] = out.ctypes.data
        rc = ix._lib.gbnns_index_tag_census(ix._h, few.ctypes.data, 300, args[0], args[1], g.binding.MEM_HOST, None)
        assert rc == 0 and np.array_equal(out, want[which]), (n, which)
    assert ix._lib.gbnns_index_tag_census(ix._h, few.ctypes.data, 300, None, None, g.binding.MEM_HOST, None) == 1
    assert ix._lib.gbnns_index_tag_census(ix._h, None, 0, None, want[0].ctypes.data, g.binding.MEM_HOST, None) == 0   # no queries: nothing to do
    # the lane map: one row of every 32 allowed, at a position of its own per query
    T2, Q2 = kt.lane_map_tags(n, 70)
    ix.set_tags(T2)
    _same_census(ix.tag_census(Q2), T2, Q2, (n, "lane map", "host"))
    a, f = ix.tag_census(_dev(Q2))
    r = _np(dict(allowed=a, first=f))
    _same_census((r["allowed"], r["first"]), T2, Q2, (n, "lane map", "device"))
    ix.close()


# ---- 2. nothing is cached --------------------------------------------------------------------------------------------------------
def test_census_follows_set_tags(g):
    n = 1037
    ix = _tiny_index(g, n)
    Q = kt.query_words(70)
    with pytest.raises(g.GbnnsError) as e:   # no table yet
        ix.tag_census(Q)
    assert e.value.code == 1
    T = kt.tag_table(1, n)
    ix.set_tags(T)
    _same_census(ix.tag_census(Q), T, Q, "first table")
    patch = kt.tag_table(2, 50) ^ np.uint32(0x3FF)
    ix.set_tags(patch, first=100)
    T2 = T.copy()
    T2[100:150] = patch
    assert not np.array_equal(np.stack(g.tag_census(T, Q)), np.stack(g.tag_census(T2, Q)))
    _same_census(ix.tag_census(Q), T2, Q, "patched table")
    ix.clear_tags()
    with pytest.raises(g.GbnnsError) as e:
        ix.tag_census(Q)
    assert e.value.code == 1
    ix.close()


# ---- 3. routing, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,ef,k,bridge", au.CONFIGS, ids=["m%d_ef%d_k%d_bridge%d" % s for s in au.CONFIGS])
def test_every_row_is_a_row_of_its_route(g, orc, metric, ef, k, bridge):
    """LOWQ on the main fixture: the one-register list (ef 8, 64) and the two-list kernel (200), every scan_below at ef 64 -- 1 023 / 1 024 put
    the words of 1 024 rows on the two sides of the boundary --, entered at the lowest allowed row and at the fixture's random entries (some
    walk-routed queries may not see theirs: the empty row)."""
    c = au.fixture(metric)
    ix = _index(g, c, metric)
    flags = g.FLAG_TAG_BRIDGE if bridge else 0
    failures = []
    for sb in au.scan_below_of(ef):
        for ent in ((None, c["ent"]) if sb == 300 else (None,)):
            e = au.expected(orc, ("fixture", metric), c, ef, k, metric, sb, ent=ent, bridge=bridge)
            r = _auto(g, ix, c, ef, k, sb, ent=ent, flags=flags)
            bad = au.differences(r, e)
            scan = e["route"] == 1
            if not (r["edges"][scan] == 0).all():
                bad.append("edges of scan-routed queries")
            # the same call with the walk of the whole batch in locality order: a work item walks under the word the ROUTING gave its query
            # (0 for a scan-routed one) from that query's entry, and the scan's rows are scattered over the walk's afterwards
            ro, in_order = lo.in_order(ix, c["q_low"], lambda: _auto(g, ix, c, ef, k, sb, ent=ent, flags=flags))
            in_order += lo.same_bytes(ro, r, ("ids", "top_ids", "top_dist", "allowed", "route") + WANT)
            bad += ["in order: " + b for b in in_order]
            print("auto", metric, ef, k, bridge, sb, "given entries" if ent is not None else "first", "scan-routed", int(scan.sum()), bad)
            if bad:
                failures.append((sb, ent is not None, bad))
            if ent is not None:   # the case is not vacuous: some walk-routed query has a disallowed entry
                assert (~scan & ~tg.entry_ok(c["T"], c["Q"], ent)).any()
    ix.close()
    assert not failures, failures


# ---- 4. NET mode ---------------------------------------------------------------------------------------------------------------------
def test_net_mode_projects_every_query(g, orc):
    metric, d, dlow, ef, k, sb = 0, 128, 32, 64, 10, 300
    c = dict(tg.contest(metric, d, dlow))
    c["Q"] = au.query_words(len(c["q_low"]))
    ix = _index(g, c, metric, net=c["net"])
    proj = ix.project(c["queries"])
    r = _auto(g, ix, c, ef, k, sb, mode=g.MODE_NET, want=WANT + ("q_low",))
    assert r["q_low"].view(np.uint32).tobytes() == proj.view(np.uint32).tobytes()   # scan-routed queries included
    e = au.expected(orc, ("contest", metric, d, dlow), c, ef, k, metric, sb, q_low=proj)
    assert 0 < (e["route"] == 1).sum() < len(c["Q"])
    assert not au.differences(r, e), au.differences(r, e)
    ix.close()


# ---- 5. byte handle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_byte_handle_equals_the_float_handle_over_the_widened_table(g, metric):
    c = au.fixture(metric)
    base8, q8 = au.quantised(c)
    ixb = _index(g, c, metric, db=base8)
    ixf = _index(g, c, metric, db=base8.astype(np.float32))
    assert ixb.is_bytes and not ixf.is_bytes
    for ef, k, sb, flags in ((64, 10, 300, 0), (8, 1, 1024, g.FLAG_TAG_BRIDGE), (200, 10, 0, 0), (64, 1, 2 ** 64 - 1, 0)):
        rb = _auto(g, ixb, c, ef, k, sb, flags=flags, queries=q8)
        rf = _auto(g, ixf, c, ef, k, sb, flags=flags, queries=q8.astype(np.float32))
        assert set(rb) == set(rf)
        for name in rb:
            assert rb[name].tobytes() == rf[name].tobytes(), (ef, k, sb, name)
        assert np.array_equal(rb["route"], au.routes(rb["allowed"], sb).astype(np.uint8))
    rd = _auto(g, ixb, c, 64, 10, 300, queries=q8, device=True)   # (DEVICE buffers on the byte handle: the same bytes)
    rb = _auto(g, ixb, c, 64, 10, 300, queries=q8)
    for name in rb:
        assert rd[name].tobytes() == rb[name].tobytes(), ("device", name)
    with pytest.raises(g.GbnnsError) as e:   # there is no mixed-pair scan
        _auto(g, ixb, c, 64, 10, 300, queries=q8.astype(np.float32))
    assert e.value.code == 5
    with pytest.raises(TypeError):
        _auto(g, ixf, c, 64, 10, 300, queries=q8)
    ixb.close()
    ixf.close()


# ---- 6. DEVICE buffers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bridge", [False, True])
def test_device_buffers_equal_host_buffers(g, orc, bridge):
    metric, ef, k, sb = 0, 64, 10, 300
    c = au.fixture(metric)
    ix = _index(g, c, metric)
    flags = g.FLAG_TAG_BRIDGE if bridge else 0
    for ent in (None, c["ent"]):
        rh = _auto(g, ix, c, ef, k, sb, ent=ent, flags=flags)
        rd = _auto(g, ix, c, ef, k, sb, ent=ent, flags=flags, device=True)
        assert set(rh) == set(rd)
        for name in rh:
            assert rd[name].tobytes() == rh[name].tobytes(), (name, ent is not None)
        e = au.expected(orc, ("fixture", metric), c, ef, k, metric, sb, ent=ent, bridge=bridge)
        assert not au.differences(rd, e), au.differences(rd, e)
    ix.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(g, orc):
    metric, ef, k, sb = 0, 64, 10, 300
    c = au.fixture(metric)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    with pytest.raises(g.GbnnsError) as e:   # no tag table
        _auto(g, ix, c, ef, k, sb)
    assert e.value.code == 1
    ix.set_tags(c["T"])
    ix.enable_half_rows()
    for what, code, kw in (("PLAIN", 1, dict(mode=g.MODE_PLAIN)), ("k = 0", 1, dict(k=0)), ("k = ef + 1", 1, dict(k=ef + 1)),
                           ("DEFER_JOIN", 5, dict(flags=g.FLAG_DEFER_JOIN)), ("HALF_ROWS", 5, dict(flags=g.FLAG_HALF_ROWS)),
                           ("MFMA_PROJECTION", 5, dict(flags=g.FLAG_MFMA_PROJECTION))):
        args = dict(ef=ef, k=k, sb=sb)
        args.update(kw)
        with pytest.raises(g.GbnnsError) as e:
            _auto(g, ix, c, **args)
        assert e.value.code == code, (what, e.value)
    # no out_top_ids: through the C ABI
    b = g.binding
    ids = np.empty(len(c["Q"]), np.uint32)
    a = b._SearchArgs(struct_size=C.sizeof(b._SearchArgs), mode=b.MODE_LOWQ, ef=ef, k=ef, mem_kind=b.MEM_HOST, n_q=len(c["Q"]),
                      queries=c["queries"].ctypes.data, queries_low=c["q_low"].ctypes.data, out_ids=ids.ctypes.data)
    assert ix._lib.gbnns_search_tagged_auto(ix._h, C.byref(a), None, c["Q"].ctypes.data, k, sb, None, None, None, None) == 1
    assert ix._lib.gbnns_search_tagged_auto(ix._h, C.byref(a), None, None, k, sb, ids.ctypes.data, None, None, None) == 1   # no query_tags
    # ... and with them, without the optional outputs: served
    top = np.empty((len(c["Q"]), k), np.uint32)
    assert ix._lib.gbnns_search_tagged_auto(ix._h, C.byref(a), None, c["Q"].ctypes.data, k, sb, top.ctypes.data, None, None, None) == 0
    e = au.expected(orc, ("fixture", metric), c, ef, k, metric, sb)
    assert np.array_equal(top, e["top_ids"]) and np.array_equal(ids, e["ids"])
    r = _auto(g, ix, c, ef, k, sb)
    assert not au.differences(r, e), au.differences(r, e)
    ix.close()
