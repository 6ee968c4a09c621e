"""gbnns_index_exact_knn_gather without a device: the exports, the refusals that need no handle, the kernel gbnns_debug_gather_plan names per
shape (and the existing scan's where the gathered kernel does not serve), gbnns_debug_gather_schedule -- the host function the call runs --
against a numpy restatement, and the preconditions that keep the GPU cases of tests/test_gpu_knn_gather.py from being vacuous."""
import ctypes as C

import numpy as np
import pytest

import knn_bytes_util as ku
import knn_gather_util as gu
import knn_tagged_util as tu


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports_and_refusals(g):
    lib = g.load_library()
    for name in ("gbnns_index_exact_knn_gather", "gbnns_debug_gather_plan", "gbnns_debug_gather_schedule"):
        assert name in g.binding.SYMBOLS and hasattr(lib, name), name
    assert g.FLAG_SCAN_GATHER == 4096 and g.FLAG_SCAN_GATHER & (g.FLAG_BYTE_WALK | g.FLAG_TAG_BRIDGE) == 0
    q, qb = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.uint8)
    tags, ids = np.ones(4, np.uint32), np.zeros((4, 3), np.uint32)
    call = lambda *a: lib.gbnns_index_exact_knn_gather(*a)
    err = lambda: lib.gbnns_last_error().decode()
    # this call's own refusals come before the handle is looked at
    assert call(None, q.ctypes.data, None, 4, None, 3, -1, ids.ctypes.data, None, 0, None) == 1 and "query_tags" in err()
    assert call(None, q.ctypes.data, None, 4, tags.ctypes.data, 0, -1, ids.ctypes.data, None, 0, None) == 1 and "k must be" in err()
    assert call(None, q.ctypes.data, qb.ctypes.data, 4, tags.ctypes.data, 3, -1, ids.ctypes.data, None, 0, None) == 1 and "exactly one" in err()
    assert call(None, None, None, 4, tags.ctypes.data, 3, -1, ids.ctypes.data, None, 0, None) == 1 and "exactly one" in err()
    assert call(None, q.ctypes.data, None, 4, tags.ctypes.data, 3, -1, ids.ctypes.data, None, 0, None) == 1 and "null argument" in err()


@pytest.mark.parametrize("bytes_", (False, True))
def test_plan(g, bytes_):
    u8 = "true" if bytes_ else "false"
    for metric, ds in ((ku.L2, (8, 30, 100, 128)), (ku.NEG_DOT, (8, 128))):
        for d in ds:
            s, qpt = (8, 2) if d <= 32 else (16, 2) if d <= 64 else (32, 1)
            for k in (1, 10, 4096):
                name, w = g.gather_plan(bytes_, metric, d, k)
                assert name == f"knn_gather_kernel<{metric}, {s}, {qpt}, {u8}>", (metric, d, k, name)
                assert w == 128 * qpt
    for d in (132, 192):   # wider rows: the existing scan, tagged -- the fallback inside the same call
        name, w = g.gather_plan(bytes_, ku.L2, d, 10)
        assert name == g.knn_plan(bytes_, ku.L2, 6000, 300, d, 10, tagged=True)[0] and "gather" not in name and w == 0, (d, name)
        assert name.startswith("knn_bytes_sweep_kernel<" if bytes_ else "knn_scan_wide_kernel<")
    if not bytes_:   # lists the heaps do not take
        name, w = g.gather_plan(False, ku.L2, 32, 5000)
        assert name.startswith("knn_scan_kernel<") and name.endswith("true>") and w == 0
    lib, buf, w = g.load_library(), C.create_string_buffer(128), C.c_uint32(0)
    assert lib.gbnns_debug_gather_plan(0, ku.NEG_DOT, 30, 10, buf, 128, C.byref(w)) == 5    # the negative dot needs d % 8 == 0
    assert lib.gbnns_debug_gather_plan(1, ku.L2, 300, 10, buf, 128, C.byref(w)) == 5        # a byte row's limit
    assert lib.gbnns_debug_gather_plan(0, ku.L2, 30, 0, buf, 128, C.byref(w)) == 1
    assert lib.gbnns_debug_gather_plan(0, ku.L2, 30, 10, None, 128, C.byref(w)) == 1


def _same_schedule(g, words, allowed, n, budget, W):
    got, want = g.gather_schedule(words, allowed, n, budget=budget, W=W), gu.schedule(words, allowed, budget, W)
    for key in ("order", "round_of", "list_offset_of"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, budget, W)
    assert (got["rounds"], got["workgroups"]) == (want["rounds"], want["workgroups"])
    nq = len(words)
    assert np.array_equal(np.sort(got["order"]), np.arange(nq))   # a permutation
    # every query that may see something lies inside its group's list range, lists of a round back to back without overlap
    live = np.nonzero(np.asarray(allowed) > 0)[0]
    assert (got["round_of"][live] != 0xFFFFFFFF).all() and (got["round_of"][np.asarray(allowed) == 0] == 0xFFFFFFFF).all()
    for r in range(got["rounds"]):
        spans = sorted({(int(got["list_offset_of"][i]), int(allowed[i]), int(words[i])) for i in live if got["round_of"][i] == r})
        assert spans and spans[0][0] == 0
        for (o0, l0, _), (o1, _, _) in zip(spans, spans[1:]):
            assert o0 + l0 == o1
        total = spans[-1][0] + spans[-1][1]
        assert total <= budget or len(spans) == 1   # a round within the budget, or one group alone
    return want


def test_schedule(g):
    n, nq = gu.N_ROUNDS, gu.NQ_ROUNDS
    T = gu.tag_table(n + 30, n)
    Q = gu.query_words(nq)
    allowed = gu.census(T, Q)
    assert np.array_equal(allowed, g.tag_census(T, Q)[0])
    W = g.gather_plan(False, ku.L2, 128, 10)[1]
    assert W == 128 and g.gather_plan(False, ku.L2, 30, 10)[1] == 256
    largest = int(allowed.max())
    assert largest == n
    for w in (128, 256):
        default = _same_schedule(g, Q, allowed, n, max(g.binding.GATHER_BUDGET, n), w)
        assert default["rounds"] == 1 and len(default["groups"]) == 14   # 15 distinct words, one of them 0
        # budget n: what the GPU rounds test runs (the call never takes a budget below n)
        at_n = _same_schedule(g, Q, allowed, n, n, w)
        assert at_n["rounds"] >= 3
        quarter = _same_schedule(g, Q, allowed, n, n // 4, w)
        assert quarter["rounds"] > at_n["rounds"]
        below = _same_schedule(g, Q, allowed, n, largest - 1, w)
        assert below["rounds"] >= 3
        alone = [grp for grp in below["groups"] if grp[1] > largest - 1]
        assert alone and all(sum(1 for o in below["groups"] if o[3] == grp[3]) == 1 for grp in alone)   # longer than the budget: a round of its own
    assert g.gather_schedule(Q, allowed, n)["rounds"] == 1   # budget=None: the default
    # one word for every query: more queries than W, hence several workgroups on one list
    one = np.full(nq, 1 << 1, np.uint32)
    a_one = gu.census(T, one)
    for w in (128, 256):
        s = _same_schedule(g, one, a_one, n, n, w)
        assert nq > w and s["rounds"] == 1 and s["workgroups"] == -(-nq // w) >= 2 and len(s["groups"]) == 1
    # 300 distinct words: every group has one query
    distinct = (np.arange(nq, dtype=np.uint32) * 2 + 1).astype(np.uint32)   # odd words: bit 0, every row
    assert np.unique(distinct).size == nq
    a_d = gu.census(T, distinct)
    assert (a_d == n).all()
    s = _same_schedule(g, distinct, a_d, n, n, W)
    assert s["workgroups"] == nq and s["rounds"] == nq
    s = _same_schedule(g, distinct, a_d, n, 4 * n, W)
    assert s["workgroups"] == nq and s["rounds"] == nq // 4
    # words that allow nothing: no group, no round, no workgroup
    nothing = np.where(np.arange(nq) % 2 == 0, 0, 1 << 20).astype(np.uint32)
    a_0 = gu.census(T, nothing)
    assert (a_0 == 0).all()
    s = _same_schedule(g, nothing, a_0, n, n, W)
    assert s["rounds"] == 0 and s["workgroups"] == 0 and np.array_equal(s["order"], np.arange(nq))
    # refusals of the diagnostic
    lib = g.load_library()
    o, r, off, nr, nw = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint64), C.c_uint32(0), C.c_uint32(0)
    w4, a4 = np.ones(4, np.uint32), np.full(4, 9, np.uint32)
    args = lambda n_, b, W_: (w4.ctypes.data, a4.ctypes.data, 4, n_, b, W_, o.ctypes.data, r.ctypes.data, off.ctypes.data, C.byref(nr), C.byref(nw))
    assert lib.gbnns_debug_gather_schedule(*args(8, 8, 128)) == 1      # allowed > n
    assert lib.gbnns_debug_gather_schedule(*args(9, 8, 0)) == 1        # W == 0
    assert lib.gbnns_debug_gather_schedule(*args(9, 0, 128)) == 1      # budget == 0
    assert lib.gbnns_debug_gather_schedule(*args(9, 8, 128)) == 0 and nr.value == 1 and nw.value == 1


def test_fixture_preconditions():
    """The list lengths the GPU cases contain: 0, 7, 40, exactly 64, exactly 128, one above 1 000 that is no multiple of 64, and n itself;
    32 distinct words in the lane-map case; equal rows on both sides of the tag test in the tie case."""
    for n in (1037, 6000):
        T = gu.tag_table(n + 30, n)
        lengths = {int(w): int(np.count_nonzero(T & np.uint32(w))) for w in gu.QUERY_WORDS}
        assert lengths[0] == 0 and lengths[1 << tu.FEW_BIT] == 7 and lengths[1 << tu.LATE_BIT] == 40
        assert lengths[1 << gu.TILE_BIT] == 64 and lengths[1 << gu.TWO_TILE_BIT] == 128
        assert lengths[tu.ALL] == n and lengths[1] == n
        rows = np.nonzero(T & np.uint32(1 << gu.TILE_BIT))[0]
        assert rows[0] == 0 and rows[-1] >= n - n // 32 and (np.diff(rows) >= n // 64 - 1).all()   # spread over the table
    T = gu.tag_table(6030, 6000)
    assert any(v > 1000 and v % 64 for v in (int(np.count_nonzero(T & np.uint32(1 << b))) for b in range(1, 4)))
    assert np.count_nonzero(gu.tag_table(35, 5) & np.uint32(1 << gu.TILE_BIT)) == 5   # a table shorter than a tile: every row
    assert len(set(gu.QUERY_WORDS)) == 15 and np.unique(gu.query_words(300)).size == 15
    Tl, Ql = tu.lane_map_tags(1037, 70)
    assert np.unique(Ql).size == 32 and all(np.count_nonzero(Tl & w) in (32, 33) for w in np.unique(Ql))
    base, q, Tt, Qt, group = tu.tie_case()
    assert (Qt == 1).all() and np.count_nonzero(Tt & 1) == 680   # one list of 680 rows: two of every triple of equal rows


from test_isa_contract import FUSED, kernels  # noqa: E402,F401  (the disassembly fixture of the arithmetic-contract test)


def test_gather_kernels_are_under_the_arithmetic_contract(kernels):  # noqa: F811
    """tests/test_isa_contract.py's check for the new unit, whose name its list does not match: every knn_gather_kernel instance (two metrics x
    three row lengths x float / byte rows) is in the library, computes with separately rounded packed multiplies and adds, and holds no
    fused multiply-add."""
    mine = {name: insts for name, insts in kernels.items() if "knn_gather_kernel" in name}
    assert len(mine) == 12, sorted(mine)
    for name, insts in mine.items():
        text = "\n".join(insts)
        assert "v_pk_mul_f32" in text and "v_pk_add_f32" in text, name
        assert not [i for i in insts if FUSED.match(i)], name
