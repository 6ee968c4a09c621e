"""gbnns_exact_knn_tagged / gbnns_exact_knn_bytes_tagged / gbnns_index_exact_knn without a device: the exports and declarations, the
refusals that come before any HIP call, the binding's TypeErrors, and the yardstick of tests/test_gpu_knn_tagged.py itself -- the helper's
oracle-derived expected values against a plain numpy lexsort over the masked integer distances, and the preconditions its fixtures rest
on (a fixture that does not do what its test says it does would let a wrong kernel pass)."""
import os

import numpy as np
import pytest

import knn_bytes_util as ku
import knn_tagged_util as tu

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5
NEW = ("gbnns_exact_knn_tagged", "gbnns_exact_knn_bytes_tagged", "gbnns_index_exact_knn")


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports_and_declarations(g):
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gbnns.h")).read()
    for name in NEW:
        assert name in binding.SYMBOLS and hasattr(lib, name), name
        assert ("int %s(" % name) in header, name
    assert callable(g.Index.exact_knn)
    assert g.version() == 100


def _free(g, name, base, q, k, row_tags, query_tags, **kw):
    lib = g.load_library()
    out = np.zeros((max(1, q.shape[0]), max(1, min(k, 8))), np.uint32)
    a = dict(n=base.shape[0], n_q=q.shape[0], d=base.shape[1], metric=ku.L2, self_offset=-1, mem_kind=0)
    a.update(kw)
    rc = getattr(lib, name)(0, base.ctypes.data, a["n"], q.ctypes.data, a["n_q"], a["d"], k, a["metric"], a["self_offset"],
                            None if row_tags is None else row_tags.ctypes.data, None if query_tags is None else query_tags.ctypes.data,
                            out.ctypes.data, None, a["mem_kind"], None)
    return rc, lib.gbnns_last_error().decode()


@pytest.mark.parametrize("name,dtype", [("gbnns_exact_knn_tagged", np.float32), ("gbnns_exact_knn_bytes_tagged", np.uint8)])
def test_free_function_refusals(g, name, dtype):
    """Null tag pointers are GBNNS_ERR_INVALID; everything else is refused as the untagged twin refuses it, before the first HIP call."""
    b, q = np.zeros((8, 16), dtype), np.zeros((2, 16), dtype)
    T, Q = np.ones(8, np.uint32), np.ones(2, np.uint32)
    assert _free(g, name, b, q, 1, None, Q) == (INVALID, "null argument")
    assert _free(g, name, b, q, 1, T, None) == (INVALID, "null argument")
    assert _free(g, name, b, q, 1, None, None) == (INVALID, "null argument")
    for kw, word in ((dict(n=0), "n must be in"), (dict(n_q=1 << 31), "n_q too large"), (dict(d=0), "d must be"), (dict(metric=2), "unknown metric"),
                     (dict(mem_kind=7), "unknown mem_kind"), (dict(self_offset=-2), "self_offset")):
        rc, msg = _free(g, name, b, q, 1, T, Q, **kw)
        assert rc == INVALID and word in msg, kw
    for k in (0, (1 << 20) + 1):
        assert _free(g, name, b, q, k, T, Q)[0] == INVALID
    rc, msg = _free(g, name, np.zeros((8, 12), dtype), np.zeros((2, 12), dtype), 1, T, Q, metric=ku.NEG_DOT)
    assert rc == UNSUPPORTED and "d % 8 == 0" in msg
    if dtype == np.uint8:
        rc, msg = _free(g, name, b, q, 1, T, Q, d=257)
        assert rc == UNSUPPORTED and "d <= 256" in msg
        assert _free(g, name, b, q, 4097, T, Q)[0] == UNSUPPORTED
    else:
        assert _free(g, name, b, q, 1, T, Q, d=8200)[0] == UNSUPPORTED
    if g.device_count() == 0:
        rc, msg = _free(g, name, b, q, 1, T, Q)
        assert rc == NO_DEVICE and "no CPU path" in msg


def test_index_call_wants_exactly_one_query_pointer(g):
    """Both or neither of queries / queries_u8: GBNNS_ERR_INVALID, before the handle is looked at."""
    lib = g.load_library()
    qf, qb, ids = np.zeros((2, 16), np.float32), np.zeros((2, 16), np.uint8), np.zeros((2, 1), np.uint32)
    for a, b in ((None, None), (qf.ctypes.data, qb.ctypes.data)):
        assert lib.gbnns_index_exact_knn(None, a, b, 2, None, 1, -1, ids.ctypes.data, None, 0, None) == INVALID
        assert "exactly one of queries / queries_u8" in lib.gbnns_last_error().decode()
    assert lib.gbnns_index_exact_knn(None, qf.ctypes.data, None, 2, None, 1, -1, ids.ctypes.data, None, 0, None) == INVALID   # (no handle)


class _Spy:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, len(a)))
            return 0
        return f


def test_binding_type_errors_and_dispatch(g, monkeypatch):
    from gbnns_dim_red_amd import binding
    spy = _Spy()
    monkeypatch.setattr(binding, "load_library", lambda: spy)
    bu, qu = np.zeros((8, 16), np.uint8), np.zeros((2, 16), np.uint8)
    bf, qf = bu.astype(np.float32), qu.astype(np.float32)
    T, Q = np.ones(8, np.uint32), np.ones(2, np.uint32)
    for kw in (dict(row_tags=T), dict(query_tags=Q)):   # both or neither
        with pytest.raises(TypeError) as e:
            binding.exact_knn(bf, qf, 3, **kw)
        assert "both or neither" in str(e.value)
    assert spy.calls == []
    binding.exact_knn(bf, qf, 3, row_tags=T, query_tags=Q)
    binding.exact_knn(bu, qu, 3, row_tags=T.astype(np.int64), query_tags=list(Q))   # (host tag arrays of another type are converted)
    binding.exact_knn(bf, qf, 3)
    assert spy.calls == [("gbnns_exact_knn_tagged", 15), ("gbnns_exact_knn_bytes_tagged", 15), ("gbnns_exact_knn", 13)]
    with pytest.raises(TypeError):   # the mixed-pair rule holds with tags too
        binding.exact_knn(bu, qf, 3, row_tags=T, query_tags=Q)
    for bad in (dict(row_tags=T[:7], query_tags=Q), dict(row_tags=T, query_tags=np.ones(3, np.uint32))):   # one word per row / query
        with pytest.raises(ValueError):
            binding.exact_knn(bf, qf, 3, **bad)
    import torch
    with pytest.raises(TypeError):   # a tensor beside host inputs
        binding.exact_knn(bf, qf, 3, row_tags=torch.ones(8, dtype=torch.int32), query_tags=Q)


def test_tag_table_preconditions():
    """Every fraction bit allows at least one and not all rows at n = 1 037 (bit 0: all, by its definition); bit 8 the last 40 rows only;
    bit 9 fewer than 10 rows; the query words reach every one of them, 0 and all ones."""
    for n in tu.NS:
        T = tu.tag_table(n, n)
        assert T.dtype == np.uint32 and T.shape == (n,)
        assert ((T >> 0) & 1).all()
        assert np.array_equal(np.nonzero((T >> tu.LATE_BIT) & 1)[0], np.arange(max(0, n - 40), n))
        assert np.array_equal(np.nonzero((T >> tu.FEW_BIT) & 1)[0], np.arange(min(n, 7)))
    T = tu.tag_table(1037, 1037)
    for b in range(1, 8):
        cnt = int(((T >> b) & 1).sum())
        assert 1 <= cnt < 1037, (b, cnt)
    assert int(((T >> tu.FEW_BIT) & 1).sum()) < 10
    Q = tu.query_words(300)
    assert set(Q.tolist()) == set(tu.QUERY_WORDS) and (Q[:13] == np.array(tu.QUERY_WORDS, np.uint32)).all()
    assert tu.query_words(1).tolist() == [1]
    T, Q = tu.lane_map_tags(1037, 70)
    allowed = (T[None, :] & Q[:, None]) != 0
    for blk in range(0, 1024, 32):   # exactly one row of every whole block of 32, at position i % 32
        assert (allowed[:, blk:blk + 32].sum(1) == 1).all()
    assert np.array_equal(np.argmax(allowed[:, :32], axis=1), np.arange(70) % 32)


@pytest.mark.parametrize("metric,d", [(ku.L2, 30), (ku.L2, 128), (ku.NEG_DOT, 8)])
def test_expected_values_equal_a_masked_integer_lexsort(orc, metric, d):
    """The helper's oracle-derived expected values against plain int64 numpy over the allowed rows: ids, distance bits, padding, the self
    row dropped whether allowed or not."""
    base, q = tu.byte_case(metric, d)
    base[5:20] //= 128   # a mass of ties among the near rows
    for n, nq, k, so in ((1037, 70, 10, -1), (1037, 70, 40, 3), (5, 26, 12, -1), (300, 26, 200, 0)):
        T, Q = tu.tag_table(n, n), tu.query_words(nq)
        ei, ed = tu.expected(orc, base[:n], q[:nq], T, Q, k, metric, self_offset=so)
        wi, wd = tu.expected_int(base[:n], q[:nq], T, Q, k, metric, self_offset=so)
        assert np.array_equal(ei, wi) and np.array_equal(ku.bits(ed), ku.bits(wd)), (n, nq, k, so)
        zero = np.nonzero(Q == 0)[0]
        assert zero.size and (ei[zero] == tu.NONE_ID).all() and np.isposinf(ed[zero]).all()   # Q[i] == 0: a row of padding
        few = np.nonzero(Q == 1 << tu.FEW_BIT)[0]
        assert few.size and (ei[few][:, 7:] == tu.NONE_ID).all()
        if so >= 0:
            assert not (ei == (np.arange(nq) + so)[:, None]).any()
    # with every word all ones the expected value is the oracle's untagged answer
    T, Q = np.full(1037, tu.ALL, np.uint32), np.full(70, tu.ALL, np.uint32)
    ei, ed = tu.expected(orc, base[:1037], q[:70], T, Q, 10, metric)
    oi, od = orc.exact_knn(ku.widen(base[:1037]), ku.widen(q[:70]), 10, metric, threads=2)
    assert np.array_equal(ei, oi) and np.array_equal(ku.bits(ed), ku.bits(od))


@pytest.mark.parametrize("metric", (ku.L2, ku.NEG_DOT))
def test_tie_fixture_ties_across_an_allowed_and_a_disallowed_row_at_rank_k(orc, metric):
    """At rank k (and every other) the reported row has a disallowed twin of the same distance and a lower id: the untagged answer would
    hold the twin instead, so a tag test that lets a disallowed row in -- or a threshold `<` that drops the allowed one -- shows."""
    k = 40
    base, q, T, Q, group = tu.tie_case()
    assert int((T == 2).sum()) == 340 and int((T == 1).sum()) == 680
    for so in (-1, 0):
        ei, ed = tu.expected(orc, base, q, T, Q, k, metric, self_offset=so)
        wi, wd = tu.expected_int(base, q, T, Q, k, metric, self_offset=so)
        assert np.array_equal(ei, wi) and np.array_equal(ku.bits(ed), ku.bits(wd))
        assert (np.diff(ed, axis=1) == 0).mean() > 0.5 and (ei != tu.NONE_ID).all()
        dist = ku.int_dist(base, q, metric)
        last = ei[:, k - 1].astype(np.int64)
        twin = np.array([np.nonzero((group == group[j]) & (T == 2))[0][0] for j in last])
        assert (twin < last).all() and ((T[twin] & Q[0]) == 0).all() and (T[last] & Q[0]).all()
        assert (dist[np.arange(200), twin] == dist[np.arange(200), last]).all()
        ui, _ = orc.exact_knn(ku.widen(base), ku.widen(q), k, metric, self_offset=so, threads=2)
        assert (T[ui] == 2).any(1).all()   # ... and the untagged lists do hold disallowed rows, for every query


@pytest.mark.parametrize("k", (30, 100))
def test_overflow_fixture_still_overflows_under_the_filter(g, k):
    """From the plan at knn_chunk = 512: at least two chunks hold more ALLOWED rows than a key list has slots, and every row of every chunk
    is a hit for query 0 (the rows come farthest first) -- so those chunks overflow its list and are swept again in pieces."""
    base, q, T, Q = tu.overflow_case(k)
    with ku.knobs(g, knn_chunk=512):
        plan = g.knn_bytes_plan(base.shape[0], q.shape[0], base.shape[1], k)
    allowed = (T & Q[0]) != 0
    assert 0.4 < allowed.mean() < 0.6
    d0 = ((base.astype(np.int64) - 128) ** 2).sum(1)
    assert (np.diff(d0) <= 0).all() and (q[0] == 128).all()
    over = [int(allowed[r0:r0 + rows].sum()) > plan["cap"] for r0, rows in ku.chunk_plan(plan, base.shape[0])]
    assert sum(over) >= 2 and not over[0]
