"""The k-answer re-rank (gbnns_rerank_topk / gbnns_search_topk), what can be checked without a device: the binding's surface, the
argument checks that fire before any HIP call, and the precondition of tests/test_gpu_topk.py -- on its contest lists the top-k
order is decided by the order of the float32 roundings and by the pop-index tie rule, so a kernel that restated the distances in
another order, or broke ties another way, cannot pass it."""
import ctypes

import numpy as np
import pytest

import gbnns_dim_red_amd as g
from gbnns_dim_red_amd import binding

import topk_util as tu

GBNNS_ERR_INVALID = 1   # include/gbnns.h


@pytest.fixture(scope="module")
def lib():
    g.build_library()
    return g.load_library()


def test_binding_surface(lib):
    assert callable(getattr(binding.Index, "rerank_topk", None))
    assert "top_k" in binding.Index.search.__code__.co_varnames
    for name in ("gbnns_rerank_topk", "gbnns_search_topk"):
        assert name in binding.SYMBOLS and hasattr(lib, name), name


def test_rerank_topk_argument_checks_need_no_device(lib):
    """A null index, a null candidate array, k = 0 and k > cand_stride: GBNNS_ERR_INVALID with a message, before any HIP call (this
    machine has no device: a HIP call would answer with GBNNS_ERR_HIP, or not at all)."""
    q = np.zeros((2, 8), np.float32)
    cand = np.zeros((2, 4), np.uint32)
    ids = np.zeros((2, 4), np.uint32)
    fake = ctypes.c_void_p(0)
    P = lambda a: a.ctypes.data

    def call(index, cand_ptr, k, stride=4):
        rc = lib.gbnns_rerank_topk(index, P(q), 2, cand_ptr, stride, None, k, P(ids), None, binding.MEM_HOST, None)
        return rc, lib.gbnns_last_error().decode()

    for what, args in (("null index", (fake, P(cand), 2)), ("null cand", (fake, None, 2)), ("k = 0", (fake, P(cand), 0)),
                       ("k > stride", (fake, P(cand), 5)), ("k < 0", (fake, P(cand), -1))):
        rc, msg = call(*args)
        assert rc == GBNNS_ERR_INVALID and msg, (what, rc, msg)
    rc = lib.gbnns_search_topk(None, None, 1, P(ids), None)
    assert rc == GBNNS_ERR_INVALID and lib.gbnns_last_error()


@pytest.mark.parametrize("d,metric", tu.RERANK_SHAPES, ids=["d%d_m%d" % s for s in tu.RERANK_SHAPES])
def test_contest_lists_are_decided_by_rounding_order_and_pop_index(orc, d, metric):
    """The lists of test_gpu_topk.py's contest test with 33 candidates and more (60 per shape): among the first min(k, count) + 1
    entries of the expected order two float32 distances are equal -- the pop index decides a column or the cut -- and the top-k
    order differs from the one float64-accumulated distances give -- the order of the roundings decides.  At least 50 of 60, at
    k = 10 and k = 64."""
    base, q, cand, count = tu.rerank_contest(d, metric)
    dist = tu.list_distances(orc, base, q, cand, count, metric)
    alt = tu.float64_distances(base, q, cand, count, metric)
    long_lists = np.flatnonzero(count >= 33)
    assert len(long_lists) == 60
    for k in (10, 64):
        ties = moved = 0
        for i in long_lists:
            c = int(count[i])
            order = np.lexsort((np.arange(c), dist[i, :c]))
            order2 = np.lexsort((np.arange(c), alt[i, :c]))
            kk = min(k, c)
            head = dist[i, order[:kk + 1]]
            ties += bool((head[1:] == head[:-1]).any())
            moved += not np.array_equal(order[:kk], order2[:kk])
        distinct = int(np.median([len(np.unique(dist[i, :count[i]])) for i in long_lists]))
        print("contest lists", (d, metric, k), "ties", ties, "order differs from float64 sums", moved, "median distinct distances", distinct)
        assert ties >= 50 and moved >= 50, (d, metric, k, ties, moved)
