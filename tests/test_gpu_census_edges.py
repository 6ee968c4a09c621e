"""gbnns_index_tag_census at the edges of its kernels, and gbnns_search_tagged_auto with a scan leg of several query slabs, on an MI355X
(run with -m gpu).  The fixtures and what each of them rests on: tests/census_edges_util.py (asserted on the CPU by
tests/test_knn_instances_cpu.py); the census must equal NumPy's (gbnns_dim_red_amd.tag_census), once also the double loop of
tag_auto_util.census_loops; the routed search's expectation is composed by tag_auto_util.expected.  Nothing takes a tolerance."""
import numpy as np
import pytest

import census_edges_util as ce
import knn_bytes_util as ku
import knn_tagged_util as kt
import tag_auto_util as au

pytestmark = pytest.mark.gpu

WANT = ("hops", "dist_calc", "cand", "cand_dist", "edges")


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _tiny_index(g, n, T):
    """n rows on a ring: the census needs a handle and a tag table, nothing of the search."""
    rng = np.random.default_rng(n)
    off = np.arange(n + 1, dtype=np.uint64)
    nbr = ((np.arange(n) + 1) % n).astype(np.uint32)
    ix = g.Index(rng.standard_normal((n, 8)).astype(np.float32), off, nbr)
    ix.set_tags(T)
    return ix


def _same(g, ix, T, Q, what):
    """The HOST call and the DEVICE call against NumPy."""
    import torch
    want = g.tag_census(T, Q)
    got = ix.tag_census(Q)
    assert np.array_equal(np.asarray(got[0]).view(np.uint32), want[0]), (what, "allowed")
    assert np.array_equal(np.asarray(got[1]).view(np.uint32), want[1]), (what, "first")
    a, f = ix.tag_census(torch.from_numpy(Q.view(np.int32)).to("cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want[0]), (what, "allowed, device buffers")
    assert np.array_equal(f.cpu().numpy().view(np.uint32), want[1]), (what, "first, device buffers")
    return want


@pytest.fixture(scope="module")
def ix1037(g):
    ix = _tiny_index(g, ce.N, ce.table())
    yield ix
    ix.close()


@pytest.mark.parametrize("u", ce.DISTINCT)
def test_distinct_words_at_the_lane_and_chunk_edges(g, ix1037, u):
    """U = 63 / 64 / 65 (a register of the word loop), 255 / 256 / 257 and 512 / 513 (its chunks of 256): once as a batch of U queries, once
    repeated to 2 U + 5 queries in a shuffled order."""
    T, words = ce.table(), ce.distinct_words(u)
    _same(g, ix1037, T, words, (u, "once"))
    _same(g, ix1037, T, ce.repeated(words), (u, "repeated"))


def test_one_word_and_half_shared_wavefronts(g, ix1037):
    T, Q = ce.one_word_batch()
    ix = _tiny_index(g, ce.N, T)
    allowed, first = _same(g, ix, T, Q, "one word")
    assert (allowed == 35).all() and (first == 517).all()
    ix.close()
    _same(g, ix1037, ce.table(), ce.half_shared_batch(), "half of every wavefront shares its first word")


@pytest.mark.parametrize("n", ce.TILE_NS)
def test_rows_at_the_tile_edges(g, n):
    T = ce.table(n)
    ix = _tiny_index(g, n, T)
    Q = kt.query_words(300)
    assert len(np.unique(Q)) == 13
    _same(g, ix, T, Q, n)
    ix.close()


def test_placement_of_single_rows(g):
    """Bit b on exactly one row: allowed 1 and first = that row for 1 << b -- the ends of the table, of a tile, of a wavefront's share (lane 63,
    element 3) --, pairs of bits: allowed 2, first the lower row."""
    T, rows, Q = ce.placement()
    ix = _tiny_index(g, ce.PLACE_N, T)
    allowed, first = _same(g, ix, T, Q, "placement")
    assert (allowed[:32] == 1).all() and np.array_equal(first[:32], rows) and (allowed[32:] == 2).all()
    ix.close()


def test_probe_sequences_wrap(g, ix1037):
    """40 queries, a table of 128 slots, every word at home in the last three: all but three claim a slot behind the wrap."""
    words = ce.wrap_words()
    slots = [g.census_slot(int(w), len(words)) for w in words]
    assert len(words) == 40 and len(np.unique(words)) == 40 and all(cap == 128 and slot in (125, 126, 127) for slot, cap in slots)
    allowed, first = _same(g, ix1037, ce.table(), words, "wrap")
    la, lf = au.census_loops(ce.table(), words)   # the definition, once
    assert np.array_equal(la, allowed) and np.array_equal(lf, first)
    rng = np.random.default_rng(5)
    _same(g, ix1037, ce.table(), np.ascontiguousarray(words[rng.permutation(40)]), "wrap, shuffled")


# ---- the routed search with a scan leg of several slabs ------------------------------------------------------------------------------
def _four_times(c):
    """The tag_auto_util fixture's 96 queries four times; the word sequence rolled by one per copy, so that a query meets four words."""
    c4 = dict(c)
    c4["queries"] = np.ascontiguousarray(np.tile(c["queries"], (4, 1)))
    c4["q_low"] = np.ascontiguousarray(np.tile(c["q_low"], (4, 1)))
    c4["ent"] = np.ascontiguousarray(np.tile(c["ent"], 4))
    c4["Q"] = np.concatenate([np.roll(c["Q"], j) for j in range(4)]).astype(np.uint32)
    nq = len(c["Q"])
    assert all((c4["Q"][j * nq:(j + 1) * nq] != c["Q"]).mean() > 0.8 for j in range(1, 4))
    return c4


@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_routed_search_scans_in_several_slabs(g, orc, kind):
    """384 queries, "knn_slab" = 128: scan_below = 2^64 - 1 gathers all of them (three slabs), 300 a sparse list of the four small words' queries
    (two slabs).  The float handle's scan runs in slabs on its pool path ("knn_filter" = 2, "knn_pool_min_k" = 1); the byte handle's always."""
    metric, ef, k = 0, 64, 10
    c = _four_times(au.fixture(metric))
    nq = len(c["Q"])
    assert nq == 384
    knobs = dict(knn_slab=128)
    if kind == "bytes":
        base8, q8 = au.quantised(c)
        c["base"], c["queries"] = ku.widen(base8), ku.widen(q8)   # the byte handle's promise: the float handle's rows over the widened table
        db, queries = base8, q8
    else:
        db, queries = c["base"], c["queries"]
        knobs.update(knn_filter=2, knn_pool_min_k=1)
    ix = g.Index(db, c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    ix.set_tags(c["T"])
    for sb, min_slabs in ((2 ** 64 - 1, 3), (300, 2)):
        e = au.expected(orc, ("four times", kind, metric), c, ef, k, metric, sb)
        m = int((e["route"] == 1).sum())
        with ku.knobs(g, **knobs):
            slab = g.knn_slab(m, k, bytes=kind == "bytes")
            assert slab == 128 and -(-m // slab) >= min_slabs, (m, slab)
            if kind == "float":
                assert g.knn_plan(False, metric, len(c["T"]), m, c["base"].shape[1], k, True) == ("knn_filter_kernel<3, 2, true>", True)
            r = ix.search_auto(queries, ef, k, c["Q"], scan_below=sb, mode=g.MODE_LOWQ, queries_low=c["q_low"], want=WANT)
        if sb == 300:   # a sparse list: scan-routed and walk-routed queries alternate
            assert 0 < m < nq and np.count_nonzero(np.diff(e["route"].astype(np.int8))) > 100
        bad = au.differences(r, e)
        assert not bad, (kind, sb, bad)
    ix.close()
