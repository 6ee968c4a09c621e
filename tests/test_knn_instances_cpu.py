"""The census of the exact-scan kernel instances without a device: gbnns_debug_knn_plan names what every case of tests/knn_instances.py
launches, the names cover the 16 + 16 + 12 + 10 instances exactly, the shapes are the ones the table promises and no tagged case is vacuous;
gbnns_debug_census_slot and the preconditions of the census fixtures of tests/census_edges_util.py.  tests/test_gpu_knn_instances.py and
tests/test_gpu_census_edges.py run what is proven here."""
import ctypes as C

import numpy as np
import pytest

import census_edges_util as ce
import knn_bytes_util as ku
import knn_instances as ki

INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _plan(g, c):
    with ku.knobs(g, **c.knob_dict):
        return g.knn_plan(c.bytes, c.metric, c.n, c.nq, c.d, c.k, c.tagged)


def test_exports(g):
    from gbnns_dim_red_amd import binding
    for name in ("gbnns_debug_knn_plan", "gbnns_debug_census_slot"):
        assert name in binding.SYMBOLS and hasattr(g.load_library(), name), name
    assert callable(g.knn_plan) and callable(g.census_slot)


def test_every_case_takes_the_instance_it_names(g):
    for c in ki.CASES:
        assert _plan(g, c) == (c.name, c.pool), c
    # the knobs came back: the same float shapes are scans by default
    for c in ki.CASES:
        if not c.bytes and "knn_filter" in c.knob_dict:
            name, pool = g.knn_plan(False, c.metric, c.n, c.nq, c.d, c.k, c.tagged)
            assert name.startswith("knn_scan_kernel<") and not pool, c


def test_the_names_cover_every_instance_exactly(g):
    want = ki.instance_names()
    assert [len(want[f]) for f in ("bytes", "filter", "scan", "wide")] == [16, 16, 12, 10]
    got = {}
    for c in ki.CASES:
        got.setdefault(c.name, []).append(c)
    assert set(got) == set().union(*want.values())
    # every filter instance on heaps; on pools at least one KSTEPS per QB class, plain and tagged; every byte instance on both
    for name in want["filter"] | want["bytes"]:
        assert any(not c.pool for c in got[name]), name
    for name in want["bytes"]:
        assert any(c.pool for c in got[name]), name
    for qb in set(ki.FILTER_QB.values()):
        for tagged in ("true", "false"):
            assert any(c.pool for name in want["filter"] if name.endswith(", %d, %s>" % (qb, tagged)) for c in got[name]), (qb, tagged)
    # heaps see k = 1 and k = 10, pools k = 64 and a short list under "knn_pool_min_k" = 1
    for family in ("bytes", "filter"):
        cases = [c for name in want[family] for c in got[name]]
        assert {c.k for c in cases if not c.pool} == {1, 10}
        assert {c.k for c in cases if c.pool} == {10, 64}
        assert all(c.knob_dict.get("knn_pool_min_k") == 1 for c in cases if c.pool and c.k < 64)
    # the float filter cases are forced ("knn_filter" = 2), nothing else is
    for c in ki.CASES:
        assert (c.knob_dict.get("knn_filter") == 2) == c.name.startswith("knn_filter_kernel"), c


def test_shapes(g):
    """n = 1 037 with chunks of 64 rows: five chunks and more; n_q = 128 QB + 37; per K step count the narrowest and the full width, byte L2
    also a width with d % 4 != 0."""
    for c in ki.CASES:
        assert c.n == 1037 and c.nq == ki.queries_per_workgroup(c.name) + 37, c
        if c.bytes:
            with ku.knobs(g, **c.knob_dict):
                plan = g.knn_bytes_plan(c.n, c.nq, c.d, c.k)
            # (a list of 64 has a first chunk of 4 k + 64 = 320 rows: four chunks)
            assert len(ku.chunk_plan(plan, c.n)) >= (5 if c.k <= 10 else 4) and plan["pool"] == c.pool, c
    for ks in range(1, 9):
        b = {(c.metric, c.d) for c in ki.CASES if c.bytes and c.name.startswith("knn_bytes_sweep_kernel<%d," % ks)}
        assert {(0, 32 * (ks - 1) + 8), (0, 32 * ks), (0, 32 * ks - 1), (1, 32 * ks), (1, 32 * (ks - 1) + 8)} <= b, (ks, b)
        f = {c.d for c in ki.CASES if c.name.startswith("knn_filter_kernel<%d," % ks)}
        assert f == {16 * (ks - 1) + 4, 16 * ks}, (ks, f)
        for tagged in (False, True):
            for d in (32 * (ks - 1) + 8, 32 * ks):
                assert any(c.bytes and c.d == d and c.tagged == tagged for c in ki.CASES), (ks, d, tagged)
            for d in (16 * (ks - 1) + 4, 16 * ks):
                assert any(not c.bytes and c.d == d and c.tagged == tagged and c.name.startswith("knn_filter") for c in ki.CASES), (ks, d, tagged)


def test_no_tagged_case_is_vacuous():
    """Every query word of a tagged case allows some rows but not all, and at least one word allows fewer than k rows."""
    seen = 0
    for c in ki.CASES:
        if not c.tagged:
            continue
        T, Q = ki.tags(c)
        assert len(T) == c.n and len(Q) == c.nq and len(np.unique(Q)) == len(ki.TAG_WORDS) == 9
        counts = np.array([np.count_nonzero(T & w) for w in np.unique(Q)])
        assert (counts > 0).all() and (counts < c.n).all(), (c, counts)
        assert (counts < c.k).any() and (counts >= c.k).any(), (c, counts)
        seen += 1
    assert seen >= 54 // 2


def test_knn_plan_refusals(g):
    lib = g.load_library()
    name, pool = C.create_string_buffer(128), C.c_int(0)
    ok = (0, 0, 1037, 165, 32, 10, 0)
    assert lib.gbnns_debug_knn_plan(*ok, name, 128, C.byref(pool)) == 0 and name.value == b"knn_scan_kernel<0, 8, 2, false>"
    assert lib.gbnns_debug_knn_plan(*ok, None, 128, C.byref(pool)) == INVALID
    assert lib.gbnns_debug_knn_plan(*ok, name, 0, C.byref(pool)) == INVALID
    assert lib.gbnns_debug_knn_plan(*ok, name, 128, None) == INVALID
    for bad in ((2, 0, 1037, 165, 32, 10, 0), (0, 2, 1037, 165, 32, 10, 0), (0, 0, 0, 165, 32, 10, 0), (0, 0, 1037, 1 << 31, 32, 10, 0),
                (0, 0, 1037, 165, 0, 10, 0), (0, 0, 1037, 165, 32, 0, 0), (1, 0, (1 << 32) - 1, 165, 32, 10, 0)):
        assert lib.gbnns_debug_knn_plan(*bad, name, 128, C.byref(pool)) == INVALID, bad
    # what the calls themselves refuse as unsupported
    for bad in ((0, 0, 1037, 165, 8196, 10, 0), (0, 1, 1037, 165, 36, 10, 0), (1, 0, 1037, 165, 257, 10, 0), (1, 0, 1037, 165, 32, 4097, 0),
                (1, 1, 1037, 165, 36, 10, 0)):
        assert lib.gbnns_debug_knn_plan(*bad, name, 128, C.byref(pool)) == UNSUPPORTED, bad
    # a short buffer gets a terminated prefix
    short = C.create_string_buffer(b"x" * 8, 8)
    assert lib.gbnns_debug_knn_plan(*ok, short, 8, C.byref(pool)) == 0 and short.value == b"knn_sca"


def test_knn_plan_follows_the_knobs_and_the_size_rule(g):
    big = (False, 0, 1 << 17, 2048, 32)
    assert g.knn_plan(*big, 10) == ("knn_filter_kernel<2, 4, false>", False)       # the default: by size
    assert g.knn_plan(*big, 64) == ("knn_filter_kernel<2, 4, false>", True)
    assert g.knn_plan(*big, 513)[0] == "knn_filter_kernel<2, 4, false>" and g.knn_plan(*big, 4097) == ("knn_scan_kernel<0, 8, 2, false>", False)
    assert g.knn_plan(False, 0, (1 << 17) - 1, 2048, 32, 10)[0] == "knn_scan_kernel<0, 8, 2, false>"
    assert g.knn_plan(False, 0, 1 << 17, 2047, 32, 10)[0] == "knn_scan_kernel<0, 8, 2, false>"
    assert g.knn_plan(False, 1, 1 << 17, 2048, 32, 10)[0] == "knn_scan_kernel<1, 8, 2, false>"
    assert g.knn_plan(False, 0, 1 << 17, 2048, 30, 10)[0] == "knn_scan_kernel<0, 8, 2, false>"   # d % 4 != 0
    assert g.knn_plan(False, 0, 1 << 17, 2048, 132, 10)[0] == "knn_scan_wide_kernel<0, 16, false>"
    with ku.knobs(g, knn_filter=0):
        assert g.knn_plan(*big, 10)[0] == "knn_scan_kernel<0, 8, 2, false>"
    with ku.knobs(g, knn_filter=2, knn_pool_min_k=1):
        assert g.knn_plan(False, 0, 41, 1, 32, 10, True) == ("knn_filter_kernel<2, 4, true>", True)
        assert g.knn_plan(False, 0, 40, 1, 32, 10, True) == ("knn_scan_kernel<0, 8, 2, true>", False)   # n > 4 k
    assert g.knn_plan(*big, 10) == ("knn_filter_kernel<2, 4, false>", False)
    assert g.knn_plan(True, 0, 10, 1, 1, 63) == ("knn_bytes_sweep_kernel<1, 4, false>", False)
    assert g.knn_plan(True, 1, 10, 1, 256, 64, True) == ("knn_bytes_sweep_kernel<8, 2, true>", True)


def _hash(w):
    """tag_census.hip's census_hash, restated."""
    m = 0xFFFFFFFF
    w ^= w >> 16
    w = w * 0x7FEB352D & m
    w ^= w >> 15
    w = w * 0x846CA68B & m
    return w ^ w >> 16


def test_census_slot(g):
    for nq, cap in ((1, 64), (32, 64), (33, 128), (40, 128), (64, 128), (65, 256), (1000, 2048), (1 << 30, 1 << 31)):
        for w in (0, 1, 0x4000, 0xDEADBEEF, 0xFFFFFFFF):
            assert g.census_slot(w, nq) == (_hash(w) & (cap - 1), cap), (nq, w)
    lib = g.load_library()
    slot, cap = C.c_uint32(0), C.c_uint32(0)
    assert lib.gbnns_debug_census_slot(5, 40, None, C.byref(cap)) == INVALID
    assert lib.gbnns_debug_census_slot(5, 40, C.byref(slot), None) == INVALID
    assert lib.gbnns_debug_census_slot(5, 0, C.byref(slot), C.byref(cap)) == INVALID
    assert lib.gbnns_debug_census_slot(5, (1 << 30) + 1, C.byref(slot), C.byref(cap)) == INVALID


def test_census_fixtures_hold_their_preconditions(g):
    for u in ce.DISTINCT:
        w = ce.distinct_words(u)
        assert len(np.unique(w)) == u and (w != 0).all()
        r = ce.repeated(w)
        assert len(r) == 2 * u + 5 and len(np.unique(r)) == u and not np.array_equal(r[:u], w)
    T, Q = ce.one_word_batch()
    allowed, first = g.tag_census(T, Q)
    assert len(Q) == 1000 and len(np.unique(Q)) == 1 and (allowed == 35).all() and (first == 517).all()
    Q = ce.half_shared_batch()
    assert len(Q) == 645 and len(np.unique(Q)) > 300
    T, rows, Q = ce.placement()
    allowed, first = g.tag_census(T, Q)
    assert (allowed[:32] == 1).all() and np.array_equal(first[:32], rows) and (allowed[32:] == 2).all()
    assert np.count_nonzero(T) == 32 and sorted(T[T != 0].tolist()) == [1 << b for b in range(32)]
    words = ce.wrap_words()
    slots = [g.census_slot(int(w), ce.WRAP_NQ) for w in words]
    assert all(cap == 128 and slot >= 125 for slot, cap in slots) and len(set(words.tolist())) == 40
