"""The query slabs of gbnns_exact_knn_bytes and of gbnns_exact_knn's pool path without a device: gbnns_debug_knn_slab against the
header's formula, the rounding and the cap of the "knn_slab" knob, that the test helper puts the knob back, and that the knob changes
nothing else of gbnns_debug_knn_bytes_plan.  tests/test_gpu_knn_slabs.py runs the slabs these functions report."""
import ctypes as C

import numpy as np
import pytest

import knn_bytes_util as ku

INVALID = 1
KS = (1, 7, 10, 63, 64, 200, 1000, 2500, 4095, 4096)
NQS = (0, 1, 44, 127, 128, 129, 300, 500, 1023, 1024, 1025, 4096, 32640, 32641, 65280, 65281, 10**6, (1 << 31) - 1)


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def formula(nq, k, key_bytes):
    """include/gbnns.h at gbnns_exact_knn_bytes: min(n_q, max(1024, floor(2^32 / (key_bytes cap)) & ~127)), cap = 4 k + 64."""
    cap = 4 * k + 64
    return min(nq, max(1024, (2 ** 32 // (key_bytes * cap)) & ~127))


def test_exports(g):
    from gbnns_dim_red_amd import binding
    assert "gbnns_debug_knn_slab" in binding.SYMBOLS and hasattr(g.load_library(), "gbnns_debug_knn_slab") and callable(g.knn_slab)


def test_default_slabs_are_the_headers_formula(g):
    for k in KS:
        for nq in NQS:
            assert g.knn_slab(nq, k, bytes=True) == formula(nq, k, 8), (k, nq)
            assert g.knn_slab(nq, k, bytes=False) == formula(nq, k, 4), (k, nq)
            if nq:
                assert g.knn_bytes_plan(5000, nq, 32, k)["slab"] == formula(nq, k, 8), (k, nq)
    assert g.knn_slab(10**6, 4096, bytes=True) == 32640
    assert g.knn_slab(10**6, 4096, bytes=False) == 65280
    assert g.knn_slab(500, 4096, bytes=True) == 500 and g.knn_slab(500, 4096, bytes=False) == 500
    assert g.knn_slab(500, 10, bytes=True) == 500 and g.knn_slab(500, 10, bytes=False) == 500
    for k in KS:   # a slab of fewer queries than there are is a multiple of 128, at least 1 024, and its key lists fit 4 GiB or it is 1 024
        for kb, by in ((8, True), (4, False)):
            s = g.knn_slab((1 << 31) - 1, k, bytes=by)
            assert s % 128 == 0 and s >= 1024 and (s == 1024 or s * (4 * k + 64) * kb <= 1 << 32)


def test_refusals(g):
    lib = g.load_library()
    out = C.c_uint32(0)
    assert lib.gbnns_debug_knn_slab(1, 300, 10, None) == INVALID
    for bytes_, nq, k in ((2, 300, 10), (-1, 300, 10), (1, 1 << 31, 10), (0, 300, 0), (0, 300, 4097), (1, 300, -5)):
        assert lib.gbnns_debug_knn_slab(bytes_, nq, k, C.byref(out)) == INVALID, (bytes_, nq, k)


def test_knob_rounding_and_cap(g):
    for v, want in ((1, 128), (127, 128), (128, 128), (200, 128), (256, 256), (257, 256), (383, 256), (384, 384)):
        with ku.knobs(g, knn_slab=v):
            for by in (True, False):
                for k in KS:
                    assert g.knn_slab(10**6, k, bytes=by) == want, (v, k, by)
                    for nq in NQS:   # never more than n_q, never more than the default
                        s = g.knn_slab(nq, k, bytes=by)
                        assert s == min(nq, want) and s <= formula(nq, k, 8 if by else 4), (v, nq, k, by)
            assert g.knn_bytes_plan(6000, 300, 64, 10)["slab"] == min(300, want)
            assert ku.slabs(min(300, want), 300) == ([(0, 128), (128, 128), (256, 44)] if want == 128 else [(0, 256), (256, 44)] if want == 256 else [(0, 300)])
    with ku.knobs(g, knn_slab=1 << 30):   # a cap above the 4 GiB rule changes nothing
        for k in KS:
            assert g.knn_slab(10**6, k, bytes=True) == formula(10**6, k, 8) and g.knn_slab(10**6, k, bytes=False) == formula(10**6, k, 4)
    for v in (0, -1, -128):   # 0 (and below) is the default rule
        with ku.knobs(g, knn_slab=128):
            assert g.load_library().gbnns_debug_knob(b"knn_slab", v) == 0
            assert g.knn_slab(10**6, 4096, bytes=True) == 32640 and g.knn_slab(10**6, 10, bytes=False) == formula(10**6, 10, 4)


def test_helper_restores_the_knob(g):
    default = [g.knn_slab(10**6, k, bytes=by) for k in KS for by in (True, False)]
    now = lambda: [g.knn_slab(10**6, k, bytes=by) for k in KS for by in (True, False)]
    with ku.knobs(g, knn_slab=128):
        assert set(now()) == {128}
    assert now() == default
    with pytest.raises(ZeroDivisionError):
        with ku.knobs(g, knn_slab=256, knn_chunk=64):
            assert set(now()) == {256}
            1 // 0
    assert now() == default and g.knn_bytes_plan(20000, 40, 32, 30)["max_chunk"] == 4 << 15
    with ku.knobs(g, knn_chunk=64):   # a block that does not name the knob leaves it alone inside and at 0 behind it
        assert now() == default
    assert now() == default


def test_knob_leaves_the_rest_of_the_plan(g):
    shapes = [(n, nq, d, k) for n in (5, 40, 1037, 12000, 10**6) for nq in (1, 300, 10**6) for d in (1, 32, 100, 256) for k in (1, 10, 64, 1000, 4096)]
    rest = lambda p: {key: v for key, v in p.items() if key != "slab"}
    for kn in (dict(), dict(knn_chunk=512, knn_pool_min_k=10)):
        with ku.knobs(g, **kn):
            before = [g.knn_bytes_plan(*s) for s in shapes]
        with ku.knobs(g, knn_slab=128, **kn):
            during = [g.knn_bytes_plan(*s) for s in shapes]
        assert [rest(p) for p in during] == [rest(p) for p in before]
        assert all(p["slab"] == min(s[1], 128) for p, s in zip(during, shapes))
        assert set(before[0]) == {"dp", "cap", "first_rows", "max_chunk", "pool", "slab"}


def test_fixture_preconditions(orc):
    """The fixtures of tests/test_gpu_knn_slabs.py hold what they promise, from the oracle alone: ordered by the k-th distance the queries
    differ strictly at stride 128, their thresholds in the sweep kernels' form the other way round (su.ordered asserts both), the tag words and their allowed rows differ at stride 128, and the three groups
    of queries end up in the three slabs."""
    import knn_slabs_util as su
    cases = [(su.byte_case(m, d, 700 + d + m), m, (10, 64, 200)) for m, d in ((ku.L2, 64), (ku.L2, 100), (ku.NEG_DOT, 128))]
    cases += [(su.float_case(d, 800 + d), ku.L2, (7, 64)) for d in (32, 128)]
    for (base, q, T, Q, group), metric, ks in cases:
        refs = su.references(orc, base, q, T, Q, metric)
        for k in ks:
            for tagged in (0, 1):
                qo, Qo, (ids, dist) = su.ordered(q, Q, refs[tagged], k, metric=metric)
                assert ids.shape == (su.NQ, k) and (np.diff(dist[:, k - 1]) >= 0).all()
                kth = refs[tagged][1][:, k - 1]
                assert kth[group == 0].max() < kth[group == 1].min() and kth[group == 1].max() < kth[group == 2].min()
                if tagged:
                    su.check_tag_offsets(T, Qo)
    assert ku.slabs(su.SLAB, su.NQ) == [(0, 128), (128, 128), (256, 44)]
    # the float input of test_overflowing_chunks_are_swept_again_in_every_slab (k = 100, "knn_chunk" = 512): the pool rule's chunk for that
    # n, and more hits of the centre query (every allowed row: the rows come farthest first) than a list holds in the first chunk of that
    # length -- the first chunk longer than cap but for the tagged input, whose 896 rows at r0 = 896 hold fewer allowed ones than cap --
    # and, for the slab loop, some query with more rows to keep than cap in some chunk of EVERY slab
    for tagged, chunk in ((False, 768), (True, 1280)):
        n = su.FLOAT_OVERFLOW_N[tagged]
        base, q, T, Q = su.overflow_case(100, n=n)
        allowed = (T & Q[0]) != 0 if tagged else np.ones(n, bool)
        assert (Q == Q[0]).all() and (not tagged or 0.45 * n < np.count_nonzero(allowed) < 0.55 * n)
        plan = su.float_pool_plan(n, 100, 512)
        assert plan["cap"] == 464 and plan["first_rows"] == 448 and plan["max_chunk"] == chunk
        chunks = ku.chunk_plan(plan, n)
        j = next(j for j, (_, rows) in enumerate(chunks) if rows == chunk)
        assert all(rows <= plan["cap"] or (tagged and rows == 896) for _, rows in chunks[:j])
        kept = su.kept_rows(plan, base, q, allowed, 100)
        r0 = chunks[j][0]
        assert kept[0, j] == np.count_nonzero(allowed[r0:r0 + chunk]) > plan["cap"], (tagged, kept[0, j])
        for q0, qn in ku.slabs(su.SLAB, su.NQ):
            assert (kept[q0:q0 + qn] > plan["cap"]).any(axis=0).sum() >= 4, (tagged, q0)
