"""The plan of gbnns_exact_knn_half under the negative dot, without a device: with "knn_half_dot" = 2 gbnns_debug_knn_half_plan names
knn_half_dot.hip's filter for d % 8 == 0, 8 <= d <= 1024, k <= 512, n > 4 k -- swept from a copy where the stride is no multiple of 8 halves
-- and the scan for every other shape; at 0, or with the other filters' knobs alone, every shape is a scan; float plans never move."""
import pytest

L2, NEG_DOT = 0, 1
N, NQ = 4096, 165
DOT_SHAPES = [(d, k, tagged) for d in (8, 96, 200, 1024) for k in (1, 512) for tagged in (False, True)]
SCAN_SHAPES = [(NEG_DOT, N, 1032, 10), (NEG_DOT, N, 200, 513), (NEG_DOT, 2048, 200, 512), (L2, N, 200, 10)]   # (metric, n, d, k): d > 1024, k > 512, n = 4 k, L2
OTHERS = (b"knn_filter", b"knn_half_wide", b"knn_filter_dot")


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


@pytest.fixture
def knob(g):
    lib = g.load_library()
    try:
        yield lambda name, v: lib.gbnns_debug_knob(name, v) == 0 or pytest.fail("knob %r refused" % name)   # (the parent refuses "knn_half_dot")
    finally:
        for name, v in ((b"knn_half_dot", 0), (b"knn_filter", 1), (b"knn_half_wide", 0), (b"knn_filter_dot", 0)):
            lib.gbnns_debug_knob(name, v)


def _scans(plan):
    return plan["path"] == "scan" and plan["kernel"].startswith("knn_scan_") and plan["kernel"].endswith("half>") and not plan["packed"]


@pytest.mark.parametrize("d,k,tagged", DOT_SHAPES)
def test_the_knob_names_the_half_dot_filter(g, knob, d, k, tagged):
    knob(b"knn_half_dot", 2)
    name = "knn_half_dot_filter_kernel<2, %s>" % ("true" if tagged else "false")
    for stride in (0, d + 4):   # the caller's array at stride d: in place; a stride of no whole 16-byte chunks: a copy
        want = {"kernel": name, "path": "filter", "pool": False, "packed": stride != 0}
        assert g.knn_half_plan(N, NQ, d, k, NEG_DOT, stride=stride, tagged=tagged) == want


@pytest.mark.parametrize("metric,n,d,k", SCAN_SHAPES)
def test_refused_shapes_keep_the_scan(g, knob, metric, n, d, k):
    knob(b"knn_half_dot", 2)
    assert _scans(g.knn_half_plan(n, NQ, d, k, metric))


@pytest.mark.parametrize("others", [(), OTHERS[:1], OTHERS[1:2], OTHERS[2:], OTHERS], ids=str)
def test_the_default_and_the_other_knobs_keep_the_scan(g, knob, others):
    for name in others:
        knob(name, 2)
    for d, k, tagged in DOT_SHAPES:
        for stride in (0, d + 4):
            assert _scans(g.knn_half_plan(N, NQ, d, k, NEG_DOT, stride=stride, tagged=tagged)), (d, k, tagged, stride)


def test_by_size_starts_at_the_smallest_measured_class(g, knob):
    knob(b"knn_half_dot", 1)
    assert g.knn_half_plan(100000, 1000, 96, 100, NEG_DOT)["kernel"] == "knn_half_dot_filter_kernel<2, false>"
    assert _scans(g.knn_half_plan(99999, 1000, 96, 100, NEG_DOT)) and _scans(g.knn_half_plan(100000, 999, 96, 100, NEG_DOT))
    knob(b"knn_half_dot", 7)    # (clamped to 2: by shape, not by size)
    assert g.knn_half_plan(100, 1, 8, 1, NEG_DOT)["kernel"] == "knn_half_dot_filter_kernel<2, false>"
    knob(b"knn_half_dot", -3)   # (clamped to 0)
    assert _scans(g.knn_half_plan(N, NQ, 200, 10, NEG_DOT))


def test_float_plans_are_unchanged_by_the_knob(g, knob):
    shapes = [(metric, d, k) for metric in (L2, NEG_DOT) for d in (96, 200, 1024) for k in (1, 512)]
    before = [g.knn_plan(False, metric, N, NQ, d, k) for metric, d, k in shapes]
    knob(b"knn_half_dot", 2)
    assert [g.knn_plan(False, metric, N, NQ, d, k) for metric, d, k in shapes] == before
