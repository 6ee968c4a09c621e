"""The plan of gbnns_exact_knn under the negative dot, without a device: with "knn_filter_dot" = 2 gbnns_debug_knn_plan names knn_dot.hip's
K-looped matrix-core filter for float rows of d % 8 == 0, 8 <= d <= 1024, k <= 512, n > 4 k, and the exact scan for every other shape;
with the knob at its default of 0, or with the L2 filters' knobs alone, every such shape is a scan; binary16 rows never take it.
tests/test_gpu_knn_dot.py runs it."""
import pytest

L2, NEG_DOT = 0, 1
N, NQ = 4096, 165
DOT_SHAPES = [(d, k, tagged) for d in (8, 96, 200, 1024) for k in (1, 512) for tagged in (False, True)]
# (metric, n, d, k): beyond 1024, k > 512, n = 4 k, the L2 metric
SCAN_SHAPES = [(NEG_DOT, N, 1032, 10), (NEG_DOT, N, 200, 513), (NEG_DOT, 2048, 200, 512), (L2, N, 200, 10)]


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _knob(g, name, value):
    assert g.load_library().gbnns_debug_knob(name, value) == 0   # (the parent refuses b"knn_filter_dot")


@pytest.fixture
def dot(g):
    try:
        _knob(g, b"knn_filter_dot", 2)
        yield g
    finally:
        _knob(g, b"knn_filter_dot", 0)


def _is_scan(name):
    return name.startswith("knn_scan_kernel<") or name.startswith("knn_scan_wide_kernel<")


@pytest.mark.parametrize("d,k,tagged", DOT_SHAPES)
def test_the_knob_names_the_dot_filter(dot, d, k, tagged):
    name = "knn_dot_filter_kernel<2, %s>" % ("true" if tagged else "false")
    assert dot.knn_plan(False, NEG_DOT, N, NQ, d, k, tagged) == (name, False)


@pytest.mark.parametrize("metric,n,d,k", SCAN_SHAPES)
def test_refused_shapes_keep_the_scan(dot, metric, n, d, k):
    name, pool = dot.knn_plan(False, metric, n, NQ, d, k)
    assert _is_scan(name) and not pool


def test_half_rows_are_unchanged_by_the_knob(g):
    before = [g.knn_half_plan(N, NQ, d, 10, NEG_DOT) for d in (96, 200)]
    try:
        _knob(g, b"knn_filter_dot", 2)
        after = [g.knn_half_plan(N, NQ, d, 10, NEG_DOT) for d in (96, 200)]
    finally:
        _knob(g, b"knn_filter_dot", 0)
    assert after == before and all(p["path"] == "scan" and p["kernel"].endswith("half>") for p in after)


def test_the_value_is_clamped(g, dot):
    _knob(g, b"knn_filter_dot", 7)   # 2: by shape, not by size
    assert g.knn_plan(False, NEG_DOT, 100, 1, 8, 1)[0] == "knn_dot_filter_kernel<2, false>"
    _knob(g, b"knn_filter_dot", -3)  # 0
    assert _is_scan(g.knn_plan(False, NEG_DOT, N, NQ, 200, 10)[0])


def test_by_size_starts_at_the_smallest_measured_class(g, dot):
    _knob(g, b"knn_filter_dot", 1)
    assert g.knn_plan(False, NEG_DOT, 100000, 1000, 96, 100)[0] == "knn_dot_filter_kernel<2, false>"
    assert _is_scan(g.knn_plan(False, NEG_DOT, 99999, 1000, 96, 100)[0])
    assert _is_scan(g.knn_plan(False, NEG_DOT, 100000, 999, 96, 100)[0])


@pytest.mark.parametrize("knobs", [(), (b"knn_filter",), (b"knn_filter_wide",), (b"knn_filter", b"knn_filter_wide")], ids=str)
def test_the_default_and_the_l2_knobs_keep_the_scan(g, knobs):
    try:
        for name in knobs:
            _knob(g, name, 2)
        for d, k, tagged in DOT_SHAPES:
            assert _is_scan(g.knn_plan(False, NEG_DOT, N, NQ, d, k, tagged)[0]), (d, k, tagged)
    finally:
        _knob(g, b"knn_filter", 1)
        _knob(g, b"knn_filter_wide", 0)
