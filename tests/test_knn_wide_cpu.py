"""The plan of gbnns_exact_knn on float rows wider than 128 dims, without a device: with "knn_filter_wide" = 2 gbnns_debug_knn_plan names
knn_wide.hip's K-looped matrix-core filter for L2, 128 < d <= 1024, d % 4 == 0, k <= 512, n > 4 k, and the exact scan for every other
shape; with the knob at its default of 0 every shape is a scan; binary16 rows never take it.  tests/test_gpu_knn_wide.py runs it."""
import pytest

L2, NEG_DOT = 0, 1
N, NQ = 4096, 165
WIDE_SHAPES = [(d, k, tagged) for d in (132, 300, 960, 1024) for k in (1, 512) for tagged in (False, True)]
# (metric, n, d, k): beyond 1024, d % 4 != 0, the dot metric, k > 512, n = 4 k
SCAN_SHAPES = [(L2, N, 1028, 10), (L2, N, 130, 10), (NEG_DOT, N, 960, 10), (L2, N, 960, 513), (L2, 2048, 960, 512)]


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


@pytest.fixture
def wide(g):
    lib = g.load_library()
    try:
        assert lib.gbnns_debug_knob(b"knn_filter_wide", 2) == 0   # (the parent refuses the name)
        yield g
    finally:
        lib.gbnns_debug_knob(b"knn_filter_wide", 0)


def _name(tagged):
    return "knn_wide_filter_kernel<2, %s>" % ("true" if tagged else "false")


@pytest.mark.parametrize("d,k,tagged", WIDE_SHAPES)
def test_the_knob_names_the_wide_filter(wide, d, k, tagged):
    assert wide.knn_plan(False, L2, N, NQ, d, k, tagged) == (_name(tagged), False)


@pytest.mark.parametrize("metric,n,d,k", SCAN_SHAPES)
def test_refused_shapes_keep_the_scan(wide, metric, n, d, k):
    name, pool = wide.knn_plan(False, metric, n, NQ, d, k)
    assert name.startswith("knn_scan_wide_kernel<") and not pool


def test_half_rows_keep_the_scan(wide):
    plan = wide.knn_half_plan(N, NQ, 960, 10)
    assert plan["path"] == "scan" and plan["kernel"].startswith("knn_scan_wide_kernel<") and plan["kernel"].endswith("half>")


def test_by_size_starts_at_the_smallest_measured_class(g):
    lib = g.load_library()
    try:
        assert lib.gbnns_debug_knob(b"knn_filter_wide", 1) == 0
        assert g.knn_plan(False, L2, 100000, 1000, 960, 100)[0] == _name(False)
        assert g.knn_plan(False, L2, 99999, 1000, 960, 100)[0].startswith("knn_scan_wide_kernel<")
        assert g.knn_plan(False, L2, 100000, 999, 960, 100)[0].startswith("knn_scan_wide_kernel<")
    finally:
        lib.gbnns_debug_knob(b"knn_filter_wide", 0)


def test_the_default_is_the_scan(g):
    for metric, n, d, k in SCAN_SHAPES + [(L2, N, d, k) for d, k, _ in WIDE_SHAPES]:
        for tagged in (False, True):
            assert g.knn_plan(False, metric, n, NQ, d, k, tagged)[0].startswith("knn_scan_wide_kernel<"), (metric, n, d, k)
