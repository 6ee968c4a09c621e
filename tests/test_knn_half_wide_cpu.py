"""The plan of gbnns_exact_knn_half on binary16 rows wider than 128 dims, without a device: with "knn_half_wide" = 2
gbnns_debug_knn_half_plan names knn_half_wide.hip's K-looped f16 matrix-core filter for L2, 128 < d <= 1024, d % 4 == 0, k <= 512,
n > 4 k -- swept from a copy where the stride is no multiple of 8 halves -- and the exact scan for every other shape; at the default of 0,
or with the float rows' "knn_filter_wide" alone, every shape is a scan.  tests/test_gpu_knn_half_wide.py runs it."""
import pytest

L2, NEG_DOT = 0, 1
N, NQ = 4096, 165
WIDE_SHAPES = [(d, k, tagged) for d in (132, 136, 300, 960, 1024) for k in (1, 512) for tagged in (False, True)]
# (metric, n, d, k): beyond 1024, d % 4 != 0, the dot metric, k > 512, n = 4 k
SCAN_SHAPES = [(L2, N, 1028, 10), (L2, N, 130, 10), (NEG_DOT, N, 960, 10), (L2, N, 960, 513), (L2, 2048, 960, 512)]


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


@pytest.fixture
def knob(g):
    lib = g.load_library()
    try:
        yield lambda name, v: lib.gbnns_debug_knob(name, v) == 0 or pytest.fail("knob %r refused" % name)   # (the parent refuses "knn_half_wide")
    finally:
        lib.gbnns_debug_knob(b"knn_half_wide", 0)
        lib.gbnns_debug_knob(b"knn_filter_wide", 0)


def _scans(plan):
    return plan["path"] == "scan" and plan["kernel"].startswith("knn_scan_wide_kernel<") and plan["kernel"].endswith("half>") and not plan["packed"]


@pytest.mark.parametrize("d,k,tagged", WIDE_SHAPES)
def test_the_knob_names_the_wide_filter(g, knob, d, k, tagged):
    knob(b"knn_half_wide", 2)
    name = "knn_half_wide_filter_kernel<2, %s>" % ("true" if tagged else "false")
    for stride in (0, (d + 7) // 8 * 8):   # the caller's array at stride d, a handle's rows at whole 16-byte chunks
        want = {"kernel": name, "path": "filter", "pool": False, "packed": (stride or d) % 8 != 0}
        assert g.knn_half_plan(N, NQ, d, k, stride=stride, tagged=tagged) == want


@pytest.mark.parametrize("metric,n,d,k", SCAN_SHAPES)
def test_refused_shapes_keep_the_scan(g, knob, metric, n, d, k):
    knob(b"knn_half_wide", 2)
    assert _scans(g.knn_half_plan(n, NQ, d, k, metric=metric))


def test_the_default_and_the_float_rows_knob_keep_the_scan(g, knob):
    for float_knob in (0, 2):
        knob(b"knn_filter_wide", float_knob)
        for d, k, tagged in WIDE_SHAPES:
            assert _scans(g.knn_half_plan(N, NQ, d, k, tagged=tagged)), (float_knob, d, k)


def test_by_size_starts_at_the_smallest_measured_class(g, knob):
    knob(b"knn_half_wide", 1)
    assert g.knn_half_plan(100000, 1000, 960, 100)["kernel"] == "knn_half_wide_filter_kernel<2, false>"
    assert _scans(g.knn_half_plan(99999, 1000, 960, 100)) and _scans(g.knn_half_plan(100000, 999, 960, 100))
    knob(b"knn_half_wide", 7)   # (clamped to 2)
    assert g.knn_half_plan(99999, 999, 960, 100)["path"] == "filter"
