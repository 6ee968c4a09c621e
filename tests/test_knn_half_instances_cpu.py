"""The census of the half-row exact-kNN kernel instances without a device: gbnns_debug_knn_half_plan names what every case of
tests/knn_half_instances.py launches, on which path and from which table (in place / a copy); the names cover the 16 + 12 + 10 instances
exactly, the shapes are the ones the table promises, the wide classes' bounds are knn_scan_pick<uint16_t>'s and no tagged case is vacuous.
tests/test_gpu_knn_half_instances.py runs what is proven here."""
import numpy as np
import pytest

import knn_bytes_util as ku
import knn_half_instances as kh
import knn_half_util as hu


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _plan(g, c):
    with ku.knobs(g, **c.knob_dict):
        return g.knn_half_plan(c.n, c.nq, c.d, c.k, c.metric, tagged=c.tagged)


def test_every_case_takes_the_instance_it_names(g):
    for c in kh.CASES:
        p = _plan(g, c)
        assert (p["kernel"], p["path"], p["packed"]) == (c.name, c.path, c.packed), (c, p)
        assert p["pool"] == (c.path == "pool"), (c, p)
    # the knobs came back: the swept shapes are scans by default, nothing packed
    for c in kh.CASES:
        p = g.knn_half_plan(c.n, c.nq, c.d, c.k, c.metric, tagged=c.tagged)
        assert p["path"] == "scan" and p["kernel"].startswith("knn_scan_") and p["kernel"].endswith(", half>") and not p["packed"], (c, p)


def test_the_names_cover_every_instance_exactly():
    want = kh.instance_names()
    assert [len(want[f]) for f in ("sweep", "scan", "wide")] == [16, 12, 10]
    got = {}
    for c in kh.CASES:
        got.setdefault(c.name, []).append(c)
    assert set(got) == set().union(*want.values()) and len(got) == 38
    # every sweep instance in front of heaps and of pools, on a copy and in place, at k = 64 and as a short pool under "knn_pool_min_k" = 1
    for name in want["sweep"]:
        cs = got[name]
        assert {c.path for c in cs} == {"filter", "pool"}, name
        assert {c.packed for c in cs} == {False, True}, name
        assert {(c.path, c.packed) for c in cs} >= {("filter", True), ("filter", False), ("pool", True), ("pool", False)}, name
        assert any(c.path == "pool" and c.k == 64 for c in cs) and any(c.path == "pool" and c.knob_dict.get("knn_pool_min_k") == 1 for c in cs), name
        # ... and on mostly subnormal halves and on halves near the format's end
        assert {"subnormal", "large", "unit"} <= {c.cls for c in cs}, name
    cases = [c for name in want["sweep"] for c in got[name]]
    assert {c.k for c in cases if c.path == "filter"} == {1, 10}
    assert {c.k for c in cases if c.path == "pool"} == {10, 64}
    assert all(c.knob_dict.get("knn_pool_min_k") == 1 for c in cases if c.path == "pool" and c.k < 64)
    # the sweep cases are forced ("knn_filter" = 2), nothing else is
    for c in kh.CASES:
        assert (c.knob_dict.get("knn_filter") == 2) == c.name.startswith("knn_half_sweep_kernel") == (c.path != "scan"), c
        assert c.tagged == (", true" in c.name) and (not c.tagged or c.k >= 10), c
        assert not c.packed or c.path != "scan", c


def test_shapes():
    """n = 1 037 with chunks of 64 rows; n_q = 128 QB + 37; per K step count d = 16 K - 12 (a copy), 16 K - 8 (in place, clamped) and 16 K;
    per scan class the narrowest and the widest d, L2 also widest - 2."""
    for c in kh.CASES:
        assert c.n == 1037 and c.nq == kh.queries_per_workgroup(c.name) + 37, c
        assert c.knob_dict.get("knn_chunk", 64) == 64, c
    for ks, qb in kh.SWEEP_QB.items():
        for tagged in (False, True):
            cs = [c for c in kh.CASES if c.name == "knn_half_sweep_kernel<%d, %d, %s>" % (ks, qb, "true" if tagged else "false")]
            assert {(c.d, c.packed) for c in cs} == {(16 * ks - 12, True), (16 * ks - 8, False), (16 * ks, False)}, (ks, tagged)
            assert all(c.metric == kh.L2 for c in cs)
    for s, qpt, narrow, full in kh.SCAN_CLASSES:
        for tagged in ("false", "true"):
            l2 = {c.d for c in kh.CASES if c.name == "knn_scan_kernel<0, %d, %d, %s, half>" % (s, qpt, tagged)}
            dot = {c.d for c in kh.CASES if c.name == "knn_scan_kernel<1, %d, %d, %s, half>" % (s, qpt, tagged)}
            assert l2 == {narrow[0], full - 2, full} and dot == {narrow[1], full}, (s, tagged)
    for metric, r, narrow, full, full_tagged in kh.WIDE_CLASSES:
        for tagged in (False, True):
            ds = {c.d for c in kh.CASES if c.name == "knn_scan_wide_kernel<%d, %d, %s, half>" % (metric, r, "true" if tagged else "false")}
            assert ds == {narrow, full_tagged if tagged else full}, (metric, r, tagged)


def test_class_bounds_are_the_half_row_pick_s(g):
    """The scan classes' and the wide classes' bounds against knn_scan_pick<uint16_t>, from both sides: the widest d of a class takes it,
    the next row length the metric allows does not (or is refused: d > 8 192)."""
    def kernel(metric, d, tagged):
        return g.knn_half_plan(kh.N, 165, d, 10, metric, tagged=tagged)["kernel"]
    step = {kh.L2: 1, kh.NEG_DOT: 8}
    for s, qpt, narrow, full in kh.SCAN_CLASSES:
        for metric in (kh.L2, kh.NEG_DOT):
            for tagged in (False, True):
                name = "knn_scan_kernel<%d, %d, %d, %s, half>" % (metric, s, qpt, "true" if tagged else "false")
                assert kernel(metric, narrow[metric], tagged) == name and kernel(metric, full, tagged) == name
                assert kernel(metric, full + step[metric], tagged) != name
                if narrow[metric] > 8:
                    assert kernel(metric, narrow[metric] - 4 * (1 + metric), tagged) != name
    for metric, r, narrow, full, full_tagged in kh.WIDE_CLASSES:
        for tagged in (False, True):
            name = "knn_scan_wide_kernel<%d, %d, %s, half>" % (metric, r, "true" if tagged else "false")
            top = full_tagged if tagged else full
            assert kernel(metric, narrow, tagged) == name and kernel(metric, top, tagged) == name, (name, narrow, top)
            # (a tagged class begins where the 64 bytes of tag words push the class before it out: at that one's widest tagged d + 32)
            prev = [c[4] for c in kh.WIDE_CLASSES if c[0] == metric and c[1] == 2 * r]
            if tagged and prev:
                assert kernel(metric, prev[0], True) != name and kernel(metric, prev[0] + 32, True) == name, name
            else:
                assert kernel(metric, narrow - 4 * (1 + metric), tagged) != name, name
            # (the tile rounds d / 4 up to 8 steps: the next length that needs more room is 32 columns on)
            if top < 8192:
                assert kernel(metric, top + 32, tagged) != name, name
            else:
                with pytest.raises(g.GbnnsError):
                    kernel(metric, top + 8, tagged)


def test_no_tagged_case_is_vacuous():
    """Every query word of a tagged case allows some rows but not all, and at least one word allows fewer than k rows."""
    seen = set()
    for c in kh.CASES:
        if not c.tagged:
            continue
        T, Q = kh.tags(c)
        assert len(T) == c.n and len(Q) == c.nq and len(np.unique(Q)) == len(kh.TAG_WORDS) == 9
        counts = np.array([np.count_nonzero(T & w) for w in np.unique(Q)])
        assert (counts > 0).all() and (counts < c.n).all(), (c, counts)
        assert (counts < c.k).any() and (counts >= c.k).any(), (c, counts)
        seen.add(c.name)
    assert len(seen) == 38 // 2


def test_data():
    """Every eighth row duplicates the row before it, the first four queries are rows (one of them a duplicated row), the subnormal class
    is mostly subnormal halves and the large class reaches beyond 2^15 without an infinity; the named queries of a d > 128 case."""
    for cls in hu.SCALE:
        rows, q = kh.data(24, 165, cls)
        assert rows.dtype == np.float16 and q.dtype == np.float32 and rows.shape == (kh.N, 24) and q.shape == (165, 24)
        assert np.isfinite(rows.astype(np.float32)).all() and np.isfinite(q).all()
        assert np.array_equal(rows[7::8], rows[6::8][:len(rows[7::8])])
        assert np.array_equal(q[:4], rows[list(kh.QUERY_ROWS)].astype(np.float32))
        dup = kh.QUERY_ROWS[kh.DUPLICATE_QUERY]
        assert np.array_equal(rows[dup], rows[dup + 1])
        a = np.abs(rows.astype(np.float32))
        if cls == "subnormal":
            assert np.count_nonzero((a > 0) & (a < 2.0 ** -14)) > a.size // 2
        if cls == "large":
            assert a.max() > 2.0 ** 14
    named = kh.named_queries(165)
    assert len(set(named.tolist())) == 8 and {0, kh.DUPLICATE_QUERY, 127, 128, 164} <= set(named.tolist())
