"""Every instance of knn_half_sweep_kernel and every binary16 instance of knn_scan_kernel / knn_scan_wide_kernel on an MI355X (run with
-m gpu): the cases of tests/knn_half_instances.py, ids and distance bit patterns against the plain reference of tests/knn_half_util.py --
ordered float32 sums on the widened rows, numpy's sort of (distance, id); tagged cases filter the same reference.  Rows of d <= 128: every
query.  Wider rows (the per-column numpy loop over every query is too slow there): every query against the CPU oracle over the widened
rows, and the eight named queries of knn_half_instances.named_queries against the plain reference.  gbnns_debug_knn_half_plan, asked
under the case's knobs right before the call, says that the instance, the path and the table the case names are what the call takes
(tests/test_knn_half_instances_cpu.py: the names cover all 38).  No tolerance."""
import pytest

import knn_bytes_util as ku
import knn_half_instances as kh
import knn_half_util as hu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@pytest.mark.parametrize("c", kh.CASES, ids=[c.id for c in kh.CASES])
def test_instance_equals_the_reference(g, orc, c):
    rows, q = kh.data(c.d, c.nq, c.cls)
    kw = {}
    if c.tagged:
        T, Q = kh.tags(c)
        kw = dict(row_tags=T, query_tags=Q)
    with ku.knobs(g, **c.knob_dict):
        p = g.knn_half_plan(c.n, c.nq, c.d, c.k, c.metric, tagged=c.tagged)
        assert (p["kernel"], p["path"], p["packed"]) == (c.name, c.path, c.packed), p
        got = g.exact_knn(rows, q, c.k, c.metric, want_dist=True, **kw)
    if c.d <= 128:
        hu.same(got, kh.expected(c), c.id)
    else:
        named = kh.named_queries(c.nq)
        hu.same(got, kh.expected(c, named), c.id + " named queries", queries=named)
        hu.same(got, kh.expected_oracle(orc, c), c.id + " oracle")
