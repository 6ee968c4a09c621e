"""Every instance of knn_bytes_sweep_kernel, knn_filter_kernel, knn_scan_kernel and knn_scan_wide_kernel on an MI355X (run with -m gpu):
the cases of tests/knn_instances.py, ids and distance bit patterns of every query against the CPU oracle -- orc.exact_knn over the widened
arrays, knn_tagged_util.expected for the tagged calls.  gbnns_debug_knn_plan, asked under the case's knobs right before the call, says
that the instance the case names is what the call takes (tests/test_knn_instances_cpu.py: the names cover all 54).  No tolerance."""
import pytest

import knn_bytes_util as ku
import knn_instances as ki
import knn_tagged_util as kt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@pytest.mark.parametrize("c", ki.CASES, ids=[c.id for c in ki.CASES])
def test_instance_equals_the_oracle(g, orc, c):
    base, q = ki.data(c.bytes, c.d, c.nq)
    kw = {}
    if c.tagged:
        T, Q = ki.tags(c)
        kw = dict(row_tags=T, query_tags=Q)
    want = ki.expected(orc, c)
    with ku.knobs(g, **c.knob_dict):
        assert g.knn_plan(c.bytes, c.metric, c.n, c.nq, c.d, c.k, c.tagged) == (c.name, c.pool)
        got = g.exact_knn(base, q, c.k, c.metric, want_dist=True, **kw)
    kt.same(got, want, c)
