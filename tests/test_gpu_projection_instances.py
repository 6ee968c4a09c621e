"""Every reachable projection kernel instance on the device (run with -m gpu on an MI355X): the cases of tests/projection_instances.py.

Per case: the handle's knobs are set, gbnns_debug_project_plan for the handle's CU count must name the case's instances (the table is
written for 256 compute units), the search runs -- a plain call, or three deferred calls in flight and a join --, and
gbnns_index_project_last must report the same instances from the launchers.  Exact instances: q_low equals the CPU oracle's projection
bit for bit on full-mantissa queries through full-mantissa nets, ids equal the oracle's search at ef 40.  The matrix-core option is
approximate by contract: 0 < max |q_low - exact| < 2e-6, at most max(1, n_q / 200) ids differ, and copies of one query in different row
blocks and workgroups (projection_instances.copy_rows) come out bit-identical.
"""
import time

import numpy as np
import pytest

import golden_util as gu
import oracle as orc_mod
import projection_instances as pi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


_REF = {}


def _reference(orc, c):
    """The oracle's projections and answers of a case's data, computed once per (net, queries) and shared (read only)."""
    key = (c.d, c.dh, c.dl, c.nq * pi.batches(c), c.mfma)
    if key not in _REF:
        base, queries, net, off, nbr, ent = pi.data(*key)
        want_q, db_low = orc.project(net, queries, threads=8), orc.project(net, base, threads=8)
        ids = orc.search_batch(orc_mod.MODE_NET, queries, base, off, nbr, pi.EF, db_low=db_low, net=net, entries=ent, threads=8)["ids"]
        for a in (want_q, db_low, ids):
            a.setflags(write=False)
        _REF[key] = (want_q, db_low, ids)
    return _REF[key]


@pytest.mark.parametrize("c", pi.CASES, ids=[c.id for c in pi.CASES])
def test_instance(g, orc, c):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)   # (a copy: the shared arrays are read only)
    t0 = time.perf_counter()
    nb = pi.batches(c)
    base, queries, net, off, nbr, ent = pi.data(c.d, c.dh, c.dl, c.nq * nb, c.mfma)
    want_q, db_low, want_ids = _reference(orc, c)
    t1 = time.perf_counter()
    ix = g.Index(t(base), off, nbr, db_low=t(db_low), net=tuple(t(x) for x in net))
    try:
        for name, value in c.knobs:
            ix.knob(name, value)
        cus = ix.knob_get("cus")
        plan = g.project_plan(c.d, c.dh, c.dl, c.nq, cus, c.flight, c.mfma, **{k: ix.knob_get(k) for k in ("mlp_net", "mlp_slab", "mlp_small")})
        assert plan == c.names, "the table of tests/projection_instances.py is written for 256 compute units; this device has %d and plans %r" % (cus, plan)
        flags = (g.FLAG_MFMA_PROJECTION if c.mfma else 0) | (g.FLAG_DEFER_JOIN if c.flight else 0)
        parts = [slice(i * c.nq, (i + 1) * c.nq) for i in range(nb)]
        outs, launched = [], []
        for p in parts:
            kw = dict(flags=flags, defer_depth=3) if c.flight else dict(flags=flags)
            outs.append(ix.search(t(queries[p]), pi.EF, entry_ids=t(ent[p].astype(np.int32)), want=("q_low",), out={}, **kw))
            launched.append(ix.project_last())
        if c.flight:
            ix.join()
        torch.cuda.synchronize()
        assert launched == [c.names] * nb, launched
        t2 = time.perf_counter()
        for p, r in zip(parts, outs):
            q_low, ids = r["q_low"].cpu().numpy(), r["ids"].cpu().numpy().view(np.uint32)
            if not c.mfma:
                bad = int((gu.bits(q_low) != gu.bits(want_q[p])).sum())
                assert bad == 0, "%s: %d of %d q_low words differ from the oracle's (batch %d)" % (c.id, bad, q_low.size, p.start // c.nq)
                assert np.array_equal(ids, want_ids[p]), (c.id, p, int((ids != want_ids[p]).sum()))
                continue
            err = float(np.abs(q_low - want_q[p]).max())
            diff = int((ids != want_ids[p]).sum())
            print("matrix-core", c.id, "max |q_low - exact| %.3g, ids that differ %d of %d" % (err, diff, c.nq))
            assert 0 < err < 2e-6, (c.id, err)
            assert diff <= max(1, c.nq // 200), (c.id, diff)
            dst, src = pi.copy_rows(c.nq)
            assert len(dst) or pi.mfma_rows(c.nq) < 4
            bad = int((gu.bits(q_low[dst]) != gu.bits(q_low[src])).sum())
            assert bad == 0, "%s: %d q_low words of %d copied queries differ from their sources'" % (c.id, bad, len(dst))
    finally:
        ix.close()
    print("projection instance %s: data and oracle %.2f s, device %.2f s, checks %.2f s" % (c.id, t1 - t0, t2 - t1, time.perf_counter() - t2))
