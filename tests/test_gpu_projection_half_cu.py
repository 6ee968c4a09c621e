"""GPU parity of the half-CU form of the one-launch projection (run with -m gpu on an MI355X).

mlp_net_kernel has two forms (csrc/mlp_net.hip): workgroups of eight wavefronts, one per CU, and of four wavefronts and at most
80 KB of LDS, two per CU, which batches in flight take (one fits a CU the walks of the other batches have half left).  Both
restate GetLowQueryFromNet (support_func.h:645-658) rounding for rounding; here the half-CU form runs on full-mantissa
queries through full-mantissa nets (tests/test_gpu_rounding.py: every product and partial sum of layer 1 rounds) and is compared
bit for bit with the CPU oracle and with the per-layer kernels.  Knob "mlp_net": 3 = the half-CU form wherever it fits;
"mlp_net_form" (read only) = the form of the handle's last one-launch projection, 0 whole-CU, 1 half-CU.
"""
import functools

import numpy as np
import pytest

import datagen
import golden_util as gu
import oracle as orc_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@functools.lru_cache(maxsize=None)
def _case(seed, d, dh, dl, nq, n=1000):
    rng = np.random.Generator(np.random.PCG64(seed))
    base = datagen.full_mantissa(rng, n, d)
    queries = datagen.full_mantissa(rng, nq, d)
    net = datagen.net_layers_full(rng, d, dh, dl)
    off, nbr = datagen.random_graph(rng, n, 4, 28)
    ent = rng.integers(0, n, size=nq).astype(np.uint32)
    return base, queries, net, off, nbr, ent


# d, d_hidden, d_low, queries: a last block of 9 of its 20 queries; whole blocks only; a padded hidden layer and d % 16 != 0;
# the last layer's four-neuron form
HALF_SHAPES = [(128, 256, 32, 2049), (128, 256, 32, 2060), (200, 72, 32, 2049), (96, 128, 64, 2051)]


@pytest.mark.parametrize("d,dh,dl,nq", HALF_SHAPES, ids=["%d_%d_%d_%d" % s for s in HALF_SHAPES])
def test_half_cu_form_bits(g, orc, d, dh, dl, nq):
    """Knob "mlp_net" = 3: q_low of a search equals the oracle's bit patterns and those of the per-layer kernels ("mlp_net" 0,
    "mlp_slab" 0) on the same handle; the profile names mlp_net_kernel, the handle reports the half-CU form."""
    base, queries, net, off, nbr, ent = _case(7100 + d, d, dh, dl, nq)
    want_q = orc.project(net, queries, threads=8)
    db_low = orc.project(net, base, threads=8)
    ix = g.Index(base, off, nbr, db_low=db_low, net=net)
    assert ix.knob_get("mlp_net_form") == -1
    got = {}
    for tag, knobs, kernel, form in (("half", {"mlp_net": 3}, "mlp_net_kernel", 1),
                                     ("layers", {"mlp_net": 0, "mlp_slab": 0}, "mlp_layer_kernels", 1)):
        for name, val in knobs.items():
            ix.knob(name, val)
        r = ix.search(queries, 40, entry_ids=ent, want=("q_low",))
        key = (d, dh, dl, nq, tag, ix.profile_read(reset=False)["project_kernel"], ix.knob_get("mlp_net_form"))
        print("half-CU projection", key)
        assert key[-2] == kernel and key[-1] == form, key   # (the per-layer kernels leave the last one-launch form in place)
        bad = int((gu.bits(r["q_low"]) != gu.bits(want_q)).sum())
        assert bad == 0, (key, bad, r["q_low"].size)
        got[tag] = r
    assert np.array_equal(gu.bits(got["half"]["q_low"]), gu.bits(got["layers"]["q_low"]))
    assert np.array_equal(got["half"]["ids"], got["layers"]["ids"])
    ix.close()


def test_batches_in_flight_take_the_half_cu_form(g, orc):
    """Three 2 049-query batches with GBNNS_FLAG_DEFER_JOIN, depth 3, default knobs: the projections run in the half-CU form
    (asserted through "mlp_net_form", not through timing); ids, hops, dist_calc and q_low equal those of plain calls, which keep the
    whole-CU form, and the oracle's."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d, dh, dl, nq, ef = 128, 256, 32, 2049, 48
    base, queries, net, off, nbr, ent = _case(7300, d, dh, dl, 3 * nq)
    db_low = orc.project(net, base, threads=8)
    want_q = orc.project(net, queries, threads=8)
    sref = orc.search_batch(orc_mod.MODE_NET, queries, base, off, nbr, ef, db_low=db_low, net=net, entries=ent, threads=8)
    ix = g.Index(t(base), off, nbr, db_low=t(db_low), net=tuple(t(x) for x in net))
    assert ix.knob_get("mlp_net") == 1
    parts = [slice(i * nq, (i + 1) * nq) for i in range(3)]
    qs, es = [t(queries[p]) for p in parts], [t(ent[p].astype(np.int32)) for p in parts]
    want = ("hops", "dist_calc", "q_low")
    plain = [ix.search(q, ef, entry_ids=e, want=want, out={}) for q, e in zip(qs, es)]
    torch.cuda.synchronize()
    assert ix.profile_read(reset=False)["project_kernel"] == "mlp_net_kernel" and ix.knob_get("mlp_net_form") == 0
    flight = [ix.search(q, ef, entry_ids=e, want=want, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for q, e in zip(qs, es)]
    ix.join()
    torch.cuda.synchronize()
    assert ix.profile_read(reset=False)["project_kernel"] == "mlp_net_kernel"
    assert ix.knob_get("mlp_net_form") == 1, "the batches in flight did not take the half-CU form"
    for p, a, b in zip(parts, plain, flight):
        for name in ("ids",) + want:
            x, y = a[name].cpu().numpy(), b[name].cpu().numpy()
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (p, name)
        assert np.array_equal(gu.bits(b["q_low"].cpu().numpy()), gu.bits(want_q[p])), p
        assert np.array_equal(b["ids"].cpu().numpy().view(np.uint32), sref["ids"][p]), p
        assert np.array_equal(b["hops"].cpu().numpy(), sref["hops"][p]), p
    ix.close()


# 256 -> 512 -> 512 -> 64: no one-launch form holds it; 128 -> 384 -> 384 -> 32: the whole-CU form does, half a CU's LDS does not
REFUSED_SHAPES = [(256, 512, 64, 2049), (128, 384, 32, 2049)]


@pytest.mark.parametrize("d,dh,dl,nq", REFUSED_SHAPES, ids=["%d_%d_%d" % s[:3] for s in REFUSED_SHAPES])
def test_nets_beyond_half_a_cu_keep_the_existing_form(g, orc, d, dh, dl, nq):
    """A net whose half-CU block needs more than 80 KB runs on what it ran on before under knob 1, in flight too, and on the same
    under knob 3 (a fallback, not an error), answered exactly; the half-CU form is never reported."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base, queries, net, off, nbr, ent = _case(7500 + d, d, dh, dl, nq, n=600)
    want_q = orc.project(net, queries, threads=8)
    db_low = orc.project(net, base, threads=8)
    ix = g.Index(t(base), off, nbr, db_low=t(db_low), net=tuple(t(x) for x in net))
    q, e = t(queries), t(ent.astype(np.int32))
    names = {}
    for knob in (1, 3):
        ix.knob("mlp_net", knob)
        for flight in (False, True):
            kw = dict(flags=g.FLAG_DEFER_JOIN, defer_depth=3) if flight else {}
            r = ix.search(q, 40, entry_ids=e, want=("q_low",), out={}, **kw)
            if flight:
                ix.join()
            torch.cuda.synchronize()
            names[(knob, flight)] = ix.profile_read(reset=False)["project_kernel"]
            key = (d, dh, dl, knob, flight, names[(knob, flight)], ix.knob_get("mlp_net_form"))
            print("beyond half a CU", key)
            assert key[-1] != 1, key
            assert np.array_equal(gu.bits(r["q_low"].cpu().numpy()), gu.bits(want_q)), key
    assert names[(3, False)] == names[(1, False)] and names[(3, True)] == names[(1, True)], names
    if dh == 384:
        assert names[(1, False)] == "mlp_net_kernel" and ix.knob_get("mlp_net_form") == 0, names
    ix.close()
