"""GPU parity of the one-launch projection with its weights streamed to LDS by DMA (run with -m gpu on an MI355X).

mlp_net_kernel (csrc/mlp_net.hip) reads its weights from a staged-order image the index builds once (csrc/handle.cpp
pack_net_image): a wavefront's chunk goes from memory into its staging buffer by LDS-DMA, 1 KiB per instruction, one chunk ahead of
the arithmetic.  A chunk read before it has landed, a piece in the wrong place or a slice of the wrong wavefront changes results;
the arithmetic is untouched, so q_low must equal the CPU oracle's and the per-layer kernels' bit patterns, in both forms of the
kernel (whole-CU: plain calls; half-CU: knob "mlp_net" 3, and batches in flight), on full-mantissa queries through full-mantissa
nets.  Shapes: the smallest that reach every branch of the image -- a partial last block (2 048 is the least batch the kernel
serves), whole blocks only, a hidden layer that is no multiple of a slice with d % 16 != 0 (clamped rows, zero tails, a wavefront
without a slice), and the last layer's four-neuron form.
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


_REF = {}


def _reference(orc, key, net, base, queries):
    """The oracle's projections of a case, computed once and shared (read only)."""
    if key not in _REF:
        want_q, db_low = orc.project(net, queries, threads=8), orc.project(net, base, threads=8)
        want_q.setflags(write=False)
        db_low.setflags(write=False)
        _REF[key] = (want_q, db_low)
    return _REF[key]


DMA_SHAPES = [(128, 256, 32, 2049), (128, 256, 32, 2060), (200, 72, 32, 2049), (96, 128, 64, 2051)]


@pytest.mark.parametrize("d,dh,dl,nq", DMA_SHAPES, ids=["%d_%d_%d_%d" % s for s in DMA_SHAPES])
def test_both_forms_bits(g, orc, d, dh, dl, nq):
    """q_low of a search in the half-CU form (knob "mlp_net" 3) and in the whole-CU form (plain calls, the default knob) equals the
    oracle's bit patterns and those of the per-layer kernels ("mlp_net" 0, "mlp_slab" 0) on the same handle; ids are equal; the
    profile names mlp_net_kernel and the handle reports the form."""
    base, queries, net, off, nbr, ent = _case(8100 + d, d, dh, dl, nq)
    want_q, db_low = _reference(orc, (d, dh, dl, nq), net, base, queries)
    ix = g.Index(base, off, nbr, db_low=db_low, net=net)
    got = {}
    for tag, knobs, kernel, form in (("half", {"mlp_net": 3}, "mlp_net_kernel", 1),
                                     ("whole", {"mlp_net": 1}, "mlp_net_kernel", 0),
                                     ("layers", {"mlp_net": 0, "mlp_slab": 0}, "mlp_layer_kernels", 0)):
        for name, val in knobs.items():
            ix.knob(name, val)
        r = ix.search(queries, 40, entry_ids=ent, want=("q_low",))
        key = (d, dh, dl, nq, tag, ix.profile_read(reset=False)["project_kernel"], ix.knob_get("mlp_net_form"))
        bad = int((gu.bits(r["q_low"]) != gu.bits(want_q)).sum())
        print("DMA projection", key, "words that differ from the oracle's:", bad, "of", r["q_low"].size)
        assert key[-2] == kernel and key[-1] == form, key   # (the per-layer kernels leave the last one-launch form in place)
        assert bad == 0, (key, bad, r["q_low"].size)
        got[tag] = r
    for tag in ("half", "whole"):
        assert np.array_equal(gu.bits(got[tag]["q_low"]), gu.bits(got["layers"]["q_low"])), tag
        assert np.array_equal(got[tag]["ids"], got["layers"]["ids"]), tag
    ix.close()


def test_three_batches_in_flight(g, orc):
    """Three 2 049-query batches with GBNNS_FLAG_DEFER_JOIN, depth 3: their projections run in the half-CU form beside the other
    batches' walks; ids, hops, dist_calc and q_low equal those of plain calls (whole-CU form) and the oracle's."""
    import torch
    dev = torch.device("cuda:0")
    # (a copy: the shared reference arrays are read only.  The copies stay alive to the end of the test: a pageable array that is freed at
    # once hands its addresses to the next copy of the same size, and a plain copy from pageable memory leaves the runtime a page-locked
    # mapping of those addresses -- the stale-mapping fault handle.cpp describes at h2d_staged, met here in the three query copies below)
    held = []
    t = lambda a: (held.append(np.array(a)), torch.from_numpy(held[-1]).to(dev))[1]
    d, dh, dl, nq, ef = 128, 256, 32, 2049, 48
    base, queries, net, off, nbr, ent = _case(8300, d, dh, dl, 3 * nq)
    want_q, db_low = _reference(orc, ("flight", d, dh, dl, 3 * nq), net, base, queries)
    sref = orc.search_batch(orc_mod.MODE_NET, queries, base, off, nbr, ef, db_low=db_low, net=net, entries=ent, threads=8)
    ix = g.Index(t(base), off, nbr, db_low=t(db_low), net=tuple(t(x) for x in net))
    parts = [slice(i * nq, (i + 1) * nq) for i in range(3)]
    qs, es = [t(queries[p]) for p in parts], [t(ent[p].astype(np.int32)) for p in parts]
    want = ("hops", "dist_calc", "q_low")
    plain = [ix.search(q, ef, entry_ids=e, want=want, out={}) for q, e in zip(qs, es)]
    torch.cuda.synchronize()
    assert ix.profile_read(reset=False)["project_kernel"] == "mlp_net_kernel" and ix.knob_get("mlp_net_form") == 0
    flight = [ix.search(q, ef, entry_ids=e, want=want, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for q, e in zip(qs, es)]
    ix.join()
    torch.cuda.synchronize()
    assert ix.profile_read(reset=False)["project_kernel"] == "mlp_net_kernel" and ix.knob_get("mlp_net_form") == 1
    for p, a, b in zip(parts, plain, flight):
        for name in ("ids",) + want:
            x, y = a[name].cpu().numpy(), b[name].cpu().numpy()
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (p, name)
        for r in (a, b):
            assert np.array_equal(gu.bits(r["q_low"].cpu().numpy()), gu.bits(want_q[p])), p
            assert np.array_equal(r["ids"].cpu().numpy().view(np.uint32), sref["ids"][p]), p
            assert np.array_equal(r["hops"].cpu().numpy(), sref["hops"][p]), p
            assert np.array_equal(r["dist_calc"].cpu().numpy() + ef, sref["dist_calc"][p]), p   # (the oracle counts the re-rank's ef too)
    ix.close()
