"""The census of the walk kernel instances on the device (run with -m gpu on an MI355X): every case of tests/walk_instances.py -- which
tests/test_cabi_cpu.py proves to cover all 210 instances of the first, the bitmap and the retry pass -- runs bit-exact against the CPU
oracle on full-mantissa data (a wrong summation order changes distance bits), and the library's profile must name exactly the planned
instances: gbnns_profile.walk_kernel EQUALS the case's `first`, full template tail included, and for a case with a small visited set
gbnns_profile.retry_kernel equals its `retry`, with the retry instance itself finishing at least half the batch (a retry kernel that
hands everything on to the always-exact general kernel would pass every result comparison).

One test per (metric, walked dimension); the vectors, graphs and oracle walks of a set are computed once and shared by its cases, one
Index per graph.  Searches are MODE_LOWQ over independent low-dimensional rows with a 40-dimensional original space, so every instance
that re-ranks its own query does; each set adds one MODE_PLAIN walk over the original space.  Nothing takes a tolerance.
"""
import ctypes

import numpy as np
import pytest

import golden_util as gu
import locality_order_util as lo
import walk_instances as wi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


WANT = ("hops", "dist_calc", "cand", "cand_dist")


def _search(g, ix, v, case, hash_capacity):
    """One profiled LOWQ search of the case -> (results, profile of that call)."""
    for name, val in case.knobs.items():
        ix.knob(name, val)
    kw = dict(aux=True, llf=True, hops_bound=50) if case.aux else {}
    ix.profile_read(reset=True)
    r = ix.search(v["queries"], case.ef, mode=g.MODE_LOWQ, queries_low=v["q_low"], entry_ids=v["ent"], want=WANT, flags=case.flags,
                  hash_capacity=hash_capacity, **kw)
    return r, ix.profile_read(reset=True)


def _against_walk(r, w, what):
    """Names of the outputs of r that differ from the oracle walk w (candidate ids in pop order, distance bit patterns, hops, dist_calc)."""
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append(what + " candidate ids")
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append(what + " distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append(what + " hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append(what + " dist_calc")
    return bad


@pytest.mark.parametrize("metric,dim", wi.SETS, ids=["m%d_d%d" % s for s in wi.SETS])
def test_every_walk_instance_bit_exact_and_by_name(g, orc, metric, dim):
    """Every case of the set: candidate ids in pop order, their distance bit patterns, hops and dist_calc equal the oracle's walk, the
    answers equal getRealNearest over that walk, and walk_kernel (less its " (...)" suffix) equals the planned name.  A case with
    hash_capacity 128 also: retry_kernel equals the planned retry name, retry_queries - retry_general_queries >= nq / 2 (by
    test_walk_instance_retry_cases_outgrow_their_visited_set the first pass hands over at least 3 / 4 of the batch, and the retry
    pass's visited set -- a CU's whole LDS -- holds more entries than the index has rows), and every output equals the same case's at
    hash_capacity 0.  Mismatches are collected over the set, so one run names every failing case.
    Every case then runs once more with its batch walked in locality order (knob "order_min" = 1; 12 key bits, the first case of each
    index at 10 and 16 too): the whole batch is ordered, the permutation read back from the handle is a valid order of the walked-space
    queries, the same kernels are named and every output equals the unordered run's byte for byte; a retry case hands over at least 3 / 4
    of the batch again.  tests/test_locality_order_cpu.py proves that the sort moves nearly every work item of these batches."""
    cases = [c for c in wi.CASES if (c.metric, c.dim) == (metric, dim)]
    failures, ran, ordered = [], 0, 0
    plain_done = False
    for key in sorted({c.graph_key for c in cases}):
        group = [c for c in cases if c.graph_key == key]
        n, deg = key[2], key[3]
        v = wi.vectors(metric, dim, n)
        off, nbr = wi.graph(*key)
        ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=metric)
        if any(c.aux for c in group):
            ix.set_aux_graph(*wi.aux_graph(metric, dim, n))
        ix.profile_enable(True)
        for c in group:
            w, want = wi.oracle_walk(orc, c)
            r, p = _search(g, ix, v, c, c.hash_capacity)
            ran += 1
            bad = _against_walk(r, w, "")
            if not np.array_equal(r["ids"], want):
                bad.append("answers (%d differ)" % int((r["ids"] != want).sum()))
            launched = p["walk_kernel"].split(" (")[0]
            if launched != c.first:
                bad.append("first pass launched %s" % launched)
            if c.hash_capacity:
                finished = int(p["retry_queries"]) - int(p["retry_general_queries"])
                print("retry", tuple(c[:11]), p["retry_kernel"], "handed over", p["retry_queries"], "to the general kernel", p["retry_general_queries"])
                if p["retry_kernel"] != c.retry:
                    bad.append("retry pass launched '%s'" % p["retry_kernel"])
                if 2 * finished < wi.NQ:
                    bad.append("retry pass finished %d of %d handed over (%d queries)" % (finished, p["retry_queries"], wi.NQ))
                # (the same case with the library's own capacity; no name is asserted there: a non-compact table for ef >= 1 024 does not
                # fit the LDS, and the general kernel takes that batch)
                r0, _ = _search(g, ix, v, c, 0)
                for name in ("ids",) + WANT:
                    if r[name].tobytes() != r0[name].tobytes():
                        bad.append("%s differs from hash_capacity 0" % name)
            elif p["retry_queries"] < p["retry_general_queries"]:
                bad.append("counts: %d handed over, %d to the general kernel" % (p["retry_queries"], p["retry_general_queries"]))
            for bits in (lo.BITS if c is group[0] else (12,)):
                (ro, po), in_order = lo.in_order(ix, v["q_low"], lambda: _search(g, ix, v, c, c.hash_capacity), bits)
                ordered += 1
                in_order += lo.same_bytes(ro, r, ("ids",) + WANT)
                in_order += lo.same_kernels(po, p, c.hash_capacity != 0)
                if c.hash_capacity and 4 * int(po["retry_queries"]) < 3 * wi.NQ:
                    in_order.append("first pass handed over %d of %d" % (po["retry_queries"], wi.NQ))
                bad += ["in order, %d bits: %s" % (bits, b) for b in in_order]
            if bad:
                failures.append((tuple(c), bad))
        if not plain_done and n == 3000:
            # one PLAIN walk (the graph walked in the 40-dimensional original space, k = ef) on the run-time-length two-list instance
            plain_done = True
            ef = 200
            name, lds = ctypes.create_string_buffer(128), ctypes.c_uint64()
            assert g.load_library().gbnns_debug_walk_plan(metric, wi.D_ORIG, wi.D_ORIG, n, wi.ELL_STRIDE[deg], 0, ef, 1, 0, 0, 0, 0, 0, 0, name, 128,
                                                          ctypes.byref(lds)) == 0
            assert name.value.decode().startswith("walk_reg_big_kernel<%d, 0, true, false, false, " % metric), name.value
            for kn, val in (("coop", 0), ("late_rows", 0), ("spec_min_nq", 0), ("spec_any_form", 0), ("spec_tail", 0)):
                ix.knob(kn, val)
            w = orc.walk(v["queries"], v["base"], off, nbr, ef, entries=v["ent"], metric=metric, threads=8)
            ix.profile_read(reset=True)
            r = ix.search(v["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=v["ent"], want=WANT)
            launched = ix.profile_read(reset=True)["walk_kernel"].split(" (")[0]
            bad = _against_walk(r, w, "PLAIN")
            if launched != name.value.decode():
                bad.append("PLAIN first pass launched %s, planned %s" % (launched, name.value.decode()))
            if bad:
                failures.append((("PLAIN", metric, dim, deg, ef), bad))
        ix.close()
    print("census", (metric, dim), "cases", ran, "ordered runs", ordered, "failures", len(failures))
    assert plain_done and ran == len(cases) and ordered == ran + 2 * len({c.graph_key for c in cases})
    assert not failures, failures


def test_profile_read_keeps_serving_the_192_byte_layout(g):
    """gbnns_profile grew at its end (retry_kernel, retry_queries, retry_general_queries): a caller built against the 192-byte layout says so
    in struct_size and gets that prefix -- walk_kernel included -- with nothing written behind it; a current caller gets all 304 bytes."""
    from gbnns_dim_red_amd import binding
    c = next(c for c in wi.CASES if c.hash_capacity and c.metric == 0 and c.dim == 32 and c.ef == 64 and not (c.wide or c.aux))
    v = wi.vectors(c.metric, c.dim, c.n)
    off, nbr = wi.graph(*c.graph_key)
    ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=c.metric)
    ix.profile_enable(True)
    for name, val in c.knobs.items():
        ix.knob(name, val)
    ix.search(v["queries"], c.ef, mode=g.MODE_LOWQ, queries_low=v["q_low"], entry_ids=v["ent"], hash_capacity=c.hash_capacity)
    buf = (ctypes.c_ubyte * ctypes.sizeof(binding.Profile))(*([0xA5] * ctypes.sizeof(binding.Profile)))
    old = ctypes.cast(buf, ctypes.POINTER(binding.Profile))
    old.contents.struct_size = 192
    assert ix._lib.gbnns_profile_read(ix._h, old, 0) == 0
    assert old.contents.struct_size == 192 and old.contents.calls == 1 and old.contents.walk_kernel.decode().split(" (")[0] == c.first
    assert bytes(buf[192:]) == b"\xa5" * (ctypes.sizeof(binding.Profile) - 192)
    p = ix.profile_read(reset=True)
    assert ctypes.sizeof(binding.Profile) == 304 and p["walk_kernel"].split(" (")[0] == c.first and p["retry_kernel"] == c.retry
    assert p["retry_queries"] >= 3 * wi.NQ // 4 and p["retry_general_queries"] <= p["retry_queries"]
    # a call that hands nothing over names no retry kernel it did not launch, and a reset clears the fields
    assert ix.profile_read(reset=True)["retry_kernel"] == "" and ix.profile_read()["retry_queries"] == 0
    ix.close()
