"""One table, three storage kinds (run with -m gpu).  A handle's original-space rows are float32, uint8 (Index(db=<uint8>)) or binary16
(Index(db=<float16>)); the kinds differ in storage only.  Coordinates that are integers in 0 .. 255 are exact in all three, so three
handles over the same values must answer every call alike, bit for bit: ids, distances (compared as bit patterns) and the hops / dist_calc
counters -- for a LOWQ search with its re-rank, for search_topk, and for the PLAIN walks untagged, tagged-cut and tagged-bridged (the float
handle unflagged, the byte handle with FLAG_BYTE_WALK, the half-base handle with FLAG_HALF_WALK).

d = 20: a lane per row everywhere, and the general kernel takes every flagged PLAIN call (walk_general_bwalk_kernel / walk_general_hwalk_kernel
<METRIC, TAG>, all twelve, beside the float handle's walk_general_kernel / _tag_ / _bridge_); d = 96: the half-walk fast instance; d = 128:
the byte-walk fast instance.  Both metrics.  Nothing takes a tolerance.
"""
import functools

import numpy as np
import pytest

import byte_rows_util as bu
import datagen
import half_base_util as hb
import tag_util as tg
import topk_util as tu

pytestmark = pytest.mark.gpu

N, NQ, EF, K, D_LOW = 2000, 64, 40, 10, 32
WANT = ("hops", "dist_calc", "cand", "cand_dist")


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """The shared inputs of dimension d: the table as bytes, a degree-16 graph, float low-dimensional rows and queries, original-space queries
    (a row plus a full-mantissa offset), tag words with half the rows allowed and entry points every query may see."""
    rng = tu.rng_of(11200 + d)
    base = rng.integers(0, 256, size=(N, d)).astype(np.uint8)
    off, nbr = datagen.random_graph(rng, N, 16, 16)
    queries = np.ascontiguousarray(bu.wide(base)[rng.integers(0, N, size=NQ)] + datagen.full_mantissa(rng, NQ, d))
    T, Q = tg.row_tags(N), np.full(NQ, 0x0F, np.uint32)
    ent = tg.allowed_entries(rng, T, Q, [np.arange(N)] * NQ)
    return dict(base=base, off=off, nbr=nbr, db_low=datagen.full_mantissa(rng, N, D_LOW), q_low=datagen.full_mantissa(rng, NQ, D_LOW),
                queries=queries, T=T, Q=Q, ent=ent)


def _differ(a, b, names):
    """Names of the outputs that are not bit-identical (distances compared as bytes, like everything else)."""
    return [n for n in names if np.ascontiguousarray(a[n]).tobytes() != np.ascontiguousarray(b[n]).tobytes()]


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("d", (20, 96, 128))
def test_three_kinds_answer_alike(g, d, metric):
    c = _inputs(d)
    half = c["base"].astype(np.float16)
    assert np.array_equal(hb.wide(half), bu.wide(c["base"]))   # exact in all three kinds
    handles = [(g.Index(bu.wide(c["base"]), c["off"], c["nbr"], db_low=c["db_low"], metric=metric), 0, "float"),
               (g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric), g.FLAG_BYTE_WALK, "byte"),
               (g.Index(half, c["off"], c["nbr"], db_low=c["db_low"], metric=metric), g.FLAG_HALF_WALK, "half")]
    assert [(ix.is_bytes, ix.is_half_base) for ix, _, _ in handles] == [(False, False), (True, False), (False, True)]
    for ix, _, _ in handles:
        ix.set_tags(c["T"])
        ix.profile_enable(True)
    failures = []

    def alike(what, names, call, general=False):
        got = []
        for ix, flag, kind in handles:
            ix.profile_read(reset=True)
            got.append(call(ix, flag))
            first = ix.profile_read(reset=True)["walk_kernel"].split(" (")[0]
            print("row kinds: d", d, "metric", metric, what, kind, first)
            if general and flag and first != "walk_general_kernel":
                failures.append((what, kind, "first pass %s, not the general kernel" % first))
        for r, (_, _, kind) in zip(got[1:], handles[1:]):
            if _differ(r, got[0], names):
                failures.append((what, kind, "differs from the float handle in %s" % _differ(r, got[0], names)))

    lowq = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT)
    alike("LOWQ", ("ids",) + WANT, lambda ix, flag: ix.search(c["queries"], EF, **lowq))
    alike("search_topk", ("ids", "top_ids", "top_dist") + WANT, lambda ix, flag: ix.search(c["queries"], EF, top_k=K, **lowq))
    plain = dict(mode=g.MODE_PLAIN, k=K, entry_ids=c["ent"], want=WANT)
    for fast in ((1, 0) if d == 20 else (1,)):   # the handle knob half_walk_fast = 0: the general instance by the knob as well
        handles[2][0].knob("half_walk_fast", fast)
        what = "PLAIN" if fast else "PLAIN, half_walk_fast 0"
        alike(what, ("ids",) + WANT, lambda ix, flag: ix.search(c["queries"], EF, flags=flag, **plain), general=d == 20)
        alike(what + " tagged, cut", ("ids",) + WANT, lambda ix, flag: ix.search(c["queries"], EF, flags=flag, query_tags=c["Q"], **plain), general=d == 20)
        alike(what + " tagged, bridged", ("ids",) + WANT,
              lambda ix, flag: ix.search(c["queries"], EF, flags=flag | g.FLAG_TAG_BRIDGE, query_tags=c["Q"], **plain), general=d == 20)
    for ix, _, _ in handles:
        ix.close()
    assert not failures, failures
