"""GBNNS_FLAG_TAG_BRIDGE without a device: the exports, the plan of a bridged call, bridge_graph (the NumPy definition of G'') against a
plain-loop restatement, and the hand-built fixtures of tests/test_gpu_bridge.py.
"""
import os
import re

import numpy as np
import pytest

import bridge_util as bu
import datagen
import tag_util as tg
import topk_util as tu


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports_and_the_flag_constant(g):
    from gbnns_dim_red_amd import binding
    assert "gbnns_debug_bridge_plan" in binding.SYMBOLS and hasattr(g.load_library(), "gbnns_debug_bridge_plan")
    assert callable(g.bridge_graph) and callable(g.bridge_plan)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gbnns.h")).read()
    m = re.search(r"#define\s+GBNNS_FLAG_TAG_BRIDGE\s+(\d+)u", header)
    assert m and int(m.group(1)) == g.FLAG_TAG_BRIDGE == 1024
    flags = [getattr(g, n) for n in dir(g) if n.startswith("FLAG_")]
    assert len(set(flags)) == len(flags)   # a bit of its own


def _random_case(rng, n):
    """A CSR graph over n nodes with the cases the definition has to get right, and a mask that allows about a third of the rows."""
    off, nbr = datagen.random_graph(rng, n, 0, 12)
    lists = [list(nbr[int(off[i]):int(off[i + 1])]) for i in range(n)]
    allowed = rng.random(n) < 0.35
    banned, ok = np.flatnonzero(~allowed), np.flatnonzero(allowed)
    lists[int(ok[0])] = []                                            # an empty row
    lists[int(ok[1])] = [int(x) for x in banned[:5]]                  # a row whose neighbours are all disallowed
    lists[int(banned[0])] = [int(ok[2]), int(banned[3]), int(ok[3])]  # ... and the row of one of them: it contains u = ok[2] below
    lists[int(ok[2])] = [int(ok[4]), int(banned[0]), int(ok[5])]      # a disallowed neighbour whose row contains u
    lists[int(banned[1])] = lists[int(banned[2])] = [int(x) for x in ok[6:10]]   # two disallowed neighbours with identical rows ...
    lists[int(ok[3])] = [int(banned[1]), int(banned[2]), int(ok[6])]             # ... side by side in one row
    new_off = np.zeros(n + 1, np.uint64)
    new_off[1:] = np.cumsum([len(x) for x in lists])
    return new_off, np.array([x for row in lists for x in row], np.uint32), allowed, ok, banned


@pytest.mark.parametrize("n", [64, 257, 2048])
def test_bridge_graph_is_the_plain_loop(g, n):
    rng = tu.rng_of(9800 + n)
    off, nbr, allowed, ok, banned = _random_case(rng, n)
    o2, n2 = g.bridge_graph(off, nbr, allowed)
    o3, n3 = bu.bridge_graph_loops(off, nbr, allowed)
    assert o2.dtype == np.uint64 and n2.dtype == np.uint32 and len(o2) == n + 1 and o2[0] == 0 and o2[-1] == len(n2)
    assert np.array_equal(o2, o3) and np.array_equal(n2, n3)
    assert allowed[n2].all()
    row = lambda u: list(n2[int(o2[u]):int(o2[u + 1])])
    assert row(ok[0]) == []
    assert row(ok[2]) == [ok[4], ok[2], ok[3], ok[5]]                   # u itself, through banned[0]; banned[3] is not looked through
    assert row(ok[3]) == list(ok[6:10]) + list(ok[6:10]) + [ok[6]]      # a plain concatenation: repeated ids stay
    assert set(row(ok[1])) <= set(ok)


def test_bridge_graph_all_and_none_allowed(g):
    rng = tu.rng_of(9801)
    off, nbr, _, _, _ = _random_case(rng, 512)
    o2, n2 = g.bridge_graph(off, nbr, np.ones(512, bool))
    assert np.array_equal(o2, off) and np.array_equal(n2, nbr)
    o2, n2 = g.bridge_graph(off, nbr, np.zeros(512, bool))
    assert not o2.any() and len(o2) == 513 and len(n2) == 0 and n2.dtype == np.uint32
    o2, n2 = g.bridge_graph(np.zeros(5, np.uint64), np.zeros(0, np.uint32), np.ones(4, bool))   # a graph without edges
    assert not o2.any() and len(n2) == 0
    with pytest.raises(ValueError):
        g.bridge_graph(off, nbr, np.ones(511, bool))


@pytest.mark.parametrize("stride", [32, 48])
def test_bridge_plan_names_a_bridge_instance_inside_the_domain(g, stride):
    for metric, dlow in tg.TWO_PASS_SHAPES:
        for ef in tg.BEAMS + (128, 129):
            name, lds = g.bridge_plan(metric, dlow, tg.N, stride, ef, with_lds=True)
            assert name == bu.bridge_kernel(metric, dlow, ef), (metric, dlow, ef, name)
            if name.startswith("walk_bridge_kernel"):
                import ctypes as C
                tname, tlds = C.create_string_buffer(128), C.c_uint64(0)
                assert g.load_library().gbnns_debug_tag_plan(metric, dlow, dlow, tg.N, stride, 0, ef, 1, 0, 0, tname, 128, C.byref(tlds)) == 0
                assert tname.value.decode().startswith("walk_reg_tag_kernel") and lds >= tlds.value + 4 * 32, (name, lds, tlds.value)


def test_bridge_plan_outside_the_domain_is_the_general_kernel(g):
    for ef in (8, 64, 100, 200):
        assert g.bridge_plan(0, 32, tg.N, 32, ef, aux_stride=16) == "walk_general_kernel"
        assert g.bridge_plan(0, 32, tg.N, 32, ef, n_entries=2) == "walk_general_kernel"
        assert g.bridge_plan(0, 32, tg.N, 32, ef, wide=True) == "walk_general_kernel"
    assert g.bridge_plan(0, 32, tg.N, 32, 1100) == "walk_general_kernel"
    assert g.bridge_plan(1, 48, tg.N, 32, 64) == "walk_general_kernel"
    assert g.bridge_plan(0, 30, tg.N, 32, 64) == "walk_general_kernel"
    assert g.bridge_plan(0, 32, 1 << 24, 32, 64) == "walk_general_kernel"
    with pytest.raises(g.GbnnsError):
        g.bridge_plan(0, 32, tg.N, 33, 64)
    # the plan of a tagged call without the flag is what it was
    assert g.tag_plan(0, 32, tg.N, 32, 64) == tg.tag_kernel(0, 32, 64, True) and g.tag_plan(0, 32, tg.N, 32, 200) == tg.tag_kernel(0, 32, 200, True)


def test_hand_built_fixtures(g, orc):
    """(a) / (d): the parity graph -- the cut walk returns the entry alone, the bridged walk goes on, and looked-through rows contain u.
    (b): the twin rows put every looked-through id twice into one chunk."""
    c = bu.parity()
    off, nbr = c["off"].astype(np.int64), c["nbr"]
    assert (np.diff(off) == 16).all() and ((nbr.reshape(tg.N, 16) % 2) != (np.arange(tg.N)[:, None] % 2)).all()
    back = sum(1 for u in range(0, tg.N, 2) for v in nbr[off[u]:off[u + 1]] if u in nbr[off[v]:off[v + 1]])
    assert back >= tg.N   # a looked-through row that contains u: about eight per even row
    cut = tg.expected(orc, c, 8, 0)
    assert (cut["count"] == 1).all() and (cut["ids"][:, 0] == c["ent"]).all()
    w = bu.expected(orc, c, 8, 0)
    assert (w["hops"] > 1).all() and (w["count"] == 8).all() and (w["ids"] % 2 == 0).all()
    c = bu.twins()
    o2, n2 = g.bridge_graph(c["off"], c["nbr"], (c["T"] & 1) != 0)
    assert (np.diff(o2.astype(np.int64))[::2] == 32).all()
    for u in range(0, tg.N, 2):
        r = n2[int(o2[u]):int(o2[u + 1])]
        assert np.array_equal(r[4:16], r[16:28]) and len(set(r[4:16].tolist())) == 12, u
