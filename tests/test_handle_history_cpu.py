"""The decks of tests/handle_history.py without a device: the call sequence of every deck is an Eulerian circuit of the complete directed
graph on its cards, the surprise cards are surprises by their inputs, the decks do not collapse onto one kernel, buffers are reused both
larger and smaller than needed, and a stale tag table would show.
"""
import collections

import numpy as np
import pytest

import handle_history as hh


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


@pytest.mark.parametrize("name", hh.DECKS)
def test_the_sequence_is_an_eulerian_circuit(name):
    """F * F + 1 calls that start and end at the same card; every ordered pair of cards, a card with itself included, is adjacent exactly
    once (by counting); the per-call view names each call's predecessor; the replay covers the last 2 F calls at least."""
    d = hh.deck(name)
    F, seq = d.F, d.circuit
    assert len(seq) == F * F + 1 and seq[0] == seq[-1] and set(seq) == set(range(F))
    pairs = collections.Counter(zip(seq, seq[1:]))
    assert len(pairs) == F * F and set(pairs.values()) == {1}
    assert all(sum(1 for c in seq[:-1] if c == i) == F for i in range(F))          # every card is called F times (the start once more)
    calls = d.calls()
    assert calls[0][1] is None and all(prev is d.cards[seq[i - 1]] and card is d.cards[seq[i]] for i, prev, card in calls[1:])
    assert 0 < d.replay_from <= len(seq) - 2 * F
    assert hh.deck(name) is d and hh.build_circuit(F, d.seed, **d.circuit_shape())[0] == seq   # deterministic


def test_float_deck_lists_every_family():
    d = hh.deck("float")
    c = {x.name: x for x in d.cards}
    F = hh
    lowq = lambda ef, **kw: [x for x in d.cards if x.kind == "search" and x.mode == F.MODE_LOWQ and x.ef == ef and x.tags is None and
                             all(getattr(x, k) == v for k, v in kw.items())]
    for ef in (8, 64, 200):
        assert any(x.hc == 0 and x.flags == 0 and not x.knobs for x in lowq(ef)), ef
    assert lowq(64, hc=128) and lowq(200, hc=128) and lowq(64, flags=F.FLAG_WIDE_INDEX) and lowq(128, flags=F.FLAG_BITMAP_PASS) and lowq(1100)
    assert any(x.knobs.get("coop") == 1 for x in lowq(200)) and any(x.aux for x in d.cards) and any(x.n_entries == 3 for x in d.cards)
    assert any(x.mode == F.MODE_PLAIN and x.ef == 200 for x in d.cards)
    assert any(x.mode == F.MODE_NET and x.ef == 64 and "q_low" in x.want for x in d.cards)
    assert any(x.mode == F.MODE_NET and x.flags & F.FLAG_NO_FUSED_RERANK for x in d.cards)
    assert any(x.kind == "search" and x.top_k == 10 and not x.defer for x in d.cards)
    assert c["tag64"].ef == 64 and c["tag200"].ef == 200 and len(np.unique(d.data["words"]["tag"][:96])) == 3
    assert c["bridge64"].flags & F.FLAG_TAG_BRIDGE
    assert sorted(bool(x.flags & F.FLAG_SCAN_GATHER) for x in d.cards if x.kind == "auto") == [False, True]
    assert sorted(x.gather for x in d.cards if x.kind == "knn") == [False, True] and any(x.kind == "census" for x in d.cards)
    assert {"rerank", "rerank_topk", "project", "refuse", "swap"} <= {x.kind for x in d.cards} and c["project_300"].nq == 300
    assert any(x.half and x.ef == 64 for x in d.cards) and any(x.knobs.get("order_min") == 1 and x.ef == 64 for x in d.cards)
    deferred = [x for x in d.cards if x.defer]
    assert sorted(x.mem for x in deferred) == ["device", "pinned"] and any(x.top_k for x in deferred if x.mem == "pinned")
    assert {x.mem for x in d.cards} == {"numpy", "pinned", "device"}
    lo_, hi_ = d.SWAP
    assert 0 < lo_ < d.N_A < hi_ < d.data["n"]   # a partial range over both parts
    # both routes of the routed call, under either table
    from gbnns_dim_red_amd import tag_census
    for table in "AB":
        for card in (x for x in d.cards if x.kind == "auto"):
            allowed, _ = tag_census(d.data["T"][table], d.data["words"]["auto"][:card.nq])
            scan = allowed <= hh.SCAN_BELOW
            assert scan.any() and (~scan).any() and (allowed[scan] > 0).any(), (table, card)


def test_float_circuit_makes_every_surprise_key_calm_first_and_replays_from_the_surprises():
    """What the existence checks of the device test stand on.  Every card that feeds the sizing statistics of a surprise key, the
    surprise cards apart, enters in the sparse part; the circuit opens with the circuit of the non-deferred ones alone, so each key has
    seen every calm batch at least CALM_AFTER + 2 times (a longest walk seen for the first time restarts the streak; then CALM_AFTER
    calm ones) before its first surprise.  The replay on a fresh handle starts with calm card, surprise twin of each key in turn: the key
    has seen one short batch (its table is sized for that) and is not calm, so the retry pass is launched and takes the hand-overs.  The
    deferred cards form one run, so three of their batches are outstanding at once."""
    d = hh.deck("float")
    seq = d.circuit
    surprise = [c for c in d.cards if c.twin]
    keys = {c.skey for c in surprise}
    assert len(keys) == len(surprise) == 4
    for c in d.cards:
        if c.feeds_sizing and c.skey in keys and not c.twin:
            assert c.calm_side and c.ent == "a", c
    for s in surprise:
        first = next(i for i, x in enumerate(seq) if d.cards[x] is s)
        before = collections.Counter(d.cards[x].name for x in seq[:first] if d.cards[x].skey == s.skey and d.cards[x].feeds_sizing and not d.cards[x].defer)
        calm_cards = [c for c in d.cards if c.skey == s.skey and c.feeds_sizing and not c.twin and not c.defer]
        assert calm_cards and all(before[c.name] >= hh.CALM_AFTER + 2 for c in calm_cards), (s, before)
    want = [x for s in surprise for x in (d.index[s.twin], d.index[s.name])]
    assert seq[d.replay_from:d.replay_from + len(want) + 1] == want + want[:1]
    runs, run = [], 0
    for x in seq:
        run = run + 1 if d.cards[x].defer else 0
        runs.append(run)
    assert max(runs) >= 3


def test_surprise_cards_are_surprises_by_their_inputs(orc):
    """Same ef, mode, flags, auxiliary graph, wide index and knobs as the calm twin (the same sizing key: the knob "hot" is touched by no
    card), and the oracle's longest walk of the surprise batch computes more than 3 times the distances of the calm twin's longest."""
    d = hh.deck("float")
    for s in (c for c in d.cards if c.twin):
        t = d.cards[d.index[s.twin]]
        assert (s.ef, s.mode, s.flags, s.aux, s.hc, s.knobs, s.skey, s.nq, s.table) == (t.ef, t.mode, t.flags, t.aux, 0, t.knobs, t.skey, t.nq, t.table)
        assert t.ent == "a" and s.ent == "b" and (d.data["ent"]["a"] < d.N_A).all() and (d.data["ent"]["b"] >= d.N_A).all()
        calm, long = d.dist_calc_max(orc, t), d.dist_calc_max(orc, s)
        print(s.name, "longest walk", long, "calm twin", calm)
        assert long > 3 * calm, (s, long, calm)
    assert not any("hot" in c.knobs for c in d.cards) and "hot" not in hh.KNOBS
    off = d.data["off"].astype(np.int64)
    nbr = d.data["nbr"]
    assert (nbr[:off[d.N_A]] < d.N_A).all() and (nbr[off[d.N_A]:] >= d.N_A).all()   # no edge between the parts


def test_plan_names_cover_the_kernel_families(g):
    """The first-pass names the plan functions give for the decks' cards: a later edit cannot quietly collapse a deck onto one kernel."""
    names = {}
    for deck in ("float", "bytes"):
        d = hh.deck(deck)
        names[deck] = {c.name: d.planned(g, c) for c in d.cards if c.kind == "search"}
        print(deck, names[deck])
    f, b = names["float"], names["bytes"]
    assert f["lowq64"] == f["lowq8_300"] == "walk_hot_kernel" and f["lowq200"] == "walk_hot_big_kernel"
    assert f["surprise_lowq64"] == f["lowq64"] and f["surprise_lowq200"] == f["lowq200"] and f["surprise_plain200"] == f["plain200"]
    assert f["plain200"].startswith("walk_reg_big_kernel<") and f["wide64"].startswith("walk_reg_kernel<")     # two-list / register-list instances
    assert f["coop200"].startswith("walk_coop_kernel<") and f["bitmap128"].startswith("walk_bitmap_") and f["lowq1100"].startswith("walk_fast_kernel<")
    assert f["tag64"].startswith("walk_reg_tag_kernel<") and f["tag200"].startswith("walk_reg_big_tag_kernel<")
    assert f["bridge64"].startswith("walk_bridge_kernel<")
    # (the half-row cards: no plan function takes FLAG_HALF_ROWS, their name is half_rows_util's and only the device run can hold it
    # against a launch; here: the twin shares it, and it is none of the float instances)
    assert f["surprise_half64"] == f["half64"] and f["half64"] not in {n for k, n in f.items() if "half" not in k}
    bd = hh.deck("bytes")
    assert g.byte_plan(0, hh.D_LOW, bd.data["n"], bd.stride, 64) == (b["fused64"], True) and b["fused64"] != f["lowq64"]   # a fused byte instance
    assert b["byte_walk64"] not in ("walk_general_kernel", b["fused64"]) and b["byte_walk64_u8"].startswith("beam_u8_")
    assert b["tag64"] != "walk_general_kernel" and b["bridge64"] != "walk_general_kernel"
    assert len(set(f.values())) >= 12 and len(set(b.values())) >= 5


@pytest.mark.parametrize("name", hh.DECKS)
def test_buffers_are_reused_larger_and_smaller(name):
    """At least three batch sizes per deck; in every group of families that share lane buffers there is a card of 300 and one of 33
    queries, and the circuit holds both the shrink 300 -> 33 and the growth 33 -> 300 for every such pair; the first call of 300 queries comes
    after smaller ones, so the buffers regrow in mid-sequence."""
    d = hh.deck(name)
    assert len({c.nq for c in d.cards}) >= 3
    pairs = set(zip(d.circuit, d.circuit[1:]))
    groups = {b for c in d.cards for b in c.buffers}
    assert "search" in groups and (name == "ties" or "census" in groups) and (name != "float" or "order" in groups)
    for grp in groups:
        big = [i for i, c in enumerate(d.cards) if grp in c.buffers and c.nq == 300]
        small = [i for i, c in enumerate(d.cards) if grp in c.buffers and c.nq == 33]
        assert big and small, grp
        assert all((x, y) in pairs and (y, x) in pairs for x in big for y in small), grp
        first_big = next(i for i, x in enumerate(d.circuit) if x in big)
        assert any(grp in d.cards[x].buffers and d.cards[x].nq < 300 for x in d.circuit[:first_big]), grp


def test_a_stale_tag_table_would_show(orc):
    """Every tag-dependent card of the float deck: its expectation under table A differs from that under table B in at least half of its
    answer rows; the swap card toggles between them, and both tables are in force for about half of the calls."""
    d = hh.deck("float")
    dep = [c for c in d.cards if c.tagdep]
    assert len(dep) >= 8
    for c in dep:
        a, b = d.expect(orc, c, "A"), d.expect(orc, c, "B")
        key = "ids" if "ids" in a else "knn_ids" if "knn_ids" in a else "allowed"
        differ = (a[key].reshape(c.nq, -1) != b[key].reshape(c.nq, -1)).any(axis=1).sum()
        print(c.name, key, "rows that differ", int(differ), "of", c.nq)
        assert 2 * differ >= c.nq, (c, differ)
    tables, last = d.tables()
    assert min(tables.count("A"), tables.count("B")) >= len(tables) // 4
    for c in dep:   # every tag-dependent card runs under both tables
        assert {t for t, x in zip(tables, d.circuit) if d.cards[x] is c} == {"A", "B"}, c
