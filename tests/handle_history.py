"""History as an axis of the suite: what tests/test_handle_history_cpu.py and tests/test_gpu_handle_history.py share.

A gbnns_index carries state from call to call so that a call need not pay for a reset: two control blocks per lane that the general kernel
of call N clears for call N + 1, the general kernel's tie bits (zeroed once, kept zero by the kernel), the persistent general-kernel
total, grow-only lane buffers shared by every call family, the adaptive visited-set sizing per (ef, mode, ...) key with its calm streak
and the retry launch that is left out once a key is calm, lanes, knobs, the tag table, the half-row tables.  Every other test builds a
handle for its family.  Here a CARD is one call a user can make (entry point, arguments, knobs, batch size, memory kind, deferred or not),
a DECK the cards of one handle, and the call sequence of a deck an Eulerian circuit of the complete directed graph on its cards, self
loops included: F * F + 1 calls in which every card follows every card exactly once.

Expected values come from the existing oracles and helpers only (Oracle.walk / rerank / project / exact_knn / search_batch, tag_util,
bridge_util, topk_util, knn_tagged_util, tag_auto_util, half_rows_util, locality_order_util), computed once per (card, tag table) and
cached; data is datagen.full_mantissa, so a wrong summation order shows.  Nothing takes a tolerance.

Three decks:
  * float -- one handle with a net, db_low, an auxiliary graph, tags and half rows over a graph of two parts without an edge between them,
    6 000 sparse rows (degrees 2 .. 4) and 6 000 dense ones (26 .. 32).  The CALM cards of the four surprise keys (LOWQ ef 64, LOWQ ef 200,
    PLAIN ef 200, half rows ef 64) enter in the sparse part, as does every other card that feeds the sizing statistics of one of those keys;
    each has a SURPRISE twin of the same ef, mode and flags that enters in the dense part.  The circuit opens with the Eulerian circuit of the
    calm-side cards alone (every such key is calm before its first surprise) and holds, as one run, calm card / surprise twin of each key
    in turn; the replay on a fresh handle starts at that run (a surprise on a key that has seen one short batch and is not calm yet: the
    retry pass serves it -- an unseen key's first table, sized for 32 ef entries and more, holds these walks).
  * bytes -- one create_bytes handle with tags.
  * ties  -- test_general_kernel_paths' (b2) fixture: 2 000 rows on the shell at squared distance 5 plus 100 nearer ones, which overflows the
    LDS tie list, so the general kernel's tie bits are really used.
"""
import functools

import numpy as np

import bridge_util as bu
import datagen
import half_rows_util as hu
import knn_tagged_util as kt
import locality_order_util as lo
import oracle as orc_mod
import tag_auto_util as ta
import tag_util as tg
import topk_util as tu

D_ORIG, D_LOW, D_HIDDEN, D_BYTES = 40, 32, 64, 128   # (bytes: the byte-walk instances serve rows of 128 bytes)
FLAG_NO_FUSED_RERANK, FLAG_WIDE_INDEX, FLAG_BITMAP_PASS, FLAG_DEFER_JOIN, FLAG_HALF_ROWS = 2, 16, 32, 128, 512   # include/gbnns.h
FLAG_TAG_BRIDGE, FLAG_BYTE_WALK, FLAG_SCAN_GATHER = 1024, 2048, 4096
MODE_NET, MODE_LOWQ, MODE_PLAIN = 0, 1, 2
WANT = ("hops", "dist_calc", "cand", "cand_dist")
KNOBS = {"coop": 0, "late_rows": 0, "spec_min_nq": 0, "spec_any_form": 0, "spec_tail": 0, "order_min": 0, "order_bits": 12}
SCAN_BELOW = 5300      # float deck, 12 000 rows: words of an eighth of the rows and empty ones always scan; the half-of-the-rows words (6 000 under table A, about 4 700 under B) walk under A and scan under B; all-rows words walk
CALM_AFTER = 3         # observed batches of a key after which the library may leave the retry launch out (streak 0, 1, 2: call_plan.cpp)


class Card:
    """One call.  kind: search | auto | census | knn | rerank | rerank_topk | project | refuse | swap."""
    _defaults = dict(nq=96, ent=None, ef=0, mode=MODE_LOWQ, flags=0, knobs=(), hc=0, mem="numpy", defer=False, top_k=0, tags=None, aux=False,
                     want=WANT, u8=False, gather=False, k=10, buffers=(), twin=None, calm_side=False, table="low", n_entries=1)

    def __init__(self, name, kind, **kw):
        self.name, self.kind = name, kind
        for key, val in self._defaults.items():
            setattr(self, key, kw.pop(key, val))
        assert not kw, kw
        self.knobs = dict(self.knobs)

    def __repr__(self):
        return self.name

    @property
    def tagdep(self):
        return self.kind in ("auto", "census", "knn") or self.tags is not None

    @property
    def half(self):
        return bool(self.flags & FLAG_HALF_ROWS)

    @property
    def skey(self):
        """The ingredients of the library's sizing key (call_plan.cpp: ef, mode, aux, wide, half rows, tagged, bridged, byte instances,
        byte walk; the knob "hot" is never touched here), None for a call that does not walk."""
        if self.kind not in ("search", "auto"):
            return None
        return (self.ef, self.mode, bool(self.aux), bool(self.flags & FLAG_WIDE_INDEX), self.half, self.tagdep, bool(self.flags & FLAG_TAG_BRIDGE),
                bool(self.flags & FLAG_BYTE_WALK))

    @property
    def feeds_sizing(self):
        return self.skey is not None and self.hc == 0


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list((8200,) + key)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the circuit ---------------------------------------------------------------------------------------------------------------
def _hierholzer(out, start):
    """An Eulerian circuit over the edges out[u] (lists, consumed) from `start`, as a list of nodes."""
    stack, path = [start], []
    while stack:
        u = stack[-1]
        if out[u]:
            stack.append(out[u].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def complete_circuit(nodes, seed, start=None, without=()):
    """An Eulerian circuit of the complete directed graph on `nodes`, self loops included, less the edges (u, v) of `without`; edge
    order seeded."""
    rng = _rng(77, seed, len(nodes))
    nodes = list(nodes)
    out = {}
    for u in nodes:
        vs = [v for v in nodes if (u, v) not in without]
        rng.shuffle(vs)
        out[u] = vs
    return _hierholzer(out, nodes[0] if start is None else start)


def build_circuit(f, seed, first=(), trails=(), replay_trail=None):
    """The call sequence of a deck of f cards (indices): the circuit of the card set `first` alone, then a circuit of every other edge into
    which each closed trail of `trails` (a node list, first == last; or a node set: its complete circuit) is spliced as one run.
    -> (sequence, index at which the trail `replay_trail` starts, or the index 2 f calls before the end).  Every ordered pair is adjacent
    exactly once: `first` and the trails share no edge, each takes as many edges into a node as out of it, and what is left is connected.
    A trail replaces one occurrence of its first node in the circuit of the other edges; the places are chosen in that circuit as it is
    before any splice (so none lies inside a trail) and filled from the last to the first (so none moves)."""
    first = list(first)
    trails = [list(t) if isinstance(t, (list, tuple)) else complete_circuit(sorted(t), seed + 1 + i, start=min(t)) for i, t in enumerate(trails)]
    start = first[0] if first else 0
    head = complete_circuit(first, seed + 100, start=start) if first else [start]
    taken = [set(zip(t, t[1:])) for t in [head] + trails]
    assert all(t[0] == t[-1] and len(set(zip(t, t[1:]))) == len(t) - 1 for t in trails), "a trail repeats an edge or is not closed"
    assert sum(len(e) for e in taken) == len(set().union(*taken)), "trails that share an edge"
    rest = complete_circuit(range(f), seed, start=start, without=set().union(*taken))
    places = {}
    for ti, sub in enumerate(trails):
        where = [i for i, v in enumerate(rest) if v == sub[0]]
        # the replay's trail: the last place that leaves 2 f calls from its start to the end (later splices only add calls); else a third in
        places[ti] = [i for i in where if len(rest) - i - 1 + len(sub) >= 2 * f][-1] if ti == replay_trail else where[len(where) // 3]
    assert len(set(places.values())) == len(places)
    for ti in sorted(places, key=places.get, reverse=True):
        rest = rest[:places[ti]] + trails[ti] + rest[places[ti] + 1:]
    seq = head + rest[1:]
    if replay_trail is None:
        return seq, len(seq) - 2 * f
    sub = trails[replay_trail]
    return seq, next(i for i in range(len(seq)) if seq[i:i + len(sub)] == sub)


# ---- decks -----------------------------------------------------------------------------------------------------------------------
class Deck:
    name = None
    seed = 1
    extra_knobs = {}

    def __init__(self):
        self.cards = self.make_cards()
        self.index = {c.name: i for i, c in enumerate(self.cards)}
        assert len(self.index) == len(self.cards)
        self._exp = {}
        self.circuit, self.replay_from = build_circuit(len(self.cards), self.seed, **self.circuit_shape())

    def circuit_shape(self):
        return {}

    @property
    def F(self):
        return len(self.cards)

    def calls(self):
        """(call number, predecessor card or None, card) of the circuit."""
        return [(i, self.cards[self.circuit[i - 1]] if i else None, self.cards[c]) for i, c in enumerate(self.circuit)]

    def table_after(self, table, card):
        return ("B" if table == "A" else "A") if card.kind == "swap" else table

    def tables(self):
        """The tag table in force BEFORE each call of one pass that starts with table A, and the table after the pass."""
        t, out = "A", []
        for c in self.circuit:
            out.append(t)
            t = self.table_after(t, self.cards[c])
        return out, t

    def expect(self, orc, card, table="A"):
        key = (card.name, table if card.tagdep else None)
        if key not in self._exp:
            e = self.compute(orc, card, table)
            self._exp[key] = {k: np.ascontiguousarray(v) for k, v in e.items()}
        return self._exp[key]

    # -- running a card on a handle (device needed) --------------------------------------------------------------------------------
    def knobs_of(self, card):
        k = dict(KNOBS)
        k.update(self.extra_knobs)
        k.update(card.knobs)
        return k


def _t(a, mem):
    """A host array as the memory kind of a card: numpy as it is, a page-locked torch tensor, or a device tensor (uint32 as int32)."""
    if a is None or mem == "numpy":
        return a
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy())
    return t.pin_memory() if mem == "pinned" else t.cuda()


def host(x):
    """A result (numpy / torch) as a host numpy array."""
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def differences(result, exp):
    """Names of the outputs of `exp` that `result` does not equal byte for byte (floats by their bit patterns, ids as uint32)."""
    bad = []
    for name, want in exp.items():
        got = np.ascontiguousarray(host(result[name]))
        a = bits(got) if got.dtype.kind == "f" else got.astype(np.uint32) if got.dtype.itemsize < 4 else got.view(np.uint32)
        b = bits(want) if want.dtype.kind == "f" else want.astype(np.uint32) if want.dtype.itemsize < 4 else want.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(name if a.shape != b.shape else "%s (%d rows)" % (name, int((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1).sum())))
    return bad


def _walk_outputs(w, ids, want):
    e = dict(ids=ids)
    for out, name in (("cand", "ids"), ("cand_dist", "dists"), ("hops", "hops"), ("dist_calc", "dist_calc")):
        if out in want:
            e[out] = w[name]
    return e


class FloatDeck(Deck):
    name, seed = "float", 1
    N_A, N_B = 6000, 6000
    SWAP = (3000, 11000)   # rows whose words the swap card replaces: a partial range over both parts

    @functools.cached_property
    def data(self):
        rng = _rng(1)
        n = self.N_A + self.N_B
        d = dict(n=n, base=datagen.full_mantissa(rng, n, D_ORIG), db_low=datagen.full_mantissa(rng, n, D_LOW),
                 net=datagen.net_layers_full(rng, D_ORIG, D_HIDDEN, D_LOW), queries=datagen.full_mantissa(rng, 300, D_ORIG),
                 q_low=datagen.full_mantissa(rng, 300, D_LOW))
        off_a, nbr_a = datagen.random_graph(rng, self.N_A, 2, 4)      # sparse part: short walks
        off_b, nbr_b = datagen.random_graph(rng, self.N_B, 26, 32)    # dense part: long walks; no edge between the parts
        d["off"] = np.concatenate([off_a, off_b[1:] + off_a[-1]]).astype(np.uint64)
        d["nbr"] = np.concatenate([nbr_a, nbr_b + np.uint32(self.N_A)]).astype(np.uint32)
        d["aux"] = datagen.random_graph(rng, n, 0, 6)
        d["R"] = hu.rounded(d["db_low"])
        ent = dict(a=rng.integers(0, self.N_A, size=300).astype(np.uint32), b=(self.N_A + rng.integers(0, self.N_B, size=300)).astype(np.uint32),
                   b3=(self.N_A + rng.integers(0, self.N_B, size=(300, 3))).astype(np.uint32))
        A = tg.row_tags(n)
        B = A.copy()
        lo_, hi_ = self.SWAP
        j = np.arange(lo_, hi_)
        rot = ((A[j] << np.uint32(3)) | (A[j] >> np.uint32(5))) & np.uint32(0xFF)
        B[j] = np.where(j % 3 == 0, 0, rot).astype(np.uint32)      # other words, and a third of the rows that no query sees at all
        d["T"] = {"A": A, "B": B}
        both = A & B
        dense = np.arange(self.N_A, n)
        words = dict(tag=tg.query_tags(300), auto=ta.query_words(300), knn=kt.query_words(300))
        for name in ("tag", "auto"):   # entry points in the dense part that the query may see under either table (any dense row where it sees none)
            e = np.empty(300, np.uint32)
            for i, q in enumerate(words[name]):
                ok = dense[(both[dense] & q) != 0]
                e[i] = (ok if len(ok) else dense)[rng.integers(0, len(ok) if len(ok) else len(dense))]
            ent[name] = e
        d["ent"], d["words"] = ent, words
        for v in list(d.values()) + list(ent.values()) + list(words.values()) + list(d["T"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return d

    def make_cards(self):
        S = lambda name, **kw: Card(name, "search", buffers=("search",) + kw.pop("buffers", ()), **kw)
        cards = [
            # the calm side of the four surprise keys: sparse entries
            S("order64_33", ef=64, ent="a", calm_side=True, nq=33, knobs={"order_min": 1}, buffers=("order",)),   # (the circuit starts here: every buffer starts small)
            S("lowq64", ef=64, ent="a", calm_side=True), S("lowq200", ef=200, ent="a", calm_side=True, mem="device"),
            S("coop200", ef=200, ent="a", calm_side=True, knobs={"coop": 1}),
            S("plain200", ef=200, mode=MODE_PLAIN, ent="a", calm_side=True, table="orig"),
            S("half64", ef=64, ent="a", calm_side=True, flags=FLAG_HALF_ROWS, table="half"),
            S("order64_300", ef=64, ent="a", calm_side=True, nq=300, knobs={"order_min": 1}, buffers=("order",)),
            S("defer_dev64", ef=64, ent="a", calm_side=True, mem="device", defer=True),
            # their surprise twins: dense entries, same ef, mode and flags
            S("surprise_lowq64", ef=64, ent="b", twin="lowq64"), S("surprise_lowq200", ef=200, ent="b", twin="lowq200"),
            S("surprise_plain200", ef=200, mode=MODE_PLAIN, ent="b", twin="plain200", table="orig"),
            S("surprise_half64", ef=64, ent="b", twin="half64", flags=FLAG_HALF_ROWS, table="half"),
            # everything else enters in the dense part
            S("lowq8_300", ef=8, ent="b", nq=300),
            S("lowq64_hc128", ef=64, ent="b", hc=128), S("lowq200_hc128", ef=200, ent="b", hc=128),
            S("wide64", ef=64, ent="b", flags=FLAG_WIDE_INDEX), S("bitmap128", ef=128, ent="b", flags=FLAG_BITMAP_PASS),
            S("lowq1100", ef=1100, ent="b"), S("aux_llf48", ef=48, ent="b", aux=True),
            S("three_entries32_33", ef=32, ent="b3", nq=33, n_entries=3),
            S("net64_q_low", ef=64, mode=MODE_NET, ent="b", want=WANT + ("q_low",), table="net"),
            S("net32_no_fuse_33", ef=32, mode=MODE_NET, ent="b", nq=33, flags=FLAG_NO_FUSED_RERANK, table="net"),
            S("topk100_300", ef=100, ent="b", nq=300, top_k=10),
            S("tag64", ef=64, ent="tag", tags="tag"), S("tag200", ef=200, ent="tag", tags="tag"),
            S("bridge64", ef=64, ent="tag", tags="tag", flags=FLAG_TAG_BRIDGE),
            Card("auto64", "auto", ef=64, ent="auto", tags="auto", top_k=10, buffers=("search", "census")),
            Card("auto64_gather_33", "auto", ef=64, ent="auto", tags="auto", top_k=10, nq=33, flags=FLAG_SCAN_GATHER, buffers=("search", "census")),
            Card("census_300", "census", tags="auto", nq=300, mem="device", buffers=("census",)),
            Card("knn_gather", "knn", tags="knn", gather=True, buffers=("census",)),
            Card("knn_scan_300", "knn", tags="knn", nq=300, buffers=("census",)),
            Card("rerank", "rerank"), Card("rerank_topk", "rerank_topk"), Card("project_300", "project", nq=300),
            Card("refused", "refuse"),
            S("defer_pinned_topk48_33", ef=48, ent="b", nq=33, top_k=10, mem="pinned", defer=True),
            Card("swap_tags", "swap"),
        ]
        return cards

    def circuit_shape(self):
        """The calm side first; one run of the two deferred cards alone (five calls: three batches outstanding at once); and, where the
        replay starts, every surprise key's calm card followed at once by its surprise twin: on a fresh handle the key has then seen one
        short batch, its table is sized for that, and it is not calm yet -- the retry pass takes the hand-overs."""
        calm = [i for i, c in enumerate(self.cards) if c.calm_side and not c.defer]
        deferred = {i for i, c in enumerate(self.cards) if c.defer}
        pairs = [x for c in self.cards if c.twin for x in (self.index[c.twin], self.index[c.name])]
        return dict(first=calm, trails=(pairs + pairs[:1], deferred), replay_trail=0)

    def open(self, g, table="A"):
        d = self.data
        ix = g.Index(d["base"], d["off"], d["nbr"], db_low=d["db_low"], net=d["net"])
        ix.set_aux_graph(*d["aux"])
        ix.enable_half_rows()
        ix.set_tags(d["T"][table])
        return ix

    # -- expectations ---------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def _memo(self):
        return {}

    def _c(self, table, nq, ent, words):
        """The dict tag_util / bridge_util / tag_auto_util take: the deck's data with the table in force and the card's batch."""
        d = self.data
        return dict(base=d["base"], queries=d["queries"][:nq], db_low=d["db_low"], q_low=d["q_low"][:nq], off=d["off"], nbr=d["nbr"],
                    T=d["T"][table], Q=d["words"][words][:nq], ent=d["ent"][ent][:nq])

    def _walked(self, orc, card):
        """(walked queries, walked rows) of a card's batch."""
        d, nq = self.data, card.nq
        if card.table == "orig":
            return d["queries"][:nq], d["base"]
        if card.table == "net":
            if "q_net" not in self._memo:
                self._memo["q_net"] = orc.project(d["net"], d["queries"], threads=8)
            return self._memo["q_net"][:nq], d["db_low"]
        return d["q_low"][:nq], d["R"] if card.table == "half" else d["db_low"]

    def _walk(self, orc, card):
        d, nq = self.data, card.nq
        key = ("walk", card.table, card.ef, nq, card.ent, card.aux)
        if key not in self._memo:
            q, rows = self._walked(orc, card)
            kw = dict(aux=d["aux"], llf=True, hops_bound=50) if card.aux else {}
            self._memo[key] = orc.walk(q, rows, d["off"], d["nbr"], card.ef, entries=d["ent"][card.ent][:nq], threads=8, **kw)
        return self._memo[key]

    def _topk(self, orc, nq, w, k):
        d = self.data
        dist = tu.list_distances(orc, d["base"], d["queries"][:nq], w["ids"], w["count"], 0, self._memo.setdefault("dist", {}))
        return tu.expected_topk(dist, w["ids"], w["count"], k)

    def compute(self, orc, card, table):
        d, nq = self.data, card.nq
        if card.kind == "search" and card.tags is None:
            w = self._walk(orc, card)
            if card.mode == MODE_PLAIN:
                s = orc.search_batch(orc_mod.MODE_PLAIN, d["queries"][:nq], d["base"], d["off"], d["nbr"], card.ef, k=card.ef,
                                     entries=d["ent"][card.ent][:nq], threads=8)
                assert np.array_equal(s["hops"], w["hops"]) and np.array_equal(s["dist_calc"], w["dist_calc"])
                ids = s["ids"]
            else:
                ids = orc.rerank(d["queries"][:nq], w["ids"], w["count"], d["base"], threads=8)
            e = _walk_outputs(w, ids, card.want)
            if "q_low" in card.want:
                e["q_low"] = self._walked(orc, card)[0]
            if card.top_k:
                e["top_ids"], e["top_dist"] = self._topk(orc, nq, w, card.top_k)
            return e
        if card.kind == "search":
            c = self._c(table, nq, card.ent, card.tags)
            w = (bu if card.flags & FLAG_TAG_BRIDGE else tg).expected(orc, c, card.ef, 0)
            return _walk_outputs(w, w["want"], card.want)
        if card.kind == "auto":
            c = self._c(table, nq, card.ent, card.tags)
            e = ta.expected(orc, ("handle history", table, nq), c, card.ef, card.top_k, 0, SCAN_BELOW, ent=c["ent"])
            return {k: e[k] for k in ("ids", "top_ids", "top_dist", "cand", "cand_dist", "hops", "dist_calc", "allowed", "route")}
        if card.kind == "census":
            from gbnns_dim_red_amd import tag_census
            allowed, first = tag_census(d["T"][table], d["words"][card.tags][:nq])
            return dict(allowed=allowed, first=first)
        if card.kind == "knn":
            ids, dist = kt.expected(orc, d["base"], d["queries"][:nq], d["T"][table], d["words"][card.tags][:nq], card.k, 0)
            return dict(knn_ids=ids, knn_dist=dist)
        if card.kind in ("rerank", "rerank_topk"):
            w = self._walk(orc, self.cards[self.index["surprise_lowq64"]])
            if card.kind == "rerank":
                return dict(ids=orc.rerank(d["queries"][:nq], w["ids"], w["count"], d["base"], threads=8))
            ids, dist = self._topk(orc, nq, w, card.k)
            return dict(top_ids=ids, top_dist=dist)
        if card.kind == "project":
            return dict(q_low=orc.project(d["net"], d["queries"][:nq], threads=8))
        return {}

    def rerank_input(self, orc):
        w = self._walk(orc, self.cards[self.index["surprise_lowq64"]])
        return w["ids"], w["count"]

    def dist_calc_max(self, orc, card):
        return int(self._walk(orc, card)["dist_calc"].max())

    def planned(self, g, card):
        """The first-pass kernel the plan functions name for a search card (None: the call plans no walk of its own here)."""
        import ctypes
        d = self.data
        if card.kind != "search":
            return None
        stride = max(16, (int(np.diff(d["off"].astype(np.int64)).max()) + 15) // 16 * 16)
        if card.tags is not None:
            return (g.bridge_plan if card.flags & FLAG_TAG_BRIDGE else g.tag_plan)(0, D_LOW, d["n"], stride, card.ef)
        if card.half:   # (no plan function takes the flag: half_rows_util's name, which the device run holds against the launched one)
            return hu.half_kernel(0, D_LOW, card.ef, stride <= 32)
        knobs = self.knobs_of(card)
        wide, bitmap = bool(card.flags & FLAG_WIDE_INDEX), bool(card.flags & FLAG_BITMAP_PASS)
        dim = D_ORIG if card.mode == MODE_PLAIN else D_LOW
        fused = card.mode != MODE_PLAIN and not card.flags & FLAG_NO_FUSED_RERANK
        name, lds = ctypes.create_string_buffer(128), ctypes.c_uint64()
        rc = g.load_library().gbnns_debug_walk_plan(0, dim, dim, d["n"], stride, 16 if card.aux else 0, card.ef, card.n_entries, int(wide),
                                                    int(knobs["coop"] and not bitmap and not wide), knobs["late_rows"], 0, 1 if bitmap else 0,
                                                    4 * D_ORIG if fused else 0, name, 128, ctypes.byref(lds))
        assert rc == 0, card
        return name.value.decode()

    # -- one call -----------------------------------------------------------------------------------------------------------------
    def run(self, g, ix, card, table, orc):
        """Sets the card's knobs and makes its call -> (result dict, what must stay referenced until the result is read)."""
        d, nq = self.data, card.nq
        for name, val in self.knobs_of(card).items():
            ix.knob(name, val)
        q = d["queries"][:nq]
        if card.kind == "search":
            kw = dict(mode=card.mode, entry_ids=_t(d["ent"][card.ent][:nq], card.mem), want=card.want, flags=card.flags | (FLAG_DEFER_JOIN if card.defer else 0),
                      hash_capacity=card.hc, top_k=card.top_k)
            if card.mode == MODE_LOWQ:
                kw["queries_low"] = _t(d["q_low"][:nq], card.mem)
            if card.mode == MODE_PLAIN:
                kw["k"] = card.ef
            if card.aux:
                kw.update(aux=True, llf=True, hops_bound=50)
            if card.tags:
                kw["query_tags"] = _t(d["words"][card.tags][:nq], card.mem)
            if card.defer:
                kw.update(defer_depth=3, out={})
            qq = _t(q, card.mem)
            r = ix.search(qq, card.ef, **kw)
            return r, (qq, kw)
        if card.kind == "auto":
            r = ix.search_auto(q, card.ef, card.top_k, d["words"][card.tags][:nq], scan_below=SCAN_BELOW, mode=MODE_LOWQ, queries_low=d["q_low"][:nq],
                               entry_ids=d["ent"][card.ent][:nq], want=WANT, flags=card.flags)
            return r, None
        if card.kind == "census":
            words = _t(d["words"][card.tags][:nq], card.mem)
            allowed, first = ix.tag_census(words)
            return dict(allowed=allowed, first=first), words
        if card.kind == "knn":
            ids, dist = ix.exact_knn(q, card.k, query_tags=d["words"][card.tags][:nq], want_dist=True, gather=card.gather)
            return dict(knn_ids=ids, knn_dist=dist), None
        if card.kind == "rerank":
            cand, count = self.rerank_input(orc)
            return dict(ids=ix.rerank(q, cand, count)), None
        if card.kind == "rerank_topk":
            cand, count = self.rerank_input(orc)
            ids, dist = ix.rerank_topk(q, cand, card.k, count)
            return dict(top_ids=ids, top_dist=dist), None
        if card.kind == "project":
            return dict(q_low=ix.project(q)), None
        if card.kind == "refuse":   # half rows have no PLAIN walk: GBNNS_ERR_INVALID, and nothing changes
            try:
                ix.search(q, 64, mode=MODE_PLAIN, k=1, entry_ids=d["ent"]["b"][:nq], flags=FLAG_HALF_ROWS)
            except g.GbnnsError as e:
                return dict(), ("refused", e.code)
            return dict(), ("refused", None)
        if card.kind == "swap":
            lo_, hi_ = self.SWAP
            ix.set_tags(d["T"][self.table_after(table, card)][lo_:hi_], first=lo_)
            return dict(), None
        raise AssertionError(card.kind)

    def extra_checks(self, ix, card, held):
        """Problems of a call beyond its outputs: the refusal's code, the order a locality-ordered call walked in."""
        if card.kind == "refuse":
            return [] if held == ("refused", 1) else ["refusal: %r" % (held,)]
        if card.knobs.get("order_min"):
            last = ix.knob_get("order_last")
            if last != card.nq:
                return ["order_last %d, batch %d" % (last, card.nq)]
            return lo.problems(ix.order_last(), self.data["q_low"][:card.nq], 12)
        return []


class ByteDeck(Deck):
    name, seed = "bytes", 1
    N = 3000
    extra_knobs = {"byte_query_int": 7}

    @functools.cached_property
    def data(self):
        rng = _rng(2)
        n = self.N
        base = rng.integers(0, 256, size=(n, D_BYTES)).astype(np.uint8)
        pick = rng.integers(0, n, size=300)
        q8 = np.clip(np.rint(base[pick].astype(np.float64) + rng.normal(0.0, 20.0, size=(300, D_BYTES))), 0, 255).astype(np.uint8)
        qf = np.clip(q8.astype(np.float64) + rng.integers(-(1 << 13), 1 << 13, size=q8.shape) / float(1 << 14), 0.0, 255.0).astype(np.float32)
        off, nbr = datagen.random_graph(rng, n, 2, 30)
        T = tg.row_tags(n)
        words = dict(tag=tg.query_tags(300), auto=ta.query_words(300), knn=kt.query_words(300))
        ent = dict(b=rng.integers(0, n, size=300).astype(np.uint32))
        for name in ("tag", "auto"):
            e = np.empty(300, np.uint32)
            for i, q in enumerate(words[name]):
                ok = np.flatnonzero(T & q)
                e[i] = ok[rng.integers(0, len(ok))] if len(ok) else rng.integers(0, n)
            ent[name] = e
        return dict(n=n, base=base, wide=np.ascontiguousarray(base.astype(np.float32)), db_low=datagen.full_mantissa(rng, n, D_LOW),
                    q_low=datagen.full_mantissa(rng, 300, D_LOW), q8=np.ascontiguousarray(q8), q8f=np.ascontiguousarray(q8.astype(np.float32)),
                    queries=np.ascontiguousarray(qf), off=off, nbr=nbr, T={"A": T}, words=words, ent=ent)

    SCAN_BELOW = 500   # 3 000 rows: the words of an eighth of the rows and the empty ones scan

    def make_cards(self):
        S = lambda name, **kw: Card(name, "search", buffers=("search",), ent=kw.pop("ent", "b"), **kw)
        return [
            S("fused64", ef=64), S("u8_queries64_33", ef=64, u8=True, nq=33),
            S("byte_walk64", ef=64, mode=MODE_PLAIN, flags=FLAG_BYTE_WALK, table="orig"),
            S("byte_walk64_u8", ef=64, mode=MODE_PLAIN, flags=FLAG_BYTE_WALK, u8=True, table="orig"),
            S("tag64", ef=64, ent="tag", tags="tag"), S("bridge64", ef=64, ent="tag", tags="tag", flags=FLAG_TAG_BRIDGE),
            S("topk100_300", ef=100, nq=300, top_k=10),
            Card("knn_bytes_300", "knn", tags="knn", nq=300, u8=True, buffers=("census",)),
            Card("auto64_33", "auto", ef=64, ent="auto", tags="auto", top_k=10, nq=33, u8=True, buffers=("search", "census")),
            S("fused64_hc128", ef=64, hc=128),
            S("defer_dev64", ef=64, mem="device", defer=True),
            Card("refused", "refuse"),
        ]

    def open(self, g, table="A"):
        d = self.data
        ix = g.Index(d["base"], d["off"], d["nbr"], db_low=d["db_low"])
        ix.set_tags(d["T"]["A"])
        return ix

    @functools.cached_property
    def _memo(self):
        return {}

    def _queries(self, card):
        d = self.data
        return (d["q8f"] if card.u8 else d["queries"])[:card.nq]

    def _walk(self, orc, card):
        d, nq = self.data, card.nq
        key = ("walk", card.table, card.u8 and card.table == "orig", card.ef, nq, card.ent)
        if key not in self._memo:
            q, rows = (self._queries(card), d["wide"]) if card.table == "orig" else (d["q_low"][:nq], d["db_low"])
            self._memo[key] = orc.walk(q, rows, d["off"], d["nbr"], card.ef, entries=d["ent"][card.ent][:nq], threads=8)
        return self._memo[key]

    def compute(self, orc, card, table):
        d, nq = self.data, card.nq
        q = self._queries(card)
        c = dict(base=d["wide"], queries=q, db_low=d["db_low"], q_low=d["q_low"][:nq], off=d["off"], nbr=d["nbr"], T=d["T"]["A"],
                 Q=d["words"][card.tags][:nq] if card.tags else None, ent=d["ent"][card.ent][:nq] if card.ent else None)
        if card.kind == "search" and card.tags is None:
            w = self._walk(orc, card)
            if card.mode == MODE_PLAIN:
                s = orc.search_batch(orc_mod.MODE_PLAIN, q, d["wide"], d["off"], d["nbr"], card.ef, k=card.ef, entries=c["ent"], threads=8)
                assert np.array_equal(s["hops"], w["hops"]) and np.array_equal(s["dist_calc"], w["dist_calc"])
                ids = s["ids"]
            else:
                ids = orc.rerank(q, w["ids"], w["count"], d["wide"], threads=8)
            e = _walk_outputs(w, ids, card.want)
            if card.top_k:
                dist = tu.list_distances(orc, d["wide"], q, w["ids"], w["count"], 0, self._memo.setdefault(("dist", card.u8), {}))
                e["top_ids"], e["top_dist"] = tu.expected_topk(dist, w["ids"], w["count"], card.top_k)
            return e
        if card.kind == "search":
            w = (bu if card.flags & FLAG_TAG_BRIDGE else tg).expected(orc, c, card.ef, 0)
            return _walk_outputs(w, w["want"], card.want)
        if card.kind == "auto":
            e = ta.expected(orc, ("handle history bytes", nq), c, card.ef, card.top_k, 0, self.SCAN_BELOW, ent=c["ent"])
            return {k: e[k] for k in ("ids", "top_ids", "top_dist", "cand", "cand_dist", "hops", "dist_calc", "allowed", "route")}
        if card.kind == "knn":
            ids, dist = kt.expected(orc, d["base"], d["q8"][:nq], d["T"]["A"], c["Q"], card.k, 0)
            return dict(knn_ids=ids, knn_dist=dist)
        return {}

    @property
    def stride(self):
        return max(16, (int(np.diff(self.data["off"].astype(np.int64)).max()) + 15) // 16 * 16)

    def planned(self, g, card):
        d = self.data
        if card.kind != "search":
            return None
        stride = self.stride
        if card.flags & FLAG_BYTE_WALK:
            return (g.byte_query_plan if card.u8 else g.byte_walk_plan)(0, D_BYTES, d["n"], stride, card.ef)
        if card.tags is not None:
            return (g.bridge_plan if card.flags & FLAG_TAG_BRIDGE else g.tag_plan)(0, D_LOW, d["n"], stride, card.ef)
        return g.byte_plan(0, D_LOW, d["n"], stride, card.ef)[0]

    def run(self, g, ix, card, table, orc):
        d, nq = self.data, card.nq
        for name, val in self.knobs_of(card).items():
            ix.knob(name, val)
        q = (d["q8"] if card.u8 else d["queries"])[:nq]
        if card.kind == "search":
            kw = dict(mode=card.mode, entry_ids=_t(d["ent"][card.ent][:nq], card.mem), want=card.want, flags=card.flags | (FLAG_DEFER_JOIN if card.defer else 0),
                      hash_capacity=card.hc, top_k=card.top_k)
            if card.mode == MODE_LOWQ:
                kw["queries_low"] = _t(d["q_low"][:nq], card.mem)
            if card.mode == MODE_PLAIN:
                kw["k"] = card.ef
            if card.tags:
                kw["query_tags"] = _t(d["words"][card.tags][:nq], card.mem)
            if card.defer:
                kw.update(defer_depth=3, out={})
            qq = _t(q, card.mem)
            return ix.search(qq, card.ef, **kw), (qq, kw)
        if card.kind == "auto":
            r = ix.search_auto(q, card.ef, card.top_k, d["words"][card.tags][:nq], scan_below=self.SCAN_BELOW, mode=MODE_LOWQ, queries_low=d["q_low"][:nq],
                               entry_ids=d["ent"][card.ent][:nq], want=WANT, flags=card.flags)
            return r, None
        if card.kind == "knn":
            ids, dist = ix.exact_knn(q, card.k, query_tags=d["words"][card.tags][:nq], want_dist=True)
            return dict(knn_ids=ids, knn_dist=dist), None
        if card.kind == "refuse":   # float queries against byte rows: there is no mixed-pair scan (GBNNS_ERR_UNSUPPORTED), nothing changes
            try:
                ix.exact_knn(d["queries"][:nq], card.k)
            except g.GbnnsError as e:
                return dict(), ("refused", e.code)
            return dict(), ("refused", None)
        raise AssertionError(card.kind)

    def extra_checks(self, ix, card, held):
        if card.kind == "refuse":
            return [] if held == ("refused", 5) else ["refusal: %r" % (held,)]
        return []


class TieDeck(Deck):
    name, seed = "ties", 1

    @functools.cached_property
    def data(self):
        import itertools
        shell = sorted({p_ for base_ in ((2, 1, 0, 0),) for perm in itertools.permutations(base_)
                        for sg in itertools.product((1, -1), repeat=4)
                        for p_ in [tuple(a * b for a, b in zip(perm, sg))]})
        rng = np.random.Generator(np.random.PCG64(10))   # test_general_kernel_paths (b2), draw for draw
        far = np.array([shell[i] for i in rng.integers(0, len(shell), size=2000)], np.float32)
        near = np.zeros((100, 4), np.float32)
        near[:, 0] = (np.arange(1, 101) / 64.0).astype(np.float32)
        base = np.concatenate([far, near])[rng.permutation(2100)]
        off, nbr = datagen.random_graph(rng, 2100, 16, 32)
        ent = dict(first=rng.integers(0, 2100, size=64).astype(np.uint32))
        # the other batch: the same all-zero query -- the tie shell is the rows at squared distance 5 from it, any other query breaks the
        # ties up -- from other entry points and at other batch sizes, so the walks, and the slots their tie bits fall in, differ
        ent["second"] = rng.integers(0, 2100, size=300).astype(np.uint32)
        return dict(n=2100, base=np.ascontiguousarray(base), off=off, nbr=nbr, ent=ent, queries=np.zeros((300, 4), np.float32))

    def make_cards(self):
        P = lambda name, **kw: Card(name, "search", mode=MODE_PLAIN, table="orig", buffers=("search",), want=WANT, **kw)
        return [P("plain8", ef=8, nq=64, ent="first"), P("plain32", ef=32, nq=64, ent="first"), P("plain64", ef=64, nq=64, ent="first"),
                P("plain100", ef=100, nq=64, ent="first"), P("plain32_other_33", ef=32, nq=33, ent="second"),
                P("plain64_other_300", ef=64, nq=300, ent="second"), P("plain100_hc128", ef=100, nq=64, ent="first", hc=128)]

    def open(self, g, table="A"):
        d = self.data
        return g.Index(d["base"], d["off"], d["nbr"])

    @functools.cached_property
    def _memo(self):
        return {}

    def compute(self, orc, card, table):
        d, nq = self.data, card.nq
        key = (card.ef, nq, card.ent)
        if key not in self._memo:
            w = orc.walk(d["queries"][:nq], d["base"], d["off"], d["nbr"], card.ef, entries=d["ent"][card.ent][:nq], threads=8)
            s = orc.search_batch(orc_mod.MODE_PLAIN, d["queries"][:nq], d["base"], d["off"], d["nbr"], card.ef, k=card.ef,
                                 entries=d["ent"][card.ent][:nq], threads=8)
            assert np.array_equal(s["hops"], w["hops"]) and np.array_equal(s["dist_calc"], w["dist_calc"])
            self._memo[key] = _walk_outputs(w, s["ids"], card.want)
        return self._memo[key]

    def planned(self, g, card):
        return None   # (rows of four floats: whatever serves them, the fixture is about the general kernel's tie bits)

    def run(self, g, ix, card, table, orc):
        d, nq = self.data, card.nq
        for name, val in self.knobs_of(card).items():
            ix.knob(name, val)
        r = ix.search(d["queries"][:nq], card.ef, mode=MODE_PLAIN, k=card.ef, entry_ids=d["ent"][card.ent][:nq], want=card.want, hash_capacity=card.hc)
        return r, None

    def extra_checks(self, ix, card, held):
        return []


@functools.lru_cache(maxsize=None)
def deck(name):
    return {"float": FloatDeck, "bytes": ByteDeck, "ties": TieDeck}[name]()


DECKS = ("float", "bytes", "ties")
