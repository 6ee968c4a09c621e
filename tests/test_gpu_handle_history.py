"""One handle, any history (run with -m gpu on an MI355X): every deck of tests/handle_history.py runs its Eulerian circuit -- every call
family immediately after every other -- on ONE handle that lives for the whole circuit, and after every call all of the card's outputs
are compared with the CPU oracle's, byte for byte.  tests/test_handle_history_cpu.py proves the circuits complete.

A deck's handle makes three runs:
  1. the circuit with profiling on, the deferred cards left out (profiling pins calls to one lane): outputs, the launched first-pass
     names, the hand-over counters and the persistent general-kernel total are checked per call;
  2. the whole circuit again with profiling off, deferred cards included: after a deferred call the harness calls wait(keep=2) and checks
     what has finished; before a plain card it drains nothing itself -- the library does -- and synchronises to read;
  3. after close(), a fresh handle replays the circuit's tail (the last 2 F calls at least; the float deck: from the run of calm card /
     surprise twin pairs on) and must give the same bytes as run 2 did.
Mismatches are collected and reported as (run, call number, previous card, this card, what differs); the test asserts there are none.
"""
import collections
import hashlib
import time

import numpy as np
import pytest

import handle_history as hh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _digest(result, exp):
    h = hashlib.sha1()
    for name in sorted(exp):
        h.update(np.ascontiguousarray(hh.host(result[name])).tobytes())
    return h.hexdigest()


class Harness:
    def __init__(self, g, orc, deck):
        self.g, self.orc, self.deck = g, orc, deck
        self.failures = []
        self.planned = {c.name: deck.planned(g, c) for c in deck.cards}
        self.fixed_counters = {}     # card with an explicit visited-set capacity -> (retry_queries, general queries) of its first occurrence
        self.surprises = []          # (card, handle, earlier observed batches of its key, retry kernel, handed over, finished by the general kernel)
        self.digests = {}
        self.peak_outstanding = 0    # most deferred calls made and not yet waited for by the harness (see test_float_deck_...)
        self.general_total = 0
        self.calls = 0
        self.handle = 0              # handles opened so far: 1 the circuit's, 2 the replay's

    def open(self, table):
        self.ix = self.deck.open(self.g, table)
        self.table = table
        self.observed = {}
        self.outstanding = []
        self.handle += 1
        return self.ix

    def _check(self, run, i, prev, card, table, result, held, digest=None):
        exp = self.deck.expect(self.orc, card, table)
        bad = hh.differences(result, exp) + self.deck.extra_checks(self.ix, card, held) if not card.defer else hh.differences(result, exp)
        if digest == "keep":
            self.digests[i] = _digest(result, exp)
        elif digest == "same" and self.digests[i] != _digest(result, exp):
            bad.append("bytes differ from the first handle's")
        if bad:
            self.failures.append((run, i, str(prev), str(card), bad))

    def _drain(self, run, keep, digest):
        done, self.outstanding = self.outstanding[:len(self.outstanding) - keep], self.outstanding[len(self.outstanding) - keep:]
        for i, prev, card, table, result, held in done:
            self._check(run, i, prev, card, table, result, held, digest)

    def play(self, run, first, profiled, deferred, digest=None):
        """Calls first .. end of the circuit on the open handle.  profiled: profile every plain call; deferred: include the deferred cards."""
        import torch
        d, ix = self.deck, self.ix
        seq = d.circuit
        prev, prev_total, clean = None, None, False
        ix.profile_enable(profiled)
        for i in range(first, len(seq)):
            card = d.cards[seq[i]]
            if card.defer and not deferred:
                continue
            self.calls += 1
            if profiled and deferred:
                ix.profile_enable(not card.defer)
            seen = self.observed.get(card.skey, 0)
            result, held = d.run(self.g, ix, card, self.table, self.orc)
            if card.feeds_sizing:
                self.observed[card.skey] = seen + 1
            if card.defer:
                self.outstanding.append((i, prev, card, self.table, result, held))
                self.peak_outstanding = max(self.peak_outstanding, len(self.outstanding))
                ix.wait(keep=2)
                self._drain(run, 2, digest)
                clean = False
            else:
                torch.cuda.synchronize()   # (device tensors; and whatever was in flight: the library ordered this call behind it)
                self._drain(run, 0, digest)
                self._check(run, i, prev, card, self.table, result, held, digest)
                if profiled:
                    p = ix.profile_read(reset=False)
                    total = int(p["general_queries"])
                    bad = self._profile(card, p, None if prev_total is None or not clean else total - prev_total, seen)
                    if prev_total is not None and total < prev_total:
                        bad.append("general-kernel total fell from %d to %d" % (prev_total, total))
                    if bad:
                        self.failures.append((run, i, str(prev), str(card), bad))
                    prev_total, clean = total, True
                    self.general_total = max(self.general_total, total)
            self.table = d.table_after(self.table, card)
            prev = card
        ix.wait()
        torch.cuda.synchronize()
        self._drain(run, 0, digest)

    def _profile(self, card, p, delta, seen):
        """What the profile of a plain profiled call says against the card: the launched first pass, the growth of the persistent total,
        the counters of a card with an explicit capacity; a surprise card's evidence is recorded."""
        bad = []
        walks = card.kind in ("search", "auto")
        launched = p["walk_kernel"].split(" (")[0]
        if card.kind == "search" and self.planned[card.name] is not None and launched != self.planned[card.name]:
            bad.append("first pass launched %s, planned %s" % (launched, self.planned[card.name]))
        if delta is not None:
            if not walks:
                want = 0
            else:   # (a routed call too: it walks its whole batch through the same search, scan-routed queries under word 0, and the
                    # profile's list-B count is that walk's -- lanes.cpp, auto_device)
                want = card.nq if launched == "walk_general_kernel" else int(p["retry_general_queries"])
            if delta != want:
                bad.append("general-kernel total grew by %d, the call's general queries are %d" % (delta, want))
        if card.kind == "search" and card.hc and delta is not None:
            now = (int(p["retry_queries"]), delta)
            first = self.fixed_counters.setdefault(card.name, now)
            if now != first:
                bad.append("(retry_queries, general queries) %r, first occurrence %r" % (now, first))
        # A surprise card's evidence.  retry_kernel == "" with queries finished by the general kernel is the path that leaves the retry
        # launch out (skip_retry: the first pass appends to list B itself).  The other launch-free branch of call_plan.cpp, "nothing to
        # gain: A -> B", needs a first-pass table at least as large as the retry pass's -- a CU's whole LDS -- or a tagged / byte first pass:
        # the surprise cards are neither, and their tables are the LDS share of several wavefronts.
        if card.twin and delta is not None:
            self.surprises.append((card.name, self.handle, seen, p["retry_kernel"], int(p["retry_queries"]), delta))
        return bad


def _run(g, orc, name):
    d = hh.deck(name)
    h = Harness(g, orc, d)
    for c in d.cards:   # every expectation once, before the device runs (both tables where a card depends on the table)
        for table in ("AB" if c.tagdep and name == "float" else "A"):
            d.expect(orc, c, table)
    t0 = time.perf_counter()
    h.open("A")
    h.play("profiled", 0, profiled=True, deferred=False)
    t1 = time.perf_counter()
    start2 = h.table
    h.play("deferred", 0, profiled=False, deferred=True, digest="keep")
    t2 = time.perf_counter()
    h.ix.close()
    # the tag table in force at call replay_from of run 2
    table = start2
    for x in d.circuit[:d.replay_from]:
        table = d.table_after(table, d.cards[x])
    h.digests = {i: v for i, v in h.digests.items() if i >= d.replay_from}
    h.open(table)
    h.play("replay", d.replay_from, profiled=True, deferred=True, digest="same")
    h.ix.close()
    t3 = time.perf_counter()
    print("handle history", name, "cards", d.F, "calls", h.calls, "seconds: profiled %.2f deferred %.2f replay %.2f" % (t1 - t0, t2 - t1, t3 - t2),
          "peak deferred batches outstanding", h.peak_outstanding, "general-kernel total", h.general_total, "failures", len(h.failures))
    for s in h.surprises:
        print("surprise", s)
    for (run, card), count in sorted(collections.Counter((f[0], f[3]) for f in h.failures).items()):
        print("mismatches", run, card, count)   # (one line per run and card: an assertion message is cut short)
    return d, h


def test_float_deck_every_family_after_every_other(g, orc):
    """The float deck's circuit, bit-exact after every call.  Also: at least three deferred batches were outstanding at once -- counted by
    the harness as calls made with FLAG_DEFER_JOIN, depth 3, that it has not yet passed to wait(keep=2): it follows from the run of deferred
    cards that tests/test_handle_history_cpu.py proves the circuit to hold, the library reports no number of batches in flight; every
    surprise card was seen at least once, while its key was calm, on the path that leaves the retry launch out and appends the first
    pass's hand-overs to list B directly (retry_kernel == "" and queries finished by the general kernel), and at least once, before its key
    was calm, handed over to a named retry kernel (the replay's fresh handle); a card with hash_capacity = 128 reports the same hand-over
    counters at every occurrence; the persistent general-kernel total never falls and grows by exactly the call's general queries."""
    d, h = _run(g, orc, "float")
    assert not h.failures, (len(h.failures), h.failures[:12])
    assert h.peak_outstanding >= 3
    for c in (c for c in d.cards if c.twin):
        seen = [s for s in h.surprises if s[0] == c.name]
        assert any(n >= hh.CALM_AFTER and kernel == "" and general > 0 for _, _, n, kernel, _, general in seen), (c, seen)
        assert any(n < hh.CALM_AFTER and kernel != "" and handed > 0 for _, _, n, kernel, handed, _ in seen), (c, seen)
    assert {c.name for c in d.cards if c.kind == "search" and c.hc} == set(h.fixed_counters)
    assert all(handed > 0 for handed, _ in h.fixed_counters.values()), h.fixed_counters


def test_byte_deck_every_family_after_every_other(g, orc):
    """The byte deck's circuit on one create_bytes handle.  Its one deferred card follows itself once, so two deferred batches are
    outstanding at once (three need two deferred cards: the float deck)."""
    d, h = _run(g, orc, "bytes")
    assert not h.failures, (len(h.failures), h.failures[:12])
    assert h.peak_outstanding >= 2
    assert {c.name for c in d.cards if c.kind == "search" and c.hc} == set(h.fixed_counters)
    assert all(handed > 0 and general == handed for handed, general in h.fixed_counters.values()), h.fixed_counters   # the general byte kernel


def test_tie_deck_every_family_after_every_other(g, orc):
    """The tie deck's circuit: the tie class overflows the LDS tie list, so the general kernel serves queries (its total is positive) and
    really uses its tie bits; a bit left behind by one query would meet another query's walk in the same slot."""
    d, h = _run(g, orc, "ties")
    assert not h.failures, (len(h.failures), h.failures[:12])
    assert h.general_total > 0
