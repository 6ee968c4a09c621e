"""The row-length sweep without a device: tests/dim_sweep.py's table covers every rung of every distance ladder and both sides of every
switch between forms, and the data of tests/test_gpu_dim_sweep.py makes a wrong rung visible at every length.

Coverage: over dim_sweep.DIMS, with the form of every length asked from the library's plan functions, every rung of every ladder is seen
with 0 trips, with 1 trip and with >= 2 trips wherever its ladder allows that count (ALLOWED below says which counts a ladder cannot
produce, and why).  Switches: every form a plan function can return has a length in DIMS, the lengths next to each threshold are in
DIMS, and the two thresholds that live in device code are read back from the sources.

Data, on datagen.full_mantissa rows (512 rows, one query per length; conditions on the reference side only, shares printed with -s):
  * the numpy restatements l2_ref / negdot_ref of tests/test_rounding_fixtures.py equal the oracle bit for bit at every length;
  * a mistake in the SET of coordinates -- one 4-wide step dropped, the L2 tail included, the last coordinate of the dot product dropped --
    changes >= 99 % of the distance bit patterns at every length it applies to;
  * a mistake in the ORDER changes >= 10 % (test_rounding_fixtures.py's bar) from the first length at which a running sum holds two
    products: the L2 tree fold and the dot left fold from d = 4 (the final fold adds four sums), the L2 fused multiply-add from d = 8,
    the dot fused multiply-add from d = 16.  Below those lengths each sum holds one product, a fused multiply-add onto +0 rounds once
    like the product itself, and the mistake is invisible: nothing is asserted there;
  * d < 4 under L2: no step runs, every distance is +0, and the expected answers are the tie rules' -- the lowest ids for the scan, the
    first candidate in pop order for the re-rank.
"""
import os
import re

import numpy as np
import pytest

import datagen
import dim_sweep as ds
import golden_util as gu
import test_rounding_fixtures as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gbnns_dim_red_amd", "csrc")
F32 = np.float32


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.build_library()
    g.load_library()
    return g


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the plan function ----------------------------------------------------------------------------------------------------------------
def test_rerank_plan_reports_the_one_choice(g):
    """gbnns_debug_rerank_plan: names, DEEP and the fused flag at the lengths either side of every rule; its refusals; and the choice is
    written once -- rerank_plan.h -- with every site that used to spell it calling that header's function."""
    import ctypes as C
    assert g.rerank_plan(0, 128) == ("rerank_pair_kernel<0>", 8, True) and g.rerank_plan(0, 380) == ("rerank_pair_kernel<0>", 8, True)
    assert g.rerank_plan(0, 384) == ("rerank_pair_kernel<0>", 24, True) and g.rerank_plan(0, 960) == ("rerank_pair_kernel<0>", 24, True)
    assert g.rerank_plan(0, 4) == ("rerank_pair_kernel<0>", 8, True) and g.rerank_plan(0, 3) == ("rerank_kernel<0>", 0, False)
    assert g.rerank_plan(0, 385) == ("rerank_kernel<0>", 0, False) and g.rerank_plan(0, 45) == ("rerank_kernel<0>", 0, False)
    assert g.rerank_plan(1, 8) == ("rerank_pair_kernel<1>", 8, True) and g.rerank_plan(1, 960) == ("rerank_pair_kernel<1>", 8, True)
    assert g.rerank_plan(1, 300) == ("rerank_kernel<1>", 0, False) and g.rerank_plan(1, 4) == ("rerank_kernel<1>", 0, False)
    assert g.rerank_plan(0, 16, bytes=True) == ("rerank_bytes_pair_kernel", 4, True) and g.rerank_plan(0, 176, bytes=True)[0] == "rerank_bytes_pair_kernel"
    assert g.rerank_plan(0, 8, bytes=True) == ("rerank_bytes_kernel<0>", 0, False) and g.rerank_plan(0, 100, bytes=True) == ("rerank_bytes_kernel<0>", 0, False)
    assert g.rerank_plan(1, 16, bytes=True) == ("rerank_bytes_kernel<1>", 0, False) and g.rerank_plan(1, 45, bytes=True) == ("rerank_bytes_kernel<1>", 0, False)
    lib = g.load_library()
    name, deep, fused = C.create_string_buffer(128), C.c_int(), C.c_int()
    ok = (0, 128, 0)
    assert lib.gbnns_debug_rerank_plan(*ok, name, 128, C.byref(deep), C.byref(fused)) == 0
    for bad in ((2, 128, 0), (-1, 128, 0), (0, 0, 0), (1, 0, 1)):
        assert lib.gbnns_debug_rerank_plan(*bad, name, 128, C.byref(deep), C.byref(fused)) == 1, bad
    assert lib.gbnns_debug_rerank_plan(*ok, None, 128, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_rerank_plan(*ok, name, 0, C.byref(deep), C.byref(fused)) == 1
    assert lib.gbnns_debug_rerank_plan(*ok, name, 128, None, C.byref(fused)) == 1
    assert lib.gbnns_debug_rerank_plan(*ok, name, 128, C.byref(deep), None) == 1
    short = C.create_string_buffer(8)
    assert lib.gbnns_debug_rerank_plan(*ok, short, 8, C.byref(deep), C.byref(fused)) == 0 and short.value == b"rerank_"
    # one place: the launchers, the pair kernels and the search call's plan call rerank_plan(); no other unit spells the rule
    for unit, calls in (("rerank.hip", 2), ("rerank_bytes.hip", 2), ("call_plan.cpp", 2), ("search_core.cpp", 0), ("handle.cpp", 1)):
        assert len(re.findall(r"(?<!\w)rerank_plan\(", _src(unit))) == calls, unit
    assert _src("rerank.hip").count("rerank_pairs_deep(METRIC, p.dim) == 24") == 2    # (the pair kernels: DEEP of a length already in the pair form)
    for unit in sorted(os.listdir(CSRC)):
        if unit.endswith((".hip", ".cpp", ".h", ".inc")) and unit != "rerank_plan.h":
            text = _src(unit)
            assert "kRerankDeepMinDim" not in text and "dim >= 384" not in text and "rerank_bytes_pair_form" not in text, unit
            assert not re.search(r"% 8 == 0 \|\| \(.*% 4 == 0", text), unit


def test_device_side_thresholds_are_the_sources(g):
    """The two switches no plan function reports, read back from the sources they live in."""
    assert re.search(r"constexpr uint32_t kQuadRowsMinDim = (\d+);", _src("walk_generic.h")).group(1) == str(ds.QUAD_ROWS_MIN_DIM)
    assert _src("walk_generic.h").count("p.dim >= kQuadRowsMinDim") == 3
    assert re.search(r"const bool on_device = M <= 64 && d <= (\d+);", _src("graph_api.cpp")).group(1) == str(ds.GD_DEVICE_MAX_DIM)
    assert ds.GD_DEVICE_MAX_DIM in ds.GD_DIMS and ds.GD_DEVICE_MAX_DIM + 1 in ds.GD_DIMS and 1 in ds.GD_DIMS


# ---- every rung with 0, 1 and >= 2 trips ------------------------------------------------------------------------------------------------
def _classes(traces, rung):
    return {min(int(t[rung]), 2) for t in traces}


# counts a ladder cannot produce (everything else of {0, 1, >= 2} must be seen)
ALLOWED = {
    # d < 384: at most 47 pairs -- the 8-loop leaves at most 7, so the 4-loop runs at most once
    "l2_pairs_8": dict(deep24={0}, eight={0, 1, 2}, four={0, 1}, rest={0, 1, 2}, odd_step={0, 1}),
    # d >= 384: at least 48 pairs, two trips of the 24-loop or more; it leaves at most 23 pairs: the 8-loop runs at most twice
    "l2_pairs_24": dict(deep24={2}, eight={0, 1, 2}, four={0, 1}, rest={0, 1, 2}, odd_step={0, 1}),
    "dot_pairs": dict(eight={0, 1, 2}, rest={0, 1, 2}),
    # the re-rank runs a lane per row under L2 only at d % 4 != 0: the tail is never empty there
    "l2_lane_rerank": dict(four={0, 1, 2}, rest={0, 1, 2}, tail={1, 2}),
    "l2_lane_walk": dict(four={0, 1, 2}, rest={0, 1, 2}, tail={0, 1, 2}),
    "dot_lane": dict(eight={0, 1, 2}, four_wide={0, 1}, masked={0, 1}, masked_lanes={0, 1, 2}),
    "byte_pairs": dict(four={0, 1, 2}, rest={0, 1, 2}, odd_chunk={0, 1}),
    # d >= 128: 32 steps and more
    "quad": dict(sixteen={2}, masked={0, 1, 2}, tail={0, 1, 2}),
}


def _assert_rungs(ladder, traces):
    assert traces, ladder
    for rung, want in ALLOWED[ladder].items():
        assert _classes(traces, rung) == want, (ladder, rung, sorted(_classes(traces, rung)), sorted(want))


def test_every_rung_of_every_ladder_runs_zero_one_and_more_times(g):
    by = {k: [] for k in ALLOWED}
    for d in ds.DIMS:
        form, tr = ds.rerank_trace(g, 0, d)
        by["l2_pairs_%d" % ds.rerank_form(g, 0, d)[1] if form == "pairs" else "l2_lane_rerank"].append(tr)
        form, tr = ds.rerank_trace(g, 1, d)
        by["dot_pairs" if form == "pairs" else "dot_lane"].append(tr)
        form, tr = ds.rerank_trace(g, 0, d, bytes=True)
        if form == "chunk_pairs":
            by["byte_pairs"].append(tr)
        for ef in (40, 200):
            wf = ds.walk_form(0, d, ds.walk_plan(g, 0, d, ds.N, ds.ELL_STRIDE, ef))
            if wf in ("lane", "quad"):
                by["quad" if wf == "quad" else "l2_lane_walk"].append(ds.walk_trace(0, d, wf))
    for ladder, traces in by.items():
        _assert_rungs(ladder, traces)
    # single rows that matter, as traces
    assert ds.trace_l2_pairs(4, 8) == dict(deep24=0, eight=0, four=0, rest=0, odd_step=1)          # the even lane's lone step is all
    assert ds.trace_l2_pairs(12, 8) == dict(deep24=0, eight=0, four=0, rest=1, odd_step=1)
    assert ds.trace_l2_pairs(960, 24) == dict(deep24=5, eight=0, four=0, rest=0, odd_step=0)
    assert ds.trace_l2_pairs(508, 24) == dict(deep24=2, eight=1, four=1, rest=3, odd_step=1)       # every rung of the DEEP = 24 ladder in one row
    assert ds.trace_l2_pairs(380, 8) == dict(deep24=0, eight=5, four=1, rest=3, odd_step=1)
    assert ds.trace_byte_pairs(176) == dict(four=1, rest=1, odd_chunk=1) and ds.trace_byte_pairs(32) == dict(four=0, rest=1, odd_chunk=0)
    assert ds.trace_quad(188)["masked"] == 15 and ds.trace_quad(132)["masked"] == 1 and ds.trace_quad(129) == dict(sixteen=2, masked=0, tail=1)
    # the masked step of the dot form a lane per row: alone (d % 8 in 1 .. 3), behind the 4-wide step (5 .. 7), with no 8-wide iteration
    rems = {(t["eight"] > 0, d % 8) for d in ds.DIMS for t in [ds.trace_dot_lane(d)] if ds.rerank_form(g, 1, d)[0] == "lane"}
    assert rems == {(e, r) for e in (False, True) for r in range(1, 8)}
    # the masked batch of the quad form at 1, 15 and a count between
    quad_masked = {ds.trace_quad(d)["masked"] for d in ds.DIMS if d >= ds.QUAD_ROWS_MIN_DIM}
    assert {0, 1, 2, 11, 15} <= quad_masked, sorted(quad_masked)


def test_scan_classes_and_padding(g):
    """Every S class and the wide kernel are named over DIMS; in every S class the first length (its smallest step count), a full row and a
    tail are present; the wide kernel runs with 0, 1 and 7 zero-filled steps, with exactly four chunks at d = 129, and d = 1 .. 3 (no step at
    all) belong to the narrowest class."""
    for metric in (0, 1):
        seen = {}
        for d in ds.DIMS:
            if metric == 1 and d % 8:
                continue
            name, _ = g.knn_plan(False, metric, ds.N, ds.NQ, d, 20)
            t = ds.trace_scan(d, name)
            seen.setdefault((t["kernel"], t.get("S")), []).append((d, t))
        assert set(seen) == {("scan", 8), ("scan", 16), ("scan", 32), ("wide", None)}, (metric, sorted(seen, key=str))
        for S in (8, 16, 32):
            assert max(t["steps"] for _, t in seen[("scan", S)]) == S, (metric, S)    # a row that fills the registers
        if metric == 0:
            for S in (8, 16, 32):   # from the class's first step count (the class below ends at S / 2 steps) to a full row; 0, 1, >= 2 zero steps
                steps = {t["steps"] for _, t in seen[("scan", S)]}
                assert min(steps) == (0 if S == 8 else S // 2), (S, sorted(steps))
                assert {min(t["zero_steps"], 2) for _, t in seen[("scan", S)]} == {0, 1, 2}, S
            assert [d for d, t in seen[("scan", 8)] if t["steps"] == 0] == [1, 2, 3]
            for S in (16, 32):   # the first lengths of the class: S / 2 steps and a tail of 1 .. 3
                assert {d for d, t in seen[("scan", S)] if t["steps"] == S // 2} >= {2 * S + 1, 2 * S + 2, 2 * S + 3}, S
            wide = dict(seen[("wide", None)])
            assert {t["pad"] for t in wide.values()} >= {0, 1, 7} and wide[129] == dict(kernel="wide", chunks=4, pad=0, tail=1)
            assert {t["tail"] for t in wide.values()} == {0, 1, 2, 3}


def test_every_switch_has_a_length_on_each_side(g):
    dims = set(ds.DIMS)
    # DEEP: the last pair-form length below the threshold and the threshold itself
    assert {376, 380, 384, 388} <= dims
    assert ds.rerank_form(g, 0, 380) == ("pairs", 8, True) and ds.rerank_form(g, 0, 384) == ("pairs", 24, True)
    # the form choices by d % 4, d % 8 (float rows) and d % 16 (byte rows): every residue below and above the first period, and every
    # answer the plan function gives anywhere is given for a length of DIMS
    assert {d % 8 for d in dims if d > 8} == set(range(8)) and {d % 16 for d in dims if d > 16} == set(range(16))
    for metric in (0, 1):
        for bytes_ in (False, True):
            everywhere = {g.rerank_plan(metric, d, bytes_) for d in range(1, 1025)}
            assert {g.rerank_plan(metric, d, bytes_) for d in dims} == everywhere, (metric, bytes_)
    # 128: the quad rows of the run-time-length L2 walks, the scan's wide kernel, the GD guard
    assert {124, 127, 128, 129, 131, 132} <= dims
    forms = {d: ds.walk_form(0, d, ds.walk_plan(g, 0, d, ds.N, ds.ELL_STRIDE, 200)) for d in (124, 127, 129, 131, 132, 188, 300, 960)}
    assert forms[124] == forms[127] == "lane" and all(forms[d] == "quad" for d in (129, 131, 132, 188, 300, 960)), forms
    assert g.knn_plan(False, 0, ds.N, ds.NQ, 128, 20)[0] == "knn_scan_kernel<0, 32, 1, false>"
    assert g.knn_plan(False, 0, ds.N, ds.NQ, 129, 20)[0] == "knn_scan_wide_kernel<0, 16, false>"
    # the S classes
    for lo, hi in ((32, 33), (64, 65)):
        assert {lo, hi} <= dims and g.knn_plan(False, 0, ds.N, ds.NQ, lo, 20)[0] != g.knn_plan(False, 0, ds.N, ds.NQ, hi, 20)[0]
    # the walk forms over the sweep: a lane per row, four lanes per row, compile-time lengths, and the general kernel for two entry points
    walk_forms = {ds.walk_form(m, d, ds.walk_plan(g, m, d, ds.N, ds.ELL_STRIDE, ef)) for m in (0, 1) for d in dims for ef in (40, 200)}
    assert {"lane", "quad"} <= walk_forms and any(f.startswith("fixed") for f in walk_forms), walk_forms
    assert all(ds.walk_plan(g, m, d, ds.N, ds.ELL_STRIDE, 40, n_entries=2) == "walk_general_kernel" for m in (0, 1) for d in dims)
    print("walk forms over DIMS:", sorted(walk_forms))


# ---- the data: wrong rungs are visible at every length --------------------------------------------------------------------------------
def _l2_step_dropped(rows, q):
    w = 4 * (rows.shape[1] // 4)
    return rf.l2_ref(np.ascontiguousarray(rows[:, :w - 4]), q[:w - 4])


def _l2_tail_included(rows, q):
    d = rows.shape[1]
    pad = (-d) % 4
    return rf.l2_ref(np.pad(rows, ((0, 0), (0, pad))), np.pad(q, (0, pad)))


def _dot_last_dropped(rows, q):
    return rf.negdot_ref(np.ascontiguousarray(rows[:, :-1]), q[:-1])


def _dot_step_dropped(rows, q):
    w = 4 * (rows.shape[1] // 4)
    keep = np.r_[0:w - 4, w:rows.shape[1]]
    return rf.negdot_ref(np.ascontiguousarray(rows[:, keep]), q[keep])


# name -> (metric, wrong distance, applies at d, least share of changed bit patterns)
MISTAKES = {
    "l2 one 4-wide step dropped": (0, _l2_step_dropped, lambda d: d >= 4, 0.99),
    "l2 tail included": (0, _l2_tail_included, lambda d: d % 4 != 0, 0.99),
    "dot last coordinate dropped": (1, _dot_last_dropped, lambda d: d >= 1, 0.99),
    "dot one 4-wide step dropped": (1, _dot_step_dropped, lambda d: d >= 4, 0.99),
    "l2 tree fold": (0, rf.l2_tree, lambda d: d >= 4, 0.10),
    "l2 fused multiply-add": (0, rf.l2_fma, lambda d: d >= 8, 0.10),
    "dot left fold": (1, lambda r, q: rf.negdot_ref(r, q, final="left"), lambda d: d >= 4, 0.10),
    "dot fused multiply-add": (1, lambda r, q: rf.negdot_ref(r, q, fma=True), lambda d: d >= 16, 0.10),
}


def test_restatements_equal_the_oracle_and_mistakes_show_at_every_length(orc):
    least = {name: (2.0, None) for name in MISTAKES}
    for d in ds.DIMS:
        rng = ds.rng_of(3, d)
        rows, q = datagen.full_mantissa(rng, 512, d), datagen.full_mantissa(rng, 1, d)[0]
        want = {0: rf.l2_ref(rows, q), 1: rf.negdot_ref(rows, q)}
        for metric, fn in ((0, orc.l2), (1, orc.negdot)):
            got = np.array([fn(r, q) for r in rows], F32)
            assert np.array_equal(gu.bits(want[metric]), gu.bits(got)), ("restatement", metric, d)
        if d < 4:
            assert (gu.bits(want[0]) == 0).all(), d    # no step runs: +0, bit for bit
        for name, (metric, wrong, applies, bar) in MISTAKES.items():
            if not applies(d):
                continue
            share = float((gu.bits(wrong(rows, q)) != gu.bits(want[metric])).mean())
            if share < least[name][0]:
                least[name] = (share, d)
            assert share >= bar, (name, d, share)
    for name, (share, d) in least.items():
        print("dim sweep, %s: least share of changed distance bits %.3f (d = %d)" % (name, share, d))


@pytest.mark.parametrize("d", (1, 2, 3))
def test_below_one_step_l2_is_decided_by_the_tie_rules(orc, d):
    """d < 4 under L2: every distance is +0 -- the scan returns the lowest ids, the re-rank the first candidate in pop order."""
    v = ds.vectors(d)
    ids, dist = orc.exact_knn(v["base"], v["queries"], 20, 0, threads=4)
    assert np.array_equal(ids, np.tile(np.arange(20, dtype=np.uint32), (ds.NQ, 1))) and (gu.bits(dist) == 0).all()
    cand, count = ds.candidates()
    some = count > 0
    assert np.array_equal(orc.rerank(v["queries"][some], cand[some], count[some], v["base"], metric=0, threads=4), cand[some, 0])
    assert len(np.unique(cand[some][:, :1])) > 1


def test_byte_contest_is_decided_by_the_order_of_the_roundings(g, orc):
    """dim_sweep.byte_contest at every chunk-pair length of DIMS: the restatement on the widened rows is the oracle's distance; a group's rows
    are permutations of one vector (equidistant from a constant query in real arithmetic); and from d = 32 on at least 90 % of the candidate
    lists with 31 and more entries hold two or more distinct float32 distances, so a re-rank that sums in another order picks other rows."""
    for d in ds.DIMS:
        if ds.rerank_form(g, 0, d, bytes=True)[0] != "chunk_pairs":
            continue
        base, gq = ds.byte_contest(d)
        cand, count, qg = ds.contest_candidates(128, 8, d)
        wide = base.astype(F32)
        assert all(np.array_equal(np.sort(base[r]), np.sort(base[r // 128 * 128])) for r in range(0, len(base), 17))
        got = np.array([orc.l2(r, gq[0]) for r in wide[:128]], F32)
        assert np.array_equal(gu.bits(rf.l2_ref(wide[:128], gq[0])), gu.bits(got)), d
        long = [i for i in range(ds.NQ) if count[i] >= 31]
        distinct = [len(np.unique(gu.bits(rf.l2_ref(wide[cand[i, :count[i]]], gq[qg[i]])))) for i in long]
        share = float(np.mean([n >= 2 for n in distinct]))
        print("byte contest d=%d: distinct distances per list %d..%d, lists with >= 2: %.3f" % (d, min(distinct), max(distinct), share))
        assert d < 32 or share >= 0.9, (d, share)
