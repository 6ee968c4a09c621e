#!/usr/bin/env python3
"""Times gbnns_exact_knn_half under the negative dot with the K-looped f16 matrix-core filter ("knn_half_dot" = 2, knn_half_dot.hip) against
the same call with the knob at 0 (the half-row exact scan, the only path before the knob existed) and against gbnns_exact_knn with
"knn_filter_dot" = 2 on the widened float32 copy of the same rows (knn_dot.hip), in one run, interleaved, device buffers.  The classes are
tools/knn_dot_timing.py's:

  gist batch   10^5 x 960, 10 000 queries, k = 100
  gist truth   10^6 x 960, 1 000 queries, k = 1, 10, 100
  glove        10^6 x 200, 10 000 queries, k = 100
  deep         10^6 x 96, 10 000 queries, k = 100, rows normalised before they are rounded to binary16, queries normalised
  gist lists   the 48-NN lists of 10^5 x 960 over itself

Per case: a warm-up of the three calls -- every output byte of the three compared --, then REPS rounds of (half scan, half dot, float dot),
each timed by a host clock around the call (it returns behind a synchronisation of its stream).  Reported: the median and the spread
(max - min) of each, the ratio of the half dot call to the half scan and to the float dot call, and the f16 matrix work of the half dot
call (2 products x 2 n n_q dp flops) over its WHOLE call time as a share of the MI355X's dense f16 peak -- an end-to-end figure that
includes the row norms, the query split, the exact scan of the first rows, the rescoring and the selection.  The verdict line is the rule
the by-size value 1 of the knob follows: the half dot call must beat the half scan by more than that scan's own spread.  --case picks
cases by the first words of their names, comma separated.  Needs a HIP device; writes to stdout (profiles/knn_half_dot_timing.txt is a
copy)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402

PEAK_F16_DENSE = 2.5e15   # flop/s, the MI355X's published dense f16 matrix rate
NEG_DOT = 1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def knobs(half_dot, float_dot):
    lib = g.load_library()
    assert lib.gbnns_debug_knob(b"knn_half_dot", half_dot) == 0 and lib.gbnns_debug_knob(b"knn_filter_dot", float_dot) == 0


def same(a, b):
    return bool((a[0] == b[0]).all()) and bool((a[1].view(torch.int32) == b[1].view(torch.int32)).all())


def case(name, n, d, nq, k, reps, self_lists=False, normalised=False, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
    if normalised:
        base = base / base.norm(dim=1, keepdim=True)
    base = base.half()
    wide_base = base.float()   # the copy a caller without this path has to hold
    q = wide_base if self_lists else torch.randn((nq, d), generator=gen, device="cuda", dtype=torch.float32)
    if normalised and not self_lists:
        q = q / q.norm(dim=1, keepdim=True)
    so = 0 if self_lists else -1
    calls = [("half scan", (0, 0), base), ("half dot", (2, 0), base), ("float dot", (0, 2), wide_base)]
    run = lambda rows: g.exact_knn(rows, q, k, NEG_DOT, self_offset=so, want_dist=True)
    times, outs = {what: [] for what, _, _ in calls}, {}
    try:
        for what, kn, rows in calls:
            knobs(*kn)
            if what == "half dot":
                plan = g.knn_half_plan(n, len(q), d, k, NEG_DOT)
            outs[what] = run(rows)
        for _ in range(reps):
            for what, kn, rows in calls:
                knobs(*kn)
                times[what].append(timed(lambda: run(rows))[0])
    finally:
        knobs(0, 0)
    med = {w: statistics.median(t) for w, t in times.items()}
    spread = {w: max(t) - min(t) for w, t in times.items()}
    dp = (d + 15) // 16 * 16
    print(f"{name:30s} " + "   ".join(f"{w} {med[w]:9.2f} ms (spread {spread[w]:7.2f})" for w in times))
    print(f"{'':30s} {plan['kernel']}, packed {plan['packed']}   half dot / half scan {med['half dot'] / med['half scan']:5.3f}   "
          f"half dot / float dot {med['half dot'] / med['float dot']:5.3f}   f16 matrix work over the whole call: "
          f"{100 * 4.0 * n * len(q) * dp / (med['half dot'] * 1e-3) / PEAK_F16_DENSE:4.1f} % of peak")
    beats = med["half scan"] - med["half dot"] > spread["half scan"]
    print(f"{'':30s} every output byte the same: half dot / half scan {same(outs['half dot'], outs['half scan'])}, "
          f"float dot / half scan {same(outs['float dot'], outs['half scan'])}   verdict: half dot "
          f"{'beats' if beats else 'does not beat'} the half scan by more than the scan's spread", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a rehearsal)")
    ap.add_argument("--case", default="", help="only the cases whose name starts with one of these, comma separated")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    s = 10 if a.small else 1
    print(f"knn_half_dot_timing: {torch.cuda.get_device_name(0)}, reps {a.reps}, gbnns {g.version()}", flush=True)
    cases = [("batch 1e5x960 nq 1e4 k 100", 10**5 // s, 960, 10**4, 100, a.reps)]
    cases += [(f"truth 1e6x960 nq 1e3 k {k}", 10**6 // s, 960, 10**3, k, a.reps) for k in (1, 10, 100)]
    cases += [("glove 1e6x200 nq 1e4 k 100", 10**6 // s, 200, 10**4, 100, a.reps),
              ("deep 1e6x96 nq 1e4 k 100 unit", 10**6 // s, 96, 10**4, 100, a.reps, False, True),
              ("lists 1e5x960 self k 48", 10**5 // s, 960, 0, 48, max(2, a.reps // 2), True)]
    for c in cases:
        if any(c[0].startswith(p) for p in a.case.split(",")):
            case(*c)


if __name__ == "__main__":
    main()
