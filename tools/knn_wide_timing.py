#!/usr/bin/env python3
"""Times gbnns_exact_knn on float rows wider than 128 dims with the K-looped matrix-core filter ("knn_filter_wide" = 2, knn_wide.hip)
against the same call with the knob at 0 (the exact scan, the only path before the knob existed), in one run, interleaved, device buffers.

  gist batch   10^5 x 960, 10 000 queries, k = 100 (the README's 785 ms)
  gist truth   10^6 x 960, 1 000 queries, k = 1, 10, 100
  glove        10^6 x 300, 10 000 queries, k = 100
  gist lists   the 48-NN lists of 10^5 x 960 over itself

Per case: a warm-up of both calls -- every output byte of the two compared --, then REPS rounds of (scan, wide), each timed by a host clock
around the call (it returns behind a synchronisation of its stream).  Reported: the median and the spread (max - min) of each, the ratio of
the medians, the bf16 matrix work of the wide call (3 products x 2 n n_q dp flops) over its WHOLE call time as a share of the MI355X's
dense bf16 peak -- an end-to-end figure that includes packing, the exact scan of the first rows, the rescoring and the selection --, and the
share of (query, row) pairs within the slack of the FINAL thresholds (float64, a sample of 64 queries): a lower bound of what the filter
keeps, whose thresholds are looser while the call runs.  The verdict line is the rule the by-size value 1 of the knob follows: the wide
call must beat the scan by more than the scan's own spread.  Needs a HIP device; writes to stdout (profiles/knn_wide_timing.txt is a copy)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402

PEAK_BF16_DENSE = 2.5e15   # flop/s, the MI355X's published dense bf16 matrix rate
SLACK = 1.0 / 1024.0       # kKnnWideSlack


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def knob(v):
    assert g.load_library().gbnns_debug_knob(b"knn_filter_wide", v) == 0


def kept_share(base, q, dist, sample=64):
    """Share of pairs with |q|^2 + |x|^2 - 2 q.x <= T + c (|q|^2 + |x|^2), T the k-th distance returned, over the first `sample` queries."""
    qs, T = q[:sample].double(), dist[:sample, -1].double()
    qn, kept = (qs * qs).sum(1), 0
    for r0 in range(0, base.shape[0], 1 << 16):
        b = base[r0:r0 + (1 << 16)].double()
        S = qn[:, None] + (b * b).sum(1)[None, :]
        kept += int((S - 2.0 * qs @ b.T <= T[:, None] + SLACK * S).sum())
    return kept / (qs.shape[0] * base.shape[0])


def case(name, n, d, nq, k, reps, self_lists=False, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
    q = base if self_lists else torch.randn((nq, d), generator=gen, device="cuda", dtype=torch.float32)
    so = 0 if self_lists else -1
    run = lambda: g.exact_knn(base, q, k, self_offset=so, want_dist=True)
    try:
        knob(0)
        ids_s, dist_s = run()
        knob(2)
        plan = g.knn_plan(False, 0, n, len(q), d, k)[0]
        ids_w, dist_w = run()
        same = bool((ids_s == ids_w).all()) and bool((dist_s.view(torch.int32) == dist_w.view(torch.int32)).all())
        ts, tw = [], []
        for _ in range(reps):
            knob(0)
            ts.append(timed(run)[0])
            knob(2)
            tw.append(timed(run)[0])
    finally:
        knob(0)
    ms, mw = statistics.median(ts), statistics.median(tw)
    ss, sw = max(ts) - min(ts), max(tw) - min(tw)
    dp = (d + 15) // 16 * 16
    print(f"{name:30s} scan {ms:9.2f} ms (spread {ss:7.2f})   wide {mw:9.2f} ms (spread {sw:7.2f})   ratio {mw / ms:5.3f}   {plan}")
    print(f"{'':30s} every output byte the same: {same}   bf16 matrix work over the whole call: "
          f"{100 * 6.0 * n * len(q) * dp / (mw * 1e-3) / PEAK_BF16_DENSE:4.1f} % of peak   "
          f"pairs within the slack of the final thresholds: {100 * kept_share(base, q, dist_w):6.3f} %")
    print(f"{'':30s} verdict: wide {'beats' if ms - mw > ss else 'does not beat'} the scan by more than the scan's spread")
    return ms - mw > ss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    s = 10 if a.small else 1
    print(f"knn_wide_timing: {torch.cuda.get_device_name(0)}, reps {a.reps}, gbnns {g.version()}")
    case("gist 1e5x960 nq 1e4 k 100", 10**5 // s, 960, 10**4, 100, a.reps)
    for k in (1, 10, 100):
        case(f"gist 1e6x960 nq 1e3 k {k}", 10**6 // s, 960, 10**3, k, a.reps)
    case("glove 1e6x300 nq 1e4 k 100", 10**6 // s, 300, 10**4, 100, a.reps)
    case("gist 1e5x960 self lists k 48", 10**5 // s, 960, 0, 48, max(2, a.reps // 2), self_lists=True)


if __name__ == "__main__":
    main()
