#!/usr/bin/env python3
"""Times gbnns_exact_knn_half against gbnns_exact_knn on the widened copy of the same table, in one run, interleaved, device buffers.

  deep shape  10^6 x 96 binary16 rows: ground truth for 10 000 queries at k = 1 and k = 100, and the 48-NN self lists (every row a query)
  gist shape  10^5 x 960: the scan path only (d > 128)

Per case: a warm-up of both calls, then REPS rounds of (float call, half call), each timed by a host clock around the call (it returns
behind a synchronisation of its stream).  Reported: the median and the spread (max - min) of each call, the ratio of the medians, and --
for the swept cases -- the f16 matrix-core work of the half call (2 products x 2 n n_q dp flops) over its WHOLE call time as a share of
the MI355X's dense f16 peak: an end-to-end figure that includes the exact scan of the first rows, the rescoring and the selection, not
the sweep kernel's own share.  The verdict line is the rule the by-size default of knn_half_plan follows: the half call must beat the
float call by more than the float call's own spread.  Needs a HIP device; writes to stdout (profiles/knn_half_timing.txt is a copy)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402

PEAK_F16_DENSE = 2.5e15   # flop/s, the MI355X's published dense f16 matrix rate


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def case(name, n, d, nq, k, reps, self_lists=False, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    half = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    wide = half.to(torch.float32)
    q = wide if self_lists else torch.randn((nq, d), generator=gen, device="cuda", dtype=torch.float32)
    so = 0 if self_lists else -1
    run_f = lambda: g.exact_knn(wide, q, k, self_offset=so)
    run_h = lambda: g.exact_knn(half, q, k, self_offset=so)
    same = bool((run_f() == run_h()).all())   # (the warm-up of both, and the contract once more)
    tf, th = [], []
    for _ in range(reps):
        tf.append(timed(run_f))
        th.append(timed(run_h))
    mf, mh = statistics.median(tf), statistics.median(th)
    sf, sh = max(tf) - min(tf), max(th) - min(th)
    plan = g.knn_half_plan(n, len(q), d, k)
    line = f"{name:28s} float {mf:9.2f} ms (spread {sf:7.2f})   half {mh:9.2f} ms (spread {sh:7.2f})   ratio {mh / mf:5.3f}   {plan['kernel']}"
    if plan["path"] != "scan":
        dp = (d + 15) // 16 * 16
        line += f"   f16 matrix work over the whole call: {100 * 4.0 * n * len(q) * dp / (mh * 1e-3) / PEAK_F16_DENSE:4.1f} % of peak"
    print(line)
    print(f"{'':28s} same ids: {same}   verdict: half {'beats' if mf - mh > sf else 'does not beat'} float by more than float's spread")
    return mf - mh > sf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    s = 10 if a.small else 1
    print(f"knn_half_timing: {torch.cuda.get_device_name(0)}, reps {a.reps}, gbnns {g.version()}")
    case("deep 1e6x96 nq 1e4 k 1", 10**6 // s, 96, 10**4, 1, a.reps)
    case("deep 1e6x96 nq 1e4 k 100", 10**6 // s, 96, 10**4, 100, a.reps)
    case("deep 1e6x96 self lists k 48", 10**6 // s, 96, 0, 48, max(2, a.reps // 2), self_lists=True)
    case("gist 1e5x960 nq 1e4 k 100", 10**5 // s, 960, 10**4, 100, a.reps)


if __name__ == "__main__":
    main()
