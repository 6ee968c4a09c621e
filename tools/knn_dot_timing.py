#!/usr/bin/env python3
"""Times gbnns_exact_knn under the negative dot with the K-looped matrix-core filter ("knn_filter_dot" = 2, knn_dot.hip) against the same
call with the knob at 0 (the exact scan, the only path before the knob existed), in one run, interleaved, device buffers.

  gist batch   10^5 x 960, 10 000 queries, k = 100
  gist truth   10^6 x 960, 1 000 queries, k = 1, 10, 100
  glove        10^6 x 200, 10 000 queries, k = 100 (tools/knn_wide_timing.py's class at glove-200's width: the dot form takes d % 8 == 0, not 300)
  gist lists   the 48-NN lists of 10^5 x 960 over itself
  deep         10^6 x 96, 10 000 queries, k = 100, rows and queries normalised (an angular set's ground truth)

Per case: a warm-up of both calls -- every output byte of the two compared --, then REPS rounds of (scan, dot), each timed by a host clock
around the call (it returns behind a synchronisation of its stream).  Reported: the median and the spread (max - min) of each, the ratio of
the medians, the bf16 matrix work of the dot call (3 products x 2 n n_q dp flops) over its WHOLE call time as a share of the MI355X's
dense bf16 peak -- an end-to-end figure that includes packing, the exact scan of the first rows, the rescoring and the selection --, and a
MODEL of the call's chunks: the schedule of knn_rows_call (1 024 first rows, chunks at most as long as everything before them, "knn_chunk",
64 MiB of packed rows) replayed with torch in float32 over all queries -- per chunk the rows a query keeps under its running threshold
plus c |q||x|, c = 2^-10 -- which gives the share of chunks in which some query keeps more than its list of max(256, 4 k + 64) holds (the
call scans such a chunk exactly) and the mean rows kept per query and chunk.  The verdict line is the rule the by-size value 1 of the knob
follows: the dot call must beat the scan by more than the scan's own spread.  Needs a HIP device; writes to stdout
(profiles/knn_dot_timing.txt is a copy)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402

PEAK_BF16_DENSE = 2.5e15   # flop/s, the MI355X's published dense bf16 matrix rate
SLACK = 1.0 / 1024.0       # kKnnWideSlack, the dot filter's c
NEG_DOT = 1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def knob(v):
    assert g.load_library().gbnns_debug_knob(b"knn_filter_dot", v) == 0


def chunk_model(base, q, k, self_lists):
    """(chunks, overflowed chunks, mean rows kept per query and chunk) of the heap-filter schedule, replayed in float32."""
    n, d = base.shape
    dp = (d + 15) // 16 * 16
    cap = max(256, 4 * k + 64)
    max_chunk = min(1 << 15, max(64, (n // 16 + 63) & ~63), max(64, ((64 << 20) // (4 * dp)) & ~63))
    first = min(n, (max(min(max_chunk, 1024), 4 * k) + 63) & ~63)
    qn, bn = q.norm(dim=1), base.norm(dim=1)
    me = torch.arange(len(q), device=q.device)

    def dots(r0, r1, block_rows):
        D = q[block_rows] @ base[r0:r1].T
        if self_lists:   # a query's own row is never offered
            own = me[block_rows] - r0
            ok = (own >= 0) & (own < r1 - r0)
            D[torch.nonzero(ok)[:, 0], own[ok]] = -float("inf")
        return D

    chunks = over = 0
    kept_sum = 0.0
    top = None
    r0 = 0
    while r0 < n:
        rows = first if r0 == 0 else min(max_chunk, r0, n - r0)
        most = torch.zeros((), device=q.device)
        new_top = []
        for b0 in range(0, len(q), 2048):
            block_rows = slice(b0, b0 + 2048)
            D = dots(r0, r0 + rows, block_rows)
            if r0:
                thr = top[block_rows][:, -1:]
                kept = (D + SLACK * qn[block_rows][:, None] * bn[None, r0:r0 + rows] >= thr).sum(1)
                most = torch.maximum(most, kept.max())
                kept_sum += float(kept.sum())
            both = D if top is None else torch.cat((top[block_rows], D), 1)
            new_top.append(torch.topk(both, min(k, both.shape[1]), dim=1).values)
        top = torch.cat(new_top)
        if r0:
            chunks += 1
            over += int(most > cap)
        r0 += rows
    return chunks, over, kept_sum / max(1, chunks) / len(q)


def case(name, n, d, nq, k, reps, self_lists=False, normalised=False, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
    q = base if self_lists else torch.randn((nq, d), generator=gen, device="cuda", dtype=torch.float32)
    if normalised:
        base = base / base.norm(dim=1, keepdim=True)
        q = base if self_lists else q / q.norm(dim=1, keepdim=True)
    so = 0 if self_lists else -1
    run = lambda: g.exact_knn(base, q, k, NEG_DOT, self_offset=so, want_dist=True)
    try:
        knob(0)
        ids_s, dist_s = run()
        knob(2)
        plan = g.knn_plan(False, NEG_DOT, n, len(q), d, k)[0]
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
    chunks, over, kept = chunk_model(base, q, k, self_lists)
    print(f"{name:30s} scan {ms:9.2f} ms (spread {ss:7.2f})   dot {mw:9.2f} ms (spread {sw:7.2f})   ratio {mw / ms:5.3f}   {plan}")
    print(f"{'':30s} every output byte the same: {same}   bf16 matrix work over the whole call: "
          f"{100 * 6.0 * n * len(q) * dp / (mw * 1e-3) / PEAK_BF16_DENSE:4.1f} % of peak")
    print(f"{'':30s} model of the chunks (float32): {over} of {chunks} filtered chunks overflow a list of {max(256, 4 * k + 64)}"
          f" ({100.0 * over / max(1, chunks):.0f} %), {kept:7.1f} rows kept per query and chunk")
    print(f"{'':30s} verdict: dot {'beats' if ms - mw > ss else 'does not beat'} the scan by more than the scan's spread", flush=True)
    return ms - mw > ss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    s = 10 if a.small else 1
    print(f"knn_dot_timing: {torch.cuda.get_device_name(0)}, reps {a.reps}, gbnns {g.version()}", flush=True)
    case("gist 1e5x960 nq 1e4 k 100", 10**5 // s, 960, 10**4, 100, a.reps)
    for k in (1, 10, 100):
        case(f"gist 1e6x960 nq 1e3 k {k}", 10**6 // s, 960, 10**3, k, a.reps)
    case("glove 1e6x200 nq 1e4 k 100", 10**6 // s, 200, 10**4, 100, a.reps)
    case("gist 1e5x960 self lists k 48", 10**5 // s, 960, 0, 48, max(2, a.reps // 2), self_lists=True)
    case("deep 1e6x96 nq 1e4 k 100 unit", 10**6 // s, 96, 10**4, 100, a.reps, normalised=True)


if __name__ == "__main__":
    main()
