"""What gbnns_exact_knn_bytes costs, measured against gbnns_exact_knn on the widened copy of the same data in the same run.

SIFT-shaped uniform random bytes, n = 10^6, d = 128, everything in device buffers (the byte call holds a quarter of the float call's bytes
and, from host buffers, uploads a quarter; neither is part of the times below):

  truth     ground truth for 10 000 queries, k = 1 and k = 100 (getTruth; recall of a byte index)
  self-48   the 48-NN lists of the set over itself, in query slices with self_offset (the lists a graph is built from)
  self-1000 1 000-NN lists for 2^16 of its rows (the reference's graph builder reads 1 000-NN lists)

Per job: wall time of both calls (the calls return when the work is done; interleaved rounds, the median with the lowest and highest round
beside it), the ratio, pairs per second of the byte call, the int8 matrix-pipe utilisation its time implies -- the sweep issues one
v_mfma_i32_32x32x32_i8 (32 cycles on a SIMD) per 32 rows x 32 queries x 32 dimensions, counted once per pair, against SIMDs x clock --
and whether every output byte (ids and distance bits) of the two calls agrees.  No threshold: a row where the byte call is slower says so.
The yardstick is the float call in the same run, never the new code against itself.

    python tools/knn_bytes_timing.py [--n N] [--self-slices S] [--rounds R] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402

D = 128
SLICE = 1 << 16
MFMA_CYCLES, MFMA_K, TILE = 32, 32, 32 * 32


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def job(name, pairs, rounds, run_bytes, run_float, simds, clock_hz, lines):
    tb, tf, agree = [], [], True
    for _ in range(rounds):
        t, ob = timed(run_bytes)
        tb.append(t)
        t, of = timed(run_float)
        tf.append(t)
        agree = agree and all(same(x, y) for x, y in zip(ob, of))
        del ob, of
    mb, mf = statistics.median(tb), statistics.median(tf)
    pipe_s = pairs / TILE * (D // MFMA_K) * MFMA_CYCLES / (simds * clock_hz)
    lines.append(f"{name:<34} bytes {mb * 1e3:9.1f} ms [{min(tb) * 1e3:.1f} .. {max(tb) * 1e3:.1f}]   float {mf * 1e3:9.1f} ms "
                 f"[{min(tf) * 1e3:.1f} .. {max(tf) * 1e3:.1f}]   float / bytes {mf / mb:5.2f}   {pairs / mb:.3e} pairs/s   "
                 f"int8 pipe {100 * pipe_s / mb:5.1f} %   outputs {'identical' if agree else 'DIFFER'}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--self-slices", type=int, default=0, help="query slices of 2^16 rows of the self-48 job (0 = the whole set)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_bytes_timing.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    simds = 4 * props.multi_processor_count
    clock_hz = props.clock_rate * 1e3 if hasattr(props, "clock_rate") else 2.4e9
    gen = torch.Generator(device="cpu").manual_seed(1)
    base = torch.randint(0, 256, (a.n, D), dtype=torch.uint8, generator=gen).to(dev)
    queries = torch.randint(0, 256, (10_000, D), dtype=torch.uint8, generator=gen).to(dev)
    wide, wq = base.float(), queries.float()
    lines = [f"knn_bytes_timing: {props.name}, {simds} SIMDs at {clock_hz / 1e9:.2f} GHz (the clock the device reports), n = {a.n}, d = {D}, "
             f"uniform random bytes; device buffers; median of {a.rounds} interleaved rounds [lowest .. highest]"]
    print(lines[0], flush=True)
    # warm-up: first launches, code-object load
    g.exact_knn(base[:4096].contiguous(), queries[:256].contiguous(), 10)
    g.exact_knn(wide[:4096].contiguous(), wq[:256].contiguous(), 10)
    for k in (1, 100):
        job(f"truth 10 000 queries k = {k}", 10_000 * a.n, a.rounds,
            lambda: [g.exact_knn(base, queries, k, want_dist=True)], lambda: [g.exact_knn(wide, wq, k, want_dist=True)], simds, clock_hz, lines)
    starts = list(range(0, a.n, SLICE))
    if a.self_slices:
        starts = starts[:a.self_slices]
    rows = sum(min(SLICE, a.n - s) for s in starts)

    def self_knn(table, k, st):
        return [g.exact_knn(table, table[s:s + SLICE], k, self_offset=s, want_dist=True) for s in st]
    job(f"self-48, {rows} of its rows", rows * a.n, 1, lambda: self_knn(base, 48, starts), lambda: self_knn(wide, 48, starts), simds, clock_hz, lines)
    job("self-1000, 2^16 of its rows", min(SLICE, a.n) * a.n, 1, lambda: self_knn(base, 1000, [0]), lambda: self_knn(wide, 1000, [0]), simds, clock_hz,
        lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
