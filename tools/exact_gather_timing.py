"""What the gathered exact scan costs beside the scan it may replace: Index.exact_knn(..., gather=True) (gbnns_index_exact_knn_gather) against
Index.exact_knn (gbnns_index_exact_knn) with the same query tags, on the SIFT-shaped synthetic workload of bench.py (synth.make_dataset:
10^6 x 128 -> 32, 10 000 queries), rows and queries quantised to uint8 as in tools/exact_tagged_timing.py so that a float handle (the table
widened) and a byte handle hold the same table.  DEVICE buffers.

Tags: every row draws r uniform in 0 .. 1023 and gets  1 | (r < 512) << 1 | (r < 128) << 2 | (r < 16) << 3 | (r == 0) << 4 ; a query whose
word carries bit 0 / 1 / 2 / 3 / 4 may see all, 1/2, 1/8, 1/64 and 1/1024 of the rows.  The batch carries U = 1, 13 or 10 000 DISTINCT words
of the same fraction: the fraction's bit plus a number in bits 8 .. 23, which no row carries -- so every word allows the same rows, and the
gathered call still builds U lists.  U = 10 000: every group is one query, which uses one thread of a workgroup.

Per (handle, fraction, U, k = 1 and 10): wall ms of both calls, interleaved in the same run on the same handle (each returns when its work
has finished); median of the rounds with the lowest and highest round beside it -- the baseline's own run-to-run spread -- and the ratio
gathered / existing of the medians.  A cell whose first (warm-up) call takes more than SLOW_MS runs SLOW_REPEATS rounds instead of REPEATS;
the line says how many.  The fractions of a (handle, U, k) column run from the smallest up, and once a gathered call has taken more than
--cap-ms (default CAP_MS) the larger fractions of that column are not run -- the gathered call's time grows with the rows it may see, a
column's worst cell is minutes (10 000 lists of 10^6 ids are 150 rounds of 67 one-thread workgroups) -- and say so.  One more gathered call per cell with the handle knob "gather_timing" gives the stage
times (census, fill, scan: HIP events; the rounds of that call run one after the other) and the rounds, and its ids are compared with the
existing call's.  Last, per handle, U and k, the crossover: the largest measured fraction from which on, downwards,
every gathered median is below the existing call's lowest round.  Nothing is asserted: the table is the answer, for this one synthetic tag
recipe on this one device.

    python tools/exact_gather_timing.py [--cache-dir DIR] [--n N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402
from gbnns_dim_red_amd import synth  # noqa: E402

REPEATS, SLOW_REPEATS, SLOW_MS, CAP_MS = 5, 3, 400.0, 1500.0
SHAPE = dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256)
FRACTIONS = (("1", 0, 1024), ("1/2", 1, 512), ("1/8", 2, 128), ("1/64", 3, 16), ("1/1024", 4, 1))   # (name, bit, r below)
DISTINCT = (1, 13, 10_000)
KS = (1, 10)


def quantise(x):
    return torch.clamp(torch.round(x * 256.0 + 128.0), 0, 255).to(torch.uint8).contiguous()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--cap-ms", type=float, default=CAP_MS, help="a gathered call slower than this ends its column (0: run every cell)")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    kw = dict(SHAPE)
    if args.n:
        kw["n"] = args.n
    n, nq = kw["n"], kw["nq"]
    ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
    base_u8 = quantise(ds.base)
    q_u8 = quantise(ds.queries)
    handles = {"float32": g.Index(base_u8.to(torch.float32).contiguous(), ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net),
               "bytes": g.Index(base_u8, ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net)}
    queries = {"float32": q_u8.to(torch.float32).contiguous(), "bytes": q_u8}
    gen = torch.Generator(device="cpu").manual_seed(4321)
    r = torch.randint(0, 1024, (n,), generator=gen)
    tags = torch.zeros(n, dtype=torch.int32)
    for _, bit, below in FRACTIONS:
        tags |= (r < below).to(torch.int32) << bit
    for ix in handles.values():
        ix.set_tags(tags.to("cuda:0"))
    torch.cuda.synchronize()
    lines = ["sift-shaped  n %d  %d queries  d %d (uint8 values; float32 = the table widened)  DEVICE buffers" % (n, nq, kw["d"]),
             "gathered = Index.exact_knn(queries, k, query_tags, gather=True), existing = the same call without gather; wall ms, median of %d rounds "
             "(%d where a call takes more than %.0f ms) [lowest .. highest]; ratio = gathered / existing; stages: one gathered call with "
             "gather_timing, ms by HIP events; a column (handle, U, k) ends above its first gathered call of more than %.0f ms"
             % (REPEATS, SLOW_REPEATS, SLOW_MS, args.cap_ms)]
    for name in handles:
        lines.append("%s: %s, W = %d queries a workgroup" % ((name,) + g.gather_plan(name == "bytes", g.METRIC_L2, kw["d"], 10)))
    records = []
    wins = {}
    ended = {}   # (handle, U, k) -> (fraction, ms) of the gathered call that ended the column
    for hname, ix in handles.items():
        q = queries[hname]
        for fname, bit, _ in reversed(FRACTIONS):
            rows = int(((tags >> bit) & 1).sum())
            for u in DISTINCT:
                words = ((1 << bit) | ((torch.arange(nq, dtype=torch.int64) % u) << 8)).to(torch.int32)
                assert len(torch.unique(words)) == u
                qt = words.to("cuda:0")
                for k in KS:
                    if (hname, u, k) in ended:
                        wins[(hname, u, k, fname)] = False
                        lines.append("%-7s allowed %-6s (%7d rows)  U %-5d k %-2d  not run: the gathered call took %.0f ms at allowed %s already"
                                     % ((hname, fname, rows, u, k) + ended[(hname, u, k)][::-1]))
                        continue
                    fns = {"gathered": lambda: ix.exact_knn(q, k, query_tags=qt, gather=True), "existing": lambda: ix.exact_knn(q, k, query_tags=qt)}
                    first = {v: wall_ms(fn) for v, fn in fns.items()}   # (the warm-up round)
                    rounds = SLOW_REPEATS if max(first.values()) > SLOW_MS else REPEATS
                    if args.cap_ms and first["gathered"] > args.cap_ms:
                        ended[(hname, u, k)] = (fname, first["gathered"])
                    t = {v: [] for v in fns}
                    for rnd in range(rounds):
                        for v, fn in fns.items():
                            t[v].append(wall_ms(fn))
                    ix.knob("gather_timing", 1)
                    ids = fns["gathered"]()
                    ix.knob("gather_timing", 0)
                    same = bool((ids == fns["existing"]()).all())
                    stage = {s: ix.knob_get("gather_%s_us" % s) / 1e3 for s in ("census", "fill", "scan")}
                    n_rounds = ix.knob_get("gather_rounds")
                    med = {v: statistics.median(t[v]) for v in fns}
                    ratio = med["gathered"] / med["existing"]
                    wins[(hname, u, k, fname)] = med["gathered"] < min(t["existing"])
                    lines.append("%-7s allowed %-6s (%7d rows)  U %-5d k %-2d  gathered %9.3f [%9.3f .. %9.3f]  existing %8.3f [%8.3f .. %8.3f]  ratio %7.3f"
                                 "  | census %7.3f fill %8.3f scan %9.3f ms, %d round(s), %d timed rounds%s"
                                 % (hname, fname, rows, u, k, med["gathered"], min(t["gathered"]), max(t["gathered"]), med["existing"], min(t["existing"]),
                                    max(t["existing"]), ratio, stage["census"], stage["fill"], stage["scan"], n_rounds, rounds, "" if same else "  IDS DIFFER"))
                    print("exact_gather_timing:", lines[-1], file=sys.stderr, flush=True)
                    records.append({"handle": hname, "allowed": fname, "rows": rows, "U": u, "k": k, "gathered_ms": round(med["gathered"], 4),
                                    "existing_ms": round(med["existing"], 4), "existing_lowest": round(min(t["existing"]), 4),
                                    "existing_highest": round(max(t["existing"]), 4), "ratio": round(ratio, 4), "stages_ms": stage, "rounds": n_rounds,
                                    "same_ids": same})
    lines.append("crossover: the largest measured fraction from which on, downwards, the gathered median is below the existing call's lowest round")
    for hname in handles:
        for u in DISTINCT:
            for k in KS:
                best = "none"
                for fname, _, _ in reversed(FRACTIONS):
                    if not wins[(hname, u, k, fname)]:
                        break
                    best = fname
                lines.append("  %-7s U %-5d k %-2d  gathered wins at allowed fractions <= %s" % (hname, u, k, best))
    for ix in handles.values():
        ix.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(records))


if __name__ == "__main__":
    main()
