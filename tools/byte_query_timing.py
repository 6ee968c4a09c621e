"""What byte queries on a byte handle (Index.search(queries=<uint8>), gbnns_search_byte_queries) cost in PLAIN mode, measured against the call
they replace -- the float-query FLAG_BYTE_WALK search on the SAME handle with the widened queries, the path a user of a byte handle had before
-- in the same process, interleaved, on the sift-shaped synthetic workload of bench.py (synth.make_dataset, the same recipe and cache file;
rows and queries quantised to uint8 as in tools/byte_walk_timing.py).  10 000-query batches, k = 1, the reference's sift efs_hnsw points 20, 64,
140 plus 200, and 100 for the two-register class: two beams of the one-register class, one of the two-register class, two of the two-list class.

Four arms, one handle, round-robin:
  float32        the baseline: float queries, walk_reg*_bytes_kernel (float arithmetic on widened bytes, the query in LDS)
  float32 again  the baseline a second time: the difference of the two medians is the run-to-run spread a gain has to beat
  u8 integer     byte queries, knob byte_query_int = 7: the widening kernel + beam_u8_* (integer arithmetic, the query in registers)
  u8 widened     byte queries, knob byte_query_int = 0: the widening kernel + the baseline's kernel (what the widening alone costs or saves)

  walk_ms    gbnns_profile's (events around the first pass + hand-overs), alone (profiling serialises the kernels of a call)
  widen_ms   gbnns_profile's project_ms, which in a PLAIN call is the widening kernel (0 for float queries)
  alone      wall ms per batch of synchronous DEVICE calls, no profiling
  in flight  wall ms per batch of GBNNS_FLAG_DEFER_JOIN calls, three batches in flight, no profiling
  answers    that differ from the baseline's (the contract: 0), ids and dist_calc

Interleaved rounds; the median of the rounds' per-call means with the lowest and highest round beside it.  The decision rule, applied per beam
class and printed with the numbers: the integer first pass is the default where (walk_ms + widen_ms) of "u8 integer" is below the baseline's
walk_ms by more than the spread, at every beam of the class measured.

    python tools/byte_query_timing.py [--cache-dir DIR] [--n N] [--out FILE]
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

REPEATS, CALLS, WARMUP = 7, 5, 3
SHAPE = dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256)
BEAMS = (20, 64, 100, 140, 200)
CLASS_OF = {20: "R = 1 (ef <= 64)", 64: "R = 1 (ef <= 64)", 100: "R = 2 (ef <= 128)", 140: "two-list (ef <= 1 024)", 200: "two-list (ef <= 1 024)"}
ARMS = ("float32", "float32 again", "u8 integer", "u8 widened")
KNOB = {"float32": 7, "float32 again": 7, "u8 integer": 7, "u8 widened": 0}


def quantise(x):
    return torch.clamp(torch.round(x * 256.0 + 128.0), 0, 255).to(torch.uint8).contiguous()


def search(ix, arm, q, ef, **kw):
    ix.knob("byte_query_int", KNOB[arm])
    return ix.search(q["u8" if arm.startswith("u8") else "f32"], ef, mode=g.MODE_PLAIN, k=1, want=kw.pop("want", ()),
                     flags=g.FLAG_BYTE_WALK | kw.pop("flags", 0), **kw)


def profiled(ix, q, ef):
    """{arm: per-call means of walk_ms over the rounds}, the same for widen_ms, {arm: first-pass kernel}; the arms interleaved."""
    for arm in ARMS:
        for _ in range(WARMUP):
            search(ix, arm, q, ef)
    torch.cuda.synchronize()
    walk, widen, kernel = {a: [] for a in ARMS}, {a: [] for a in ARMS}, {}
    for _ in range(REPEATS):
        for arm in ARMS:
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(CALLS):
                search(ix, arm, q, ef)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            walk[arm].append(p["walk_ms"] / p["calls"])
            widen[arm].append(p["project_ms"] / p["calls"])
            kernel[arm] = p["walk_kernel"].split(" (")[0] + (" + %d queries on the general kernel" % p["general_queries"] if p["general_queries"] else "")
    return walk, widen, kernel


def wall(ix, q, ef, deferred):
    """{arm: wall ms per batch over the rounds}: 2 * CALLS calls, synchronous or three batches in flight, then joined and synchronised."""
    rounds = {a: [] for a in ARMS}
    for rep in range(REPEATS + 1):
        for arm in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if deferred:
                outs = [search(ix, arm, q, ef, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for _ in range(2 * CALLS)]
                ix.join()
            else:
                outs = [search(ix, arm, q, ef, out={}) for _ in range(2 * CALLS)]
            torch.cuda.synchronize()
            if rep:   # (the first round warms up)
                rounds[arm].append((time.perf_counter() - t0) * 1e3 / (2 * CALLS))
            del outs
    return rounds


def med(v):
    return {"ms": round(statistics.median(v), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    kw = dict(SHAPE)
    if args.n:
        kw["n"] = args.n
    ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
    base_u8 = quantise(ds.base)
    q = {"u8": quantise(ds.queries)}
    q["f32"] = q["u8"].to(torch.float32).contiguous()
    ix = g.Index(base_u8, ds.graph_off, ds.graph_nbr, db_low=ds.db_low)
    assert ix.is_bytes
    lines = ["per call: median of %d rounds of %d calls [lowest .. highest]; one byte handle, PLAIN with FLAG_BYTE_WALK, k = 1; arms interleaved" % (REPEATS, CALLS),
             "sift-shaped  n %d  %d queries  d %d; query bytes per batch: float32 %d, uint8 %d" % (kw["n"], kw["nq"], kw["d"], q["f32"].numel() * 4, q["u8"].numel())]
    records = {"n": kw["n"], "nq": kw["nq"], "beams": []}
    verdict = {}
    for ef in BEAMS:
        rec = {"ef": ef, "class": CLASS_OF[ef]}
        lines.append("ef %d  (%s)" % (ef, CLASS_OF[ef]))
        walk, widen, kernel = profiled(ix, q, ef)
        alone, flight = wall(ix, q, ef, False), wall(ix, q, ef, True)
        for arm in ARMS:
            rec[arm] = {"walk_ms": med(walk[arm]), "widen_ms": med(widen[arm]), "alone_ms": med(alone[arm]), "in_flight_ms": med(flight[arm]), "kernel": kernel[arm]}
            r = rec[arm]
            lines.append("  %-13s walk_ms %.4f [%.4f .. %.4f]  widen_ms %.4f  alone %.4f [%.4f .. %.4f]  in flight %.4f [%.4f .. %.4f]  %s"
                         % (arm, r["walk_ms"]["ms"], r["walk_ms"]["lowest"], r["walk_ms"]["highest"], r["widen_ms"]["ms"], r["alone_ms"]["ms"],
                            r["alone_ms"]["lowest"], r["alone_ms"]["highest"], r["in_flight_ms"]["ms"], r["in_flight_ms"]["lowest"], r["in_flight_ms"]["highest"],
                            kernel[arm]))
        base = rec["float32"]["walk_ms"]["ms"]
        spread = abs(base - rec["float32 again"]["walk_ms"]["ms"])
        cost = rec["u8 integer"]["walk_ms"]["ms"] + rec["u8 integer"]["widen_ms"]["ms"]
        rec["baseline_spread_ms"] = round(spread, 5)
        rec["integer_plus_widen_over_baseline"] = round(cost / base, 3)
        rec["alone_over_baseline"] = round(rec["u8 integer"]["alone_ms"]["ms"] / rec["float32"]["alone_ms"]["ms"], 3)
        rec["in_flight_over_baseline"] = round(rec["u8 integer"]["in_flight_ms"]["ms"] / rec["float32"]["in_flight_ms"]["ms"], 3)
        rec["integer_wins"] = bool(cost < base - spread)
        verdict.setdefault(CLASS_OF[ef], []).append(rec["integer_wins"])
        res = {arm: search(ix, arm, q, ef, want=("dist_calc",)) for arm in ARMS}
        torch.cuda.synchronize()
        rec["answers_that_differ"] = {arm: int((res[arm]["ids"] != res["float32"]["ids"]).sum().item()) +
                                      int((res[arm]["dist_calc"] != res["float32"]["dist_calc"]).sum().item()) for arm in ARMS[1:]}
        lines.append("  baseline spread %.4f ms; (integer walk_ms + widen_ms) / baseline walk_ms %.3f; wall alone %.3f, in flight %.3f of the baseline's; integer wins: %s"
                     % (spread, rec["integer_plus_widen_over_baseline"], rec["alone_over_baseline"], rec["in_flight_over_baseline"], rec["integer_wins"]))
        lines.append("  answers (ids, dist_calc) that differ from the baseline's: %s" % rec["answers_that_differ"])
        records["beams"].append(rec)
    records["default_by_class"] = {c: all(v) for c, v in verdict.items()}
    lines.append("decision (integer first pass by default where it wins at every measured beam of the class): %s" % records["default_by_class"])
    ix.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(records) + "\n")
    print(json.dumps(records))


if __name__ == "__main__":
    main()
