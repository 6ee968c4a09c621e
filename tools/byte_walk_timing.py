"""What the byte-row PLAIN walk (MODE_PLAIN with FLAG_BYTE_WALK on a byte handle) costs, measured against the float handle's PLAIN walk over
the same widened table in the same run, on the sift-shaped synthetic workload of bench.py (synth.make_dataset, the same recipe and cache
file).

The byte table is the workload's base set quantised to uint8 (round(128 + 256 x), clamped), the queries likewise (integer-valued floats, as
SIFT's are); the float handle holds that table widened to float32.  Both handles share the workload's graph; the searches are PLAIN ones with
k = 1 -- the hnsw half of the reference's final_test -- at the reference's sift efs_hnsw points 20, 64, 140 plus 200.

  walk_ms    gbnns_profile's (events around the stage), with the kernel each handle took: float32 against bytes, alone (profiling
             serialises the kernels of a call)
  in flight  wall time per batch of GBNNS_FLAG_DEFER_JOIN searches with three batches in flight (no profiling), ef 64
  answers    that differ between the two handles (the contract: 0)
  recall@1   of both handles against the workload's ground truth (the exact neighbour of the unquantised query among the unquantised rows)
  bytes      device bytes of each handle's original-space table

Interleaved rounds, the median of the rounds' per-call means with the lowest and highest round beside it.  No threshold: a row where the
byte handle is slower says so.  The yardstick is the float handle's walk in the same run, never the new code against itself.

    python tools/byte_walk_timing.py [--cache-dir DIR] [--n N] [--out FILE]
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
BEAMS = (20, 64, 140, 200)
FLAGS = {"float32": 0, "bytes": g.FLAG_BYTE_WALK}


def quantise(x):
    return torch.clamp(torch.round(x * 256.0 + 128.0), 0, 255).to(torch.uint8).contiguous()


def search(name, ix, q, ef, **kw):
    return ix.search(q, ef, mode=g.MODE_PLAIN, k=1, want=kw.pop("want", ()), flags=FLAGS[name] | kw.pop("flags", 0), **kw)


def profiled(handles, q, ef):
    """{name: per-call means of walk_ms over the rounds}, {name: first-pass kernel}, the handles interleaved."""
    for name, ix in handles.items():
        for _ in range(WARMUP):
            search(name, ix, q, ef)
    torch.cuda.synchronize()
    rounds = {name: [] for name in handles}
    kernel = {}
    for _ in range(REPEATS):
        for name, ix in handles.items():
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(CALLS):
                search(name, ix, q, ef)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            rounds[name].append(p["walk_ms"] / p["calls"])
            kernel[name] = p["walk_kernel"].split(" (")[0] + (" + %d queries on the general kernel" % p["general_queries"] if p["general_queries"] else "")
    return rounds, kernel


def in_flight(handles, q, ef):
    """{name: wall ms per batch over the rounds}: CALLS deferred calls, three batches in flight, joined and synchronised."""
    rounds = {name: [] for name in handles}
    for rep in range(REPEATS + 1):
        for name, ix in handles.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = [search(name, ix, q, ef, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for _ in range(2 * CALLS)]
            ix.join()
            torch.cuda.synchronize()
            if rep:   # (the first round warms up)
                rounds[name].append((time.perf_counter() - t0) * 1e3 / (2 * CALLS))
            del outs
    return rounds


def row(lines, rec, key, what, rounds, kernel=None):
    rec[key] = {}
    for name in ("float32", "bytes"):
        v = rounds[name]
        rec[key][name] = {"ms": round(statistics.median(v), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}
        if kernel:
            rec[key][name]["kernel"] = kernel[name]
        lines.append("  %-9s %-8s %.4f [%.4f .. %.4f] ms  %s" % (what, name, statistics.median(v), min(v), max(v), kernel[name] if kernel else ""))
    rec[key]["bytes_over_float32"] = round(rec[key]["bytes"]["ms"] / rec[key]["float32"]["ms"], 3)
    lines.append("  %-9s bytes / float32 %.3f" % (what, rec[key]["bytes_over_float32"]))


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
    base_f = base_u8.to(torch.float32).contiguous()
    q = quantise(ds.queries).to(torch.float32).contiguous()
    handles = {"float32": g.Index(base_f, ds.graph_off, ds.graph_nbr, db_low=ds.db_low),
               "bytes": g.Index(base_u8, ds.graph_off, ds.graph_nbr, db_low=ds.db_low)}
    assert handles["bytes"].is_bytes and not handles["float32"].is_bytes
    table = {"float32": base_f.numel() * 4, "bytes": base_u8.numel()}
    lines = ["per call: median of %d rounds of %d calls [lowest .. highest]; float32 = Index(db.float()), bytes = Index(db uint8) with FLAG_BYTE_WALK, the same table" % (REPEATS, CALLS),
             "sift-shaped  n %d  %d queries  d %d  PLAIN, k = 1" % (kw["n"], kw["nq"], kw["d"]),
             "original-space table on the device: float32 %d bytes, bytes %d bytes" % (table["float32"], table["bytes"])]
    records = {"n": kw["n"], "nq": kw["nq"], "table_bytes": table, "beams": []}
    gt = ds.gt.to(torch.int64)
    for ef in BEAMS:
        rec = {"ef": ef}
        lines.append("ef %d" % ef)
        rounds, kernel = profiled(handles, q, ef)
        row(lines, rec, "walk_ms", "walk_ms", rounds, kernel)
        if ef == 64:
            row(lines, rec, "in_flight_ms", "in flight", in_flight(handles, q, ef))
        res = {name: search(name, ix, q, ef, want=("dist_calc",)) for name, ix in handles.items()}
        torch.cuda.synchronize()
        ids = {name: r["ids"].to(torch.int64) for name, r in res.items()}
        rec["answers_that_differ"] = int((ids["float32"] != ids["bytes"]).sum().item())
        rec["recall_at_1"] = {name: round(float((v[:len(gt)] == gt).float().mean().item()), 4) for name, v in ids.items()}
        rec["dist_calc_mean"] = round(float(res["bytes"]["dist_calc"].float().mean().item()), 1)
        # row bytes a hop's gathers ask for (every computed distance reads one row), per second of walk_ms
        for name, row_bytes in (("float32", kw["d"] * 4), ("bytes", kw["d"])):
            rec["walk_ms"][name]["row_TBps"] = round(rec["dist_calc_mean"] * kw["nq"] * row_bytes / (rec["walk_ms"][name]["ms"] * 1e-3) / 1e12, 3)
        lines.append("  answers that differ %d of %d; recall@1 float32 %.4f bytes %.4f; %.1f distances per query; row bytes float32 %.2f TB/s, bytes %.2f TB/s"
                     % (rec["answers_that_differ"], kw["nq"], rec["recall_at_1"]["float32"], rec["recall_at_1"]["bytes"], rec["dist_calc_mean"],
                        rec["walk_ms"]["float32"]["row_TBps"], rec["walk_ms"]["bytes"]["row_TBps"]))
        records["beams"].append(rec)
    for ix in handles.values():
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
