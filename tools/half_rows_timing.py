"""What GBNNS_FLAG_HALF_ROWS does to the walk, measured: walk_ms of flagged against unflagged searches on the synthetic workloads of
bench.py's rows (synth.make_dataset, the same recipes and cache files).

  workload  n          queries  shape      beam
  sift      10^6       10 000   128 -> 32  ef 64, and ef 36 (its recall gate)
  deep      10^6       10 000    96 -> 48  ef 40
  gist      10^6        1 000   960 -> 64  ef 200
  glove     10^6       10 000   300 -> 144 ef 300            (bench.py --config glove1m)

Per row: walk_ms from gbnns_profile (events around the stage; profiling serialises the kernels; the fused re-rank is part of it in both
variants), flagged and unflagged on the SAME handle in the same run, the variants interleaved -- REPEATS rounds of CALLS calls each after a
warm-up, the figure is the median over the rounds of the per-call mean, with the lowest and highest round beside it --; the two
first-pass kernels; the row bytes a query gathers (dist_calc x bytes of a walked row: 2 a coordinate in a half kernel, else 4); recall@1 of both against
gbnns_exact_knn in the original space; and how many answers of the batch differ between the two.  The unflagged path is what every
search without the flag runs.  No threshold: a row where the half walk is slower says so.

    python tools/half_rows_timing.py [--cache-dir DIR] [--only sift,deep,gist,glove] [--n N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gbnns_dim_red_amd as g  # noqa: E402
from gbnns_dim_red_amd import synth  # noqa: E402

REPEATS, CALLS, WARMUP = 9, 10, 5
WORKLOADS = [
    ("sift", dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256), (64, 36)),
    ("deep", dict(n=1_000_000, nq=10_000, d=96, d_low=48, d_hidden=128), (40,)),
    ("gist", dict(n=1_000_000, nq=1_000, d=960, d_low=64, d_hidden=1024), (200,)),
    ("glove", dict(n=1_000_000, nq=10_000, d=300, d_low=144, d_hidden=512, unit_norm=True), (300,)),
]


def measure(ix, q, ef):
    """{variant: (walk_ms per call of each round, kernel name)} for flags 0 and FLAG_HALF_ROWS, interleaved."""
    variants = (("float32", 0), ("half", g.FLAG_HALF_ROWS))
    for _, flags in variants:
        for _ in range(WARMUP):
            ix.search(q, ef, want=(), flags=flags)
    torch.cuda.synchronize()
    rounds = {name: [] for name, _ in variants}
    kernel = {}
    for _ in range(REPEATS):
        for name, flags in variants:
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(CALLS):
                ix.search(q, ef, want=(), flags=flags)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            rounds[name].append(p["walk_ms"] / p["calls"])
            kernel[name] = p["walk_kernel"].split(" (")[0]
    return rounds, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    only = {s for s in args.only.split(",") if s}
    lines = ["walk_ms per call: median of %d rounds of %d calls [lowest .. highest]; float32 = without the flag, half = GBNNS_FLAG_HALF_ROWS" % (REPEATS, CALLS)]
    records = []
    for name, kw, efs in WORKLOADS:
        if only and name not in only:
            continue
        kw = dict(kw)
        if args.n:
            kw["n"] = args.n
        print("half_rows_timing: workload", name, file=sys.stderr, flush=True)
        ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
        ix = ds.index()
        ix.enable_half_rows()
        q = ds.queries
        truth = g.exact_knn(ds.base, q, 1).to(torch.int64)[:, 0]
        torch.cuda.synchronize()
        for ef in efs:
            rounds, kernel = measure(ix, q, ef)
            res = {}
            for vname, flags in (("float32", 0), ("half", g.FLAG_HALF_ROWS)):
                r = ix.search(q, ef, want=("dist_calc",), flags=flags)
                torch.cuda.synchronize()
                res[vname] = (r["ids"].to(torch.int64).clone(), float(r["dist_calc"].to(torch.float64).mean().item()))
            rec = {"workload": name, "n": kw["n"], "nq": kw["nq"], "d": kw["d"], "d_low": kw["d_low"], "ef": ef}
            lines.append("%s  n %d  %d queries  %d -> %d  ef %d" % (name, kw["n"], kw["nq"], kw["d"], kw["d_low"], ef))
            for vname in ("float32", "half"):
                width = 2 if "_half_kernel" in kernel[vname] else 4   # (a flagged call outside the half instances' domain reads the float32 copy)
                v = rounds[vname]
                ids, dc = res[vname]
                recall = (ids == truth).float().mean().item()
                row_bytes = dc * kw["d_low"] * width
                rec[vname] = {"walk_ms": round(statistics.median(v), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5),
                              "kernel": kernel[vname], "row_bytes_per_query": round(row_bytes), "recall_at_1": round(recall, 4)}
                lines.append("  %-8s %.4f [%.4f .. %.4f] ms  %-52s rows %7.0f B/query  recall@1 %.4f"
                             % (vname, statistics.median(v), min(v), max(v), kernel[vname], row_bytes, recall))
            rec["answers_that_differ"] = int((res["float32"][0] != res["half"][0]).sum().item())
            rec["half_over_float32"] = round(rec["half"]["walk_ms"] / rec["float32"]["walk_ms"], 3)
            lines.append("  half / float32 walk_ms %.3f   answers that differ %d of %d" % (rec["half_over_float32"], rec["answers_that_differ"], kw["nq"]))
            records.append(rec)
        ix.close()
        del ds, ix, q, truth
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(records))


if __name__ == "__main__":
    main()
