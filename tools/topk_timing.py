"""What the k-answer re-rank costs (gbnns_search_topk), on the SIFT-shaped synthetic index of bench.py: n = 10^6, 128 -> 32, 10 000 queries.

Per beam (ef 64 and 200), device time from gbnns_profile (events around the stages; profiling serialises the kernels):

  yardstick     rerank_ms of gbnns_search_ex with GBNNS_FLAG_NO_FUSED_RERANK: the stand-alone re-rank over the same candidates, which
                reads the same ef x d x 4 bytes per query as the top-k kernel and keeps one id
  top-k kernel  rerank_ms of gbnns_search_topk with the same flag, minus the yardstick -- at k = 1 (the distance pass and a selection that
                stores one column), k = 10 and k = ef; and rerank_ms of the default call, whose re-rank is fused into the walk, so that
                the stage is the top-k kernel alone
  recall@10     of top_ids at k = 10 against gbnns_exact_knn(k = 10) in the original space

The variants are interleaved, REPEATS rounds of CALLS calls each after a warm-up; the figure is the median over the rounds of the
per-call mean, with the lowest and highest round beside it.  Prints a table and one JSON line.

    python tools/topk_timing.py [--cache-dir DIR] [--n N] [--nq NQ]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    ds = synth.make_dataset(n=args.n, nq=args.nq, d=128, d_low=32, d_hidden=256, seed=1234, device="cuda:0", cache_dir=args.cache_dir)
    ix = ds.index()
    q = ds.queries
    truth = g.exact_knn(ds.base, q, 10).to(torch.int64)
    torch.cuda.synchronize()
    NF = g.FLAG_NO_FUSED_RERANK
    record = {"n": args.n, "nq": args.nq, "repeats": REPEATS, "calls_per_repeat": CALLS}
    for ef in (64, 200):
        variants = [("search_ex, own re-rank launch", NF, 0)] + [("search_topk k=%d, own re-rank launch" % k, NF, k) for k in (1, 10, ef)] + \
                   [("search_topk k=%d, fused re-rank" % k, 0, k) for k in (1, 10, ef)]
        for _, flags, k in variants:
            for _ in range(WARMUP):
                ix.search(q, ef, want=(), flags=flags, top_k=k)
        torch.cuda.synchronize()
        rounds = {name: [] for name, _, _ in variants}
        walk = {name: [] for name, _, _ in variants}
        for _ in range(REPEATS):
            for name, flags, k in variants:
                ix.profile_read(reset=True)
                ix.profile_enable(True)
                for _ in range(CALLS):
                    r = ix.search(q, ef, want=(), flags=flags, top_k=k)
                torch.cuda.synchronize()
                p = ix.profile_read(reset=True)
                ix.profile_enable(False)
                rounds[name].append(p["rerank_ms"] / p["calls"])
                walk[name].append(p["walk_ms"] / p["calls"])
        med = {name: statistics.median(v) for name, v in rounds.items()}
        yard = med[variants[0][0]]
        print("ef %d (rerank_ms per call of %d queries: median of %d rounds [lowest .. highest]; walk_ms beside it)" % (ef, args.nq, REPEATS))
        for name, flags, k in variants:
            v = rounds[name]
            extra = ""
            if k:
                kernel = med[name] - yard if flags else med[name]
                extra = "  top-k kernel %.4f ms = %.2f x the yardstick" % (kernel, kernel / yard)
                record["ef%d_k%d_%s_ratio" % (ef, k, "own" if flags else "fused")] = round(kernel / yard, 3)
                record["ef%d_k%d_%s_ms" % (ef, k, "own" if flags else "fused")] = round(kernel, 5)
            print("  %-40s %.4f [%.4f .. %.4f]  walk %.4f%s" % (name, med[name], min(v), max(v), statistics.median(walk[name]), extra))
        record["ef%d_yardstick_ms" % ef] = round(yard, 5)
        record["ef%d_yardstick_spread" % ef] = [round(min(rounds[variants[0][0]]), 5), round(max(rounds[variants[0][0]]), 5)]
        r = ix.search(q, ef, want=(), top_k=10)
        torch.cuda.synchronize()
        top = r["top_ids"].to(torch.int64)
        hits = (top[:, :, None] == truth[:, None, :]).any(dim=2).sum().item()
        record["ef%d_recall_at_10" % ef] = round(hits / (10.0 * args.nq), 4)
        record["ef%d_recall_at_1" % ef] = round((r["ids"].to(torch.int64) == truth[:, 0]).float().mean().item(), 4)
        print("  recall@10 %.4f  (recall@1 of the answer ids %.4f)" % (record["ef%d_recall_at_10" % ef], record["ef%d_recall_at_1" % ef]))
    ix.close()
    print(json.dumps(record))


if __name__ == "__main__":
    main()
