"""What gbnns_search_tagged costs and what a restricted walk finds, measured on the synthetic workloads of bench.py's rows
(synth.make_dataset, the same recipes and cache files).

  workload  n          queries  shape      beam
  sift      10^6       10 000   128 -> 32  ef 64, and ef 36 (its recall gate)
  deep      10^6       10 000    96 -> 48  ef 40

Every row of the index draws r uniform in 0 .. 63 and gets the tag word  1 | (r < 32) << 1 | (r < 8) << 2 | (r == 0) << 3 ; a batch whose
queries all carry Q = 1 / 2 / 4 / 8 may see all, 1/2, 1/8 and 1/64 of the rows.  Every query enters at a random row it may see (an entry
it may not see is the empty row by definition -- include/gbnns.h).  Per (workload, beam, fraction):

  tagged     walk_ms of gbnns_search_tagged (the tag instance of the generic kernel family)
  bridged    walk_ms of gbnns_search_tagged with GBNNS_FLAG_TAG_BRIDGE (walk_bridge_kernel: disallowed neighbours are looked through), with the
             queries per call its first pass handed to the general kernel, its hops and dist_calc per query and its recall@1
  generic    walk_ms of the untagged search from the same entries on the same family, untagged (knob "hot" = 0): at fraction 1 the two walk the
             same graph and the ratio is the cost of the tag gather per hop
  default    walk_ms of the untagged search as every caller gets it (walk_hot_kernel on sift, walk_reg_wide_kernel on deep)
  hops, dist_calc per query of the tagged walk, and recall@1 against gbnns_exact_knn over the allowed rows only

walk_ms from gbnns_profile (events around the stage; profiling serialises the kernels; the fused re-rank is part of it in every variant),
all variants on the SAME handle in the same run, interleaved -- REPEATS rounds of CALLS calls each after a warm-up, the figure is the
median over the rounds of the per-call mean, with the lowest and highest round beside it.  No threshold: a row where the restricted walk
is slower, or where its recall falls apart, says so.

    python tools/tag_timing.py [--cache-dir DIR] [--only sift,deep] [--n N] [--out FILE]
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

REPEATS, CALLS, WARMUP = 7, 10, 3
WORKLOADS = [
    ("sift", dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256), (64, 36)),
    ("deep", dict(n=1_000_000, nq=10_000, d=96, d_low=48, d_hidden=128), (40,)),
]
FRACTIONS = (("1", 1), ("1/2", 2), ("1/8", 4), ("1/64", 8))   # (name, Q)


def measure(ix, q, ef, ent, qt):
    """{variant: (walk_ms per call of each round, kernel name)} for the tagged call, the untagged generic family and the default, interleaved."""
    variants = (("tagged", dict(query_tags=qt), 1), ("bridged", dict(query_tags=qt, flags=g.FLAG_TAG_BRIDGE), 1), ("generic", {}, 0), ("default", {}, 1))
    rounds = {name: [] for name, _, _ in variants}
    kernel, handed = {}, {}
    for rnd in range(-1, REPEATS):   # (round -1: the warm-up)
        for name, kw, hot in variants:
            ix.knob("hot", hot)
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(WARMUP if rnd < 0 else CALLS):
                ix.search(q, ef, entry_ids=ent, want=(), **kw)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            if rnd >= 0:
                rounds[name].append((p["walk_ms"] + p["walk_general_ms"]) / p["calls"])
                kernel[name] = p["walk_kernel"].split(" (")[0]
                handed[name] = p["general_queries"] / p["calls"]
    ix.knob("hot", 1)
    return rounds, kernel, handed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    only = {s for s in args.only.split(",") if s}
    lines = ["walk_ms per call (first pass + general kernel): median of %d rounds of %d calls [lowest .. highest]; tagged = gbnns_search_tagged, "
             "bridged = the same with GBNNS_FLAG_TAG_BRIDGE, generic = untagged on the same kernel family (knob hot = 0), default = untagged" % (REPEATS, CALLS)]
    records = []
    for name, kw, efs in WORKLOADS:
        if only and name not in only:
            continue
        kw = dict(kw)
        if args.n:
            kw["n"] = args.n
        print("tag_timing: workload", name, file=sys.stderr, flush=True)
        ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
        ix = ds.index()
        q = ds.queries
        n, nq = kw["n"], kw["nq"]
        gen = torch.Generator(device="cpu").manual_seed(4321)
        r = torch.randint(0, 64, (n,), generator=gen)
        tags = (1 | ((r < 32).to(torch.int32) << 1) | ((r < 8).to(torch.int32) << 2) | ((r == 0).to(torch.int32) << 3)).to(torch.int32)
        ix.set_tags(tags.to("cuda:0"))
        torch.cuda.synchronize()
        for fname, qv in FRACTIONS:
            rows = torch.nonzero((tags & qv) != 0)[:, 0]
            ent = rows[torch.randint(0, len(rows), (nq,), generator=gen)].to(torch.int32).to("cuda:0")
            qt = torch.full((nq,), qv, dtype=torch.int32, device="cuda:0")
            # ground truth over the rows the batch may see
            sub = ds.base[rows.to("cuda:0")].contiguous()
            truth = rows.to("cuda:0")[g.exact_knn(sub, q, 1).to(torch.int64)[:, 0]]
            torch.cuda.synchronize()
            del sub
            for ef in efs:
                rounds, kernel, handed = measure(ix, q, ef, ent, qt)
                res = ix.search(q, ef, entry_ids=ent, query_tags=qt, want=("hops", "dist_calc"))
                br = ix.search(q, ef, entry_ids=ent, query_tags=qt, flags=g.FLAG_TAG_BRIDGE, want=("hops", "dist_calc"))
                plain = ix.search(q, ef, entry_ids=ent, want=("hops", "dist_calc"))
                torch.cuda.synchronize()
                ids = res["ids"].to(torch.int64)
                recall = (ids == truth).float().mean().item()
                b_recall = (br["ids"].to(torch.int64) == truth).float().mean().item()
                b_hops = br["hops"].to(torch.float64).mean().item()
                b_dc = br["dist_calc"].to(torch.float64).mean().item()
                found = (res["ids"] != -1).float().mean().item()
                hops = res["hops"].to(torch.float64).mean().item()
                dc = res["dist_calc"].to(torch.float64).mean().item()
                med = {v: statistics.median(rounds[v]) for v in rounds}
                rec = {"workload": name, "n": n, "nq": nq, "d": kw["d"], "d_low": kw["d_low"], "ef": ef, "allowed": fname, "allowed_rows": int(len(rows)),
                       "hops": round(hops, 2), "dist_calc": round(dc, 1), "recall_at_1_allowed": round(recall, 4), "answered": round(found, 4),
                       "untagged_hops": round(plain["hops"].to(torch.float64).mean().item(), 2),
                       "untagged_dist_calc": round(plain["dist_calc"].to(torch.float64).mean().item(), 1),
                       "tagged_over_generic": round(med["tagged"] / med["generic"], 3), "tagged_over_default": round(med["tagged"] / med["default"], 3),
                       "bridged_hops": round(b_hops, 2), "bridged_dist_calc": round(b_dc, 1), "bridged_recall_at_1_allowed": round(b_recall, 4),
                       "bridged_handed_over": round(handed["bridged"], 1), "bridged_over_tagged": round(med["bridged"] / med["tagged"], 3),
                       "bridged_over_default": round(med["bridged"] / med["default"], 3)}
                lines.append("%s  n %d  %d queries  %d -> %d  ef %d  allowed %s (%d rows)" % (name, n, nq, kw["d"], kw["d_low"], ef, fname, len(rows)))
                for v in ("tagged", "bridged", "generic", "default"):
                    rec[v] = {"walk_ms": round(med[v], 5), "lowest": round(min(rounds[v]), 5), "highest": round(max(rounds[v]), 5), "kernel": kernel[v]}
                    lines.append("  %-8s %.4f [%.4f .. %.4f] ms  %s" % (v, med[v], min(rounds[v]), max(rounds[v]), kernel[v]))
                lines.append("  tagged / generic %.3f  tagged / default %.3f   per query: hops %.1f (untagged %.1f)  dist_calc %.0f (untagged %.0f)   "
                             "recall@1 over the allowed rows %.4f" % (rec["tagged_over_generic"], rec["tagged_over_default"], hops, rec["untagged_hops"], dc,
                                                                      rec["untagged_dist_calc"], recall))
                lines.append("  bridged / tagged %.3f  bridged / default %.3f   per query: hops %.1f  dist_calc %.0f   handed over per call %.1f   "
                             "recall@1 over the allowed rows %.4f (tagged %.4f)" % (rec["bridged_over_tagged"], rec["bridged_over_default"], b_hops, b_dc,
                                                                                   handed["bridged"], b_recall, recall))
                records.append(rec)
        ix.close()
        del ds, ix, q
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
