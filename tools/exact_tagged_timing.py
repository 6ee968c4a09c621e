"""Where the tagged walks stop paying and the exact scan over the allowed rows takes over: Index.exact_knn (gbnns_index_exact_knn) with
query tags against gbnns_search_tagged and its GBNNS_FLAG_TAG_BRIDGE form, on the SIFT-shaped synthetic workload of bench.py
(synth.make_dataset: 10^6 x 128 -> 32, 10 000 queries), rows and queries quantised to uint8 as in tools/byte_rows_timing.py so that a
float handle (the table widened) and a byte handle hold the same table.

The tag table is tools/tag_timing.py's: every row draws r uniform in 0 .. 63 and gets  1 | (r < 32) << 1 | (r < 8) << 2 | (r == 0) << 3 ;
a batch whose queries all carry Q = 1 / 2 / 4 / 8 may see all, 1/2, 1/8 and 1/64 of the rows.  Per (handle, fraction):

  exact k    wall ms of Index.exact_knn(queries, k, query_tags) for k = 1 and 10 -- the call returns when its work has finished -- and
             beside it the part that does not depend on the batch (workspace, the padded copy of the tag table, packing the 10^6 rows for
             the matrix cores: "pack"), estimated as the intercept of the line through the same call with the first 2 048 queries (the
             smallest batch the float call's matrix-core path takes) and with all 10 000, given in ms and as its share of the full call
  tagged     walk_ms (gbnns_profile) of gbnns_search_tagged on the same batch at ef 64 (LOWQ mode: the low-dimensional queries are the
             net's projection of the unquantised ones), entries at random allowed rows, and its recall@1 against the exact call's first
             column
  bridged    the same with GBNNS_FLAG_TAG_BRIDGE

Medians over REPEATS rounds with the lowest and highest round beside them; the variants of a row interleaved on the same handles in the
same run.  No threshold: the table is the crossover, whatever it is.

    python tools/exact_tagged_timing.py [--cache-dir DIR] [--n N] [--out FILE]
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

REPEATS, CALLS, WARMUP = 7, 5, 2
SHAPE = dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256)
FRACTIONS = (("1", 1), ("1/2", 2), ("1/8", 4), ("1/64", 8))   # (name, Q)
KS = (1, 10)
EF = 64
NQ_SMALL = 2048


def quantise(x):
    return torch.clamp(torch.round(x * 256.0 + 128.0), 0, 255).to(torch.uint8).contiguous()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def walk_ms(ix, q, q_low, ent, qt, flags):
    ix.profile_read(reset=True)
    ix.profile_enable(True)
    for _ in range(CALLS):
        ix.search(q, EF, mode=g.MODE_LOWQ, queries_low=q_low, entry_ids=ent, query_tags=qt, flags=flags, want=())
    torch.cuda.synchronize()
    p = ix.profile_read(reset=True)
    ix.profile_enable(False)
    return (p["walk_ms"] + p["walk_general_ms"]) / p["calls"]


def spread(v):
    return {"ms": round(statistics.median(v), 4), "lowest": round(min(v), 4), "highest": round(max(v), 4)}


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
    n, nq = kw["n"], kw["nq"]
    ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
    base_u8 = quantise(ds.base)
    base_f = base_u8.to(torch.float32).contiguous()
    q_u8 = quantise(ds.queries)
    q_f = q_u8.to(torch.float32).contiguous()
    q_low = synth.project(ds.net, ds.queries).contiguous()
    handles = {"float32": g.Index(base_f, ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net),
               "bytes": g.Index(base_u8, ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net)}
    queries = {"float32": q_f, "bytes": q_u8}
    gen = torch.Generator(device="cpu").manual_seed(4321)
    r = torch.randint(0, 64, (n,), generator=gen)
    tags = (1 | ((r < 32).to(torch.int32) << 1) | ((r < 8).to(torch.int32) << 2) | ((r == 0).to(torch.int32) << 3)).to(torch.int32)
    for ix in handles.values():
        ix.set_tags(tags.to("cuda:0"))
    torch.cuda.synchronize()
    lines = ["sift-shaped  n %d  %d queries  d %d (uint8 values; float32 = the table widened)  walks: ef %d, LOWQ mode" % (n, nq, kw["d"], EF),
             "exact = Index.exact_knn(queries, k, query_tags), wall ms; pack = its batch-independent part (workspace, tag copy, pack: intercept over 2 048 and all queries) and its share; "
             "tagged / bridged = walk_ms of gbnns_search_tagged without / with GBNNS_FLAG_TAG_BRIDGE; median of %d rounds [lowest .. highest]" % REPEATS]
    records = []
    for fname, qv in FRACTIONS:
        rows = torch.nonzero((tags & qv) != 0)[:, 0]
        ent = rows[torch.randint(0, len(rows), (nq,), generator=gen)].to(torch.int32).to("cuda:0")
        qt = torch.full((nq,), qv, dtype=torch.int32, device="cuda:0")
        for name, ix in handles.items():
            q = queries[name]
            rec = {"handle": name, "allowed": fname, "allowed_rows": int(len(rows)), "n": n, "nq": nq}
            lines.append("%s  allowed %s (%d rows)" % (name, fname, len(rows)))
            print("exact_tagged_timing:", lines[-1], file=sys.stderr, flush=True)
            times = {("exact", k): [] for k in KS}
            times.update({("one", k): [] for k in KS})
            times.update({"tagged": [], "bridged": []})
            for rnd in range(-WARMUP, REPEATS):
                for k in KS:
                    a = wall_ms(lambda: ix.exact_knn(q, k, query_tags=qt))
                    b = wall_ms(lambda: ix.exact_knn(q[:NQ_SMALL], k, query_tags=qt[:NQ_SMALL]))
                    if rnd >= 0:
                        times[("exact", k)].append(a)
                        times[("one", k)].append(b)
                t = walk_ms(ix, q_f, q_low, ent, qt, 0)
                b = walk_ms(ix, q_f, q_low, ent, qt, g.FLAG_TAG_BRIDGE)
                if rnd >= 0:
                    times["tagged"].append(t)
                    times["bridged"].append(b)
            truth = ix.exact_knn(q, 1, query_tags=qt)[:, 0]
            for k in KS:
                e, o = spread(times[("exact", k)]), spread(times[("one", k)])
                pack = max(0.0, o["ms"] - (e["ms"] - o["ms"]) * NQ_SMALL / (nq - NQ_SMALL))
                rec["exact_k%d" % k] = dict(e, small_batch_ms=o["ms"], pack_ms=round(pack, 4), pack_share=round(pack / e["ms"], 3))
                lines.append("  exact k %-2d  %8.3f [%8.3f .. %8.3f] ms   %d queries %7.3f ms   pack %7.3f ms = %.2f of it" % (k, e["ms"], e["lowest"], e["highest"],
                                                                                                                       NQ_SMALL, o["ms"], pack, pack / e["ms"]))
            for what, flags in (("tagged", 0), ("bridged", g.FLAG_TAG_BRIDGE)):
                ids = ix.search(q_f, EF, mode=g.MODE_LOWQ, queries_low=q_low, entry_ids=ent, query_tags=qt, flags=flags, want=())["ids"]
                torch.cuda.synchronize()
                recall = (ids == truth).float().mean().item()
                w = spread(times[what])
                rec[what] = dict(w, recall_at_1=round(recall, 4), over_exact_k1=round(w["ms"] / rec["exact_k1"]["ms"], 3))
                lines.append("  %-10s %8.3f [%8.3f .. %8.3f] ms   recall@1 against exact %.4f   walk / exact k 1 %.3f" % (what, w["ms"], w["lowest"], w["highest"],
                                                                                                                    recall, w["ms"] / rec["exact_k1"]["ms"]))
            records.append(rec)
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
