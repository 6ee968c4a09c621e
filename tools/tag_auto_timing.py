"""What the census costs and where gbnns_search_tagged_auto should send a query: Index.tag_census and Index.search_auto beside the bridged
walk alone and the exact scan alone, on the SIFT-shaped synthetic workload of bench.py (synth.make_dataset: 10^6 x 128 -> 32, 10 000
queries) as bytes -- rows and queries quantised to uint8 as in tools/exact_tagged_timing.py, a byte handle, DEVICE buffers.

Every row draws r uniform in 0 .. 63 and gets bit b (b = 0 .. 6) when r < 64 >> b: a query of word 1 << b may see 2^-b of the rows.

  census    ms of Index.tag_census on 10 000 queries that carry U = 1, 13 and 10 000 distinct words (HIP events around CALLS calls), and
            beside it walk_ms (gbnns_profile) of the cut walk, gbnns_search_tagged at ef 64 with every row allowed, in the same run
  per allowed fraction 1 .. 1/64 and k = 1, 10: wall ms per batch and recall@k against Index.exact_knn(queries, k, query_tags) of
            bridged   the bridged walk alone (search with FLAG_TAG_BRIDGE, top_k = k) entered at the census's `first` rows
            scan      the exact scan alone (Index.exact_knn with query_tags; recall 1 by definition)
            auto w/s  search_auto with scan_below 0 (every query walks, bridged) and 2^64 - 1 (every query scans): the routed call's overhead
  mixed     one batch whose query i carries fraction 2^-(i % 7): search_auto at scan_below between every two neighbouring fractions,
            without and with FLAG_SCAN_GATHER (the scan-routed queries through the gathered exact scan), interleaved; --only-mixed runs
            this section alone

Wall ms: host clock around one call with the device idle before and after (every call here returns when its work has finished, or is
followed by a synchronisation).  Medians over REPEATS rounds with the lowest and highest round beside them, the variants of a row
interleaved on the same handle in the same run.  LOWQ mode at ef 64: the low-dimensional queries are the net's projection of the
unquantised ones.  No threshold is asserted: the table is the answer, for this one synthetic recipe on this one device.

    python tools/tag_auto_timing.py [--cache-dir DIR] [--n N] [--out FILE] [--only-mixed]
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

REPEATS, CALLS, WARMUP = 5, 5, 1
SHAPE = dict(n=1_000_000, nq=10_000, d=128, d_low=32, d_hidden=256)
BITS = range(7)                      # fraction 2^-b
KS = (1, 10)
EF = 64
ALL = 2 ** 64 - 1


def quantise(x):
    return torch.clamp(torch.round(x * 256.0 + 128.0), 0, 255).to(torch.uint8).contiguous()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def cut_walk_ms(ix, q, q_low, ent, qt):
    ix.profile_read(reset=True)
    ix.profile_enable(True)
    for _ in range(CALLS):
        ix.search(q, EF, mode=g.MODE_LOWQ, queries_low=q_low, entry_ids=ent, query_tags=qt, want=())
    torch.cuda.synchronize()
    p = ix.profile_read(reset=True)
    ix.profile_enable(False)
    return (p["walk_ms"] + p["walk_general_ms"]) / p["calls"]


def spread(v):
    return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(v), min(v), max(v))


def recall(got, truth):
    """Mean over the queries of |got row & truth row| / k (ids as int64; -1 = none, never in a truth row of an allowed set of >= k rows)."""
    got, truth = got.to(torch.int64), truth.to(torch.int64)
    hit = (got[:, :, None] == truth[:, None, :]).any(dim=2) & (got != -1)
    return hit.float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--only-mixed", action="store_true", help="the mixed batch alone")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    kw = dict(SHAPE)
    if args.n:
        kw["n"] = args.n
    n, nq = kw["n"], kw["nq"]
    dev = torch.device("cuda:0")
    ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
    q_u8 = quantise(ds.queries)
    q_low = synth.project(ds.net, ds.queries).contiguous()
    ix = g.Index(quantise(ds.base), ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net)
    gen = torch.Generator(device="cpu").manual_seed(4321)
    r = torch.randint(0, 64, (n,), generator=gen)
    tags = torch.zeros(n, dtype=torch.int32)
    for b in BITS:
        tags |= (r < (64 >> b)).to(torch.int32) << b
    ix.set_tags(tags.to(dev))
    torch.cuda.synchronize()
    lines = ["sift-shaped  n %d  %d queries  d %d as uint8 (byte handle, DEVICE buffers)  LOWQ mode, ef %d" % (n, nq, kw["d"], EF),
             "median of %d rounds [lowest .. highest]; census: ms per call by HIP events over %d calls; everything else: wall ms per batch" % (REPEATS, CALLS)]
    records = []

    # ---- the census --------------------------------------------------------------------------------------------------------------
    words13 = torch.tensor([1 << b for b in BITS] + [0, 3, 5, 0x7F, 0x100, -1], dtype=torch.int32)
    batches = {1: torch.full((nq,), 2, dtype=torch.int32), 13: words13[torch.arange(nq) % 13],
               nq: (torch.arange(nq, dtype=torch.int64) * 2654435761 % (2 ** 31)).to(torch.int32)}   # (an odd multiplier: all distinct)
    all_q = torch.full((nq,), 1, dtype=torch.int32, device=dev)
    ent_all = torch.randint(0, n, (nq,), generator=gen).to(torch.int32).to(dev)
    q_f = q_u8.to(torch.float32).contiguous()
    times = {u: [] for u in batches}
    walk = []
    for rnd in range(-WARMUP, 0 if args.only_mixed else REPEATS):
        for u, words in batches.items():
            qt = words.to(dev)
            t = event_ms(lambda: ix.tag_census(qt), CALLS)
            if rnd >= 0:
                times[u].append(t)
        w = cut_walk_ms(ix, q_f, q_low, ent_all, all_q)
        if rnd >= 0:
            walk.append(w)
    for u, words in ({} if args.only_mixed else batches).items():
        assert len(torch.unique(words)) == u
        a, f = ix.tag_census(words.to(dev))
        ha, hf = g.tag_census(tags.numpy().view("uint32"), words.numpy().view("uint32")) if u <= 13 else (None, None)
        if ha is not None:
            assert (a.cpu().numpy().view("uint32") == ha).all() and (f.cpu().numpy().view("uint32") == hf).all()
        lines.append("census  U = %-6d %s ms" % (u, spread(times[u])))
        records.append({"census_U": u, "ms": statistics.median(times[u])})
    if not args.only_mixed:
        lines.append("cut walk (gbnns_search_tagged, every row allowed), walk_ms %s" % spread(walk))
        records.append({"cut_walk_ms": statistics.median(walk)})
    print("\n".join(lines), file=sys.stderr, flush=True)

    # ---- one fraction per batch --------------------------------------------------------------------------------------------------
    def auto(qt, k, sb, gather=0):
        return ix.search_auto(q_u8, EF, k, qt, scan_below=sb, mode=g.MODE_LOWQ, queries_low=q_low, flags=g.FLAG_TAG_BRIDGE | gather, want=())

    for b in (() if args.only_mixed else BITS):
        qt = torch.full((nq,), 1 << b, dtype=torch.int32, device=dev)
        _, first = ix.tag_census(qt)
        rows = int((tags & (1 << b) != 0).sum())
        lines.append("allowed 1/%d (%d rows)" % (1 << b, rows))
        for k in KS:
            variants = {
                "bridged": lambda: ix.search(q_u8, EF, mode=g.MODE_LOWQ, queries_low=q_low, entry_ids=first, query_tags=qt, flags=g.FLAG_TAG_BRIDGE, want=(),
                                             top_k=k)["top_ids"],
                "scan": lambda: ix.exact_knn(q_u8, k, query_tags=qt),
                "auto walk": lambda: auto(qt, k, 0)["top_ids"],
                "auto scan": lambda: auto(qt, k, ALL)["top_ids"],
            }
            t = {v: [] for v in variants}
            for rnd in range(-WARMUP, REPEATS):
                for v, fn in variants.items():
                    ms = wall_ms(fn)
                    if rnd >= 0:
                        t[v].append(ms)
            truth = ix.exact_knn(q_u8, k, query_tags=qt)
            rec = {"allowed": "1/%d" % (1 << b), "rows": rows, "k": k}
            for v, fn in variants.items():
                rc = recall(fn(), truth)
                rec[v] = {"ms": round(statistics.median(t[v]), 4), "recall": round(rc, 4)}
                lines.append("  k %-2d  %-9s %s ms   recall@%d %.4f" % (k, v, spread(t[v]), k, rc))
            records.append(rec)
        print("\n".join(lines[-9:]), file=sys.stderr, flush=True)

    # ---- a batch that spans the fractions ----------------------------------------------------------------------------------------
    qt = (1 << (torch.arange(nq) % 7)).to(torch.int32).to(dev)
    lines.append("mixed batch: query i may see 2^-(i % 7) of the rows")
    cuts = [("0 (all walk)", 0)] + [("%d (scan <= 1/%d)" % (int(1.4 * n / (1 << b)), 1 << b), int(1.4 * n / (1 << b))) for b in (6, 5, 4, 3, 2, 1)] + \
           [("2^64 - 1 (all scan)", ALL)]
    for k in KS:
        truth = ix.exact_knn(q_u8, k, query_tags=qt)
        forms = (("", 0), (" + FLAG_SCAN_GATHER", g.FLAG_SCAN_GATHER))
        t = {(name, form): [] for name, _ in cuts for form, _ in forms}
        for rnd in range(-WARMUP, REPEATS):
            for name, sb in cuts:
                for form, flag in forms:
                    ms = wall_ms(lambda: auto(qt, k, sb, flag))
                    if rnd >= 0:
                        t[(name, form)].append(ms)
        for name, sb in cuts:
            for form, flag in forms:
                res = auto(qt, k, sb, flag)
                rc = recall(res["top_ids"], truth)
                scanned = int(res["route"].sum())
                lines.append("  k %-2d  scan_below %-26s %s ms   recall@%d %.4f   scan-routed %d%s" % (k, name, spread(t[(name, form)]), k, rc, scanned, form))
                records.append({"mixed": True, "k": k, "scan_below": sb, "gather": bool(flag), "ms": round(statistics.median(t[(name, form)]), 4),
                                "recall": round(rc, 4), "scanned": scanned})
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
