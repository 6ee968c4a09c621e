"""What a half-base handle (Index(db=<float16>), gbnns_index_create_half_base) does to the float workloads, measured against the float handle
over the same table widened to float32, in the same run, on the synthetic workloads of bench.py's rows (synth.make_dataset, the same
recipes and cache files).

  workload  n      queries  shape        beam     (the reference's parameter file)
  deep      10^6   10 000    96 -> 48    ef 40
  gist      10^6    1 000   960 -> 64    ef 200
  glove     10^6   10 000   300 -> 144   ef 300

The half table is the workload's base set rounded to binary16 (nearest even: gbnns_round_to_half's rounding); the float handle holds that
table widened back.  Both handles share the workload's db_low, graph and net: the walk is the same walk, only the re-ranked rows differ in
width.  The yardstick is always the float handle, never the new code against itself.

  rerank_ms   gbnns_profile's (events around the stage) of GBNNS_FLAG_NO_FUSED_RERANK searches at the walk's beam: the stand-alone half kernel
              against the float kernel on the same candidate lists (profiling serialises the kernels of a call)
  walk+rerank walk_ms + walk_general_ms + rerank_ms of the half-base handle's call against the float handle's default call (the re-rank
              fused into its walk kernels) and against the float handle's GBNNS_FLAG_NO_FUSED_RERANK call
  in flight   wall time per batch of GBNNS_FLAG_DEFER_JOIN searches with three batches in flight (no profiling): half against float default
  answers     that differ between the two handles (the contract: 0)
  bytes       device bytes of each handle's original-space table

Interleaved rounds, the median of the rounds' per-call means with the lowest and highest round beside it.  No threshold: a row where the
half-base handle is slower says so, with the ratio.

    python tools/half_base_timing.py [--cache-dir DIR] [--only deep,gist,glove] [--n N] [--standalone-only] [--out FILE]

--standalone-only: the rerank_ms rows alone (the ladder-depth experiment: one run per build of csrc/rerank_half.hip with
-DGBNNS_HALF_RERANK_DEEP=<depth>, on the gist row; half_base_plan reports the depth of the library that ran).
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

REPEATS, CALLS, WARMUP = 9, 10, 3
WORKLOADS = [
    ("deep", dict(n=1_000_000, nq=10_000, d=96, d_low=48, d_hidden=128), 40),
    ("gist", dict(n=1_000_000, nq=1_000, d=960, d_low=64, d_hidden=1024), 200),
    ("glove", dict(n=1_000_000, nq=10_000, d=300, d_low=144, d_hidden=512, unit_norm=True), 300),
]
STAGES = ("walk_ms", "walk_general_ms", "rerank_ms")


def profiled(variants, q, ef):
    """{name: {stage: per-call means over the rounds}, ...}, {name: first-pass kernel}; variants: {name: (handle, flags)}, interleaved."""
    for ix, flags in variants.values():
        for _ in range(WARMUP):
            ix.search(q, ef, want=(), flags=flags)
    torch.cuda.synchronize()
    rounds = {name: {s: [] for s in STAGES} for name in variants}
    kernel = {}
    for _ in range(REPEATS):
        for name, (ix, flags) in variants.items():
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(CALLS):
                ix.search(q, ef, want=(), flags=flags)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            for s in STAGES:
                rounds[name][s].append(p[s] / p["calls"])
            kernel[name] = p["walk_kernel"].split(" (")[0]
    return rounds, kernel


def in_flight(handles, q, ef):
    """{name: wall ms per batch over the rounds}: CALLS deferred calls, three batches in flight, joined and synchronised."""
    rounds = {name: [] for name in handles}
    for rep in range(REPEATS + 1):
        for name, ix in handles.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = [ix.search(q, ef, want=(), out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for _ in range(CALLS)]
            ix.join()
            torch.cuda.synchronize()
            if rep:   # (the first round warms up)
                rounds[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
            del outs
    return rounds


def fig(v):
    return {"ms": round(statistics.median(v), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}


def show(lines, what, name, v, tail=""):
    lines.append("  %-12s %-22s %.4f [%.4f .. %.4f] ms  %s" % (what, name, statistics.median(v), min(v), max(v), tail))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--standalone-only", action="store_true", help="the stand-alone rerank_ms rows alone")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    only = {s for s in args.only.split(",") if s}
    lines = ["per call: median of %d rounds of %d calls [lowest .. highest]; float32 = Index(db.half().float()), half = Index(db.half()), the same table"
             % (REPEATS, CALLS)]
    records = []
    for name, kw, ef in WORKLOADS:
        if only and name not in only:
            continue
        kw = dict(kw)
        if args.n:
            kw["n"] = args.n
        print("half_base_timing: workload", name, file=sys.stderr, flush=True)
        ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
        base_h = ds.base.to(torch.float16).contiguous()
        base_f = base_h.to(torch.float32).contiguous()
        q = ds.queries
        flt = g.Index(base_f, ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net)
        half = g.Index(base_h, ds.graph_off, ds.graph_nbr, db_low=ds.db_low, net=ds.net)
        assert half.is_half_base and not flt.is_half_base
        plan = g.half_base_plan(0, kw["d"])
        table = {"float32": base_f.numel() * 4, "half": base_h.numel() * 2}
        rec = {"workload": name, "n": kw["n"], "nq": kw["nq"], "d": kw["d"], "d_low": kw["d_low"], "ef": ef, "table_bytes": table,
               "half_kernel": plan[0], "half_loads_in_flight": plan[1]}
        lines.append("%s  n %d  %d queries  %d -> %d  ef %d   %s, %d loads in flight" % (name, kw["n"], kw["nq"], kw["d"], kw["d_low"], ef, plan[0], plan[1]))
        lines.append("  original-space table on the device: float32 %d bytes, half %d bytes" % (table["float32"], table["half"]))
        # stand-alone re-rank on the same candidate lists
        rounds, kernel = profiled({"float32": (flt, g.FLAG_NO_FUSED_RERANK), "half": (half, g.FLAG_NO_FUSED_RERANK)}, q, ef)
        rec["rerank_ms"] = {n_: fig(rounds[n_]["rerank_ms"]) for n_ in rounds}
        for n_ in rounds:
            show(lines, "rerank_ms", n_, rounds[n_]["rerank_ms"], "%d candidates" % ef)
        rec["rerank_half_over_float32"] = round(rec["rerank_ms"]["half"]["ms"] / rec["rerank_ms"]["float32"]["ms"], 3)
        lines.append("  rerank_ms    half / float32 %.3f" % rec["rerank_half_over_float32"])
        if not args.standalone_only:
            whole = lambda r: [sum(t) for t in zip(*(r[s] for s in STAGES))]
            unfused = {"float32, unfused": whole(rounds["float32"])}
            rounds2, kernel2 = profiled({"float32, default": (flt, 0), "half": (half, 0)}, q, ef)
            calls = {"float32, default": whole(rounds2["float32, default"]), "float32, unfused": unfused["float32, unfused"], "half": whole(rounds2["half"])}
            kernels = {"float32, default": kernel2["float32, default"], "float32, unfused": kernel["float32"], "half": kernel2["half"]}
            rec["walk_plus_rerank_ms"] = {n_: dict(fig(v), kernel=kernels[n_]) for n_, v in calls.items()}
            for n_, v in calls.items():
                show(lines, "walk+rerank", n_, v, kernels[n_])
            m = {n_: statistics.median(v) for n_, v in calls.items()}
            rec["half_over_float32_default"] = round(m["half"] / m["float32, default"], 3)
            rec["half_over_float32_unfused"] = round(m["half"] / m["float32, unfused"], 3)
            lines.append("  walk+rerank  half / float32 default (fused) %.3f   half / float32 unfused %.3f" % (rec["half_over_float32_default"], rec["half_over_float32_unfused"]))
            fl = in_flight({"float32, default": flt, "half": half}, q, ef)
            rec["in_flight_ms"] = {n_: fig(v) for n_, v in fl.items()}
            for n_, v in fl.items():
                show(lines, "in flight", n_, v, "wall per batch, three in flight")
            rec["in_flight_half_over_float32"] = round(rec["in_flight_ms"]["half"]["ms"] / rec["in_flight_ms"]["float32, default"]["ms"], 3)
            lines.append("  in flight    half / float32 default %.3f" % rec["in_flight_half_over_float32"])
        ids = {n_: ix.search(q, ef, want=())["ids"].clone() for n_, ix in (("float32", flt), ("half", half))}
        torch.cuda.synchronize()
        rec["answers_that_differ"] = int((ids["float32"] != ids["half"]).sum().item())
        lines.append("  answers that differ %d of %d" % (rec["answers_that_differ"], kw["nq"]))
        records.append(rec)
        flt.close()
        half.close()
        del ds, flt, half, base_h, base_f, q, ids
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
