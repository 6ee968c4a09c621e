"""What the half-row PLAIN walk (MODE_PLAIN with FLAG_HALF_WALK on a half-base handle, Index(db=<float16>)) costs, measured against the float
handle's PLAIN walk over the same table widened to float32 in the same run, on the synthetic workloads of bench.py's rows
(synth.make_dataset, the same recipes and cache files), at the efs_hnsw beams of the reference's parameter file.

  workload  n      queries  d     beams
  deep      10^6   10 000    96   40, 80, 120, 160, 200
  gist      10^6    1 000   960   100, 150, 200, 300, 400
  glove     10^6   10 000   300   300, 400, 600, 800, 1 000

The half table is the workload's base set rounded to binary16 (nearest even); the float handle holds that table widened back.  Both handles
share the workload's graph; the searches are PLAIN ones with k = 1 -- the hnsw half of the reference's final_test.

  float32       the float handle's unflagged PLAIN call: the yardstick, never the new code against itself
  half          the half-base handle's flagged call, knob half_walk_fast = 2: the fast instance of walk_half_base.hip, whether or not the class has been kept
  half general  the same handle with half_walk_fast = 0: the general kernel's half-walk instance takes the whole batch

  walk_ms    gbnns_profile's walk_ms + walk_general_ms (events around the stages), with the kernel each variant took (profiling serialises
             the kernels of a call)
  in flight  wall time per batch of GBNNS_FLAG_DEFER_JOIN searches with three batches in flight (no profiling), at the workload's middle beam
  answers    that differ between the float handle and either half variant (the contract: 0)
  keeps      the rule of walk_plan.cpp: a dimension class stays on its fast instance only if `half` beat `half general` by more than the
             float baseline's own run-to-run range (highest - lowest round) at every beam of the class

Interleaved rounds, the median of the rounds' per-call means with the lowest and highest round beside it.  A variant whose call takes
more than 0.1 s (the general instance on the long rows) runs rounds of one call instead of ten, after one warm-up call instead of three.  No threshold on the ratio to
float32: a row where the half-base handle is slower says so.

    python tools/half_walk_timing.py [--cache-dir DIR] [--only deep,gist,glove] [--n N] [--out FILE]
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
    ("deep", dict(n=1_000_000, nq=10_000, d=96, d_low=48, d_hidden=128), (40, 80, 120, 160, 200)),
    ("gist", dict(n=1_000_000, nq=1_000, d=960, d_low=64, d_hidden=1024), (100, 150, 200, 300, 400)),
    ("glove", dict(n=1_000_000, nq=10_000, d=300, d_low=144, d_hidden=512, unit_norm=True), (300, 400, 600, 800, 1000)),
]
VARIANTS = ("float32", "half", "half general")


def search(name, handles, q, ef, **kw):
    """One PLAIN search of a variant (the half variants share a handle: the knob says which)."""
    ix = handles["float32" if name == "float32" else "half"]
    if name != "float32":
        ix.knob("half_walk_fast", 2 if name == "half" else 0)
    flags = (0 if name == "float32" else g.FLAG_HALF_WALK) | kw.pop("flags", 0)
    return ix, ix.search(q, ef, mode=g.MODE_PLAIN, k=1, want=kw.pop("want", ()), flags=flags, **kw)


def calls_of(handles, q, ef):
    """{variant: calls per round}, from the wall time of one synchronous call (which warms up too)."""
    out = {}
    for name in VARIANTS:
        search(name, handles, q, ef)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        search(name, handles, q, ef)
        torch.cuda.synchronize()
        out[name] = CALLS if time.perf_counter() - t0 < 0.1 else 1
    return out


def profiled(handles, q, ef, calls):
    """{variant: per-call means of walk_ms + walk_general_ms over the rounds}, {variant: kernel}; the variants interleaved."""
    for name in VARIANTS:
        for _ in range(WARMUP if calls[name] == CALLS else 0):
            search(name, handles, q, ef)
    torch.cuda.synchronize()
    rounds = {name: [] for name in VARIANTS}
    kernel = {}
    for _ in range(REPEATS):
        for name in VARIANTS:
            ix = handles["float32" if name == "float32" else "half"]
            ix.profile_read(reset=True)
            ix.profile_enable(True)
            for _ in range(calls[name]):
                search(name, handles, q, ef)
            torch.cuda.synchronize()
            p = ix.profile_read(reset=True)
            ix.profile_enable(False)
            rounds[name].append((p["walk_ms"] + p["walk_general_ms"]) / p["calls"])
            kernel[name] = p["walk_kernel"].split(" (")[0] + (" + %d queries on the general kernel" % (p["general_queries"] // p["calls"]) if p["general_queries"] else "")
    return rounds, kernel


def in_flight(handles, q, ef, calls):
    """{variant: wall ms per batch over the rounds}: CALLS deferred calls, three batches in flight, joined and synchronised."""
    rounds = {name: [] for name in VARIANTS}
    for rep in range(REPEATS + 1):
        for name in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = []
            n_calls = CALLS if calls[name] == CALLS else 3
            for _ in range(n_calls):
                ix, r = search(name, handles, q, ef, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3)
                outs.append(r)
            ix.join()
            torch.cuda.synchronize()
            if rep:   # (the first round warms up)
                rounds[name].append((time.perf_counter() - t0) * 1e3 / n_calls)
            del outs
    return rounds


def fig(v):
    return {"ms": round(statistics.median(v), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", default=os.environ.get("GBNNS_CACHE", "/tmp/gbnns_cache"))
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--n", type=int, default=None, help="override the base-set size (quick looks)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    os.makedirs(args.cache_dir, exist_ok=True)
    only = {s for s in args.only.split(",") if s}
    lines = ["per call: median of %d rounds of %d calls [lowest .. highest]; float32 = Index(db.half().float()) unflagged, half = Index(db.half()) with FLAG_HALF_WALK, "
             "half general = the same with the knob half_walk_fast = 0; PLAIN, k = 1" % (REPEATS, CALLS)]
    records = []
    for wname, kw, beams in WORKLOADS:
        if only and wname not in only:
            continue
        kw = dict(kw)
        if args.n:
            kw["n"] = args.n
        print("half_walk_timing: workload", wname, file=sys.stderr, flush=True)
        ds = synth.make_dataset(seed=1234, device="cuda:0", cache_dir=args.cache_dir, **kw)
        base_h = ds.base.to(torch.float16).contiguous()
        base_f = base_h.to(torch.float32).contiguous()
        q = ds.queries
        handles = {"float32": g.Index(base_f, ds.graph_off, ds.graph_nbr, db_low=ds.db_low),
                   "half": g.Index(base_h, ds.graph_off, ds.graph_nbr, db_low=ds.db_low)}
        assert handles["half"].is_half_base and not handles["float32"].is_half_base
        table = {"float32": base_f.numel() * 4, "half": base_h.numel() * 2}
        rec = {"workload": wname, "n": kw["n"], "nq": kw["nq"], "d": kw["d"], "table_bytes": table, "beams": []}
        lines.append("%s  n %d  %d queries  d %d" % (wname, kw["n"], kw["nq"], kw["d"]))
        lines.append("  original-space table on the device: float32 %d bytes, half %d bytes" % (table["float32"], table["half"]))
        keeps = True
        for ef in beams:
            b = {"ef": ef}
            calls = calls_of(handles, q, ef)
            rounds, kernel = profiled(handles, q, ef, calls)
            b["walk_ms"] = {name: dict(fig(rounds[name]), kernel=kernel[name]) for name in VARIANTS}
            for name in VARIANTS:
                v = rounds[name]
                lines.append("  ef %-5d walk_ms   %-13s %.4f [%.4f .. %.4f] ms  %s" % (ef, name, statistics.median(v), min(v), max(v), kernel[name] + ("" if calls[name] == CALLS else "  (rounds of one call)")))
            m = {name: statistics.median(rounds[name]) for name in VARIANTS}
            spread = max(rounds["float32"]) - min(rounds["float32"])
            b["half_over_float32"] = round(m["half"] / m["float32"], 3)
            b["general_over_float32"] = round(m["half general"] / m["float32"], 3)
            b["float32_range_ms"] = round(spread, 5)
            b["fast_beats_general"] = bool(m["half general"] - m["half"] > spread)
            keeps = keeps and b["fast_beats_general"]
            if ef == beams[len(beams) // 2]:
                fl = in_flight(handles, q, ef, calls)
                b["in_flight_ms"] = {name: fig(fl[name]) for name in VARIANTS}
                for name in VARIANTS:
                    v = fl[name]
                    lines.append("  ef %-5d in flight %-13s %.4f [%.4f .. %.4f] ms  wall per batch, three in flight" % (ef, name, statistics.median(v), min(v), max(v)))
                b["in_flight_half_over_float32"] = round(b["in_flight_ms"]["half"]["ms"] / b["in_flight_ms"]["float32"]["ms"], 3)
            ids, dc = {}, None
            for name in VARIANTS:
                _, r = search(name, handles, q, ef, want=("dist_calc",))
                torch.cuda.synchronize()
                ids[name] = r["ids"].clone()
                dc = r["dist_calc"].float().mean().item()
            b["answers_that_differ"] = {name: int((ids["float32"] != ids[name]).sum().item()) for name in VARIANTS[1:]}
            b["dist_calc_mean"] = round(dc, 1)
            # row bytes a hop's gathers ask for (every computed distance reads one row), per second of walk_ms
            for name, row_bytes in (("float32", kw["d"] * 4), ("half", (kw["d"] + 7) // 8 * 16)):
                b["walk_ms"][name]["row_TBps"] = round(dc * kw["nq"] * row_bytes / (b["walk_ms"][name]["ms"] * 1e-3) / 1e12, 3)
            lines.append("  ef %-5d half / float32 %.3f   half general / float32 %.3f   float32 range %.4f ms   fast beats general by more: %s   answers that differ %d / %d of %d"
                         "   %.0f distances per query; row bytes float32 %.2f TB/s, half %.2f TB/s"
                         % (ef, b["half_over_float32"], b["general_over_float32"], spread, "yes" if b["fast_beats_general"] else "NO", b["answers_that_differ"]["half"],
                            b["answers_that_differ"]["half general"], kw["nq"], dc, b["walk_ms"]["float32"]["row_TBps"], b["walk_ms"]["half"]["row_TBps"]))
            rec["beams"].append(b)
        rec["keeps_fast_instance"] = keeps
        lines.append("  %s (d %d): the class %s its fast instance" % (wname, kw["d"], "keeps" if keeps else "goes to the general instance, not"))
        records.append(rec)
        for ix in handles.values():
            ix.close()
        del ds, handles, base_h, base_f, q
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(records) + "\n")
    print(json.dumps(records))


if __name__ == "__main__":
    main()
