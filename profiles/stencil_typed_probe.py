"""Config 2's stream (strict SEQ(A,B,C), 1e8 events / 1e4 keys, in HBM) on the stencil session
with the value column as int (the control), long, double, and an int + double pair: the mask
pass's typed range fast path against the int32 one.  Per case: warm-up pushes,
then --reps windows of --steps pushes each, every window ending in a device synchronise; the
figure of a window is the device-event kernel time per push (stencil_mask + stencil_emit), and
the case reports the windows' median and spread (min..max), the algorithmic bytes (4 or 8 B per
event per column read + 16 B per match) and their rate against the 8 TB/s roofline.  The cases
run interleaved, window by window.  One JSON line per case.
Usage (GPU box, repo root): python profiles/stencil_typed_probe.py [--cases int,long,...]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cepamd  # noqa: E402,F401
from kafkastreams_cep_amd import EventSchema, QueryBuilder  # noqa: E402
from kafkastreams_cep_amd import native as N  # noqa: E402
from kafkastreams_cep_amd import workloads as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="int,long,double,int+double")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--keys", type=int, default=W.CONFIGS[2].n_keys)
args = ap.parse_args()
cfg = W.CONFIGS[2]
base = N.synth_stream("abc", cfg.seed, args.keys, cfg.mean_events)
v = base.cols[0].download(np.int32, base.n_events)


def pair_query():
    """strict_abc_query's ranges on the double column, every stage also reading the int one."""
    b = QueryBuilder(EventSchema({"v": "int", "px": "double"}))
    return (b.select("A").where(lambda k, e, ts, s: (e.px < 4) & (e.v >= 0)).then()
            .select("B").where(lambda k, e, ts, s: (e.px >= 4) & (e.px < 8) & (e.v >= 0)).then()
            .select("C").where(lambda k, e, ts, s: (e.px >= 8) & (e.v >= 0)).build())


def column(t):
    if t == "int":
        return base.cols[0]
    c = v.astype({"long": np.int64, "double": np.float64}[t])
    b = N.DeviceBuffer(c.nbytes)
    b.upload(c)
    return b


cases = []
for name in args.cases.split(","):
    types = name.split("+")
    q = N.Query((pair_query() if len(types) > 1 else W.strict_abc_query(EventSchema({"v": types[0]}))).to_ir())
    stream = N.DeviceStream(base.n_keys, base.n_events, base.key_off, [column(t) for t in types])
    s = N.Session(q)
    for _ in range(5):
        s.push_device(stream)
    N.lib().cep_sync(s.h)
    plan = q.stencil_plan() if hasattr(q, "stencil_plan") else None  # (absent before the typed path)
    cases.append({"name": name, "s": s, "stream": stream, "ms": [], "plan": plan,
                  "col_bytes": sum(4 if t == "int" else 8 for t in types)})
for _ in range(args.reps):
    for c in cases:
        s = c["s"]
        s.timing_totals(0, reset=True)
        for _ in range(args.steps):
            s.push_device(c["stream"])
        N.lib().cep_sync(s.h)
        kern, _aux, n = s.timing_totals(0)
        c["ms"].append(kern / n)
for c in cases:
    matches = c["s"].digest(0)[0]
    alg = float(c["col_bytes"]) * base.n_events + 16.0 * matches
    med = statistics.median(c["ms"])
    print(json.dumps({"case": c["name"], "plan": c["plan"], "events": base.n_events, "matches": matches,
                      "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(c["ms"]), 4),
                      "kernel_ms_max": round(max(c["ms"]), 4), "windows": len(c["ms"]), "steps": args.steps,
                      "alg_bytes": alg, "bytes_per_s": round(alg / (med * 1e-3), 1),
                      "roofline_frac": round(alg / (med * 1e-3) / 8e12, 4)}), flush=True)
