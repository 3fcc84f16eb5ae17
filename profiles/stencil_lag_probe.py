"""Config 2's stream (1e8 events / 1e4 keys, in HBM) under "three rising values"
(workloads.rising_query(3, t), a lagged strict chain) with the value column as int, long and
double.  Per type three sessions of one process: the lag fast route (stencil_mask_lag), the
interpreted lagged route (the same chain with the read value under `+ 0`) and a force_nfa session
of the fast route's query - the path the query took before lagged chains ran on the stencil.
strict_abc_query over the int column is the control.  Per case: warm-up pushes, then --reps
windows of pushes, every window ending in a device synchronise; the figure of a window is the
device-event kernel time per push, and a case reports the windows' median and spread
(min..max), the algorithmic bytes (4 or 8 B per event + 16 B per match) and their rate against
the 8 TB/s roofline.  The cases run interleaved, window by window.  One JSON line per case.
Usage (GPU box, repo root): python profiles/stencil_lag_probe.py [--types int,long,double]"""
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
ap.add_argument("--types", default="int,long,double")
ap.add_argument("--steps", type=int, default=20)  # pushes per window (the slow routes: a fifth)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--keys", type=int, default=W.CONFIGS[2].n_keys)
ap.add_argument("--no-nfa", action="store_true")
args = ap.parse_args()
cfg = W.CONFIGS[2]
base = N.synth_stream("abc", cfg.seed, args.keys, cfg.mean_events)
v = base.cols[0].download(np.int32, base.n_events)


def rising_interp(t):
    """rising_query(3, t) with the read value under `+ 0`: no fast form, the interpreted route"""
    b = QueryBuilder(EventSchema({"v": t}))
    return (b.select("S0").where(lambda k, e, ts, s: e.v >= 0).fold("p", lambda k, e, c: e.v).then()
            .select("S1").where(lambda k, e, ts, s: e.v > s.get("p") + 0).fold("p", lambda k, e, c: e.v).then()
            .select("S2").where(lambda k, e, ts, s: e.v > s.get("p") + 0).build())


def column(t):
    if t == "int":
        return base.cols[0]
    c = v.astype({"long": np.int64, "double": np.float64}[t])
    b = N.DeviceBuffer(c.nbytes)
    b.upload(c)
    return b


cases = []


def add(name, query, t, steps, **kw):
    q = N.Query(query.to_ir())
    stream = N.DeviceStream(base.n_keys, base.n_events, base.key_off, [column(t)])
    s = N.Session(q, **kw)
    for _ in range(2):
        s.push_device(stream)
    N.lib().cep_sync(s.h)
    cases.append({"name": name, "s": s, "stream": stream, "ms": [], "steps": max(1, steps),
                  "plan": None if kw else q.stencil_plan(), "col_bytes": 4 if t == "int" else 8})


add("abc_int_control", W.strict_abc_query(), "int", args.steps)
for t in args.types.split(","):
    add(f"rising3_{t}_fast", W.rising_query(3, t), t, args.steps)
    add(f"rising3_{t}_interp", rising_interp(t), t, args.steps // 5)
    if not args.no_nfa:
        add(f"rising3_{t}_force_nfa", W.rising_query(3, t), t, args.steps // 5, force_nfa=True)
for _ in range(args.reps):
    for c in cases:
        s = c["s"]
        s.timing_totals(0, reset=True)
        for _ in range(c["steps"]):
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
                      "kernel_ms_max": round(max(c["ms"]), 4), "windows": len(c["ms"]), "steps": c["steps"],
                      "alg_bytes": alg, "bytes_per_s": round(alg / (med * 1e-3), 1),
                      "roofline_frac": round(alg / (med * 1e-3) / 8e12, 4)}), flush=True)
