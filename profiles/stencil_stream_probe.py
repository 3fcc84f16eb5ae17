"""Strict SEQ(A,B,C) through a streaming session (stencil_mask, stencil_edge,
stencil_emit with a per-key carry) against the NFA path such a session took before
(force_nfa=True keeps it) and against one per-batch stencil push of the whole stream.
Shape a: config 2's stream (1e8 events, 1e4 keys) cut per key into --slices device slices.
Shape b: --keys-b keys with --per-b events per key and batch (stencil_edge's dense route).
Per case: one warm-up pass over the slices, then --reps passes, every pass ending in a device
synchronise; the figures of a pass are cep_timing_totals' kernel time summed over its slices
and the host's wall time (the session is reset before each pass, outside the kernel time).
One JSON line per case.
Usage (GPU box, repo root): python profiles/stencil_stream_probe.py [--shapes a,b] [--nfa 0]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import cepamd  # noqa: E402,F401
from kafkastreams_cep_amd import native as N  # noqa: E402
from kafkastreams_cep_amd import workloads as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="a,b")
ap.add_argument("--slices", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--keys-b", type=int, default=1_000_000)
ap.add_argument("--per-b", type=int, default=2)
ap.add_argument("--batches-b", type=int, default=8)
ap.add_argument("--nfa", type=int, default=1, help="0: skip the force_nfa sessions")
args = ap.parse_args()
cfg = W.CONFIGS[2]
q = N.Query(W.strict_abc_query().to_ir())


def passes(s, parts, reset):
    out, wall = [], []
    for rep in range(args.reps + 1):
        if reset:
            s.reset()
        s.timing_totals(0, reset=True)
        n, t0 = 0, time.perf_counter()
        for p in parts:
            s.push_device(p)
            n += s.digest(0)[0] if rep == 0 else 0
        N.lib().cep_sync(s.h)
        if rep == 0:
            matches = n
        else:
            wall.append((time.perf_counter() - t0) * 1e3)
            out.append(s.timing_totals(0)[0])
    return (out, wall), matches


def report(shape, case, times, matches, events, batches):
    ms, wall = times
    print(json.dumps({"shape": shape, "case": case, "events": events, "batches": batches, "matches": matches,
                      "kernel_ms_median": round(statistics.median(ms), 4), "kernel_ms_min": round(min(ms), 4),
                      "kernel_ms_max": round(max(ms), 4), "wall_ms_median": round(statistics.median(wall), 4),
                      "passes": len(ms)}), flush=True)


for shape in args.shapes.split(","):
    if shape == "a":
        stream = N.synth_stream("abc", cfg.seed, cfg.n_keys, cfg.mean_events)
        parts = bench.slice_stream(stream, args.slices)
        ms, m = passes(N.Session(q), [stream], reset=False)
        report("a", "per_batch_whole", ms, m, stream.n_events, 1)
    else:
        stream = N.synth_stream("abc", cfg.seed, args.keys_b, args.per_b * args.batches_b)
        parts = bench.slice_stream(stream, args.batches_b)
    ms, m = passes(N.Session(q, streaming=True), parts, reset=True)
    report(shape, "stream_stencil", ms, m, stream.n_events, len(parts))
    if args.nfa:
        ms, m = passes(N.Session(q, streaming=True, force_nfa=True), parts, reset=True)
        report(shape, "stream_nfa", ms, m, stream.n_events, len(parts))
    del parts, stream
