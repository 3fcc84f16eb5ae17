"""Strict SEQ(A,B,C) with a window on its last stage under semantic WITHIN (DESIGN.md §3.3:
stencil_within between the mask and emit passes) against the NFA path such a query took before
(force_nfa=True keeps it), per batch and as a stream.
Config 2's stream (1e8 events, 1e4 keys); event times a walk with steps 0..3 and the window
1 ms, so about half the candidate matches expire (C's time less B's is 0 or 1 for the rest).
Cases: the whole stream as one per-batch push and cut per key into --slices slices of a
streaming session, each on the stencil and on the NFA kernel; and, for the pass's own cost, the
un-windowed query and the same window at 2^62 ms (the pass runs and clears nothing).  Per case:
one warm-up pass, then --reps passes, every pass ending in a device synchronise; the figures of
a pass are cep_timing_totals' kernel time summed over its batches and the host's wall time.
One JSON line per case, and one with the pass's bytes.
Usage (GPU box, repo root): python profiles/stencil_within_probe.py [--nfa 0] [--slices 10]
stencil_within's own time: rocprofv3 --kernel-trace --stats -d DIR -- python profiles/stencil_within_probe.py
--nfa 0 --reps 3 (a run of its own; --precompile beforehand fills the JIT cache for the force_nfa sessions)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cepamd  # noqa: E402,F401
from kafkastreams_cep_amd import EventSchema, QueryBuilder  # noqa: E402
from kafkastreams_cep_amd import native as N  # noqa: E402
from kafkastreams_cep_amd import workloads as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slices", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--nfa", type=int, default=1, help="0: skip the force_nfa sessions")
ap.add_argument("--precompile", action="store_true", help="fill the JIT cache for the force_nfa sessions and exit")
args = ap.parse_args()
cfg = W.CONFIGS[2]


def abc_within(ms):
    """workloads.strict_abc_query with WITHIN `ms` on C (None: no window)"""
    b = QueryBuilder(EventSchema({"v": "int"}))
    c = (b.select("A").where(lambda k, v, ts, s: v.v < 4).then()
         .select("B").where(lambda k, v, ts, s: (v.v >= 4) & (v.v < 8)).then()
         .select("C").where(lambda k, v, ts, s: v.v >= 8))
    return N.Query((c.within(ms, W.TimeUnit.MILLISECONDS) if ms is not None else c).build().to_ir(semantic_within=True))


q_win, q_wide, q_plain = abc_within(1), abc_within(1 << 62), abc_within(None)
assert q_win.kind == q_wide.kind == q_plain.kind == N.CEP_KIND_STENCIL
if args.precompile:
    print("jit", q_win.precompile())
    sys.exit(0)


def passes(s, parts, reset):
    """parts: [(DeviceStream, device times)]"""
    out, wall = [], []
    for rep in range(args.reps + 1):
        if reset:
            s.reset()
        s.timing_totals(0, reset=True)
        n, t0 = 0, time.perf_counter()
        for p, t in parts:
            s.push_device(p, t.ptr)
            n += s.digest(0)[0] if rep == 0 else 0
        N.lib().cep_sync(s.h)
        if rep == 0:
            matches = n
        else:
            wall.append((time.perf_counter() - t0) * 1e3)
            out.append(s.timing_totals(0)[0])
    return (out, wall), matches


def report(case, times, matches, events, batches):
    ms, wall = times
    print(json.dumps({"case": case, "events": events, "batches": batches, "matches": matches,
                      "kernel_ms_median": round(statistics.median(ms), 4), "kernel_ms_min": round(min(ms), 4),
                      "kernel_ms_max": round(max(ms), 4), "wall_ms_median": round(statistics.median(wall), 4),
                      "passes": len(ms)}), flush=True)
    return statistics.median(ms)


def upload(a):
    b = N.DeviceBuffer(max(8, a.nbytes))
    b.upload(a)
    return b


stream = N.synth_stream("abc", cfg.seed, cfg.n_keys, cfg.mean_events)
n = stream.n_events
ts_host = np.cumsum(np.random.default_rng(2).integers(0, 4, n, dtype=np.int8), dtype=np.int64) + 1_600_000_000_000
whole = [(stream, upload(ts_host))]
# the slices of bench.slice_stream, with each slice's event times gathered on the host
off = stream.key_off.download(np.uint64, stream.n_keys + 1).astype(np.int64)
cnt = np.diff(off)
parts = []
for b in range(args.slices):
    lo, hi = cnt * b // args.slices, cnt * (b + 1) // args.slices
    part = N.gather_ranges(stream, (off[:-1] + lo).astype(np.uint64), (off[:-1] + hi).astype(np.uint64))
    local = np.concatenate([[0], np.cumsum(hi - lo)])
    idx = np.arange(local[-1]) + np.repeat(off[:-1] + lo - local[:-1], hi - lo)
    parts.append((part, upload(ts_host[idx])))
del ts_host, idx

med = {}
for name, q in [("plain", q_plain), ("within", q_win), ("within_never_expires", q_wide)]:
    t, m = passes(N.Session(q), whole, reset=False)
    med[name] = report("per_batch_" + name, t, m, n, 1), m
t, m = passes(N.Session(q_win, streaming=True), parts, reset=True)
report("stream_within", t, m, n, len(parts))
t, m = passes(N.Session(q_plain, streaming=True), parts, reset=True)
report("stream_plain", t, m, n, len(parts))
if args.nfa:
    t, m = passes(N.Session(q_win, force_nfa=True), whole, reset=False)
    report("per_batch_nfa", t, m, n, 1)
    t, m = passes(N.Session(q_win, streaming=True, force_nfa=True), parts, reset=True)
    report("stream_nfa", t, m, n, len(parts))
# The pass's bytes.  Every word record is read (16 B a 64-event word); a word with a candidate
# reads 64 + 1 event times, against the 8 B x (M - 1) = 16 B a candidate strictly needs.
# Candidate words are counted on the host from the un-windowed matches' end positions.
s = N.Session(q_plain)
s.push_device(stream)
m = s.matches(0)
end = off[:-1][m["key"].astype(np.int64)] + m["emit_seq"].astype(np.int64)
cand_words = int(len(np.unique(end // 64)))
words = (n + 63) // 64
within_ms = med["within_never_expires"][0] - med["plain"][0]
moved = 16 * words + 8 * 65 * cand_words
print(json.dumps({"case": "within_pass_bytes", "words": words, "candidate_words": cand_words,
                  "candidates": int(m["n_matches"]), "bytes_moved": moved,
                  "bytes_needed_8B_x_(M-1)_per_candidate_word": 8 * 2 * cand_words,
                  "within_ms_by_difference": round(within_ms, 4),
                  "moved_GBps": round(moved / within_ms / 1e6, 1) if within_ms > 0 else None}), flush=True)
