"""Timing of the schema-driven JSON decoder (cep_decode_json) beside the pinned stock decoder
(cep_decode_stock_json) on the same serializer-layout batch (~2e7 records, bench.py's ingest
workload), and on a batch with one double field of 17-digit decimals.  HIP events around `steps`
launches after a warm-up, the decoders alternated over `rounds`; ms, bytes/s and the fraction
of the HBM read floor (algorithmic bytes / 8 TB/s over the measured time) per decoder.
Usage: python profiles/decode_json_probe.py [--keys 20000] [--steps 10] [--rounds 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cepamd  # noqa: E402,F401
from kafkastreams_cep_amd import EventSchema  # noqa: E402
from kafkastreams_cep_amd import native as N  # noqa: E402
from kafkastreams_cep_amd import workloads as W  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def timed(hip, fn, steps):
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    fn()
    assert hip.hipDeviceSynchronize() == 0
    hip.hipEventRecord(e0, None)
    for _ in range(steps):
        fn()
    hip.hipEventRecord(e1, None)
    assert hip.hipEventSynchronize(e1) == 0
    f = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(f), e0, e1) == 0
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return f.value / steps


def figure(ms_list, batch, out_bytes):
    ms = float(np.median(ms_list))
    alg = batch.nbytes + 8 * (batch.n + 1) + out_bytes * batch.n
    return {"ms": ms, "ms_all": ms_list, "records_per_s": batch.n / (ms * 1e-3), "bytes_per_s": batch.nbytes / (ms * 1e-3),
            "hbm_floor_frac": alg / HBM_PEAK / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipSetDevice(0) == 0
    stream = N.synth_stream("stock", W.CONFIGS[3].seed, a.keys, 1000)
    batch = N.JsonBatch.synth(stream.cols[0], stream.cols[1], stream.n_events)
    n = batch.n
    S = EventSchema({"price": "int", "volume": "int"})
    stock_out, gen_out = N.DecodedStock(n, 4, name_spans=False), N.DecodedJson(n, S)
    t_stock, t_gen = [], []
    for _ in range(a.rounds):
        t_stock.append(timed(hip, lambda: N.decode_stock_json(batch, 4, stock_out), a.steps))
        t_gen.append(timed(hip, lambda: N.decode_json(batch, S, out=gen_out), a.steps))
    same = all(np.array_equal(x.download(np.int32, n), y.download(np.int32, n)) for x, y in
               ((stock_out.price, gen_out.cols[0]), (stock_out.volume, gen_out.cols[1]), (stock_out.status, gen_out.status)))
    res = {"records": n, "batch_bytes": batch.nbytes, "outputs_equal": bool(same),
           "decode_stock_json": figure(t_stock, batch, 12), "decode_json": figure(t_gen, batch, 12)}
    del stock_out, gen_out, batch, stream
    # one double field of 17-digit decimals: 2^20 distinct records, repeated to the same count
    rng = np.random.default_rng(5)
    block = [b'{"px":%s}' % (b"%.17g" % x) for x in rng.random(1 << 20) * 1000]
    reps = max(1, n >> 20)
    dbatch = N.JsonBatch.from_records(block * reps)
    D = EventSchema({"px": "double"})
    dout = N.DecodedJson(dbatch.n, D)
    t_dbl = [timed(hip, lambda: N.decode_json(dbatch, D, out=dout), a.steps) for _ in range(a.rounds)]
    st = dout.status.download(np.int32, dbatch.n)
    res["decode_json_double"] = dict(figure(t_dbl, dbatch, 12), records=dbatch.n, batch_bytes=dbatch.nbytes,
                                     precision_records=int(np.count_nonzero(st == 8)),
                                     failed_records=int(np.count_nonzero(st)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
