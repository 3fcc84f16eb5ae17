"""cep_decode_json on the GPU (csrc/ingest_generic.hip): parity with the pinned stock decoder, schema
shapes vs json.loads, decimals vs float() by bit pattern, the HBM and unaligned paths, end to end."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import json_cases as JC
import json_generic_cpu as G
import oracle
from kafkastreams_cep_amd import EventSchema, QueryBuilder
from kafkastreams_cep_amd import native as N
from kafkastreams_cep_amd import workloads as W

pytestmark = pytest.mark.gpu


def assert_stock_parity(batch, n, types=(2, 2)):  # {price, volume} + span "name" vs decode_stock_json
    width = 4 if types[0] == 1 else 8
    got = N.decode_json(batch, EventSchema({"price": types[0], "volume": types[1]}), "name").download()
    exp = N.decode_stock_json(batch, width).download()
    for k in ("status", "price", "volume", "name_span"):
        bad = np.nonzero((got[k] != exp[k]).reshape(n, -1).any(axis=1))[0]
        assert len(bad) == 0, (k, [(int(i), got[k][i], exp[k][i]) for i in bad[:5]])


@pytest.mark.parametrize("types", [(2, 2), (1, 1)])
def test_parity_with_stock_decoder(types):
    recs = [c for c, _ in JC.CASES] * 3 + JC.fuzz(11, 5000)
    assert_stock_parity(N.JsonBatch.from_records(recs), len(recs), types)


def _wide():  # 32 fields of all three types; keys in written, reversed and shuffled order
    fields = [("f%d" % i, 1 + i % 3) for i in range(32)]
    vals = ['%d' % (i * 1000003 - 7) if t != 3 else '%d.%03de%d' % (i, i * 37, i - 16) for i, (_, t) in enumerate(fields)]
    kv = ['"%s":%s' % (nm, v) for (nm, _), v in zip(fields, vals)]
    orders = [kv, kv[::-1]] + [random.Random(s).sample(kv, 32) for s in range(6)]
    return fields, [("{" + ",".join(o) + "}").encode() for o in orders]


AB = [("a", 1), ("b", 2), ("c", 3)]
SHAPES = {
    "one field": ([("x", 3)], [b'{"x":1.5}', b'{"y":2,"x":-3}', b'{"x":2.5e3,"x":7}']),
    "32 fields": _wide(),
    "duplicate keys": (AB, [b'{"a":1,"b":2,"c":3,"a":4,"c":0.5,"b":-9}', b'{"a":"x","a":5,"b":1,"c":1,"c":2e0}']),
    "missing, null, wrong kind": (AB, [b'{"b":2,"c":3}', b'{"a":1,"c":3}', b'{"a":1,"b":2}', b'{"a":null,"b":2,"c":3}',
                                       b'{"a":1,"b":null,"c":3}', b'{"a":1,"b":2,"c":null}', b'{"a":1.0,"b":2,"c":3}',
                                       b'{"a":1,"b":"2","c":3}', b'{"a":1,"b":2,"c":true}', b'{"a":1,"b":2,"c":[3]}',
                                       b'{"a":1,"b":2,"c":{"c":3}}', b'{"a":4294967296,"b":2,"c":3}',
                                       b'{"a":1,"b":4294967296,"c":9223372036854775807}']),
    "escaped key": ([("price", 2)], [b'{"pr\\u0069ce":5}', b'{"p\\u0072ic\\u0065":6,"price ":1}', b'{"pr\\u00e9ce":1}']),
    "nested same-named key": ([("a", 2)], [b'{"o":{"a":1},"a":2}', b'{"a":3,"o":{"a":4},"l":[{"a":5}]}', b'{"o":{"a":1}}']),
    "equal length names": ([("ab", 1), ("ba", 1), ("aa", 3)], [b'{"ba":1,"ab":2,"aa":3}', b'{"aa":1,"ab":2,"bb":3}']),
}


@pytest.mark.parametrize("shape", SHAPES)
def test_schema_shapes_vs_json_loads(shape):
    fields, recs = SHAPES[shape]
    recs = recs * 90  # more than one block
    got = N.decode_json(N.JsonBatch.from_records(recs), EventSchema(dict(fields))).download()
    want = [G.reference(r, [(nm.encode(), t) for nm, t in fields]) for r in recs]
    assert got["status"].tolist() == [st for st, _ in want]
    for f, (nm, t) in enumerate(fields):
        exp = np.array([v[f] for _, v in want], G.DTYPES[t])
        assert got[nm].tobytes() == exp.tobytes(), (nm, got[nm][:8], exp[:8])  # doubles by bit pattern


def test_numbers_vs_float():
    rep = [repr(x) for x in G.random_doubles(20000)[:2000]]
    texts = G.BOUNDARY + rep
    got = N.decode_json(N.JsonBatch.from_records([b'{"x":%s}' % s.encode() for s in texts]),
                        EventSchema({"x": "double"})).download()
    G.check_doubles(G.BOUNDARY, got["status"][:len(G.BOUNDARY)], got["x"][:len(G.BOUNDARY)])
    n_prec = G.check_doubles(rep, got["status"][len(G.BOUNDARY):], got["x"][len(G.BOUNDARY):])
    assert n_prec * 1000 <= len(rep)


def test_hbm_path_long_record():  # a block whose span exceeds the LDS tile parses from HBM
    recs = [b'{"name":"e%d",%s"price":%d,"volume":%d}' % (i, b" " * (i % 300), i * 7 - 500, i) for i in range(3000)]
    recs[1000] = b'{"x":"' + b"y" * 100000 + b'","price":1,"volume":2}'
    assert_stock_parity(N.JsonBatch.from_records(recs), len(recs))


@pytest.mark.parametrize("skew", [1, 3, 7, 13])
def test_unaligned_spans(skew):
    recs = JC.fuzz(3, 3000)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    off += 5  # the batch starts 5 bytes into the buffer, the buffer `skew` bytes into the allocation
    blob = np.frombuffer(b"#####" + b"".join(recs), np.uint8)
    host = np.zeros(blob.nbytes + 64, np.uint8)
    host[skew:skew + blob.nbytes] = blob
    d, o = N.DeviceBuffer(host.nbytes), N.DeviceBuffer(off.nbytes)
    d.upload(host)
    o.upload(off)
    assert_stock_parity(N.JsonBatch(len(recs), blob.nbytes, SimpleNamespace(ptr=d.ptr + skew), o), len(recs))


def test_empty_batch_and_empty_records():
    S = EventSchema({"price": "long", "volume": "long"})
    assert N.decode_json(N.JsonBatch.from_records([]), S, "name").download()["status"].tolist() == []
    recs = [b""] * 300 + [b"{}"] + [b""] * 300
    assert_stock_parity(N.JsonBatch.from_records(recs), len(recs))


def test_json_to_double_query_matches():
    """records -> decode_json -> symbol keys -> a query with a double predicate and fold == the oracle"""
    cfg = W.SynthConfig("t", "stock", 100, 120, W.CONFIGS[3].seed)
    akeys, acols = W.generate_arrival(cfg)
    px = [repr(int(p) + (i % 8) / 8 + 0.1) for i, p in enumerate(acols[0])]
    recs = [b'{"sym":"S%d","px":%s,"qty":%d}' % (int(k), p.encode(), int(v)) for k, p, v in zip(akeys, px, acols[1])]
    S = EventSchema({"px": "double", "qty": "int"})
    b = N.JsonBatch.from_records(recs)
    d = N.decode_json(b, S, "sym")
    keys, n_sym = N.symbol_keys(b, d)
    assert n_sym == cfg.n_keys and not d.status.download(np.int32, len(recs)).any()
    q = (QueryBuilder(S).select().where(lambda k, v, ts, s: v.qty > 1000).fold("avg", lambda k, v, c: v.px).then()
         .select().oneOrMore().skipTillNextMatch().where(lambda k, v, ts, s: v.px > s.get("avg"))
         .fold("avg", lambda k, v, c: (c + v.px) / 2).fold("qty", lambda k, v, c: v.qty).then()
         .select().skipTillNextMatch().where(lambda k, v, ts, s: v.qty < 0.8 * s.get("qty"))
         .within(1, W.TimeUnit.HOURS).build())
    s = N.Session(N.Query(q.to_ir()), tier=N.CEP_TIER_INTERP)  # (no kernel to compile for this one query)
    s.push_arrival_device(N.ArrivalStream(n_sym, len(recs), keys, d.cols))
    m = s.matches(0)
    order = np.argsort(akeys, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(akeys, minlength=cfg.n_keys))]).astype(np.uint64)
    r = oracle.run(q.to_ir(), off, [np.array([float(p) for p in px])[order], acols[1].astype(np.int32)[order]])
    assert m["n_matches"] == r["n_matches"] > 0
    np.testing.assert_array_equal(m["key"], r["key"])
    np.testing.assert_array_equal(m["emit_seq"], r["emit_pos"].astype(np.uint64) - off[r["key"].astype(np.int64)])
    np.testing.assert_array_equal(m["pair_stage"], r["pair_stage"])
