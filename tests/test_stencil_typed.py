"""The stencil's typed range fast path: strict chains over long and double columns (and
pairs mixing them with int) take stencil_mask's range route and match the oracle bit for bit."""
import types

import numpy as np
import pytest

import oracle
from gpu_helpers import assert_parity, gpu_run
from kafkastreams_cep_amd import EventSchema, QueryBuilder
from kafkastreams_cep_amd import native as N
from kafkastreams_cep_amd import workloads as W

DT = {"int": np.int32, "long": np.int64, "double": np.float64}
NAN, INF, TINY, DMAX = float("nan"), float("inf"), 5e-324, 1.7976931348623157e308
I64 = (-(1 << 63), (1 << 63) - 1)


def chain(cols, preds):
    """SEQ of ONE + strict stages over columns c0, c1.. of types `cols`; preds[i](c0, c1..)."""
    b = QueryBuilder(EventSchema({f"c{j}": t for j, t in enumerate(cols)}))
    for i, p in enumerate(preds):
        sel = b.select(f"S{i}").where(lambda k, v, ts, s, p=p: p(*[getattr(v, f"c{j}") for j in range(len(cols))]))
        b = sel.then() if i < len(preds) - 1 else sel
    return b.build()


def mod4_chain(cols, m):
    """Stage i: c0 == i % 4 as a range; a second column (an independent draw from 0..9) in [i % 2, 8]."""
    def pred(i):
        if len(cols) == 1:
            return lambda x: (x >= i % 4) & (x <= i % 4)
        return lambda x, y: (x >= i % 4) & (i % 2 <= y) & (x <= i % 4) & (y <= 8)
    return chain(cols, [pred(i) for i in range(m)])


PLANS = [
    (lambda: mod4_chain(["double"], 3), (1, [0], [3])),
    (lambda: mod4_chain(["long"], 3), (1, [0], [2])),
    (lambda: mod4_chain(["int", "double"], 3), (1, [0, 1], [1, 3])),
    (lambda: mod4_chain(["double", "int"], 3), (1, [1, 0], [1, 3])),  # a mixed pair: the int first
    (lambda: mod4_chain(["long", "double"], 3), (1, [0, 1], [2, 3])),
    (lambda: mod4_chain(["int"], 3), (1, [0], [1])),
    (lambda: chain(["double"], [lambda x: x != 1.0, lambda x: x < 2.0]), (0, [], [])),
    (lambda: chain(["int", "long", "double"], [lambda x, y, z: (x < 1) & (y < 1), lambda x, y, z: z < 1.0]), (0, [], [])),
    (lambda: chain(["int"], [lambda x: x < 2.5, lambda x: x > 1]), (0, [], [])),  # the field under a cast
]


@pytest.mark.parametrize("case", range(len(PLANS)))
def test_stencil_plan(case):
    build, (rng, fields, tps) = PLANS[case]
    q = N.Query(build().to_ir())
    assert q.kind == N.CEP_KIND_STENCIL
    assert q.stencil_plan() == {"range": rng, "n_cols": len(fields), "col_field": fields, "col_type": tps}


def test_stencil_plan_refuses_nfa_query():
    with pytest.raises(N.CepError):
        N.Query(W.stock_query("readme").to_ir()).stencil_plan()


def check(ir, off, cols, min_matches, session=None):
    assert N.Query(ir).stencil_plan()["range"] == 1
    r = oracle.run(ir, off, cols, threads=8)
    assert r["n_matches"] >= min_matches, r["n_matches"]
    assert_parity(gpu_run(ir, off, cols, session=session, push=session is None), r, off)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("cols", ["long", "double", "int+double", "double+int", "long+double", "double+double",
                                  "long+long"])
def test_typed_key_boundaries(cols, m):
    """test_stencil_key_boundaries' stream (key starts around the 4096-event wave edges, empty
    keys, a key over 16 waves, a ragged end) cast to every column type."""
    from test_gpu_parity import _boundary_stream
    cols = cols.split("+")
    off, v = _boundary_stream(m)
    data = [v.astype(DT[cols[0]])]
    if len(cols) > 1:
        data.append(np.random.default_rng(99).integers(0, 10, len(v)).astype(DT[cols[1]]))
    check(mod4_chain(cols, m).to_ir(), off, data, 1001)


SPECIALS = {  # chains whose bounds sit on the zeros, the infinities and a NaN
    "lt+0,ge-0": [lambda x: x < 0.0, lambda x: x >= -0.0],
    "le+0,gt+0": [lambda x: x <= 0.0, lambda x: x > 0.0],
    "gt-0,le-0": [lambda x: x > -0.0, lambda x: x <= -0.0],
    "ge+0,eq+0": [lambda x: x >= 0.0, lambda x: 0.0 == x],
    "eq-0,lt-0": [lambda x: x == -0.0, lambda x: -0.0 > x],
    "lt+inf,ge-inf": [lambda x: x < INF, lambda x: x >= -INF],
    "ge+inf,le-inf": [lambda x: x >= INF, lambda x: x <= -INF],
    "gt-inf,le+inf": [lambda x: x > -INF, lambda x: x <= INF],
    "nan": [lambda x: x >= -INF, lambda x: x < NAN],
    "other_column": [lambda x, y: x >= -1.5, lambda x, y: y <= 1.5],  # each stage leaves a column free
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPECIALS))
def test_double_special_values(name):
    """NaNs of both signs, both zeros, infinities, denormals: the order-key compare is Java's."""
    vals = np.array([NAN, -NAN, 0.0, -0.0, INF, -INF, TINY, -TINY, 1.5, -1.5, DMAX])
    rng = np.random.default_rng(5)
    off = np.array([0, 3000, 9000], np.uint64)  # the second key starts inside a wave; the last wave is partial
    x, y = vals[rng.integers(0, len(vals), 9000)], vals[rng.integers(0, len(vals), 9000)]
    two = name == "other_column"
    r = check(chain(["double"] * (2 if two else 1), SPECIALS[name]).to_ir(), off, [x, y] if two else [x],
              0 if name == "nan" else 20)
    if name == "nan":
        assert r["n_matches"] == 0
    if two:  # a NaN in the column a stage does not constrain still matches
        pos, st = r["pair_pos"].astype(np.int64), r["pair_stage"]
        assert np.isnan(y[pos[st == 0]]).any() and np.isnan(x[pos[st == 1]]).any()


LONGS = {
    "le_max,ge_min,eq_2^53+1": [lambda x: x <= I64[1], lambda x: x >= I64[0], lambda x: x == (1 << 53) + 1],
    "gt_2^31,lt_-2^31": [lambda x: x > (1 << 31), lambda x: x < -(1 << 31)],
    "ge_max,le_min": [lambda x: I64[1] <= x, lambda x: x <= I64[0]],
    "between_-2^53-1_2^31": [lambda x: (x >= -(1 << 53) - 1) & (x <= (1 << 31)), lambda x: x > -(1 << 53) - 1],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LONGS))
def test_long_extremes(name):
    """The full int64 range, no clamping and no trip through a double (2^53 + 1 is not 2^53)."""
    vals = np.array([I64[0], I64[1], 1 << 31, -(1 << 31), (1 << 53) + 1, -(1 << 53) - 1, 1 << 53, (1 << 53) + 2,
                     -(1 << 53), 0], np.int64)
    off = np.array([0, 3000, 9000], np.uint64)
    x = vals[np.random.default_rng(6).integers(0, len(vals), 9000)]
    check(chain(["long"], LONGS[name]).to_ir(), off, [x], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("route,n", [("unaligned", 10000), ("short", 100)])
def test_typed_slow_routes(route, n):
    """A device column 8 B off a 16-B boundary, and a batch shorter than one wave."""
    off = np.array([0, n // 3, n], np.uint64)
    x = (np.arange(n) % 4).astype(np.float64)
    ir = mod4_chain(["double"], 3).to_ir()
    k = 1 if route == "unaligned" else 2  # elements before the column in its 16-B aligned buffer
    pad = N.DeviceBuffer(8 * (n + k))
    pad.upload(np.concatenate([[NAN] * k, x]))
    kb = N.DeviceBuffer(off.nbytes)
    kb.upload(off)
    col = types.SimpleNamespace(ptr=pad.ptr + 8 * k)
    s = N.Session(N.Query(ir))
    s.push_device(N.DeviceStream(2, n, kb, [col], keep=pad))
    check(ir, off, [x], 10, session=s)
