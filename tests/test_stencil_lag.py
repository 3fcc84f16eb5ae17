"""Strict chains whose stages compare an event with an earlier event of the match (state.get of a fold of
an earlier stage) run on the stencil: the lag fast route and the interpreted route, exact against the oracle."""
import functools
import operator

import numpy as np
import pytest

import oracle
import stream_split as SS
from kafkastreams_cep_amd import EventSchema, QueryBuilder
from kafkastreams_cep_amd import native as N
from kafkastreams_cep_amd import workloads as W

OPS = [operator.le, operator.eq, operator.gt]
BASE = {"int": 0, "long": 1 << 40, "double": 0}


def chain(tp, m, kind, route="fast", window=None):
    """m strict stages over one column x; stage 0: x >= base - 3, folds "a" and "p".  "adj": every later stage
    x >= the stage before (lag 1).  "first": the middle stages <=, ==, > the stage before in turn, the last one
    `a <= x` against stage 0 (lag m - 1) and a range.  route "interp": the read value under `+ 0` (no fast form)."""
    rd = (lambda s, n: s.get(n) + 0) if route == "interp" else (lambda s, n: s.get(n))
    b = QueryBuilder(EventSchema({"x": tp}))
    for i in range(m):
        if i == 0:
            pred = lambda k, v, ts, s: v.x >= BASE[tp] - 3
        elif kind == "adj":
            pred = lambda k, v, ts, s: v.x >= rd(s, "p")
        elif i < m - 1:
            pred = lambda k, v, ts, s, op=OPS[(i - 1) % 3]: op(v.x, rd(s, "p"))
        else:
            pred = lambda k, v, ts, s: (rd(s, "a") <= v.x) & (v.x < BASE[tp] + 1000)
        sel = b.select(f"S{i}").where(pred)
        if window and i == m - 1:
            sel = sel.within(window, W.TimeUnit.MILLISECONDS)
        if i == 0:
            sel = sel.fold("a", lambda k, v, c: v.x)
        b = sel.fold("p", lambda k, v, c: v.x).then() if i < m - 1 else sel
    return b.build()


def one(pred1, fold0=lambda k, v, c: v.x, pred0=lambda k, v, ts, s: v.x > 0, cols=("x",)):
    b = QueryBuilder(EventSchema({c: "int" for c in cols}))
    return (b.select("A").where(pred0).fold("p", fold0).then()
            .select("B").where(pred1).fold("q", lambda k, v, c: v.x).build())


def nine():
    b = QueryBuilder(EventSchema({"x": "int"}))
    for i in range(8):
        b = b.select(f"S{i}").where(lambda k, v, ts, s: v.x > 0).fold("p", lambda k, v, c: v.x).then()
    return b.select("S8").where(lambda k, v, ts, s: v.x > s.get("p")).build()


S, X = N.CEP_KIND_STENCIL, N.CEP_KIND_NFA
PLANS = [
    (lambda: W.rising_query(3, "int"), S, (2, [0], [1])),
    (lambda: W.rising_query(8, "long"), S, (2, [0], [2])),
    (lambda: chain("double", 4, "first"), S, (2, [0], [3])),
    (lambda: one(lambda k, v, ts, s: v.x > s.get("p") * 2), S, (0, [], [])),
    (lambda: one(lambda k, v, ts, s: v.x != s.get("p")), S, (0, [], [])),
    (lambda: one(lambda k, v, ts, s: (v.x > s.get("p")) & (v.y > 0), cols=("x", "y")), S, (0, [], [])),
    (lambda: one(lambda k, v, ts, s: v.x > s.getOrElse("p", 0)), X, None),
    (lambda: one(lambda k, v, ts, s: v.x > 1, pred0=lambda k, v, ts, s: v.x > s.get("p")), X, None),  # read in stage 0
    (lambda: one(lambda k, v, ts, s: v.x > s.get("q")), X, None),  # read in the only stage that folds it
    (lambda: one(lambda k, v, ts, s: v.x > s.get("p"), fold0=lambda k, v, c: c), X, None),
    (nine, X, None),
    (lambda: W.strict_abc_query(), S, (1, [0], [1])),
]


@pytest.mark.parametrize("case", range(len(PLANS)))
def test_lag_kind_and_plan(case):
    build, kind, plan = PLANS[case]
    q = N.Query(build().to_ir())
    assert q.kind == kind
    if plan:
        assert q.stencil_plan() == {"range": plan[0], "n_cols": len(plan[1]), "col_field": plan[1], "col_type": plan[2]}


@functools.lru_cache(maxsize=None)
def data(m, tp):
    """40 keys around the word (64) and chunk (4096) sizes, most starting inside a word; x a walk of steps
    -1, 0, 0, 1 (ties in half of them) wrapped into base - 4 .. base + 4; double: NaN, -0.0 and 0.0 sprinkled in; times
    a random walk"""
    head = [9000, 4097, 4096, 4095, 65, 64, 63, m, m - 1, 1, 0, 10]
    lens = np.array(head + (head[:-1] * 3)[:27], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rng, n = np.random.default_rng(70 + m), int(off[-1])
    x = np.cumsum(rng.choice([-1, 0, 0, 1], n)) % 9 - 4 + BASE[tp]  # (stays around the base)
    if tp == "double":
        x = x.astype(np.float64)
        u = rng.random(n)
        x[u < 0.01] = np.nan
        x[(u > 0.9) & (x == 0)] = -0.0
    ts = np.cumsum(rng.integers(-2, 8, n)).astype(np.int64)
    return off, x.astype({"int": np.int32, "long": np.int64, "double": np.float64}[tp]), ts


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["fast", "interp"])
@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("tp", ["int", "long", "double"])
def test_lag_parity(tp, m, route):
    from gpu_helpers import assert_parity, gpu_run
    off, x, _ = data(m, tp)
    for kind in ("adj", "first"):
        ir = chain(tp, m, kind, route).to_ir()
        r = oracle.run(ir, off, [x], threads=8)
        assert r["n_matches"] >= 100 and not r["err_code"].any(), (kind, r["n_matches"])
        s = N.Session(N.Query(ir))
        assert s.queries[0].stencil_plan()["range"] == (2 if route == "fast" else 0)
        g = gpu_run(ir, off, [x], session=s)
        assert g["kind"] == N.CEP_KIND_STENCIL and s.stats(0)["group"] == 0xFFFFFFFF
        assert_parity(g, r, off)


@pytest.mark.gpu
def test_lag_within():
    """A windowed lagged chain keeps the stencil and the extra pass"""
    from gpu_helpers import assert_parity, gpu_run
    off, x, ts = data(3, "int")
    pat = chain("int", 3, "adj", window=5)
    ir = pat.to_ir(semantic_within=True)
    r, par = oracle.run(ir, off, [x], ts=ts, threads=8), oracle.run(pat.to_ir(), off, [x], ts=ts, threads=8)
    assert 100 <= r["n_matches"] < par["n_matches"] and not r["err_code"].any()
    s = N.Session(N.Query(ir))
    g = gpu_run(ir, off, [x], ts=ts, session=s)
    assert g["kind"] == N.CEP_KIND_STENCIL and s.stats(0)["group"] == 0xFFFFFFFF and s.timing(0)[2] == 3
    assert_parity(g, r, off)


@pytest.mark.gpu
def test_lag_stream_runs_on_the_nfa():
    """A streaming session runs a lagged chain on the NFA path (the carry word holds no lagged values)"""
    from test_stencil_stream import run_batches
    rng = np.random.default_rng(5)  # (300 keys of 0..119 events: the NFA stream's capacity is not the subject)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 120, 300))]).astype(np.uint64)
    x = (np.cumsum(rng.choice([-1, 0, 0, 1], int(off[-1]))) % 9 - 4).astype(np.int32)
    ir = chain("int", 3, "first").to_ir()
    r = oracle.run(ir, off, [x], threads=8)
    assert r["n_matches"] >= 100 and not r["err_code"].any()
    s = N.Session(N.Query(ir), streaming=True, tier=N.CEP_TIER_INTERP)
    outs = run_batches(s, SS.split(off, [x], 4, seed=3))
    assert s.stats(0)["group"] != 0xFFFFFFFF and not outs[-1]["err_code"].any()
    assert SS.merge(outs) == SS.oracle_per_key(r, off)
