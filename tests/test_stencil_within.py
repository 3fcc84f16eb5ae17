"""Windowed strict chains under semantic WITHIN run on the stencil (stencil_within): exact against the oracle."""
import functools

import numpy as np
import pytest

import oracle
import stream_split as SS
from kafkastreams_cep_amd import EventSchema, QueryBuilder
from kafkastreams_cep_amd import native as N
from kafkastreams_cep_amd import processor as P
from kafkastreams_cep_amd import workloads as W

NB = 10


def wchain(plan, m, windows):
    """m ONE + strict stages, c0 == i % 4 as a range ("interp": c0 != (i + 1) % 4); windows: {stage: ms}"""
    b = QueryBuilder(EventSchema({"c0": "int" if plan == "interp" else plan}))
    for i in range(m):
        sel = b.select(f"S{i}").where((lambda k, v, ts, s, i=i: v.c0 != (i + 1) % 4) if plan == "interp" else
                                      (lambda k, v, ts, s, i=i: (v.c0 >= i % 4) & (v.c0 <= i % 4)))
        if i in windows:
            sel = sel.within(windows[i], W.TimeUnit.MILLISECONDS)
        b = sel.then() if i < m - 1 else sel
    return b.build()


def placement(m, place):
    """Stage t's window binds position t + 1 of a match (none for the last stage) and, inherited by
    stage t - 1, position t.  Times step by -2..7 (mean 2.5): 2.5 t expires about half at t + 1."""
    if place == "two":
        return {1: 2, m - 1: 5 * (m - 1) // 2 + 1} if m > 2 else {0: 1, 1: 2}
    return {m - 1: 5 * (m - 1) // 2} if place == "last" else {m // 2: 5 * (m // 2) // 2}


@functools.lru_cache(maxsize=None)
def data(m):
    """40 keys around the word (64) and chunk (4096) sizes, most starting inside a word; c0 = position in
    the key mod 4, a tenth redrawn; times a random walk that also steps backwards, around +-2^61 by key"""
    head = [9000, 4097, 4096, 4095, 65, 64, 63, m, m - 1, 1, 0, NB]
    lens = np.array(head + (head[:-1] * 3)[:27], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rng, n = np.random.default_rng(40 + m), int(off[-1])
    kid = np.repeat(np.arange(len(lens)), lens)
    x = np.where(rng.random(n) < 0.1, rng.integers(0, 4, n), (np.arange(n) - off[:-1].astype(np.int64)[kid]) % 4)
    ts = np.cumsum(rng.integers(-2, 8, n)) + np.where(kid % 2, -(1 << 61), 1 << 61)
    return off, lens, x, ts.astype(np.int64)


def test_windowed_chain_compiles_to_the_stencil():
    for plan in ("int", "double", "interp"):
        for m, place in [(3, "last"), (4, "middle"), (8, "two"), (2, "last")]:
            pat = wchain(plan, m, placement(m, place))
            q, plain = N.Query(pat.to_ir(semantic_within=True)), N.Query(wchain(plan, m, {}).to_ir(semantic_within=True))
            assert q.kind == plain.kind == N.CEP_KIND_STENCIL and q.stencil_plan() == plain.stencil_plan()
            assert "sk_window" in q.jit_source and q.info.n_stages == plain.info.n_stages  # the NFA build as before
            assert N.Query(pat.to_ir()).kind == N.CEP_KIND_STENCIL and "sk_window" not in N.Query(pat.to_ir()).jit_source
    assert N.Query(W.stock_query("readme").to_ir(semantic_within=True)).kind == N.CEP_KIND_NFA  # Kleene + skip


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["int", "double", "interp"])
@pytest.mark.parametrize("place", ["last", "middle", "two"])
@pytest.mark.parametrize("m", [2, 3, 4, 8])
def test_within_parity(m, place, plan):
    from gpu_helpers import assert_parity, gpu_run
    off, _, x, ts = data(m)
    cols = [x.astype(np.float64 if plan == "double" else np.int32)]
    pat = wchain(plan, m, placement(m, place))
    ir = pat.to_ir(semantic_within=True)
    r = oracle.run(ir, off, cols, ts=ts, threads=8)
    par = oracle.run(pat.to_ir(), off, cols, ts=ts, threads=8)
    assert r["n_matches"] >= 100 and not r["err_code"].any()
    assert r["n_matches"] < par["n_matches"] if m >= 3 else r["n_matches"] == par["n_matches"]  # the window prunes
    s = N.Session(N.Query(ir))
    g = gpu_run(ir, off, cols, ts=ts, session=s)
    assert g["kind"] == N.CEP_KIND_STENCIL and s.stats(0)["group"] == 0xFFFFFFFF
    assert s.timing(0)[2] == (3 if m >= 3 else 2)  # the pass runs only where a window can fire
    assert_parity(g, r, off)  # (err_code too: all zero above)


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["last", "middle"])
@pytest.mark.parametrize("m", [3, 8])
def test_within_stream(m, place):
    from test_stencil_stream import cut
    off, lens, x, ts = data(m)
    cols = [x.astype(np.int32), ts]
    counts = np.array([np.diff(ko.astype(np.int64)) for ko, _ in SS.split(off, cols, NB, seed=m)])
    # key starts at 4096, 4091 and 4094 of a batch; key 4 absent from a middle batch; key 11: one event a batch
    for k, first in [(0, [100, 4096, 4091]), (1, [50, 1000, 3]), (2, [10, 10, 2000]), (4, [20, 0, 25])]:
        counts[:, k] = (first + [lens[k] - sum(first)] + [0] * NB)[:NB]  # the rest in the next batch
    counts[:, 11] = 1
    batches, batch_of = cut(off, cols, counts)
    assert batches[1][0][1] == 4096 and batches[2][0][1] == 4091 and batches[2][0][2] == 4094
    pat = wchain("int", m, placement(m, place))
    q = N.Query(pat.to_ir(semantic_within=True))
    r = oracle.run(pat.to_ir(semantic_within=True), off, cols[:1], ts=ts, threads=8)  # (the survivors: a subset)
    par = oracle.run(pat.to_ir(), off, cols[:1], ts=ts, threads=8)

    def crossing(res):  # matches whose first and last event lie in different batches
        po, pp = res["pair_off"].astype(np.int64), res["pair_pos"].astype(np.int64)
        return int((batch_of[pp[po[:-1]]] != batch_of[pp[po[1:] - 1]]).sum())

    kept, pruned = crossing(r), crossing(par) - crossing(r)
    assert r["n_matches"] >= 100 and kept > 0 and pruned > 0 and not r["err_code"].any(), (kept, pruned)
    want = SS.oracle_per_key(r, off)

    def run(s, fresh_each_batch):
        outs = []
        for ko, cs in batches:
            s.push(ko, cs[:1], cs[1])
            outs.append(s.matches(0))
            assert not s.key_errors(0)[0].any() and s.stats(0)["group"] == 0xFFFFFFFF and s.timing(0)[2] == 4
            if fresh_each_batch:  # the state moves to a brand-new session after every batch
                s, blob = N.Session(q, streaming=True), s.snapshot()
                s.restore(blob)
        return s, SS.merge(outs)

    s, got = run(N.Session(q, streaming=True), True)
    s.reset()
    assert got == want and run(s, False)[1] == want


@pytest.mark.gpu
def test_within_processor():
    """The processor forwards the oracle's sequences of a windowed strict chain and runs on the stencil."""
    from test_processor import T0, forwarded_view
    rng, n, nk = np.random.default_rng(9), 240, 3
    kid = rng.integers(0, nk, n)
    by_key = np.argsort(kid, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(kid, minlength=nk))]).astype(np.uint64)
    v = np.zeros(n, np.int64)
    v[by_key] = (np.arange(n) - off[:-1].astype(np.int64)[kid[by_key]]) % 4  # 0, 1, 2, 3 in turn within a key
    t = T0 + np.cumsum(rng.integers(0, 12, n))
    pat, ctx = wchain("int", 3, {2: 20}), P.RecordContext("t", 0)
    proc = P.CEPProcessor(pat, batch_size=7, max_keys=8, semantic_within=True)
    proc.init(ctx)
    for i in range(n):
        ctx.send(int(kid[i]), {"c0": int(v[i])}, int(t[i]))
    proc.flush()
    assert proc.session.stats(0)["group"] == 0xFFFFFFFF
    proc.close()
    cols = [v[by_key].astype(np.int32)]
    r = oracle.run(pat.to_ir(semantic_within=True), off, cols, ts=t[by_key], threads=1)
    assert 3 <= r["n_matches"] < oracle.run(pat.to_ir(), off, cols, ts=t[by_key], threads=1)["n_matches"]
    names = N.Query(pat.to_ir()).stage_names
    po, pos, st = r["pair_off"].astype(np.int64), by_key[r["pair_pos"].astype(np.int64)], r["pair_stage"]
    order = np.argsort(by_key[r["emit_pos"].astype(np.int64)], kind="stable")
    assert forwarded_view(ctx) == [[(names[st[i]], [int(pos[i])]) for i in range(po[k], po[k + 1])] for k in order]
