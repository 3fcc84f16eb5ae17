"""Strict chains in streaming sessions run the stencil with a per-key carry (stencil_edge), checked
against the oracle's single pass over the whole stream."""
import numpy as np
import pytest

import oracle
import stream_split as SS
from kafkastreams_cep_amd import native as N
from kafkastreams_cep_amd import workloads as W
from test_stencil_typed import DT, chain, mod4_chain

pytestmark = pytest.mark.gpu

NB = 10  # batches: more than the longest chain's 8 stages


def pattern(off, seed):
    """c0 = position in the key mod 4, a tenth redrawn (dense matches for 8 stages too); c1 from 0..9"""
    rng = np.random.default_rng(seed)
    n = int(off[-1])
    j = np.arange(n) - np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
    return np.where(rng.random(n) < 0.1, rng.integers(0, 4, n), j % 4), rng.integers(0, 10, n)


def cut(off, cols, counts):
    """counts[b, k] events of key k in batch b -> [(key_off_b, cols_b)], and each event's batch"""
    start = off[:-1].astype(np.int64) + np.cumsum(counts, axis=0) - counts
    out, batch_of = [], np.zeros(int(off[-1]), np.int64)
    for b in range(len(counts)):
        idx = np.concatenate([np.arange(a, a + c) for a, c in zip(start[b], counts[b])]).astype(np.int64)
        batch_of[idx] = b
        ko = np.concatenate([[0], np.cumsum(counts[b])]).astype(np.uint64)
        out.append((ko, [c[idx] for c in cols]))
    return out, batch_of


def run_batches(s, batches):
    outs = []
    for ko, cs in batches:
        s.push(ko, cs)
        m = s.matches(0)
        m["err_code"], m["err_seq"] = s.key_errors(0)
        outs.append(m)
    return outs


@pytest.mark.parametrize("m,ev", [(1, "int"), (2, "int"), (3, "long"), (8, "double"), (3, "int+double"),
                                  (8, "int+double"), (2, "interp"), (8, "interp"), (1, "double"), (2, "long")])
def test_stream_parity(m, ev):
    h = m - 1
    head = [9000, 4097, 4096, 4095, 65, 64, 63, h + 1, h, max(h - 1, 0), 1, 0, NB]
    lens = np.array(head + (head[:-1] * 3)[:27], np.int64)  # 40 keys
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x, y = pattern(off, 7 + m)
    types = ["int"] if ev == "interp" else ev.split("+")
    cols = [v.astype(DT[t]) for v, t in zip((x, y), types)]
    counts = np.array([np.diff(ko.astype(np.int64)) for ko, _ in SS.split(off, cols, NB, seed=m)])

    def place(k, first):  # key k: `first` in batches 0.., the rest in the next batch
        counts[:, k] = 0
        counts[:len(first), k] = first
        counts[len(first), k] = lens[k] - sum(first)

    place(0, [100, 4096, 4091])  # key 1 starts on event 4096 of batch 1, at 4091 of batch 2
    place(1, [50, 1000, 3])      # key 2 starts at 4094 of batch 2: within 8 events of the wave boundary
    place(2, [10, 10, 2000])
    place(4, [20, 0, 25])        # absent from a middle batch
    counts[:, 12] = 1            # one event per batch, for more than m batches
    batches, batch_of = cut(off, cols, counts)
    assert batches[1][0][1] == 4096 and batches[2][0][1] == 4091 and batches[2][0][2] == 4094

    if ev == "interp":  # a != stage is no range: interpreted predicates
        ir = chain(["int"], [lambda x, i=i: x != (i + 1) % 4 for i in range(m)]).to_ir()
    else:
        ir = mod4_chain(types, m).to_ir()
    q = N.Query(ir)
    assert q.kind == N.CEP_KIND_STENCIL and q.stencil_plan()["range"] == (0 if ev == "interp" else 1)
    r = oracle.run(ir, off, cols, threads=8)
    po, pp = r["pair_off"].astype(np.int64), r["pair_pos"].astype(np.int64)
    crossing = int((batch_of[pp[po[:-1]]] != batch_of[pp[po[1:] - 1]]).sum())
    assert r["n_matches"] > 100 and (crossing > 0 or m == 1), (r["n_matches"], crossing)  # (m = 1: one event)
    outs = run_batches(N.Session(q, streaming=True), batches)
    assert SS.merge(outs) == SS.oracle_per_key(r, off)
    assert not any(o["err_code"].any() for o in outs)


@pytest.fixture(scope="module")
def abc():
    off, cols = W.generate(W.SynthConfig("t", "abc", 300, 60, 0xCE90000 + 2))
    ir = W.strict_abc_query().to_ir()
    return ir, off, cols, SS.oracle_per_key(oracle.run(ir, off, cols, threads=8), off), SS.split(off, cols, 4, seed=4)


def test_stream_takes_the_stencil(abc):
    ir, off, cols, want, parts = abc
    s, nfa = N.Session(N.Query(ir), streaming=True), N.Session(N.Query(ir), streaming=True, force_nfa=True)
    a, b = run_batches(s, parts), run_batches(nfa, parts)
    assert s.stats(0)["group"] == 0xFFFFFFFF and s.timing(0)[2] == 3 and nfa.stats(0)["group"] != 0xFFFFFFFF
    assert SS.merge(a) == SS.merge(b) == want


def abc_floor(off, v, seen):
    """cep_live_floor's formula for SEQ(A, B, C) over each key's first seen[k] events"""
    out = np.full(len(seen), 0xFFFFFFFF, np.uint32)
    for k, n in enumerate(seen.tolist()):
        x = v[int(off[k]):int(off[k]) + n]
        if n >= 2 and x[-2] < 4 and 4 <= x[-1] < 8:
            out[k] = n - 2
        elif n >= 1 and x[-1] < 4:
            out[k] = n - 1
    return out


@pytest.mark.parametrize("service", ["snapshot", "reset", "floor", "reject"])
def test_stream_services(abc, service):
    ir, off, cols, want, parts = abc
    s, nfa = N.Session(N.Query(ir), streaming=True), N.Session(N.Query(ir), streaming=True, force_nfa=True)
    if service == "reset":
        run_batches(s, parts[:2])
        s.reset()
        assert SS.merge(run_batches(s, parts)) == want
        return
    if service == "reject":  # a blob of the other path's state
        run_batches(s, parts[:1])
        run_batches(nfa, parts[:1])
        with pytest.raises(N.CepError):
            N.Session(N.Query(ir), streaming=True).restore(nfa.snapshot())
        with pytest.raises(N.CepError):
            N.Session(N.Query(ir), streaming=True, force_nfa=True).restore(s.snapshot())
        return
    outs, seen = [], np.zeros(len(off) - 1, np.int64)
    for ko, cs in parts:
        outs += run_batches(s, [(ko, cs)])
        if service == "snapshot":  # the state moves to a brand-new session after every batch
            blob = s.snapshot()
            s = N.Session(N.Query(ir), streaming=True)
            s.restore(blob)
        else:
            nfa.push(ko, cs)
            seen += np.diff(ko.astype(np.int64))
            floor = s.live_floor(0)
            np.testing.assert_array_equal(floor, abc_floor(off, cols[0], seen))
            assert (floor >= nfa.live_floor(0)).all()
    assert SS.merge(outs) == want


def test_stream_arrival_order_dense():
    """1000 keys with 2 events a batch in arrival order: four stencil_edge blocks on the dense route"""
    nk, per, nb = 1000, 2, 3
    off = (np.arange(nk + 1) * per * nb).astype(np.uint64)
    v = pattern(off, 3)[0].astype(np.int32)
    ir = mod4_chain(["int"], 3).to_ir()
    r = oracle.run(ir, off, [v], threads=8)
    assert r["n_matches"] > 100
    rng = np.random.default_rng(11)
    s, outs = N.Session(N.Query(ir), streaming=True), []
    for b in range(nb):
        keys = rng.permutation(np.repeat(np.arange(nk), per))
        j = np.zeros(nk * per, np.int64)
        j[np.argsort(keys, kind="stable")] = np.arange(nk * per) % per  # the event's rank within its key
        s.push_arrival(keys, [v[off[keys].astype(np.int64) + per * b + j]], nk)
        outs.append(s.matches(0))
    assert SS.merge(outs) == SS.oracle_per_key(r, off)
