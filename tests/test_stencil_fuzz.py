"""Seeded differential fuzz of the stencil routes (fuzz_chains.py) against the oracle: every chain must
compile to the route its generator predicts, and match the oracle bit for bit per batch, in arrival order, in
streaming sessions and next to other queries.  A failing case prints its chain (ChainRec.describe)."""
import functools
import types

import numpy as np
import pytest

import oracle
import stream_split as SS
from fuzz_chains import DT, FAMILIES, OPS, TYPES, random_chain, random_chain_stream, random_schema
from kafkastreams_cep_amd import native as N

# The seeds, chosen on the CPU so that the oracle's results meet test_fuzz_coverage (odd seeds draw their
# values from the special pools).
BATCH = {
    "range": [13, 1, 3, 5, 9, 11, 21, 35, 7, 19, 33, 0, 2, 4, 6, 8],
    "lag": [35, 3, 1, 5, 7, 36, 0, 2, 8, 18, 26, 4, 6, 9, 10, 11],
    "lagi": [27, 7, 0, 4, 9, 37, 2, 1, 3, 5, 6, 8, 10, 11, 12, 13],
    "interp": [19, 17, 7, 8, 18, 0, 20, 30, 2, 3, 4, 5, 6, 9, 10, 11],
}
ARRIVAL = {f: BATCH[f][:4] for f in FAMILIES}
STREAM = {f: BATCH[f][:6] for f in FAMILIES}
MIXED = [0, 1, 2, 3]
NFA_LEN = 120  # a streamed lag chain runs on the NFA: keys within its capacity (test_lag_stream_runs_on_the_nfa)

cases = lambda seeds: [pytest.param(f, s, id=f"{f}-{s}") for f in FAMILIES for s in seeds[f]]


@functools.lru_cache(maxsize=None)
def case(family, seed, short=False):
    """The chain, its stream and the oracle's results, shared by the tests (read-only): r the result the GPU
    must give for irs[0] (semantic WITHIN where the chain has a window), par the reference's own WITHIN."""
    pat, rec = random_chain(seed, family)
    off, cols, ts = random_chain_stream(seed, rec, max_len=NFA_LEN if short else None)
    c = types.SimpleNamespace(pat=pat, rec=rec, off=off, cols=cols, ts=ts if rec.needs_ts else None)
    c.ir = pat.to_ir()
    c.par = oracle.run(c.ir, off, cols, ts=c.ts, threads=8)
    c.sem_ir = pat.to_ir(semantic_within=True) if rec.windows else None
    c.sem = oracle.run(c.sem_ir, off, cols, ts=c.ts, threads=8) if rec.windows else None
    return c


def variants(c):
    """(ir, oracle result, semantic) of a case: the reference's WITHIN, and the semantic one of a windowed chain"""
    return [(c.ir, c.par, False)] + ([(c.sem_ir, c.sem, True)] if c.sem_ir else [])


# ---- without a GPU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,seed", cases(BATCH))
def test_fuzz_plan(family, seed):
    """A chain that falls to a slower route or to the NFA is a failure, not a skipped case."""
    pat, rec = random_chain(seed, family)
    for semantic in (False, True) if rec.windows else (False,):
        q = N.Query(pat.to_ir(semantic_within=semantic))
        assert q.kind == N.CEP_KIND_STENCIL, rec.describe()
        assert q.stencil_plan() == rec.plan, rec.describe()
    assert 1 <= rec.m <= 8 and (rec.m >= 2 or family in ("range", "interp"))


def coverage(seeds):
    """What the seeds with oracle matches cover, from the oracle alone."""
    cov = {"lag m": set(), "lag": set(), "op": set(), "lag type": set(), "lag special": set(), "type": set(),
           "special": set(), "window before the last stage": [], "semantic prunes": [], "no match": {}, "matches": {}}
    for f in FAMILIES:
        cov["no match"][f] = []
        for s in seeds[f]:
            c = case(f, s)
            rec, n = c.rec, [r["n_matches"] for _, r, _ in variants(c)]
            for _, r, _ in variants(c):
                assert not r["err_code"].any(), rec.describe()
            cov["matches"][f"{f}-{s}"] = n
            if min(n) == 0:
                cov["no match"][f].append(s)
                continue
            cov["type"] |= set(rec.types)
            if rec.special:
                cov["special"] |= set(rec.types)
            if f == "lag":
                cov["lag m"].add(rec.m)
                for _, d, op, tp in rec.lags:
                    cov["lag"].add(d)
                    cov["op"].add(op)
                    cov["lag type"].add(tp)
                    if rec.special:
                        cov["lag special"].add(tp)
            if any(t < rec.m - 1 for t in rec.windows):
                cov["window before the last stage"].append(f"{f}-{s}")
            if c.sem and 0 < c.sem["n_matches"] < c.par["n_matches"]:
                cov["semantic prunes"].append(f"{f}-{s}")
    return cov


def test_fuzz_coverage():
    cov = coverage(BATCH)
    for k, v in cov.items():
        print(f"{k}: {sorted(v) if isinstance(v, set) else v}")
    assert cov["lag m"] == set(range(2, 9)), cov["lag m"]
    assert cov["lag"] == set(range(1, 8)), cov["lag"]
    assert cov["op"] == set(OPS), cov["op"]
    assert cov["lag type"] == cov["lag special"] == cov["type"] == cov["special"] == set(TYPES)
    assert cov["window before the last stage"] and cov["semantic prunes"]
    for f in FAMILIES:
        assert len(set(BATCH[f])) == 16 and 10 * len(cov["no match"][f]) <= len(BATCH[f]), (f, cov["no match"][f])


# ---- with a GPU -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,seed", cases(BATCH))
def test_fuzz_batch(family, seed):
    from gpu_helpers import assert_parity, gpu_run
    c = case(family, seed)
    for ir, r, semantic in variants(c):
        what = f"{c.rec.describe()} semantic={semantic}"
        s = N.Session(N.Query(ir))
        assert s.queries[0].stencil_plan() == c.rec.plan, what
        g = gpu_run(ir, c.off, c.cols, ts=c.ts, session=s)
        assert g["kind"] == N.CEP_KIND_STENCIL and s.stats(0)["group"] == 0xFFFFFFFF, what
        assert s.timing(0)[2] == c.rec.launches(semantic), what
        try:
            assert_parity(g, r, c.off)
        except AssertionError as e:
            raise AssertionError(f"{what}\n{e}") from None


def interleave(off, seed):
    """-> (keys, pos): the stream's events in a random arrival order that keeps each key's own order"""
    rng = np.random.default_rng(seed)
    lens = np.diff(off.astype(np.int64))
    keys = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    rank = np.zeros(len(keys), np.int64)
    by_key = np.argsort(keys, kind="stable")
    rank[by_key] = np.arange(len(keys)) - np.repeat(off[:-1].astype(np.int64), lens)
    return keys.astype(np.uint32), off[:-1].astype(np.int64)[keys] + rank


@pytest.mark.gpu
@pytest.mark.parametrize("family,seed", cases(ARRIVAL))
def test_fuzz_arrival(family, seed):
    from gpu_helpers import assert_parity, session_result
    c = case(family, seed)
    ir, r, semantic = variants(c)[-1]
    what = f"{c.rec.describe()} semantic={semantic}"
    keys, pos = interleave(c.off, seed)
    s = N.Session(N.Query(ir))
    s.push_arrival(keys, [x[pos] for x in c.cols], len(c.off) - 1, None if c.ts is None else c.ts[pos])
    np.testing.assert_array_equal(s.layout()[0], c.off, what)
    assert s.stats(0)["group"] == 0xFFFFFFFF and s.timing(0)[2] == c.rec.launches(semantic), what
    try:
        assert_parity(session_result(s, 0, c.off, N.CEP_KIND_STENCIL), r, c.off)
    except AssertionError as e:
        raise AssertionError(f"{what}\n{e}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("family,seed", cases(STREAM))
def test_fuzz_stream(family, seed):
    """3..10 slices; range and interp chains keep the stencil (half of the seeds move to a fresh session through
    a snapshot after a random slice), lagged chains run on the NFA path"""
    lagged = family in ("lag", "lagi")
    c = case(family, seed, short=lagged)
    ir, r, semantic = variants(c)[0 if lagged else -1]  # (semantic WITHIN on the NFA needs the JIT tier)
    what = f"{c.rec.describe()} semantic={semantic}"
    rng = np.random.default_rng(1000 + seed)
    nb = int(rng.integers(3, 11))
    move = int(rng.integers(0, nb - 1)) if not lagged and rng.random() < 0.5 else -1
    stream = lambda: N.Session(N.Query(ir), streaming=True, tier=N.CEP_TIER_INTERP if lagged else N.CEP_TIER_JIT)
    s, outs = stream(), []
    for b, (ko, cs) in enumerate(SS.split(c.off, c.cols + ([] if c.ts is None else [c.ts]), nb, seed=seed)):
        s.push(ko, cs[:len(c.cols)], None if c.ts is None else cs[-1])
        m = s.matches(0)
        assert not s.key_errors(0)[0].any(), what
        assert (s.stats(0)["group"] != 0xFFFFFFFF) == lagged, what
        outs.append(m)
        if b == move:
            blob, s = s.snapshot(), stream()
            s.restore(blob)
    assert SS.merge(outs) == SS.oracle_per_key(r, c.off), what


@pytest.mark.gpu
@pytest.mark.parametrize("seed", MIXED)
def test_fuzz_mixed_session(seed):
    """Three chains of different families over one schema in one session, each against its own oracle run"""
    import random
    from gpu_helpers import assert_parity, session_result
    rng = random.Random(500 + seed)
    tps = rng.sample(TYPES, 3)
    shared = (tps, random_schema(rng, tps, seed % 2 == 1), seed % 2 == 1)
    chains = [random_chain(seed, f, shared) for f in rng.sample(FAMILIES, 3)]
    rec0 = chains[0][1]
    off, cols, ts = random_chain_stream(seed, rec0)
    irs = [pat.to_ir(semantic_within=bool(rec.windows)) for pat, rec in chains]
    qs = [N.Query(ir) for ir in irs]
    for q, (_, rec) in zip(qs, chains):
        assert q.kind == N.CEP_KIND_STENCIL and q.stencil_plan() == rec.plan, rec.describe()
    s = N.Session(qs)
    s.push(off, cols, ts)
    for i, (_, rec) in enumerate(chains):
        r = oracle.run(irs[i], off, cols, ts=ts, threads=8)
        assert not r["err_code"].any() and s.stats(i)["group"] == 0xFFFFFFFF, rec.describe()
        try:
            assert_parity(session_result(s, i, off), r, off)
        except AssertionError as e:
            raise AssertionError(f"query {i} of {[x.family for _, x in chains]}: {rec.describe()}\n{e}") from None


def lag_chain(tp, base):
    """x within 3 of the base; x <= the event before; x >= the event before; ... ; the 8th stage x >= the first
    event (a lag of 7)"""
    from kafkastreams_cep_amd import EventSchema, QueryBuilder
    b = QueryBuilder(EventSchema({"x": tp}))
    for i in range(8):
        if i == 0:
            sel = b.select("S0").where(lambda k, v, ts, s: (v.x >= base - 3) & (v.x <= base + 3))
            sel = sel.fold("a", lambda k, v, c: v.x, type=tp)
        elif i < 7:
            sel = b.select(f"S{i}").where((lambda k, v, ts, s: v.x <= s.get("p")) if i % 2 else
                                          (lambda k, v, ts, s: v.x >= s.get("p")))
        else:
            sel = b.select("S7").where(lambda k, v, ts, s: v.x >= s.get("a"))
        b = sel.fold("p", lambda k, v, c: v.x, type=tp).then() if i < 7 else sel
    return b.build()


@pytest.mark.gpu
@pytest.mark.parametrize("tp,route", [("int", "unaligned1"), ("int", "unaligned2"), ("int", "unaligned3"),
                                      ("long", "unaligned1"), ("double", "unaligned1"),
                                      ("int", "short"), ("long", "short"), ("double", "short")])
def test_lag_slow_routes(tp, route):
    """The lag fast kernel's one-event route (load1): a device column 1, 2 or 3 elements off a 16-byte boundary,
    and a batch of 100 events; a lag of 7 reaches before event 0 at the events 0..6."""
    from gpu_helpers import assert_parity, gpu_run
    w = np.dtype(DT[tp]).itemsize
    k = 16 // w if route == "short" else int(route[-1])  # elements before the column in its 16-byte aligned buffer
    n = 100 if route == "short" else 10000
    base = {"int": 0, "long": 1 << 40, "double": 0}[tp]
    off = np.array([0, 9, n // 3, n], np.uint64)
    x = (np.cumsum(np.random.default_rng(8).choice([-1, 0, 0, 1], n)) % 5 - 2 + base).astype(DT[tp])
    ir = lag_chain(tp, base).to_ir()
    assert N.Query(ir).stencil_plan()["range"] == 2
    r = oracle.run(ir, off, [x], threads=8)
    assert r["n_matches"] >= (1 if route == "short" else 50) and not r["err_code"].any(), r["n_matches"]
    pad = N.DeviceBuffer(w * (n + k))
    pad.upload(np.concatenate([np.full(k, base + 1, DT[tp]), x]))  # (what a lag before event 0 would read matches)
    kb = N.DeviceBuffer(off.nbytes)
    kb.upload(off)
    s = N.Session(N.Query(ir))
    s.push_device(N.DeviceStream(len(off) - 1, n, kb, [types.SimpleNamespace(ptr=pad.ptr + w * k)], keep=pad))
    assert s.stats(0)["group"] == 0xFFFFFFFF
    assert_parity(gpu_run(ir, off, [x], session=s, push=False), r, off)
