"""Seeded random strict chains and streams for differential testing of the stencil routes (GPU vs oracle).

`random_chain(seed, family)` draws a SEQ of ONE + strict stages that stays inside the stencil gate of
compile.cpp by construction (total predicates and folds, distinct names, at most 8 stages) and says which
route it must compile to:

  range   conjunctions of `field OP const` over one or two columns         stencil_plan()["range"] == 1
  lag     one column; a stage: a range and one `x OP state.get(S)`         == 2 (StEvalLag)
  lagi    a lag chain with one feature the fast route has no form for      == 0 (StEvalLagI)
  interp  a state-free chain that is no range                              == 0

`random_chain_stream(seed, rec)` draws a CSR stream for it: key lengths around the chain length, the
word (64) and the chunk (4096), values from an alphabet of five per column - around a base, or the
type's extremes - and times that also step backwards.
"""
import math
import random

import numpy as np

from kafkastreams_cep_amd import EventSchema, QueryBuilder, TimeUnit
from kafkastreams_cep_amd import expr as X

FAMILIES = ("range", "lag", "lagi", "interp")
TYPES = ("int", "long", "double")
TCODE = {"int": 1, "long": 2, "double": 3}
DT = {"int": np.int32, "long": np.int64, "double": np.float64}
OPS = ("<", "<=", ">", ">=", "==")
_CMP = {"<": X.OP_LT, "<=": X.OP_LE, ">": X.OP_GT, ">=": X.OP_GE, "==": X.OP_EQ, "!=": X.OP_NE}
_FLIP = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "==": "==", "!=": "!="}
LAGI_FEATURES = ("arith", "ne", "or", "col2", "foldexpr", "ts")
INTERP_FEATURES = ("ne", "or", "cast", "three", "ts")

NAN, INF, TINY, DMAX = float("nan"), float("inf"), 5e-324, 1.7976931348623157e308
BASE = {"int": 0, "long": 1 << 40, "double": 0.0}
SPECIAL = {
    "int": [-(1 << 31), (1 << 31) - 1, -1, 0, 1],
    # pairs that differ in the low word only, in the high word only, or only below a double's precision
    "long": [-(1 << 63), (1 << 63) - 1, 1 << 53, (1 << 53) + 1, 1 << 32, (1 << 32) + 1, 1, 0, -(1 << 53) - 1],
    "double": [NAN, -NAN, 0.0, -0.0, INF, -INF, TINY, -TINY, 1.5, -1.5, DMAX],
}


def _ordered(vals):
    """the values in their type's order, NaNs last (a walk over neighbours meets `<`, `==` and `>` alike)"""
    nans = [v for v in vals if v != v]
    return sorted((v for v in vals if v == v), key=lambda v: (v, math.copysign(1, v))) + nans  # (-0.0 before 0.0)


def random_schema(rng, types, special):
    """per column an alphabet of at most five values: base - 2 .. base + 2, or five of the type's special pool"""
    alpha = []
    for t in types:
        if special:
            alpha.append(_ordered(rng.sample(SPECIAL[t], 5)))
        else:
            alpha.append([BASE[t] + d for d in (-2, -1, 0, 1, 2)])
    return alpha


class ChainRec:
    """What random_chain drew, and what the chain must compile to."""

    def __init__(self, family, seed):
        self.family, self.seed = family, seed
        self.types = []        # the schema: the type of column c0, c1 ..
        self.alpha = []        # per column its alphabet, in order
        self.special = False   # the alphabets come from the special pools
        self.m = 0
        self.reads_ts = False
        self.windows = {}      # stage -> ms
        self.plan = None       # stencil_plan()
        self.lags = []         # (stage, lag, op with the field on the left, column type) of every lag conjunct
        self.feature = None    # lagi, interp: what keeps the chain off the fast routes
        self.text = ""

    @property
    def needs_ts(self):
        return self.reads_ts or bool(self.windows)

    def launches(self, semantic):
        """matching launches of a per-batch session: stencil_mask and stencil_emit, and stencil_within where a
        window can fire - the window of a stage 1.. of a chain of three or more (a stage without one takes its
        successor's; stage 0's and the last position's never expire a run)"""
        return 3 if semantic and self.m >= 3 and any(t >= 1 for t in self.windows) else 2

    def describe(self):
        return (f"{self.family}/{self.seed}: {'+'.join(self.types)} m={self.m} {'special' if self.special else 'plain'}"
                f"{' ' + self.feature if self.feature else ''} ts={int(self.reads_ts)} within={self.windows} "
                f"lags={[(t, d, op) for t, d, op, _ in self.lags]} plan={self.plan['range']} | {self.text}")


# ---- predicates: built as expr nodes, so that a constant can stand on either side ------------------------
def _lit(tp, c):
    return X.Const(TCODE[tp], c)


def _cmp(op, a, b, swap):
    """a OP b, written b OP' a when swap"""
    return X.Cmp(_CMP[_FLIP[op]], b, a) if swap else X.Cmp(_CMP[op], a, b)


def _atom(spec, types, v, ts, s):
    kind = spec[0]
    if kind == "cmp":  # field OP const
        _, c, op, k, swap = spec
        return _cmp(op, getattr(v, f"c{c}"), _lit(types[c], k), swap)
    if kind == "lag":  # field OP state.get(S) [+ k | * k]
        _, c, op, st, swap, arith = spec
        y = s.get(st)
        if arith:
            y = y + _lit(types[c], arith[1]) if arith[0] == "+" else y * _lit(types[c], arith[1])
        return _cmp(op, getattr(v, f"c{c}"), y, swap)
    if kind == "or":
        return X.Or(_atom(spec[1], types, v, ts, s), _atom(spec[2], types, v, ts, s))
    if kind == "cast":  # an int or long field against a double constant
        _, c, op, k, swap = spec
        return _cmp(op, getattr(v, f"c{c}"), X.Const(X.F64, k), swap)
    if kind == "ts":  # Java's remainder of a time that may be negative
        return X.Cmp(X.OP_NE, ts % X.Const(X.I64, 3), X.Const(X.I64, 0))
    raise ValueError(kind)


def _pred(specs, types):
    def fn(k, v, ts, s):
        e = None
        for spec in specs:
            a = _atom(spec, types, v, ts, s)
            e = a if e is None else X.And(e, a)
        return e
    return fn


def _fold(spec):
    if spec[0] == "col":
        return lambda k, v, c, j=spec[1]: getattr(v, f"c{j}")
    return lambda k, v, c, a=spec[1], b=spec[2]: getattr(v, f"c{a}") * 2 - getattr(v, f"c{b}")  # "expr"


def _range_specs(rng, c, alpha, tight=0.15):
    """one or two `field OP const` conjuncts on column c that accept most of its alphabet (the bounds sit on
    alphabet values; a NaN is never a bound)"""
    a = [x for x in alpha if x == x]
    r = rng.random()
    if r < tight:
        return [("cmp", c, "==", rng.choice(a), rng.random() < 0.5)]
    lo = [(">=", a[rng.choice([0, 0, 1])]), (">", a[0])]
    hi = [("<=", a[rng.choice([-1, -1, -2])]), ("<", a[-1])]
    picks = [rng.choice(lo)] if r < 0.4 else [rng.choice(hi)] if r < 0.65 else [rng.choice(lo), rng.choice(hi)]
    rng.shuffle(picks)
    return [("cmp", c, op, k, rng.random() < 0.5) for op, k in picks]


def _lag_stages(rng, rec, c, m):
    """the stages of a lag chain on column c: [(conjunct specs, {state: fold spec})]"""
    states = ["a", "b"][:rng.choice([1, 2])]
    refold = rng.choice([0.15, 0.5, 0.5, 0.85])  # about 1/2 over the seeds; the ends give lags of 7 and chains of 1s
    last = {st: 0 for st in states}
    stages = [(_range_specs(rng, c, rec.alpha[c], tight=0), {st: ("col", c) for st in states})]
    for t in range(1, m):
        specs = _range_specs(rng, c, rec.alpha[c], tight=0) if rng.random() < 0.5 else []
        if rng.random() < 0.85:
            st, op = rng.choice(states), rng.choice(OPS)
            specs.insert(rng.randint(0, len(specs)), ("lag", c, op, st, rng.random() < 0.5, None))
            rec.lags.append((t, t - last[st], op, rec.types[c]))
        folds = {}
        for st in states:
            if t < m - 1 and rng.random() < refold:
                folds[st] = ("col", c)
                last[st] = t
        stages.append((specs, folds))
    if not rec.lags:  # (a chain without a read is a range chain)
        st, op = rng.choice(states), rng.choice(OPS)
        stages[-1][0].append(("lag", c, op, st, rng.random() < 0.5, None))
        rec.lags.append((m - 1, m - 1 - last[st], op, rec.types[c]))
    for t in range(1, m):
        if not stages[t][0]:  # every stage has a predicate
            stages[t] = (_range_specs(rng, c, rec.alpha[c], tight=0), stages[t][1])
    return stages


def random_chain(seed, family, shared=None):
    """-> (pattern, ChainRec).  shared = (types, alphabets, special): the chain over that schema (several queries
    of one session), else over a schema of its own."""
    rng = random.Random(seed * len(FAMILIES) + FAMILIES.index(family))
    rec = ChainRec(family, seed)
    own = shared is None
    if own:
        rec.special = seed % 2 == 1
    else:
        rec.types, rec.alpha, rec.special = list(shared[0]), [list(a) for a in shared[1]], shared[2]
    feature = None
    if family == "lagi":
        feature = rec.feature = rng.choice(LAGI_FEATURES)
    elif family == "interp":
        feature = rec.feature = rng.choice(INTERP_FEATURES)
    if own:
        if family == "range":
            rec.types = [rng.choice(TYPES) for _ in range(rng.choice([1, 2, 2]))]
        elif family == "lag":
            rec.types = [rng.choice(TYPES)]
        elif family == "lagi":
            t = rng.choice(TYPES)
            rec.types = [t, t] if feature == "foldexpr" else [t, rng.choice(TYPES)] if feature == "col2" else [t]
        else:
            n = 3 if feature == "three" else rng.choice([1, 2])
            rec.types = [rng.choice(TYPES) for _ in range(n)]
            if feature == "cast":
                rec.types[0] = rng.choice(["int", "long"])
        rec.alpha = random_schema(rng, rec.types, rec.special)
    nc = len(rec.types)
    m = rec.m = rng.randint(2 if family in ("lag", "lagi") else 1, 8)
    stages = []  # [(conjunct specs, {state: fold spec})]
    order = []   # the columns the ranges constrain, in first appearance

    def ranged(t_specs):
        for spec in t_specs:
            if spec[0] == "cmp" and spec[1] not in order:
                order.append(spec[1])

    if family == "range":
        cols = rng.sample(range(nc), min(nc, 2))
        for t in range(m):
            specs = []
            use = [c for c in cols if rng.random() < 0.75] or [rng.choice(cols)]  # some stages leave a column free
            for c in use:
                specs += _range_specs(rng, c, rec.alpha[c])
            rng.shuffle(specs)
            ranged(specs)
            stages.append((specs, {}))
        tps = [TCODE[rec.types[c]] for c in order]
        if len(order) == 2 and tps[0] != 1 and tps[1] == 1:  # a mixed pair runs as (4-byte, 8-byte)
            order.reverse()
            tps.reverse()
        rec.plan = {"range": 1, "n_cols": len(order), "col_field": order, "col_type": tps}
    elif family == "lag":
        c = rng.randrange(nc)
        stages = _lag_stages(rng, rec, c, m)
        rec.plan = {"range": 2, "n_cols": 1, "col_field": [c], "col_type": [TCODE[rec.types[c]]]}
    elif family == "lagi":
        if feature == "foldexpr":  # two columns of one type
            pairs = [(a, b) for a in range(nc) for b in range(nc) if a != b and rec.types[a] == rec.types[b]]
            c, c2 = rng.choice(pairs) if pairs else (rng.randrange(nc), None)
            if c2 is None:
                feature = rec.feature = "arith"
        else:
            c = rng.randrange(nc)
            c2 = rng.choice([j for j in range(nc) if j != c]) if nc > 1 else None
            if feature == "col2" and c2 is None:
                feature = rec.feature = "ne"
        stages = _lag_stages(rng, rec, c, m)
        t, d, op, _ = rng.choice(rec.lags)  # the conjunct that changes
        i = next(i for i, sp in enumerate(stages[t][0]) if sp[0] == "lag")
        lag = stages[t][0][i]
        if feature == "arith":
            stages[t][0][i] = lag[:5] + (rng.choice([("+", 0), ("+", 1), ("*", 2)]),)
        elif feature == "ne":
            stages[t][0][i] = ("lag", c, "!=", lag[3], lag[4], None)
            rec.lags[rec.lags.index((t, d, op, rec.types[c]))] = (t, d, "!=", rec.types[c])
        elif feature == "or":
            stages[t][0][i] = ("or", lag, ("cmp", c, "==", rng.choice([x for x in rec.alpha[c] if x == x]), False))
        elif feature == "col2":
            stages[rng.randrange(m)][0].extend(_range_specs(rng, c2, rec.alpha[c2], tight=0))
        elif feature == "foldexpr":  # the state the conjunct reads is folded as an expression where it was the column
            st = lag[3]
            u = t - d
            stages[u][1][st] = ("expr", c, c2)
        else:
            stages[rng.randrange(m)][0].append(("ts",))
            rec.reads_ts = True
        rec.plan = {"range": 0, "n_cols": 0, "col_field": [], "col_type": []}
    else:
        cols = list(range(nc)) if feature == "three" else rng.sample(range(nc), min(nc, 2))
        if feature == "cast":
            ints = [j for j in range(nc) if rec.types[j] != "double"]
            if ints:
                cols = [rng.choice(ints)] + [j for j in cols if j not in ints][:1]
            else:
                feature = rec.feature = "ne"
        odd = rng.randrange(m)  # the stage that is no range
        for t in range(m):
            specs = []
            use = [c for c in cols if rng.random() < 0.75] or [rng.choice(cols)]
            if feature == "three" and t == odd:
                use = cols
            for c in use:
                specs += _range_specs(rng, c, rec.alpha[c])
            if t == odd:
                c = cols[0]
                a = [x for x in rec.alpha[c] if x == x]
                if feature == "ne":
                    specs.append(("cmp", c, "!=", rng.choice(a), rng.random() < 0.5))
                elif feature == "or":
                    specs.append(("or", ("cmp", c, "<=", a[1], rng.random() < 0.5), ("cmp", c, ">", a[2], rng.random() < 0.5)))
                elif feature == "cast":
                    specs.append(("cast", c, rng.choice(["<", ">="]), float(a[2]) + 0.5, rng.random() < 0.5))
                elif feature == "ts":
                    specs.append(("ts",))
                    rec.reads_ts = True
            stages.append((specs, {}))
        rec.plan = {"range": 0, "n_cols": 0, "col_field": [], "col_type": []}

    if rng.random() < 1 / 3:  # WITHIN on one to three stages, not only the last; times step by 2.5 on average
        for t in rng.sample(range(m), min(m, rng.randint(1, 3))):
            rec.windows[t] = max(1, int(2.5 * t) + rng.randint(-1, 2))

    b = QueryBuilder(EventSchema({f"c{j}": t for j, t in enumerate(rec.types)}))
    for t, (specs, folds) in enumerate(stages):
        sel = b.select(f"S{t}").where(_pred(specs, rec.types))
        for st, f in folds.items():
            sel = sel.fold(st, _fold(f), type=rec.types[f[1]])
        if t in rec.windows:
            sel = sel.within(rec.windows[t], TimeUnit.MILLISECONDS)
        b = sel.then() if t < m - 1 else sel
    pat = b.build()
    rec.text = "; ".join(line.split(" where ", 1)[1] for line in pat.describe().split("\n"))
    return pat, rec


BOUNDARY = (63, 64, 65, 4095, 4096, 4097, 9000)


def random_chain_stream(seed, rec, max_len=None, n_keys=30, cap=40000):
    """-> (key_off, cols, ts).  About n_keys keys with lengths 0, 1, m - 1, m, m + 1, the word and chunk sizes
    +- 1, 9000 and a few random ones, in random order, `cap` events at the most; a key starts inside a wave
    and the last wave is partial.  max_len: keys of 0..max_len events (the NFA stream's capacity), 10 n_keys."""
    rng = np.random.default_rng([seed, FAMILIES.index(rec.family), 77])
    m = rec.m
    if max_len is None:
        lens = [0, 1, m - 1, m, m + 1, *BOUNDARY]
        for extra in rng.permutation(BOUNDARY[3:]):  # a second long key while the total allows
            if sum(lens) + extra + 300 * (n_keys - len(lens) - 1) <= cap:
                lens.append(int(extra))
                break
        lens += rng.integers(2, 300, n_keys - len(lens)).tolist()
        lens = rng.permutation(np.array(lens, np.int64))
        if not (np.cumsum(lens)[:-1] % 64).any():  # a key starts inside a word
            lens = np.concatenate([[m + 1], lens])
        if lens.sum() % 64 == 0:  # the last word, and with it the last chunk, is partial
            lens = np.concatenate([lens, [3]])
    else:
        lens = rng.integers(0, max_len + 1, 10 * n_keys)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    cols = []
    for tp, alpha in zip(rec.types, rec.alpha):
        # a walk over neighbours (ties in half of the steps), a third of the events redrawn
        step = np.where(rng.random(n) < 0.3, rng.integers(0, len(alpha), n), rng.choice([-1, 0, 0, 1], n))
        cols.append(np.array(alpha, DT[tp])[np.cumsum(step) % len(alpha)])
    kid = np.repeat(np.arange(len(lens)), lens)
    ts = np.cumsum(rng.integers(-2, 8, n)) + np.where(kid % 2, -(1 << 61), 1 << 61)  # (some steps negative)
    return off, cols, ts.astype(np.int64)
