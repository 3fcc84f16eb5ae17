"""cep_decode_json's host build (csrc/json_generic.h) against Python: the powers-of-five table, the
decimal-to-double path by bit pattern, the argument checks (the state machine: test_gpu_json_generic)."""
import ctypes as C

import pytest

import json_generic_cpu as G
from kafkastreams_cep_amd import native as N


def test_pow5_table_matches_python_integers():
    got = G.pow5_table()
    for q in range(-342, 309):
        if q >= 0:
            c = 5 ** q
        else:
            p = 5 ** -q
            z = (p - 1).bit_length()  # the least z with 2^z >= p
            c = 2 ** (z + 127 if q >= -27 else 2 * z + 128) // p + 1
        c = c << (128 - c.bit_length()) if c.bit_length() < 128 else c >> (c.bit_length() - 128)
        assert (int(got[q + 342, 0]), int(got[q + 342, 1])) == (c >> 64, c & (2**64 - 1)), q


def _numbers(cls):
    if cls == "exact":
        return G.EXACT
    if cls == "boundary":
        return G.BOUNDARY + ["-" + s for s in G.BOUNDARY if s[0] != "-"]
    xs = G.random_doubles(20000)
    return [repr(x) for x in xs] if cls == "repr" else ["%.15g" % x for x in xs]


@pytest.mark.parametrize("cls", ["exact", "boundary", "repr", "g15"])
def test_numbers_vs_float(cls):
    texts = _numbers(cls)
    st, cols, _ = G.decode([b'{"x":%s}' % s.encode() for s in texts], [(b"x", 3)])
    n_prec = G.check_doubles(texts, st, cols[0])
    print(f"{cls}: {n_prec} of {len(texts)} PRECISION")
    if cls == "exact":
        assert n_prec == 0
    if cls == "repr":
        assert n_prec * 1000 <= len(texts)


BAD_TABLES = {
    "0 fields": [],
    "33 fields": [(b"f%d" % i, 1) for i in range(33)],
    "empty name": [(b"a", 1), (b"", 2)],
    "65-byte name": [(b"n" * 65, 1)],
    "non-ASCII name": [("é".encode(), 1)],
    "duplicate name": [(b"a", 1), (b"b", 3), (b"a", 2)],
    "unknown type": [(b"a", 4)],
}


@pytest.mark.parametrize("what", BAD_TABLES)
def test_bad_field_table_is_invalid(what):
    bad = BAD_TABLES[what]
    with pytest.raises(ValueError):
        G.decode([b"{}"], bad)
    G.decode([b"{}"], [(b"n" * 64, 1)] + [(b"f%d" % i, 1 + i % 3) for i in range(31)])  # the limits themselves hold
    # cep_decode_json itself: CEP_E_INVALID with a message before any pointer is followed
    fa = (N.JsonField * max(1, len(bad)))(*[N.JsonField(nm, t) for nm, t in bad])
    cols = (C.c_void_p * max(1, len(bad)))(*[8] * len(bad))
    assert N.lib().cep_decode_json(0, 8, 8, 1, fa, len(bad), cols, None, None, 8, None) == -1
    assert N.lib().cep_last_error()
