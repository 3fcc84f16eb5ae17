"""CPU build of cep_decode_json's state machine, number path and table builders (csrc/json_generic.h)
- test infrastructure - and what its CPU and GPU tests share: the number corpus, the references."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np

import json_cpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRECISION = 8
DTYPES = {1: np.int32, 2: np.int64, 3: np.float64}
_lib = None


class Field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_uint8)]


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cep_json_generic_cpu.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               f"-I{json_cpu.CSRC}", os.path.join(HERE, "json_generic_cpu", "json_generic_cpu.cpp"),
                               "-o", out])
        _lib = C.CDLL(out)
        _lib.jg_decode.restype = C.c_char_p
    return _lib


def pow5_table():
    out = np.zeros(2 * 651, np.uint64)
    lib().jg_pow5(out.ctypes.data_as(C.c_void_p))
    return out.reshape(-1, 2)


def decode(records, fields, span_field=None):
    """fields: [(name bytes, type code)] -> (status, [columns], spans); ValueError for a bad table."""
    buf, off = json_cpu.pack(records)
    n = len(records)
    cols = [np.zeros(n, DTYPES.get(t, np.int64)) for _, t in fields]
    st, span = np.zeros(n, np.int32), np.zeros(2 * n, np.uint32)
    fa = (Field * max(1, len(fields)))(*[Field(nm, t) for nm, t in fields])
    ca = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
    msg = lib().jg_decode(C.c_void_p(buf.ctypes.data + 8), off.ctypes.data_as(C.c_void_p), C.c_uint64(n), fa,
                          C.c_uint32(len(fields)), ca, span_field, span.ctypes.data_as(C.c_void_p),
                          st.ctypes.data_as(C.c_void_p))
    if msg is not None:
        raise ValueError(msg.decode())
    return st, cols, span.reshape(-1, 2)


def reference(record: bytes, fields):
    """(status, values) of the typed getters on a well-formed record (json.loads: last duplicate wins)"""
    o = json.loads(record)
    vals, st = [], 0
    for nm, t in fields:
        v = o.get(nm.decode())
        if v is None:
            st = st or 3
        elif isinstance(v, bool) or not isinstance(v, (int, float) if t == 3 else int):
            st = st or 2
        vals.append(v)
    if not st and any(t == 1 and not -2**31 <= v < 2**31 for (_, t), v in zip(fields, vals)):
        st = 6
    return st, [0 if st else (float(v) if t == 3 else v) for (_, t), v in zip(fields, vals)]


BOUNDARY = ["4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.2250738585072014e-308",
            "1.7976931348623157e308", "1.7976931348623159e308", "1e309", "1e-400", "-0.0", "0e999", "1E+2",
            "9007199254740993.0", "0.1000000000000000055511151231257827", "1234567890" * 4 + ".0"]
EXACT = ["123.45", "1e22", "0.001", "1.0", "-2.5e-3", "9007199254740992.0", "1.5E22", "0.000000000000000000001",
         "100000000000000.0e8", "7e-22", "123456789012345e7", "0.30", "12345.678e-10", "-1e0"]


def random_doubles(n, seed=20240229):  # finite doubles drawn by random bit pattern
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x = rng.integers(0, 2**64, 2 * n, dtype=np.uint64).view(np.float64)
        out += [float(v) for v in x[np.isfinite(x)]]
    return out[:n]


def decimal_form(s):
    """(significant digits, power of ten of the last digit written) of a decimal literal"""
    m, _, e = s.lower().lstrip("-").partition("e")
    ip, _, fp = m.partition(".")
    return len((ip + fp).lstrip("0").rstrip("0")), int(e or 0) - len(fp)


def check_doubles(texts, status, col):
    """Every result that is not PRECISION bit-equal to float(text), none undecided among <= 15
    significant digits with |q| <= 22 -> the number of PRECISION records."""
    got = np.asarray(col).view(np.uint64)
    n_prec = 0
    for s, st, g in zip(texts, status, got):
        if st == PRECISION:
            nd, q = decimal_form(s)
            assert not (nd <= 15 and abs(q) <= 22), s
            assert g == 0, s
            n_prec += 1
        else:
            assert st == 0 and g.tobytes() == struct.pack("<d", float(s)), (s, st, hex(int(g)))
    return n_prec
