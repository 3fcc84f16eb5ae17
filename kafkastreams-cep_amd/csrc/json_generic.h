// json_generic.h — the schema-driven JSON decoder's per-record state machine (cep_decode_json,
// ingest_generic.hip): json-simple 1.1.1's scanner and parser as json_parser.h restates them
// (same whitespace, INT / DOUBLE longest match, escapes, skipped commas and colons, depth limit
// and failure codes), followed by typed getters over a field table instead of StockEvent's
// three fixed keys:
//   int / long   (Long) o.get(name)                 an INT token, else ClassCastException
//   double       ((Number) o.get(name)).doubleValue() an INT token ((double) of the long) or a
//                DOUBLE token (Double.valueOf(text): correctly rounded, half-even)
// Plain C++ with __device__ markers like json_parser.h: ingest_generic.hip runs it one lane per
// record, tests/json_generic_cpu compiles it for the host with the markers defined away.
//
// Keys: a running FNV-1a hash and length of the unescaped key text are carried through the
// string states of top-level keys only; at the closing quote hash + length are compared against
// the table and a hit is verified byte by byte (re-reading the raw key text).  Values are stored
// to their column as they are lexed (the last write wins: HashMap.put); per-field kinds are kept
// packed 4 bits each; a failed record's columns are overwritten with 0 at the end.
//
// Decimal to double: sign, up to 19 significant digits in a u64 `w`, the decimal exponent `q`
// and a "non-zero digits were dropped" flag are accumulated while lexing.  w <= 2^53 and
// |q| <= 22 is one IEEE multiply or divide by an exact power of ten (Clinger's fast path);
// anything else is the Eisel-Lemire construction (D. Lemire, "Number parsing at a gigabyte per
// second", 2021): w x 5^q from a table of 128-bit truncated powers of five, the binary exponent
// from clz, round half-even, with the subnormal and overflow branches.  Where the truncated
// product cannot decide the rounding, or w and w + 1 disagree when digits were dropped, the
// record gets CEP_JSON_PRECISION: never a wrong bit.
#pragma once
#include <stdint.h>
#include <string.h>

#include "json_parser.h"

namespace cep {

namespace jsong {

using namespace json;

constexpr int kMaxJsonFields = 32, kMaxJsonName = 64;
constexpr int kTypeInt = 1, kTypeLong = 2, kTypeDouble = 3;  // the IR's type codes (expr.py)
// field kinds beyond json::Kind (decoder limits, decided after the Java outcomes)
constexpr uint8_t K_NARROW = 8, K_PRECISION = 9;

// the field table: entries 0..n-1 are the columns, entry n (when n_all == n + 1) the span field
struct Table {
  uint32_t n, n_all;
  uint32_t hash[kMaxJsonFields + 1];
  uint8_t len[kMaxJsonFields + 1];
  uint8_t type[kMaxJsonFields + 1];
  void* col[kMaxJsonFields + 1];
  uint8_t name[kMaxJsonFields + 1][kMaxJsonName];
};
static_assert(sizeof(Table) % 8 == 0 && sizeof(Table) <= 3072, "passed by value in the kernel argument");

constexpr uint32_t kFnvBasis = 2166136261u, kFnvPrime = 16777619u;

// ---- powers of five: 128-bit truncated 5^q, q in [kPow5Min, kPow5Max], (hi, lo) pairs ----
constexpr int kPow5Min = -342, kPow5Max = 308, kPow5Count = kPow5Max - kPow5Min + 1;

// A fixed-width unsigned integer for building the table (host only): 64 x 32 bits hold
// 2^(2 * 795 + 128), the largest dividend (5^342 has 795 bits).
struct Big {
  static constexpr int kLimbs = 64;
  uint32_t v[kLimbs] = {};
  int bit(int i) const { return (v[i >> 5] >> (i & 31)) & 1; }
  void set(int i) { v[i >> 5] |= 1u << (i & 31); }
  int bits() const {
    for (int i = kLimbs * 32 - 1; i >= 0; i--)
      if (bit(i)) return i + 1;
    return 0;
  }
  void mul_small(uint32_t m) {
    uint64_t c = 0;
    for (int i = 0; i < kLimbs; i++) {
      c += (uint64_t)v[i] * m;
      v[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  void add_small(uint32_t a) {
    uint64_t c = a;
    for (int i = 0; i < kLimbs && c; i++) {
      c += v[i];
      v[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  void shl1(int in) {
    uint32_t c = (uint32_t)in;
    for (int i = 0; i < kLimbs; i++) {
      const uint32_t t = v[i] >> 31;
      v[i] = (v[i] << 1) | c;
      c = t;
    }
  }
  bool ge(const Big& o) const {
    for (int i = kLimbs - 1; i >= 0; i--)
      if (v[i] != o.v[i]) return v[i] > o.v[i];
    return true;
  }
  void sub(const Big& o) {
    int64_t b = 0;
    for (int i = 0; i < kLimbs; i++) {
      const int64_t d = (int64_t)v[i] - o.v[i] + b;
      v[i] = (uint32_t)d;
      b = d >> 32;
    }
  }
  // bits [top - 128, top) of the value, top = bits()
  void top128(uint64_t* hi, uint64_t* lo) const {
    const int top = bits();
    uint64_t w[2] = {0, 0};
    for (int k = 0; k < 128; k++) {
      const int i = top - 1 - k;
      if (i >= 0 && bit(i)) w[k >> 6] |= 1ull << (63 - (k & 63));
    }
    *hi = w[0];
    *lo = w[1];
  }
};

// out[2 * (q - kPow5Min)] = high, [.. + 1] = low 64 bits.  q >= 0: 5^q shifted to 128 bits,
// truncated.  q < 0: floor(2^b / 5^-q) + 1 cut to 128 bits, with b = z + 127 for q >= -27 and
// 2 z + 128 below, z the smallest power of two >= 5^-q (the construction of the paper's table).
inline void build_pow5_table(uint64_t* out) {
  Big p;  // 5^|q|
  p.v[0] = 1;
  for (int q = 0; q <= kPow5Max; q++) {
    p.top128(&out[2 * (q - kPow5Min)], &out[2 * (q - kPow5Min) + 1]);
    p.mul_small(5);
  }
  p = Big();
  p.v[0] = 1;
  for (int q = -1; q >= kPow5Min; q--) {
    p.mul_small(5);
    const int z = p.bits();  // 5^n is no power of two: 2^(z-1) < 5^n < 2^z
    const int b = q >= -27 ? z + 127 : 2 * z + 128;
    Big rem, quo;  // restoring division of 2^b by 5^n, a bit at a time
    for (int i = b; i >= 0; i--) {
      rem.shl1(i == b);
      if (rem.ge(p)) {
        rem.sub(p);
        quo.set(i);
      }
    }
    quo.add_small(1);
    quo.top128(&out[2 * (q - kPow5Min)], &out[2 * (q - kPow5Min) + 1]);
  }
}

// Fills the table from a field list; a message when the list breaks cep_decode_json's limits.
inline const char* fill_table(Table* T, const cep_json_field* fields, uint32_t n_fields, void* const* cols,
                              const char* span_field) {
  if (!fields || !cols) return "null argument";
  if (n_fields < 1 || n_fields > (uint32_t)kMaxJsonFields) return "1..32 fields";
  memset(T, 0, sizeof *T);
  T->n = n_fields;
  T->n_all = n_fields + (span_field ? 1 : 0);
  for (uint32_t f = 0; f < T->n_all; f++) {
    const char* nm = f < n_fields ? fields[f].name : span_field;
    if (!nm) return "null field name";
    const size_t len = strnlen(nm, kMaxJsonName + 1);
    if (len < 1 || len > (size_t)kMaxJsonName) return "a field name holds 1..64 bytes";
    uint32_t h = kFnvBasis;
    for (size_t i = 0; i < len; i++) {
      if ((uint8_t)nm[i] >= 0x80) return "a field name must be ASCII";
      h = (h ^ (uint8_t)nm[i]) * kFnvPrime;
    }
    for (uint32_t g = 0; g < f; g++)
      if (T->len[g] == len && !memcmp(T->name[g], nm, len)) return "duplicate field name";
    if (f < n_fields) {
      if (fields[f].type < kTypeInt || fields[f].type > kTypeDouble) return "field type must be 1 (int), 2 (long) or 3 (double)";
      if (!cols[f]) return "null column";
      T->type[f] = fields[f].type;
      T->col[f] = cols[f];
    }
    T->hash[f] = h;
    T->len[f] = (uint8_t)len;
    memcpy(T->name[f], nm, len);
  }
  return nullptr;
}

// ---- decimal to double ----

__device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIPCC__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

__device__ __forceinline__ double bits_double(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// w x 10^q (w != 0) as the bits of the nearest double, ties to even; false where the truncated
// 128-bit product cannot decide.  Eisel-Lemire; pow5 is build_pow5_table's output.
__device__ __forceinline__ bool eisel_lemire(uint64_t w, int32_t q, const uint64_t* pow5, uint64_t* out) {
  if (q < kPow5Min) { *out = 0; return true; }                       // below half the least subnormal
  if (q > kPow5Max) { *out = 0x7FF0000000000000ull; return true; }   // Infinity
  const int lz = __builtin_clzll(w);
  w <<= lz;
  const uint64_t th = pow5[2 * (q - kPow5Min)], tl = pow5[2 * (q - kPow5Min) + 1];
  uint64_t lo = w * th, hi = mulhi64(w, th);
  if ((hi & 0x1FF) == 0x1FF) {  // the 55 bits needed are not settled by the high word alone
    const uint64_t hi2 = mulhi64(w, tl);
    lo += hi2;
    if (hi2 > lo) hi++;
  }
  // the truncated table could still carry into the kept bits (never for q in [-27, 55], where
  // the product with the table entry is exact)
  if (lo == 0xFFFFFFFFFFFFFFFFull && (q < -27 || q > 55)) return false;
  const int upper = (int)(hi >> 63);
  const int shift = upper + 64 - 52 - 3;
  uint64_t m = hi >> shift;
  // floor(log2(10^q)) + 63 = ((152170 + 65536) q >> 16) + 63; biased by 1023
  int32_t e2 = (int32_t)(((152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023;
  if (e2 <= 0) {  // subnormal (or zero)
    if (-e2 + 1 >= 64) { *out = 0; return true; }
    m >>= -e2 + 1;
    m += m & 1;
    m >>= 1;
    *out = m;  // m == 2^52: the least normal, exponent field 1, the same bits
    return true;
  }
  // exactly half way (all lower bits zero): round to even
  if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
  m += m & 1;
  m >>= 1;
  if (m >= (2ull << 52)) {
    m = 1ull << 52;
    e2++;
  }
  m &= ~(1ull << 52);
  if (e2 >= 0x7FF) { *out = 0x7FF0000000000000ull; return true; }
  *out = m | ((uint64_t)e2 << 52);
  return true;
}

// magnitude bits of w x 10^q; false: undecided
__device__ __forceinline__ bool decimal_bits(uint64_t w, int64_t q, const uint64_t* pow5, uint64_t* out) {
  if (w == 0) { *out = 0; return true; }
  if (w <= (1ull << 53) && q >= -22 && q <= 22) {
    // 10^0..10^22 are exact doubles, as is w: one correctly rounded operation
    uint64_t p = 1;
    const int a = (int)(q < 0 ? -q : q);
    for (int i = 0; i < a && i < 19; i++) p *= 10;
    double pd = (double)p;  // exact: p <= 10^19 = 2^19 x 5^19, 5^19 < 2^53
    if (a > 19) pd *= a == 20 ? 1e1 : (a == 21 ? 1e2 : 1e3);  // exact: 5^22 < 2^53
    const double d = q < 0 ? (double)w / pd : (double)w * pd;
    memcpy(out, &d, 8);
    return true;
  }
  const int32_t qc = q < -1000 ? -1000 : (q > 1000 ? 1000 : (int32_t)q);
  return eisel_lemire(w, qc, pow5, out);
}

// ---- the state machine ----

template <typename Word>
struct Parser {
  Word word;      // the record's j-th aligned 32-bit word
  uint32_t lead;  // the record's first byte is byte `lead` of word(0)
  const Table* tab;
  const uint64_t* pow5;
  uint64_t rec;  // the record's row in the columns
  // outcome
  int32_t status = 0;
  bool done = false;
  // lexer
  uint8_t lex = L_WS;
  uint8_t lit = 0, lit_pos = 0, uhex = 0;
  uint32_t ucode = 0;
  // number being lexed
  bool neg = false, frac_seen = false, dropped = false, eneg = false;
  uint8_t nsig = 0;  // significant digits seen, 20 = more than 19
  uint64_t w = 0;
  int64_t q = 0, eacc = 0;
  // string being lexed
  uint32_t s_start = 0;
  bool s_esc = false, keying = false;
  uint32_t khash = 0, klen = 0;
  // parser
  uint8_t par = P_INIT;
  int depth = 0;
  uint64_t stack = 0;
  uint8_t top_kind = K_ABSENT, span_kind = K_ABSENT;
  int cur_key = -1;
  uint64_t kinds0 = 0, kinds1 = 0;  // 4 bits per field
  uint32_t span_off = 0, span_len = 0;

  __device__ __forceinline__ Parser(Word wd, uint32_t ld, const Table* t, const uint64_t* p5, uint64_t r)
      : word(wd), lead(ld), tab(t), pow5(p5), rec(r) {}

  __device__ __forceinline__ void fail(int32_t code) {
    status = code;
    done = true;
  }
  __device__ __forceinline__ uint32_t byte(uint32_t i) const {
    const uint32_t p = i + lead;
    return (word(p >> 2) >> (8 * (p & 3))) & 0xFF;
  }
  __device__ __forceinline__ uint8_t kind(uint32_t f) const {
    return (uint8_t)(((f < 16 ? kinds0 : kinds1) >> (4 * (f & 15))) & 15);
  }
  __device__ __forceinline__ void set_kind(uint32_t f, uint8_t k) {
    if (f == tab->n) { span_kind = k; return; }
    const uint64_t m = 15ull << (4 * (f & 15)), v = (uint64_t)k << (4 * (f & 15));
    if (f < 16) kinds0 = (kinds0 & ~m) | v;
    else kinds1 = (kinds1 & ~m) | v;
  }

  __device__ __forceinline__ void str_char(uint32_t ch) {
    if (!keying) return;
    khash = (khash ^ ch) * kFnvPrime;
    klen += ch < 0x80 ? 1 : 0x100;  // a non-ASCII key never matches: its length leaves 1..64
  }

  // the key string that just closed at raw offset `end`: its table entry or -1
  __device__ __forceinline__ int lookup(uint32_t end) const {
    for (uint32_t t = 0; t < tab->n_all; t++) {
      if (tab->hash[t] != khash || tab->len[t] != klen) continue;
      // verify: the unescaped text again, from the record (the escapes are known well formed)
      bool ok = true;
      uint32_t k = 0;
      for (uint32_t i = s_start; i < end && ok; k++) {
        uint32_t ch = byte(i++);
        if (ch == '\\') {
          const uint32_t e = byte(i++);
          switch (e) {
            case 'b': ch = '\b'; break;
            case 'f': ch = '\f'; break;
            case 'n': ch = '\n'; break;
            case 'r': ch = '\r'; break;
            case 't': ch = '\t'; break;
            case 'u':
              ch = 0;
              for (int j = 0; j < 4; j++) ch = ch * 16 + (uint32_t)hexval((uint8_t)byte(i++));
              break;
            default: ch = e;  // \" \\ \/
          }
        }
        ok = ch == tab->name[t][k];
      }
      if (ok) return (int)t;
    }
    return -1;
  }

  __device__ __forceinline__ void pop_container() {
    depth--;
    par = depth == 0 ? P_FIN : (((stack >> (depth - 1)) & 1) ? P_OBJ : P_ARR);
  }
  __device__ __forceinline__ void push_container(bool obj) {
    if (depth >= kMaxDepth) { fail(CEP_JSON_DEPTH); return; }
    if (obj) stack |= 1ull << depth;
    else stack &= ~(1ull << depth);
    depth++;
    par = obj ? P_OBJ : P_ARR;
  }

  // the value of the pending top-level key: its kind, and a number straight to its column
  __device__ __forceinline__ void assign(uint8_t vk) {
    const uint32_t f = (uint32_t)cur_key;
    if (f == tab->n) {
      if (vk == K_STRING) { span_off = s_start; span_len = klen; }
      span_kind = vk;
      return;
    }
    const uint8_t type = tab->type[f];
    void* col = tab->col[f];
    if (vk == K_INT) {
      const int64_t v = neg ? (int64_t)(0ull - w) : (int64_t)w;
      if (type == kTypeInt) {
        if (v < INT32_MIN || v > INT32_MAX) vk = K_NARROW;
        else ((int32_t*)col)[rec] = (int32_t)v;
      } else if (type == kTypeLong) {
        ((int64_t*)col)[rec] = v;
      } else {
        ((double*)col)[rec] = (double)v;  // Java's (double) of a long: nearest, ties to even
      }
    } else if (vk == K_DOUBLE && type == kTypeDouble) {
      const int64_t qq = q + (eneg ? -eacc : eacc);
      uint64_t b, b1;
      bool ok = decimal_bits(w, qq, pow5, &b);
      if (ok && dropped) ok = decimal_bits(w + 1, qq, pow5, &b1) && b1 == b;
      if (ok) ((uint64_t*)col)[rec] = b | (neg ? 0x8000000000000000ull : 0);
      else vk = K_PRECISION;
    }
    set_kind(f, vk);
  }

  // a value token (string, number, literal)
  __device__ __forceinline__ void value(uint8_t vk, int key) {
    switch (par) {
      case P_INIT: par = P_FIN; top_kind = vk; return;
      case P_OBJ:
        if (vk != K_STRING) { fail(CEP_JSON_PARSE); return; }
        cur_key = key;
        par = P_KEY;
        return;
      case P_KEY:
        if (cur_key >= 0) assign(vk);
        par = P_OBJ;
        return;
      case P_ARR: return;
      default: fail(CEP_JSON_PARSE);  // P_FIN
    }
  }

  // { } [ ] , :
  __device__ __forceinline__ void punct(uint8_t c) {
    const bool open = c == '{' || c == '[';
    switch (par) {
      case P_INIT:
        if (!open) { fail(CEP_JSON_PARSE); return; }
        top_kind = c == '{' ? K_OBJECT : K_ARRAY;
        push_container(c == '{');
        return;
      case P_OBJ:
        if (c == '}') pop_container();
        else if (c != ',') fail(CEP_JSON_PARSE);
        return;
      case P_KEY:
        if (c == ':') return;
        if (!open) { fail(CEP_JSON_PARSE); return; }
        if (cur_key >= 0) set_kind((uint32_t)cur_key, c == '{' ? K_OBJECT : K_ARRAY);
        push_container(c == '{');
        return;
      case P_ARR:
        if (c == ']') pop_container();
        else if (open) push_container(c == '{');
        else if (c != ',') fail(CEP_JSON_PARSE);
        return;
      default: fail(CEP_JSON_PARSE);  // P_FIN
    }
  }

  __device__ __forceinline__ void begin_number(bool negative) {
    neg = negative;
    frac_seen = dropped = eneg = false;
    nsig = 0;
    w = 0;
    q = eacc = 0;
  }
  __device__ __forceinline__ void int_digit(uint32_t d) {
    if (nsig == 0 && d == 0) return;  // leading zeros
    if (nsig < 19) { w = w * 10 + d; nsig++; }
    else { nsig = 20; q++; dropped |= d != 0; }
  }
  __device__ __forceinline__ void frac_digit(uint32_t d) {
    if (nsig == 0 && d == 0) { q--; return; }
    if (nsig < 19) { w = w * 10 + d; nsig++; q--; }
    else dropped |= d != 0;
  }
  __device__ __forceinline__ void exp_digit(uint32_t d) {
    if (eacc < (1ll << 40)) eacc = eacc * 10 + d;  // saturates far beyond any digit count
  }

  // a byte outside any token
  __device__ __forceinline__ void start(uint8_t c, uint32_t pos) {
    switch (c) {
      case ' ': case '\t': case '\n': case '\r': case '\f': return;
      case '{': case '}': case '[': case ']': case ',': case ':': punct(c); return;
      case '"':
        lex = L_STR; s_start = pos + 1; s_esc = false;
        keying = par == P_OBJ && depth == 1;
        khash = kFnvBasis; klen = 0;
        return;
      case 't': lex = L_LIT; lit = 0; lit_pos = 1; return;
      case 'f': lex = L_LIT; lit = 1; lit_pos = 1; return;
      case 'n': lex = L_LIT; lit = 2; lit_pos = 1; return;
      case '-': lex = L_NEG; begin_number(true); return;
      default:
        if (c >= '0' && c <= '9') { lex = L_INT; begin_number(false); int_digit(c - '0'); return; }
        fail(CEP_JSON_PARSE);
    }
  }

  // one byte; the end of input is fed as one more space (it ends a number or fails a cut-off
  // escape or literal exactly as json_parser.h's finish() does, and is nothing anywhere else)
  __device__ __forceinline__ void feed(uint8_t c, uint32_t pos) {
    const bool dig = c >= '0' && c <= '9';
    uint8_t vk = 0;        // a value token ended
    int key = -1;
    bool relex = false, bad = false;  // after a number: c lexed again / c is an unexpected char
    switch (lex) {
      case L_WS: relex = true; break;
      case L_STR:
        if (c == '"') {
          lex = L_WS;
          vk = K_STRING;
          if (keying) key = lookup(pos);
          else klen = (pos - s_start) | (s_esc ? 0x80000000u : 0u);  // a value: the span encoding
        } else if (c == '\\') {
          lex = L_ESC; s_esc = true;
        } else {
          str_char(c < 0x80 ? c : 0xFFFFu);
        }
        break;
      case L_ESC: {
        uint32_t ch = c;
        switch (c) {
          case '"': case '\\': case '/': break;
          case 'b': ch = '\b'; break;
          case 'f': ch = '\f'; break;
          case 'n': ch = '\n'; break;
          case 'r': ch = '\r'; break;
          case 't': ch = '\t'; break;
          case 'u': lex = L_UHEX; uhex = 0; ucode = 0; return;
          default: fail(CEP_JSON_LEX); return;
        }
        str_char(ch);
        lex = L_STR;
        break;
      }
      case L_UHEX: {
        const int h = hexval(c);
        if (h < 0) { fail(CEP_JSON_LEX); return; }
        ucode = ucode * 16 + (uint32_t)h;
        if (++uhex == 4) { str_char(ucode); lex = L_STR; }
        break;
      }
      case L_LIT: {
        const uint64_t s = lit == 0 ? 0x65757274ull : (lit == 1 ? 0x65736C6166ull : 0x6C6C756Eull);  // true false null
        if (((s >> (8 * lit_pos)) & 0xFF) != c) { fail(CEP_JSON_PARSE); return; }
        lit_pos++;
        if (((s >> (8 * lit_pos)) & 0xFF) == 0) { lex = L_WS; vk = lit == 2 ? K_NULL : K_BOOL; }
        break;
      }
      case L_NEG:
        if (!dig) { fail(CEP_JSON_PARSE); return; }  // a lone '-'
        lex = L_INT; int_digit(c - '0');
        break;
      case L_INT:
        if (dig) int_digit(c - '0');
        else if (c == '.') lex = L_DOT;
        else if (c == 'e' || c == 'E') lex = L_E;
        else { vk = K_INT; relex = true; }
        break;
      case L_DOT:  // "1." + non-digit: INT, then '.' is an unexpected char
        if (dig) { lex = L_FRAC; frac_seen = true; frac_digit(c - '0'); }
        else { vk = K_INT; bad = true; }
        break;
      case L_FRAC:
        if (dig) frac_digit(c - '0');
        else if (c == 'e' || c == 'E') lex = L_E;
        else { vk = K_DOUBLE; relex = true; }
        break;
      case L_E: case L_ESIGN:  // a cut-off exponent: the number before it, then 'e' is unexpected
        if (dig) { lex = L_EXP; exp_digit(c - '0'); }
        else if (lex == L_E && (c == '+' || c == '-')) { lex = L_ESIGN; eneg = c == '-'; }
        else { vk = frac_seen ? K_DOUBLE : K_INT; bad = true; eacc = 0; }
        break;
      case L_EXP:
        if (dig) exp_digit(c - '0');
        else { vk = K_DOUBLE; relex = true; }
        break;
    }
    if (vk) {
      if (vk == K_INT || vk == K_DOUBLE) lex = L_WS;
      // Long.valueOf: NumberFormatException outside long
      if (vk == K_INT && (nsig > 19 || w > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull))) {
        fail(CEP_JSON_NUMBER);
        return;
      }
      value(vk, key);
      if (done) return;
      if (bad) { fail(CEP_JSON_PARSE); return; }
    }
    if (relex) start(c, pos);
  }

  // end of the record: the typed getters.  Java outcomes first (top value, span field, fields in
  // table order), then this decoder's own limits (NARROW, PRECISION) as cep_decode_stock_json
  // orders them; a failed record's columns are zeroed.
  __device__ __forceinline__ void finish(uint32_t* span) {
    if (!status && par != P_FIN) status = CEP_JSON_PARSE;  // end of input inside a value
    if (!status) {
      if (top_kind == K_NULL) status = CEP_JSON_NULL;
      else if (top_kind != K_OBJECT) status = CEP_JSON_CLASS_CAST;
      else if (span_kind != K_ABSENT && span_kind != K_NULL && span_kind != K_STRING) status = CEP_JSON_CLASS_CAST;
    }
    int32_t limit = 0;
    for (uint32_t f = 0; f < tab->n && !status; f++) {
      const uint8_t k = kind(f);
      const bool dbl = tab->type[f] == kTypeDouble;
      if (k == K_ABSENT || k == K_NULL) status = CEP_JSON_NULL;
      else if (k == K_NARROW || k == K_PRECISION) { if (!limit) limit = k == K_NARROW ? CEP_JSON_NARROW : CEP_JSON_PRECISION; }
      else if (k != K_INT && !(dbl && k == K_DOUBLE)) status = CEP_JSON_CLASS_CAST;
    }
    if (!status) status = limit;
    if (status)
      for (uint32_t f = 0; f < tab->n; f++) {
        if (tab->type[f] == kTypeInt) ((int32_t*)tab->col[f])[rec] = 0;
        else ((uint64_t*)tab->col[f])[rec] = 0;
      }
    if (span) {
      const bool has = status == 0 && span_kind == K_STRING;
      span[2 * rec] = has ? span_off : 0;
      span[2 * rec + 1] = has ? span_len : 0xFFFFFFFFu;
    }
  }

  // the whole record: one pass, no fixed-layout fast path
  __device__ __forceinline__ int32_t run(uint32_t len, uint32_t* span) {
    uint32_t wd = 0;
    for (uint32_t i = 0; i <= len && !done; i++) {
      uint32_t c = ' ';
      if (i < len) {
        const uint32_t p = i + lead;
        if (i == 0 || (p & 3) == 0) wd = word(p >> 2);
        c = (wd >> (8 * (p & 3))) & 0xFF;
      } else if (lex == L_WS || lex == L_STR) {  // (a string cut off by the end is end of input)
        break;
      }
      feed((uint8_t)c, i);
    }
    finish(span);
    return status;
  }
};

// the record at `base` in flat memory
__device__ __forceinline__ int32_t decode_record(const uint8_t* base, uint32_t len, const Table* tab,
                                                 const uint64_t* pow5, uint64_t rec, uint32_t* span) {
  const uint32_t* words = (const uint32_t*)((uintptr_t)base & ~(uintptr_t)3);
  auto wd = [words](uint32_t j) { return words[j]; };
  Parser<decltype(wd)> P(wd, (uint32_t)((uintptr_t)base & 3), tab, pow5, rec);
  return P.run(len, span);
}

}  // namespace jsong

}  // namespace cep
