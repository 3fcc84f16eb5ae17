// stencil_args.h — kernel arguments of the strict-contiguity stencil (stencil.hip).  Kept out
// of kernel_args.h, which is embedded into every JIT compile (and its cache key).
#pragma once
#include "kernel_args.h"

namespace cep {

// conjunction of lo <= col_c <= hi for c in {0, 1}, as int64 in the column's order: an int or a
// long as itself, a double as its order key okey(bits) = bits ^ ((bits >> 63) & INT64_MAX)
// (signed compare of keys = IEEE compare of the doubles, -0.0 and +0.0 adjacent keys -1 and 0,
// NaNs beyond okey(-inf) and okey(+inf)).  That is the unsigned key `bits ^ ((bits >> 63) |
// 2^63)` less 2^63: the kernel tests (uint64)(key - lo) <= (uint64)(hi - lo), where the 2^63
// cancels.  A constrained double side is clamped to the infinities' keys by compile.cpp (a NaN
// fails); INT64_MIN .. INT64_MAX accepts every value, NaN included.
struct RangeStage {
  int64_t lo[2], hi[2];
};

struct StencilArgs {
  uint64_t n_keys, n_events;
  const uint64_t* key_off;
  const uint32_t* wave_key;  // key holding the first event of each wave's span (kStWave events)
  const void* col[2];        // range fast path: up to two columns, of
  uint8_t col_w[2];          // 4 (int) or 8 bytes (long, double) an event; a mixed pair is (4, 8)
  bool col_dbl[2];           // a double column: its values compare by their order key
  RangeStage rs[8];
  // generic path (interpreted predicates)
  const DevQuery* q;
  const uint32_t* code;
  Cols cols;
  const int64_t* ts;
  uint16_t prog[kMaxStencil];
  uint16_t stage_name[kMaxStencil];    // walk order: stage name of pair t (t = 0 is the final event)
  bool aligned;              // col[] 16-B aligned: vector loads
  uint64_t n_chunk;          // stencil_mask: kStWave-event chunks (one a wave)
  // pass 1 -> pass 3
  // per 64-event word w (pass 1): {match bits lo, hi (bit i: a match ends at event 64 w + i), the
  // key holding event 64 w (bit 31: a key starts inside the word after its first event), event
  // 64 w's sequence number within that key}
  uint4* words;
  uint32_t* group_cnt;       // matches per stencil_emit block's span (pass 1, atomics; zeroed per batch)
  // streaming sessions (null otherwise): a word per key, count << 32 | live (stencil.hip
  // stencil_edge).  A batch reads carry_prev and writes carry_next; the session swaps them
  const uint64_t* carry_prev;
  uint64_t* carry_next;
  // semantic WITHIN (stencil.hip stencil_within; win_mask 0: the pass does not run).  A match of
  // m events whose start is event s survives iff ts[s + p] - ts[s + 1] <= win[p] for every
  // position p of win_mask (2 <= p < m; win[p]: the window of stage p - 1)
  int64_t win[kMaxStencil];
  uint32_t win_mask;
  // streaming sessions: the last m - 2 event times of every key's stream, oldest first
  // (tsc[k * (m - 2) + x]); read and written as the carry words are
  const int64_t* tsc_prev;
  int64_t* tsc_next;
  // output
  uint32_t* m_key;
  uint32_t* p_seq;           // [n_matches * m]
  uint64_t* total;           // number of matches (written by the last tile of stencil_emit)
  uint64_t* total_host;      // the same, into the session's pinned host copy (no D2H copy per batch)
  uint64_t out_cap;          // matches that fit the output arrays
  uint32_t* overflow;
  // lagged strict chains (stencil_lag.hip; compile.cpp): stage s reads fold state X as the fold
  // program lag_prog[s][X] evaluated lag_of[s][X] events back (0: the stage does not read X)
  uint16_t lag_prog[kMaxStencil][kMaxStates];
  uint8_t lag_of[kMaxStencil][kMaxStates];
  // the lag fast route: stage s holds rs[s] on col[0] and col[0][i] OP col[0][i - lag_d[s]]
  // (lag_d 0: no such conjunct; lag_op: 0 lt, 1 le, 2 gt, 3 ge, 4 eq, compared as values)
  uint8_t lag_d[kMaxStencil], lag_op[kMaxStencil];
};

}  // namespace cep
