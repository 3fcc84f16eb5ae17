// stencil.hip — CEP_KIND_STENCIL: SEQ(p_0, ..., p_{m-1}) with every stage ONE + strict
// contiguity and total, state-free predicates and folds.
//
// For such queries the reference NFA (nfa/NFA.java) never branches, each run lives at most
// m events, and every run's buffer nodes are private; so the matches of a key's stream
// x_0..x_{n-1} are exactly the windows (i-m+1 .. i) with p_t(x_{i-m+1+t}) for all t,
// emitted in increasing i, each the walk (stage m-1, x_i), ..., (stage 0, x_{i-m+1})
// (proof: SURVEY Appendix A.5).  That is a 1-D stencil over the column:
// HBM-bound, one pass.
//
// Layout.  A tile is 4 waves x 4096 consecutive events.  A wave streams its events with 16-B
// loads (lane l holds events 4l..4l+3 of a 256-event step), evaluates the m stage predicates
// straight into scalar ballot words and ANDs them shifted (match bit i = Π_x P_{m-1-x}(i-x));
// the windows reaching back before the wave and those crossing a key start are settled after
// the loop on natural 64-event words (key starts from key_off around the wave's first key,
// wave_keys), and a match's key is its word's first key advanced over the key starts.
//
// Passes.  (1) stencil_mask streams the column once and writes one 64-bit match word per 64
// events (1 bit/event), the word's key and sequence number, and adds each wave's match count to
// its stencil_emit block's counter; (2) stencil_emit sums the counters of the blocks before its
// own, reads the words back (1/32 of the column's bytes) and writes the matches in order.  No
// tile waits on another.  (A single pass
// with a decoupled look-back over the tile counts was measured slower: 126.7 us against 112.6
// for the two passes at round 5's start, profiles/r05/ - a tile waits for every tile before
// it, ~24 look-back round trips deep within one round of co-resident tiles.)
// In a streaming session stencil_edge runs between the two passes: a carry word per key settles
// the windows that begin in an earlier batch (below, "streaming sessions").  A query with
// semantic windows runs stencil_within before stencil_emit: it clears the match bits whose
// event times break a window (below, "semantic WITHIN").
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cep_layout.h"
#include "dewey.h"
#include "interp.h"
#include "java.h"
#include "stencil_args.h"
#include "stencil_mask.h"

namespace cep {

// ---------------------------------------------------------------- per-batch key index
constexpr int kWkInline = 16;  // wave starts a thread writes itself; longer keys: the block

// wave_key[w] = the key holding event w * kStWave (wave starts inside key k: ceil(s/W) ..
// ceil(e/W) - 1; empty keys hold none).  A thread per key; a key spanning more than kWkInline
// wave starts is written by its whole block (a single key of the whole stream stays parallel).
// (It also zeroes the batch's counters, `zero[0..n_zero)`, which the mask pass accumulates
// into after it: one launch fewer per batch than a separate memset.)
__global__ void __launch_bounds__(256) wave_keys(const uint64_t* key_off, uint64_t n_keys, uint64_t n_waves,
                                                 uint32_t* wave_key, uint32_t* zero, uint32_t n_zero) {
  __shared__ uint32_t s_big[256];
  __shared__ uint32_t s_nbig;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_zero; i += (uint64_t)gridDim.x * 256) zero[i] = 0;
  if (threadIdx.x == 0) s_nbig = 0;
  __syncthreads();
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n_keys) {
    const uint64_t s = key_off[k], e = key_off[k + 1];
    const uint64_t w0 = (s + kStWave - 1) / kStWave;
    uint64_t w1 = (e + kStWave - 1) / kStWave;
    w1 = w1 < n_waves ? w1 : n_waves;
    if (w1 > w0 + kWkInline) {
      s_big[atomicAdd(&s_nbig, 1u)] = (uint32_t)k;
    } else {
      for (uint64_t w = w0; w < w1; w++) wave_key[w] = (uint32_t)k;
    }
  }
  __syncthreads();
  const uint32_t nbig = s_nbig;
  for (uint32_t i = 0; i < nbig; i++) {
    const uint32_t kk = s_big[i];
    const uint64_t w0 = (key_off[kk] + kStWave - 1) / kStWave;
    uint64_t w1 = (key_off[kk + 1] + kStWave - 1) / kStWave;
    w1 = w1 < n_waves ? w1 : n_waves;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += 256) wave_key[w] = kk;
  }
}

// ---------------------------------------------------------------- the stencil
__device__ __forceinline__ uint64_t mix64s(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ bool in_range(int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi; }

// An evaluator (StEval: int columns and interpreted predicates; StEvalT: columns that are not
// all int) gives wave_mask the column-typed parts of the mask phase: Ld, a lane's 4 events of a
// step as loaded; Cur, the wave's load cursor; keys(), what the stages compare; ballot4(); and
// for the slow routes Sd, one event's values (load1), range() and slow4().
template <int M, bool RANGE_, int NCOL>
struct StEval {
  static constexpr int STAGES = M;
  static constexpr bool RANGE = RANGE_;
  struct Ld {
    v4i x, y;
  };
  struct Sd {
    int32_t x0, x1;
  };
  struct Cur {
    const v4i *c0, *c1;
    __device__ __forceinline__ Cur(const StencilArgs& A, uint64_t wbase, int lane)
        : c0(reinterpret_cast<const v4i*>(static_cast<const int32_t*>(A.col[0]) + wbase) + lane),
          c1(reinterpret_cast<const v4i*>(static_cast<const int32_t*>(A.col[NCOL - 1]) + wbase) + lane) {}
    __device__ __forceinline__ Ld load(int q) const {
      Ld d;
      d.x = __builtin_nontemporal_load(c0 + q * 64);
      d.y = NCOL > 1 ? __builtin_nontemporal_load(c1 + q * 64) : d.x;
      return d;
    }
  };
  int32_t lo[M][2], hi[M][2];
  uint32_t span[M][2];
  bool never = false;  // an empty range: no stage-s event, no match (the slow path handles it)
  __device__ __forceinline__ explicit StEval(const StencilArgs& A) {
    if (RANGE) {
      // int32 bounds (a range outside int32 is clamped: empty stays empty)
#pragma unroll
      for (int s = 0; s < M; s++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
          const int64_t l = A.rs[s].lo[c], h = A.rs[s].hi[c];
          lo[s][c] = l < INT32_MIN ? INT32_MIN : (l > INT32_MAX ? INT32_MAX : (int32_t)l);
          hi[s][c] = h > INT32_MAX ? INT32_MAX : (h < INT32_MIN ? INT32_MIN : (int32_t)h);
          if (l > INT32_MAX || h < INT32_MIN || l > h) {
            lo[s][c] = 1;
            hi[s][c] = 0;
          }
          // lo <= x <= hi  <=>  (uint)(x - lo) <= (uint)(hi - lo): one subtract and one
          // compare, both vector ops (no scalar AND of two compare masks)
          span[s][c] = (uint32_t)hi[s][c] - (uint32_t)lo[s][c];
          if (c < NCOL && lo[s][c] > hi[s][c]) never = true;
        }
    }
  }
  // stage bits of one event into bit `bit` of P[s]
  __device__ __forceinline__ void range(int32_t x0, int32_t x1, uint32_t* P, int bit) const {
#pragma unroll
    for (int s = 0; s < M; s++) {
      bool ok = x0 >= lo[s][0] && x0 <= hi[s][0];
      if (NCOL > 1) ok = ok && x1 >= lo[s][1] && x1 <= hi[s][1];
      P[s] |= (ok ? 1u : 0u) << bit;
    }
  }
  // stage s over the 4 events of a step: W[k] = ballot word of event 4 l + k.  Every
  // operation is a vector op whose result lands in scalar registers (the compare mask)
  __device__ __forceinline__ bool in1(int s, int c, int32_t v) const {
    return (uint32_t)v - (uint32_t)lo[s][c] <= span[s][c];
  }
  __device__ __forceinline__ void ballot4(int s, const v4i x, const v4i y, uint64_t* W) const {
    if (NCOL == 1) {
      W[0] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.x));
      W[1] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.y));
      W[2] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.z));
      W[3] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.w));
    } else {
      W[0] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.x)) & __builtin_amdgcn_ballot_w64(in1(s, 1, y.x));
      W[1] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.y)) & __builtin_amdgcn_ballot_w64(in1(s, 1, y.y));
      W[2] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.z)) & __builtin_amdgcn_ballot_w64(in1(s, 1, y.z));
      W[3] = __builtin_amdgcn_ballot_w64(in1(s, 0, x.w)) & __builtin_amdgcn_ballot_w64(in1(s, 1, y.w));
    }
  }
  __device__ __forceinline__ const Ld& keys(const Ld& d) const { return d; }
  __device__ __forceinline__ void ballot4(int s, const Ld& d, uint64_t* W) const { ballot4(s, d.x, d.y, W); }
  __device__ __forceinline__ Sd load1(const StencilArgs& A, uint64_t p) const {
    return Sd{static_cast<const int32_t*>(A.col[0])[p], static_cast<const int32_t*>(A.col[NCOL - 1])[p]};
  }
  __device__ __forceinline__ void range(const Sd& v, uint32_t* P, int bit) const { range(v.x0, v.x1, P, bit); }
  // the 4 events from e0 of a step off the fast path into bits 0..3 of P[s]
  __device__ __forceinline__ void slow4(const StencilArgs& A, uint64_t e0, uint32_t* P) const {
    if (RANGE && A.aligned && e0 + 4 <= A.n_events) {
      const v4i xs = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(static_cast<const int32_t*>(A.col[0]) + e0));
      v4i ys = xs;
      if (NCOL > 1)
        ys = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(static_cast<const int32_t*>(A.col[1]) + e0));
      range(xs.x, ys.x, P, 0);
      range(xs.y, ys.y, P, 1);
      range(xs.z, ys.z, P, 2);
      range(xs.w, ys.w, P, 3);
    } else if (e0 < A.n_events) {  // events past the end stay 0: no window can end there
#pragma unroll
      for (int i = 0; i < 4; i++) one(A, e0 + i, P, i);
    }
  }
  // stencil_edge's dense route: the same (one 16-B load per column where aligned)
  __device__ __forceinline__ void bits4(const StencilArgs& A, uint64_t e0, uint32_t* P) const { slow4(A, e0, P); }
  __device__ __forceinline__ void one(const StencilArgs& A, uint64_t p, uint32_t* P, int bit) const {
    if (p >= A.n_events) return;
    if (RANGE) {
      range(load1(A, p), P, bit);
    } else {
      EvalIn in{&A.cols, A.q->field_type, A.ts, p, nullptr, 0, 0, true};
      for (int s = 0; s < M; s++) {
        bool rn;
        int ee = 0;
        if (interp(A.code, A.prog[s], in, &rn, &ee) != 0) P[s] |= 1u << bit;  // total: never throws
      }
    }
  }
};

// The typed range evaluator: one or two columns of W0 and W1 bytes an event (W1 = 0: one
// column), {8}, {4, 8} or {8, 8} - a long or a double column each 8, told apart by the
// wave-uniform A.col_dbl alone.  A lane keeps the int path's events 4l..4l+3 of a step, so an
// 8-byte column is two 16-B loads per lane (32 contiguous bytes: each instruction covers every
// other 16 B of the step's 2 KiB, the pair all of it), a mixed pair shares one ballot layout,
// and everything after the ballots is wave_mask's own.  An 8-byte value becomes its order key
// on load (stencil_args.h RangeStage; a long is its own key) and a stage is, as for ints, one
// subtract and one unsigned compare: (uint64)(key - lo) <= (uint64)(hi - lo).
template <int W>
struct ColLd {};  // a lane's 4 events of one column, as loaded
template <>
struct ColLd<4> {
  v4i a;
};
template <>
struct ColLd<8> {
  v4i a, b;  // events 4l, 4l+1 | 4l+2, 4l+3 (low word first)
};
template <int W>
struct ColKey {};  // the same as the stages compare them
template <>
struct ColKey<4> {
  v4i v;
};
template <>
struct ColKey<8> {
  uint64_t k[4];
};

template <int M, int W0, int W1>
struct StEvalT {
  static_assert(W1 == 0 || W1 == 8, "a mixed pair is (4, 8)");
  static_assert((W0 == 4 && W1 == 8) || W0 == 8, "two int columns: StEval");
  static constexpr int STAGES = M;
  static constexpr bool RANGE = true;
  static constexpr int NCOL = W1 ? 2 : 1;
  struct Ld {
    ColLd<W0> x;
    ColLd<W1> y;
  };
  struct Key {
    ColKey<W0> x;
    ColKey<W1> y;
  };
  struct Sd {
    uint64_t v[2];  // raw bits (a 4-byte value: the low word)
  };
  template <int W>
  static __device__ __forceinline__ const v4i* cursor(const void* col, uint64_t wbase, int lane) {
    if constexpr (W == 4) return reinterpret_cast<const v4i*>(static_cast<const int32_t*>(col) + wbase) + lane;
    else return reinterpret_cast<const v4i*>(static_cast<const uint64_t*>(col) + wbase) + 2 * lane;
  }
  template <int W>
  static __device__ __forceinline__ void load_col(const v4i* c, int q, ColLd<W>& d) {
    if constexpr (W == 4) {
      d.a = __builtin_nontemporal_load(c + q * 64);
    } else if constexpr (W == 8) {
      d.a = __builtin_nontemporal_load(c + q * 128);
      d.b = __builtin_nontemporal_load(c + q * 128 + 1);
    }
  }
  struct Cur {
    const v4i *c0, *c1;
    __device__ __forceinline__ Cur(const StencilArgs& A, uint64_t wbase, int lane)
        : c0(cursor<W0>(A.col[0], wbase, lane)), c1(cursor<8>(A.col[NCOL - 1], wbase, lane)) {}
    __device__ __forceinline__ Ld load(int q) const {
      Ld d;
      load_col<W0>(c0, q, d.x);
      load_col<W1>(c1, q, d.y);
      return d;
    }
  };
  int32_t lo4[M];  // the 4-byte column (slot 0): int32 bounds, clamped as StEval's
  uint32_t span4[M];
  uint64_t lo8[M][2], span8[M][2];
  uint64_t dmask[2];  // INT64_MAX: a double column (okey flips a negative value's magnitude bits)
  bool never = false;  // an empty range: no match (range() says so; the spans of one wrap)
  __device__ __forceinline__ explicit StEvalT(const StencilArgs& A) {
#pragma unroll
    for (int c = 0; c < 2; c++) dmask[c] = A.col_dbl[c] ? (uint64_t)INT64_MAX : 0ull;
#pragma unroll
    for (int s = 0; s < M; s++)
#pragma unroll
      for (int c = 0; c < NCOL; c++) {
        const int64_t l = A.rs[s].lo[c], h = A.rs[s].hi[c];
        if (l > h) never = true;
        if (c == 0 && W0 == 4) {
          const int32_t l4 = l < INT32_MIN ? INT32_MIN : (l > INT32_MAX ? INT32_MAX : (int32_t)l);
          const int32_t h4 = h > INT32_MAX ? INT32_MAX : (h < INT32_MIN ? INT32_MIN : (int32_t)h);
          if (l > INT32_MAX || h < INT32_MIN) never = true;
          lo4[s] = l4;
          span4[s] = (uint32_t)h4 - (uint32_t)l4;
        } else {
          lo8[s][c] = (uint64_t)l;
          span8[s][c] = (uint64_t)h - (uint64_t)l;
        }
      }
  }
  __device__ __forceinline__ uint64_t key(int c, uint64_t bits) const {
    return bits ^ ((uint64_t)((int64_t)bits >> 63) & dmask[c]);
  }
  __device__ __forceinline__ uint64_t key(int c, int lo, int hi) const {
    return key(c, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  }
  __device__ __forceinline__ void keys_col(int, const ColLd<0>&, ColKey<0>&) const {}
  __device__ __forceinline__ void keys_col(int, const ColLd<4>& d, ColKey<4>& k) const { k.v = d.a; }
  __device__ __forceinline__ void keys_col(int c, const ColLd<8>& d, ColKey<8>& k) const {
    k.k[0] = key(c, d.a.x, d.a.y);
    k.k[1] = key(c, d.a.z, d.a.w);
    k.k[2] = key(c, d.b.x, d.b.y);
    k.k[3] = key(c, d.b.z, d.b.w);
  }
  // once per step, not per stage
  __device__ __forceinline__ Key keys(const Ld& d) const {
    Key k;
    keys_col(0, d.x, k.x);
    keys_col(1, d.y, k.y);
    return k;
  }
  __device__ __forceinline__ bool in4(int s, uint32_t v) const { return v - (uint32_t)lo4[s] <= span4[s]; }
  __device__ __forceinline__ bool in8(int s, int c, uint64_t k) const { return k - lo8[s][c] <= span8[s][c]; }
  __device__ __forceinline__ bool in(int s, int, const ColKey<4>& k, int e) const { return in4(s, (uint32_t)k.v[e]); }
  __device__ __forceinline__ bool in(int s, int c, const ColKey<8>& k, int e) const { return in8(s, c, k.k[e]); }
  __device__ __forceinline__ void ballot4(int s, const Key& k, uint64_t* W) const {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      W[e] = __builtin_amdgcn_ballot_w64(in(s, 0, k.x, e));
      if constexpr (NCOL > 1) W[e] &= __builtin_amdgcn_ballot_w64(in(s, 1, k.y, e));
    }
  }
  // The slow routes (the tail chunk, unaligned columns, an empty stage, the seed events):
  // one event at a time, the same compares
  __device__ __forceinline__ Sd load1(const StencilArgs& A, uint64_t p) const {
    Sd v;
    v.v[0] = W0 == 4 ? static_cast<const uint32_t*>(A.col[0])[p] : static_cast<const uint64_t*>(A.col[0])[p];
    v.v[1] = NCOL > 1 ? static_cast<const uint64_t*>(A.col[1])[p] : 0;
    return v;
  }
  __device__ __forceinline__ void range(const Sd& v, uint32_t* P, int bit) const {
#pragma unroll
    for (int s = 0; s < M; s++) {
      bool ok = !never && (W0 == 4 ? in4(s, (uint32_t)v.v[0]) : in8(s, 0, key(0, v.v[0])));
      if (NCOL > 1) ok = ok && in8(s, 1, key(1, v.v[1]));
      P[s] |= (ok ? 1u : 0u) << bit;
    }
  }
  __device__ __forceinline__ void slow4(const StencilArgs& A, uint64_t e0, uint32_t* P) const {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (e0 + i < A.n_events) range(load1(A, e0 + i), P, i);
  }
  // stencil_edge's dense route: 4 whole events from e0 (a multiple of 4) with the fast path's
  // 16-B loads and compares, the rest as slow4
  __device__ __forceinline__ void bits4(const StencilArgs& A, uint64_t e0, uint32_t* P) const {
    if (!A.aligned || e0 + 4 > A.n_events || never) return slow4(A, e0, P);
    Ld d;
    load_col<W0>(cursor<W0>(A.col[0], e0, 0), 0, d.x);
    load_col<W1>(cursor<8>(A.col[NCOL - 1], e0, 0), 0, d.y);
    const Key k = keys(d);
#pragma unroll
    for (int s = 0; s < M; s++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        bool ok = in(s, 0, k.x, e);
        if constexpr (NCOL > 1) ok = ok && in(s, 1, k.y, e);
        P[s] |= (ok ? 1u : 0u) << e;
      }
  }
};

template <int M, bool RANGE, int NCOL>
__global__ void __launch_bounds__(kStThreads) stencil_mask(StencilArgs A) {
  mask_chunk<StEval<M, RANGE, NCOL>>(A);
}

// The typed variant: columns of W0 (and W1) bytes an event, not all int (StEvalT)
template <int M, int W0, int W1>
__global__ void __launch_bounds__(kStThreads) stencil_mask_typed(StencilArgs A) {
  mask_chunk<StEvalT<M, W0, W1>>(A);
}

// Pass 2: a thread per kEmW consecutive 64-event words (a block: kEmW mask tiles), the block's
// offset from the group and tile counts, a block scan for the threads' offsets.  A match's key
// is its word's first key advanced over the key offsets it passes.  (One word per
// thread ran 6104 blocks for 1e8 events, three rounds of resident blocks each paying a load
// and a store round trip: ~18 us; kEmW words per thread issue their loads together and the
// grid fits the chip in one round.)
constexpr uint32_t kEmStage = 3072;  // matches staged in LDS (24 KB: 6 blocks per CU)

//
// STREAM (streaming sessions): the words hold in-batch sequence numbers; a match's is that plus
// the events its key had before the batch (carry_prev's count).
template <int M, bool STREAM>
__global__ void __launch_bounds__(kStThreads) stencil_emit(StencilArgs A) {
  __shared__ uint32_t s_wsum[kStThreads / 64];
  __shared__ uint64_t s_toff[kStThreads / 64];
  __shared__ uint2 s_stage[kEmStage];  // (key, sequence number of the final event)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t t0 = (uint64_t)blockIdx.x * kEmW;  // the block's first mask tile
  const uint64_t n_words = (A.n_events + 63) / 64;
  const uint64_t w0 = t0 * (kStTile / 64) + (uint64_t)tid * kEmW;  // this thread's first word
  // Every independent load is issued before the first use: the thread's words (a 16-B record
  // each: match bits, first key, sequence number) and the counts of the blocks before this one.
  uint64_t wm[kEmW];
  uint32_t wk[kEmW], ws[kEmW];
#pragma unroll
  for (int i = 0; i < kEmW; i++) {
    const uint4 x = w0 + i < n_words ? A.words[w0 + i] : uint4{0, 0, 0, 0};
    wm[i] = ((uint64_t)x.y << 32) | x.x;
    wk[i] = x.z;
    ws[i] = x.w;
  }
  uint64_t part = 0;  // the matches of the blocks before this one: their group counts
  // (the first 8 per thread issued together: a late block of 1e8 events has ~1500 before it)
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint32_t i = (uint32_t)tid + (uint32_t)r * kStThreads;
    part += i < blockIdx.x ? A.group_cnt[i] : 0u;
  }
  for (uint64_t i = (uint64_t)tid + 8 * kStThreads; i < blockIdx.x; i += kStThreads) part += A.group_cnt[i];
  uint32_t cnt = 0;
#pragma unroll
  for (int i = 0; i < kEmW; i++) cnt += (uint32_t)__popcll(wm[i]);
  // block exclusive scan of the threads' match counts
  uint32_t incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if (lane == 63) s_wsum[wv] = incl;
  if (lane == 0) s_toff[wv] = part;
  __syncthreads();
  uint32_t woff = 0;
#pragma unroll
  for (int w = 0; w < kStThreads / 64; w++)
    if (w < wv) woff += s_wsum[w];
  const uint32_t excl = woff + incl - cnt;
  const uint64_t toff = s_toff[0] + s_toff[1] + s_toff[2] + s_toff[3];
  if (blockIdx.x + 1 == gridDim.x && tid == kStThreads - 1) {  // all matches
    *A.total = toff + woff + incl;
    if (A.total_host) *A.total_host = toff + woff + incl;  // pinned host memory, read after the batch's event
  }
  const uint32_t block_total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
  const bool staged = block_total <= kEmStage;  // block-uniform
  uint64_t o = toff + excl;
  uint32_t so = excl;  // slot within the block
#pragma unroll
  for (int i = 0; i < kEmW; i++) {
    uint64_t match = wm[i];
    if (!match) continue;
    const uint64_t p0 = (w0 + i) * 64;
    uint32_t key = wk[i] & 0x7FFFFFFFu;
    const bool cross = (wk[i] >> 31) != 0;  // a key starts inside this word
    uint64_t kstart = 0, knext = 0;
    if (cross) {
      kstart = A.key_off[key];
      knext = A.key_off[key + 1];
    }
    uint32_t base = 0;  // the key's events before this batch
    if (STREAM) base = (uint32_t)(A.carry_prev[key] >> 32);
    while (match) {
      const int b = __builtin_ctzll(match);
      match &= match - 1;
      const uint64_t p = p0 + b;
      uint32_t seq = ws[i] + (uint32_t)b;
      if (cross) {
        bool moved = false;
        while (p >= knext) {  // the next key (empty keys share their offset: skipped too)
          key++;
          kstart = knext;
          knext = A.key_off[key + 1];
          moved = true;
        }
        if (STREAM && moved) base = (uint32_t)(A.carry_prev[key] >> 32);
        seq = (uint32_t)(p - kstart);
      }
      if (STREAM) seq += base;
      if (staged) {
        s_stage[so++] = uint2{key, seq};
      } else if (o < A.out_cap) {
        A.m_key[o] = key;
#pragma unroll
        for (int x = 0; x < M; x++) A.p_seq[o * M + x] = seq - x;
      } else {
        atomicOr(A.overflow, 1u);
      }
      o++;
    }
  }
  if (!staged) return;
  __syncthreads();
  // thread i writes matches i, i + 256, ...: adjacent threads, adjacent slots
  for (uint32_t i = tid; i < block_total; i += kStThreads) {
    const uint64_t slot = toff + i;
    const uint2 e = s_stage[i];
    if (slot < A.out_cap) {
      A.m_key[slot] = e.x;
      if (M == 3) {  // one 12-B store per match
        *reinterpret_cast<uint3*>(A.p_seq + slot * 3) = uint3{e.y, e.y - 1, e.y - 2};
      } else {
#pragma unroll
        for (int x = 0; x < M; x++) A.p_seq[slot * M + x] = e.y - x;
      }
    } else {
      atomicOr(A.overflow, 1u);
    }
  }
}

// ---------------------------------------------------------------- streaming sessions
// A key's stream goes on from batch to batch.  A run of a strict chain lives at most M events,
// so all a key carries is one word: count << 32 | live, count its events so far and bit t of
// live (t < H = M - 1) set when its last t + 1 events satisfy stages 0..t - a run waits in
// stage t + 1.  One event with stage bits P (bit t = p_t(x)) steps it as
// live' = ((live << 1) | 1) & P; bit M - 1 of live' is a match ending at the event and is
// dropped (SURVEY A.5 over the concatenated stream).
//
// stencil_edge runs between stencil_mask and stencil_emit, a lane per key.  The head: the
// carried live stepped over the key's first min(len, H) events of the batch.  A match there is
// a window that begins in an earlier batch - wave_mask killed it as one crossing a key start,
// so its bit is this kernel's alone to set, ORed into the word's 32-bit half (keys share words)
// and counted for its stencil_emit block.  The tail: the state after the key's last event, from
// live = 0 over its last H events (a run older than H events is gone), or the head's state when
// the key has no more than H.  carry_next[k] = {count + len, live}; the session swaps the two
// arrays after the batch, so stencil_emit (sequence numbers: count before the batch) and this
// kernel read the same unmodified carry_prev.
//
// Two block-uniform routes, by the events the block's kEdgeKeys keys span.  Dense (the span
// fits kEdgeTile events; a processor's micro-batches, many keys of a few events each): the
// block streams the span once, 4 events a thread with 16-B loads, evaluates the stage bits of
// every event into an LDS byte each, and the lanes walk their heads and tails out of LDS - no
// event is loaded twice, no lane waits on a global load per event.  Sparse (long keys): a lane
// reads its key's first and last H events itself, at most 2 H scalar loads per key against the
// > kEdgeTile / kEdgeKeys events per key the mask pass streams.
// kEdgeTile: a byte an event, 8 KiB a block; 8 blocks a CU (the 32 waves a CU holds) take
// 64 KiB of its 160 KiB, so LDS never limits the occupancy.
constexpr int kEdgeKeys = 256;
constexpr int kEdgeTile = 8192;
constexpr uint64_t kStGroupEvents = kStGroupChunks * kStWave;  // events per group count

// c matches into counter g, for every lane of the wave: lanes with the same counter add once
__device__ __forceinline__ void edge_count(uint32_t* group_cnt, uint32_t g, uint32_t c, int lane) {
  uint64_t todo = __ballot(c != 0);
  while (todo) {  // (wave-uniform)
    const int j = __builtin_ctzll(todo);
    const uint32_t gj = (uint32_t)__builtin_amdgcn_readlane((int)g, j);
    const bool same = c != 0 && g == gj;
    uint32_t sum = same ? c : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == j) atomicAdd(group_cnt + gj, sum);
    todo &= ~__ballot(same);
  }
}

template <class EV>
__global__ void __launch_bounds__(kEdgeKeys) stencil_edge(StencilArgs A) {
  constexpr int M = EV::STAGES, H = M - 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint64_t k0 = (uint64_t)blockIdx.x * kEdgeKeys, k = k0 + tid;
  const bool valid = k < A.n_keys;
  uint64_t s = 0, e = 0, word = 0;
  if (valid) {
    s = A.key_off[k];
    e = A.key_off[k + 1];
    word = A.carry_prev[k];
  }
  const uint64_t len = e - s;
  if constexpr (H == 0) {  // a match is its own event: only the count advances
    if (valid) A.carry_next[k] = word + (len << 32);
  } else {
    __shared__ uint32_t s_bits[kEdgeTile / 4 + 2];  // a byte per event from `base`
    const EV ev(A);
    const uint64_t k1 = k0 + kEdgeKeys < A.n_keys ? k0 + kEdgeKeys : A.n_keys;
    const uint64_t b0 = A.key_off[k0], b1 = A.key_off[k1];  // the block's span
    const bool dense = b1 - b0 <= (uint64_t)kEdgeTile;
    const uint64_t base = b0 & ~3ull;  // (16-B loads: whole groups of 4 events)
    if (dense) {
      const uint32_t n4 = (uint32_t)((b1 - base + 3) / 4);  // <= kEdgeTile / 4 + 2
      for (uint32_t g = tid; g < n4; g += kEdgeKeys) {
        uint32_t P[M];
#pragma unroll
        for (int t = 0; t < M; t++) P[t] = 0;
        ev.bits4(A, base + 4ull * g, P);  // (events past the batch's end stay 0)
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < M; t++)
#pragma unroll
          for (int i = 0; i < 4; i++) w |= ((P[t] >> i) & 1u) << (8 * i + t);
        s_bits[g] = w;
      }
      __syncthreads();
    }
    // stage bits of event p (of this lane's key)
    auto bits = [&](uint64_t p) -> uint32_t {
      if (dense) return reinterpret_cast<const uint8_t*>(s_bits)[p - base];
      uint32_t P[M];
#pragma unroll
      for (int t = 0; t < M; t++) P[t] = 0;
      if constexpr (EV::RANGE) ev.range(ev.load1(A, p), P, 0);
      else ev.one(A, p, P, 0);
      uint32_t w = 0;
#pragma unroll
      for (int t = 0; t < M; t++) w |= (P[t] & 1u) << t;
      return w;
    };
    constexpr uint32_t kLive = (1u << H) - 1u;
    uint32_t live = (uint32_t)word & kLive;
    // head: at most H events, in at most two groups
    const uint32_t nh = len < (uint64_t)H ? (uint32_t)len : (uint32_t)H;
    const uint32_t g0 = (uint32_t)(s / kStGroupEvents);
    uint32_t c0 = 0, c1 = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < nh; i++) {
      const uint64_t p = s + i;
      live = ((live << 1) | 1u) & bits(p);
      if (live >> H) {
        atomicOr(reinterpret_cast<uint32_t*>(A.words + p / 64) + ((p >> 5) & 1), 1u << (p & 31));
        if ((uint32_t)(p / kStGroupEvents) == g0) c0++;
        else c1++;
      }
      live &= kLive;
    }
    edge_count(A.group_cnt, g0, c0, lane);
    edge_count(A.group_cnt, g0 + 1, c1, lane);
    if (len > (uint64_t)H) {  // tail
      live = 0;
#pragma unroll 1
      for (uint64_t p = e - H; p < e; p++) live = ((live << 1) | 1u) & bits(p);
      live &= kLive;
    }
    if (valid) A.carry_next[k] = (((word >> 32) + len) << 32) | live;
  }
}

// ---------------------------------------------------------------- semantic WITHIN
// With semantic windows (compile.cpp: an epsilon stage keeps its source stage's window) a run of
// a strict chain is dropped at the event of position p (2 <= p < M) when stage p - 1 has a
// window w and ts[s + p] - ts[s + 1] > w: the run's start time restarts at s + 1, because the
// epsilon stage after stage 0 is BEGIN-typed, and the subtraction is Java's (wrapping, signed
// compare).  Dropping it is the removePattern of a failed predicate on private nodes, so the
// matches are the predicate windows whose time conditions all hold - a conjunct independent of
// the stage bits.  stencil_within runs after stencil_mask (and stencil_edge) and before
// stencil_emit: it clears the match bits that fail and takes them off the emit blocks' counts,
// so stencil_emit reads what it would have read had the mask pass pruned.
//
// A wave owns the 64 word records of one mask chunk, a lane per word, and ballots the words
// holding a match bit: the others cost their record load and nothing else, and event times
// are read only around possible match ends.  Such a word is then the whole wave's: lane l
// stands for the match ending at event 64 w + l, the word's 64 times (one coalesced 8-B load)
// and the M - 2 before them (the halo) go to LDS once, and the start (lag M - 2) and the
// constrained positions (lag M - 1 - p, a wave-uniform mask) are read from there.  The loads
// of kWnBatch candidate words are in flight together.  A halo event before event 0, or before
// the key's start, belongs to a window the mask pass has killed; it is not loaded.
//
// STREAM: a match ending in a key's first M - 1 events of the batch began in an earlier one.
// Per key the session carries the last M - 2 event times of its stream (tsc_prev / tsc_next,
// swapped as the carry words are); a lag that reaches before the key's first event of the
// batch (the in-batch sequence number from the word record, or key_off where a key starts
// inside the word) is taken from tsc_prev.  The blocks after the chunks' write tsc_next, a
// lane per key: the last M - 2 times of tsc_prev followed by the key's events of the batch.
// (The live bits of the carry word stay unpruned: a run the window has already dropped still
// counts as live for cep_live_floor, which is then lower than it need be - never unsafe.)
constexpr int kWnBatch = 4;

// the time of event p (no times pushed: the event's position, as the NFA kernels take it)
__device__ __forceinline__ int64_t event_time(const StencilArgs& A, uint64_t p) {
  return A.ts ? A.ts[p] : (int64_t)p;
}

template <int M, bool STREAM>
__global__ void __launch_bounds__(kStThreads) stencil_within(StencilArgs A) {
  static_assert(M >= 3 && M <= kMaxStencil, "no position of a shorter chain is constrained");
  constexpr int L = M - 2;  // the start's lag behind the match end
  __shared__ int64_t s_t[kStThreads / 64][64 + L];  // a wave's word: events 64 w - L .. 64 w + 63
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n_blocks = (uint32_t)((A.n_chunk + 3) / 4);  // the chunks' blocks
  if (STREAM && blockIdx.x >= n_blocks) {  // (block-uniform) the keys' carried times
    const uint64_t k = (uint64_t)(blockIdx.x - n_blocks) * kStThreads + threadIdx.x;
    if (k >= A.n_keys) return;
    const uint64_t s = A.key_off[k], e = A.key_off[k + 1], len = e - s;
#pragma unroll
    for (int x = 0; x < L; x++) {
      const uint64_t r = (uint64_t)(L - 1 - x);  // events from the stream's end
      A.tsc_next[k * L + x] = r < len ? event_time(A, e - 1 - r) : A.tsc_prev[k * L + (L - 1) - (r - len)];
    }
    return;
  }
  const uint64_t chunk = (uint64_t)blockIdx.x * (kStThreads / 64) + wv;
  if (chunk >= A.n_chunk) return;  // (wave-uniform; no block-wide barrier below)
  const uint64_t n_words = (A.n_events + 63) / 64;
  const uint64_t w0 = chunk * (kStWave / 64);
  const uint4 rec = w0 + lane < n_words ? A.words[w0 + lane] : uint4{0, 0, 0, 0};
  uint64_t todo = __ballot((rec.x | rec.y) != 0);
  int64_t* const st = s_t[wv];
  uint32_t cleared = 0;  // (wave-uniform)
  while (todo) {
    int jw[kWnBatch];
    int64_t tm[kWnBatch], th[kWnBatch];
#pragma unroll
    for (int b = 0; b < kWnBatch; b++) {
      jw[b] = -1;
      tm[b] = th[b] = 0;
      if (todo) {
        jw[b] = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint64_t e0 = (w0 + (uint64_t)jw[b]) * 64;  // (< n_events: the word exists)
        if (e0 + lane < A.n_events) tm[b] = event_time(A, e0 + lane);
        if (lane < L && e0 >= (uint64_t)L) th[b] = event_time(A, e0 - L + lane);
      }
    }
#pragma unroll
    for (int b = 0; b < kWnBatch; b++) {
      const int j = jw[b];
      if (j < 0) break;
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)rec.x, j);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)rec.y, j);
      const uint32_t wk = (uint32_t)__builtin_amdgcn_readlane((int)rec.z, j);
      const uint32_t wsq = (uint32_t)__builtin_amdgcn_readlane((int)rec.w, j);
      const uint64_t nat = ((uint64_t)hi << 32) | lo;
      wave_sync();  // (the word before is read)
      st[L + lane] = tm[b];
      if (lane < L) st[lane] = th[b];
      wave_sync();
      const bool bit = (nat >> lane) & 1ull;
      bool ok = true;
      if (bit) {
        // events of the lane's key in the batch before the match end: a lag beyond them is
        // in an earlier batch (per-batch sessions: such a window is dead in the mask word)
        uint64_t seq = ~0ull;
        uint32_t key = wk & 0x7FFFFFFFu;
        if (STREAM) {
          seq = (uint64_t)wsq + (uint64_t)lane;
          if (wk >> 31) {  // a key starts inside the word
            const uint64_t p = (w0 + (uint64_t)j) * 64 + lane;
            while (p >= A.key_off[key + 1]) key++;  // (p < n_events = key_off[n_keys])
            seq = p - A.key_off[key];
          }
        }
        auto lag = [&](int d) -> int64_t {
          if (!STREAM || (uint64_t)d <= seq) return st[L + lane - d];
          return A.tsc_prev[(uint64_t)key * L + (uint64_t)(L - d) + seq];  // (d - seq events before the batch)
        };
        const uint64_t t0 = (uint64_t)lag(L);
#pragma unroll
        for (int p = 2; p < M; p++)
          if ((A.win_mask >> p) & 1u) ok = ok && (int64_t)((uint64_t)lag(M - 1 - p) - t0) <= A.win[p];
      }
      const uint64_t keep = nat & __ballot(ok);
      if (keep != nat) {
        cleared += (uint32_t)__popcll(nat ^ keep);
        if (lane == j) *reinterpret_cast<uint2*>(A.words + w0 + j) = uint2{(uint32_t)keep, (uint32_t)(keep >> 32)};
      }
    }
  }
  if (lane == 0 && cleared) atomicSub(A.group_cnt + chunk / kStGroupChunks, cleared);
}

// ---------------------------------------------------------------- host launchers
hipError_t launch_wave_keys(const uint64_t* key_off, uint64_t n_keys, uint64_t n_events, uint32_t* wave_key,
                            uint32_t* zero, uint32_t n_zero, hipStream_t st) {
  const uint64_t n_waves = (n_events + kStWave - 1) / kStWave;
  if (n_keys == 0 || n_waves == 0) return hipMemsetAsync(zero, 0, 4ull * n_zero, st);
  hipLaunchKernelGGL(wave_keys, dim3((uint32_t)((n_keys + 255) / 256)), dim3(256), 0, st, key_off, n_keys, n_waves,
                     wave_key, zero, n_zero);
  return hipGetLastError();
}

uint64_t stencil_waves(uint64_t n_events) { return (n_events + kStWave - 1) / kStWave; }

// the mask kernel of evaluator EV (an int32 or a typed instantiation for M stages), then the emit
// pass; a streaming session's batch (a.carry_prev): the edge kernel between them; semantic
// windows (a.win_mask): stencil_within before the emit pass
template <int M, class EV>
static hipError_t launch_one(void (*mask)(StencilArgs), const StencilArgs& a, uint64_t n_tiles, hipStream_t st) {
  // (a separate build for the whole fast-path chunks, without the slow path's code and
  // registers, measured the same - 79.5 against 79.6 us for 1e8 events - and cost a launch)
  StencilArgs b = a;
  b.n_chunk = (a.n_events + kStWave - 1) / kStWave;
  hipLaunchKernelGGL(mask, dim3((uint32_t)((b.n_chunk + 3) / 4)), dim3(kStThreads), 0, st, b);
  const dim3 eg((uint32_t)((n_tiles + kEmW - 1) / kEmW));
  const uint32_t wg = (uint32_t)((b.n_chunk + 3) / 4);  // stencil_within: a wave per chunk's words
  if (a.carry_prev) {
    if (a.n_keys)
      hipLaunchKernelGGL(stencil_edge<EV>, dim3((uint32_t)((a.n_keys + kEdgeKeys - 1) / kEdgeKeys)), dim3(kEdgeKeys), 0,
                         st, a);
    if constexpr (M >= 3)
      if (a.win_mask)  // (and a lane per key after them: the carried times)
        hipLaunchKernelGGL((stencil_within<M, true>), dim3(wg + (uint32_t)((a.n_keys + kStThreads - 1) / kStThreads)),
                           dim3(kStThreads), 0, st, b);
    hipLaunchKernelGGL((stencil_emit<M, true>), eg, dim3(kStThreads), 0, st, a);
  } else {
    if constexpr (M >= 3)
      if (a.win_mask) hipLaunchKernelGGL((stencil_within<M, false>), dim3(wg), dim3(kStThreads), 0, st, b);
    hipLaunchKernelGGL((stencil_emit<M, false>), eg, dim3(kStThreads), 0, st, a);
  }
  return hipGetLastError();
}

// The mask kernel by the widths of the range columns (StencilArgs.col_w): all int, the int32
// instantiations; any other, the typed ones
template <int M>
static hipError_t launch_m(const StencilArgs& a, bool range, int ncol, uint64_t n_tiles, hipStream_t st) {
  if (!range) return launch_one<M, StEval<M, false, 1>>(stencil_mask<M, false, 1>, a, n_tiles, st);
  const int w0 = a.col_w[0], w1 = ncol > 1 ? a.col_w[1] : 0;
  if (w0 == 4 && w1 == 0) return launch_one<M, StEval<M, true, 1>>(stencil_mask<M, true, 1>, a, n_tiles, st);
  if (w0 == 4 && w1 == 4) return launch_one<M, StEval<M, true, 2>>(stencil_mask<M, true, 2>, a, n_tiles, st);
  if (w0 == 8 && w1 == 0) return launch_one<M, StEvalT<M, 8, 0>>(stencil_mask_typed<M, 8, 0>, a, n_tiles, st);
  if (w0 == 4 && w1 == 8) return launch_one<M, StEvalT<M, 4, 8>>(stencil_mask_typed<M, 4, 8>, a, n_tiles, st);
  if (w0 == 8 && w1 == 8) return launch_one<M, StEvalT<M, 8, 8>>(stencil_mask_typed<M, 8, 8>, a, n_tiles, st);
  return hipErrorInvalidValue;  // (compile.cpp orders a mixed pair (4, 8))
}

hipError_t launch_stencil(int m, const StencilArgs& a, bool range, int ncol, hipStream_t st) {
  const uint64_t n_tiles = (a.n_events + kStTile - 1) / kStTile;
  if (n_tiles == 0) return hipSuccess;
  switch (m) {
    case 1: return launch_m<1>(a, range, ncol, n_tiles, st);
    case 2: return launch_m<2>(a, range, ncol, n_tiles, st);
    case 3: return launch_m<3>(a, range, ncol, n_tiles, st);
    case 4: return launch_m<4>(a, range, ncol, n_tiles, st);
    case 5: return launch_m<5>(a, range, ncol, n_tiles, st);
    case 6: return launch_m<6>(a, range, ncol, n_tiles, st);
    case 7: return launch_m<7>(a, range, ncol, n_tiles, st);
    case 8: return launch_m<8>(a, range, ncol, n_tiles, st);
  }
  return hipErrorInvalidValue;
}

// The passes after a mask kernel of another translation unit (stencil_lag.hip; per-batch
// sessions only: no carry): stencil_within where a window can fire, then stencil_emit
template <int M>
static hipError_t tail_m(const StencilArgs& a, hipStream_t st) {
  StencilArgs b = a;
  b.n_chunk = (a.n_events + kStWave - 1) / kStWave;
  const uint64_t n_tiles = (a.n_events + kStTile - 1) / kStTile;
  if constexpr (M >= 3)
    if (a.win_mask)
      hipLaunchKernelGGL((stencil_within<M, false>), dim3((uint32_t)((b.n_chunk + 3) / 4)), dim3(kStThreads), 0, st, b);
  hipLaunchKernelGGL((stencil_emit<M, false>), dim3((uint32_t)((n_tiles + kEmW - 1) / kEmW)), dim3(kStThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_stencil_tail(int m, const StencilArgs& a, hipStream_t st) {
  switch (m) {
    case 2: return tail_m<2>(a, st);
    case 3: return tail_m<3>(a, st);
    case 4: return tail_m<4>(a, st);
    case 5: return tail_m<5>(a, st);
    case 6: return tail_m<6>(a, st);
    case 7: return tail_m<7>(a, st);
    case 8: return tail_m<8>(a, st);
  }
  return hipErrorInvalidValue;
}

uint64_t stencil_tiles(uint64_t n_events) { return (n_events + kStTile - 1) / kStTile; }

}  // namespace cep
