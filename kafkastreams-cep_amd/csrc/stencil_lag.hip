// stencil_lag.hip — mask kernels of lagged strict chains: CEP_KIND_STENCIL queries whose stages
// compare an event with an earlier event of the same match (compile.cpp, "lagged chains").
//
// A stage t of such a chain reads a fold state X; the reference stores folds under (state, run)
// and a run of a ONE + strict chain never branches (nfa/NFA.java:148-157, 259-265), so what it
// reads is the fold expression of the last stage u < t that folds X, evaluated at the event
// t - u positions back: the predicate of a window position reads the columns at fixed lags of
// 1..7 inside the window, and a match is still a window of M events.  The mask
// phase (stencil_mask.h wave_mask: layout, window ANDs, key starts, seeds, word records) is the
// stencil's own, over two new evaluators; stencil_within and stencil_emit run on its output.
//
//   StEvalLag<M, T>   the fast route: one column of T (int, long, double); a stage is a range on
//                     it and at most one conjunct x[i] OP x[i - d], d wave-uniform in 1..7
//   StEvalLagI<M>     any other lagged chain: the stage's bytecode with its fold registers
//                     filled by the fold programs run at the lagged positions
//
// A lag never has to reach before the wave in the step loop: stage s reads at most s events
// back (d = t - u <= t), so a stage bit computed from an event before the wave's base belongs
// only to windows that begin before the base - those are ANDed with the zero words of "the step
// before the first" and settled from the seed events, which read global memory one event at a
// time.  The same holds for event 0 and (with the key-start kill) for a key's first event.
#include <hip/hip_runtime.h>

#include "cep_layout.h"
#include "interp.h"
#include "stencil_mask.h"

namespace cep {

// The fast route's data movement.  The value at i - d sits in the same lane, in lane l - 1 or
// l - 2, or in the previous step's last lanes: each wave keeps its last two steps in a private
// LDS ring, written once per step and read back at the lags.  The ring is transposed - element
// k of every quad together, ring[k][quad], quad = 64 (q & 1) + lane - so that the lanes of a
// read (event 4l + k - d: element (k - d) & 3 of quad l + floor((k - d) / 4)) and of a write
// touch consecutive words: no bank conflicts, where the events' own order (a 16-B store, reads
// at a stride of 4 words) would serialise every read 4 ways.  2 KiB a wave for int, 4 KiB for
// long and double; waves never share a ring, so no block barrier - wave_sync orders a step's
// writes before its reads and the reads before the next step's writes.
constexpr int kLagQuads = 128;  // quads of two steps

template <class T>
__device__ __forceinline__ T* lag_ring(int wv) {
  __shared__ T ring[kStThreads / 64][4 * kLagQuads];
  return ring[wv];
}

template <class T>
__device__ __forceinline__ bool lag_cmp(int op, T x, T y) {  // Java's primitive compares (IEEE for double)
  switch (op) {
    case 0: return x < y;
    case 1: return x <= y;
    case 2: return x > y;
    case 3: return x >= y;
    default: return x == y;
  }
}

template <int M, class T>
struct StEvalLag {
  static constexpr int STAGES = M;
  static constexpr bool RANGE = true;
  static constexpr int W = sizeof(T);
  static_assert(W == 4 || W == 8, "int, long or double");
  struct Ld {
    v4i v[W / 4];  // events 4l..4l+3 (8-byte: 4l, 4l+1 | 4l+2, 4l+3, low word first)
    int q;         // the step
  };
  struct Key {
    T x[4];
    int q;
  };
  struct Sd {
    uint32_t bits;  // bit s: stage s holds at the event
  };
  struct Cur {
    const v4i* c;
    __device__ __forceinline__ Cur(const StencilArgs& A, uint64_t wbase, int lane)
        : c(reinterpret_cast<const v4i*>(static_cast<const T*>(A.col[0]) + wbase) + (W / 4) * lane) {}
    __device__ __forceinline__ Ld load(int q) const {
      Ld d;
#pragma unroll
      for (int i = 0; i < W / 4; i++) d.v[i] = __builtin_nontemporal_load(c + q * 64 * (W / 4) + i);
      d.q = q;
      return d;
    }
  };
  // ranges as StEval (int32, clamped) and StEvalT (order keys); lags and compare ops per stage
  uint32_t lo4[M], span4[M];
  uint64_t lo8[M], span8[M], dmask;
  int d[M], op[M];
  T* ring;
  int lane;
  bool never = false;
  __device__ __forceinline__ explicit StEvalLag(const StencilArgs& A) {
    lane = threadIdx.x & 63;
    ring = lag_ring<T>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));  // (a wave per chunk: mask_chunk)
    dmask = A.col_dbl[0] ? (uint64_t)INT64_MAX : 0ull;
#pragma unroll
    for (int s = 0; s < M; s++) {
      const int64_t l = A.rs[s].lo[0], h = A.rs[s].hi[0];
      if (l > h) never = true;
      if (W == 4) {
        const int32_t l4 = l < INT32_MIN ? INT32_MIN : (l > INT32_MAX ? INT32_MAX : (int32_t)l);
        const int32_t h4 = h > INT32_MAX ? INT32_MAX : (h < INT32_MIN ? INT32_MIN : (int32_t)h);
        if (l > INT32_MAX || h < INT32_MIN) never = true;
        lo4[s] = (uint32_t)l4;
        span4[s] = (uint32_t)h4 - (uint32_t)l4;
      } else {
        lo8[s] = (uint64_t)l;
        span8[s] = (uint64_t)h - (uint64_t)l;
      }
      d[s] = A.lag_d[s];
      op[s] = A.lag_op[s];
    }
  }
  __device__ __forceinline__ bool in(int s, T x) const {
    if constexpr (W == 4) {
      return (uint32_t)x - lo4[s] <= span4[s];
    } else {
      uint64_t b;
      __builtin_memcpy(&b, &x, 8);
      return (b ^ ((uint64_t)((int64_t)b >> 63) & dmask)) - lo8[s] <= span8[s];
    }
  }
  static __device__ __forceinline__ T value(const Ld& l, int e) {
    if constexpr (W == 4) {
      return l.v[0][e];
    } else {
      const uint64_t b = ((uint64_t)(uint32_t)l.v[e >> 1][2 * (e & 1) + 1] << 32) | (uint32_t)l.v[e >> 1][2 * (e & 1)];
      T x;
      __builtin_memcpy(&x, &b, 8);
      return x;
    }
  }
  // once per step, in step order: the step's values, and into the ring
  __device__ __forceinline__ Key keys(const Ld& l) const {
    Key k;
    k.q = l.q;
#pragma unroll
    for (int e = 0; e < 4; e++) k.x[e] = value(l, e);
    const int quad = (l.q & 1) * 64 + lane;
    wave_sync();  // (the step before is read)
#pragma unroll
    for (int e = 0; e < 4; e++) ring[e * kLagQuads + quad] = k.x[e];
    wave_sync();
    return k;
  }
  __device__ __forceinline__ void ballot4(int s, const Key& k, uint64_t* Wd) const {
#pragma unroll
    for (int e = 0; e < 4; e++) Wd[e] = __builtin_amdgcn_ballot_w64(in(s, k.x[e]));
    const int dd = d[s];  // (wave-uniform, as op[s]: scalar branches)
    if (dd == 0) return;
    T y[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int j = e - dd;  // event 4 lane + j of this step (j < 0: earlier lanes, the step before)
      y[e] = ring[(j & 3) * kLagQuads + (((k.q & 1) * 64 + lane + (j >> 2)) & (kLagQuads - 1))];
    }
    auto conj = [&](auto f) {
#pragma unroll
      for (int e = 0; e < 4; e++) Wd[e] &= __builtin_amdgcn_ballot_w64(f(k.x[e], y[e]));
    };
    switch (op[s]) {
      case 0: conj([](T a, T b) { return a < b; }); break;
      case 1: conj([](T a, T b) { return a <= b; }); break;
      case 2: conj([](T a, T b) { return a > b; }); break;
      case 3: conj([](T a, T b) { return a >= b; }); break;
      default: conj([](T a, T b) { return a == b; }); break;
    }
  }
  // The slow routes (the tail chunk, an unaligned column, an empty stage, the seed events): one
  // event at a time from global memory, the same compares.  A lag before event 0: the window
  // crosses it and is dead, the stage bit stays 0.
  __device__ __forceinline__ Sd load1(const StencilArgs& A, uint64_t p) const {
    const T* col = static_cast<const T*>(A.col[0]);
    const T x = col[p];
    Sd v{0};
#pragma unroll
    for (int s = 0; s < M; s++) {
      bool ok = !never && in(s, x) && p >= (uint64_t)d[s];
      if (ok && d[s]) ok = lag_cmp<T>(op[s], x, col[p - (uint64_t)d[s]]);
      v.bits |= (ok ? 1u : 0u) << s;
    }
    return v;
  }
  __device__ __forceinline__ void range(const Sd& v, uint32_t* P, int bit) const {
#pragma unroll
    for (int s = 0; s < M; s++) P[s] |= ((v.bits >> s) & 1u) << bit;
  }
  __device__ __forceinline__ void slow4(const StencilArgs& A, uint64_t e0, uint32_t* P) const {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (e0 + i < A.n_events) range(load1(A, e0 + i), P, i);
  }
};

// The interpreted route: before stage s is evaluated at position p, the fold registers it reads
// are filled by running each state's fold program at p - lag (total and state-free: compile.cpp),
// none of them null.  A lag that reaches into the previous key is harmless - the programs are
// total and the mask phase kills every window crossing a key start.
template <int M>
struct StEvalLagI {
  static constexpr int STAGES = M;
  static constexpr bool RANGE = false;
  struct Ld {};
  struct Key {};
  struct Sd {};
  struct Cur {
    __device__ __forceinline__ Cur(const StencilArgs&, uint64_t, int) {}
    __device__ __forceinline__ Ld load(int) const { return {}; }
  };
  bool never = false;
  __device__ __forceinline__ explicit StEvalLagI(const StencilArgs&) {}
  // (the fast path's parts: never run, RANGE is false)
  __device__ __forceinline__ Key keys(const Ld&) const { return {}; }
  __device__ __forceinline__ void ballot4(int, const Key&, uint64_t* Wd) const { Wd[0] = Wd[1] = Wd[2] = Wd[3] = 0; }
  __device__ __forceinline__ Sd load1(const StencilArgs&, uint64_t) const { return {}; }
  __device__ __forceinline__ void one(const StencilArgs& A, uint64_t p, uint32_t* P, int bit) const {
    if (p >= A.n_events) return;
    for (int s = 0; s < M; s++) {
      int64_t Wf[kMaxStates];
      bool ok = true, rn;
      int ee = 0;
#pragma unroll
      for (int x = 0; x < kMaxStates; x++) {
        const uint64_t lag = A.lag_of[s][x];
        Wf[x] = 0;
        if (lag == 0 || !ok) continue;
        if (p < lag) {  // the window crosses event 0
          ok = false;
          continue;
        }
        const EvalIn fin{&A.cols, A.q->field_type, A.ts, p - lag, nullptr, 0, 0, true};
        Wf[x] = interp(A.code, A.lag_prog[s][x], fin, &rn, &ee);
      }
      const EvalIn in{&A.cols, A.q->field_type, A.ts, p, Wf, 0, 0, true};
      if (ok && interp(A.code, A.prog[s], in, &rn, &ee) != 0) P[s] |= 1u << bit;  // total: never throws
    }
  }
  __device__ __forceinline__ void slow4(const StencilArgs& A, uint64_t e0, uint32_t* P) const {
#pragma unroll
    for (int i = 0; i < 4; i++) one(A, e0 + i, P, i);
  }
};

template <int M, class T>
__global__ void __launch_bounds__(kStThreads) stencil_mask_lag(StencilArgs A) {
  mask_chunk<StEvalLag<M, T>>(A);
}

template <int M>
__global__ void __launch_bounds__(kStThreads) stencil_mask_lagi(StencilArgs A) {
  mask_chunk<StEvalLagI<M>>(A);
}

// ---------------------------------------------------------------- host launcher
hipError_t launch_stencil_tail(int m, const StencilArgs& a, hipStream_t st);  // stencil.hip

template <int M>
static void (*lag_kernel(const StencilArgs& a, bool fast))(StencilArgs) {
  if (!fast) return stencil_mask_lagi<M>;
  if (a.col_w[0] == 4) return stencil_mask_lag<M, int32_t>;
  return a.col_dbl[0] ? stencil_mask_lag<M, double> : stencil_mask_lag<M, int64_t>;
}

// the mask kernel of a lagged chain of m stages (fast: StEvalLag on col[0], else interpreted),
// then stencil.hip's passes
hipError_t launch_stencil_lag(int m, const StencilArgs& a, bool fast, hipStream_t st) {
  if (a.n_events == 0) return hipSuccess;
  void (*mask)(StencilArgs) = nullptr;
  switch (m) {
    case 2: mask = lag_kernel<2>(a, fast); break;
    case 3: mask = lag_kernel<3>(a, fast); break;
    case 4: mask = lag_kernel<4>(a, fast); break;
    case 5: mask = lag_kernel<5>(a, fast); break;
    case 6: mask = lag_kernel<6>(a, fast); break;
    case 7: mask = lag_kernel<7>(a, fast); break;
    case 8: mask = lag_kernel<8>(a, fast); break;
    default: return hipErrorInvalidValue;  // (a state read needs an earlier stage)
  }
  StencilArgs b = a;
  b.n_chunk = (a.n_events + kStWave - 1) / kStWave;
  hipLaunchKernelGGL(mask, dim3((uint32_t)((b.n_chunk + 3) / 4)), dim3(kStThreads), 0, st, b);
  return launch_stencil_tail(m, a, st);
}

}  // namespace cep
