// stencil_mask.h — the mask phase of the strict-contiguity stencil, shared by the translation
// units that instantiate a mask kernel (stencil.hip: range and interpreted predicates;
// stencil_lag.hip: predicates that read the column at a lag).  wave_mask<EV> is the phase of one
// wave over an evaluator EV, mask_chunk<EV> a mask kernel's whole body.
//
// An evaluator gives wave_mask the column-typed parts: STAGES, RANGE (false: interpreted
// predicates, one event at a time); Ld, a lane's 4 events of a step as loaded; Cur(A, wbase,
// lane), the wave's load cursor with load(q); keys(Ld), what the stages compare, once per step
// and in step order; ballot4(s, keys, W); `never`; and for the slow routes Sd, one event's
// values (load1), range(Sd, P, bit), slow4() and one().
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "stencil_args.h"

namespace cep {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kStThreads = 256;
constexpr int kStPer = 64;  // events per thread (one 64-bit mask)
constexpr uint64_t kStTile = (uint64_t)kStThreads * kStPer;
constexpr int kStWave = kStTile / (kStThreads / 64);  // 4096 events per wave of stencil_mask

// bit m of a 16-bit value -> bit 4 m
__device__ __forceinline__ uint64_t spread4(uint32_t x16) {
  uint64_t x = x16;
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

// Pass 1 layout.  A wave owns kStWave consecutive events and reads them with 16-B loads in
// which lane l holds events 4l..4l+3 of a 256-event step: every load instruction covers
// 1 KiB contiguous (fully coalesced).  Per step the M stage predicates go straight into scalar
// ballot words and the windows are ANDs of shifted words (stage s sits M-1-s events back).
constexpr int kStSteps = kStWave / 256;               // 16 load steps per wave

// LDS writes of a wave's lanes ordered before the reads of its other lanes (no instruction)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// What the mask phase leaves a wave (kStWave events from wbase), per lane, for its natural
// 64-event word (events ws .. ws + 63, ws = wbase + 64 lane):
struct WaveMask {
  uint64_t nat;   // bit i: a match (a window of M events of one key) ends at event ws + i
  uint64_t bw;    // bit i: a key starts at event ws + i
  uint32_t wkey;  // the key holding event ws (the largest key whose offset is <= ws)
  uint64_t wks;   // that key's first event
};

// The mask phase of one wave.  The steps' loads are double-buffered (one step in flight while
// the other computes) and the step loop carries nothing but the stage words of the previous
// step: the windows that reach back before the wave (the first M-1 ending in it) and the
// windows crossing a key start are settled after the loop, on the natural words, with vector
// work.  (This keeps the loop's scalar registers down - 58 instead of 106, 8 waves per SIMD
// instead of 6 - and the pass at ~75 us for 1e8 events instead of ~90: profiles/r05/.)
template <class EV>
__device__ __forceinline__ void wave_mask(const StencilArgs& A, const uint64_t wbase, const int lane, WaveMask& out) {
  constexpr int M = EV::STAGES;
  constexpr bool RANGE = EV::RANGE;
  constexpr int H = M - 1;              // events a window reaches back
  using Ld = typename EV::Ld;
  const EV ev(A);
  const bool fast = RANGE && A.aligned && wbase + kStWave <= A.n_events && !ev.never;
  // The fast path's first step is requested before anything else: the key-start words and
  // the seed events below are dependent round trips
  const typename EV::Cur cur(A, wbase, lane);
  Ld la{};
  if (fast) la = cur.load(0);
  // the key holding the wave's first event (wave_keys)
  const uint64_t n_waves = (A.n_events + kStWave - 1) / kStWave;  // n_events >= 1: the tile exists
  const uint64_t wi = wbase / kStWave;
  const uint32_t k0 = A.wave_key[wi < n_waves ? wi : n_waves - 1];
  // the seed events wbase - H .. wbase + H - 1 (lane j < 2H: event wbase - H + j): the windows
  // ending at the wave's first H events, settled after the loop
  const int64_t sp = (int64_t)wbase - H + lane;
  const bool sv = H > 0 && lane < 2 * H && sp >= 0 && (uint64_t)sp < A.n_events;
  typename EV::Sd sd{};
  if (RANGE && sv) sd = ev.load1(A, (uint64_t)sp);
  // Key starts in [wbase - 8, wend): lanes read key_off[k0 - 8 + 64 c + lane] (the 8 keys
  // before k0 may start among the 8 events before the wave) and a wave-uniform loop visits
  // the starts in range, in key order.  bw: this lane's start bits, pkb: starts among the 8
  // events before the wave (bit x: event wbase - 8 + x), wkey: the key holding event ws (for
  // stencil_emit: the largest key whose offset is <= it; empty keys share their successor's
  // offset and lose to it).
  const uint64_t wend = wbase + kStWave < A.n_events ? wbase + kStWave : A.n_events;
  const uint64_t lo = wbase >= 8 ? wbase - 8 : 0;
  const uint64_t ws = wbase + (uint64_t)lane * 64;
  uint64_t bw = 0;
  uint32_t pkb = 0, wkey = k0;
  uint64_t wks = 0;  // wkey's first event (stencil_emit: sequence numbers without key_off)
  if (wbase < A.n_events) {
    for (int64_t i0 = (int64_t)k0 - 8;; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool valid = i >= 0 && (uint64_t)i < A.n_keys;
      const uint64_t sj = valid ? A.key_off[i] : 0;
      if (i0 == (int64_t)k0 - 8)  // (lane 8 of the first chunk read k0's offset)
        wks = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(sj >> 32), 8) << 32) |
              (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sj, 8);
      uint64_t inr = __ballot(valid && sj >= lo && sj < wend);
      while (inr) {
        const int j = __builtin_ctzll(inr);
        inr &= inr - 1;
        const uint64_t sjj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(sj >> 32), j) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sj, j);
        if (sjj >= wbase) {
          if (((sjj - wbase) >> 6) == (uint64_t)lane) bw |= 1ull << (sjj & 63);
        } else {
          pkb |= 1u << (uint32_t)(sjj - (wbase - 8));
        }
        if (sjj <= ws) {
          wkey = (uint32_t)(i0 + j);
          wks = sjj;
        }
      }
      const uint64_t s63 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(sj >> 32), 63) << 32) |
                           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sj, 63);
      if (!(i0 + 64 < (int64_t)A.n_keys && s63 < wend)) break;  // no key after this chunk starts in range
    }
  }
  // Ballot words of the previous step (bit l of W[s][k] = stage s holds at event 4l + k),
  // zero before the wave's first step: windows reaching back before the wave are settled
  // below from the seed events
  uint64_t pW[M][4];
#pragma unroll
  for (int s = 0; s < M; s++)
#pragma unroll
    for (int k = 0; k < 4; k++) pW[s][k] = 0;
  uint64_t myword = 0;  // ballot layout: word k of step q for lane 4q + k
  // step q of the wave: x holds its 4 events per lane on the fast path (FAST: a
  // std::integral_constant, so each loop below gets its own straight-line body)
  auto step = [&](const int q, const Ld& x, auto fast_c) {
    constexpr bool FAST = decltype(fast_c)::value;
    const uint64_t e0 = wbase + (uint64_t)q * 256 + (uint64_t)lane * 4;
    // stage words of this step (wave-uniform, scalar registers)
    uint64_t W[M][4];
    if (FAST) {
      const auto& k = ev.keys(x);
#pragma unroll
      for (int s = 0; s < M; s++) ev.ballot4(s, k, W[s]);
    } else {
      uint32_t P[M];
#pragma unroll
      for (int s = 0; s < M; s++) P[s] = 0;
      ev.slow4(A, e0, P);
#pragma unroll
      for (int s = 0; s < M; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) W[s][k] = __builtin_amdgcn_ballot_w64((P[s] >> k) & 1u);
    }
    // word k: windows ending at events 4l + k.  Stage s sits o = M-1-s events back: event
    // 4l + k - o is word (k - o) mod 4, `cr` lanes back (bits shifted up, the previous
    // step's top bits carried in).
    uint64_t m[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      m[k] = ~0ull;
#pragma unroll
      for (int s = 0; s < M; s++) {
        const int t = k - (M - 1 - s);
        const int cr = t >= 0 ? 0 : (3 - t) / 4;
        const int kk = t + 4 * cr;
        m[k] &= cr == 0 ? W[s][kk] : ((W[s][kk] << cr) | (pW[s][kk] >> (64 - cr)));
      }
    }
    // lane 4q + k keeps word k (vector compare + select: no scalar work)
    const int lrel = lane - 4 * q;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (lrel == k) myword = m[k];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int s = 0; s < M; s++) pW[s][k] = W[s][k];
  };
  if (fast) {
    // two one-step buffers: while one step computes, the other's load is in flight.  The
    // loads are unconditional (the last pair re-reads its own step): a load under a branch
    // makes the waitcnt pass drain every outstanding load before the first use.
    Ld lb;
#pragma unroll 1
    for (int q = 0; q < kStSteps; q += 2) {
      lb = cur.load(q + 1);
      step(q, la, std::true_type{});
      const int qn = q + 2 < kStSteps ? q + 2 : q;
      la = cur.load(qn);
      step(q + 1, lb, std::true_type{});
    }
  } else {
    const Ld z{};
    for (int q = 0; q < kStSteps; q++) step(q, z, std::false_type{});
  }
  // natural words: events wbase + 256 q + 64 r + i (q = lane / 4, r = lane % 4) are bits
  // 16 r .. 16 r + 15 of the ballot words of step q, held by lanes 4q .. 4q + 3
  uint64_t nat = 0;
  {
    const int q4 = lane & ~3, r16 = 16 * (lane & 3);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t wk = __shfl(myword, q4 + k, 64);
      nat |= spread4((uint32_t)(wk >> r16) & 0xFFFFu) << k;
    }
  }
  if (H > 0) {
    // the windows ending at events wbase + i, i < H (they reach back before the wave): stage
    // bits of the seed events, bit j of S[s] = stage s holds at event wbase - H + j; the window
    // ending at wbase + i holds iff bit i + s of S[s] is set for every s
    uint32_t P[M];
#pragma unroll
    for (int s = 0; s < M; s++) P[s] = 0;
    if (sv) {
      if constexpr (RANGE) ev.range(sd, P, 0);
      else ev.one(A, (uint64_t)sp, P, 0);
    }
    uint64_t seed = wbase >= (uint64_t)H ? (1ull << H) - 1ull : 0ull;
#pragma unroll
    for (int s = 0; s < M; s++) seed &= __ballot(P[s] & 1u) >> s;
    if (lane == 0) nat |= seed;
    // a key start at any of a window's last M-1 events (offsets 0 .. M-2) kills it: the start
    // bits spread over the H events after them, carried across words (lane 0: the starts among
    // the 8 events before the wave)
    // (the shuffle outside the select: a permute reading an inactive lane returns 0)
    const uint64_t up = __shfl_up(bw, 1, 64);
    const uint64_t pw = lane == 0 ? (uint64_t)pkb << 56 : up;
    uint64_t kill = bw;
#pragma unroll
    for (int o = 1; o < H; o++) kill |= (bw << o) | (pw >> (64 - o));
    nat &= ~kill;
  }
  if (ws >= A.n_events) nat = 0;  // (the seed bits of a wave past the end)
  out.nat = nat;
  out.bw = bw;
  out.wkey = wkey;
  out.wks = wks;
}

// stencil_emit's block: kEmW mask tiles; the mask pass counts matches per emit block
constexpr int kEmW = 4;
constexpr uint64_t kStGroupChunks = kEmW * (kStTile / kStWave);  // chunks per group count: an emit block's

// Pass 1: per 4096-event chunk (a wave) the mask phase, its natural words, their keys and
// sequence numbers, and the match count per kStGroupChunks chunks (one stencil_emit block's
// span: its offset is the sum of the counts before it).  Each wave adds its own count: no
// block-wide barrier ties four waves together, and a counter takes 16 waves' atomics (probe,
// profiles/r05/: for 1e8 events the mask phase alone 65.4 us, with the three word stores 76.6,
// with a block-wide tile count and an atomic per 64 tiles 84.4; an atomic per wave into
// counters of 256 waves 156).  (A launch of resident waves looping over the chunks, so a
// chunk's stores overlap the next chunk's loads, measured 142 us: the loop's scalar state spills.)

template <class EV>
__device__ __forceinline__ void mask_chunk(const StencilArgs& A) {
  // wv through readfirstlane: the compiler cannot see that threadIdx.x >> 6 is wave-uniform,
  // and everything derived from it (the fast-path branch, the ballot words) would go to VGPRs
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t chunk = (uint64_t)blockIdx.x * (kStThreads / 64) + wv;
  if (chunk >= A.n_chunk) return;  // (wave-uniform; no barrier below)
  const uint64_t wbase = chunk * kStWave;
  WaveMask o;
  wave_mask<EV>(A, wbase, lane, o);
  const uint64_t ws = wbase + (uint64_t)lane * 64;
  // (bit 31: a key starts inside the word after its first event - stencil_emit walks key_off
  // there; elsewhere a match's sequence number is word_seq + its offset in the word)
  if (ws < A.n_events)  // one 16-B store per word (three separate word arrays cost 2-3 us more)
    A.words[ws / 64] = uint4{(uint32_t)o.nat, (uint32_t)(o.nat >> 32), o.wkey | ((o.bw & ~1ull) ? 0x80000000u : 0u),
                             (uint32_t)(ws - o.wks)};
  // matches of the chunk: popcount of each lane's word, summed over the wave
  uint32_t cnt = (uint32_t)__popcll(o.nat);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane == 0 && cnt) atomicAdd(A.group_cnt + chunk / kStGroupChunks, cnt);  // (no return value)
}

}  // namespace cep
