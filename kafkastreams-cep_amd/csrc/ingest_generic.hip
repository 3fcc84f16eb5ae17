// ingest_generic.hip — cep_decode_json: JSON record values -> typed event columns for any field
// table (int, long and double columns; json_generic.h has the semantics and the number path).
//
// One lane per record, one pass.  A 256-record block stages its byte span into a 16 KiB LDS tile
// with coalesced 16-byte loads (a block whose span exceeds the tile parses from HBM) and copies
// the field table from the kernel argument into LDS beside it: hashes, lengths, types, column
// pointers and the packed names are read by every lane at the same address (LDS broadcast), the
// name bytes only on a hash + length hit.  Values go to their columns as they are lexed; a
// lane's state is registers only (no run-time-indexed arrays: the per-field kinds are packed
// 4 bits each).  There is no fixed-layout fast path and so no second pass: every record runs
// the state machine once.  The powers-of-five table of the number path (10 KiB, read-only,
// wave-divergent) stays in HBM/L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "json_generic.h"

namespace cep {

constexpr int kGenBlock = 256;
constexpr uint32_t kGenLds = 16384;  // bytes of record text staged per block
static_assert(kGenLds % (16 * kGenBlock) == 0, "the staging loads: whole 16-B chunks per thread");
static_assert(sizeof(jsong::Table) % 4 == 0, "the table is copied to LDS word by word");

__global__ void __launch_bounds__(kGenBlock) decode_json_kernel(
    const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ rec_off, uint64_t n, const jsong::Table targ,
    const uint64_t* __restrict__ pow5, uint32_t* __restrict__ span, int32_t* __restrict__ status) {
  __shared__ uint4 tile[kGenLds / 16];
  __shared__ jsong::Table tab;
  {
    const uint32_t* src = (const uint32_t*)&targ;
    uint32_t* dst = (uint32_t*)&tab;
    for (uint32_t i = threadIdx.x; i < sizeof(jsong::Table) / 4; i += kGenBlock) dst[i] = src[i];
  }
  const uint64_t r0 = (uint64_t)blockIdx.x * kGenBlock;
  const uint64_t r1 = r0 + kGenBlock < n ? r0 + kGenBlock : n;
  const uint64_t A = rec_off[r0], B = rec_off[r1];
  // aligned 16-byte chunks g0..g1 cover the block's span [A, B); a chunk that holds at least one
  // byte of the span never leaves its pages
  const uint64_t skew = (uintptr_t)bytes & 15;
  const uint64_t g0 = (A + skew) >> 4, g1 = (B + skew + 15) >> 4;
  const bool staged = (g1 - g0) * 16 <= kGenLds;
  if (staged) {
    const uint4* src = (const uint4*)((uintptr_t)bytes - skew);
    constexpr int kIt = kGenLds / 16 / kGenBlock;
    uint4 v[kIt];  // every load of the thread in flight before its LDS stores
#pragma unroll
    for (int i = 0; i < kIt; i++) {
      const uint64_t c = g0 + threadIdx.x + (uint64_t)i * kGenBlock;
      v[i] = c < g1 ? src[c] : uint4{0u, 0u, 0u, 0u};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kIt; i++) {
      const uint64_t c = g0 + threadIdx.x + (uint64_t)i * kGenBlock;
      if (c < g1) tile[c - g0] = v[i];
    }
  }
  __syncthreads();
  const uint64_t r = r0 + threadIdx.x;
  if (r >= n) return;
  const uint64_t a = rec_off[r], b = rec_off[r + 1];
  const uint32_t len = (uint32_t)(b - a);
  int32_t st;
  if (staged) {
    // LDS: 32-bit byte offset into the tile, words read with ds_read
    const uint32_t o = (uint32_t)(a + skew - (g0 << 4));
    const uint32_t* tw = (const uint32_t*)tile;
    const uint32_t w0 = o >> 2;
    auto wd = [tw, w0](uint32_t j) { return tw[w0 + j]; };
    jsong::Parser<decltype(wd)> P(wd, o & 3, &tab, pow5, r);
    st = P.run(len, span);
  } else {
    const uint32_t* words = (const uint32_t*)((uintptr_t)(bytes + a) & ~(uintptr_t)3);
    auto wd = [words](uint32_t j) { return words[j]; };
    jsong::Parser<decltype(wd)> P(wd, (uint32_t)((uintptr_t)(bytes + a) & 3), &tab, pow5, r);
    st = P.run(len, span);
  }
  status[r] = st;
}

hipError_t launch_decode_json(const uint8_t* bytes, const uint64_t* rec_off, uint64_t n, const jsong::Table& tab,
                              const uint64_t* pow5, uint32_t* span, int32_t* status, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((uint32_t)((n + kGenBlock - 1) / kGenBlock));
  hipLaunchKernelGGL(decode_json_kernel, grid, dim3(kGenBlock), 0, st, bytes, rec_off, n, tab, pow5, span, status);
  return hipGetLastError();
}

}  // namespace cep
