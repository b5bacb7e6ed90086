// Operand staging for the tile of mma_tile.h, shared by swav.hip and dino.hip.  Loads are clamped into the matrix, never
// predicated, so all of a chunk's loads are in flight at once; the store into LDS masks.  Everything here is local to the
// translation unit that includes it.
#pragma once
#include "mma_tile.h"

namespace {

// x-form: the matrix (R, L) is row-major along the reduction axis L.  Thread: reduction index k (= k0 + (tid & 31)), tile rows
// (tid >> 5) + 8 it  ->  dst[tid & 31][row].
__device__ __forceinline__ void xfetch(float (&v)[NPT], const float* __restrict__ m, int r0, int k, int R, int L, int tid) {
  const int kc = k < L ? k : L - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int r = r0 + (tid >> 5) + 8 * it;
    v[it] = m[(size_t)(r < R ? r : R - 1) * L + kc];
  }
}
__device__ __forceinline__ void xstore(const float (&v)[NPT], float* dst, int r0, int k, int R, int L, int tid) {
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int c = (tid >> 5) + 8 * it;
    dst[(tid & 31) * TP + c] = (r0 + c < R && k < L) ? v[it] : 0.f;
  }
}
// r-form: the matrix (R, W) has the reduction axis down its rows.  Thread: column `col` (= c0 + lane), rows k0 + wave + 4 it  ->
// dst[wave + 4 it][lane].
__device__ __forceinline__ void rfetch(float (&v)[NPT], const float* __restrict__ m, int k0, int col, int R, int W, int wave) {
  const int c = col < W ? col : W - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int r = k0 + wave + 4 * it;
    v[it] = m[(size_t)(r < R ? r : R - 1) * W + c];
  }
}
__device__ __forceinline__ void rstore(const float (&v)[NPT], float* dst, int k0, int col, int R, int W, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int kk = wave + 4 * it;
    dst[kk * TP + lane] = (k0 + kk < R && col < W) ? v[it] : 0.f;
  }
}

}  // namespace
