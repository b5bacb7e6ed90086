// The 64 x 64 output tile on v_mfma_f32_32x32x2_f32 that barlow.hip and vicreg.hip share: a workgroup of 4 waves (2 x 2 waves
// of 32 x 32) walks the reduction axis in chunks of KC, staged in LDS as [k][TW] at pitch TP.  Everything here is local to the
// translation unit that includes it.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int KC = 32;               // reduction elements per staged chunk
constexpr int TW = 64;               // output tile edge of a workgroup
constexpr int TP = TW + 1;           // LDS pitch of a [k][64] chunk: the transposed staging writes with stride TP
constexpr int NPT = KC * TW / 256;   // elements of a chunk per thread
constexpr int FLUSH = 2048;          // rows of N after which the forward moves its accumulator tile into a second one

__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }
__device__ __forceinline__ float half_sum(float v) {         // over the 32 lanes of a wave half, valid in every lane
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// acc[A index][B index] += sum_k As[k][arow + .] Bs[k][bcol + .] over one chunk
__device__ __forceinline__ void chunk_mma(f32x16& acc, const float* As, const float* Bs, int arow, int bcol, int ll, int lh) {
#pragma unroll
  for (int k = 0; k < KC; k += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(k + lh) * TP + arow + ll], Bs[(k + lh) * TP + bcol + ll], acc, 0, 0, 0);
}

}  // namespace
