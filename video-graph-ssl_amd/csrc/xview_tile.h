// The 32-row tile machinery of the cross-view contrastive kernels (mocov3.hip, nnclr.hip) on v_mfma_f32_32x32x2_f32: staging
// of 32 x 128-feature chunks through LDS, the k-ordered score chain, and the backward pass that both share -- a workgroup owns
// a 32-row tile of the gradient, streams the tiles of the other operand, recomputes the s tile transposed and multiplies P
// into the streamed rows without a trip through LDS.  The two users differ in ONE place: which row's log-sum-exp normalises
// P (template parameter COL_LSE of the backward kernels):
//   COL_LSE = false   the softmax runs over the STREAMED rows: P = exp(s - lse[owned row])       MoCo v3, gradient to q
//   COL_LSE = true    the softmax runs over the OWNED rows:    P = exp(s - lse[streamed row])    NNCLR, gradient to p
// Everything here is local to the translation unit that includes it.
#pragma once
#include <cstdint>
#include "gca_common.h"
#include <math.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int FD = 128;              // features per staged chunk
constexpr int FP = FD + 4;           // LDS row pitch: 128-bit fragment reads of 32 rows are conflict-free
constexpr int NPC = FD / 8;          // float4 pieces of a 32 x FD tile per lane
constexpr int TILE = 32 * FP;
constexpr int MAXCH = 2;             // chunks of the fast path
constexpr int FAST_MAXD = MAXCH * FD;
constexpr int TARGET_WG = 256;       // workgroups (per direction) the splits aim for

__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }
__device__ __forceinline__ float half_max(float v) {        // over the 32 lanes of a wave half, valid in every lane
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Rows past the end are clamped (every load is unconditional; the epilogues mask what they produce).
__device__ __forceinline__ int tile_row(int base, int r, int N) {
  const int i = base + r;
  return i < N ? i : N - 1;
}

// One chunk of the feature axis: columns [c0, c0 + 4 d4) of a row, d4 float4 wide.
struct Chunk { int c0, d4; gca_magic md4; };

// fast path: a 32-row chunk as NPC float4 per lane, all loads in flight at once (clamped, never predicated)
__device__ __forceinline__ void tile_fetch(f32x4 (&v)[NPC], const float* __restrict__ x, int base, int N, int D, Chunk ch,
                                           int lane) {
#pragma unroll
  for (int it = 0; it < NPC; ++it) {
    const int i = lane + 64 * it;
    const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
    v[it] = *reinterpret_cast<const f32x4*>(x + (long long)tile_row(base, r, N) * D + ch.c0 + c4 * 4);
  }
}
// ... into a wave's LDS tile; an odd number of float4 gets four zeros behind it (the MFMA steps take 8 features)
__device__ __forceinline__ void tile_store(const f32x4 (&v)[NPC], float* dst, Chunk ch, int lane) {
#pragma unroll
  for (int it = 0; it < NPC; ++it) {
    const int i = lane + 64 * it;
    const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
    if (i < 32 * ch.d4) *reinterpret_cast<f32x4*>(&dst[r * FP + c4 * 4]) = v[it];
  }
  if ((ch.d4 & 1) && lane < 32) *reinterpret_cast<float4*>(&dst[lane * FP + ch.d4 * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
}
// generic path: features [d0, d0 + FD) of a tile, zeros past D (one wave; lanes along the feature axis)
__device__ __forceinline__ void tile_stage_scalar(float* dst, const float* __restrict__ x, int base, int N, int D, int d0,
                                                  int lane) {
  for (int e = lane; e < 32 * FD; e += 64) {
    const int r = e / FD, c = e % FD;
    dst[r * FP + c] = d0 + c < D ? x[(long long)tile_row(base, r, N) * D + d0 + c] : 0.f;
  }
}
__device__ __forceinline__ void tile_zero(float* dst, int lane) {
  for (int e = lane; e < TILE / 4; e += 64) *reinterpret_cast<float4*>(&dst[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
}
// wave-private LDS tile: DS operations of one wave execute in order, so a fence for the compiler is all a store -> read
// (or read -> next store) hand-over between the lanes of that wave needs
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc[rows of A][rows of B] += A . B^T over `nt` 8-feature steps (both operands [row][k], the same k permutation)
__device__ __forceinline__ void tile_mma(f32x16& acc, const float* A, const float* B, int nt, int ll, int lh) {
  for (int t = 0; t < nt; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(&A[ll * FP + 8 * t + 4 * lh]);
    const float4 bq = *reinterpret_cast<const float4*>(&B[ll * FP + 8 * t + 4 * lh]);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq.w, acc, 0, 0, 0);
  }
}

// generic path: acc += (rows abase .. of a, Na rows in all) x (rows bbase .. of b, Nb rows in all) over every feature, staged
// chunk by chunk into A_ / B_
__device__ __forceinline__ void s_tile_generic(f32x16& acc, float* A_, float* B_, const float* __restrict__ a, int abase, int Na,
                                               const float* __restrict__ b, int bbase, int Nb, int D, int lane) {
  const int ll = lane & 31, lh = lane >> 5;
  for (int d0 = 0; d0 < D; d0 += FD) {
    wave_lds_sync();
    tile_stage_scalar(A_, a, abase, Na, D, d0, lane);
    tile_stage_scalar(B_, b, bbase, Nb, D, d0, lane);
    wave_lds_sync();
    const int dc = D - d0 < FD ? D - d0 : FD;
    tile_mma(acc, A_, B_, (dc + 7) >> 3, ll, lh);
  }
}

// fast path: chunk c of a D-wide row (md4a divides by 32, a full chunk's float4 count; md4b by the last chunk's)
__device__ __forceinline__ Chunk chunk_of(int c, int nch, int D, gca_magic md4a, gca_magic md4b) {
  Chunk ch;
  ch.c0 = c * FD;
  const bool last = c == nch - 1;
  ch.d4 = last ? (D - ch.c0) >> 2 : FD / 4;
  ch.md4 = last ? md4b : md4a;
  return ch;
}

// fast path: the whole q tile (rows i0 ..) into Zs[chunk][TILE], zero-padded; ends with a workgroup barrier
template <int WAVES>
__device__ __forceinline__ void stage_q_tile(float* Zs, const float* __restrict__ q, int i0, int N, int D, int nch,
                                             gca_magic md4a, gca_magic md4b, int tid) {
  for (int e = tid; e < MAXCH * TILE / 4; e += WAVES * 64) *reinterpret_cast<float4*>(&Zs[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
    for (int i = tid; i < 32 * ch.d4; i += WAVES * 64) {
      const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
      *reinterpret_cast<float4*>(&Zs[c * TILE + r * FP + c4 * 4]) =
          *reinterpret_cast<const float4*>(q + (long long)tile_row(i0, r, N) * D + ch.c0 + c4 * 4);
    }
  }
  __syncthreads();
}

// ----------------------------------------------------------------------------------------------------------- backward
// grid (splits, row tiles of dq, 2 directions).  out_d + split * slab: where direction d's partial sums of this split go.
// q is the OWNED operand (a workgroup owns 32 of its rows and their gradient), k the STREAMED one.

// Y[i, :] += sum_j P[i,j] k[j, :] for the 128 features in `Nw`: register r of P is the A operand of MFMA r
__device__ __forceinline__ void y_mma(f32x16 (&Y)[4], const f32x16& P, const float* Nw, int ll, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* kr = &Nw[acc_row(r, lh) * FP + ll];
#pragma unroll
    for (int c = 0; c < 4; ++c) Y[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(P[r], kr[32 * c], Y[c], 0, 0, 0);
  }
}
// s^T tile (streamed row j in the registers, owned row i = i0 + ll on the lane) -> P in place.  lse_i: the owned row's
// log-sum-exp; lse_d: the direction's N log-sum-exps, read by streamed row when COL_LSE.
template <bool COL_LSE>
__device__ __forceinline__ void p_tile(f32x16& acc, int jb, int i, int N, float inv_T, float lse_i,
                                       const float* __restrict__ lse_d, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = jb + acc_row(r, lh);
    const float x = acc[r] * inv_T;
    const float l = COL_LSE ? lse_d[j < N ? j : N - 1] : lse_i;
    acc[r] = (i < N && j < N) ? __expf(x - l) : 0.f;
  }
}
__device__ __forceinline__ void y_to_lds(float* Nw, const f32x16 (&Y)[4], int ll, int lh) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) Nw[acc_row(r, lh) * FP + 32 * c + ll] = Y[c][r];
}

// fast path: the workgroup holds ALL of its dq tile (MAXCH x 4 accumulators per wave).  Per k tile a wave stages chunks
// 0 .. nch - 1 (s accumulates), forms P, multiplies it into the chunk still in LDS (the last), then stages the earlier chunks
// once more for their part of Y: one more trip of those chunks through LDS, no second s tile.
template <int WAVES, bool COL_LSE>
__global__ __launch_bounds__(WAVES * 64) void xview_bwd_fast_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ k1, const float* __restrict__ k2,
    const float* __restrict__ lse, int N, int D, float inv_T, int ntiles, int tps, float* __restrict__ out0,
    float* __restrict__ out1, long long slab, gca_magic md4a, gca_magic md4b) {
  static_assert(MAXCH == 2, "the Y accumulators below are written out for two chunks");
  __shared__ __attribute__((aligned(16))) float Zs[MAXCH * TILE];                // the workgroup's q tile (rows of dq)
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];                 // per-wave streamed k tile (one chunk)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32, dir = blockIdx.z;
  const float* __restrict__ q = dir ? q2 : q1;
  const float* __restrict__ k = dir ? k1 : k2;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  const int jt0 = split * tps + wave;
  const int ntw = jt0 < t_end ? (t_end - jt0 + WAVES - 1) / WAVES : 0;
  const int nch = (D + FD - 1) / FD;
  const int ni = 2 * nch - 1;                                                    // pieces per k tile: chunks 0 .. nch-1, 0 .. nch-2
  const int i = i0 + ll;
  const float* __restrict__ lse_d = lse + (long long)dir * N;
  const float lse_i = lse_d[i < N ? i : N - 1];
  float* out = (dir ? out1 : out0) + (long long)split * slab;

  f32x4 v[NPC];
  if (ntw > 0) tile_fetch(v, k, jt0 * 32, N, D, chunk_of(0, nch, D, md4a, md4b), lane);
  tile_zero(Nw, lane);
  stage_q_tile<WAVES>(Zs, q, i0, N, D, nch, md4a, md4b, tid);

  f32x16 Y0[4], Y1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { Y0[c][r] = 0.f; Y1[c][r] = 0.f; }

  for (int t = 0; t < ntw; ++t) {
    const int jb = (jt0 + t * WAVES) * 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int x = 0; x < ni; ++x) {
      const int c = x < nch ? x : x - nch;
      const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
      wave_lds_sync();                                                           // the previous piece's operand reads are done
      tile_store(v, Nw, ch, lane);
      wave_lds_sync();
      int nx = x + 1, nt = t;                                                    // the next piece streams in behind the MFMAs
      if (nx == ni) { nx = 0; nt = t + 1; }
      if (nt >= ntw) { nx = x; nt = t; }
      tile_fetch(v, k, (jt0 + nt * WAVES) * 32, N, D, chunk_of(nx < nch ? nx : nx - nch, nch, D, md4a, md4b), lane);
      if (x < nch) {
        tile_mma(acc, Nw, Zs + c * TILE, (4 * ch.d4 + 7) >> 3, ll, lh);
        if (x == nch - 1) p_tile<COL_LSE>(acc, jb, i, N, inv_T, lse_i, lse_d, lh);
      }
      if (x >= nch - 1) {                                                        // P exists: this chunk's part of Y
        if (c == 0) y_mma(Y0, acc, Nw, ll, lh);
        else y_mma(Y1, acc, Nw, ll, lh);
      }
    }
  }

  // ---- waves fold through LDS in wave order, chunk by chunk: Nw <- Y as [row i][feature]
  for (int c = 0; c < nch; ++c) {
    wave_lds_sync();
    if (c == 0) y_to_lds(Nw, Y0, ll, lh);
    else y_to_lds(Nw, Y1, ll, lh);
    __syncthreads();
    const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
    for (int e = tid; e < 32 * ch.d4; e += WAVES * 64) {
      const int r = (int)gca_fdiv((unsigned)e, ch.md4), c4 = e - r * ch.d4;
      if (i0 + r < N) {
        float4 s = *reinterpret_cast<const float4*>(&Ns[0][r * FP + c4 * 4]);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
          const float4 u = *reinterpret_cast<const float4*>(&Ns[w][r * FP + c4 * 4]);
          s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        *reinterpret_cast<float4*>(out + (long long)(i0 + r) * D + ch.c0 + c4 * 4) = s;
      }
    }
    __syncthreads();
  }
}

// generic path: one wave; the s tile is repeated per 128-column chunk of dq
template <bool COL_LSE>
__global__ __launch_bounds__(64) void xview_bwd_generic_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ k1, const float* __restrict__ k2,
    const float* __restrict__ lse, int N, int D, float inv_T, int ntiles, int tps, float* __restrict__ out0,
    float* __restrict__ out1, long long slab) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];                        // the q tile (rows of dq), one chunk at a time
  __shared__ __attribute__((aligned(16))) float Nw[TILE];                        // the streamed k tile, one chunk at a time
  const int lane = threadIdx.x;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32, dir = blockIdx.z;
  const float* __restrict__ q = dir ? q2 : q1;
  const float* __restrict__ k = dir ? k1 : k2;
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  const int i = i0 + ll;
  const float* __restrict__ lse_d = lse + (long long)dir * N;
  const float lse_i = lse_d[i < N ? i : N - 1];
  float* out = (dir ? out1 : out0) + (long long)split * slab;

  for (int oc = 0; oc < D; oc += FD) {                                 // 128-column chunk of dq
    f32x16 Y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[c][r] = 0.f;
    for (int jt = split * tps; jt < t_end; ++jt) {
      const int jb = jt * 32;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      s_tile_generic(acc, Nw, Zs, k, jb, N, q, i0, N, D, lane);
      if (D > FD) {                                                    // the chunk of k_j that this chunk of dq multiplies
        wave_lds_sync();
        tile_stage_scalar(Nw, k, jb, N, D, oc, lane);
        wave_lds_sync();
      }
      p_tile<COL_LSE>(acc, jb, i, N, inv_T, lse_i, lse_d, lh);
      y_mma(Y, acc, Nw, ll, lh);
    }
    wave_lds_sync();
    y_to_lds(Nw, Y, ll, lh);
    wave_lds_sync();
    for (int e = lane; e < 32 * FD; e += 64) {
      const int r = e / FD, c = e % FD;
      if (i0 + r < N && oc + c < D) out[(long long)(i0 + r) * D + oc + c] = Nw[r * FP + c];
    }
  }
}

// dq = g w inv_T / N (sum over the splits, in split order, - k).  With one split `part` IS dq (in place, element-wise).
// grid.y is the direction; direction d reads k = d ? k1 : k2.
__global__ __launch_bounds__(256) void xview_dq_kernel(const float* __restrict__ k1, const float* __restrict__ k2,
                                                       const float* part0, const float* part1, long long slab, int N, int D,
                                                       int splits, float inv_T, float w, const float* __restrict__ gscale_dev,
                                                       float gscale_host, float* dq1, float* dq2) {
  const int dir = blockIdx.y;
  const float* __restrict__ k = dir ? k1 : k2;
  const float* part = dir ? part1 : part0;
  float* dq = dir ? dq2 : dq1;
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  const float coef = g * w * inv_T / (float)N;
  const long long n = (long long)N * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    float s = part[e];
    for (int sp = 1; sp < splits; ++sp) s += part[(long long)sp * slab + e];
    dq[e] = coef * (s - k[e]);
  }
}

struct Plan { bool fast; int waves, ntiles, splits, tps; };

bool sizes_ok(int64_t N, int64_t D) { return N >= 1 && N <= 65536 && D >= 1 && N * D < (1ll << 31); }
bool scalar_ok(float x) { return x > 0.f && !isinf(x); }                        // (NaN fails the comparison)
Plan make_plan(int64_t N, int64_t D, bool aligned) {
  Plan p;
  p.fast = D <= FAST_MAXD && D % 4 == 0 && aligned;
  p.waves = p.fast ? 4 : 1;
  p.ntiles = (int)gca_ceil_div(N, 32);
  const int want = (int)gca_ceil_div(TARGET_WG, p.ntiles), cap = (int)gca_ceil_div(p.ntiles, p.waves);
  p.splits = want < 1 ? 1 : (want > cap ? cap : want);
  p.tps = (int)gca_ceil_div(p.ntiles, p.splits);
  return p;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool overlap2(const float* a, int64_t na, const float* b, int64_t nb) {         // an na-float and an nb-float array
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)nb * 4 && y < x + (uintptr_t)na * 4;
}
bool overlap(const float* a, const float* b, int64_t n) { return overlap2(a, n, b, n); }
void last_chunk_magics(bool fast, int64_t D, gca_magic* a, gca_magic* b) {
  *a = gca_make_magic(FD / 4);
  const int64_t rest = D - (gca_ceil_div(D, FD) - 1) * FD;
  *b = gca_make_magic((unsigned)(fast ? rest / 4 : 1));
}
// bytes of the backward pass's slabs in `ws`: [split][direction][N * D] (none with one split)
int64_t xview_bwd_ws_bytes(int64_t N, int64_t D, int splits) { return splits > 1 ? (int64_t)splits * 2 * N * D * 4 : 0; }

// The backward entry both users share: dq1 (direction 0: q1 owned, k2 streamed, lse[0 .. N)) and dq2 (direction 1: q2 owned,
// k1 streamed, lse[N .. 2 N)) = g w inv_T / N (sum_streamed P k - k[owned index]).  Refuses (GCA_EINVAL, nothing launched) bad
// sizes or scalars, NULL pointers and an output overlapping an input or the other output.
template <bool COL_LSE>
int xview_bwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* row_lse, int64_t N, int64_t D,
              float inv_T, float w, const float* gscale_dev, float gscale_host, float* dq1, float* dq2, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(inv_T) || !scalar_ok(w)) return GCA_EINVAL;
  if (!q1 || !q2 || !k1 || !k2 || !row_lse || !dq1 || !dq2 || !ws) return GCA_EINVAL;
  // dq is written (as partial sums, with one split) while other workgroups still read q and k: no output may overlap an input
  const int64_t n = N * D;
  const float* ins[4] = {q1, q2, k1, k2};
  for (int a = 0; a < 4; ++a)
    if (overlap(ins[a], dq1, n) || overlap(ins[a], dq2, n)) return GCA_EINVAL;
  if (overlap(dq1, dq2, n)) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned16(q1) && aligned16(q2) && aligned16(k1) && aligned16(k2) && aligned16(dq1) &&
                                     aligned16(dq2) && aligned16(ws));
  hipStream_t st = (hipStream_t)stream;
  // slabs in `ws`: [split][direction][N * D]
  float* part0 = p.splits > 1 ? reinterpret_cast<float*>(ws) : dq1;
  float* part1 = p.splits > 1 ? reinterpret_cast<float*>(ws) + n : dq2;
  const long long slab = p.splits > 1 ? 2 * n : 0;
  gca_magic ma, mb;
  last_chunk_magics(p.fast, D, &ma, &mb);
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles, 2);
  if (p.fast)
    hipLaunchKernelGGL((xview_bwd_fast_kernel<4, COL_LSE>), grid, dim3(256), 0, st, q1, q2, k1, k2, row_lse, (int)N, (int)D,
                       inv_T, p.ntiles, p.tps, part0, part1, slab, ma, mb);
  else
    hipLaunchKernelGGL((xview_bwd_generic_kernel<COL_LSE>), grid, dim3(64), 0, st, q1, q2, k1, k2, row_lse, (int)N, (int)D,
                       inv_T, p.ntiles, p.tps, part0, part1, slab);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  const int64_t blocks = gca_ceil_div(n, 256 * 4);
  hipLaunchKernelGGL(xview_dq_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks), 2), dim3(256), 0, st, k1, k2, part0,
                     part1, slab, (int)N, (int)D, p.splits, inv_T, w, gscale_dev, gscale_host, dq1, dq2);
  return gca_launch_status();
}

}  // namespace
