// NT-Xent (SimCLR's in-batch contrastive loss) and its gradient on gfx950.  tests/ntxent_ref.py is the numpy statement.
//
//   z (N, D) fp32, N = 2b: rows 0..b-1 are view 1, rows b..2b-1 view 2;  pos(i) = (i + b) mod N
//   s[i,j]  = (sum_d z[i,d] z[j,d]) * inv_T                 exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32), fp32 accumulation
//   lse[i]  = log sum_{j != i} exp(s[i,j])                  online max / sum, rows are NOT assumed unit-norm
//   sp[i]   = s[i,pos(i)]          loss = mean_i (lse[i] - sp[i])          rank[i] = #{j != i, pos(i) : s[i,j] >= sp[i]}
//   P[i,j]  = exp(s[i,j] - lse[i]) (0 on the diagonal)      W = P + P^T
//   dz[i,:] = g inv_T / N ( sum_j W[i,j] z[j,:] - 2 z[pos(i),:] )
//
// Both directions stream 32-row tiles of z against one staged 32-row tile per workgroup; no N x N tensor exists.
//
//   forward   workgroup (row tile, column split): wave w takes the split's column tiles w, w + WAVES, ...; A = the staged row
//             tile, B = the streamed tile, so a lane holds 16 rows of ONE column.  sp comes first, from one more MFMA tile
//             against the gathered rows pos(i) -- the same k-ordered fma chain as the streamed value of s[i,pos(i)], so the
//             two are the same bits and `>=` ties are exact.  Per-lane running (reference, sum, count) for the lane's 16
//             rows; one cross-lane fold per wave, one per workgroup -> (m, sum, count) partials per (row, split) in `ws`.
//             ntxent_finish_kernel folds the splits in order and writes lse, rank and the loss (one workgroup, fp64 sum).
//   backward  W is symmetric, so a workgroup owns a tile of COLUMNS j (= rows of dz) and streams the row tiles i: the s tile
//             is recomputed with A = streamed tile i, B = staged tile j; W[i,j] then sits with j on the lane and i in the 16
//             accumulator registers, which is the A operand layout of the next product Y[j,:] += sum_i W[i,j] z[i,:]
//             (register r of lane half h is k = h of MFMA r: row i = (r&3) + 8(r>>2) + 4h) -- no trip through LDS; the B
//             operand is row i of the streamed tile, still in this wave's LDS.  Waves fold through LDS in wave order, row
//             splits go to `ws` (or straight into dz for one split) and ntxent_dz_kernel adds them in split order, applies
//             the -2 z[pos] term and the scale.
//
// One owner per output element and fixed fold orders everywhere: no atomics, bitwise reproducible.  Nothing reads the host.
//
// Dispatch (restated in tests/ntxent_ref.py: ntxent_path):
//   fast     D <= 128, D % 4 == 0, z (and dz) 16-byte aligned: 4 waves per workgroup, float4 loads with the next tile in flight
//            behind the MFMAs of the current one, features zero-padded to a multiple of 8 in LDS.
//   generic  everything else: 1 wave per workgroup, guarded scalar staging in 128-feature chunks (s accumulates over the
//            chunks; the backward pass repeats the s tile per 128-column chunk of dz).
//   splits   T = ceil(N / 32) tiles; splits = clamp(ceil(256 / T), 1, ceil(T / waves)) for both directions -- a constant
//            of the code, not of the device, so results do not depend on where they were computed.
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
constexpr int TARGET_WG = 256;       // workgroups the splits aim for

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

// Row of z that slot r of a tile holds.  POS: the positives of rows base .. base + 31; else rows base .. base + 31.
// Rows past the end are clamped (every load is unconditional; the epilogues mask what they produce).
template <bool POS>
__device__ __forceinline__ int tile_row(int base, int r, int N, int b) {
  int i = base + r;
  i = i < N ? i : N - 1;
  if (POS) i = i + b < N ? i + b : i + b - N;
  return i;
}

// fast path: a 32 x D tile as NPC float4 per lane, all loads in flight at once (clamped, never predicated)
template <bool POS>
__device__ __forceinline__ void tile_fetch(f32x4 (&v)[NPC], const float* __restrict__ z, int base, int N, int b, int D,
                                           int d4, gca_magic md4, int lane) {
#pragma unroll
  for (int it = 0; it < NPC; ++it) {
    const int i = lane + 64 * it;
    const int r = (int)gca_fdiv((unsigned)i, md4), c4 = i - r * d4;
    v[it] = *reinterpret_cast<const f32x4*>(z + (long long)tile_row<POS>(base, r, N, b) * D + c4 * 4);
  }
}
__device__ __forceinline__ void tile_store(const f32x4 (&v)[NPC], float* dst, int d4, gca_magic md4, int lane) {
#pragma unroll
  for (int it = 0; it < NPC; ++it) {
    const int i = lane + 64 * it;
    const int r = (int)gca_fdiv((unsigned)i, md4), c4 = i - r * d4;
    if (i < 32 * d4) *reinterpret_cast<f32x4*>(&dst[r * FP + c4 * 4]) = v[it];
  }
}
// generic path: features [d0, d0 + FD) of a tile, zeros past D (one wave; lanes along the feature axis)
template <bool POS>
__device__ __forceinline__ void tile_stage_scalar(float* dst, const float* __restrict__ z, int base, int N, int b, int D,
                                                  int d0, int lane) {
  for (int e = lane; e < 32 * FD; e += 64) {
    const int r = e / FD, c = e % FD;
    dst[r * FP + c] = d0 + c < D ? z[(long long)tile_row<POS>(base, r, N, b) * D + d0 + c] : 0.f;
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

// s tile of (rows `abase` .. as A) x (rows `bbase` .. as B) into acc.  FAST: both tiles are already staged (A_, B_).
// Generic: stages both, chunk by chunk, into A_ / B_ (one wave).
template <bool FAST, bool APOS, bool BPOS>
__device__ __forceinline__ void s_tile(f32x16& acc, float* A_, float* B_, const float* __restrict__ z, int abase, int bbase,
                                       int N, int b, int D, int lane) {
  const int ll = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (FAST) {
    tile_mma(acc, A_, B_, (D + 7) >> 3, ll, lh);
  } else {
    for (int d0 = 0; d0 < D; d0 += FD) {
      wave_lds_sync();
      tile_stage_scalar<APOS>(A_, z, abase, N, b, D, d0, lane);
      tile_stage_scalar<BPOS>(B_, z, bbase, N, b, D, d0, lane);
      wave_lds_sync();
      const int dc = D - d0 < FD ? D - d0 : FD;
      tile_mma(acc, A_, B_, (dc + 7) >> 3, ll, lh);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ forward
template <int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void ntxent_fwd_kernel(
    const float* __restrict__ z, int N, int b, int D, float inv_T, int ntiles, int tps,
    float* __restrict__ pm, float* __restrict__ ps, int* __restrict__ pc, float* __restrict__ sp_out, gca_magic md4) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];              // the workgroup's row tile
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];       // per-wave streamed tile
  __shared__ float L0[WAVES][32];
  __shared__ float Red[WAVES][3][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32;
  const int d4 = D >> 2;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  int ct = split * tps + wave;

  f32x4 v[NPC];
  f32x16 acc;
  if (FAST) {
    tile_fetch<true>(v, z, i0, N, b, D, d4, md4, lane);                // the positives' rows, in flight while Zs is staged
    tile_zero(Nw, lane);                                               // (the zero padding of features D .. D + 3)
    for (int e = tid; e < TILE / 4; e += WAVES * 64) *reinterpret_cast<float4*>(&Zs[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int i = tid; i < 32 * d4; i += WAVES * 64) {
      const int r = (int)gca_fdiv((unsigned)i, md4), c4 = i - r * d4;
      *reinterpret_cast<float4*>(&Zs[r * FP + c4 * 4]) =
          *reinterpret_cast<const float4*>(z + (long long)tile_row<false>(i0, r, N, b) * D + c4 * 4);
    }
    tile_store(v, Nw, d4, md4, lane);
    __syncthreads();
    tile_fetch<false>(v, z, (ct < t_end ? ct : 0) * 32, N, b, D, d4, md4, lane);      // first streamed tile
  }
  // ---- positive logits of the 32 rows: the diagonal of (row tile) x (gathered positives)
  s_tile<FAST, false, true>(acc, Zs, Nw, z, i0, i0, N, b, D, lane);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (acc_row(r, lh) == ll) L0[wave][ll] = acc[r] * inv_T;
  wave_lds_sync();
  float l0r[16], mx[16], sm[16];
  int cn[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    l0r[r] = L0[wave][acc_row(r, lh)];
    mx[r] = l0r[r]; sm[r] = 0.f; cn[r] = 0;
  }
  if (split == 0 && wave == 0 && lane < 32 && i0 + lane < N) sp_out[i0 + lane] = L0[0][lane];

  // ---- stream the split's column tiles
  for (; ct < t_end; ct += WAVES) {
    if (FAST) {
      wave_lds_sync();                                                 // the previous tile's fragment reads are done
      tile_store(v, Nw, d4, md4, lane);
      wave_lds_sync();
      const int nxt = ct + WAVES;
      tile_fetch<false>(v, z, (nxt < t_end ? nxt : ct) * 32, N, b, D, d4, md4, lane);   // streams in behind the MFMAs
    }
    s_tile<FAST, false, false>(acc, Zs, Nw, z, i0, ct * 32, N, b, D, lane);
    const int j = ct * 32 + ll;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + acc_row(r, lh);
      const int pi = i + b < N ? i + b : i + b - N;
      const float x = acc[r] * inv_T;
      if (j < N && j != i) {
        float d = x - mx[r];
        if (d > 8.f) { sm[r] *= __expf(-d); mx[r] = x; d = 0.f; }      // moving reference: exp(d) stays far from overflow
        sm[r] += __expf(d);
        cn[r] += (j != pi && x >= l0r[r]) ? 1 : 0;
      }
    }
  }

  // ---- one cross-lane fold per wave, then the waves in order
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float M = half_max(mx[r]);
    const float S = half_sum(sm[r] * expf(mx[r] - M));
    const float Cn = half_sum((float)cn[r]);
    if (ll == 0) { const int m = acc_row(r, lh); Red[wave][0][m] = M; Red[wave][1][m] = S; Red[wave][2][m] = Cn; }
  }
  __syncthreads();
  if (tid < 32 && i0 + tid < N) {
    float M = Red[0][0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) M = fmaxf(M, Red[w][0][tid]);
    float S = 0.f, Cn = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { S += Red[w][1][tid] * expf(Red[w][0][tid] - M); Cn += Red[w][2][tid]; }
    const long long o = (long long)split * N + i0 + tid;
    pm[o] = M; ps[o] = S; pc[o] = (int)Cn;
  }
}

// One workgroup: folds the splits of every row in split order, writes lse / rank, then the loss (fp64, fixed order).
__global__ __launch_bounds__(1024) void ntxent_finish_kernel(
    const float* __restrict__ pm, const float* __restrict__ ps, const int* __restrict__ pc, const float* __restrict__ sp,
    int N, int splits, float* __restrict__ lse, int* __restrict__ rank, float* __restrict__ pos_logit,
    float* __restrict__ loss) {
  __shared__ double sh[16];
  double part = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    float M = pm[i];
    for (int s = 1; s < splits; ++s) M = fmaxf(M, pm[(long long)s * N + i]);
    float S = 0.f;
    int Cn = 0;
    for (int s = 0; s < splits; ++s) {
      const long long o = (long long)s * N + i;
      S += ps[o] * expf(pm[o] - M);
      Cn += pc[o];
    }
    const float l = M + logf(S);
    const float p = sp[i];
    lse[i] = l;
    if (rank) rank[i] = Cn;
    if (pos_logit) pos_logit[i] = p;
    part += (double)l - (double)p;
  }
  part = gca_wave_sum_d(part);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sh[w];
    *loss = (float)(t / (double)N);
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
template <int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void ntxent_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ lse, int N, int b, int D, float inv_T, int ntiles, int tps,
    float* __restrict__ part, gca_magic md4) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];              // the workgroup's column tile j (rows of dz)
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];       // per-wave streamed row tile i
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, j0 = blockIdx.y * 32;
  const int d4 = D >> 2;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  const int j = j0 + ll;
  const float lse_j = lse[j < N ? j : N - 1];
  float* out = part + (long long)split * N * D;

  for (int oc = 0; oc < D; oc += FD) {                                 // 128-column chunk of dz (fast path: the only one)
    int it = split * tps + wave;
    f32x4 v[NPC];
    if (FAST) {
      tile_fetch<false>(v, z, (it < t_end ? it : 0) * 32, N, b, D, d4, md4, lane);
      tile_zero(Nw, lane);
      for (int e = tid; e < TILE / 4; e += WAVES * 64) *reinterpret_cast<float4*>(&Zs[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
      __syncthreads();
      for (int i = tid; i < 32 * d4; i += WAVES * 64) {
        const int r = (int)gca_fdiv((unsigned)i, md4), c4 = i - r * d4;
        *reinterpret_cast<float4*>(&Zs[r * FP + c4 * 4]) =
            *reinterpret_cast<const float4*>(z + (long long)tile_row<false>(j0, r, N, b) * D + c4 * 4);
      }
      __syncthreads();
    }
    f32x16 Y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[q][r] = 0.f;

    for (; it < t_end; it += WAVES) {
      const int ib = it * 32;
      float li[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) { const int i = ib + acc_row(r, lh); li[r] = lse[i < N ? i : N - 1]; }
      if (FAST) {
        wave_lds_sync();                                               // the previous tile's operand reads are done
        tile_store(v, Nw, d4, md4, lane);
        wave_lds_sync();
        const int nxt = it + WAVES;
        tile_fetch<false>(v, z, (nxt < t_end ? nxt : it) * 32, N, b, D, d4, md4, lane);
      }
      f32x16 acc;
      s_tile<FAST, false, false>(acc, Nw, Zs, z, ib, j0, N, b, D, lane);
      if (!FAST && (D > FD)) {                                         // the chunk of z_i that this chunk of dz multiplies
        wave_lds_sync();
        tile_stage_scalar<false>(Nw, z, ib, N, b, D, oc, lane);
        wave_lds_sync();
      }
      // W = P + P^T in place, then Y[j, :] += sum_i W[i,j] z[i, :]: register r is the A operand of MFMA r
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ib + acc_row(r, lh);
        const float x = acc[r] * inv_T;
        acc[r] = (i < N && j < N && i != j) ? __expf(x - li[r]) + __expf(x - lse_j) : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* zr = &Nw[acc_row(r, lh) * FP + ll];
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], zr[32 * q], Y[q], 0, 0, 0);
      }
    }

    // ---- waves fold through LDS in wave order: Nw <- Y as [row j][feature]
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) Nw[acc_row(r, lh) * FP + 32 * q + ll] = Y[q][r];
    __syncthreads();
    if (FAST) {
      for (int e = tid; e < 32 * d4; e += WAVES * 64) {
        const int r = (int)gca_fdiv((unsigned)e, md4), c4 = e - r * d4;
        if (j0 + r < N) {
          float4 s = *reinterpret_cast<const float4*>(&Ns[0][r * FP + c4 * 4]);
#pragma unroll
          for (int w = 1; w < WAVES; ++w) {
            const float4 t = *reinterpret_cast<const float4*>(&Ns[w][r * FP + c4 * 4]);
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
          }
          *reinterpret_cast<float4*>(out + (long long)(j0 + r) * D + c4 * 4) = s;
        }
      }
    } else {
      for (int e = tid; e < 32 * FD; e += WAVES * 64) {
        const int r = e / FD, c = e % FD;
        if (j0 + r < N && oc + c < D) {
          float s = Ns[0][r * FP + c];
#pragma unroll
          for (int w = 1; w < WAVES; ++w) s += Ns[w][r * FP + c];
          out[(long long)(j0 + r) * D + oc + c] = s;
        }
      }
    }
    __syncthreads();
  }
}

// dz = g inv_T / N (sum over the splits, in split order, - 2 z[pos]).  With one split `part` IS dz (in place, element-wise).
__global__ __launch_bounds__(256) void ntxent_dz_kernel(const float* __restrict__ z, const float* part, int N, int b, int D,
                                                        int splits, float inv_T, const float* __restrict__ gscale_dev,
                                                        float gscale_host, float* dz) {
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  const float coef = g * inv_T / (float)N;
  const long long n = (long long)N * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int i = (int)e / D, d = (int)e - i * D;                      // (N * D < 2^31)
    const int pi = i + b < N ? i + b : i + b - N;
    float s = part[e];
    for (int sp = 1; sp < splits; ++sp) s += part[(long long)sp * n + e];
    dz[e] = coef * (s - 2.f * z[(long long)pi * D + d]);
  }
}

struct Plan { bool fast; int waves, ntiles, splits, tps; };

bool sizes_ok(int64_t N, int64_t D) {
  return N >= 2 && N <= 65536 && (N & 1) == 0 && D >= 1 && N * D < (1ll << 31);
}
Plan make_plan(int64_t N, int64_t D, bool aligned) {
  Plan p;
  p.fast = D <= FD && D % 4 == 0 && aligned;
  p.waves = p.fast ? 4 : 1;
  p.ntiles = (int)gca_ceil_div(N, 32);
  const int want = (int)gca_ceil_div(TARGET_WG, p.ntiles), cap = (int)gca_ceil_div(p.ntiles, p.waves);
  p.splits = want < 1 ? 1 : (want > cap ? cap : want);
  p.tps = (int)gca_ceil_div(p.ntiles, p.splits);
  return p;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// forward partials: (m, sum, count) per (split, row) + the positive logits; 16-byte multiples so the backward slabs stay aligned
int64_t fwd_ws_bytes(int64_t N, int splits) { return gca_round_up((3 * (int64_t)splits + 1) * N * 4, 16); }

}  // namespace

extern "C" {

int64_t gca_ntxent_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  int64_t need = 0;
  for (int aligned = 0; aligned < 2; ++aligned) {                        // the caller's pointers are not known here
    const Plan p = make_plan(N, D, aligned != 0);
    const int64_t f = fwd_ws_bytes(N, p.splits), bw = p.splits > 1 ? (int64_t)p.splits * N * D * 4 : 0;
    need = f > need ? f : need;
    need = bw > need ? bw : need;
  }
  return need;
}

int gca_ntxent_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits) {
  if (!sizes_ok(N, D)) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned != 0);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_ntxent_fwd(const float* z, int64_t N, int64_t D, float inv_T, float* row_lse, float* pos_logit, int32_t* rank_ge,
                   float* loss, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !(inv_T > 0.f) || isinf(inv_T)) return GCA_EINVAL;
  if (!z || !row_lse || !loss || !ws) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned16(z));
  hipStream_t st = (hipStream_t)stream;
  float* pm = reinterpret_cast<float*>(ws);
  float* ps = pm + (int64_t)p.splits * N;
  int* pc = reinterpret_cast<int*>(ps + (int64_t)p.splits * N);
  float* sp = reinterpret_cast<float*>(pc + (int64_t)p.splits * N);
  const gca_magic md4 = gca_make_magic((unsigned)(p.fast ? D / 4 : 1));
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles);
  if (p.fast)
    hipLaunchKernelGGL((ntxent_fwd_kernel<4, true>), grid, dim3(256), 0, st, z, (int)N, (int)(N / 2), (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, md4);
  else
    hipLaunchKernelGGL((ntxent_fwd_kernel<1, false>), grid, dim3(64), 0, st, z, (int)N, (int)(N / 2), (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, md4);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(ntxent_finish_kernel, dim3(1), dim3(1024), 0, st, pm, ps, pc, sp, (int)N, p.splits, row_lse, rank_ge,
                     pos_logit, loss);
  return gca_launch_status();
}

int gca_ntxent_bwd(const float* z, const float* row_lse, int64_t N, int64_t D, float inv_T, const float* gscale_dev,
                   float gscale_host, float* dz, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !(inv_T > 0.f) || isinf(inv_T)) return GCA_EINVAL;
  if (!z || !row_lse || !dz || !ws) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned16(z) && aligned16(dz) && aligned16(ws));
  hipStream_t st = (hipStream_t)stream;
  float* part = p.splits > 1 ? reinterpret_cast<float*>(ws) : dz;
  const gca_magic md4 = gca_make_magic((unsigned)(p.fast ? D / 4 : 1));
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles);
  if (p.fast)
    hipLaunchKernelGGL((ntxent_bwd_kernel<4, true>), grid, dim3(256), 0, st, z, row_lse, (int)N, (int)(N / 2), (int)D, inv_T,
                       p.ntiles, p.tps, part, md4);
  else
    hipLaunchKernelGGL((ntxent_bwd_kernel<1, false>), grid, dim3(64), 0, st, z, row_lse, (int)N, (int)(N / 2), (int)D, inv_T,
                       p.ntiles, p.tps, part, md4);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  const int64_t n = N * D;
  const int64_t blocks = gca_ceil_div(n, 256 * 4);
  hipLaunchKernelGGL(ntxent_dz_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, z, part, (int)N,
                     (int)(N / 2), (int)D, p.splits, inv_T, gscale_dev, gscale_host, dz);
  return gca_launch_status();
}

}  // extern "C"
