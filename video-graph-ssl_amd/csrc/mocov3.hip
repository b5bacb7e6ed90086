// MoCo v3's symmetrised cross-view InfoNCE (Chen, Xie, He 2021, Algorithm 1) and its gradient on gfx950.
// tests/mocov3_ref.py is the numpy statement.
//
//   q1, q2 (N, D) fp32: the student's predictor outputs;  k1, k2 (N, D) fp32: the momentum teacher's projector outputs.
//   direction 0 pairs (q, k) = (q1, k2), direction 1 pairs (q2, k1).  Per direction:
//   s[i,j]  = (sum_e q[i,e] k[j,e]) * inv_T                 exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32), fp32 accumulation
//   lse[i]  = log sum_j exp(s[i,j])                         ALL j, the diagonal included; online max / sum, rows NOT assumed unit
//   sp[i]   = s[i,i]          l_d = mean_i (lse[i] - sp[i])          rank[i] = #{j != i : s[i,j] >= sp[i]}
//   P[i,j]  = exp(s[i,j] - lse[i])
//   dq[i,:] = g w inv_T / N ( sum_j P[i,j] k[j,:] - k[i,:] )         nothing flows to k: the teacher is detached
//   loss    = w (l_0 + l_1)
//
// Both directions of a pass run in ONE grid (blockIdx.z), 32-row tiles of k streamed against one staged 32-row tile of q per
// workgroup; no N x N tensor exists.  Forward is 2 launches (tiles, then fold + loss), backward is 2 (tiles, then fold + scale).
//
//   forward   workgroup (column split, row tile, direction): wave w takes the split's column tiles w, w + WAVES, ...; A = the
//             staged q tile, B = the streamed k tile, so a lane holds 16 rows of ONE column.  sp comes first, from the diagonal of
//             the diagonal tile (q tile t against k tile t) -- the same k-ordered fma chain as the streamed value of s[i,i], so
//             the two are the same bits and `>=` ties are exact.  Per-lane running (reference, sum, count) for the lane's 16
//             rows; one cross-lane fold per wave, one per workgroup -> (m, sum, count) partials per (split, row) in `ws`.
//             mocov3_finish_kernel folds the splits in order and writes lse, rank and the three losses (one workgroup, fp64).
//   backward  a workgroup owns a 32-row tile of dq and streams the column tiles j of k: the s tile is recomputed TRANSPOSED
//             (A = streamed k tile, B = staged q tile), by the forward's fma chain, so P[i,j] sits with i on the lane and j in
//             the 16 accumulator registers, which is the A operand layout of the next product Y[i,:] += sum_j P[i,j] k[j,:]
//             (register r of lane half h is k = h of MFMA r: row j = (r&3) + 8(r>>2) + 4h) -- no trip through LDS; the B
//             operand is row j of the streamed tile, still in this wave's LDS.  (ntxent.hip does this with the roles swapped.)
//             Waves fold through LDS in wave order, column splits go to `ws` (or straight into dq for one split) and
//             mocov3_dq_kernel adds them in split order, applies the -k[i,:] term and the scale.
//
// One owner per output element and fixed fold orders everywhere: no atomics, bitwise reproducible.  Nothing reads the host, so
// both entries can be captured in a hipGraph.
//
// Dispatch (restated in tests/mocov3_ref.py: mocov3_path), a function of the arguments alone:
//   fast     D <= 256, D % 4 == 0, every pointer 16-byte aligned: 4 waves per workgroup, float4 loads with the next piece in
//            flight behind the MFMAs of the current one.  Features go through LDS in 128-wide chunks (zero-padded to a multiple
//            of 8) and s accumulates over them; the q tile is staged whole (2 chunks), which together with the 4 wave tiles is
//            99 KiB of LDS -- a third chunk would not leave room for them, hence the limit of 256.  The backward pass holds all
//            of its dq tile in accumulators; for D > 128 the first chunk of each k tile goes through LDS a second time, for
//            its part of P k, once P exists.
//   generic  everything else: 1 wave per workgroup, guarded scalar staging in 128-feature chunks (the backward pass repeats
//            the s tile per 128-column chunk of dq).
//   splits   as ntxent.hip, per direction: T = ceil(N / 32) tiles; splits = clamp(ceil(256 / T), 1, ceil(T / waves)) -- a
//            constant of the code, not of the device.
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

// generic path: acc += (rows abase .. of a) x (rows bbase .. of b) over every feature, staged chunk by chunk into A_ / B_
__device__ __forceinline__ void s_tile_generic(f32x16& acc, float* A_, float* B_, const float* __restrict__ a, int abase,
                                               const float* __restrict__ b, int bbase, int N, int D, int lane) {
  const int ll = lane & 31, lh = lane >> 5;
  for (int d0 = 0; d0 < D; d0 += FD) {
    wave_lds_sync();
    tile_stage_scalar(A_, a, abase, N, D, d0, lane);
    tile_stage_scalar(B_, b, bbase, N, D, d0, lane);
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

// ------------------------------------------------------------------------------------------------------------ forward
// grid (splits, row tiles, 2 directions).  Partials and sp are indexed by R = direction * N + i.
template <int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void mocov3_fwd_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ k1, const float* __restrict__ k2,
    int N, int D, float inv_T, int ntiles, int tps, float* __restrict__ pm, float* __restrict__ ps, int* __restrict__ pc,
    float* __restrict__ sp_out, gca_magic md4a, gca_magic md4b) {
  __shared__ __attribute__((aligned(16))) float Zs[(FAST ? MAXCH : 1) * TILE];   // the workgroup's q tile
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];                 // per-wave streamed k tile (one chunk)
  __shared__ float L0[WAVES][32];
  __shared__ float Red[WAVES][3][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, dt = blockIdx.y, i0 = dt * 32, dir = blockIdx.z;
  const float* __restrict__ q = dir ? q2 : q1;
  const float* __restrict__ k = dir ? k1 : k2;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  const int ct0 = split * tps + wave;
  const int ntw = ct0 < t_end ? (t_end - ct0 + WAVES - 1) / WAVES : 0;          // streamed tiles of this wave
  const int nch = FAST ? (D + FD - 1) / FD : 1;

  f32x4 v[NPC];
  if (FAST) {
    tile_fetch(v, k, i0, N, D, chunk_of(0, nch, D, md4a, md4b), lane);          // in flight while the q tile is staged
    tile_zero(Nw, lane);
    stage_q_tile<WAVES>(Zs, q, i0, N, D, nch, md4a, md4b, tid);
  }

  float l0r[16], mx[16], sm[16];
  int cn[16];
  // tile 0 of the sequence is the diagonal tile (the positives); tiles 1 .. ntw are the wave's share of the split
  for (int t = 0; t <= ntw; ++t) {
    const int ct = t == 0 ? dt : ct0 + (t - 1) * WAVES;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (FAST) {
      for (int c = 0; c < nch; ++c) {
        const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
        wave_lds_sync();                                                         // the previous piece's fragment reads are done
        tile_store(v, Nw, ch, lane);
        wave_lds_sync();
        int nc = c + 1, nt = t;                                                  // the next piece streams in behind the MFMAs
        if (nc == nch) { nc = 0; nt = t + 1; }
        if (nt > ntw) { nc = c; nt = t; }
        const int nct = nt == 0 ? dt : ct0 + (nt - 1) * WAVES;
        tile_fetch(v, k, nct * 32, N, D, chunk_of(nc, nch, D, md4a, md4b), lane);
        tile_mma(acc, Zs + c * TILE, Nw, (4 * ch.d4 + 7) >> 3, ll, lh);
      }
    } else {
      s_tile_generic(acc, Zs, Nw, q, i0, k, ct * 32, N, D, lane);
    }
    if (t == 0) {
      // ---- positive logits of the 32 rows: the diagonal of the diagonal tile
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc_row(r, lh) == ll) L0[wave][ll] = acc[r] * inv_T;
      wave_lds_sync();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        l0r[r] = L0[wave][acc_row(r, lh)];
        mx[r] = l0r[r]; sm[r] = 0.f; cn[r] = 0;
      }
      if (split == 0 && wave == 0 && lane < 32 && i0 + lane < N) sp_out[(long long)dir * N + i0 + lane] = L0[0][lane];
    } else {
      const int j = ct * 32 + ll;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + acc_row(r, lh);
        const float x = acc[r] * inv_T;
        if (j < N) {                                                             // the diagonal is inside the softmax
          float d = x - mx[r];
          if (d > 8.f) { sm[r] *= __expf(-d); mx[r] = x; d = 0.f; }              // moving reference: exp(d) stays far from overflow
          sm[r] += __expf(d);
          cn[r] += (j != i && x >= l0r[r]) ? 1 : 0;
        }
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
    const long long o = ((long long)split * 2 + dir) * N + i0 + tid;
    pm[o] = M; ps[o] = S; pc[o] = (int)Cn;
  }
}

// One workgroup: folds the splits of every row in split order, writes lse / rank / sp, then the losses (fp64, fixed order):
// loss[0] = w (l_0 + l_1), loss[1] = l_0, loss[2] = l_1.
__global__ __launch_bounds__(1024) void mocov3_finish_kernel(
    const float* __restrict__ pm, const float* __restrict__ ps, const int* __restrict__ pc, const float* __restrict__ sp,
    int N, int splits, float w, float* __restrict__ lse, int* __restrict__ rank, float* __restrict__ pos_logit,
    float* __restrict__ loss) {
  __shared__ double sh[2][16];
  const long long N2 = 2ll * N;
  for (int dir = 0; dir < 2; ++dir) {
    double part = 0.0;
    for (int i = threadIdx.x; i < N; i += 1024) {
      const long long R = (long long)dir * N + i;
      float M = pm[R];
      for (int s = 1; s < splits; ++s) M = fmaxf(M, pm[s * N2 + R]);
      float S = 0.f;
      int Cn = 0;
      for (int s = 0; s < splits; ++s) {
        const long long o = s * N2 + R;
        S += ps[o] * expf(pm[o] - M);
        Cn += pc[o];
      }
      const float l = M + logf(S);
      const float p = sp[R];
      lse[R] = l;
      if (rank) rank[R] = Cn;
      if (pos_logit) pos_logit[R] = p;
      part += (double)l - (double)p;
    }
    part = gca_wave_sum_d(part);
    if ((threadIdx.x & 63) == 0) sh[dir][threadIdx.x >> 6] = part;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l[2];
    for (int dir = 0; dir < 2; ++dir) {
      double t = 0.0;
      for (int wv = 0; wv < 16; ++wv) t += sh[dir][wv];
      l[dir] = t / (double)N;
    }
    loss[0] = (float)((double)w * (l[0] + l[1]));
    loss[1] = (float)l[0];
    loss[2] = (float)l[1];
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// grid (splits, row tiles of dq, 2 directions).  out_d + split * slab: where direction d's partial sums of this split go.

// Y[i, :] += sum_j P[i,j] k[j, :] for the 128 features in `Nw`: register r of P is the A operand of MFMA r
__device__ __forceinline__ void y_mma(f32x16 (&Y)[4], const f32x16& P, const float* Nw, int ll, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* kr = &Nw[acc_row(r, lh) * FP + ll];
#pragma unroll
    for (int c = 0; c < 4; ++c) Y[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(P[r], kr[32 * c], Y[c], 0, 0, 0);
  }
}
// s^T tile (row j in the registers, row i = i0 + ll on the lane) -> P in place
__device__ __forceinline__ void p_tile(f32x16& acc, int jb, int i, int N, float inv_T, float lse_i, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = jb + acc_row(r, lh);
    const float x = acc[r] * inv_T;
    acc[r] = (i < N && j < N) ? __expf(x - lse_i) : 0.f;
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
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void mocov3_bwd_fast_kernel(
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
  const float lse_i = lse[(long long)dir * N + (i < N ? i : N - 1)];
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
        if (x == nch - 1) p_tile(acc, jb, i, N, inv_T, lse_i, lh);
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
__global__ __launch_bounds__(64) void mocov3_bwd_generic_kernel(
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
  const float lse_i = lse[(long long)dir * N + (i < N ? i : N - 1)];
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
      s_tile_generic(acc, Nw, Zs, k, jb, q, i0, N, D, lane);
      if (D > FD) {                                                    // the chunk of k_j that this chunk of dq multiplies
        wave_lds_sync();
        tile_stage_scalar(Nw, k, jb, N, D, oc, lane);
        wave_lds_sync();
      }
      p_tile(acc, jb, i, N, inv_T, lse_i, lh);
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
__global__ __launch_bounds__(256) void mocov3_dq_kernel(const float* __restrict__ k1, const float* __restrict__ k2,
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
bool overlap(const float* a, const float* b, int64_t n) {                       // two n-float arrays
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * 4;
  return x < y + len && y < x + len;
}
// forward partials: (m, sum, count) per (split, direction, row) + the positive logits; 16-byte multiples
int64_t fwd_ws_bytes(int64_t N, int splits) { return gca_round_up((3 * (int64_t)splits + 1) * 2 * N * 4, 16); }
void last_chunk_magics(const Plan& p, int64_t D, gca_magic* a, gca_magic* b) {
  *a = gca_make_magic(FD / 4);
  const int64_t rest = D - (gca_ceil_div(D, FD) - 1) * FD;
  *b = gca_make_magic((unsigned)(p.fast ? rest / 4 : 1));
}

}  // namespace

extern "C" {

int64_t gca_mocov3_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {                        // the caller's pointers are not known here
    const Plan p = make_plan(N, D, aligned != 0);
    const int64_t f = fwd_ws_bytes(N, p.splits), bw = p.splits > 1 ? (int64_t)p.splits * 2 * N * D * 4 : 0;
    need = f > need ? f : need;
    need = bw > need ? bw : need;
  }
  return need;
}

int gca_mocov3_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits) {
  if (!sizes_ok(N, D)) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned != 0);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_mocov3_fwd(const float* q1, const float* q2, const float* k1, const float* k2, int64_t N, int64_t D, float inv_T,
                   float w, float* row_lse, float* pos_logit, int32_t* rank_ge, float* loss, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(inv_T) || !scalar_ok(w)) return GCA_EINVAL;
  if (!q1 || !q2 || !k1 || !k2 || !row_lse || !loss || !ws) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned16(q1) && aligned16(q2) && aligned16(k1) && aligned16(k2));
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)p.splits * 2 * N;
  float* pm = reinterpret_cast<float*>(ws);
  float* ps = pm + rows;
  int* pc = reinterpret_cast<int*>(ps + rows);
  float* sp = reinterpret_cast<float*>(pc + rows);
  gca_magic ma, mb;
  last_chunk_magics(p, D, &ma, &mb);
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles, 2);
  if (p.fast)
    hipLaunchKernelGGL((mocov3_fwd_kernel<4, true>), grid, dim3(256), 0, st, q1, q2, k1, k2, (int)N, (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, ma, mb);
  else
    hipLaunchKernelGGL((mocov3_fwd_kernel<1, false>), grid, dim3(64), 0, st, q1, q2, k1, k2, (int)N, (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, ma, mb);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(mocov3_finish_kernel, dim3(1), dim3(1024), 0, st, pm, ps, pc, sp, (int)N, p.splits, w, row_lse, rank_ge,
                     pos_logit, loss);
  return gca_launch_status();
}

int gca_mocov3_bwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* row_lse, int64_t N,
                   int64_t D, float inv_T, float w, const float* gscale_dev, float gscale_host, float* dq1, float* dq2, void* ws,
                   void* stream) {
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
  last_chunk_magics(p, D, &ma, &mb);
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles, 2);
  if (p.fast)
    hipLaunchKernelGGL((mocov3_bwd_fast_kernel<4>), grid, dim3(256), 0, st, q1, q2, k1, k2, row_lse, (int)N, (int)D, inv_T,
                       p.ntiles, p.tps, part0, part1, slab, ma, mb);
  else
    hipLaunchKernelGGL(mocov3_bwd_generic_kernel, grid, dim3(64), 0, st, q1, q2, k1, k2, row_lse, (int)N, (int)D, inv_T,
                       p.ntiles, p.tps, part0, part1, slab);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  const int64_t blocks = gca_ceil_div(n, 256 * 4);
  hipLaunchKernelGGL(mocov3_dq_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks), 2), dim3(256), 0, st, k1, k2, part0,
                     part1, slab, (int)N, (int)D, p.splits, inv_T, w, gscale_dev, gscale_host, dq1, dq2);
  return gca_launch_status();
}

}  // extern "C"
