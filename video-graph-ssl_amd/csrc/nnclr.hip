// NNCLR (Dwibedi et al. 2021, "With a Little Help from My Friends", Algorithm 1) on gfx950: the nearest-neighbour search of
// both views in the support set, with the gather of the winning rows, and the gradient of the loss to the predictions.
// tests/nnclr_ref.py is the numpy statement.  The forward loss is gca_mocov3_fwd(q1 = nn1, q2 = nn2, k1 = p1, k2 = p2, w = 1/2).
//
//   search   z1, z2 (N, D), Q (K, D) fp32:  s[v][i,j] = sum_e z_v[i,e] Q[j,e]      exact-fp32 matrix cores, one k-ordered chain
//            key(s) = s, -inf where s is NaN;   idx[v][i] = the SMALLEST j with key = max_j key;   sim[v][i] = that key;
//            nn_v[i,:] = Q[idx[v][i],:], bit for bit.  Candidates are pairs (key, j) under ONE order everywhere -- a beats b
//            iff key_a > key_b or (key_a == key_b and j_a < j_b) -- starting from (-inf, INT_MAX), which every real column
//            beats: idx is always in [0, K) (and clamped into it once more before the gather).
//   launch 1 nnclr_search_*_kernel, grid (K-splits, row-tile groups): a workgroup scores its split's 32-row tiles of Q
//            against its group's row tiles of BOTH views (the 2 ceil(N/32) tiles of z1 then z2, taken in order), keeps a
//            running (key, j) per lane and row in registers, folds the 32 lanes of a column half once at the end and writes
//            one pair per (split, view, row) to `ws`.  No (2N, K) tensor exists.
//   launch 2 nnclr_pick_kernel, one 64-thread workgroup per (view, row): folds the splits in split order, writes idx and sim
//            and copies the winning row of Q.
//   fast     D <= 256, D % 4 == 0, z1, z2, Q 16-byte aligned: 4 waves, each owning ONE row tile staged whole in LDS (4 tiles
//            x 2 chunks x 16.5 KiB = 132 KiB); the Q tile goes through ONE shared 16.5 KiB chunk buffer that the 256 threads
//            fill with float4 loads issued a piece ahead, under the MFMAs of the current piece.  148.5 KiB of the 160 KiB of
//            LDS: a fifth row tile, or a second Q buffer, does not fit, so groups hold 4 row tiles -- up to N = 64 per view
//            the support set is streamed ONCE for both views; past that once per group of 128 rows.
//   generic  everything else: 1 wave, one row tile per workgroup, guarded scalar staging (xview_tile.h: s_tile_generic).
//   splits   kt = ceil(K / 32) tiles of Q, G row-tile groups: want = clamp(ceil(256 / G), 1, kt), tps = ceil(kt / want),
//            splits = ceil(kt / tps): no split is empty, and each holds a real column.  A constant of the code, not the device.
//
//   backward dp[j,:] = g w inv_T / N ( sum_i P[i,j] nn[i,:] - nn[j,:] ),  P[i,j] = exp(s[i,j] - lse[i]),  s = (nn[i] . p[j]) inv_T
//            -- the softmax runs over the predictions, so the gradient goes to the COLUMN operand and lse is indexed by the
//            streamed row.  That is xview_tile.h's backward with COL_LSE: owned operand p, streamed operand nn.  Direction 0
//            (rows nn1, columns p2) gives dp2, direction 1 (nn2, p1) gives dp1.
//
// No atomics, one owner per output, fixed fold orders: bitwise repeatable.  Nothing reads the host: capturable.
#include "xview_tile.h"
#include <limits.h>

namespace {

constexpr int SRT = 4;               // row tiles (of the two views together) beside the Q chunk on the fast path
constexpr int NPW = NPC / 4;         // float4 pieces of a 32 x FD chunk per thread of a 4-wave workgroup
constexpr int64_t MAX_K = (1ll << 31) - 1;

// (key, j) candidates: a beats b iff its key is larger, or equal with the lower index
__device__ __forceinline__ bool beats(float ka, int ja, float kb, int jb) { return ka > kb || (ka == kb && ja < jb); }
__device__ __forceinline__ float key_of(float s) { return s == s ? s : -INFINITY; }

// a Q chunk spread over the 256 threads of the workgroup (clamped rows, never predicated) ...
__device__ __forceinline__ void coop_fetch(f32x4 (&v)[NPW], const float* __restrict__ Q, int base, int K, int D, Chunk ch,
                                           int tid) {
#pragma unroll
  for (int it = 0; it < NPW; ++it) {
    const int i = tid + 256 * it;
    const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
    v[it] = *reinterpret_cast<const f32x4*>(Q + (long long)tile_row(base, r, K) * D + ch.c0 + c4 * 4);
  }
}
// ... into the shared chunk buffer (between two workgroup barriers)
__device__ __forceinline__ void coop_store(const f32x4 (&v)[NPW], float* dst, Chunk ch, int tid) {
#pragma unroll
  for (int it = 0; it < NPW; ++it) {
    const int i = tid + 256 * it;
    const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
    if (i < 32 * ch.d4) *reinterpret_cast<f32x4*>(&dst[r * FP + c4 * 4]) = v[it];
  }
  if ((ch.d4 & 1) && tid < 32) *reinterpret_cast<float4*>(&dst[tid * FP + ch.d4 * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the lane's 16 rows of column j: running best per row
__device__ __forceinline__ void take_column(const f32x16& acc, int j, float (&bk)[16], int (&bj)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float key = key_of(acc[r]);
    if (beats(key, j, bk[r], bj[r])) { bk[r] = key; bj[r] = j; }
  }
}
// fold the 32 lanes (columns) of each wave half, then one pair per row of the tile to the split's partials
__device__ __forceinline__ void fold_and_write(float (&bk)[16], int (&bj)[16], int i0, int N, long long obase,
                                               float* __restrict__ pk, int* __restrict__ pj, int ll, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk[r], o, 64);
      const int oj = __shfl_xor(bj[r], o, 64);
      if (beats(ok, oj, bk[r], bj[r])) { bk[r] = ok; bj[r] = oj; }
    }
    const int i = i0 + acc_row(r, lh);
    if (ll == 0 && i < N) { pk[obase + i] = bk[r]; pj[obase + i] = bj[r]; }
  }
}

// grid (splits, groups of SRT virtual row tiles).  Virtual row tile vt in [0, 2 T): view vt / T, rows 32 (vt % T) ..
// Partials are indexed by (split * 2 + view) * N + i.
__global__ __launch_bounds__(256) void nnclr_search_fast_kernel(
    const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ Q, int N, int D, int K, int T,
    int ktiles, int tps, float* __restrict__ pk, int* __restrict__ pj, gca_magic md4a, gca_magic md4b) {
  __shared__ __attribute__((aligned(16))) float Zs[SRT][MAXCH * TILE];           // wave w's row tile, whole
  __shared__ __attribute__((aligned(16))) float Qs[TILE];                        // the streamed Q tile, one chunk at a time
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, vt = blockIdx.y * SRT + wave;
  const bool active = vt < 2 * T;                                                // wave-uniform
  const int view = vt >= T ? 1 : 0, i0 = (vt - view * T) * 32;
  const float* __restrict__ z = view ? z2 : z1;
  const int t0 = split * tps, t_end = t0 + tps < ktiles ? t0 + tps : ktiles;
  const int nch = (D + FD - 1) / FD;
  float* Zw = Zs[wave];

  f32x4 v[NPW];
  coop_fetch(v, Q, t0 * 32, K, D, chunk_of(0, nch, D, md4a, md4b), tid);         // in flight while the row tiles are staged
  if (active) {
    for (int e = lane; e < MAXCH * TILE / 4; e += 64) *reinterpret_cast<float4*>(&Zw[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    wave_lds_sync();
    for (int c = 0; c < nch; ++c) {
      const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
      for (int i = lane; i < 32 * ch.d4; i += 64) {
        const int r = (int)gca_fdiv((unsigned)i, ch.md4), c4 = i - r * ch.d4;
        *reinterpret_cast<float4*>(&Zw[c * TILE + r * FP + c4 * 4]) =
            *reinterpret_cast<const float4*>(z + (long long)tile_row(i0, r, N) * D + ch.c0 + c4 * 4);
      }
    }
  }
  for (int e = tid; e < TILE / 4; e += 256) *reinterpret_cast<float4*>(&Qs[e * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);

  float bk[16];
  int bj[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { bk[r] = -INFINITY; bj[r] = INT_MAX; }

  for (int t = t0; t < t_end; ++t) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int c = 0; c < nch; ++c) {
      const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
      __syncthreads();                                                           // every wave is done reading the previous piece
      coop_store(v, Qs, ch, tid);
      __syncthreads();
      int nc = c + 1, nt = t;                                                    // the next piece streams in behind the MFMAs
      if (nc == nch) { nc = 0; nt = t + 1; }
      if (nt >= t_end) { nc = c; nt = t; }
      coop_fetch(v, Q, nt * 32, K, D, chunk_of(nc, nch, D, md4a, md4b), tid);
      if (active) tile_mma(acc, Zw + c * TILE, Qs, (4 * ch.d4 + 7) >> 3, ll, lh);
    }
    const int j = t * 32 + ll;
    if (j < K) take_column(acc, j, bk, bj);
  }
  if (active) fold_and_write(bk, bj, i0, N, ((long long)split * 2 + view) * N, pk, pj, ll, lh);
}

// generic path: one wave, grid (splits, 2 T virtual row tiles)
__global__ __launch_bounds__(64) void nnclr_search_generic_kernel(
    const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ Q, int N, int D, int K, int T,
    int ktiles, int tps, float* __restrict__ pk, int* __restrict__ pj) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];
  __shared__ __attribute__((aligned(16))) float Qs[TILE];
  const int lane = threadIdx.x, lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, vt = blockIdx.y;
  const int view = vt >= T ? 1 : 0, i0 = (vt - view * T) * 32;
  const float* __restrict__ z = view ? z2 : z1;
  const int t0 = split * tps, t_end = t0 + tps < ktiles ? t0 + tps : ktiles;
  float bk[16];
  int bj[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { bk[r] = -INFINITY; bj[r] = INT_MAX; }
  for (int t = t0; t < t_end; ++t) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile_generic(acc, Zs, Qs, z, i0, N, Q, t * 32, K, D, lane);
    const int j = t * 32 + ll;
    if (j < K) take_column(acc, j, bk, bj);
  }
  fold_and_write(bk, bj, i0, N, ((long long)split * 2 + view) * N, pk, pj, ll, lh);
}

// One workgroup per R = view * N + i: the splits in split order, then idx, sim and the row of Q.
__global__ __launch_bounds__(64) void nnclr_pick_kernel(const float* __restrict__ pk, const int* __restrict__ pj,
                                                        const float* __restrict__ Q, int N, int D, int K, int splits,
                                                        int* __restrict__ idx, float* __restrict__ sim, float* __restrict__ nn1,
                                                        float* __restrict__ nn2) {
  const long long R = blockIdx.x, N2 = 2ll * N;
  float bk = pk[R];
  int bj = pj[R];
  for (int s = 1; s < splits; ++s) {
    const float k = pk[s * N2 + R];
    const int j = pj[s * N2 + R];
    if (beats(k, j, bk, bj)) { bk = k; bj = j; }
  }
  bj = bj < 0 ? 0 : (bj > K - 1 ? K - 1 : bj);                                   // the gather never leaves the queue
  if (threadIdx.x == 0) { idx[R] = bj; sim[R] = bk; }
  float* out = R < N ? nn1 + R * D : nn2 + (R - N) * D;
  const float* src = Q + (long long)bj * D;
  for (int e = threadIdx.x; e < D; e += 64) out[e] = src[e];
}

struct SearchPlan { bool fast; int waves, T, groups, ktiles, splits, tps; };

bool search_sizes_ok(int64_t N, int64_t D, int64_t K) {
  return sizes_ok(N, D) && K >= 1 && K <= MAX_K && K * D < (1ll << 31);
}
SearchPlan make_search_plan(int64_t N, int64_t D, int64_t K, bool aligned) {
  SearchPlan p;
  p.fast = D <= FAST_MAXD && D % 4 == 0 && aligned;
  p.waves = p.fast ? 4 : 1;
  p.T = (int)gca_ceil_div(N, 32);
  p.groups = p.fast ? (int)gca_ceil_div(2 * p.T, SRT) : 2 * p.T;
  p.ktiles = (int)gca_ceil_div(K, 32);
  int want = (int)gca_ceil_div(TARGET_WG, p.groups);
  want = want < 1 ? 1 : (want > p.ktiles ? p.ktiles : want);
  p.tps = (int)gca_ceil_div(p.ktiles, want);
  p.splits = (int)gca_ceil_div(p.ktiles, p.tps);
  return p;
}
int64_t search_ws_bytes(int64_t N, int splits) { return gca_round_up((int64_t)splits * 2 * N * 8, 16); }

}  // namespace

extern "C" {

int64_t gca_nnclr_search_ws_bytes(int64_t N, int64_t D, int64_t K) {
  if (!search_sizes_ok(N, D, K)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {                        // the caller's pointers are not known here
    const int64_t b = search_ws_bytes(N, make_search_plan(N, D, K, aligned != 0).splits);
    need = b > need ? b : need;
  }
  return need;
}

int gca_nnclr_search_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits) {
  if (!search_sizes_ok(N, D, K)) return GCA_EINVAL;
  const SearchPlan p = make_search_plan(N, D, K, aligned != 0);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_nnclr_search(const float* z1, const float* z2, const float* Q, int64_t N, int64_t D, int64_t K, int32_t* idx, float* sim,
                     float* nn1, float* nn2, void* ws, int64_t ws_bytes, void* stream) {
  if (!search_sizes_ok(N, D, K)) return GCA_EINVAL;
  if (!z1 || !z2 || !Q || !idx || !sim || !nn1 || !nn2 || !ws) return GCA_EINVAL;
  if (ws_bytes < gca_nnclr_search_ws_bytes(N, D, K)) return GCA_EINVAL;
  // nn is written by the second launch only, but a caller that aliases it to an input has made a mistake worth refusing
  const int64_t n = N * D;
  if (overlap(nn1, nn2, n) || overlap2(nn1, n, Q, K * D) || overlap2(nn2, n, Q, K * D)) return GCA_EINVAL;
  if (overlap(nn1, z1, n) || overlap(nn1, z2, n) || overlap(nn2, z1, n) || overlap(nn2, z2, n)) return GCA_EINVAL;
  const SearchPlan p = make_search_plan(N, D, K, aligned16(z1) && aligned16(z2) && aligned16(Q));
  hipStream_t st = (hipStream_t)stream;
  float* pk = reinterpret_cast<float*>(ws);
  int* pj = reinterpret_cast<int*>(pk + (int64_t)p.splits * 2 * N);
  const dim3 grid((unsigned)p.splits, (unsigned)p.groups);
  if (p.fast) {
    gca_magic ma, mb;
    last_chunk_magics(true, D, &ma, &mb);
    hipLaunchKernelGGL(nnclr_search_fast_kernel, grid, dim3(256), 0, st, z1, z2, Q, (int)N, (int)D, (int)K, p.T, p.ktiles, p.tps,
                       pk, pj, ma, mb);
  } else {
    hipLaunchKernelGGL(nnclr_search_generic_kernel, grid, dim3(64), 0, st, z1, z2, Q, (int)N, (int)D, (int)K, p.T, p.ktiles,
                       p.tps, pk, pj);
  }
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(nnclr_pick_kernel, dim3((unsigned)(2 * N)), dim3(64), 0, st, pk, pj, Q, (int)N, (int)D, (int)K, p.splits,
                     idx, sim, nn1, nn2);
  return gca_launch_status();
}

int64_t gca_nnclr_bwd_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {
    const int64_t b = xview_bwd_ws_bytes(N, D, make_plan(N, D, aligned != 0).splits);
    need = b > need ? b : need;
  }
  return need;
}

int gca_nnclr_bwd_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits) {
  if (!sizes_ok(N, D)) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned != 0);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_nnclr_bwd(const float* nn1, const float* nn2, const float* p1, const float* p2, const float* row_lse, int64_t N,
                  int64_t D, float inv_T, float w, const float* gscale_dev, float gscale_host, float* dp1, float* dp2, void* ws,
                  void* stream) {
  // direction 0 owns p2 and streams nn1 (-> dp2), direction 1 owns p1 and streams nn2 (-> dp1)
  return xview_bwd<true>(p2, p1, nn2, nn1, row_lse, N, D, inv_T, w, gscale_dev, gscale_host, dp2, dp1, ws, stream);
}

}  // extern "C"
