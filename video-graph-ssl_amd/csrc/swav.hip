// SwAV's swapped-prediction loss (Sinkhorn-Knopp codes, softmax cross-entropy) and its gradient on gfx950.  tests/swav_ref.py is
// the numpy statement.
//
//   z1, z2 (N, D) fp32 with unit rows: the projection-head outputs of view 1 / view 2 of the same N clips; C (K, D) fp32 with unit
//   rows: the prototypes.  Per view v:  S_v = z_v C^T (N, K)      P_v = exp((S_v - 1) / eps)   (1 bounds S for unit rows; the codes do
//   not depend on the constant)
//   u_v[k] = 1 / (K sum_n P_v[n,k] v_v[n])      v_v[n] = 1 / (N sum_k P_v[n,k] u_v[k])      `iters` times, v_v = 1 before the first
//   q_v[n,k] = N P_v[n,k] u_v[k] v_v[n]         (rows sum to 1; no gradient flows through q)
//   lse_v[n] = log sum_k exp(S_v[n,k] / T)      l12 = -sum_{n,k} q_2 (S_1 / T - lse_1) / N      l21 likewise with 1 <-> 2
//   loss = (l12 + l21) / 2                      dS_1 = (exp(S_1 / T - lse_1) - q_2) / (2 N T)   dS_2 likewise
//   dz_v = g dS_v C                             dC (+)= g (dS_1^T z_1 + dS_2^T z_2)
//
// The Sinkhorn iteration is carried as the two scaling vectors u (K) and v (N) over the fixed matrix P, which is recomputed from
// the stored scores in every pass and never written.  Each pass has a global dependency (sums over N, then over K), so the passes
// are separate launches with both views in one grid; the last row pass is fused with the loss and gradient sweep.
//
//   forward   swav_scores_kernel   (64 prototypes, 64 rows of N, view): S on the tile of mma_tile.h, reduction along D, both
//                                  operands row-major along it (staged as barlow.hip's backward stages its X operand).
//             swav_col_kernel      (64 prototypes, view): u.  Lanes along K, the 4 waves take rows w, w + 4, ...
//             swav_row_kernel      (4 rows of N, view): v.  One wave per row, lanes along K.
//             swav_codes_kernel    (4 rows of N): one wave per row and both views: the last row sum, the row log-sum-exp of S / T
//                                  (one online pass), then q, the row's two loss terms and dS, which overwrites S in place.
//             swav_fold_kernel     folds the 2 N row terms in row order in fp64: loss, l12, l21.
//   backward  swav_dz_kernel       (64 columns of D, 64 rows of N, view x slab of K): dS_v C, reduction along K.  A small batch leaves
//                                  this grid a handful of workgroups that each walk all of K, so K is cut into up to 32 slabs
//                                  (dz_splits); swav_dz_fold_kernel then adds the slabs' partial tiles in slab order.
//             swav_dc_kernel       (64 columns of D, 64 prototypes): reduction over the 2 N rows, view 1 first.
//   and       rows_normalize_kernel (4 rows): one wave per row of C, C[k,:] /= ||C[k,:]||, an all-zero row left as it is.
//
// One owner per output element and fixed fold orders: no atomics, bitwise reproducible.  Nothing reads the host.  One dispatch
// path: every global access is a guarded 4-byte one, so no alignment or divisibility is assumed; element offsets are 64-bit
// (N K reaches 2^29 per view).
#include <cstdint>
#include "gca_common.h"
#include "mma_tile.h"
#include "mma_stage.h"                                             // xfetch / xstore / rfetch / rstore, shared with dino.hip
#include <math.h>

namespace {

__device__ __forceinline__ float fold4(const float (&s)[4]) { return (s[0] + s[1]) + (s[2] + s[3]); }

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void swav_scores_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                          const float* __restrict__ C, int N, int D, int K, float* __restrict__ S) {
  __shared__ float Zs[KC * TP];
  __shared__ float Cs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int view = blockIdx.z, p0 = blockIdx.x * TW, n0 = blockIdx.y * TW;
  const float* __restrict__ z = view ? z2 : z1;
  const bool live = n0 + wr * 32 < N && p0 + wc * 32 < K;
  const int kk = tid & 31;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float vz[NPT], vc[NPT];
  xfetch(vz, z, n0, kk, N, D, tid);
  xfetch(vc, C, p0, kk, K, D, tid);
  for (int d0 = 0; d0 < D; d0 += KC) {
    xstore(vz, Zs, n0, d0 + kk, N, D, tid);
    xstore(vc, Cs, p0, d0 + kk, K, D, tid);
    __syncthreads();
    if (d0 + KC < D) {                                             // the next chunk streams in behind the MFMAs
      xfetch(vz, z, n0, d0 + KC + kk, N, D, tid);
      xfetch(vc, C, p0, d0 + KC + kk, K, D, tid);
    }
    if (live) chunk_mma(acc, Zs, Cs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int p = p0 + wc * 32 + ll;
  if (!live || p >= K) return;
  float* __restrict__ Sv = S + (size_t)view * N * K;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    if (n < N) Sv[(size_t)n * K + p] = acc[r];
  }
}

__device__ __forceinline__ float shifted_exp(float s, float inv_eps) { return expf((s - 1.f) * inv_eps); }

// u[view][k] = 1 / (K sum_n P[n,k] v[view][n]);  vv == nullptr: the first pass, v = 1
__global__ __launch_bounds__(256) void swav_col_kernel(const float* __restrict__ S, const float* __restrict__ vv, int N, int K,
                                                       float inv_eps, float* __restrict__ u) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane, view = blockIdx.y;
  const float* __restrict__ Sv = S + (size_t)view * N * K;
  const float* __restrict__ vr = vv ? vv + view * N : nullptr;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (k < K) {
    int n = w;
    for (; n + 12 < N; n += 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int nn = n + 4 * j;
        s[j] += shifted_exp(Sv[(size_t)nn * K + k], inv_eps) * (vr ? vr[nn] : 1.f);
      }
    for (; n < N; n += 4) s[0] += shifted_exp(Sv[(size_t)n * K + k], inv_eps) * (vr ? vr[n] : 1.f);
  }
  red[w][lane] = fold4(s);
  __syncthreads();
  if (w == 0 && k < K) u[view * K + k] = 1.f / ((float)K * (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]));
}

// sum_k P[n,k] u[k] of one row, by one wave; valid in every lane
__device__ __forceinline__ float row_sum(const float* __restrict__ row, const float* __restrict__ u, int K, float inv_eps, int lane) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int k = lane;
  for (; k + 192 < K; k += 256)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += shifted_exp(row[k + 64 * j], inv_eps) * u[k + 64 * j];
  for (; k < K; k += 64) s[0] += shifted_exp(row[k], inv_eps) * u[k];
  return gca_wave_sum(fold4(s));
}

// v[view][n] = 1 / (N sum_k P[n,k] u[view][k])
__global__ __launch_bounds__(256) void swav_row_kernel(const float* __restrict__ S, const float* __restrict__ u, int N, int K,
                                                       float inv_eps, float* __restrict__ v) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), view = blockIdx.y;
  if (n >= N) return;
  const float t = row_sum(S + ((size_t)view * N + n) * K, u + view * K, K, inv_eps, lane);
  if (lane == 0) v[view * N + n] = 1.f / ((float)N * t);
}

// log sum_k exp(row[k] / T) of one row, by one wave, in one online pass; valid in every lane
__device__ __forceinline__ float row_lse(const float* __restrict__ row, int K, float inv_T, int lane) {
  float m = -INFINITY, s = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float x = row[k] * inv_T;
    if (x > m) { s = s * expf(m - x) + 1.f; m = x; }
    else s += expf(x - m);
  }
  const float M = gca_wave_max(m);                                  // (a lane without elements holds m = -inf, s = 0)
  s = gca_wave_sum(s * expf(m - M));
  return M + logf(s);
}

// Rows n of both views: the last row pass of the iteration, then q, the loss terms and dS over S.  codes: (2, N, K) or nullptr.
__global__ __launch_bounds__(256) void swav_codes_kernel(float* __restrict__ S, const float* __restrict__ u, int N, int K,
                                                         float inv_eps, float inv_T, float cgrad, float* __restrict__ rowp,
                                                         float* __restrict__ codes) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float* __restrict__ r1 = S + (size_t)n * K;
  float* __restrict__ r2 = S + ((size_t)N + n) * K;
  const float* __restrict__ u1 = u;
  const float* __restrict__ u2 = u + K;
  const float i1 = 1.f / row_sum(r1, u1, K, inv_eps, lane), i2 = 1.f / row_sum(r2, u2, K, inv_eps, lane);
  const float lse1 = row_lse(r1, K, inv_T, lane), lse2 = row_lse(r2, K, inv_T, lane);
  float t12 = 0.f, t21 = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float s1 = r1[k], s2 = r2[k];
    const float q1 = shifted_exp(s1, inv_eps) * u1[k] * i1, q2 = shifted_exp(s2, inv_eps) * u2[k] * i2;
    const float ls1 = s1 * inv_T - lse1, ls2 = s2 * inv_T - lse2;
    t12 += q2 * ls1;
    t21 += q1 * ls2;
    r1[k] = (expf(ls1) - q2) * cgrad;
    r2[k] = (expf(ls2) - q1) * cgrad;
    if (codes) {
      codes[(size_t)n * K + k] = q1;
      codes[((size_t)N + n) * K + k] = q2;
    }
  }
  t12 = gca_wave_sum(t12);
  t21 = gca_wave_sum(t21);
  if (lane == 0) { rowp[n] = -t12; rowp[N + n] = -t21; }
}

__global__ __launch_bounds__(256) void swav_fold_kernel(const float* __restrict__ rowp, int N, float* __restrict__ parts) {
  __shared__ double sh[8];
  double a = 0.0, b = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) { a += (double)rowp[n]; b += (double)rowp[N + n]; }
  a = gca_block_sum256_d(a, sh);
  b = gca_block_sum256_d(b, sh + 4);
  if (threadIdx.x == 0) {
    const double l12 = a / (double)N, l21 = b / (double)N;
    parts[0] = (float)(0.5 * (l12 + l21));
    parts[1] = (float)l12;
    parts[2] = (float)l21;
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// The reduction over K runs in `splits` slabs of `slab` prototypes (blockIdx.z = view + 2 slab index): one slab writes g x its sum
// into dz, several leave their unscaled sums in `part` (splits, 2, N, D) for swav_dz_fold_kernel.
__global__ __launch_bounds__(256) void swav_dz_kernel(const float* __restrict__ dS, const float* __restrict__ C, int N, int D, int K,
                                                      int slab, int splits, const float* __restrict__ gscale_dev, float gscale_host,
                                                      float* __restrict__ dz1, float* __restrict__ dz2, float* __restrict__ part) {
  __shared__ float Gs[KC * TP];
  __shared__ float Cs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int view = blockIdx.z & 1, sl = blockIdx.z >> 1, c0 = blockIdx.x * TW, n0 = blockIdx.y * TW;
  const int kb = sl * slab, ke = kb + slab < K ? kb + slab : K;    // (a slab past the end of K sums nothing)
  const float* __restrict__ G = dS + (size_t)view * N * K;
  const bool live = n0 + wr * 32 < N && c0 + wc * 32 < D;
  const int kk = tid & 31;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float vg[NPT], vc[NPT];
  xfetch(vg, G, n0, kb + kk, N, K, tid);
  rfetch(vc, C, kb, c0 + lane, K, D, wave);
  for (int k0 = kb; k0 < ke; k0 += KC) {
    xstore(vg, Gs, n0, k0 + kk, N, ke, tid);
    rstore(vc, Cs, k0, c0 + lane, ke, D, wave, lane);
    __syncthreads();
    if (k0 + KC < ke) {                                            // the next chunk streams in behind the MFMAs
      xfetch(vg, G, n0, k0 + KC + kk, N, K, tid);
      rfetch(vc, C, k0 + KC, c0 + lane, K, D, wave);
    }
    if (live) chunk_mma(acc, Gs, Cs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int c = c0 + wc * 32 + ll;
  if (!live || c >= D) return;
  const float g = splits == 1 ? gscale_host * (gscale_dev ? *gscale_dev : 1.f) : 1.f;
  float* __restrict__ out = splits == 1 ? (view ? dz2 : dz1) : part + ((size_t)sl * 2 + view) * N * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    if (n < N) out[(size_t)n * D + c] = g * acc[r];
  }
}

// dz_v[e] = g (part[0][v][e] + part[1][v][e] + ...), slab after slab
__global__ __launch_bounds__(256) void swav_dz_fold_kernel(const float* __restrict__ part, int splits, int ND,
                                                           const float* __restrict__ gscale_dev, float gscale_host,
                                                           float* __restrict__ dz1, float* __restrict__ dz2) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * ND) return;
  float s = part[e];
  for (int t = 1; t < splits; ++t) s += part[(size_t)t * 2 * ND + e];
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  if (e < ND) dz1[e] = g * s;
  else dz2[e - ND] = g * s;
}

__global__ __launch_bounds__(256) void swav_dc_kernel(const float* __restrict__ dS, const float* __restrict__ z1,
                                                      const float* __restrict__ z2, int N, int D, int K,
                                                      const float* __restrict__ gscale_dev, float gscale_host, int accumulate,
                                                      float* __restrict__ dC) {
  __shared__ float Gs[KC * TP];
  __shared__ float Zs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int c0 = blockIdx.x * TW, p0 = blockIdx.y * TW;
  const bool live = p0 + wr * 32 < K && c0 + wc * 32 < D;
  const int nch = (N + KC - 1) / KC;                               // chunks per view; chunk j: view j / nch, rows (j % nch) KC ...

  f32x16 acc, tot;                                                 // tot takes acc every FLUSH rows: short fp32 chains at large N
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
  float vg[NPT], vz[NPT];
  rfetch(vg, dS, 0, p0 + lane, N, K, wave);
  rfetch(vz, z1, 0, c0 + lane, N, D, wave);
  for (int j = 0; j < 2 * nch; ++j) {
    const int n0 = (j < nch ? j : j - nch) * KC;
    if (j > 0 && (j * KC) % FLUSH == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
    }
    rstore(vg, Gs, n0, p0 + lane, N, K, wave, lane);
    rstore(vz, Zs, n0, c0 + lane, N, D, wave, lane);
    __syncthreads();
    if (j + 1 < 2 * nch) {                                         // the next chunk streams in behind the MFMAs
      const int jn = j + 1, second = jn >= nch;
      const int nn = (second ? jn - nch : jn) * KC;
      rfetch(vg, dS + (second ? (size_t)N * K : 0), nn, p0 + lane, N, K, wave);
      rfetch(vz, second ? z2 : z1, nn, c0 + lane, N, D, wave);
    }
    if (live) chunk_mma(acc, Gs, Zs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int c = c0 + wc * 32 + ll;
  if (!live || c >= D) return;
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int p = p0 + wr * 32 + acc_row(r, lh);
    if (p < K) {
      const float val = g * (tot[r] + acc[r]);
      float* __restrict__ o = dC + (size_t)p * D + c;
      *o = accumulate ? *o + val : val;
    }
  }
}

// ------------------------------------------------------------------------------------------------- prototype rows
__global__ __launch_bounds__(256) void rows_normalize_kernel(float* __restrict__ C, int K, int D) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  float* __restrict__ row = C + (size_t)k * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += row[d] * row[d];
  s = gca_wave_sum(s);
  if (!(s > 0.f)) return;                                          // an all-zero row stays as it is
  const float nrm = sqrtf(s);
  for (int d = lane; d < D; d += 64) row[d] = row[d] / nrm;
}

bool sizes_ok(int64_t N, int64_t D, int64_t K) { return N >= 2 && N <= 8192 && K >= 2 && K <= 65536 && D >= 1 && D <= 8192; }
// eps in [0.025, 1]: exp(-2 / eps) stays a normal fp32 number.  T positive with 1 / T finite in fp32.  (false for NaN)
bool params_ok(float eps, float T, int64_t iters) {
  return eps >= 0.025f && eps <= 1.f && T > 0.f && !isinf(T) && !isinf(1.f / T) && iters >= 1 && iters <= 16;
}

// Slabs of the reduction over K in swav_dz_kernel: as many as bring its grid to 256 workgroups, at most 32, and none shorter than
// 256 prototypes.  tests/swav_ref.py: dz_splits.
int dz_splits(int64_t N, int64_t D, int64_t K) {
  const int64_t tiles = 2 * gca_ceil_div(N, TW) * gca_ceil_div(D, TW);
  int64_t s = 256 / tiles;
  s = s < 1 ? 1 : (s > 32 ? 32 : s);
  const int64_t by_k = gca_ceil_div(K, 256);
  return (int)(s < by_k ? s : by_k);
}

}  // namespace

extern "C" {

int gca_rows_normalize(float* C, int64_t K, int64_t D, void* stream) {
  if (!C || K < 1 || K > 65536 || D < 1 || D > 8192) return GCA_EINVAL;
  hipLaunchKernelGGL(rows_normalize_kernel, dim3((unsigned)gca_ceil_div(K, 4)), dim3(256), 0, (hipStream_t)stream, C, (int)K, (int)D);
  return gca_launch_status();
}

int64_t gca_swav_ws_bytes(int64_t N, int64_t D, int64_t K) {
  if (!sizes_ok(N, D, K)) return -1;
  const int64_t fwd = (2 * K + 4 * N) * 4;                         // u (2, K), v (2, N), the row terms (2, N)
  const int64_t splits = dz_splits(N, D, K);
  const int64_t bwd = splits > 1 ? splits * 2 * N * D * 4 : 0;     // the slabs' partial dz
  return fwd > bwd ? fwd : bwd;
}

int gca_swav_dz_splits(int64_t N, int64_t D, int64_t K) { return sizes_ok(N, D, K) ? dz_splits(N, D, K) : -1; }

int gca_swav_fwd(const float* z1, const float* z2, const float* C, int64_t N, int64_t D, int64_t K, float eps, float T, int64_t iters,
                 float* parts, float* dS, float* codes, void* ws, void* stream) {
  if (!sizes_ok(N, D, K) || !params_ok(eps, T, iters)) return GCA_EINVAL;
  if (!z1 || !z2 || !C || !parts || !dS || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* u = reinterpret_cast<float*>(ws);
  float* v = u + 2 * K;
  float* rowp = v + 2 * N;
  const float inv_eps = (float)(1.0 / (double)eps), inv_T = (float)(1.0 / (double)T);
  const float cgrad = (float)(1.0 / (2.0 * (double)N * (double)T));
  const unsigned TK = (unsigned)gca_ceil_div(K, TW), TN = (unsigned)gca_ceil_div(N, TW), RN = (unsigned)gca_ceil_div(N, 4);
  hipLaunchKernelGGL(swav_scores_kernel, dim3(TK, TN, 2), dim3(256), 0, st, z1, z2, C, (int)N, (int)D, (int)K, dS);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  for (int64_t it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(swav_col_kernel, dim3(TK, 2), dim3(256), 0, st, (const float*)dS, (const float*)(it ? v : nullptr), (int)N,
                       (int)K, inv_eps, u);
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
    if (it + 1 == iters) break;                                    // the last row pass belongs to swav_codes_kernel
    hipLaunchKernelGGL(swav_row_kernel, dim3(RN, 2), dim3(256), 0, st, (const float*)dS, (const float*)u, (int)N, (int)K, inv_eps, v);
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  }
  hipLaunchKernelGGL(swav_codes_kernel, dim3(RN), dim3(256), 0, st, dS, (const float*)u, (int)N, (int)K, inv_eps, inv_T, cgrad, rowp,
                     codes);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(swav_fold_kernel, dim3(1), dim3(256), 0, st, (const float*)rowp, (int)N, parts);
  return gca_launch_status();
}

int gca_swav_bwd(const float* z1, const float* z2, const float* C, const float* dS, int64_t N, int64_t D, int64_t K,
                 const float* gscale_dev, float gscale_host, float* dz1, float* dz2, float* dC, int accumulate_dC, void* ws,
                 void* stream) {
  if (!sizes_ok(N, D, K) || isnan(gscale_host) || isinf(gscale_host)) return GCA_EINVAL;
  if (!z1 || !z2 || !C || !dS || !dz1 || !dz2 || !dC || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned TD = (unsigned)gca_ceil_div(D, TW);
  const int splits = dz_splits(N, D, K);
  const int slab = (int)gca_round_up(gca_ceil_div(K, splits), KC);
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(swav_dz_kernel, dim3(TD, (unsigned)gca_ceil_div(N, TW), 2u * splits), dim3(256), 0, st, dS, C, (int)N, (int)D,
                     (int)K, slab, splits, gscale_dev, gscale_host, dz1, dz2, part);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  if (splits > 1) {
    hipLaunchKernelGGL(swav_dz_fold_kernel, dim3((unsigned)gca_ceil_div(2 * N * D, 256)), dim3(256), 0, st, (const float*)part, splits,
                       (int)(N * D), gscale_dev, gscale_host, dz1, dz2);
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  }
  hipLaunchKernelGGL(swav_dc_kernel, dim3(TD, (unsigned)gca_ceil_div(K, TW)), dim3(256), 0, st, dS, z1, z2, (int)N, (int)D, (int)K,
                     gscale_dev, gscale_host, accumulate_dC ? 1 : 0, dC);
  return gca_launch_status();
}

}  // extern "C"
