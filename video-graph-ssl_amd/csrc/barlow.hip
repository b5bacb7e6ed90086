// Barlow Twins' cross-correlation loss and its gradient on gfx950.  tests/barlow_ref.py is the numpy statement.
//
//   z1, z2 (N, D) fp32: the projector outputs of view 1 / view 2 of the same N clips
//   mean_v[d] = sum_n z_v[n,d] / N      var_v[d] = sum_n (z_v[n,d] - mean_v[d])^2 / N      rstd_v[d] = 1 / sqrt(var_v[d] + eps)
//   a = (z1 - mean_1) rstd_1            b = (z2 - mean_2) rstd_2                           (never stored)
//   C[i,j] = sum_n a[n,i] b[n,j] / N    on = sum_i (C[i,i] - 1)^2    off = sum_{i != j} C[i,j]^2    loss = on + lambda off
//   G[i,j] = 2 (C[i,i] - 1) on the diagonal, 2 lambda C[i,j] off it                        (never stored)
//   r1[i] = sum_j G[i,j] C[i,j]         r2[j] = sum_i G[i,j] C[i,j]
//   dz1[n,i] = g rstd_1[i] / N (sum_j G[i,j] b[n,j] - a[n,i] r1[i])        dz2[n,j] = g rstd_2[j] / N (sum_i G[i,j] a[n,i] - b[n,j] r2[j])
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).  A workgroup of 4 waves owns a 64 x 64
// output tile (2 x 2 waves of 32 x 32) and walks the reduction axis in chunks of 32, staged in LDS as [k][64] with the next
// chunk's global loads in flight behind the MFMAs of the current one.  Operands are standardised (a, b) or turned into G
// (from cmat) on their way into LDS.
//
//   forward   barlow_stats_kernel   (column tile of 64, view): lanes along D, the 4 waves take rows w, w + 4, ...; the mean
//                                   first, then the centred squares -- two passes, never E[x^2] - mean^2.
//             barlow_corr_kernel    (64 x 64 tile of C): reduction over N; writes cmat and, per 32 x 32 wave tile, the
//                                   partials of on, off, r1 (row sums over the tile's columns), r2 (column sums) into `ws`.
//             barlow_fold_kernel    folds the partials in tile order: rsum, and (workgroup 0, fp64) loss / on / off.
//   backward  barlow_grad_kernel    (64 columns, 64 rows of N, view): (N x D) * (D x D) with G formed from cmat on load; the
//                                   epilogue subtracts the r term and applies g rstd / N.  One launch for both views.
//
// One owner per output element and fixed fold orders: no atomics, bitwise reproducible.  Nothing reads the host.  One dispatch
// path: every global access is a guarded 4-byte one with lanes along D, so no alignment or divisibility is assumed.
#include <cstdint>
#include "gca_common.h"
#include "mma_tile.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void barlow_stats_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int N, int D,
                                                           float eps, float* __restrict__ stats) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, v = blockIdx.y;
  const float* __restrict__ z = v ? z2 : z1;
  const bool ok = c < D;
  // eight running sums per thread: eight loads in flight, and sum chains of N / 32 terms at most (rounding at N = 65536)
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    int n = w;
    for (; n + 28 < N; n += 32)
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += z[(long long)(n + 4 * u) * D + c];
    for (; n < N; n += 4) s[0] += z[(long long)n * D + c];
  }
  red[w][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  const float mean = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)N;
  __syncthreads();
  float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    int n = w;
    for (; n + 28 < N; n += 32)
#pragma unroll
      for (int u = 0; u < 8; ++u) { const float d = z[(long long)(n + 4 * u) * D + c] - mean; q[u] += d * d; }
    for (; n < N; n += 4) { const float d = z[(long long)n * D + c] - mean; q[0] += d * d; }
  }
  red[w][lane] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
  __syncthreads();
  if (w == 0 && ok) {
    const float var = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)N;
    stats[(2 * v) * D + c] = mean;
    stats[(2 * v + 1) * D + c] = 1.0f / sqrtf(var + eps);
  }
}

// rows n0 + kk of one view, columns c0 + lane, standardised; zeros outside (N, D).  Thread: column `lane`, rows (tid >> 6) + 4 it.
// Loads are clamped into the tensor, never predicated, so all of a chunk's loads are in flight at once; the store masks.
__device__ __forceinline__ void corr_fetch(float (&v)[NPT], const float* __restrict__ z, int n0, int col, int N, int D, int wave) {
  const int c = col < D ? col : D - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int n = n0 + wave + 4 * it;
    v[it] = z[(long long)(n < N ? n : N - 1) * D + c];
  }
}
__device__ __forceinline__ void corr_store(const float (&v)[NPT], float* dst, int n0, int col, int N, int D, float mean, float rstd,
                                           int wave, int lane) {
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int kk = wave + 4 * it;
    dst[kk * TP + lane] = (n0 + kk < N && col < D) ? (v[it] - mean) * rstd : 0.f;
  }
}

__global__ __launch_bounds__(256) void barlow_corr_kernel(
    const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ stats, int N, int D, float lambda,
    int T32, float* __restrict__ cmat, float* __restrict__ r1p, float* __restrict__ r2p, float* __restrict__ onp,
    float* __restrict__ offp) {
  __shared__ float As[KC * TP];
  __shared__ float Bs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int i0 = blockIdx.y * TW, j0 = blockIdx.x * TW;
  const int ci = i0 + lane, cj = j0 + lane;                      // the columns of z1 / z2 this thread stages
  const float m1 = ci < D ? stats[ci] : 0.f, s1 = ci < D ? stats[D + ci] : 0.f;
  const float m2 = cj < D ? stats[2 * D + cj] : 0.f, s2 = cj < D ? stats[3 * D + cj] : 0.f;
  const int ti = (i0 >> 5) + wr, tj = (j0 >> 5) + wc;            // this wave's 32 x 32 tile of C
  const bool live = ti < T32 && tj < T32;

  f32x16 acc, tot;                                               // tot takes acc every FLUSH rows: short fp32 chains at large N
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
  float va[NPT], vb[NPT];
  corr_fetch(va, z1, 0, ci, N, D, wave);
  corr_fetch(vb, z2, 0, cj, N, D, wave);
  for (int n0 = 0; n0 < N; n0 += KC) {
    if (n0 > 0 && n0 % FLUSH == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
    }
    corr_store(va, As, n0, ci, N, D, m1, s1, wave, lane);
    corr_store(vb, Bs, n0, cj, N, D, m2, s2, wave, lane);
    __syncthreads();
    if (n0 + KC < N) {                                           // the next chunk streams in behind the MFMAs
      corr_fetch(va, z1, n0 + KC, ci, N, D, wave);
      corr_fetch(vb, z2, n0 + KC, cj, N, D, wave);
    }
    if (live) chunk_mma(acc, As, Bs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  if (!live) return;

  // ---- epilogue: C, and this tile's share of on / off / r1 / r2
  const int j = j0 + wc * 32 + ll;
  float on = 0.f, off = 0.f, colsum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + wr * 32 + acc_row(r, lh);
    const bool ok = i < D && j < D;
    const float c = (tot[r] + acc[r]) / (float)N;
    float gc = 0.f;
    if (ok) {
      cmat[i * D + j] = c;
      if (i == j) { const float t = c - 1.f; on += t * t; gc = 2.f * t * c; }
      else { off += c * c; gc = 2.f * lambda * c * c; }
    }
    colsum += gc;
    const float rowsum = half_sum(gc);
    if (ll == 0 && i < D) r1p[tj * D + i] = rowsum;
  }
  colsum += __shfl_xor(colsum, 32, 64);
  if (lh == 0 && j < D) r2p[ti * D + j] = colsum;
  on = gca_wave_sum(on);
  off = gca_wave_sum(off);
  if (lane == 0) { onp[ti * T32 + tj] = on; offp[ti * T32 + tj] = off; }
}

__global__ __launch_bounds__(256) void barlow_fold_kernel(const float* __restrict__ r1p, const float* __restrict__ r2p,
                                                          const float* __restrict__ onp, const float* __restrict__ offp, int D,
                                                          int T32, float lambda, float* __restrict__ rsum,
                                                          float* __restrict__ loss) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < 2 * D) {
    const float* __restrict__ p = e < D ? r1p + e : r2p + (e - D);
    float s = p[0];
    for (int t = 1; t < T32; ++t) s += p[t * D];
    rsum[e] = s;
  }
  if (blockIdx.x == 0) {
    __shared__ double sh[8];
    double on = 0.0, off = 0.0;
    for (int t = threadIdx.x; t < T32 * T32; t += 256) { on += (double)onp[t]; off += (double)offp[t]; }
    on = gca_block_sum256_d(on, sh);
    off = gca_block_sum256_d(off, sh + 4);
    if (threadIdx.x == 0) {
      loss[0] = (float)(on + (double)lambda * off);
      loss[1] = (float)on;
      loss[2] = (float)off;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// X chunk: rows n0 + c of the OTHER view, columns k0 + kk, standardised -> Xs[kk][c].  Thread: kk = tid & 31, c = (tid >> 5) + 8 it.
// (Clamped loads, as corr_fetch; the store into LDS masks.)
__device__ __forceinline__ void grad_fetch_x(float (&v)[NPT], const float* __restrict__ zo, int n0, int k, int N, int D, int tid) {
  const int kc = k < D ? k : D - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int n = n0 + (tid >> 5) + 8 * it;
    v[it] = zo[(long long)(n < N ? n : N - 1) * D + kc];
  }
}
// G chunk -> Gs[kk][c] for output columns c0 + c.  view 1 (dz2, columns j, k = i): rows of cmat are k, lanes along the columns.
// view 0 (dz1, columns i, k = j): rows of cmat are the columns, lanes along k (read transposed).
// The fetch only loads (clamped); G is formed branch-free when the chunk goes into LDS, so the loads stay back to back.
__device__ __forceinline__ void grad_ij(int& i, int& j, int view, int c0, int k0, int tid, int it) {
  if (view) { i = k0 + (tid >> 6) + 4 * it; j = c0 + (tid & 63); }
  else { i = c0 + (tid >> 5) + 8 * it; j = k0 + (tid & 31); }
}
__device__ __forceinline__ void grad_fetch_c(float (&v)[NPT], const float* __restrict__ cmat, int view, int c0, int k0, int D,
                                             int tid) {
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    int i, j;
    grad_ij(i, j, view, c0, k0, tid, it);
    v[it] = cmat[(i < D ? i : D - 1) * D + (j < D ? j : D - 1)];
  }
}
__device__ __forceinline__ float grad_g(float c, int i, int j, int D, float lambda) {
  const bool diag = i == j;
  const float g = (diag ? 2.f : 2.f * lambda) * (c - (diag ? 1.f : 0.f));
  return (i < D && j < D) ? g : 0.f;
}

__global__ __launch_bounds__(256) void barlow_grad_kernel(
    const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ stats, const float* __restrict__ cmat,
    const float* __restrict__ rsum, int N, int D, float lambda, const float* __restrict__ gscale_dev, float gscale_host,
    float* __restrict__ dz1, float* __restrict__ dz2) {
  __shared__ float Xs[KC * TP];
  __shared__ float Gs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int view = blockIdx.z, c0 = blockIdx.x * TW, n0 = blockIdx.y * TW;
  const float* __restrict__ zs = view ? z2 : z1;                  // own view
  const float* __restrict__ zo = view ? z1 : z2;                  // the other one: the operand of the product
  const float* __restrict__ st_s = stats + (view ? 2 * D : 0);
  const float* __restrict__ st_o = stats + (view ? 0 : 2 * D);
  float* __restrict__ dz = view ? dz2 : dz1;
  const bool live = n0 + wr * 32 < N && c0 + wc * 32 < D;
  const int kk = tid & 31;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float vx[NPT], vg[NPT];
  grad_fetch_x(vx, zo, n0, kk, N, D, tid);
  grad_fetch_c(vg, cmat, view, c0, 0, D, tid);
  float mo = st_o[kk < D ? kk : D - 1], ro = st_o[D + (kk < D ? kk : D - 1)];
  for (int k0 = 0; k0 < D; k0 += KC) {
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
      const int c = (tid >> 5) + 8 * it;
      int i, j;
      grad_ij(i, j, view, c0, k0, tid, it);
      Xs[kk * TP + c] = (n0 + c < N && k0 + kk < D) ? (vx[it] - mo) * ro : 0.f;
      Gs[(view ? (tid >> 6) + 4 * it : kk) * TP + (view ? (tid & 63) : c)] = grad_g(vg[it], i, j, D, lambda);
    }
    __syncthreads();
    if (k0 + KC < D) {                                            // the next chunk streams in behind the MFMAs
      const int k = k0 + KC + kk, kc = k < D ? k : D - 1;
      grad_fetch_x(vx, zo, n0, k, N, D, tid);
      grad_fetch_c(vg, cmat, view, c0, k0 + KC, D, tid);
      mo = st_o[kc];
      ro = st_o[D + kc];
    }
    if (live) chunk_mma(acc, Xs, Gs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int c = c0 + wc * 32 + ll;
  if (!live || c >= D) return;
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  const float ms = st_s[c], rs = st_s[D + c], rc = rsum[view * D + c];
  const float scale = g * rs / (float)N;
  float own[16];                                                  // clamped loads first, all in flight; only the store is guarded
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    own[r] = zs[(long long)(n < N ? n : N - 1) * D + c];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    const float val = scale * (acc[r] - (own[r] - ms) * rs * rc);
    if (n < N) dz[(long long)n * D + c] = val;
  }
}

bool sizes_ok(int64_t N, int64_t D) { return N >= 2 && N <= 65536 && D >= 1 && D <= 8192 && N * D < (1ll << 31); }
bool scalar_ok(float v) { return v >= 0.f && !isinf(v); }        // (false for NaN)

}  // namespace

extern "C" {

int64_t gca_barlow_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  const int64_t T32 = gca_ceil_div(D, 32);
  return (2 * T32 * D + 2 * T32 * T32) * 4;
}

int gca_barlow_fwd(const float* z1, const float* z2, int64_t N, int64_t D, float lambda, float eps, float* stats, float* cmat,
                   float* rsum, float* loss, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(lambda) || !scalar_ok(eps)) return GCA_EINVAL;
  if (!z1 || !z2 || !stats || !cmat || !rsum || !loss || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int T32 = (int)gca_ceil_div(D, 32), T64 = (int)gca_ceil_div(D, TW);
  float* r1p = reinterpret_cast<float*>(ws);
  float* r2p = r1p + (int64_t)T32 * D;
  float* onp = r2p + (int64_t)T32 * D;
  float* offp = onp + (int64_t)T32 * T32;
  hipLaunchKernelGGL(barlow_stats_kernel, dim3((unsigned)T64, 2), dim3(256), 0, st, z1, z2, (int)N, (int)D, eps, stats);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(barlow_corr_kernel, dim3((unsigned)T64, (unsigned)T64), dim3(256), 0, st, z1, z2, stats, (int)N, (int)D,
                     lambda, T32, cmat, r1p, r2p, onp, offp);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(barlow_fold_kernel, dim3((unsigned)gca_ceil_div(2 * D, 256)), dim3(256), 0, st, r1p, r2p, onp, offp, (int)D,
                     T32, lambda, rsum, loss);
  return gca_launch_status();
}

int gca_barlow_bwd(const float* z1, const float* z2, const float* stats, const float* cmat, const float* rsum, int64_t N, int64_t D,
                   float lambda, const float* gscale_dev, float gscale_host, float* dz1, float* dz2, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(lambda) || isnan(gscale_host) || isinf(gscale_host)) return GCA_EINVAL;
  if (!z1 || !z2 || !stats || !cmat || !rsum || !dz1 || !dz2 || !ws) return GCA_EINVAL;
  hipLaunchKernelGGL(barlow_grad_kernel, dim3((unsigned)gca_ceil_div(D, TW), (unsigned)gca_ceil_div(N, TW), 2), dim3(256), 0,
                     (hipStream_t)stream, z1, z2, stats, cmat, rsum, (int)N, (int)D, lambda, gscale_dev, gscale_host, dz1, dz2);
  return gca_launch_status();
}

}  // extern "C"
