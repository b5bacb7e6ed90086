// VICReg's variance / invariance / covariance loss and its gradient on gfx950.  tests/vicreg_ref.py is the numpy statement.
//
//   z1, z2 (N, D) fp32: the projector outputs of view 1 / view 2 of the same N clips; per view v, x = z_v:
//   mean_v[d] = sum_n x[n,d] / N        xc = x - mean_v        var_v[d] = sum_n xc[n,d]^2 / (N - 1)      sd_v[d] = sqrt(var_v[d] + eps)
//   Cov_v[i,j] = sum_n xc[n,i] xc[n,j] / (N - 1)
//   inv  = sum_{n,d} (z1 - z2)^2 / (N D)      varl = sum_v sum_d max(0, 1 - sd_v[d]) / (2 D)      covl = sum_v sum_{i != j} Cov_v[i,j]^2 / D
//   loss = sim inv + std varl + cov covl
//   dz_v[n,j] = g (s_v 2 sim (z1 - z2)[n,j] / (N D) - std [sd_v[j] < 1] xc[n,j] / (2 D sd_v[j] (N - 1))
//                  + 4 cov / (D (N - 1)) sum_{i != j} xc[n,i] Cov_v[i,j]),                          s_1 = +1, s_2 = -1
// (the centring adds no term: the columns of xc sum to zero, so both gradients through it already have zero column means).
//
// The products run on the tile of mma_tile.h (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation; 64 x 64 per
// workgroup, chunks of 32 in LDS, the next chunk's global loads in flight behind the MFMAs).  Operands are centred (xc) or
// have their diagonal zeroed (covm) on their way into LDS.
//
//   forward   vicreg_stats_kernel   (column tile of 64; view 1, view 2, or the difference): lanes along D, the 4 waves take rows
//                                   w, w + 4, ...; the mean first, then the centred squares -- two passes, never E[x^2] - mean^2;
//                                   writes mean, sd and the tile's hinge sum.  The third slice sums (z1 - z2)^2 over its columns.
//             vicreg_cov_kernel     (64 x 64 tile of Cov_v with tj >= ti, view): Cov is symmetric, so only the upper triangle of
//                                   tiles is launched; an off-diagonal tile writes itself and its transpose into covm and its
//                                   square-sum counts twice.  The diagonal is written but left out of the square-sum.
//             vicreg_fold_kernel    folds the partials in tile order in fp64: loss, inv, varl, covl.
//   backward  vicreg_grad_kernel    (64 columns, 64 rows of N, view): (N x D) * (D x D), xc formed on load, covm[v] with its
//                                   diagonal zeroed on load; the epilogue adds the hinge and invariance terms and applies g.
//
// One owner per output element and fixed fold orders: no atomics, bitwise reproducible.  Nothing reads the host.  One dispatch
// path: every global access is a guarded 4-byte one with lanes along D (but the mirrored store of an off-diagonal Cov tile,
// whose lanes run down a column), so no alignment or divisibility is assumed.
#include <cstdint>
#include "gca_common.h"
#include "mma_tile.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------ forward
// eight running sums per thread: eight loads in flight, and sum chains of N / 32 terms at most
__device__ __forceinline__ float fold8(const float (&s)[8]) { return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])); }

__global__ __launch_bounds__(256) void vicreg_stats_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int N, int D,
                                                           float eps, int T64, float* __restrict__ stats,
                                                           float* __restrict__ hingep, float* __restrict__ invp) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, v = blockIdx.y;
  const bool ok = c < D;
  if (v == 2) {                                                  // the invariance term's share of this column tile
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
      int n = w;
      for (; n + 28 < N; n += 32)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const long long e = (long long)(n + 4 * u) * D + c;
          const float d = z1[e] - z2[e];
          s[u] += d * d;
        }
      for (; n < N; n += 4) { const long long e = (long long)n * D + c; const float d = z1[e] - z2[e]; s[0] += d * d; }
    }
    red[w][lane] = fold8(s);
    __syncthreads();
    if (w == 0) {
      const float t = gca_wave_sum(((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
      if (lane == 0) invp[blockIdx.x] = t;
    }
    return;
  }
  const float* __restrict__ z = v ? z2 : z1;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    int n = w;
    for (; n + 28 < N; n += 32)
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += z[(long long)(n + 4 * u) * D + c];
    for (; n < N; n += 4) s[0] += z[(long long)n * D + c];
  }
  red[w][lane] = fold8(s);
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
  red[w][lane] = fold8(q);
  __syncthreads();
  if (w == 0) {
    const float var = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)(N - 1);
    const float sd = sqrtf(var + eps);
    if (ok) {
      stats[(2 * v) * D + c] = mean;
      stats[(2 * v + 1) * D + c] = sd;
    }
    const float h = gca_wave_sum(ok ? fmaxf(0.f, 1.f - sd) : 0.f);
    if (lane == 0) hingep[v * T64 + blockIdx.x] = h;
  }
}

// rows n0 + kk of one view, columns c0 + lane, centred; zeros outside (N, D).  Thread: column `lane`, rows (tid >> 6) + 4 it.
// Loads are clamped into the tensor, never predicated, so all of a chunk's loads are in flight at once; the store masks.
__device__ __forceinline__ void cov_fetch(float (&v)[NPT], const float* __restrict__ z, int n0, int col, int N, int D, int wave) {
  const int c = col < D ? col : D - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int n = n0 + wave + 4 * it;
    v[it] = z[(long long)(n < N ? n : N - 1) * D + c];
  }
}
__device__ __forceinline__ void cov_store(const float (&v)[NPT], float* dst, int n0, int col, int N, int D, float mean, int wave,
                                          int lane) {
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int kk = wave + 4 * it;
    dst[kk * TP + lane] = (n0 + kk < N && col < D) ? v[it] - mean : 0.f;
  }
}

__global__ __launch_bounds__(256) void vicreg_cov_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                         const float* __restrict__ stats, int N, int D, int T64,
                                                         float* __restrict__ covm, float* __restrict__ covp) {
  __shared__ float As[KC * TP];
  __shared__ float Bs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int view = blockIdx.z;
  int ti = 0, tj = blockIdx.x;                                   // blockIdx.x counts the tiles with tj >= ti row by row
  while (tj >= T64 - ti) { tj -= T64 - ti; ++ti; }
  tj += ti;
  const bool mirror = tj != ti;
  const float* __restrict__ z = view ? z2 : z1;
  const float* __restrict__ mean = stats + 2 * view * D;
  const int i0 = ti * TW, j0 = tj * TW;
  const int ci = i0 + lane, cj = j0 + lane;                      // the columns this thread stages for the two operands
  const float mi = ci < D ? mean[ci] : 0.f, mj = cj < D ? mean[cj] : 0.f;
  const bool live = i0 + wr * 32 < D && j0 + wc * 32 < D;
  const float* Bp = mirror ? Bs : As;                            // a diagonal tile multiplies one staged chunk by itself

  f32x16 acc, tot;                                               // tot takes acc every FLUSH rows: short fp32 chains at large N
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
  float va[NPT], vb[NPT];
  cov_fetch(va, z, 0, ci, N, D, wave);
  if (mirror) cov_fetch(vb, z, 0, cj, N, D, wave);
  for (int n0 = 0; n0 < N; n0 += KC) {
    if (n0 > 0 && n0 % FLUSH == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
    }
    cov_store(va, As, n0, ci, N, D, mi, wave, lane);
    if (mirror) cov_store(vb, Bs, n0, cj, N, D, mj, wave, lane);
    __syncthreads();
    if (n0 + KC < N) {                                           // the next chunk streams in behind the MFMAs
      cov_fetch(va, z, n0 + KC, ci, N, D, wave);
      if (mirror) cov_fetch(vb, z, n0 + KC, cj, N, D, wave);
    }
    if (live) chunk_mma(acc, As, Bp, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }

  // ---- epilogue: Cov (and its transpose), and this wave tile's share of the off-diagonal square-sum
  float* __restrict__ cv = covm + (size_t)view * D * D;
  const int j = j0 + wc * 32 + ll;
  float off = 0.f;
  if (live) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wr * 32 + acc_row(r, lh);
      const float c = (tot[r] + acc[r]) / (float)(N - 1);
      if (i < D && j < D) {
        cv[(size_t)i * D + j] = c;
        if (mirror) cv[(size_t)j * D + i] = c;
        if (i != j) off += c * c;
      }
    }
  }
  off = gca_wave_sum(off);
  if (lane == 0) covp[((size_t)view * gridDim.x + blockIdx.x) * 4 + wave] = mirror ? 2.f * off : off;
}

__global__ __launch_bounds__(256) void vicreg_fold_kernel(const float* __restrict__ invp, const float* __restrict__ hingep,
                                                          const float* __restrict__ covp, int N, int D, int T64, int ncov,
                                                          float sim, float stdc, float cov, float* __restrict__ loss4) {
  __shared__ double sh[12];
  double si = 0.0, sv = 0.0, sc = 0.0;
  for (int t = threadIdx.x; t < T64; t += 256) si += (double)invp[t];
  for (int t = threadIdx.x; t < 2 * T64; t += 256) sv += (double)hingep[t];
  for (int t = threadIdx.x; t < ncov; t += 256) sc += (double)covp[t];
  si = gca_block_sum256_d(si, sh);
  sv = gca_block_sum256_d(sv, sh + 4);
  sc = gca_block_sum256_d(sc, sh + 8);
  if (threadIdx.x == 0) {
    const double inv = si / ((double)N * (double)D), varl = sv / (2.0 * (double)D), covl = sc / (double)D;
    loss4[0] = (float)((double)sim * inv + (double)stdc * varl + (double)cov * covl);
    loss4[1] = (float)inv;
    loss4[2] = (float)varl;
    loss4[3] = (float)covl;
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// X chunk: rows n0 + c of the view, columns k0 + kk, centred -> Xs[kk][c].  Thread: kk = tid & 31, c = (tid >> 5) + 8 it.
// Cov chunk: rows k0 + kk of covm[view], columns c0 + c, diagonal zeroed -> Cs[kk][c].  Thread: kk = (tid >> 6) + 4 it, c = tid & 63.
// (Clamped loads, as cov_fetch; the stores into LDS mask.)
__device__ __forceinline__ void grad_fetch(float (&vx)[NPT], float (&vc)[NPT], const float* __restrict__ z,
                                           const float* __restrict__ cv, int n0, int c0, int k0, int N, int D, int tid) {
  const int k = k0 + (tid & 31), kc = k < D ? k : D - 1;
  const int j = c0 + (tid & 63), jc = j < D ? j : D - 1;
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int n = n0 + (tid >> 5) + 8 * it;
    vx[it] = z[(long long)(n < N ? n : N - 1) * D + kc];
  }
#pragma unroll
  for (int it = 0; it < NPT; ++it) {
    const int i = k0 + (tid >> 6) + 4 * it;
    vc[it] = cv[(size_t)(i < D ? i : D - 1) * D + jc];
  }
}

__global__ __launch_bounds__(256) void vicreg_grad_kernel(
    const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ stats, const float* __restrict__ covm,
    int N, int D, float cinv, float chinge, float ccov, const float* __restrict__ gscale_dev, float gscale_host,
    float* __restrict__ dz1, float* __restrict__ dz2) {
  __shared__ float Xs[KC * TP];
  __shared__ float Cs[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int view = blockIdx.z, c0 = blockIdx.x * TW, n0 = blockIdx.y * TW;
  const float* __restrict__ zs = view ? z2 : z1;                  // own view
  const float* __restrict__ zo = view ? z1 : z2;                  // the other one, for the invariance term only
  const float* __restrict__ st = stats + 2 * view * D;            // mean, sd of the own view
  const float* __restrict__ cv = covm + (size_t)view * D * D;
  float* __restrict__ dz = view ? dz2 : dz1;
  const bool live = n0 + wr * 32 < N && c0 + wc * 32 < D;
  const int kk = tid & 31;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float vx[NPT], vc[NPT];
  grad_fetch(vx, vc, zs, cv, n0, c0, 0, N, D, tid);
  float mk = st[kk < D ? kk : D - 1];
  for (int k0 = 0; k0 < D; k0 += KC) {
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
      const int c = (tid >> 5) + 8 * it;
      const int i = k0 + (tid >> 6) + 4 * it, j = c0 + (tid & 63);
      Xs[kk * TP + c] = (n0 + c < N && k0 + kk < D) ? vx[it] - mk : 0.f;
      Cs[((tid >> 6) + 4 * it) * TP + (tid & 63)] = (i < D && j < D && i != j) ? vc[it] : 0.f;
    }
    __syncthreads();
    if (k0 + KC < D) {                                            // the next chunk streams in behind the MFMAs
      const int k = k0 + KC + kk;
      grad_fetch(vx, vc, zs, cv, n0, c0, k0 + KC, N, D, tid);
      mk = st[k < D ? k : D - 1];
    }
    if (live) chunk_mma(acc, Xs, Cs, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int c = c0 + wc * 32 + ll;
  if (!live || c >= D) return;
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  const float ms = st[c], sd = st[D + c];
  const float hs = sd < 1.f ? chinge / sd : 0.f;                  // the hinge is active below a standard deviation of 1
  float own[16], oth[16];                                         // clamped loads first, all in flight; only the store is guarded
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    const long long e = (long long)(n < N ? n : N - 1) * D + c;
    own[r] = zs[e];
    oth[r] = zo[e];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    const float val = g * ((cinv * (own[r] - oth[r]) - hs * (own[r] - ms)) + ccov * acc[r]);
    if (n < N) dz[(long long)n * D + c] = val;
  }
}

bool sizes_ok(int64_t N, int64_t D) { return N >= 2 && N <= 65536 && D >= 1 && D <= 8192 && N * D < (1ll << 31); }
bool scalar_ok(float v) { return v >= 0.f && !isinf(v); }        // (false for NaN)
int64_t cov_tiles(int64_t D) { const int64_t T64 = gca_ceil_div(D, TW); return T64 * (T64 + 1) / 2; }

}  // namespace

extern "C" {

int64_t gca_vicreg_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  return (3 * gca_ceil_div(D, TW) + 8 * cov_tiles(D)) * 4;
}

int gca_vicreg_fwd(const float* z1, const float* z2, int64_t N, int64_t D, float sim, float stdc, float cov, float eps, float* stats,
                   float* covm, float* loss4, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(sim) || !scalar_ok(stdc) || !scalar_ok(cov) || !scalar_ok(eps)) return GCA_EINVAL;
  if (!z1 || !z2 || !stats || !covm || !loss4 || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int T64 = (int)gca_ceil_div(D, TW), P = (int)cov_tiles(D);
  float* invp = reinterpret_cast<float*>(ws);
  float* hingep = invp + T64;
  float* covp = hingep + 2 * T64;
  hipLaunchKernelGGL(vicreg_stats_kernel, dim3((unsigned)T64, 3), dim3(256), 0, st, z1, z2, (int)N, (int)D, eps, T64, stats, hingep,
                     invp);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(vicreg_cov_kernel, dim3((unsigned)P, 1, 2), dim3(256), 0, st, z1, z2, stats, (int)N, (int)D, T64, covm, covp);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(vicreg_fold_kernel, dim3(1), dim3(256), 0, st, invp, hingep, covp, (int)N, (int)D, T64, 8 * P, sim, stdc, cov,
                     loss4);
  return gca_launch_status();
}

int gca_vicreg_bwd(const float* z1, const float* z2, const float* stats, const float* covm, int64_t N, int64_t D, float sim,
                   float stdc, float cov, const float* gscale_dev, float gscale_host, float* dz1, float* dz2, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(sim) || !scalar_ok(stdc) || !scalar_ok(cov) || isnan(gscale_host) || isinf(gscale_host))
    return GCA_EINVAL;
  if (!z1 || !z2 || !stats || !covm || !dz1 || !dz2 || !ws) return GCA_EINVAL;
  const double n = (double)N, d = (double)D;
  const float cinv = (float)(2.0 * (double)sim / (n * d));
  const float chinge = (float)((double)stdc / (2.0 * d * (n - 1.0)));
  const float ccov = (float)(4.0 * (double)cov / (d * (n - 1.0)));
  hipLaunchKernelGGL(vicreg_grad_kernel, dim3((unsigned)gca_ceil_div(D, TW), (unsigned)gca_ceil_div(N, TW), 2), dim3(256), 0,
                     (hipStream_t)stream, z1, z2, stats, covm, (int)N, (int)D, cinv, chinge, ccov, gscale_dev, gscale_host, dz1, dz2);
  return gca_launch_status();
}

}  // extern "C"
