// Action-recognition class head on gfx950: linear classifier fused with softmax cross-entropy.
//
//   logits[i,j] = (sum_d x[i,d] * w[j,d]) + bias[j]      fp32 matrix cores (v_mfma_f32_32x32x2_f32), fp32 accumulation
//   row_lse[i]  = m_i + log sum_j exp(logits[i,j] - m_i)  m_i the row maximum
//   rank_ge[i]  = #{ j != target[i] : logits[i,j] >= logits[i,target[i]] }      (gca_rank_ge's definition)
//   loss        = (1/b) sum_i (row_lse[i] - logits[i,target[i]])
//   g[i,j]      = s (exp(logits[i,j] - row_lse[i]) - [j == target[i]])          formed where it is consumed, never stored
//   dw = g^T x,  dbias = column sums of g,  dx = g w
//
// Forward: logits tiles -> row statistics -> loss.  Backward: (dw, dbias) and dx, two independent launches, plus a fold of
// the dw slabs when the batch is long enough to be cut into runs (b > 512).  A workgroup
// owns one 32 x 32 output tile; its four waves split the contraction axis (features, batch rows or classes) in an interleaved
// way and their partial tiles are added in wave order through LDS, so every sum has an order fixed by the shapes alone.  No
// atomics, no hand-off between workgroups.  The target's logit is found by comparing the column index with the target inside
// the sweep, never by address: an out-of-range target cannot touch memory it should not.
// Reference: lib/modeling/model_wrappers.py:74-82,99-117 (nn.Linear head) + nn.CrossEntropyLoss (tools/train_ds.py:111-112).
#include <cstdint>
#include "gca_common.h"
#include <math.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TM = 32;               // output tile: 32 x 32, one MFMA accumulator per wave
constexpr int UN = 4;                // contraction steps whose loads are issued together

// Four consecutive features of a row, zeros where the row is not wanted or the feature lies past F.  The load itself is
// unconditional (a clamped address) so that the compiler keeps several in flight.  VEC: F % 4 == 0 and 16-byte aligned bases.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, long long d, long long F, bool want) {
  if (VEC) {
    const bool ok = want && d < F;
    const float4 v = *reinterpret_cast<const float4*>(row + (ok ? d : 0));
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float e[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool ok = want && d + u < F;
    const float v = row[ok ? d + u : 0];
    e[u] = ok ? v : 0.f;
  }
  return make_float4(e[0], e[1], e[2], e[3]);
}

// The four waves' partial tiles -> LDS; after the barrier thread `tid` owns registers r = (tid >> 6) + 4 q, q < 4, of lane
// tid & 63 and adds the partials in wave order.
__device__ __forceinline__ void fold_store(float (*fold)[16][64], const f32x16& acc, int wave, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) fold[wave][r][lane] = acc[r];
  __syncthreads();
}
__device__ __forceinline__ float fold_sum(float (*fold)[16][64], int r, int lane) {
  return ((fold[0][r][lane] + fold[1][r][lane]) + fold[2][r][lane]) + fold[3][r][lane];
}

// Workgroup = logits tile (32 rows x 32 classes).  Wave w contracts features [32 t + 8 w, 32 t + 8 w + 8), t = 0, 1, ...:
// lane (lh, ll) reads four features of row ll of each operand, which are four MFMA steps.
template <bool VEC>
__global__ __launch_bounds__(256) void classifier_logits_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, long long b, long long F,
                                                                long long C, long long tiles_c, float* __restrict__ logits) {
  __shared__ float fold[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5, ll = lane & 31;
  const long long tb = blockIdx.x / tiles_c, tc = blockIdx.x - tb * tiles_c;
  const long long i = tb * TM + ll, j = tc * TM + ll;
  const bool iok = i < b, jok = j < C;
  const float* xr = x + (iok ? i : b - 1) * F;
  const float* wr = w + (jok ? j : C - 1) * F;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long long f0 = 8 * wave; f0 < F; f0 += 32 * UN) {      // UN loads in flight; steps past F contribute zeros
    float4 a[UN], c[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      a[u] = load4<VEC>(xr, f0 + 32 * u + 4 * lh, F, iok);
      c[u] = load4<VEC>(wr, f0 + 32 * u + 4 * lh, F, jok);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, c[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, c[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, c[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, c[u].w, acc, 0, 0, 0);
    }
  }
  fold_store(fold, acc, wave, lane);
  const float bj = (bias && jok) ? bias[j] : 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave + 4 * q;
    const long long row = tb * TM + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (row < b && jok) logits[row * C + j] = fold_sum(fold, r, lane) + bj;
  }
}

// One wave per row of the stored logits: maximum and the target's logit, then sum of exponentials and the ">=" count.
// Lane l sees columns l, l + 64, ...; the lanes are folded by a fixed butterfly.
__global__ __launch_bounds__(256) void classifier_rows_kernel(const float* __restrict__ logits,
                                                              const long long* __restrict__ target, long long b, long long C,
                                                              float* __restrict__ row_lse, int* __restrict__ rank_ge,
                                                              float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= b) return;
  const float* row = logits + i * C;
  const long long t = target ? target[i] : -1;
  float m = -INFINITY, tv = 0.f;
  bool mine = false;
  for (long long j = lane; j < C; j += 64) {
    const float v = row[j];
    m = fmaxf(m, v);
    if (j == t) { tv = v; mine = true; }
  }
  m = gca_wave_max(m);
  const unsigned long long owner = __ballot(mine);
  const float tl = owner ? __shfl(tv, __ffsll((long long)owner) - 1, 64) : 0.f;
  float s = 0.f;
  int cnt = 0;
  for (long long j = lane; j < C; j += 64) {
    const float v = row[j];
    s += expf(v - m);
    cnt += (j != t && v >= tl) ? 1 : 0;
  }
  s = gca_wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    const float lse = m + logf(s);
    if (row_lse) row_lse[i] = lse;
    if (rank_ge) rank_ge[i] = cnt;
    if (row_loss) row_loss[i] = lse - tl;
  }
}

// loss = (sum_i row_loss[i]) / b: thread t adds rows t, t + 256, ... in fp64, then lanes and waves in a fixed order.
__global__ __launch_bounds__(256) void classifier_loss_kernel(const float* __restrict__ row_loss, long long b,
                                                              float* __restrict__ loss) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long long i = threadIdx.x; i < b; i += 256) s += (double)row_loss[i];
  s = gca_block_sum256_d(s, sh);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)b);
}

__device__ __forceinline__ float grad_scale(const float* __restrict__ gs_dev, float gs_host, long long b) {
  return gs_host * (gs_dev ? *gs_dev : 1.f) / (float)b;
}

// Workgroup = dw tile (32 classes x 32 features), contraction over the batch: wave w takes rows 8 t + 2 w + lh.  A = g^T
// (lane (lh, ll): class ll, row lh of the pair), B = x.  The workgroups of the first feature tile also fold dbias.  A long
// batch is cut into `splits` runs of rows_per_split rows: workgroup (tile, split) then writes its sums to slab `split` of
// the scratch (dw: splits x C x F, dbias: splits x C) and classifier_fold_kernel adds the slabs in split order.
__global__ __launch_bounds__(256) void classifier_dw_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                            const float* __restrict__ lse, const long long* __restrict__ target,
                                                            const float* __restrict__ gs_dev, float gs_host, long long b,
                                                            long long F, long long C, long long tiles_f, int splits,
                                                            long long rows_per_split, float* __restrict__ dw,
                                                            float* __restrict__ dbias, int accumulate) {
  __shared__ float fold[4][16][64];
  __shared__ float bfold[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5, ll = lane & 31;
  const long long tile = blockIdx.x / splits, sp = blockIdx.x - tile * splits;
  const long long tc = tile / tiles_f, tf = tile - tc * tiles_f;
  const long long r0 = sp * rows_per_split, r1 = min(b, r0 + rows_per_split);
  if (splits > 1) {
    dw += sp * C * F;
    if (dbias) dbias += sp * C;
  }
  const long long j = tc * TM + ll, d = tf * TM + ll;
  const bool jok = j < C, dok = d < F;
  const long long jc = jok ? j : C - 1, dc = dok ? d : F - 1;
  const float s = grad_scale(gs_dev, gs_host, b);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  for (long long i0 = r0 + 2 * wave; i0 < r1; i0 += 8 * UN) {  // UN loads in flight; rows past the run contribute zeros
    float a[UN], xv[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long long i = i0 + 8 * u + lh;
      const bool iok = i < r1;
      const long long ic = iok ? i : b - 1;
      const float l = logits[ic * C + jc], ls = lse[ic], v = x[ic * F + dc];
      const long long t = target[ic];
      a[u] = (iok && jok) ? s * (expf(l - ls) - (j == t ? 1.f : 0.f)) : 0.f;
      xv[u] = (iok && dok) ? v : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], xv[u], acc, 0, 0, 0);
      bsum += a[u];
    }
  }
  bfold[wave][lane] = bsum;
  fold_store(fold, acc, wave, lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave + 4 * q;
    const long long row = tc * TM + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (row < C && dok) {
      const float v = fold_sum(fold, r, lane);
      float* o = dw + row * F + d;
      *o = accumulate ? *o + v : v;
    }
  }
  if (dbias && tf == 0 && tid < 32 && tc * TM + tid < C) {
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) v += bfold[u][tid] + bfold[u][32 + tid];
    float* o = dbias + tc * TM + tid;
    *o = accumulate ? *o + v : v;
  }
}

// out[e] (+)= slab[0][e] + slab[1][e] + ... in split order, for the n elements of dw followed by the m of dbias.
__global__ __launch_bounds__(256) void classifier_fold_kernel(const float* __restrict__ wslab, const float* __restrict__ bslab,
                                                              int splits, long long n, long long m, float* __restrict__ dw,
                                                              float* __restrict__ dbias, int accumulate) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n + m) return;
  const bool isw = e < n;
  const float* src = isw ? wslab + e : bslab + (e - n);
  const long long stride = isw ? n : m;
  float v = 0.f;
  for (int sp = 0; sp < splits; ++sp) v += src[sp * stride];
  float* o = isw ? dw + e : dbias + (e - n);
  *o = accumulate ? *o + v : v;
}

// Workgroup = dx tile (32 rows x 32 features), contraction over the classes: wave w takes classes 8 t + 2 w + lh.  A = g
// (lane (lh, ll): row ll, class lh of the pair), B = w.
__global__ __launch_bounds__(256) void classifier_dx_kernel(const float* __restrict__ w, const float* __restrict__ logits,
                                                            const float* __restrict__ lse, const long long* __restrict__ target,
                                                            const float* __restrict__ gs_dev, float gs_host, long long b,
                                                            long long F, long long C, long long tiles_f, float* __restrict__ dx,
                                                            int accumulate) {
  __shared__ float fold[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5, ll = lane & 31;
  const long long tb = blockIdx.x / tiles_f, tf = blockIdx.x - tb * tiles_f;
  const long long i = tb * TM + ll, d = tf * TM + ll;
  const bool iok = i < b, dok = d < F;
  const long long ic = iok ? i : b - 1, dc = dok ? d : F - 1;
  const float s = grad_scale(gs_dev, gs_host, b);
  const float ls = lse[ic];
  const long long t = target[ic];
  const float* lrow = logits + ic * C;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long long j0 = 2 * wave; j0 < C; j0 += 8 * UN) {        // UN loads in flight; classes past C contribute zeros
    float a[UN], wv[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long long j = j0 + 8 * u + lh;
      const bool jok = j < C;
      const long long jc = jok ? j : C - 1;
      const float l = lrow[jc], v = w[jc * F + dc];
      a[u] = (iok && jok) ? s * (expf(l - ls) - (j == t ? 1.f : 0.f)) : 0.f;
      wv[u] = (jok && dok) ? v : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], wv[u], acc, 0, 0, 0);
  }
  fold_store(fold, acc, wave, lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave + 4 * q;
    const long long row = tb * TM + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (row < b && dok) {
      const float v = fold_sum(fold, r, lane);
      float* o = dx + row * F + d;
      *o = accumulate ? *o + v : v;
    }
  }
}

constexpr long long LIM = 0x7FFFFFFFll;
constexpr int SPLIT_ROWS = 512, SPLIT_MAX = 16;       // dw: one run of batch rows per 512, at most 16 runs

// Runs of the batch axis in the dw launch: a function of b alone, so the summation order is fixed by the shapes.
int dw_splits(int64_t b) {
  const long long s = gca_ceil_div(b, SPLIT_ROWS);
  return (int)(s < 1 ? 1 : (s > SPLIT_MAX ? SPLIT_MAX : s));
}

// Sizes every entry accepts: b >= 0, F, C >= 1, all below 2^31, and every 1-D grid of tiles below 2^31 blocks.
bool sizes_ok(int64_t b, int64_t F, int64_t C) {
  if (b < 0 || F < 1 || C < 1 || b > LIM || F > LIM || C > LIM) return false;
  const long long tb = gca_ceil_div(b, TM), tf = gca_ceil_div(F, TM), tc = gca_ceil_div(C, TM);
  return tb * tc <= LIM && tc * tf * SPLIT_MAX <= LIM && tb * tf <= LIM && C * F + C <= LIM * 256;
}

}  // namespace

extern "C" {

int64_t gca_classifier_ws_bytes(int64_t b, int64_t F, int64_t C) {
  if (!sizes_ok(b, F, C)) return GCA_EINVAL;
  const int64_t rows = gca_round_up((b > 0 ? b : 1) * 4, 16);            // one loss term per row (forward)
  const int S = dw_splits(b);
  return rows + (S > 1 ? (int64_t)S * (C * F + C) * 4 : 0);               // dw / dbias slabs of a long batch (backward)
}

int gca_classifier_fwd(const float* x, const float* w, const float* bias, const int64_t* target, int64_t b, int64_t F,
                       int64_t C, float* logits, float* row_lse, int32_t* rank_ge, float* loss, void* ws, int64_t ws_bytes,
                       void* stream) {
  if (!sizes_ok(b, F, C) || ws_bytes < gca_classifier_ws_bytes(b, F, C)) return GCA_EINVAL;
  if ((loss || rank_ge) && !target) return GCA_EINVAL;
  if (target && !row_lse) return GCA_EINVAL;
  if (b == 0) return GCA_OK;
  const bool given = !x && !w && !bias && target;          // the logits are an input: row statistics and loss only
  if (!logits || (loss && !ws) || (!given && (!x || !w))) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long tiles_c = gca_ceil_div(C, TM);
  const dim3 grid((unsigned)(gca_ceil_div(b, TM) * tiles_c));
  const bool vec = F % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0;
  if (given) {
  } else if (vec)
    hipLaunchKernelGGL(classifier_logits_kernel<true>, grid, dim3(256), 0, st, x, w, bias, (long long)b, (long long)F,
                       (long long)C, tiles_c, logits);
  else
    hipLaunchKernelGGL(classifier_logits_kernel<false>, grid, dim3(256), 0, st, x, w, bias, (long long)b, (long long)F,
                       (long long)C, tiles_c, logits);
  int rc = gca_launch_status();
  if (rc || !row_lse) return rc;
  float* row_loss = loss ? reinterpret_cast<float*>(ws) : nullptr;
  hipLaunchKernelGGL(classifier_rows_kernel, dim3((unsigned)gca_ceil_div(b, 4)), dim3(256), 0, st, (const float*)logits,
                     reinterpret_cast<const long long*>(target), (long long)b, (long long)C, row_lse, rank_ge, row_loss);
  rc = gca_launch_status();
  if (rc || !loss) return rc;
  hipLaunchKernelGGL(classifier_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)row_loss, (long long)b, loss);
  return gca_launch_status();
}

int gca_classifier_bwd(const float* x, const float* w, const float* logits, const float* row_lse, const int64_t* target,
                       const float* gscale_dev, float gscale_host, int64_t b, int64_t F, int64_t C, float* dw, float* dbias,
                       int accumulate, float* dx, int dx_accumulate, void* ws, int64_t ws_bytes, void* stream) {
  if (!sizes_ok(b, F, C) || ws_bytes < gca_classifier_ws_bytes(b, F, C)) return GCA_EINVAL;
  if (b == 0) return GCA_OK;
  if (!x || !logits || !row_lse || !target || !dw || (dx && !w)) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long tiles_f = gca_ceil_div(F, TM);
  const long long* tg = reinterpret_cast<const long long*>(target);
  const int S = dw_splits(b);
  const long long rps = gca_round_up(gca_ceil_div(b, S), 8);
  float* wslab = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + gca_round_up(b * 4, 16));
  float* bslab = wslab + (long long)S * C * F;
  if (S > 1 && !ws) return GCA_EINVAL;
  hipLaunchKernelGGL(classifier_dw_kernel, dim3((unsigned)(gca_ceil_div(C, TM) * tiles_f * S)), dim3(256), 0, st, x, logits,
                     row_lse, tg, gscale_dev, gscale_host, (long long)b, (long long)F, (long long)C, tiles_f, S, rps,
                     S > 1 ? wslab : dw, S > 1 ? (dbias ? bslab : nullptr) : dbias, S > 1 ? 0 : accumulate);
  if (S > 1) {
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
    const long long n = (long long)C * F, m = dbias ? C : 0;
    hipLaunchKernelGGL(classifier_fold_kernel, dim3((unsigned)gca_ceil_div(n + m, 256)), dim3(256), 0, st, (const float*)wslab,
                       (const float*)bslab, S, n, m, dw, dbias, accumulate);
  }
  int rc = gca_launch_status();
  if (rc || !dx) return rc;
  hipLaunchKernelGGL(classifier_dx_kernel, dim3((unsigned)(gca_ceil_div(b, TM) * tiles_f)), dim3(256), 0, st, w, logits, row_lse,
                     tg, gscale_dev, gscale_host, (long long)b, (long long)F, (long long)C, tiles_f, dx, dx_accumulate);
  return gca_launch_status();
}

}  // extern "C"
