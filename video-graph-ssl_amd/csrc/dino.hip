// DINO's centred-teacher self-distillation loss (Caron et al. 2021) and its score gradient on gfx950.  tests/dino_ref.py is the
// numpy statement.
//
//   student features zs1, zs2 (N, D) and prototypes Cs (K, D); teacher features zt1, zt2 (N, D) and prototypes Ct (K, D); all fp32
//   with unit rows.  The centre c (K).  Per view v:  Ss_v = zs_v Cs^T      St_v = zt_v Ct^T      (N, K)
//   p_v  = softmax((St_v - c) / Tt)   (rows; no gradient)                  ls_v = Ss_v / Ts - lse(Ss_v / Ts)
//   l12 = -(1/N) sum_{n,k} p_1 ls_2      l21 = -(1/N) sum_{n,k} p_2 ls_1      loss = (l12 + l21) / 2
//   ent = -(1/(2N)) sum_{v,n,k} p_v ((St_v - c) / Tt - lse_t)               (the mean teacher entropy)
//   dSs_2 = (exp(ls_2) - p_1) / (2 N Ts)                                    dSs_1 = (exp(ls_1) - p_2) / (2 N Ts)
//   c' = cm c + (1 - cm) (1/(2N)) sum_{v,n} St_v[n,:]                       after the loss has used c, and only when asked
//
//   dino_scores_kernel   (64 prototypes, 64 rows of N, pair): the four products on the tile of mma_tile.h, reduction along D;
//                        pairs 0, 1: student views into dS, pairs 2, 3: teacher views into the workspace.
//   dino_row_kernel      (row n, direction d): one 256-thread workgroup, lanes along K (gca_dino_fwd_grid can give a row one
//                        wave instead, SwAV's grid, for the micro-benchmark that chose between the two).  Teacher row (view
//                        d + 1) and student row (the other view): online max / sum of both in one sweep, four elements in
//                        flight per thread; then a second sweep writes the teacher probabilities, dS over the student scores
//                        in place and the row's loss and entropy terms.
//   dino_center_kernel   (64 prototypes): column sums of the 2 N teacher rows, view 1 first, the 4 waves take rows w, w + 4, ...
//                        and are folded in wave order; then the EMA.  After the row kernel in stream order.
//   dino_fold_kernel     folds the 2 N row terms in row order in fp64: loss, l12, l21, ent.
//
// Tt is read from one device float, so a captured graph follows the teacher-temperature schedule.  The backward is
// gca_swav_bwd on (zs1, zs2, Cs, dS).  One owner per output element and fixed fold orders: no atomics, bitwise reproducible.
// Nothing reads the host.  One dispatch path: every global access is a guarded 4-byte one; element offsets are 64-bit.
#include <cstdint>
#include "gca_common.h"
#include "mma_tile.h"
#include "mma_stage.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void dino_scores_kernel(const float* __restrict__ zs1, const float* __restrict__ zs2,
                                                          const float* __restrict__ Cs, const float* __restrict__ zt1,
                                                          const float* __restrict__ zt2, const float* __restrict__ Ct, int N, int D,
                                                          int K, float* __restrict__ Ss, float* __restrict__ St) {
  __shared__ float Zl[KC * TP];
  __shared__ float Cl[KC * TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ll = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int pair = blockIdx.z, view = pair & 1, p0 = blockIdx.x * TW, n0 = blockIdx.y * TW;
  const float* __restrict__ z = pair < 2 ? (view ? zs2 : zs1) : (view ? zt2 : zt1);
  const float* __restrict__ C = pair < 2 ? Cs : Ct;
  const bool live = n0 + wr * 32 < N && p0 + wc * 32 < K;
  const int kk = tid & 31;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float vz[NPT], vc[NPT];
  xfetch(vz, z, n0, kk, N, D, tid);
  xfetch(vc, C, p0, kk, K, D, tid);
  for (int d0 = 0; d0 < D; d0 += KC) {
    xstore(vz, Zl, n0, d0 + kk, N, D, tid);
    xstore(vc, Cl, p0, d0 + kk, K, D, tid);
    __syncthreads();
    if (d0 + KC < D) {                                             // the next chunk streams in behind the MFMAs
      xfetch(vz, z, n0, d0 + KC + kk, N, D, tid);
      xfetch(vc, C, p0, d0 + KC + kk, K, D, tid);
    }
    if (live) chunk_mma(acc, Zl, Cl, wr * 32, wc * 32, ll, lh);
    __syncthreads();
  }
  const int p = p0 + wc * 32 + ll;
  if (!live || p >= K) return;
  float* __restrict__ Sv = (pair < 2 ? Ss : St) + (size_t)view * N * K;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wr * 32 + acc_row(r, lh);
    if (n < N) Sv[(size_t)n * K + p] = acc[r];
  }
}

__device__ __forceinline__ void online(float x, float& m, float& s) {
  if (x > m) { s = s * expf(m - x) + 1.f; m = x; }
  else s += expf(x - m);
}

// max over the workgroup's 256 threads, valid in every thread
__device__ __forceinline__ float block_max256(float v, float* sh /* >= 4 floats */) {
  v = gca_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

constexpr int RU = 4;                // elements of a row that a thread of dino_row_kernel keeps in flight

// the RU chains of one thread folded in chain order: their max, and their sums brought to the row's max M (a chain that met no
// element holds m = -inf, s = 0 and adds 0; M is finite, the row has elements)
__device__ __forceinline__ float chains_max(const float (&m)[RU]) { return fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])); }
__device__ __forceinline__ float chains_sum(const float (&m)[RU], const float (&s)[RU], float M) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < RU; ++j) a += s[j] * expf(m[j] - M);
  return a;
}

// max / sum over the T threads that share a row: the workgroup's 256 (through LDS) or one wave's 64; valid in every thread
template <int T> __device__ __forceinline__ float row_max(float v, float* sh) {
  if constexpr (T == 256) return block_max256(v, sh);
  else return gca_wave_max(v);
}
template <int T> __device__ __forceinline__ float row_sum(float v, float* sh) {
  if constexpr (T == 256) return gca_block_sum256(v, sh);
  else return gca_wave_sum(v);
}

// Row n, direction d = blockIdx.y: the teacher's view d + 1 teaches the student's other view.  T threads along K per row:
// T = 256, the whole workgroup (grid (N, 2)), or T = 64, one wave (grid (ceil(N / 4), 2)).  probs: (2, N, K) or nullptr.
template <int T>
__global__ __launch_bounds__(256) void dino_row_kernel(float* __restrict__ Ss, const float* __restrict__ St,
                                                       const float* __restrict__ center, const float* __restrict__ tt_dev, int N,
                                                       int K, float inv_Ts, float cgrad, float* __restrict__ rowp,
                                                       float* __restrict__ probs) {
  __shared__ float sh[4];
  const int tid = T == 256 ? threadIdx.x : threadIdx.x & 63;
  const int n = T == 256 ? blockIdx.x : blockIdx.x * 4 + (threadIdx.x >> 6), d = blockIdx.y;
  if (n >= N) return;                                              // (T = 64 only, a whole wave: nothing below meets a barrier then)
  const float* __restrict__ t = St + ((size_t)d * N + n) * K;
  float* __restrict__ s = Ss + ((size_t)(1 - d) * N + n) * K;
  const float inv_Tt = 1.f / *tt_dev;
  // RU elements of a row in flight per thread, each with an online (max, sum) chain of its own: a row has few waves to hide
  // the loads behind, so the chains are what keeps several of them outstanding
  float mt[RU], st[RU], ms[RU], ss[RU];
#pragma unroll
  for (int j = 0; j < RU; ++j) { mt[j] = ms[j] = -INFINITY; st[j] = ss[j] = 0.f; }
  int k = tid;
  for (; k + (RU - 1) * T < K; k += RU * T) {
    float xt[RU], xs[RU];
#pragma unroll
    for (int j = 0; j < RU; ++j) { xt[j] = (t[k + j * T] - center[k + j * T]) * inv_Tt; xs[j] = s[k + j * T] * inv_Ts; }
#pragma unroll
    for (int j = 0; j < RU; ++j) { online(xt[j], mt[j], st[j]); online(xs[j], ms[j], ss[j]); }
  }
  for (; k < K; k += T) {
    online((t[k] - center[k]) * inv_Tt, mt[0], st[0]);
    online(s[k] * inv_Ts, ms[0], ss[0]);
  }
  const float Mt = row_max<T>(chains_max(mt), sh);                 // (a thread without elements holds m = -inf, s = 0)
  const float lse_t = Mt + logf(row_sum<T>(chains_sum(mt, st, Mt), sh));
  const float Ms = row_max<T>(chains_max(ms), sh);
  const float lse_s = Ms + logf(row_sum<T>(chains_sum(ms, ss, Ms), sh));
  float tl = 0.f, te = 0.f;
  float* __restrict__ pr = probs ? probs + ((size_t)d * N + n) * K : nullptr;
  auto finish = [&](int kk, float tv, float cv, float sv) {
    const float xt = (tv - cv) * inv_Tt - lse_t;
    const float p = expf(xt);
    const float ls = sv * inv_Ts - lse_s;
    tl += p * ls;
    te += p * xt;
    s[kk] = (expf(ls) - p) * cgrad;
    if (pr) pr[kk] = p;
  };
  k = tid;
  for (; k + (RU - 1) * T < K; k += RU * T) {
    float tv[RU], cv[RU], sv[RU];
#pragma unroll
    for (int j = 0; j < RU; ++j) { tv[j] = t[k + j * T]; cv[j] = center[k + j * T]; sv[j] = s[k + j * T]; }
#pragma unroll
    for (int j = 0; j < RU; ++j) finish(k + j * T, tv[j], cv[j], sv[j]);
  }
  for (; k < K; k += T) finish(k, t[k], center[k], s[k]);
  tl = row_sum<T>(tl, sh);
  te = row_sum<T>(te, sh);
  if (tid == 0) { rowp[d * N + n] = -tl; rowp[2 * N + d * N + n] = -te; }
}

__device__ __forceinline__ float fold4(const float (&s)[4]) { return (s[0] + s[1]) + (s[2] + s[3]); }

// center[k] = cm center[k] + (1 - cm) / (2 N) sum_r St[r,k] over the R = 2 N teacher rows, view 1 first
__global__ __launch_bounds__(256) void dino_center_kernel(const float* __restrict__ St, int R, int K, float cm, float om_over_R,
                                                          float* __restrict__ center) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (k < K) {
    int r = w;
    for (; r + 12 < R; r += 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += St[(size_t)(r + 4 * j) * K + k];
    for (; r < R; r += 4) s[0] += St[(size_t)r * K + k];
  }
  red[w][lane] = fold4(s);
  __syncthreads();
  if (w == 0 && k < K)
    center[k] = cm * center[k] + om_over_R * (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

__global__ __launch_bounds__(256) void dino_fold_kernel(const float* __restrict__ rowp, int N, float* __restrict__ parts) {
  __shared__ double sh[16];
  double a = 0.0, b = 0.0, e = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    a += (double)rowp[n];
    b += (double)rowp[N + n];
    e += (double)rowp[2 * N + n] + (double)rowp[3 * N + n];
  }
  a = gca_block_sum256_d(a, sh);
  b = gca_block_sum256_d(b, sh + 4);
  e = gca_block_sum256_d(e, sh + 8);
  if (threadIdx.x == 0) {
    const double l12 = a / (double)N, l21 = b / (double)N;
    parts[0] = (float)(0.5 * (l12 + l21));
    parts[1] = (float)l12;
    parts[2] = (float)l21;
    parts[3] = (float)(e / (2.0 * (double)N));
  }
}

bool sizes_ok(int64_t N, int64_t D, int64_t K) { return N >= 2 && N <= 8192 && K >= 2 && K <= 65536 && D >= 1 && D <= 8192; }
// Ts positive with Ts and 1 / Ts finite in fp32; cm in [0, 1).  (false for NaN)
bool params_ok(float Ts, float cm) { return Ts > 0.f && !isinf(Ts) && !isinf(1.f / Ts) && cm >= 0.f && cm < 1.f; }

}  // namespace

extern "C" {

int64_t gca_dino_ws_bytes(int64_t N, int64_t D, int64_t K) {
  if (!sizes_ok(N, D, K)) return -1;
  return (2 * N * K + 4 * N) * 4;                                  // the teacher scores (2, N, K), the row terms (4, N)
}

int gca_dino_fwd_grid(const float* zs1, const float* zs2, const float* Cs, const float* zt1, const float* zt2, const float* Ct,
                      int64_t N, int64_t D, int64_t K, float Ts, const float* tt_dev, float cm, float* center, int update_center,
                      float* parts, float* dS, float* probs, int row_grid, void* ws, void* stream) {
  if (!sizes_ok(N, D, K) || !params_ok(Ts, cm) || row_grid < 0 || row_grid > 1) return GCA_EINVAL;
  if (!zs1 || !zs2 || !Cs || !zt1 || !zt2 || !Ct || !tt_dev || !center || !parts || !dS || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* St = reinterpret_cast<float*>(ws);
  float* rowp = St + 2 * N * K;
  const float inv_Ts = (float)(1.0 / (double)Ts);
  const float cgrad = (float)(1.0 / (2.0 * (double)N * (double)Ts));
  const unsigned TK = (unsigned)gca_ceil_div(K, TW), TN = (unsigned)gca_ceil_div(N, TW);
  hipLaunchKernelGGL(dino_scores_kernel, dim3(TK, TN, 4), dim3(256), 0, st, zs1, zs2, Cs, zt1, zt2, Ct, (int)N, (int)D, (int)K, dS, St);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  if (row_grid == GCA_DINO_ROW_WORKGROUP)
    hipLaunchKernelGGL(dino_row_kernel<256>, dim3((unsigned)N, 2), dim3(256), 0, st, dS, (const float*)St, (const float*)center,
                       tt_dev, (int)N, (int)K, inv_Ts, cgrad, rowp, probs);
  else
    hipLaunchKernelGGL(dino_row_kernel<64>, dim3((unsigned)gca_ceil_div(N, 4), 2), dim3(256), 0, st, dS, (const float*)St,
                       (const float*)center, tt_dev, (int)N, (int)K, inv_Ts, cgrad, rowp, probs);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  if (update_center) {
    hipLaunchKernelGGL(dino_center_kernel, dim3(TK), dim3(256), 0, st, (const float*)St, (int)(2 * N), (int)K, cm,
                       (float)((1.0 - (double)cm) / (2.0 * (double)N)), center);
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  }
  hipLaunchKernelGGL(dino_fold_kernel, dim3(1), dim3(256), 0, st, (const float*)rowp, (int)N, parts);
  return gca_launch_status();
}

int gca_dino_fwd(const float* zs1, const float* zs2, const float* Cs, const float* zt1, const float* zt2, const float* Ct, int64_t N,
                 int64_t D, int64_t K, float Ts, const float* tt_dev, float cm, float* center, int update_center, float* parts,
                 float* dS, float* probs, void* ws, void* stream) {
  return gca_dino_fwd_grid(zs1, zs2, Cs, zt1, zt2, Ct, N, D, K, Ts, tt_dev, cm, center, update_center, parts, dS, probs,
                           GCA_DINO_ROW_WORKGROUP, ws, stream);
}

}  // extern "C"
