// Head pieces (ReLU, row L2-normalise, negative cosine) and the multi-tensor parameter updates
// (EMA key-encoder update, SGD, LARS, Adam / AdamW) over flat parameter arenas.  All HBM-bound float4 streaming.
// Reference call sites: see include/gca_hip.h.
#include <cstdint>
#include "gca_common.h"

namespace {

inline unsigned ew_blocks(long long n4) {
  long long b = gca_ceil_div(n4, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

__global__ void relu_fwd_kernel(const float* __restrict__ x, long long n, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = fmaxf(x[i], 0.f);
}
__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, long long n,
                                float* __restrict__ dx) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// one wave per row: y = x / max(||x||, eps)
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, long long rows, int dim, float eps,
                                                         float* __restrict__ y, float* __restrict__ inv) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + r * dim;
  float s = 0.f;
  for (int i = lane; i < dim; i += 64) s += xr[i] * xr[i];
  s = gca_wave_sum(s);
  const float iv = 1.f / fmaxf(sqrtf(s), eps);
  for (int i = lane; i < dim; i += 64) y[r * dim + i] = xr[i] * iv;
  if (lane == 0 && inv) inv[r] = iv;
}
// dx = inv * (dy - y * <dy, y>)    (exact where ||x|| > eps)
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                         const float* __restrict__ inv, long long rows, int dim,
                                                         float* __restrict__ dx) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int i = lane; i < dim; i += 64) s += dy[r * dim + i] * y[r * dim + i];
  s = gca_wave_sum(s);
  const float iv = inv[r];
  for (int i = lane; i < dim; i += 64) dx[r * dim + i] = iv * (dy[r * dim + i] - y[r * dim + i] * s);
}

// loss (+)= -scale/rows * sum_i cos(p_i, z_i);  dp_i = -scale/rows * ( z_i/(|p||z|) - cos * p_i/|p|^2 )
// F.cosine_similarity clamps each norm with eps = 1e-8.
__global__ __launch_bounds__(256) void negcos_kernel(const float* __restrict__ p, const float* __restrict__ z,
                                                     long long rows, int dim, float scale, float* __restrict__ rowcos,
                                                     float* __restrict__ dp) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float pp = 0.f, zz = 0.f, pz = 0.f;
  for (int i = lane; i < dim; i += 64) {
    const float a = p[r * dim + i], b = z[r * dim + i];
    pp += a * a; zz += b * b; pz += a * b;
  }
  pp = gca_wave_sum(pp); zz = gca_wave_sum(zz); pz = gca_wave_sum(pz);
  const float np = fmaxf(sqrtf(pp), 1e-8f), nz = fmaxf(sqrtf(zz), 1e-8f);
  const float c = pz / (np * nz);
  if (lane == 0) rowcos[r] = c;
  if (dp) {
    const float k = -scale / (float)rows;
    for (int i = lane; i < dim; i += 64)
      dp[r * dim + i] = k * (z[r * dim + i] / (np * nz) - c * p[r * dim + i] / (np * np));
  }
}
__global__ __launch_bounds__(256) void negcos_finish_kernel(const float* __restrict__ rowcos, long long rows, float scale,
                                                            float* __restrict__ loss, int accumulate) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long long i = threadIdx.x; i < rows; i += 256) s += rowcos[i];
  s = gca_block_sum256(s, sh);
  if (threadIdx.x == 0) {
    const float v = -scale * s / (float)rows;
    *loss = accumulate ? *loss + v : v;
  }
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ pe, const float* __restrict__ p, long long n4, float m) {
  const float om = 1.f - m;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 a = reinterpret_cast<float4*>(pe)[i];
    const float4 b = reinterpret_cast<const float4*>(p)[i];
    // p_k.mul_(m).add_(p_q, alpha=1-m)  (tools/train_video_contrast_dis.py:180)
    a.x = a.x * m + om * b.x; a.y = a.y * m + om * b.y; a.z = a.z * m + om * b.z; a.w = a.w * m + om * b.w;
    reinterpret_cast<float4*>(pe)[i] = a;
  }
}

// One element of ema_kernel as the compiler contracts it there: (1 - m) b rounded, then one fused a m + that.  Spelled out so that
// the element-wise tail below keeps ema_kernel's bits.
__device__ __forceinline__ float ema_one(float a, float b, float m, float om) { return __fmaf_rn(a, m, __fmul_rn(om, b)); }

// gca_ema_update with the momentum read from one device float (a captured step follows the momentum schedule).  Whole float4s
// when both pointers are 16-byte aligned (n4 of them, else none), the remaining elements one by one.
__global__ __launch_bounds__(256) void ema_dev_kernel(float* __restrict__ pe, const float* __restrict__ p, long long n4, long long n,
                                                      const float* __restrict__ m_dev) {
  const float m = *m_dev, om = 1.f - m;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long i = gid; i < n4; i += stride) {
    float4 a = reinterpret_cast<float4*>(pe)[i];
    const float4 b = reinterpret_cast<const float4*>(p)[i];
    a.x = ema_one(a.x, b.x, m, om); a.y = ema_one(a.y, b.y, m, om); a.z = ema_one(a.z, b.z, m, om); a.w = ema_one(a.w, b.w, m, om);
    reinterpret_cast<float4*>(pe)[i] = a;
  }
  for (long long i = 4 * n4 + gid; i < n; i += stride) pe[i] = ema_one(pe[i], p[i], m, om);
}

// The LARS factor times d, rounded on its own (the pragma withholds the product from contraction): fused into
// mom * buf + q * d it would round mom * buf instead, and a tensor with q == 1 would leave the SGD kernel's bits.
__device__ __forceinline__ float lars_scaled(float q, float d) {
#pragma clang fp contract(off)
  return q * d;
}

// torch.optim.SGD: d = g + wd*p; buf = (first ? d : mom*buf + d); d = nesterov ? d + mom*buf : buf; p -= lr*d
// One 256-element chunk per (lr, wd) pair: chunk c = i4 / 64.
// TRUST (LARS, gca_lars_step): d = ctr[c] * (g + wd*p), one more per-chunk factor (the tensor's trust ratio, written by
// lars_trust_kernel); the SGD instantiation never touches ctr and compiles to the operations it had without the parameter.
template <bool TRUST>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  long long n4, const float* __restrict__ clr, const float* __restrict__ cwd,
                                                  float lr_scale, float mom, int nesterov, int first,
                                                  const float* __restrict__ gscale, const float* __restrict__ ctr) {
  const float gs = gscale ? gscale[1] : 1.f;       // clip coefficient of gca_grad_clip_coef (grads.mul_(coef) folded in)
  if (gscale && gscale[2] != 0.f) return;          // a non-finite gradient was found (gca_grad_unscale_clip): optimizer.step() is skipped
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long c = i >> 6;
    const float lr = clr[c] * lr_scale, wd = cwd[c];
    const float q = TRUST ? ctr[c] : 1.f;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    if (gscale) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<float4*>(buf)[i];
    float d;
#define GCA_SGD1(f)                                   \
    d = gv.f + wd * pv.f;                             \
    if (TRUST) d = lars_scaled(q, d);                 \
    bv.f = first ? d : mom * bv.f + d;                \
    d = nesterov ? d + mom * bv.f : bv.f;             \
    pv.f = pv.f - lr * d;
    GCA_SGD1(x) GCA_SGD1(y) GCA_SGD1(z) GCA_SGD1(w)
#undef GCA_SGD1
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(buf)[i] = bv;
  }
}

// LARS (apex LARC(clip=False) around torch.optim.SGD): every tensor i of the arena scales its d = g + wd*p by
//   q_i = tau * |w_i| / (|g_i| + wd_i * |w_i| + eps)      (1 where the tensor is not adapted, or |w_i| == 0, or |g_i| == 0)
// Three launches, no atomics, every sum in a fixed order:
//   lars_sqsum_kernel   one workgroup per JOB (a run of <= LARS_JOB_CHUNKS chunks inside ONE tensor; the host lays the job
//                       table out once per arena): fp64 sums of w^2 and grad^2 (squares of fp32 values are exact in fp64;
//                       padding elements are zero) -> two partials per job
//   lars_trust_kernel   one workgroup per tensor: its jobs' partials folded in job order by one thread, the norms, q formed
//                       in fp64 and rounded once, written per tensor and per chunk of the tensor
//   sgd_kernel<true>    the SGD update with the per-chunk q
// A set skip flag (grad_clip[2] != 0) ends all three at once: the last norms / trust record stays.
constexpr int LARS_JOB_CHUNKS = 32;
struct LarsJob { int param, chunk0, chunks; };                 // host table: int32 triples
struct LarsParam { int job0, jobs, chunk0, chunks; };          // host table: int32 quadruples
__global__ __launch_bounds__(256) void lars_sqsum_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                         const LarsJob* __restrict__ jobs, const float* __restrict__ gscale,
                                                         double* __restrict__ part) {
  if (gscale && gscale[2] != 0.f) return;
  __shared__ double sh[4];
  const LarsJob j = jobs[blockIdx.x];
  const long long i0 = (long long)j.chunk0 * 64, i1 = i0 + (long long)j.chunks * 64;
  double sw = 0.0, sg = 0.0;
#pragma unroll 4
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const float4 a = reinterpret_cast<const float4*>(p)[i];
    const float4 b = reinterpret_cast<const float4*>(g)[i];
    sw += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
    sg += (double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z + (double)b.w * b.w;
  }
  sw = gca_block_sum256_d(sw, sh);
  sg = gca_block_sum256_d(sg, sh);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = sw;
    part[2 * (long long)blockIdx.x + 1] = sg;
  }
}
__global__ __launch_bounds__(256) void lars_trust_kernel(const double* __restrict__ part, const LarsParam* __restrict__ params,
                                                         const int* __restrict__ adapt, const float* __restrict__ cwd,
                                                         double tau, double eps, const float* __restrict__ gscale,
                                                         double* __restrict__ norms, float* __restrict__ trust,
                                                         float* __restrict__ ctr) {
  if (gscale && gscale[2] != 0.f) return;
  __shared__ double shw[256], shg[256];
  __shared__ float shq;
  const LarsParam t = params[blockIdx.x];
  double sw = 0.0, sg = 0.0;                                    // (thread 0's are the sums)
  for (int base = 0; base < t.jobs; base += 256) {              // staged through LDS: the partials arrive in parallel,
    const int k = base + threadIdx.x;                           // the fold stays one chain in job order
    if (k < t.jobs) {
      shw[threadIdx.x] = part[2 * (long long)(t.job0 + k)];
      shg[threadIdx.x] = part[2 * (long long)(t.job0 + k) + 1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = t.jobs - base < 256 ? t.jobs - base : 256;
      for (int k2 = 0; k2 < m; ++k2) { sw += shw[k2]; sg += shg[k2]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nw = sqrt(sw), ng = (gscale ? (double)gscale[1] : 1.0) * sqrt(sg);
    float q = 1.f;
    if (adapt[blockIdx.x] && nw > 0.0 && ng > 0.0) q = (float)(tau * nw / (ng + (double)cwd[t.chunk0] * nw + eps));
    norms[2 * (long long)blockIdx.x] = nw;
    norms[2 * (long long)blockIdx.x + 1] = ng;
    trust[blockIdx.x] = q;
    shq = q;
  }
  __syncthreads();
  const float q = shq;
  for (int c = threadIdx.x; c < t.chunks; c += 256) ctr[t.chunk0 + c] = q;
}

// torch.optim.Adam / AdamW (amsgrad=False, maximize=False) for step t = state[0] + 1, one pass over the arena:
//   g = grad * coef;   Adam: g += wd*p   AdamW: p *= 1 - lr*wd
//   m = b1*m + (1-b1)*g;   v = b2*v + (1-b2)*g*g;   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The number of steps taken lives on the device (state[0], an exact integer that adam_advance_kernel increments behind
// this kernel): a t passed by the host would be frozen into a captured hipGraph and with it the bias corrections.
// 1 - beta^t is formed in fp64 from that integer by every thread (repeated squaring: at most 2 * 63 multiplications next to the
// HBM traffic of its share of the arena) -- in fp32, 1 - 0.999f^1 has already lost four digits to cancellation.
__device__ inline double adam_one_minus_pow(double beta, long long t) {
  double r = 1.0, b = beta;
  for (unsigned long long e = (unsigned long long)t; e; e >>= 1) {
    if (e & 1) r *= b;
    b *= b;
  }
  return 1.0 - r;
}
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n4, const float* __restrict__ clr,
                                                   const float* __restrict__ cwd, double beta1, double beta2, float eps,
                                                   int decoupled, const float* __restrict__ gscale,
                                                   const long long* __restrict__ state) {
  if (gscale && gscale[2] != 0.f) return;          // non-finite gradient under loss scaling: optimizer.step() is skipped
  const float gs = gscale ? gscale[1] : 1.f;
  const long long t = state[0] + 1;
  const float inv_bc1 = (float)(1.0 / adam_one_minus_pow(beta1, t));
  const float inv_bc2s = (float)(1.0 / sqrt(adam_one_minus_pow(beta2, t)));
  // 1 - beta from the fp64 beta: 1.f - 0.999f is 1.3e-5 (relative) away from 0.001
  const float b1 = (float)beta1, b2 = (float)beta2, ob1 = (float)(1.0 - beta1), ob2 = (float)(1.0 - beta2);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long c = i >> 6;
    const float lr = clr[c], wd = cwd[c];
    const float ss = lr * inv_bc1, keep = 1.f - lr * wd;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    if (gscale) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    float d;
#define GCA_ADAM1(f)                                  \
    d = gv.f;                                         \
    if (decoupled) pv.f *= keep; else d += wd * pv.f; \
    mv.f = b1 * mv.f + ob1 * d;                       \
    vv.f = b2 * vv.f + ob2 * (d * d);                 \
    pv.f -= ss * (mv.f / (sqrtf(vv.f) * inv_bc2s + eps));
    GCA_ADAM1(x) GCA_ADAM1(y) GCA_ADAM1(z) GCA_ADAM1(w)
#undef GCA_ADAM1
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}
__global__ void adam_advance_kernel(long long* __restrict__ state, const float* __restrict__ gscale) {
  if (threadIdx.x == 0 && !(gscale && gscale[2] != 0.f)) state[0] += 1;      // a skipped step is not counted
}

// clip_grad_norm_ (tools/train_video_contrast_dis.py:420-423; torch.nn.utils.clip_grad_norm_, 2-norm): per-block partial
// sums of squares in fp64 over the whole gradient arena (padding elements are zero), then one block folds them in a fixed
// order: out[0] = total_norm, out[1] = min(1, max_norm / (total_norm + 1e-6)).  Deterministic.
constexpr int CLIP_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sqsum_partial_kernel(const float* __restrict__ g, long long n4, double* __restrict__ part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  s = gca_block_sum256_d(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ part, int nparts, float max_norm,
                                                        float* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = gca_block_sum256_d(s, sh);
  if (threadIdx.x == 0) {
    const float tn = (float)sqrt(s);
    out[0] = tn;
    out[1] = fminf(max_norm / (tn + 1e-6f), 1.0f);
    out[2] = 0.f;                                   // (torch's clip_grad_norm_ does not skip on a non-finite norm: neither does this)
    out[3] = 0.f;
  }
}

// Dynamic loss scaling (the reference's apex amp, tools/train_video_contrast_dis.py:134-141,413-418: scaled loss, un-scaled
// gradients, optimizer.step() skipped and the scale halved when a gradient is inf / nan, scale doubled after
// `interval` clean steps), decided on the device from the same fp64 sum of squares the clip uses: a non-finite element
// makes the sum non-finite.  state = {scale S, clean steps in a row, skipped steps so far, steps seen}.
__global__ __launch_bounds__(256) void unscale_clip_kernel(const double* __restrict__ part, int nparts, float max_norm,
                                                           float* __restrict__ state, float growth, float backoff,
                                                           int interval, float max_scale, float* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = gca_block_sum256_d(s, sh);
  if (threadIdx.x == 0) {
    float S = state[0];
    const bool finite = s == s && s < 1.7e308 && s >= 0.0;
    if (finite) {
      const float tn = (float)(sqrt(s) / (double)S);            // norm of the UN-scaled gradient
      const float coef = max_norm > 0.f ? fminf(max_norm / (tn + 1e-6f), 1.0f) : 1.0f;
      out[0] = tn; out[1] = coef / S; out[2] = 0.f; out[3] = S;
      const float clean = state[1] + 1.f;
      if (interval > 0 && clean >= (float)interval) { S = fminf(S * growth, max_scale); state[1] = 0.f; }
      else state[1] = clean;
    } else {
      out[0] = __builtin_inff(); out[1] = 0.f; out[2] = 1.f; out[3] = S;
      S = fmaxf(S * backoff, 1.f);
      state[1] = 0.f;
      state[2] += 1.f;
    }
    state[0] = S;
    state[3] += 1.f;
  }
}
__global__ void scale_dev_kernel(float* __restrict__ y, long long n, const float* __restrict__ a_dev, float a_host) {
  const float a = (a_dev ? *a_dev : 1.f) * a_host;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] *= a;
}

__global__ void fill_kernel(float* __restrict__ p, long long n, float v) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, long long n, float a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] += a * x[i];
}
// fp16-storage activations: gradient accumulation y += a*x in fp32, one rounding; and the fp32 -> fp16 cast of the input clips
__global__ void axpy_f16_kernel(gca_half* __restrict__ y, const gca_half* __restrict__ x, long long n, float a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = (gca_half)((float)y[i] + a * (float)x[i]);
}
// rows of re elements (re % 4 == 0), source rows src_stride apart (a channel slice of a wider clip batch), dense output
__global__ void cast_f16_kernel(const float* __restrict__ x, long long re4, long long src_stride, gca_half* __restrict__ y) {
  const float* xr = x + (long long)blockIdx.y * src_stride;
  gca_half* yr = y + (long long)blockIdx.y * re4 * 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < re4; i += (long long)gridDim.x * blockDim.x)
    gca_act<gca_half>::st4(yr + 4 * i, *reinterpret_cast<const float4*>(xr + 4 * i));
}
__global__ void scale_kernel(float* __restrict__ y, long long n, float a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] *= a;
}
// dst[r, :] = src[idx[r] * src_stride : +re]  -- one grid row per gathered row, float4 when alignment allows.
template <int V>
__global__ void gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ idx, long long re,
                                   long long src_stride, float* __restrict__ dst) {
  const long long r = blockIdx.y;
  const float* s = src + idx[r] * src_stride;
  float* d = dst + r * re;
  const long long step = (long long)gridDim.x * blockDim.x;
  if (V == 4) {
    const long long n4 = re >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += step)
      reinterpret_cast<float4*>(d)[i] = reinterpret_cast<const float4*>(s)[i];
  } else {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < re; i += step) d[i] = s[i];
  }
}

}  // namespace

extern "C" {

int gca_relu_fwd(const float* x, int64_t n, float* y, void* stream) {
  if (!x || !y || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(relu_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, y);
  return gca_launch_status();
}
int gca_relu_bwd(const float* dy, const float* y, int64_t n, float* dx, void* stream) {
  if (!dy || !y || !dx || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, y, (long long)n, dx);
  return gca_launch_status();
}
int gca_l2norm_fwd(const float* x, int64_t rows, int64_t dim, float eps, float* y, float* inv_norm, void* stream) {
  if (!x || !y || rows <= 0 || dim <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((unsigned)gca_ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x,
                     (long long)rows, (int)dim, eps, y, inv_norm);
  return gca_launch_status();
}
int gca_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, int64_t rows, int64_t dim,
                   float* dx, void* stream) {
  if (!dy || !y || !inv_norm || !dx || rows <= 0 || dim <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)gca_ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, dy,
                     y, inv_norm, (long long)rows, (int)dim, dx);
  return gca_launch_status();
}
int gca_negcos_fwd_bwd(const float* p, const float* z, int64_t rows, int64_t dim, float scale,
                       float* loss, int accumulate, float* dp, void* stream) {
  // `loss` must have room for 1 + rows floats: loss[0] = value, loss[1..rows] = per-row cosines
  // (no hidden allocation across the ABI).
  if (!p || !z || !loss || !dp || rows <= 0 || dim <= 0) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(negcos_kernel, dim3((unsigned)gca_ceil_div(rows, 4)), dim3(256), 0, st, p, z, (long long)rows,
                     (int)dim, scale, loss + 1, dp);
  hipLaunchKernelGGL(negcos_finish_kernel, dim3(1), dim3(256), 0, st, loss + 1, (long long)rows, scale, loss,
                     accumulate ? 1 : 0);
  return gca_launch_status();
}

int gca_ema_update(float* p_ema, const float* p, int64_t n, float m, void* stream) {
  if (!p_ema || !p || n <= 0 || (n & 3)) return GCA_EINVAL;
  hipLaunchKernelGGL(ema_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p_ema, p, (long long)(n / 4), m);
  return gca_launch_status();
}
int gca_ema_update_dev(float* p_ema, const float* p, int64_t n, const float* m_dev, void* stream) {
  if (!p_ema || !p || !m_dev || n <= 0) return GCA_EINVAL;
  const bool aligned = (((uintptr_t)p_ema | (uintptr_t)p) & 15) == 0;
  const long long n4 = aligned ? n / 4 : 0, rest = n - 4 * n4;
  hipLaunchKernelGGL(ema_dev_kernel, dim3(ew_blocks(n4 > rest ? n4 : rest)), dim3(256), 0, (hipStream_t)stream, p_ema, p, n4,
                     (long long)n, m_dev);
  return gca_launch_status();
}
int gca_sgd_step(float* p, const float* grad, float* mom_buf, int64_t n, const float* chunk_lr,
                 const float* chunk_wd, float lr_scale, float momentum, int nesterov, int first_step,
                 const float* grad_clip, void* stream) {
  if (!p || !grad || !mom_buf || !chunk_lr || !chunk_wd || n <= 0 || (n & 255)) return GCA_EINVAL;
  hipLaunchKernelGGL(sgd_kernel<false>, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p, grad, mom_buf,
                     (long long)(n / 4), chunk_lr, chunk_wd, lr_scale, momentum, nesterov, first_step, grad_clip,
                     (const float*)nullptr);
  return gca_launch_status();
}
int gca_lars_job_chunks(void) { return LARS_JOB_CHUNKS; }
int gca_lars_step(float* p, const float* grad, float* mom_buf, int64_t n, const float* chunk_lr, const float* chunk_wd,
                  const int32_t* jobs, int64_t n_jobs, const int32_t* params, const int32_t* adapt, int64_t n_params,
                  double* partials, double* norms, float* trust, float* chunk_trust, float momentum, int nesterov,
                  double trust_coef, double eps, const float* grad_clip, void* stream) {
  if (!p || !grad || !mom_buf || !chunk_lr || !chunk_wd || !jobs || !params || !adapt || !partials || !norms || !trust ||
      !chunk_trust || n <= 0 || (n & 255) || n / 256 > INT32_MAX || n_params <= 0 || n_jobs < n_params || n_jobs > n / 256 ||
      !(trust_coef > 0.0) || !(eps >= 0.0) || !(momentum >= 0.f && momentum < 1.f))
    return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_sqsum_kernel, dim3((unsigned)n_jobs), dim3(256), 0, st, p, grad,
                     reinterpret_cast<const LarsJob*>(jobs), grad_clip, partials);
  hipLaunchKernelGGL(lars_trust_kernel, dim3((unsigned)n_params), dim3(256), 0, st, partials,
                     reinterpret_cast<const LarsParam*>(params), adapt, chunk_wd, trust_coef, eps, grad_clip, norms, trust,
                     chunk_trust);
  hipLaunchKernelGGL(sgd_kernel<true>, dim3(ew_blocks(n / 4)), dim3(256), 0, st, p, grad, mom_buf, (long long)(n / 4),
                     chunk_lr, chunk_wd, 1.f, momentum, nesterov, 0, grad_clip, chunk_trust);
  return gca_launch_status();
}
int gca_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* chunk_lr,
                  const float* chunk_wd, double beta1, double beta2, double eps, int decoupled, const float* grad_clip,
                  const int64_t* state, void* stream) {
  if (!p || !grad || !exp_avg || !exp_avg_sq || !chunk_lr || !chunk_wd || !state || n <= 0 || (n & 255) ||
      !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
    return GCA_EINVAL;
  hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p, grad, exp_avg, exp_avg_sq,
                     (long long)(n / 4), chunk_lr, chunk_wd, beta1, beta2, (float)eps, decoupled ? 1 : 0, grad_clip,
                     (const long long*)state);
  return gca_launch_status();
}
int gca_adam_advance(int64_t* state, const float* grad_clip, void* stream) {
  if (!state) return GCA_EINVAL;
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)state, grad_clip);
  return gca_launch_status();
}
int64_t gca_grad_clip_ws_bytes(void) { return (int64_t)CLIP_BLOCKS * (int64_t)sizeof(double); }
int gca_grad_clip_coef(const float* grad, int64_t n, float max_norm, float* out4, void* ws, void* stream) {
  float* out2 = out4;
  if (!grad || !out2 || !ws || n <= 0 || (n & 3) || !(max_norm > 0.f)) return GCA_EINVAL;
  long long blocks = gca_ceil_div(n / 4, 256 * 8);
  if (blocks > CLIP_BLOCKS) blocks = CLIP_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, (long long)(n / 4),
                     reinterpret_cast<double*>(ws));
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws),
                     (int)blocks, max_norm, out2);
  return gca_launch_status();
}
int gca_grad_unscale_clip(const float* grad, int64_t n, float max_norm, float* scale_state4, float growth, float backoff,
                          int growth_interval, float max_scale, float* out4, void* ws, void* stream) {
  if (!grad || !out4 || !scale_state4 || !ws || n <= 0 || (n & 3) || !(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f) ||
      growth_interval < 0 || !(max_scale >= 1.f))
    return GCA_EINVAL;
  long long blocks = gca_ceil_div(n / 4, 256 * 8);
  if (blocks > CLIP_BLOCKS) blocks = CLIP_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, (long long)(n / 4),
                     reinterpret_cast<double*>(ws));
  hipLaunchKernelGGL(unscale_clip_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws),
                     (int)blocks, max_norm, scale_state4, growth, backoff, growth_interval, max_scale, out4);
  return gca_launch_status();
}
int gca_scale_dev(float* y, int64_t n, const float* a_dev, float a_host, void* stream) {
  if (!y || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(scale_dev_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, y, (long long)n, a_dev, a_host);
  return gca_launch_status();
}
int gca_fill(float* p, int64_t n, float v, void* stream) {
  if (!p || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(fill_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, (long long)n, v);
  return gca_launch_status();
}
int gca_axpy(float* y, const float* x, int64_t n, float a, void* stream) {
  if (!y || !x || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(axpy_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, y, x, (long long)n, a);
  return gca_launch_status();
}
int gca_axpy_f16(void* y, const void* x, int64_t n, float a, void* stream) {
  if (!y || !x || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(axpy_f16_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, (gca_half*)y, (const gca_half*)x,
                     (long long)n, a);
  return gca_launch_status();
}
int gca_cast_f16(const float* x, int64_t rows, int64_t row_elems, int64_t src_row_stride, void* y, void* stream) {
  if (!y || !x || rows <= 0 || rows > 65535 || row_elems <= 0 || row_elems % 4 || src_row_stride < row_elems ||
      src_row_stride % 4 || ((uintptr_t)x % 16) || ((uintptr_t)y % 8))
    return GCA_EINVAL;
  const long long re4 = row_elems / 4;
  const unsigned bx = (unsigned)(re4 / 256 + 1 < 4096 ? re4 / 256 + 1 : 4096);
  hipLaunchKernelGGL(cast_f16_kernel, dim3(bx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, re4,
                     (long long)src_row_stride, (gca_half*)y);
  return gca_launch_status();
}
int gca_scale(float* y, int64_t n, float a, void* stream) {
  if (!y || n <= 0) return GCA_EINVAL;
  hipLaunchKernelGGL(scale_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, y, (long long)n, a);
  return gca_launch_status();
}
int gca_gather_rows(const float* src, const int64_t* idx, int64_t rows, int64_t row_elems, int64_t src_row_stride,
                    float* dst, void* stream) {
  if (!src || !idx || !dst || rows <= 0 || rows > 65535 || row_elems <= 0 || src_row_stride < row_elems) return GCA_EINVAL;
  const bool v4 = row_elems % 4 == 0 && src_row_stride % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
  const long long per = v4 ? row_elems / 4 : row_elems;
  long long bx = gca_ceil_div(per, 256 * 4);
  if (bx < 1) bx = 1;
  if (bx > 1024) bx = 1024;
  const dim3 grid((unsigned)bx, (unsigned)rows);
  if (v4) hipLaunchKernelGGL(gather_rows_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src, (const long long*)idx,
                             (long long)row_elems, (long long)src_row_stride, dst);
  else hipLaunchKernelGGL(gather_rows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, (const long long*)idx,
                          (long long)row_elems, (long long)src_row_stride, dst);
  return gca_launch_status();
}

}  // extern "C"
