// Device-side contrastive augmentations: uint8 source frames + one parameter record per (clip, view) -> normalised NCDHW clips.
//
// The reference's contrastive chain (lib/data/transform/build.py:45-62) runs on the host through cv2 / albumentations:
//   VideoRandomResizedCrop -> ColorJitter (p 0.8) -> GrayScale (p 0.2) -> GaussianBlur (p 0.5) -> HorizontalFlip -> Normalize
//   -> ToTensor  (lib/data/transform/consistency_transforms.py:81-145, 226-340).
// gca_clip_prepare (input.hip) takes over the last three stages; this file takes the whole chain.  The arithmetic is fixed by
// tests/augment_ref.py, NOT by cv2 (not available to check against): every stage maps uint8 -> uint8 in integer / fixed-point
// arithmetic or in fp32 with one rounding per written operation, and whatever needs exp / log / a floating division arrives
// from the host as data (resize taps, look-up tables, 1 - factor, blur weights, the HSV division tables).  Floating-point
// contraction is OFF for this whole file: a fused multiply-add would drop a rounding the specification counts.
//
// Two launches.  Contrast blends every pixel with the frame's mean gray AFTER the jitter ops that precede it, so a first
// kernel recomputes resize + those ops and adds the gray values of each frame into one 32-bit integer (integer atomics: any
// order gives the same bits); frames whose record has no contrast op leave at once, and the launch is skipped when no record
// has one.  The main kernel gives a workgroup one 16 x 64 tile of one output frame: tile + blur halo after resize / jitter /
// gray as uint8 planes in LDS (the halo is looked up through reflect-101, so the image border costs nothing special),
// horizontal blur pass LDS -> LDS, vertical pass in registers, then flip + normalise + store as gca_clip_prepare does (four
// columns per thread, 16-byte stores when W % 4 == 0).  A record without blur has no halo and skips both blur passes.
#pragma clang fp contract(off)
#include "gca_common.h"

namespace {

constexpr int REC = 24;            // int32 words per (clip, view) record; layout in include/gca_hip.h
constexpr int TH = 16, TW = 64;    // output tile of a workgroup (256 threads: 16 rows x 16 four-column groups)
constexpr int RMAX = 3;            // blur radius of k = 7
constexpr int AW = TW + 2 * RMAX + 2;   // LDS row pitch of the halo planes
constexpr int TAP_SHIFT = 11, BLUR_SHIFT = 12, HSV_SHIFT = 12;

struct AugParams {
  int views, T, Hs, Ws, H, W;
  int tiles_x;
  float inv_n;                     // f32(1) / f32(H * W)
  float m[3], d[3];
};

struct Tap { short i0, i1, c0, c1; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int gray_of(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return clampi(i, 0, n - 1);      // (radius < n is checked by the entry; the clamp only keeps a bad call inside the plane)
}

// Bilinear sample of output pixel (y, x): horizontal blend of two source rows, vertical blend, one rounding shift.
__device__ __forceinline__ void resized_px(const unsigned char* __restrict__ frame, const AugParams& p, const Tap* __restrict__ taps,
                                           int y, int x, int px[3]) {
  const Tap a = taps[y], c = taps[p.H + x];
  // (indices are clamped into the frame: a bad table can mis-sample, never read outside the buffer)
  const unsigned char* r0 = frame + (long long)clampi(a.i0, 0, p.Hs - 1) * p.Ws * 3;
  const unsigned char* r1 = frame + (long long)clampi(a.i1, 0, p.Hs - 1) * p.Ws * 3;
  const int j0 = clampi(c.i0, 0, p.Ws - 1) * 3, j1 = clampi(c.i1, 0, p.Ws - 1) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int top = c.c0 * r0[j0 + ch] + c.c1 * r0[j1 + ch];
    const int bot = c.c0 * r1[j0 + ch] + c.c1 * r1[j1 + ch];
    px[ch] = clampi((a.c0 * top + a.c1 * bot + (1 << (2 * TAP_SHIFT - 1))) >> (2 * TAP_SHIFT), 0, 255);
  }
}

__device__ __forceinline__ void hue_px(int px[3], const unsigned char* __restrict__ lut, const int* __restrict__ divtab) {
  const int r = px[0], g = px[1], b = px[2];
  const int v = max(max(r, g), b), diff = v - min(min(r, g), b);
  const int s = (diff * divtab[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * divtab[256 + diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT;       // arithmetic shift: floor for negative h
  if (h < 0) h += 180;
  h = lut[clampi(h, 0, 255)];
  const int sec = h / 30, f = h - 30 * sec;
  const int pp = (v * (255 - s) + 127) / 255;
  const int q = (v * (7650 - s * f) + 3825) / 7650;
  const int t = (v * (7650 - s * (30 - f)) + 3825) / 7650;
  switch (sec) {
    case 0: px[0] = v; px[1] = t; px[2] = pp; break;
    case 1: px[0] = q; px[1] = v; px[2] = pp; break;
    case 2: px[0] = pp; px[1] = v; px[2] = t; break;
    case 3: px[0] = pp; px[1] = q; px[2] = v; break;
    case 4: px[0] = t; px[1] = pp; px[2] = v; break;
    default: px[0] = v; px[1] = pp; px[2] = q; break;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) px[ch] = clampi(px[ch], 0, 255);           // (no-op for s <= 255; a bound for what follows)
}

// The jitter ops of a record in its order.  UPTO_CONTRAST: stop in front of the contrast op (the reduction pass).
// contrast_off = mean gray * (1 - f_c) of this frame.
template <bool UPTO_CONTRAST>
__device__ __forceinline__ void jitter_px(int px[3], const int* __restrict__ rec, const unsigned char* __restrict__ luts,
                                          const int* __restrict__ divtab, float contrast_off) {
  const int mask = rec[11];
  for (int j = 0; j < 4; ++j) {
    const int op = rec[7 + j] & 3;
    if (!((mask >> op) & 1)) continue;
    if (op == 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) px[ch] = luts[px[ch]];
    } else if (op == 1) {
      if (UPTO_CONTRAST) return;
      const float f = __int_as_float(rec[12]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float y = (float)px[ch] * f;                   // one rounding
        const float z = y + contrast_off;                    // one rounding
        px[ch] = (int)fminf(fmaxf(z, 0.f), 255.f);           // clamp, truncate
      }
    } else if (op == 2) {
      const float f = __int_as_float(rec[14]), omf = __int_as_float(rec[15]);
      const float g = (float)gray_of(px[0], px[1], px[2]) * omf;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float y = (float)px[ch] * f;
        const float z = y + g;
        px[ch] = (int)fminf(fmaxf(rintf(z), 0.f), 255.f);    // round half to even, clamp
      }
    } else {
      hue_px(px, luts + 256, divtab);
    }
  }
}

// Reduction pass: grid (frames, ceil(H * W / 256)); sums[frame] += gray of every pixel as the contrast op will see it.
__global__ __launch_bounds__(256) void augment_gray_sum_kernel(const unsigned char* __restrict__ frames,
                                                               const int* __restrict__ records, const Tap* __restrict__ taps,
                                                               const unsigned char* __restrict__ luts,
                                                               const int* __restrict__ divtab, unsigned* __restrict__ sums,
                                                               const AugParams p) {
  const long long fr = blockIdx.x;
  const long long nv = blockIdx.x / (unsigned)p.T;
  const int* rec = records + nv * REC;
  if (!((rec[11] >> 1) & 1)) return;                          // no contrast op in this record (uniform over the block)
  const int i = blockIdx.y * 256 + threadIdx.x;
  int g = 0;
  if (i < p.H * p.W) {
    int px[3];
    resized_px(frames + fr * ((long long)p.Hs * p.Ws * 3), p, taps + nv * (p.H + p.W), i / p.W, i % p.W, px);
    jitter_px<true>(px, rec, luts + nv * 512, divtab, 0.f);
    g = gray_of(px[0], px[1], px[2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(sums + fr, (unsigned)g);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void augment_main_kernel(const unsigned char* __restrict__ frames,
                                                           const int* __restrict__ records, const Tap* __restrict__ taps,
                                                           const unsigned char* __restrict__ luts,
                                                           const int* __restrict__ divtab, const unsigned* __restrict__ sums,
                                                           T* __restrict__ out, const AugParams p) {
  __shared__ unsigned char A[3][TH + 2 * RMAX][AW];           // tile + halo after resize / jitter / gray
  __shared__ unsigned char B[3][TH + 2 * RMAX][TW];           // after the horizontal blur pass
  const long long fr = blockIdx.x;
  const long long nv = blockIdx.x / (unsigned)p.T;
  const int t = (int)(fr - nv * p.T);
  const int* rec = records + nv * REC;
  const int ty0 = ((int)blockIdx.y / p.tiles_x) * TH, tx0 = ((int)blockIdx.y % p.tiles_x) * TW;
  const int th = min(TH, p.H - ty0), tw = min(TW, p.W - tx0);
  int k = rec[6];
  if (k != 3 && k != 5 && k != 7) k = 0;                      // (the entry checks the host copy; this bounds the LDS indices)
  const int R = k >> 1, flip = rec[4], gray = rec[5], mask = rec[11];
  const unsigned char* frame = frames + fr * ((long long)p.Hs * p.Ws * 3);
  const Tap* tp = taps + nv * (p.H + p.W);
  const unsigned char* lut = luts + nv * 512;
  float contrast_off = 0.f;
  if ((mask >> 1) & 1) {
    const float mean = (float)sums[fr] * p.inv_n;             // exact integer sum -> fp32 (one rounding), times f32(1 / n)
    contrast_off = mean * __int_as_float(rec[13]);
  }
  // ---- tile + halo -> A
  const int rows = th + 2 * R, cols = tw + 2 * R;
  for (int i = threadIdx.x; i < rows * cols; i += 256) {
    const int ry = i / cols, rx = i - ry * cols;
    int px[3];
    resized_px(frame, p, tp, reflect101(ty0 - R + ry, p.H), reflect101(tx0 - R + rx, p.W), px);
    if (mask) jitter_px<false>(px, rec, lut, divtab, contrast_off);
    if (gray) px[0] = px[1] = px[2] = gray_of(px[0], px[1], px[2]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) A[ch][ry][rx] = (unsigned char)px[ch];
  }
  __syncthreads();
  int w[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) w[i] = rec[16 + i];
  // ---- horizontal blur pass A -> B (rows keep their vertical halo)
  if (k) {
    for (int i = threadIdx.x; i < rows * tw; i += 256) {
      const int ry = i / tw, x = i - ry * tw;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        int acc = 1 << (BLUR_SHIFT - 1);
#pragma unroll
        for (int j = 0; j < 7; ++j)
          if (j < k) acc += w[j] * A[ch][ry][x + j];
        B[ch][ry][x] = (unsigned char)clampi(acc >> BLUR_SHIFT, 0, 255);
      }
    }
    __syncthreads();
  }
  // ---- vertical pass, flip, normalise, store: thread = (row, four columns), as gca_clip_prepare
  const int y = threadIdx.x >> 4, xq = (threadIdx.x & 15) * 4;
  if (y >= th || xq >= tw) return;
  const int nw = min(4, tw - xq);
  const long long plane = (long long)p.T * p.H * p.W;
  T* o = out + nv * 3 * plane + ((long long)t * p.H + (ty0 + y)) * p.W;
  const int x = tx0 + xq;                                     // first of this thread's columns, before the flip
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = xq + (j < nw ? j : 0);
      int q;
      if (k) {
        int acc = 1 << (BLUR_SHIFT - 1);
#pragma unroll
        for (int i = 0; i < 7; ++i)
          if (i < k) acc += w[i] * B[ch][y + i][xx];
        q = clampi(acc >> BLUR_SHIFT, 0, 255);
      } else {
        q = A[ch][y][xx];
      }
      const float s = (float)q - p.m[ch];                      // img -= mean   (one rounding)
      v[j] = s * p.d[ch];                                      // img *= 1/std  (one rounding)
    }
    T* oc = o + ch * plane;
    if (VEC) {
      if (flip) gca_act<T>::st4(oc + (p.W - 4 - x), make_float4(v[3], v[2], v[1], v[0]));
      else gca_act<T>::st4(oc + x, make_float4(v[0], v[1], v[2], v[3]));
    } else {
      for (int j = 0; j < nw; ++j) gca_act<T>::st(oc + (flip ? p.W - 1 - (x + j) : x + j), v[j]);
    }
  }
}

}  // namespace

extern "C" {

int64_t gca_clip_augment_ws_bytes(int64_t b, int64_t views, int64_t T) {
  if (b <= 0 || views <= 0 || T <= 0) return 0;
  return b * views * T * (int64_t)sizeof(unsigned);
}

int gca_clip_augment(const uint8_t* frames, int64_t b, int64_t views, int64_t T, int64_t Hs, int64_t Ws,
                     const int32_t* records_host, const int32_t* records, const int16_t* taps, const uint8_t* luts,
                     const int32_t* divtab, const float* mean255, const float* inv_std255, int64_t H, int64_t W,
                     void* out, int out_f16, void* ws, void* stream) {
  if (!frames || !records_host || !records || !taps || !luts || !divtab || !mean255 || !inv_std255 || !out || !ws || b <= 0 ||
      views <= 0 || views > 8 || T <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Hs > 32767 || Ws > 32767 || H > 32767 ||
      W > 32767 || T > 32767 || H * W > (1 << 23) || ((uintptr_t)taps % 8) != 0 || ((uintptr_t)records % 4) != 0 ||
      ((uintptr_t)ws % 4) != 0)
    return GCA_EINVAL;
  const int64_t frames_total = b * views * T;
  const int64_t tiles_x = gca_ceil_div(W, TW), tiles = tiles_x * gca_ceil_div(H, TH);
  if (frames_total > 0x7fffffffLL || tiles > 65535) return GCA_EINVAL;
  bool any_contrast = false;
  for (int64_t i = 0; i < b * views; ++i) {
    const int32_t* r = records_host + i * REC;
    const int k = r[6];
    if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || (int64_t)r[0] + r[2] > Hs || (int64_t)r[1] + r[3] > Ws) return GCA_EINVAL;
    if ((r[4] | r[5]) & ~1) return GCA_EINVAL;
    if (k != 0 && k != 3 && k != 5 && k != 7) return GCA_EINVAL;
    if (k / 2 >= H || k / 2 >= W) return GCA_EINVAL;          // reflect-101 needs radius < size
    int seen = 0;
    for (int j = 0; j < 4; ++j) {
      if (r[7 + j] < 0 || r[7 + j] > 3) return GCA_EINVAL;
      seen |= 1 << r[7 + j];
    }
    if (seen != 15 || (r[11] & ~15)) return GCA_EINVAL;
    int64_t wsum = 0;
    for (int j = 0; j < 7; ++j) {
      if (r[16 + j] < 0 || (j >= k && r[16 + j] != 0)) return GCA_EINVAL;
      wsum += r[16 + j];
    }
    if (k && wsum != (1 << BLUR_SHIFT)) return GCA_EINVAL;
    any_contrast = any_contrast || ((r[11] >> 1) & 1);
  }
  AugParams p;
  p.views = (int)views; p.T = (int)T; p.Hs = (int)Hs; p.Ws = (int)Ws; p.H = (int)H; p.W = (int)W;
  p.tiles_x = (int)tiles_x;
  p.inv_n = 1.0f / (float)(H * W);
  for (int c = 0; c < 3; ++c) { p.m[c] = mean255[c]; p.d[c] = inv_std255[c]; }      // HOST pointers: six floats by value
  hipStream_t st = (hipStream_t)stream;
  const Tap* tp = reinterpret_cast<const Tap*>(taps);
  unsigned* sums = (unsigned*)ws;
  if (any_contrast) {
    if (hipMemsetAsync(sums, 0, (size_t)frames_total * sizeof(unsigned), st) != hipSuccess) return GCA_ELAUNCH;
    const dim3 g1((unsigned)frames_total, (unsigned)gca_ceil_div(H * W, 256));
    hipLaunchKernelGGL(augment_gray_sum_kernel, g1, dim3(256), 0, st, frames, records, tp, luts, divtab, sums, p);
  }
  const bool vec = W % 4 == 0 && ((uintptr_t)out % 16) == 0;
  const dim3 grid((unsigned)frames_total, (unsigned)tiles);
  if (out_f16) {
    if (vec) hipLaunchKernelGGL((augment_main_kernel<gca_half, true>), grid, dim3(256), 0, st, frames, records, tp, luts, divtab, sums, (gca_half*)out, p);
    else hipLaunchKernelGGL((augment_main_kernel<gca_half, false>), grid, dim3(256), 0, st, frames, records, tp, luts, divtab, sums, (gca_half*)out, p);
  } else {
    if (vec) hipLaunchKernelGGL((augment_main_kernel<float, true>), grid, dim3(256), 0, st, frames, records, tp, luts, divtab, sums, (float*)out, p);
    else hipLaunchKernelGGL((augment_main_kernel<float, false>), grid, dim3(256), 0, st, frames, records, tp, luts, divtab, sums, (float*)out, p);
  }
  return gca_launch_status();
}

}  // extern "C"
