// Downstream (action-recognition) input stage: many views of ONE decoded uint8 source per video -> normalised NCDHW clips.
//
// The reference builds its fine-tuning and test samples on the host:
//   training  VideoMultiScaleCrop -> VideoRandomHorizontalFlip -> VideoNormalize -> VideoToTensor
//             (lib/data/transform/build.py:27-35, consistency_transforms.py:366-468)
//   testing   VideoResize(scale_size) -> VideoCenterCrop | VideoFullResSample (3 crops) | VideoOverSampleCrop (5 / 10 crops)
//             -> VideoNormalize -> VideoToTensor  (tools/test_ds.py:95-120, consistency_transforms.py:159-170, 341-349, 470-551)
// and ships every finished fp32 view over PCIe: 100 views of one video at test_clips = test_crops = 10.  All of those views
// are windows of ONE resized copy of the video's frames, and a crop of a resized uint8 frame is a window of the resize's tap
// table.  So the host ships the source once plus a table, and every view names (source, first frame, table, window origin,
// flip) in an 8-word record.  gca_clip_augment (augment.hip) cannot do that: it wants a private copy of the frames per view.
//
// The arithmetic is tests/views_ref.py's, which is tests/augment_ref.py's resize (horizontal blend of two source rows,
// vertical blend, ONE rounding shift to uint8) followed by (float(px) - m_c) * d_c with two fp32 roundings.  Floating-point
// contraction is OFF for this file, as in augment.hip.
//
// One launch.  Write-bound: 12 B stored per output pixel, the uint8 reads come out of the caches (a source frame is read by
// every view of it).  A workgroup owns a 16 x 64 tile of one output frame of one view: grid.x = tiles (x the fold of
// n_views above the grid-z limit), grid.y = t, grid.z = view, so nothing is divided per thread.  A thread produces four
// consecutive x of one row for the three channels: three 16-byte stores, coalesced along x; the record and the row tap are
// the same for the 16 threads of a tile row and are loaded once per thread, the flip reverses the column-tap lookup and never
// the store order.  Rows that are no multiple of four wide (or an output that is not 16-byte aligned) store scalars.
#pragma clang fp contract(off)
#include "gca_common.h"

namespace {

constexpr int REC = 8;             // int32 words per view record: src, t0, tab, oy, ox, flip, 0, 0 (include/gca_hip.h)
constexpr int TH = 16, TW = 64;    // output tile of a workgroup (256 threads: 16 rows x 16 four-column groups)
constexpr int TAP_SHIFT = 11;
constexpr unsigned GRID_Z = 65535; // views per grid.z sweep; the rest folds into grid.x

struct ViewParams {
  int n_src, F, Hs, Ws, n_views, n_tab, Lh, Lw, T, H, W;
  int tiles_x, tiles;              // tiles of one output frame
  float m[3], d[3];
};

struct Tap { short i0, i1, c0, c1; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <bool VEC>
__global__ __launch_bounds__(256) void clip_views_kernel(const unsigned char* __restrict__ frames,
                                                         const int* __restrict__ records, const Tap* __restrict__ taps,
                                                         float* __restrict__ out, const ViewParams p) {
  // ---- workgroup-uniform: which view, which frame, which tile
  unsigned tile = blockIdx.x, hi = 0;
  if (gridDim.x != (unsigned)p.tiles) {                        // n_views > GRID_Z (one 32-bit division, on uniform values)
    hi = blockIdx.x / (unsigned)p.tiles;
    tile = blockIdx.x - hi * (unsigned)p.tiles;
  }
  const long long view = (long long)hi * GRID_Z + blockIdx.z;
  if (view >= p.n_views) return;
  const int t = blockIdx.y;
  const int* rec = records + view * REC;
  // (every word is clamped: the entry validates the HOST copy of the records; whatever the device copy and the tap table
  // hold, no address leaves its buffer -- a bad table can mis-sample, never read or write outside)
  const int src = clampi(rec[0], 0, p.n_src - 1), fr = clampi(rec[1] + t, 0, p.F - 1), tab = clampi(rec[2], 0, p.n_tab - 1);
  const int oy = rec[3], ox = rec[4], flip = rec[5] & 1;
  const int ty = (int)(tile / (unsigned)p.tiles_x), tx = (int)tile - ty * p.tiles_x;
  // ---- thread: one row, four columns
  const int y = ty * TH + (int)(threadIdx.x >> 4), x = tx * TW + (int)(threadIdx.x & 15) * 4;
  if (y >= p.H || x >= p.W) return;
  const int nw = min(4, p.W - x);
  const Tap* tp = taps + (long long)tab * (p.Lh + p.Lw);
  const Tap a = tp[clampi(oy + y, 0, p.Lh - 1)];
  const unsigned char* frame = frames + ((long long)src * p.F + fr) * ((long long)p.Hs * p.Ws * 3);
  const unsigned char* r0 = frame + (long long)clampi(a.i0, 0, p.Hs - 1) * p.Ws * 3;
  const unsigned char* r1 = frame + (long long)clampi(a.i1, 0, p.Hs - 1) * p.Ws * 3;
  float v[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xx = x + (j < nw ? j : 0);                       // (a column past the row repeats the first: computed, never stored)
    const Tap c = tp[p.Lh + clampi(ox + (flip ? p.W - 1 - xx : xx), 0, p.Lw - 1)];
    const int j0 = clampi(c.i0, 0, p.Ws - 1) * 3, j1 = clampi(c.i1, 0, p.Ws - 1) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int top = c.c0 * r0[j0 + ch] + c.c1 * r0[j1 + ch];
      const int bot = c.c0 * r1[j0 + ch] + c.c1 * r1[j1 + ch];
      const int q = clampi((a.c0 * top + a.c1 * bot + (1 << (2 * TAP_SHIFT - 1))) >> (2 * TAP_SHIFT), 0, 255);
      const float s = (float)q - p.m[ch];                      // img -= mean   (one rounding)
      v[ch][j] = s * p.d[ch];                                  // img *= 1/std  (one rounding)
    }
  }
  const long long plane = (long long)p.T * p.H * p.W;
  float* o = out + view * 3 * plane + ((long long)t * p.H + y) * p.W + x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* oc = o + ch * plane;
    if (VEC) {
      *reinterpret_cast<float4*>(oc) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
    } else {
      for (int j = 0; j < nw; ++j) oc[j] = v[ch][j];
    }
  }
}

}  // namespace

extern "C" {

int gca_clip_views(const uint8_t* frames, int64_t n_src, int64_t F, int64_t Hs, int64_t Ws, const int32_t* records_host,
                   const int32_t* records, int64_t n_views, const int16_t* taps, int64_t n_tab, int64_t Lh, int64_t Lw,
                   const float* mean255, const float* inv_std255, int64_t T, int64_t H, int64_t W, float* out, void* stream) {
  const int64_t LIM = 0x7fffffffLL;
  if (n_src < 1 || F < 1 || Hs < 1 || Ws < 1 || n_views < 0 || n_tab < 1 || Lh < 1 || Lw < 1 || T < 1 || H < 1 || W < 1)
    return GCA_EINVAL;
  // every factor is bounded before a product is formed, so no product below overflows 64 bits
  if (n_src > LIM || F > LIM || Hs > 32767 || Ws > 32767 || n_views > LIM || n_tab > LIM || Lh > LIM || Lw > LIM || T > 65535 ||
      H > LIM || W > LIM)
    return GCA_EINVAL;                                         // (taps are int16: Hs, Ws <= 32767; T is grid.y)
  if (H > Lh || W > Lw || T > F) return GCA_EINVAL;
  if (n_src * F > LIM || n_src * F * Hs * Ws * 3 > LIM) return GCA_EINVAL;            // frames: < 2^31 elements
  if (n_tab * (Lh + Lw) > LIM || n_tab * (Lh + Lw) * 4 > LIM) return GCA_EINVAL;      // taps
  if (n_views * REC > LIM) return GCA_EINVAL;                                          // records
  if (T * H > LIM || T * H * W > LIM || n_views * 3 > LIM || n_views * 3 * (T * H * W) > LIM) return GCA_EINVAL;   // out
  if (n_views == 0) return GCA_OK;                             // nothing to do, nothing launched
  if (!frames || !records_host || !records || !taps || !mean255 || !inv_std255 || !out || ((uintptr_t)taps % 8) != 0 ||
      ((uintptr_t)records % 4) != 0 || ((uintptr_t)out % 4) != 0)
    return GCA_EINVAL;
  for (int64_t i = 0; i < n_views; ++i) {
    const int32_t* r = records_host + i * REC;
    if (r[0] < 0 || r[0] >= n_src || r[2] < 0 || r[2] >= n_tab) return GCA_EINVAL;
    if (r[1] < 0 || (int64_t)r[1] + T > F) return GCA_EINVAL;
    if (r[3] < 0 || (int64_t)r[3] + H > Lh || r[4] < 0 || (int64_t)r[4] + W > Lw) return GCA_EINVAL;
    if (r[5] & ~1) return GCA_EINVAL;
  }
  ViewParams p;
  p.n_src = (int)n_src; p.F = (int)F; p.Hs = (int)Hs; p.Ws = (int)Ws; p.n_views = (int)n_views; p.n_tab = (int)n_tab;
  p.Lh = (int)Lh; p.Lw = (int)Lw; p.T = (int)T; p.H = (int)H; p.W = (int)W;
  const int64_t tiles_x = gca_ceil_div(W, TW), tiles = tiles_x * gca_ceil_div(H, TH);
  const int64_t gz = n_views < (int64_t)GRID_Z ? n_views : (int64_t)GRID_Z, fold = gca_ceil_div(n_views, gz);
  if (tiles * fold * 256 > 0xffffffffLL) return GCA_EINVAL;      // grid.x * 256 threads must fit 32 bits
  p.tiles_x = (int)tiles_x; p.tiles = (int)tiles;
  for (int c = 0; c < 3; ++c) { p.m[c] = mean255[c]; p.d[c] = inv_std255[c]; }      // HOST pointers: six floats by value
  const bool vec = W % 4 == 0 && ((uintptr_t)out % 16) == 0;
  const dim3 grid((unsigned)(tiles * fold), (unsigned)T, (unsigned)gz);
  hipStream_t st = (hipStream_t)stream;
  const Tap* tp = reinterpret_cast<const Tap*>(taps);
  if (vec) hipLaunchKernelGGL(clip_views_kernel<true>, grid, dim3(256), 0, st, frames, records, tp, out, p);
  else hipLaunchKernelGGL(clip_views_kernel<false>, grid, dim3(256), 0, st, frames, records, tp, out, p);
  return gca_launch_status();
}

}  // extern "C"
