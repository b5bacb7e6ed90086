// Shared by conv3d.hip (forward / dgrad implicit GEMM) and conv3d_wgrad.hip.
#pragma once
#include "gca_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

namespace gca_conv {

// Conv arithmetic (include/gca_hip.h, gca_set_conv_math): 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = bf16x3, 2 = bf16x6:
// fp32 operands split in the kernel into 2 / 3 bf16 parts, products on v_mfma_f32_32x32x16_bf16, fp32 accumulation.
// Defined in conv3d.hip (gca_set_conv_math / GCA_CONV_MATH).
int conv_math();
constexpr int math_parts(int math) { return math == 2 ? 3 : (math == 3 ? 1 : 2); }   // 16-bit parts per operand element (3 = fp16 storage: the element itself)
// arithmetic of one pass: the tune_*_math override (1 + m) when m is at least as accurate as the mode in force
inline int math_rank(int m) { return m == 0 ? 2 : m == 2 ? 1 : 0; }     // f32 > bf16x6 > bf16x3
// act_f16: the activations of this convolution are fp16 in HBM (gca_conv_geom.act_f16) -> arithmetic 3: v_mfma_f32_32x32x16_f16
// on the stored halves and on the weights rounded to fp16 (RNE) where they become an MFMA operand; nothing to pin
inline int resolve_math(int tune_math, int act_f16 = 0) {
  const int mode = conv_math();
  if (act_f16) return 3;
  if (tune_math >= 1 && tune_math <= 3 && math_rank(tune_math - 1) >= math_rank(mode)) return tune_math - 1;
  return mode;
}

// (x0, x1) -> packed bf16 pairs hi = bf16(x) and lo = bf16(x - hi)  (round to nearest even, v_cvt_pk_bf16_f32)
__device__ __forceinline__ void split_bf16x2(float x0, float x1, unsigned& hi, unsigned& lo) {
  const f32x2 v = {x0, x1};
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 r = {x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
}
// three parts: x = hi + mid + lo up to 2^-27 |x| (both residuals are exact in fp32)
__device__ __forceinline__ void split_bf16x3(float x0, float x1, unsigned& hi, unsigned& mid, unsigned& lo) {
  const f32x2 v = {x0, x1};
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 r = {x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u)};
  mid = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
  const f32x2 r2 = {r.x - __uint_as_float(mid << 16), r.y - __uint_as_float(mid & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}

constexpr int BK = 16;          // GEMM-K tile of the forward/dgrad kernels
constexpr int WBK = 32;         // GEMM-K (spatial) tile of the wgrad kernel
constexpr int MPAD = 64;        // packed weights: M padded to this
constexpr int TABLE_PAD_W = 192;   // widest wgrad tile: the table holds this many invalid rows past C*taps
constexpr int FAST_MAX_TAPS = 62;
constexpr int NUM_CU = 256;

// row table entry: x = offset of the row's (channel, tap) inside one image of the gathered tensor (BYTES for the
// forward/dgrad tables, elements for the wgrad table); y = tap6 | valid<<6 | dd<<8 | dh<<16 | dw<<24 (signed
// bytes).  The tap id sits in the low bits so that v_bfe_i32(mask, y, 1) tests its validity bit directly.
__device__ __forceinline__ void decode_row(int2 e, int& off, int& dd, int& dh, int& dw, int& valid) {
  off = e.x;
  dd = (e.y << 16) >> 24;
  dh = (e.y << 8) >> 24;
  dw = e.y >> 24;
  valid = (e.y >> 6) & 1;
}
inline int pack_row_meta(int dd, int dh, int dw, int valid, int tap6) {
  return (tap6 & 63) | ((valid & 1) << 6) | ((dd & 0xff) << 8) | ((dh & 0xff) << 16) | (int)((unsigned)(dw & 0xff) << 24);
}

// Sum over the 32 lanes of each wave half with DPP adds (no LDS traffic).  The total lands in lanes 16..31 of
// the lower half and 48..63 of the upper half (row_bcast15 feeds rows 1 and 3).
__device__ __forceinline__ float half_wave_sum_hi(float v) {
#define GCA_DPP(x, ctrl, rmask) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (ctrl), (rmask), 0xf, false))
  v += GCA_DPP(v, 0xB1, 0xf);     // quad_perm [1,0,3,2]
  v += GCA_DPP(v, 0x4E, 0xf);     // quad_perm [2,3,0,1]
  v += GCA_DPP(v, 0x141, 0xf);    // row_half_mirror
  v += GCA_DPP(v, 0x140, 0xf);    // row_mirror   -> every lane of a 16-lane row holds the row total
  v += GCA_DPP(v, 0x142, 0xa);    // row_bcast15 into rows 1 and 3
#undef GCA_DPP
  return v;
}

// Byte ranges of buffer resources are 32-bit: a range past BUF_MAX_BYTES is clamped to it, or refused where the whole range
// must be addressable -- geom_ok refuses an activation tensor larger than this, so for x, y, dy and dx the clamp never cuts.
constexpr long long BUF_MAX_BYTES = 0xfffff000LL;
inline unsigned clamp_buf_bytes(long long b) { return b > BUF_MAX_BYTES ? (unsigned)BUF_MAX_BYTES : (unsigned)b; }

inline bool geom_ok(const gca_conv_geom* g) {
  if (!g) return false;
  if (g->N <= 0 || g->C <= 0 || g->D <= 0 || g->H <= 0 || g->W <= 0 || g->K <= 0) return false;
  if (g->kd <= 0 || g->kh <= 0 || g->kw <= 0 || g->sd <= 0 || g->sh <= 0 || g->sw <= 0) return false;
  if (g->pd < 0 || g->ph < 0 || g->pw < 0) return false;
  if (g->kd > 127 || g->kh > 127 || g->kw > 127) return false;
  const int od = (g->D + 2 * g->pd - g->kd) / g->sd + 1;
  const int oh = (g->H + 2 * g->ph - g->kh) / g->sh + 1;
  const int ow = (g->W + 2 * g->pw - g->kw) / g->sw + 1;
  if (od != g->OD || oh != g->OH || ow != g->OW || od <= 0 || oh <= 0 || ow <= 0) return false;
  // the kernels address both tensors with 32-bit byte offsets from their base, through buffer resources whose byte range
  // ends at BUF_MAX_BYTES at the latest: < 2^30 elements each, and no more than BUF_MAX_BYTES bytes (2^30 - 1024 fp32
  // elements) -- a larger tensor would read its tail as zeros and drop the stores to it
  const long long cdhw = (long long)g->C * g->D * g->H * g->W;
  if (g->x_batch_stride != 0 && g->x_batch_stride < cdhw) return false;
  const long long in_elems = (long long)g->N * (g->x_batch_stride ? g->x_batch_stride : cdhw);
  const long long out_elems = (long long)g->N * g->K * od * oh * ow;
  if (in_elems >= (1LL << 30) || out_elems >= (1LL << 30)) return false;
  const long long es = g->act_f16 == 1 ? 2 : 4;
  if (in_elems * es > BUF_MAX_BYTES || out_elems * es > BUF_MAX_BYTES) return false;
  for (int v : {g->tune_fwd_bm, g->tune_dgrad_bm}) if (v != 0 && !((v & 1023) % 32 == 0 && (v & 1023) >= 32 && (v & 1023) <= 160 && ((v >> 10) <= 2 || (v >> 10) == 4 || (v >> 10) == 8))) return false;   // | 1024 float4 gathers, | 2048 LDS halo, | 4096 stem, | 8192 pointwise fp16 GEMM
  for (int v : {g->tune_fwd_box, g->tune_dgrad_box}) if (v < 0 || v > 0xffffff) return false;
  if (g->act_f16 != 0 && g->act_f16 != 1) return false;
  for (int v : {g->tune_fwd_splits, g->tune_dgrad_splits, g->tune_wgrad_splits}) if (v < 0 || v > 1024) return false;
  if (g->tune_wgrad_tile < 0 || g->tune_wgrad_tile > 14) return false;     // 1..10 tile shapes of conv_wgrad_kernel, 11 / 12 the streaming temporal kernel, 13 the streaming (1,3,3) kernel, 14 the stem kernel
  for (int v : {g->tune_fwd_math, g->tune_dgrad_math, g->tune_wgrad_math}) if (v < 0 || v > 3) return false;
  for (int v : {g->tune_fwd_tail, g->tune_dgrad_tail}) if (v < 0 || (v != 0 && ((v & 255) < 1 || (v & 255) > 4))) return false;
  return true;
}

inline int taps(const gca_conv_geom* g) { return g->kd * g->kh * g->kw; }

// ---- weight gradient (conv3d_wgrad*.hip) --------------------------------------------------------------------------------
// Parameter blocks of the weight-gradient kernels.  Each kernel file takes its block by a derived type of its own
// (WgradParams, TsParams, SsParams, StwParams: those names are part of the kernel symbols).

struct WgradArgs {               // conv3d_wgrad.hip: the gather kernel
  int C, D, H, W, K, OD, OH, OW;
  int kd, kh, kw;
  int sd, sh, sw, pd, ph, pw;
  int Kred;                 // C*taps  (GEMM N)
  int tilesM, tilesN, splits;
  int kt_per_split, kt_total;
  int chk;
  int math;                 // arithmetic of this launch (host side only)
  int half;                 // x and dy are fp16 in HBM (host side only)
  unsigned Ktot;            // NB*OD*OH*OW (GEMM K) -- < 2^30
  unsigned x_nstride;       // elements between clips of x
  unsigned x_bytes, dy_bytes, slab_bytes;
  gca_magic m_osp, m_ohw, m_ow;
};

struct TsArgs {                  // conv3d_wgrad_ts.hip: the streaming temporal kernel
  int K, C, D, OD, HW, pd;
  int Kred;                      // C * KD
  int tilesM, tilesC, splits;
  int units, units_per_split;    // unit = (clip, chunk of 16 positions)
  int chunks;                    // HW / 16
  int S;                         // steps per unit, padded to a multiple of KD
  unsigned x_nstride, dy_nstride;   // elements between clips
  unsigned x_bytes, dy_bytes, slab_bytes;
  gca_magic m_chunks;
  // optional input transform: x stands for relu(x * in_scale[c] + in_shift[c]) (the producer's BatchNorm + ReLU, never
  // materialised); a lane's fragment row IS a channel, so the pair sits in two registers for the whole kernel
  const float* in_scale;
  const float* in_shift;
};

struct SsArgs {                  // conv3d_wgrad_ts.hip: the streaming (1,3,3) kernel
  int K, C, D, H, W;
  int Kred;                      // C * 9
  int tilesM, tilesC, splits;
  int units, units_per_split;    // unit = (clip, plane, chunk of 16 columns)
  int chunks;                    // ceil(W / 16)
  int S;                         // steps per unit: rows 0 .. H (one past the end), padded to a multiple of 3
  unsigned x_nstride, dy_nstride;
  unsigned x_bytes, dy_bytes, slab_bytes;
};

struct StwArgs {                 // conv3d_wgrad_stem.hip: the stem kernel
  int K, C, D, H, W, OD, OH, OW, KD, KH, KW, pd, ph, pw;
  int nrt;                       // row tiles of 32 output channels per workgroup: 2 or 4
  int g;                         // tap planes per workgroup: 2 when KD > 1 and nrt = 2, else 1
  int wk;                        // waves sharing a tile set, interleaved over the steps: 2 when KD = 1 and nrt = 2, else 1
  int ngroups;                   // ceil(KD / g)
  int units, ups, splits;        // unit = (clip, od, chunk of ohl output rows); units per split
  int ohc, ohl;                  // row chunks per (clip, od), rows per chunk
  int steps;                     // ceil(OW / 16)
  int SS, nstg;                  // steps per dY stage, stages per output row
  int ncols;                     // KH * C * KW
  int LQ;                        // dwords of one array: 8 * steps + 1 (odd: consecutive arrays walk all banks)
  int ARRB, RS, PLS, ZB;         // bytes: one array, one row slot (C * NP * 4 arrays), one plane (RING slots), zero region
  int DYB;                       // bytes of one dY stage buffer
  int ntask;                     // staging tasks of a round: 2 * C * g * LQ
  unsigned x_nstride, dy_nstride;   // elements between clips
  unsigned osp;                  // OD * OH * OW
  unsigned x_bytes, dy_bytes, slab_bytes;
  long long nW;                  // elements of dW (slab stride)
};

// Kernel family of a weight gradient.  The values are the tune_wgrad_tile codes that request the streaming kernels, which are
// also the shape field gca_conv_wgrad_cfg reports for them.
enum class WgradKernel { Gather = 0, Temporal32 = 11, Temporal64 = 12, Spatial = 13, Stem = 14 };

// The resolved launch of one weight gradient (resolve_wgrad): every entry point reads this one plan.
struct WgradLaunch {
  WgradKernel kernel;
  int math;                      // resolved arithmetic (resolve_math)
  int splits;                    // fp32 slabs the kernel leaves (gca_conv_wgrad_ws_bytes)
  long long blocks;              // workgroups of the launch (256 threads each)
  size_t lds;                    // dynamic LDS bytes
  int x_align, dy_align;         // byte alignment the kernel needs of x / dy
  bool xf;                       // takes a pre-activation x with in_scale / in_shift (gca_conv_xf_ok)
  // the gather kernel: tile shape index, float4 dY, tap-mask kind, float4 X
  int shape; bool avec; int fast; bool bvec;
  // the block of the chosen kernel; the others stay unset
  WgradArgs gather;
  TsArgs ts;
  SsArgs ss;
  StwArgs stw;
};

// conv3d_wgrad.hip (geom_ok(g) holds)
WgradLaunch resolve_wgrad(const gca_conv_geom* g);
// conv3d_wgrad_ts.hip: the streaming temporal (kernel Temporal32 / Temporal64) or (1,3,3) (Spatial) kernel.  Fills L (math
// already resolved) and returns true when g can run there.
bool wgrad_ts_plan(const gca_conv_geom* g, WgradKernel kernel, WgradLaunch& L);
int wgrad_ts_run(const gca_conv_geom* g, const WgradLaunch& L, const float* x, const float* dy, float* slab, hipStream_t st,
                 const float* in_scale, const float* in_shift);
// conv3d_wgrad_stem.hip: the <= 4-channel, stride-2 stem kernel, same contract
bool wgrad_stem_plan(const gca_conv_geom* g, WgradLaunch& L);
int wgrad_stem_run(const WgradLaunch& L, const void* x, const void* dy, float* slab, hipStream_t st);
// the same kernel forming dY from (dz, y, constants of gca_bn_bwd_sums) in registers: re-plans the stages of a Stem launch in L
// (false: not a Stem launch, or the geometry is refused), then runs it
bool wgrad_stem_dzf_plan(const gca_conv_geom* g, WgradLaunch& L);
int wgrad_stem_dzf_run(const WgradLaunch& L, const void* x, const void* dz, const void* y, const float* consts, int relu,
                       float* slab, hipStream_t st);
inline bool unit_stride(const gca_conv_geom* g) { return g->sd == 1 && g->sh == 1 && g->sw == 1; }


}  // namespace gca_conv
