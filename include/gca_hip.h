/*
 * gca_hip.h -- C ABI of libgca_hip.so: the MI355X (gfx950) kernels behind the GCA
 * contrastive pre-training hot path (encoder -> graph block -> head -> MoCo queue / InfoNCE).
 *
 * The reference (ACMMM2021-Anonymous/video-graph-ssl) is pure Python: it has no FFI layer,
 * every "kernel" is an ATen/cuDNN call made through torch.nn.  Each entry point below
 * therefore cites the reference call site (file:line under /root/reference) whose
 * arithmetic it replaces.  Conventions for every function:
 *
 *   - plain device pointers + sizes, fp32 data, NCDHW contiguous activations;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); nothing synchronises;
 *   - no hidden allocations: workspaces are caller-owned, sizes come from the *_ws_bytes() queries;
 *   - return 0 on success, negative on invalid arguments (GCA_EINVAL) or launch failure
 *     (GCA_ELAUNCH); no exceptions cross the ABI.
 *
 * The host side (Python, ctypes) lives in video-graph-ssl_amd/_hip.py; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 */
#ifndef GCA_HIP_H
#define GCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCA_OK 0
#define GCA_EINVAL (-1)
#define GCA_ELAUNCH (-2)

int gca_version(void);

/* Diagnostic: workgroups of the LDS-halo conv kernel with `tm` x `tn` tiles per wave (rows 32 tm, columns 128 tn) in
 * arithmetic `math` that the runtime co-schedules on one CU at `lds_bytes` of dynamic LDS; -1 for a shape the entry does not
 * know.  (DESIGN.md quotes it for the dominant kernel; nothing on the product path calls it.) */
int gca_conv_halo_occupancy(int tm, int tn, int math, int64_t lds_bytes);

/* Arithmetic of the convolution kernels (forward, dgrad, wgrad; tensors stay fp32 in HBM in every mode):
 *   0  f32:     v_mfma_f32_32x32x2_f32, bitwise an fmaf chain (157 TFLOP/s peak)
 *   1  bf16x3:  every fp32 operand is split in the kernel into hi = bf16(x), lo = bf16(x - hi); a product becomes
 *               hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: ~2^-17 relative error per
 *               product (16+ of fp32's 24 significand bits; TF32 -- the reference's default on its own GPUs,
 *               torch.backends.cudnn.allow_tf32 -- keeps 11), 5.3x less matrix-pipe time than mode 0.
 *   2  bf16x6:  three parts (x = hi + mid + lo to 2^-27) and the six products hh, hm, mh, hl, lh, mm: the dropped terms
 *               are <= 2^-25 relative, below fp32's own rounding -- fp32-grade results (same parity bars as mode 0 in
 *               tests/) at 2.7x less matrix-pipe time.
 * The default comes from the environment (GCA_CONV_MATH=f32|bf16x3|bf16x6, unset = bf16x6).  GCA_EINVAL for another mode. */
int gca_set_conv_math(int mode);
int gca_get_conv_math(void);

/* ---------------------------------------------------------------------------------------
 * 3D convolution as an MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM, NCDHW, no bias.
 * Replaces every nn.Conv3d on the path: resnet2p1d.py:13-36,162-174; s3d_1.py:40,53,57;
 * resnet.py:14-22,77-78,120-126; temporal_graph.py:46,119-122 (1x1x1); nn.Linear of the heads
 * (project_head.py:23-28,39-50) runs through the same kernels as a 1x1x1 conv on (b,C,1,1,1).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t N, C, D, H, W;       /* input  (N,C,D,H,W)            */
  int32_t K;                   /* output channels               */
  int32_t kd, kh, kw;          /* kernel                        */
  int32_t sd, sh, sw;          /* stride                        */
  int32_t pd, ph, pw;          /* zero padding                  */
  int32_t OD, OH, OW;          /* output spatial (caller-computed, checked).  Each activation tensor must span
                                  at most 0xfffff000 bytes (32-bit byte offsets through buffer resources inside
                                  the kernels): <= 2^30 - 1024 fp32 elements, < 2^30 fp16 elements.  A larger
                                  one is refused (GCA_EINVAL). */
  int64_t x_batch_stride;      /* elements between consecutive clips of x; 0 = C*D*H*W (contiguous).
                                  Lets the two views of a (b,6,T,H,W) batch be read in place
                                  (tools/train_video_contrast_dis.py:404 torch.chunk on dim 1).
                                  Honoured by gca_conv_fwd and gca_conv_wgrad; dgrad needs 0. */
  /* Launch tuning (0 = built-in heuristic).  The host measures a few candidates per geometry once
   * -- the reference does the same through cudnn.benchmark = True, tools/train_video_contrast_dis.py:50 --
   * and pins the winner here.  Results are deterministic for a fixed setting. */
  int32_t tune_fwd_bm, tune_fwd_splits;       /* tile rows 32..160 (x128 columns), | 1024 = x256 columns with float4
                                                 gathers (pointwise-in-space convs only), | 2048 = LDS-halo kernel (tile
                                                 box in tune_*_box), 4096 | 64 = stem kernel (forward, C <= 4, stride 2
                                                 and <= 8 taps along W; bf16x3 / bf16x6 / fp16 storage), 8192 | 128 =
                                                 pointwise fp16 GEMM kernel (1x1x1, unit stride, act_f16); split-K factor */
  int32_t tune_dgrad_bm, tune_dgrad_splits;
  int32_t tune_wgrad_splits, tune_wgrad_tile;  /* split-K factor; tile: 0 = heuristic, 1..10 = shapes of the gather kernel (see
                                                * gca_conv_wgrad_cfg), 11 / 12 = streaming temporal kernel (32 / 64 output channels per
                                                * wave), 13 = streaming (1,3,3) kernel, 14 = stem kernel (<= 4 input channels, stride
                                                * (1,2,2)); a tile the geometry / arithmetic does not admit falls back to the heuristic
                                                * (gca_conv_wgrad_cfg reports what will run) */
  int32_t tune_fwd_tail, tune_dgrad_tail;      /* two-phase launch: (short tile rows / 32) | (column tiles run with the tall
                                                  tile << 8); 0 = single launch.  Used only with 128-column tiles, split 1 */
  int32_t tune_fwd_math, tune_dgrad_math, tune_wgrad_math;  /* 0 = the arithmetic set by gca_set_conv_math; 1 + m = run this
                                                  pass with arithmetic m, honoured only when m is at least as accurate as
                                                  the mode in force (f32 > bf16x6 > bf16x3): the mode is a floor on
                                                  accuracy and the host pins whichever admissible kernel is fastest */
  int32_t tune_fwd_box, tune_dgrad_box;        /* LDS-halo kernel (tune_*_bm & 2048): a tile is a box of bd x bh x bw output
                                                  positions inside one clip, coded bd | bh << 8 | bw << 16 (powers of two,
                                                  product 128 or 256); its input window is staged once per 16 channels in
                                                  LDS and every tap is formed from there.  0 with the flag clear */
  int32_t act_f16;                             /* 1: the activation tensors of this convolution (x, y, dy, dx) are IEEE fp16 in
                                                  HBM -- the fp16-storage path (the reference's apex-amp option,
                                                  tools/train_video_contrast_dis.py:134-141,415-417).  Weights stay fp32
                                                  masters (their packed copies are fp16 where the kernel multiplies in fp16),
                                                  accumulation, BatchNorm statistics and dw are fp32.  The LDS-halo kernels
                                                  multiply on v_mfma_f32_32x32x16_f16; the gather and weight-gradient kernels
                                                  widen each fp16 operand to its exact bf16 hi + lo pair (three bf16 MFMAs).
                                                  The conv arithmetic selector (gca_set_conv_math) does not apply. */
} gca_conv_geom;

/* Weight re-layout for the GEMM A operand (k-major, zero padded).  which: 0 = forward
 * ([C*taps -> pad16][K -> pad64]), 1 = dgrad ([K*taps -> pad16][C -> pad64]).
 * gca_conv_pack_elems() gives the float count of the packed buffer. */
int64_t gca_conv_pack_elems(const gca_conv_geom* g, int which);
int gca_conv_pack(const gca_conv_geom* g, int which, const float* w, float* packed, void* stream);

/* Batched form of gca_conv_pack for a whole encoder (one launch instead of one per layer and problem class;
 * the reference re-reads nn.Conv3d.weight in place, so this is part of what replaces cuDNN's per-call filter
 * transform).  gca_conv_pack_jobs_host writes one GCA_PACK_JOB_BYTES record per problem class of (g, which)
 * for weights `w` (device) -> `packed` (device) into HOST memory `jobs_out` and returns the number of records
 * (pass jobs_out = NULL to only count).  The caller concatenates the records of all layers, calls
 * gca_conv_pack_jobs_finalize_host on the concatenation (assigns each job its block range; returns the grid
 * size), copies the records to the device once, and replays gca_conv_pack_batched every step; the weight and
 * packed pointers must stay valid. */
#define GCA_PACK_JOB_BYTES 128
int64_t gca_conv_pack_jobs_host(const gca_conv_geom* g, int which, const float* w, float* packed, void* jobs_out);
int64_t gca_conv_pack_jobs_finalize_host(void* jobs, int64_t njobs);
int gca_conv_pack_batched(const void* jobs_dev, int64_t njobs, int64_t total_blocks, void* stream);

/* Gather table (one int2 per packed k-row: element offset + packed tap deltas); built on the
 * host once per geometry.  which as above, 2 = wgrad (same rows as forward). */
int64_t gca_conv_table_rows(const gca_conv_geom* g, int which);
int gca_conv_table_build_host(const gca_conv_geom* g, int which, int32_t* table_host /* 2*rows ints */);

/* y = conv(x, w) [+ bias[k]].  `wpack` from gca_conv_pack(which=0), `table` device copy of
 * the which=0 table.  If stat_sum/stat_sq are non-NULL the epilogue also writes per-channel
 * partial sums / sums of squares of y (training-mode BatchNorm statistics, fused):
 * layout [K][P], P = gca_conv_fwd_stat_parts(g). */
int64_t gca_conv_fwd_stat_parts(const gca_conv_geom* g);
/* Tooling: the launch configuration in force for which = 0 (fwd) / 1 (dgrad), first non-empty class:
 * out4 = {tile rows, tile columns, split-K factor, classes | tap-mask kind (0 none, 1: <=31 taps, 2: <=62)<<8 | float4-gather<<10 |
 *         arithmetic (0 f32, 1 bf16x3, 2 bf16x6, 3 fp16 MFMA)<<12 | LDS-halo kernel<<14 | fp16 storage<<15 | stem kernel<<16 | pointwise fp16 GEMM kernel<<17}. */
int gca_conv_kernel_cfg(const gca_conv_geom* g, int which, int32_t* out4);
/* Signature of the packed-weight layout that pass `which` (0 fwd, 1 dgrad) reads under the launch configuration in force:
 * one hex digit per problem class (0 = k-major fp32 rows of the gather kernels, 4 + arithmetic = the LDS-halo layout,
 * 1..3 = the stem layout in that arithmetic, 8 = fp16 [rows][channels] of the pointwise GEMM kernel).
 * A buffer packed by gca_conv_pack is valid exactly as long as this value does not change (the host re-packs when a
 * tune_* field moves it). */
int64_t gca_conv_pack_layout(const gca_conv_geom* g, int which);
/* Layers whose output grid cannot fill the 256 CUs split the reduction over workgroups; the fp32
 * partial slabs live in `ws` (gca_conv_fwd_ws_bytes / gca_conv_dgrad_ws_bytes; 0 = not needed, ws may
 * then be NULL) and are summed in a fixed order (deterministic). */
int64_t gca_conv_fwd_ws_bytes(const gca_conv_geom* g);
/* x / y / dy / dx: fp32, or IEEE fp16 when g->act_f16 = 1 (weights, bias, statistics and slabs are fp32 either way). */
int gca_conv_fwd(const gca_conv_geom* g, const void* x, const float* wpack, const int32_t* table,
                 const float* bias, void* y, float* stat_sum, float* stat_sq, void* ws, void* stream);

/* dx (+)= conv_transpose(dy, w).  `wpack`/`table` from which=1.  accumulate != 0 adds into dx. */
int64_t gca_conv_dgrad_ws_bytes(const gca_conv_geom* g);
int gca_conv_dgrad(const gca_conv_geom* g, const void* dy, const float* wpack, const int32_t* table,
                   void* dx, int accumulate, void* ws, void* stream);
/* A strided dgrad is one problem class per stride residue.  The classes write disjoint outputs, so when they run the same
 * gather-kernel instantiation they go out in ONE launch (and one finishing launch); their split-K slabs then have to exist
 * side by side: gca_conv_dgrad_ws_bytes_merged is the SUM over classes where gca_conv_dgrad_ws_bytes is the maximum.
 * gca_conv_dgrad_ws is gca_conv_dgrad told how many bytes `ws` holds: with fewer than the sum (gca_conv_dgrad passes the
 * maximum) the classes are launched one after another as before.  Same bits either way.  Inside the launch the classes go in
 * by falling reduction length, so that the grid ends on its shortest workgroups.  GCA_DGRAD_MERGE=0 (read once) or
 * gca_set_dgrad_merge(0) keep the per-class launches (A/B runs; 2 = merged with the classes in residue order, the A/B of
 * the ordering); gca_set_dgrad_merge returns whether merging was on.
 * gca_conv_dgrad_merged: 1 when gca_conv_dgrad_ws given `ws_bytes` of work space takes the single launch under the launch
 * shape and setting in force, else 0 (tooling, tests).
 * GCA_CLASS_BLOCK_BYTES bounds the by-value argument block of the merged launch (gca_conv_class_block_bytes: its size). */
#define GCA_CLASS_BLOCK_BYTES 2048
int gca_conv_dgrad_merged(const gca_conv_geom* g, int64_t ws_bytes);
int64_t gca_conv_dgrad_ws_bytes_merged(const gca_conv_geom* g);
int gca_conv_dgrad_ws(const gca_conv_geom* g, const void* dy, const float* wpack, const int32_t* table,
                      void* dx, int accumulate, void* ws, int64_t ws_bytes, void* stream);
int gca_set_dgrad_merge(int on);
int64_t gca_conv_class_block_bytes(void);

/* dw (+)= sum_{n,o} dy[n,k,o] * x[n,c,o*s-p+tap].  `table` from which=2.  Split-K partial slabs go
 * to `ws` (gca_conv_wgrad_ws_bytes) and are reduced deterministically. */
int64_t gca_conv_wgrad_ws_bytes(const gca_conv_geom* g);
int gca_conv_wgrad(const gca_conv_geom* g, const void* x, const void* dy, const int32_t* table,
                   float* dw, int accumulate, void* ws, void* stream);
/* The same in two halves, so that the fixed-order reductions of MANY layers run as ONE launch at the end of the backward
 * pass (the reference gets a weight gradient per cuDNN call; here 39 per-layer reduce launches of 8-12 us are pure
 * latency): gca_conv_wgrad_partial leaves the `*out_splits` fp32 slabs in `slabs` (gca_conv_wgrad_ws_bytes, caller-owned,
 * must stay untouched until reduced); gca_splitk_reduce_batched does dw (+)= sum of slabs for every job, bit-identical
 * to gca_conv_wgrad's own reduction.  Jobs: fill slabs / dw / n (= K*C*taps) / splits / accumulate on the host, call
 * gca_reduce_jobs_finalize_host (assigns block ranges, returns the grid size), copy the records to the device once.
 * Two jobs of one launch must not write the same dw. */
typedef struct {
  const float* slabs;
  float* dw;
  int64_t n;
  int32_t splits, accumulate;
  int32_t first_block, nblocks;     /* filled by gca_reduce_jobs_finalize_host */
} gca_reduce_job;
int gca_conv_wgrad_partial(const gca_conv_geom* g, const void* x, const float* in_scale, const float* in_shift, const void* dy,
                           const int32_t* table, void* slabs, int32_t* out_splits, void* stream);   /* in_scale / in_shift: see below; NULL = x as it is */

/* BatchNorm + ReLU of the PRODUCING layer applied where the consumer reads its input, so the normalised tensor
 * z = relu(y * scale[c] + shift[c]) of a conv -> BN -> ReLU -> conv link (resnet2p1d.py:66-85: bn1_s -> conv1_t, bn1_t -> conv2_s,
 * bn2_s -> conv2_t; :252-253 the stem) is never written or read: 2 of the 7 tensor passes of such a BatchNorm.
 * gca_conv_fwd_xf / gca_conv_wgrad_xf take the PRE-activation tensor y as `x` plus (scale, shift) of gca_bn_finalize
 * (arrays padded to a multiple of 16 floats + 16) and compute exactly what gca_conv_fwd / gca_conv_wgrad compute on z
 * (zero padding pads z).  Only launch configurations that pass their input through registers can do it:
 * gca_conv_xf_ok(g) = 1 when, under the tune_* fields in force, the forward runs on the LDS-halo kernels and the weight
 * gradient on the streaming temporal kernels (fp32 storage, split-product arithmetic); otherwise these entries return
 * GCA_EINVAL and the caller materialises z with gca_bn_apply. */
int gca_conv_xf_ok(const gca_conv_geom* g);
int gca_conv_fwd_xf(const gca_conv_geom* g, const void* x, const float* in_scale, const float* in_shift, const float* wpack,
                    const int32_t* table, const float* bias, void* y, float* stat_sum, float* stat_sq, void* ws, void* stream);
int gca_conv_wgrad_xf(const gca_conv_geom* g, const void* x, const float* in_scale, const float* in_shift, const void* dy,
                      const int32_t* table, float* dw, int accumulate, void* ws, void* stream);
/* BatchNorm BACKWARD of the conv's own BatchNorm applied where the weight gradient reads dy.  A first-layer conv has no dgrad
 * (resnet2p1d.py:162-168, s3d_1.py:35, resnet.py:120-126: the clip needs no gradient), so the dy that gca_bn_bwd writes has one
 * reader, this weight gradient: a full write and a full read of the largest tensor of the model.  gca_bn_bwd_sums (BatchNorm
 * section) leaves the per-channel constants instead; gca_conv_wgrad_dzf / _partial take dz (gradient behind BatchNorm + ReLU,
 * dense), the conv output y and those constants where gca_conv_wgrad / gca_conv_wgrad_partial take dy, and form
 * dy = A * (m * dz - B - (y - mean) * invstd * Cc) per element in registers, operation for operation what gca_bn_bwd stores.
 * relu: 0 or 2, as given to gca_bn_bwd_sums.  gca_conv_dzf_ok(g) = 1 when, under the tune_* fields in force, the weight
 * gradient of g runs on the stem kernel (tune_wgrad_tile 14 on a geometry it takes); otherwise these entries return GCA_EINVAL
 * and the caller runs gca_bn_bwd + gca_conv_wgrad.  `table` is not read (may be NULL).  Same slabs, splits and workspace as
 * gca_conv_wgrad. */
int gca_conv_dzf_ok(const gca_conv_geom* g);
int gca_conv_wgrad_dzf(const gca_conv_geom* g, const void* x, const void* dz, const void* y, const float* consts, int relu,
                       const int32_t* table, float* dw, int accumulate, void* ws, void* stream);
int gca_conv_wgrad_dzf_partial(const gca_conv_geom* g, const void* x, const void* dz, const void* y, const float* consts, int relu,
                               const int32_t* table, void* slabs, int32_t* out_splits, void* stream);
int64_t gca_reduce_jobs_finalize_host(gca_reduce_job* jobs, int64_t njobs);
int gca_splitk_reduce_batched(const gca_reduce_job* jobs_dev, int64_t njobs, int64_t total_blocks, void* stream);
/* Launch shape the wgrad kernel will use for g: out4 = {tile rows (output channels), tile columns (C*taps),
 * split-K factor, shape index | float4 dY loads<<8 | tap-mask kind<<9 | float4 X gathers<<11 | arithmetic<<12}. */
int gca_conv_wgrad_cfg(const gca_conv_geom* g, int32_t* out4);

/* db[k] (+)= sum over (n, spatial) of dy[n,k,:]   (bias gradient of the nn.Linear layers) */
int gca_bias_grad(const float* dy, int64_t N, int64_t K, int64_t SP, float* db, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm (training mode: batch statistics + running-stat update), fused with ReLU and the
 * residual add.  Replaces nn.BatchNorm3d/1d + ReLU + `out += residual`:
 * resnet2p1d.py:49-57,66-85; s3d_1.py:41-47,54-68; project_head.py:39-50,64-68.
 * Data layout (N, C, SP) with SP = D*H*W (1 for BatchNorm1d).
 * act_f16 = 1: the activation tensors (x, residual, z, dz_in, dx, dres -- the `void*` arguments) are IEEE fp16
 * (the fp16-storage path of BASELINE configs[4]); statistics, parameters and all arithmetic stay fp32/fp64.
 * ------------------------------------------------------------------------------------- */
/* From conv-epilogue partials [C][P] (or computed by gca_bn_stats): mean/invstd (saved for
 * backward), running stats update (momentum, unbiased var), and the folded affine
 * scale = gamma*invstd, shift = beta - mean*scale.  count = N*SP. */
int gca_bn_stats(const void* x, int64_t N, int64_t C, int64_t SP, float* stat_sum, float* stat_sq,
                 int64_t* parts_out, int act_f16, void* stream);          /* P is fixed: gca_bn_stats_parts() */
int64_t gca_bn_stats_parts(int64_t N, int64_t C, int64_t SP);
int gca_bn_finalize(const float* stat_sum, const float* stat_sq, int64_t P, int64_t C, double count,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* save_mean, float* save_invstd, float* scale, float* shift, void* stream);
/* A conv whose launch shape splits the reduction, followed by a small BatchNorm (N*SP <= 32768), in two launches instead of
 * three.  gca_conv_fwd_slabs runs the forward class and LEAVES the fp32 slabs [splits][K][N*SP] in `ws` (no bias; fp32
 * tensors only; GCA_EINVAL when the pinned launch shape does not split -- gca_conv_kernel_cfg tells beforehand);
 * gca_bn_train_fwd_slabs folds them in the finishing kernel's order (same bits for y), writes y (the backward pass reads
 * it), takes the batch statistics from those values in fp64 and normalises: finalize + apply as gca_bn_train_fwd.
 * Replaces the conv -> BatchNorm link of resnet2p1d.py:66-85 / s3d_1.py:43-47 on the deep, narrow layers. */
int gca_conv_fwd_slabs(const gca_conv_geom* g, const void* x, const float* wpack, const int32_t* table, void* ws,
                       int32_t* out_splits, void* stream);
int gca_bn_train_fwd_slabs(const float* slabs, int64_t splits, double count, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float* save_mean, float* save_invstd, float* scale, float* shift, float* y, const float* residual,
                           int relu, int64_t N, int64_t C, int64_t SP, float* z, int64_t z_batch_stride, void* stream);
/* gca_bn_finalize followed by gca_bn_apply behind one call (one LAUNCH when N*SP is small: the deep layers, and
 * every layer of a small batch, are launch-latency bound).  count must equal N*SP. */
int gca_bn_train_fwd(const float* stat_sum, const float* stat_sq, int64_t P, int64_t C, double count,
                     const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float* save_mean, float* save_invstd, float* scale, float* shift,
                     const void* x, const void* residual, int relu, int64_t N, int64_t SP, void* z,
                     int64_t z_batch_stride, int act_f16, void* stream);
/* Eval-mode fold (running stats): scale/shift only. */
int gca_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, int64_t C, float* scale, float* shift, void* stream);
/* z = [relu]( x*scale[c] + shift[c] [+ residual] ).  z_batch_stride (elements; 0 = C*SP) lets z be a
 * channel slice of a wider (N, Ctot, SP) buffer: the Inception branches write straight into their
 * slice of the concat output (s3d_1.py:96 torch.cat) instead of being copied there. */
int gca_bn_apply(const void* x, const float* scale, const float* shift, const void* residual,
                 int relu, int64_t N, int64_t C, int64_t SP, void* z, int64_t z_batch_stride, int act_f16, void* stream);
/* Backward of the fused op.  dz_in = gradient wrt z; x = saved conv output.  relu: 0 none; 1 mask from the saved
 * output z (z > 0); 2 mask recomputed from x with the forward's own scale/shift (x*scale+shift > 0) -- z may be
 * NULL and is not read: one tensor less to stream, valid when no residual was added before the ReLU.
 * Writes dx (gradient wrt x), accumulates dgamma/dbeta (+=) and, if dres != NULL, writes (dres_accumulate=0) or
 * adds (=1) the gradient wrt the residual input.  ws: gca_bn_bwd_ws_bytes(). */
int64_t gca_bn_bwd_ws_bytes(int64_t N, int64_t C, int64_t SP);
int gca_bn_bwd(const void* dz_in, const void* z, const void* x, const float* gamma,
               const float* save_mean, const float* save_invstd, int relu,
               int64_t N, int64_t C, int64_t SP, void* dx, float* dgamma, float* dbeta,
               void* dres, int dres_accumulate, int64_t z_batch_stride /* of dz_in and z */,
               const float* scale, const float* shift, void* ws, int act_f16, void* stream);
/* gca_bn_bwd without its apply pass, for a consumer that forms dx itself (gca_conv_wgrad_dzf): the same reduce and finalize
 * launches at every size, so dgamma / dbeta (+=) get the bits gca_bn_bwd gives them above the one-workgroup regime
 * (N*SP > 32768).  relu: 0 or 2.  consts: gca_bn_bwd_consts_elems(C) floats = 7 rows of stride Cp = 16*ceil(C/16) + 16
 * (the padding of the _xf scale / shift rows): A = gamma*invstd, B = sum(m*dz)/M, Cc = sum(m*dz*xhat)/M, mean, invstd, and
 * the forward's scale, shift (zeros when relu = 0); the pad c >= C of every row is zero.  ws: gca_bn_bwd_ws_bytes(). */
int64_t gca_bn_bwd_consts_elems(int64_t C);
int gca_bn_bwd_sums(const void* dz_in, const void* x, const float* gamma, const float* save_mean, const float* save_invstd,
                    int relu, int64_t N, int64_t C, int64_t SP, float* dgamma, float* dbeta, int64_t z_batch_stride /* of dz_in */,
                    const float* scale, const float* shift, float* consts, void* ws, int act_f16, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pooling.  MaxPool3d: resnet2p1d.py:178, s3d_1.py:10,13,16,22,87, temporal_graph.py:100
 * (first-max tie break in (d,h,w) scan order, as ATen).  Global/temporal-weighted average:
 * resnet2p1d.py:197,260 (AdaptiveAvgPool3d(1)); s3d_1.py:30-33 (avg_pool3d((2,H,W),1) then mean
 * over T' == frame-weighted global mean); resnet.py:137-140,187.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t N, C, D, H, W;
  int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
  int32_t OD, OH, OW;
} gca_pool_geom;
/* scale/shift (both or neither): pool relu(x*scale[c] + shift[c]) instead of x -- the BatchNorm+ReLU in front of
 * the pool (resnet2p1d.py:252-255 conv1_t -> bn1_t -> relu -> maxpool) evaluated on the fly. */
int gca_maxpool3d_fwd(const gca_pool_geom* g, const void* x, void* y, int32_t* argmax, const float* scale,
                      const float* shift, int act_f16, void* stream);
int gca_maxpool3d_bwd(const gca_pool_geom* g, const void* dy, const int32_t* argmax, void* dx,
                      int accumulate, int act_f16, void* stream);
/* nn.AvgPool3d(kernel_size=k) (stride = k, no padding, floor mode; fp32 maps): the `max_pool=False` option of
 * TemporalGraphAug (lib/ops/module_wrappers/temporal_graph.py:100).  Other strides / paddings: GCA_EINVAL. */
int gca_avgpool3d_fwd(const gca_pool_geom* g, const float* x, float* y, void* stream);
int gca_avgpool3d_bwd(const gca_pool_geom* g, const float* dy, float* dx, int accumulate, void* stream);
/* y[n,c] = sum_{d,h,w} wt[d] * x[n,c,d,h,w] * norm   (wt == NULL -> all ones) */
/* x_f16: the feature map (x, dx) is stored fp16; the pooled features y / dy are fp32 either way (the head is fp32). */
int gca_wavgpool_fwd(const void* x, const float* wt, float norm, int64_t NC, int64_t D, int64_t HW,
                     float* y, int x_f16, void* stream);
int gca_wavgpool_bwd(const float* dy, const float* wt, float norm, int64_t NC, int64_t D, int64_t HW,
                     void* dx, int x_f16, void* stream);

/* ---------------------------------------------------------------------------------------
 * Head pieces.  ReLU between the two Linear layers (project_head.py:24-27) and row L2
 * normalisation `Normalize` (project_head.py:4-10, F.normalize eps 1e-12).
 * ------------------------------------------------------------------------------------- */
int gca_relu_fwd(const float* x, int64_t n, float* y, void* stream);
int gca_relu_bwd(const float* dy, const float* y, int64_t n, float* dx, void* stream);
int gca_l2norm_fwd(const float* x, int64_t rows, int64_t dim, float eps, float* y, float* inv_norm, void* stream);
int gca_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, int64_t rows, int64_t dim,
                   float* dx, void* stream);
/* Negative cosine similarity D(p, stopgrad(z)) of SimSiam (graph_wrappers.py:105-106):
 * loss[0] (+)= -scale * mean_i cos(p_i, z_i); dp = d loss / d p.  `loss` needs 1 + rows floats
 * (loss[1..rows] receives the per-row cosines). */
int gca_negcos_fwd_bwd(const float* p, const float* z, int64_t rows, int64_t dim, float scale,
                       float* loss, int accumulate, float* dp, void* stream);

/* ---------------------------------------------------------------------------------------
 * MoCo queue + InfoNCE.  RGBMoCo._compute_logit (lib/memory/mem_moco.py:29-49):
 * logits[i,0] = q_i.k_i / T, logits[i,1+j] = q_i.queue_j / T, as one clip x queue MFMA GEMM
 * streaming the queue once.  NCESoftmaxLoss (lib/memory/criterion.py:34-45) = mean_i
 * (logsumexp(logits_i) - logits_i0).  _update_memory/_update_pointer (mem_moco.py:14-27).
 * ------------------------------------------------------------------------------------- */
/* logits (b, K+1).  Optional fused row statistics (any may be NULL): row_lse (b), rank_ge (b) = number of negatives
 * with logit >= the positive's (top-1 hit <=> 0, top-5 <=> < 5; lib/evaluation/metric.py:44-67 with label 0), and
 * loss (1) = NCESoftmaxLoss of these logits (needs row_lse) -- the whole forward of mem_moco.py:60-88 +
 * criterion.py:34-45 behind one call.  ws: gca_infonce_ws_bytes(b, K).
 * sync_counter: one device uint32 that is ZERO before the first call (every call leaves it zero); with it, b <= 32 and
 * D <= 128 the whole forward is ONE launch -- persistent waves stream the queue, the last workgroup to arrive folds the
 * row statistics.  NULL selects the multi-launch path. */
int64_t gca_infonce_ws_bytes(int64_t b, int64_t K);
int gca_moco_logits_fwd(const float* q, const float* k, const float* queue, int64_t b, int64_t K,
                        int64_t D, float inv_T, float* logits, float* row_lse, int32_t* rank_ge, float* loss,
                        void* ws, uint32_t* sync_counter, void* stream);
/* loss = mean_i (lse_i - logits[i,0]); lse computed here if row_lse_in == NULL. */
int gca_nce_softmax_loss_fwd(const float* logits, int64_t b, int64_t ncol, const float* row_lse_in,
                             float* row_lse_out, float* loss, void* stream);
/* dlogits[i,j] = gscale * (softmax(logits_i)[j] - [j==0]) / b   (gscale: upstream d loss) */
int gca_nce_softmax_loss_bwd(const float* logits, const float* row_lse, int64_t b, int64_t ncol,
                             const float* gscale_dev, float gscale_host, float* dlogits, void* stream);
/* dq = dlogits[:,0:1]*k/T + dlogits[:,1:] @ queue / T.  Rows [ov_start, ov_start+ov_n) mod K of
 * `queue` are read from ov_rows instead (the rows the enqueue of this step has already
 * overwritten -- the reference computes the gradient against the pre-enqueue snapshot,
 * mem_moco.py:72).  If dlogits == NULL it is formed on the fly from logits/row_lse as in
 * gca_nce_softmax_loss_bwd (fused path; no dlogits tensor is materialised). */
int gca_moco_logits_bwd(const float* dlogits, const float* logits, const float* row_lse,
                        const float* gscale_dev, float gscale_host,
                        const float* k, const float* queue, int64_t b, int64_t K, int64_t D, float inv_T,
                        int64_t ov_start, const int64_t* ov_start_dev /* overrides ov_start if non-NULL */,
                        int64_t ov_n, const float* ov_rows, float* dq, void* ws, void* stream);
/* accuracy(output, target, topk) of lib/evaluation/metric.py:44-67 (called at tools/train_video_contrast_dis.py:428) without
 * the top-k sort or a host sync: rank_ge[i] = number of columns j != target[i] with output[i,j] >= output[i,target[i]];
 * the target is in the top k of row i iff rank_ge[i] < k.  target must lie in [0, ncol) (not checked on the device). */
int gca_rank_ge(const float* output, const int64_t* target, int64_t b, int64_t ncol, int32_t* rank_ge, void* stream);
/* queue[(ptr + i) % K] = keys[i], i < n; optionally saves the overwritten rows first.  The
 * reference keeps the pointer as a Python int (mem_moco.py:12); for hipGraph replay it can live in
 * device memory instead: ptr_dev (non-NULL) overrides ptr, gca_queue_advance moves it. */
int gca_queue_enqueue(float* queue, int64_t K, int64_t D, const float* keys, int64_t n, int64_t ptr,
                      const int64_t* ptr_dev, float* saved_rows, void* stream);
int gca_queue_advance(int64_t* ptr_dev, int64_t n, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------
 * Temporal-graph block (lib/ops/module_wrappers/temporal_graph.py).  The 1x1x1 convs and the
 * (1,2,2) max pool go through gca_conv_* / gca_maxpool3d_*; these are the graph-specific parts.
 * ------------------------------------------------------------------------------------- */
/* sim = softmax_j( sum_f gq[b,i,f]*gk[b,j,f] ), gq/gk stored (B, Ci, T, HW) as the pooled convs
 * leave them (temporal_graph.py:159-176); then adj_pre = sim * theta(hop(i,j)) within max_hop
 * else 0 (:204-210); then adj = sigmoid((logit(u)+logit(adj_pre))/temperature)  (:187-192,
 * RelaxedBernoulli.rsample with explicit uniforms u).  ws: gca_graph_gram_ws_bytes(B, Ci, T, HW) bytes of scratch
 * for the two-pass (T x F)(F x T) product (NULL = slower one-workgroup-per-entry fallback). */
int64_t gca_graph_gram_ws_bytes(int64_t B, int64_t C, int64_t T, int64_t HW);
int gca_graph_adj_fwd(const float* gq, const float* gk, int64_t B, int64_t Ci, int64_t T, int64_t HW,
                      int max_hop, float alpha, float temperature, const float* u,
                      float* sim, float* adj_pre, float* adj, void* ws, void* stream);
/* NOTE: dadj is in/out -- it is overwritten with the gradient wrt the pre-softmax similarity. */
int gca_graph_adj_bwd(const float* dadj, const float* gq, const float* gk, const float* sim,
                      const float* adj_pre, const float* adj, int64_t B, int64_t Ci, int64_t T, int64_t HW,
                      int max_hop, float alpha, float temperature, float* dgq, float* dgk, void* stream);
/* out[b,c,i,:] = sum_j adj[b,i,j]*s[b,c,j,:] + s[b,c,i,:]   (einsum 'bij,bcjhw->bcihw' + skip,
 * temporal_graph.py:59-62): wave-reduced dense neighbourhood GEMV, one pass over s. */
int gca_graph_gcn_fwd(const float* adj, const float* s, int64_t B, int64_t C, int64_t T, int64_t HW,
                      float* out, void* stream);
/* ds[b,c,j,:] = sum_i adj[b,i,j]*dout[b,c,i,:] + dout[b,c,j,:];  dadj[b,i,j] = sum_{c,hw} dout[b,c,i,:]*s[b,c,j,:] */
int64_t gca_graph_gcn_bwd_ws_bytes(int64_t B, int64_t C, int64_t T, int64_t HW);
int gca_graph_gcn_bwd(const float* adj, const float* s, const float* dout, int64_t B, int64_t C, int64_t T,
                      int64_t HW, float* ds, float* dadj, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device-side tail of the input pipeline.  Replaces, for uint8 frames already decoded / resized on the
 * host, the last stages of the reference's transform chain and its collation:
 *   VideoRandomHorizontalFlip + VideoNormalize + VideoToTensor  (lib/data/transform/consistency_transforms.py:11-65,
 *   composed in lib/data/transform/build.py:45-62), an integer crop window (albumentations random_crop coordinates as
 *   VideoRandomCrop / VideoCenterCrop use them), the channel concatenation of the two views
 *   (lib/data/datasets/video_contrast_dataset.py:196-203) and the H2D copy of the fp32 batch (tools/...dis.py:402).
 *   frames : (b, views, T, Hs, Ws, 3) uint8, HWC frames as cv2 delivers them (device memory)
 *   params : (b, views, 4) int32 on the device: {h0, w0, flip, 0} -- ONE crop origin and flip decision per (clip, view), shared
 *            by its T frames (the reference's transforms draw them once per clip); windows are clamped into the frame
 *   mean255, inv_std255 : HOST pointers to 3 floats each: f32(mean_c)*255 and 1/(f32(std_c)*255), computed in fp32 as numpy
 *            does in VideoNormalize.normalize (:53-65)
 *   out    : (b, 3*views, T, H, W) fp32, or fp16 when out_f16 (the fp16-storage path): out = (float(px) - m_c) * d_c,
 *            two fp32 roundings -- bit-identical to the reference's arithmetic
 * One pass over HBM, 3 B read + 12 (6) B written per pixel. */
int gca_clip_prepare(const uint8_t* frames, int64_t b, int64_t views, int64_t T, int64_t Hs, int64_t Ws,
                     const int32_t* params, const float* mean255, const float* inv_std255, int64_t H, int64_t W,
                     void* out, int out_f16, void* stream);

/* The whole contrastive chain on the device (opt-in; gca_clip_prepare is unchanged): VideoRandomResizedCrop -> colour jitter
 * -> grayscale -> Gaussian blur -> flip -> normalise -> to-tensor (lib/data/transform/build.py:45-62,
 * consistency_transforms.py:81-145, 226-340) from decoded uint8 source frames and one parameter record per (clip, view).
 * The arithmetic is the one written down in tests/augment_ref.py (integer / fixed point, or fp32 with one rounding per
 * operation, no contraction), which the kernels reproduce bit for bit.  cv2 / albumentations are not available to compare
 * with: parity with cv2's own rounding is UNVERIFIED and not claimed.
 *   frames       : (b, views, T, Hs, Ws, 3) uint8, device
 *   records      : (b, views, 24) int32, device; records_host: the same words in HOST memory (they are validated there)
 *                  0 y0  1 x0  2 ch  3 cw   crop box inside the source frame (it may be smaller than the output: upscaling)
 *                  4 flip  5 gray  6 k      blur size, 0 (off) | 3 | 5 | 7, radius < min(H, W)
 *                  7..10 perm               order of the jitter ops: 0 brightness, 1 contrast, 2 saturation, 3 hue
 *                  11 mask                  bit op set = op applied (0 = no jitter; factor 1 / hue 0 = identity = bit clear)
 *                  12 f_c  13 1 - f_c  14 f_s  15 1 - f_s   contrast / saturation factors, fp32 bit patterns
 *                  16..22 blur taps         k 12-bit fixed-point weights >= 0 that sum to 4096, the rest 0;   23: 0
 *   taps         : (b, views, H + W, 4) int16, device, 8-byte aligned: per output row (first H) / column (last W)
 *                  {i0, i1, c0, c1}: two source indices in frame coordinates and their 11-bit weights, c0 + c1 = 2048
 *   luts         : (b, views, 2, 256) uint8, device: brightness table; hue table (H in [0, 180) -> shifted H)
 *   divtab       : (2, 256) int32, device: round((255 << 12) / i) and round((180 << 12) / (6 i)), entry 0 = 0
 *   mean255, inv_std255, out, out_f16 : as gca_clip_prepare
 *   ws           : gca_clip_augment_ws_bytes(b, views, T) bytes, device: one integer gray sum per frame (contrast)
 * GCA_EINVAL for a crop box outside the frame, k outside {0, 3, 5, 7} or too wide for the output, a perm that is no
 * permutation, blur taps that do not sum to 4096.  At most two launches (the reduction for contrast, the main pass). */
int64_t gca_clip_augment_ws_bytes(int64_t b, int64_t views, int64_t T);
int gca_clip_augment(const uint8_t* frames, int64_t b, int64_t views, int64_t T, int64_t Hs, int64_t Ws,
                     const int32_t* records_host, const int32_t* records, const int16_t* taps, const uint8_t* luts,
                     const int32_t* divtab, const float* mean255, const float* inv_std255, int64_t H, int64_t W,
                     void* out, int out_f16, void* ws, void* stream);

/* Downstream (action-recognition) views: many views of ONE decoded source per video (gca_clip_prepare and gca_clip_augment
 * are unchanged).  Replaces the reference's host transforms for fine-tuning and testing and the H2D copy of every finished
 * fp32 view:
 *   training  VideoMultiScaleCrop -> VideoRandomHorizontalFlip -> VideoNormalize -> VideoToTensor
 *             (lib/data/transform/build.py:27-35, consistency_transforms.py:366-468)
 *   testing   VideoResize -> VideoCenterCrop | VideoFullResSample | VideoOverSampleCrop -> VideoNormalize -> VideoToTensor
 *             (tools/test_ds.py:95-120, consistency_transforms.py:159-170, 341-349, 470-551)
 * A crop of a resized uint8 frame is a window of the resize's tap table, so all test-time views of a video share one source
 * and one table.  The arithmetic is the one written down in tests/views_ref.py (the resize of tests/augment_ref.py: two
 * blends, one rounding shift to uint8; then (float(px) - m_c) * d_c, two fp32 roundings), reproduced bit for bit.  As for
 * gca_clip_augment, parity with cv2's own rounding is UNVERIFIED and not claimed.
 *   frames       : (n_src, F, Hs, Ws, 3) uint8, device: one decoded source per video (F = T for training, test_clips * T
 *                  for testing); Hs, Ws <= 32767
 *   records      : (n_views, 8) int32, device; records_host: the same words in HOST memory (they are validated there)
 *                  0 src  1 t0  2 tab  3 oy  4 ox  5 flip  6, 7: 0
 *   taps         : (n_tab, Lh + Lw, 4) int16, device, 8-byte aligned: Lh row taps, then Lw column taps, each {i0, i1, c0, c1}:
 *                  two source indices in frame coordinates and their 11-bit weights, c0 + c1 = 2048
 *   mean255, inv_std255 : HOST pointers to 3 floats each, as gca_clip_prepare
 *   out          : (n_views, 3, T, H, W) fp32.  Pixel (y, x) of frame t of a view samples frames[src, t0 + t] through the row
 *                  tap taps[tab, oy + y] and the column tap taps[tab, Lh + ox + (flip ? W - 1 - x : x)]
 * GCA_EINVAL, with nothing launched and nothing written, for src outside [0, n_src), tab outside [0, n_tab), t0 < 0 or
 * t0 + T > F, a window (oy, H) / (ox, W) outside (Lh) / (Lw), flip not 0 or 1, any size below 1, a tensor of 2^31 elements
 * or more, T > 65535.  n_views = 0: returns 0, nothing launched.  The kernel clamps every index it forms from the device
 * tables into its buffer: tap contents can mis-sample, never reach outside.  One launch, for any n_views. */
int gca_clip_views(const uint8_t* frames, int64_t n_src, int64_t F, int64_t Hs, int64_t Ws,
                   const int32_t* records_host, const int32_t* records, int64_t n_views,
                   const int16_t* taps, int64_t n_tab, int64_t Lh, int64_t Lw,
                   const float* mean255, const float* inv_std255,
                   int64_t T, int64_t H, int64_t W, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Nearest-neighbour video retrieval (tools/video_retrieval.py:174-197: sklearn cosine_distances / euclidean_distances
 * followed by np.argsort of every row of the (nq, ng) matrix, of which the first 50 entries are used).  Fused: the matrix
 * is never written.  q (nq, D) and g (ng, D) contiguous fp32; metric 0 = cosine, 1 = euclidean; 1 <= k <= 64.
 *   s = sum_d q[i,d] * g[j,d] on the fp32 matrix cores; squared row norms n2 by a pass of their own
 *   cosine:    r = 1 / sqrt(n2) (both correctly rounded; 0 for an all-zero row), dist = 1 - (s * r_q) * r_g
 *   euclidean: d2 = max(0, (n2_q + n2_g) - 2 s) is the ranking key, dist = sqrt(d2)
 *   order:     ascending by (key, gallery index) -- np.argsort(kind='stable'); NaN keys after +inf, -0 counts as +0
 *   idx (nq, k) int32 gallery rows, nearest first; dist (nq, k) fp32; with ng < k the tail is idx = -1, dist = +inf
 *   q_label (nq) / g_label (ng) int64, both or neither: first_hit (nq) int32 = 1-based rank of the first returned row whose
 *   label equals the query's, k + 1 if none (R@k' = mean(first_hit <= k') for every k' <= k).  Without labels first_hit is
 *   not written.
 * The gallery is cut into `slabs` contiguous slabs (0 = enough to fill the device, at most 64 and at most one per 128 rows);
 * results are bitwise the same for every value.  ws: gca_retrieval_ws_bytes() bytes = the norms + nq * slabs_used * k * 8
 * (instead of nq * ng * 4); ws_bytes is checked.  tests/retrieval_ref.py is the numpy statement of all of the above.
 * GCA_EINVAL (nothing launched) for k outside [1, 64], D < 1, negative sizes or slabs, ng >= 2^31, another metric, labels
 * on one side only, ws_bytes too small.  nq = 0 or ng = 0: nothing is launched and nothing written (the caller presets the
 * tails).  Three launches: norms, per-slab top-k lists, merge. */
int64_t gca_retrieval_ws_bytes(int64_t nq, int64_t ng, int64_t D, int32_t k, int32_t slabs);
int gca_retrieval_topk(const float* q, const float* g, int64_t nq, int64_t ng, int64_t D, int32_t k, int32_t metric,
                       const int64_t* q_label, const int64_t* g_label, int32_t slabs, int32_t* idx, float* dist,
                       int32_t* first_hit, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Weighted k-NN classifier vote on the lists of gca_retrieval_topk (the evaluation of InstDisc / MoCo / SimSiam code bases on
 * frozen features).  idx / dist (nq, k) as the search writes them: nearest first, tail slots idx = -1, dist = +inf;
 * g_label (ng) int64; 1 <= kvote <= k <= 64; C classes.
 *   valid slot j of query i: 0 <= idx[i,j] < ng, idx[i,j] != self_base + i when self_base >= 0 (leave-one-out: the queries
 *                are rows self_base.. of the gallery), g_label[idx[i,j]] in [0, C), dist[i,j] not NaN
 *   voters:      the first kvote valid slots in rank order
 *   weight:      weighting 0: 1;  weighting 1: expf(-(dist * inv_T)), the product rounded once, the library expf -- for
 *                cosine distances InstDisc's exp(sim / T) over the constant exp(1 / T): same ranking, no overflow
 *   scores[i,c]: fp32 sum of the weights of class c's voters, added in rank order; 0 for a class without voters
 *   order:       score descending, then class index ascending, over all C classes
 *   pred[i]:     the first class of that order;  rank[i]: how many classes c != q_label[i] come before q_label[i]
 *                (top-k' is correct iff rank < k'; rank == 0 iff pred == q_label).  No voter: pred = -1, rank = C.
 * scores (nq, C) may be NULL (nothing of that size is then touched); rank may be NULL, and needs q_label (nq) int64.
 * g_label is read and scores written only through range-checked indices: bad tables change results, never touch memory
 * outside the buffers.  A q_label outside [0, C) leaves that row's rank unspecified and nothing else.  No atomics; outputs
 * are bitwise the same from call to call.  No workspace.  Launches: the zero fill of scores when given, then one vote
 * kernel (one wave per query).  tests/knn_ref.py is the numpy statement of all of the above.
 * GCA_EINVAL (nothing launched, nothing written) for k outside [1, 64], kvote outside [1, k], C < 1, negative sizes,
 * ng >= 2^31, nq >= 2^31, nq * C >= 2^31 with scores, another weighting, inv_T negative or not finite, rank without
 * q_label, a NULL idx / dist / pred (or g_label with ng > 0).  nq == 0: returns 0, nothing launched. */
int gca_knn_vote(const int32_t* idx, const float* dist, int64_t nq, int32_t k, int32_t kvote,
                 const int64_t* g_label, int64_t ng, const int64_t* q_label, int64_t self_base, int64_t C,
                 int32_t weighting, float inv_T, float* scores, int32_t* pred, int32_t* rank, void* stream);

/* ---------------------------------------------------------------------------------------
 * NT-Xent: SimCLR's in-batch contrastive loss and its gradient (csrc/ntxent.hip).  The reference trains with a MoCo queue
 * or SimSiam only; this is the objective its LARS-era relatives use (every other clip of the batch is a negative, no queue,
 * no momentum encoder), on the reference's own encoder + 'mlp' head + Normalize (lib/modeling/graph_wrappers.py:9-27).
 *   z (N, D) fp32, N = 2b: rows 0..b-1 are view 1, rows b..2b-1 are view 2;  pos(i) = (i + b) mod N
 *   s[i,j]  = (sum_d z[i,d] * z[j,d]) * inv_T
 *   lse[i]  = m_i + log sum_{j != i} exp(s[i,j] - m_i),  m_i = max_{j != i} s[i,j]      (rows need not be unit-norm)
 *   sp[i]   = s[i, pos(i)]
 *   loss    = (1/N) sum_i (lse[i] - sp[i])
 *   rank[i] = #{ j : j != i, j != pos(i), s[i,j] >= sp[i] }          (top-k hit iff rank < k, as rank_ge of the InfoNCE entry)
 *   P[i,j]  = exp(s[i,j] - lse[i]) for j != i, 0 on the diagonal
 *   dz[i,:] = g * inv_T / N * ( sum_j (P[i,j] + P[j,i]) z[j,:] - 2 z[pos(i),:] ),   g = gscale_host * (gscale_dev ? *gscale_dev : 1)
 * Products on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation); sp[i] is computed by the same fma chain as the
 * streamed s[i,pos(i)], so ties with the positive compare equal.  No N x N tensor, no atomics: outputs are bitwise the same
 * from call to call.  No host sync, allocation or read: both entries can be captured in a hipGraph.  Launches: forward 2
 * (tiles, then the fold of the column splits + loss), backward 2 (tiles, then the fold of the row splits + scale).
 * pos_logit and rank_ge may be NULL.  `ws`: gca_ntxent_ws_bytes(N, D) bytes (always > 0 for valid sizes), shared by both.
 * gca_ntxent_path reports the dispatch for these sizes (`aligned`: z, dz and ws 16-byte aligned): returns 1 for the fast path
 * (D <= 128, D % 4 == 0, aligned; 4 waves per workgroup), 0 for the generic one (1 wave), and writes the waves per workgroup
 * and the number of tile splits when the pointers are non-NULL.  tests/ntxent_ref.py restates arithmetic and dispatch.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_ntxent_ws_bytes) for N odd, N < 2, N > 65536, D < 1,
 * N * D >= 2^31, inv_T not finite or <= 0, a NULL z / row_lse / loss / dz / ws. */
int64_t gca_ntxent_ws_bytes(int64_t N, int64_t D);
int gca_ntxent_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits);
int gca_ntxent_fwd(const float* z, int64_t N, int64_t D, float inv_T, float* row_lse, float* pos_logit, int32_t* rank_ge,
                   float* loss, void* ws, void* stream);
int gca_ntxent_bwd(const float* z, const float* row_lse, int64_t N, int64_t D, float inv_T, const float* gscale_dev,
                   float gscale_host, float* dz, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------
 * Barlow Twins: the cross-correlation (redundancy-reduction) loss of two views and its gradient (csrc/barlow.hip).  Not in
 * the reference; it needs no negatives, queue, momentum encoder or predictor.  z1, z2 (N, D) fp32 contiguous: the projector
 * outputs of view 1 / view 2 of the same N clips.  Per view v and column d, in two passes:
 *   mean_v[d] = (sum_n z_v[n,d]) / N      var_v[d] = (sum_n (z_v[n,d] - mean_v[d])^2) / N      rstd_v[d] = 1 / sqrt(var_v[d] + eps)
 *   a = (z1 - mean_1) * rstd_1            b = (z2 - mean_2) * rstd_2          (BatchNorm1d(affine=False); never stored)
 *   C[i,j]  = (sum_n a[n,i] * b[n,j]) / N
 *   on = sum_i (C[i,i] - 1)^2             off = sum_{i != j} C[i,j]^2         loss = on + lambda * off
 *   G[i,j]  = 2 (C[i,i] - 1) if i == j else 2 lambda C[i,j]                   (formed from cmat on load; never stored)
 *   r1[i]   = sum_j G[i,j] C[i,j]         r2[j] = sum_i G[i,j] C[i,j]
 *   dz1[n,i] = g * rstd_1[i] / N * (sum_j G[i,j] b[n,j] - a[n,i] r1[i])
 *   dz2[n,j] = g * rstd_2[j] / N * (sum_i G[i,j] a[n,i] - b[n,j] r2[j]),      g = gscale_host * (gscale_dev ? *gscale_dev : 1)
 * the full gradient through the standardisation (its mean term vanishes: a and b have zero column means).
 * Saved state, caller-owned, written by the forward and read by the backward: stats (4, D) = mean_1, rstd_1, mean_2, rstd_2;
 * cmat (D, D) = C, 4 D^2 bytes; rsum (2, D) = r1, r2.  loss[3] = loss, on, off.  `ws`: gca_barlow_ws_bytes(N, D) bytes
 * (always > 0 for valid sizes) of scratch; nothing survives in it between the two entries.
 * Products on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation).  No atomics: outputs are bitwise the same from call to
 * call.  No host sync, allocation or read: both entries can be captured in a hipGraph.  Launches: forward 3 (column
 * statistics; C tiles with per-tile partials of on / off / r1 / r2; their fold), backward 1 (both views).  One dispatch path
 * (guarded 4-byte accesses, no alignment assumed).  tests/barlow_ref.py restates the arithmetic.
 * eps == 0 with a constant column gives var = 0, rstd = inf and inf / NaN outputs by the formula: the caller's business, not
 * a refusal.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_barlow_ws_bytes) for N < 2, N > 65536, D < 1, D > 8192,
 * N * D >= 2^31, lambda or eps negative or not finite, gscale_host not finite, any NULL pointer other than gscale_dev. */
int64_t gca_barlow_ws_bytes(int64_t N, int64_t D);
int gca_barlow_fwd(const float* z1, const float* z2, int64_t N, int64_t D, float lambda, float eps, float* stats, float* cmat,
                   float* rsum, float* loss, void* ws, void* stream);
int gca_barlow_bwd(const float* z1, const float* z2, const float* stats, const float* cmat, const float* rsum, int64_t N,
                   int64_t D, float lambda, const float* gscale_dev, float gscale_host, float* dz1, float* dz2, void* ws,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * VICReg: the variance / invariance / covariance loss of two views and its gradient (csrc/vicreg.hip).  Not in the reference;
 * like Barlow Twins it needs no negatives, queue, momentum encoder or predictor, and it does not standardise the features.
 * z1, z2 (N, D) fp32 contiguous: the projector outputs of view 1 / view 2 of the same N clips.  Per view v (x = z_v), in two passes:
 *   mean_v[d] = (sum_n x[n,d]) / N        xc = x - mean_v       var_v[d] = (sum_n xc[n,d]^2) / (N - 1)    (unbiased)
 *   sd_v[d]   = sqrt(var_v[d] + eps)                            Cov_v[i,j] = (sum_n xc[n,i] xc[n,j]) / (N - 1)
 *   inv  = sum_{n,d} (z1 - z2)^2 / (N D)      varl = sum_v sum_d max(0, 1 - sd_v[d]) / (2 D)      covl = sum_v sum_{i != j} Cov_v[i,j]^2 / D
 *   loss = sim * inv + std * varl + cov * covl
 *   dz_v[n,j] = g * (s_v * 2 sim (z1 - z2)[n,j] / (N D) - std * [sd_v[j] < 1] * xc[n,j] / (2 D sd_v[j] (N - 1))
 *                    + 4 cov / (D (N - 1)) * sum_{i != j} xc[n,i] Cov_v[i,j]),      s_1 = +1, s_2 = -1,
 *   g = gscale_host * (gscale_dev ? *gscale_dev : 1), as in gca_barlow_bwd.  The centring adds no term to the gradient.
 * Saved state, caller-owned, written by the forward and read by the backward: stats (4, D) = mean_1, sd_1, mean_2, sd_2;
 * covm (2, D, D) = Cov_1, Cov_2 (diagonals included), 8 D^2 bytes.  loss4[4] = loss, inv, varl, covl (the parts unweighted).
 * `ws`: gca_vicreg_ws_bytes(N, D) bytes (always > 0 for valid sizes) of scratch of the forward; the backward uses none of it.
 * Products on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation).  Cov is symmetric: only the 64 x 64 tiles on and above
 * the diagonal are computed, and each off-diagonal one is written twice.  No atomics: outputs are bitwise the same from call
 * to call.  No host sync, allocation or read: both entries can be captured in a hipGraph.  Launches: forward 3 (column
 * statistics with the hinge and invariance partials; Cov tiles with their square-sums; the fold in fp64), backward 1 (both
 * views).  One dispatch path (guarded 4-byte accesses, no alignment assumed).  tests/vicreg_ref.py restates the arithmetic.
 * eps == 0 with a constant column gives sd = 0 and 0 / 0 = NaN in that column's gradient, as the chain of torch ops does: the
 * caller's business, not a refusal.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_vicreg_ws_bytes) for N < 2, N > 65536, D < 1, D > 8192,
 * N * D >= 2^31, sim, std, cov or eps negative or not finite, gscale_host not finite, any NULL pointer other than gscale_dev. */
int64_t gca_vicreg_ws_bytes(int64_t N, int64_t D);
int gca_vicreg_fwd(const float* z1, const float* z2, int64_t N, int64_t D, float sim, float std, float cov, float eps, float* stats,
                   float* covm, float* loss4, void* ws, void* stream);
int gca_vicreg_bwd(const float* z1, const float* z2, const float* stats, const float* covm, int64_t N, int64_t D, float sim,
                   float std, float cov, const float* gscale_dev, float gscale_host, float* dz1, float* dz2, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------
 * SwAV: Sinkhorn-Knopp codes, the swapped-prediction loss of two views against learned prototypes, and its gradient
 * (csrc/swav.hip; Caron et al. 2020).  Not in the reference.  z1, z2 (N, D) and the prototypes C (K, D), fp32 contiguous, all
 * with unit rows (a precondition, not checked on the device).  Per view v:
 *   S_v = z_v C^T (N, K)                         P_v = exp((S_v - 1) / eps)      (the codes do not depend on the constant)
 *   u_v[k] = 1 / (K sum_n P_v[n,k] v_v[n])       v_v[n] = 1 / (N sum_k P_v[n,k] u_v[k])     `iters` times, v_v = 1 at first
 *   q_v[n,k] = N P_v[n,k] u_v[k] v_v[n]          the Sinkhorn-Knopp loop of the paper as two scaling vectors; no gradient
 *   lse_v[n] = log sum_k exp(S_v[n,k] / T)       l12 = -(1/N) sum_{n,k} q_2 (S_1 / T - lse_1)     l21 with 1 <-> 2
 *   loss = (l12 + l21) / 2                       dS_1 = (exp(S_1 / T - lse_1) - q_2) / (2 N T)    dS_2 with 1 <-> 2
 *   dz_v = g dS_v C       dC (+)= g (dS_1^T z_1 + dS_2^T z_2)       g = gscale_host * (gscale_dev ? *gscale_dev : 1)
 * parts[3] = loss, l12, l21.  Saved state, caller-owned, written by the forward and read by the backward: dS (2, N, K), 8 N K
 * bytes (it holds the scores until the last forward launch replaces them in place).  codes: NULL, or (2, N, K) that receives
 * q_1, q_2 (tests and monitoring).  `ws`: gca_swav_ws_bytes(N, D, K) bytes (> 0 for valid sizes) of scratch, enough for either
 * entry; nothing in it passes from the forward to the backward.
 * Products on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation), 64 x 64 tiles, all edges guarded.  Launches: forward
 * 2 iters + 2 (scores; column sums and row sums alternately, both views per grid; the last row sums with codes, loss terms and
 * dS; the fold in fp64), backward 2 or 3 (dz of both views, its reduction over K cut into gca_swav_dz_splits(N, D, K) slabs --
 * min(32, max(1, 256 / (2 ceil(N / 64) ceil(D / 64))), ceil(K / 256)) -- whose partial tiles a second launch adds in slab
 * order when there is more than one; dC over the 2 N rows, view 1 first).  No atomics: outputs are bitwise
 * the same from call to call.  No host sync, allocation or read: every entry can be captured in a hipGraph.  One dispatch
 * path, 4-byte accesses only.  tests/swav_ref.py restates the arithmetic.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_swav_ws_bytes) for N outside [2, 8192], K outside [2, 65536],
 * D outside [1, 8192], iters outside [1, 16], eps outside [0.025, 1] (exp(-2 / eps) stays a normal fp32 number), T not
 * positive or T or 1 / T not finite in fp32, gscale_host not finite, any NULL pointer other than codes and gscale_dev.
 * gca_swav_bwd never looks at how dS was made: it serves the DINO loss below as well (gca_dino_fwd's dS on the student's operands).
 * gca_rows_normalize: C[k,:] /= ||C[k,:]|| in place, one wave per row, an all-zero row left as it is; GCA_EINVAL for NULL,
 * K outside [1, 65536], D outside [1, 8192]. */
int gca_rows_normalize(float* C, int64_t K, int64_t D, void* stream);
int64_t gca_swav_ws_bytes(int64_t N, int64_t D, int64_t K);
int gca_swav_fwd(const float* z1, const float* z2, const float* C, int64_t N, int64_t D, int64_t K, float eps, float T, int64_t iters,
                 float* parts, float* dS, float* codes, void* ws, void* stream);
int gca_swav_dz_splits(int64_t N, int64_t D, int64_t K);
int gca_swav_bwd(const float* z1, const float* z2, const float* C, const float* dS, int64_t N, int64_t D, int64_t K,
                 const float* gscale_dev, float gscale_host, float* dz1, float* dz2, float* dC, int accumulate_dC, void* ws,
                 void* stream);

/* ---------------------------------------------------------------------------------------
 * DINO: self-distillation from a centred momentum teacher (csrc/dino.hip; Caron et al. 2021).  Not in the reference.  Student
 * features zs1, zs2 (N, D) and prototypes Cs (K, D), teacher features zt1, zt2 (N, D) and prototypes Ct (K, D), fp32 contiguous,
 * all with unit rows (a precondition, not checked on the device); the centre `center` (K).  Per view v:
 *   Ss_v = zs_v Cs^T     St_v = zt_v Ct^T  (N, K)     p_v = softmax((St_v - c) / Tt)  (rows; no gradient)
 *   ls_v = Ss_v / Ts - lse(Ss_v / Ts)      l12 = -(1/N) sum_{n,k} p_1 ls_2      l21 = -(1/N) sum_{n,k} p_2 ls_1
 *   loss = (l12 + l21) / 2                 ent = -(1/(2N)) sum_{v,n,k} p_v ((St_v - c) / Tt - lse_t)   (mean teacher entropy)
 *   dSs_2 = (exp(ls_2) - p_1) / (2 N Ts)   dSs_1 = (exp(ls_1) - p_2) / (2 N Ts)
 *   c' = cm c + (1 - cm) (1/(2N)) sum_{v,n} St_v[n,:]     written after the loss has used c, and only when update_center != 0
 * parts[4] = loss, l12, l21, ent.  Ts and cm are host floats; the teacher temperature Tt is read from the one device float
 * tt_dev, so a captured graph follows its warm-up schedule (the host that writes it checks it: positive, Tt and 1 / Tt finite).
 * Saved state, caller-owned: dS (2, N, K), 8 N K bytes -- it holds the student scores until the row launch replaces them in
 * place -- and is all the backward needs: gca_swav_bwd(zs1, zs2, Cs, dS, ...) gives dzs1, dzs2 and dCs.  probs: NULL, or
 * (2, N, K) that receives p_1, p_2 (tests and monitoring).  `ws`: gca_dino_ws_bytes(N, D, K) = (2 N K + 4 N) 4 bytes: the teacher
 * scores and the row terms; nothing in it outlives the call.
 * Launches: 3 or 4.  The four products in one grid on v_mfma_f32_32x32x2_f32 (exact fp32), 64 x 64 tiles, all edges guarded;
 * one 256-thread workgroup per row and direction (online max / sum of the teacher row and the student row, then a second
 * sweep: probabilities, dS, the row's loss and entropy terms); the centre (column sums over the 2 N teacher rows, view 1
 * first, then the EMA) behind it in stream order; the fp64 fold of the 2 N row terms.  No atomics: outputs are bitwise the
 * same from call to call.  No host sync, allocation or read: capturable in a hipGraph.  One dispatch path, 4-byte accesses only.
 * tests/dino_ref.py restates the arithmetic.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_dino_ws_bytes) for N outside [2, 8192], K outside [2, 65536],
 * D outside [1, 8192], Ts not positive or Ts or 1 / Ts not finite in fp32, cm outside [0, 1), any NULL pointer other than
 * probs. */
enum { GCA_DINO_ROW_WORKGROUP = 0, GCA_DINO_ROW_WAVE = 1 };
int64_t gca_dino_ws_bytes(int64_t N, int64_t D, int64_t K);
int gca_dino_fwd(const float* zs1, const float* zs2, const float* Cs, const float* zt1, const float* zt2, const float* Ct, int64_t N,
                 int64_t D, int64_t K, float Ts, const float* tt_dev, float cm, float* center, int update_center, float* parts,
                 float* dS, float* probs, void* ws, void* stream);
/* gca_dino_fwd with the row launch's grid chosen by the caller: GCA_DINO_ROW_WORKGROUP, what gca_dino_fwd uses, or
 * GCA_DINO_ROW_WAVE, one wave per row and direction as SwAV's row kernels have it (tools/dino_micro.py times both; each is
 * reproducible on its own, the two differ in their fold order).  GCA_EINVAL for any other row_grid. */
int gca_dino_fwd_grid(const float* zs1, const float* zs2, const float* Cs, const float* zt1, const float* zt2, const float* Ct,
                      int64_t N, int64_t D, int64_t K, float Ts, const float* tt_dev, float cm, float* center, int update_center,
                      float* parts, float* dS, float* probs, int row_grid, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------
 * MoCo v3: the queue-free, symmetrised cross-view InfoNCE of Chen, Xie, He 2021 (Algorithm 1) and its gradient
 * (csrc/mocov3.hip).  Not in the reference.  q1, q2 (N, D) fp32 contiguous: the student's predictor outputs of the two views;
 * k1, k2 (N, D): the momentum teacher's projector outputs (rows need not be unit-norm).  Direction 0 pairs (q, k) = (q1, k2),
 * direction 1 pairs (q2, k1); per direction d:
 *   s[i,j]  = (sum_e q[i,e] * k[j,e]) * inv_T
 *   lse[i]  = m_i + log sum_j exp(s[i,j] - m_i),  m_i = max_j s[i,j]      (ALL j: the positive is inside the softmax)
 *   sp[i]   = s[i,i]
 *   l_d     = (1/N) sum_i (lse[i] - sp[i])
 *   rank[i] = #{ j != i : s[i,j] >= sp[i] }                              (top-k hit iff rank < k)
 *   P[i,j]  = exp(s[i,j] - lse[i])
 *   dq[i,:] = g * w * inv_T / N * ( sum_j P[i,j] k[j,:] - k[i,:] ),   g = gscale_host * (gscale_dev ? *gscale_dev : 1)
 *   loss    = w * (l_0 + l_1)          (the paper: w = 2 T).  Nothing flows to k1 / k2: the teacher is detached.
 * row_lse, pos_logit, rank_ge hold 2 N entries, direction 0 first; loss holds 3 floats: w (l_0 + l_1), l_0, l_1.
 * Guarantees:
 *   products     v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation, bitwise an fmaf chain); no N x N tensor is formed.
 *   one grid     both directions of a pass run in ONE grid.  Launches: forward 2 (tiles, then the fold of the column splits +
 *                losses), backward 2 (tiles, then the fold of the column splits, the -k[i,:] term and the scale).
 *   positive     sp[i] is the diagonal of the diagonal tile, computed first by the same k-ordered fma chain as the streamed
 *                s[i,i]: ties with the positive compare equal.
 *   forward      online max, sum and count per row; column splits folded in split order.
 *   backward     a workgroup owns a 32-row tile of dq and streams the tiles of k; the s tile is recomputed transposed, so P is
 *                already the A operand of sum_j P[i,j] k[j,:] (no trip through LDS); the fast path holds the whole dq tile in
 *                accumulators; splits go to `ws` and are added in split order.  It recomputes s by the forward's chain:
 *                N = 1 gives lse == sp, loss 0 and dq exactly 0.
 *   determinism  no atomics, one owner per output element, fixed fold orders: outputs are bitwise the same from call to call.
 *   capture      no host sync, allocation or read: both entries can be captured in a hipGraph.
 *   dispatch     a function of the arguments alone, never of the device.  gca_mocov3_path reports it (`aligned`: every
 *                pointer, outputs and ws included, 16-byte aligned): returns 1 for the fast path (D <= 256, D % 4 == 0,
 *                aligned; 4 waves per workgroup, float4 loads with the next piece in flight under the current MFMAs, s
 *                accumulated over 128-feature chunks -- two are what the LDS holds next to the four wave tiles), 0 for the
 *                generic one (1 wave), and writes the waves per workgroup and the number of tile splits (ntxent's rule, per
 *                direction) when the pointers are non-NULL.  tests/mocov3_ref.py restates arithmetic and dispatch.
 * pos_logit and rank_ge may be NULL.  `ws`: gca_mocov3_ws_bytes(N, D) bytes (always > 0 for valid sizes), shared by both.
 * GCA_EINVAL (nothing launched, nothing written; -1 from gca_mocov3_ws_bytes) for N < 1, N > 65536, D < 1, N * D >= 2^31,
 * inv_T or w not finite or <= 0, a NULL q1 / q2 / k1 / k2 / row_lse / loss / dq1 / dq2 / ws, and in the backward entry dq1 or
 * dq2 overlapping each other or any of q1, q2, k1, k2 (dq is written while other workgroups still read the inputs). */
int64_t gca_mocov3_ws_bytes(int64_t N, int64_t D);
int gca_mocov3_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits);
int gca_mocov3_fwd(const float* q1, const float* q2, const float* k1, const float* k2, int64_t N, int64_t D, float inv_T,
                   float w, float* row_lse, float* pos_logit, int32_t* rank_ge, float* loss, void* ws, void* stream);
int gca_mocov3_bwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* row_lse, int64_t N,
                   int64_t D, float inv_T, float w, const float* gscale_dev, float gscale_host, float* dq1, float* dq2, void* ws,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * NNCLR: nearest-neighbour contrastive learning (Dwibedi et al. 2021, Algorithm 1) -- the support-set search with its gather,
 * and the loss gradient to the predictions (csrc/nnclr.hip).  Not in the reference.  The forward loss needs no entry of its
 * own: gca_mocov3_fwd(q1 = nn1, q2 = nn2, k1 = p1, k2 = p2, w = 1/2) is L(nn1, p2) / 2 + L(nn2, p1) / 2.
 * Search.  z1, z2 (N, D): the projections of the two views; Q (K, D): the support set (a FIFO of past projections); all
 * contiguous fp32, unit rows are the caller's business.  Per view v:
 *   s[v][i,j]  = sum_e z_v[i,e] * Q[j,e]
 *   key(s)     = s, or -inf where s is NaN
 *   idx[v][i]  = the smallest j that attains max_j key(s[v][i,j])        (int32, ALWAYS in [0, K), whatever the inputs)
 *   sim[v][i]  = that key
 *   nn_v[i,:]  = Q[idx[v][i],:]                                          (copied bit for bit)
 * idx and sim hold 2 N entries, view 1 first.
 * Backward.  nn1, nn2, p1, p2 (N, D); row_lse (2 N) as gca_mocov3_fwd(nn1, nn2, p1, p2, ...) wrote it.  Direction 0 has rows nn1
 * and columns p2, direction 1 rows nn2 and columns p1; per direction, with s[i,j] = (nn[i] . p[j]) * inv_T:
 *   P[i,j]     = exp(s[i,j] - lse[i])                                    (the softmax runs over the predictions)
 *   dp[j,:]    = g * w * inv_T / N * ( sum_i P[i,j] nn[i,:] - nn[j,:] ),   g = gscale_host * (gscale_dev ? *gscale_dev : 1)
 * dp2 comes from direction 0 and dp1 from direction 1.  Nothing flows to nn1 / nn2.
 * Guarantees:
 *   products     v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation, one k-ordered fma chain per element); neither a
 *                (2 N, K) nor an N x N tensor is formed.
 *   one pass     the search scores a staged tile of Q against the row tiles of BOTH views before the next one is fetched;
 *                4 row tiles (128 rows of the two views together) sit beside it in LDS, so up to N = 64 per view the support
 *                set is read once per call, past that once per 128 rows.
 *   launches     search 2: per-split (best key, best j) pairs to `ws`, then the fold of the splits in split order (the lower
 *                index wins a tie -- the ONE order on pairs used throughout), idx, sim and the gather.  Backward 2: tiles,
 *                then the fold of the splits of the streamed rows in split order, the -nn[j,:] term and the scale.
 *   backward     a workgroup owns a 32-row tile of dp and streams the tiles of nn with their lse; s is recomputed by the
 *                forward's chain, so N = 1 gives dp exactly 0.  The kernels are gca_mocov3_bwd's (csrc/xview_tile.h) with the
 *                log-sum-exp taken by streamed row instead of by owned row.
 *   determinism  no atomics, one owner per output element, fixed fold orders: outputs are bitwise the same from call to call.
 *   capture      no host sync, allocation or read: both entries can be captured in a hipGraph.
 *   dispatch     a function of the arguments alone, never of the device.  gca_nnclr_search_path (`aligned`: z1, z2, Q 16-byte
 *                aligned) and gca_nnclr_bwd_path (`aligned`: every pointer, outputs and ws included) return 1 for the fast path
 *                (D <= 256, D % 4 == 0, aligned; 4 waves per workgroup, float4 loads with the next piece in flight under the
 *                current MFMAs), 0 for the generic one (1 wave), and write waves per workgroup and the number of splits.
 *                Search: kt = ceil(K / 32) tiles, G = ceil(2 ceil(N / 32) / 4) row-tile groups (fast; 2 ceil(N / 32)
 *                generic), want = clamp(ceil(256 / G), 1, kt), tps = ceil(kt / want), splits = ceil(kt / tps).  Backward:
 *                gca_mocov3_path's rule.  tests/nnclr_ref.py restates arithmetic and dispatch.
 * `ws`: gca_nnclr_search_ws_bytes(N, D, K) / gca_nnclr_bwd_ws_bytes(N, D) bytes (always > 0 for valid sizes).
 * GCA_EINVAL (nothing launched, nothing written; -1 from the ws_bytes functions) for N < 1, N > 65536, D < 1, N * D >= 2^31,
 * and in the search K < 1, K >= 2^31, K * D >= 2^31, a NULL z1 / z2 / Q / idx / sim / nn1 / nn2 / ws, ws_bytes below
 * gca_nnclr_search_ws_bytes, nn1 or nn2 overlapping each other, Q, z1 or z2; in the backward entry inv_T or w not finite or
 * <= 0, a NULL nn1 / nn2 / p1 / p2 / row_lse / dp1 / dp2 / ws, dp1 or dp2 overlapping each other or any of nn1, nn2, p1, p2. */
int64_t gca_nnclr_search_ws_bytes(int64_t N, int64_t D, int64_t K);
int gca_nnclr_search_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits);
int gca_nnclr_search(const float* z1, const float* z2, const float* Q, int64_t N, int64_t D, int64_t K, int32_t* idx, float* sim,
                     float* nn1, float* nn2, void* ws, int64_t ws_bytes, void* stream);
int64_t gca_nnclr_bwd_ws_bytes(int64_t N, int64_t D);
int gca_nnclr_bwd_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits);
int gca_nnclr_bwd(const float* nn1, const float* nn2, const float* p1, const float* p2, const float* row_lse, int64_t N,
                  int64_t D, float inv_T, float w, const float* gscale_dev, float gscale_host, float* dp1, float* dp2, void* ws,
                  void* stream);

/* ---------------------------------------------------------------------------------------
 * ReSSL: relational self-supervised learning (Zheng et al. 2021) -- the teacher-weighted relational loss of student rows
 * against the MoCo queue, and its gradient to the student (csrc/ressl.hip).  Not in the reference.
 * q, k (N, D): student and teacher rows (nothing flows to k); Q (K, D): the queue BEFORE this step's enqueue; all contiguous fp32.
 *   s[i,j] = inv_Ts q_i . Q_j,  t[i,j] = inv_Tt k_i . Q_j      exact-fp32 matrix cores, one k-ordered chain per score
 *   row_lse[i] = logsumexp_j s[i,:],  row_lse[N + i] = logsumexp_j t[i,:];   Ps = exp(s - lse_s),  Pt = exp(t - lse_t)
 *   row_loss[i] = lse_s[i] - sum_j Pt[i,j] s[i,j];   out[0] = mean_i row_loss[i]
 *   out[1] = mean_i (lse_t[i] - sum_j Pt[i,j] t[i,j])             the teacher's entropy
 *   dq[i,:] = g inv_Ts / N (sum_j Ps[i,j] Q_j - sum_j Pt[i,j] Q_j),  g = gscale_host * (*gscale_dev if not NULL)
 *   forward      ONE pass over Q: six running scalars per row (two maxima, two sums, two teacher-weighted sums), one record
 *                per (K-split, row) in `ws`, folded in split order by a second, one-workgroup launch that also takes the two
 *                means through one fixed tree.  Columns past K are -inf before the maximum.  No (N, K) tensor.
 *   backward     grid (K-splits, row tiles, 2 sides): side 0 owns q with lse_s and inv_Ts, side 1 owns k with lse_t and inv_Tt,
 *                the same instructions; P is recomputed by the forward's chain and multiplied into the streamed rows from
 *                registers; one slab per (split, side) in `ws`, summed in split order by the launch that writes dq.
 *   determinism  no atomics, one owner per output element, fixed fold orders: outputs are bitwise the same from call to call.
 *   capture      no host sync, allocation or read: both entries can be captured in a hipGraph.
 *   dispatch     a function of the arguments alone.  gca_ressl_fwd_path (`aligned`: q, k, Q 16-byte aligned) and
 *                gca_ressl_bwd_path (`aligned`: q, k, Q and ws) return 1 for the fast path (D <= 256, D % 4 == 0, aligned;
 *                4 waves), 0 for the generic one (1 wave), and write waves per workgroup and the number of splits:
 *                kt = ceil(K / 32), G = ceil(N / 32) (forward) or 2 ceil(N / 32) (backward), want = clamp(ceil(256 / G), 1,
 *                ceil(kt / waves)), tps = ceil(kt / want), splits = ceil(kt / tps) -- no split is empty.
 * `ws`: gca_ressl_fwd_ws_bytes / gca_ressl_bwd_ws_bytes (N, D, K) bytes (always > 0 for valid sizes).
 * GCA_EINVAL (nothing launched, nothing written; -1 from the ws_bytes functions) for N < 1, N > 65536, D < 1, K < 1, K >= 2^31,
 * N * D or K * D >= 2^31, inv_Ts or inv_Tt not finite or <= 0, a NULL pointer other than gscale_dev, ws_bytes too small, an
 * output (row_lse, row_loss, out; dq) overlapping an input or another output. */
int64_t gca_ressl_fwd_ws_bytes(int64_t N, int64_t D, int64_t K);
int64_t gca_ressl_bwd_ws_bytes(int64_t N, int64_t D, int64_t K);
int gca_ressl_fwd_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits);
int gca_ressl_bwd_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits);
int gca_ressl_fwd(const float* q, const float* k, const float* Q, int64_t N, int64_t D, int64_t K, float inv_Ts, float inv_Tt,
                  float* row_lse, float* row_loss, float* out, void* ws, int64_t ws_bytes, void* stream);
int gca_ressl_bwd(const float* q, const float* k, const float* Q, const float* row_lse, int64_t N, int64_t D, int64_t K,
                  float inv_Ts, float inv_Tt, const float* gscale_dev, float gscale_host, float* dq, void* ws, int64_t ws_bytes,
                  void* stream);

/* ---------------------------------------------------------------------------------------
 * Action-recognition class head (lib/modeling/model_wrappers.py:74-82,99-117: nn.Linear on the pooled features) fused with
 * nn.CrossEntropyLoss (tools/train_ds.py:111-112) and accuracy() (:120).  x (b, F), w (C, F), logits (b, C) contiguous fp32;
 * bias (C) or NULL; target (b) int64.
 *   logits[i,j] = (sum_d x[i,d] * w[j,d]) + bias[j]    fp32 matrix cores, fp32 accumulation, the bias added once at the end
 *   row_lse[i]  = m_i + log sum_j exp(logits[i,j] - m_i), m_i the row maximum
 *   rank_ge[i]  = gca_rank_ge of the stored logits;  loss[0] = (1/b) sum_i (row_lse[i] - logits[i,target[i]])
 * target == NULL writes the logits only (and row_lse if given): the eval path.  rank_ge and loss may each be NULL; loss and
 * rank_ge need target, target needs row_lse.  x == w == bias == NULL with a target: `logits` is an input and only the row
 * statistics and the loss are computed (nn.CrossEntropyLoss of existing logits).
 *   backward: g[i,j] = s (exp(logits[i,j] - row_lse[i]) - [j == target[i]]), s = gscale_host * (gscale_dev ? *gscale_dev : 1) / b,
 *   formed on the fly;  dw[j,d] (+)= sum_i g[i,j] x[i,d];  dbias[j] (+)= sum_i g[i,j] (dbias may be NULL; `accumulate`
 *   covers both);  dx[i,d] (+)= sum_j g[i,j] w[j,d], skipped for dx == NULL (linear probe).
 * The target's column is found by comparing indices inside the sweep, never by address: a target outside [0, C) reads and
 * writes nothing out of bounds (the row's results are unspecified; the host layer checks the labels).  No floating-point
 * atomics, every sum in an order fixed by the shapes: outputs are bitwise the same from call to call.  At most three
 * launches forward (tiles, row statistics, loss) and three backward (dw + dbias, for b > 512 the fold of its per-run slabs,
 * dx), all on `stream`.  ws: gca_classifier_ws_bytes() bytes (one loss term per row, and for b > 512 ceil(b / 512) <= 16
 * slabs of C * F + C floats); ws_bytes is checked.  tests/classify_ref.py is the fp64 statement of all of the above.
 * GCA_EINVAL (nothing launched) for F < 1, C < 1, b < 0, a size of 2^31 or more, ws_bytes too small, loss or rank_ge without
 * target, target without row_lse.  b == 0: returns 0, nothing launched. */
int64_t gca_classifier_ws_bytes(int64_t b, int64_t F, int64_t C);
int gca_classifier_fwd(const float* x, const float* w, const float* bias, const int64_t* target,
                       int64_t b, int64_t F, int64_t C, float* logits, float* row_lse, int32_t* rank_ge,
                       float* loss, void* ws, int64_t ws_bytes, void* stream);
int gca_classifier_bwd(const float* x, const float* w, const float* logits, const float* row_lse,
                       const int64_t* target, const float* gscale_dev, float gscale_host,
                       int64_t b, int64_t F, int64_t C, float* dw, float* dbias, int accumulate,
                       float* dx, int dx_accumulate, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-tensor parameter updates over flat, 256-element-aligned parameter arenas.
 * _momentum_update (tools/train_video_contrast_dis.py:177-180) and torch.optim.SGD as
 * configured by make_optimizer (lib/solver/build.py:24-59: one group per parameter).
 * ------------------------------------------------------------------------------------- */
int gca_ema_update(float* p_ema, const float* p, int64_t n, float m, void* stream);
/* The same update with the momentum read from one device float (a captured step follows a momentum schedule); any n >= 1,
 * no alignment required. */
int gca_ema_update_dev(float* p_ema, const float* p, int64_t n, const float* m_dev, void* stream);
/* seg table: per 256-element chunk i: lr[i], wd[i] (device arrays of length n/256).
 * grad_clip: NULL, or the 4-float result of gca_grad_clip_coef / gca_grad_unscale_clip -- every gradient is multiplied by
 * grad_clip[1] on the fly (the grads.mul_(clip_coef) pass of clip_grad_norm_ without a pass over the arena), and when
 * grad_clip[2] != 0 (a non-finite gradient under loss scaling) the whole update is skipped: parameters and momentum stay
 * as they are, as apex amp skips optimizer.step() (tools/train_video_contrast_dis.py:413-419 under APEX.FLAG). */
int gca_sgd_step(float* p, const float* grad, float* mom_buf, int64_t n, const float* chunk_lr,
                 const float* chunk_wd, float lr_scale, float momentum, int nesterov, int first_step,
                 const float* grad_clip, void* stream);
/* LARS (apex LARC(clip = False) around torch.optim.SGD, dampening 0) over the same arena layout and chunk tables as
 * gca_sgd_step (n % 256 == 0).  For tensor i with weights w, its chunks' lr / wd, coef = grad_clip[1] (1 without a record):
 *   g = grad * coef;  nw = ||w||_2;  ng = ||g||_2 = coef * ||grad||_2
 *   q = trust_coef * nw / (ng + wd * nw + eps)   if adapt[i] and nw > 0 and ng > 0, else 1
 *   d = q * (g + wd * w);  buf = momentum * buf + d;  w -= lr * (nesterov ? d + momentum * buf : buf)
 * Three launches on `stream`, no host sync, no atomics, every sum in a fixed order (bit-reproducible):
 *   1. one workgroup per job sums w^2 and grad^2 in fp64 -> partials[2 * job], partials[2 * job + 1];
 *   2. one workgroup per tensor folds its jobs' partials in job order, writes norms[2 * i] = nw, norms[2 * i + 1] = ng (fp64),
 *      forms q in fp64, rounds it once to fp32 and writes trust[i] and chunk_trust[c] for every chunk c of the tensor;
 *   3. gca_sgd_step's kernel with the per-chunk factor q, in the order written above.
 * Host tables, int32, built once per arena and resident on the device:
 *   jobs   [n_jobs][3]   (tensor, first chunk, chunk count <= gca_lars_job_chunks()); a job lies inside ONE tensor, the jobs
 *                        of a tensor are consecutive and in chunk order, every chunk of the arena is in exactly one job
 *   params [n_params][4] (first job, job count, first chunk, chunk count) of every tensor
 *   adapt  [n_params]    non-zero: the tensor takes the trust ratio (torch-side rule: p.ndim > 1)
 * The library cannot see inside them: indices out of range are out-of-bounds accesses.  partials: 2 * n_jobs doubles;
 * norms: 2 * n_params doubles; trust: n_params floats; chunk_trust: n / 256 floats.  trust_coef > 0, eps >= 0,
 * 0 <= momentum < 1.  grad_clip as for gca_sgd_step, read on the device by all three launches: when grad_clip[2] != 0
 * neither p, mom_buf, norms, trust nor chunk_trust change.  Padding elements (p = grad = buf = 0) stay exactly 0.  A tensor
 * with q == 1 takes gca_sgd_step's (lr_scale = 1) operations bit for bit. */
int gca_lars_job_chunks(void);
int gca_lars_step(float* p, const float* grad, float* mom_buf, int64_t n, const float* chunk_lr, const float* chunk_wd,
                  const int32_t* jobs, int64_t n_jobs, const int32_t* params, const int32_t* adapt, int64_t n_params,
                  double* partials, double* norms, float* trust, float* chunk_trust, float momentum, int nesterov,
                  double trust_coef, double eps, const float* grad_clip, void* stream);
/* torch.optim.Adam (decoupled = 0) / AdamW (decoupled = 1), amsgrad = False, over the same arena layout and chunk tables
 * as gca_sgd_step (n % 256 == 0), for step t = state[0] + 1:
 *   g = grad * grad_clip[1];  Adam: g += wd * p   AdamW: p *= 1 - lr * wd
 *   m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * g * g
 *   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * state: ONE int64 on the device, the number of steps taken.  gca_adam_step only reads it (the bias corrections are formed
 * in fp64 from it inside the kernel); gca_adam_advance, a one-thread launch behind it, increments it -- so a captured
 * hipGraph that replays both keeps counting.  0 <= beta < 1, eps > 0.  grad_clip as for gca_sgd_step: when grad_clip[2] != 0
 * neither p, exp_avg, exp_avg_sq nor the step count change.  Padding elements (p = grad = m = v = 0) stay exactly 0. */
int gca_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* chunk_lr,
                  const float* chunk_wd, double beta1, double beta2, double eps, int decoupled, const float* grad_clip,
                  const int64_t* state, void* stream);
int gca_adam_advance(int64_t* state, const float* grad_clip, void* stream);
/* clip_grad_norm_(parameters, max_norm) of tools/train_video_contrast_dis.py:420-423 over the flat gradient arena
 * (n % 4 == 0; padding elements are zero): out4[0] = total 2-norm, out4[1] = min(1, max_norm / (norm + 1e-6)),
 * out4[2] = out4[3] = 0.  fp64 partial sums folded in a fixed order (deterministic); `ws` = gca_grad_clip_ws_bytes() bytes. */
int64_t gca_grad_clip_ws_bytes(void);
int gca_grad_clip_coef(const float* grad, int64_t n, float max_norm, float* out4, void* ws, void* stream);
/* Dynamic loss scaling for the fp16-storage path -- what `amp.scale_loss(loss, optimizer)` + the patched optimizer.step()
 * do in the reference (tools/train_video_contrast_dis.py:134-141 amp.initialize, :413-418 scale_loss; apex's LossScaler:
 * 2x after 2000 clean steps, 0.5x and a skipped step on inf / nan), decided ON THE DEVICE (no host sync, hipGraph-safe):
 *   scale_state4 = {loss scale S, clean steps in a row, skipped steps, steps seen}; S is read by the loss-gradient kernels
 *   through their gscale_dev argument (gca_moco_logits_bwd, gca_nce_softmax_loss_bwd, gca_scale_dev).
 *   out4[0] = 2-norm of grad / S, out4[1] = (1/S) * clip coefficient (max_norm <= 0: no clipping) -- the factor the SGD
 *   kernel multiplies every gradient by, out4[2] = 1 when any element of grad is inf / nan (then out4[1] = 0, S is
 *   multiplied by `backoff` and gca_sgd_step leaves parameters and momentum untouched), out4[3] = the S these gradients
 *   were computed with.  After `growth_interval` clean steps S *= growth (capped at max_scale). `ws`: gca_grad_clip_ws_bytes(). */
int gca_grad_unscale_clip(const float* grad, int64_t n, float max_norm, float* scale_state4, float growth, float backoff,
                          int growth_interval, float max_scale, float* out4, void* ws, void* stream);
int gca_scale_dev(float* y, int64_t n, const float* a_dev, float a_host, void* stream);   /* y *= (*a_dev) * a_host */
int gca_fill(float* p, int64_t n, float v, void* stream);
int gca_axpy(float* y, const float* x, int64_t n, float a, void* stream);          /* y += a*x */
int gca_scale(float* y, int64_t n, float a, void* stream);
/* fp16-storage path: y += a*x on fp16 tensors (fp32 arithmetic, one rounding), and the fp32 -> fp16 cast of the input clips */
int gca_axpy_f16(void* y, const void* x, int64_t n, float a, void* stream);
/* rows x row_elems (row_elems % 4 == 0), source rows src_row_stride elements apart (a channel slice of a clip batch) */
int gca_cast_f16(const float* x, int64_t rows, int64_t row_elems, int64_t src_row_stride, void* y, void* stream);
/* dst[r,:] = src[idx[r]*src_row_stride : +row_elems]; rows <= 65535.  src rows may be strided (the key view of a
 * (b,6,T,H,W) batch is gathered in place for the ShuffleBN exchange, tools/...dis.py:404,213-217). */
int gca_gather_rows(const float* src, const int64_t* idx, int64_t rows, int64_t row_elems, int64_t src_row_stride,
                    float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCA_HIP_H */
