// ReSSL (Zheng et al. 2021, "Relational Self-Supervised Learning with Weak Augmentation") on gfx950: the relational loss of a
// student row q_i against a momentum teacher's row k_i over the MoCo queue Q, and its gradient to q.  tests/ressl_ref.py is the
// fp64 statement.
//
//   s[i,j] = inv_Ts q_i . Q_j      t[i,j] = inv_Tt k_i . Q_j         exact-fp32 matrix cores, one k-ordered chain per score
//   lse_s[i] = logsumexp_j s       lse_t[i] = logsumexp_j t          Ps = exp(s - lse_s)    Pt = exp(t - lse_t)
//   loss_i = lse_s[i] - sum_j Pt[i,j] s[i,j]                         loss = mean_i loss_i
//   ent_i  = lse_t[i] - sum_j Pt[i,j] t[i,j]                         ent  = mean_i ent_i    (the teacher's entropy)
//   dq[i]  = g inv_Ts / N ( sum_j Ps[i,j] Q_j - sum_j Pt[i,j] Q_j )
//
//   forward  launch 1, grid (K-splits, row tiles): a workgroup stages rows i0 .. i0 + 31 of q AND of k once and streams its
//            split's 32-row tiles of Q past them, s^T and t^T tiles side by side (streamed row j in the accumulator registers,
//            owned row i on the lane).  A lane keeps six running scalars of its row -- m_s, l_s = sum exp(s - m_s), m_t, l_t,
//            c = sum exp(t - m_t) s, c_t = sum exp(t - m_t) t -- rescaled when a maximum moves.  Columns past K are -inf
//            before the maximum and contribute exactly nothing.  The two lanes of a row, then the waves (in wave order),
//            merge; one record per (split, row) goes to `ws` as [split][6][N].
//            launch 2, one workgroup: folds the records in split order, writes row_lse (lse_s then lse_t), row_loss, and the
//            two means through one fixed tree.
//   backward launch 1, grid (K-splits, row tiles, 2 sides): side 0 owns q rows with lse_s and inv_Ts, side 1 owns k rows with
//            lse_t and inv_Tt; the sides differ in three selected arguments and run the same instructions.  A workgroup
//            recomputes its score tile by the forward's chain, forms P = exp(x - lse) and accumulates Y += P Q from registers
//            (xview_tile.h: y_mma).  One slab per (split, side) in `ws` as [split][side][N D].
//            launch 2 sums the slabs in split order and writes dq = coef (O_s - O_t).
//   fast     D <= 256, D % 4 == 0, 16-byte aligned pointers: 4 waves, each streaming every 4th tile of the split through its own
//            16.5 KiB LDS chunk buffer, float4 loads of the next piece in flight under the MFMAs of the current one.
//   generic  everything else: 1 wave, guarded scalar staging (xview_tile.h: s_tile_generic).
//   splits   kt = ceil(K / 32) tiles of Q, G workgroups per split (row tiles; x 2 sides in the backward pass), W waves:
//            want = clamp(ceil(256 / G), 1, ceil(kt / W)), tps = ceil(kt / want), splits = ceil(kt / tps): no split is empty.
//            A constant of the code, not the device.
//
// No atomics, one owner per output, fixed fold orders: bitwise repeatable.  Nothing reads the host: capturable.
#include "xview_tile.h"

namespace {

constexpr int64_t MAX_K = (1ll << 31) - 1;
constexpr int NREC = 6;              // floats of a record: m_s, l_s, m_t, l_t, c, c_t

struct Rel { float ms, ls, mt, lt, c, ct; };

__device__ __forceinline__ Rel rel_empty() { return Rel{-INFINITY, 0.f, -INFINITY, 0.f, 0.f, 0.f}; }
// scale of a state whose maximum m moves to mx >= m (1 when it does not move, -inf == -inf included; 0 from -inf)
__device__ __forceinline__ float rel_scale(float m, float mx) { return m == mx ? 1.f : __expf(m - mx); }
// a then b, in that order everywhere
__device__ __forceinline__ Rel rel_merge(const Rel& a, const Rel& b) {
  Rel o;
  o.ms = fmaxf(a.ms, b.ms);
  o.mt = fmaxf(a.mt, b.mt);
  const float as = rel_scale(a.ms, o.ms), bs = rel_scale(b.ms, o.ms);
  const float at = rel_scale(a.mt, o.mt), bt = rel_scale(b.mt, o.mt);
  o.ls = a.ls * as + b.ls * bs;
  o.lt = a.lt * at + b.lt * bt;
  o.c = a.c * at + b.c * bt;
  o.ct = a.ct * at + b.ct * bt;
  return o;
}

// the lane's 16 columns of one Q tile (streamed rows jb + acc_row(r, lh)) into the running state of its row
__device__ __forceinline__ void rel_update(Rel& st, const f32x16& as, const f32x16& at, int jb, int K, float inv_Ts, float inv_Tt,
                                           int lh) {
  // x = acc * inv_T is rounded ONCE, here and in the backward pass: fused into x - m it would not be the x that m was taken from
  // (exp(x - m) != 1 at the maximum itself, and the two sides of the backward pass would no longer cancel exactly)
#pragma clang fp contract(off)
  float xs[16], xt[16];
  float ms = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool ok = jb + acc_row(r, lh) < K;
    xs[r] = as[r] * inv_Ts;
    xt[r] = at[r] * inv_Tt;
    ms = fmaxf(ms, ok ? xs[r] : -INFINITY);
    mt = fmaxf(mt, ok ? xt[r] : -INFINITY);
  }
  const float nms = fmaxf(st.ms, ms), nmt = fmaxf(st.mt, mt);
  const float fs = rel_scale(st.ms, nms), ft = rel_scale(st.mt, nmt);
  float ls = st.ls * fs, lt = st.lt * ft, c = st.c * ft, ct = st.ct * ft;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool ok = jb + acc_row(r, lh) < K;
    const float es = ok ? __expf(xs[r] - nms) : 0.f;                             // (nms is finite wherever ok holds once)
    const float et = ok ? __expf(xt[r] - nmt) : 0.f;
    ls += es;
    lt += et;
    c += ok ? et * xs[r] : 0.f;
    ct += ok ? et * xt[r] : 0.f;
  }
  st.ms = nms; st.ls = ls; st.mt = nmt; st.lt = lt; st.c = c; st.ct = ct;
}

// the two lanes of a row (columns 4 lh ..): lower half first, on both lanes
__device__ __forceinline__ Rel rel_fold_halves(const Rel& st, int lh) {
  Rel o;
  o.ms = __shfl_xor(st.ms, 32, 64); o.ls = __shfl_xor(st.ls, 32, 64);
  o.mt = __shfl_xor(st.mt, 32, 64); o.lt = __shfl_xor(st.lt, 32, 64);
  o.c = __shfl_xor(st.c, 32, 64);   o.ct = __shfl_xor(st.ct, 32, 64);
  return lh ? rel_merge(o, st) : rel_merge(st, o);
}
__device__ __forceinline__ void rel_write(float* __restrict__ rec, int split, int N, int i, const Rel& a) {
  float* p = rec + (long long)split * NREC * N + i;
  p[0] = a.ms; p[N] = a.ls; p[2 * (long long)N] = a.mt; p[3 * (long long)N] = a.lt; p[4 * (long long)N] = a.c;
  p[5 * (long long)N] = a.ct;
}

// ------------------------------------------------------------------------------------------------------------ forward
// grid (splits, row tiles).  LDS: q tile + k tile (2 x 2 chunks) + one chunk buffer per wave.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ressl_fwd_fast_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ Q, int N, int D, int K, float inv_Ts,
    float inv_Tt, int ktiles, int tps, float* __restrict__ rec, gca_magic md4a, gca_magic md4b) {
  __shared__ __attribute__((aligned(16))) float Zq[MAXCH * TILE];                // the workgroup's q rows
  __shared__ __attribute__((aligned(16))) float Zk[MAXCH * TILE];                // ... and the same rows of k
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];                 // per-wave streamed Q tile (one chunk)
  __shared__ float Rs[WAVES][NREC][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ktiles ? (split + 1) * tps : ktiles;
  const int jt0 = split * tps + wave;
  const int ntw = jt0 < t_end ? (t_end - jt0 + WAVES - 1) / WAVES : 0;
  const int nch = (D + FD - 1) / FD;

  f32x4 v[NPC];
  if (ntw > 0) tile_fetch(v, Q, jt0 * 32, K, D, chunk_of(0, nch, D, md4a, md4b), lane);
  tile_zero(Nw, lane);
  stage_q_tile<WAVES>(Zq, q, i0, N, D, nch, md4a, md4b, tid);
  stage_q_tile<WAVES>(Zk, k, i0, N, D, nch, md4a, md4b, tid);

  Rel st = rel_empty();
  for (int t = 0; t < ntw; ++t) {
    const int jb = (jt0 + t * WAVES) * 32;
    f32x16 as, at;
#pragma unroll
    for (int r = 0; r < 16; ++r) { as[r] = 0.f; at[r] = 0.f; }
    for (int c = 0; c < nch; ++c) {
      const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
      wave_lds_sync();                                                           // the previous piece's operand reads are done
      tile_store(v, Nw, ch, lane);
      wave_lds_sync();
      int nc = c + 1, nt = t;                                                    // the next piece streams in behind the MFMAs
      if (nc == nch) { nc = 0; nt = t + 1; }
      if (nt >= ntw) { nc = c; nt = t; }
      tile_fetch(v, Q, (jt0 + nt * WAVES) * 32, K, D, chunk_of(nc, nch, D, md4a, md4b), lane);
      tile_mma(as, Nw, Zq + c * TILE, (4 * ch.d4 + 7) >> 3, ll, lh);
      tile_mma(at, Nw, Zk + c * TILE, (4 * ch.d4 + 7) >> 3, ll, lh);
    }
    rel_update(st, as, at, jb, K, inv_Ts, inv_Tt, lh);
  }

  st = rel_fold_halves(st, lh);
  if (lh == 0) {
    Rs[wave][0][ll] = st.ms; Rs[wave][1][ll] = st.ls; Rs[wave][2][ll] = st.mt;
    Rs[wave][3][ll] = st.lt; Rs[wave][4][ll] = st.c;  Rs[wave][5][ll] = st.ct;
  }
  __syncthreads();
  if (tid < 32 && i0 + tid < N) {
    Rel a = Rel{Rs[0][0][tid], Rs[0][1][tid], Rs[0][2][tid], Rs[0][3][tid], Rs[0][4][tid], Rs[0][5][tid]};
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      a = rel_merge(a, Rel{Rs[w][0][tid], Rs[w][1][tid], Rs[w][2][tid], Rs[w][3][tid], Rs[w][4][tid], Rs[w][5][tid]});
    rel_write(rec, split, N, i0 + tid, a);
  }
}

__global__ __launch_bounds__(64) void ressl_fwd_generic_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ Q, int N, int D, int K, float inv_Ts,
    float inv_Tt, int ktiles, int tps, float* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];                        // the owned tile (q, then k), one chunk at a time
  __shared__ __attribute__((aligned(16))) float Nw[TILE];                        // the streamed Q tile, one chunk at a time
  const int lane = threadIdx.x, lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32;
  const int t_end = (split + 1) * tps < ktiles ? (split + 1) * tps : ktiles;
  Rel st = rel_empty();
  for (int jt = split * tps; jt < t_end; ++jt) {
    f32x16 as, at;
#pragma unroll
    for (int r = 0; r < 16; ++r) { as[r] = 0.f; at[r] = 0.f; }
    s_tile_generic(as, Nw, Zs, Q, jt * 32, K, q, i0, N, D, lane);
    s_tile_generic(at, Nw, Zs, Q, jt * 32, K, k, i0, N, D, lane);
    rel_update(st, as, at, jt * 32, K, inv_Ts, inv_Tt, lh);
  }
  st = rel_fold_halves(st, lh);
  if (lh == 0 && i0 + ll < N) rel_write(rec, split, N, i0 + ll, st);
}

// One workgroup: rows strided over the threads, splits in split order, then the means through one fixed tree.
__global__ __launch_bounds__(256) void ressl_finish_kernel(const float* __restrict__ rec, int N, int splits,
                                                           float* __restrict__ row_lse, float* __restrict__ row_loss,
                                                           float* __restrict__ out) {
  __shared__ float red[2][256];
  const int tid = threadIdx.x;
  const long long n = N;
  float sl = 0.f, se = 0.f;
  for (int i = tid; i < N; i += 256) {
    const float* p = rec + i;
    Rel a = Rel{p[0], p[n], p[2 * n], p[3 * n], p[4 * n], p[5 * n]};
    for (int s = 1; s < splits; ++s) {
      const float* u = rec + (long long)s * NREC * n + i;
      a = rel_merge(a, Rel{u[0], u[n], u[2 * n], u[3 * n], u[4 * n], u[5 * n]});
    }
    const float lse_s = a.ms + logf(a.ls), lse_t = a.mt + logf(a.lt);
    const float li = lse_s - a.c / a.lt, ei = lse_t - a.ct / a.lt;
    row_lse[i] = lse_s;
    row_lse[n + i] = lse_t;
    row_loss[i] = li;
    sl += li;
    se += ei;
  }
  red[0][tid] = sl;
  red[1][tid] = se;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { out[0] = red[0][0] / (float)N; out[1] = red[1][0] / (float)N; }
}

// ----------------------------------------------------------------------------------------------------------- backward
// grid (splits, row tiles, 2 sides).  The owned operand is z = side ? k : q (N rows), the streamed one Q (K rows).
__device__ __forceinline__ void rel_p_tile(f32x16& acc, int jb, int i, int N, int K, float inv_T, float lse_i, int lh) {
#pragma clang fp contract(off)                                                   // the forward's x, bit for bit (rel_update)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = jb + acc_row(r, lh);
    const float x = acc[r] * inv_T;
    acc[r] = (i < N && j < K) ? __expf(x - lse_i) : 0.f;
  }
}

// the structure of xview_bwd_fast_kernel: all of the 32 x D tile of Y in registers, chunks 0 .. nch - 2 staged a second time
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ressl_bwd_fast_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ Q, const float* __restrict__ lse, int N,
    int D, int K, float inv_Ts, float inv_Tt, int ktiles, int tps, float* __restrict__ slabs, gca_magic md4a, gca_magic md4b) {
  static_assert(MAXCH == 2, "the Y accumulators below are written out for two chunks");
  __shared__ __attribute__((aligned(16))) float Zs[MAXCH * TILE];                // the workgroup's owned tile
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];                 // per-wave streamed Q tile (one chunk)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32, side = blockIdx.z;
  const float* __restrict__ z = side ? k : q;
  const float inv_T = side ? inv_Tt : inv_Ts;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ktiles ? (split + 1) * tps : ktiles;
  const int jt0 = split * tps + wave;
  const int ntw = jt0 < t_end ? (t_end - jt0 + WAVES - 1) / WAVES : 0;
  const int nch = (D + FD - 1) / FD;
  const int ni = 2 * nch - 1;                                                    // pieces per Q tile: chunks 0 .. nch-1, 0 .. nch-2
  const int i = i0 + ll;
  const float lse_i = lse[(long long)side * N + (i < N ? i : N - 1)];
  float* out = slabs + ((long long)split * 2 + side) * N * D;

  f32x4 v[NPC];
  if (ntw > 0) tile_fetch(v, Q, jt0 * 32, K, D, chunk_of(0, nch, D, md4a, md4b), lane);
  tile_zero(Nw, lane);
  stage_q_tile<WAVES>(Zs, z, i0, N, D, nch, md4a, md4b, tid);

  f32x16 Y0[4], Y1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { Y0[c][r] = 0.f; Y1[c][r] = 0.f; }

  for (int t = 0; t < ntw; ++t) {
    const int jb = (jt0 + t * WAVES) * 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int x = 0; x < ni; ++x) {
      const int c = x < nch ? x : x - nch;
      const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
      wave_lds_sync();                                                           // the previous piece's operand reads are done
      tile_store(v, Nw, ch, lane);
      wave_lds_sync();
      int nx = x + 1, nt = t;                                                    // the next piece streams in behind the MFMAs
      if (nx == ni) { nx = 0; nt = t + 1; }
      if (nt >= ntw) { nx = x; nt = t; }
      tile_fetch(v, Q, (jt0 + nt * WAVES) * 32, K, D, chunk_of(nx < nch ? nx : nx - nch, nch, D, md4a, md4b), lane);
      if (x < nch) {
        tile_mma(acc, Nw, Zs + c * TILE, (4 * ch.d4 + 7) >> 3, ll, lh);
        if (x == nch - 1) rel_p_tile(acc, jb, i, N, K, inv_T, lse_i, lh);
      }
      if (x >= nch - 1) {                                                        // P exists: this chunk's part of Y
        if (c == 0) y_mma(Y0, acc, Nw, ll, lh);
        else y_mma(Y1, acc, Nw, ll, lh);
      }
    }
  }

  // ---- waves fold through LDS in wave order, chunk by chunk: Nw <- Y as [row i][feature]
  for (int c = 0; c < nch; ++c) {
    wave_lds_sync();
    if (c == 0) y_to_lds(Nw, Y0, ll, lh);
    else y_to_lds(Nw, Y1, ll, lh);
    __syncthreads();
    const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
    for (int e = tid; e < 32 * ch.d4; e += WAVES * 64) {
      const int r = (int)gca_fdiv((unsigned)e, ch.md4), c4 = e - r * ch.d4;
      if (i0 + r < N) {
        float4 s = *reinterpret_cast<const float4*>(&Ns[0][r * FP + c4 * 4]);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
          const float4 u = *reinterpret_cast<const float4*>(&Ns[w][r * FP + c4 * 4]);
          s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        *reinterpret_cast<float4*>(out + (long long)(i0 + r) * D + ch.c0 + c4 * 4) = s;
      }
    }
    __syncthreads();
  }
}

// generic path: one wave; the score tile is repeated per 128-column chunk of Y
__global__ __launch_bounds__(64) void ressl_bwd_generic_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ Q, const float* __restrict__ lse, int N,
    int D, int K, float inv_Ts, float inv_Tt, int ktiles, int tps, float* __restrict__ slabs) {
  __shared__ __attribute__((aligned(16))) float Zs[TILE];
  __shared__ __attribute__((aligned(16))) float Nw[TILE];
  const int lane = threadIdx.x;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, i0 = blockIdx.y * 32, side = blockIdx.z;
  const float* __restrict__ z = side ? k : q;
  const float inv_T = side ? inv_Tt : inv_Ts;
  const int t_end = (split + 1) * tps < ktiles ? (split + 1) * tps : ktiles;
  const int i = i0 + ll;
  const float lse_i = lse[(long long)side * N + (i < N ? i : N - 1)];
  float* out = slabs + ((long long)split * 2 + side) * N * D;

  for (int oc = 0; oc < D; oc += FD) {                                 // 128-column chunk of Y
    f32x16 Y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[c][r] = 0.f;
    for (int jt = split * tps; jt < t_end; ++jt) {
      const int jb = jt * 32;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      s_tile_generic(acc, Nw, Zs, Q, jb, K, z, i0, N, D, lane);
      if (D > FD) {                                                    // the chunk of Q_j that this chunk of Y multiplies
        wave_lds_sync();
        tile_stage_scalar(Nw, Q, jb, K, D, oc, lane);
        wave_lds_sync();
      }
      rel_p_tile(acc, jb, i, N, K, inv_T, lse_i, lh);
      y_mma(Y, acc, Nw, ll, lh);
    }
    wave_lds_sync();
    y_to_lds(Nw, Y, ll, lh);
    wave_lds_sync();
    for (int e = lane; e < 32 * FD; e += 64) {
      const int r = e / FD, c = e % FD;
      if (i0 + r < N && oc + c < D) out[(long long)(i0 + r) * D + oc + c] = Nw[r * FP + c];
    }
    wave_lds_sync();                                                   // the next chunk's staging overwrites Nw
  }
}

// dq = g inv_Ts / N (O_s - O_t): each side's slabs summed in split order
__global__ __launch_bounds__(256) void ressl_dq_kernel(const float* __restrict__ slabs, int N, int D, int splits, float inv_Ts,
                                                       const float* __restrict__ gscale_dev, float gscale_host,
                                                       float* __restrict__ dq) {
  const float g = gscale_host * (gscale_dev ? *gscale_dev : 1.f);
  const float coef = g * inv_Ts / (float)N;
  const long long n = (long long)N * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    float os = slabs[e], ot = slabs[n + e];
    for (int sp = 1; sp < splits; ++sp) {
      os += slabs[(long long)sp * 2 * n + e];
      ot += slabs[((long long)sp * 2 + 1) * n + e];
    }
    dq[e] = coef * (os - ot);
  }
}

struct RelPlan { bool fast; int waves, T, ktiles, splits, tps; };

bool rel_sizes_ok(int64_t N, int64_t D, int64_t K) { return sizes_ok(N, D) && K >= 1 && K <= MAX_K && K * D < (1ll << 31); }
// sides: workgroups per (split, row tile) -- 1 in the forward pass, 2 in the backward pass
RelPlan make_rel_plan(int64_t N, int64_t D, int64_t K, bool aligned, int sides) {
  RelPlan p;
  p.fast = D <= FAST_MAXD && D % 4 == 0 && aligned;
  p.waves = p.fast ? 4 : 1;
  p.T = (int)gca_ceil_div(N, 32);
  p.ktiles = (int)gca_ceil_div(K, 32);
  const int want = (int)gca_ceil_div(TARGET_WG, (int64_t)p.T * sides), cap = (int)gca_ceil_div(p.ktiles, p.waves);
  const int w = want < 1 ? 1 : (want > cap ? cap : want);
  p.tps = (int)gca_ceil_div(p.ktiles, w);
  p.splits = (int)gca_ceil_div(p.ktiles, p.tps);
  return p;
}
int64_t fwd_bytes(int64_t N, int splits) { return gca_round_up((int64_t)splits * NREC * N * 4, 16); }
int64_t bwd_bytes(int64_t N, int64_t D, int splits) { return gca_round_up((int64_t)splits * 2 * N * D * 4, 16); }

}  // namespace

extern "C" {

int64_t gca_ressl_fwd_ws_bytes(int64_t N, int64_t D, int64_t K) {
  if (!rel_sizes_ok(N, D, K)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {                        // the caller's pointers are not known here
    const int64_t b = fwd_bytes(N, make_rel_plan(N, D, K, aligned != 0, 1).splits);
    need = b > need ? b : need;
  }
  return need;
}

int64_t gca_ressl_bwd_ws_bytes(int64_t N, int64_t D, int64_t K) {
  if (!rel_sizes_ok(N, D, K)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {
    const int64_t b = bwd_bytes(N, D, make_rel_plan(N, D, K, aligned != 0, 2).splits);
    need = b > need ? b : need;
  }
  return need;
}

int gca_ressl_fwd_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits) {
  if (!rel_sizes_ok(N, D, K)) return GCA_EINVAL;
  const RelPlan p = make_rel_plan(N, D, K, aligned != 0, 1);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_ressl_bwd_path(int64_t N, int64_t D, int64_t K, int aligned, int32_t* waves, int32_t* splits) {
  if (!rel_sizes_ok(N, D, K)) return GCA_EINVAL;
  const RelPlan p = make_rel_plan(N, D, K, aligned != 0, 2);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_ressl_fwd(const float* q, const float* k, const float* Q, int64_t N, int64_t D, int64_t K, float inv_Ts, float inv_Tt,
                  float* row_lse, float* row_loss, float* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!rel_sizes_ok(N, D, K) || !scalar_ok(inv_Ts) || !scalar_ok(inv_Tt)) return GCA_EINVAL;
  if (!q || !k || !Q || !row_lse || !row_loss || !out || !ws) return GCA_EINVAL;
  if (ws_bytes < gca_ressl_fwd_ws_bytes(N, D, K)) return GCA_EINVAL;
  const float* ins[3] = {q, k, Q};
  const int64_t nin[3] = {N * D, N * D, K * D};
  float* outs[3] = {row_lse, row_loss, out};
  const int64_t nout[3] = {2 * N, N, 2};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b)
      if (overlap2(ins[a], nin[a], outs[b], nout[b])) return GCA_EINVAL;
    for (int b = a + 1; b < 3; ++b)
      if (overlap2(outs[a], nout[a], outs[b], nout[b])) return GCA_EINVAL;
  }
  const RelPlan p = make_rel_plan(N, D, K, aligned16(q) && aligned16(k) && aligned16(Q), 1);
  hipStream_t st = (hipStream_t)stream;
  float* rec = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)p.splits, (unsigned)p.T);
  if (p.fast) {
    gca_magic ma, mb;
    last_chunk_magics(true, D, &ma, &mb);
    hipLaunchKernelGGL(ressl_fwd_fast_kernel<4>, grid, dim3(256), 0, st, q, k, Q, (int)N, (int)D, (int)K, inv_Ts, inv_Tt,
                       p.ktiles, p.tps, rec, ma, mb);
  } else {
    hipLaunchKernelGGL(ressl_fwd_generic_kernel, grid, dim3(64), 0, st, q, k, Q, (int)N, (int)D, (int)K, inv_Ts, inv_Tt, p.ktiles,
                       p.tps, rec);
  }
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(ressl_finish_kernel, dim3(1), dim3(256), 0, st, rec, (int)N, p.splits, row_lse, row_loss, out);
  return gca_launch_status();
}

int gca_ressl_bwd(const float* q, const float* k, const float* Q, const float* row_lse, int64_t N, int64_t D, int64_t K,
                  float inv_Ts, float inv_Tt, const float* gscale_dev, float gscale_host, float* dq, void* ws, int64_t ws_bytes,
                  void* stream) {
  if (!rel_sizes_ok(N, D, K) || !scalar_ok(inv_Ts) || !scalar_ok(inv_Tt)) return GCA_EINVAL;
  if (!q || !k || !Q || !row_lse || !dq || !ws) return GCA_EINVAL;
  if (ws_bytes < gca_ressl_bwd_ws_bytes(N, D, K)) return GCA_EINVAL;
  const int64_t n = N * D;
  if (overlap(dq, q, n) || overlap(dq, k, n) || overlap2(dq, n, Q, K * D) || overlap2(dq, n, row_lse, 2 * N)) return GCA_EINVAL;
  const RelPlan p = make_rel_plan(N, D, K, aligned16(q) && aligned16(k) && aligned16(Q) && aligned16(ws), 2);
  hipStream_t st = (hipStream_t)stream;
  float* slabs = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)p.splits, (unsigned)p.T, 2);
  if (p.fast) {
    gca_magic ma, mb;
    last_chunk_magics(true, D, &ma, &mb);
    hipLaunchKernelGGL(ressl_bwd_fast_kernel<4>, grid, dim3(256), 0, st, q, k, Q, row_lse, (int)N, (int)D, (int)K, inv_Ts, inv_Tt,
                       p.ktiles, p.tps, slabs, ma, mb);
  } else {
    hipLaunchKernelGGL(ressl_bwd_generic_kernel, grid, dim3(64), 0, st, q, k, Q, row_lse, (int)N, (int)D, (int)K, inv_Ts, inv_Tt,
                       p.ktiles, p.tps, slabs);
  }
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  const int64_t blocks = gca_ceil_div(n, 256 * 4);
  hipLaunchKernelGGL(ressl_dq_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, slabs, (int)N, (int)D,
                     p.splits, inv_Ts, gscale_dev, gscale_host, dq);
  return gca_launch_status();
}

}  // extern "C"
