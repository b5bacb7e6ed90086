// MoCo v3's symmetrised cross-view InfoNCE (Chen, Xie, He 2021, Algorithm 1) and its gradient on gfx950.
// tests/mocov3_ref.py is the numpy statement.
//
//   q1, q2 (N, D) fp32: the student's predictor outputs;  k1, k2 (N, D) fp32: the momentum teacher's projector outputs.
//   direction 0 pairs (q, k) = (q1, k2), direction 1 pairs (q2, k1).  Per direction:
//   s[i,j]  = (sum_e q[i,e] k[j,e]) * inv_T                 exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32), fp32 accumulation
//   lse[i]  = log sum_j exp(s[i,j])                         ALL j, the diagonal included; online max / sum, rows NOT assumed unit
//   sp[i]   = s[i,i]          l_d = mean_i (lse[i] - sp[i])          rank[i] = #{j != i : s[i,j] >= sp[i]}
//   P[i,j]  = exp(s[i,j] - lse[i])
//   dq[i,:] = g w inv_T / N ( sum_j P[i,j] k[j,:] - k[i,:] )         nothing flows to k: the teacher is detached
//   loss    = w (l_0 + l_1)
//
// Both directions of a pass run in ONE grid (blockIdx.z), 32-row tiles of k streamed against one staged 32-row tile of q per
// workgroup; no N x N tensor exists.  Forward is 2 launches (tiles, then fold + loss), backward is 2 (tiles, then fold + scale).
//
//   forward   workgroup (column split, row tile, direction): wave w takes the split's column tiles w, w + WAVES, ...; A = the
//             staged q tile, B = the streamed k tile, so a lane holds 16 rows of ONE column.  sp comes first, from the diagonal of
//             the diagonal tile (q tile t against k tile t) -- the same k-ordered fma chain as the streamed value of s[i,i], so
//             the two are the same bits and `>=` ties are exact.  Per-lane running (reference, sum, count) for the lane's 16
//             rows; one cross-lane fold per wave, one per workgroup -> (m, sum, count) partials per (split, row) in `ws`.
//             mocov3_finish_kernel folds the splits in order and writes lse, rank and the three losses (one workgroup, fp64).
//   backward  a workgroup owns a 32-row tile of dq and streams the column tiles j of k: the s tile is recomputed TRANSPOSED
//             (A = streamed k tile, B = staged q tile), by the forward's fma chain, so P[i,j] sits with i on the lane and j in
//             the 16 accumulator registers, which is the A operand layout of the next product Y[i,:] += sum_j P[i,j] k[j,:]
//             (register r of lane half h is k = h of MFMA r: row j = (r&3) + 8(r>>2) + 4h) -- no trip through LDS; the B
//             operand is row j of the streamed tile, still in this wave's LDS.  (ntxent.hip does this with the roles swapped.)
//             Waves fold through LDS in wave order, column splits go to `ws` (or straight into dq for one split) and
//             xview_dq_kernel adds them in split order, applies the -k[i,:] term and the scale.  The tile helpers and the
//             backward kernels live in xview_tile.h, which nnclr.hip shares (its softmax runs over the other axis).
//
// One owner per output element and fixed fold orders everywhere: no atomics, bitwise reproducible.  Nothing reads the host, so
// both entries can be captured in a hipGraph.
//
// Dispatch (restated in tests/mocov3_ref.py: mocov3_path), a function of the arguments alone:
//   fast     D <= 256, D % 4 == 0, every pointer 16-byte aligned: 4 waves per workgroup, float4 loads with the next piece in
//            flight behind the MFMAs of the current one.  Features go through LDS in 128-wide chunks (zero-padded to a multiple
//            of 8) and s accumulates over them; the q tile is staged whole (2 chunks), which together with the 4 wave tiles is
//            99 KiB of LDS -- a third chunk would not leave room for them, hence the limit of 256.  The backward pass holds all
//            of its dq tile in accumulators; for D > 128 the first chunk of each k tile goes through LDS a second time, for
//            its part of P k, once P exists.
//   generic  everything else: 1 wave per workgroup, guarded scalar staging in 128-feature chunks (the backward pass repeats
//            the s tile per 128-column chunk of dq).
//   splits   as ntxent.hip, per direction: T = ceil(N / 32) tiles; splits = clamp(ceil(256 / T), 1, ceil(T / waves)) -- a
//            constant of the code, not of the device.
#include "xview_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ forward
// grid (splits, row tiles, 2 directions).  Partials and sp are indexed by R = direction * N + i.
template <int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void mocov3_fwd_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ k1, const float* __restrict__ k2,
    int N, int D, float inv_T, int ntiles, int tps, float* __restrict__ pm, float* __restrict__ ps, int* __restrict__ pc,
    float* __restrict__ sp_out, gca_magic md4a, gca_magic md4b) {
  __shared__ __attribute__((aligned(16))) float Zs[(FAST ? MAXCH : 1) * TILE];   // the workgroup's q tile
  __shared__ __attribute__((aligned(16))) float Ns[WAVES][TILE];                 // per-wave streamed k tile (one chunk)
  __shared__ float L0[WAVES][32];
  __shared__ float Red[WAVES][3][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31;
  const int split = blockIdx.x, dt = blockIdx.y, i0 = dt * 32, dir = blockIdx.z;
  const float* __restrict__ q = dir ? q2 : q1;
  const float* __restrict__ k = dir ? k1 : k2;
  float* Nw = Ns[wave];
  const int t_end = (split + 1) * tps < ntiles ? (split + 1) * tps : ntiles;
  const int ct0 = split * tps + wave;
  const int ntw = ct0 < t_end ? (t_end - ct0 + WAVES - 1) / WAVES : 0;          // streamed tiles of this wave
  const int nch = FAST ? (D + FD - 1) / FD : 1;

  f32x4 v[NPC];
  if (FAST) {
    tile_fetch(v, k, i0, N, D, chunk_of(0, nch, D, md4a, md4b), lane);          // in flight while the q tile is staged
    tile_zero(Nw, lane);
    stage_q_tile<WAVES>(Zs, q, i0, N, D, nch, md4a, md4b, tid);
  }

  float l0r[16], mx[16], sm[16];
  int cn[16];
  // tile 0 of the sequence is the diagonal tile (the positives); tiles 1 .. ntw are the wave's share of the split
  for (int t = 0; t <= ntw; ++t) {
    const int ct = t == 0 ? dt : ct0 + (t - 1) * WAVES;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (FAST) {
      for (int c = 0; c < nch; ++c) {
        const Chunk ch = chunk_of(c, nch, D, md4a, md4b);
        wave_lds_sync();                                                         // the previous piece's fragment reads are done
        tile_store(v, Nw, ch, lane);
        wave_lds_sync();
        int nc = c + 1, nt = t;                                                  // the next piece streams in behind the MFMAs
        if (nc == nch) { nc = 0; nt = t + 1; }
        if (nt > ntw) { nc = c; nt = t; }
        const int nct = nt == 0 ? dt : ct0 + (nt - 1) * WAVES;
        tile_fetch(v, k, nct * 32, N, D, chunk_of(nc, nch, D, md4a, md4b), lane);
        tile_mma(acc, Zs + c * TILE, Nw, (4 * ch.d4 + 7) >> 3, ll, lh);
      }
    } else {
      s_tile_generic(acc, Zs, Nw, q, i0, N, k, ct * 32, N, D, lane);
    }
    if (t == 0) {
      // ---- positive logits of the 32 rows: the diagonal of the diagonal tile
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc_row(r, lh) == ll) L0[wave][ll] = acc[r] * inv_T;
      wave_lds_sync();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        l0r[r] = L0[wave][acc_row(r, lh)];
        mx[r] = l0r[r]; sm[r] = 0.f; cn[r] = 0;
      }
      if (split == 0 && wave == 0 && lane < 32 && i0 + lane < N) sp_out[(long long)dir * N + i0 + lane] = L0[0][lane];
    } else {
      const int j = ct * 32 + ll;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + acc_row(r, lh);
        const float x = acc[r] * inv_T;
        if (j < N) {                                                             // the diagonal is inside the softmax
          float d = x - mx[r];
          if (d > 8.f) { sm[r] *= __expf(-d); mx[r] = x; d = 0.f; }              // moving reference: exp(d) stays far from overflow
          sm[r] += __expf(d);
          cn[r] += (j != i && x >= l0r[r]) ? 1 : 0;
        }
      }
    }
  }

  // ---- one cross-lane fold per wave, then the waves in order
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float M = half_max(mx[r]);
    const float S = half_sum(sm[r] * expf(mx[r] - M));
    const float Cn = half_sum((float)cn[r]);
    if (ll == 0) { const int m = acc_row(r, lh); Red[wave][0][m] = M; Red[wave][1][m] = S; Red[wave][2][m] = Cn; }
  }
  __syncthreads();
  if (tid < 32 && i0 + tid < N) {
    float M = Red[0][0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) M = fmaxf(M, Red[w][0][tid]);
    float S = 0.f, Cn = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { S += Red[w][1][tid] * expf(Red[w][0][tid] - M); Cn += Red[w][2][tid]; }
    const long long o = ((long long)split * 2 + dir) * N + i0 + tid;
    pm[o] = M; ps[o] = S; pc[o] = (int)Cn;
  }
}

// One workgroup: folds the splits of every row in split order, writes lse / rank / sp, then the losses (fp64, fixed order):
// loss[0] = w (l_0 + l_1), loss[1] = l_0, loss[2] = l_1.
__global__ __launch_bounds__(1024) void mocov3_finish_kernel(
    const float* __restrict__ pm, const float* __restrict__ ps, const int* __restrict__ pc, const float* __restrict__ sp,
    int N, int splits, float w, float* __restrict__ lse, int* __restrict__ rank, float* __restrict__ pos_logit,
    float* __restrict__ loss) {
  __shared__ double sh[2][16];
  const long long N2 = 2ll * N;
  for (int dir = 0; dir < 2; ++dir) {
    double part = 0.0;
    for (int i = threadIdx.x; i < N; i += 1024) {
      const long long R = (long long)dir * N + i;
      float M = pm[R];
      for (int s = 1; s < splits; ++s) M = fmaxf(M, pm[s * N2 + R]);
      float S = 0.f;
      int Cn = 0;
      for (int s = 0; s < splits; ++s) {
        const long long o = s * N2 + R;
        S += ps[o] * expf(pm[o] - M);
        Cn += pc[o];
      }
      const float l = M + logf(S);
      const float p = sp[R];
      lse[R] = l;
      if (rank) rank[R] = Cn;
      if (pos_logit) pos_logit[R] = p;
      part += (double)l - (double)p;
    }
    part = gca_wave_sum_d(part);
    if ((threadIdx.x & 63) == 0) sh[dir][threadIdx.x >> 6] = part;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l[2];
    for (int dir = 0; dir < 2; ++dir) {
      double t = 0.0;
      for (int wv = 0; wv < 16; ++wv) t += sh[dir][wv];
      l[dir] = t / (double)N;
    }
    loss[0] = (float)((double)w * (l[0] + l[1]));
    loss[1] = (float)l[0];
    loss[2] = (float)l[1];
  }
}

// forward partials: (m, sum, count) per (split, direction, row) + the positive logits; 16-byte multiples
int64_t fwd_ws_bytes(int64_t N, int splits) { return gca_round_up((3 * (int64_t)splits + 1) * 2 * N * 4, 16); }

}  // namespace

extern "C" {

int64_t gca_mocov3_ws_bytes(int64_t N, int64_t D) {
  if (!sizes_ok(N, D)) return -1;
  int64_t need = 16;
  for (int aligned = 0; aligned < 2; ++aligned) {                        // the caller's pointers are not known here
    const Plan p = make_plan(N, D, aligned != 0);
    const int64_t f = fwd_ws_bytes(N, p.splits), bw = xview_bwd_ws_bytes(N, D, p.splits);
    need = f > need ? f : need;
    need = bw > need ? bw : need;
  }
  return need;
}

int gca_mocov3_path(int64_t N, int64_t D, int aligned, int32_t* waves, int32_t* splits) {
  if (!sizes_ok(N, D)) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned != 0);
  if (waves) *waves = p.waves;
  if (splits) *splits = p.splits;
  return p.fast ? 1 : 0;
}

int gca_mocov3_fwd(const float* q1, const float* q2, const float* k1, const float* k2, int64_t N, int64_t D, float inv_T,
                   float w, float* row_lse, float* pos_logit, int32_t* rank_ge, float* loss, void* ws, void* stream) {
  if (!sizes_ok(N, D) || !scalar_ok(inv_T) || !scalar_ok(w)) return GCA_EINVAL;
  if (!q1 || !q2 || !k1 || !k2 || !row_lse || !loss || !ws) return GCA_EINVAL;
  const Plan p = make_plan(N, D, aligned16(q1) && aligned16(q2) && aligned16(k1) && aligned16(k2));
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)p.splits * 2 * N;
  float* pm = reinterpret_cast<float*>(ws);
  float* ps = pm + rows;
  int* pc = reinterpret_cast<int*>(ps + rows);
  float* sp = reinterpret_cast<float*>(pc + rows);
  gca_magic ma, mb;
  last_chunk_magics(p.fast, D, &ma, &mb);
  const dim3 grid((unsigned)p.splits, (unsigned)p.ntiles, 2);
  if (p.fast)
    hipLaunchKernelGGL((mocov3_fwd_kernel<4, true>), grid, dim3(256), 0, st, q1, q2, k1, k2, (int)N, (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, ma, mb);
  else
    hipLaunchKernelGGL((mocov3_fwd_kernel<1, false>), grid, dim3(64), 0, st, q1, q2, k1, k2, (int)N, (int)D, inv_T, p.ntiles,
                       p.tps, pm, ps, pc, sp, ma, mb);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  hipLaunchKernelGGL(mocov3_finish_kernel, dim3(1), dim3(1024), 0, st, pm, ps, pc, sp, (int)N, p.splits, w, row_lse, rank_ge,
                     pos_logit, loss);
  return gca_launch_status();
}

int gca_mocov3_bwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* row_lse, int64_t N,
                   int64_t D, float inv_T, float w, const float* gscale_dev, float gscale_host, float* dq1, float* dq2, void* ws,
                   void* stream) {
  return xview_bwd<false>(q1, q2, k1, k2, row_lse, N, D, inv_T, w, gscale_dev, gscale_host, dq1, dq2, ws, stream);
}

}  // extern "C"
