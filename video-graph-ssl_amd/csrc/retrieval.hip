// Nearest-neighbour retrieval on gfx950: fused distance + top-k, the (nq x ng) distance matrix is never written.
//
//   s[i,j] = sum_d q[i,d] * g[j,d]                     fp32 matrix cores (v_mfma_f32_32x32x2_f32), fp32 accumulation
//   cosine     dist = 1 - (s * r_q[i]) * r_g[j]        r = 1 / sqrt(|row|^2), 0 for an all-zero row
//   euclidean  d2   = max(0, (n2_q[i] + n2_g[j]) - 2 s)   ranking key d2, dist = sqrt(d2)
//   result     the k smallest 64-bit words  (order-preserving u32 of the key) << 32 | gallery index  per query:
//              ascending by (key, index), NaN keys last, -0 == +0.  The words are distinct, so "the k smallest" does not
//              depend on the order in which candidates arrive, on the slab count or on the launch shape.
//
// Three ordinary launches on one stream: row norms -> per (query tile, gallery slab) top-k lists -> merge of the lists.
// No hand-off between workgroups, no global atomics, no spin; every counter lives in LDS.
// Reference: tools/video_retrieval.py:174-197 (sklearn cosine_distances / euclidean_distances + np.argsort).
#include <cstdint>
#include "gca_common.h"
#include <math.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TQ = 128;              // queries per workgroup
constexpr int TG = 128;              // gallery rows per score tile
constexpr int CH = 32;               // features staged per pass
constexpr int LP = CH + 4;           // LDS pitch of a staged row (float4-aligned, conflict-free 128-bit fragment reads)
constexpr int KMAX = 64;
constexpr int CAP = 96;              // candidate slots per query: at least 32 beyond k, 6 per lane of a 16-lane group
constexpr int SMAX = 64;             // most slabs (the merge walks one list per lane)
constexpr unsigned long long TAIL = ~0ull;
static_assert(CAP % 16 == 0 && CAP >= KMAX + 32 && TQ % 16 == 0, "select_k: 16 lanes per query, room for a round of appends");

// fp32 -> u32 whose unsigned order is the float order; -0 -> +0, every NaN -> the largest value.
__device__ __forceinline__ unsigned key_of(float v) {
  if (v != v) return 0xFFFFFFFFu;
  v = v + 0.f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Score -> ranking key, one fp32 rounding per operation (no contraction into fma).  Division and square root are the
// IEEE-rounded `/` and sqrtf: in this toolchain's headers __fsqrt_rn is the 1-ulp native approximation and __fmul_rn /
// __fsub_rn are plain operators that the compiler may still contract.
__device__ __forceinline__ float key_value(int metric, float s, float a, float b) {
#pragma clang fp contract(off)
  if (metric == 0) {
    const float t = s * a;
    const float u = t * b;
    return 1.0f - u;
  }
  const float n = a + b;
  const float t = 2.0f * s;
  const float d = n - t;
  return d < 0.f ? 0.f : d;                              // (a NaN stays a NaN)
}

// One wave per row: lane l accumulates d = l, l + 64, ... as an fmaf chain, then a fixed butterfly.  cosine: 1 / sqrt(n2)
// (0 for n2 == 0), euclidean: n2.
__global__ __launch_bounds__(256) void retrieval_norm_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                             long long nq, long long ng, long long D, int metric,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq + ng) return;
  const float* p = row < nq ? q + row * D : g + (row - nq) * D;
  float s = 0.f;
  for (long long d = lane; d < D; d += 64) s = fmaf(p[d], p[d], s);
  s = gca_wave_sum(s);
  if (lane == 0) out[row] = metric == 0 ? (s == 0.f ? 0.f : 1.0f / sqrtf(s)) : s;
}

struct Stage { float v[2][16]; };    // one thread's share of a (128 x CH) chunk of each operand

// rows [r0, r0 + 128) x features [d0, d0 + CH) of `m` -> registers; rows >= nrows and features >= D read as zeros.
template <bool VEC>
__device__ __forceinline__ void stage_load(float* v, const float* __restrict__ m, long long r0, long long nrows, long long D,
                                           long long d0, int tid) {
  if (VEC) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = tid + 256 * it, r = i >> 3, c4 = i & 7;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < nrows && d0 + c4 * 4 < D) x = *reinterpret_cast<const float4*>(m + (r0 + r) * D + d0 + c4 * 4);
      v[4 * it] = x.x; v[4 * it + 1] = x.y; v[4 * it + 2] = x.z; v[4 * it + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int i = tid + 256 * it, r = i >> 5, c = i & 31;
      v[it] = (r0 + r < nrows && d0 + c < D) ? m[(r0 + r) * D + d0 + c] : 0.f;
    }
  }
}
template <bool VEC>
__device__ __forceinline__ void stage_store(const float* v, float* lds, int tid) {
  if (VEC) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = tid + 256 * it, r = i >> 3, c4 = i & 7;
      *reinterpret_cast<float4*>(&lds[r * LP + c4 * 4]) = make_float4(v[4 * it], v[4 * it + 1], v[4 * it + 2], v[4 * it + 3]);
    }
  } else {
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int i = tid + 256 * it, r = i >> 5, c = i & 31;
      lds[r * LP + c] = v[it];
    }
  }
}

// Keep the k smallest words of every query's candidate buffer, sorted, in its first slots, and tighten its threshold.
// Whole workgroup, between barriers.  Sixteen lanes own a query (a wave works on four at a time) and each lane holds up to
// CAP / 16 words of its buffer in registers.  Words are distinct, so the rank of a word (how many are smaller) is its sorted
// position; the buffer is read four words per step, every lane of the group the same ones.  Every lane's reads precede
// every lane's writes: one wave, one program counter, and the ranks that address the writes depend on all the reads.
__device__ __forceinline__ void select_k(unsigned long long* buf, int* cnt, int* srt, unsigned long long* thr, int k,
                                         int wave, int lane) {
  constexpr int E = CAP / 16;
  const int sub = lane & 15;
  for (int base = wave * 4; base < TQ; base += 16) {
    const int ql = base + (lane >> 4);
    int n = min(cnt[ql], CAP);
    const bool work = n != srt[ql];
    if (!work) n = 0;
    unsigned long long* b = buf + (size_t)ql * CAP;
    unsigned long long w[E];
    int rank[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      w[e] = sub + 16 * e < n ? b[sub + 16 * e] : TAIL;
      rank[e] = 0;
    }
    for (int i = 0; i < n; i += 4) {
      unsigned long long x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = b[min(i + u, CAP - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i + u >= n) x[u] = TAIL;
#pragma unroll
        for (int e = 0; e < E; ++e) rank[e] += x[u] < w[e];
      }
    }
    __builtin_amdgcn_wave_barrier();
    const int m = min(n, k);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (sub + 16 * e < n && rank[e] < k) b[rank[e]] = w[e];
      if (n >= k && sub + 16 * e < n && rank[e] == k - 1) thr[ql] = w[e];
    }
    if (work && sub == 0) { cnt[ql] = m; srt[ql] = m; }
  }
}

// Workgroup (query tile, slab): 4 waves as 2 x 2, each 64 queries x 64 gallery rows of a 128 x 128 score tile (2 x 2 MFMA
// tiles).  A = q (M = queries), B = gallery (N = gallery rows): register r of lane (lh, ll) is query (r & 3) + 8 (r >> 2)
// + 4 lh, gallery row ll.  Operands are staged [row][feature] and read as 128-bit fragments (4 MFMA steps per read): within
// every 8 features the products are added in the order 0 4 1 5 2 6 3 7, the same for every launch shape.
template <bool VEC>
__global__ __launch_bounds__(256) void retrieval_slab_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                             long long nq, long long ng, long long D, int k, int metric,
                                                             int S, long long tiles_per_slab, const float* __restrict__ norms,
                                                             unsigned long long* __restrict__ lists) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Qs = reinterpret_cast<float*>(smem);                               // [TQ][LP]
  float* Gs = Qs + TQ * LP;                                                 // [TG][LP]
  unsigned long long* thr = reinterpret_cast<unsigned long long*>(Gs + TG * LP);   // [TQ]  current k-th word of the query
  unsigned long long* buf = thr + TQ;                                       // [TQ][CAP]
  float* nQ = reinterpret_cast<float*>(buf + (size_t)TQ * CAP);             // [TQ]  r_q or n2_q
  int* cnt = reinterpret_cast<int*>(nQ + TQ);                               // [TQ]  appended so far (may run past CAP)
  int* srt = cnt + TQ;                                                      // [TQ]  count left sorted by the last select
  int* full = srt + TQ;                                                     // [1]   a lane found its query's buffer full

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lh = lane >> 5, ll = lane & 31, wm = wave >> 1, wn = wave & 1;
  const int slab = blockIdx.x % S;
  const long long q0 = (long long)(blockIdx.x / S) * TQ;
  const long long gtiles = (ng + TG - 1) / TG;
  const long long t_begin = slab * tiles_per_slab, t_end = min(gtiles, t_begin + tiles_per_slab);
  const long long nchunks = (D + CH - 1) / CH;

  for (int i = tid; i < TQ; i += 256) {
    thr[i] = TAIL; cnt[i] = 0; srt[i] = 0;
    nQ[i] = q0 + i < nq ? norms[q0 + i] : 0.f;
  }
  if (tid == 0) *full = 0;
  __syncthreads();

  for (long long gt = t_begin; gt < t_end; ++gt) {
    const long long g0 = gt * TG;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    Stage st;
    stage_load<VEC>(st.v[0], q, q0, nq, D, 0, tid);
    stage_load<VEC>(st.v[1], g, g0, ng, D, 0, tid);
    for (long long c = 0; c < nchunks; ++c) {
      __syncthreads();                                  // the previous chunk's fragment reads are done
      stage_store<VEC>(st.v[0], Qs, tid);
      stage_store<VEC>(st.v[1], Gs, tid);
      __syncthreads();
      if (c + 1 < nchunks) {                            // next chunk in flight under the MFMAs
        stage_load<VEC>(st.v[0], q, q0, nq, D, (c + 1) * CH, tid);
        stage_load<VEC>(st.v[1], g, g0, ng, D, (c + 1) * CH, tid);
      }
#pragma unroll
      for (int t = 0; t < CH / 8; ++t) {
        float4 a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          a[u] = *reinterpret_cast<const float4*>(&Qs[(wm * 64 + u * 32 + ll) * LP + 8 * t + 4 * lh]);
          b[u] = *reinterpret_cast<const float4*>(&Gs[(wn * 64 + u * 32 + ll) * LP + 8 * t + 4 * lh]);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].x, b[ni].x, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].y, b[ni].y, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].z, b[ni].z, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].w, b[ni].w, acc[mi][ni], 0, 0, 0);
          }
      }
    }

    // scores -> words -> candidate buffers.  A lane tries each of its 16 scores of a 32 x 32 tile once; what found its
    // query's buffer full stays pending, the workgroup selects and the lane tries again against the tighter threshold.
    // select_k leaves at most k <= 64 of the CAP = 96 slots taken, so every round places candidates: the loop ends.
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const long long j = g0 + wn * 64 + ni * 32 + ll;
        const bool jv = j < ng;
        const float ng_j = jv ? norms[nq + j] : 0.f;
        unsigned key[16];
        unsigned pending = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const float s = acc[mi][ni][r];
          key[r] = key_of(key_value(metric, s, nQ[ql], ng_j));
          if (jv && q0 + ql < nq) pending |= 1u << r;
        }
        while (true) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (pending >> r & 1u) {
              const int ql = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
              const unsigned long long w = (unsigned long long)key[r] << 32 | (unsigned long long)(unsigned)j;
              if (w < thr[ql]) {
                const int pos = atomicAdd(&cnt[ql], 1);
                if (pos < CAP) { buf[(size_t)ql * CAP + pos] = w; pending &= ~(1u << r); }
              } else {
                pending &= ~(1u << r);
              }
            }
          }
          if (pending) *full = 1;
          __syncthreads();
          const int any = *full;
          __syncthreads();                              // everyone has read the flag before it can change again
          if (!any) break;
          select_k(buf, cnt, srt, thr, k, wave, lane);
          if (tid == 0) *full = 0;
          __syncthreads();
        }
      }
  }

  __syncthreads();
  select_k(buf, cnt, srt, thr, k, wave, lane);
  __syncthreads();
  for (int i = tid; i < TQ * k; i += 256) {
    const int ql = i / k, p = i - ql * k;
    if (q0 + ql < nq) lists[((q0 + ql) * S + slab) * k + p] = p < cnt[ql] ? buf[(size_t)ql * CAP + p] : TAIL;
  }
}

// One wave per query: lane s walks the sorted list of slab s (S <= 64); k times the smallest head goes to the output and
// its lane advances.  Result j ends up in lane j (k <= 64), which writes idx / dist and tests the label.
__global__ __launch_bounds__(256) void retrieval_merge_kernel(const unsigned long long* __restrict__ lists, long long nq, int S,
                                                              int k, int metric, const long long* __restrict__ q_label,
                                                              const long long* __restrict__ g_label, int* __restrict__ idx,
                                                              float* __restrict__ dist, int* __restrict__ first_hit) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nq) return;
  const unsigned long long* mine = lists + (i * S + lane) * k;
  int p = 0;
  unsigned long long head = lane < S ? mine[0] : TAIL;
  unsigned long long out = TAIL;
  for (int j = 0; j < k; ++j) {
    unsigned long long m = head;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)m, o, 64), hi = __shfl_xor((unsigned)(m >> 32), o, 64);
      const unsigned long long other = (unsigned long long)hi << 32 | lo;
      m = other < m ? other : m;
    }
    if (lane == j) out = m;
    if (m == TAIL) break;                                // every list is exhausted: the rest is tail
    if (head == m) {                                     // words are distinct: exactly one lane
      ++p;
      head = p < k ? mine[p] : TAIL;
    }
  }
  bool hit = false;
  if (lane < k) {
    const bool tail = out == TAIL;
    const int gi = tail ? -1 : (int)(unsigned)out;
    float d = INFINITY;
    if (!tail) {
      d = value_of((unsigned)(out >> 32));
      if (metric != 0) d = sqrtf(d);
    }
    idx[i * k + lane] = gi;
    dist[i * k + lane] = d;
    if (first_hit && !tail) hit = g_label[gi] == q_label[i];
  }
  if (first_hit) {
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) first_hit[i] = mask ? __ffsll((long long)mask) : k + 1;
  }
}

struct Plan { int S; long long tiles_per_slab, norm_bytes; };

bool make_plan(int64_t nq, int64_t ng, int64_t D, int k, int slabs, Plan* p) {
  if (nq < 0 || ng < 0 || D < 1 || k < 1 || k > KMAX || slabs < 0) return false;
  if (ng > 0x7FFFFFFFll || nq > (0x7FFFFFFFll / SMAX) * TQ) return false;     // 31-bit gallery index; 1-D grid of tiles x slabs
  const long long qtiles = gca_ceil_div(nq, TQ), gtiles = gca_ceil_div(ng, TG);
  long long S = slabs > 0 ? slabs : gca_ceil_div(256, qtiles > 0 ? qtiles : 1);
  S = S > SMAX ? SMAX : S;
  S = S > gtiles ? gtiles : S;
  S = S < 1 ? 1 : S;
  p->tiles_per_slab = gtiles > 0 ? gca_ceil_div(gtiles, S) : 1;
  p->S = gtiles > 0 ? (int)gca_ceil_div(gtiles, p->tiles_per_slab) : 1;      // no empty slab
  p->norm_bytes = gca_round_up((nq + ng) * 4, 16);
  return true;
}

}  // namespace

extern "C" {

int64_t gca_retrieval_ws_bytes(int64_t nq, int64_t ng, int64_t D, int32_t k, int32_t slabs) {
  Plan p;
  if (!make_plan(nq, ng, D, k, slabs, &p)) return GCA_EINVAL;
  return p.norm_bytes + nq * (int64_t)p.S * k * 8;
}

int gca_retrieval_topk(const float* q, const float* g, int64_t nq, int64_t ng, int64_t D, int32_t k, int32_t metric,
                       const int64_t* q_label, const int64_t* g_label, int32_t slabs, int32_t* idx, float* dist,
                       int32_t* first_hit, void* ws, int64_t ws_bytes, void* stream) {
  Plan p;
  if (!make_plan(nq, ng, D, k, slabs, &p)) return GCA_EINVAL;
  if (metric != 0 && metric != 1) return GCA_EINVAL;
  if ((q_label == nullptr) != (g_label == nullptr)) return GCA_EINVAL;
  if (q_label && !first_hit) return GCA_EINVAL;
  if (ws_bytes < p.norm_bytes + nq * (int64_t)p.S * k * 8) return GCA_EINVAL;
  if (nq == 0 || ng == 0) return GCA_OK;                 // nothing to search: the caller's outputs stay as they are
  if (!q || !g || !idx || !dist || !ws) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* norms = reinterpret_cast<float*>(ws);
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(ws) + p.norm_bytes);

  hipLaunchKernelGGL(retrieval_norm_kernel, dim3((unsigned)gca_ceil_div(nq + ng, 4)), dim3(256), 0, st, q, g, (long long)nq,
                     (long long)ng, (long long)D, (int)metric, norms);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;

  const size_t lds = (size_t)(TQ + TG) * LP * 4 + (size_t)TQ * 8 + (size_t)TQ * CAP * 8 + (size_t)TQ * 12 + 16;
  const bool vec = D % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0;
  const dim3 grid((unsigned)(gca_ceil_div(nq, TQ) * p.S));
  static bool raised[2] = {false, false};
  if (!raised[vec]) {
    const void* fn = vec ? reinterpret_cast<const void*>(&retrieval_slab_kernel<true>)
                         : reinterpret_cast<const void*>(&retrieval_slab_kernel<false>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10) != hipSuccess) return GCA_ELAUNCH;
    raised[vec] = true;
  }
  if (vec)
    hipLaunchKernelGGL(retrieval_slab_kernel<true>, grid, dim3(256), lds, st, q, g, (long long)nq, (long long)ng, (long long)D,
                       (int)k, (int)metric, p.S, p.tiles_per_slab, (const float*)norms, lists);
  else
    hipLaunchKernelGGL(retrieval_slab_kernel<false>, grid, dim3(256), lds, st, q, g, (long long)nq, (long long)ng, (long long)D,
                       (int)k, (int)metric, p.S, p.tiles_per_slab, (const float*)norms, lists);
  if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;

  hipLaunchKernelGGL(retrieval_merge_kernel, dim3((unsigned)gca_ceil_div(nq, 4)), dim3(256), 0, st,
                     (const unsigned long long*)lists, (long long)nq, p.S, (int)k, (int)metric,
                     reinterpret_cast<const long long*>(q_label), reinterpret_cast<const long long*>(g_label), idx, dist,
                     q_label ? first_hit : nullptr);
  return gca_launch_status();
}

}  // extern "C"
