// Weighted k-NN vote on gfx950: the classifier that InstDisc / MoCo / SimSiam code bases run on frozen features, taken from
// the (idx, dist) lists gca_retrieval_topk writes.  tests/knn_ref.py is the numpy statement of everything below.
//
//   valid slot   0 <= idx < ng,  idx != self_base + query (leave-one-out),  g_label[idx] in [0, C),  dist not NaN
//   voters       the first kvote valid slots in rank order
//   weight       uniform: 1      exp: expf(-(dist * inv_T))   (one rounding of the product, the library expf)
//   score[c]     fp32 sum of the weights of class c's voters, added in rank order
//   class order  score descending, then class index ascending, over all C classes (unvoted classes score 0)
//   pred         first class of that order;  rank = how many classes other than q_label come before q_label
//
// One wave per query, four queries per 256-thread workgroup, lane j owns slot j (k <= 64).  Everything is ballots, lane
// reads and registers: no LDS, no atomics, no limit on C.  The (nq, C) score block, when asked for, is zero-filled by a
// launch of its own and the lowest lane of every voted class (its leader) scatters the class total into it.
#include <cstdint>
#include "gca_common.h"
#include <math.h>

namespace {

constexpr int KMAX = 64;

__device__ __forceinline__ float lane_read(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__device__ __forceinline__ float vote_weight(int weighting, float d, float inv_T) {
#pragma clang fp contract(off)
  if (weighting == 0) return 1.0f;
  const float t = d * inv_T;
  return expf(-t);
}

__global__ __launch_bounds__(256) void knn_zero_kernel(float* __restrict__ p, long long n) {
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n && (reinterpret_cast<uintptr_t>(p + i) & 15) == 0) {
      *reinterpret_cast<float4*>(p + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (long long e = i; e < n && e < i + 4; ++e) p[e] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void knn_vote_kernel(const int* __restrict__ idx, const float* __restrict__ dist,
                                                       long long nq, int k, int kvote,
                                                       const long long* __restrict__ g_label, long long ng,
                                                       const long long* __restrict__ q_label, long long self_base,
                                                       long long C, int weighting, float inv_T,
                                                       float* __restrict__ scores, int* __restrict__ pred,
                                                       int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nq) return;                                   // whole waves leave: every cross-lane step below sees 64 lanes

  // ---- slot -> (class, weight); invalid and non-voting slots carry class -1 and weight 0
  bool valid = false;
  long long cls = -1;
  float d = 0.f;
  if (lane < k) {
    const long long gi = idx[i * k + lane];
    d = dist[i * k + lane];
    if (gi >= 0 && gi < ng && !(self_base >= 0 && gi == self_base + i) && d == d) {
      const long long c = g_label[gi];
      if (c >= 0 && c < C) { valid = true; cls = c; }
    }
  }
  const unsigned long long vmask = __ballot(valid);
  const int before = __popcll(vmask & ((1ull << lane) - 1ull));
  const bool vote = valid && before < kvote;
  const unsigned long long votes = __ballot(vote);
  if (!vote) cls = -1;
  const float w = vote ? vote_weight(weighting, d, inv_T) : 0.f;

  if (votes == 0) {                                      // no voting slot (wave-uniform)
    if (lane == 0) {
      pred[i] = -1;
      if (rank) rank[i] = (int)(C < 0x7FFFFFFFll ? C : 0x7FFFFFFFll);
    }
    return;
  }

  // ---- class totals in rank order: adding +0 for another class's slot leaves a non-negative partial sum as it is
  const int clo = (int)cls, chi = (int)(cls >> 32);      // classes may exceed 32 bits: compare both halves
  float total = 0.f;
  bool leader = vote;
  for (int j = 0; j < k; ++j) {
    if (!(votes >> j & 1ull)) continue;                  // wave-uniform
    const int jlo = __builtin_amdgcn_readlane(clo, j), jhi = __builtin_amdgcn_readlane(chi, j);
    const float wj = lane_read(w, j);
    const bool same = jlo == clo && jhi == chi;
    total += same ? wj : 0.f;
    if (same && j < lane) leader = false;
  }

  // ---- pred: the best (score desc, class asc) among the leaders.  Scores are >= 0, so when the best voted score is 0
  // every class scores 0 and class 0 comes first.
  float bs = leader ? total : -1.f;
  long long bc = leader ? cls : 0x7FFFFFFFFFFFFFFFll;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int olo = __shfl_xor((int)bc, o, 64), ohi = __shfl_xor((int)(bc >> 32), o, 64);
    const long long oc = (long long)ohi << 32 | (unsigned)olo;
    if (os > bs || (os == bs && oc < bc)) { bs = os; bc = oc; }
  }
  if (lane == 0) pred[i] = bs > 0.f ? (int)bc : 0;

  // ---- rank of the query's own class
  if (rank) {
    const long long t = q_label[i];
    const unsigned long long tm = __ballot(leader && cls == t);
    const float st = tm ? lane_read(total, __ffsll((long long)tm) - 1) : 0.f;
    const bool ahead = leader && cls != t && (total > st || (total == st && cls < t));
    long long r = __popcll(__ballot(ahead));
    if (st == 0.f) {                                     // the target scores 0: unvoted classes below it come first
      const long long tc = t < 0 ? 0 : (t > C ? C : t);
      r += tc - __popcll(__ballot(leader && cls < tc));
    }
    if (lane == 0) rank[i] = (int)(r < 0x7FFFFFFFll ? r : 0x7FFFFFFFll);
  }

  // ---- scores: the row was zero-filled by the launch before this one; cls is in [0, C) for every leader
  if (scores && leader) scores[i * C + cls] = total;
}

}  // namespace

extern "C" {

int gca_knn_vote(const int32_t* idx, const float* dist, int64_t nq, int32_t k, int32_t kvote, const int64_t* g_label,
                 int64_t ng, const int64_t* q_label, int64_t self_base, int64_t C, int32_t weighting, float inv_T,
                 float* scores, int32_t* pred, int32_t* rank, void* stream) {
  if (k < 1 || k > KMAX || kvote < 1 || kvote > k || C < 1 || nq < 0 || ng < 0 || ng > 0x7FFFFFFFll) return GCA_EINVAL;
  if (nq > 0x7FFFFFFFll) return GCA_EINVAL;              // 1-D grid of nq / 4 workgroups, 32-bit slot arithmetic per row
  if (weighting != 0 && weighting != 1) return GCA_EINVAL;
  if (!(inv_T >= 0.f) || isinf(inv_T)) return GCA_EINVAL;
  if (rank && !q_label) return GCA_EINVAL;
  if (scores && (nq > 0x7FFFFFFFll / C || nq * C > 0x7FFFFFFFll)) return GCA_EINVAL;
  if (nq == 0) return GCA_OK;
  if (!idx || !dist || !pred || (!g_label && ng > 0)) return GCA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (scores) {
    const long long n = (long long)nq * C;
    const long long blocks = gca_ceil_div(n, 256 * 4 * 4);           // four float4 per thread, capped
    hipLaunchKernelGGL(knn_zero_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, scores, n);
    if (gca_launch_status() != GCA_OK) return GCA_ELAUNCH;
  }
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)gca_ceil_div(nq, 4)), dim3(256), 0, st, idx, dist, (long long)nq, (int)k,
                     (int)kvote, reinterpret_cast<const long long*>(g_label), (long long)ng,
                     reinterpret_cast<const long long*>(q_label), (long long)self_base, (long long)C, (int)weighting, inv_T,
                     scores, pred, rank);
  return gca_launch_status();
}

}  // extern "C"
