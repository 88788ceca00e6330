// Risk weights for minimum-risk training (include/astk.h astk_risk_weights): from the integers of astk_pair_stats
// and the candidates' sequence log-probabilities to the per-row weights of astk_decoder_fwd_w, per list (utterance)
//     Q_i = exp(alpha (s_i - s_max)) / sum_j ..,   Rbar = sum_i Q_i c_i,   weight_i = risk_scale alpha Q_i (Rbar - c_i) + [bit 1] ref_weight
// in float64, each output rounded once to float32 (the convention of features.hip and resample.hip).
//
// k_risk_weights: one wavefront per list, a lane per row (a list has at most ASTK_RISK_MAX_LIST = 64 rows), RK_WAVES lists per
// workgroup.  The three reductions (max, sum, weighted sum) are __shfl_xor trees over the 64 lanes in a fixed order, dead lanes holding
// the neutral element: every lane ends with the same value and the result is bit-identical from run to run.  Plain vector stores, no
// atomics, no LDS.  Contraction is off in the arithmetic so that it is the host model's sequence of roundings (tests/risk_model.py)
// up to the library's exp and log.
// k_risk_count_bad (only with n_bad): one workgroup re-validates every list and stores the count.
#include "common.h"
#include <cmath>

namespace astk {

namespace {

constexpr int RK_MAX_LIST = ASTK_RISK_MAX_LIST;
constexpr int RK_WAVES = 4;
constexpr int RK_COUNT_THREADS = 1024;
static_assert(RK_MAX_LIST == 64, "a lane per row: a list is one wavefront");

struct RiskArgs {
  int U, R, cost;
  double alpha, risk_scale, ref_weight;
  const int32_t* first;        // (U + 1)
  const float* score;          // (R)
  const int32_t* stats;        // (R, 8)
  const int32_t* lens;
  const int32_t* pairs;        // (R, 2)
  const int32_t* flags;        // (R)
  float *weight, *risk, *cost_out;
};

// The rows [lo, hi) of list u, or false for a bad list: more than RK_MAX_LIST rows, offsets that do not ascend inside [0, R], or a
// descent right in front of it (first[u-1] > first[u]: the list would share rows with an earlier one).  [zlo, zhi) are the rows a bad
// list zeroes: its own, inside [0, R) and behind the preceding offset.
__device__ __forceinline__ bool rk_list(const RiskArgs& a, int u, int& lo, int& hi, int& zlo, int& zhi) {
  lo = a.first[u];
  hi = a.first[u + 1];
  const int prev = u > 0 ? a.first[u - 1] : 0;
  zlo = max(max(lo, prev), 0);
  zhi = min(hi, a.R);
  return lo >= 0 && hi <= a.R && lo <= hi && prev <= lo && hi - lo <= RK_MAX_LIST;
}

#pragma clang fp contract(off)
// 1 - sentence BLEU from the clipped matches and the two lengths: ast_amd.eval.bleu_from_counts, the same operations in the same order
__device__ __forceinline__ double rk_bleu_cost(const int32_t* st, int hyp_len, int ref_len) {
  if (st[4] == 0) return 1.0;
  double logp = 0.0;
#pragma unroll
  for (int n = 1; n <= 4; ++n) {
    int m = st[3 + n], t = max(1, hyp_len - n + 1);
    if (n > 1) { m += 1; t += 1; }
    if (m == 0) return 1.0;
    logp += 0.25 * log((double)m / (double)t);
  }
  const double bp = hyp_len > ref_len ? 1.0 : (hyp_len == 0 ? 0.0 : exp(1.0 - (double)ref_len / (double)hyp_len));
  return 1.0 - bp * exp(logp);
}

__device__ __forceinline__ double rk_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double rk_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(RK_WAVES * 64) void k_risk_weights(RiskArgs a) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * RK_WAVES + (threadIdx.x >> 6);
  if (u >= a.U) return;      // (whole wavefronts leave: the shuffles below run on full ones)
  int lo, hi, zlo, zhi;
  if (!rk_list(a, u, lo, hi, zlo, zhi)) {
    for (long i = (long)zlo + lane; i < zhi; i += 64) {
      a.weight[i] = 0.f;
      if (a.cost_out) a.cost_out[i] = 0.f;
    }
    if (lane == 0 && a.risk) a.risk[u] = 0.f;
    return;
  }
  const int i = lo + lane;
  const bool in = i < hi;
  int flag = 0;
  bool live = false;
  double c = 0.0, s = -INFINITY;
  if (in) {
    flag = a.flags[i];
    const int32_t* st = a.stats + 8 * (size_t)i;
    live = (flag & 1) && st[0] >= 0;      // (a bad row of astk_pair_stats is eight -1: its pair may name no string, lens is not read)
    if (live) {
      const int hyp_len = a.lens[a.pairs[2 * (size_t)i]], ref_len = a.lens[a.pairs[2 * (size_t)i + 1]];
      c = a.cost == ASTK_RISK_COST_BLEU ? rk_bleu_cost(st, hyp_len, ref_len) : (double)st[0] / (double)max(1, ref_len);
      s = (double)a.score[i];
    }
  }
  const double smax = rk_wave_max(s);
  const double e = live ? exp(a.alpha * (s - smax)) : 0.0;
  const double sum = rk_wave_sum(e);
  const double q = live ? e / sum : 0.0;
  const double rbar = rk_wave_sum(q * c);
  if (in) {
    a.weight[i] = (float)(a.risk_scale * a.alpha * q * (rbar - c) + ((flag & 2) ? a.ref_weight : 0.0));
    if (a.cost_out) a.cost_out[i] = (float)c;
  }
  if (lane == 0 && a.risk) a.risk[u] = (float)rbar;
}

__global__ __launch_bounds__(RK_COUNT_THREADS) void k_risk_count_bad(RiskArgs a, int32_t* n_bad) {
  __shared__ int s_cnt[RK_COUNT_THREADS / 64];
  int c = 0;
  for (int u = threadIdx.x; u < a.U; u += RK_COUNT_THREADS) {
    int lo, hi, zlo, zhi;
    c += rk_list(a, u, lo, hi, zlo, zhi) ? 0 : 1;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < RK_COUNT_THREADS / 64; ++i) total += s_cnt[i];
    *n_bad = total;
  }
}

}  // namespace

}  // namespace astk

using namespace astk;

int astk_risk_weights(const astk_risk_desc* d, const int32_t* first, const float* score, const int32_t* stats, const int32_t* lens,
                      const int32_t* pairs, const int32_t* flags, float* weight, float* risk, float* cost_out, int32_t* n_bad,
                      void* stream) {
  ASTK_CHECK_DESC(d, astk_risk_desc);
  ASTK_CHECK(d->U >= 1, "risk_weights: U = %d lists, there must be at least one", d->U);
  ASTK_CHECK(d->R >= 1, "risk_weights: R = %d rows, there must be at least one", d->R);
  ASTK_CHECK(d->cost == ASTK_RISK_COST_BLEU || d->cost == ASTK_RISK_COST_EDIT, "risk_weights: cost = %d is neither BLEU (0) nor EDIT (1)", d->cost);
  ASTK_CHECK(std::isfinite(d->alpha) && d->alpha >= 0.f, "risk_weights: alpha = %g (finite, >= 0)", (double)d->alpha);
  ASTK_CHECK(std::isfinite(d->risk_scale), "risk_weights: risk_scale = %g is not finite", (double)d->risk_scale);
  ASTK_CHECK(std::isfinite(d->ref_weight), "risk_weights: ref_weight = %g is not finite", (double)d->ref_weight);
  ASTK_CHECK(first && score && stats && lens && pairs && flags && weight,
             "risk_weights: first, score, stats, lens, pairs, flags and weight must not be null");
  RiskArgs a;
  a.U = d->U; a.R = d->R; a.cost = d->cost;
  a.alpha = (double)d->alpha; a.risk_scale = (double)d->risk_scale; a.ref_weight = (double)d->ref_weight;
  a.first = first; a.score = score; a.stats = stats; a.lens = lens; a.pairs = pairs; a.flags = flags;
  a.weight = weight; a.risk = risk; a.cost_out = cost_out;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_risk_weights, dim3((d->U + RK_WAVES - 1) / RK_WAVES), dim3(RK_WAVES * 64), 0, s, a);
  ASTK_LAUNCH_CHECK();
  if (n_bad) {
    hipLaunchKernelGGL(k_risk_count_bad, dim3(1), dim3(RK_COUNT_THREADS), 0, s, a, n_bad);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}
