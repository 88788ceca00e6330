// Pair statistics of token strings (include/astk.h astk_pair_stats): for every pair (a, b) of a pool of int32
// strings the Levenshtein statistics [dist, sub, del, ins] under a fixed tie rule and the clipped n-gram matches m1..m4 of BLEU, all
// integers, so the outcome is a host model's (tests/pair_stats_model.py) bit for bit.  tokens, lens and pairs are only read; no
// atomics, no workspace.
//
// k_pair_stats: one wavefront per pair, PS_WAVES per workgroup, a grid-stride loop over the pairs.  Both strings are copied into the
// wave's LDS slice, so nothing after the copy touches global memory but the eight result words.
//   edit statistics   the columns (positions of b) run over the 64 lanes in blocks of 64, skewed: in step s lane l is at the cell
//                     (i, j) = (s - l + 1, j0 + l + 1).  "Up" D[i-1][j] is the lane's own last value, "left" D[i][j-1] is lane l - 1's
//                     last value (one __shfl_up per step) and "diagonal" D[i-1][j-1] is what that shuffle returned one step earlier.
//                     Lane 0 reads its left neighbour from the column the previous block's lane 63 parked in LDS (the boundary
//                     D[i][0] = i insertions in the first block); two parked columns take turns, so a block never writes the one
//                     it reads.  A cell is one 32-bit word: bits 0-9 the cost, 10-19 the substitutions, 20-29 the deletions (all
//                     <= 512); insertions = cost - sub - del.  The candidates are tried diagonal, deletion, insertion and a later one
//                     wins only if it is strictly cheaper: the tie rule of the header.
//   clipped matches   lane l owns the positions p = l, l + 64, .. of a.  For every position q of a string x it extends the common
//                     length of a[p..] and x[q..] up to 4 tokens (x slides through a four-word window every lane reads at the same
//                     address), which serves n = 1..4 at once: cnt[n] counts the equal n-grams of b, rank[n] those of a at q < p.
//                     Position p contributes to m_n iff its n-gram exists and rank[n] < cnt[n]: summed over the occurrences of one
//                     n-gram that is min(count_a, count_b).  Tokens are compared directly, so any int32 is an id.  A wave reduction.
// k_pair_count_bad (only with n_bad): one workgroup re-validates every row and stores the count -- no atomics there either.
#include "common.h"
#include <algorithm>

namespace astk {

namespace {

constexpr int PS_MAX_LEN = ASTK_PAIR_MAX_LEN;
constexpr int PS_WAVES = 4;                                  // pairs in flight per workgroup: 4 * (2 * 512 + 2 * 513) words = 32.0 KiB of LDS
constexpr int PS_MAX_BLOCKS = 1024;                          // the grid: four workgroups per CU; beyond it the loop strides
constexpr int PS_COUNT_THREADS = 1024;
constexpr int PS_FIELD = 1023;                               // a 10-bit field of a cell
constexpr int PS_SUB1 = 1 | (1 << 10), PS_DEL1 = 1 | (1 << 20), PS_INS1 = 1;      // one edit: the cost and its own count

struct PairArgs {
  int S, Lmax, P;
  const int32_t* tokens;       // (S, Lmax)
  const int32_t* lens;         // (S)
  const int32_t* pairs;        // (P, 2)
  int32_t* stats;              // (P, 8)
};

// the row's two strings, or false for a bad row; reads lens only at indices inside the pool
__device__ __forceinline__ bool ps_row(const PairArgs& a, int p, int& ia, int& ib, int& La, int& Lb) {
  ia = a.pairs[2 * (size_t)p];
  ib = a.pairs[2 * (size_t)p + 1];
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= a.S) return false;
  La = a.lens[ia];
  Lb = a.lens[ib];
  return La >= 0 && La <= a.Lmax && Lb >= 0 && Lb <= a.Lmax;
}

// the lanes of one wavefront exchange data through their LDS slice: order the accesses on both sides (what __syncwarp() is made of)
__device__ __forceinline__ void ps_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int ps_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// acc[n-1] += the positions q < qend of x (of them only q < p when BEFORE) whose n-gram equals g[0..n), for n = 1..4 with n <= ka
template <bool BEFORE>
__device__ __forceinline__ void ps_scan(const int* x, int Lx, int qend, int p, int ka, const int (&g)[4], int (&acc)[4]) {
  int w0 = Lx > 0 ? x[0] : 0, w1 = Lx > 1 ? x[1] : 0, w2 = Lx > 2 ? x[2] : 0;
  for (int q = 0; q < qend; ++q) {
    const int w3 = q + 3 < Lx ? x[q + 3] : 0;
    const int k = min(ka, Lx - q);                           // tokens both n-grams have from here on
    bool e = (!BEFORE || q < p) && k > 0 && g[0] == w0;
    acc[0] += e ? 1 : 0;
    e = e && k > 1 && g[1] == w1;
    acc[1] += e ? 1 : 0;
    e = e && k > 2 && g[2] == w2;
    acc[2] += e ? 1 : 0;
    e = e && k > 3 && g[3] == w3;
    acc[3] += e ? 1 : 0;
    w0 = w1; w1 = w2; w2 = w3;
  }
}

__global__ __launch_bounds__(PS_WAVES * 64) void k_pair_stats(PairArgs a) {
  __shared__ int s_a[PS_WAVES][PS_MAX_LEN], s_b[PS_WAVES][PS_MAX_LEN], s_col[PS_WAVES][2][PS_MAX_LEN + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* sa = s_a[wv];
  int* sb = s_b[wv];
  for (long pl = (long)blockIdx.x * PS_WAVES + wv; pl < a.P; pl += (long)gridDim.x * PS_WAVES) {      // (wave-uniform)
    const int p = (int)pl;
    int32_t* out = a.stats + (size_t)p * 8;
    int ia, ib, La, Lb;
    if (!ps_row(a, p, ia, ib, La, Lb)) {
      if (lane < 8) out[lane] = -1;
      continue;
    }
    ps_wave_sync();                                          // the last pair's reads are behind us
    const int32_t* ga = a.tokens + (size_t)ia * a.Lmax;
    const int32_t* gb = a.tokens + (size_t)ib * a.Lmax;
    for (int i = lane; i < La; i += 64) sa[i] = ga[i];
    for (int i = lane; i < Lb; i += 64) sb[i] = gb[i];
    ps_wave_sync();
    // ---- edit statistics
    int cur = 0;
    for (int j0 = 0; j0 < Lb; j0 += 64) {
      const int j = j0 + lane + 1;                           // this lane's column
      const bool col = j <= Lb;
      const int bj = col ? sb[j - 1] : 0;
      cur = j * PS_DEL1;                                     // D[0][j]: j deletions
      int diag = (j - 1) * PS_DEL1;                          // D[0][j-1]
      const bool park = j0 + 64 < Lb;                        // another block follows: lane 63 leaves its column behind
      const int nsteps = La + min(64, Lb - j0) - 1;
      const int* left_col = s_col[wv][(j0 >> 6) & 1];        // the column in front of this block, parked by the last one
      int* right_col = s_col[wv][((j0 >> 6) & 1) ^ 1];
      for (int s = 0; s < nsteps; ++s) {
        const int i = s - lane + 1;                          // this lane's row
        const bool on = col && i >= 1 && i <= La;
        int lft = __shfl_up(cur, 1);
        if (lane == 0 && on) lft = j0 == 0 ? i * PS_INS1 : left_col[i];
        if (on) {
          int best = diag + (sa[i - 1] != bj ? PS_SUB1 : 0);
          const int d = lft + PS_DEL1, u = cur + PS_INS1;
          if ((d & PS_FIELD) < (best & PS_FIELD)) best = d;
          if ((u & PS_FIELD) < (best & PS_FIELD)) best = u;
          cur = best;
          if (lane == 63 && park) right_col[i] = cur;
        }
        diag = lft;
      }
      ps_wave_sync();
    }
    const int cell = Lb == 0 ? La * PS_INS1 : __shfl(cur, (Lb - 1) & 63);
    // ---- clipped matches
    int m[4] = {0, 0, 0, 0};
    for (int p0 = 0; p0 < La; p0 += 64) {
      const int pos = p0 + lane;
      const int ka = min(4, La - pos);                       // the n-grams that start here: n <= ka (<= 0 behind the string)
      int g[4], cnt[4] = {0, 0, 0, 0}, rank[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = k < ka ? sa[pos + k] : 0;
      ps_scan<false>(sb, Lb, Lb, pos, ka, g, cnt);
      ps_scan<true>(sa, La, min(La, p0 + 63), pos, ka, g, rank);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] += (k < ka && rank[k] < cnt[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = ps_wave_sum(m[k]);
    if (lane == 0) {
      const int dist = cell & PS_FIELD, sub = (cell >> 10) & PS_FIELD, del = (cell >> 20) & PS_FIELD;
      out[0] = dist; out[1] = sub; out[2] = del; out[3] = dist - sub - del;
      out[4] = m[0]; out[5] = m[1]; out[6] = m[2]; out[7] = m[3];
    }
  }
}

__global__ __launch_bounds__(PS_COUNT_THREADS) void k_pair_count_bad(PairArgs a, int32_t* n_bad) {
  __shared__ int s_cnt[PS_COUNT_THREADS / 64];
  int c = 0;
  for (long p = threadIdx.x; p < a.P; p += PS_COUNT_THREADS) {
    int ia, ib, La, Lb;
    c += ps_row(a, (int)p, ia, ib, La, Lb) ? 0 : 1;
  }
  c = ps_wave_sum(c);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < PS_COUNT_THREADS / 64; ++i) total += s_cnt[i];
    *n_bad = total;
  }
}

}  // namespace

}  // namespace astk

using namespace astk;

int astk_pair_stats(const astk_pair_stats_desc* d, const int32_t* tokens, const int32_t* lens, const int32_t* pairs, int32_t* stats,
                    int32_t* n_bad, void* stream) {
  ASTK_CHECK_DESC(d, astk_pair_stats_desc);
  ASTK_CHECK(d->S >= 1, "pair_stats: S = %d strings, the pool must hold at least one", d->S);
  ASTK_CHECK(d->P >= 1, "pair_stats: P = %d pairs, there must be at least one", d->P);
  ASTK_CHECK(d->Lmax >= 1 && d->Lmax <= PS_MAX_LEN, "pair_stats: Lmax = %d lies outside 1..%d", d->Lmax, PS_MAX_LEN);
  ASTK_CHECK(tokens && lens && pairs && stats, "pair_stats: tokens, lens, pairs and stats must not be null");
  PairArgs a;
  a.S = d->S; a.Lmax = d->Lmax; a.P = d->P;
  a.tokens = tokens; a.lens = lens; a.pairs = pairs; a.stats = stats;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)std::min<long>(((long)d->P + PS_WAVES - 1) / PS_WAVES, PS_MAX_BLOCKS);
  hipLaunchKernelGGL(k_pair_stats, dim3(blocks), dim3(PS_WAVES * 64), 0, s, a);
  ASTK_LAUNCH_CHECK();
  if (n_bad) {
    hipLaunchKernelGGL(k_pair_count_bad, dim3(1), dim3(PS_COUNT_THREADS), 0, s, a, n_bad);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}
