// CTC prefix beam search: n-best label strings from the CTC head alone (include/astk.h astk_ctc_beam).  Float64 in
// the log domain, no atomics: every output is the same bits from run to run, and the discrete outcome is a host model's
// (tests/ctc_beam_model.py).  logits is only read.
//
// Two launches on the caller's stream:
//   k_ctc_beam_frames  one wavefront per valid frame (b, t): the float64 log-sum-exp over V (ctc_rows.h ctc_wave_lse), the blank's
//                      log-probability and the C best labels >= first_label in the candidate order (higher first, equal ones lower id
//                      first).  Independent of the recursion, coalesced over V.
//   k_ctc_beam_scan    one workgroup per row, one thread per candidate: thread j < N is the stay candidate of slot j, thread
//                      N + j * C + k the extension of slot j by the frame's k-th proposal -- the thread index IS the tie order.  The beam
//                      lives in two LDS buffers; the frames' records are read CB_PF frames at a time in front of the recursion.  Per
//                      frame, four barriers:
//                        A  every candidate's terms; an extension that spells a member of the beam hands its p_nb to that member's
//                           stay candidate (one writer per member) instead of standing itself
//                        B  the stay candidates take what was handed to them; every score to LDS
//                        C  the rank of every live candidate by counting (score, then thread index); rank < N writes slot `rank`
//                        D  wave 0 makes the new extensions' nodes canonical (below) and fetches the slots' stay emissions
//                           logits[t + 1][last label], the one read that depends on the beam
//                      then the backtrace into tokens, a lane per slot.
// Prefixes are nodes of a per-row trie that IS an open-addressed hash table in the workspace: an entry holds the key (parent node,
// label), and its index is the node id.  A kept extension looks its key up (every lane its own, they differ) and takes the entry it
// finds -- so a string that left the beam and comes back gets its old node, and "the same string" is "the same node" -- or inserts it
// at the first free entry of its probe sequence; two lanes that meet at one free entry are ordered by rank, the loser probes on.
// Entries are never removed.  A row uses the first 2^k >= 2 (n N + 1) entries of its table, so probe sequences stay short.
#include "ctc_rows.h"
#include <math.h>

namespace astk {

namespace {

constexpr int CB_MAX_N = 16, CB_MAX_C = 16, CB_MAX_T = 2048;
constexpr int CB_PF = 8;                                     // frames of records a thread reads in one go
constexpr int CB_THREADS = (CB_MAX_N * (CB_MAX_C + 1) + 63) / 64 * 64;
constexpr int CB_ROOT = -1;                                  // the empty prefix's node
constexpr int CB_NO_PARENT = -2;                             // parent of the root and of an unused slot: equals no node
constexpr int CB_PENDING = -3;                               // a kept extension in front of step D
constexpr unsigned long long CB_EMPTY = ~0ull;

struct CtcBeamWs {
  double2* fr;                 // [B][T]      .x = log p(blank), .y = lse
  double* px;                  // [B][T][C]   log p of the proposals
  int* pid;                    // [B][T][C]   their ids
  unsigned long long* tab;     // [B][2^tab_bits]  the tries
  int tab_bits;
  size_t bytes;
};
static int table_bits(long nodes) {
  int bits = 2;
  while ((1l << bits) < 2 * nodes) ++bits;
  return bits;
}
static CtcBeamWs beam_carve(const astk_ctc_beam_desc* d, void* base) {
  CtcBeamWs w;
  const size_t bt = (size_t)d->B * d->T;
  CtcBump c(base);
  w.tab_bits = table_bits((long)d->T * d->N + 1);
  w.fr = c.take<double2>(bt);
  w.px = c.take<double>(bt * d->C);
  w.pid = c.take<int>(bt * d->C);
  w.tab = c.take<unsigned long long>((size_t)d->B << w.tab_bits);
  w.bytes = c.off;
  return w;
}

// the proposal order of one frame: higher log-probability first, equal ones lower id first
__device__ __forceinline__ bool cb_before(double a, int ia, double b, int ib) { return a > b || (a == b && ia < ib); }

__global__ __launch_bounds__(256) void k_ctc_beam_frames(int B, int T, int V, long ldv, int C, int first_label, int blank,
                                                         const float* __restrict__ logits, const int32_t* __restrict__ len, CtcBeamWs w) {
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= (long)B * T) return;
  const int b = (int)(f / T), t = (int)(f - (long)b * T);
  if (t >= ctc_row_len(len, b, T)) return;
  const float* x = logits + f * ldv;
  const double lse = ctc_wave_lse<double>(x, V, lane);
  if (lane == 0) w.fr[f] = make_double2((double)x[blank] - lse, lse);
  double pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < C; ++k) {
    double bv = -INFINITY;
    int bi = -1;
    for (int v = first_label + lane; v < V; v += 64) {
      const double lp = (double)x[v] - lse;
      if (cb_before(pv, pi, lp, v) && (bi < 0 || cb_before(lp, v, bv, bi))) { bv = lp; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || cb_before(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {                                    // (no label left, NaN logits: a proposal at -inf, which no beam keeps)
      w.px[f * C + k] = bi < 0 ? -INFINITY : bv;
      w.pid[f * C + k] = bi < 0 ? first_label : bi;
    }
    pv = bv; pi = bi;
  }
}

struct CtcBeamArgs {
  int T, V, N, C, Lm, blank;
  long ldv;
  const float* logits;
  const int32_t* len;
  int32_t* tokens;             // (B, N, Lm)
  int32_t* n_labels;           // (B, N)
  double* score;               // (B, N)
};

__device__ __forceinline__ unsigned long long cb_key(int parent, int label) {
  return ((unsigned long long)(unsigned)(parent + 1) << 32) | (unsigned)label;
}

__global__ __launch_bounds__(CB_THREADS) void k_ctc_beam_scan(CtcBeamArgs a, CtcBeamWs w) {
  __shared__ double s_pb[2][CB_MAX_N], s_pnb[2][CB_MAX_N], s_tot[2][CB_MAX_N];       // tot = logaddexp(p_b, p_nb); -inf: an unused slot
  __shared__ int s_node[2][CB_MAX_N], s_par[2][CB_MAX_N], s_last[2][CB_MAX_N], s_len[2][CB_MAX_N];
  __shared__ double s_mrg[CB_MAX_N];                    // what an extension hands to the member it spells
  __shared__ double c_score[CB_MAX_N * (CB_MAX_C + 1)];
  __shared__ int s_wcnt[CB_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int N = a.N, C = a.C, ncand = N * (C + 1);
  const int n = ctc_row_len(a.len, b, a.T);
  const bool is_stay = tid < N, is_ext = tid >= N && tid < ncand;
  const int ej = is_ext ? (tid - N) / C : tid;          // the candidate's source slot
  const int ek = is_ext ? (tid - N) - ej * C : 0;       // an extension's proposal rank
  // ---- the row's trie: the first 2^rb entries of its table
  int rb = 2;
  while ((1l << rb) < 2 * ((long)n * N + 1)) ++rb;      // (<= tab_bits: n <= T)
  const int mask = (1 << rb) - 1;
  unsigned long long* tab = w.tab + ((size_t)b << w.tab_bits);
  if (n > 0)
    for (int i = tid; i <= mask; i += nt) tab[i] = CB_EMPTY;
  if (tid < 2 * CB_MAX_N) {
    const int bf = tid / CB_MAX_N, j = tid % CB_MAX_N;
    const bool root = bf == 0 && j == 0;                // before frame 0: the empty prefix with p_b = 0
    s_pb[bf][j] = root ? 0.0 : -INFINITY;
    s_pnb[bf][j] = -INFINITY;
    s_tot[bf][j] = root ? 0.0 : -INFINITY;
    s_node[bf][j] = CB_ROOT;
    s_par[bf][j] = CB_NO_PARENT;
    s_last[bf][j] = -1;
    s_len[bf][j] = 0;
  }
  if (tid < CB_MAX_N) s_mrg[tid] = -INFINITY;
  __syncthreads();
  const double2* fr = w.fr + (size_t)b * a.T;
  const double* px = w.px + (size_t)b * a.T * C;
  const int* pid = w.pid + (size_t)b * a.T * C;
  const float* lg = a.logits + (size_t)b * a.T * a.ldv;
  int cur = 0;
  float em_next = 0.f;                                  // a stay thread: logits[t][last label of its slot] of the coming frame
  for (int t0 = 0; t0 < n; t0 += CB_PF) {
    double qa[CB_PF], qb[CB_PF];                        // stay: log p(blank), lse; extension: log p(proposal), its id
    int qi[CB_PF];
#pragma unroll
    for (int k = 0; k < CB_PF; ++k) {
      const int t = t0 + k;
      qa[k] = 0.0; qb[k] = 0.0; qi[k] = -1;
      if (t < n) {
        if (is_stay) {
          const double2 v = fr[t];
          qa[k] = v.x; qb[k] = v.y;
        } else if (is_ext) {
          qa[k] = px[(size_t)t * C + ek];
          qi[k] = pid[(size_t)t * C + ek];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CB_PF; ++k) {
      const int t = t0 + k;
      if (t >= n) break;                                // (uniform)
      // ---- A: the candidates' terms
      double my_pb = -INFINITY, my_pnb = -INFINITY, my_score = -INFINITY;
      int my_c = -1;
      if (is_stay) {
        const double tot = s_tot[cur][tid];
        if (tot > -INFINITY) {
          my_pb = tot + qa[k];
          if (s_last[cur][tid] >= 0) my_pnb = s_pnb[cur][tid] + ((double)em_next - qb[k]);
        }
      } else if (is_ext) {
        const double tot = s_tot[cur][ej];
        if (tot > -INFINITY && s_len[cur][ej] < a.Lm) {
          my_c = qi[k];
          const double p = (my_c == s_last[cur][ej] ? s_pb[cur][ej] : tot) + qa[k];
          const int node = s_node[cur][ej];
          int hit = -1;
          for (int j = 0; j < N; ++j)
            if (s_par[cur][j] == node && s_last[cur][j] == my_c) hit = j;
          if (hit >= 0) s_mrg[hit] = p;                 // (at most one extension spells a given member)
          else { my_pnb = p; my_score = p; }
        }
      }
      __syncthreads();
      // ---- B: the scores
      if (is_stay) {
        const double m = s_mrg[tid];
        if (m > -INFINITY) my_pnb = lae(my_pnb, m);
        my_score = lae(my_pb, my_pnb);
      }
      if (tid < ncand) c_score[tid] = my_score;
      const bool live = my_score > -INFINITY;
      const unsigned long long lm = __ballot(live);
      if (lane == 0) s_wcnt[wv] = __popcll(lm);
      __syncthreads();
      // ---- C: rank by counting; the new beam in rank order
      const int nxt = cur ^ 1;
      if (is_stay) s_mrg[tid] = -INFINITY;
      int nlive = 0;
      for (int i = 0; i < nw; ++i) nlive += s_wcnt[i];
      if (live) {
        int rank = 0;
        for (int i = 0; i < ncand; ++i) {
          const double s = c_score[i];
          rank += (s > my_score || (s == my_score && i < tid)) ? 1 : 0;
        }
        if (rank < N) {
          s_pb[nxt][rank] = my_pb;
          s_pnb[nxt][rank] = my_pnb;
          s_tot[nxt][rank] = my_score;
          s_node[nxt][rank] = is_stay ? s_node[cur][ej] : CB_PENDING;
          s_par[nxt][rank] = is_stay ? s_par[cur][ej] : s_node[cur][ej];
          s_last[nxt][rank] = is_stay ? s_last[cur][ej] : my_c;
          s_len[nxt][rank] = s_len[cur][ej] + (is_stay ? 0 : 1);
        }
      }
      if (tid < N && tid >= nlive) {                    // fewer live candidates than slots
        s_pb[nxt][tid] = -INFINITY; s_pnb[nxt][tid] = -INFINITY; s_tot[nxt][tid] = -INFINITY;
        s_node[nxt][tid] = CB_ROOT; s_par[nxt][tid] = CB_NO_PARENT; s_last[nxt][tid] = -1; s_len[nxt][tid] = 0;
      }
      __syncthreads();
      // ---- D: wave 0, lane r = slot r: the stay emission of the coming frame, the nodes of the kept extensions
      if (wv == 0) {
        const bool slot = lane < N;
        const int last = slot ? s_last[nxt][lane] : -1;
        if (slot && last >= 0 && t + 1 < n && s_tot[nxt][lane] > -INFINITY) em_next = lg[(size_t)(t + 1) * a.ldv + last];
        const bool pend = slot && s_node[nxt][lane] == CB_PENDING;
        const unsigned long long key = pend ? cb_key(s_par[nxt][lane], last) : 0ull;
        int pos = (int)((key * 0x9E3779B97F4A7C15ull) >> (64 - rb));
        bool need = false;
        if (pend) {
          need = true;
          for (int it = 0; it <= mask; ++it) {          // (the table is at most half full: an empty entry ends the probe)
            const unsigned long long q = tab[pos];
            if (q == key) { need = false; break; }
            if (q == CB_EMPTY) break;
            pos = (pos + 1) & mask;
          }
        }
        for (int round = 0; round < CB_MAX_N && __ballot(need); ++round) {      // (every round places the lowest waiting lane)
          const unsigned long long waiting = __ballot(need);
          bool lose = false;
          for (int i = 0; i < N; ++i) {
            const int pi = __shfl(pos, i);
            if (((waiting >> i) & 1ull) && i < lane && pi == pos) lose = true;
          }
          if (need && !lose) { tab[pos] = key; need = false; }
          __threadfence_block();
          if (need) {
            for (int it = 0; it <= mask; ++it) {
              pos = (pos + 1) & mask;
              if (tab[pos] == CB_EMPTY) break;
            }
          }
        }
        if (pend) s_node[nxt][lane] = pos;
      }
      __syncthreads();
      cur = nxt;
    }
  }
  // ---- the result: slots in rank order, the labels by a walk to the root (a lane per slot)
  int32_t* tok = a.tokens + (size_t)b * N * a.Lm;
  if (tid < N) {
    const bool used = s_tot[cur][tid] > -INFINITY;
    const int len = used ? s_len[cur][tid] : 0;
    a.n_labels[(size_t)b * N + tid] = used ? len : -1;
    a.score[(size_t)b * N + tid] = used ? s_tot[cur][tid] : -INFINITY;
    int node = s_node[cur][tid];
    for (int i = len - 1; i >= 0 && node >= 0; --i) {
      const unsigned long long q = tab[node];
      tok[(size_t)tid * a.Lm + i] = (int)(unsigned)q;
      node = (int)(unsigned)(q >> 32) - 1;
    }
  }
  for (int i = tid; i < N * a.Lm; i += nt) {
    const int r = i / a.Lm;
    const int len = s_tot[cur][r] > -INFINITY ? s_len[cur][r] : 0;
    if (i - r * a.Lm >= len) tok[i] = a.blank;
  }
}

static int beam_check_desc(const astk_ctc_beam_desc* d, const char* who) {
  ASTK_CHECK_DESC(d, astk_ctc_beam_desc);
  ASTK_CHECK(d->B > 0 && d->T > 0, "%s: B and T must be positive, got B = %d, T = %d", who, d->B, d->T);
  ASTK_CHECK(d->T <= CB_MAX_T, "%s: T = %d frames exceed the %d a row is limited to", who, d->T, CB_MAX_T);
  ASTK_CHECK(d->first_label >= 1 && d->V > d->first_label, "%s: V = %d must lie above first_label = %d (at least one label)", who, d->V,
             d->first_label);
  ASTK_CHECK(d->ldv >= d->V, "%s: ldv = %ld is below V = %d", who, d->ldv, d->V);
  ASTK_CHECK(d->blank >= 0 && d->blank < d->V && d->blank < d->first_label, "%s: blank = %d must lie in [0, V = %d) and below first_label = %d",
             who, d->blank, d->V, d->first_label);
  ASTK_CHECK(d->N >= 1 && d->N <= CB_MAX_N, "%s: the beam width N = %d lies outside 1..%d", who, d->N, CB_MAX_N);
  ASTK_CHECK(d->C >= 1 && d->C <= CB_MAX_C && d->C <= d->V - d->first_label,
             "%s: C = %d proposals per frame lie outside 1..min(%d, V - first_label = %d)", who, d->C, CB_MAX_C, d->V - d->first_label);
  ASTK_CHECK(d->max_labels >= 1 && d->max_labels <= ASTK_CTC_MAX_LABELS, "%s: max_labels = %d lies outside 1..%d", who, d->max_labels,
             ASTK_CTC_MAX_LABELS);
  ASTK_CHECK((size_t)d->B * d->T <= 0x7fffffffu / 4, "%s: B * T = %zu frames do not fit the launch grid", who, (size_t)d->B * d->T);
  return 0;
}

}  // namespace

}  // namespace astk

using namespace astk;

size_t astk_ctc_beam_workspace_bytes(const astk_ctc_beam_desc* d) {
  if (beam_check_desc(d, "ctc_beam_workspace_bytes") != 0) return 0;
  return beam_carve(d, nullptr).bytes;
}

int astk_ctc_beam(const astk_ctc_beam_desc* d, const float* logits, const int32_t* input_len, int32_t* tokens, int32_t* n_labels,
                  double* score, void* ws, size_t ws_bytes, void* stream) {
  ASTK_TRY(beam_check_desc(d, "ctc_beam"));
  const CtcBeamWs w = beam_carve(d, ws);
  ASTK_TRY(ctc_check_ptrs("ctc_beam", logits && tokens && n_labels && score, "logits, tokens, n_labels, score", ws));
  ASTK_TRY(ctc_check_ws_bytes("ctc_beam", "ctc_beam", ws_bytes, w.bytes));
  hipStream_t s = (hipStream_t)stream;
  const unsigned frames = (unsigned)((size_t)d->B * d->T);
  hipLaunchKernelGGL(k_ctc_beam_frames, dim3((frames + 3) / 4), dim3(256), 0, s, d->B, d->T, d->V, d->ldv, d->C, d->first_label, d->blank,
                     logits, input_len, w);
  ASTK_LAUNCH_CHECK();
  CtcBeamArgs a;
  a.T = d->T; a.V = d->V; a.N = d->N; a.C = d->C; a.Lm = d->max_labels; a.blank = d->blank;
  a.ldv = d->ldv;
  a.logits = logits; a.len = input_len; a.tokens = tokens; a.n_labels = n_labels; a.score = score;
  const int nt = (d->N * (d->C + 1) + 63) / 64 * 64;    // one thread per candidate (<= 320)
  hipLaunchKernelGGL(k_ctc_beam_scan, dim3(d->B), dim3(nt), 0, s, a, w);
  ASTK_LAUNCH_CHECK();
  return 0;
}
