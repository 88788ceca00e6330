// Batched beam search (nn.py:235-322 of the reference, many utterances per decoder step).
//
// Every live hypothesis of U utterances is one row of ONE decoder step over R = U*N rows: row u*N + j is slot j of utterance u.
// A step (astk_beam_step) is
//   the eval-mode decoder step of decoder.hip (decoder_step_run: embedding, LSTM cells, LayerNorm, heads, Wc, Wo) with the per-row
//   attention of attn.hip (row r attends over enc[u, 0:T''_u] only), the new states left in the decoder's workspace
//   -> k_beam_select: one workgroup per utterance -- float64 log-sum-exp and top-K of every live row, the merge with the carried
//      (finished) and empty slots in the reference's candidate order, stable top-N, the step's history, and the state gather into
//      the slots' buffers.
// Rows of different utterances never interact (eval mode: BatchNorm on running statistics, no dropout), so the N-best list of every
// utterance is the one decode_beam finds for it alone.  No workgroup waits for another.
#include "common.h"

namespace astk {

namespace {

constexpr int MAXN = ASTK_BEAM_MAX_N, MAXK = ASTK_BEAM_MAX_K;
constexpr int ST_EMPTY = 0, ST_LIVE = 1, ST_DONE = 2;

struct BeamSelArgs {
  int U, N, K, V, T, eos, step, nl, H, A;
  const float* logits; long ld_logits;           // (R, V)
  const float* alpha; long ld_alpha;             // (R, >= T): the first head's alpha of this step
  const float* c_new[ASTK_MAX_RNN_LAYERS];       // (R, H) each: the states this step computed for every row
  const float* h_new[ASTK_MAX_RNN_LAYERS];
  const float* ht_new;                           // (R, A)
  float* c; float* h; float* ht;                 // the slots' states (n_layers, R, H) / (R, A): old in, gathered out
  int32_t* tokens; double* score; int32_t* status; int32_t* frozen; unsigned* n_frozen;
  int32_t* hist; float* hist_alpha;
  // the joint CTC-attention step (k_beam_select<true>) only
  double w;                                      // the CTC weight
  const int32_t* row_len;                        // (R)
  const int32_t* cand_tok; const double* cand_lp; const double* cand_psi; const double* cand_state;   // the proposals (R, K) and their new CTC states (R, K, T, 2)
  double* ctc_state; double* att_score; double* psi; int32_t* n_labels;      // the slots' (R, T, 2), (R), (R), (R): old in, gathered out
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the candidate order of one row: higher log-probability first, equal ones lower token id first
__device__ __forceinline__ bool before(double a, int ia, double b, int ib) { return a > b || (a == b && ia < ib); }

// One wavefront: the float64 log-sum-exp of a row's V logits, then its K best tokens in the candidate order; lane 0 writes
// top[k] = base + logp and topi[k] = the token.
__device__ __forceinline__ void row_topk(const float* x, int V, int K, int lane, double base, double* top, int* topi) {
  double mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmax(mx, (double)x[v]);
  mx = wave_max_d(mx);
  double sum = 0.0;
  for (int v = lane; v < V; v += 64) sum += exp((double)x[v] - mx);
  sum = wave_sum_d(sum);
  const double lse = log(sum) + mx;
  double pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    double bv = -INFINITY;
    int bi = -1;
    for (int v = lane; v < V; v += 64) {
      const double lp = (double)x[v] - lse;
      if (before(pv, pi, lp, v) && (bi < 0 || before(lp, v, bv, bi))) { bv = lp; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || before(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      top[k] = base + bv;
      topi[k] = bi < 0 ? 0 : bi;
    }
    pv = bv; pi = bi;
  }
}

// The proposals of the joint step: every live row's K best tokens and their log-probabilities, for the prefix scorer.  One wavefront per row.
__global__ __launch_bounds__(256) void k_beam_propose(int R, int K, int V, const float* __restrict__ logits, long ld_logits,
                                                      const int32_t* __restrict__ status, int32_t* __restrict__ cand_tok,
                                                      double* __restrict__ cand_lp) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R || status[r] != ST_LIVE) return;
  row_topk(logits + (long)r * ld_logits, V, K, threadIdx.x & 63, 0.0, cand_lp + (long)r * K, cand_tok + (long)r * K);
}

// CTC: the joint step -- the proposals and their prefix scores come from k_beam_propose and the scorer (ctc_prefix.hip)
template <bool CTC>
__global__ __launch_bounds__(256) void k_beam_select(BeamSelArgs a) {
  __shared__ double s_score[MAXN];
  __shared__ int s_status[MAXN], s_tok[MAXN];
  __shared__ double s_top[MAXN * MAXK];
  __shared__ int s_topi[MAXN * MAXK];
  __shared__ double c_score[MAXN * MAXK];
  __shared__ int c_parent[MAXN * MAXK], c_tok[MAXN * MAXK], c_carried[MAXN * MAXK];
  __shared__ int sel[MAXN];
  __shared__ int s_ncand;
  __shared__ int n_parent[MAXN], n_carried[MAXN], n_status[MAXN];
  __shared__ double s_att[MAXN], s_psi[MAXN];                                  // CTC only: the slots' terms, the candidates' proposal index
  __shared__ int s_nlab[MAXN], c_kidx[MAXN * MAXK], n_kidx[MAXN];
  const int u = blockIdx.x, N = a.N, K = a.K, V = a.V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = (long)u * N;
  const long R = (long)a.U * N;
  if (threadIdx.x < N) {
    s_score[threadIdx.x] = a.score[row0 + threadIdx.x];
    s_status[threadIdx.x] = a.status[row0 + threadIdx.x];
    s_tok[threadIdx.x] = a.tokens[row0 + threadIdx.x];
    if constexpr (CTC) {
      s_att[threadIdx.x] = a.att_score[row0 + threadIdx.x];
      s_psi[threadIdx.x] = a.psi[row0 + threadIdx.x];
      s_nlab[threadIdx.x] = a.n_labels[row0 + threadIdx.x];
    }
  }
  __syncthreads();
  // ---- every live slot: float64 log-sum-exp over V, then its K best tokens (one wave per slot)
  if constexpr (!CTC) {
    for (int j = wave; j < N; j += 4) {
      if (s_status[j] != ST_LIVE) continue;
      row_topk(a.logits + (row0 + j) * a.ld_logits, V, K, lane, s_score[j], s_top + j * MAXK, s_topi + j * MAXK);
    }
  }
  __syncthreads();
  // ---- the candidates in the reference's order: slot by slot, a finished slot itself, a live one its K expansions
  if (threadIdx.x == 0) {
    int n = 0;
    for (int j = 0; j < N; ++j) {
      if (s_status[j] == ST_DONE) {
        c_score[n] = s_score[j]; c_parent[n] = j; c_tok[n] = s_tok[j]; c_carried[n] = 1; ++n;
      } else if (s_status[j] == ST_LIVE) {
        for (int k = 0; k < K; ++k) {
          if constexpr (CTC) {           // the two absolute terms, never a running sum of increments; a dead CTC term ranks as -inf
            const long ck = (row0 + j) * K + k;
            const double ps = a.cand_psi[ck];
            c_score[n] = ps == -INFINITY ? -INFINITY : (1.0 - a.w) * (s_att[j] + a.cand_lp[ck]) + a.w * ps;
            c_tok[n] = a.cand_tok[ck];
            c_kidx[n] = k;
          } else {
            c_score[n] = s_top[j * MAXK + k]; c_tok[n] = s_topi[j * MAXK + k];
          }
          c_parent[n] = j; c_carried[n] = 0; ++n;
        }
      }
    }
    for (int i = 0; i < n; ++i)      // (a NaN score ranks last: the ranks below stay a permutation)
      if (isnan(c_score[i])) c_score[i] = -INFINITY;
    s_ncand = n;
  }
  __syncthreads();
  // ---- stable top-N: candidate i lands at its rank (higher score first, equal scores keep the earlier candidate)
  const int C = s_ncand;
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    const double si = c_score[i];
    int rank = 0;
    for (int c = 0; c < C; ++c) rank += (c_score[c] > si || (c_score[c] == si && c < i)) ? 1 : 0;
    if (rank < N) sel[rank] = i;
  }
  __syncthreads();
  const int nsel = C < N ? C : N;
  if (threadIdx.x < N) {
    const int i = threadIdx.x;
    const long r = row0 + i;
    int32_t* hr = a.hist + ((long)a.step * R + r) * 4;
    if (i < nsel) {
      const int c = sel[i];
      const int carried = c_carried[c], tok = c_tok[c];
      n_parent[i] = c_parent[c];
      n_carried[i] = carried;
      n_status[i] = (carried || tok == a.eos) ? ST_DONE : ST_LIVE;
      a.score[r] = c_score[c];
      a.tokens[r] = tok;
      hr[0] = c_parent[c]; hr[1] = tok; hr[2] = carried; hr[3] = 0;
      if constexpr (CTC) {
        const int p = c_parent[c];
        const long ck = (row0 + p) * K + c_kidx[c];
        n_kidx[i] = (carried || tok == a.eos) ? -1 : c_kidx[c];          // -1: the slot keeps its parent's own CTC state
        a.att_score[r] = carried ? s_att[p] : s_att[p] + a.cand_lp[ck];
        a.psi[r] = carried ? s_psi[p] : a.cand_psi[ck];
        a.n_labels[r] = s_nlab[p] + (n_kidx[i] >= 0 ? 1 : 0);
      }
    } else {
      if constexpr (CTC) { a.att_score[r] = 0.0; a.psi[r] = 0.0; a.n_labels[r] = 0; }
      n_parent[i] = -1;
      n_carried[i] = 0;
      n_status[i] = ST_EMPTY;
      a.score[r] = 0.0;
      hr[0] = -1; hr[1] = 0; hr[2] = 0; hr[3] = 0;
    }
    a.status[r] = n_status[i];
  }
  __syncthreads();
  // ---- history: a new expansion records its parent row's alpha of this step
  for (int i = 0; i < nsel; ++i) {
    if (n_carried[i]) continue;
    const float* src = a.alpha + (row0 + n_parent[i]) * a.ld_alpha;
    float* dst = a.hist_alpha + ((long)a.step * R + row0 + i) * a.T;
    for (int t = threadIdx.x; t < a.T; t += blockDim.x) dst[t] = src[t];
  }
  // ---- state gather: a new expansion takes its parent row's new state, a carried slot its own old one (which may sit in another row
  // of this utterance).  One thread owns one column of all N rows: it reads every source before it writes, so the permutation can run
  // in place.
  const int nl = a.nl, H = a.H, A = a.A;
  for (int l = 0; l <= 2 * nl; ++l) {
    const int w = l < 2 * nl ? H : A;
    float* dst = l < 2 * nl ? ((l & 1) ? a.h : a.c) + (size_t)(l >> 1) * R * H : a.ht;
    const float* fresh = l < 2 * nl ? ((l & 1) ? a.h_new[l >> 1] : a.c_new[l >> 1]) : a.ht_new;
    for (int col = threadIdx.x; col < w; col += blockDim.x) {
      float v[MAXN];
#pragma unroll
      for (int i = 0; i < MAXN; ++i) {
        v[i] = 0.f;
        if (i < nsel) {
          const long src = row0 + n_parent[i];
          v[i] = n_carried[i] ? dst[src * w + col] : fresh[src * w + col];
        }
      }
#pragma unroll
      for (int i = 0; i < MAXN; ++i)
        if (i < nsel) dst[(row0 + i) * w + col] = v[i];
    }
  }
  if constexpr (CTC) {
    // ---- the CTC states (T''_u, 2) the same way: a new label expansion takes its candidate's new state, every other slot its parent's own
    const int cols = 2 * a.row_len[row0];
    const long ld = 2 * (long)a.T;
    for (int col = threadIdx.x; col < cols; col += blockDim.x) {
      double v[MAXN];
#pragma unroll
      for (int i = 0; i < MAXN; ++i) {
        v[i] = 0.0;
        if (i < nsel) {
          const long src = row0 + n_parent[i];
          v[i] = n_kidx[i] < 0 ? a.ctc_state[src * ld + col] : a.cand_state[(src * K + n_kidx[i]) * ld + col];
        }
      }
#pragma unroll
      for (int i = 0; i < MAXN; ++i)
        if (i < nsel) a.ctc_state[(row0 + i) * ld + col] = v[i];
    }
  }
  if (threadIdx.x == 0) {
    bool all_done = true;
    for (int i = 0; i < N; ++i) all_done = all_done && n_status[i] != ST_LIVE;
    if (all_done && a.frozen[u] == 0) {
      a.frozen[u] = 1;
      atomicAdd(a.n_frozen, 1u);
    }
  }
}

int check_beam(const astk_beam_desc* b, const astk_beam_state* st, int step) {
  ASTK_CHECK_DESC(b, astk_beam_desc);
  ASTK_CHECK_DESC(st, astk_beam_state);
  ASTK_CHECK(b->U > 0 && b->T > 0 && b->S > 0 && b->V > 1, "beam: bad dims (U=%d T=%d S=%d V=%d)", b->U, b->T, b->S, b->V);
  ASTK_CHECK(b->N >= 1 && b->N <= MAXN, "beam: N = %d outside 1..%d (the select kernel's limit)", b->N, MAXN);
  ASTK_CHECK(b->K >= 1 && b->K <= MAXK, "beam: K = %d outside 1..%d (the select kernel's limit)", b->K, MAXK);
  ASTK_CHECK(b->K <= b->V, "beam: K = %d larger than the vocabulary V = %d", b->K, b->V);
  ASTK_CHECK(step >= 0 && step < b->S, "beam: step %d outside the history's 0..%d", step, b->S - 1);
  ASTK_CHECK(b->lengths_host, "beam: lengths_host is null");
  for (int u = 0; u < b->U; ++u)
    ASTK_CHECK(b->lengths_host[u] >= 1 && b->lengths_host[u] <= b->T, "beam: utterance %d has T'' = %d outside 1..%d", u,
               b->lengths_host[u], b->T);
  ASTK_CHECK(st->row_utt && st->row_len && st->c && st->h && st->ht && st->tokens && st->score && st->status && st->frozen &&
                 st->n_frozen && st->hist && st->hist_alpha, "beam: null state buffer");
  return 0;
}

int beam_select_launch(const astk_beam_desc* b, const astk_beam_state* st, BeamSelArgs& a, hipStream_t s) {
  a.U = b->U; a.N = b->N; a.K = b->K; a.V = b->V; a.T = b->T; a.eos = b->eos;
  a.c = st->c; a.h = st->h; a.ht = st->ht;
  a.tokens = st->tokens; a.score = st->score; a.status = st->status; a.frozen = st->frozen; a.n_frozen = st->n_frozen;
  a.hist = st->hist; a.hist_alpha = st->hist_alpha;
  hipLaunchKernelGGL(k_beam_select<false>, dim3(b->U), dim3(256), 0, s, a);
  ASTK_LAUNCH_CHECK();
  return 0;
}

// The joint step behind the decoder step: proposals, prefix scores (ctc_prefix.hip), selection and gather.
int beam_select_ctc_launch(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* ctc, BeamSelArgs& a, hipStream_t s) {
  a.U = b->U; a.N = b->N; a.K = b->K; a.V = b->V; a.T = b->T; a.eos = b->eos;
  a.c = st->c; a.h = st->h; a.ht = st->ht;
  a.tokens = st->tokens; a.score = st->score; a.status = st->status; a.frozen = st->frozen; a.n_frozen = st->n_frozen;
  a.hist = st->hist; a.hist_alpha = st->hist_alpha;
  CtcPrefixWs w;
  ctc_prefix_ws_carve(ctc->ws, b->U, b->N, b->K, b->T, b->V, w);
  const int R = b->U * b->N;
  hipLaunchKernelGGL(k_beam_propose, dim3((R + 3) / 4), dim3(256), 0, s, R, b->K, b->V, a.logits, a.ld_logits, st->status, w.cand_tok,
                     w.cand_lp);
  ASTK_LAUNCH_CHECK();
  ASTK_TRY(ctc_prefix_score_launch(b, st, ctc, w.cand_tok, w.cand_psi, w.cand_state, 0, s));
  a.w = ctc->weight; a.row_len = st->row_len;
  a.cand_tok = w.cand_tok; a.cand_lp = w.cand_lp; a.cand_psi = w.cand_psi; a.cand_state = w.cand_state;
  a.ctc_state = ctc->state; a.att_score = ctc->att_score; a.psi = ctc->psi; a.n_labels = ctc->n_labels;
  hipLaunchKernelGGL(k_beam_select<true>, dim3(b->U), dim3(256), 0, s, a);
  ASTK_LAUNCH_CHECK();
  return 0;
}

struct BeamRows { const int32_t* row_utt; const int32_t* row_len; };

int beam_attn(const void* ctx, int B, int T, int H, const float* enc, const float* q, long ldq, float* alpha, float* cv, long ldcv,
              void* ws, hipStream_t s) {
  const BeamRows* m = (const BeamRows*)ctx;
  return attn_fwd_rows_launch(B, T, H, enc, m->row_utt, m->row_len, q, ldq, alpha, cv, ldcv, ws, s);
}

int beam_dec_desc(const astk_beam_desc* b, const astk_decoder_desc* d, astk_decoder_desc& dd) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(d->B == b->U * b->N && d->T == b->T && d->V == b->V, "beam: decoder descriptor needs B = U*N (%d), T = T''max (%d), V = %d",
             b->U * b->N, b->T, b->V);
  dd = *d;
  dd.L = 2;        // one step
  return 0;
}

size_t beam_ws_bytes(const astk_decoder_desc& dd) {
  Carver c(nullptr);
  c.take<char>(decoder_step_ws_bytes(&dd));
  c.take<float>((size_t)dd.B * dd.V);
  c.take<float>((size_t)dd.B * dd.A);
  return c.total();
}

// The decoder step of all R rows into the workspace, and the selection's arguments that describe its results.
int beam_decoder_step(const astk_decoder_desc& dd, const astk_decoder_params* p, const float* enc, const astk_beam_state* st, int step,
                      void* ws, BeamSelArgs& a, hipStream_t s) {
  Carver c(ws);
  const size_t dws = decoder_step_ws_bytes(&dd);
  void* dec_ws = c.take<char>(dws);
  float* logits = c.take<float>((size_t)dd.B * dd.V);
  float* ht_new = c.take<float>((size_t)dd.B * dd.A);
  BeamRows rows{st->row_utt, st->row_len};
  DecStepIO io;
  memset(&io, 0, sizeof(io));
  io.enc = enc; io.c = st->c; io.h = st->h; io.ht_in = st->ht; io.ht_out = ht_new; io.tokens = st->tokens; io.logits = logits;
  io.attn = beam_attn; io.attn_ctx = &rows;
  io.states_in_place = false;          // the carried slots keep their old states: k_beam_select gathers
  ASTK_TRY(decoder_step_run(&dd, p, io, dec_ws, dws, s));
  memset(&a, 0, sizeof(a));
  a.step = step; a.nl = dd.n_layers; a.H = dd.H; a.A = dd.A;
  a.logits = logits; a.ld_logits = dd.V;
  a.alpha = io.alpha_ws; a.ld_alpha = io.ld_alpha_ws;
  for (int l = 0; l < dd.n_layers; ++l) { a.c_new[l] = io.c_new[l]; a.h_new[l] = io.h_new[l]; }
  a.ht_new = ht_new;
  return 0;
}

// ... the same for a step's results supplied by the caller (astk_beam_select, astk_beam_select_ctc)
void caller_sel_args(BeamSelArgs& a, const astk_beam_desc* b, int n_layers, int H, int A, const float* logits, const float* alpha,
                     long ld_alpha, const float* c_new, const float* h_new, const float* ht_new, int step) {
  const size_t R = (size_t)b->U * b->N;
  memset(&a, 0, sizeof(a));
  a.step = step; a.nl = n_layers; a.H = H; a.A = A;
  a.logits = logits; a.ld_logits = b->V;
  a.alpha = alpha; a.ld_alpha = ld_alpha;
  for (int l = 0; l < n_layers; ++l) { a.c_new[l] = c_new + l * R * H; a.h_new[l] = h_new + l * R * H; }
  a.ht_new = ht_new;
}

}  // namespace

}  // namespace astk

using namespace astk;

extern "C" {

size_t astk_beam_workspace_bytes(const astk_beam_desc* b, const astk_decoder_desc* d) {
  if (!b || b->struct_size != sizeof(astk_beam_desc)) return 0;
  astk_decoder_desc dd;
  if (beam_dec_desc(b, d, dd) != 0) return 0;
  return beam_ws_bytes(dd);
}

int astk_beam_step(const astk_beam_desc* b, const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                   const astk_beam_state* st, int step, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ASTK_TRY(check_beam(b, st, step));
  astk_decoder_desc dd;
  ASTK_TRY(beam_dec_desc(b, d, dd));
  ASTK_CHECK(ws && ws_bytes >= beam_ws_bytes(dd), "beam: workspace too small (%zu < %zu bytes)", ws_bytes, beam_ws_bytes(dd));
  ASTK_CHECK(dd.n_layers <= ASTK_MAX_RNN_LAYERS, "beam: layers");
  BeamSelArgs a;
  ASTK_TRY(beam_decoder_step(dd, p, enc, st, step, ws, a, s));
  return beam_select_launch(b, st, a, s);
}

size_t astk_beam_ctc_workspace_bytes(const astk_beam_desc* b, const astk_beam_ctc* ctc) {
  if (!b || b->struct_size != sizeof(astk_beam_desc) || !ctc || ctc->struct_size != sizeof(astk_beam_ctc)) {
    set_error("beam_ctc: null descriptor or wrong struct_size");
    return 0;
  }
  if (b->U < 1 || b->N < 1 || b->N > MAXN || b->K < 1 || b->K > MAXK || b->T < 1 || b->T > ASTK_BEAM_CTC_MAX_T || b->V < 2) {
    set_error("beam_ctc: bad dims (U=%d N=%d K=%d T=%d V=%d; T at most %d)", b->U, b->N, b->K, b->T, b->V, ASTK_BEAM_CTC_MAX_T);
    return 0;
  }
  CtcPrefixWs w;
  return ctc_prefix_ws_carve(nullptr, b->U, b->N, b->K, b->T, b->V, w);
}

int astk_beam_ctc_init(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* ctc, void* stream) {
  ASTK_TRY(check_beam(b, st, 0));
  ASTK_TRY(ctc_prefix_check(b, ctc));
  return ctc_prefix_init_launch(b, st, ctc, (hipStream_t)stream);
}

int astk_beam_step_ctc(const astk_beam_desc* b, const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                       const astk_beam_state* st, const astk_beam_ctc* ctc, int step, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ASTK_TRY(check_beam(b, st, step));
  ASTK_TRY(ctc_prefix_check(b, ctc));
  astk_decoder_desc dd;
  ASTK_TRY(beam_dec_desc(b, d, dd));
  ASTK_CHECK(ws && ws_bytes >= beam_ws_bytes(dd), "beam: workspace too small (%zu < %zu bytes)", ws_bytes, beam_ws_bytes(dd));
  ASTK_CHECK(dd.n_layers <= ASTK_MAX_RNN_LAYERS, "beam: layers");
  BeamSelArgs a;
  ASTK_TRY(beam_decoder_step(dd, p, enc, st, step, ws, a, s));
  return beam_select_ctc_launch(b, st, ctc, a, s);
}

int astk_beam_select_ctc(const astk_beam_desc* b, int n_layers, int H, int A, const float* logits, const float* alpha, long ld_alpha,
                         const float* c_new, const float* h_new, const float* ht_new, const astk_beam_state* st,
                         const astk_beam_ctc* ctc, int step, void* stream) {
  ASTK_TRY(check_beam(b, st, step));
  ASTK_TRY(ctc_prefix_check(b, ctc));
  ASTK_CHECK(n_layers >= 1 && n_layers <= ASTK_MAX_RNN_LAYERS && H > 0 && A > 0, "beam_select: bad state dims");
  ASTK_CHECK(logits && alpha && ld_alpha >= b->T && c_new && h_new && ht_new, "beam_select: null pointer or short alpha rows");
  BeamSelArgs a;
  caller_sel_args(a, b, n_layers, H, A, logits, alpha, ld_alpha, c_new, h_new, ht_new, step);
  return beam_select_ctc_launch(b, st, ctc, a, (hipStream_t)stream);
}

int astk_beam_select(const astk_beam_desc* b, int n_layers, int H, int A, const float* logits, const float* alpha, long ld_alpha,
                     const float* c_new, const float* h_new, const float* ht_new, const astk_beam_state* st, int step, void* stream) {
  ASTK_TRY(check_beam(b, st, step));
  ASTK_CHECK(n_layers >= 1 && n_layers <= ASTK_MAX_RNN_LAYERS && H > 0 && A > 0, "beam_select: bad state dims");
  ASTK_CHECK(logits && alpha && ld_alpha >= b->T && c_new && h_new && ht_new, "beam_select: null pointer or short alpha rows");
  BeamSelArgs a;
  caller_sel_args(a, b, n_layers, H, A, logits, alpha, ld_alpha, c_new, h_new, ht_new, step);
  return beam_select_launch(b, st, a, (hipStream_t)stream);
}

}  // extern "C"
