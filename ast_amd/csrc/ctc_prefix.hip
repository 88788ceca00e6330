// CTC prefix scores for the joint CTC-attention beam search (include/astk.h "joint CTC-attention beam search").
//
// Once per search (ctc_prefix_init_launch):
//   k_ctcp_lse        one wavefront per frame (u, t < T''_u): the float64 log-sum-exp of the head's float32 logits (ctc_rows.h
//                     ctc_wave_lse)
//   k_ctcp_transpose  the logits as (U, V, Tp): a candidate's column x[.][c] becomes contiguous over t (64 x 64 tiles through LDS)
//   k_ctcp_empty      one thread per utterance: the empty prefix's state in slot 0, att_score = psi = 0 and n_labels = 0 in every slot
// Once per step (ctc_prefix_score_launch), for every live row and each of its K proposals:
//   k_ctcp_wave       one workgroup per row, one wavefront per candidate.  phi of the row (both forms: the candidate repeats the last
//                     label or not), r_b and the blank emissions are staged in LDS once for the K candidates.  Both recursions are
//                     first-order linear recurrences in the linear domain, y[t] = p[t] (y[t-1] + f[t-1]): a lane runs its contiguous
//                     slice of frames from -inf and keeps the slice's map y_out = logaddexp(A + y_in, B); the 64 maps are composed by
//                     a wavefront scan in the log domain; a second pass over the slice from the true y_in writes the state.  r_b'
//                     needs the finished r_n', so: pass 1 (r_n' maps, psi terms), scan, pass 2 (r_n' written, r_b' maps), scan,
//                     pass 3 (r_b' written).
//                     The emissions come from the (U, V, Tp) copy; form 2 of the test hook reads them strided from the head's own layout
//                     (the measurement the copy was chosen by: DESIGN.md section 30).
//   k_ctcp_serial     the plain form, one thread per candidate, serial over the frames (test-hook build only: the operator test's
//                     second implementation, and the launch the shipped one is measured against)
// Everything is float64 in the log domain; logaddexp (ctc_rows.h lae) of two dead terms is -inf, never NaN.
#include "ctc_rows.h"

namespace astk {

namespace {

constexpr int ST_LIVE = 1;

__global__ __launch_bounds__(256) void k_ctcp_lse(int U, int T, int V, long ldv, const float* __restrict__ logits,
                                                  const int32_t* __restrict__ row_len, int N, double* __restrict__ lse) {
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= (long)U * T) return;
  const int u = (int)(f / T), t = (int)(f % T), lane = threadIdx.x & 63;
  if (t >= row_len[(long)u * N]) return;
  const double l = ctc_wave_lse<double>(logits + f * ldv, V, lane);
  if (lane == 0) lse[f] = l;
}

// grid (ceil(T / 64), ceil(V / 64), U), 256 threads: tile[t][v] in, [v][t] out; frames behind T''_u are written as 0 and not read
__global__ __launch_bounds__(256) void k_ctcp_transpose(int T, int V, long ldv, long Tp, const float* __restrict__ logits,
                                                        const int32_t* __restrict__ row_len, int N, float* __restrict__ xt) {
  __shared__ float tile[64][65];
  const int u = blockIdx.z, t0 = blockIdx.x * 64, v0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int len = row_len[(long)u * N];
  for (int i = ty; i < 64; i += 4) {
    const int t = t0 + i, v = v0 + tx;
    tile[i][tx] = (t < len && v < V) ? logits[((long)u * T + t) * ldv + v] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int v = v0 + i, t = t0 + tx;
    if (v < V && t < Tp) xt[((long)u * V + v) * Tp + t] = tile[tx][i];
  }
}

struct CtcpArgs {
  int R, N, K, T, V, eos, blank, first_label;
  const double* lse;              // (U, T)
  const float* x; long su, st, sc; // the logit of (u, t, c) is x[u su + t st + c sc]: the (U, V, Tp) copy, or the head's own (U, T, ldv) layout
  const int32_t* row_utt; const int32_t* row_len; const int32_t* status; const int32_t* tokens; const int32_t* n_labels;
  const double* state;            // (R, T, 2)
  const int32_t* cand_tok;        // (R, K)
  double* psi; double* new_state; // (R, K), (R, K, T, 2)
};

__global__ void k_ctcp_empty(int U, int N, int T, int V, int blank, long Tp, const double* __restrict__ lse, const float* __restrict__ xt,
                             const int32_t* __restrict__ row_len, double* __restrict__ state, double* __restrict__ att,
                             double* __restrict__ psi, int32_t* __restrict__ n_labels) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  for (int j = 0; j < N; ++j) {
    att[(long)u * N + j] = 0.0;
    psi[(long)u * N + j] = 0.0;
    n_labels[(long)u * N + j] = 0;
  }
  const int len = row_len[(long)u * N];
  double* st = state + (long)u * N * T * 2;
  const float* xb = xt + ((long)u * V + blank) * Tp;
  double acc = 0.0;
  for (int t = 0; t < len; ++t) {
    acc += (double)xb[t] - lse[(long)u * T + t];
    st[2 * t] = -INFINITY;
    st[2 * t + 1] = acc;
  }
}

// what a candidate is by its id alone: 0 a label, 1 eos, 2 no CTC path (blank, GO, ...)
__device__ __forceinline__ int cand_kind(const CtcpArgs& a, int c) { return c == a.eos ? 1 : (c < a.first_label || c == a.blank) ? 2 : 0; }

__device__ __forceinline__ void scan_maps(double& A, double& B, int lane) {
  // inclusive scan of the maps y -> logaddexp(A + y, B) over the lanes: lane l ends with the composition of lanes 0..l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double Ao = __shfl_up(A, o), Bo = __shfl_up(B, o);
    if (lane >= o) {
      B = lae(A + Bo, B);
      A = Ao + A;
    }
  }
}

__global__ __launch_bounds__(256) void k_ctcp_wave(CtcpArgs a) {
  extern __shared__ double s_dyn[];
  const int r = blockIdx.x;
  if (a.status[r] != ST_LIVE) return;
  const int T = a.T, len = a.row_len[r], u = a.row_utt[r], K = a.K;
  double* s_phi = s_dyn;                 // logaddexp(r_n, r_b)
  double* s_rb = s_dyn + T;
  double* s_xb = s_dyn + 2 * (long)T;
  const double* st = a.state + (long)r * T * 2;
  const double* lse = a.lse + (long)u * T;
  const float* xbp = a.x + u * a.su + a.blank * a.sc;
  const long xs = a.st;
  for (int t = threadIdx.x; t < len; t += blockDim.x) {
    const double rn = st[2 * t], rb = st[2 * t + 1];
    s_phi[t] = lae(rn, rb);
    s_rb[t] = rb;
    s_xb[t] = (double)xbp[t * xs] - lse[t];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = a.n_labels[r];
  const int last = n > 0 ? a.tokens[r] : -1;
  const int m = n > 1 ? n : 1;
  for (int k = wave; k < K; k += 4) {
    const long ck = (long)r * K + k;
    const int c = a.cand_tok[ck];
    double* out = a.new_state + ck * T * 2;
    const int kind = cand_kind(a, c);
    if (kind == 1) {                     // eos: the utterance is exactly g; the slot keeps its parent's state
      if (lane == 0) a.psi[ck] = s_phi[len - 1];
      continue;
    }
    if (kind == 2 || m > len) {          // no path: a dead state
      for (int t = lane; t < len; t += 64) { out[2 * t] = -INFINITY; out[2 * t + 1] = -INFINITY; }
      if (lane == 0) a.psi[ck] = -INFINITY;
      continue;
    }
    const double* phi = c == last ? s_rb : s_phi;
    const float* xcp = a.x + u * a.su + c * a.sc;
    const double rn_init = n == 0 ? (double)xcp[0] - lse[0] : -INFINITY;
    for (int t = lane; t < m; t += 64) { out[2 * t] = t == m - 1 ? rn_init : -INFINITY; out[2 * t + 1] = -INFINITY; }
    const int per = (len - m + 63) / 64;
    const int t0 = min(len, m + lane * per), t1 = min(len, t0 + per);
    // pass 1: the slice's r_n' map from -inf, and its psi terms
    double A = 0.0, B = -INFINITY, P = -INFINITY;
    for (int t = t0; t < t1; ++t) {
      const double e = (double)xcp[t * xs] - lse[t], f = phi[t - 1];
      B = lae(B, f) + e;
      A += e;
      P = lae(P, f + e);
    }
    scan_maps(A, B, lane);
    double rn_in = __shfl_up(lae(A + rn_init, B), 1);
    if (lane == 0) rn_in = rn_init;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) P = lae(P, __shfl_xor(P, o));
    if (lane == 0) a.psi[ck] = lae(rn_init, P);
    // pass 2: r_n' from the true incoming value; the slice's r_b' map (its f[t-1] is r_n'[t-1])
    double v = rn_in;
    A = 0.0; B = -INFINITY;
    for (int t = t0; t < t1; ++t) {
      const double prev = v;
      v = lae(v, phi[t - 1]) + ((double)xcp[t * xs] - lse[t]);
      out[2 * t] = v;
      const double eb = s_xb[t];
      B = lae(B, prev) + eb;
      A += eb;
    }
    scan_maps(A, B, lane);
    double rb_in = __shfl_up(B, 1);      // (the value in front of frame m is -inf: the map's A term is dead)
    if (lane == 0) rb_in = -INFINITY;
    // pass 3: r_b'
    double w = rb_in, prev = rn_in;
    for (int t = t0; t < t1; ++t) {
      w = lae(prev, w) + s_xb[t];
      out[2 * t + 1] = w;
      prev = out[2 * t];
    }
  }
}

#ifdef ASTK_TEST_HOOKS
__global__ __launch_bounds__(64) void k_ctcp_serial(CtcpArgs a) {
  const long ck = (long)blockIdx.x * 64 + threadIdx.x;
  if (ck >= (long)a.R * a.K) return;
  const int r = (int)(ck / a.K);
  if (a.status[r] != ST_LIVE) return;
  const int T = a.T, len = a.row_len[r], u = a.row_utt[r];
  const double* st = a.state + (long)r * T * 2;
  const double* lse = a.lse + (long)u * T;
  const float* xbp = a.x + u * a.su + a.blank * a.sc;
  const long xs = a.st;
  const int n = a.n_labels[r];
  const int last = n > 0 ? a.tokens[r] : -1;
  const int m = n > 1 ? n : 1;
  const int c = a.cand_tok[ck];
  double* out = a.new_state + ck * T * 2;
  const int kind = cand_kind(a, c);
  if (kind == 1) {
    a.psi[ck] = lae(st[2 * (len - 1)], st[2 * (len - 1) + 1]);
    return;
  }
  if (kind == 2 || m > len) {
    for (int t = 0; t < len; ++t) { out[2 * t] = -INFINITY; out[2 * t + 1] = -INFINITY; }
    a.psi[ck] = -INFINITY;
    return;
  }
  const float* xcp = a.x + u * a.su + c * a.sc;
  double rn = n == 0 ? (double)xcp[0] - lse[0] : -INFINITY, rb = -INFINITY;
  for (int t = 0; t < m; ++t) { out[2 * t] = t == m - 1 ? rn : -INFINITY; out[2 * t + 1] = -INFINITY; }
  double psi = rn;
  for (int t = m; t < len; ++t) {
    const double f = c == last ? st[2 * (t - 1) + 1] : lae(st[2 * (t - 1)], st[2 * (t - 1) + 1]);
    const double e = (double)xcp[t * xs] - lse[t];
    const double rn_new = lae(rn, f) + e;
    rb = lae(rn, rb) + ((double)xbp[t * xs] - lse[t]);
    rn = rn_new;
    psi = lae(psi, f + e);
    out[2 * t] = rn;
    out[2 * t + 1] = rb;
  }
  a.psi[ck] = psi;
}
#endif

}  // namespace

size_t ctc_prefix_ws_carve(void* base, int U, int N, int K, int T, int V, CtcPrefixWs& w) {
  Carver c(base);
  const size_t R = (size_t)U * N;
  w.Tp = (T + 3) / 4 * 4;
  w.lse = c.take<double>((size_t)U * T);
  w.xt = c.take<float>((size_t)U * V * w.Tp);
  w.cand_tok = c.take<int32_t>(R * K);
  w.cand_lp = c.take<double>(R * K);
  w.cand_psi = c.take<double>(R * K);
  w.cand_state = c.take<double>(R * K * T * 2);
  return c.total();
}

int ctc_prefix_check(const astk_beam_desc* b, const astk_beam_ctc* c) {
  ASTK_CHECK_DESC(c, astk_beam_ctc);
  ASTK_CHECK(c->weight > 0.0 && c->weight <= 1.0, "beam_ctc: weight %g outside (0, 1]", c->weight);
  ASTK_CHECK(c->blank >= 0 && c->blank < b->V && c->first_label > c->blank && c->first_label < b->V,
             "beam_ctc: blank %d / first_label %d outside the vocabulary V = %d or not in order", c->blank, c->first_label, b->V);
  ASTK_CHECK(b->eos != c->blank && b->eos < c->first_label, "beam_ctc: eos %d must lie below first_label %d and differ from the blank", b->eos,
             c->first_label);
  ASTK_CHECK(c->ldv >= b->V, "beam_ctc: ldv %ld < V = %d", c->ldv, b->V);
  ASTK_CHECK(b->T <= ASTK_BEAM_CTC_MAX_T, "beam_ctc: T = %d above the limit of %d frames (the row's phi is staged in LDS)", b->T,
             ASTK_BEAM_CTC_MAX_T);
  ASTK_CHECK(c->logits && c->state && c->att_score && c->psi && c->n_labels && c->ws, "beam_ctc: null buffer");
  CtcPrefixWs w;
  const size_t need = ctc_prefix_ws_carve(nullptr, b->U, b->N, b->K, b->T, b->V, w);
  ASTK_CHECK(c->ws_bytes >= need, "beam_ctc: workspace too small (%zu < %zu bytes)", c->ws_bytes, need);
  ASTK_CHECK(((uintptr_t)c->ws & 255) == 0, "beam_ctc: workspace not 256-byte aligned");
  return 0;
}

int ctc_prefix_init_launch(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* c, hipStream_t s) {
  CtcPrefixWs w;
  ctc_prefix_ws_carve(c->ws, b->U, b->N, b->K, b->T, b->V, w);
  const long frames = (long)b->U * b->T;
  hipLaunchKernelGGL(k_ctcp_lse, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, b->U, b->T, b->V, c->ldv, c->logits, st->row_len, b->N,
                     w.lse);
  ASTK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ctcp_transpose, dim3((b->T + 63) / 64, (b->V + 63) / 64, b->U), dim3(256), 0, s, b->T, b->V, c->ldv, w.Tp, c->logits,
                     st->row_len, b->N, w.xt);
  ASTK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ctcp_empty, dim3((b->U + 63) / 64), dim3(64), 0, s, b->U, b->N, b->T, b->V, c->blank, w.Tp, w.lse, w.xt, st->row_len,
                     c->state, c->att_score, c->psi, c->n_labels);
  ASTK_LAUNCH_CHECK();
  return 0;
}

int ctc_prefix_score_launch(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* c, const int32_t* cand_tok,
                            double* psi, double* new_state, int form, hipStream_t s) {
  CtcPrefixWs w;
  ctc_prefix_ws_carve(c->ws, b->U, b->N, b->K, b->T, b->V, w);
  CtcpArgs a;
  a.R = b->U * b->N; a.N = b->N; a.K = b->K; a.T = b->T; a.V = b->V; a.eos = b->eos; a.blank = c->blank; a.first_label = c->first_label;
  a.lse = w.lse;
  if (form == 2) { a.x = c->logits; a.su = (long)b->T * c->ldv; a.st = c->ldv; a.sc = 1; }
  else { a.x = w.xt; a.su = (long)b->V * w.Tp; a.st = 1; a.sc = w.Tp; }
  a.row_utt = st->row_utt; a.row_len = st->row_len; a.status = st->status; a.tokens = st->tokens; a.n_labels = c->n_labels;
  a.state = c->state; a.cand_tok = cand_tok; a.psi = psi; a.new_state = new_state;
  if (form == 1) {
#ifdef ASTK_TEST_HOOKS
    hipLaunchKernelGGL(k_ctcp_serial, dim3((unsigned)(((long)a.R * a.K + 63) / 64)), dim3(64), 0, s, a);
#else
    ASTK_CHECK(false, "ctc_prefix: the serial kernel exists in the test-hook build only");
#endif
  } else {
    hipLaunchKernelGGL(k_ctcp_wave, dim3(a.R), dim3(256), (size_t)3 * a.T * sizeof(double), s, a);
  }
  ASTK_LAUNCH_CHECK();
  return 0;
}

}  // namespace astk

#ifdef ASTK_TEST_HOOKS
extern "C" int astk_debug_ctc_prefix(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* ctc, const int32_t* cand_tok,
                                     int form, double* psi, double* new_state, void* stream) {
  using namespace astk;
  ASTK_CHECK_DESC(b, astk_beam_desc);
  ASTK_CHECK_DESC(st, astk_beam_state);
  ASTK_CHECK(b->U > 0 && b->N >= 1 && b->K >= 1 && b->T > 0 && b->V > 1, "debug_ctc_prefix: bad dims");
  ASTK_TRY(ctc_prefix_check(b, ctc));
  ASTK_CHECK(cand_tok && psi && new_state && form >= 0 && form <= 2, "debug_ctc_prefix: null pointer or form %d", form);
  return ctc_prefix_score_launch(b, st, ctc, cand_tok, psi, new_state, form, (hipStream_t)stream);
}
#endif
