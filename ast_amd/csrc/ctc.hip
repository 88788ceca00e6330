// CTC loss on the encoder states (joint CTC-attention training; include/astk.h astk_ctc_loss).  Float32, log
// domain, no floating-point atomics: row_nll, loss_acc and dlogits are the same bits from run to run.
//
// Four launches on the caller's stream:
//   k_ctc_lse     one wavefront per frame (b, t): lse[b][t] = log sum_v exp(logits[b][t][v]), maximum subtracted (ctc_rows.h
//                 ctc_wave_lse).  Coalesced over V.
//   k_ctc_rows    one workgroup per batch row, one thread per state s of the extended sequence (S' = 2U + 1 <= 511, blanks at the even
//                 positions).  The workgroup compacts the row's labels from y into LDS (ctc_rows.h ctc_row_setup: ballot prefix sums, no
//                 launch of its own), runs the alpha recursion over t with alpha rolled in two LDS buffers (one barrier per step) and
//                 stored to the workspace, T * S' floats per row, next to the emissions e[t][s] = logits[t][class(s)] - lse[t] it
//                 gathered (once: the beta pass reads them back).  The gathers do not depend on the recursion and are issued sixteen
//                 steps ahead (ctc_rows.h ctc_run_ahead, the loop of both passes).  Then beta is rolled in LDS from t = len - 1 down,
//                 and the occupancy gamma[t][s] = exp(alpha + beta - e - log p) overwrites alpha[t][s].
//   k_ctc_grad    one workgroup per frame, the V-wide coalesced pass: dlogits = scale * softmax, then scale * occupancy of every class
//                 that has states is subtracted by ONE writer per class in a fixed order: the blank's states by a fixed-shape tree (two
//                 per thread, xor tree per wave, the four waves in order), a label's states by the class's first state, which walks the
//                 chain of its later occurrences in index order.
//   k_ctc_finish  one thread: loss_acc += scale * nll of the feasible rows, in row order; the count of infeasible rows.
// A dead state (alpha or beta = -inf) is the normal case at the sequence ends: the three-way log-add returns -inf for three -inf terms
// instead of forming -inf - -inf.
#include "ctc_rows.h"
#include <math.h>

namespace astk {

namespace {

constexpr int CTC_META = 4;                                  // ints per row: U, feasible, len, unused

// the workspace, carved from the descriptor alone
struct CtcWs {
  float* lse;        // [B][T]
  float* alpha;      // [B][T][Smax]   alpha, then the occupancies
  float* em;         // [B][T][Smax]   emissions
  int* own;          // [B][Smax]      class a state owns (the first state of a label class), else -1
  int* nxt;          // [B][Smax]      next state of the same class, else -1
  int* meta;         // [B][CTC_META]
  int Smax;
  size_t bytes;
};
static CtcWs ctc_carve(const astk_ctc_desc* d, void* base) {
  CtcWs w;
  w.Smax = 2 * d->L + 1;
  const size_t bt = (size_t)d->B * d->T;
  CtcBump c(base);
  w.lse = c.take<float>(bt);
  w.alpha = c.take<float>(bt * w.Smax);
  w.em = c.take<float>(bt * w.Smax);
  w.own = c.take<int>((size_t)d->B * w.Smax);
  w.nxt = c.take<int>((size_t)d->B * w.Smax);
  w.meta = c.take<int>((size_t)d->B * CTC_META);
  w.bytes = c.off;
  return w;
}

// log(exp(a) + exp(b) + exp(c)); -inf when all three are
__device__ __forceinline__ float logadd3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

__global__ __launch_bounds__(256) void k_ctc_lse(int B, int T, int V, long ldv, const float* __restrict__ logits, const int32_t* __restrict__ len,
                                                 float* __restrict__ lse) {
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= (long)B * T) return;
  const int b = (int)(f / T), t = (int)(f - (long)b * T);
  if (t >= ctc_row_len(len, b, T)) return;
  const float l = ctc_wave_lse<float>(logits + f * ldv, V, lane);
  if (lane == 0) lse[f] = l;
}

struct CtcRowArgs : CtcRowIn {
  float* row_nll;
};

__global__ __launch_bounds__(CTC_ROW_THREADS) void k_ctc_rows(CtcRowArgs a, CtcWs w) {
  __shared__ int ext[CTC_ROW_THREADS];                  // class of state s
  __shared__ float ab[2][CTC_ROW_THREADS + 4];          // the rolled recursion, two guard cells on either side
  __shared__ int wcnt[CTC_ROW_THREADS / 64];
  __shared__ int s_rep;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = ctc_row_len(a.len, b, a.T);
  const int Smax = w.Smax;
  const CtcRow r = ctc_row_setup(a, b, Tb, ext, wcnt, &s_rep, &ab[0][0]);
  const int U = r.U, S = r.S, cls = r.cls;
  const bool act = r.act, odd = r.odd, skip_f = r.skip, feasible = r.feasible;
  const bool skip_b = odd && tid + 2 < S && ext[tid + 2] != cls;    // the transition s -> s + 2
  if (tid < Smax) {
    // the class chains k_ctc_grad walks: a label's first state owns the class
    int own = -1, nx = -1;
    if (odd) {
      own = cls;
      for (int j = 1; j < tid; j += 2) if (ext[j] == cls) { own = -1; break; }
      for (int j = tid + 2; j < S; j += 2) if (ext[j] == cls) { nx = j; break; }
    }
    w.own[(size_t)b * Smax + tid] = own;
    w.nxt[(size_t)b * Smax + tid] = nx;
  }
  if (tid == 0) {
    w.meta[b * CTC_META + 0] = U;
    w.meta[b * CTC_META + 1] = feasible ? 1 : 0;
    w.meta[b * CTC_META + 2] = Tb;
    if (!feasible) a.row_nll[b] = INFINITY;
  }
  if (!feasible) return;
  if (tid == 0) ab[0][2] = 0.f;                         // the virtual step in front of t = 0: all mass in front of state 0
  __syncthreads();
  const float* lg = a.logits + (size_t)b * a.T * a.ldv + cls;
  const float* ls = w.lse + (size_t)b * a.T;
  float* al = w.alpha + (size_t)b * a.T * Smax + tid;
  float* em = w.em + (size_t)b * a.T * Smax + tid;
  int cur = 0;
  // ---- alpha, t = 0 .. len - 1
  ctc_run_ahead(
      Tb,
      [&](int t, float& x, float& l) {
        l = t < Tb ? ls[t] : 0.f;                         // (the uniform guard first: it stays a scalar branch)
        x = (act && t < Tb) ? lg[(size_t)t * a.ldv] : 0.f;
      },
      [&](int t, float x, float l) {
        if (act) {
          const float* p = &ab[cur][2 + tid];
          const float e = x - l;
          const float v = logadd3(p[0], p[-1], skip_f ? p[-2] : -INFINITY) + e;
          ab[cur ^ 1][2 + tid] = v;
          al[(size_t)t * Smax] = v;
          em[(size_t)t * Smax] = e;
        }
        __syncthreads();
        cur ^= 1;
      });
  const float ll = logadd3(ab[cur][2 + S - 1], S >= 2 ? ab[cur][2 + S - 2] : -INFINITY, -INFINITY);
  if (tid == 0) a.row_nll[b] = -ll;
  __syncthreads();
  // ---- beta, t = len - 1 .. 0, and the occupancies in place of alpha
  if (act) { ab[0][2 + tid] = -INFINITY; ab[1][2 + tid] = -INFINITY; }
  __syncthreads();
  if (tid == 0) ab[0][2 + S - 1] = 0.f;                 // the virtual step behind t = len - 1
  __syncthreads();
  cur = 0;
  ctc_run_ahead(
      Tb,
      [&](int i, float& alpha, float& e) {
        const int t = Tb - 1 - i;
        alpha = (act && t >= 0) ? al[(size_t)t * Smax] : 0.f;
        e = (act && t >= 0) ? em[(size_t)t * Smax] : 0.f;
      },
      [&](int i, float alpha, float e) {
        const int t = Tb - 1 - i;
        if (act) {
          const float* p = &ab[cur][2 + tid];
          const float v = logadd3(p[0], p[1], skip_b ? p[2] : -INFINITY) + e;
          ab[cur ^ 1][2 + tid] = v;
          al[(size_t)t * Smax] = (alpha == -INFINITY || v == -INFINITY) ? 0.f : expf(alpha + v - e - ll);
        }
        __syncthreads();
        cur ^= 1;
      });
}

__global__ __launch_bounds__(256) void k_ctc_grad(int T, int V, long ldv, int blank, float scale, const float* logits, float* dlogits, CtcWs w) {
  __shared__ float part[4];
  const long f = blockIdx.x;
  const int b = (int)(f / T), t = (int)(f - (long)b * T), tid = threadIdx.x;
  const int* meta = w.meta + b * CTC_META;
  float* g = dlogits + f * ldv;
  if (!meta[1] || t >= meta[2]) {                       // an infeasible row, or a frame behind the row's length
    for (int v = tid; v < ldv; v += 256) g[v] = 0.f;
    return;
  }
  const float* x = logits + f * ldv;                    // (may be g: every element is read by the thread that then writes it)
  const float lse = w.lse[f];
  for (int v = tid; v < ldv; v += 256) g[v] = v < V ? scale * expf(x[v] - lse) : 0.f;
  const int S = 2 * meta[0] + 1;
  const float* gam = w.alpha + (size_t)f * w.Smax;
  float pb = 0.f;
  for (int s = 2 * tid; s < S; s += 512) pb += gam[s];
  pb = wave_sum(pb);
  if ((tid & 63) == 0) part[tid >> 6] = pb;
  __syncthreads();                                      // (also: the stores above are visible to the class owners below)
  const int* own = w.own + (size_t)b * w.Smax;
  const int* nxt = w.nxt + (size_t)b * w.Smax;
  for (int s = 2 * tid + 1; s < S; s += 512) {
    const int c = own[s];
    if (c < 0) continue;
    float o = gam[s];
    for (int j = nxt[s]; j >= 0; j = nxt[j]) o += gam[j];
    g[c] -= scale * o;
  }
  if (tid == 0) g[blank] -= scale * (((part[0] + part[1]) + part[2]) + part[3]);
}

__global__ void k_ctc_finish(int B, float scale, const float* __restrict__ row_nll, const int* __restrict__ meta, float* loss_acc,
                             int32_t* n_infeasible) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float acc = 0.f;
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    if (meta[b * CTC_META + 1]) acc += scale * row_nll[b];
    else ++bad;
  }
  if (loss_acc) *loss_acc += acc;
  if (n_infeasible) *n_infeasible = bad;
}

// per-frame argmax class over the valid frames (ties: the lowest index), the blank behind a row's length; one wavefront per frame
__global__ __launch_bounds__(256) void k_ctc_greedy(int B, int T, int V, long ldv, int blank, const float* __restrict__ logits,
                                                    const int32_t* __restrict__ len, int32_t* __restrict__ best) {
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= (long)B * T) return;
  const int b = (int)(f / T), t = (int)(f - (long)b * T);
  if (t >= ctc_row_len(len, b, T)) {
    if (lane == 0) best[f] = blank;
    return;
  }
  const float* x = logits + f * ldv;
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float xv = x[v];
    if (xv > m || mi == 0x7fffffff) { m = xv; mi = v; }       // (v ascends per lane: a later equal value does not replace)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oi = __shfl_xor(mi, o);
    if (oi != 0x7fffffff && (mi == 0x7fffffff || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
  }
  if (lane == 0) best[f] = mi == 0x7fffffff ? blank : mi;
}

}  // namespace

int ctc_check_desc(const astk_ctc_desc* d, const char* who) {
  ASTK_CHECK_DESC(d, astk_ctc_desc);
  ASTK_CHECK(d->B > 0 && d->T > 0, "%s: B and T must be positive, got B = %d, T = %d", who, d->B, d->T);
  ASTK_CHECK(d->V >= 2, "%s: V must be at least 2 (a blank and a label), got %d", who, d->V);
  ASTK_CHECK(d->ldv >= d->V, "%s: ldv = %ld is below V = %d", who, d->ldv, d->V);
  ASTK_CHECK(d->L > 0 && d->ldy >= d->L, "%s: L must be positive and ldy >= L, got L = %d, ldy = %ld", who, d->L, d->ldy);
  ASTK_CHECK(d->L <= ASTK_CTC_MAX_LABELS, "%s: a row of L = %d targets may hold more than the %d labels a row is limited to (astk.h)", who,
             d->L, ASTK_CTC_MAX_LABELS);
  ASTK_CHECK(d->blank >= 0 && d->blank < d->V, "%s: blank = %d lies outside [0, V = %d)", who, d->blank, d->V);
  ASTK_CHECK(d->first_label > d->blank, "%s: first_label = %d must lie above blank = %d (the blank is no label)", who, d->first_label, d->blank);
  ASTK_CHECK((size_t)d->B * d->T <= 0x7fffffffu / 4, "%s: B * T = %zu frames do not fit the launch grid", who, (size_t)d->B * d->T);
  return 0;
}

int ctc_lse_launch(const astk_ctc_desc* d, const float* logits, const int32_t* input_len, float* lse, hipStream_t s) {
  const unsigned frames = (unsigned)((size_t)d->B * d->T);
  hipLaunchKernelGGL(k_ctc_lse, dim3((frames + 3) / 4), dim3(256), 0, s, d->B, d->T, d->V, d->ldv, logits, input_len, lse);
  ASTK_LAUNCH_CHECK();
  return 0;
}

}  // namespace astk

using namespace astk;

size_t astk_ctc_workspace_bytes(const astk_ctc_desc* d) {
  if (ctc_check_desc(d, "ctc_workspace_bytes") != 0) return 0;
  return ctc_carve(d, nullptr).bytes;
}

int astk_ctc_loss(const astk_ctc_desc* d, const float* logits, const int32_t* y, const int32_t* input_len, float scale, float* row_nll,
                  float* loss_acc, float* dlogits, int32_t* n_infeasible, void* ws, size_t ws_bytes, void* stream) {
  ASTK_TRY(ctc_check_desc(d, "ctc_loss"));
  const CtcWs w = ctc_carve(d, ws);
  ASTK_TRY(ctc_check_ptrs("ctc_loss", logits && y && row_nll && dlogits, "logits, y, row_nll, dlogits", ws));
  ASTK_CHECK(scale == scale && fabsf(scale) <= 3.4e38f, "ctc_loss: scale must be finite, got %g", (double)scale);
  ASTK_TRY(ctc_check_ws_bytes("ctc_loss", "ctc", ws_bytes, w.bytes));
  hipStream_t s = (hipStream_t)stream;
  const unsigned frames = (unsigned)((size_t)d->B * d->T);
  ASTK_TRY(ctc_lse_launch(d, logits, input_len, w.lse, s));
  CtcRowArgs a;
  ctc_row_in(a, d, logits, y, input_len);
  a.row_nll = row_nll;
  const int nt = (w.Smax + 63) / 64 * 64;               // one thread per state of the longest row the descriptor admits (<= 512)
  hipLaunchKernelGGL(k_ctc_rows, dim3(d->B), dim3(nt), 0, s, a, w);
  ASTK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ctc_grad, dim3(frames), dim3(256), 0, s, d->T, d->V, d->ldv, d->blank, scale, logits, dlogits, w);
  ASTK_LAUNCH_CHECK();
  if (loss_acc || n_infeasible) {
    hipLaunchKernelGGL(k_ctc_finish, dim3(1), dim3(64), 0, s, d->B, scale, row_nll, w.meta, loss_acc, n_infeasible);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

int astk_ctc_greedy(const astk_ctc_desc* d, const float* logits, const int32_t* input_len, int32_t* best, void* stream) {
  ASTK_TRY(ctc_check_desc(d, "ctc_greedy"));
  ASTK_CHECK(logits && best, "ctc_greedy: logits and best must not be null");
  const unsigned frames = (unsigned)((size_t)d->B * d->T);
  hipLaunchKernelGGL(k_ctc_greedy, dim3((frames + 3) / 4), dim3(256), 0, (hipStream_t)stream, d->B, d->T, d->V, d->ldv, d->blank, logits,
                     input_len, best);
  ASTK_LAUNCH_CHECK();
  return 0;
}

int astk_ctc_head_fwd(int rows, int V, int H, const float* enc, const float* W, const float* b, float* logits, long ldv, int precision,
                      void* stream) {
  ASTK_CHECK(rows > 0 && V > 0 && H > 0 && ldv >= V, "ctc_head_fwd: bad dimensions (rows = %d, V = %d, H = %d, ldv = %ld)", rows, V, H, ldv);
  ASTK_CHECK(enc && W && logits, "ctc_head_fwd: null pointer");
  ASTK_CHECK(precision >= ASTK_PREC_DEFAULT && precision <= ASTK_PREC_F32, "ctc_head_fwd: precision must be 0 (default), 1 (fp16x2), 2 (bf16x3) or 3 (f32): the enum of astk.h");
  PrecScope ps(precision, ASTK_OPERANDS_DEFAULT);
  DetScope ds(0);
  GemmForwardScope fs;
  return gemm_launch(GEMM_NT, gemm_args(rows, V, H, mat(enc, H), mat(W, H), logits, ldv, b), (hipStream_t)stream);
}

int astk_ctc_head_bwd(int rows, int V, int H, const float* dlogits, long ldv, const float* W, const float* enc, float* d_enc, float* dW,
                      float* db, int precision, int deterministic, void* stream) {
  ASTK_CHECK(rows > 0 && V > 0 && H > 0 && ldv >= V, "ctc_head_bwd: bad dimensions (rows = %d, V = %d, H = %d, ldv = %ld)", rows, V, H, ldv);
  ASTK_CHECK(dlogits && W && enc && d_enc && dW && db, "ctc_head_bwd: null pointer");
  ASTK_CHECK(precision >= ASTK_PREC_DEFAULT && precision <= ASTK_PREC_F32, "ctc_head_bwd: precision must be 0 (default), 1 (fp16x2), 2 (bf16x3) or 3 (f32): the enum of astk.h");
  PrecScope ps(precision, ASTK_OPERANDS_DEFAULT);
  DetScope ds(deterministic);
  hipStream_t s = (hipStream_t)stream;
  ASTK_TRY(gemm_launch(GEMM_NN, gemm_args(rows, H, V, mat(dlogits, ldv), mat(W, H), d_enc, H, nullptr, GEMM_ACCUM), s));
  ASTK_TRY(gemm_launch(GEMM_TN, gemm_args(V, H, rows, mat(dlogits, ldv), mat(enc, H), dW, H, nullptr, GEMM_ACCUM), s));
  return colsum_add_f32(db, dlogits, ldv, rows, V, s);
}
