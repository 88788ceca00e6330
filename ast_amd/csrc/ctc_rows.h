// What the CTC family shares (ctc.hip loss and greedy decode, ctc_prefix.hip prefix scores, ctc_align.hip forced alignment, ctc_beam.hip
// prefix beam search), each piece written once: the wavefront log-sum-exp of a frame, the float64 logaddexp, a row's clamped length,
// the row kernels' setup (label compaction, state flags, feasibility) and their run-ahead step loop; on the host the 16-byte bump
// allocator of the workspaces, the row kernels' descriptor-derived arguments and the workspace refusals.  Device code in a header,
// because the library is built without relocatable device code; the host side the translation units share (ctc_check_desc,
// ctc_lse_launch) is declared here and defined once, in ctc.hip.
#pragma once
#include "common.h"

namespace astk {

constexpr int CTC_ROW_THREADS = 512;                         // one thread per state of the longest row ASTK_CTC_MAX_LABELS admits (S' <= 511)
constexpr int CTC_PF = 16;                                   // steps the emission gathers run ahead of the recursion (a memory latency is several steps long)

// the refusals of every entry point that takes an astk_ctc_desc; `who` names the caller in the message
int ctc_check_desc(const astk_ctc_desc* d, const char* who);
// lse[b][t] = log sum_v exp(logits[b][t][v]), maximum subtracted, for t < input_len[b] (one wavefront per frame; frames behind a row's
// length are not written)
int ctc_lse_launch(const astk_ctc_desc* d, const float* logits, const int32_t* input_len, float* lse, hipStream_t s);

// The workspace refusals of an entry point `who`, in two parts, since astk_ctc_loss refuses its scale between them: the pointers
// (`ptrs` says that those `names` lists are all set) and the alignment, then the size against what astk_<query>_workspace_bytes gave.
static inline int ctc_check_ptrs(const char* who, bool ptrs, const char* names, const void* ws) {
  ASTK_CHECK(ptrs && ws, "%s: %s and ws must not be null", who, names);
  ASTK_CHECK(aligned16(ws), "%s: the workspace must be 16-byte aligned", who);
  return 0;
}
static inline int ctc_check_ws_bytes(const char* who, const char* query, size_t ws_bytes, size_t need) {
  ASTK_CHECK(ws_bytes >= need, "%s: workspace of %zu bytes, astk_%s_workspace_bytes asks for %zu", who, ws_bytes, query, need);
  return 0;
}

// Bump allocator of the family's workspaces: slices rounded up to 16 bytes (common.h's Carver rounds to 256, and the sizes are public
// through the astk_*_workspace_bytes queries).  A null base only counts.
struct CtcBump {
  char* base;
  size_t off;
  explicit CtcBump(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(size_t n) {
    const size_t o = off;
    off += (n * sizeof(T) + 15) & ~(size_t)15;
    return (T*)(base + o);
  }
};

// what a row kernel's arguments take from the descriptor and the call (k_ctc_rows and k_ctc_align append their outputs)
struct CtcRowIn {
  int T, V, L, first_label, blank;
  long ldv, ldy;
  const float* logits;
  const int32_t* y;
  const int32_t* len;
};
static inline void ctc_row_in(CtcRowIn& a, const astk_ctc_desc* d, const float* logits, const int32_t* y, const int32_t* input_len) {
  a.T = d->T; a.V = d->V; a.L = d->L; a.first_label = d->first_label; a.blank = d->blank;
  a.ldv = d->ldv; a.ldy = d->ldy;
  a.logits = logits; a.y = y; a.len = input_len;
}

__device__ __forceinline__ int ctc_row_len(const int32_t* len, int b, int T) { return len ? min(max(len[b], 0), T) : T; }

// log(exp(a) + exp(b)) in float64, symmetric in its arguments; -inf for two -inf terms, never NaN
__device__ __forceinline__ double lae(double a, double b) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1p(exp(fmin(a, b) - m));
}

// log sum_v exp(x[v]) over x[0 .. V) by one wavefront, accumulated in A (float or double), the same value in every lane: the strided
// maximum, an xor butterfly, the strided sum of exp(x - maximum), a butterfly.  fmax / exp / log resolve by the type of A: fmaxf, expf
// and logf for float.
template <typename A>
__device__ __forceinline__ A ctc_wave_lse(const float* __restrict__ x, int V, int lane) {
  A m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmax(m, (A)x[v]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  A s = 0;
  for (int v = lane; v < V; v += 64) s += exp((A)x[v] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return m + log(s);
}

// The row's labels: the entries of y_row[0 .. L) with id >= first_label, in order (ids >= V read as V - 1), to the odd positions of
// ext[0 .. blockDim.x), the blank everywhere else.  Ballot prefix sums, no launch of its own.  Returns U.  Called by every thread of
// the workgroup (L <= blockDim.x, a multiple of 64, at most CTC_ROW_THREADS); holds two barriers, the second behind the last write of ext.
__device__ __forceinline__ int ctc_compact_labels(const int32_t* y_row, int L, int first_label, int V, int blank, int* ext, int* wcnt) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6;
  int id = -1;
  if (tid < L) id = y_row[tid];
  const bool keep = id >= first_label;
  const unsigned long long km = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(km);
  ext[tid] = blank;
  __syncthreads();
  int before = 0, U = 0;
  for (int i = 0; i < nt / 64; ++i) { before += i < wv ? wcnt[i] : 0; U += wcnt[i]; }
  if (keep) ext[2 * (before + __popcll(km & ((1ull << lane) - 1ull))) + 1] = min(id, V - 1);
  __syncthreads();
  return U;
}

// A thread's view of its row: state s = threadIdx.x of the extended sequence (S = 2U + 1 states, blanks at the even positions).
struct CtcRow {
  int U, S;
  int cls;                     // class of the state (the blank behind S)
  bool act, odd;               // s < S; a label state
  bool skip;                   // the transition s - 2 -> s exists
  bool feasible;               // the row's frames hold its labels and a blank between adjacent repeats
};

// The setup of a row kernel, called by every thread of row b's workgroup with the kernel's own LDS: ext and wcnt as
// ctc_compact_labels takes them, s_rep one int, roll the two rolled buffers of the recursion (2 * (CTC_ROW_THREADS + 4) floats, left
// at -inf).  Holds three barriers: the compaction's two, and one behind the count of adjacent repeats and the fill of roll.
__device__ __forceinline__ CtcRow ctc_row_setup(const CtcRowIn& a, int b, int Tb, int* ext, int* wcnt, int* s_rep, float* roll) {
  const int tid = threadIdx.x, nt = blockDim.x;
  CtcRow r;
  if (tid == 0) *s_rep = 0;
  r.U = ctc_compact_labels(a.y + (long)b * a.ldy, a.L, a.first_label, a.V, a.blank, ext, wcnt);
  r.S = 2 * r.U + 1;
  r.act = tid < r.S;
  r.cls = r.act ? ext[tid] : a.blank;
  r.odd = r.act && (tid & 1);
  r.skip = r.odd && tid >= 3 && ext[tid - 2] != r.cls;
  const unsigned long long rm = __ballot(r.odd && tid >= 3 && ext[tid - 2] == r.cls);
  if ((tid & 63) == 0 && rm) atomicAdd(s_rep, __popcll(rm));          // (an integer count: order-free)
  for (int i = tid; i < 2 * (CTC_ROW_THREADS + 4); i += nt) roll[i] = -INFINITY;
  __syncthreads();
  r.feasible = Tb >= r.U + *s_rep;
  return r;
}

// The step loop of a row kernel: step(i, q0, q1) for i = 0 .. n - 1 in order, where load(i, q0, q1) fetched the step's two values
// CTC_PF steps earlier (the loads do not depend on the recursion; load returns zeros for i >= n).  step holds the step's barrier.
// The callables are inlined at every call, whatever the inliner's cost model says.
template <typename Load, typename Step>
__device__ __forceinline__ void ctc_run_ahead(int n, Load load, Step step) {
  float q0[CTC_PF], q1[CTC_PF];
#pragma unroll
  for (int k = 0; k < CTC_PF; ++k) [[clang::always_inline]] load(k, q0[k], q1[k]);
  for (int i0 = 0; i0 < n; i0 += CTC_PF) {
    float c0[CTC_PF], c1[CTC_PF];
#pragma unroll
    for (int k = 0; k < CTC_PF; ++k) { c0[k] = q0[k]; c1[k] = q1[k]; }
    // The block's values are in registers HERE, in front of the next loads: the block's one wait on memory.  Left to itself the
    // compiler may drop the copies, and a step that then meets its value first behind the newer loads waits for those too, and for
    // the store of the step before it.  No no-op: astk_ctc_align at B 32, T 200, V 1098, L 40 on an MI355X took 86.3 us without
    // this line, 71.3 us with it, 72.9 us with the loop written out in the kernel.
#pragma unroll
    for (int k = 0; k < CTC_PF; ++k) asm volatile("" : "+v"(c0[k]), "+v"(c1[k]));
#pragma unroll
    for (int k = 0; k < CTC_PF; ++k) [[clang::always_inline]] load(i0 + CTC_PF + k, q0[k], q1[k]);
#pragma unroll
    for (int k = 0; k < CTC_PF; ++k)
      if (i0 + k < n) [[clang::always_inline]] step(i0 + k, c0[k], c1[k]);       // (uniform)
  }
}

}  // namespace astk
