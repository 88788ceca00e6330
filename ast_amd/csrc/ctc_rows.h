// What the per-row CTC kernels share (ctc.hip k_ctc_rows, ctc_align.hip k_ctc_align): a row's clamped length and the compaction of its
// labels into the extended sequence.  Device code in a header, because the library is built without relocatable device code; the host
// side the two translation units share (ctc_check_desc, ctc_lse_launch) is declared here and defined once, in ctc.hip.
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

__device__ __forceinline__ int ctc_row_len(const int32_t* len, int b, int T) { return len ? min(max(len[b], 0), T) : T; }

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

}  // namespace astk
