// CTC forced alignment: the best monotonic path of a row's labels through its frames (include/astk.h astk_ctc_align, DESIGN.md section
// 31).  Float32 max-plus recursion over the emissions e[t][s] = logits[t][z_s] - lse[t] of ctc.hip's extended sequence, no atomics on
// anything a result depends on: every output is the same bits from run to run.  logits is only read.
//
// Two launches on the caller's stream (three with n_infeasible):
//   k_ctc_lse     ctc.hip's, through ctc_lse_launch: one wavefront per frame.
//   k_ctc_align   one workgroup per batch row, one thread per state s (ctc_rows.h ctc_row_setup: the labels, the state flags and the
//                 feasibility as k_ctc_rows has them).
//     forward     delta rolled in two LDS buffers, one barrier per step, the emission gathers sixteen steps ahead (ctc_rows.h
//                 ctc_run_ahead, k_ctc_rows' loop); per state a
//                 compare chain (stay, s - 1, s - 2: a later one wins only when strictly greater) and one add, no transcendental.  The
//                 choice, 0 / 1 / 2 states back, goes out as two wavefront ballots (bit 0, bit 1) per wave and step: lane 0 of each
//                 wave stores them as ONE 16-byte vector store, T * blockDim / 64 * 16 bytes per row.
//     backtrace   wave 0 walks t = n - 1 .. 0 over back-pointer chunks of 64 steps that the other waves copy into LDS one chunk
//                 ahead (double-buffered, one barrier per chunk; a single-wave workgroup copies for itself); a lane keeps the state
//                 of its step, so frame_state / frame_class leave as coalesced stores.
//     spans       parallel over t: the first and last frame of every label state (one writer each, frame_state is monotone), then
//                 parallel over u: label_logp = the sum of e over the span, in frame order, the loads eight ahead of the adds.
//   k_ctc_align_finish  one thread: the count of rows without a path.
#include "ctc_rows.h"
#include <math.h>

namespace astk {

namespace {

constexpr int ALIGN_CHUNK = 64;                              // steps of back-pointers per LDS buffer of the backtrace (a lane per step)
constexpr int ALIGN_SUM_PF = 8;                              // emission loads in flight in front of a label's ordered sum

struct CtcAlignWs {
  float* lse;                  // [B][T]
  ulonglong2* bp;              // [B][T][W]   .x = bit 0, .y = bit 1 of the 64 states of a wave: states back (0, 1, 2)
  int* feasible;               // [B]
  int W;                       // wavefronts per row's workgroup
  size_t bytes;
};
static CtcAlignWs align_carve(const astk_ctc_desc* d, void* base) {
  CtcAlignWs w;
  w.W = (2 * d->L + 1 + 63) / 64;
  const size_t bt = (size_t)d->B * d->T;
  CtcBump c(base);
  w.lse = c.take<float>(bt);
  w.bp = c.take<ulonglong2>(bt * w.W);
  w.feasible = c.take<int>((size_t)d->B);
  w.bytes = c.off;
  return w;
}

struct CtcAlignArgs : CtcRowIn {
  int32_t* frame_state;        // (B, T)
  int32_t* frame_class;        // (B, T) or null
  int32_t* label_start;        // (B, L) or null
  int32_t* label_end;          // (B, L) or null
  float* label_logp;           // (B, L) or null
  float* row_score;            // (B)
};

__global__ __launch_bounds__(CTC_ROW_THREADS) void k_ctc_align(CtcAlignArgs a, CtcAlignWs w) {
  __shared__ int ext[CTC_ROW_THREADS];                  // class of state s
  __shared__ float dl[2][CTC_ROW_THREADS + 4];          // the rolled recursion, two guard cells on either side
  __shared__ ulonglong2 bpl[2][ALIGN_CHUNK * (CTC_ROW_THREADS / 64)];
  __shared__ int span[2][ASTK_CTC_MAX_LABELS + 1];      // first frame, one past the last frame of label u
  __shared__ int wcnt[CTC_ROW_THREADS / 64];
  __shared__ int s_rep;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, W = nt >> 6;
  const int Tb = ctc_row_len(a.len, b, a.T);
  const CtcRow r = ctc_row_setup(a, b, Tb, ext, wcnt, &s_rep, &dl[0][0]);
  const int U = r.U, S = r.S;
  const bool act = r.act, skip = r.skip, feasible = r.feasible;
  // (a path through NaN logits may miss a label: an empty span; the spans are written behind the barriers of the recursion)
  for (int i = tid; i < 2 * (ASTK_CTC_MAX_LABELS + 1); i += nt) (&span[0][0])[i] = 0;
  const int nv = feasible ? Tb : 0;                     // frames that carry a path
  int32_t* fs = a.frame_state + (size_t)b * a.T;
  int32_t* fc = a.frame_class ? a.frame_class + (size_t)b * a.T : nullptr;
  // ---- what does not depend on the path: the frames behind it, the labels behind U
  for (int t = nv + tid; t < a.T; t += nt) {
    fs[t] = -1;
    if (fc) fc[t] = a.blank;
  }
  if (tid < a.L && (!feasible || tid >= U)) {
    if (a.label_start) a.label_start[(size_t)b * a.L + tid] = -1;
    if (a.label_end) a.label_end[(size_t)b * a.L + tid] = -1;
    if (a.label_logp) a.label_logp[(size_t)b * a.L + tid] = 0.f;
  }
  if (tid == 0) {
    w.feasible[b] = feasible ? 1 : 0;
    if (!feasible) a.row_score[b] = -INFINITY;
  }
  if (!feasible) return;
  if (tid == 0) dl[0][2] = 0.f;                         // the virtual step in front of t = 0: the path stands in front of state 0
  __syncthreads();
  const float* lg = a.logits + (size_t)b * a.T * a.ldv + r.cls;
  const float* ls = w.lse + (size_t)b * a.T;
  ulonglong2* bp = w.bp + (size_t)b * a.T * W;
  int cur = 0;
  // ---- delta and the back-pointers, t = 0 .. len - 1
  ctc_run_ahead(
      Tb,
      [&](int t, float& x, float& l) {
        l = t < Tb ? ls[t] : 0.f;                         // (the uniform guard first: it stays a scalar branch)
        x = (act && t < Tb) ? lg[(size_t)t * a.ldv] : 0.f;
      },
      [&](int t, float x, float l) {
        int back = 0;
        if (act) {
          const float* p = &dl[cur][2 + tid];
          float best = p[0];
          const float p1 = p[-1], p2 = skip ? p[-2] : -INFINITY;
          if (p1 > best) { best = p1; back = 1; }
          if (p2 > best) { best = p2; back = 2; }
          dl[cur ^ 1][2 + tid] = best + (x - l);
        }
        const unsigned long long b0 = __ballot(back & 1), b1 = __ballot(back >> 1);
        if (lane == 0) bp[(size_t)t * W + wv] = make_ulonglong2(b0, b1);
        __syncthreads();
        cur ^= 1;
      });
  // ---- the final state: the trailing blank, unless the last label is strictly better
  int sF = S - 1;
  if (S >= 2 && dl[cur][2 + S - 2] > dl[cur][2 + S - 1]) sF = S - 2;
  if (tid == 0) a.row_score[b] = dl[cur][2 + sF];
  // ---- backtrace, t = len - 1 .. 0, in chunks of ALIGN_CHUNK steps from the top: chunk c covers t in [lo_c, lo_c + ALIGN_CHUNK) n [0, len)
  const int nchunk = (Tb + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
  const int first_loader = nt > 64 ? 64 : 0, loaders = nt - first_loader;       // wave 0 walks; it copies only when it is alone
  auto stage = [&](int c) {                             // chunk c's back-pointers to bpl[c & 1]; contiguous in the workspace
    const int lo = c * ALIGN_CHUNK, n = (min(Tb, lo + ALIGN_CHUNK) - lo) * W;
    const ulonglong2* src = bp + (size_t)lo * W;
    if (tid >= first_loader)
      for (int i = tid - first_loader; i < n; i += loaders) bpl[c & 1][i] = src[i];
  };
  if (nchunk > 0) stage(nchunk - 1);                    // (behind the last step's barrier: the back-pointer stores are visible to the workgroup)
  __syncthreads();
  int s = sF;                                           // (uniform)
  for (int c = nchunk - 1; c >= 0; --c) {
    if (c > 0 && (wv != 0 || nt == 64)) stage(c - 1);
    if (wv == 0) {
      const int lo = c * ALIGN_CHUNK, hi = min(Tb, lo + ALIGN_CHUNK) - 1;
      int mine = -1;
      for (int t = hi; t >= lo; --t) {
        if (lane == t - lo) mine = s;
        const ulonglong2 q = bpl[c & 1][(t - lo) * W + (s >> 6)];       // (one address: a broadcast read)
        s -= (int)((q.x >> (s & 63)) & 1ull) + 2 * (int)((q.y >> (s & 63)) & 1ull);
      }
      if (lo + lane <= hi) {
        fs[lo + lane] = mine;
        if (fc) fc[lo + lane] = ext[mine];
      }
    }
    __syncthreads();
  }
  // ---- spans of the labels from frame_state (monotone: a label's frames are one run, and every label has one)
  if (!a.label_start && !a.label_end && !a.label_logp) return;
  for (int t = tid; t < Tb; t += nt) {
    const int st = fs[t];
    if (st & 1) {
      if (t == 0 || fs[t - 1] != st) span[0][st >> 1] = t;
      if (t == Tb - 1 || fs[t + 1] != st) span[1][st >> 1] = t + 1;
    }
  }
  __syncthreads();
  if (tid < U) {
    const int t0 = span[0][tid], t1 = span[1][tid];
    if (a.label_start) a.label_start[(size_t)b * a.L + tid] = t0;
    if (a.label_end) a.label_end[(size_t)b * a.L + tid] = t1;
    if (a.label_logp) {
      const float* lu = a.logits + (size_t)b * a.T * a.ldv + ext[2 * tid + 1];
      float acc = 0.f;
      for (int t = t0; t < t1; t += ALIGN_SUM_PF) {
        float x[ALIGN_SUM_PF], l[ALIGN_SUM_PF];
#pragma unroll
        for (int k = 0; k < ALIGN_SUM_PF; ++k) {
          x[k] = t + k < t1 ? lu[(size_t)(t + k) * a.ldv] : 0.f;
          l[k] = t + k < t1 ? ls[t + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < ALIGN_SUM_PF; ++k)
          if (t + k < t1) acc += x[k] - l[k];
      }
      a.label_logp[(size_t)b * a.L + tid] = acc;
    }
  }
}

__global__ void k_ctc_align_finish(int B, const int* __restrict__ feasible, int32_t* n_infeasible) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int bad = 0;
  for (int b = 0; b < B; ++b) bad += feasible[b] ? 0 : 1;
  *n_infeasible = bad;
}

}  // namespace

}  // namespace astk

using namespace astk;

size_t astk_ctc_align_workspace_bytes(const astk_ctc_desc* d) {
  if (ctc_check_desc(d, "ctc_align_workspace_bytes") != 0) return 0;
  return align_carve(d, nullptr).bytes;
}

int astk_ctc_align(const astk_ctc_desc* d, const float* logits, const int32_t* y, const int32_t* input_len, int32_t* frame_state,
                   int32_t* frame_class, int32_t* label_start, int32_t* label_end, float* label_logp, float* row_score,
                   int32_t* n_infeasible, void* ws, size_t ws_bytes, void* stream) {
  ASTK_TRY(ctc_check_desc(d, "ctc_align"));
  const CtcAlignWs w = align_carve(d, ws);
  ASTK_TRY(ctc_check_ptrs("ctc_align", logits && y && frame_state && row_score, "logits, y, frame_state, row_score", ws));
  ASTK_TRY(ctc_check_ws_bytes("ctc_align", "ctc_align", ws_bytes, w.bytes));
  hipStream_t s = (hipStream_t)stream;
  ASTK_TRY(ctc_lse_launch(d, logits, input_len, w.lse, s));
  CtcAlignArgs a;
  ctc_row_in(a, d, logits, y, input_len);
  a.frame_state = frame_state; a.frame_class = frame_class; a.label_start = label_start; a.label_end = label_end;
  a.label_logp = label_logp; a.row_score = row_score;
  hipLaunchKernelGGL(k_ctc_align, dim3(d->B), dim3(w.W * 64), 0, s, a, w);     // one thread per state of the longest row the descriptor admits (<= 512)
  ASTK_LAUNCH_CHECK();
  if (n_infeasible) {
    hipLaunchKernelGGL(k_ctc_align_finish, dim3(1), dim3(64), 0, s, d->B, w.feasible, n_infeasible);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}
