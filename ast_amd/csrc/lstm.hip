// Encoder LSTM stacks (seq2seq.py:182-242): n_dirs independent stacks of L.LSTM links.
//
// Three kernel paths; lstm_route chooses one per call, and every function below serves one of them:
//   persistent (h in 64..512): the layer-0 upward projection of both directions as ONE grouped MFMA GEMM over all time steps (rows in
//              loop-step order; the reverse direction reads frames through the Q1 permutation table 0,T-1,...,1 instead of a permuted
//              copy), then the whole stack -- or one group of layers after the other, where the cells exceed one workgroup per CU -- in
//              ONE launch of the wavefront kernel (lstm_persist.hip).  Backward: one launch per group, top group first, then the batched
//              products for dWl, dWu and the gradient wrt the frames; the bias gradients come from the recurrence kernel.
//   hoisted    (h = 1024): every layer a launch of its own over cells that read their input projection from a batched product in
//              front of it (forward) and leave the gradient for the layer below to a batched product behind it (backward).
//   per-step   (every other h, or "lstm.persist" / "lstm.hoist" 0): per layer one batched GEMM per direction for the upward projection,
//              then T launches of the fused cell kernel (both directions in one launch: lateral product on f32 MFMA + interleaved-gate
//              epilogue, activated gates overwrite ZG in place, dropped output written straight into the (B,T,H) enc_states slice for
//              the top layer -- no concat growth, no flipud copy).  Backward, per layer, top down: T launches of the fused backward cell
//              (dh_rec = dz_{t+1} Wl via the transposed weight, gate derivatives, dz overwrites the gates in place), then that layer's
//              batched GEMMs for dWl, dWu, db and the gradient wrt the layer input, which the layer below reads.
// Beside the persistent recurrences (astk_lstm_stack_desc.side_stream): the tail of the layer-0 projection in time chunks behind flags
// (plan_side_fwd), and the gradient wrt the frames in chunks behind the backward's progress counter (plan_side_bwd).  A SideJoin orders
// the caller's stream behind the side stream on every exit.  Everything is graph-capturable, no host sync.
// HBM layout (per direction d, layer l, all f32, step-major):
//   ZG (T,B,4h) gates -> dz | HR (T,B,h) raw h | CC (T,B,h) cell | HD (T,B,h) dropped output (only with masks)
#include "lstm_persist.h"
#include <algorithm>
#include <vector>

namespace astk {

namespace {

constexpr int SIDE_CHUNKS_MAX = 60;

// ---- the route: which kernel path a call takes and how the persistent launches are shaped.  Filled once per call (under the caller's
// PrecScope: the 512-thread form is bf16x3's) and read by the queries, the plans, the forward and the backward, so that the two passes
// cannot disagree about the grouping of the layers or the rows of the counters.  The knobs are read in here, so at every call.
enum LstmPath { LSTM_PER_STEP = 0, LSTM_PERSIST = 1, LSTM_HOISTED = 2 };      // what astk_lstm_stack_path returns
struct LstmRoute {
  LstmPath path;
  int rows;        // form of the recurrence workgroups (lstm_persist.h: LSTM_ROWS_16, _MT2 or _DUO); 16 on the hoisted path
  int xs;          // arithmetic of the recurrence kernels of that form (lstm_persist.h: LSTM_XS_*), what astk_lstm_stack_form reports
  int lpl;         // layers per launch: groups start at multiples of it (<= n_layers; 1 on the hoisted path)
  int wgs_first;   // workgroups of the first launch: what the side-stream plans leave to the recurrence
  int wg_rows;     // (virtual) workgroup rows of a cell: rows of the counters, arrivals per unit slice, rows of the db sums
};
LstmRoute lstm_route(const astk_lstm_stack_desc* d) {
  LstmRoute R = {LSTM_PER_STEP, LSTM_ROWS_16, lstm_persist_xs(d->h, LSTM_ROWS_16), 0, 0, lstm_persist_wg_rows(d->B, LSTM_ROWS_16)};
  if (!lstm_persist_applicable(d->T, d->B, d->h, d->n_layers, d->n_dirs)) return R;
  R.path = lstm_persist_hoisted(d->h) ? LSTM_HOISTED : LSTM_PERSIST;
  R.rows = lstm_persist_rows(d->B, d->h, d->n_layers, d->n_dirs, d->side_stream != nullptr);
  R.xs = lstm_persist_xs(d->h, R.rows);
  R.lpl = lstm_persist_layers_per_launch(d->B, d->h, d->n_layers, d->n_dirs, R.rows);
  R.wgs_first = lstm_persist_grid_wgs(d->B, d->h, R.lpl, d->n_dirs, R.rows);
  R.wg_rows = lstm_persist_wg_rows(d->B, R.rows);
  return R;
}

// ---- work beside the recurrences (astk_lstm_stack_desc.side_stream): the plan of the forward pass.
// The layer-0 input projection (per direction (T B) x 4h x in, the largest product of the step) is cut along time: steps [0, s0) are
// multiplied in line, at full width, in front of the recurrence launch; the rest in chunks of `cs` steps on the side stream, every launch
// capped at `cap` workgroups (the CUs the recurrence grid leaves free), a one-lane kernel behind each chunk raising its flag.  A chunk holds as
// many 128-row tile rows as give `cap` tiles over all directions, so a chunk launch is ONE WHOLE TILE PER WORKGROUP: plain stores, no split
// tiles, the same sum order in every run.  s0 is the smallest head for which, by a rate model (a tile pass ~ 0.66 us per 16 k + 15 us; a
// recurrence step 2.9 / 4.4 us at 16 / 32 rows per workgroup, 3.8 at h = 512), no chunk is late; if the model is wrong the layer-0 cells wait
// on a flag (bounded like every other hand-off) -- slower, never wrong.  n = 0: everything in line.
struct SidePlan { int s0, cs, n, cap; };
SidePlan plan_side_fwd(const astk_lstm_stack_desc* d, const LstmRoute& R) {
  SidePlan sp = {d->T, 0, 0, 0};
  if (R.path != LSTM_PERSIST || !d->side_stream || !tune_on(TUNE_LSTM_SIDE_FWD) || d->deterministic || tune_on(TUNE_GEMM_DETERMINISTIC)) return sp;
  int cap = device_cu_count() - R.wgs_first;
  if (d->side_wgs > 0) cap = std::min(cap, d->side_wgs);
  cap = cap / 8 * 8;
  const int tiles_per_row = d->n_dirs * ((4 * d->h + 127) / 128);       // 128 x 128 tiles per 128 rows of all directions
  const int tile_rows = cap / tiles_per_row;
  if (cap < 16 || tile_rows < 1) return sp;
  int cs = (int)tune(TUNE_LSTM_OVERLAP_CHUNK);
  if (cs <= 0) cs = tile_rows * 128 / d->B;
  if (cs < 4 || d->T < 3 * cs / 2) return sp;
  const double t_chunk = ((d->in_dim + 15) / 16) * 0.66 + 15.0;           // one tile pass (every workgroup of a chunk launch does one)
  const double r_step = (d->h > 256 ? 3.8 : R.rows == LSTM_ROWS_MT2 ? 4.4 : R.rows == LSTM_ROWS_DUO ? 3.3 : 2.9) * 0.9; // (10 % margin)
  // (the side stream starts together with the in-line head, so the chunks have the head's time -- ~190 TFLOP/s on the whole chip -- on top)
  const double head_step = 0.8 * d->n_dirs * 2.0 * d->B * 4.0 * d->h * d->in_dim / 190e6;
  for (int n = std::min(SIDE_CHUNKS_MAX, (d->T - 2) / cs); n >= 1; --n) {
    const int s0 = d->T - n * cs;
    bool ok = s0 >= 2;
    for (int k = 0; k < n && ok; ++k) ok = (k + 1) * t_chunk <= s0 * head_step + (s0 + (double)k * cs) * r_step;
    if (ok) { sp.s0 = s0; sp.cs = cs; sp.n = n; sp.cap = cap; return sp; }
  }
  return sp;
}
__global__ void k_set_flag(unsigned* f) {
  if (threadIdx.x == 0) __hip_atomic_store(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ---- the backward pass beside its recurrence.  The layer-0 cells write dz through and arrive on a progress counter per direction once per
// chunk of `cs` loop steps (lstm_persist_bwd_rs, PCellB::prog); on the side stream a one-wave kernel waits for a chunk's arrivals -- bounded
// spin with s_sleep; a time-out sets the encoder-backward bit of the sticky status word, so the step is reported, and exits, so nothing
// hangs -- and the input-gradient products of that chunk follow it in stream order (a kernel boundary behind the wait: their loads see
// the written-through dz).  Every launch is capped at the CUs the recurrence grid leaves free.
__global__ void k_wait_progress(const unsigned* p0, const unsigned* p1, unsigned target, AbortCtl ab) {
  if (threadIdx.x != 0) return;
  unsigned spins = 0;
  while (__hip_atomic_load(p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target ||
         (p1 && __hip_atomic_load(p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target)) {
    __builtin_amdgcn_s_sleep(32);
    if (++spins > ab.limit) { abort_raise(ab); return; }
    if ((spins & 63u) == 0 && abort_seen(ab)) return;
  }
}
// deterministic calls: db[cell][c] += sum over the workgroup rows, in order, of the sums the persistent backward kernel left per row
struct FoldDbJobs { int n, nby, cols; float* db[16]; const float* part[16]; };
__global__ void k_fold_db(FoldDbJobs j) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (c >= j.cols || q >= j.n) return;
  float sum = 0.f;
  for (int by = 0; by < j.nby; ++by) sum += j.part[q][(long)by * j.cols + c];
  j.db[q][c] += sum;
}
__global__ void k_zero_words(unsigned* p, int n, int stride) {
  if ((int)threadIdx.x < n) __hip_atomic_store(p + threadIdx.x * stride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
SidePlan plan_side_bwd(const astk_lstm_stack_desc* d, const LstmRoute& R, bool want_dx) {
  SidePlan sp = {d->T, 0, 0, 0};
  // (one launch over the whole stack only: its grid is R.wgs_first)
  if (R.path != LSTM_PERSIST || !d->side_stream || !want_dx || R.lpl < d->n_layers || low_precision_gemms() || !tune_on(TUNE_LSTM_SIDE_BWD) || deterministic_mode()) return sp;
  int cap = device_cu_count() - R.wgs_first;
  if (d->side_wgs > 0) cap = std::min(cap, d->side_wgs);
  cap = cap / 8 * 8;
  if (cap < 16) return sp;
  int cs = (int)tune(TUNE_LSTM_OVERLAP_CHUNK);
  // (as many 128-row tile rows of ONE direction's product as give at most `cap` tiles: one whole tile per workgroup, no split tiles)
  if (cs <= 0) cs = std::max(4, std::max(1, cap / ((d->in_dim + 127) / 128)) * 128 / d->B);
  cs = std::max(4, cs);
  const int nall = std::min(SIDE_CHUNKS_MAX, (d->T + cs - 1) / cs);
  if (nall < 2) return sp;
  // "lstm.side_bwd" = how many chunks (the LAST loop steps, which the backward passes first) go to the side stream; the rest of dx follows in
  // line, at full width, behind the recurrence.  (< 0: every chunk.)  The side stream is the caller's: what else it has queued there --
  // the decoder's parameter gradients in the train step -- decides how many chunks finish inside the recurrence's duration.
  const int want = (int)tune(TUNE_LSTM_SIDE_BWD);
  sp.cs = cs; sp.n = want < 0 ? nall : std::min(want, nall); sp.cap = cap; sp.s0 = 0;
  return sp;
}

// ---- fork and join of the side stream.  fork() lets the side stream loose behind the caller's and arms the guard; join() is the explicit
// join of a success path (the caller sees one-stream semantics) and disarms it.  A return in between -- every ASTK_TRY / ASTK_CHECK /
// ASTK_LAUNCH_CHECK that fails behind the fork -- leaves through the destructor, which issues the same join: what is queued on the side
// stream still writes ZG / dx and the workspace, and the caller, who may retry, is ordered behind it.  The backward passes the wait
// kernels' abort word along: the guard raises it from the caller's stream first (k_set_flag, behind the launch that zeroed it), so a
// k_wait_progress whose recurrence was never launched leaves at its next look at the word (every 64 polls) and not at the spin bound.
// Failures of the guard's own calls are dropped: the call is returning an error already.
struct SideJoin {
  hipStream_t s = nullptr, side = nullptr;
  unsigned* abort_word = nullptr;
  bool armed = false;
  int fork(hipStream_t s_, hipStream_t side_, unsigned* abort_word_ = nullptr) {
    ASTK_TRY(stream_order(s_, side_));
    s = s_; side = side_; abort_word = abort_word_; armed = true;
    return 0;
  }
  int join() { armed = false; return stream_order(side, s); }
  ~SideJoin() {
    if (!armed) return;
    if (abort_word) { hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(64), 0, s, abort_word); (void)hipGetLastError(); }
    (void)stream_order(side, s);
  }
};

struct LstmPlan {
  int T, B, in, h, nl, nd;
  int* perm;      // [T] frame consumed at loop step i by direction 1: (T-i)%T
  int* inv;       // [T] loop step of direction 1 that consumed frame f
  float* ZG[2][ASTK_MAX_RNN_LAYERS];
  float* HR[2][ASTK_MAX_RNN_LAYERS];
  float* CC[2][ASTK_MAX_RNN_LAYERS];
  float* HD[2][ASTK_MAX_RNN_LAYERS];
  float* WlT[2][ASTK_MAX_RNN_LAYERS];  // (h, 4h) transposed lateral weights (per-step backward)
  unsigned* counters;                  // arrival counters of the persistent kernels
  unsigned* zflags;                    // side-stream chunks: forward [SIDE_CHUNKS_MAX + 2] chunk flags, then 2 progress counters of the backward and the wait kernels' abort word (one word per 256-byte line)
  float* PR[2][ASTK_MAX_RNN_LAYERS];   // persistent backward (reduce-scatter): partial dh_rec ring of each cell
  float* PD[2][ASTK_MAX_RNN_LAYERS];   // partial dx handed to the layer below (layers >= 1)
  unsigned long long* ax;              // the frames' maximum, folded from desc.x_amax into one line by the forward call (read by both calls)
  float* GATH;                         // (T,B,4h) dz of the reverse stack's layer 0 re-ordered to frame order
  float* DX[2];                        // (T,B,h) gradient wrt a layer's input (layers >= 1)
  float* DC[2][2];                     // dc ping-pong (B,h)
  float* DBP[2][ASTK_MAX_RNN_LAYERS];  // deterministic calls: [workgroup rows][4h] bias-gradient sums of the persistent backward kernel
  int* rows_perm;                      // [T*B] perm expanded to row indices: rows[i*B+b] = perm[i]*B + b
  int* rows_inv;                       // [T*B] the same of inv
  size_t bytes;
};

// Validates the descriptor, routes the call (under the caller's PrecScope) and carves the workspace (ws null: sizes only).
int make_plan(const astk_lstm_stack_desc* d, void* ws, LstmRoute& R, LstmPlan& P) {
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  ASTK_CHECK(d && d->T > 0 && d->B > 0 && d->in_dim > 0 && d->h > 0, "lstm_stack: bad dims");
  ASTK_CHECK(d->n_layers >= 1 && d->n_layers <= ASTK_MAX_RNN_LAYERS && (d->n_dirs == 1 || d->n_dirs == 2), "lstm_stack: layers/dirs");
  ASTK_CHECK((d->in_dim % 4) == 0 && (d->h % 4) == 0, "lstm_stack: in_dim and h must be multiples of 4");
  R = lstm_route(d);
  P.T = d->T; P.B = d->B; P.in = d->in_dim; P.h = d->h; P.nl = d->n_layers; P.nd = d->n_dirs;
  Carver c(ws);
  const size_t tb = (size_t)P.T * P.B;
  // what is sized by the workgroup rows holds an EVEN number of 16-row tiles, whatever form a call takes: the 512-thread form's count
  const size_t wg_rows_max = (size_t)lstm_persist_wg_rows(P.B, LSTM_ROWS_DUO);
  P.perm = c.take<int>(P.T);
  P.inv = c.take<int>(P.T);
  for (int dd = 0; dd < P.nd; ++dd) {
    for (int l = 0; l < P.nl; ++l) {
      P.ZG[dd][l] = c.take<float>(tb * 4 * P.h);
      P.HR[dd][l] = c.take<float>(tb * P.h);
      P.CC[dd][l] = c.take<float>(tb * P.h);
      // the workspace size must not depend on whether masks are passed: always reserve HD
      P.HD[dd][l] = c.take<float>(tb * P.h);
      P.WlT[dd][l] = c.take<float>((size_t)P.h * 4 * P.h);
      c.take<float>((size_t)P.h * 4 * P.h);      // (unused: once the transposed upward weights; the layout is kept)
    }
    P.DX[dd] = c.take<float>(tb * P.h);
    P.DC[dd][0] = c.take<float>((size_t)P.B * P.h);
    P.DC[dd][1] = c.take<float>((size_t)P.B * P.h);
  }
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) P.DBP[dd][l] = c.take<float>(wg_rows_max * 4 * P.h);
  P.GATH = c.take<float>(P.nd > 1 ? tb * 4 * P.h : 4);
  P.ax = c.take<unsigned long long>(AMAX_SLOT_WORDS);
  P.counters = c.take<unsigned>(((size_t)2 * P.nd * P.nl * wg_rows_max + 2) * 64);
  P.zflags = c.take<unsigned>((size_t)(SIDE_CHUNKS_MAX + 2 + 3) * 64);      // chunk flags (+ 2 zero words), two progress counters, the wait kernels' abort word
  const bool pp = R.path != LSTM_PER_STEP, hoist = R.path == LSTM_HOISTED;
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) {
      // (hoisted form: the layers run one launch after the other, every cell of a direction uses the ring of layer 0; no down partials)
      P.PR[dd][l] = (hoist && l > 0) ? P.PR[dd][0] : c.take<float>(pp ? lstm_persist_pr_floats(P.B, P.h) : 4);
      P.PD[dd][l] = c.take<float>(pp && l > 0 && !hoist ? lstm_persist_pd_floats(P.T, P.B, P.h) : 4);
    }
  P.rows_perm = c.take<int>(tb);
  P.rows_inv = c.take<int>(tb);
  P.bytes = c.total();
  return 0;
}

// quirk Q1: the reverse stack reads frame X[-i] = (T - i) % T at step i -- an involution, so the frame permutation is its own inverse.
// One launch writes it (perm = inv) and its expansions to (T*B) row indices: rows[i*B+b] = perm[i]*B + b.
__global__ void k_perm_rows(int* perm, int* inv, int* rows_perm, int* rows_inv, int T, int B, const unsigned long long* fold_src,
                            unsigned long long* fold_dst, unsigned* zflags, int nzf) {
  // (rides along: the frames' maximum arrives in a STRIDED producer slot -- thousands of blocks wrote it -- and the GEMMs read one line)
  if (fold_src && blockIdx.x == 0 && threadIdx.x < 64) amax_compact(fold_src, fold_dst);
  // (rides along: the chunk flags of the side-stream plan go down before the side stream is let loose)
  if (zflags && blockIdx.x == 0 && (int)threadIdx.x < nzf) __hip_atomic_store(zflags + threadIdx.x * 64, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T) {
    const int f = (T - i) % T;
    perm[i] = f;
    inv[f] = i;
  }
  if (i < T * B) {
    const int r = ((T - i / B) % T) * B + (i % B);
    rows_perm[i] = r;
    rows_inv[i] = r;
  }
}
// dst[r][:] = src[idx[r]][:]  (float4 columns)
__global__ void k_gather_rows(float* __restrict__ dst, const float* __restrict__ src, const int* __restrict__ idx, int rows, int cols4) {
  const long n = (long)rows * cols4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols4), c = (int)(i % cols4);
    reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[(long)idx[r] * cols4 + c];
  }
}

// ---- per-row lengths (astk_lstm_stack_fwd_rows).  Row b holds n = row_len[b] frames (host-checked: 1..T).
// k_perm_rows per row: loop step i < n of direction 1 reads frame (n - i) % n of its own row -- the lone utterance's permutation; a step
// i >= n reads frame i (in range; both directions are causal in loop-step order, so no step < n sees it).  Only the forward table.
__global__ void k_perm_rows_len(int* rows_perm, int T, int B, const int* __restrict__ row_len, const unsigned long long* fold_src,
                                unsigned long long* fold_dst, unsigned* zflags, int nzf) {
  if (fold_src && blockIdx.x == 0 && threadIdx.x < 64) amax_compact(fold_src, fold_dst);
  if (zflags && blockIdx.x == 0 && (int)threadIdx.x < nzf) __hip_atomic_store(zflags + threadIdx.x * 64, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T * B) {
    const int st = i / B, b = i % B, n = row_len[b];
    rows_perm[i] = (st < n ? (n - st) % n : st) * B + b;
  }
}
// enc_states[b][p][dd * h + :] = the top layer's h of loop step (dd == 0 ? p : n - 1 - p) for p < n, zero behind  (float4 columns)
struct RowsTop { const float* HR[2]; };
__global__ void k_rows_place_enc(float* __restrict__ enc, RowsTop top, const int* __restrict__ row_len, int T, int B, int h, int nd) {
  const int h4 = h / 4;
  const long total = (long)B * T * nd * h4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % h4), dd = (int)(i / h4 % nd), p = (int)(i / ((long)h4 * nd) % T), b = (int)(i / ((long)h4 * nd * T));
    const int n = row_len[b];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < n) v = reinterpret_cast<const float4*>(top.HR[dd] + ((long)(dd == 0 ? p : n - 1 - p) * B + b) * h)[c];
    reinterpret_cast<float4*>(enc)[i] = v;      // ((b * T + p) * nd + dd) * h4 + c: the (B,T,nd*h) layout
  }
}
// cT / hT [cell][b][:] = the cell's CC / HR at loop step row_len[b] - 1
struct RowsCells { int n; const float* CC[16]; const float* HR[16]; };
__global__ void k_rows_final_states(float* __restrict__ cT, float* __restrict__ hT, RowsCells cells, const int* __restrict__ row_len, int B, int h) {
  const int h4 = h / 4;
  const long total = (long)cells.n * B * h4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % h4), b = (int)(i / h4 % B), q = (int)(i / ((long)h4 * B));
    const long src = ((long)(row_len[b] - 1) * B + b) * h4 + c;
    if (cT) reinterpret_cast<float4*>(cT)[i] = reinterpret_cast<const float4*>(cells.CC[q])[src];
    if (hT) reinterpret_cast<float4*>(hT)[i] = reinterpret_cast<const float4*>(cells.HR[q])[src];
  }
}

// ---- what the functions of one call share
struct LstmCall {
  const astk_lstm_stack_desc* d;
  const astk_lstm_params* prm;
  const float *x, *masks;
  LstmRoute R;
  LstmPlan P;
  hipStream_t s;
  SideJoin join;
};
struct LstmFwdCall : LstmCall {
  float *enc_states, *cT, *hT;
  SidePlan side;
  const int* row_len;                  // astk_lstm_stack_fwd_rows: the rows' lengths (device), else null
};
struct LstmBwdCall : LstmCall {
  const astk_lstm_grads* gr;
  const float *d_enc, *d_cT, *d_hT;
  float* dx;
  hipStream_t sr;                      // the recurrence kernels' stream (astk_lstm_stack_bwd_on), else s
  SidePlan bside;
  std::vector<char> touched;           // side chunks of dx: the frames some product has written (bwd_dx_steps)
  unsigned long long* dz_amax[16];     // persistent paths: max |dz| of every cell, left by the recurrence kernel (else null)
  unsigned dz_amax_gen;
  // the batched products (bwd_products_*)
  const unsigned long long *ax, *aw0[2], *ahb;
  GemmArgs wg[GEMM_GROUP_MAX];         // weight-gradient products, issued as grouped launches
  int nwg;
  ColsumBatch cb;                      // per-step path: bias gradients of all cells in one launch
};

// a strided producer slot (bit 0 of the handle) is folded into the plan's plain slot by the forward call; a plain one is used as it is
bool x_amax_strided(const astk_lstm_stack_desc* d) { return d->x_amax && (((uintptr_t)d->x_amax) & 1u); }
// Maxima (fp16x2 GEMM scales) of the frames -- both directions multiply the same ones -- and, if wanted, of the two layer-0 upward weights
// in ONE launch: the products that read them then need no maximum pass of their own.  (The frames' maximum comes with them when the
// caller passes it on from the kernel that wrote them: desc.x_amax.)
void layer0_amax(const LstmCall& c, bool weights, const unsigned long long*& ax, const unsigned long long* aw0[2]) {
  const LstmPlan& P = c.P;
  ax = x_amax_strided(c.d) ? P.ax : (const unsigned long long*)c.d->x_amax;
  AmaxMatrix am[3] = {{ax ? nullptr : c.x, (long)P.T * P.B, (long)P.in, P.in}, {weights ? c.prm[0].Wu : nullptr, 4L * P.h, (long)P.in, P.in},
                      {weights && P.nd > 1 ? c.prm[P.nl].Wu : nullptr, 4L * P.h, (long)P.in, P.in}};
  const unsigned long long* out[3];
  gemm_amax_many(am, 3, out, c.s);
  if (!ax) ax = out[0];
  aw0[0] = out[1]; aw0[1] = out[2];
}

// ---- forward
// the cells of the persistent launches, [direction][layer] (lstm_persist.h)
int persist_fwd_cells(const LstmFwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const size_t bh = (size_t)P.B * P.h;
  memset(cells, 0, 16 * sizeof(PersistCellHost));
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) {
      const astk_lstm_params& p = c.prm[dd * P.nl + l];
      ASTK_CHECK(p.Wu && p.b && p.Wl, "lstm_stack_fwd: null parameter (dir %d layer %d)", dd, l);
      PersistCellHost& q = cells[dd * P.nl + l];
      const bool top = l == P.nl - 1;
      q.Wl = p.Wl;
      q.Wu = l > 0 ? p.Wu : nullptr;
      q.bias = l > 0 ? p.b : nullptr;
      q.zx = l == 0 ? P.ZG[dd][0] : nullptr;
      q.gates = P.ZG[dd][l];
      q.C = P.CC[dd][l];
      q.HR = P.HR[dd][l];
      q.HD = (!top && c.masks) ? P.HD[dd][l] : nullptr;
      q.xin = l > 0 ? (c.masks ? P.HD[dd][l - 1] : P.HR[dd][l - 1]) : nullptr;
      q.mask = c.masks ? c.masks + ((size_t)dd * P.nl + l) * P.T * bh : nullptr;
      q.enc = top ? c.enc_states + (size_t)dd * P.h : nullptr;
      q.reverse_pos = dd == 1;
      q.layer = l;
    }
  return 0;
}

// The layer-0 upward projections of both directions (K9): one grouped launch in line, or -- with a side plan -- time-chunked: the head in
// line, the rest on the side stream beside the recurrence (plan_side_fwd), a flag behind every chunk for the layer-0 cells.  Rows are
// loop-step major in both directions (direction 1 reads its frames through the permutation table), so a chunk is a row range of both products.
int fwd_project_layer0(LstmFwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const SidePlan& side = c.side;
  const int T = P.T, B = P.B, h = P.h;
  const unsigned long long *ax, *aw0[2];
  layer0_amax(c, true, ax, aw0);
  GemmArgs k9[2];
  for (int dd = 0; dd < P.nd; ++dd) {
    const astk_lstm_params& p0 = c.prm[dd * P.nl];
    MatView A = dd == 0 ? mat(c.x, P.in) : mat_idx(c.x, P.in, P.rows_perm);
    k9[dd] = with_amax_b(with_amax_a(lowp(gemm_args(T * B, 4 * h, P.in, A, mat(p0.Wu, P.in), P.ZG[dd][0], 4 * h, p0.b)), ax), aw0[dd]);
  }
  if (side.n == 0) return gemm_launch_group(GEMM_NT, k9, P.nd, c.s);
  auto rows_of = [&](int s_begin, int s_end, GemmArgs* out) {
    for (int dd = 0; dd < P.nd; ++dd) {
      GemmArgs g = k9[dd];
      const size_t r0 = (size_t)s_begin * B;
      g.M = (s_end - s_begin) * B;
      if (dd == 0) g.A.p = c.x + r0 * P.in; else { g.A.rowidx = P.rows_perm + r0; g.A.idx_rows = (long)T * B; }
      g.C = P.ZG[dd][0] + r0 * 4 * h;
      out[dd] = g;
    }
  };
  hipStream_t sside = (hipStream_t)c.d->side_stream;
  GemmArgs part[2];
  ASTK_TRY(c.join.fork(c.s, sside));                   // the frames, the index table, the lowered flags
  rows_of(0, side.s0, part);
  ASTK_TRY(gemm_launch_group(GEMM_NT, part, P.nd, c.s));
  GemmWgCap cap_scope(side.cap);
  for (int k = 0; k < side.n; ++k) {
    rows_of(side.s0 + k * side.cs, std::min(T, side.s0 + (k + 1) * side.cs), part);
    ASTK_TRY(gemm_launch_group(GEMM_NT, part, P.nd, sside));
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(64), 0, sside, P.zflags + (size_t)k * 64);
    ASTK_LAUNCH_CHECK();
  }
  for (int dd = 0; dd < P.nd; ++dd) {
    cells[dd * P.nl].zx_flags = P.zflags; cells[dd * P.nl].zx_s0 = side.s0; cells[dd * P.nl].zx_cs = side.cs;
  }
  return 0;
}

// hoisted form: every layer a launch of its own over "layer-0 like" cells -- the input projection of all time steps comes from a
// batched product in front of the launch (written into the gates buffer, where the cell replaces it step by step)
int fwd_hoisted_launches(const LstmFwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h;
  for (int l = 0; l < P.nl; ++l) {
    PersistCellHost grp[16];
    GemmArgs up[2];
    for (int dd = 0; dd < P.nd; ++dd) {
      PersistCellHost& q = cells[dd * P.nl + l];
      if (l > 0) up[dd] = gemm_args(T * B, 4 * h, h, mat(q.xin, h), mat(q.Wu, h), P.ZG[dd][l], 4 * h, q.bias);
      q.Wu = nullptr; q.bias = nullptr; q.xin = nullptr;
      q.zx = P.ZG[dd][l];
      grp[dd] = q;
    }
    if (l > 0) ASTK_TRY(gemm_launch_group(GEMM_NT, up, P.nd, c.s));
    ASTK_TRY(lstm_persist_fwd_launch(grp, P.nd, 1, T, B, h, P.nd * h, P.counters, c.R.rows, c.s));
  }
  return 0;
}

// one launch per group of layers (normally a single group: the whole stack); a later group finds the outputs of the layer below
// complete (its sentinel polls succeed at once).  The side stream's chunks are consumed by the first group: joined behind the last.
int fwd_grouped_launches(LstmFwdCall& c, const PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const int lpl = c.R.lpl;
  for (int l0 = 0; l0 < P.nl; l0 += lpl) {
    const int ngl = std::min(lpl, P.nl - l0);
    PersistCellHost grp[16];
    for (int dd = 0; dd < P.nd; ++dd)
      for (int l = 0; l < ngl; ++l) grp[dd * ngl + l] = cells[dd * P.nl + l0 + l];
    ASTK_TRY(lstm_persist_fwd_launch(grp, P.nd * ngl, ngl, P.T, P.B, P.h, P.nd * P.h, P.counters, c.R.rows, c.s));
  }
  if (c.side.n > 0) ASTK_TRY(c.join.join());      // join: the caller sees one-stream semantics
  return 0;
}

// final states of every cell: one launch
int fwd_final_states(const LstmFwdCall& c) {
  const LstmPlan& P = c.P;
  const size_t bh = (size_t)P.B * P.h;
  CopySegs cp;
  cp.n = 0;
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) {
      if (cp.n + 2 > FILL_SEG_MAX) { ASTK_TRY(copy_segments(cp, c.s)); cp.n = 0; }
      if (c.cT) copy_seg_add(cp, c.cT + ((size_t)dd * P.nl + l) * bh, P.CC[dd][l] + (size_t)(P.T - 1) * bh, bh * sizeof(float));
      if (c.hT) copy_seg_add(cp, c.hT + ((size_t)dd * P.nl + l) * bh, P.HR[dd][l] + (size_t)(P.T - 1) * bh, bh * sizeof(float));
    }
  return copy_segments(cp, c.s);
}

// calls with row lengths: the recurrences have left every step's h and c in the workspace (and, in enc_states, the batch's placement, which
// is overwritten here); one launch places both halves of enc_states per row, one gathers every cell's states at the row's last step
int fwd_rows_outputs(const LstmFwdCall& c) {
  const LstmPlan& P = c.P;
  RowsTop top = {{P.HR[0][P.nl - 1], P.nd > 1 ? P.HR[1][P.nl - 1] : nullptr}};
  hipLaunchKernelGGL(k_rows_place_enc, dim3(std::min(2048, cdiv(P.B * P.T * P.nd * (P.h / 4), 256))), dim3(256), 0, c.s, c.enc_states, top, c.row_len, P.T, P.B, P.h, P.nd);
  ASTK_LAUNCH_CHECK();
  if (!c.cT && !c.hT) return 0;
  RowsCells cells;
  cells.n = P.nd * P.nl;
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) { cells.CC[dd * P.nl + l] = P.CC[dd][l]; cells.HR[dd * P.nl + l] = P.HR[dd][l]; }
  hipLaunchKernelGGL(k_rows_final_states, dim3(std::min(2048, cdiv(cells.n * P.B * (P.h / 4), 256))), dim3(256), 0, c.s, c.cT, c.hT, cells, c.row_len, P.B, P.h);
  ASTK_LAUNCH_CHECK();
  return 0;
}

// persistent and hoisted paths: layer-0 upward projection batched over time, then the recurrence launches
int fwd_persist(LstmFwdCall& c) {
  PersistCellHost cells[16];
  ASTK_TRY(persist_fwd_cells(c, cells));
  ASTK_TRY(fwd_project_layer0(c, cells));
  ASTK_TRY(c.R.path == LSTM_HOISTED ? fwd_hoisted_launches(c, cells) : fwd_grouped_launches(c, cells));
  return c.row_len ? fwd_rows_outputs(c) : fwd_final_states(c);
}

// per-step path: per layer the upward projection of each direction, T cell launches, the final states
int fwd_steps(const LstmFwdCall& c) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h, H = P.nd * P.h;
  const size_t bh = (size_t)B * h;
  const float* masks = c.masks;
  for (int l = 0; l < P.nl; ++l) {
    const int in = l == 0 ? P.in : h;
    for (int dd = 0; dd < P.nd; ++dd) {
      const astk_lstm_params& p = c.prm[dd * P.nl + l];
      ASTK_CHECK(p.Wu && p.b && p.Wl, "lstm_stack_fwd: null parameter (dir %d layer %d)", dd, l);
      MatView A;
      if (l == 0) A = dd == 0 ? mat(c.x, in) : mat_idx(c.x, in, P.rows_perm);
      else A = mat(masks ? P.HD[dd][l - 1] : P.HR[dd][l - 1], h);
      ASTK_TRY(gemm_launch(GEMM_NT, gemm_args(T * B, 4 * h, in, A, mat(p.Wu, in), P.ZG[dd][l], 4 * h, p.b), c.s));
    }
    const bool top = l == P.nl - 1;
    for (int i = 0; i < T; ++i) {
      LstmCellFwdArgs cells[2];
      for (int dd = 0; dd < P.nd; ++dd) {
        const astk_lstm_params& p = c.prm[dd * P.nl + l];
        LstmCellFwdArgs& q = cells[dd];
        memset(&q, 0, sizeof(q));
        q.npairs = 1;
        q.p[0].A = i > 0 ? P.HR[dd][l] + (size_t)(i - 1) * bh : nullptr;
        q.p[0].lda = h;
        q.p[0].W = p.Wl;
        q.p[0].ldw = h;
        q.p[0].K = i > 0 ? h : 0;     // h is None at the first step: lateral skipped (Chainer-sem A1)
        q.B = B; q.h = h;
        q.zx = P.ZG[dd][l] + (size_t)i * B * 4 * h;
        q.ld_zx = 4 * h;
        q.c_prev = i > 0 ? P.CC[dd][l] + (size_t)(i - 1) * bh : nullptr;
        q.gates = P.ZG[dd][l] + (size_t)i * B * 4 * h;
        q.ld_g = 4 * h;
        q.c_out = P.CC[dd][l] + (size_t)i * bh;
        q.h_out = P.HR[dd][l] + (size_t)i * bh;
        q.mask = masks ? masks + (((size_t)dd * P.nl + l) * T + i) * bh : nullptr;
        if (!top && masks) { q.hd_out = P.HD[dd][l] + (size_t)i * bh; q.ld_hd = h; }
        if (top) {
          const int pos = dd == 0 ? i : T - 1 - i;   // flipud of the reverse stack's output list
          q.hd_out2 = c.enc_states + (size_t)pos * H + (size_t)dd * h;
          q.ld_hd2 = (long)T * H;
        }
      }
      ASTK_TRY(lstm_cell_fwd_launch(cells, P.nd, c.s));
    }
    for (int dd = 0; dd < P.nd && !c.row_len; ++dd) {
      if (c.cT) ASTK_TRY(copy_f32(c.cT + ((size_t)dd * P.nl + l) * bh, P.CC[dd][l] + (size_t)(T - 1) * bh, bh, c.s));
      if (c.hT) ASTK_TRY(copy_f32(c.hT + ((size_t)dd * P.nl + l) * bh, P.HR[dd][l] + (size_t)(T - 1) * bh, bh, c.s));
    }
  }
  return c.row_len ? fwd_rows_outputs(c) : 0;
}

// ---- backward
// the cells of the persistent launches, [direction][layer]
// (the recurrence kernel reads its weight fragments straight from the (4h, h) parameters: no transposed copies)
void persist_bwd_cells(const LstmBwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const int T = P.T, h = P.h, H = P.nd * P.h;
  const size_t bh = (size_t)P.B * h;
  memset(cells, 0, 16 * sizeof(PersistCellHost));
  for (int dd = 0; dd < P.nd; ++dd)
    for (int l = 0; l < P.nl; ++l) {
      PersistCellHost& q = cells[dd * P.nl + l];
      const bool top = l == P.nl - 1;
      q.Wl = c.prm[dd * P.nl + l].Wl;
      q.Wu = l > 0 ? c.prm[dd * P.nl + l].Wu : nullptr;
      q.PR = P.PR[dd][l];
      q.PD = l > 0 ? P.PD[dd][l] : nullptr;
      q.PD_up = top ? nullptr : P.PD[dd][l + 1];
      q.db = c.gr[dd * P.nl + l].db;      // the recurrence kernel sums its dz columns itself
      q.db_part = deterministic_mode() ? P.DBP[dd][l] : nullptr;
      q.gates = P.ZG[dd][l];
      q.C = P.CC[dd][l];
      q.mask = c.masks ? c.masks + ((size_t)dd * P.nl + l) * T * bh : nullptr;
      q.d_enc = top ? c.d_enc + (size_t)dd * h : nullptr;
      q.dy_sb = (long)T * H; q.dy_st = H;
      q.d_hT = c.d_hT ? c.d_hT + ((size_t)dd * P.nl + l) * bh : nullptr;
      q.d_cT = c.d_cT ? c.d_cT + ((size_t)dd * P.nl + l) * bh : nullptr;
      q.reverse_pos = dd == 1;
      q.layer = l;
      q.amax = c.dz_amax[dd * P.nl + l];
    }
}

// Frames of direction dd's loop steps [i0, i1), as maximal runs [f0, f1) of equal "written yet?" state.  Loop step i of direction 0 is
// frame i, of direction 1 frame (T - i) % T (quirk Q1).  Pure: reads the book, touches no stream.
struct DxRun { int f0, f1; bool accumulate; };
std::vector<DxRun> dx_runs(int dd, int T, int i0, int i1, const std::vector<char>& touched) {
  int runs[2][2], nruns = 0;
  if (dd == 0) { runs[0][0] = i0; runs[0][1] = i1; nruns = 1; }
  else {
    const int lo = std::max(i0, 1);                                    // loop steps lo .. i1-1 -> frames T-i1+1 .. T-lo
    if (i1 > lo) { runs[nruns][0] = T - i1 + 1; runs[nruns][1] = T - lo + 1; ++nruns; }
    if (i0 == 0) { runs[nruns][0] = 0; runs[nruns][1] = 1; ++nruns; }   // loop step 0 = frame 0
  }
  std::vector<DxRun> out;
  for (int r = 0; r < nruns; ++r)
    for (int f = runs[r][0], g; f < runs[r][1]; f = g) {
      for (g = f; g < runs[r][1] && touched[g] == touched[f]; ++g) {}
      out.push_back({f, g, touched[f] != 0});
    }
  return out;
}
// dx (T,B,in) = dz_0 W_u0 of direction dd for the loop steps [i0, i1) (side-stream chunks, and the rest in line).  A product STORES the
// frames nobody has written yet and ACCUMULATES into the others (the host keeps the book: no zero fill of dx -- 79 MB at the flagship
// shape -- and the sums are the in-line schedule's).
int bwd_dx_steps(LstmBwdCall& c, int dd, int i0, int i1, hipStream_t st, const unsigned long long* amax_dz, const unsigned long long* amax_w) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h;
  const astk_lstm_params& p0 = c.prm[dd * P.nl];
  const float* dz = P.ZG[dd][0];
  for (const DxRun& r : dx_runs(dd, T, i0, i1, c.touched)) {
    MatView A = dd == 0 ? mat(dz + (size_t)r.f0 * B * 4 * h, 4 * h) : mat_idx(dz, 4 * h, P.rows_inv + (size_t)r.f0 * B);
    if (dd == 1) A.idx_rows = (long)T * B;
    ASTK_TRY(gemm_launch(GEMM_NN, with_amax_b(with_amax_a(gemm_args((r.f1 - r.f0) * B, P.in, 4 * h, A, mat(p0.Wu, P.in), c.dx + (size_t)r.f0 * B * P.in, P.in, nullptr,
                                                                    r.accumulate ? GEMM_ACCUM : GEMM_STORE), amax_dz), amax_w), st));
    for (int q = r.f0; q < r.f1; ++q) c.touched[q] = 1;
  }
  return 0;
}

// The input gradient chunk by chunk behind the recurrence (see k_wait_progress): the backward recurrence passes loop steps T-1 .. 0, so
// direction 0 delivers the high frames first and direction 1 the low ones.  Queues, on the side stream, a wait and the products of every
// chunk of the plan; the recurrence launch that makes the arrivals follows on the caller's stream.
int bwd_side_chunks(LstmBwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const SidePlan& sp = c.bside;
  hipStream_t sside = (hipStream_t)c.d->side_stream;
  unsigned* prog = P.zflags + (size_t)(SIDE_CHUNKS_MAX + 2) * 64;
  const unsigned wgs_cell = (unsigned)((P.h / 16) * c.R.wg_rows);      // arrivals per chunk: (virtual) workgroups of a cell
  for (int dd = 0; dd < P.nd; ++dd) { cells[dd * P.nl].prog = prog + dd * 64; cells[dd * P.nl].prog_cs = sp.cs; }
  hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, c.s, prog, 3, 64);      // the two counters and the wait kernels' abort word
  ASTK_LAUNCH_CHECK();
  ASTK_TRY(c.join.fork(c.s, sside, prog + 2 * 64));      // everything the products read besides dz (weights, index tables) and the zeroed counters
  c.touched.assign((size_t)P.T, 0);
  const AbortCtl wab = abort_ctl(prog + 2 * 64, PERSIST_ENC_BWD);
  GemmWgCap cap_scope(sp.cap);
  for (int k = 0; k < sp.n; ++k) {
    const int i1 = P.T - k * sp.cs, i0 = std::max(0, i1 - sp.cs);       // loop steps [i0, i1) are final when chunk k has arrived
    hipLaunchKernelGGL(k_wait_progress, dim3(1), dim3(64), 0, sside, prog, P.nd > 1 ? prog + 64 : nullptr, (unsigned)(k + 1) * wgs_cell, wab);
    ASTK_LAUNCH_CHECK();
    for (int dd = 0; dd < P.nd; ++dd) ASTK_TRY(bwd_dx_steps(c, dd, i0, i1, sside, nullptr, nullptr));
  }
  return 0;
}

// hoisted form: layer by layer from the top; a lower layer's incoming gradient is the dense (T,B,h) product dz W_u of the layer
// above, one batched product per direction between the launches (no partial tiles handed down)
int bwd_hoisted_launches(const LstmBwdCall& c, PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h;
  for (int l = P.nl - 1; l >= 0; --l) {
    PersistCellHost grp[16];
    for (int dd = 0; dd < P.nd; ++dd) {
      PersistCellHost& q = cells[dd * P.nl + l];
      q.PD = nullptr; q.PD_up = nullptr; q.up_external = 0;
      if (l < P.nl - 1) { q.d_enc = P.DX[dd]; q.dy_sb = h; q.dy_st = (long)B * h; q.reverse_pos = 0; }
      grp[dd] = q;
    }
    ASTK_TRY(lstm_persist_bwd_launch(grp, P.nd, 1, T, B, h, P.nd * h, P.counters, c.dz_amax_gen, c.R.rows, c.sr));
    if (l > 0)
      for (int dd = 0; dd < P.nd; ++dd)
        ASTK_TRY(gemm_launch(GEMM_NN, with_amax_a(gemm_args(T * B, h, 4 * h, mat(P.ZG[dd][l], 4 * h), mat(c.prm[dd * P.nl + l].Wu, h), P.DX[dd], h), c.dz_amax[dd * P.nl + l]), c.sr));
  }
  return 0;
}

// groups of layers, top group first -- the forward's groups: they start at multiples of R.lpl; the top layer of a lower group reads the
// partial dx tiles the previous launch left
int bwd_grouped_launches(const LstmBwdCall& c, const PersistCellHost* cells) {
  const LstmPlan& P = c.P;
  for (int l1 = P.nl, l0; l1 > 0; l1 = l0) {
    l0 = ((l1 - 1) / c.R.lpl) * c.R.lpl;
    const int ngl = l1 - l0;
    PersistCellHost grp[16];
    for (int dd = 0; dd < P.nd; ++dd)
      for (int l = 0; l < ngl; ++l) {
        grp[dd * ngl + l] = cells[dd * P.nl + l0 + l];
        if (l == ngl - 1 && l1 < P.nl) grp[dd * ngl + l].up_external = 1;
      }
    ASTK_TRY(lstm_persist_bwd_launch(grp, P.nd * ngl, ngl, P.T, P.B, P.h, P.nd * P.h, P.counters, c.dz_amax_gen, c.R.rows, c.sr));
  }
  return 0;
}

// persistent and hoisted paths: the whole recurrence, with the side chunks of dx queued in front of it and, on deterministic calls, the
// fold of the bias-gradient rows behind it.  The recurrence kernel leaves max |dz| of every cell for the batched products (fp16x2 scales).
int bwd_persist_recurrence(LstmBwdCall& c) {
  const LstmPlan& P = c.P;
  PersistCellHost cells[16];
  gemm_amax_reserve(P.nd * P.nl, c.dz_amax, &c.dz_amax_gen, c.s);
  persist_bwd_cells(c, cells);
  c.bside = plan_side_bwd(c.d, c.R, c.dx != nullptr && c.sr == c.s);
  if (c.bside.n > 0) ASTK_TRY(bwd_side_chunks(c, cells));
  ASTK_TRY(stream_order(c.s, c.sr));     // the recurrence kernel may live on its own (CU-masked) stream, see astk.h
  ASTK_TRY(c.R.path == LSTM_HOISTED ? bwd_hoisted_launches(c, cells) : bwd_grouped_launches(c, cells));
  ASTK_TRY(stream_order(c.sr, c.s));
  if (deterministic_mode()) {
    FoldDbJobs j;
    j.n = P.nd * P.nl; j.cols = 4 * P.h; j.nby = c.R.wg_rows;
    for (int i = 0; i < j.n; ++i) { j.db[i] = cells[i].db; j.part[i] = cells[i].db_part; }
    hipLaunchKernelGGL(k_fold_db, dim3(cdiv(4 * P.h, 256), j.n), dim3(256), 0, c.s, j);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

// per-step path, one layer: the transposed lateral weights, then T launches of the fused backward cell (both directions in one)
int bwd_step_layer(const LstmBwdCall& c, int l) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h, H = P.nd * P.h;
  const size_t bh = (size_t)B * h;
  const bool top = l == P.nl - 1;
  for (int dd = 0; dd < P.nd; ++dd)
    ASTK_TRY(transpose_f32(P.WlT[dd][l], 4 * h, c.prm[dd * P.nl + l].Wl, h, 4 * h, h, c.s));
  for (int i = T - 1; i >= 0; --i) {
    LstmCellBwdArgs cells[2];
    for (int dd = 0; dd < P.nd; ++dd) {
      LstmCellBwdArgs& q = cells[dd];
      memset(&q, 0, sizeof(q));
      q.npairs = 1;
      const bool last = i == T - 1;
      q.p[0].A = last ? nullptr : P.ZG[dd][l] + (size_t)(i + 1) * B * 4 * h;   // dz of step i+1
      q.p[0].lda = 4 * h;
      q.p[0].W = P.WlT[dd][l];
      q.p[0].ldw = 4 * h;
      q.p[0].K = last ? 0 : 4 * h;
      q.B = B; q.h = h;
      q.dh_add = (last && c.d_hT) ? c.d_hT + ((size_t)dd * P.nl + l) * bh : nullptr;
      if (top) {
        const int pos = dd == 0 ? i : T - 1 - i;
        q.dy2 = c.d_enc + (size_t)pos * H + (size_t)dd * h;
        q.ld_dy2 = (long)T * H;
      } else {
        q.dy = P.DX[dd] + (size_t)i * bh;
        q.ld_dy = h;
      }
      q.mask = c.masks ? c.masks + (((size_t)dd * P.nl + l) * T + i) * bh : nullptr;
      q.dc_next = last ? (c.d_cT ? c.d_cT + ((size_t)dd * P.nl + l) * bh : nullptr) : P.DC[dd][(i + 1) & 1];
      q.c_prev = i > 0 ? P.CC[dd][l] + (size_t)(i - 1) * bh : nullptr;
      q.c_cur = P.CC[dd][l] + (size_t)i * bh;
      q.gates_dz = P.ZG[dd][l] + (size_t)i * B * 4 * h;
      q.ld_g = 4 * h;
      q.dc_prev = P.DC[dd][i & 1];
    }
    ASTK_TRY(lstm_cell_bwd_launch(cells, P.nd, c.s));
  }
  return 0;
}

// ---- the batched products over all time steps.  begin: absolute maxima (fp16x2 GEMM scales) of the matrices that feed several products --
// the frames (B operand of both directions' layer-0 dWu) and the layer-0 upward weights (dx) by a pass here; the layer outputs are bounded
// by construction (|h| < 1, times the dropout scale): no pass over them.  Every cell's dz: see bwd_products_layer.
void bwd_products_begin(LstmBwdCall& c) {
  layer0_amax(c, c.dx != nullptr, c.ax, c.aw0);
  c.ahb = c.d->out_bound > 0.f ? gemm_amax_bound(exp2f(ceilf(log2f(c.d->out_bound))), c.s) : nullptr;
  c.nwg = 0;
}
int bwd_group_add(LstmBwdCall& c, const GemmArgs& g) {
  if (c.nwg == GEMM_GROUP_MAX) { ASTK_TRY(gemm_launch_group(GEMM_TN, c.wg, c.nwg, c.s)); c.nwg = 0; }
  c.wg[c.nwg++] = g;
  return 0;
}
// One layer: dWl, dWu (collected into grouped launches), and the gradient wrt the layer's input.  On the per-step path also db, and the
// call sits BETWEEN the recurrences of layers l and l - 1: DX feeds the layer below.  On the persistent paths db, DX and max |dz| are the
// recurrence kernel's, and all layers follow the recurrence.
int bwd_products_layer(LstmBwdCall& c, int l) {
  const LstmPlan& P = c.P;
  const int T = P.T, B = P.B, h = P.h, rows = T * B, in = l == 0 ? P.in : h;
  const bool persist = c.R.path != LSTM_PER_STEP;
  const float* masks = c.masks;
  for (int dd = 0; dd < P.nd; ++dd) {
    const astk_lstm_params& p = c.prm[dd * P.nl + l];
    const astk_lstm_grads& g = c.gr[dd * P.nl + l];
    const float* dz = P.ZG[dd][l];
    // dz feeds up to three products (dWl, dWu, the input gradient): one absolute-maximum pass for all of them
    const unsigned long long* adz = persist ? c.dz_amax[dd * P.nl + l] : gemm_amax(dz, rows, 4 * h, 4 * h, c.s);
    // dWl (4h,h) += sum_{i>=1} dz_i^T h_{i-1}
    if (T > 1)
      ASTK_TRY(bwd_group_add(c, with_amax_b(with_amax_a(gemm_args(4 * h, h, rows - B, mat(dz + (size_t)B * 4 * h, 4 * h), mat(P.HR[dd][l], h), g.dWl, h, nullptr, GEMM_ATOMIC, 1), adz), c.ahb)));
    // dWu (4h,in) += dz^T X   (reverse stack, layer 0: dz is first re-ordered to frame order, sum_i dz_i^T x[perm i] = sum_f dz[inv f]^T x_f)
    MatView Xv = l == 0 ? mat(c.x, in) : mat(masks ? P.HD[dd][l - 1] : P.HR[dd][l - 1], h);
    const float* dzu = dz;
    if (l == 0 && dd == 1) {
      hipLaunchKernelGGL(k_gather_rows, dim3(2048), dim3(256), 0, c.s, P.GATH, dz, P.rows_inv, rows, h);
      ASTK_LAUNCH_CHECK();
      dzu = P.GATH;
    }
    if (l == 0 && (dd == 1 || low_precision_gemms())) {   // GATH is a single scratch buffer: issue this product right away
      // (K9's weight gradient; in low-precision mode also direction 0's, which otherwise rides in the grouped launch)
      // (the gathered copy holds the same values as dz: same maximum)
      ASTK_TRY(gemm_launch(GEMM_TN, with_amax_b(with_amax_a(lowp(gemm_args(4 * h, in, rows, mat(dzu, 4 * h), Xv, g.dWu, in, nullptr, GEMM_ATOMIC, 1)), adz), c.ax), c.s));
    } else {
      ASTK_TRY(bwd_group_add(c, with_amax_b(with_amax_a(gemm_args(4 * h, in, rows, mat(dzu, 4 * h), Xv, g.dWu, in, nullptr, GEMM_ATOMIC, 1), adz), l == 0 ? c.ax : c.ahb)));
    }
    if (!persist) ASTK_TRY(c.cb.add(g.db, dz, 4 * h, rows, 4 * h, c.s));
    // gradient wrt the layer input
    if (l > 0) {
      if (!persist) ASTK_TRY(gemm_launch(GEMM_NN, with_amax_a(gemm_args(rows, h, 4 * h, mat(dz, 4 * h), mat(p.Wu, h), P.DX[dd], h), adz), c.s));
    } else if (c.dx && c.bside.n == 0) {
      // dx (T,B,in) in frame order: direction 0 stores, direction 1 accumulates through the inverse permutation
      MatView A = dd == 0 ? mat(dz, 4 * h) : mat_idx(dz, 4 * h, P.rows_inv);
      ASTK_TRY(gemm_launch(GEMM_NN, with_amax_b(with_amax_a(lowp(gemm_args(rows, in, 4 * h, A, mat(p.Wu, in), c.dx, in, nullptr, dd == 0 ? GEMM_STORE : GEMM_ACCUM)), adz), c.aw0[dd]), c.s));
    } else if (c.dx) {
      // the loop steps the side stream did not take, at full width; the side chunks were sized to be done by now, and their frames are in `touched`
      if (dd == 0) ASTK_TRY(c.join.join());
      const int i1 = T - c.bside.n * c.bside.cs;
      if (i1 > 0) ASTK_TRY(bwd_dx_steps(c, dd, 0, i1, c.s, adz, c.aw0[dd]));
    }
  }
  return 0;
}
int bwd_products_end(LstmBwdCall& c) {
  ASTK_TRY(c.cb.flush(c.s));
  if (c.nwg > 0) ASTK_TRY(gemm_launch_group(GEMM_TN, c.wg, c.nwg, c.s));
  if (c.bside.n > 0) ASTK_TRY(c.join.join());      // join: the caller sees one-stream semantics
  return 0;
}
}  // namespace
}  // namespace astk

using namespace astk;

extern "C" {

// (the queries resolve the arithmetic like the calls they describe: the descriptor's wish, else the process default)
int astk_lstm_stack_path(const astk_lstm_stack_desc* d) {
  if (!d || d->struct_size != sizeof(astk_lstm_stack_desc)) return 0;
  PrecScope prec_scope(d->precision, d->gemm_operands);
  return lstm_route(d).path;
}

int astk_lstm_stack_side_plan(const astk_lstm_stack_desc* d, int* fwd_head_steps, int* fwd_chunks, int* bwd_chunks) {
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  ASTK_CHECK(d->T > 0 && d->B > 0 && d->in_dim > 0 && d->h > 0 && d->n_layers >= 1 && d->n_layers <= ASTK_MAX_RNN_LAYERS && (d->n_dirs == 1 || d->n_dirs == 2),
             "lstm_stack_side_plan: bad dims");
  PrecScope prec_scope(d->precision, d->gemm_operands);
  DetScope det_scope(d->deterministic);      // (for plan_side_bwd only, as in astk_lstm_stack_bwd_on: plan_side_fwd reads the field and the knob itself)
  // the calls' own plans (astk_lstm_stack_fwd / _bwd_on with an input gradient and the recurrence on the call's stream)
  const LstmRoute R = lstm_route(d);
  const SidePlan f = plan_side_fwd(d, R), b = plan_side_bwd(d, R, true);
  if (fwd_head_steps) *fwd_head_steps = f.s0;
  if (fwd_chunks) *fwd_chunks = f.n;
  if (bwd_chunks) *bwd_chunks = b.n;
  return 0;
}

int astk_lstm_stack_free_cus(const astk_lstm_stack_desc* d) {
  if (!d || d->struct_size != sizeof(astk_lstm_stack_desc)) return 0;
  PrecScope prec_scope(d->precision, d->gemm_operands);
  const LstmRoute R = lstm_route(d);
  return R.path == LSTM_PER_STEP ? 0 : std::max(0, device_cu_count() - R.wgs_first);
}

int astk_lstm_stack_form(const astk_lstm_stack_desc* d, int* rows, int* xs) {
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  ASTK_CHECK(d->T > 0 && d->B > 0 && d->in_dim > 0 && d->h > 0 && d->n_layers >= 1 && d->n_layers <= ASTK_MAX_RNN_LAYERS && (d->n_dirs == 1 || d->n_dirs == 2),
             "lstm_stack_form: bad dims");
  PrecScope prec_scope(d->precision, d->gemm_operands);
  const LstmRoute R = lstm_route(d);
  if (rows) *rows = R.rows;
  if (xs) *xs = R.xs;
  return 0;
}

size_t astk_lstm_stack_workspace_bytes(const astk_lstm_stack_desc* d) {
  LstmRoute R;
  LstmPlan P;
  return make_plan(d, nullptr, R, P) != 0 ? 0 : P.bytes;
}

// the forward pass of both entry points; row_len (device, host-checked by astk_lstm_stack_fwd_rows): the per-row index table and outputs
static int lstm_fwd(const astk_lstm_stack_desc* d, const astk_lstm_params* prm, const float* x, const float* masks, const int* row_len,
                    float* enc_states, float* cT, float* hT, void* ws, size_t ws_bytes, void* stream) {
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  PrecScope prec_scope(d->precision, d->gemm_operands);
  GemmForwardScope forward_scope;      // split tiles of this op's products have at most two contributors (reproducible forward pass)
  LstmFwdCall c;
  c.d = d; c.prm = prm; c.x = x; c.masks = masks; c.enc_states = enc_states; c.cT = cT; c.hT = hT; c.s = (hipStream_t)stream;
  c.row_len = row_len;
  ASTK_TRY(make_plan(d, ws, c.R, c.P));
  const LstmPlan& P = c.P;
  ASTK_CHECK(ws && ws_bytes >= P.bytes, "lstm_stack_fwd: workspace too small (%zu < %zu)", ws_bytes, P.bytes);
  ASTK_CHECK(prm && x && enc_states, "lstm_stack_fwd: null pointer");
  c.side = plan_side_fwd(d, c.R);
  const unsigned long long* fold_src = x_amax_strided(d) ? (const unsigned long long*)d->x_amax : nullptr;
  if (row_len)
    hipLaunchKernelGGL(k_perm_rows_len, dim3(cdiv(P.T * P.B, 256)), dim3(256), 0, c.s, P.rows_perm, P.T, P.B, row_len, fold_src, P.ax,
                       c.side.n > 0 ? P.zflags : nullptr, c.side.n + 2);
  else
  hipLaunchKernelGGL(k_perm_rows, dim3(cdiv(P.T * P.B, 256)), dim3(256), 0, c.s, P.perm, P.inv, P.rows_perm, P.rows_inv, P.T, P.B,
                     fold_src, P.ax, c.side.n > 0 ? P.zflags : nullptr, c.side.n + 2);
  ASTK_LAUNCH_CHECK();
  return c.R.path == LSTM_PER_STEP ? fwd_steps(c) : fwd_persist(c);
}

int astk_lstm_stack_fwd(const astk_lstm_stack_desc* d, const astk_lstm_params* prm, const float* x, const float* masks,
                        float* enc_states, float* cT, float* hT, void* ws, size_t ws_bytes, void* stream) {
  return lstm_fwd(d, prm, x, masks, nullptr, enc_states, cT, hT, ws, ws_bytes, stream);
}

// (every route keeps each step's h and c of every cell in the workspace, which is all the per-row outputs need: no route reports 0;
//  what does is a batch above the rows limit, and a descriptor astk_lstm_stack_workspace_bytes refuses)
size_t astk_lstm_stack_rows_workspace_bytes(const astk_lstm_stack_desc* d) {
  if (!d || d->struct_size != sizeof(astk_lstm_stack_desc) || d->B > ASTK_ENCODE_ROWS_MAX) return 0;
  return astk_lstm_stack_workspace_bytes(d);
}

int astk_lstm_stack_fwd_rows(const astk_lstm_stack_desc* d, const astk_lstm_params* prm, const float* x, const int32_t* row_len,
                             float* enc_states, float* cT, float* hT, void* ws, size_t ws_bytes, void* stream) {
  if (!row_len) return astk_lstm_stack_fwd(d, prm, x, nullptr, enc_states, cT, hT, ws, ws_bytes, stream);
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  ASTK_CHECK(d->B >= 1 && d->B <= ASTK_ENCODE_ROWS_MAX, "lstm_stack_fwd_rows: 1..%d rows, got %d", ASTK_ENCODE_ROWS_MAX, d->B);
  // the lengths index the workspace: read back and checked before anything is launched
  int32_t len[ASTK_ENCODE_ROWS_MAX];
  ASTK_CHECK(hipMemcpyAsync(len, row_len, (size_t)d->B * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess &&
             hipStreamSynchronize((hipStream_t)stream) == hipSuccess, "lstm_stack_fwd_rows: reading row_len failed");
  for (int b = 0; b < d->B; ++b)
    ASTK_CHECK(len[b] >= 1 && len[b] <= d->T, "lstm_stack_fwd_rows: row_len[%d] = %d outside 1..T = %d", b, len[b], d->T);
  return lstm_fwd(d, prm, x, nullptr, row_len, enc_states, cT, hT, ws, ws_bytes, stream);
}

int astk_lstm_stack_bwd(const astk_lstm_stack_desc* d, const astk_lstm_params* prm, const astk_lstm_grads* gr, const float* x,
                        const float* masks, const float* d_enc, const float* d_cT, const float* d_hT, float* dx, void* ws,
                        size_t ws_bytes, void* stream) {
  return astk_lstm_stack_bwd_on(d, prm, gr, x, masks, d_enc, d_cT, d_hT, dx, ws, ws_bytes, stream, nullptr);
}

int astk_lstm_stack_bwd_on(const astk_lstm_stack_desc* d, const astk_lstm_params* prm, const astk_lstm_grads* gr, const float* x,
                           const float* masks, const float* d_enc, const float* d_cT, const float* d_hT, float* dx, void* ws,
                           size_t ws_bytes, void* stream, void* recurrence_stream) {
  ASTK_CHECK_DESC(d, astk_lstm_stack_desc);
  PrecScope prec_scope(d->precision, d->gemm_operands);
  DetScope det_scope(d->deterministic);
  LstmBwdCall c;
  c.d = d; c.prm = prm; c.gr = gr; c.x = x; c.masks = masks; c.d_enc = d_enc; c.d_cT = d_cT; c.d_hT = d_hT; c.dx = dx;
  c.s = (hipStream_t)stream;
  c.sr = recurrence_stream ? (hipStream_t)recurrence_stream : c.s;
  for (int i = 0; i < 16; ++i) c.dz_amax[i] = nullptr;
  c.dz_amax_gen = 0;
  ASTK_TRY(make_plan(d, ws, c.R, c.P));
  c.bside = SidePlan{c.P.T, 0, 0, 0};
  ASTK_CHECK(ws && ws_bytes >= c.P.bytes, "lstm_stack_bwd: workspace too small");
  ASTK_CHECK(prm && gr && x && d_enc, "lstm_stack_bwd: null pointer");
  // persistent paths: the whole recurrence, then the products of every layer; per-step path: the products of layer l BETWEEN the
  // recurrences of layers l and l - 1 (they write the DX that the layer below reads)
  if (c.R.path != LSTM_PER_STEP) ASTK_TRY(bwd_persist_recurrence(c));
  bwd_products_begin(c);
  for (int l = c.P.nl - 1; l >= 0; --l) {
    if (c.R.path == LSTM_PER_STEP) ASTK_TRY(bwd_step_layer(c, l));
    ASTK_TRY(bwd_products_layer(c, l));
  }
  return bwd_products_end(c);
}

}  // extern "C"
