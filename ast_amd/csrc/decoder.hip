// Attention decoder loop (seq2seq.py:318-333, 361-473) and its hand-written backward.
//
// Per step s (all on one stream, graph-capturable; the teacher-forcing coin of quirk Q4 is a device flag so
// the launch sequence is static):
//   embed(+dropout) into the [emb ; ht_{s-1}] input-feeding buffer -> fused LSTM cells (row-panel MFMA +
//   gate epilogue) -> q = Wa h + ba -> attention scan (attn.hip) -> ht = tanh(Wc[cv;h] + bc) (written to HT and
//   into the next step's concat buffer) -> logits = Wo ht + bo -> fused softmax-CE / argmax / dlogits.
// Everything the backward needs is saved step-major in the workspace; weight gradients are NOT computed per
// step: the per-step data-path gradients (dz, d_pre, dq, ...) are saved and every dW is one batched TN GEMM
// over S*B rows after the loop; d_enc_states is one batched GEMM over the saved (alpha, ds).
#include "common.h"
#include <mutex>
#include "decoder_persist.h"
#include "decoder_wide.h"

namespace astk {

namespace {

struct DecPlan {
  int B, L, S, T, Tp, H, E, A, V, Vp, XI, nl;
  int NA, CW;    // attention heads; width of the [cv_0; ..; cv_{NA-1}; h] buffer = (NA+1)*H
  bool feed, ln; // input feeding (ht_{s-1} behind the embedding); LayerNorm behind every LSTM's dropped output
  float* HDL[ASTK_MAX_RNN_LAYERS];   // ln: [S][B][H] dropped outputs BEFORE the LayerNorm (its saved input)
  float* DLN;    // ln: [B][H] gradient wrt a LayerNorm's output / input (scratch)
  float* DLN2;
  int* TOK;      // [S][B] token fed at step s
  int* PRED;     // [S][B] argmax of step s
  float* X0;     // [S][B][XI]  concat(emb, ht_prev)
  float* G[ASTK_MAX_RNN_LAYERS];    // [S][B][4H] gates -> dz
  float* C[ASTK_MAX_RNN_LAYERS];    // [(S+1)][B][H], C[0] = c0
  float* HR[ASTK_MAX_RNN_LAYERS];   // [(S+1)][B][H], HR[0] = h0
  float* HD[ASTK_MAX_RNN_LAYERS];   // [S][B][H] dropped outputs of layers < top (with masks)
  float* Q;      // [NA][S][B][H]
  float* ALPHA;  // [NA][S][B][Tp]
  float* CVH;    // [S][B][CW]  concat(cv_0, .., cv_{NA-1}, h_top_dropped)
  float* HT;     // [(S+1)][B][A], HT[0] = 0
  float* LOGITS; // [S][B][Vp] -> dlogits
  float* LOSSROWS;  // [S][B]
  // backward
  float* DPRE;   // [S][B][A]
  float* DCVH;   // [S][B][CW]
  float* DS;     // [NA][S][B][Tp]
  float* DQ;     // [NA][S][B][H]
  float* DX0;    // [S][B][XI]
  float* DHTOP;  // [B][H]
  float* DC[ASTK_MAX_RNN_LAYERS][2];
  float* WoT;    // [A][Vp]
  float* LG1;    // [B][Vp] logits of a step whose argmax is fed back (when every step is scored behind the loop)
  float* WPART;  // wide persistent forward loop (decoder_wide.hip): partial attention sums, counters
  unsigned* WCTR;
  float* WBWD;   // wide persistent backward loop: partial sums, counters
  unsigned* WBCTR;
  float* WcT;    // [CW][A]
  float* WaT;    // [NA][H][H]
  float* WuT[ASTK_MAX_RNN_LAYERS];  // [in][4H]
  float* WlT[ASTK_MAX_RNN_LAYERS];  // [H][4H]
  float *LSE, *PART, *CESTAT, *ENCA, *MLB, *DXH;       // persistent path only
  unsigned* PCTR;
  void* attn_ws;
  size_t bytes;
};

// Which kernel path a forward call took on a workspace (diagnostics only, never read by a kernel): every call routes itself (dec_route,
// below) from the shape AND the tuning knobs ("dec.persist" / "dec.wide"), and the workspace carve follows, so a backward call made under
// other knobs than its forward call would read the saved activations at shifted offsets without any error.  The forward records
// (workspace, route.path), the backward refuses a workspace whose record differs.
struct PathRecord { const void* ws; int path; };
static std::mutex g_path_mu;
static PathRecord g_path_ring[64];
static unsigned g_path_next = 0;
static void path_record(const void* ws, int path) {
  std::lock_guard<std::mutex> lock(g_path_mu);
  for (auto& r : g_path_ring)
    if (r.ws == ws) { r.path = path; return; }
  g_path_ring[g_path_next++ % 64] = PathRecord{ws, path};
}
static int path_lookup(const void* ws) {      // -1: no forward call recorded for this workspace
  std::lock_guard<std::mutex> lock(g_path_mu);
  for (auto& r : g_path_ring)
    if (r.ws == ws) return r.path;
  return -1;
}

// ---- the route of a call.  Three kernel paths run the loop: the persistent loops of decoder_persist.hip (1-3 layers, all weights
// resident), the wide loops of decoder_wide.hip (H = A = 1024) and the per-launch loop of this file; a batch too large for one persistent
// launch may run as two calls over halves of its rows (row split, below).  Which of them a call takes is decided HERE, once per call, from
// the descriptor, the tuning knobs ("dec.persist" / "dec.wide" / "dec.b6_split", read at every call) and whether the call brings an
// out_mask (dropout on the logits is in no persistent loop's CE role: per-launch loop).  Everything else reads the struct.
enum DecPath { DEC_PER_LAUNCH = 0, DEC_PERSIST = 1, DEC_WIDE = 2 };      // (the numbers are what the path record's error message prints)
struct DecRoute {
  DecPath path;
  bool persist_carve;   // the shape fits the persistent loop: make_plan carves its buffers, whichever path THIS call takes (a call with an
                        // out_mask runs the per-launch loop on the same workspace)
  bool split;           // two calls over the rows [0, B0) and [B0, B), each routed on its own (never with an out_mask)
  int B0;
  int nsplit, chunk;    // persistent loop: time slices per batch row and the rows of a slice
  bool special;         // ... its H == 512 attention phase (astk_decoder_path bit 1)
  bool b6_split;        // ... its backward's d_x0 phase as two K halves per item (DXH)
};
DecRoute dec_route(const astk_decoder_desc* d, bool has_out_mask) {
  DecRoute r;
  memset(&r, 0, sizeof(r));
  r.nsplit = r.chunk = 1;
  r.persist_carve = decoder_persist_applicable(d, &r.nsplit, &r.chunk);
  const bool wide_fits = decoder_wide_applicable(d, nullptr, nullptr);
  r.path = has_out_mask ? DEC_PER_LAUNCH : (r.persist_carve ? DEC_PERSIST : (wide_fits ? DEC_WIDE : DEC_PER_LAUNCH));
  if (r.path == DEC_PERSIST) {
    r.special = pdec_special(d->H, r.chunk);
    r.b6_split = decoder_persist_b6_split(d);
  }
  // row split: no loop holds the whole batch, one holds each half
  if (has_out_mask || r.persist_carve || wide_fits) return r;
  if (d->B < 2 || d->n_attn > 1 || d->no_feed_attn || d->ln || d->L < 2) return r;
  const int B0 = ((d->B / 2 + 15) / 16) * 16;
  if (B0 >= d->B) return r;
  for (int i = 0; i < 2; ++i) {
    astk_decoder_desc half = *d;
    half.B = i == 0 ? B0 : d->B - B0;
    int ns = 1, ch = 1;
    // (the wide decoder's loops only for more than 32 rows: at 32 rows and slices too long for LDS two half launches are no faster than the
    //  per-launch loop)
    if (!decoder_persist_applicable(&half, &ns, &ch) && !(d->B > 32 && decoder_wide_applicable(&half, nullptr, nullptr))) return r;
  }
  r.split = true;
  r.B0 = B0;
  return r;
}

bool label_smoothing_ok(float eps) { return std::isfinite(eps) && eps >= 0.f && eps < 1.f; }

int dec_validate(const astk_decoder_desc* d) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(d && d->B > 0 && d->L >= 2 && d->T > 0 && d->V > 1, "decoder: bad dims");
  ASTK_CHECK(d->n_layers >= 1 && d->n_layers <= ASTK_MAX_RNN_LAYERS, "decoder: layers");
  ASTK_CHECK((d->H % 4) == 0 && (d->E % 4) == 0 && (d->A % 4) == 0, "decoder: H, E, A must be multiples of 4");
  ASTK_CHECK(d->n_attn >= 0 && d->n_attn <= ASTK_MAX_ATTN, "decoder: n_attn %d (max %d)", d->n_attn, ASTK_MAX_ATTN);
  ASTK_CHECK(label_smoothing_ok(d->label_smoothing), "decoder: label_smoothing %g (finite, 0 <= eps < 1)", (double)d->label_smoothing);
  return 0;
}

// the workspace carve of a validated descriptor (ws == nullptr: sizes only)
void make_plan(const astk_decoder_desc* d, const DecRoute& r, void* ws, DecPlan& P) {
  P.B = d->B; P.L = d->L; P.S = d->L - 1; P.T = d->T; P.Tp = (d->T + 3) / 4 * 4;
  P.H = d->H; P.E = d->E; P.A = d->A; P.V = d->V; P.Vp = (d->V + 3) / 4 * 4; P.nl = d->n_layers;
  P.NA = d->n_attn > 1 ? d->n_attn : 1;
  P.CW = (P.NA + 1) * d->H;
  P.feed = d->no_feed_attn == 0;
  P.ln = d->ln != 0;
  P.XI = P.feed ? d->E + d->A : d->E;
  Carver c(ws);
  const size_t S = P.S, B = P.B, H = P.H, NA = P.NA, CW = P.CW;
  P.TOK = c.take<int>(S * B);
  P.PRED = c.take<int>(S * B);
  P.X0 = c.take<float>(S * B * P.XI);
  for (int l = 0; l < P.nl; ++l) {
    P.G[l] = c.take<float>(S * B * 4 * H);
    P.C[l] = c.take<float>((S + 1) * B * H);
    P.HR[l] = c.take<float>((S + 1) * B * H);
    P.HD[l] = c.take<float>(S * B * H);
    P.DC[l][0] = c.take<float>(B * H);
    P.DC[l][1] = c.take<float>(B * H);
    const size_t in = l == 0 ? P.XI : H;
    P.WuT[l] = c.take<float>(in * 4 * H);
    P.WlT[l] = c.take<float>(H * 4 * H);
    P.HDL[l] = c.take<float>(P.ln ? S * B * H : 4);
  }
  P.DLN = c.take<float>(B * H);
  P.DLN2 = c.take<float>(B * H);
  P.Q = c.take<float>(NA * S * B * H);
  P.ALPHA = c.take<float>(NA * S * B * P.Tp);
  P.CVH = c.take<float>(S * B * CW);
  P.HT = c.take<float>((S + 1) * B * P.A);
  P.LOGITS = c.take<float>(S * B * P.Vp);
  P.LOSSROWS = c.take<float>(S * B);
  P.DPRE = c.take<float>(S * B * P.A);
  P.DCVH = c.take<float>(S * B * CW);
  P.DS = c.take<float>(NA * S * B * P.Tp);
  P.DQ = c.take<float>(NA * S * B * H);
  P.DX0 = c.take<float>(S * B * P.XI);
  P.DHTOP = c.take<float>(B * H);
  P.WoT = c.take<float>((size_t)P.A * P.Vp);
  P.LG1 = c.take<float>((size_t)P.B * P.Vp);
  P.WPART = c.take<float>(decoder_wide_part_floats(d));
  P.WCTR = c.take<unsigned>(decoder_wide_ctr_words(d));
  P.WBWD = c.take<float>(decoder_wide_bwd_floats(d));
  P.WBCTR = c.take<unsigned>(decoder_wide_bwd_ctr_words(d));
  P.WcT = c.take<float>(CW * P.A);
  P.WaT = c.take<float>(NA * H * H);
  P.attn_ws = c.take<char>(attn_ws_bytes(P.B, P.T, P.H));
  const bool pp = r.persist_carve;
  P.LSE = c.take<float>(pp ? S * B : 4);
  P.PART = c.take<float>(pp ? S * B * r.nsplit * (H + 4) : 4);
  P.CESTAT = c.take<float>(pp ? S * B * (size_t)((P.V + 15) / 16) * 4 : 4);
  P.ENCA = c.take<float>(pp ? B * (size_t)P.T * H : 4);
  P.MLB = c.take<float>(pp ? S * B * 2 : 4);
  P.PCTR = c.take<unsigned>(pp ? (size_t)(8 * 32 * ((P.B + 15) / 16) + 2 + P.B + 1) * 64 : 4);   // sharded phase counters, abort word, per-row
                                                                                                 // counters, k_decoder_post's arrival counter
  P.DXH = c.take<float>(pp ? 2 * S * B * (size_t)P.A : 4);
  P.bytes = c.total();
}

// the slices of a plan the persistent and the wide launchers take (decoder_persist.h, decoder_wide.h)
DecPersistBuffers persist_fwd_buffers(const DecPlan& P, const float* c0, const float* h0) {
  DecPersistBuffers bf;
  memset(&bf, 0, sizeof(bf));
  bf.TOK = P.TOK; bf.PRED = P.PRED; bf.X0 = P.X0; bf.Q = P.Q; bf.ALPHA = P.ALPHA;
  for (int l = 0; l < P.nl; ++l) { bf.G[l] = P.G[l]; bf.C[l] = P.C[l]; bf.HR[l] = P.HR[l]; bf.HD[l] = P.HD[l]; }
  bf.CVH = P.CVH; bf.HT = P.HT; bf.LOGITS = P.LOGITS; bf.LOSSROWS = P.LOSSROWS; bf.LSE = P.LSE; bf.PART = P.PART;
  bf.CESTAT = P.CESTAT; bf.ENCA = P.ENCA; bf.ML = P.MLB; bf.ctr = P.PCTR;
  // initial states and zero attention vector (seq2seq.py:318-333, :420): the launcher copies / zeroes them with its own fill launch
  bf.zero_a = P.HT; bf.zero_a_bytes = (size_t)P.B * P.A * sizeof(float);
  bf.zero_b = P.X0; bf.zero_b_bytes = (size_t)P.B * P.XI * sizeof(float);
  bf.c0 = c0; bf.h0 = h0;
  return bf;
}
DecWideBuffers wide_fwd_buffers(const DecPlan& P) {
  DecWideBuffers wb;
  wb.TOK = P.TOK; wb.PRED = P.PRED; wb.X0 = P.X0; wb.G = P.G[0]; wb.C = P.C[0]; wb.HR = P.HR[0]; wb.Q = P.Q; wb.ALPHA = P.ALPHA;
  wb.CVH = P.CVH; wb.HT = P.HT; wb.PART = P.WPART; wb.ctr = P.WCTR;
  return wb;
}
DecPersistBwdBuffers persist_bwd_buffers(const DecPlan& P, const astk_decoder_desc* d, const DecRoute& r, float* d_enc, float* d_c0) {
  DecPersistBwdBuffers bf;
  memset(&bf, 0, sizeof(bf));
  bf.WoT = P.WoT; bf.WcT = P.WcT; bf.ENCA = P.ENCA; bf.ALPHA = P.ALPHA; bf.CVH = P.CVH; bf.ML = P.MLB;
  for (int l = 0; l < P.nl; ++l) { bf.WlT[l] = P.WlT[l]; bf.WuT[l] = P.WuT[l]; bf.C[l] = P.C[l]; bf.G[l] = P.G[l]; }
  bf.HT = P.HT; bf.LOGITS = P.LOGITS; bf.DPRE = P.DPRE; bf.DCVH = P.DCVH; bf.DS = P.DS; bf.DX0 = P.DX0;
  bf.DHATT = P.PART; bf.d_c0 = d_c0; bf.ctr = P.PCTR;
  bf.DXH = r.b6_split ? P.DXH : nullptr;
  bf.zero_ptr = d->zero_ptr; bf.zero_bytes = d->zero_bytes;
  bf.zero2_ptr = d_enc; bf.zero2_bytes = (size_t)P.B * P.T * P.H * sizeof(float);
  return bf;
}
DecWideBwdBuffers wide_bwd_buffers(const DecPlan& P) {
  DecWideBwdBuffers wb;
  wb.WcT = P.WcT; wb.WaT = P.WaT; wb.WlT = P.WlT[0]; wb.WuT = P.WuT[0]; wb.ALPHA = P.ALPHA; wb.CVH = P.CVH; wb.HT = P.HT; wb.C = P.C[0];
  wb.G = P.G[0]; wb.DPRE = P.DPRE; wb.DCVH = P.DCVH; wb.DS = P.DS; wb.DQ = P.DQ; wb.DHTOP = P.DHTOP; wb.DC0 = P.DC[0][0];
  wb.scratch = P.WBWD; wb.ctr = P.WBCTR;
  return wb;
}

// tok = use_truth[s] ? y[b][s] : pred_prev[b] ; x0[b][0:E] = embed[tok] * mask   (seq2seq.py:365, 431-436)
__global__ void k_embed(const float* __restrict__ embed, const int32_t* __restrict__ y, int L, int s, const int32_t* __restrict__ use_truth,
                        const int32_t* __restrict__ pred_prev, const int32_t* __restrict__ tokens_direct, int32_t* __restrict__ tok_out,
                        const float* __restrict__ mask, float* __restrict__ x0, int B, int E, int XI, int V) {
  const int b = blockIdx.x;
  int tok;
  if (tokens_direct) tok = tokens_direct[b];
  else tok = (use_truth[s] || !pred_prev) ? y[(long)b * L + s] : pred_prev[b];
  tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
  if (threadIdx.x == 0 && tok_out) tok_out[b] = tok;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float v = embed[(long)tok * E + e];
    if (mask) v *= mask[(long)b * E + e];
    x0[(long)b * XI + e] = v;
  }
}

// d_embed[tok][e] += dx0[s][b][e] * mask  for all (s,b)
__global__ void k_embed_bwd(float* __restrict__ d_embed, const int32_t* __restrict__ tok, const float* __restrict__ dx0,
                            const float* __restrict__ mask, int SB, int E, int XI, int V) {
  const int r = blockIdx.x;
  if (r >= SB) return;
  // (clamped: after a forward launch that timed out -- the step is discarded, but its backward still runs before the host reads the status
  // word -- the token buffer may hold whatever the workspace held; never an index outside the table)
  const int t = min(max(tok[r], 0), V - 1);
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float v = dx0[(long)r * XI + e];
    if (mask) v *= mask[(long)r * E + e];
    atomicAdd(&d_embed[(long)t * E + e], v);
  }
}

// deterministic calls: one block per TOKEN adds the rows that embedded it, in row order (no atomics: the table row is the block's own)
__global__ void k_embed_bwd_det(float* __restrict__ d_embed, const int32_t* __restrict__ tok, const float* __restrict__ dx0,
                                const float* __restrict__ mask, int SB, int E, int XI, int V) {
  const int t = blockIdx.x;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float sum = 0.f;
    bool any = false;
    for (int r = 0; r < SB; ++r) {
      if (min(max(tok[r], 0), V - 1) != t) continue;
      float v = dx0[(long)r * XI + e];
      if (mask) v *= mask[(long)r * E + e];
      sum += v;
      any = true;
    }
    if (any) d_embed[(long)t * E + e] += sum;
  }
}

// One block per row: log-softmax, weighted NLL / count, first-max argmax, dlogits in place (Chainer-sem A6).
// Row r is (step r / rows_per_step, batch row r % rows_per_step); its class id is targets[(r % rows_per_step) * t_stride + r / rows_per_step]
// (one decoder step: rows_per_step = B and `targets` points at the step's column).  argmax_only: feedback tokens of a step whose loss is
// scored later (the batched pass); fed_flags (the loop's use_truth, n_steps entries): that batched pass leaves the argmax of the steps
// whose token was fed back (flag of the NEXT step 0) as the loop wrote it.
// eps > 0: label smoothing (astk_decoder_desc.label_smoothing).  The uniform term LSE - mean(x) is formed as
// log(se) - mean(x - mx) from the deviations the sum of exponentials reads anyway (all <= 0: no cancellation, whatever the offset of the
// row); eps == 0 runs the arithmetic this kernel always had.
// rw: per-row weights (astk_decoder_fwd_w / astk_softmax_ce_fwd_w), one per batch row of a step, or null: a factor
// on the class weight, so on the loss row and on the gradient row alike; null runs the arithmetic without it.
__global__ __launch_bounds__(256) void k_softmax_ce(int V, long ld, float* logits, const int32_t* __restrict__ targets,
                                                    long t_stride, int rows_per_step, const float* __restrict__ cw, float inv_count, float eps,
                                                    float* __restrict__ loss_rows, int32_t* __restrict__ argmax, int argmax_only,
                                                    const int32_t* __restrict__ fed_flags, int n_steps, const float* __restrict__ rw) {
  __shared__ float sv[4], sd[4];
  __shared__ int si[4];
  const int b = blockIdx.x;
  const int step = b / rows_per_step, brow = b - step * rows_per_step;
  float* x = logits + (long)b * ld;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx = -INFINITY;
  int mi = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float a = x[v];
    if (a > mx) { mx = a; mi = v; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    const int oi = __shfl_xor(mi, o);
    if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
  }
  if (lane == 0) { sv[wave] = mx; si[wave] = mi; }
  __syncthreads();
  mx = sv[0]; mi = si[0];
  for (int w = 1; w < 4; ++w)
    if (sv[w] > mx || (sv[w] == mx && si[w] < mi)) { mx = sv[w]; mi = si[w]; }
  __syncthreads();
  if (argmax_only) {
    if (threadIdx.x == 0 && argmax) argmax[b] = mi;
    return;
  }
  float sum = 0.f, dev = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float dv = x[v] - mx;
    sum += expf(dv);
    dev += dv;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (eps > 0.f)
    for (int o = 32; o > 0; o >>= 1) dev += __shfl_xor(dev, o);
  if (lane == 0) { sv[wave] = sum; sd[wave] = dev; }
  __syncthreads();
  sum = sv[0] + sv[1] + sv[2] + sv[3];
  dev = (sd[0] + sd[1]) + (sd[2] + sd[3]);
  const float lse = mx + logf(sum);
  int t = targets[(long)brow * t_stride + step];
  const bool ignore = t < 0;                      // ignore_label = -1 never occurs on this path (PAD is 0)
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);
  float w = ignore ? 0.f : (cw ? cw[t] : 1.f);
  if (rw) w *= rw[brow];
  // The target's logit has to be READ before any thread overwrites the row with the gradient below.  It used to be an ordinary load in
  // front of the barrier whose only use sat behind it; with `logits` declared __restrict__ the compiler was free to sink the load to
  // that use, i.e. behind the barrier, where thread (t % 256) may already have stored the gradient: one loss row in a few thousand
  // came out wrong by the difference, depending on which wave ran first (found at the end of round 3; the gradient was never affected).
  // Now: no __restrict__ on the row, a volatile load, and the loss row is finished in front of the barrier.
  const float xt = *reinterpret_cast<const volatile float*>(&x[t]);
  if (threadIdx.x == 0) {
    if (loss_rows) {
      if (eps > 0.f) loss_rows[b] = w * inv_count * ((1.f - eps) * (lse - xt) + eps * (logf(sum) - dev / (float)V));
      else loss_rows[b] = -(xt - lse) * w * inv_count;
    }
    const bool fed = fed_flags && step + 1 < n_steps && fed_flags[step + 1] == 0;
    if (argmax && !fed) argmax[b] = mi;
  }
  __syncthreads();
  const float scale = w * inv_count;
  if (eps > 0.f) {
    const float uni = eps / (float)V, hot = (1.f - eps) * scale;
    for (int v = threadIdx.x; v < ld; v += 256) {
      float g = 0.f;
      if (v < V) {
        g = (expf(x[v] - lse) - uni) * scale;
        if (v == t) g -= hot;
      }
      x[v] = g;
    }
    return;
  }
  for (int v = threadIdx.x; v < ld; v += 256) {
    float g = 0.f;
    if (v < V) {
      g = expf(x[v] - lse) * scale;
      if (v == t) g -= scale;
    }
    x[v] = g;
  }
}

__global__ void k_sum_to(const float* __restrict__ src, int n, float* __restrict__ dst) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)src[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (float)(red[0] + red[1] + red[2] + red[3]);
}

__global__ void k_copy_i32(int32_t* dst, const int32_t* src, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// x *= 1 - y^2 (the tanh' factor of d_pre on the rows that take no carry from a later step)
__global__ void k_dtanh_inplace(float* __restrict__ x, const float* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float t = y[i];
    x[i] *= 1.f - t * t;
  }
}

RowGemmArgs rg(int M, int N, const float* A, long lda, const float* W, long ldw, int K, float* out, long ld_out) {
  RowGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.npairs = 1;
  a.p[0].A = A; a.p[0].lda = lda; a.p[0].W = W; a.p[0].ldw = ldw; a.p[0].K = K;
  a.M = M; a.N = N; a.out = out; a.ld_out = ld_out;
  return a;
}

// dW (M x N) += A^T B over `rows` rows (A: rows x M, B: rows x N).  The weight gradients of one backward call are
// independent products with few tiles each: they are collected and issued as ONE grouped launch.
struct WgradBatch {
  GemmArgs list[GEMM_GROUP_MAX];
  int n = 0;
  bool low = false;      // every product of this batch may run with fp16 operands under astk_set_low_precision_gemms(1) (K18 / K24)
  explicit WgradBatch(bool lowp_eligible = false) : low(lowp_eligible) {}
  // (amax_a: the maximum of A, where the caller measured it -- common.h gemm_amax_many)
  int add(float* dW, long ldw, int M, int N, const float* A, long lda, const float* Bm, long ldb, int rows, hipStream_t s,
          const unsigned long long* amax_a = nullptr) {
    if (n == GEMM_GROUP_MAX) ASTK_TRY(flush(s));
    list[n] = with_amax_a(gemm_args(M, N, rows, mat(A, lda), mat(Bm, ldb), dW, ldw, nullptr, GEMM_ATOMIC, 1), amax_a);
    if (low) list[n] = lowp(list[n]);
    ++n;
    return 0;
  }
  int flush(hipStream_t s) {
    const int m = n;
    n = 0;
    return m > 0 ? gemm_launch_group(GEMM_TN, list, m, s) : 0;
  }
};

int cell_fwd(const DecPlan& P, const astk_decoder_params* prm, int l, const float* x_in, long ld_x, int in, const float* h_prev,
             const float* c_prev, float* gates, float* c_out, float* h_out, const float* mask, float* hd_out, long ld_hd,
             hipStream_t s) {
  LstmCellFwdArgs c;
  memset(&c, 0, sizeof(c));
  c.npairs = 2;
  c.p[0].A = h_prev; c.p[0].lda = P.H; c.p[0].W = prm->lstm[l].Wl; c.p[0].ldw = P.H; c.p[0].K = P.H;
  c.p[1].A = x_in; c.p[1].lda = ld_x; c.p[1].W = prm->lstm[l].Wu; c.p[1].ldw = in; c.p[1].K = in;
  c.B = P.B; c.h = P.H;
  c.bias = prm->lstm[l].b;
  c.c_prev = c_prev;
  c.gates = gates; c.ld_g = 4 * P.H;
  c.c_out = c_out; c.h_out = h_out;
  c.mask = mask;
  c.hd_out = hd_out; c.ld_hd = ld_hd;
  return lstm_cell_fwd_launch(&c, 1, s);
}

// ---- row split.  The persistent loop holds at most 32 batch rows at the shipped width (its cell, context and logits items own 16 rows
// each and the grid is one workgroup per CU).  The decoder couples no batch rows -- weights and the 1/B of the loss are all two rows
// share -- so a larger batch runs as TWO persistent launches over halves of its rows, each a complete call of this library on a
// contiguous sub-problem (inputs that are not contiguous per half -- initial states, dropout masks -- are staged; `loss_rows` keeps the
// cross-entropy mean over the WHOLE batch; parameter gradients accumulate).  3.1 ms for batch 64 instead of the per-launch loop.
struct SplitPlan {
  astk_decoder_desc sub[2];
  int off[2];
  void* ws[2];
  size_t wsb[2];
  float *c0[2], *h0[2], *dc0[2], *dh0[2], *emb[2], *rnn[2];
  int32_t* pred[2];
  float* loss2;
  size_t bytes;
};
void make_split(const astk_decoder_desc* d, const DecRoute& r, void* ws, SplitPlan& sp) {      // (r.split holds)
  const int Bs[2] = {r.B0, d->B - r.B0};
  Carver c(ws);
  const size_t S = d->L - 1, H = d->H, E = d->E, nl = d->n_layers;
  for (int i = 0; i < 2; ++i) {
    sp.sub[i] = *d;
    sp.sub[i].status_dst = nullptr;      // (the whole op's call takes the snapshot, once)
    sp.sub[i].zero_ptr = nullptr;        // (... and zeroes the caller's buffer, once: bwd_split)
    sp.sub[i].zero_bytes = 0;
    sp.sub[i].B = Bs[i];
    sp.sub[i].loss_rows = d->loss_rows > 0 ? d->loss_rows : d->B;
    sp.off[i] = i == 0 ? 0 : r.B0;
    DecPlan P;
    make_plan(&sp.sub[i], dec_route(&sp.sub[i], false), nullptr, P);
    sp.wsb[i] = P.bytes;
    sp.ws[i] = c.take<char>(P.bytes);
    const size_t b = Bs[i];
    sp.c0[i] = c.take<float>(nl * b * H); sp.h0[i] = c.take<float>(nl * b * H);
    sp.dc0[i] = c.take<float>(nl * b * H); sp.dh0[i] = c.take<float>(nl * b * H);
    sp.emb[i] = c.take<float>(S * b * E);
    sp.rnn[i] = c.take<float>(nl * S * b * H);
    sp.pred[i] = c.take<int32_t>(S * b);
  }
  sp.loss2 = c.take<float>(4);
  sp.bytes = c.total();
}

// ---- one per-launch forward step: LSTM cells (+ LayerNorm), q_k = Wa_k h + ba_k and the attention scan of every head, ht = tanh(Wc
// [cv..; h] + bc).  The training loop (fwd_steps) and the eval step (decoder_step_run) run THIS sequence; they differ in where a step's
// buffers live, which is all the struct says.
struct DecStepBufs {
  const float* x0;                                // [B][XI] the input row block [emb ; ht_prev]
  struct {
    const float *c_prev, *h_prev, *mask;          // [B][H]; mask: the layer's dropout mask or null
    float *c_new, *h_new, *gates;                 // [B][H], [B][H], [B][4H]
    float *hd, *pre_ln;                           // [B][H] dropped (normalised) output of a layer below the top one; ln: the LayerNorm's input
  } layer[ASTK_MAX_RNN_LAYERS];
  float *q[ASTK_MAX_ATTN], *alpha[ASTK_MAX_ATTN]; // [B][H], [B][Tp] per head
  float *cvh, *ht;                                // [B][CW] context vectors with the top layer's output behind them; [B][A]
  float* ht2; long ld_ht2;                        // input feeding: ht's second destination (the next step's input block), or null
  AttnFwdFn attn; const void* attn_ctx;           // null: attn_fwd_launch over enc (B, T, H)
  // the eval step's copies, where its launch order has them (null in the training loop): the new states over (n_layers, B, H) buffers
  // behind each layer's launches, the first head's alpha as (B, T) rows behind the heads
  float *c_copy, *h_copy, *alpha_copy;
};
int step_fwd(const DecPlan& P, const astk_decoder_params* prm, const float* enc, const DecStepBufs& b, hipStream_t s) {
  const int B = P.B, H = P.H, A = P.A, nl = P.nl, NA = P.NA, CW = P.CW, top = P.nl - 1;
  const size_t bh = (size_t)B * H;
  float* htop = b.cvh + (size_t)NA * H;        // the top layer's (dropped, normalised) output sits behind the NA context vectors
  const float* x_in = b.x0;
  long ld_x = P.XI;
  int in = P.XI;
  for (int l = 0; l < nl; ++l) {
    float* hd = l == top ? htop : b.layer[l].hd;
    const long ld_hd = l == top ? CW : H;
    // ln: hs = LN(dropout(LSTM(x))) (seq2seq.py:198-202): the cell leaves the dropped output in pre_ln, the LayerNorm writes the layer's output
    const auto& ly = b.layer[l];
    ASTK_TRY(cell_fwd(P, prm, l, x_in, ld_x, in, ly.h_prev, ly.c_prev, ly.gates, ly.c_new, ly.h_new, ly.mask, P.ln ? ly.pre_ln : hd, P.ln ? H : ld_hd, s));
    if (P.ln) {
      ASTK_CHECK(prm->ln_gamma[l] && prm->ln_beta[l], "decoder_fwd: ln parameters missing (layer %d)", l);
      ASTK_TRY(layernorm_fwd_launch(B, H, ly.pre_ln, H, prm->ln_gamma[l], prm->ln_beta[l], LN_EPS, hd, ld_hd, s));
    }
    if (b.c_copy) ASTK_TRY(copy_f32(b.c_copy + l * bh, ly.c_new, bh, s));
    if (b.h_copy) ASTK_TRY(copy_f32(b.h_copy + l * bh, ly.h_new, bh, s));
    x_in = hd; ld_x = ld_hd; in = H;
  }
  // every attention head on the same h (seq2seq.py:379-383): q_k = Wa_k h + ba_k, scan -> cv_k
  for (int k = 0; k < NA; ++k) {
    const float* Wa = k == 0 ? prm->Wa : prm->Wa_x[k - 1];
    const float* ba = k == 0 ? prm->ba : prm->ba_x[k - 1];
    ASTK_CHECK(Wa && ba, "decoder_fwd: attention head %d has no parameters", k);
    RowGemmArgs a = rg(B, H, htop, CW, Wa, H, H, b.q[k], H);
    a.bias = ba;
    ASTK_TRY(rowgemm_launch(a, s));
    if (b.attn) ASTK_TRY(b.attn(b.attn_ctx, B, P.T, H, enc, b.q[k], H, b.alpha[k], b.cvh + (size_t)k * H, CW, P.attn_ws, s));
    else ASTK_TRY(attn_fwd_launch(B, P.T, H, enc, b.q[k], H, b.alpha[k], b.cvh + (size_t)k * H, CW, nullptr, 0, P.attn_ws, s));
  }
  if (b.alpha_copy) ASTK_TRY(copy2d_f32(b.alpha_copy, P.T, b.alpha[0], P.Tp, B, P.T, P.T, s));
  // ht = tanh(Wc [cv..;h] + bc)
  RowGemmArgs a = rg(B, A, b.cvh, CW, prm->Wc, CW, CW, b.ht, A);
  a.bias = prm->bc;
  a.act = ACT_TANH;
  if (b.ht2) { a.out2 = b.ht2; a.ld_out2 = b.ld_ht2; }
  return rowgemm_launch(a, s);
}

// ---- forward.  astk_decoder_fwd_w validates, routes and calls one of fwd_split, fwd_persist, fwd_wide, fwd_steps.
struct DecFwdCall {
  const astk_decoder_desc* d; const astk_decoder_params* prm;
  const float *enc, *c0, *h0; const int32_t *y, *use_truth;
  const float *emb_mask, *rnn_masks, *out_mask;
  const int32_t *targets, *tgt;      // the caller's class ids or null; tgt = targets ? targets : y (scored at step s: column s + 1)
  const float* row_weight;           // (B) per-row loss weights or null (astk_decoder_fwd_w)
  float* loss; int32_t* pred;
  hipStream_t s;
};

// two calls of this library over halves of the rows; leaves the halves' losses in sp.loss2 and the predictions in the caller's buffer
int fwd_split(const DecFwdCall& f, const SplitPlan& sp) {
  const astk_decoder_desc* d = f.d;
  const int B = d->B, S = d->L - 1, H = d->H, E = d->E, nl = d->n_layers;
  for (int i = 0; i < 2; ++i) {
    const int b = sp.sub[i].B, off = sp.off[i];
    // initial states (n_layers, B, H) and masks (.., S, B, X): rows of this half, staged contiguously
    ASTK_TRY(copy2d_f32(sp.c0[i], (long)b * H, f.c0 + (size_t)off * H, (long)B * H, nl, b * H, b * H, f.s));
    ASTK_TRY(copy2d_f32(sp.h0[i], (long)b * H, f.h0 + (size_t)off * H, (long)B * H, nl, b * H, b * H, f.s));
    if (f.emb_mask) ASTK_TRY(copy2d_f32(sp.emb[i], (long)b * E, f.emb_mask + (size_t)off * E, (long)B * E, S, b * E, b * E, f.s));
    if (f.rnn_masks) ASTK_TRY(copy2d_f32(sp.rnn[i], (long)b * H, f.rnn_masks + (size_t)off * H, (long)B * H, nl * S, b * H, b * H, f.s));
    ASTK_TRY(astk_decoder_fwd_w(&sp.sub[i], f.prm, f.enc + (size_t)off * d->T * H, sp.c0[i], sp.h0[i], f.y + (size_t)off * d->L, f.use_truth,
                                 f.emb_mask ? sp.emb[i] : nullptr, f.rnn_masks ? sp.rnn[i] : nullptr, nullptr,
                                 f.targets ? f.targets + (size_t)off * d->L : nullptr, f.row_weight ? f.row_weight + off : nullptr, sp.loss2 + i, f.pred ? sp.pred[i] : nullptr, sp.ws[i], sp.wsb[i], f.s));
    if (f.pred) ASTK_TRY(copy2d_f32((float*)f.pred + off, B, (const float*)sp.pred[i], b, S, b, b, f.s));      // (S, b) -> columns of (S, B); a bit copy
  }
  return 0;
}

// the persistent loop: ONE launch (and its fill), including the loss sum, the predictions and the status snapshot
int fwd_persist(const DecFwdCall& f, const DecPlan& P) {
  return decoder_persist_fwd_launch(f.d, f.prm, f.enc, f.y, f.tgt, f.use_truth, f.emb_mask, f.rnn_masks, persist_fwd_buffers(P, f.c0, f.h0), f.loss,
                                    f.pred, f.s, f.row_weight);
}

// what the wide and the per-launch loop need in front: initial states and zero attention vector (seq2seq.py:318-333, :420) in one fill
// launch, the attention scan's ticket counters
int fwd_init(const DecFwdCall& f, const DecPlan& P) {
  const size_t bh = (size_t)P.B * P.H;
  FillSegs fz;      // one launch: the two zero fills and the state copies
  fz.n = 0;
  fill_seg_add(fz, P.HT, (size_t)P.B * P.A * sizeof(float));
  fill_seg_add(fz, P.X0, (size_t)P.B * P.XI * sizeof(float));   // ht_{-1} half of the first concat buffer
  for (int l = 0; l < P.nl; ++l) {
    if (fz.n + 2 > FILL_SEG_MAX) { ASTK_TRY(fill_u32_segments(fz, 0u, f.s)); fz.n = 0; }
    fill_seg_add_copy(fz, P.C[l], f.c0 + l * bh, bh * sizeof(float));
    fill_seg_add_copy(fz, P.HR[l], f.h0 + l * bh, bh * sizeof(float));
  }
  ASTK_TRY(fill_u32_segments(fz, 0u, f.s));
  return attn_ws_init(P.attn_ws, P.B, P.T, P.H, f.s);
}

// every step scored behind the loop: one product for the logits of all S*B rows, one softmax-CE launch (which leaves the argmax of the
// steps whose token was fed back as the loop wrote it)
int fwd_score_all(const DecFwdCall& f, const DecPlan& P) {
  const int B = P.B, S = P.S, A = P.A, V = P.V;
  const float inv_count = 1.f / (float)(f.d->loss_rows > 0 ? f.d->loss_rows : B);
  ASTK_TRY(gemm_launch(GEMM_NT, gemm_args(S * B, V, A, mat(P.HT + (size_t)B * A, A), mat(f.prm->Wo, A), P.LOGITS, P.Vp, f.prm->bo), f.s));
  if (f.out_mask) ASTK_TRY(mul_rows_launch(P.LOGITS, P.Vp, f.out_mask, V, S * B, V, f.s));
  hipLaunchKernelGGL(k_softmax_ce, dim3(S * B), dim3(256), 0, f.s, V, (long)P.Vp, P.LOGITS, f.tgt + 1, (long)P.L, B, f.prm->class_weight, inv_count,
                     f.d->label_smoothing, P.LOSSROWS, P.PRED, 0, f.use_truth, S, f.row_weight);
  ASTK_LAUNCH_CHECK();
  if (f.out_mask) ASTK_TRY(mul_rows_launch(P.LOGITS, P.Vp, f.out_mask, V, S * B, V, f.s));
  return 0;
}

// The wide decoder (configs[4]: H = A = 1024) on its persistent forward loop (decoder_wide.hip): ONE launch for all steps.  The kernel
// computes logits itself on the steps whose argmax is fed back (streamed weights) and leaves the class in PRED; every step is scored
// behind the loop like in the per-launch form with host flags.
int fwd_wide(const DecFwdCall& f, const DecPlan& P) {
  ASTK_TRY(fwd_init(f, P));
  ASTK_TRY(decoder_wide_fwd_launch(f.d, f.prm, f.enc, f.y, f.use_truth, f.emb_mask, f.rnn_masks, wide_fwd_buffers(P), 0, P.S - 1, f.s));
  return fwd_score_all(f, P);
}

// the per-launch loop
int fwd_steps(const DecFwdCall& f, const DecPlan& P) {
  const astk_decoder_params* prm = f.prm;
  hipStream_t s = f.s;
  const int B = P.B, S = P.S, H = P.H, E = P.E, A = P.A, V = P.V, XI = P.XI, nl = P.nl, NA = P.NA, CW = P.CW;
  const size_t bh = (size_t)B * H;
  const int32_t* uth = f.d->use_truth_host;      // optional host copy of use_truth: which steps feed their argmax back
  const float inv_count = 1.f / (float)(f.d->loss_rows > 0 ? f.d->loss_rows : B);
  ASTK_TRY(fwd_init(f, P));
  for (int st = 0; st < S; ++st) {
    float* x0 = P.X0 + (size_t)st * B * XI;
    hipLaunchKernelGGL(k_embed, dim3(B), dim3(128), 0, s, prm->embed, f.y, P.L, st, f.use_truth, st > 0 ? P.PRED + (size_t)(st - 1) * B : nullptr,
                       (const int32_t*)nullptr, P.TOK + (size_t)st * B, f.emb_mask ? f.emb_mask + (size_t)st * B * E : nullptr, x0, B, E, XI, V);
    ASTK_LAUNCH_CHECK();
    DecStepBufs b;
    memset(&b, 0, sizeof(b));
    b.x0 = x0;
    for (int l = 0; l < nl; ++l)
      b.layer[l] = {P.C[l] + (size_t)st * bh, P.HR[l] + (size_t)st * bh, f.rnn_masks ? f.rnn_masks + ((size_t)l * S + st) * bh : nullptr,
                    P.C[l] + (size_t)(st + 1) * bh, P.HR[l] + (size_t)(st + 1) * bh, P.G[l] + (size_t)st * B * 4 * H,
                    P.HD[l] + (size_t)st * bh, P.HDL[l] + (size_t)st * bh};
    for (int k = 0; k < NA; ++k) {
      b.q[k] = P.Q + ((size_t)k * S + st) * bh;
      b.alpha[k] = P.ALPHA + ((size_t)k * S + st) * B * P.Tp;
    }
    b.cvh = P.CVH + (size_t)st * B * CW;
    float* ht = P.HT + (size_t)(st + 1) * B * A;      // HT[st+1] and (input feeding) the next step's concat buffer
    b.ht = ht;
    if (P.feed && st + 1 < S) { b.ht2 = P.X0 + (size_t)(st + 1) * B * XI + E; b.ld_ht2 = XI; }
    ASTK_TRY(step_fwd(P, prm, f.enc, b, s));
    // logits, dropout on the logits (seq2seq.py:394: argmax feedback and loss see the dropped logits; the gradient passes the same mask),
    // softmax cross-entropy.  With the caller's host copy of the flags only the steps whose argmax is FED BACK compute their logits
    // inside the loop (into a scratch panel, argmax only); every step is scored by one product and one launch behind the loop.
    const float* om = f.out_mask ? f.out_mask + (size_t)st * B * V : nullptr;
    const bool fed_back = st + 1 < S && (!uth || uth[st + 1] == 0);
    if (!uth || fed_back) {
      float* lg = uth ? P.LG1 : P.LOGITS + (size_t)st * B * P.Vp;
      RowGemmArgs a = rg(B, V, ht, A, prm->Wo, A, A, lg, P.Vp);
      a.bias = prm->bo;
      ASTK_TRY(rowgemm_launch(a, s));
      if (om) ASTK_TRY(mul_rows_launch(lg, P.Vp, om, V, B, V, s));
      if (uth) {
        hipLaunchKernelGGL(k_softmax_ce, dim3(B), dim3(256), 0, s, V, (long)P.Vp, lg, f.tgt + st + 1, (long)P.L, B, (const float*)nullptr, 1.f,
                           0.f, (float*)nullptr, P.PRED + (size_t)st * B, 1, (const int32_t*)nullptr, 0, (const float*)nullptr);
        ASTK_LAUNCH_CHECK();
      } else {
        ASTK_TRY(softmax_ce_launch(B, V, P.Vp, lg, f.tgt + st + 1, P.L, prm->class_weight, inv_count, f.d->label_smoothing, P.LOSSROWS + (size_t)st * B,
                                  P.PRED + (size_t)st * B, s, f.row_weight));
        if (om) ASTK_TRY(mul_rows_launch(lg, P.Vp, om, V, B, V, s));
      }
    }
  }
  return uth ? fwd_score_all(f, P) : 0;
}

// ---- backward.  astk_decoder_bwd_phase_ex validates, routes and handles the split; the chain phase is bwd_chain (a common head, one of
// bwd_chain_persist / bwd_chain_wide / bwd_chain_steps, a common tail), the parameter phase bwd_params.
struct DecBwdCall {
  const astk_decoder_desc* d; const astk_decoder_params* prm; const astk_decoder_grads* g;
  const float *enc, *emb_mask, *rnn_masks;
  float *d_enc, *d_c0, *d_h0;
  int phase;
  hipStream_t s;
};

// the two halves the forward call ran (their masks are still staged in the workspace)
int bwd_split(const DecBwdCall& b, const SplitPlan& sp) {
  const astk_decoder_desc* d = b.d;
  if (b.phase != ASTK_DEC_BWD_PARAMS && d->zero_ptr && d->zero_bytes) ASTK_TRY(fill_zero(d->zero_ptr, d->zero_bytes, b.s));   // (once, in front of both halves)
  const int B = d->B, H = d->H, nl = d->n_layers;
  for (int i = 0; i < 2; ++i) {
    const int bi = sp.sub[i].B, off = sp.off[i];
    ASTK_TRY(astk_decoder_bwd_phase_ex(&sp.sub[i], b.prm, b.g, b.enc + (size_t)off * d->T * H, sp.c0[i], sp.h0[i], nullptr, b.emb_mask ? sp.emb[i] : nullptr,
                                       b.rnn_masks ? sp.rnn[i] : nullptr, nullptr, b.d_enc + (size_t)off * d->T * H, sp.dc0[i], sp.dh0[i], sp.ws[i], sp.wsb[i],
                                       b.phase, b.s));
    if (b.phase != ASTK_DEC_BWD_PARAMS) {
      ASTK_TRY(copy2d_f32(b.d_c0 + (size_t)off * H, (long)B * H, sp.dc0[i], (long)bi * H, nl, bi * H, bi * H, b.s));
      ASTK_TRY(copy2d_f32(b.d_h0 + (size_t)off * H, (long)B * H, sp.dh0[i], (long)bi * H, nl, bi * H, bi * H, b.s));
    }
  }
  return 0;
}

// the persistent loop: the whole reversed loop in one launch, whose fill takes zero_ptr and d_enc along
int bwd_chain_persist(const DecBwdCall& b, const DecPlan& P, const DecRoute& r) {
  return decoder_persist_bwd_launch(b.d, b.enc, b.rnn_masks, persist_bwd_buffers(P, b.d, r, b.d_enc, b.d_c0), b.s);
}

// d_pre = (dlogits Wo + d_ht carried from step st+1 through input feeding) * (1 - ht^2).  dlogits Wo does not depend on the recurrence:
// ONE product over all S*B rows (K = V; as a per-step row panel it is 2*ceil(B/16)*A/16 workgroups walking K = V each), then tanh' on
// the rows that take no carry -- the last step, or every step without input feeding; the others get carry and tanh' from the epilogue
// of step st+1's d_x0 product (RowGemmArgs::carry), in the wide loop from the kernel.
int bwd_dpre_linear(const DecBwdCall& b, const DecPlan& P) {
  const int B = P.B, S = P.S, A = P.A;
  ASTK_TRY(gemm_launch(GEMM_NN, gemm_args(S * B, A, P.V, mat(P.LOGITS, P.Vp), mat(b.prm->Wo, A), P.DPRE, A), b.s));
  const long r0 = P.feed ? (long)(S - 1) * B * A : 0, n = (long)S * B * A - r0;
  hipLaunchKernelGGL(k_dtanh_inplace, dim3((unsigned)std::min<long>(cdiv(n, 256), 2048)), dim3(256), 0, b.s, P.DPRE + r0, P.HT + (size_t)B * A + r0, n);
  ASTK_LAUNCH_CHECK();
  return 0;
}

// the wide loop: the whole reversed loop in one launch (decoder_wide.hip)
int bwd_chain_wide(const DecBwdCall& b, const DecPlan& P) {
  ASTK_TRY(bwd_dpre_linear(b, P));
  return decoder_wide_bwd_launch(b.d, b.enc, b.rnn_masks, wide_bwd_buffers(P), b.s);
}

// the per-launch reversed loop
int bwd_chain_steps(const DecBwdCall& b, const DecPlan& P) {
  const astk_decoder_params* prm = b.prm;
  const astk_decoder_grads* g = b.g;
  hipStream_t s = b.s;
  const int B = P.B, S = P.S, H = P.H, E = P.E, A = P.A, XI = P.XI, nl = P.nl, T = P.T, Tp = P.Tp, NA = P.NA, CW = P.CW;
  const size_t bh = (size_t)B * H;
  const int top = nl - 1;
  ASTK_TRY(bwd_dpre_linear(b, P));
  for (int st = S - 1; st >= 0; --st) {
    const bool last = st == S - 1;
    float* dpre = P.DPRE + (size_t)st * B * A;
    float* dcvh = P.DCVH + (size_t)st * B * CW;
    ASTK_TRY(rowgemm_launch(rg(B, CW, dpre, A, P.WcT, A, A, dcvh, CW), s));
    float* cvh = P.CVH + (size_t)st * B * CW;
    for (int k = 0; k < NA; ++k)
      ASTK_TRY(attn_bwd_launch(B, T, H, b.enc, P.ALPHA + ((size_t)k * S + st) * B * Tp, cvh + (size_t)k * H, CW, dcvh + (size_t)k * H, CW,
                               P.DS + ((size_t)k * S + st) * B * Tp, P.DQ + ((size_t)k * S + st) * bh, P.attn_ws, s));
    // gradient wrt the top layer's output: dh_top = dcvh[:, NA*H:] + sum_k dq_k Wa_k   (two heads per row-panel launch)
    const float* add = dcvh + (size_t)NA * H;
    long ld_add = CW;
    float* outb = P.DHTOP;
    for (int k = 0; k < NA; k += 2) {
      RowGemmArgs a = rg(B, H, P.DQ + ((size_t)k * S + st) * bh, H, P.WaT + (size_t)k * H * H, H, H, outb, H);
      if (k + 1 < NA) {
        a.npairs = 2;
        a.p[1].A = P.DQ + ((size_t)(k + 1) * S + st) * bh; a.p[1].lda = H; a.p[1].W = P.WaT + (size_t)(k + 1) * H * H; a.p[1].ldw = H; a.p[1].K = H;
      }
      a.addend = add;
      a.ld_add = ld_add;
      ASTK_TRY(rowgemm_launch(a, s));
      add = outb; ld_add = H;
      outb = outb == P.DHTOP ? P.DLN2 : P.DHTOP;       // (a launch never adds into the buffer it reads)
    }
    if (add != P.DHTOP) ASTK_TRY(copy_f32(P.DHTOP, add, bh, s));
    for (int l = top; l >= 0; --l) {
      LstmCellBwdArgs c;
      memset(&c, 0, sizeof(c));
      c.npairs = 1;
      c.p[0].A = last ? nullptr : P.G[l] + (size_t)(st + 1) * B * 4 * H;
      c.p[0].lda = 4 * H; c.p[0].W = P.WlT[l]; c.p[0].ldw = 4 * H; c.p[0].K = last ? 0 : 4 * H;
      if (P.ln) {
        // gradient wrt the LayerNorm's output (top: dh_top; below: dz_{l+1,st} Wu_{l+1}) -> through the LayerNorm -> the cell's dropped output
        const float* dout = P.DHTOP;
        if (l < top) {
          ASTK_TRY(rowgemm_launch(rg(B, H, P.G[l + 1] + (size_t)st * B * 4 * H, 4 * H, P.WuT[l + 1], 4 * H, 4 * H, P.DLN, H), s));
          dout = P.DLN;
        }
        ASTK_TRY(layernorm_bwd_launch(B, H, P.HDL[l] + (size_t)st * bh, H, prm->ln_gamma[l], LN_EPS, dout, H, P.DLN2, H, g->d_ln_gamma[l],
                                      g->d_ln_beta[l], s));
        c.dy = P.DLN2;
        c.ld_dy = H;
      } else if (l < top) {   // gradient from the layer above at the same step: dz_{l+1,st} Wu_{l+1}
        c.npairs = 2;
        c.p[1].A = P.G[l + 1] + (size_t)st * B * 4 * H;
        c.p[1].lda = 4 * H; c.p[1].W = P.WuT[l + 1]; c.p[1].ldw = 4 * H; c.p[1].K = 4 * H;
      } else {
        c.dy = P.DHTOP;
        c.ld_dy = H;
      }
      c.B = B; c.h = H;
      c.mask = b.rnn_masks ? b.rnn_masks + ((size_t)l * S + st) * bh : nullptr;
      c.dc_next = last ? nullptr : P.DC[l][(st + 1) & 1];
      c.c_prev = P.C[l] + (size_t)st * bh;
      c.c_cur = P.C[l] + (size_t)(st + 1) * bh;
      c.gates_dz = P.G[l] + (size_t)st * B * 4 * H;
      c.ld_g = 4 * H;
      c.dc_prev = P.DC[l][st & 1];
      ASTK_TRY(lstm_cell_bwd_launch(&c, 1, s));
    }
    // gradient wrt the layer-0 input [emb ; ht_{st-1}] (or the embedding alone)
    RowGemmArgs a = rg(B, XI, P.G[0] + (size_t)st * B * 4 * H, 4 * H, P.WuT[0], 4 * H, 4 * H, P.DX0 + (size_t)st * B * XI, XI);
    if (P.feed && st > 0) {     // columns E.. are d_ht of step st-1: finish that step's d_pre in place
      a.carry = P.DPRE + (size_t)(st - 1) * B * A; a.ld_carry = A;
      a.carry_aux = P.HT + (size_t)st * B * A; a.ld_carry_aux = A;
      a.carry_col0 = E;
    }
    ASTK_TRY(rowgemm_launch(a, s));
  }
  return 0;
}

// the chain phase: everything the encoder's backward needs (d_enc, d_c0, d_h0), and the per-step gradients the parameter phase reads
int bwd_chain(const DecBwdCall& b, const DecPlan& P, const DecRoute& r) {
  const astk_decoder_desc* d = b.d;
  const astk_decoder_params* prm = b.prm;
  hipStream_t s = b.s;
  const int B = P.B, H = P.H, A = P.A, V = P.V, Vp = P.Vp, XI = P.XI, nl = P.nl, NA = P.NA, CW = P.CW;
  const size_t bh = (size_t)B * H;
  const bool persist = r.path == DEC_PERSIST;
  // astk_decoder_desc.zero_ptr (the gradient arena): in front of everything this call accumulates -- the persistent launcher's fill takes
  // it along (nothing in front of that launch touches the gradients), every other path fills here
  if (d->zero_ptr && d->zero_bytes) {
    ASTK_CHECK(aligned16(d->zero_ptr) && (d->zero_bytes % 4) == 0, "decoder_bwd: zero_ptr must be 16-byte aligned, zero_bytes a multiple of 4");
    if (!persist) ASTK_TRY(fill_zero(d->zero_ptr, d->zero_bytes, s));
  }
  // transposed weights for the data-path products (dY W as row-panel NT products)
  TransposeJobs tj;
  tj.n = 0;
  if (persist) transpose_add(tj, P.WoT, Vp, prm->Wo, A, V, A);          // (V,A) -> (A,Vp); the other paths batch dlogits Wo over the steps
  transpose_add(tj, P.WcT, A, prm->Wc, CW, A, CW);         // (A,CW) -> (CW,A)
  for (int k = 0; k < NA; ++k) transpose_add(tj, P.WaT + (size_t)k * H * H, H, k == 0 ? prm->Wa : prm->Wa_x[k - 1], H, H, H);
  for (int l = 0; l < nl; ++l) {
    const int in = l == 0 ? XI : H;
    if (tj.n + 2 > FILL_SEG_MAX) { ASTK_TRY(transpose_batch(tj, s)); tj.n = 0; }
    transpose_add(tj, P.WuT[l], 4 * H, prm->lstm[l].Wu, in, 4 * H, in);   // (4H,in) -> (in,4H)
    transpose_add(tj, P.WlT[l], 4 * H, prm->lstm[l].Wl, H, 4 * H, H);     // (4H,H)  -> (H,4H)
  }
  ASTK_TRY(transpose_batch(tj, s));
  if (!persist) ASTK_TRY(attn_ws_init(P.attn_ws, B, P.T, H, s));   // the persistent loop has its own counters
  switch (r.path) {
    case DEC_PERSIST: ASTK_TRY(bwd_chain_persist(b, P, r)); break;
    case DEC_WIDE: ASTK_TRY(bwd_chain_wide(b, P)); break;
    case DEC_PER_LAUNCH: ASTK_TRY(bwd_chain_steps(b, P)); break;
  }
  // ---- gradients wrt the initial states (flow into the encoder's final states, seq2seq.py:326-329)
  for (int l = 0; l < nl; ++l) {
    ASTK_TRY(rowgemm_launch(rg(B, H, P.G[l], 4 * H, P.WlT[l], 4 * H, 4 * H, b.d_h0 + l * bh, H), s));
    if (!persist) ASTK_TRY(copy_f32(b.d_c0 + l * bh, P.DC[l][0], bh, s));      // (the persistent kernel wrote d_c0 itself)
  }
  // ---- d_enc[b] = sum_k alpha_k,b^T d_cv_k,b + ds_k,b^T q_k,b   (batched over b, K = S).  The persistent launcher's fill zeroed d_enc: both
  // products of every head ADD into it, all of them in ONE grouped launch (two 18-us launches of three k-iterations each were one after
  // the other on the backward's chain; two contributions per element: the same sum in either order).  The other paths: a launch each.
  static_assert(2 * ASTK_MAX_ATTN <= GEMM_GROUP_MAX, "d_enc: one grouped launch holds both products of every head");
  const int T = P.T, Tp = P.Tp, S = P.S;
  GemmArgs list[2 * ASTK_MAX_ATTN];
  for (int k = 0; k < NA; ++k) {
    GemmArgs& ga = list[2 * k] = gemm_args(T, H, S, mat(P.ALPHA + (size_t)k * S * B * Tp, (long)B * Tp), mat(P.DCVH + (size_t)k * H, (long)B * CW), b.d_enc, H,
                                           nullptr, persist ? GEMM_ATOMIC : (k == 0 ? GEMM_STORE : GEMM_ACCUM));
    ga.batch = B; ga.sA = Tp; ga.sB = CW; ga.sC = (long)T * H;
    GemmArgs& gb = list[2 * k + 1] = gemm_args(T, H, S, mat(P.DS + (size_t)k * S * B * Tp, (long)B * Tp), mat(P.Q + (size_t)k * S * bh, (long)B * H), b.d_enc, H,
                                               nullptr, persist ? GEMM_ATOMIC : GEMM_ACCUM);
    gb.batch = B; gb.sA = Tp; gb.sB = H; gb.sC = (long)T * H;
  }
  if (persist) return gemm_launch_group(GEMM_TN, list, 2 * NA, s);
  for (int i = 0; i < 2 * NA; ++i) ASTK_TRY(gemm_launch(GEMM_TN, list[i], s));
  return 0;
}

// ==== parameter gradients: read only what the chain phase left in the workspace; nothing downstream of the decoder needs them, so a
// caller may run this phase on a second stream beside the encoder's backward recurrence (ASTK_DEC_BWD_PARAMS)
int bwd_params(const DecBwdCall& b, const DecPlan& P, const DecRoute& r) {
  const astk_decoder_params* prm = b.prm;
  const astk_decoder_grads* g = b.g;
  hipStream_t s = b.s;
  const int B = P.B, S = P.S, H = P.H, E = P.E, A = P.A, V = P.V, Vp = P.Vp, XI = P.XI, nl = P.nl, T = P.T, Tp = P.Tp, NA = P.NA, CW = P.CW;
  const size_t bh = (size_t)B * H;
  GemmWgCap cap(b.phase == ASTK_DEC_BWD_PARAMS ? b.d->side_wgs : 0);   // on its own stream this phase shares the CUs with the encoder's recurrence kernel
  // ---- what the persistent kernels left to this phase.  The embedding columns of d_x0 (only the embedding scatter reads them; K18's input
  // gradient): one batched product over all steps, for the wide loop and for the persistent loop's split d_x0 phase
  // fp16-operand mode: the gradient operands of the eligible products -- dlogits (K24) and every cell's dz (K18; layer 0's also feeds gx)
  // -- go in behind their measured scale: one maximum pass over all of them here (null handles outside that mode: nothing is launched).
  // dlogits are 1 / B at most and about 1 / (B V) elsewhere, dz smaller still: cast as they are they sit on fp16's subnormals.
  const unsigned long long* a_dz[ASTK_MAX_RNN_LAYERS + 1];      // [nl]: dlogits
  {
    AmaxMatrix am[ASTK_MAX_RNN_LAYERS + 1];
    for (int l = 0; l < nl; ++l) am[l] = AmaxMatrix{low_precision_gemms() ? P.G[l] : nullptr, (long)S * B, 4L * H, 4 * H};
    am[nl] = AmaxMatrix{low_precision_gemms() ? P.LOGITS : nullptr, (long)S * B, (long)Vp, V};
    gemm_amax_many(am, nl + 1, a_dz, s);
  }
  const GemmArgs gx = with_amax_a(lowp(gemm_args(S * B, E, 4 * H, mat(P.G[0], 4 * H), mat(prm->lstm[0].Wu, XI), P.DX0, XI)), a_dz[0]);
  if (r.path == DEC_WIDE) ASTK_TRY(gemm_launch(GEMM_NN, gx, s));
  if (r.path == DEC_PERSIST) {
    // dq[s][b][:] = sum_t ds[s][b][t] enc[b][t][:]  (batched over b) -- only the weight gradients of attn_Wa need it
    GemmArgs gq = gemm_args(S, H, T, mat(P.DS, (long)B * Tp), mat(b.enc, H), P.DQ, (long)B * H);
    gq.batch = B; gq.sA = Tp; gq.sB = (long)T * H; gq.sC = H;
    if (r.b6_split && low_precision_gemms() == 0) {      // two small independent NN products: one grouped launch (a launch less on the way to the weight gradients)
      const GemmArgs two[2] = {gx, gq};
      ASTK_TRY(gemm_launch_group(GEMM_NN, two, 2, s));
    } else {
      if (r.b6_split) ASTK_TRY(gemm_launch(GEMM_NN, gx, s));
      ASTK_TRY(gemm_launch(GEMM_NN, gq, s));
    }
  }
  // ---- weight gradients: one batched TN GEMM each over the S*B saved rows
  const int SB = S * B;
  // BASELINE configs[4] ("fp16 MFMA GEMMs"; SURVEY 8d: fp16 operands for K6, K9, K18, K24): the batched products of the decoder LSTMs (K18)
  // and of the output layer (K24) form their own grouped launch, eligible for fp16 operands under astk_set_low_precision_gemms(1);
  // attention and context products stay f32-accurate.  (Without that mode both groups run exactly as one did.)
  WgradBatch wb, wbl(true);
  ColsumBatch cb;   // the bias gradients: one launch
  ASTK_TRY(wbl.add(g->dWo, A, V, A, P.LOGITS, Vp, P.HT + (size_t)B * A, A, SB, s, a_dz[nl]));
  ASTK_TRY(cb.add(g->dbo, P.LOGITS, Vp, SB, V, s));
  ASTK_TRY(wb.add(g->dWc, CW, A, CW, P.DPRE, A, P.CVH, CW, SB, s));
  ASTK_TRY(cb.add(g->dbc, P.DPRE, A, SB, A, s));
  for (int k = 0; k < NA; ++k) {
    float* dWa = k == 0 ? g->dWa : g->dWa_x[k - 1];
    float* dba = k == 0 ? g->dba : g->dba_x[k - 1];
    ASTK_CHECK(dWa && dba, "decoder_bwd: attention head %d has no gradient buffers", k);
    ASTK_TRY(wb.add(dWa, H, H, H, P.DQ + (size_t)k * S * bh, H, P.CVH + (size_t)NA * H, CW, SB, s));
    ASTK_TRY(cb.add(dba, P.DQ + (size_t)k * S * bh, H, SB, H, s));
  }
  for (int l = 0; l < nl; ++l) {
    const int in = l == 0 ? XI : H;
    const float* xin;
    long ldx;
    if (l == 0) { xin = P.X0; ldx = XI; }
    else if (b.rnn_masks || P.ln) { xin = P.HD[l - 1]; ldx = H; }       // (with LayerNorm the layer's input is always the normalised copy)
    else { xin = P.HR[l - 1] + bh; ldx = H; }
    ASTK_TRY(wbl.add(g->lstm[l].dWu, in, 4 * H, in, P.G[l], 4 * H, xin, ldx, SB, s, a_dz[l]));
    ASTK_TRY(wbl.add(g->lstm[l].dWl, H, 4 * H, H, P.G[l], 4 * H, P.HR[l], H, SB, s, a_dz[l]));
    ASTK_TRY(cb.add(g->lstm[l].db, P.G[l], 4 * H, SB, 4 * H, s));
  }
  ASTK_TRY(cb.flush(s));
  if (low_precision_gemms()) {
    ASTK_TRY(wb.flush(s));
    ASTK_TRY(wbl.flush(s));
  } else {            // one grouped launch, as before the two were told apart
    for (int i = 0; i < wbl.n; ++i) {
      if (wb.n == GEMM_GROUP_MAX) ASTK_TRY(wb.flush(s));
      wb.list[wb.n++] = wbl.list[i];
    }
    wbl.n = 0;
    ASTK_TRY(wb.flush(s));
  }
  if (deterministic_mode()) hipLaunchKernelGGL(k_embed_bwd_det, dim3(V), dim3(128), 0, s, g->d_embed, P.TOK, P.DX0, b.emb_mask, SB, E, XI, V);
  else hipLaunchKernelGGL(k_embed_bwd, dim3(SB), dim3(128), 0, s, g->d_embed, P.TOK, P.DX0, b.emb_mask, SB, E, XI, V);
  ASTK_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int softmax_ce_launch(int B, int V, long ld, float* logits, const int32_t* targets, long t_stride, const float* cw, float inv_count,
                      float eps, float* loss_rows, int32_t* argmax, hipStream_t s, const float* row_weight) {
  ASTK_CHECK(B > 0 && V > 0 && ld >= V && logits && targets, "softmax_ce: bad arguments");
  ASTK_CHECK(label_smoothing_ok(eps), "softmax_ce: label_smoothing %g (finite, 0 <= eps < 1)", (double)eps);
  hipLaunchKernelGGL(k_softmax_ce, dim3(B), dim3(256), 0, s, V, ld, logits, targets, t_stride, B, cw, inv_count, eps, loss_rows, argmax, 0,
                     (const int32_t*)nullptr, 0, row_weight);
  ASTK_LAUNCH_CHECK();
  return 0;
}

}  // namespace astk

using namespace astk;

extern "C" {

int astk_decoder_path(const astk_decoder_desc* d) {
  if (!d || d->struct_size != sizeof(astk_decoder_desc)) return 0;
  const DecRoute r = dec_route(d, false);
  if (r.split) {      // two launches over halves of the rows: bit 2 beside the path of a half (a descriptor no call accepts has none)
    astk_decoder_desc half = *d;
    half.B = r.B0;
    return dec_validate(d) != 0 ? 0 : (astk_decoder_path(&half) | 4);
  }
  if (r.path == DEC_WIDE) return 16;      // wide loops (decoder_wide.hip)
  if (r.path != DEC_PERSIST) return 0;
  return 1 | (r.special ? 2 : 0) | (d->n_layers << 8);
}

size_t astk_decoder_workspace_bytes(const astk_decoder_desc* d) {
  if (dec_validate(d) != 0) return 0;
  const DecRoute r = dec_route(d, false);
  DecPlan P;
  make_plan(d, r, nullptr, P);
  if (r.split) {
    SplitPlan sp;
    make_split(d, r, nullptr, sp);
    if (sp.bytes > P.bytes) return sp.bytes;      // (a call with an out_mask keeps the per-launch layout: the larger of the two)
  }
  return P.bytes;
}

int astk_softmax_ce_fwd(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride, const float* class_weight,
                        float inv_count, float* loss_rows, int32_t* argmax, void* stream) {
  return astk_softmax_ce_fwd_ex(B, V, ld, logits_inout, targets, t_stride, class_weight, inv_count, 0.f, loss_rows, argmax, stream);
}

int astk_softmax_ce_fwd_ex(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride, const float* class_weight,
                           float inv_count, float label_smoothing, float* loss_rows, int32_t* argmax, void* stream) {
  return astk_softmax_ce_fwd_w(B, V, ld, logits_inout, targets, t_stride, class_weight, nullptr, inv_count, label_smoothing, loss_rows, argmax,
                               stream);
}

int astk_softmax_ce_fwd_w(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride, const float* class_weight,
                          const float* row_weight, float inv_count, float label_smoothing, float* loss_rows, int32_t* argmax, void* stream) {
  return softmax_ce_launch(B, V, ld, logits_inout, targets, t_stride, class_weight, inv_count, label_smoothing, loss_rows, argmax,
                           (hipStream_t)stream, row_weight);
}

int astk_decoder_fwd(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                     const int32_t* y, const int32_t* use_truth, const float* emb_mask, const float* rnn_masks, float* loss,
                     int32_t* pred, void* ws, size_t ws_bytes, void* stream) {
  return astk_decoder_fwd_ex(d, prm, enc, c0, h0, y, use_truth, emb_mask, rnn_masks, nullptr, nullptr, loss, pred, ws, ws_bytes, stream);
}

int astk_decoder_fwd_ex(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                        const int32_t* y, const int32_t* use_truth, const float* emb_mask, const float* rnn_masks, const float* out_mask,
                        const int32_t* targets, float* loss, int32_t* pred, void* ws, size_t ws_bytes, void* stream) {
  return astk_decoder_fwd_w(d, prm, enc, c0, h0, y, use_truth, emb_mask, rnn_masks, out_mask, targets, nullptr, loss, pred, ws, ws_bytes, stream);
}

int astk_decoder_fwd_w(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                       const int32_t* y, const int32_t* use_truth, const float* emb_mask, const float* rnn_masks, const float* out_mask,
                       const int32_t* targets, const float* row_weight, float* loss, int32_t* pred, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  PrecScope prec_scope(d->precision, d->gemm_operands);
  GemmForwardScope forward_scope;      // split tiles of this op's products have at most two contributors (reproducible forward pass)
  ASTK_TRY(dec_validate(d));
  const DecRoute r = dec_route(d, out_mask != nullptr);
  SplitPlan sp;
  DecPlan P;
  if (r.split) make_split(d, r, ws, sp);
  else make_plan(d, r, ws, P);
  const size_t need = r.split ? sp.bytes : P.bytes;
  ASTK_CHECK(ws && ws_bytes >= need, "decoder_fwd: workspace too small (%zu < %zu)", ws_bytes, need);
  ASTK_CHECK(prm && enc && c0 && h0 && y && use_truth && loss, "decoder_fwd: null pointer");
  const DecFwdCall f = {d, prm, enc, c0, h0, y, use_truth, emb_mask, rnn_masks, out_mask, targets, targets ? targets : y, row_weight, loss, pred, s};
  const float* loss_parts;      // what the tail sums
  int n_parts;
  if (r.split) {
    ASTK_TRY(fwd_split(f, sp));      // (each half copied its predictions)
    loss_parts = sp.loss2;
    n_parts = 2;
  } else {
    path_record(ws, r.path);
    if (r.path == DEC_PERSIST) return fwd_persist(f, P);      // (the launch is its own tail)
    ASTK_TRY(r.path == DEC_WIDE ? fwd_wide(f, P) : fwd_steps(f, P));
    loss_parts = P.LOSSROWS;
    n_parts = P.S * P.B;
  }
  // the tail: loss sum, predictions out of the workspace, status snapshot
  hipLaunchKernelGGL(k_sum_to, dim3(1), dim3(256), 0, s, loss_parts, n_parts, loss);
  ASTK_LAUNCH_CHECK();
  if (pred && !r.split) {
    hipLaunchKernelGGL(k_copy_i32, dim3(cdiv(n_parts, 256)), dim3(256), 0, s, pred, P.PRED, n_parts);
    ASTK_LAUNCH_CHECK();
  }
  // status_dst: the persistent loop's scoring kernel wrote it; every other path takes the snapshot with a launch behind the op
  if (d->status_dst) ASTK_TRY(status_snapshot_launch(d->status_dst, s));
  return 0;
}

int astk_decoder_bwd(const astk_decoder_desc* d, const astk_decoder_params* prm, const astk_decoder_grads* g, const float* enc,
                     const float* c0, const float* h0, const int32_t* y, const float* emb_mask, const float* rnn_masks, float* d_enc,
                     float* d_c0, float* d_h0, void* ws, size_t ws_bytes, void* stream) {
  return astk_decoder_bwd_phase_ex(d, prm, g, enc, c0, h0, y, emb_mask, rnn_masks, nullptr, d_enc, d_c0, d_h0, ws, ws_bytes, ASTK_DEC_BWD_ALL, stream);
}

int astk_decoder_bwd_phase(const astk_decoder_desc* d, const astk_decoder_params* prm, const astk_decoder_grads* g, const float* enc,
                           const float* c0, const float* h0, const int32_t* y, const float* emb_mask, const float* rnn_masks,
                           float* d_enc, float* d_c0, float* d_h0, void* ws, size_t ws_bytes, int phase, void* stream) {
  return astk_decoder_bwd_phase_ex(d, prm, g, enc, c0, h0, y, emb_mask, rnn_masks, nullptr, d_enc, d_c0, d_h0, ws, ws_bytes, phase, stream);
}

int astk_decoder_bwd_phase_ex(const astk_decoder_desc* d, const astk_decoder_params* prm, const astk_decoder_grads* g, const float* enc,
                              const float* c0, const float* h0, const int32_t* y, const float* emb_mask, const float* rnn_masks,
                              const float* out_mask, float* d_enc, float* d_c0, float* d_h0, void* ws, size_t ws_bytes, int phase,
                              void* stream) {
  (void)c0; (void)h0; (void)y;
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  PrecScope prec_scope(d->precision, d->gemm_operands);
  DetScope det_scope(d->deterministic);
  ASTK_CHECK(phase == ASTK_DEC_BWD_ALL || phase == ASTK_DEC_BWD_CHAIN || phase == ASTK_DEC_BWD_PARAMS, "decoder_bwd: bad phase %d", phase);
  // the fix-up workspace of the deterministic split tiles serves one launch at a time: a capped phase is one that runs beside other launches
  ASTK_CHECK(!(deterministic_mode() && d->side_wgs > 0), "decoder_bwd: `deterministic` (the field, or the process default gemm.deterministic) and `side_wgs` = %d "
             "exclude each other: deterministic calls run on one stream (astk.h)", d->side_wgs);
  ASTK_TRY(dec_validate(d));
  const DecRoute r = dec_route(d, out_mask != nullptr);
  SplitPlan sp;
  DecPlan P;
  if (r.split) make_split(d, r, ws, sp);
  else make_plan(d, r, ws, P);
  ASTK_CHECK(ws && ws_bytes >= (r.split ? sp.bytes : P.bytes), "decoder_bwd: workspace too small");
  ASTK_CHECK(prm && g && enc && d_enc && d_c0 && d_h0, "decoder_bwd: null pointer");
  const DecBwdCall b = {d, prm, g, enc, emb_mask, rnn_masks, d_enc, d_c0, d_h0, phase, (hipStream_t)stream};
  if (r.split) return bwd_split(b, sp);
  const int fwd_path = path_lookup(ws);
  ASTK_CHECK(fwd_path < 0 || fwd_path == r.path, "decoder_bwd: the forward call on this workspace took kernel path %d, this call would take %d "
             "(the dec.persist / dec.wide knobs changed between the two calls?)", fwd_path, (int)r.path);
  if (phase != ASTK_DEC_BWD_PARAMS) ASTK_TRY(bwd_chain(b, P, r));
  if (phase != ASTK_DEC_BWD_CHAIN) ASTK_TRY(bwd_params(b, P, r));
  return 0;
}

int astk_decoder_step_infer(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, float* c, float* h, float* ht,
                            const int32_t* tokens, float* logits, float* alpha, int32_t* argmax, void* ws, size_t ws_bytes,
                            void* stream) {
  DecStepIO io;
  memset(&io, 0, sizeof(io));
  io.enc = enc; io.c = c; io.h = h; io.ht_in = ht; io.ht_out = ht; io.tokens = tokens; io.logits = logits; io.alpha = alpha;
  io.argmax = argmax; io.states_in_place = true;
  return decoder_step_run(d, prm, io, ws, ws_bytes, (hipStream_t)stream);
}

size_t astk_greedy_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return greedy_workspace_bytes(d, stop_limit); }

int astk_greedy_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                       int go, int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst,
                       void* ws, size_t ws_bytes, void* stream) {
  return greedy_decode_launch(d, p, enc, c0, h0, go, eos, stop_limit, tokens, n_steps, status_dst, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int astk_greedy_decode_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst,
                            void* ws, size_t ws_bytes, void* stream, const int32_t* row_len) {
  return greedy_decode_launch(d, p, enc, c0, h0, go, eos, stop_limit, tokens, n_steps, status_dst, ws, ws_bytes, row_len, (hipStream_t)stream);
}

size_t astk_greedy_scored_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return greedy_scored_workspace_bytes(d, stop_limit); }

int astk_greedy_decode_scored(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                              int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight, int32_t* tokens,
                              float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream) {
  return greedy_decode_scored_launch(d, p, enc, c0, h0, go, eos, stop_limit, y, ldy, class_weight, tokens, logp, nll, n_steps, status_dst, ws,
                                     ws_bytes, nullptr, (hipStream_t)stream);
}

int astk_greedy_decode_scored_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0,
                                   const float* h0, int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight,
                                   int32_t* tokens, float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws,
                                   size_t ws_bytes, void* stream, const int32_t* row_len) {
  return greedy_decode_scored_launch(d, p, enc, c0, h0, go, eos, stop_limit, y, ldy, class_weight, tokens, logp, nll, n_steps, status_dst, ws,
                                     ws_bytes, row_len, (hipStream_t)stream);
}

size_t astk_sample_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return sample_workspace_bytes(d, stop_limit); }

int astk_sample_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                       int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp,
                       int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream) {
  return sample_decode_launch(d, p, enc, c0, h0, go, eos, stop_limit, row_keys, inv_temp, tokens, logp, n_steps, status_dst, ws, ws_bytes,
                              nullptr, (hipStream_t)stream);
}

int astk_sample_decode_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp,
                            int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream, const int32_t* row_len) {
  return sample_decode_launch(d, p, enc, c0, h0, go, eos, stop_limit, row_keys, inv_temp, tokens, logp, n_steps, status_dst, ws, ws_bytes,
                              row_len, (hipStream_t)stream);
}

size_t astk_sample_topk_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return sample_topk_workspace_bytes(d, stop_limit); }

int astk_sample_decode_topk(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int top_k, float top_p,
                            int32_t* tokens, float* logp, int32_t* n_kept, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                            void* stream, const int32_t* row_len) {
  return sample_decode_topk_launch(d, p, enc, c0, h0, go, eos, stop_limit, row_keys, inv_temp, top_k, top_p, tokens, logp, n_kept, n_steps,
                                   status_dst, ws, ws_bytes, row_len, (hipStream_t)stream);
}

int astk_gumbel_rows(const uint64_t* row_keys, int B, int step, int V, float* out, void* stream) {
  return gumbel_rows_launch(row_keys, B, step, V, out, (hipStream_t)stream);
}

uint64_t astk_sample_row_key(uint64_t seed, uint64_t stream) { return sample_row_key(seed, stream); }

size_t astk_forced_workspace_bytes(const astk_decoder_desc* d, int n_steps, int with_alpha) {
  return forced_workspace_bytes(d, n_steps, with_alpha);
}

int astk_forced_score(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                      const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst, void* ws,
                      size_t ws_bytes, void* stream) {
  return forced_score_launch(d, p, enc, c0, h0, y, ldy, logp, logp_max, pred, alpha, status_dst, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int astk_forced_score_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                           const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst,
                           void* ws, size_t ws_bytes, void* stream, const int32_t* row_len) {
  return forced_score_launch(d, p, enc, c0, h0, y, ldy, logp, logp_max, pred, alpha, status_dst, ws, ws_bytes, row_len, (hipStream_t)stream);
}

size_t astk_beam_decode_workspace_bytes(const astk_decoder_desc* d, int N, int K, int stop_limit, int with_alpha) {
  return beam_decode_workspace_bytes(d, N, K, stop_limit, with_alpha);
}

int astk_beam_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                     const int32_t* row_len, int N, int K, int go, int eos, int stop_limit, int32_t* n_steps, float* status_dst, int32_t* hist,
                     int32_t* slot_status, double* score, float* c_fin, float* h_fin, float* ht_fin, float* alpha, void* ws, size_t ws_bytes,
                     void* stream) {
  return beam_decode_launch(d, p, enc, c0, h0, row_len, N, K, go, eos, stop_limit, n_steps, status_dst, hist, slot_status, score, c_fin, h_fin,
                            ht_fin, alpha, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"

namespace astk {

size_t decoder_step_ws_bytes(const astk_decoder_desc* d) {
  if (dec_validate(d) != 0) return 0;
  DecPlan P;
  make_plan(d, dec_route(d, false), nullptr, P);
  return P.bytes;
}

int decoder_step_run(const astk_decoder_desc* d, const astk_decoder_params* prm, DecStepIO& io, void* ws, size_t ws_bytes, hipStream_t s) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  PrecScope prec_scope(d->precision, d->gemm_operands);
  ASTK_TRY(dec_validate(d));
  DecPlan P;
  make_plan(d, dec_route(d, false), ws, P);      // (the training call's carve: one workspace size serves both)
  ASTK_CHECK(ws && ws_bytes >= P.bytes, "decoder_step_infer: workspace too small");
  ASTK_CHECK(prm && io.enc && io.c && io.h && io.ht_in && io.ht_out && io.tokens && io.logits, "decoder_step_infer: null pointer");
  const int B = P.B, E = P.E, A = P.A, V = P.V, XI = P.XI;
  const size_t bh = (size_t)B * P.H;
  ASTK_TRY(attn_ws_init(P.attn_ws, B, P.T, P.H, s));
  hipLaunchKernelGGL(k_embed, dim3(B), dim3(128), 0, s, prm->embed, (const int32_t*)nullptr, 0, 0, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, io.tokens, (int32_t*)nullptr, (const float*)nullptr, P.X0, B, E, XI, V);
  ASTK_LAUNCH_CHECK();
  if (P.feed) ASTK_TRY(copy2d_f32(P.X0 + E, XI, io.ht_in, A, B, A, A, s));
  DecStepBufs b;
  memset(&b, 0, sizeof(b));
  b.x0 = P.X0;
  for (int l = 0; l < P.nl; ++l) {
    // new states go to scratch first (the cell reads h_prev while other workgroups write h_new)
    b.layer[l] = {io.c + l * bh, io.h + l * bh, nullptr, P.C[l], P.HR[l], P.G[l], P.HD[l], P.HDL[l]};
    io.c_new[l] = P.C[l];
    io.h_new[l] = P.HR[l];
  }
  if (io.states_in_place) { b.c_copy = io.c; b.h_copy = io.h; }
  for (int k = 0; k < P.NA; ++k) {
    b.q[k] = P.Q + (size_t)k * bh;
    b.alpha[k] = k == 0 ? P.ALPHA : P.DS;      // (the alphas handed back are the FIRST head's, seq2seq.py:379-383)
  }
  b.cvh = P.CVH;
  b.ht = io.ht_out;
  b.attn = io.attn; b.attn_ctx = io.attn_ctx;
  b.alpha_copy = io.alpha;
  io.alpha_ws = P.ALPHA;
  io.ld_alpha_ws = P.Tp;
  ASTK_TRY(step_fwd(P, prm, io.enc, b, s));
  RowGemmArgs a = rg(B, V, io.ht_out, A, prm->Wo, A, A, io.logits, V);
  a.bias = prm->bo;
  ASTK_TRY(rowgemm_launch(a, s));
  if (io.argmax) {
    // argmax only: run the CE kernel on a scratch copy so that `logits` stays intact
    ASTK_TRY(copy2d_f32(P.LOGITS, P.Vp, io.logits, V, B, V, P.Vp, s));
    ASTK_TRY(softmax_ce_launch(B, V, P.Vp, P.LOGITS, io.tokens, 1, nullptr, 1.f, 0.f, nullptr, io.argmax, s));
  }
  return 0;
}

}  // namespace astk
