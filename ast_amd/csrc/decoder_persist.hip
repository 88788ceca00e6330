// Persistent decoder-loop kernels (seq2seq.py:361-473): ONE launch runs all S = L-1 decoder steps.
//
// Why: a decoder step is ~9 tiny dependent kernels (M = batch rows); at ~4.4 us per launch the loop is launch-floor
// bound and the attention scan can never exceed ~3 TB/s.  Here every phase of a step is a set of fixed "items"
// owned by fixed workgroups for the whole loop:
//   * the weight slice of an item lives in VGPRs as f32-MFMA B fragments (all decoder weights = 14.6 MB = 57 KB per
//     workgroup), loaded once;
//   * each attention item keeps its (batch row, time chunk) slice of enc_states in LDS for all steps, so after the
//     first step the attention scan moves no global memory at all;
//   * phases hand activations over with the same protocol as lstm_persist.hip (write-through stores, drained, one
//     arrival add per item on a per-(phase, batch-tile) counter that lives on its own 256-byte line; consumers poll
//     with one lane, barrier, then sc1 loads).  The decoder has no cross-batch-row dependency, so a consumer only
//     waits for the producers of ITS 16 batch rows.
// Forward phases per step (critical chain P1 -> P2 -> P3 -> P3b -> P4 -> next P1; P5/P6 only gate the next step when
// it is not teacher-forced):
//   P1 embed + LSTM cell (16 rows x 8 units)      P2 q = Wa h + ba        P3 attention partial (b, chunk)
//   P3b attention combine per b (cv, alpha)       P4 ht = tanh(Wc[cv;h]+bc)   P5 logits tile + per-tile CE stats
//   P6 CE combine per batch tile: lse, loss row, argmax (feedback token)
// The saved-state layout is exactly decoder.hip's DecPlan, so either backward works on it.
// Decoder layers 1..NL-1 (the shipped es_en_20h / asr_gpfr models have 3): layer l at step s needs layer l-1 at step s and its own
// step s-1, and layer 0 needs ht_{s-1} (input feeding), so the layers of one step are strictly sequential: one more hand-off
// per layer on the chain.  Every cell item (batch tile, 8 units) of every layer has a fixed owner: layers below the top live on
// the workgroups that own the same item of layer 0, the top layer on the otherwise lightly loaded upper half of the grid
// (ctx / logits owners), so that no workgroup holds more than 68 float4 (272 VGPRs) of weights.
// Applicability (else the per-launch path of decoder.hip runs): 1-3 decoder layers, H,A multiples of 16, sizes within the
// register budgets below, grid of 256 workgroups fully resident.  All spins are bounded (abort word).
// Where the forward phases are: decoder_persist_fwd_body -- P6 is its lambda run_p6 (beam branch first), P1, P1b, P3, P3b, P4, P5 the
// banners of its step loop in that order; lse_merge in front of it.  The backward loop: decoder_persist_bwd.
#include "decoder_persist.h"
#include "handoff.h"
#include <initializer_list>
#include <type_traits>

// -DASTK_PDEC_TIMING_ALL=1: the per-phase timers of ASTK_PERSIST_DBG in the multi-layer variants too (16 more registers per lane there)
// (the timers exist only in the test-hook build, libastk_test.so: the product library's kernels see dbg = 0 as a constant)
#ifndef ASTK_PDEC_TIMING_ALL
#define ASTK_PDEC_TIMING_ALL 0
#endif
namespace astk {

namespace {

constexpr int G = 256;            // workgroups (one per CU)
enum Phase { PH_CELL = 0 /* + layer: 0..2 */, PH_CELL1, PH_CELL2, PH_CMB, PH_CTX, PH_LOG, PH_CE, PH_N };
// Specialised attention phase (H = 512): at most this many rows of a (batch row, time chunk) slice stay resident in LDS (2 x 28 x 2 KB =
// 112 KB of enc + encA); a chunk's remaining rows (chunks of up to 60 rows: T'' <= 480 at batch 32, i.e. the loader's longest
// utterances of 1680 frames) are streamed from L2 / Infinity Cache every step -- they are the same bytes for every step of the loop.
constexpr int PDEC_RES_ROWS = 28, PDEC_CHUNK_MAX = 60;
constexpr int PDEC_BEAM_NSPLIT = 8;     // beam mode: attention slices per row, whatever the launch's row count (G / 32 rows)
constexpr int NPHASE_SLOTS = 8;   // counter lines reserved per batch tile ahead of the abort word and the per-row counters
// The top cell's hand-off to the attention scan is of the sentinel kind: the h half of CVH is filled with this word before the launch and
// polled itself (2 KB per workgroup, once).  (Rejected: the same between decoder LAYERS, HD[l] sentinel-filled and polled by the waves that
// multiply it -- es_en_20h, 3 layers, 6.79 -> 6.83 ms in a same-box A/B: 4 waves x 128 workgroups re-reading 8 KB each per poll cost the
// chain more than the drain + counter they replace.)
constexpr unsigned PDEC_SENTINEL = 0xffffffffu;

struct PDecArgs {
  int B, S, L, T, Tp, H, E, A, V, Vp, XI, nbt, nsplit, chunk, ntile_v;
  float inv_count;         // 1 / (rows in the cross-entropy mean): 1 / B, or 1 / (the whole batch) when this launch scores a slice of it
  const float *embed, *Wa, *ba, *Wc, *bc, *Wo, *bo, *cw;
  const float *Wu[PDEC_MAX_LAYERS], *bias[PDEC_MAX_LAYERS], *Wl[PDEC_MAX_LAYERS];     // per decoder layer
  const float* enc;
  const float* encA;       // enc . Wa  (B,T,H): score = encA.h + enc.ba
  const int32_t* y;
  const int32_t* ytgt;     // (B,L) class ids scored by the CE role (column s+1): y, or forward_loss's random_out replacements
  const int32_t* use_truth;
  const float* emb_mask;   // [S][B][E] or null
  const float* rnn_mask[PDEC_MAX_LAYERS];   // [S][B][H] per layer, or null
  int32_t* TOK; int32_t* PRED;
  float *Gt[PDEC_MAX_LAYERS], *Cst[PDEC_MAX_LAYERS], *HR[PDEC_MAX_LAYERS];
  float* HD[PDEC_MAX_LAYERS];                // [S][B][H] dropped outputs of the layers below the top (the top's go to CVH[:, H:])
  float *X0, *Q, *ALPHA, *CVH, *HT, *LOGITS, *LOSSROWS, *LSE;
  float* PART;             // [S][B][nsplit][H+4]
  float* ML;               // [S][B][2] softmax max and 1/sum of every attention row
  float* CESTAT;           // [S][B][ntile_v][4]
  unsigned* ctr;           // [PH_N][nbt] * CTRS
  AbortCtl ab;
  int dbg;
  float* tick_out;         // profiler: [G] accumulated attention-phase microseconds per workgroup, [G+0] launches
  // greedy mode (GR): feed `go` at step 0, stop once every row has emitted `eos` (S = the stop limit; PRED = the caller's tokens)
  // scored greedy mode (SC) reuses training fields: LSE = LOGP [S][B], LOSSROWS = NLL [S][B] or null, ytgt = targets [B][L] or null
  // (L = their row length, column s+1 scored at step s; steps with s+1 >= L have none), cw = class weights or null
  int go, eos;
  unsigned* gctl;          // 4 counter lines: [0] max over batch tiles of the step their last row finished, [1] tiles reported,
                           // [2] workgroups that left, [3] the stop word (n_steps; preset to S)
  int32_t* n_steps_out;    // written by the last workgroup to leave: the stop word
  float* status_dst;       // ... and a copy of the persistent status word (or null)
  // sampled mode (SM): Gumbel-max draws from softmax(logits * inv_temp); LSE = LOGP [S][B] as in the scored mode
  const uint64_t* row_keys;   // [B] sample_row_key(seed, stream) of every batch row
  float inv_temp;
  // inference modes (GR): per-row source lengths, 1 <= row_len[b] <= T, or null = every row attends over all T positions.  Read once,
  // in front of the step loop, by the attention workgroups
  const int32_t* row_len;
  // beam mode (BM): bN hypotheses kept and bK expansions per utterance, rows laid out by the tile rule of include/astk.h (astk_beam_decode).
  // PRED = the token every row feeds at the next step [S][B]; LOGITS = the step's logits [S][B][Vp], kept by P5 for P6's top-K passes
  int bN, bK;
  int32_t* PAR;            // [S][B] parent ROW of the slot a row holds after step s (its own row: an empty or padding row)
  int32_t* BHIST;          // [S][B][4] the history record of astk_beam_state.hist: parent slot, token, carried, 0
  int32_t* BSTATUS;        // [B] slot status (0 empty, 1 live, 2 finished), double BSCORE [B], and BORG [B] = step * B + row of the cell
  double* BSCORE;          //     state the slot's hypothesis was last expanded from (-1: none), all rewritten at every step
  int32_t* BORG;
  float* CS[PDEC_MAX_LAYERS];   // [S + 1][B][H] c of every step (slot s + 1 = after step s): the final states are gathered behind the loop
  // truncated sampled mode (TK): the draw among the top_k largest xs = logits * inv_temp, cut to the nucleus of mass top_p (include/astk.h
  // astk_sample_decode_topk).  LOGITS = the step's xs [S][B][Vp], kept by P5 for P6's top_k sweeps; row_keys, inv_temp, LSE = LOGP as in SM
  int top_k;
  float top_p;
  int32_t* NKEPT;          // [S][B] the kept count m of every draw, or null
};

// A UNIFORM base pointer, re-formed where it is used (opaque to loop-invariant code motion).  An element address is then base (scalar
// registers) + one 32-bit lane offset shared by all arrays of the same shape, instead of a hoisted 64-bit per-lane pointer per array: in the
// multi-layer kernels (512 registers, the weights resident) ~30 such pointers were spilled, and a scratch reload between two written-through
// stores waits (vmcnt counts in order) for the store in front of it -- a memory round trip per reload, on the decoder's chain.
// ua(base, i): &base[i] with `base` uniform and i this lane's 32-bit element offset -- a scalar base + a 32-bit BYTE offset register, the
// form the global instructions take as it is (a 64-bit element offset would be shifted and added per lane, and kept, and spilled).
template <class T>
__device__ __forceinline__ T* ua(T* base, unsigned i) {
  unsigned long long v = (unsigned long long)base;
  asm volatile("" : "+s"(v));
  // (integer -> GLOBAL pointer: through a generic pointer the accesses become FLAT)
  return (T*)((char __attribute__((address_space(1)))*)v + i * (unsigned)sizeof(T));
}
// Written-through store to base[i], `base` uniform, i this lane's 32-bit element offset: the instruction's scalar-base form, by hand -- for
// an atomic store the compiler adds base and offset per lane into a 64-bit register pair (and keeps the extended offset alive, and spills it).
// (The compiler does not count this store in its s_waitcnt bookkeeping: harmless -- memory operations return in order, an uncounted one can
//  only make a wait longer -- and every publish() drains with an explicit s_waitcnt vmcnt(0).)
__device__ __forceinline__ void st_sc1_u(float* base, unsigned i, float v) {
  asm volatile("global_store_dword %0, %1, %2 sc1" ::"v"(i * 4u), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// Resident weight fragments (NB k-blocks of 16 floats per wave): MFMA column j = lane&15 -> W row `row`.
template <int NB>
__device__ __forceinline__ void wload(float4* w, const float* W, long ldw, int row, int K, int lane, int wave) {
  const int q = lane >> 4;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int k = 16 * (wave + 4 * i) + 4 * q;
    w[i] = k < K ? *reinterpret_cast<const float4*>(W + (long)row * ldw + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// A fragments of a handed-off row block: 16-byte loads (AUX = 16: sc1) at float offset a_off + k, k = 16 (wave + 4 (i0 + i)) + 4 q.
// Blocks that all lie inside K (the shipped widths): ONE address register and immediate offsets.  Otherwise k is clamped (the matching w
// is zero beyond K) -- one address register per load: in the multi-layer kernels those were spilled, and a scratch reload between two
// buffer loads waits for every load issued before it (vmcnt counts in order): the 16 loads of a product came back in 8 round trips.
template <int NB, int AUX = 16>
__device__ __forceinline__ void aload_sc1(float4* a, __amdgpu_buffer_rsrc_t ra, long a_off, int K, int lane, int wave, int i0 = 0) {
  const int kb = 16 * (wave + 4 * i0) + 4 * (lane >> 4);
  if (64 * (i0 + NB) <= K) {
    const int vo = (int)((a_off + kb) * 4);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const u32q v = __builtin_amdgcn_raw_buffer_load_b128(ra, vo + 256 * i, 0, AUX);
      a[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
  } else {
    int kbv = kb;
    asm volatile("" : "+v"(kbv));      // (opaque: the NB clamped offsets are formed here, not hoisted out of the step loop as NB live registers)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const u32q v = __builtin_amdgcn_raw_buffer_load_b128(ra, (int)((a_off + min(kbv + 64 * i, K - 4)) * 4), 0, AUX);
      a[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
  }
}
// acc += A[arow][0:K] . W^T : A read with sc1 loads through `ra` at float offset a_off (+k)
template <int NB>
__device__ __forceinline__ void wmac(f32x4& acc, const float4* w, __amdgpu_buffer_rsrc_t ra, long a_off, int K, int lane, int wave) {
  float4 a[NB];
  aload_sc1<NB>(a, ra, a_off, K, lane, wave);
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, w[i].x, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, w[i].y, acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, w[i].z, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, w[i].w, acc2, 0, 0, 0);
  }
  acc += acc2;
}

// 4-wave reduction of one 16x16 accumulator: returns element (row = tid>>4, col = tid&15)
__device__ __forceinline__ float reduce16(f32x4 acc, float* red /* [4][256] */) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  *reinterpret_cast<f32x4*>(&red[(wave * 64 + lane) * 4]) = acc;
  __syncthreads();
  const int row = tid >> 4, col = tid & 15;
  const int src = ((row >> 2) * 16 + col) * 4 + (row & 3);
  const float v = red[src] + red[256 + src] + red[512 + src] + red[768 + src];
  __syncthreads();
  return v;
}

// Register budgets (k-blocks of 16 per wave): cell emb-part E <= 128, ht-part A <= 512, h-part H <= 512; ctx 2H <= 1024;
// logits A <= 512.  A workgroup is either a cell owner or a ctx/logits owner, so both roles share one register array:
// cell = 2 tiles x (we[2] + wa[8] + wh[8]) = 36 float4 ; other = wc[16] + wl[2][8] = 32 float4.
constexpr int NB_E = 2, NB_A = 8, NB_H = 8, NB_C = 16, NB_L = 8;
constexpr int CELLW = NB_E + NB_A + NB_H;            // per gate tile
constexpr int OFF_WC = 0, OFF_WL = NB_C, NWREG = 2 * CELLW;
static_assert(OFF_WL + 2 * NB_L <= NWREG, "register budget");
// NL > 1: two cell slots of 2 tiles x (8 + 8) k-blocks = 32 float4 each: [0, 32) layer 0 ([ht | lateral]; its embedding columns are
// re-read every step, off the chain) or ctx / logits, [32, 64) a layer >= 1 ([upward | lateral]).  64 float4 = 256 registers = the
// whole AGPR file.  (Streaming the lateral weights of the second slot from L2 instead -- 48 float4 resident -- halved the spills of
// the specialised attention phase but cost 4 us per decoder step: the reads compete with the chain's hand-offs.  Not kept.)
constexpr int CELLW2 = 2 * NB_H, OFF_C2 = 2 * CELLW2, NWREG_ML = 4 * CELLW2;
static_assert(OFF_WL + 2 * NB_L <= OFF_C2, "register budget");

// sampled mode: the batch rows' keys, 256 bytes of LDS that only the sampled instantiations have.  One slot per batch row of the device
// loop: greedy_plan() refuses B > PDEC_SM_ROWS, so a row index is a slot index (raise the two together).
constexpr int PDEC_SM_ROWS = 32;
__device__ __forceinline__ uint64_t* sm_row_keys() {
  __shared__ uint64_t keys[PDEC_SM_ROWS];
  return keys;
}
// ... and the CE role's sticky per-row done flags: one word per row of the batch tile, read and written by that row's thread sub == 0
// alone (in the 3-layer instantiation, all 512 registers taken, the flag was spilled as a register: a scratch round trip per step in P6)
__device__ __forceinline__ int* sm_row_done() {
  __shared__ int done[16];
  return done;
}

// beam mode: the slot table of the CE role's batch tile and the step's candidates, LDS that only the beam instantiations have.
// Candidate (row i, k) sits at i * 16 + k: a finished slot's own entry at k = 0, a live slot's k-th expansion at k; ctok = -1: none.
struct BeamTile {
  double score[16];
  double cscore[256];
  int ctok[256];
  int status[16], tok[16], org[16], sel[16];
};
constexpr int BM_EMPTY = 0, BM_LIVE = 1, BM_DONE = 2;      // (beam.hip's ST_*)
__device__ __forceinline__ BeamTile* bm_tile() {
  __shared__ BeamTile t;
  return &t;
}
// ... and the cells' exchange of the register-held c among the rows of their tile: [0, 128) the first cell slot, [128, 256) the second
__device__ __forceinline__ float* bm_cperm() {
  __shared__ float c[256];
  return c;
}

template <int NB>
__device__ __forceinline__ void mfma_blocks(f32x4& acc, const float4* a, const float4* w) {
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, w[i].x, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, w[i].y, acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, w[i].z, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, w[i].w, acc2, 0, 0, 0);
  }
  acc += acc2;
}

// ---------------------------------------------------------------------------------------------------------------------
// The forward loop: decoder_persist_fwd_body<NC, NL, XS, MODE>, a prologue (item ownership, resident weights, LDS slices, initial state) and
// the step loop, whose phases are the blocks under the `// ===== P...` banners; what a mode changes in a phase is described at that banner.
// NC > 0: H = 64 * NC and chunk <= PDEC_CHUNK_MAX are compile-time facts for the attention phase (fully unrolled, batched reads);
// NC = 0: generic loops.
// XS: the slice has more rows than stay resident (chunk > PDEC_RES_ROWS): the streamed-row code is compiled into its own instantiation
// so that the common short-chunk case keeps its register budget.
// MODE: what the loop runs (PDecMode); the switches GR, SC, FD, SM, BM, STOP and SUMS are derived from it at the top of the body.
// TRAIN: teacher forcing by flagS, the saved state of the backward pass, the loss rows.
// GR (every other mode), greedy decoding (inference): no targets, masks, loss or saved state for a backward pass (Gt, Cst, X0, ALPHA, ML,
// LOGITS, LSE and loss rows are neither read nor written).  Touches P1 (token, stop), P3 / P3b (no ALPHA / ML), P4 (no X0), P5 and P6 (the
// stop).  DESIGN.md section 11.
// SC (with GR), scored greedy decoding: P5 keeps the sums, P6 stores LOGP and NLL.  DESIGN.md section 12.
// FD (with GR and SC), forced decoding -- the model run along a given translation: P1 feeds y, there is no stop (STOP = false); P5, P6, and
// the raw scores of P3 / P3b.  DESIGN.md section 13.
// SM (with GR and SC, without FD), sampled decoding -- ancestral sampling by the Gumbel-max identity: the draw in P5, its merge in P6.
// DESIGN.md section 14.
// TK (with GR and SC, without FD, SM and BM), truncated sampled decoding -- top-k / nucleus: P5 keeps the tempered logits, P6 finds a row's
// top_k best, cuts them to the nucleus and draws among the kept by the Gumbel-max identity.  DESIGN.md section 20.
// BM (with GR and SC, without FD and SM), beam search -- every slot of every utterance is one row: P5 keeps the logits, the beam branch of
// P6 selects, the cells (P1, P1b) follow the parents.  DESIGN.md section 16.
// A stored row's K best values, by K sweeps on the 16 lanes of the row (beam mode's and the truncated sampled mode's P6): sweep k keeps the
// first value behind the pick of sweep k-1 -- higher value first, equal ones lower id first -- from 16-byte sc1 reads of the row P5 stored
// written through at float offset `lrow`; lane k of the row (sub == k) keeps pick k in (my_x, my_i).  K <= 16, K <= V.
__device__ __forceinline__ void row_top_k(__amdgpu_buffer_rsrc_t r_lg, long lrow, int V, int K, int sub, float& my_x, int& my_i) {
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bi = -1;
    for (int j = sub * 4; j < V; j += 64) {
      const float4 v = ldb128_sc1(r_lg, lrow + j);
      const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = j + e;
        const float x = xs[e];
        if (n < V && (pv > x || (pv == x && pi < n)) && (bi < 0 || x > bv || (x == bv && n < bi))) { bv = x; bi = n; }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (sub == k) { my_x = bv; my_i = bi; }
    pv = bv; pi = bi;
  }
}
// Two partial sums of exponentials, `se` relative to m and `os` relative to om, merged relative to nm = max(m, om): a side whose reference
// is -inf holds nothing (its factor would be exp(nan)).  P6 merges the guarded form three times; its sweep over the tile records, which
// guards one side only, is another expression and stays where it is.
__device__ __forceinline__ float lse_merge(float m, float se, float om, float os, float nm) {
  return (m == -INFINITY ? 0.f : se * expf(m - nm)) + (om == -INFINITY ? 0.f : os * expf(om - nm));
}
enum PDecMode { PDEC_TRAIN, PDEC_GREEDY, PDEC_SCORED, PDEC_FORCED, PDEC_SAMPLED, PDEC_BEAM, PDEC_TOPK };
template <int NC, int NL, bool XS, PDecMode MODE>
__device__ __forceinline__ void decoder_persist_fwd_body(const PDecArgs& a) {
  constexpr bool GR = MODE != PDEC_TRAIN, SC = GR && MODE != PDEC_GREEDY, FD = MODE == PDEC_FORCED, SM = MODE == PDEC_SAMPLED;
  constexpr bool BM = MODE == PDEC_BEAM;
  constexpr bool TK = MODE == PDEC_TOPK;   // (with GR and SC, without SM: the draw is P6's)
  constexpr bool DRAW = SM || TK;          // the modes that draw: the row keys and the sticky done flags in LDS
  constexpr bool STOP = GR && !FD;         // the greedy modes' stop word exists
  constexpr bool SUMS = !GR || SC;         // P5 / P6 keep the sum of exponentials and the target logit
  extern __shared__ __attribute__((aligned(16))) float lds[];   // enc slice [chunk][H], encA slice [chunk][H], scratch
  __shared__ __attribute__((aligned(16))) float red[4 * 256];
  __shared__ __attribute__((aligned(16))) float zt[2 * 256];
  __shared__ int s_flag;
  __shared__ int yS[GR ? 1 : 16 * 192];    // targets of this workgroup's batch tile (L <= 192)
  __shared__ int flagS[GR ? 1 : 192];      // teacher-forcing flags
  __shared__ int s_stop;                   // GR: a sentinel poll saw the stop
  __shared__ int s_wdone[4];               // GR: per wave of the CE role, all of its rows are done
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (GR && tid == 0) s_stop = 0;          // (the first barrier below orders it before every use)
  if constexpr (DRAW) {
    if (tid < PDEC_SM_ROWS) sm_row_keys()[tid] = a.row_keys[min(tid, a.B - 1)];     // (ordered by that barrier too; B <= PDEC_SM_ROWS)
  }
  const int wg = blockIdx.x;
  const int B = a.B, S = a.S, H = a.H, E = a.E, A = a.A, V = a.V, XI = a.XI, T = a.T, Tp = a.Tp;
  const int nbt = a.nbt;
  unsigned* ctr = a.ctr;
#define CTR(ph, bt) (ctr + ((ph) * nbt + (bt)) * NSH * CTRS)
#define ROWCTR(row) (ctr + ((long)NPHASE_SLOTS * NSH * nbt + 2 + (row)) * CTRS)

  // ---------------- static item ownership
  const int n_cell = nbt * (H / 8);                       // cell items (bt, 8 units): workgroups [0, n_cell)
  const bool has_cell = wg < n_cell;
  const int cell_bt = has_cell ? wg / (H / 8) : 0, cell_u0 = has_cell ? (wg % (H / 8)) * 8 : 0;
  const int n_c = nbt * (A / 16);                         // ctx items: first non-cell workgroups
  const int rest = G - n_cell;
  const int r_idx = wg - n_cell;
  const bool has_c = r_idx >= 0 && r_idx < n_c;
  const int c_bt = has_c ? r_idx / (A / 16) : 0, c_n0 = has_c ? (r_idx % (A / 16)) * 16 : 0;
  const int n_l = nbt * a.ntile_v;                        // logits items: up to 2 per non-cell workgroup
  int l_item[2] = {-1, -1};
  if (r_idx >= 0) {
    if (r_idx < n_l) l_item[0] = r_idx;
    if (r_idx + rest < n_l) l_item[1] = r_idx + rest;
  }
  const int n_att = B * a.nsplit;                         // attention items (b, split): one per workgroup
  const bool has_att = wg < n_att;
  const int att_b = has_att ? wg % B : 0, att_sp = has_att ? wg / B : 0;
  const int cmb_rank = wg - (G - B);                      // combine items (b): the last B workgroups
  const bool has_cmb = cmb_rank >= 0 && cmb_rank < B;
  const int cmb_b = has_cmb ? cmb_rank : 0;
  const int ce_rank = wg - (G - B - nbt);                 // CE items (bt)
  const bool has_ce = ce_rank >= 0 && ce_rank < nbt;

  // upper decoder layers (NL > 1): layers 1..NL-2 on the owner of the same layer-0 item, the top layer on the upper workgroups
  constexpr int TOP = NL - 1;
  const bool has_mid = NL > 2 && has_cell;
  const int top_rank = wg - (G - n_cell);
  const bool has_top = NL > 1 && top_rank >= 0;
  const int top_bt = has_top ? top_rank / (H / 8) : 0, top_u0 = has_top ? (top_rank % (H / 8)) * 8 : 0;

  // ---------------- resident weights
  constexpr int NW = NL > 1 ? NWREG_ML : NWREG;
  float4 wreg[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) wreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r16 = lane & 15;
  if constexpr (NL > 1) {
    // second cell slot: [tile][upward 8 | lateral 8] of layer 1 (mid, NL == 3) or of the top layer
    const int l2 = has_mid ? 1 : TOP;
    if (has_mid || has_top) {
      const int u0 = has_mid ? cell_u0 : top_u0;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int row = 4 * u0 + 16 * t + r16;
        wload<NB_H>(wreg + OFF_C2 + t * CELLW2, a.Wu[l2] + (long)row * H, 0, 0, H, lane, wave);
        wload<NB_H>(wreg + OFF_C2 + t * CELLW2 + NB_H, a.Wl[l2] + (long)row * H, 0, 0, H, lane, wave);
      }
    }
  }
  // layer-0 slot: [emb | ht | lateral] per tile with one layer, [ht | lateral] with more (the embedding columns are streamed)
  constexpr bool EMB_RES = NL == 1;
  constexpr int CW0 = EMB_RES ? CELLW : CELLW2, W0_A = EMB_RES ? NB_E : 0, W0_H = W0_A + NB_A;
  if (has_cell) {   // two 16-row gate tiles (units u0..u0+3, u0+4..u0+7): [emb cols | ht cols] of Wu, then Wl
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 4 * cell_u0 + 16 * t + r16;
      if constexpr (EMB_RES) wload<NB_E>(wreg + t * CW0, a.Wu[0] + (long)row * XI, 0, 0, E, lane, wave);
      wload<NB_A>(wreg + t * CW0 + W0_A, a.Wu[0] + (long)row * XI + E, 0, 0, A, lane, wave);
      wload<NB_H>(wreg + t * CW0 + W0_H, a.Wl[0] + (long)row * H, 0, 0, H, lane, wave);
    }
  } else {
    if (has_c) wload<NB_C>(wreg + OFF_WC, a.Wc, 2 * H, c_n0 + r16, 2 * H, lane, wave);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (l_item[t] >= 0) {
        const int n0 = (l_item[t] % a.ntile_v) * 16;
        wload<NB_L>(wreg + OFF_WL + t * NB_L, a.Wo, A, min(n0 + r16, V - 1), A, lane, wave);
      }
  }
  if constexpr (!GR) {
    if (has_cell) {
      for (int i = tid; i < 16 * a.L; i += 256) yS[i] = a.y[(long)min(cell_bt * 16 + i / a.L, B - 1) * a.L + (i % a.L)];
      for (int i = tid; i < S; i += 256) flagS[i] = a.use_truth[i];
    } else if (has_ce) {
      for (int i = tid; i < S; i += 256) flagS[i] = a.use_truth[i];     // (which steps feed their argmax back: decides when P6 may be deferred)
    }
  }
  // ---------------- resident slices of enc_states and encA = enc Wa in LDS: rows [t0, t1) of batch row att_b
  // BM: a row's slices are cut by ITS OWN length -- chunk = ceil(length / PDEC_BEAM_NSPLIT) <= a.chunk, which only sizes the LDS -- so
  // that its attention arithmetic is the same in every launch; trailing slices of a short row are empty
  int chunk_r = a.chunk;
  if constexpr (BM) {
    if (a.row_len) chunk_r = min(a.chunk, (max(1, min(T, a.row_len[att_b])) + PDEC_BEAM_NSPLIT - 1) / PDEC_BEAM_NSPLIT);
  }
  const int t0 = att_sp * chunk_r;
  int t1 = min(T, t0 + chunk_r);
  if constexpr (BM) t1 = max(t0, t1);        // (8 slices of ceil(T / 8) may start beyond T: empty, with or without lengths)
  if constexpr (GR) {        // a row with a length: this workgroup's slice ends where the row does, and is EMPTY (nrow = 0) beyond it
    if (a.row_len) t1 = max(t0, min(t1, min(T, a.row_len[att_b])));
  }
  const int nrow0 = has_att ? t1 - t0 : 0;
  const int cres = NC > 0 ? min(a.chunk, PDEC_RES_ROWS) : a.chunk;      // rows of the slice kept in LDS
  const int nres0 = min(nrow0, cres);
  // GR: the row count is a loaded value now, which a register would have to hold across the whole step loop (the 3-layer kernels have
  // none to spare): it is kept in LDS (yS[0], otherwise unused in these modes) and P3 reads it back at the top of every step
  if (GR && tid == 0) yS[0] = nrow0;        // (ordered by the barriers below)
  float* encS = lds;
  float* encAS = lds + cres * H;
  float* ebS = lds + 2 * cres * H;               // [chunk] enc.ba, computed once
  float* scr = ebS + ((a.chunk + 3) & ~3);       // per-step scratch: hS[H] | score[chunk] | p[chunk]  -- or the combine's partial rows
  const float* gEnc = a.enc + ((long)att_b * T + t0) * H;       // this slice in global memory (rows >= nres are read from here every step)
  const float* gEncA = a.encA + ((long)att_b * T + t0) * H;
  if (has_att) {
    const int n4 = nres0 * H / 4;
    for (int i = tid; i < n4; i += 256) {
      reinterpret_cast<float4*>(encS)[i] = reinterpret_cast<const float4*>(gEnc)[i];
      reinterpret_cast<float4*>(encAS)[i] = reinterpret_cast<const float4*>(gEncA)[i];
    }
    if constexpr (GR) {
      if (nrow0 == 0)        // an empty slice: the scans read LDS row 0 with weight 0, so it holds zeros (the partial is then exact zeros)
        for (int i = tid; i < H; i += 256) encS[i] = encAS[i] = 0.f;
    }
    __syncthreads();
    for (int t = tid; t < nrow0; t += 256) {      // eb[t] = enc[t,:] . ba  (score = encA.h + eb)
      float d = 0.f;
      for (int k = 0; k < H; ++k) d += gEnc[(long)t * H + k] * a.ba[k];
      ebS[t] = d;
    }
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t r_x0 = make_rsrc(a.X0), r_hr = make_rsrc(a.HR[0]), r_cvh = make_rsrc(a.CVH), r_ht = make_rsrc(a.HT);
  bool att_dead = false;     // this wave gave up polling a sentinel hand-off (abort / time-out): it goes on without waiting
  const __amdgpu_buffer_rsrc_t r_part = make_rsrc(a.PART), r_ces = make_rsrc(a.CESTAT);
  // cell epilogue ownership: threads 0..127: tile = tid>>6, (row = (tid>>2)&15, unit = tid&3)
  const int ce_tile = tid >> 6, ce_row = (tid >> 2) & 15, ce_u = tid & 3;
  const int cell_b = cell_bt * 16 + ce_row, cell_u = cell_u0 + 4 * ce_tile + ce_u;
  float c_state = 0.f;
  if (has_cell && tid < 128 && cell_b < B) c_state = a.Cst[0][(long)cell_b * H + cell_u];   // C[0] = c0
  float4 cbias = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_cell && tid < 128) cbias = *reinterpret_cast<const float4*>(a.bias[0] + 4 * cell_u);
  // second cell slot: state and bias of this thread's (row, unit) of layer l2
  const int l2 = has_mid ? 1 : TOP;
  const int c2_bt = has_mid ? cell_bt : top_bt, c2_u0 = has_mid ? cell_u0 : top_u0;
  const int c2_b = c2_bt * 16 + ce_row, c2_u = c2_u0 + 4 * ce_tile + ce_u;
  // this thread's (row, unit) element of a [.][B][H] array, as ONE 32-bit offset per cell slot (the arrays' uniform bases: ua(), st_sc1_u())
  const unsigned cell_off = (unsigned)(cell_b * H + cell_u), c2_off = (unsigned)(c2_b * H + c2_u);
  const bool has_c2 = NL > 1 && (has_mid || has_top);
  float c_state2 = 0.f;
  float4 cbias2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_c2 && tid < 128) {
    if (c2_b < B) c_state2 = a.Cst[l2][(long)c2_b * H + c2_u];
    cbias2 = *reinterpret_cast<const float4*>(a.bias[l2] + 4 * c2_u);
  }

  long long tk[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) tk[i] = 0;
  // per-phase debug timers (ASTK_PERSIST_DBG): 50 registers when live -- compiled in only where they fit without spills (one layer)
  const bool timing = (NL == 1 || ASTK_PDEC_TIMING_ALL) && PERSIST_DBG(a) != 0;
  long long tlast = timing ? wall_clock64() : 0;
  long long tk_att = 0;
  long long tq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define TQ(i) if (timing) { const long long now_ = wall_clock64(); tq[i] += now_ - tlast; tlast = now_; }
#define TICK(i) if (timing) { const long long now_ = wall_clock64(); tk[i] += now_ - tlast; tlast = now_; }
  int p6_pending = -1;
  bool row_done = ce_rank * 16 + (tid >> 4) >= B;     // GR, CE role: sticky "this thread's row has emitted EOS" (padding rows: done)
  if constexpr (DRAW) {
    if ((tid & 15) == 0) sm_row_done()[tid >> 4] = row_done ? 1 : 0;
  }
  bool tile_done = false;                             // GR, CE role (thread 0): this batch tile has reported
  if constexpr (BM) {        // step 0: slot 0 of every utterance is live, with score 0 and `go` as its token (ordered by the first wait's barrier)
    if (has_ce && tid < 16) {
      BeamTile* t = bm_tile();
      const bool live = ce_rank * 16 + tid < B && tid < (16 / a.bN) * a.bN && tid % a.bN == 0;
      t->score[tid] = 0.0; t->status[tid] = live ? BM_LIVE : BM_EMPTY; t->tok[tid] = a.go; t->org[tid] = -1;
    }
  }
  // P6 of step s (run in place or deferred: see the P6 banner in the step loop).
  // GR: the CE owner of each batch tile keeps a sticky per-row done flag (padding rows are done); once its tile is all done it reports that
  // step (atomic max, then one arrival), and the tile that completes the count writes the stop word n_steps = max + 1 before its PH_CE
  // arrival of that step.
  // SC: merges the sums as the training mode does and stores, beside the token, the log-probability of that token and the weighted negative
  // log-likelihood of the target (PDecArgs: LSE = LOGP, LOSSROWS = NLL, ytgt / L / cw).  Two more plain stores in front of the vmcnt(0) and
  // the barrier that the token store already had: no wait, arrival, counter or exit condition is added.
  // FD: stores LOGP = log p(y[b][s+1]) (PDecArgs: LSE), the confidence max logit - LSE (LOSSROWS, or null) and the argmax (PRED, or null).
  // SM: merges the winner by z and the sums relative to the largest reference, stores the token and LOGP = (xs_tok - ref) - logf(se), then
  // runs the greedy branch on the SAMPLED token as it stands: no wait, arrival, counter or exit condition is added.
  // TK: behind the same wait, the draw among the kept candidates of the stored row (top_k sweeps, the nucleus cut, Gumbel-max), then the
  // stores of SM plus the kept count, then the greedy branch on the drawn token as SM runs it: no wait, arrival, counter or exit is added.
  auto run_p6 = [&](const int s) -> bool {
      const int bt = ce_rank, m0 = bt * 16;
      const int row = m0 + (tid >> 4), sub = tid & 15;       // 16 threads per row sweep the tiles
      // BM: every slot of every utterance is one row.  Forms, per row, the float32 LSE of the scored mode and the row's K best tokens (K sweeps over
      // the stored logits: higher logit first, equal ones lower id first), lists the candidates of every utterance slot by slot (a finished slot
      // itself, a live slot its K expansions), takes the stable top N by float64 score, and writes -- in front of its PH_CE arrival -- the history
      // record, the token the row feeds next (PRED) and the PARENT row (PAR) of every row.  A tile reports once none of its slots is live.
      if constexpr (BM) {
        BeamTile* const t = bm_tile();
        // (every per-lane value of this role is formed from `tl` here, behind an empty asm: hoisted out of the step loop they would each
        //  hold a register over the whole loop, and the multi-layer kernels have none to spare -- sections 12-15)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        const int N = a.bN, K = a.bK, i = tl >> 4, sub = tl & 15, row = m0 + i;
        if (!wg_wait_sh(CTR(PH_LOG, bt), a.ntile_v, s + 1, a.ab, &s_flag, StopCtl{a.gctl + 3 * CTRS, s, false})) return false;
        const int rl = min(row, B - 1);
        // the row's LSE = mx + logf(se): the scored mode's float32 merge of the tile records
        float mx = -INFINITY, se = 0.f;
        for (int k = sub; k < a.ntile_v; k += 16) {
          const float4 cs = ldb128_sc1(r_ces, (((long)s * B + rl) * a.ntile_v + k) * 4);
          const float nm = fmaxf(mx, cs.x);
          se = (mx == -INFINITY ? 0.f : se * expf(mx - nm)) + cs.y * expf(cs.x - nm);
          mx = nm;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          const float om = __shfl_xor(mx, o), os = __shfl_xor(se, o);
          const float nm = fmaxf(mx, om);
          se = lse_merge(mx, se, om, os, nm);
          mx = nm;
        }
        const float lg = logf(se);
        // the row's K best tokens (row_top_k: K sweeps over the row P5 stored); lane k of the row keeps pick k
        float my_x = 0.f;
        int my_i = -1;
        row_top_k(make_rsrc(a.LOGITS), ((long)s * B + rl) * a.Vp, V, K, sub, my_x, my_i);
        // candidate (row i, k = sub): float64 score = the slot's + logp, logp = (x - mx) - logf(se) formed without rounding the LSE first
        const int st_i = t->status[i];
        const bool valid = row < B && ((st_i == BM_LIVE && sub < K && my_i >= 0) || (st_i == BM_DONE && sub == 0));
        double cs = -INFINITY;
        int ct = -1;
        if (valid) {
          if (st_i == BM_DONE) { cs = t->score[i]; ct = t->tok[i]; }
          else { cs = t->score[i] + (double)((my_x - mx) - lg); ct = my_i; }
          if (cs != cs) cs = -INFINITY;          // (a NaN score ranks last: the ranks below stay a permutation)
        }
        t->cscore[tl] = cs;
        t->ctok[tl] = ct;
        if (tl < 16) t->sel[tl] = -1;
        __syncthreads();
        // stable top N of the utterance's candidates: a candidate lands at its rank (higher score first, equal scores in list order)
        const int ui = i / N;
        if (valid) {
          int rank = 0;
          const int c0 = ui * N * 16, c1 = c0 + N * 16;
          for (int c = c0; c < c1; ++c) rank += (t->ctok[c] >= 0 && (t->cscore[c] > cs || (t->cscore[c] == cs && c < tl))) ? 1 : 0;
          if (rank < N) t->sel[ui * N + rank] = tl;
        }
        __syncthreads();
        // the new slot of row tl < 16: read the old table, barrier, then write
        int n_par = tl & 15, n_tok = a.eos, n_st = BM_EMPTY, n_org = -1, n_car = 0, h_par = -1;
        double n_sc = 0.0;
        if (tl < 16) {
          const int c = t->sel[tl];
          if (c >= 0) {
            n_par = c >> 4;
            n_car = t->status[n_par] == BM_DONE ? 1 : 0;
            n_tok = t->ctok[c];
            n_sc = t->cscore[c];
            n_st = (n_car || n_tok == a.eos) ? BM_DONE : BM_LIVE;
            n_org = n_car ? t->org[n_par] : s * B + m0 + n_par;
            h_par = n_par - (tl / N) * N;
          }
        }
        __syncthreads();
        if (tl < 16) {
          t->score[tl] = n_sc; t->status[tl] = n_st; t->tok[tl] = n_tok; t->org[tl] = n_org;
          if (m0 + tl < B) {
            const unsigned r = (unsigned)(m0 + tl);
            sti_sc1(ua(a.PAR + (long)s * B, r), m0 + n_par);
            sti_sc1(ua(a.PRED + (long)s * B, r), n_tok);
            *ua(reinterpret_cast<int4*>(a.BHIST + (long)s * B * 4), r) = make_int4(h_par, n_st == BM_EMPTY ? 0 : n_tok, n_car, 0);
            *ua(a.BSTATUS, r) = n_st;
            *ua(a.BSCORE, r) = n_sc;
            *ua(a.BORG, r) = n_org;
          }
        }
        const bool any_live = __any(tl < 16 && n_st == BM_LIVE);
        if (tl == 0) s_wdone[0] = any_live ? 0 : 1;
        // the tile's report between the barrier and the arrival, as in the greedy modes: the stop word is written in front of PH_CE(s)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tl == 0) {
          if (!tile_done && s_wdone[0]) {
            tile_done = true;
            unsigned* gc = a.gctl;
            __hip_atomic_fetch_max(gc, (unsigned)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(gc + CTRS, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == (unsigned)a.nbt) {
              const unsigned n = __hip_atomic_load(gc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
              __hip_atomic_store(gc + 3 * CTRS, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
          }
          __hip_atomic_fetch_add(CTR(PH_CE, bt), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return true;
      }
      [[maybe_unused]] bool sc_tgt = false;                  // SC: step s has a target (column s+1 of y); its class weight
      [[maybe_unused]] float sc_w = 0.f;
      if constexpr (SC && !FD && !DRAW) {       // (read in front of the wait: neither load is on the chain)
        sc_tgt = a.ytgt && s + 1 < a.L;
        if (sc_tgt && sub == 0 && row < B) {
          int r = row;
          asm volatile("" : "+v"(r));       // (keeps the address out of the loop-invariant registers: they are full, it would spill)
          const int tgt = *ua(a.ytgt + s + 1, (unsigned)(r * a.L));
          sc_w = a.cw ? a.cw[tgt < 0 ? 0 : (tgt >= V ? V - 1 : tgt)] : 1.f;
        }
      }
      if (!wg_wait_sh(CTR(PH_LOG, bt), a.ntile_v, s + 1, a.ab, &s_flag, StopCtl{STOP ? a.gctl + 3 * CTRS : nullptr, s, false})) return false;
      float mx = -INFINITY, se = 0.f, xt = 0.f;
      int mi = 0x7fffffff;
      [[maybe_unused]] float rf = -INFINITY;                 // SM: the reference of `se` (the largest winner's xs merged so far)
      [[maybe_unused]] int tk_m = 0;                         // TK: the kept count of the draw
      // TK: the draw of include/astk.h (astk_sample_decode_topk) on the row of xs that P5 stored -- the tile records are not used.  Lane j of
      // the row's 16 holds candidate j; mi = the drawn token, xt = its log-probability among the kept, tk_m = the kept count.
      if constexpr (TK) {
        // (every per-lane value formed from `tl` here, behind an empty asm, as in beam mode's P6: the multi-layer kernels have no
        //  register to hold one over the step loop)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        const int K = a.top_k, j = tl & 15, rl = min(m0 + (tl >> 4), B - 1);
        float my_x = 0.f;
        int my_i = -1;
        row_top_k(make_rsrc(a.LOGITS), ((long)s * B + rl) * a.Vp, V, K, j, my_x, my_i);
        const bool cand = j < K && my_i >= 0;
        const float x0 = __shfl(my_x, 0, 16);                // the row's largest xs: the reference of every exponential below
        const float e = cand ? expf(my_x - x0) : 0.f;
        // nucleus: q_j = e_j / sum_K e; m = the smallest count whose prefix sum of q reaches top_p (K if none does; top_p == 1: K exactly)
        float cum = e, tot = e;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float up = __shfl_up(cum, o, 16);
          if (j >= o) cum += up;
          tot += __shfl_xor(tot, o);
        }
        const unsigned below = (unsigned)(__ballot(cand && cum / tot < a.top_p) >> (tl & 48)) & 0xffffu;
        tk_m = a.top_p >= 1.f ? K : min(K, __popc(below) + 1);
        // the draw among the kept: the largest z = xs + g(row key, s, id), equal z: the lower id; the sum of the kept exponentials
        const bool kept = cand && j < tk_m;
        mx = kept ? my_x + sample_gumbel(sm_row_keys()[rl & (PDEC_SM_ROWS - 1)], s, my_i) : -INFINITY;
        mi = kept ? my_i : 0x7fffffff;
        xt = my_x;
        se = kept ? e : 0.f;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          const float om = __shfl_xor(mx, o), ox = __shfl_xor(xt, o);
          const int oi = __shfl_xor(mi, o);
          se += __shfl_xor(se, o);
          if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; xt = ox; }
        }
        xt = (xt - x0) - logf(se);       // logp = xs_tok - LSE over the kept, formed without rounding an LSE first
      }
      if (!TK && row < B)
        for (int k = sub; k < a.ntile_v; k += 16) {
          const float4 cs = ldb128_sc1(r_ces, (((long)s * B + row) * a.ntile_v + k) * 4);
          const float tm = cs.x, ts = cs.y, tx = cs.w;
          const int ti = __float_as_int(cs.z);
          if constexpr (SM) {          // record: (z of the winner, sum of exp(xs - tx), index, tx = xs at the winner); xt = xs of the winner so far
            const float nr = fmaxf(rf, tx);
            se = (rf == -INFINITY ? 0.f : se * expf(rf - nr)) + ts * expf(tx - nr);
            rf = nr;
            if (tm > mx || (tm == mx && ti < mi)) { mi = ti; mx = tm; xt = tx; }
          } else {
            const float nm = fmaxf(mx, tm);
            if constexpr (SUMS) se = se * expf(mx - nm) + ts * expf(tm - nm);
            if (tm > mx || (tm == mx && ti < mi)) mi = ti;
            mx = nm;
            xt += tx;
          }
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        if constexpr (TK) break;         // (merged above)
        const float om = __shfl_xor(mx, o), os = __shfl_xor(se, o), ox = __shfl_xor(xt, o);
        const int oi = __shfl_xor(mi, o);
        if constexpr (SM) {
          const float orf = __shfl_xor(rf, o);
          const float nr = fmaxf(rf, orf);
          se = lse_merge(rf, se, orf, os, nr);
          rf = nr;
          if (om > mx || (om == mx && oi < mi)) { mi = oi; mx = om; xt = ox; }
        } else {
          const float nm = fmaxf(mx, om);
          if constexpr (SUMS) se = lse_merge(mx, se, om, os, nm);
          if (om > mx || (om == mx && oi < mi)) mi = oi;
          mx = nm;
          xt += ox;
        }
      }
      if constexpr (FD) {
        if (sub == 0 && row < B) {
          // log p(target) = xt - lse, lse = mx + logf(se): formed as (xt - mx) - logf(se), without rounding lse first
          const float lg = logf(se);
          int r = row;
          asm volatile("" : "+v"(r));       // (keeps the addresses out of the loop-invariant registers: they are full, they would spill)
          *ua(a.LSE + (long)s * B, (unsigned)r) = (xt - mx) - lg;
          if (a.LOSSROWS) *ua(a.LOSSROWS + (long)s * B, (unsigned)r) = -lg;
          if (a.PRED) *ua(a.PRED + (long)s * B, (unsigned)r) = mi;
        }
        publish_sh(CTR(PH_CE, bt), 0);      // (the training loop's arrival; nothing waits for it in this mode)
      } else if constexpr (GR) {
        if constexpr (SC) {
          if (sub == 0 && row < B) {
            // lse = mx + logf(se): log p(token) = mx - lse and the target's -log p = lse - xt, formed without rounding lse first
            const float lg = logf(se);
            int r = row;
            asm volatile("" : "+v"(r));     // (as above)
            if constexpr (SM) {
              // log p(token) under softmax(xs) = xs_tok - lse, lse = rf + logf(se): formed as (xs_tok - rf) - logf(se), likewise
              *ua(a.LSE + (long)s * B, (unsigned)r) = (xt - rf) - lg;
            } else if constexpr (TK) {
              *ua(a.LSE + (long)s * B, (unsigned)r) = xt;
              if (a.NKEPT) *ua(a.NKEPT + (long)s * B, (unsigned)r) = tk_m;
            } else {
              *ua(a.LSE + (long)s * B, (unsigned)r) = -lg;
              if (a.LOSSROWS) *ua(a.LOSSROWS + (long)s * B, (unsigned)r) = sc_tgt ? sc_w * ((mx - xt) + lg) : 0.f;
            }
            sti_sc1(ua(a.PRED + (long)s * B, (unsigned)r), mi);
            if constexpr (DRAW) {
              if (mi == a.eos) {
                int i = tid >> 4;
                asm volatile("" : "+v"(i));   // (as above: the LDS address formed here, not kept over the loop and spilled)
                sm_row_done()[i] = 1;
              }
            }
            else row_done = row_done || mi == a.eos;
          }
        } else if (sub == 0 && row < B) {
          sti_sc1(ua(a.PRED + (long)s * B, (unsigned)row), mi);
          row_done = row_done || mi == a.eos;
        }
        bool wdone;
        if constexpr (DRAW) {
          int i = tid >> 4;
          asm volatile("" : "+v"(i));         // (likewise)
          wdone = __all(sub != 0 || sm_row_done()[i] != 0);
        }
        else wdone = __all(sub != 0 || row_done);
        if (lane == 0) s_wdone[wave] = wdone ? 1 : 0;
        // publish_sh() with the tile's report between its barrier and its arrival: the stop word is written in front of PH_CE(s)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
          if (!tile_done && s_wdone[0] && s_wdone[1] && s_wdone[2] && s_wdone[3]) {
            tile_done = true;
            unsigned* gc = a.gctl;
            __hip_atomic_fetch_max(gc, (unsigned)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(gc + CTRS, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == (unsigned)a.nbt) {
              const unsigned n = __hip_atomic_load(gc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
              __hip_atomic_store(gc + 3 * CTRS, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
          }
          __hip_atomic_fetch_add(CTR(PH_CE, bt), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
        if (sub == 0 && row < B) {
          const float lse = mx + logf(se);
          const int tgt = *ua(a.ytgt + s + 1, (unsigned)(row * a.L));
          const float w = a.cw ? a.cw[tgt < 0 ? 0 : (tgt >= V ? V - 1 : tgt)] : 1.f;
          *ua(a.LSE + (long)s * B, (unsigned)row) = lse;
          *ua(a.LOSSROWS + (long)s * B, (unsigned)row) = -(xt - lse) * w * a.inv_count;
          sti_sc1(ua(a.PRED + (long)s * B, (unsigned)row), mi);
        }
        publish_sh(CTR(PH_CE, bt), 0);
      }
      TICK(12)
    return true;
  };
  const unsigned* const stopw = STOP ? a.gctl + 3 * CTRS : nullptr;
  for (int s = 0; s < S; ++s) {
    const StopCtl sc{stopw, s, false};
    // ================= P1: embed + LSTM cell =================
    // GR: step 0 feeds `go` to every row, every later step its own argmax; the input-feeding part reads ht_{s-1} from HT.  The layer-0 cells
    // read the stop word behind their tile's PH_CE arrival and leave at step n_steps; every other wait learns of it in its slow path (StopCtl).
    // FD: step s feeds y[b][s] (read from global memory, clamped), so no step waits for an argmax: the hand-offs are the training loop's with
    // every step teacher-forced (P6 deferred behind the next step's attention partial), and there is no stop: the stop word is never passed to
    // a wait (STOP = false), no tile reports, every workgroup runs all S steps.
    // BM: the cells gather through PAR: they read h and ht of their row's parent row, and permute the register-held c among the rows of their
    // tile through LDS.
    if (has_cell) {
      const int bt = cell_bt, m0 = bt * 16;
      const int brow = min(m0 + r16, B - 1);             // this lane's A-operand batch row
      const bool truth = FD || s == 0 || (!GR && flagS[s] != 0);
      // (GR: the stop word is read behind this tile's P6 of step s-1, which wrote it in front of that arrival: the cells leave at n_steps)
      if (!truth) { if (!wg_wait_sh(CTR(PH_CE, bt), 1, s, a.ab, &s_flag, StopCtl{stopw, s, true})) return; }
      int tok;
      if constexpr (FD) {
        int r = brow;
        asm volatile("" : "+v"(r));         // (as in P5: the address is formed here, not kept over the loop)
        tok = *ua(a.y + s, (unsigned)(r * a.L));
      } else tok = truth ? (GR ? a.go : yS[r16 * a.L + s]) : ldi_sc1(ua(a.PRED + (long)(s - 1) * B, (unsigned)brow));
      tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
      [[maybe_unused]] int prow = brow;           // BM: the row whose h_{s-1} and ht_{s-1} this lane's row continues
      if constexpr (BM) {
        if (s > 0) {       // (behind PH_CE(s-1): P6 wrote the parent words in front of that arrival)
          const int32_t* par = a.PAR + (long)(s - 1) * B;
          int tl = tid;
          asm volatile("" : "+v"(tl));         // (the addresses below formed here, not kept over the loop: as in P5)
          prow = ldi_sc1(ua(par, (unsigned)min(m0 + (tl & 15), B - 1)));
          const int pr = tl < 128 ? (ldi_sc1(ua(par, (unsigned)min(m0 + ((tl >> 2) & 15), B - 1))) - m0) & 15 : 0;
          float* cp = bm_cperm();
          if (tl < 128) {
            cp[tl] = c_state;
            if (NL > 2) cp[128 + tl] = c_state2;
          }
          __syncthreads();
          if (tl < 128) {        // (tid = tile * 64 + row * 4 + unit: the parent's c of the same unit)
            const int src = (tl & ~63) | (pr << 2) | (tl & 3);
            c_state = cp[src];
            if (NL > 2) c_state2 = cp[128 + src];
          }
        }
      }
      if (s > 0) { if (!wg_wait_sh(CTR(PH_CELL, bt), H / 8, s, a.ab, &s_flag, sc)) return; }
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      {
        // (a) embedding part and (b) recurrent part: neither depends on this step's ht, so they run before the wait on P4
        const int q = lane >> 4;
        float4 ae[NB_E], ah[NB_H];
#pragma unroll
        for (int i = 0; i < NB_E; ++i) {
          const int k = min(16 * (wave + 4 * i) + 4 * q, E - 4);
          float4 v = *reinterpret_cast<const float4*>(a.embed + (long)tok * E + k);
          if (a.emb_mask) {
            const float4 mk = *reinterpret_cast<const float4*>(a.emb_mask + ((long)s * B + brow) * E + k);
            v.x *= mk.x; v.y *= mk.y; v.z *= mk.z; v.w *= mk.w;
          }
          ae[i] = v;
        }
        aload_sc1<NB_H>(ah, r_hr, ((long)s * B + (BM ? prow : brow)) * H, H, lane, wave);     // h_{s-1}: published a whole step ago (waited above)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if constexpr (EMB_RES) mfma_blocks<NB_E>(acc[t], ae, wreg + t * CW0);
          else {
            float4 we[NB_E];
            wload<NB_E>(we, a.Wu[0] + (long)(4 * cell_u0 + 16 * t + r16) * XI, 0, 0, E, lane, wave);
            mfma_blocks<NB_E>(acc[t], ae, we);
          }
          mfma_blocks<NB_H>(acc[t], ah, wreg + t * CW0 + W0_H);
        }
      }
      TICK(0)
      // (c) input-feeding part: ht_{s-1}, written into X0[s][:, E:] by P4 of step s-1
      if (s > 0) {
        if (!wg_wait_sh(CTR(PH_CTX, bt), A / 16, s, a.ab, &s_flag, sc)) return;
        TICK(1)
        float4 at[NB_A];
        if constexpr (GR) aload_sc1<NB_A>(at, r_ht, ((long)s * B + (BM ? prow : brow)) * A, A, lane, wave);     // (HT[s] = ht_{s-1}: no X0)
        else aload_sc1<NB_A>(at, r_x0, ((long)s * B + brow) * XI + E, A, lane, wave);
        __builtin_amdgcn_sched_barrier(0);
        mfma_blocks<NB_A>(acc[0], at, wreg + W0_A);
        mfma_blocks<NB_A>(acc[1], at, wreg + CW0 + W0_A);
      }
      const float z0 = reduce16(acc[0], red);
      const float z1 = reduce16(acc[1], red);
      zt[tid] = z0;
      zt[256 + tid] = z1;
      __syncthreads();
      float4 gsave = make_float4(0.f, 0.f, 0.f, 0.f);
      const bool ev = tid < 128 && cell_b < B;
      if (ev) {
        const float4 z = *reinterpret_cast<const float4*>(&zt[ce_tile * 256 + ce_row * 16 + ce_u * 4]);
        const float ga = tanh_fast(z.x + cbias.x), gi = sigm_fast(z.y + cbias.y), gf = sigm_fast(z.z + cbias.z), go = sigm_fast(z.w + cbias.w);
        c_state = ga * gi + gf * c_state;
        const float hh = go * tanh_fast(c_state);
        const float hd = a.rnn_mask[0] ? hh * *ua(a.rnn_mask[0] + (long)s * B * H, cell_off) : hh;
        gsave = make_float4(ga, gi, gf, go);
        st_sc1_u(a.HR[0] + (long)(s + 1) * B * H, cell_off, hh);
        if constexpr (NL > 1) st_sc1_u(a.HD[0] + (long)s * B * H, cell_off, hd);     // input of layer 1
        else st_sc1_u(a.CVH + (long)s * B * 2 * H + H, cell_off + cell_b * H, hd);
      }
      TICK(2)
      publish_sh(CTR(PH_CELL, bt), cell_u0 / 8);
      TICK(3)
      if (!GR && ev) {                             // saved for the backward (plain stores, off the critical path)
        *ua(reinterpret_cast<float4*>(a.Gt[0] + (long)s * B * 4 * H), cell_off) = gsave;
        *ua(a.Cst[0] + (long)(s + 1) * B * H, cell_off) = c_state;
      }
      if constexpr (BM) {
        if (ev) *ua(a.CS[0] + (long)(s + 1) * B * H, cell_off) = c_state;      // (plain store, off the chain: read behind the loop)
      }
    }
    // ================= P1b: decoder layers 1..NL-1 (one cell item per workgroup: layer 1 of a 3-layer stack on the lower
    // workgroups, the top layer on the upper ones).  z = Wu hd_{l-1,s} + Wl h_{l,s-1} + b: the recurrent half runs before the wait.
    // BM: the top layer's cells, which wait for no PH_CE in the other modes, wait for PH_CE(s-1) of their tile in front of their recurrent half,
    // then gather through PAR as the layer-0 cells do.
    if constexpr (NL > 1) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        // pass 0: layer 1 as a MID layer (NL == 3 only); pass 1: the TOP layer
        const bool mine = pass == 0 ? has_mid : has_top;
        if ((pass == 0 && NL < 3) || !mine) continue;
        const int l = pass == 0 ? 1 : TOP;
        const int bt = c2_bt, m0 = bt * 16;
        const int brow = min(m0 + r16, B - 1);
        [[maybe_unused]] int prow = brow;
        if constexpr (BM) {
          if (s > 0) {
            // the top layer's workgroups wait for no P6 in the other modes: here the parent words of step s-1 become visible behind
            // PH_CE(s-1) of their tile (the mid layer shares the layer-0 workgroup, which has waited and has permuted c_state2 already)
            if (pass == 1) { if (!wg_wait_sh(CTR(PH_CE, bt), 1, s, a.ab, &s_flag, StopCtl{stopw, s, true})) return; }
            const int32_t* par = a.PAR + (long)(s - 1) * B;
            int tl = tid;
            asm volatile("" : "+v"(tl));       // (as in the layer-0 cells)
            prow = ldi_sc1(ua(par, (unsigned)min(m0 + (tl & 15), B - 1)));
            if (pass == 1) {
              const int pr = tl < 128 ? (ldi_sc1(ua(par, (unsigned)min(m0 + ((tl >> 2) & 15), B - 1))) - m0) & 15 : 0;
              float* cp = bm_cperm();
              if (tl < 128) cp[tl] = c_state2;
              __syncthreads();
              if (tl < 128) c_state2 = cp[(tl & ~63) | (pr << 2) | (tl & 3)];
            }
          }
        }
        if (s > 0) { if (!wg_wait_sh(CTR(PH_CELL + l, bt), H / 8, s, a.ab, &s_flag, sc)) return; }
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        {
          float4 ah[NB_H];
          aload_sc1<NB_H>(ah, make_rsrc(a.HR[l]), ((long)s * B + (BM ? prow : brow)) * H, H, lane, wave);     // h_{l,s-1} (h0 at s = 0)
          __builtin_amdgcn_sched_barrier(0);
          mfma_blocks<NB_H>(acc[0], ah, wreg + OFF_C2 + NB_H);
          mfma_blocks<NB_H>(acc[1], ah, wreg + OFF_C2 + CELLW2 + NB_H);
        }
        if (!wg_wait_sh(CTR(PH_CELL + l - 1, bt), H / 8, s + 1, a.ab, &s_flag, sc)) return;
        {
          float4 ax[NB_H];
          aload_sc1<NB_H>(ax, make_rsrc(a.HD[l - 1]), ((long)s * B + brow) * H, H, lane, wave);  // dropped output of the layer below
          __builtin_amdgcn_sched_barrier(0);
          mfma_blocks<NB_H>(acc[0], ax, wreg + OFF_C2);
          mfma_blocks<NB_H>(acc[1], ax, wreg + OFF_C2 + CELLW2);
        }
        const float z0 = reduce16(acc[0], red);
        const float z1 = reduce16(acc[1], red);
        zt[tid] = z0;
        zt[256 + tid] = z1;
        __syncthreads();
        float4 gsave = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool ev = tid < 128 && c2_b < B;
        if (ev) {
          const float4 z = *reinterpret_cast<const float4*>(&zt[ce_tile * 256 + ce_row * 16 + ce_u * 4]);
          const float ga = tanh_fast(z.x + cbias2.x), gi = sigm_fast(z.y + cbias2.y), gf = sigm_fast(z.z + cbias2.z), go = sigm_fast(z.w + cbias2.w);
          c_state2 = ga * gi + gf * c_state2;
          const float hh = go * tanh_fast(c_state2);
          const float hd = a.rnn_mask[l] ? hh * *ua(a.rnn_mask[l] + (long)s * B * H, c2_off) : hh;
          gsave = make_float4(ga, gi, gf, go);
          st_sc1_u(a.HR[l] + (long)(s + 1) * B * H, c2_off, hh);
          if (l == TOP) st_sc1_u(a.CVH + (long)s * B * 2 * H + H, c2_off + c2_b * H, hd);
          else st_sc1_u(a.HD[l] + (long)s * B * H, c2_off, hd);
        }
        publish_sh(CTR(PH_CELL + l, bt), c2_u0 / 8);
        if (!GR && ev) {
          *ua(reinterpret_cast<float4*>(a.Gt[l] + (long)s * B * 4 * H), c2_off) = gsave;
          *ua(a.Cst[l] + (long)(s + 1) * B * H, c2_off) = c_state2;
        }
        if constexpr (BM) {
          if (ev) *ua(a.CS[l] + (long)(s + 1) * B * H, c2_off) = c_state2;
        }
      }
    }
    // ================= P3: attention over the LDS-resident slices: score = encA.h + eb, p = exp(score - max), cv partial =========
    // GR: the slice's row count is read back from LDS (yS[0]) at the top of every step.  TRAIN stores the raw scores to ALPHA, normalised by the
    // backward pass; FD, BM: with ALPHA / ML given, the attention and combine roles store the raw scores and (max, 1 / sum) as the training mode
    // does; k_alpha_normalise turns them into alpha behind the loop.
    if (has_att) {
      const int b = att_b, bt = b / 16;
      TICK(15)
      const int nrow = GR ? __builtin_amdgcn_readfirstlane(*(volatile int*)yS) : nrow0;     // (GR: in front of the poll, which hides the read)
      const int nres = GR ? min(nrow, cres) : nres0;
      const int c4 = (a.chunk + 3) & ~3;
      float* hS = scr;                 // [H]
      float* scS = scr + H;            // [c4] raw scores (tail padded with -inf)
      float* pS = scr + H + c4;        // [c4] exp(score - m) (tail 0)
      // The data is the flag (lstm_persist.hip): the h half of CVH is sentinel-filled before the launch and this row's 2 KB are polled
      // themselves -- no drain, counter, counter poll or barrier between the top cell's stores and the scan.  (Rejected: waiting on the top
      // cell's counter here, then one sc1 load -- 0.6 us more per decoder step, 1.55 against 1.53 ms per train step in an A/B inside one call.)
      if (tid < H / 4) {
        const int off = (int)((((long)s * B + b) * 2 * H + H + 4 * tid) * 4);
        u32q v;
        unsigned spins = 0;
        for (;;) {
          v = __builtin_amdgcn_raw_buffer_load_b128(r_cvh, off, 0, 16);
          if (__all((v.x != PDEC_SENTINEL) & (v.y != PDEC_SENTINEL) & (v.z != PDEC_SENTINEL) & (v.w != PDEC_SENTINEL)) || att_dead) break;
          if (++spins > (a.ab.limit >> 1)) { abort_raise(a.ab); att_dead = true; }
          else if ((spins & 63u) == 0 && abort_seen(a.ab)) att_dead = true;
          else if ((spins & 63u) == 0 && __any(stop_seen(sc))) { if (lane == 0) s_stop = 1; break; }   // (GR: read behind the barrier below)
        }
        *reinterpret_cast<float4*>(hS + 4 * tid) = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
      }
      TICK(4)
      const long long ta0 = a.tick_out ? wall_clock64() : 0;
      float m, l = 0.f, my_score;
      float* prow = a.PART + (((long)s * B + b) * a.nsplit + att_sp) * (H + 4);
      if constexpr (NC > 0) {
        // ---- specialised scan: H = 64 NC, nrow <= 60: rows [0, nres) from LDS, rows [nres, nrow) (nx <= 32 of them) from global memory.
        // Every read of a pass is issued before its first use.
        constexpr int HH = 64 * NC;
        const int nx = XS ? nrow - nres : 0;
        float* const pS_ = scr + HH + 64;                // scratch: hS[H] | scores[64] | p[64] | fold
        if (tid >= nrow && tid < 64) scS[tid] = -INFINITY;
        __syncthreads();
        if (STOP && s_stop) return;
        TICK(13)
        {
          // pass 1: 16 lanes per row; group g owns rows g and g + 16; lane l covers floats 4l + 64c of the row
          const int grp = tid >> 4, l16 = tid & 15;
          const int rlast = GR ? max(nres, 1) - 1 : nres - 1;     // (GR: row 0, which holds zeros, of an empty slice)
          const int ta = min(grp, rlast), tb2 = min(grp + 16, rlast);
          const float* e1 = encAS + ta * HH + 4 * l16;
          const float* e2 = encAS + tb2 * HH + 4 * l16;
          float4 hv[NC], x1[NC], x2[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            hv[c] = *reinterpret_cast<const float4*>(hS + 64 * c + 4 * l16);
            x1[c] = *reinterpret_cast<const float4*>(e1 + 64 * c);
            x2[c] = *reinterpret_cast<const float4*>(e2 + 64 * c);
          }
          float d1 = 0.f, d2 = 0.f;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            d1 += x1[c].x * hv[c].x + x1[c].y * hv[c].y + x1[c].z * hv[c].z + x1[c].w * hv[c].w;
            d2 += x2[c].x * hv[c].x + x2[c].y * hv[c].y + x2[c].z * hv[c].z + x2[c].w * hv[c].w;
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
          if (l16 == 0) {
            if (grp < nres) scS[grp] = d1 + ebS[grp];
            if (grp + 16 < nres) scS[grp + 16] = d2 + ebS[grp + 16];
          }
          if (nx > 0) {        // streamed rows nres + g, nres + g + 16 (workgroup-uniform branch)
            const int ua = nres + min(grp, nx - 1), ub = nres + min(grp + 16, nx - 1);
            const float* g1 = gEncA + (long)ua * HH + 4 * l16;
            const float* g2 = gEncA + (long)ub * HH + 4 * l16;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              x1[c] = *reinterpret_cast<const float4*>(g1 + 64 * c);
              x2[c] = *reinterpret_cast<const float4*>(g2 + 64 * c);
            }
            d1 = 0.f; d2 = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              d1 += x1[c].x * hv[c].x + x1[c].y * hv[c].y + x1[c].z * hv[c].z + x1[c].w * hv[c].w;
              d2 += x2[c].x * hv[c].x + x2[c].y * hv[c].y + x2[c].z * hv[c].z + x2[c].w * hv[c].w;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
            if (l16 == 0) {
              if (grp < nx) scS[nres + grp] = d1 + ebS[nres + grp];
              if (grp + 16 < nx) scS[nres + grp + 16] = d2 + ebS[nres + grp + 16];
            }
          }
        }
        TQ(0)
        __syncthreads();
        TQ(1)
        {
          // chunk max / exp / sum: wave 0 holds one (padded) score per lane -- two shuffle reductions instead of 64-entry sweeps in
          // every thread (32 float4 registers that the multi-layer variants, whose weights fill the AGPR file, do not have)
          my_score = 0.f;
          m = 0.f;
          if (tid < 64) {
            const float sc = scS[tid];
            float mx = sc;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float pe = tid < nrow ? expf(sc - mx) : 0.f;
            pS_[tid] = pe;
            l = wave_sum(pe);
            m = mx;
            my_score = tid < nrow ? sc : 0.f;
          }
        }
        TQ(2)
        __syncthreads();
        TQ(3)
        {
          // pass 2: context partial.  Thread (cq, rh): columns 4cq..4cq+3, rows rh, rh+RH, ... (16-byte reads), the RH row groups
          // are folded through LDS and row group 0 publishes with 16-byte write-through stores.
          constexpr int RH = 256 / (16 * NC);            // row groups (2 for H = 512)
          constexpr int RPT = (32 + RH - 1) / RH;        // rows per thread (max) of each half (resident / streamed)
          const int cq = tid % (16 * NC), rh = tid / (16 * NC);
          float4 ev[RPT];
          float pv[RPT];
#pragma unroll
          for (int i = 0; i < RPT; ++i) {
            const int t = rh + RH * i;
            const int tc = min(t, GR ? max(nres, 1) - 1 : nres - 1);
            ev[i] = *reinterpret_cast<const float4*>(encS + tc * HH + 4 * cq);
            pv[i] = t < nres ? pS_[t] : 0.f;
          }
          float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int i = 0; i < RPT; ++i) {
            acc4.x += pv[i] * ev[i].x; acc4.y += pv[i] * ev[i].y; acc4.z += pv[i] * ev[i].z; acc4.w += pv[i] * ev[i].w;
          }
          if (nx > 0) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
              const int t = rh + RH * i;
              ev[i] = *reinterpret_cast<const float4*>(gEnc + (long)(nres + min(t, nx - 1)) * HH + 4 * cq);
              pv[i] = t < nx ? pS_[nres + t] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
              acc4.x += pv[i] * ev[i].x; acc4.y += pv[i] * ev[i].y; acc4.z += pv[i] * ev[i].z; acc4.w += pv[i] * ev[i].w;
            }
          }
          float4* fold = reinterpret_cast<float4*>(scr + HH + 128);   // [RH-1][16 NC] float4 (the launcher checks the scratch size)
          if (RH > 1) {
            if (rh > 0) fold[(rh - 1) * (16 * NC) + cq] = acc4;
            __syncthreads();
          }
          if (rh == 0) {
#pragma unroll
            for (int k = 1; k < RH; ++k) {
              const float4 o = fold[(k - 1) * (16 * NC) + cq];
              acc4.x += o.x; acc4.y += o.y; acc4.z += o.z; acc4.w += o.w;
            }
            u32q u;
            u.x = __float_as_uint(acc4.x); u.y = __float_as_uint(acc4.y); u.z = __float_as_uint(acc4.z); u.w = __float_as_uint(acc4.w);
            __builtin_amdgcn_raw_buffer_store_b128(u, r_part, (int)((prow - a.PART + 4 + 4 * cq) * 4), 0, 16);
          }
          TQ(4)
        }
      } else {
        float mg = -INFINITY;
        if (tid >= nrow && tid < c4) scS[tid] = -INFINITY;        // pad the score vector for the float4 sweeps below
        __syncthreads();
        if (STOP && s_stop) return;
        TICK(13)
        {
          // pass 1: 16 lanes per row, two rows per trip; lane l covers floats 4l + 64c (conflict-free LDS reads)
          const int grp = tid >> 4, l16 = tid & 15;
          for (int t = grp; t < nrow; t += 32) {
            const int t2 = t + 16;
            const bool two = t2 < nrow;
            const float* e1 = encAS + t * H + 4 * l16;
            const float* e2 = encAS + (two ? t2 : t) * H + 4 * l16;
            float d1 = 0.f, d2 = 0.f;
  #pragma unroll
            for (int c = 0; c < 16; ++c) {
              if (64 * c < H) {                                     // wave-uniform: H is a multiple of 64, <= 1024
                const float4 hv = *reinterpret_cast<const float4*>(hS + 64 * c + 4 * l16);
                const float4 x1 = *reinterpret_cast<const float4*>(e1 + 64 * c);
                const float4 x2 = *reinterpret_cast<const float4*>(e2 + 64 * c);
                d1 += x1.x * hv.x + x1.y * hv.y + x1.z * hv.z + x1.w * hv.w;
                d2 += x2.x * hv.x + x2.y * hv.y + x2.z * hv.z + x2.w * hv.w;
              }
            }
  #pragma unroll
            for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
            if (l16 == 0) {
              scS[t] = d1 + ebS[t];
              if (two) scS[t2] = d2 + ebS[t2];
            }
          }
        }
        TQ(0)
        __syncthreads();
        TQ(1)
        // chunk max / exp / sum: every thread sweeps the (<= 256) scores with broadcast float4 LDS reads -- no shuffles
        for (int t = 0; t < nrow; t += 4) {
          const float4 v = *reinterpret_cast<const float4*>(scS + t);
          mg = fmaxf(fmaxf(mg, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
        m = mg;
        if (tid < c4) pS[tid] = tid < nrow ? expf(scS[tid] - m) : 0.f;
        my_score = tid < nrow ? scS[tid] : 0.f;
        TQ(2)
        __syncthreads();
        TQ(3)
        float cvp[4] = {0.f, 0.f, 0.f, 0.f};
        TICK(14)
        {
          // pass 2: context partial; thread owns columns tid + 256 j (consecutive threads -> consecutive LDS words); 4 rows per trip
          const int c0 = min(tid, H - 1), c1 = min(tid + 256, H - 1), c2 = min(tid + 512, H - 1), c3 = min(tid + 768, H - 1);
          for (int t = 0; t < nrow; t += 4) {
            const float4 pv = *reinterpret_cast<const float4*>(pS + t);      // rows beyond nrow have p = 0 and read the next slice rows
            l += (pv.x + pv.y) + (pv.z + pv.w);
            const float* e0 = encS + t * H;
            const int r1 = min(t + 1, nrow - 1) - t, r2 = min(t + 2, nrow - 1) - t, r3 = min(t + 3, nrow - 1) - t;
            cvp[0] += pv.x * e0[c0] + pv.y * e0[r1 * H + c0] + pv.z * e0[r2 * H + c0] + pv.w * e0[r3 * H + c0];
            if (H > 256) cvp[1] += pv.x * e0[c1] + pv.y * e0[r1 * H + c1] + pv.z * e0[r2 * H + c1] + pv.w * e0[r3 * H + c1];
            if (H > 512) {
              cvp[2] += pv.x * e0[c2] + pv.y * e0[r1 * H + c2] + pv.z * e0[r2 * H + c2] + pv.w * e0[r3 * H + c2];
              cvp[3] += pv.x * e0[c3] + pv.y * e0[r1 * H + c3] + pv.z * e0[r2 * H + c3] + pv.w * e0[r3 * H + c3];
            }
          }
  #pragma unroll
          for (int j = 0; j < 4; ++j)
            if (tid + 256 * j < H) st_sc1(&prow[4 + tid + 256 * j], cvp[j]);
          TQ(4)
        }
      }
      if (tid == 0) { st_sc1(&prow[0], m); st_sc1(&prow[1], l); }
      publish(ROWCTR(b));      // per-row counter: 8 arrivals instead of 128 on one word, and the combine waits for ITS row only
      TQ(5)
      if (a.tick_out) tk_att += wall_clock64() - ta0;
      if (!GR && tid < nrow) a.ALPHA[((long)s * B + b) * Tp + t0 + tid] = my_score;   // raw score, normalised by the backward (M, 1/L in ML)
      if constexpr (FD || BM) {
        if (a.ALPHA && tid < nrow) {        // raw score, normalised behind the loop (k_alpha_normalise)
          int t = tid;
          asm volatile("" : "+v"(t));
          *ua(a.ALPHA + ((long)s * B + b) * Tp + t0, (unsigned)t) = my_score;
        }
      }
      TICK(5)
    }
    if (has_ce && p6_pending >= 0) {       // P6 of the previous step, deferred behind this step's attention partial (see P6 below)
      if (!run_p6(p6_pending)) return;
      p6_pending = -1;
    }
    // ================= P3b: combine the nsplit partials of one batch row =================
    // TRAIN stores (max, 1 / sum) to ML; FD, BM: with ML given, likewise (k_alpha_normalise reads them behind the loop).
    if (has_cmb) {
      const int b = cmb_b, bt = b / 16;
      const int rows_bt = min(16, B - bt * 16);
      TICK(15)
      if (!wg_wait(ROWCTR(b), (unsigned)(a.nsplit * (s + 1)), a.ab, &s_flag, sc)) return;
      TICK(6)
      // No staging, no barrier: lane k of EVERY wave reads the header {max_k, sum_k} of partial k, the softmax weights of the
      // nsplit partials are formed with wave shuffles (identically in every wave), and thread tid < H/4 folds its four columns of the
      // nsplit partial context vectors straight from 16-byte sc1 loads (8 in flight) into one 16-byte write-through store.
      const long pbo = ((long)s * B + b) * a.nsplit * (H + 4);
      float mk = -INFINITY, lk = 0.f;
      if (lane < a.nsplit) {
        const float4 hd = ldb128_sc1(r_part, pbo + (long)lane * (H + 4));
        mk = hd.x; lk = hd.y;
      }
      const int cq = min(tid, H / 4 - 1);
      float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);
      float Mx = mk;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) Mx = fmaxf(Mx, __shfl_xor(Mx, o));
      const float wk_mine = lane < a.nsplit ? expf(mk - Mx) : 0.f;
      const float Ls = wave_sum(lk * wk_mine);
      const float inv = 1.f / Ls;
      for (int k0 = 0; k0 < a.nsplit; k0 += 8) {
        float4 pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = ldb128_sc1(r_part, pbo + (long)min(k0 + j, a.nsplit - 1) * (H + 4) + 4 + 4 * cq);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float wk = __shfl(wk_mine, min(k0 + j, 63));     // 0 for k >= nsplit
          const float wv = k0 + j < a.nsplit ? wk : 0.f;
          acc4.x += wv * pv[j].x; acc4.y += wv * pv[j].y; acc4.z += wv * pv[j].z; acc4.w += wv * pv[j].w;
        }
      }
      if (tid < H / 4) {
        u32q u;
        u.x = __float_as_uint(acc4.x * inv); u.y = __float_as_uint(acc4.y * inv); u.z = __float_as_uint(acc4.z * inv); u.w = __float_as_uint(acc4.w * inv);
        __builtin_amdgcn_raw_buffer_store_b128(u, r_cvh, (int)((((long)s * B + b) * 2 * H + 4 * tid) * 4), 0, 16);
      }
      publish_sh(CTR(PH_CMB, bt), b - bt * 16);
      TICK(7)
      if (!GR && tid == 0) { a.ML[((long)s * B + b) * 2] = Mx; a.ML[((long)s * B + b) * 2 + 1] = inv; }
      if constexpr (FD || BM) {
        if (a.ML && tid == 0) { float* ml = ua(a.ML + ((long)s * B + b) * 2, 0u); ml[0] = Mx; ml[1] = inv; }
      }
    }
    // ================= P4: ht = tanh(Wc [cv;h] + bc) =================
    if (has_c) {
      const int bt = c_bt, m0 = bt * 16;
      const int rows_bt = min(16, B - bt * 16);
      TICK(15)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const long crow = ((long)s * B + min(m0 + r16, B - 1)) * 2 * H;
      if constexpr (NC > 0) {
        // the h half of [cv ; h] was published by the cells long ago: its fragments (k-blocks NC..2NC-1 of each wave) and their MFMAs
        // run BEFORE the wait on the combine; only the cv half is fetched and multiplied behind it
        if (!wg_wait_sh(CTR(PH_CELL + TOP, bt), H / 8, s + 1, a.ab, &s_flag, sc)) return;
        {
          float4 ahd[NC];
          const int q = lane >> 4;
#pragma unroll
          for (int i = 0; i < NC; ++i) ahd[i] = ldb128_sc1(r_cvh, crow + 16 * (wave + 4 * (NC + i)) + 4 * q);
          __builtin_amdgcn_sched_barrier(0);
          mfma_blocks<NC>(acc, ahd, wreg + OFF_WC + NC);
        }
        if (!wg_wait_sh(CTR(PH_CMB, bt), rows_bt, s + 1, a.ab, &s_flag, sc)) return;
        TICK(8)
        {
          float4 acv[NC];
          const int q = lane >> 4;
#pragma unroll
          for (int i = 0; i < NC; ++i) acv[i] = ldb128_sc1(r_cvh, crow + 16 * (wave + 4 * i) + 4 * q);
          __builtin_amdgcn_sched_barrier(0);
          mfma_blocks<NC>(acc, acv, wreg + OFF_WC);
        }
      } else {
        if (!wg_wait_sh(CTR(PH_CMB, bt), rows_bt, s + 1, a.ab, &s_flag, sc)) return;
        TICK(8)
        wmac<NB_C>(acc, wreg + OFF_WC, r_cvh, crow, 2 * H, lane, wave);
      }
      const float v = reduce16(acc, red);
      const int row = m0 + (tid >> 4), n = c_n0 + (tid & 15);
      if (row < B) {
        const float ht = tanh_fast(v + a.bc[n]);
        st_sc1_u(a.HT + (long)(s + 1) * B * A, (unsigned)(row * A + n), ht);
        if (!GR && s + 1 < S) st_sc1_u(a.X0 + (long)(s + 1) * B * XI + E, (unsigned)(row * XI + n), ht);
      }
      publish_sh(CTR(PH_CTX, bt), c_n0 / 16);
      TICK(9)
    }
    // ================= P5: logits tiles + per-tile softmax statistics =================
    // TRAIN: the logits are stored; the tile record is (max, sum of exp(x - max), argmax, target logit).  GR: the record holds the maximum and
    // its index only (SUMS = false), unless SC: the sum and, with targets, the target logit too (the target is read in front of the wait); FD: a
    // step of this mode always has a target.
    // SM: perturbs the tempered logit xs = x * inv_temp with the noise of (row key, step, class) (common.h sample_gumbel) and keeps the tile's
    // winner by z = xs + g, xs at that winner, and the tile's sum of exp(xs - xs at the winner) (g lies in [-2.9, 16.7]: the winner's xs is
    // within 20 of the tile's largest, the sum cannot overflow) -- the four words of the tile record, as before.
    // BM: keeps what the scored mode keeps and stores the step's logits for P6's top-K passes.
    // TK: stores the step's tempered logits xs = x * inv_temp for P6 and nothing else: no noise over V, no tile record.
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (l_item[t] < 0) continue;
      const int bt = l_item[t] / a.ntile_v, tile = l_item[t] % a.ntile_v, m0 = bt * 16, n0 = tile * 16;
      TICK(15)
      [[maybe_unused]] int sc_tgt = -1;          // SC: this row's target of step s, read in front of the wait (-1: none)
      if constexpr (SC && !DRAW) {
        int r = m0 + (tid >> 4);
        asm volatile("" : "+v"(r));         // (keeps the address out of the loop-invariant registers: they are full, it would spill)
        if (a.ytgt && s + 1 < a.L && r < B) sc_tgt = *ua(a.ytgt + s + 1, (unsigned)(r * a.L));
        if constexpr (FD) sc_tgt = sc_tgt < 0 ? 0 : (sc_tgt >= V ? V - 1 : sc_tgt);      // (a step of this mode always has a target)
      }
      if (!wg_wait_sh(CTR(PH_CTX, bt), A / 16, s + 1, a.ab, &s_flag, sc)) return;
      TICK(10)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      wmac<NB_L>(acc, wreg + OFF_WL + t * NB_L, r_ht, ((long)(s + 1) * B + min(m0 + r16, B - 1)) * A, A, lane, wave);
      const float v = reduce16(acc, red);
      const int row = m0 + (tid >> 4), n = n0 + (tid & 15);
      const bool ok = row < B && n < V;
      float x = -INFINITY;
      if constexpr (GR) {      // (the bias address formed here: hoisted out of the step loop it is a 64-bit register pair per tile, and spills)
        int nn = n;
        asm volatile("" : "+v"(nn));
        if (ok) x = v + *ua(a.bo, (unsigned)nn);
      } else {
        x = ok ? v + a.bo[n] : -INFINITY;
      }
      if constexpr (BM) {      // (P6 sweeps the row for its K best: written through, in front of the tile's arrival)
        int rr = row, nn = n;
        asm volatile("" : "+v"(rr), "+v"(nn));
        if (ok) st_sc1_u(a.LOGITS + (long)s * B * a.Vp, (unsigned)(rr * a.Vp + nn), x);
      }
      if constexpr (TK) {      // (P6 draws from the row of xs = x * inv_temp: written through, in front of the tile's arrival; no tile record)
        int rr = row, nn = n;
        asm volatile("" : "+v"(rr), "+v"(nn));
        if (ok) st_sc1_u(a.LOGITS + (long)s * B * a.Vp, (unsigned)(rr * a.Vp + nn), x * a.inv_temp);
        publish_sh(CTR(PH_LOG, bt), tile);
        TICK(11)
        continue;
      }
      if (!GR) {       // (GR: P6 needs the tile's maximum and its index only)
        if (ok) *ua(a.LOGITS + (long)s * B * a.Vp, (unsigned)(row * a.Vp + n)) = x;
        else if (row < B && n < a.Vp) *ua(a.LOGITS + (long)s * B * a.Vp, (unsigned)(row * a.Vp + n)) = 0.f;
      }
      float mx = x;
      int mi = n;
      float se = 0.f, xt = 0.f;
      if constexpr (SM) {
        // the draw: the tile's first maximum of z = xs + g; xt = xs at that winner, the reference of the tile's sum of exponentials
        const float xs = x * a.inv_temp;                     // (-inf stays -inf: inv_temp > 0)
        mx = ok ? xs + sample_gumbel(sm_row_keys()[row & (PDEC_SM_ROWS - 1)], s, n) : -INFINITY;      // (the key from LDS, here: 64 bits held over the wait spill)
        xt = xs;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          const float om = __shfl_xor(mx, o), ox = __shfl_xor(xt, o);
          const int oi = __shfl_xor(mi, o);
          if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; xt = ox; }
        }
        se = ok ? expf(xs - xt) : 0.f;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o);
      } else {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          const float om = __shfl_xor(mx, o);
          const int oi = __shfl_xor(mi, o);
          if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
        }
        if constexpr (SUMS) {
          se = ok ? expf(x - mx) : 0.f;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o);
          int tgt;
          if constexpr (SC) tgt = sc_tgt;
          else tgt = row < B ? *ua(a.ytgt + s + 1, (unsigned)(row * a.L)) : 0;
          xt = (ok && n == tgt) ? x : 0.f;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) xt += __shfl_xor(xt, o);
        }
      }
      if ((tid & 15) == 0 && row < B) {
        float* cs = ua(a.CESTAT + ((long)s * B * a.ntile_v + tile) * 4, (unsigned)(row * a.ntile_v * 4));
        st_sc1(cs, mx); st_sc1(cs + 1, se); st_sc1(cs + 2, __int_as_float(mi)); st_sc1(cs + 3, xt);
      }
      publish_sh(CTR(PH_LOG, bt), tile);
      TICK(11)
    }
    // ================= P6: cross-entropy combine per batch tile =================
    // The CE workgroups also own attention items of the NEXT step's chain.  P6(s) ends ~4 us after h_{s+1} is there (it waits for the
    // last logits tile), so run in program order it delayed those attention partials -- and with them their batch rows' combine, the
    // whole batch tile's ht and every later step -- by 3.3 us per decoder step (phase stamps: the combine of row 31 waited 4.8 us for
    // its partials, that of row 0 1.5 us).  Nothing on the chain needs P6(s) when step s+1 is teacher-forced (its token is the truth):
    // it is then DEFERRED behind the workgroup's P3 of step s+1.  When step s+1 feeds the argmax back its cells wait for PH_CE(s)
    // anyway and P6(s) runs in place (deferring it there would dead-lock: P3(s+1) waits for cells that wait for P6(s)).
    if (has_ce) {
      bool defer;
      if constexpr (FD) defer = s + 1 < S;                           // (FD: no step does)
      else defer = !GR && s + 1 < S && flagS[s + 1] != 0;            // (GR: every step feeds its argmax back)
      if (defer) p6_pending = s;
      else if (!run_p6(s)) return;
    }
  }
  if (has_ce && p6_pending >= 0) { if (!run_p6(p6_pending)) return; }
  if (a.tick_out && tid == 0 && has_att) {     // attention phase = hand-off satisfied -> partial published (10 ns ticks -> us)
    atomicAdd(&a.tick_out[wg], (float)tk_att * 0.01f / (float)S);
    if (wg == 0) atomicAdd(&a.tick_out[G], 1.0f);
  }
  if (timing && tid == 0 && (wg == 0 || wg == n_cell || wg == G - B || wg == G - 1))
    printf("pdec wg %3d per-step 10ns: P1[pre %lld waitctx %lld ht+epi %lld publish %lld] P3[wait %lld work %lld] P3b[wait %lld work %lld] "
           "P4[wait %lld work %lld] P5[wait %lld work %lld] P6 %lld other %lld | P3: hload %lld pass1+max %lld\n", wg, tk[0] / S, tk[1] / S, tk[2] / S, tk[3] / S,
           tk[4] / S, tk[5] / S, tk[6] / S, tk[7] / S, tk[8] / S, tk[9] / S, tk[10] / S, tk[11] / S, tk[12] / S, tk[15] / S, tk[13] / S, tk[14] / S);
  if (timing && tid == 0 && (wg == 0 || wg == G - 1))
    printf("pdec-att wg %3d per-step 10ns: pass1 %lld barrier %lld max+exp %lld barrier %lld pass2+stores %lld publish %lld\n", wg, tq[0] / S, tq[1] / S,
           tq[2] / S, tq[3] / S, tq[4] / S, tq[5] / S);
#undef TICK
#undef TQ
#undef CTR
#undef ROWCTR
}

// greedy modes: the last workgroup to leave -- after every stop, abort or time-out of the launch -- writes n_steps and the status copy
__device__ __forceinline__ void greedy_last_out(const PDecArgs& a) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && __hip_atomic_fetch_add(a.gctl + 2 * CTRS, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == (unsigned)G) {
    *a.n_steps_out = (int32_t)__hip_atomic_load(a.gctl + 3 * CTRS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.status_dst) *a.status_dst = (float)__hip_atomic_load(a.ab.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int NC, int NL, bool XS, bool GR>
__global__ __launch_bounds__(256, 1) void decoder_persist_fwd(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, GR ? PDEC_GREEDY : PDEC_TRAIN>(a);     // (every return in it is workgroup-uniform)
  if constexpr (GR) greedy_last_out(a);
}

// The scored greedy mode as a kernel of its own: the instantiations above keep their names and their code.
template <int NC, int NL, bool XS>
__global__ __launch_bounds__(256, 1) void decoder_persist_greedy_scored(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, PDEC_SCORED>(a);
  greedy_last_out(a);
}

// The sampled mode as a kernel of its own, likewise: the greedy modes' control words and exit as they are.
template <int NC, int NL, bool XS>
__global__ __launch_bounds__(256, 1) void decoder_persist_sampled(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, PDEC_SAMPLED>(a);
  greedy_last_out(a);
}

// The truncated sampled mode (top-k / nucleus) as a kernel of its own, likewise.
template <int NC, int NL, bool XS>
__global__ __launch_bounds__(256, 1) void decoder_persist_sampled_topk(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, PDEC_TOPK>(a);
  greedy_last_out(a);
}

// The beam mode as a kernel of its own, likewise.
template <int NC, int NL, bool XS>
__global__ __launch_bounds__(256, 1) void decoder_persist_beam(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, PDEC_BEAM>(a);
  greedy_last_out(a);
}

// Behind the beam loop: the final state of every slot = c, h and ht of the step and row its hypothesis was last expanded from
// (org = step * B + row; -1, an empty slot: zeros).  One workgroup per row.
struct BeamFinalArgs {
  const int32_t* org;
  const float *CS[PDEC_MAX_LAYERS], *HR[PDEC_MAX_LAYERS], *HT;
  float *c_fin, *h_fin, *ht_fin;
  int B, H, A, nl;
};
__global__ __launch_bounds__(256) void k_beam_final_states(BeamFinalArgs a) {
  const int r = blockIdx.x, o = a.org[r], B = a.B, H = a.H;
  const long src = o < 0 ? 0 : ((long)(o / B + 1) * B + o % B);
  for (int l = 0; l < a.nl; ++l)
    for (int k = threadIdx.x; k < H; k += 256) {
      a.c_fin[((long)l * B + r) * H + k] = o < 0 ? 0.f : a.CS[l][src * H + k];
      a.h_fin[((long)l * B + r) * H + k] = o < 0 ? 0.f : a.HR[l][src * H + k];
    }
  for (int k = threadIdx.x; k < a.A; k += 256) a.ht_fin[(long)r * a.A + k] = o < 0 ? 0.f : a.HT[src * a.A + k];
}

// out[b][n] = the Gumbel noise of (row_keys[b], step, n), n < V: one decoder step's draws as a dense (B, V) buffer, through the function
// the loop's P5 calls (the per-step sampled loop and the tests read it)
__global__ __launch_bounds__(256) void k_gumbel_rows(const uint64_t* __restrict__ row_keys, int step, int V, float* __restrict__ out) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n < V) out[(long)b * V + n] = sample_gumbel(row_keys[b], step, n);
}

// The forced mode as a kernel of its own, likewise.  Of the greedy modes' control words it keeps one, the exit count (gctl[2]): the last
// workgroup to leave writes the status copy.  It is an arrival at the end of the kernel that nothing waits for.
template <int NC, int NL, bool XS>
__global__ __launch_bounds__(256, 1) void decoder_persist_forced(PDecArgs a) {
  decoder_persist_fwd_body<NC, NL, XS, PDEC_FORCED>(a);
  if (!a.status_dst) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && __hip_atomic_fetch_add(a.gctl + 2 * CTRS, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == (unsigned)G)
    *a.status_dst = (float)__hip_atomic_load(a.ab.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// alpha[r][t] = exp(score[r][t] - M[r]) / L[r], r = (step, row), t < T: the raw scores of the forced loop (rows of Tp floats) into the
// caller's dense (S, B, T) buffer.  With lengths (row_len[b], b = r % B, or null) the loop stored scores for t < row_len[b] only: alpha is
// an exact 0 from there on
__global__ __launch_bounds__(256) void k_alpha_normalise(const float* __restrict__ raw, const float* __restrict__ ml, float* __restrict__ alpha,
                                                         const int32_t* __restrict__ row_len, int B, int T, int Tp) {
  const long r = blockIdx.x;
  const float M = ml[2 * r], inv = ml[2 * r + 1];
  const int n = row_len ? min(T, row_len[r % B]) : T;
  for (int t = threadIdx.x; t < T; t += 256) alpha[r * T + t] = t < n ? expf(raw[r * Tp + t] - M) * inv : 0.f;
}

// =====================================================================================================================
// Backward loop.  Phases per step (s descending; n = S-1-s steps already done):
//   B1 d_pre = (dlogits Wo + d_ht carried from step s+1) (1 - ht^2)      items (bt, 16 cols of A)
//   B2 d_cvh = d_pre Wc  -> d_cv | dh (direct part)                      items (bt, 32 cols of 2H)
//   B3 attention backward over the LDS-resident slices:  ds = alpha (enc.d_cv - cv.d_cv) ; dh_att partial = sum_t ds encA
//   B5 cell backward: dh = mask (dh_direct + sum_splits dh_att) + dz_{s+1} Wl ; dz ; dc carried in a register
//      NL > 1: one B5 per layer, top first.  A layer below the top takes the gradient of its dropped output from the layer above by
//      multiplying dz_{l+1,s} with its 16 columns of Wu_{l+1} ITSELF (no separate d_x phase, one hand-off per layer):
//      dh_l = mask_l (dz_{l+1,s} Wu_{l+1}) + dz_{l,s+1} Wl_l
//   B6 d_x0 = dz_0 Wu_0  (its [E:] half is the d_ht carry of step s-1)   items (bt, 16 cols of E+A)
// Products that do not depend on the current step's chain (dlogits Wo in B1, dz_{s+1} Wl in B5) run before the wait.
// Weight gradients, d_enc, dq and d_embed are batched products over all steps after the loop (decoder.hip).
enum BPhase { PB1 = 0, PB2, PB5 /* + layer: 0..2 */, PB5_1, PB5_2, PB6, PB_N };

// The forms of the d_x0 role (PDecBwdArgs::b6_split; the older two are kept behind the knobs dec.b6_split / dec.b6_fused for A/B runs):
//   B6_WHOLE  one layer only: B6 items of 16 columns of all of d_x0, handing the carry to the B1 items
//   B6_SPLIT  B6 covers only the ht columns, every item split into two K halves (the embedding columns are one batched GEMM after
//             the launch)
//   B6_FUSED  no B6 role and no d_pre hand-off: the B1 items (two K halves each) add dz_{s+1} Wu[:, ht cols] to their half of
//             dlogits Wo and leave the two partial pre-activations in DXH; B2 forms d_pre = (p0 + p1) (1 - ht^2) while it loads its
//             operand (two hand-offs less on the chain; the embedding columns as under B6_SPLIT)
enum B6Form { B6_WHOLE = 0, B6_SPLIT = 1, B6_FUSED = 2 };

// The backward role layout, stated once: workgroups per role and whether they fit the G of the grid.
//   NL == 1: [0, n5) cell backward, then n6 of d_x0, then d_pre and d_cvh on the same max(n1, n2) workgroups; B6_FUSED: n1 half-items of
//            the pre-activation, then n2 of d_cvh on workgroups of their own.
//   NL > 1:  [l n5, (l + 1) n5) cell backward of layer l; d_pre and d_cvh on the last max(n1, n2) workgroups; the split d_x0 items on the
//            last n6, never on a workgroup that also holds the 64 float4 of a below-top cell backward.  B6_FUSED: the half-items on the
//            last n1 -- top-layer cell owners among them, never a lower layer's -- and d_cvh on the last n2, none of which owns a cell.
struct PDecBwdRoles {
  int n5, n6, n1, n2;       // cell backward (per layer), d_x0, d_pre (B6_FUSED: its half-items), d_cvh
  bool fits;
};
inline PDecBwdRoles pdec_bwd_roles(int nbt, int H, int A, int XI, int n_layers, int form) {
  PDecBwdRoles r;
  r.n5 = nbt * (H / 16);
  r.n6 = form == B6_FUSED ? 0 : (form == B6_SPLIT ? 2 * nbt * (A / 16) : nbt * (XI / 16));
  r.n1 = (form == B6_FUSED ? 2 : 1) * nbt * (A / 16);
  r.n2 = nbt * (2 * H / 32);
  const int n12 = r.n1 > r.n2 ? r.n1 : r.n2, below = (n_layers - 1) * r.n5;
  if (form == B6_FUSED) r.fits = n_layers == 1 ? r.n5 + r.n1 + r.n2 <= G : (below + r.n1 <= G && below + r.n5 + r.n2 <= G);
  else if (n_layers == 1) r.fits = r.n5 + r.n6 + n12 <= G;
  else r.fits = form == B6_SPLIT && below + r.n5 + n12 <= G && r.n6 <= G - below;
  return r;
}

struct PDecBwdArgs {
  int B, S, L, T, Tp, H, E, A, V, Vp, XI, nbt, nsplit, chunk;
  int NL;
  const float *WoT, *WcT;                  // (A,Vp) (2H,A)
  const float *WlT[PDEC_MAX_LAYERS], *WuT[PDEC_MAX_LAYERS];      // per layer: (H,4H), (in,4H) with in = XI for layer 0, H above
  const float *enc, *encA;
  const float *CVH, *HT, *LOGITS, *ML;
  const float *Cst[PDEC_MAX_LAYERS], *rnn_mask[PDEC_MAX_LAYERS];
  float *ALPHA;                            // raw scores in, normalised alpha out
  float *Gt[PDEC_MAX_LAYERS];              // gates -> dz
  float *DPRE, *DCVH, *DS, *DX0, *DHATT;   // DHATT [S][B][nsplit][H]
  float* DXH;                              // B6_SPLIT, B6_FUSED: [2][S][B][A] K-halves of d_x0[:, E:] (the carry of the next step's B1)
  int b6_split;                            // a B6Form (an int here: the argument's offset is part of the machine code)
  float *d_c0;                             // [NL][B][H]
  unsigned* ctr;
  AbortCtl ab;
  int dbg;
  float* tick_out;
};

constexpr int NB_B1 = 18, NB_B2 = 8, NB_B5 = 32, NB_B6 = 32;     // k-blocks per wave: Vp <= 1152, A <= 512, 4H <= 2048
constexpr int NWB = 36;
// NL > 1: B5 of layer l on workgroups [l n5, (l+1) n5) with Wl_l^T rows in [0, 32) and (below the top) Wu_{l+1}^T rows in [32, 64);
// B1/B2 on the last max(n1, n2) workgroups in [0, 34); the split B6 items on the last n6 workgroups in [48, 64)
constexpr int NWB_ML = 64, OFF_B5UP = NB_B5, OFF_B6_ML = 48;

// acc += A . W over NB blocks, A fetched in chunks of CH blocks (bounds the live A registers)
template <int NB, int CH>
__device__ __forceinline__ void wmac_chunked(f32x4& acc, const float4* w, __amdgpu_buffer_rsrc_t ra, long a_off, int K, int lane, int wave) {
#pragma unroll
  for (int c0 = 0; c0 < NB; c0 += CH) {
    if (c0 > 0 && 64 * c0 >= K) break;     // a chunk wholly beyond K (narrow models in the full-width register layout): its round trip
                                           // would sit on the chain for nothing
    float4 a[CH];
    aload_sc1<CH>(a, ra, a_off, K, lane, wave, c0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_blocks<CH>(acc, a, w + c0);
  }
}

// Vector pieces of the backward kernel, all by value: a float4 taken by reference is not a function the optimiser leaves no trace of
// (DESIGN.md section 29).  as_u32q: the operand of a 16-byte buffer store (as in lstm_persist.hip); dot4, fma4: the four-term dot product
// and the four-lane multiply-add of the H = 512 attention phase (B3); dpre4: d_pre = (p0 + p1) (1 - ht^2) of the fused form's B2
template <class V> __device__ __forceinline__ u32q as_u32q(const V v) { return __builtin_bit_cast(u32q, v); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 fma4(float4 acc, const float g, const float4 e) {
  acc.x += g * e.x; acc.y += g * e.y; acc.z += g * e.z; acc.w += g * e.w;
  return acc;
}
__device__ __forceinline__ float4 dpre4(const float4 p0, const float4 p1, const float4 y) {
  return make_float4((p0.x + p1.x) * (1.f - y.x * y.x), (p0.y + p1.y) * (1.f - y.y * y.y), (p0.z + p1.z) * (1.f - y.z * y.z), (p0.w + p1.w) * (1.f - y.w * y.w));
}

template <int NC, int NL, bool XS>   // as in decoder_persist_fwd
__global__ __launch_bounds__(256, 1) void decoder_persist_bwd(PDecBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ __attribute__((aligned(16))) float red[4 * 256];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = blockIdx.x;
  const int B = a.B, S = a.S, H = a.H, E = a.E, A = a.A, XI = a.XI, T = a.T, Tp = a.Tp, Vp = a.Vp;
  const int nbt = a.nbt, K4 = 4 * H;
  unsigned* ctr = a.ctr;
#define CTR(ph, bt) (ctr + ((ph) * nbt + (bt)) * NSH * CTRS)
#define ROWCTR(row) (ctr + ((long)NPHASE_SLOTS * NSH * nbt + 2 + (row)) * CTRS)
  // ---------------- roles: the layout of pdec_bwd_roles, which states the counts below and what the launcher checked before it chose the
  // form (these lines must match it: n1 here is the count of whole d_pre items, n1f that function's n1); attention: all workgroups
  constexpr int TOP = NL - 1;
  const bool fused6 = a.b6_split == B6_FUSED;
  const int n5 = nbt * (H / 16), n6 = fused6 ? 0 : (a.b6_split != B6_WHOLE ? 2 * nbt * (A / 16) : nbt * (XI / 16)), n1 = nbt * (A / 16), n2 = nbt * (2 * H / 32);
  const int n12 = n1 > n2 ? n1 : n2;
  const bool has5 = wg < NL * n5;
  const int b5_l = has5 ? wg / n5 : 0, b5_i = has5 ? wg % n5 : 0;
  const int b5_bt = b5_i / (H / 16), b5_u0 = (b5_i % (H / 16)) * 16;
  const int r6 = NL > 1 ? wg - (G - n6) : wg - n5;
  const bool has6 = r6 >= 0 && r6 < n6;
  // B6 item: 16 columns of d_x0 for one batch tile; split mode: ht columns only, item (r6 >> 1), K half (r6 & 1)
  const int b6_half = a.b6_split != B6_WHOLE ? (r6 & 1) : 0;
  const int b6_item = a.b6_split != B6_WHOLE ? (r6 >> 1) : r6;
  const int b6_per_bt = a.b6_split != B6_WHOLE ? A / 16 : XI / 16;
  const int b6_bt = has6 ? b6_item / b6_per_bt : 0, b6_n0 = has6 ? (a.b6_split != B6_WHOLE ? E : 0) + (b6_item % b6_per_bt) * 16 : 0;
  const int b6_k0 = b6_half * (K4 / 2);
  // fused form: 2 n1 half-items of the pre-activation, on other workgroups than the d_cvh items
  const int n1f = fused6 ? 2 * n1 : n1;
  const int r1 = fused6 ? (NL > 1 ? wg - (G - n1f) : wg - n5) : (NL > 1 ? wg - (G - n12) : wg - n5 - n6);
  const bool has1 = r1 >= 0 && r1 < n1f;
  const int b1_half = fused6 ? (r1 & 1) : 0, b1_item = fused6 ? (r1 >> 1) : r1;
  const int b1_bt = has1 ? b1_item / (A / 16) : 0, b1_n0 = has1 ? (b1_item % (A / 16)) * 16 : 0;
  constexpr int KV_HALF = 64 * (NB_B1 / 2);          // fused form: dlogits Wo split at this k (9 k-blocks per wave and half)
  const int b1_kv0 = b1_half * KV_HALF, b1_kvn = b1_half ? Vp - KV_HALF : min(Vp, KV_HALF);
  // (NL > 1: the pre-activation half-items on the last 2 n1 workgroups -- top-layer cell owners among them, never a lower layer's --
  //  and the d_cvh items on the last n2, none of which owns a cell: pdec_bwd_roles(.., B6_FUSED).fits says both)
  const int r2 = fused6 ? (NL > 1 ? wg - (G - n2) : wg - n5 - n1f) : r1;
  const bool has2 = r2 >= 0 && r2 < n2;
  const int b2_bt = has2 ? r2 / (2 * H / 32) : 0, b2_n0 = has2 ? (r2 % (2 * H / 32)) * 32 : 0;
  const int n_att = B * a.nsplit;
  const bool has_att = wg < n_att;
  const int att_b = has_att ? wg % B : 0, att_sp = has_att ? wg / B : 0;

  constexpr int NW = NL > 1 ? NWB_ML : NWB;
  constexpr int OFF_B6 = NL > 1 ? OFF_B6_ML : 0;
  // fused form: the pre-activation half-item's 9 + 16 blocks.  NL > 1: behind the d_cvh item's blocks [NB_B1, NB_B1 + 2 NB_B2) and a
  // top-layer cell owner's [0, NB_B5), either of which the same workgroup may hold
  constexpr int OFF_B1F = NL > 1 ? NB_B1 + 2 * NB_B2 : 0;
  static_assert(OFF_B1F + NB_B1 / 2 + NB_B6 / 2 <= NW && NB_B5 <= NB_B1 + 2 * NB_B2, "fused pre-activation fragments");
  float4 wreg[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) wreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r16 = lane & 15;
  if (has5) {
    wload<NB_B5>(wreg, a.WlT[b5_l], K4, b5_u0 + r16, K4, lane, wave);
    if constexpr (NL > 1) {
      if (b5_l < TOP) wload<NB_B5>(wreg + OFF_B5UP, a.WuT[b5_l + 1], K4, b5_u0 + r16, K4, lane, wave);
    }
  }
  if (has6 && (NL > 1 || !has5)) {
    if (a.b6_split != B6_WHOLE) wload<NB_B6 / 2>(wreg + OFF_B6, a.WuT[0] + b6_k0, K4, b6_n0 + r16, K4 / 2, lane, wave);
    else wload<NB_B6>(wreg + OFF_B6, a.WuT[0], K4, b6_n0 + r16, K4, lane, wave);
  }
  if (fused6) {
    if (has1) {
      wload<NB_B1 / 2>(wreg + OFF_B1F, a.WoT + b1_kv0, Vp, b1_n0 + r16, b1_kvn, lane, wave);
      wload<NB_B6 / 2>(wreg + OFF_B1F + NB_B1 / 2, a.WuT[0] + b1_half * (K4 / 2), K4, E + b1_n0 + r16, K4 / 2, lane, wave);
    }
    if (has2) {
      wload<NB_B2>(wreg + NB_B1, a.WcT, A, b2_n0 + r16, A, lane, wave);
      wload<NB_B2>(wreg + NB_B1 + NB_B2, a.WcT, A, b2_n0 + 16 + r16, A, lane, wave);
    }
  } else if (!has5 && (NL > 1 || !has6)) {
    if (has1) wload<NB_B1>(wreg, a.WoT, Vp, b1_n0 + r16, Vp, lane, wave);
    if (has2) {
      wload<NB_B2>(wreg + NB_B1, a.WcT, A, b2_n0 + r16, A, lane, wave);
      wload<NB_B2>(wreg + NB_B1 + NB_B2, a.WcT, A, b2_n0 + 16 + r16, A, lane, wave);
    }
  }
  const int t0 = att_sp * a.chunk, t1 = min(T, t0 + a.chunk);
  const int nrow = has_att ? t1 - t0 : 0;
  const int cres = NC > 0 ? min(a.chunk, PDEC_RES_ROWS) : a.chunk;      // rows of the slice kept in LDS (as in the forward kernel)
  const int nres = min(nrow, cres);
  float* encS = lds;
  float* encAS = lds + cres * H;
  float* scr = lds + 2 * cres * H;           // dS[H] (d_cv) | cvS[H] | ds[chunk] | wred[8]
  const float* gEnc = a.enc + ((long)att_b * T + t0) * H;
  const float* gEncA = a.encA + ((long)att_b * T + t0) * H;
  if (has_att) {
    const int n4 = nres * H / 4;
    for (int i = tid; i < n4; i += 256) {
      reinterpret_cast<float4*>(encS)[i] = reinterpret_cast<const float4*>(gEnc)[i];
      reinterpret_cast<float4*>(encAS)[i] = reinterpret_cast<const float4*>(gEncA)[i];
    }
  }
  __syncthreads();
  const __amdgpu_buffer_rsrc_t r_dl = make_rsrc(a.LOGITS), r_dpre = make_rsrc(a.DPRE), r_dcvh = make_rsrc(a.DCVH),
                               r_g = make_rsrc(a.Gt[b5_l]), r_g0 = make_rsrc(a.Gt[0]), r_dx0 = make_rsrc(a.DX0), r_dha = make_rsrc(a.DHATT);
  const int e_row = tid >> 4, e_col = tid & 15;
  float dc_state = 0.f;
  long long tk_att = 0;
  long long tb[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) tb[i] = 0;
  const bool timing = (NL == 1 || ASTK_PDEC_TIMING_ALL) && PERSIST_DBG(a) != 0;
  long long tlast = timing ? wall_clock64() : 0;
#define TB(i) if (timing) { const long long now_ = wall_clock64(); tb[i] += now_ - tlast; tlast = now_; }

  for (int s = S - 1; s >= 0; --s) {
    const int n = S - 1 - s;
    // ================= B1 =================
    if (has1) {
      const int bt = b1_bt, m0 = bt * 16;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int row = m0 + e_row, col = b1_n0 + e_col;
      if (fused6) {
        // this half of dlogits Wo (no dependency on the chain), then -- in the same accumulators -- this half of the carry
        // d_x0[s+1][:, E + col] = dz_{0,s+1} Wu_0[:, E + col]: the cell backward of step s+1 hands its dz straight to this product
        if (b1_kvn > 0) wmac_chunked<NB_B1 / 2, 9>(acc, wreg + OFF_B1F, r_dl, ((long)s * B + min(m0 + r16, B - 1)) * Vp + b1_kv0, b1_kvn, lane, wave);
        TB(0)
        if (n > 0) {
          if (!wg_wait_sh(CTR(PB5, bt), H / 16, n, a.ab, &s_flag)) return;
          TB(1)
          wmac_chunked<NB_B6 / 2, 16>(acc, wreg + OFF_B1F + NB_B1 / 2, r_g0, ((long)(s + 1) * B + min(m0 + r16, B - 1)) * K4 + b1_half * (K4 / 2), K4 / 2, lane, wave);
        }
        const float v = reduce16(acc, red);
        if (row < B) st_sc1(a.DXH + ((long)(b1_half * S + s) * B + row) * A + col, v);
      } else {
        wmac_chunked<NB_B1, 9>(acc, wreg, r_dl, ((long)s * B + min(m0 + r16, B - 1)) * Vp, Vp, lane, wave);   // no dependency on the chain
        const float v = reduce16(acc, red);
        float carry = 0.f;
        TB(0)
        if (n > 0) {
          if (!wg_wait_sh(CTR(PB6, bt), a.b6_split != B6_WHOLE ? 2 * (A / 16) : XI / 16, n, a.ab, &s_flag)) return;
          TB(1)
          if (row < B) {
            if (a.b6_split != B6_WHOLE) {
              const float c0 = ld_sc1(a.DXH + ((long)(s + 1) * B + row) * A + col);
              const float c1 = ld_sc1(a.DXH + ((long)(S + s + 1) * B + row) * A + col);
              carry = c0 + c1;
            } else carry = ld_sc1(a.DX0 + ((long)(s + 1) * B + row) * XI + E + col);
          }
        }
        if (row < B) {
          const float y = a.HT[((long)(s + 1) * B + row) * A + col];
          st_sc1(a.DPRE + ((long)s * B + row) * A + col, (v + carry) * (1.f - y * y));
        }
      }
      publish_sh(CTR(PB1, bt), fused6 ? 2 * (b1_n0 / 16) + b1_half : b1_n0 / 16);
      TB(2)
    }
    // ================= B2 =================
    if (has2) {
      const int bt = b2_bt, m0 = bt * 16;
      TB(15)
      float4 av[NB_B2];
      if (fused6) {
        // d_pre = (p0 + p1) (1 - ht^2) formed on the operand fragments; ht fetched in front of the wait; every item leaves its share
        // of the 4 NB_B2 fragments of d_pre for the weight gradients behind the launch
        float4 yv[NB_B2], p1[NB_B2];
        const __amdgpu_buffer_rsrc_t r_ht = make_rsrc(a.HT), r_dxh = make_rsrc(a.DXH);
        const long rowo = (long)s * B + min(m0 + r16, B - 1);
        aload_sc1<NB_B2, 0>(yv, r_ht, (rowo + B) * A, A, lane, wave);
        if (!wg_wait_sh(CTR(PB1, bt), 2 * (A / 16), n + 1, a.ab, &s_flag)) return;
        TB(3)
        aload_sc1<NB_B2>(av, r_dxh, rowo * A, A, lane, wave);
        aload_sc1<NB_B2>(p1, r_dxh, ((long)S * B + rowo) * A, A, lane, wave);
        const int nb2 = 2 * H / 32, my = b2_n0 / 32;
#pragma unroll
        for (int i = 0; i < NB_B2; ++i) {
          av[i] = dpre4(av[i], p1[i], yv[i]);
          const int k = 16 * (wave + 4 * i) + 4 * (lane >> 4);
          if ((wave * NB_B2 + i) % nb2 == my && k < A && m0 + r16 < B) *reinterpret_cast<float4*>(a.DPRE + rowo * A + k) = av[i];
        }
      } else {
        if (!wg_wait_sh(CTR(PB1, bt), A / 16, n + 1, a.ab, &s_flag)) return;
        TB(3)
        aload_sc1<NB_B2>(av, r_dpre, ((long)s * B + min(m0 + r16, B - 1)) * A, A, lane, wave);
      }
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      mfma_blocks<NB_B2>(acc0, av, wreg + NB_B1);
      mfma_blocks<NB_B2>(acc1, av, wreg + NB_B1 + NB_B2);
      const float v0 = reduce16(acc0, red);
      const float v1 = reduce16(acc1, red);
      const int row = m0 + e_row;
      if (row < B) {
        st_sc1(a.DCVH + ((long)s * B + row) * 2 * H + b2_n0 + e_col, v0);
        st_sc1(a.DCVH + ((long)s * B + row) * 2 * H + b2_n0 + 16 + e_col, v1);
      }
      publish_sh(CTR(PB2, bt), b2_n0 / 32);
      TB(4)
    }
    // ================= B5, the part that does not depend on this step's chain: dh_rec = dz_{s+1} Wl and the saved forward state.
    // In FRONT of the attention phase in program order: dz_{s+1} has been there since the previous step's cell backward, and a cell
    // workgroup that started this product only after its own attention item kept its batch tile's dz -- the whole chain -- waiting
    // for it (5 us per step in the phase timers) =================
    float v = 0.f;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    float ccur = 0.f, cp = 0.f, mk = 1.f;
    if (has5) {
      const int bt = b5_bt, m0 = bt * 16, l = b5_l;
      TB(15)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (n > 0) {
        if (!wg_wait_sh(CTR(PB5 + l, bt), H / 16, n, a.ab, &s_flag)) return;
        wmac_chunked<NB_B5, 16>(acc, wreg, r_g, ((long)(s + 1) * B + min(m0 + r16, B - 1)) * K4, K4, lane, wave);
      }
      v = reduce16(acc, red);
      const int row = m0 + e_row, u = b5_u0 + e_col;
      if (row < B) {
        g = *reinterpret_cast<const float4*>(a.Gt[l] + ((long)s * B + row) * K4 + 4 * u);
        ccur = a.Cst[l][((long)(s + 1) * B + row) * H + u];
        cp = a.Cst[l][((long)s * B + row) * H + u];
        if (a.rnn_mask[l]) mk = a.rnn_mask[l][((long)s * B + row) * H + u];
      }
      TB(6)
    }
    // ================= B3: attention backward =================
    if (has_att) {
      const int b = att_b, bt = b / 16;
      long long tb0 = 0;
      TB(15)
      if constexpr (NC > 0) {
        // ---- specialised scan (H = 64 NC, nrow <= 60; rows >= nres come from global memory): everything that does not depend on this
        // step's chain (alpha from the saved raw scores, cv) is fetched BEFORE the wait; every read of a pass is issued before its first use
        constexpr int HH = 64 * NC;
        const int nx = XS ? nrow - nres : 0;
        float* dS = scr;                       // d_cv[b][:]
        float* dsS = scr + 2 * HH;             // ds[64] (tail 0)
        float* aS = dsS + 64;                  // alpha[64] (tail 0)
        float* wred = aS + 64;                 // [8]
        float4* fold = reinterpret_cast<float4*>(scr + 2 * HH + 160);
        float* al = a.ALPHA + ((long)s * B + b) * Tp + t0;
        float a_t = 0.f;
        float4 cv4 = make_float4(0.f, 0.f, 0.f, 0.f);
        {
          const float mlM = a.ML[((long)s * B + b) * 2], mlI = a.ML[((long)s * B + b) * 2 + 1];
          const float raw = al[min(tid, nrow - 1)];
          if (tid < HH / 4) cv4 = *reinterpret_cast<const float4*>(a.CVH + ((long)s * B + b) * 2 * HH + 4 * tid);
          a_t = tid < nrow ? expf(raw - mlM) * mlI : 0.f;
        }
        if (!wg_wait_sh(CTR(PB2, bt), 2 * H / 32, n + 1, a.ab, &s_flag)) return;
        tb0 = a.tick_out ? wall_clock64() : 0;
        float cdp = 0.f;                       // cv . d_cv
        if (tid < HH / 4) {
          const float4 d4 = ldb128_sc1(r_dcvh, ((long)s * B + b) * 2 * HH + 4 * tid);
          *reinterpret_cast<float4*>(dS + 4 * tid) = d4;
          cdp = dot4(cv4, d4);
        }
        cdp = wave_sum(cdp);
        if (lane == 0) wred[wave] = cdp;
        if (tid < 64) { aS[tid] = a_t; dsS[tid] = 0.f; }
        if (tid < nrow) al[tid] = a_t;          // normalised alpha for the deferred d_enc product (off the chain)
        __syncthreads();
        const float cd = wred[0] + wred[1] + wred[2] + wred[3];
        {
          const int grp = tid >> 4, l16 = tid & 15;
          const int ta = min(grp, nres - 1), tb2 = min(grp + 16, nres - 1);
          const float* e1 = encS + ta * HH + 4 * l16;
          const float* e2 = encS + tb2 * HH + 4 * l16;
          float4 dv[NC], x1[NC], x2[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            dv[c] = *reinterpret_cast<const float4*>(dS + 64 * c + 4 * l16);
            x1[c] = *reinterpret_cast<const float4*>(e1 + 64 * c);
            x2[c] = *reinterpret_cast<const float4*>(e2 + 64 * c);
          }
          float d1 = 0.f, d2 = 0.f;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            d1 += dot4(x1[c], dv[c]);
            d2 += dot4(x2[c], dv[c]);
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
          if (l16 == 0) {
            if (grp < nres) {
              const float g1 = aS[grp] * (d1 - cd);
              dsS[grp] = g1;
              a.DS[((long)s * B + b) * Tp + t0 + grp] = g1;
            }
            if (grp + 16 < nres) {
              const float g2 = aS[grp + 16] * (d2 - cd);
              dsS[grp + 16] = g2;
              a.DS[((long)s * B + b) * Tp + t0 + grp + 16] = g2;
            }
          }
          if (nx > 0) {        // streamed rows (workgroup-uniform branch)
            const int ua = nres + min(grp, nx - 1), ub = nres + min(grp + 16, nx - 1);
            const float* g1p = gEnc + (long)ua * HH + 4 * l16;
            const float* g2p = gEnc + (long)ub * HH + 4 * l16;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              x1[c] = *reinterpret_cast<const float4*>(g1p + 64 * c);
              x2[c] = *reinterpret_cast<const float4*>(g2p + 64 * c);
            }
            d1 = 0.f; d2 = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              d1 += dot4(x1[c], dv[c]);
              d2 += dot4(x2[c], dv[c]);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
            if (l16 == 0) {
              if (grp < nx) {
                const float g1 = aS[nres + grp] * (d1 - cd);
                dsS[nres + grp] = g1;
                a.DS[((long)s * B + b) * Tp + t0 + nres + grp] = g1;
              }
              if (grp + 16 < nx) {
                const float g2 = aS[nres + grp + 16] * (d2 - cd);
                dsS[nres + grp + 16] = g2;
                a.DS[((long)s * B + b) * Tp + t0 + nres + grp + 16] = g2;
              }
            }
          }
        }
        __syncthreads();
        {
          constexpr int RH = 256 / (16 * NC);
          constexpr int RPT = (32 + RH - 1) / RH;
          const int cq = tid % (16 * NC), rh = tid / (16 * NC);
          float4 ev[RPT];
          float gv[RPT];
#pragma unroll
          for (int i = 0; i < RPT; ++i) {
            const int t = rh + RH * i;
            ev[i] = *reinterpret_cast<const float4*>(encAS + min(t, nres - 1) * HH + 4 * cq);
            gv[i] = t < nres ? dsS[t] : 0.f;
          }
          float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int i = 0; i < RPT; ++i) acc4 = fma4(acc4, gv[i], ev[i]);
          if (nx > 0) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
              const int t = rh + RH * i;
              ev[i] = *reinterpret_cast<const float4*>(gEncA + (long)(nres + min(t, nx - 1)) * HH + 4 * cq);
              gv[i] = t < nx ? dsS[nres + t] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < RPT; ++i) acc4 = fma4(acc4, gv[i], ev[i]);
          }
          if (RH > 1) {
            if (rh > 0) fold[(rh - 1) * (16 * NC) + cq] = acc4;
            __syncthreads();
          }
          if (rh == 0) {
#pragma unroll
            for (int k = 1; k < RH; ++k) {
              const float4 o = fold[(k - 1) * (16 * NC) + cq];
              acc4.x += o.x; acc4.y += o.y; acc4.z += o.z; acc4.w += o.w;
            }
            __builtin_amdgcn_raw_buffer_store_b128(as_u32q(acc4), r_dha, (int)(((((long)s * B + b) * a.nsplit + att_sp) * HH + 4 * cq) * 4), 0, 16);
          }
        }
      } else {
        if (!wg_wait_sh(CTR(PB2, bt), 2 * H / 32, n + 1, a.ab, &s_flag)) return;
        tb0 = a.tick_out ? wall_clock64() : 0;
        float* dS = scr;                  // d_cv[b][:]
        float* cvS = scr + H;             // cv[b][:]
        float* dsS = scr + 2 * H;         // ds[c4] (tail 0)
        const int c4 = (a.chunk + 3) & ~3;
        float* wred = dsS + c4;           // [8]
        if (tid >= nrow && tid < c4) dsS[tid] = 0.f;
        if (tid < H / 4) {
          *reinterpret_cast<float4*>(dS + 4 * tid) = ldb128_sc1(r_dcvh, ((long)s * B + b) * 2 * H + 4 * tid);
          *reinterpret_cast<float4*>(cvS + 4 * tid) = *reinterpret_cast<const float4*>(a.CVH + ((long)s * B + b) * 2 * H + 4 * tid);
        }
        __syncthreads();
        float cdp = 0.f;                  // cv . d_cv
        for (int k = tid; k < H; k += 256) cdp += cvS[k] * dS[k];
        cdp = wave_sum(cdp);
        if (lane == 0) wred[wave] = cdp;
        __syncthreads();
        const float cd = wred[0] + wred[1] + wred[2] + wred[3];
        const float mlM = a.ML[((long)s * B + b) * 2], mlI = a.ML[((long)s * B + b) * 2 + 1];
        {
          const int grp = tid >> 4, l16 = tid & 15;
          for (int t = grp; t < nrow; t += 32) {
            const int t2 = t + 16;
            const bool two = t2 < nrow;
            const float* e1 = encS + t * H + 4 * l16;
            const float* e2 = encS + (two ? t2 : t) * H + 4 * l16;
            float d1 = 0.f, d2 = 0.f;
  #pragma unroll
            for (int c = 0; c < 16; ++c) {
              if (64 * c < H) {
                const float4 dv = *reinterpret_cast<const float4*>(dS + 64 * c + 4 * l16);
                const float4 x1 = *reinterpret_cast<const float4*>(e1 + 64 * c);
                const float4 x2 = *reinterpret_cast<const float4*>(e2 + 64 * c);
                d1 += x1.x * dv.x + x1.y * dv.y + x1.z * dv.z + x1.w * dv.w;
                d2 += x2.x * dv.x + x2.y * dv.y + x2.z * dv.z + x2.w * dv.w;
              }
            }
  #pragma unroll
            for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); }
            if (l16 == 0) {
              float* al = a.ALPHA + ((long)s * B + b) * Tp + t0;
              const float a1 = expf(al[t] - mlM) * mlI;
              al[t] = a1;                                  // normalised alpha for the deferred d_enc product
              const float g1 = a1 * (d1 - cd);
              dsS[t] = g1;
              a.DS[((long)s * B + b) * Tp + t0 + t] = g1;
              if (two) {
                const float a2 = expf(al[t2] - mlM) * mlI;
                al[t2] = a2;
                const float g2 = a2 * (d2 - cd);
                dsS[t2] = g2;
                a.DS[((long)s * B + b) * Tp + t0 + t2] = g2;
              }
            }
          }
        }
        __syncthreads();
        {
          float acc4[4] = {0.f, 0.f, 0.f, 0.f};
          const int c0 = min(tid, H - 1), c1 = min(tid + 256, H - 1), c2 = min(tid + 512, H - 1), c3 = min(tid + 768, H - 1);
          for (int t = 0; t < nrow; t += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(dsS + t);
            const float* e0 = encAS + t * H;
            const int r1 = min(t + 1, nrow - 1) - t, r2 = min(t + 2, nrow - 1) - t, r3 = min(t + 3, nrow - 1) - t;
            acc4[0] += gv.x * e0[c0] + gv.y * e0[r1 * H + c0] + gv.z * e0[r2 * H + c0] + gv.w * e0[r3 * H + c0];
            if (H > 256) acc4[1] += gv.x * e0[c1] + gv.y * e0[r1 * H + c1] + gv.z * e0[r2 * H + c1] + gv.w * e0[r3 * H + c1];
            if (H > 512) {
              acc4[2] += gv.x * e0[c2] + gv.y * e0[r1 * H + c2] + gv.z * e0[r2 * H + c2] + gv.w * e0[r3 * H + c2];
              acc4[3] += gv.x * e0[c3] + gv.y * e0[r1 * H + c3] + gv.z * e0[r2 * H + c3] + gv.w * e0[r3 * H + c3];
            }
          }
          float* out = a.DHATT + (((long)s * B + b) * a.nsplit + att_sp) * H;
  #pragma unroll
          for (int j = 0; j < 4; ++j)
            if (tid + 256 * j < H) st_sc1(&out[tid + 256 * j], acc4[j]);
        }
      }
      publish(ROWCTR(b));
      if (a.tick_out) tk_att += wall_clock64() - tb0;
      TB(5)
    }
    // ================= B5: cell backward (one per decoder layer, top first) =================
    if (has5) {
      const int bt = b5_bt, m0 = bt * 16, l = b5_l;
      const int rows_bt = min(16, B - bt * 16);
      const int row = m0 + e_row, u = b5_u0 + e_col;
      const bool ev = row < B;
      TB(15)
      float dy = 0.f;
      if (NL == 1 || l == TOP) {
        if (!wg_wait_multi(ROWCTR(m0), CTRS, rows_bt, (unsigned)(a.nsplit * (n + 1)), a.ab, &s_flag)) return;
        TB(7)
        if (ev) {
          dy = ld_sc1(a.DCVH + ((long)s * B + row) * 2 * H + H + u);
          float hs = 0.f;
          for (int k0 = 0; k0 < a.nsplit; k0 += 8) {      // 8 partial loads in flight (a plain loop waits for each one)
            float hv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
              hv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                  r_dha, (int)(((((long)s * B + row) * a.nsplit + min(k0 + j, a.nsplit - 1)) * H + u) * 4), 0, 16));
#pragma unroll
            for (int j = 0; j < 8; ++j) hs += k0 + j < a.nsplit ? hv[j] : 0.f;
          }
          dy += hs;
        }
      } else {
        if constexpr (NL > 1) {
          // gradient of this layer's dropped output: dz_{l+1,s} times this workgroup's 16 columns of Wu_{l+1}
          if (!wg_wait_sh(CTR(PB5 + l + 1, bt), H / 16, n + 1, a.ab, &s_flag)) return;
          TB(7)
          f32x4 accu = {0.f, 0.f, 0.f, 0.f};
          wmac_chunked<NB_B5, 16>(accu, wreg + OFF_B5UP, make_rsrc(a.Gt[l + 1]), ((long)s * B + min(m0 + r16, B - 1)) * K4, K4, lane, wave);
          dy = reduce16(accu, red);
        }
      }
      if (ev) {
        const float dh = v + dy * mk;
        const float tc = tanh_fast(ccur);
        const float dcv = dh * g.w * (1.f - tc * tc) + dc_state;
        const float4 dz = make_float4(dcv * g.y * (1.f - g.x * g.x), dcv * g.x * g.y * (1.f - g.y), dcv * cp * g.z * (1.f - g.z), dh * tc * g.w * (1.f - g.w));
        __builtin_amdgcn_raw_buffer_store_b128(as_u32q(dz), r_g, (int)((((long)s * B + row) * K4 + 4 * u) * 4), 0, 16);
        dc_state = dcv * g.z;
      }
      publish_sh(CTR(PB5 + l, bt), b5_u0 / 16);
      TB(8)
    }
    // ================= B6: d_x0 = dz Wu =================
    if (has6) {
      const int bt = b6_bt, m0 = bt * 16;
      TB(15)
      if (!wg_wait_sh(CTR(PB5, bt), H / 16, n + 1, a.ab, &s_flag)) return;
      TB(9)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (a.b6_split != B6_WHOLE) wmac_chunked<NB_B6 / 2, 16>(acc, wreg + OFF_B6, r_g0, ((long)s * B + min(m0 + r16, B - 1)) * K4 + b6_k0, K4 / 2, lane, wave);
      else wmac_chunked<NB_B6, 16>(acc, wreg + OFF_B6, r_g0, ((long)s * B + min(m0 + r16, B - 1)) * K4, K4, lane, wave);
      const float v = reduce16(acc, red);
      const int row = m0 + e_row;
      if (row < B) {
        if (a.b6_split != B6_WHOLE) st_sc1(a.DXH + ((long)(b6_half * S + s) * B + row) * A + (b6_n0 - E) + e_col, v);
        else st_sc1(a.DX0 + ((long)s * B + row) * XI + b6_n0 + e_col, v);
      }
      publish_sh(CTR(PB6, bt), a.b6_split != B6_WHOLE ? 2 * (b6_item % b6_per_bt) + b6_half : b6_item % b6_per_bt);
      TB(10)
    }
  }
  if (timing && tid == 0 && (wg == 0 || wg == n5 || wg == n5 + 20 || wg == 2 * n5 + 1 || wg == n5 + n6 || wg == n5 + n6 + n1 - 1 || wg == G - 1))
    printf("pdecb wg %3d per-step 10ns: B1[pre %lld wait %lld tail %lld] B2[wait %lld work %lld] B3[wait+work %lld] B5[pre %lld wait %lld tail %lld] B6[wait %lld work %lld] other %lld\n",
           wg, tb[0] / S, tb[1] / S, tb[2] / S, tb[3] / S, tb[4] / S, tb[5] / S, tb[6] / S, tb[7] / S, tb[8] / S, tb[9] / S, tb[10] / S, tb[15] / S);
#undef TB
  if (has5) {
    const int row = b5_bt * 16 + e_row, u = b5_u0 + e_col;
    if (row < B) a.d_c0[((long)b5_l * B + row) * H + u] = dc_state;
  }
  if (a.tick_out && tid == 0 && has_att) {
    atomicAdd(&a.tick_out[wg], (float)tk_att * 0.01f / (float)S);
    if (wg == 0) atomicAdd(&a.tick_out[G], 1.0f);
  }
#undef CTR
#undef ROWCTR
}

// Everything that follows the forward loop in ONE launch (a dependent launch costs ~5 us whatever it does), one block per (s, b) row:
//   * TOK[s][b] (the token that was fed) and X0[s][b][:E] = embed[TOK] * mask for the backward's wgrad / scatter,
//   * dlogits = w[t] (softmax - onehot) / B in place of the saved logits,
//   * the copy of the prediction; block 0 also sums the per-row losses (in double).
// eps > 0 (astk_decoder_desc.label_smoothing): the sweep that forms the gradient also accumulates sum_v (x_v - lse)
// -- deviations of one sign, whatever the offset of the row -- and the block replaces its loss row (the loop's P6 wrote w c (LSE - x_t)) by
// (1-eps) row + eps w c (-(1/V) sum).  Block 0 can then no longer sum rows that other blocks of this launch rewrite: every block stores its
// row, fences and arrives ONCE on `done_ctr` (a word the forward launcher's fill zeroes); the block whose arrival completes S*B sums all
// rows the way block 0 does.  No block waits for another, nothing spins, and there are no float atomics: the sum is the same whichever
// block comes last.  eps == 0 is the code this kernel always ran.
// rw (astk_decoder_fwd_w's row_weight, (B) or null): the loop kernels know no row weights (P6 writes the unweighted
// row), so the block of row (s, b) scales its gradient sweep and its loss row by rw[b].  That rewrites rows as eps > 0 does, and takes the
// same path: "rows are rewritten" is eps > 0 || rw.  rw == null is the code without it.
template <bool ATOMIC_LOADS>
__device__ __forceinline__ void post_sum_rows(const float* rows, int n, float* loss, double* red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256)
    acc += (double)(ATOMIC_LOADS ? __hip_atomic_load(rows + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : rows[i]);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (float)(red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_decoder_post(const float* __restrict__ embed, const int32_t* __restrict__ y, const int32_t* __restrict__ ytgt,
                                                      const int32_t* __restrict__ use_truth,
                                                      const int32_t* __restrict__ pred, const float* __restrict__ emb_mask, int32_t* __restrict__ tok_out,
                                                      float* __restrict__ x0, float* __restrict__ logits, const float* __restrict__ lse,
                                                      const float* __restrict__ cw, float* lossrows, float* __restrict__ loss,
                                                      int32_t* __restrict__ pred_out, int S, int B, int L, int E, int XI, int V, int Vp, float inv_count,
                                                      float eps, unsigned* done_ctr, const unsigned* __restrict__ status,
                                                      float* __restrict__ status_dst, const float* __restrict__ rw) {
  __shared__ double red[4];
  const int r = blockIdx.x, s = r / B, b = r % B;
  if (r == 0 && threadIdx.x == 0 && status_dst) *status_dst = (float)(*status);      // (astk_decoder_desc.status_dst: the snapshot without its launch)
  {
    int tok = (s == 0 || use_truth[s]) ? y[(long)b * L + s] : pred[(long)(s - 1) * B + b];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    if (threadIdx.x == 0) {
      tok_out[r] = tok;
      if (pred_out) pred_out[r] = pred[r];
    }
    for (int e = threadIdx.x; e < E; e += 256) {
      float v = embed[(long)tok * E + e];
      if (emb_mask) v *= emb_mask[(long)r * E + e];
      x0[(long)r * XI + e] = v;
    }
  }
  {
    int t = ytgt[(long)b * L + s + 1];        // the class that was SCORED (y, or forward_loss's random_out replacement)
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    const float scale = (cw ? cw[t] : 1.f) * inv_count;
    const float ls = lse[r];
    float* x = logits + (long)r * Vp;
    if (eps > 0.f || rw) {      // the rows are rewritten
      __shared__ float sdev[4];
      __shared__ int s_last;
      const float rb = rw ? rw[b] : 1.f, gs = scale * rb;
      const float uni = eps / (float)V, hot = (1.f - eps) * gs;
      float dev = 0.f;
      for (int v = threadIdx.x; v < Vp; v += 256) {
        float g = 0.f;
        if (v < V) {
          const float dv = x[v] - ls;
          dev += dv;
          g = (expf(dv) - uni) * gs;
          if (v == t) g -= hot;
        }
        x[v] = g;
      }
      for (int o = 32; o > 0; o >>= 1) dev += __shfl_xor(dev, o);
      if ((threadIdx.x & 63) == 0) sdev[threadIdx.x >> 6] = dev;
      __syncthreads();
      if (threadIdx.x == 0) {
        dev = (sdev[0] + sdev[1]) + (sdev[2] + sdev[3]);
        float row = lossrows[r];
        if (eps > 0.f) row = (1.f - eps) * row + eps * scale * (-(dev / (float)V));
        if (rw) row *= rb;
        __hip_atomic_store(lossrows + r, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // release: the row is visible to the device before the arrival; acquire: the last block sees every other block's row
        s_last = __hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u == (unsigned)(S * B);
      }
      __syncthreads();
      if (s_last && loss) post_sum_rows<true>(lossrows, S * B, loss, red);
      return;
    }
    for (int v = threadIdx.x; v < Vp; v += 256) {
      float g = 0.f;
      if (v < V) {
        g = expf(x[v] - ls) * scale;
        if (v == t) g -= scale;
      }
      x[v] = g;
    }
  }
  if (r == 0 && loss) post_sum_rows<false>(lossrows, S * B, loss, red);
}

}  // namespace

bool pdec_special(int H, int chunk) { return H == 512 && chunk <= PDEC_CHUNK_MAX; }     // the NC = 8 attention phase
static int pdec_res_rows(int H, int chunk) { return pdec_special(H, chunk) && chunk > PDEC_RES_ROWS ? PDEC_RES_ROWS : chunk; }
static size_t pdec_lds_floats(int chunk, int H, int nsplit) {
  size_t scratch = (size_t)H + 2 * (size_t)((chunk + 3) & ~3) + 16;
  if (pdec_special(H, chunk) && scratch < (size_t)H + 128 + 512) scratch = (size_t)H + 128 + 512;
  if (scratch < (size_t)nsplit * (H + 4)) scratch = (size_t)nsplit * (H + 4);
  return 2 * (size_t)pdec_res_rows(H, chunk) * H + (size_t)((chunk + 3) & ~3) + scratch;
}
static size_t pdec_bwd_lds_floats(int chunk, int H) {
  return 2 * (size_t)pdec_res_rows(H, chunk) * H + 2 * (size_t)H + (size_t)((chunk + 3) & ~3) + 16 + 160 + 512;
}

// max_L: the training kernel keeps a batch tile's targets and the teacher-forcing flags in LDS (yS / flagS: L <= 192); greedy mode
// reads neither and passes its own cap (d->L = stop_limit + 1)
static bool pdec_applicable(const astk_decoder_desc* d, int max_L, int* nsplit_out, int* chunk_out) {
  if (!tune_on(TUNE_DEC_PERSIST)) return false;
  if (d->n_attn > 1 || d->no_feed_attn || d->ln) return false;      // optional model features: per-launch loop (decoder.hip)
  if (d->n_layers < 1 || d->n_layers > PDEC_MAX_LAYERS) return false;
  if (device_cu_count() < G) return false;        // fixed roles over G workgroups, all of them resident (one per CU)
  if ((d->H % 64) || (d->A % 16) || (d->E % 16) || d->A < 16 || d->E < 16) return false;
  const int nbt = (d->B + 15) / 16, ntv = (d->V + 15) / 16;
  if (d->E > 64 * NB_E || d->A > 64 * NB_A || d->H > 64 * NB_H || 2 * d->H > 64 * NB_C || d->A > 64 * NB_L || d->H > 1024) return false;
  const int n_cell = nbt * (d->H / 8);
  const int rest = G - n_cell;
  if (n_cell >= G || rest < nbt * (d->A / 16) || 2 * rest < nbt * ntv) return false;
  if (rest < d->B + nbt || d->B > G) return false;
  if (d->n_layers > 1 && 2 * n_cell > G) return false;       // the top layer's cell items live on the upper workgroups
  int nsplit = G / d->B;
  if (nsplit > 64) nsplit = 64;
  if (nsplit > d->T) nsplit = d->T;
  if (nsplit < 1) return false;
  int chunk = (d->T + nsplit - 1) / nsplit;
  nsplit = (d->T + chunk - 1) / chunk;
  if (chunk > 256 || d->L > max_L) return false;
  {   // backward roles and register budgets
    const int XI = d->E + d->A, Vp = (d->V + 3) / 4 * 4;
    if (Vp > 64 * NB_B1 || d->A > 64 * NB_B2 || 4 * d->H > 64 * NB_B5 || (XI % 16) || ((2 * d->H) % 32)) return false;
    // (the one-layer layout with whole d_x0 items is asked of every layer count, as it has been since the multi-layer layout came)
    if (!pdec_bwd_roles(nbt, d->H, d->A, XI, 1, B6_WHOLE).fits) return false;
    if (pdec_bwd_lds_floats(chunk, d->H) * sizeof(float) > 148 * 1024) return false;
    if (d->n_layers > 1 && (((4 * d->H) % 128) || !pdec_bwd_roles(nbt, d->H, d->A, XI, d->n_layers, B6_SPLIT).fits)) return false;
  }                       // pass-1 bookkeeping uses one thread per row
  if (pdec_lds_floats(chunk, d->H, nsplit) * sizeof(float) > 136 * 1024) return false;
  *nsplit_out = nsplit;
  *chunk_out = chunk;
  return true;
}
bool decoder_persist_applicable(const astk_decoder_desc* d, int* nsplit_out, int* chunk_out) { return pdec_applicable(d, 192, nsplit_out, chunk_out); }

// d_x0 phase of the backward kernel as 2 K-halves per item over the ht columns only: fits when the roles still fit 256 workgroups
bool decoder_persist_b6_split(const astk_decoder_desc* d) {
  if ((4 * d->H) % 128) return false;
  if (d->n_layers > 1) return true;           // the multi-layer role layout always uses the split form (decoder_persist_applicable checked it)
  if (!tune_on(TUNE_DEC_B6_SPLIT)) return false;
  return pdec_bwd_roles((d->B + 15) / 16, d->H, d->A, d->E + d->A, 1, B6_SPLIT).fits;
}

// The one launcher of the persistent decoder kernels.  pick(nc, nl, xs) names the instantiation <NC, NL, XS> of one kernel template (its
// arguments are std::integral_constant values); the shape selects among the three of a layer count: generic, NC = 8, NC = 8 streamed.
// Every `pick` is a type of its own, so each (kernel template, NL) has its own `attr_done`: a kernel's LDS cap is raised once per process.
template <int NL, class Pick, class Args>
static void pdec_launch_nl(Pick pick, int lds_cap, int H, int chunk, size_t shm, hipStream_t s, const Args& a) {
  using Layers = std::integral_constant<int, NL>;
  const auto k0 = pick(std::integral_constant<int, 0>{}, Layers{}, std::false_type{});
  const auto k8 = pick(std::integral_constant<int, 8>{}, Layers{}, std::false_type{});
  const auto k8x = pick(std::integral_constant<int, 8>{}, Layers{}, std::true_type{});
  static bool attr_done = false;
  if (!attr_done) {
    for (auto k : {k0, k8, k8x}) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
    attr_done = true;
  }
  const bool special = pdec_special(H, chunk);
  const auto k = !special ? k0 : (chunk > PDEC_RES_ROWS ? k8x : k8);
  hipLaunchKernelGGL(k, dim3(G), dim3(256), shm, s, a);
}
template <class Pick, class Args>
static void pdec_launch(Pick pick, int n_layers, int lds_cap, int H, int chunk, size_t shm, hipStream_t s, const Args& a) {
  if (n_layers == 1) pdec_launch_nl<1>(pick, lds_cap, H, chunk, shm, s, a);
  else if (n_layers == 2) pdec_launch_nl<2>(pick, lds_cap, H, chunk, shm, s, a);
  else pdec_launch_nl<3>(pick, lds_cap, H, chunk, shm, s, a);
}

// The fourteen shape fields that PDecArgs and PDecBwdArgs share, for a loop of S steps
template <class Args>
static void pdec_fill_shapes(Args& a, const astk_decoder_desc* d, int S, int nsplit, int chunk) {
  a.B = d->B; a.S = S; a.L = S + 1; a.T = d->T; a.Tp = (d->T + 3) / 4 * 4; a.H = d->H; a.E = d->E; a.A = d->A; a.V = d->V;
  a.Vp = (d->V + 3) / 4 * 4; a.XI = d->E + d->A; a.nbt = (d->B + 15) / 16; a.nsplit = nsplit; a.chunk = chunk;
}

int decoder_persist_bwd_launch(const astk_decoder_desc* d, const float* enc, const float* rnn_masks, const DecPersistBwdBuffers& bf,
                               hipStream_t s) {
  int nsplit = 1, chunk = 1;
  ASTK_CHECK(decoder_persist_applicable(d, &nsplit, &chunk), "decoder_persist_bwd: not applicable");
  PDecBwdArgs a;
  memset(&a, 0, sizeof(a));
  pdec_fill_shapes(a, d, d->L - 1, nsplit, chunk);
  a.NL = d->n_layers;
  a.WoT = bf.WoT; a.WcT = bf.WcT; a.enc = enc; a.encA = bf.ENCA; a.ALPHA = bf.ALPHA; a.CVH = bf.CVH; a.ML = bf.ML;
  for (int l = 0; l < d->n_layers; ++l) {
    a.WlT[l] = bf.WlT[l]; a.WuT[l] = bf.WuT[l]; a.Cst[l] = bf.C[l]; a.Gt[l] = bf.G[l];
    a.rnn_mask[l] = rnn_masks ? rnn_masks + (size_t)l * (d->L - 1) * d->B * d->H : nullptr;
  }
  a.HT = bf.HT; a.LOGITS = bf.LOGITS; a.DPRE = bf.DPRE; a.DCVH = bf.DCVH; a.DS = bf.DS;
  a.DX0 = bf.DX0; a.DHATT = bf.DHATT; a.d_c0 = bf.d_c0;
  a.DXH = bf.DXH;
  a.b6_split = bf.DXH != nullptr && decoder_persist_b6_split(d) ? B6_SPLIT : B6_WHOLE;
  // (astk_set_tuning("dec.b6_fused", 0): the d_x0 role of rounds 2-3, kept for A/B runs)
  if (a.b6_split == B6_SPLIT && tune_on(TUNE_DEC_B6_FUSED) && pdec_bwd_roles(a.nbt, a.H, a.A, a.XI, d->n_layers, B6_FUSED).fits) a.b6_split = B6_FUSED;
  ASTK_CHECK(d->n_layers == 1 || a.b6_split != B6_WHOLE, "decoder_persist_bwd: the multi-layer role layout needs the split d_x0 buffers");
  a.ctr = bf.ctr;
  a.ab = abort_ctl(bf.ctr + (size_t)NPHASE_SLOTS * NSH * a.nbt * CTRS, PERSIST_DEC_BWD);
  a.tick_out = prof_tick_buffer(1);
  a.dbg = persist_dbg_env();
  {      // (a fill kernel, not hipMemsetAsync: the runtime's fill path left a 6 us gap in front of the launch)
    FillSegs f;
    f.n = 0;
    fill_seg_add(f, bf.ctr, ((size_t)NPHASE_SLOTS * NSH * a.nbt + 2 + a.B) * CTRS * sizeof(unsigned));
    if (bf.zero_ptr && bf.zero_bytes) fill_seg_add(f, bf.zero_ptr, bf.zero_bytes);      // (the caller's gradient arena: astk_decoder_desc.zero_ptr)
    if (bf.zero2_ptr && bf.zero2_bytes) fill_seg_add(f, bf.zero2_ptr, bf.zero2_bytes);   // (d_enc: decoder.hip adds both of its products into it)
    ASTK_TRY(fill_u32_segments(f, 0u, s));
  }
  const size_t shm = pdec_bwd_lds_floats(chunk, a.H) * sizeof(float);       // slices + dS/cvS/ds + ds/alpha/fold of the specialised scan
  {
    ProfScope prof(PROF_DEC_BWD, s);
    pdec_launch([](auto nc, auto nl, auto xs) { return decoder_persist_bwd<nc, nl, xs>; }, d->n_layers, 150 * 1024, a.H, chunk, shm, s, a);
  }
  ASTK_LAUNCH_CHECK();
  return 0;
}

int decoder_persist_fwd_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const int32_t* y,
                               const int32_t* ytgt, const int32_t* use_truth, const float* emb_mask, const float* rnn_masks, const DecPersistBuffers& bf,
                               float* loss, int32_t* pred_out, hipStream_t s, const float* row_weight) {
  int nsplit = 1, chunk = 1;
  // encA = enc . Wa (one batched GEMM): the score of decoder step s is encA[b,t,:].h_s + enc[b,t,:].ba, so the per-step
  // q = Wa h phase drops out of the sequential chain; Q itself is rebuilt after the loop for the backward.
  ASTK_TRY(gemm_launch(GEMM_NN, gemm_args(d->B * d->T, d->H, d->H, mat(enc, d->H), mat(prm->Wa, d->H), bf.ENCA, d->H), s));
  ASTK_CHECK(decoder_persist_applicable(d, &nsplit, &chunk), "decoder_persist: not applicable");
  PDecArgs a;
  memset(&a, 0, sizeof(a));
  pdec_fill_shapes(a, d, d->L - 1, nsplit, chunk);
  a.ntile_v = (d->V + 15) / 16;
  a.inv_count = 1.f / (float)(d->loss_rows > 0 ? d->loss_rows : d->B);
  a.embed = prm->embed;
  for (int l = 0; l < d->n_layers; ++l) {
    a.Wu[l] = prm->lstm[l].Wu; a.bias[l] = prm->lstm[l].b; a.Wl[l] = prm->lstm[l].Wl;
    a.Gt[l] = bf.G[l]; a.Cst[l] = bf.C[l]; a.HR[l] = bf.HR[l]; a.HD[l] = bf.HD[l];
    a.rnn_mask[l] = rnn_masks ? rnn_masks + (size_t)l * (d->L - 1) * d->B * d->H : nullptr;
  }
  a.Wa = prm->Wa; a.ba = prm->ba; a.Wc = prm->Wc; a.bc = prm->bc; a.Wo = prm->Wo; a.bo = prm->bo; a.cw = prm->class_weight;
  a.enc = enc; a.encA = bf.ENCA; a.y = y; a.ytgt = ytgt ? ytgt : y; a.use_truth = use_truth; a.emb_mask = emb_mask;
  a.TOK = bf.TOK; a.PRED = bf.PRED; a.X0 = bf.X0; a.Q = bf.Q; a.ALPHA = bf.ALPHA;
  a.CVH = bf.CVH; a.HT = bf.HT; a.LOGITS = bf.LOGITS; a.LOSSROWS = bf.LOSSROWS; a.LSE = bf.LSE; a.PART = bf.PART; a.CESTAT = bf.CESTAT; a.ML = bf.ML;
  a.ctr = bf.ctr;
  a.ab = abort_ctl(bf.ctr + (size_t)NPHASE_SLOTS * NSH * a.nbt * CTRS, PERSIST_DEC_FWD);
  a.dbg = persist_dbg_env();
  a.tick_out = prof_tick_buffer(0);
  // (one fill launch, not hipMemsetAsync calls: the counters zeroed, the h half of CVH sentinel-filled, the initial states copied)
  {
    FillSegs f;
    f.n = 0;
    // (... and one more line behind the per-row counters: k_decoder_post's arrival counter, `post_ctr` below)
    fill_seg_add(f, bf.ctr, ((size_t)NPHASE_SLOTS * NSH * a.nbt + 2 + a.B + 1) * CTRS * sizeof(unsigned), 0u);
    fill_seg_add(f, bf.CVH, (size_t)a.S * a.B * 2 * a.H * sizeof(float));
    if (bf.zero_a) fill_seg_add(f, bf.zero_a, bf.zero_a_bytes, 0u);
    if (bf.zero_b) fill_seg_add(f, bf.zero_b, bf.zero_b_bytes, 0u);
    if (bf.c0 && bf.h0) {
      const size_t bh = (size_t)d->B * d->H;
      ASTK_CHECK(f.n + 2 * d->n_layers <= FILL_SEG_MAX, "decoder_persist: too many fill segments");
      for (int l = 0; l < d->n_layers; ++l) {
        fill_seg_add_copy(f, bf.C[l], bf.c0 + l * bh, bh * sizeof(float));
        fill_seg_add_copy(f, bf.HR[l], bf.h0 + l * bh, bh * sizeof(float));
      }
    }
    ASTK_TRY(fill_u32_segments(f, PDEC_SENTINEL, s));
  }
  const size_t shm = pdec_lds_floats(chunk, a.H, nsplit) * sizeof(float);
  {
    ProfScope prof(PROF_DEC_FWD, s);
    pdec_launch([](auto nc, auto nl, auto xs) { return decoder_persist_fwd<nc, nl, xs, false>; }, d->n_layers, 138 * 1024, a.H, chunk, shm, s, a);
  }
  ASTK_LAUNCH_CHECK();
  // Q[s][b][:] = Wa h_top + ba for all steps (needed by the backward's deferred d_enc product)
  ASTK_TRY(gemm_launch(GEMM_NT, gemm_args(a.S * a.B, a.H, a.H, mat(bf.CVH + a.H, 2 * a.H), mat(prm->Wa, a.H), bf.Q, a.H, prm->ba), s));
  unsigned* post_ctr = bf.ctr + ((size_t)NPHASE_SLOTS * NSH * a.nbt + 2 + a.B) * CTRS;
  hipLaunchKernelGGL(k_decoder_post, dim3(a.S * a.B), dim3(256), 0, s, prm->embed, y, ytgt ? ytgt : y, use_truth, bf.PRED, emb_mask, bf.TOK, bf.X0, bf.LOGITS, bf.LSE,
                     prm->class_weight, bf.LOSSROWS, loss, pred_out, a.S, a.B, a.L, a.E, a.XI, a.V, a.Vp, a.inv_count, d->label_smoothing, post_ctr,
                     persist_status_word(), d->status_dst, row_weight);
  ASTK_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------- greedy decoding
// decoder_persist_fwd<.., GR = true> on a workspace of its own: the step-indexed hand-off buffers of the training loop, sized by the stop
// limit, without the ones greedy mode never touches (X0, Q, G, C, ALPHA, ML, LOGITS, LSE, loss rows).
struct GreedyPlan {
  float *ENCA, *CVH, *HT, *PART, *CESTAT;
  float *HR[PDEC_MAX_LAYERS], *HD[PDEC_MAX_LAYERS];
  unsigned* ctr;           // phase counters, abort word, per-row counters, then the 4 lines of PDecArgs::gctl
  int nsplit, chunk;
  size_t bytes;
};
static size_t greedy_ctr_lines(int B) { return (size_t)NPHASE_SLOTS * NSH * ((B + 15) / 16) + 2 + B + 4; }

static bool greedy_plan(const astk_decoder_desc* d0, int stop_limit, void* ws, GreedyPlan& g) {
  if (!d0 || d0->struct_size != sizeof(astk_decoder_desc)) return false;
  static_assert((PDEC_SM_ROWS & (PDEC_SM_ROWS - 1)) == 0 && PDEC_SM_ROWS <= 256, "sampled mode: the row mask and the one-thread-per-key load");
  if (stop_limit < 1 || stop_limit > ASTK_GREEDY_MAX_STEPS || d0->B < 1 || d0->B > PDEC_SM_ROWS || d0->T < 1 || d0->V < 2) return false;
  astk_decoder_desc d = *d0;
  d.L = stop_limit + 1;
  if (!pdec_applicable(&d, ASTK_GREEDY_MAX_STEPS + 1, &g.nsplit, &g.chunk)) return false;
  const size_t S = stop_limit, B = d.B, H = d.H;
  Carver c(ws);
  g.ENCA = c.take<float>(B * d.T * H);
  g.CVH = c.take<float>(S * B * 2 * H);
  g.HT = c.take<float>((S + 1) * B * d.A);
  for (int l = 0; l < PDEC_MAX_LAYERS; ++l) {
    g.HR[l] = l < d.n_layers ? c.take<float>((S + 1) * B * H) : nullptr;
    g.HD[l] = l + 1 < d.n_layers ? c.take<float>(S * B * H) : nullptr;
  }
  g.PART = c.take<float>(S * B * g.nsplit * (H + 4));
  g.CESTAT = c.take<float>(S * B * (size_t)((d.V + 15) / 16) * 4);
  g.ctr = c.take<unsigned>(greedy_ctr_lines(d.B) * CTRS);
  g.bytes = c.total();
  return true;
}

size_t greedy_workspace_bytes(const astk_decoder_desc* d, int stop_limit) {
  GreedyPlan g;
  return greedy_plan(d, stop_limit, nullptr, g) ? g.bytes : 0;
}

// (the scored mode needs no workspace of its own: LOGP and NLL are the caller's)
size_t greedy_scored_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return greedy_workspace_bytes(d, stop_limit); }

// What the launchers of the inference modes (greedy, scored greedy, forced) share.  inference_args: the PDecArgs of a loop of S steps on
// a greedy plan -- shapes, parameters, hand-off buffers, counters, abort control, the control lines; a mode's own fields (tokens, targets,
// outputs) are its launcher's.  inference_run: everything enqueued for such a loop -- encA = enc . Wa, the one fill launch in front of the
// loop (counters, abort word, tile reports and exit count to 0, the stop word to S, the sentinel hand-offs, h0), the mode's kernel.
static PDecArgs inference_args(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, int S,
                               const GreedyPlan& g) {
  PDecArgs a;
  memset(&a, 0, sizeof(a));
  pdec_fill_shapes(a, d, S, g.nsplit, g.chunk);
  a.ntile_v = (d->V + 15) / 16;
  a.inv_count = 1.f / (float)d->B;
  a.embed = prm->embed;
  const size_t bh = (size_t)d->B * d->H;
  for (int l = 0; l < d->n_layers; ++l) {
    a.Wu[l] = prm->lstm[l].Wu; a.bias[l] = prm->lstm[l].b; a.Wl[l] = prm->lstm[l].Wl;
    a.Cst[l] = const_cast<float*>(c0 + l * bh);       // (read once: the cells keep c in a register and save no states)
    a.HR[l] = g.HR[l]; a.HD[l] = g.HD[l];
  }
  a.Wa = prm->Wa; a.ba = prm->ba; a.Wc = prm->Wc; a.bc = prm->bc; a.Wo = prm->Wo; a.bo = prm->bo;
  a.enc = enc; a.encA = g.ENCA;
  a.CVH = g.CVH; a.HT = g.HT; a.PART = g.PART; a.CESTAT = g.CESTAT;
  a.ctr = g.ctr;
  a.ab = abort_ctl(g.ctr + (size_t)NPHASE_SLOTS * NSH * a.nbt * CTRS, PERSIST_DEC_FWD);
  a.dbg = persist_dbg_env();
  a.gctl = g.ctr + (greedy_ctr_lines(d->B) - 4) * CTRS;
  return a;
}

static int inference_run(PDecMode mode, const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* h0,
                         const PDecArgs& a, const GreedyPlan& g, hipStream_t s) {
  PrecScope prec_scope(d->precision, d->gemm_operands);
  GemmForwardScope forward_scope;
  ASTK_TRY(gemm_launch(GEMM_NN, gemm_args(d->B * d->T, d->H, d->H, mat(enc, d->H), mat(prm->Wa, d->H), g.ENCA, d->H), s));   // encA = enc . Wa
  const size_t bh = (size_t)d->B * d->H;
  FillSegs f;
  f.n = 0;
  fill_seg_add(f, g.ctr, (greedy_ctr_lines(d->B) - 1) * CTRS * sizeof(unsigned), 0u);
  fill_seg_add(f, a.gctl + 3 * CTRS, CTRS * sizeof(unsigned), (unsigned)a.S);
  fill_seg_add(f, g.CVH, (size_t)a.S * a.B * 2 * a.H * sizeof(float));
  for (int l = 0; l < d->n_layers; ++l) fill_seg_add_copy(f, g.HR[l], h0 + l * bh, bh * sizeof(float));
  ASTK_TRY(fill_u32_segments(f, PDEC_SENTINEL, s));
  const size_t shm = pdec_lds_floats(g.chunk, a.H, g.nsplit) * sizeof(float);
  const auto launch = [&](auto pick) { pdec_launch(pick, d->n_layers, 138 * 1024, a.H, g.chunk, shm, s, a); };
  if (mode == PDEC_FORCED) launch([](auto nc, auto nl, auto xs) { return decoder_persist_forced<nc, nl, xs>; });
  else if (mode == PDEC_SAMPLED) launch([](auto nc, auto nl, auto xs) { return decoder_persist_sampled<nc, nl, xs>; });
  else if (mode == PDEC_SCORED) launch([](auto nc, auto nl, auto xs) { return decoder_persist_greedy_scored<nc, nl, xs>; });
  else if (mode == PDEC_BEAM) launch([](auto nc, auto nl, auto xs) { return decoder_persist_beam<nc, nl, xs>; });
  else if (mode == PDEC_TOPK) launch([](auto nc, auto nl, auto xs) { return decoder_persist_sampled_topk<nc, nl, xs>; });
  else launch([](auto nc, auto nl, auto xs) { return decoder_persist_fwd<nc, nl, xs, true>; });
  ASTK_LAUNCH_CHECK();
  return 0;
}

// the scored mode's arguments
struct GreedyScoredIO {
  const int32_t* y; int ldy;       // targets [B][ldy] or null
  const float* class_weight;       // [V] or null = all 1
  float *logp, *nll;               // [stop_limit][B]; nll null iff y is null
  const uint64_t* row_keys;        // sampled mode: [B] row keys (null: the scored greedy mode) and 1 / temperature
  float inv_temp;
  int top_k;                       // truncated sampled mode (0: untruncated): the candidates, the nucleus mass, the kept counts [stop_limit][B]
  float top_p;                     // or null -- and the workspace then holds the step's tempered logits behind the greedy plan
  int32_t* n_kept;
};
// truncated sampled mode: the bytes of the xs buffer [stop_limit][B][Vp] behind the greedy plan
static size_t topk_xs_bytes(const astk_decoder_desc* d, int stop_limit) {
  Carver c(nullptr);
  c.take<float>((size_t)stop_limit * d->B * (size_t)((d->V + 3) / 4 * 4));
  return c.total();
}
// sc: null for the unscored kernel
static int greedy_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0, int go,
                         int eos, int stop_limit, const GreedyScoredIO* sc, int32_t* tokens, int32_t* n_steps, float* status_dst, void* ws,
                         size_t ws_bytes, const int32_t* row_len, hipStream_t s) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(d->V > 1 && go >= 0 && go < d->V && eos >= 0 && eos < d->V, "greedy_decode: go %d / eos %d outside [0, V = %d)", go, eos, d->V);
  ASTK_CHECK(stop_limit >= 1 && stop_limit <= ASTK_GREEDY_MAX_STEPS, "greedy_decode: stop_limit %d outside [1, %d]", stop_limit, ASTK_GREEDY_MAX_STEPS);
  GreedyPlan g;
  ASTK_CHECK(greedy_plan(d, stop_limit, nullptr, g), "greedy_decode: B = %d, H = %d, %d layers (or the knob dec.persist = 0) does not run on the "
             "device loop: astk_greedy_workspace_bytes returns 0, decode with astk_decoder_step_infer", d->B, d->H, d->n_layers);
  const bool topk = sc && sc->top_k != 0;
  const size_t need = g.bytes + (topk ? topk_xs_bytes(d, stop_limit) : 0);
  ASTK_CHECK(ws && ws_bytes >= need, "greedy_decode: workspace too small (%zu < %zu)", ws_bytes, need);
  ASTK_CHECK(prm && enc && c0 && h0 && tokens && n_steps, "greedy_decode: null pointer");
  if (sc) {
    ASTK_CHECK(sc->logp, "greedy_decode_scored: null pointer (logp)");
    ASTK_CHECK((sc->y != nullptr) == (sc->nll != nullptr), "greedy_decode_scored: nll goes with y (%s given without %s)",
               sc->y ? "y" : "nll", sc->y ? "nll" : "y");
    ASTK_CHECK(!sc->y || sc->ldy >= 1, "greedy_decode_scored: ldy %d < 1", sc->ldy);
  }
  greedy_plan(d, stop_limit, ws, g);
  PDecArgs a = inference_args(d, prm, enc, c0, stop_limit, g);
  a.PRED = tokens;
  a.go = go; a.eos = eos;
  a.n_steps_out = n_steps; a.status_dst = status_dst;
  a.row_len = row_len;
  if (sc) {
    a.LSE = sc->logp; a.LOSSROWS = sc->nll; a.ytgt = sc->y; a.L = sc->y ? sc->ldy : 1; a.cw = sc->class_weight;
    a.row_keys = sc->row_keys; a.inv_temp = sc->inv_temp;
    if (topk) { a.top_k = sc->top_k; a.top_p = sc->top_p; a.NKEPT = sc->n_kept; a.LOGITS = (float*)((char*)ws + g.bytes); }
  }
  return inference_run(!sc ? PDEC_GREEDY : (topk ? PDEC_TOPK : (sc->row_keys ? PDEC_SAMPLED : PDEC_SCORED)), d, prm, enc, h0, a, g, s);
}

int greedy_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0, int go,
                         int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                         const int32_t* row_len, hipStream_t s) {
  return greedy_launch(d, prm, enc, c0, h0, go, eos, stop_limit, nullptr, tokens, n_steps, status_dst, ws, ws_bytes, row_len, s);
}

int greedy_decode_scored_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                                int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight, int32_t* tokens,
                                float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                                const int32_t* row_len, hipStream_t s) {
  const GreedyScoredIO sc{y, ldy, class_weight, logp, nll, nullptr, 1.f, 0, 1.f, nullptr};
  return greedy_launch(d, prm, enc, c0, h0, go, eos, stop_limit, &sc, tokens, n_steps, status_dst, ws, ws_bytes, row_len, s);
}

// ---------------------------------------------------------------------------------------------------- sampled decoding
// decoder_persist_sampled on the greedy plan as it is: the tile record keeps its four words (z, se relative to xs at the winner, index, xs
// at the winner), so the workspace is the greedy modes'.
size_t sample_workspace_bytes(const astk_decoder_desc* d, int stop_limit) { return greedy_workspace_bytes(d, stop_limit); }

int sample_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0, int go,
                         int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp, int32_t* n_steps,
                         float* status_dst, void* ws, size_t ws_bytes, const int32_t* row_len, hipStream_t s) {
  ASTK_CHECK(row_keys, "sample_decode: null pointer (row_keys)");
  ASTK_CHECK(logp, "sample_decode: null pointer (logp)");
  ASTK_CHECK(inv_temp > 0.f && inv_temp <= 3.402823466e38f, "sample_decode: inv_temp %g is not a finite number above 0", (double)inv_temp);
  const GreedyScoredIO sc{nullptr, 0, nullptr, logp, nullptr, row_keys, inv_temp, 0, 1.f, nullptr};
  return greedy_launch(d, prm, enc, c0, h0, go, eos, stop_limit, &sc, tokens, n_steps, status_dst, ws, ws_bytes, row_len, s);
}

// ---------------------------------------------------------------------------------------------------- truncated sampling
// decoder_persist_sampled_topk through greedy_launch, as the sampled mode: the greedy plan, plus the step's tempered logits [S][B][Vp] that P5
// keeps for P6's top_k sweeps (topk_xs_bytes, behind the plan).  Every check of the sampled mode is greedy_launch's and
// sample_decode_launch's own; this entry adds top_k and top_p.  (The plan's tile-record buffer CESTAT is carried and not used in this mode.)
size_t sample_topk_workspace_bytes(const astk_decoder_desc* d, int stop_limit) {
  const size_t g = greedy_workspace_bytes(d, stop_limit);
  return g ? g + topk_xs_bytes(d, stop_limit) : 0;
}

int sample_decode_topk_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                              int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int top_k, float top_p,
                              int32_t* tokens, float* logp, int32_t* n_kept, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                              const int32_t* row_len, hipStream_t s) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(top_k >= 1 && top_k <= ASTK_SAMPLE_MAX_TOPK && top_k <= d->V, "sample_decode_topk: top_k %d outside [1, %d] or above V = %d", top_k,
             ASTK_SAMPLE_MAX_TOPK, d->V);
  ASTK_CHECK(top_p > 0.f && top_p <= 1.f, "sample_decode_topk: top_p %g is not a number in (0, 1]", (double)top_p);
  ASTK_CHECK(row_keys, "sample_decode: null pointer (row_keys)");
  ASTK_CHECK(logp, "sample_decode: null pointer (logp)");
  ASTK_CHECK(inv_temp > 0.f && inv_temp <= 3.402823466e38f, "sample_decode: inv_temp %g is not a finite number above 0", (double)inv_temp);
  const GreedyScoredIO sc{nullptr, 0, nullptr, logp, nullptr, row_keys, inv_temp, top_k, top_p, n_kept};
  return greedy_launch(d, prm, enc, c0, h0, go, eos, stop_limit, &sc, tokens, n_steps, status_dst, ws, ws_bytes, row_len, s);
}

int gumbel_rows_launch(const uint64_t* row_keys, int B, int step, int V, float* out, hipStream_t s) {
  ASTK_CHECK(row_keys && out, "gumbel_rows: null pointer");
  ASTK_CHECK(B >= 1 && B <= 65535 && V >= 1 && step >= 0, "gumbel_rows: B %d outside [1, 65535], V %d < 1 or step %d < 0", B, V, step);
  hipLaunchKernelGGL(k_gumbel_rows, dim3((V + 255) / 256, B), dim3(256), 0, s, row_keys, step, V, out);
  ASTK_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------- forced decoding
// decoder_persist_forced on the greedy plan sized by S = ldy - 1, plus -- with an alpha output -- the raw scores [S][B][Tp] and the
// (max, 1 / sum) pairs [S][B][2] that k_alpha_normalise reads behind the loop.
struct ForcedPlan {
  GreedyPlan g;
  float *RAW, *ML;
  size_t bytes;
};
static bool forced_plan(const astk_decoder_desc* d, int n_steps, int with_alpha, void* ws, ForcedPlan& f) {
  if (!greedy_plan(d, n_steps, ws, f.g)) return false;
  f.RAW = f.ML = nullptr;
  f.bytes = f.g.bytes;
  if (with_alpha) {
    Carver c(ws ? (char*)ws + f.g.bytes : nullptr);
    const size_t S = n_steps, B = d->B, Tp = (d->T + 3) / 4 * 4;
    f.RAW = c.take<float>(S * B * Tp);
    f.ML = c.take<float>(S * B * 2);
    f.bytes += c.total();
  }
  return true;
}

size_t forced_workspace_bytes(const astk_decoder_desc* d, int n_steps, int with_alpha) {
  ForcedPlan f;
  return forced_plan(d, n_steps, with_alpha, nullptr, f) ? f.bytes : 0;
}

int forced_score_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                        const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst, void* ws,
                        size_t ws_bytes, const int32_t* row_len, hipStream_t s) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(ldy >= 2 && ldy - 1 <= ASTK_GREEDY_MAX_STEPS, "forced_score: ldy %d outside [2, %d]", ldy, ASTK_GREEDY_MAX_STEPS + 1);
  const int S = ldy - 1;
  ForcedPlan f;
  ASTK_CHECK(forced_plan(d, S, alpha != nullptr, nullptr, f), "forced_score: B = %d, H = %d, %d layers (or the knob dec.persist = 0) does not run "
             "on the device loop: astk_forced_workspace_bytes returns 0, score with astk_decoder_step_infer", d->B, d->H, d->n_layers);
  ASTK_CHECK(ws && ws_bytes >= f.bytes, "forced_score: workspace too small (%zu < %zu)", ws_bytes, f.bytes);
  ASTK_CHECK(prm && enc && c0 && h0 && y && logp, "forced_score: null pointer");
  forced_plan(d, S, alpha != nullptr, ws, f);
  PDecArgs a = inference_args(d, prm, enc, c0, S, f.g);
  a.y = y; a.ytgt = y;                  // (a.L = S + 1 = ldy)
  a.LSE = logp; a.LOSSROWS = logp_max; a.PRED = pred; a.ALPHA = f.RAW; a.ML = f.ML;
  a.status_dst = status_dst;            // (of the control lines only the exit count, line 2, is used: the stop word is never read)
  a.row_len = row_len;
  ASTK_TRY(inference_run(PDEC_FORCED, d, prm, enc, h0, a, f.g, s));
  if (alpha) {
    hipLaunchKernelGGL(k_alpha_normalise, dim3(a.S * a.B), dim3(256), 0, s, f.RAW, f.ML, alpha, row_len, a.B, a.T, a.Tp);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------- beam search
// decoder_persist_beam on the greedy plan, plus the step's logits [S][B][Vp], the fed tokens and parent rows [S][B], the slots' origins
// [B], c of every step and layer [S + 1][B][H], and -- with an alpha output -- the forced mode's raw scores and (max, 1 / sum) pairs.
struct BeamPlan {
  GreedyPlan g;
  float *LOGITS, *CS[PDEC_MAX_LAYERS], *RAW, *ML;
  int32_t *FEED, *PAR, *ORG;
  size_t bytes;
};
// the row layout of include/astk.h: N slots of an utterance inside one 16-row tile, B ending with an utterance's last slot
static bool beam_layout_ok(int B, int N, int K, int V) {
  if (N < 1 || N > ASTK_BEAM_MAX_N || K < 1 || K > ASTK_BEAM_MAX_K || K > V || B < 1) return false;
  const int last = (B - 1) % 16 + 1;                 // rows of the last tile
  return last <= (16 / N) * N && last % N == 0;
}
static bool beam_plan(const astk_decoder_desc* d, int N, int K, int stop_limit, int with_alpha, void* ws, BeamPlan& p) {
  if (!greedy_plan(d, stop_limit, ws, p.g)) return false;
  if (!beam_layout_ok(d->B, N, K, d->V)) return false;
  // The attention split of this mode does not depend on the launch's row count or T: PDEC_BEAM_NSPLIT slices per row (the split of a
  // 32-row launch), each row cut by its own length in the kernel; chunk = the longest slice any row can have.  One scan kernel per H:
  // H = 512 always takes the specialised scan (T <= 480), so a row never meets the generic one in one launch and the other in the next.
  p.g.nsplit = d->T < PDEC_BEAM_NSPLIT ? d->T : PDEC_BEAM_NSPLIT;
  p.g.chunk = (d->T + PDEC_BEAM_NSPLIT - 1) / PDEC_BEAM_NSPLIT;
  if (p.g.chunk > 256 || (d->H == 512 && !pdec_special(d->H, p.g.chunk))) return false;
  if (pdec_lds_floats(p.g.chunk, d->H, p.g.nsplit) * sizeof(float) > 136 * 1024) return false;
  Carver c(ws ? (char*)ws + p.g.bytes : nullptr);
  const size_t S = stop_limit, B = d->B, H = d->H, Vp = (d->V + 3) / 4 * 4, Tp = (d->T + 3) / 4 * 4;
  p.g.PART = c.take<float>(S * B * p.g.nsplit * (H + 4));      // (the greedy plan's was sized by its own split)
  p.LOGITS = c.take<float>(S * B * Vp);
  for (int l = 0; l < PDEC_MAX_LAYERS; ++l) p.CS[l] = l < d->n_layers ? c.take<float>((S + 1) * B * H) : nullptr;
  p.FEED = c.take<int32_t>(S * B);
  p.PAR = c.take<int32_t>(S * B);
  p.ORG = c.take<int32_t>(B);
  p.RAW = with_alpha ? c.take<float>(S * B * Tp) : nullptr;
  p.ML = with_alpha ? c.take<float>(S * B * 2) : nullptr;
  p.bytes = p.g.bytes + c.total();
  return true;
}

size_t beam_decode_workspace_bytes(const astk_decoder_desc* d, int N, int K, int stop_limit, int with_alpha) {
  BeamPlan p;
  return beam_plan(d, N, K, stop_limit, with_alpha, nullptr, p) ? p.bytes : 0;
}

int beam_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                       const int32_t* row_len, int N, int K, int go, int eos, int stop_limit, int32_t* n_steps, float* status_dst, int32_t* hist,
                       int32_t* slot_status, double* score, float* c_fin, float* h_fin, float* ht_fin, float* alpha, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  ASTK_CHECK_DESC(d, astk_decoder_desc);
  ASTK_CHECK(N >= 1 && N <= ASTK_BEAM_MAX_N && K >= 1 && K <= ASTK_BEAM_MAX_K, "beam_decode: N = %d / K = %d outside 1..%d / 1..%d", N, K,
             ASTK_BEAM_MAX_N, ASTK_BEAM_MAX_K);
  ASTK_CHECK(d->V > 1 && K <= d->V && go >= 0 && go < d->V && eos >= 0 && eos < d->V, "beam_decode: go %d / eos %d outside [0, V = %d), or K = %d above V",
             go, eos, d->V, K);
  ASTK_CHECK(stop_limit >= 1 && stop_limit <= ASTK_GREEDY_MAX_STEPS, "beam_decode: stop_limit %d outside [1, %d]", stop_limit, ASTK_GREEDY_MAX_STEPS);
  ASTK_CHECK(beam_layout_ok(d->B, N, K, d->V), "beam_decode: B = %d rows do not end with the last of the N = %d slots of an utterance (%d "
             "utterances per 16-row tile)", d->B, N, 16 / N);
  BeamPlan p;
  ASTK_CHECK(beam_plan(d, N, K, stop_limit, alpha != nullptr, nullptr, p), "beam_decode: B = %d, H = %d, %d layers (or the knob dec.persist = 0) does "
             "not run on the device loop: astk_beam_decode_workspace_bytes returns 0, decode with astk_beam_step", d->B, d->H, d->n_layers);
  ASTK_CHECK(ws && ws_bytes >= p.bytes, "beam_decode: workspace too small (%zu < %zu)", ws_bytes, p.bytes);
  ASTK_CHECK(prm && enc && c0 && h0 && n_steps && hist && slot_status && score && c_fin && h_fin && ht_fin, "beam_decode: null pointer");
  ASTK_CHECK(((uintptr_t)hist & 15) == 0 && ((uintptr_t)score & 7) == 0, "beam_decode: hist must be 16-byte aligned and score 8-byte aligned");
  beam_plan(d, N, K, stop_limit, alpha != nullptr, ws, p);
  PDecArgs a = inference_args(d, prm, enc, c0, stop_limit, p.g);
  a.PRED = p.FEED; a.PAR = p.PAR; a.LOGITS = p.LOGITS; a.ALPHA = p.RAW; a.ML = p.ML;
  a.BHIST = hist; a.BSTATUS = slot_status; a.BSCORE = score; a.BORG = p.ORG;
  for (int l = 0; l < d->n_layers; ++l) a.CS[l] = p.CS[l];
  a.bN = N; a.bK = K; a.go = go; a.eos = eos;
  a.n_steps_out = n_steps; a.status_dst = status_dst;
  a.row_len = row_len;
  ASTK_TRY(inference_run(PDEC_BEAM, d, prm, enc, h0, a, p.g, s));
  BeamFinalArgs f;
  memset(&f, 0, sizeof(f));
  f.org = p.ORG; f.HT = p.g.HT; f.c_fin = c_fin; f.h_fin = h_fin; f.ht_fin = ht_fin;
  f.B = d->B; f.H = d->H; f.A = d->A; f.nl = d->n_layers;
  for (int l = 0; l < d->n_layers; ++l) { f.CS[l] = p.CS[l]; f.HR[l] = p.g.HR[l]; }
  hipLaunchKernelGGL(k_beam_final_states, dim3(d->B), dim3(256), 0, s, f);
  ASTK_LAUNCH_CHECK();
  if (alpha) {
    hipLaunchKernelGGL(k_alpha_normalise, dim3(a.S * a.B), dim3(256), 0, s, p.RAW, p.ML, alpha, row_len, a.B, a.T, a.Tp);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace astk
