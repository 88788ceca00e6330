// Persistent decoder loops (1-3 layers, all weights resident): decoder_persist.hip, driven by decoder.hip.
#pragma once
#include "common.h"

namespace astk {

constexpr int PDEC_MAX_LAYERS = 3;

struct DecPersistBuffers {  // slices of decoder.hip's DecPlan
  int32_t *TOK, *PRED;
  float *X0, *Q, *ALPHA, *CVH, *HT, *LOGITS, *LOSSROWS;
  float *G[PDEC_MAX_LAYERS], *C[PDEC_MAX_LAYERS], *HR[PDEC_MAX_LAYERS], *HD[PDEC_MAX_LAYERS];
  float *LSE, *PART, *CESTAT, *ENCA, *ML;
  unsigned* ctr;
  // two small buffers the forward launcher zeroes with its own fill launch (HT of step -1 and the first concat row: decoder.hip)
  void* zero_a; size_t zero_a_bytes; void* zero_b; size_t zero_b_bytes;
  // ... and the initial states (n_layers, B, H) it copies into C[l] / HR[l] with the same launch (nullptr: the caller copied them)
  const float *c0, *h0;
};
bool decoder_persist_applicable(const astk_decoder_desc* d, int* nsplit_out, int* chunk_out);
// a slice of `chunk` rows at H = 512 takes the specialised (NC = 8) attention phase: astk_decoder_path reports it
bool pdec_special(int H, int chunk);
int decoder_persist_fwd_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const int32_t* y,
                               const int32_t* ytgt, const int32_t* use_truth, const float* emb_mask, const float* rnn_masks, const DecPersistBuffers& bf,
                               float* loss, int32_t* pred_out, hipStream_t s, const float* row_weight = nullptr);

struct DecPersistBwdBuffers {
  void* zero_ptr; size_t zero_bytes;      // astk_decoder_desc.zero_ptr: zeroed by the launcher's fill launch
  void* zero2_ptr; size_t zero2_bytes;    // d_enc: zeroed there too, its two batched products then ADD into it from one grouped launch
  const float *WoT, *WcT, *ENCA, *CVH, *HT, *LOGITS, *ML;
  const float *WlT[PDEC_MAX_LAYERS], *WuT[PDEC_MAX_LAYERS], *C[PDEC_MAX_LAYERS];
  float *G[PDEC_MAX_LAYERS];
  float *ALPHA, *DPRE, *DCVH, *DS, *DX0, *DHATT, *d_c0;
  float* DXH;        // [2][S][B][A] or null (no K split of the d_x0 phase)
  unsigned* ctr;
};
// d_x0 phase of the backward kernel as 2 K-halves per item over the ht columns only: fits when the roles still fit 256 workgroups
bool decoder_persist_b6_split(const astk_decoder_desc* d);
int decoder_persist_bwd_launch(const astk_decoder_desc* d, const float* enc, const float* rnn_masks, const DecPersistBwdBuffers& bf,
                               hipStream_t s);

// the inference modes of the forward loop: greedy, scored greedy, sampled, forced and beam decoding (include/astk.h has their contracts)
size_t greedy_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int greedy_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0, int go,
                         int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                         const int32_t* row_len, hipStream_t s);
size_t greedy_scored_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int greedy_decode_scored_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                                int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight, int32_t* tokens,
                                float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                                const int32_t* row_len, hipStream_t s);
size_t sample_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int sample_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0, int go,
                         int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp, int32_t* n_steps,
                         float* status_dst, void* ws, size_t ws_bytes, const int32_t* row_len, hipStream_t s);
size_t sample_topk_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int sample_decode_topk_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                              int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int top_k, float top_p,
                              int32_t* tokens, float* logp, int32_t* n_kept, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                              const int32_t* row_len, hipStream_t s);
int gumbel_rows_launch(const uint64_t* row_keys, int B, int step, int V, float* out, hipStream_t s);
size_t forced_workspace_bytes(const astk_decoder_desc* d, int n_steps, int with_alpha);
int forced_score_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                        const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst, void* ws,
                        size_t ws_bytes, const int32_t* row_len, hipStream_t s);
size_t beam_decode_workspace_bytes(const astk_decoder_desc* d, int N, int K, int stop_limit, int with_alpha);
int beam_decode_launch(const astk_decoder_desc* d, const astk_decoder_params* prm, const float* enc, const float* c0, const float* h0,
                       const int32_t* row_len, int N, int K, int go, int eos, int stop_limit, int32_t* n_steps, float* status_dst, int32_t* hist,
                       int32_t* slot_status, double* score, float* c_fin, float* h_fin, float* ht_fin, float* alpha, void* ws, size_t ws_bytes,
                       hipStream_t s);

}  // namespace astk
