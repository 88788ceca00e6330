/* astk.h -- C ABI of libastk.so: the MI355X (gfx950) encoder-decoder train-step kernels.
 *
 * The reference (0xSameer/ast) has no FFI: its hot path is Python calling Chainer links/functions.
 * Each entry point below replaces the Chainer call sequence of one reference function, cited as
 * /root/reference/<file>:<lines>.  Conventions:
 *   - every pointer is a caller-owned DEVICE pointer (16-byte aligned), sizes are explicit;
 *   - no allocation, no ownership transfer, no implicit synchronisation: functions only enqueue
 *     work on `stream` (a hipStream_t passed as void*), so a caller may capture them in a hipGraph;
 *   - the caller supplies one workspace per op (size from the matching *_workspace_bytes query);
 *     the forward call leaves saved activations in it and the backward call reads them, so it must
 *     stay untouched between the two;
 *   - return 0 on success, <0 on error; astk_last_error() gives the thread-local message;
 *   - weight layouts are Chainer's (A1/A2/A3/A10 of SURVEY.md): Linear W (out,in), LSTM gates
 *     interleaved (unit j, gate k -> row 4j+k, k = a,i,f,o), Conv W (out,in,kh,kw).
 * Storage and accumulation are float32 everywhere, matching the reference's dtype (seq2seq.py:154,302,420).  The PRODUCTS of the
 * batched dense GEMMs run on the 16-bit matrix pipe as bf16x3 splits by default: every f32 operand value is split inside the kernel
 * into three bf16 terms that represent it EXACTLY (f32 exponent range), six term products per useful product, each product exact to
 * 2^-26 -- at least as accurate as an f32 fma chain on any data.  ASTK_PREC_F32 selects the literal f32-input MFMA chain,
 * ASTK_PREC_FP16X2 a faster, NARROWER two-term fp16 split (22 bits, limited exponent range; opt-in, never the default).  Decoder loop,
 * attention, softmax-CE and optimizer are IEEE f32 in every mode; the encoder recurrences follow the mode (bf16x3: weight fragments and
 * every step's activations as exact three-term bf16 splits on v_mfma_f32_16x16x32_bf16; fp16x2: two scaled fp16 terms; f32: f32-input MFMAs).
 * The arithmetic is chosen per call by the descriptors' `precision` field (ASTK_PREC_DEFAULT = the process-wide default).
 */
#ifndef ASTK_H
#define ASTK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASTK_VERSION 113
#define ASTK_MAX_CNN_LAYERS 4
#define ASTK_MAX_RNN_LAYERS 8
#define ASTK_MAX_ATTN 4

int astk_version(void);
const char* astk_last_error(void);

/* Arithmetic of an op's f32-accurate products: field `precision` of the descriptors below, argument of astk_gemm_f32_ex.
 *   ASTK_PREC_DEFAULT  the process-wide default (bf16x3 unless astk_set_gemm_precision changed it)
 *   ASTK_PREC_FP16X2   two fp16 terms per operand behind a per-operand power-of-two scale: 22 significant bits, and only for values within
 *                      2^-17 of the operand's maximum (NARROWER than float32: opt-in), three MFMAs per 16 k; encoder recurrences likewise
 *   ASTK_PREC_BF16X3   three bf16 terms per operand (exact representation of every f32 value, f32 exponent range), six MFMAs per 16 k
 *   ASTK_PREC_F32      v_mfma_f32_32x32x2_f32 / 16x16x4_f32: IEEE f32 products, the reference's literal arithmetic
 * `gemm_operands`: ASTK_OPERANDS_FP16 lets the products a caller marks eligible (K6, K9, batched K18 / K24: BASELINE configs[4]) run with
 * ONE fp16 term per operand (reduced precision; the 1e-4 parity gate does not apply); ASTK_OPERANDS_F32 forces the f32-accurate scheme;
 * ASTK_OPERANDS_DEFAULT = the process-wide setting of astk_set_low_precision_gemms. */
enum { ASTK_PREC_DEFAULT = 0, ASTK_PREC_FP16X2 = 1, ASTK_PREC_BF16X3 = 2, ASTK_PREC_F32 = 3 };
enum { ASTK_OPERANDS_DEFAULT = 0, ASTK_OPERANDS_F32 = 1, ASTK_OPERANDS_FP16 = 2 };

/* ---------------------------------------------------------------- generic f32 MFMA GEMM
 * C[M,N] (+)= op(A) op(B) (+ bias[n]).  layout: 0 = "NT"  A[M,K] K-contiguous, B[N,K] K-contiguous (Linear forward)
 *                                               1 = "NN"  A[M,K], B[K,N]                             (dgrad)
 *                                               2 = "TN"  A[K,M], B[K,N]                             (wgrad)
 * mode: 0 store, 1 C += result (single pass), 2 atomic add with split-K over `ksplit` slices.
 * batch > 1 repeats with element strides sA/sB/sC.  Leading dimensions must be multiples of 4.
 * Replaces the cuBLAS sgemm behind chainer.functions.linear / its backward (Chainer-sem A2). */
int astk_gemm_f32(int layout, int M, int N, int K,
                  const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                  const float* bias, int mode, int ksplit, int batch, long sA, long sB, long sC, void* stream);
/* The same product under the arithmetic `precision` names (ASTK_PREC_*); astk_gemm_f32 = ASTK_PREC_DEFAULT. */
int astk_gemm_f32_ex(int layout, int M, int N, int K,
                     const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                     const float* bias, int mode, int ksplit, int batch, long sA, long sB, long sC, int precision, void* stream);

/* BASELINE configs[4] ("fp16 MFMA GEMMs"): mode 1 lets the batched products of the CNN layers >= 1 (K6), of the encoder's layer-0
 * input projection (K9) -- forward and backward -- and of the decoder LSTMs' and the output layer's backward (K18, K24: their weight
 * gradients over all steps, the embedding columns of the input gradient) run with operands rounded to fp16 (one
 * v_mfma_f32_32x32x16_f16 per tile, f32 accumulation) instead of the f32-accurate split (below).  Whatever the `precision`, every
 * gradient operand (the CNN's dY, the encoder cells' dz, the decoder's dlogits and dz) and the CNN's and encoder's activations, frames
 * and weights are rounded behind a power-of-two scale taken from the operand's measured absolute maximum (the maximum lands in
 * [2^14, 2^15): fp16's subnormal floor sits 2^-39 below it); the decoder's weights and saved activations, all inside fp16's range, are
 * cast as they are.  A result is the product of the rounded operands up to f32 summation (tests/lowp_model.py).  The per-step products of K18 / K24 live inside the latency-bound decoder loop kernels and stay on f32 MFMAs.  Reduced precision: the 1e-4 fp32 parity gate does not apply in
 * this mode (SURVEY.md 8d asks for the loss drift instead: tests/test_gpu_model.py).  Process-wide DEFAULT for descriptors whose
 * gemm_operands field is ASTK_OPERANDS_DEFAULT; 0 (default) = off. */
int astk_set_low_precision_gemms(int mode);
int astk_get_low_precision_gemms(void);
/* fp16x2 mode only: launches below `flops` floating-point operations do not repay the absolute-maximum pass the scaled fp16 terms
 * need and run as bf16x3 instead.  Default 3e9; 0 = fp16 terms always.  Process-wide; returns the
 * previous value. */
double astk_set_gemm_bf16_split_below(double flops);
/* The process-wide DEFAULT arithmetic (what ASTK_PREC_DEFAULT resolves to), switchable at run time (bench.py times the same step under each):
 *   0  fp16x2: two fp16 terms per operand behind a power-of-two scale, 22 significant bits per operand value, in the batched GEMMs AND in
 *      the encoder's persistent recurrence kernels -- NARROWER than float32, opt-in;
 *   1  bf16x3 (default): three bf16 terms (exact operands, no scales) in the batched GEMMs, exact-f32 MFMAs in the recurrences;
 *   2  f32: v_mfma_f32_32x32x2_f32 / 16x16x4_f32 everywhere (IEEE f32 products, the reference's literal arithmetic).
 * Returns the previous mode (<0: error). */
int astk_set_gemm_precision(int mode);
int astk_get_gemm_precision(void);
/* Tuning knobs: the ONE documented, process-wide switchboard for A/B measurements and fall-backs (the library reads no environment
 * variable).  Read at every launch; not meant to be flipped between a forward call and its backward call (the decoder / CNN backward
 * refuse a workspace whose forward took another kernel path).  Keys (default):
 *   gemm.tile (0 = per launch; 64 | 128 | 256 forces the block tile)     gemm.t256_above (2e10 flops: the 12-wave 256 x 128 kernel from here on)
 *   gemm.grid (-1 = per launch)   gemm.hybrid (1)   gemm.chunk (1)   gemm.chunk_div (4)   gemm.log (0: 1 prints every launch to stderr)
 *   gemm.deterministic (0: process default of the descriptors' `deterministic` field)   gemm.forward_pairs (1; 2 = the forward ops' two-contributor rule for every launch, plain astk_gemm_f32 calls included)   gemm.ticket (libastk_test.so only)
 *   conv.direct0 (1)   conv.seq_fwd (1)   conv.seq_bwd (1)   conv.seq_stats_blocks (1024)   conv.seq_apply_blocks (1024)
 *   dec.persist (1: 0 = per-launch decoder loop)   dec.b6_split (1)   dec.b6_fused (1)   dec.wide (1)
 *   lstm.persist (1: 0 = one fused-cell launch per step)   lstm.hoist (1)   lstm.x3 (1)   lstm.x4 (1)
 *   lstm.rows32 (-1 = 32 batch rows per recurrence workgroup when that spares launches; 0 never; 1 = one wave set doing two tiles, 2 = two
 *   wave sets per SIMD, whenever possible)   lstm.duo_side (0)
 *   lstm.overlap_chunk (0 = sized from the free CUs; else time steps per side-stream chunk)   lstm.side_fwd (1)   lstm.side_bwd (0 = off; n = chunks of the input gradient on side_stream behind the backward recurrence, the rest in line; < 0 every chunk)
 *   row.longk (2048)   persist.spin_limit (0 = 2^22 polls)   colreduce.blocks (256)
 * astk_set_tuning returns 0, or -1 for an unknown key; astk_tuning_key(i) enumerates the keys (NULL behind the last). */
int astk_set_tuning(const char* key, double value);
int astk_get_tuning(const char* key, double* value);
const char* astk_tuning_key(int index);
#ifdef ASTK_TEST_HOOKS
/* Test hook (libastk_test.so only): sets the generation counter of the fp16x2 scale slots (tests preset it close to the 32-bit wrap). */
int astk_debug_set_amax_generation(unsigned gen);
/* Test hook (libastk_test.so only): ONE grouped launch of n products C_i = op(A_i) op(B_i) (dense row-major operands) the way a forward op
 * issues it -- under the forward ops' two-contributor rule when `forward` is set -- for shapes no op of the step produces. */
int astk_debug_gemm_group(int layout, int n, const int* M, const int* N, const int* K, const float* const* A, const float* const* B,
                          float* const* C, int forward, int precision, void* stream);
/* Test hook (libastk_test.so only): astk_debug_gemm_group plus what an op sets per product -- `mode` (0 store / 1 accumulate / 2 atomic),
 * `batch` with the strides sA / sB / sC, the leading dimensions, the fp16-operand mark `lowp` -- and `measure` (bit 0: A, bit 1: B): the
 * operand's absolute maximum is taken in front of the launch and handed to it, as an op does for the operands it measures.  The launch
 * runs under the descriptor fields `precision` / `gemm_operands`.  Not a forward launch. */
int astk_debug_gemm_group_lowp(int layout, int n, const int* M, const int* N, const int* K, const int* batch, const int* mode, const int* lowp,
                               const int* measure, const float* const* A, const long* lda, const long* sA, const float* const* B,
                               const long* ldb, const long* sB, float* const* C, const long* ldc, const long* sC, int precision,
                               int gemm_operands, void* stream);
/* Test hook (libastk_test.so only): astk_debug_gemm_group_lowp plus the addressing an op can give each operand and the result -- per
 * product and operand two-level rows (`tn` > 0: row r at (r / tn) * sg + (r % tn) * st floats; the leading dimension is ignored), indexed
 * rows (`rowidx`, device int32: row r at rowidx[r] * ld; `idx_rows` = rows of the array the indices point into, 0 = a permutation of the
 * operand's own rows), two-level C rows (c_tn, c_sg, c_st) -- and a bias per product (`bias` or its entries may be NULL).  Runs the real
 * grouped launch under `precision` / `gemm_operands`, the process default of "gemm.deterministic" and the tuning knobs in force.  A
 * measured operand (`measure`) must have plain rows.  With `plan_out` the launch's plan is written there as text first (the lines of
 * astk_debug_gemm_plan, `twolvl` as the views decide it, then per product "contrib <product> <n> ...": the workgroups that contribute to each
 * tile, for launches in plain stream-K order with at most 64 tiles); `launch` = 0 stops behind the plan: no operand is touched, no device is needed. */
int astk_debug_gemm_views(int layout, int n, const int* M, const int* N, const int* K, const int* batch, const int* mode, const int* lowp,
                          const int* measure, const float* const* A, const long* lda, const long* sA, const float* const* B,
                          const long* ldb, const long* sB, float* const* C, const long* ldc, const long* sC,
                          const int* a_tn, const long* a_sg, const long* a_st, const int* const* a_rowidx, const long* a_idx_rows,
                          const int* b_tn, const long* b_sg, const long* b_st, const int* const* b_rowidx, const long* b_idx_rows,
                          const int* c_tn, const long* c_sg, const long* c_st, const float* const* bias, int precision,
                          int gemm_operands, int launch, char* plan_out, size_t plan_bytes, void* stream);
/* Test hook (libastk_test.so only): what ONE grouped launch of n dense row-major products (leading dimensions as in astk_debug_gemm_group;
 * per product M, N, K, batch, mode 0 store / 1 accumulate / 2 atomic, the fp16-operand mark `lowp`, and `given` = the caller supplies both
 * operands' maxima) WOULD do under `forward`, the descriptor fields `precision` / `gemm_operands` / `deterministic`, a workgroup cap
 * (0 = none), leading dimensions rounded up to a multiple of 4 floats when `pad_ld` is set, and the astk_set_tuning knobs in force:
 * the launcher's plan as text, one "gemm.log" line per product that is launched, in out[0, out_bytes).  Plans only: no operand is touched, nothing is launched, no device is needed.  Returns 0, or -1 and the
 * usual error text where the launch would be refused. */
int astk_debug_gemm_plan(int layout, int n, const int* M, const int* N, const int* K, const int* batch, const int* mode, const int* lowp,
                         const int* given, int forward, int precision, int gemm_operands, int deterministic, int wg_cap, int pad_ld,
                         char* out, size_t out_bytes);
#endif

/* ---------------------------------------------------------------- CNN front-end  (seq2seq.py:158-180)
 * [Conv2D(no bias) -> (max-pool) -> BatchNorm(train: batch stats) -> ReLU] x n_layers (or, with no_bn, [Conv2D(bias) -> ReLU]), then the (T'',B,C*F') time-major
 * re-layout with feature index c*F'+f (quirk Q9).  Layer 0: in_channels 1, kernel (kt,kf), stride (st,sf),
 * pad (pt,0).  Layers >= 1: kernel (kt,1), stride (st,1), pad (pt,0) -- the shipped cnn_config.
 *
 * Supported geometry: 1..ASTK_MAX_CNN_LAYERS layers; every C a multiple of 4; layer 0 any 1 <= kf <= D, sf >= 1 (sf != kf included:
 * overlapping frequency windows or bins no window covers); every layer kt >= st >= 1 and pt >= 0; no frequency padding, no dilation;
 * every layer's padded input at least kt long.  Anything else is refused by every entry point with a message naming the cause,
 * before a launch.  The shipped stack is (9,13)/(2,13)/4 then (9,1)/(2,1)/4; tests/test_gpu_cnn_geometry.py runs fourteen other
 * stacks (1, 2, 3 and 4 layers, kt 2..13, kf 1..16, st 1..13, pt 0..6, sf below / equal to / above kf) against the float64 reference
 * under the three arithmetic schemes, and the refusals.  Layer-0 shapes with st = 2, kt <= 9, kf <= 14, C a multiple of 16 up to 128
 * and no pooling run as a direct convolution under the default arithmetic; every other shape, and every pooled layer 0, as
 * im2col + GEMM. */
typedef struct {
  size_t struct_size;  /* sizeof(astk_cnn_desc) of the header the caller was built against: every entry point refuses a descriptor whose size
                          differs from its own (the descriptors carry pointers the library writes through -- status_dst here, zero_ptr in the
                          decoder's -- so a caller built against an older layout must fail loudly, not hand over garbage).  ZERO-INITIALISE the
                          struct, set struct_size, then the fields you use: every optional field's "off" value is 0 / NULL. */
  int B, T, D;
  int n_layers;
  int C[ASTK_MAX_CNN_LAYERS];
  int kt[ASTK_MAX_CNN_LAYERS], kf[ASTK_MAX_CNN_LAYERS];
  int st[ASTK_MAX_CNN_LAYERS], sf[ASTK_MAX_CNN_LAYERS];
  int pt[ASTK_MAX_CNN_LAYERS];
  float bn_eps;    /* 2e-5  (Chainer-sem A4) */
  float bn_decay;  /* 0.9 */
  int no_bn;       /* cnn_config.bn = false (seq2seq.py:43-57): Conv2D WITH bias -> ReLU, no BatchNorm; 0 = the shipped configs */
  /* OLD-path extra (enc_dec.py:444-456, `cnn_pool`): F.max_pooling_nd(h, (pool_t, pool_f)) between a layer's convolution and its
   * BatchNorm -- window = stride, no padding, cover_all (the last window may be partial: out = ceil(in / window)).  0 or 1 = none,
   * -1 = the whole extent.  No shipped config sets it. */
  int pool_t[ASTK_MAX_CNN_LAYERS], pool_f[ASTK_MAX_CNN_LAYERS];
  int precision;       /* ASTK_PREC_*: arithmetic of this op's products (0 = process default) */
  int gemm_operands;   /* ASTK_OPERANDS_* (0 = process default) */
  float* status_dst;   /* optional (NULL = none): astk_conv_bn_relu_bwd(_sync) also leaves a copy of the persistent kernels' status word
                          there, written by the op's last kernel -- astk_persist_status_snapshot without a launch of its own (the CNN
                          backward is the train step's last op behind the recurrences).  Ignored by the forward call. */
  int deterministic;   /* backward call: 1 = every accumulated sum of this op (split tiles of the weight / input gradient products) is formed in a
                          fixed order -- bit-reproducible from run to run, a few per cent slower; 0 = the process default (astk_set_tuning
                          "gemm.deterministic", default off: float atomics in arrival order) */
} astk_cnn_desc;

typedef struct {
  const float* W;      /* (C, Cin, kt, kf) */
  const float* gamma;  /* (C) */
  const float* beta;   /* (C) */
  float* avg_mean;     /* (C) running stats, updated in train mode */
  float* avg_var;      /* (C) */
  const float* bias;   /* (C) only with no_bn (gamma, beta, avg_* unused then) */
} astk_cnn_layer_params;

typedef struct {
  float* dW;
  float* dgamma;
  float* dbeta;
  float* dbias;        /* only with no_bn */
} astk_cnn_layer_grads;

/* output dims: T_out = T'', F_out = F', feature dim = C_last*F' */
int astk_conv_bn_relu_out_dims(const astk_cnn_desc* d, int* T_out, int* F_out, int* feat_dim);
size_t astk_conv_bn_relu_workspace_bytes(const astk_cnn_desc* d);
/* X (B,T,D); noise (B,T,D) or NULL: X*noise is the speech-noise product of seq2seq.py:297-305;
 * out (T'',B,C_last*F').  train=0 uses running statistics (chainer.config.train False). */
int astk_conv_bn_relu_fwd(const astk_cnn_desc* d, const astk_cnn_layer_params* layers, const float* X,
                          const float* noise, float* out, void* ws, size_t ws_bytes, int train, void* stream);
/* d_out (T'',B,C_last*F') is overwritten.  Gradients are ACCUMULATED into grads (caller zeroes = cleargrads).
 * The backward call must see the descriptor (incl. `precision` / `gemm_operands`) and the process defaults its forward call saw: which
 * of the workspace's layer-0 buffers exists (the patch matrix of im2col + GEMM, or the frequency-blocked input of the direct convolution
 * kernel, conv.hip) follows from them. */
int astk_conv_bn_relu_bwd(const astk_cnn_desc* d, const astk_cnn_layer_params* layers,
                          const astk_cnn_layer_grads* grads, float* d_out, void* ws, size_t ws_bytes, void* stream);
/* Evaluation mode with PER-ROW frame counts: X (B,T,D) is a batch of utterances of different lengths, row b holding
 * row_len[b] frames (B device int32, 1..T) and ZEROS behind them -- the caller pads; that is a contract, not checked.  Running
 * statistics, no noise.  Every layer's activation of row b is written as zero from the row's own output length on, so
 * out[t < T''(b), b] is what the utterance gives alone (B = 1, T = row_len[b], train = 0) and out[t >= T''(b), b] is exactly 0.
 * out_len (device, B int32; may be NULL) receives T''(b), the T_out astk_conv_bn_relu_out_dims reports for T = row_len[b].
 * At most ASTK_ENCODE_ROWS_MAX rows.  The call reads row_len back and SYNCHRONISES `stream` before its first launch (not capturable)
 * and refuses, before any launch: pooled layers, a length outside 1..T, a row whose lone geometry the library would refuse (a
 * padded input shorter than kt).  Workspace: astk_conv_bn_relu_workspace_bytes.  row_len == NULL: astk_conv_bn_relu_fwd(train = 0). */
#define ASTK_ENCODE_ROWS_MAX 32
int astk_conv_bn_relu_fwd_rows(const astk_cnn_desc* d, const astk_cnn_layer_params* layers, const float* X, const int32_t* row_len,
                               float* out, int32_t* out_len, void* ws, size_t ws_bytes, void* stream);
/* Where the forward call leaves the absolute maximum of `out` (16 64-bit words inside ws; taken by the kernel that writes `out`):
 * pass it on as astk_lstm_stack_desc.x_amax.  Valid from the forward call until ws is reused.  NULL: bad arguments. */
const void* astk_conv_out_amax(const astk_cnn_desc* d, void* ws, size_t ws_bytes);

#ifdef ASTK_TEST_HOOKS
/* Test instrumentation, compiled into libastk_test.so only (tests/test_gpu_model.py, the batch-permutation property).  astk_conv_debug_preact: after a forward call, out
 * [(b,f,t)][c] = the post-BatchNorm pre-activation of `layer` (what the ReLU sees), rows = B*F'*T_layer.  astk_conv_debug_kill_units:
 * the following backward calls of this process zero the upstream gradient of the listed units (n triples layer, row, channel in
 * device memory, caller-owned; n = 0 switches it off).  Two valid float32 evaluations of one batch can disagree on the SIGN of a
 * pre-activation that lies within rounding of the ReLU kink; the test names those units and shows that nothing else differs. */
int astk_conv_debug_preact(const astk_cnn_desc* d, void* ws, size_t ws_bytes, int layer, float* out, void* stream);
int astk_conv_debug_kill_units(const int32_t* units, int n);
#endif

/* Data-parallel BatchNorm with GLOBAL batch statistics (SURVEY.md 8e "SyncBN"): the same two calls with an exchange step.
 * After a layer's local per-channel sums are on the device -- forward (sum y, sum y^2), backward (sum g, sum g*xhat), `n` = 2*C
 * doubles at `stat`, inside the caller's workspace -- the library calls `exchange(user, stat, n, stream)` on the host; the callee
 * enqueues, on `stream`, an in-place SUM of that buffer over the `world` replicas (RCCL all-reduce) and returns 0.  Statistics,
 * running averages and the input gradient then use world * rows samples, which is what one process would compute on the
 * concatenated batch; dgamma / dbeta accumulate the LOCAL sums, like every other parameter gradient (the caller's gradient
 * all-reduce adds the replicas).  exchange == NULL (or world == 1) is astk_conv_bn_relu_fwd / _bwd. */
typedef int (*astk_stat_exchange_fn)(void* user, double* stat, int n, void* stream);
int astk_conv_bn_relu_fwd_sync(const astk_cnn_desc* d, const astk_cnn_layer_params* layers, const float* X, const float* noise,
                               float* out, void* ws, size_t ws_bytes, int train, astk_stat_exchange_fn exchange, void* user,
                               int world, void* stream);
int astk_conv_bn_relu_bwd_sync(const astk_cnn_desc* d, const astk_cnn_layer_params* layers, const astk_cnn_layer_grads* grads,
                               float* d_out, void* ws, size_t ws_bytes, astk_stat_exchange_fn exchange, void* user, int world,
                               void* stream);

/* ---------------------------------------------------------------- encoder LSTM stacks  (seq2seq.py:182-242)
 * n_dirs independent uni-directional stacks of n_layers L.LSTM links (Chainer-sem A1), dropout on each
 * layer's *output* copy only.  Direction 1 consumes frames in the reference's order 0,T-1,...,1 (quirk Q1)
 * and its outputs are flipped before the concat, so enc_states[b,p,h:2h] is what seq2seq.py:231-242 builds. */
typedef struct {
  size_t struct_size;  /* sizeof(astk_lstm_stack_desc), see astk_cnn_desc.struct_size */
  int T, B, in_dim, h, n_layers, n_dirs;
  /* Optional hints that spare the f32-accurate GEMMs their absolute-maximum passes (0 / NULL: every launch measures its operands):
   *   out_bound  an upper bound of |layer output| as the next layer and the weight-gradient products read it: 1 without dropout
   *              (|h| < 1), 1 / (1 - ratio) with the masks of astk_fill_dropout_mask;
   *   x_amax     the maximum words of the input frames x, as left by the kernel that wrote them (astk_conv_out_amax). */
  float out_bound;
  const void* x_amax;
  int precision;       /* ASTK_PREC_*: batched products AND the persistent recurrence kernels (0 = process default) */
  int gemm_operands;   /* ASTK_OPERANDS_* (0 = process default) */
  /* Work BESIDE the recurrences (optional; NULL / 0 = everything in line on `stream`).  The persistent recurrence kernels are latency-bound
   * and occupy one workgroup per (direction, layer, 16-unit slice, batch tile): 96-192 of the 256 CUs at the shipped shape.  With a
   * caller-owned ORDINARY second stream in `side_stream` (hipStream_t; no CU mask needed) the layer-0 batched products run on it in time
   * chunks, each launch capped at `side_wgs` workgroups (0 = the CUs the recurrence grid leaves free), gated by flags in the workspace:
   * forward, chunk k of the input projection is produced on the side stream while the recurrence consumes chunk k-1 (the cells of layer 0 wait
   * for the chunk's flag, bounded spins + abort word like every other hand-off); backward, the input / weight gradient of a chunk starts when the
   * recurrence has passed it.  The capped grids can never keep the recurrence grid from becoming resident.  Both calls join the side stream
   * before they return, so callers see one-stream semantics.  Results are bit-identical to the in-line schedule in the forward pass and
   * equal up to the order of float atomics in the backward pass (identical under `deterministic`: such calls, and calls under the process
   * default "gemm.deterministic", run everything in line).  EXCEPTION, ASTK_PREC_FP16X2: capped launches must not use the scheme's scale slots
   * (a process-wide ring ordered by one stream), so the chunks run on bf16x3 operands while the in-line head runs fp16x2 -- the chunked steps
   * of a tensor are then the more accurate ones, and the result is within the scheme's accuracy of the in-line schedule, not bit-identical.
   * astk_lstm_stack_side_plan reports what a descriptor gets. */
  void* side_stream;
  int side_wgs;
  int deterministic;   /* backward call: 1 = bias gradients and split tiles summed in a fixed order (see astk_cnn_desc.deterministic); 0 = process default */
} astk_lstm_stack_desc;

typedef struct {
  const float* Wu; /* upward.W  (4h, in)  */
  const float* b;  /* upward.b  (4h)      */
  const float* Wl; /* lateral.W (4h, h)   */
} astk_lstm_params;

typedef struct {
  float* dWu;
  float* db;
  float* dWl;
} astk_lstm_grads;

size_t astk_lstm_stack_workspace_bytes(const astk_lstm_stack_desc* d);
/* x (T,B,in); params[dir*n_layers+layer]; masks: NULL or (n_dirs,n_layers,T,B,h) scaled keep-masks indexed by
 * loop step; enc_states (B,T,n_dirs*h); cT,hT (n_dirs,n_layers,B,h) final UN-dropped states. */
int astk_lstm_stack_fwd(const astk_lstm_stack_desc* d, const astk_lstm_params* params, const float* x,
                        const float* masks, float* enc_states, float* cT, float* hT,
                        void* ws, size_t ws_bytes, void* stream);
/* The forward pass (no dropout masks) with PER-ROW lengths: row b of x (T,B,in) holds row_len[b] frames (B device
 * int32, 1..T); what lies behind them is never read into a result.  Row b comes out as the utterance does alone (B = 1, T = row_len[b]):
 * the reverse direction reads its frames 0, n-1, ..., 1 (quirk Q1 with n = row_len[b]), enc_states[b, p < n] holds both halves at the
 * row's own positions, enc_states[b, p >= n] is exactly 0, and cT / hT are the states behind the row's last step.  At most
 * ASTK_ENCODE_ROWS_MAX rows.  Reads row_len back and SYNCHRONISES `stream` before its first launch (not capturable); a length outside
 * 1..T is refused before any launch.  astk_lstm_stack_rows_workspace_bytes: the workspace, or 0 for a descriptor the call does not
 * serve.  row_len == NULL: astk_lstm_stack_fwd without masks. */
size_t astk_lstm_stack_rows_workspace_bytes(const astk_lstm_stack_desc* d);
int astk_lstm_stack_fwd_rows(const astk_lstm_stack_desc* d, const astk_lstm_params* params, const float* x, const int32_t* row_len,
                             float* enc_states, float* cT, float* hT, void* ws, size_t ws_bytes, void* stream);
/* d_enc_states (B,T,n_dirs*h); d_cT,d_hT (n_dirs,n_layers,B,h) or NULL; dx (T,B,in) written (may be NULL). */
int astk_lstm_stack_bwd(const astk_lstm_stack_desc* d, const astk_lstm_params* params, const astk_lstm_grads* grads,
                        const float* x, const float* masks, const float* d_enc_states, const float* d_cT,
                        const float* d_hT, float* dx, void* ws, size_t ws_bytes, void* stream);
/* Same, with the persistent recurrence kernel (all T steps of all cells in one launch, one workgroup on each of 192 CUs at cfg 2,
 * latency-bound) enqueued on `recurrence_stream` and ordered against `stream` with events on both sides; everything else stays on
 * `stream`.  Meant for a stream created with hipExtStreamCreateWithCUMask: with the recurrence confined to one set of CUs and
 * independent work (astk_decoder_bwd_phase PARAMS) on a stream masked to the others, the two overlap without slowing the chain
 * (scratch/overlap_probe.py).  NULL = astk_lstm_stack_bwd. */
int astk_lstm_stack_bwd_on(const astk_lstm_stack_desc* d, const astk_lstm_params* params, const astk_lstm_grads* grads,
                           const float* x, const float* masks, const float* d_enc_states, const float* d_cT,
                           const float* d_hT, float* dx, void* ws, size_t ws_bytes, void* stream, void* recurrence_stream);

/* ---------------------------------------------------------------- attention step  (seq2seq.py:336-357)
 * q = Wa h + ba is computed by the caller (GEMM); this is the scan over enc_states:
 * s[b,t] = enc[b,t,:].q[b,:]; alpha = softmax_t(s) (no mask, quirk Q2); cv[b,:] = sum_t alpha[b,t] enc[b,t,:].
 * One streaming read of enc_states (online softmax), split over nsplit time chunks per batch row.
 * Needs B, T > 0, H % 4 == 0, H <= 2048; anything else, a short workspace or (rows variant) a null row map is refused before the
 * workspace is touched, and astk_attn_workspace_bytes answers 0 for dimensions that are not positive. */
size_t astk_attn_workspace_bytes(int B, int T, int H);
int astk_attn_step_fwd(int B, int T, int H, const float* enc, const float* q, float* alpha, float* cv,
                       void* ws, size_t ws_bytes, void* stream);
/* given d_cv: ds[b,t] = alpha (enc.d_cv - cv.d_cv); dq[b,:] = sum_t ds enc[b,t,:].  One read of enc_states.
 * d_enc is NOT touched here: it is produced once per train step by the deferred batched GEMM in
 * astk_decoder_bwd (d_enc[b] = alpha_b^T d_cv_b + ds_b^T q_b over all steps). */
int astk_attn_step_bwd(int B, int T, int H, const float* enc, const float* alpha, const float* cv,
                       const float* d_cv, float* ds, float* dq, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- decoder loop  (seq2seq.py:318-333, 361-473)
 * embed(+dropout) -> [emb; ht] (input feeding) -> n_layers LSTM(H) -> attention -> ht = tanh(Wc[cv;h]+bc)
 * -> logits = Wo ht + bo -> argmax feedback when not teacher-forced (quirk Q4) -> class-weighted softmax-CE
 * with denominator B (quirk Q6), summed over the L-1 steps. */
typedef struct {
  size_t struct_size;  /* sizeof(astk_decoder_desc), see astk_cnn_desc.struct_size */
  int B, L, T, H, E, A, V, n_layers;
  /* optional features of the reference's model (rnn_config; zero = the shipped configs).  Any of them set routes the loop through
   * the per-launch kernels (astk_decoder_path returns 0): the persistent loop is built for the shipped model only. */
  int n_attn;        /* attention heads on the same decoder state (seq2seq.py:107-121, 381-383); 0 or 1 = one; context W is (A,(n_attn+1)H) */
  int no_feed_attn;  /* rnn_config.feed_attn = false (seq2seq.py:369-374): the decoder LSTM input is the embedding alone (layer-0 in = E) */
  int ln;            /* rnn_config.ln (seq2seq.py:141-143, 200-202): L.LayerNormalization(H) behind every decoder LSTM's dropped output */
  int loss_rows;     /* denominator of the per-step cross-entropy mean (quirk Q6: the batch size); 0 = B.  Set when this call scores a
                        SLICE of a larger batch (the library's own row split of batches the persistent loop cannot hold in one launch) */
  const int32_t* use_truth_host; /* optional HOST copy of the use_truth flags handed to astk_decoder_fwd(_ex) (L-1 entries), or NULL.  A hint for
                        the per-launch loop only: it then computes logits inside the loop just for the steps whose argmax is fed back and
                        scores every step with one product and one softmax-CE launch behind the loop.  Read during the call, not kept. */
  int precision;       /* ASTK_PREC_*: the batched products around the loop (encA, weight gradients, d_enc); the loop itself is IEEE f32 */
  int gemm_operands;   /* ASTK_OPERANDS_* (0 = process default) */
  float* status_dst;   /* optional (NULL = none): astk_decoder_fwd(_ex) also leaves a copy of the persistent kernels' status word there (the
                          Python shim passes &loss[1]), written by the kernel that writes the loss when the persistent loop runs --
                          astk_persist_status_snapshot without a launch of its own.  Ignored by the backward calls. */
  void* zero_ptr;      /* optional (NULL = none): zero_bytes bytes (16-byte aligned, a multiple of 4) that astk_decoder_bwd(_phase)(_ex) zeroes IN
                          FRONT of everything it accumulates -- the Python shim passes the gradient arena when cleargrads() was called since the
                          last backward pass (model.cleargrads() sits between forward_loss and backward in nn.py:175-189): the persistent loop's
                          launcher does it with the fill launch it has anyway, the other paths with a fill of their own.  Ignored by the forward
                          calls and by ASTK_DEC_BWD_PARAMS. */
  size_t zero_bytes;
  int side_wgs;        /* ASTK_DEC_BWD_PARAMS only: cap on the workgroups of every batched product of the phase (0 = none).  A caller that runs the
                          phase on a second stream beside the encoder's backward recurrence passes the CUs that recurrence leaves free, so that
                          these launches can never keep its grid from becoming resident.  ONE STREAM for deterministic calls: the fix-up
                          workspace of the deterministic split tiles is process-wide and serves one launch at a time, so a call for which
                          `deterministic` resolves to 1 (the field, else "gemm.deterministic") must not run beside other GEMM launches --
                          astk_decoder_bwd_phase_ex refuses `side_wgs` > 0 together with it */
  int deterministic;   /* backward calls: 1 = weight-gradient split tiles summed in a fixed order (see astk_cnn_desc.deterministic); 0 = process default */
  float label_smoothing; /* eps of the training loss, finite and 0 <= eps < 1 (0 = the plain cross-entropy):
                          row = w[t]/count ((1-eps)(LSE - x_t) + eps (LSE - mean_v x_v)), uniform over all V classes and weighted by the TARGET's
                          class weight.  Read by astk_decoder_fwd(_ex) only, on every path: the gradient of the logits is formed in the forward
                          call, so the backward calls need nothing.  The greedy, scored, sampled, forced, beam and step-infer entry points
                          ignore it (they only validate it with the rest of the descriptor); argmax and `pred` do not depend on it. */
} astk_decoder_desc;

typedef struct {
  const float* embed;                         /* (V,E) */
  astk_lstm_params lstm[ASTK_MAX_RNN_LAYERS]; /* layer 0 in = E+A, others in = H */
  const float* Wa; const float* ba;           /* attn_Wa (H,H) */
  const float* Wc; const float* bc;           /* context (A,2H) */
  const float* Wo; const float* bo;           /* out     (V,A)  */
  const float* class_weight;                  /* (V) : mask_pad_id, seq2seq.py:152-156 */
  const float* Wa_x[ASTK_MAX_ATTN - 1];       /* attn_Wa1.. (H,H) when n_attn > 1 */
  const float* ba_x[ASTK_MAX_ATTN - 1];
  const float* ln_gamma[ASTK_MAX_RNN_LAYERS]; /* L{i}_dec_ln (H) when ln */
  const float* ln_beta[ASTK_MAX_RNN_LAYERS];
} astk_decoder_params;

typedef struct {
  float* d_embed;
  astk_lstm_grads lstm[ASTK_MAX_RNN_LAYERS];
  float* dWa; float* dba;
  float* dWc; float* dbc;
  float* dWo; float* dbo;
  float* dWa_x[ASTK_MAX_ATTN - 1];
  float* dba_x[ASTK_MAX_ATTN - 1];
  float* d_ln_gamma[ASTK_MAX_RNN_LAYERS];
  float* d_ln_beta[ASTK_MAX_RNN_LAYERS];
} astk_decoder_grads;

size_t astk_decoder_workspace_bytes(const astk_decoder_desc* d);
/* enc (B,T,H); c0,h0 (n_layers,B,H) initial states (zeros for layers the encoder does not seed);
 * y (B,L) int32 targets; use_truth (L-1) int32 flags; emb_mask NULL or (L-1,B,E); rnn_masks NULL or
 * (n_layers,L-1,B,H); outputs: loss (1) = sum over steps, pred (L-1,B) int32 argmax per step (may be NULL). */
int astk_decoder_fwd(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                     const float* c0, const float* h0, const int32_t* y, const int32_t* use_truth,
                     const float* emb_mask, const float* rnn_masks, float* loss, int32_t* pred,
                     void* ws, size_t ws_bytes, void* stream);
/* gradients of `loss` (upstream 1.0).  d_enc (B,T,H), d_c0, d_h0 (n_layers,B,H) are written;
 * parameter gradients are ACCUMULATED into g. */
int astk_decoder_bwd(const astk_decoder_desc* d, const astk_decoder_params* p, const astk_decoder_grads* g,
                     const float* enc, const float* c0, const float* h0, const int32_t* y,
                     const float* emb_mask, const float* rnn_masks,
                     float* d_enc, float* d_c0, float* d_h0, void* ws, size_t ws_bytes, void* stream);
/* The loop with the two per-call options of the reference's train step:
 *   out_mask  NULL or (L-1,B,V) scaled keep-masks of dropout.out (seq2seq.py:394: dropout on the LOGITS; argmax feedback and the
 *             loss both see the dropped logits);
 *   targets   NULL or (B,L) int32: the class ids that are SCORED at step s (column s+1), when they differ from the tokens that are
 *             FED (y): forward_loss's random_out replacement (seq2seq.py:456-465), drawn by the caller on the host.
 * astk_decoder_fwd / astk_decoder_bwd_phase are these with both NULL. */
int astk_decoder_fwd_ex(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                        const float* c0, const float* h0, const int32_t* y, const int32_t* use_truth,
                        const float* emb_mask, const float* rnn_masks, const float* out_mask, const int32_t* targets,
                        float* loss, int32_t* pred, void* ws, size_t ws_bytes, void* stream);
/* ... with one weight per batch row: row_weight NULL or (B) float32.  With r_b = row_weight[b] (NULL: 1) every
 * step's row of batch row b is
 *     row_{s,b}  = r_b w[t] c [ (1 - eps)(LSE - x_t) + eps (LSE - mean_v x_v) ]
 *     dx_{s,b,v} = r_b w[t] c [ softmax(x)_v - (1 - eps)[v == t] - eps / V ]
 * (w = class_weight, c = 1 / loss_rows, eps = label_smoothing).  r_b is any FINITE float, negative and zero included; the weights are
 * not checked on the device.  A row with r_b == 0 adds exactly 0 to the loss and has an exactly-zero gradient row.  pred, the argmax,
 * the fed-back tokens and the status word do not depend on the weights; the backward calls need nothing (the gradient of the logits is
 * formed in this call).  Every path takes it (per-launch, persistent, wide, the row split, which hands each half its part of the
 * vector).  astk_decoder_fwd_ex is this call with row_weight = NULL: the same bits as before the argument existed. */
int astk_decoder_fwd_w(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                       const float* c0, const float* h0, const int32_t* y, const int32_t* use_truth,
                       const float* emb_mask, const float* rnn_masks, const float* out_mask, const int32_t* targets,
                       const float* row_weight, float* loss, int32_t* pred, void* ws, size_t ws_bytes, void* stream);
/* The same backward in two phases, for callers that overlap them: ASTK_DEC_BWD_CHAIN runs the reversed loop and writes
 * everything the encoder's backward needs (d_enc, d_c0, d_h0); ASTK_DEC_BWD_PARAMS accumulates the parameter gradients from
 * what the chain phase left in `ws` -- it only has to be ordered after the chain phase (an event), so it can run on a second
 * stream beside the encoder's latency-bound backward recurrence, which leaves most of the device idle.  The caller joins that
 * stream before it reads g or reuses ws.  ASTK_DEC_BWD_ALL = astk_decoder_bwd. */
enum { ASTK_DEC_BWD_ALL = 0, ASTK_DEC_BWD_CHAIN = 1, ASTK_DEC_BWD_PARAMS = 2 };
int astk_decoder_bwd_phase(const astk_decoder_desc* d, const astk_decoder_params* p, const astk_decoder_grads* g,
                           const float* enc, const float* c0, const float* h0, const int32_t* y,
                           const float* emb_mask, const float* rnn_masks,
                           float* d_enc, float* d_c0, float* d_h0, void* ws, size_t ws_bytes, int phase, void* stream);
int astk_decoder_bwd_phase_ex(const astk_decoder_desc* d, const astk_decoder_params* p, const astk_decoder_grads* g,
                              const float* enc, const float* c0, const float* h0, const int32_t* y,
                              const float* emb_mask, const float* rnn_masks, const float* out_mask,
                              float* d_enc, float* d_c0, float* d_h0, void* ws, size_t ws_bytes, int phase, void* stream);
/* eval-mode single step for predict()/beam (seq2seq.py:361-396 under train=False): states (n_layers,B,H)
 * and ht (B,A) are updated in place; logits (B,V) and alpha (B,T) written. */
int astk_decoder_step_infer(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                            float* c, float* h, float* ht, const int32_t* tokens, float* logits, float* alpha,
                            int32_t* argmax, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- greedy decoding on the device  (seq2seq.py:475-527, predict)
 * The whole eval-mode greedy decode of a batch in ONE persistent launch (the persistent decoder loop in its greedy mode, after a
 * fill launch and the encA product): step 0 feeds `go` to every row, every later step the row's own argmax (first maximum).  Stop
 * rule, the reference's: a row is done from the first step whose argmax is `eos` and stays done, but keeps decoding (its later
 * tokens are defined output); the decode ends after n_steps = the first step count s+1 at which every row is done, or stop_limit.
 * Runs where the persistent training loop runs (astk_decoder_path != 0 for the same shape, with the step count set to stop_limit)
 * and the tuning knob dec.persist is on, for B <= 32 and stop_limit <= ASTK_GREEDY_MAX_STEPS; otherwise
 * astk_greedy_workspace_bytes returns 0 and the caller decodes with astk_decoder_step_infer step by step.  d->L and d->status_dst
 * are ignored. */
#define ASTK_GREEDY_MAX_STEPS 512
size_t astk_greedy_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
/* enc (B,T,H), c0/h0 (n_layers,B,H) as for astk_decoder_fwd; tokens (stop_limit,B) int32 device, rows [0, *n_steps) defined (rows at
 * and past n_steps: unspecified); n_steps: one device int32; status_dst (optional, NULL = none): a copy of the persistent kernels'
 * status word as a float (see astk_persist_status_snapshot), written by the launch -- non-zero: a bounded spin timed out and the
 * tokens are invalid.  n_steps and status_dst are written by the last workgroup to finish.  Returns < 0 with a message (and launches
 * nothing) for a wrong struct_size, go / eos outside [0, V), stop_limit outside [1, ASTK_GREEDY_MAX_STEPS], a shape that does not
 * run on the device loop, a null pointer or a workspace below astk_greedy_workspace_bytes. */
int astk_greedy_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                       int go, int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst,
                       void* ws, size_t ws_bytes, void* stream);

/* The same decode, scored (the greedy loop of the reference's older trainer with targets: enc_dec.py:372-429): the kernel keeps each
 * step's log-sum-exp and returns, beside the tokens,
 *   logp[s][b] = log p(tokens[s][b])                                  (maximum logit - LSE), and, with targets,
 *   nll[s][b]  = w[y[b][s+1]] * (LSE - logit[y[b][s+1]])              the free-running cross-entropy term of step s, row b
 * (w = class_weight, NULL = all 1; its index is clamped to [0, V)).  y is (B, ldy) int32 on the device or NULL; a step with
 * s + 1 >= ldy has no target and writes nll = 0.  tokens, logp and nll are (stop_limit, B) on the device, rows [0, *n_steps) defined;
 * nll is NULL exactly when y is.  The decode is astk_greedy_decode's in every case: same stop rule, same tokens, same shapes (the
 * workspace query returns 0 where astk_greedy_workspace_bytes does).  Fails like astk_greedy_decode, and also for a null logp, nll
 * without y or y without nll, or ldy < 1. */
size_t astk_greedy_scored_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int astk_greedy_decode_scored(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                              int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight, int32_t* tokens,
                              float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- sampled decoding on the device  (ancestral sampling, Gumbel-max)
 * The greedy decode with every step's token DRAWN from softmax(logits / temperature) instead of taken at the maximum: a draw from
 * softmax(x * inv_temp) is the first maximum of x_n * inv_temp + g_n over independent Gumbel noise g_n, so the persistent loop runs
 * its greedy protocol unchanged (same hand-offs, stop rule and exits) on perturbed scores.  The noise is a contract, a pure function
 * of (seed, stream, decoder step s, class id n) that a host can restate (ast_amd.seq2seq.sample_row_key / gumbel_noise):
 *   mix64(z)              : z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                           z ^ z >> 31                                           (uint64 arithmetic, the splitmix64 finaliser)
 *   row_key(seed, stream) = mix64(seed ^ mix64(stream))                             one per batch row, formed on the host
 *   word(b, s, n)         = mix64(row_key[b] ^ ((uint64)s << 32 | (uint64)n))
 *   u                     = (float)((word >> 40) + 1) * c                           one float32 multiply, c = the float32 next to
 *                           1 / 16777217 (0x1.fffffep-25 = 2^-24 (1 - 2^-24)): u lies in (0, 1), 1 - 2^-24 at the most
 *   g(b, s, n)            = -ln(-ln(u))                                             float32, within 5e-6 of the float64 value of u
 *   tokens[s][b]          = the first maximum over n < V of z_n = x_n * inv_temp + g(b, s, n)
 *   logp[s][b]            = x_tok * inv_temp - LSE_n(x_n * inv_temp)                log-probability under the sampled distribution
 * A row's draws depend on (seed, stream, s, n) alone: not on the row's position, nor on the batch around it.  (mix64(0) =
 * 0xE220A8397B1DCDAF, row_key(2024, 0) = 0xEE8C6C05E85E6BD6.)
 * astk_sample_decode is astk_greedy_decode_scored without targets, plus row_keys (B uint64 on the device) and inv_temp = 1 /
 * temperature: tokens and logp are (stop_limit, B) on the device, rows [0, *n_steps) defined; a row counts as finished once it has
 * DRAWN eos.  Same shapes and workspace as the greedy modes (astk_sample_workspace_bytes returns 0 where astk_greedy_workspace_bytes
 * does; such shapes sample step by step: astk_decoder_step_infer, astk_gumbel_rows, argmax of logits * inv_temp + g).  Fails with a
 * message (and launches nothing) for everything astk_greedy_decode_scored refuses, a null row_keys or logp, or an inv_temp that is
 * not finite or is <= 0.
 * astk_gumbel_rows writes one step's noise, out[b][n] = g(b, step, n) for b < B, n < V, as a dense (B, V) buffer.
 * astk_sample_row_key is row_key(seed, stream): host arithmetic only. */
size_t astk_sample_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int astk_sample_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                       int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp,
                       int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream);
int astk_gumbel_rows(const uint64_t* row_keys, int B, int step, int V, float* out, void* stream);
uint64_t astk_sample_row_key(uint64_t seed, uint64_t stream);

/* ---------------------------------------------------------------- truncated sampling on the device  (top-k and top-p / nucleus)
 * astk_sample_decode with every draw restricted to a few of the best tokens.  The noise contract above stays as it is.  One draw per
 * row b and step s, from the float32 logits x_n; the parameters are inv_temp > 0, top_k in 1..ASTK_SAMPLE_MAX_TOPK (= 16), top_k <= V,
 * and top_p in (0, 1]:
 *   1. Scaled logits.   xs_n = x_n * inv_temp in float32, as in the sampled mode.
 *   2. Candidates.      The top_k largest xs_n form the candidates (xs_j, id_j), j = 0..K-1: higher values first, among equal values
 *                       the lower token id first (beam mode's order).  The rank is taken on the float32 xs.
 *   3. Nucleus.         q_j = exp(xs_j - LSE_K) over the K candidates; m is the smallest count >= 1 whose prefix sum of q is >= top_p,
 *                       m = K if no prefix reaches top_p, and top_p == 1 skips the cut: m = K exactly, whatever the rounding.  So
 *                       top-p is applied to the renormalised top-k survivors: the order the common toolkits use when both are given.
 *   4. Draw.            tokens[s][b] = the id_j with the largest z_j = xs_j + g(b, s, id_j), j < m: g is the noise function above, of
 *                       (row key, step, class id); among equal z the lower token id wins.
 *   5. Log-probability. logp[s][b] = xs_tok - LSE over the m kept, formed as (xs_tok - xs_0) - logf(sum_j exp(xs_j - xs_0)), without
 *                       rounding an LSE first.  This is the log-probability under the distribution actually sampled.  It is NOT the
 *                       model's full-softmax log-probability; forced scoring (astk_forced_score) gives that.
 * Consequences: top_k = 1 gives the greedy tokens and logp == 0; a row's draws depend on (seed, stream, s, its own logits) alone; the
 * stop rule is the sampled mode's: a row is finished once it has DRAWN eos.
 * astk_sample_decode_topk is astk_sample_decode_rows plus top_k, top_p and n_kept ((stop_limit, B) int32 on the device, the kept count
 * m of every draw, rows [0, *n_steps) defined; NULL = none); row_len as for the *_rows entry points below, NULL allowed.  The
 * persistent loop keeps each step's xs and finds the candidates in its combine phase: no noise is evaluated beyond the kept ids.
 * The workspace is the greedy plan plus that buffer; astk_sample_topk_workspace_bytes returns 0 exactly where
 * astk_greedy_workspace_bytes does (such shapes sample step by step).  Fails with a message (and launches nothing) for everything
 * astk_sample_decode refuses, for top_k outside 1..ASTK_SAMPLE_MAX_TOPK or above V, for a top_p that is not finite, is <= 0 or > 1,
 * and for a workspace below the query. */
#define ASTK_SAMPLE_MAX_TOPK 16
size_t astk_sample_topk_workspace_bytes(const astk_decoder_desc* d, int stop_limit);
int astk_sample_decode_topk(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int top_k, float top_p,
                            int32_t* tokens, float* logp, int32_t* n_kept, int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes,
                            void* stream, const int32_t* row_len);

/* ---------------------------------------------------------------- forced decoding on the device  (score a given translation)
 * The eval-mode decoder run along given tokens in ONE persistent launch (the persistent decoder loop in its forced mode, after a fill
 * launch and the encA product): step s feeds y[b][s] to row b and scores y[b][s+1], for s in [0, S), S = ldy - 1 (ids are clamped to
 * [0, V) where they index).  There is no stop rule: every step of every row is computed.  Outputs, on the device:
 *   logp[s][b]     = logit[y[b][s+1]] - LSE          the unweighted log-probability of the target (PAD weights are the caller's)
 *   logp_max[s][b] = maximum logit - LSE             optional (NULL = none)
 *   pred[s][b]     = argmax, first maximum           optional
 *   alpha[s][b][t] = the attention row, t < d->T     optional, (S, B, d->T) dense; written by one more small launch behind the loop
 *   status_dst     = as for astk_greedy_decode       optional
 * y is (B, ldy) int32 on the device.  Runs where astk_greedy_workspace_bytes(d, S) is non-zero; otherwise
 * astk_forced_workspace_bytes returns 0 and the caller scores with astk_decoder_step_infer step by step.  with_alpha != 0: the
 * workspace also holds the raw scores (pass the same choice as alpha != NULL).  d->L and d->status_dst are ignored.  Returns < 0 with
 * a message (and launches nothing) for a wrong struct_size, ldy outside [2, ASTK_GREEDY_MAX_STEPS + 1], a shape that does not run on
 * the device loop, a null enc / c0 / h0 / y / logp / p or a workspace below astk_forced_workspace_bytes. */
size_t astk_forced_workspace_bytes(const astk_decoder_desc* d, int n_steps, int with_alpha);
int astk_forced_score(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                      const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst,
                      void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- per-row source lengths in the four decode modes
 * Each *_rows entry point is its counterpart above plus row_len (B int32 on the device, or NULL): row b attends over positions
 * [0, row_len[b]) of enc[b] only -- a batch of DIFFERENT utterances, each encoded alone and padded to d->T rows, decodes every row as
 * that row alone would (ast_amd.seq2seq RowBatch).  enc rows at and beyond a row's length enter no sum: whatever finite values they
 * hold, no output bit depends on them.  astk_forced_score_rows writes alpha[s][b][t] = 0 for t >= row_len[b].  NULL is the
 * counterpart itself (which forwards here with NULL), and row_len[b] = d->T for every b gives its results to the bit.  Workspaces
 * are the counterparts' (the same queries, the same bytes), and so is every failure with a message.  The lengths are device data
 * and are NOT checked here: the caller guarantees 1 <= row_len[b] <= d->T for every b < d->B (ast_amd checks before it uploads); a
 * length outside that range is clamped to it by the kernel, and a row of length 0 would divide by an empty softmax sum. */
int astk_greedy_decode_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, int32_t* tokens, int32_t* n_steps, float* status_dst,
                            void* ws, size_t ws_bytes, void* stream, const int32_t* row_len);
int astk_greedy_decode_scored_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0,
                                   const float* h0, int go, int eos, int stop_limit, const int32_t* y, int ldy, const float* class_weight,
                                   int32_t* tokens, float* logp, float* nll, int32_t* n_steps, float* status_dst, void* ws,
                                   size_t ws_bytes, void* stream, const int32_t* row_len);
int astk_sample_decode_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                            int go, int eos, int stop_limit, const uint64_t* row_keys, float inv_temp, int32_t* tokens, float* logp,
                            int32_t* n_steps, float* status_dst, void* ws, size_t ws_bytes, void* stream, const int32_t* row_len);
int astk_forced_score_rows(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                           const int32_t* y, int ldy, float* logp, float* logp_max, int32_t* pred, float* alpha, float* status_dst,
                           void* ws, size_t ws_bytes, void* stream, const int32_t* row_len);

/* ---------------------------------------------------------------- batched beam search  (nn.py:235-322 over many utterances)
 * U utterances, N hypotheses kept per utterance, K candidates per live hypothesis: every slot is one row of ONE decoder step over
 * R = U*N rows, row u*N + j = slot j of utterance u.  enc is (U, T, H): utterance u's encoder states in enc[u, 0:T''_u] (the rest
 * is never read); row r attends over its utterance's T''_u positions only.  A step, per utterance and in the reference's order:
 * slot by slot, an empty slot contributes nothing, a finished one (status 2) itself, a live one (status 1) its K best tokens by
 * float64 log_softmax (equal log-probabilities: lower token id first) with score = score_j + logp; the N best candidates are kept
 * (equal scores: the earlier candidate).  A new expansion takes the states its parent row computed in this step, a carried slot
 * keeps its own.  An utterance whose non-empty slots have all finished is frozen (frozen[u] = 1, *n_frozen counts them); further
 * steps only carry it again.  Limits: N and K at most 16. */
#define ASTK_BEAM_MAX_N 16
#define ASTK_BEAM_MAX_K 16
typedef struct {
  size_t struct_size;  /* sizeof(astk_beam_desc), see astk_cnn_desc.struct_size */
  int U, N, K;
  int S;               /* steps the history buffers hold (the stop limit); `step` runs 0..S-1 */
  int T;               /* T''max: positions per utterance of enc and of the alpha history */
  int V;               /* vocabulary (the decoder's) */
  int eos;             /* id of the token that finishes a hypothesis */
  const int32_t* lengths_host;  /* HOST, U entries: T''_u in 1..T (checked at every call; the kernels read row_len) */
} astk_beam_desc;

typedef struct {       /* caller-owned DEVICE buffers of a search; the caller seeds them (slot 0 live with the encoder's final states) */
  size_t struct_size;  /* sizeof(astk_beam_state) */
  const int32_t* row_utt;  /* (R) utterance of every row (r / N) */
  const int32_t* row_len;  /* (R) T''_u of every row's utterance */
  float* c; float* h;      /* (n_layers, R, H) decoder states of every slot */
  float* ht;               /* (R, A) attentional vector of every slot */
  int32_t* tokens;         /* (R) last token of every slot */
  double* score;           /* (R) */
  int32_t* status;         /* (R) 0 empty, 1 live, 2 finished */
  int32_t* frozen;         /* (U) */
  uint32_t* n_frozen;      /* (1) */
  int32_t* hist;           /* (S, R, 4) per step and new slot: parent slot (-1: empty), token, carried (1) or new expansion (0), 0 */
  float* hist_alpha;       /* (S, R, T) the parent row's (first head's) alpha of the step, for new expansions only */
} astk_beam_state;

/* d: the decoder's descriptor with B = U*N, T = T''max (its L is ignored: one step). 0 = bad arguments. */
size_t astk_beam_workspace_bytes(const astk_beam_desc* b, const astk_decoder_desc* d);
/* One step for all R rows: decoder step (astk_decoder_step_infer's kernels, per-row attention), selection, history row `step`,
 * state gather. */
int astk_beam_step(const astk_beam_desc* b, const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                   const astk_beam_state* st, int step, void* ws, size_t ws_bytes, void* stream);
/* The selection and gather alone, on a step's results supplied by the caller: logits (R, V), alpha (R, ld_alpha >= T), the new
 * states c_new / h_new (n_layers, R, H) and ht_new (R, A) every row computed. */
int astk_beam_select(const astk_beam_desc* b, int n_layers, int H, int A, const float* logits, const float* alpha, long ld_alpha,
                     const float* c_new, const float* h_new, const float* ht_new, const astk_beam_state* st, int step, void* stream);
/* ---------------------------------------------------------------- joint CTC-attention beam search
 * astk_beam_step with every candidate ranked by (1 - w) * log p_att + w * log p_ctc(prefix): the CTC prefix score psi of Hori /
 * Watanabe over the logits of the section-28 head, float64 in the log domain.  Not in the reference: a caller asks for it.
 *   x[t][c]      float64 log_softmax of utterance u's float32 logits[u][t][0:V] (log-sum-exp in float64), t < T''_u; frames behind
 *                T''_u are never read
 *   a slot       holds a prefix g of n_labels tokens behind GO whose last one is astk_beam_state.tokens, att_score = its attention
 *                log-probability, psi = psi(g), and its CTC state (T, 2): r_n[t], r_b[t] = the log-probability of all alignments of g
 *                over frames 0..t that end in a non-blank / a blank.  Empty prefix: r_n = -inf, r_b[t] = sum_{s<=t} x[s][blank], psi = 0
 *   g.c, c >= first_label, m = max(n, 1):   phi[t] = r_b[t] if c is g's last token, else logaddexp(r_n[t], r_b[t]);
 *                r_n'[m-1] = x[0][c] if n = 0, else -inf;  r_b'[m-1] = -inf;  everything in front -inf;  for t >= m
 *                r_n'[t] = logaddexp(r_n'[t-1], phi[t-1]) + x[t][c],  r_b'[t] = logaddexp(r_n'[t-1], r_b'[t-1]) + x[t][blank];
 *                psi(g.c) = logsumexp(r_n'[m-1], {phi[t-1] + x[t][c] : m <= t < T''_u});  m > T''_u: psi = -inf, the state all -inf
 *   c = eos      psi = logaddexp(r_n[T''_u - 1], r_b[T''_u - 1]) (the utterance is exactly g); state and n_labels stay the parent's
 *   other c      (ids below first_label: the blank, GO) psi = -inf, the state all -inf
 * A step: every live row proposes its K best tokens by float64 attention log_softmax exactly as astk_beam_step does; a proposal's
 * ranking score is (1 - w) * (att_score_j + logp) + w * psi(g.c) from the two absolute terms, -inf where psi is -inf (NaN ranks as
 * -inf); merge with the carried slots, stable top-N, history, frozen flags and the decoder-state gather are astk_beam_step's.  The
 * gather also moves att_score, psi, n_labels and the CTC state (a new expansion takes its candidate's, a carried slot and an eos
 * expansion keep the parent's own); astk_beam_state.score holds the ranking score.  Limits: T <= ASTK_BEAM_CTC_MAX_T, eos and the
 * blank below first_label.  Every -inf case yields -inf, never NaN. */
#define ASTK_BEAM_CTC_MAX_T 2048
typedef struct {
  size_t struct_size;    /* sizeof(astk_beam_ctc) */
  double weight;         /* w in (0, 1] */
  int blank;             /* the CTC blank (the model's PAD) */
  int first_label;       /* ids >= first_label are labels (the model's UNK) */
  const float* logits;   /* DEVICE (U, T, ldv): the head's logits of the padded encoder states (astk_ctc_head_fwd) */
  long ldv;              /* >= V */
  double* state;         /* DEVICE (R, T, 2) caller-owned: the slots' r_n, r_b */
  double* att_score;     /* DEVICE (R) */
  double* psi;           /* DEVICE (R) */
  int32_t* n_labels;     /* DEVICE (R) */
  void* ws;              /* DEVICE, astk_beam_ctc_workspace_bytes, 256-byte aligned; holds what astk_beam_ctc_init computed: keep it */
  size_t ws_bytes;       /*         untouched between the init and the last step of a search */
} astk_beam_ctc;
/* 0 = bad arguments (astk_last_error).  Per-frame lse (U, T) float64, the logits as (U, V, T) so that a candidate's column is
 * contiguous, the proposals (R, K) and their new CTC states (R, K, T, 2). */
size_t astk_beam_ctc_workspace_bytes(const astk_beam_desc* b, const astk_beam_ctc* ctc);
/* Once per search, three launches: lse and the (U, V, T) copy into ctc->ws, then the empty prefix's state in slot 0 of every utterance
 * and att_score = psi = 0, n_labels = 0 in every slot. */
int astk_beam_ctc_init(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* ctc, void* stream);
/* astk_beam_step with the joint ranking: decoder step, proposals, prefix scores, selection and gather (ws: astk_beam_workspace_bytes). */
int astk_beam_step_ctc(const astk_beam_desc* b, const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc,
                       const astk_beam_state* st, const astk_beam_ctc* ctc, int step, void* ws, size_t ws_bytes, void* stream);
/* astk_beam_select's counterpart: proposals, prefix scores, selection and gather on a step's results supplied by the caller. */
int astk_beam_select_ctc(const astk_beam_desc* b, int n_layers, int H, int A, const float* logits, const float* alpha, long ld_alpha,
                         const float* c_new, const float* h_new, const float* ht_new, const astk_beam_state* st,
                         const astk_beam_ctc* ctc, int step, void* stream);
/* ---------------------------------------------------------------- beam search on the device  (the whole search in one launch)
 * The search of astk_beam_step for up to 32 rows in ONE persistent launch (the persistent decoder loop in its beam mode, after a fill
 * launch and the encA product, followed by one small launch that gathers the final states and, with alpha, one that normalises it).
 * Row layout: every slot of every utterance is one row of d->B <= 32 rows.  The N slots of an utterance lie inside one 16-row batch
 * tile: a tile holds 16 / N (integer division) utterances, utterance i of tile t in rows 16 t + i N .. 16 t + i N + N - 1; the tile's
 * remaining rows are padding that is never live (6 utterances per launch at N = 5, 2 at N = 16).  d->B ends with the last slot of the
 * last utterance.  enc is (B, T, H) -- every row holds its utterance's encoder states, as for the *_rows entry points -- and row_len
 * (B, or NULL) its length; c0 / h0 (n_layers, B, H) seed slot 0 of every utterance (every other row: any finite values, e.g. zeros).
 * At step 0 only slot 0 of an utterance is live and every row is fed `go`.  Selection is astk_beam_step's rule with two differences
 * of arithmetic: the K best tokens of a row are ranked by the float32 logit (equal logits: lower id first), and logp = logit - LSE uses
 * the float32 LSE of astk_greedy_decode_scored; scores accumulate in float64.  The loop stops after the step at which no utterance has
 * a live slot (n_steps, as astk_greedy_decode; stop_limit otherwise).  Outputs, on the device:
 *   n_steps, status_dst                   as for astk_greedy_decode
 *   hist (stop_limit, B, 4)               astk_beam_state.hist's record of every row and step < n_steps; 16-byte aligned (checked)
 *   slot_status (B), score (B) float64    of the slots after the last step; score 8-byte aligned (checked)
 *   c_fin, h_fin (n_layers, B, H), ht_fin (B, A)   the state every slot's hypothesis was last expanded from (an empty slot: zeros)
 *   alpha (stop_limit, B, d->T)           optional: alpha[s][r] is the attention row that ROW r computed at step s; the alpha of the
 *                                         expansion recorded at hist[s][r] is that of its PARENT row, alpha[s][parent row].
 *                                         Defined for s < n_steps only: the rows of steps the loop never ran hold no meaningful value
 * Every row attends through PDEC_BEAM_NSPLIT = 8 slices cut by its OWN length, whatever d->B and d->T: the results of an utterance's
 * rows are the same to the bit in every launch that holds them, next to whatever other utterances.
 * astk_beam_decode_workspace_bytes returns 0 where astk_greedy_workspace_bytes does, and for N or K outside 1..16, K > V, a d->B
 * that the layout above does not produce, or H = 512 with d->T > 480 (one attention kernel per H, see above); the caller then searches with astk_beam_step. */
size_t astk_beam_decode_workspace_bytes(const astk_decoder_desc* d, int N, int K, int stop_limit, int with_alpha);
int astk_beam_decode(const astk_decoder_desc* d, const astk_decoder_params* p, const float* enc, const float* c0, const float* h0,
                     const int32_t* row_len, int N, int K, int go, int eos, int stop_limit, int32_t* n_steps, float* status_dst,
                     int32_t* hist, int32_t* slot_status, double* score, float* c_fin, float* h_fin, float* ht_fin, float* alpha,
                     void* ws, size_t ws_bytes, void* stream);

/* The attention scan of astk_attn_step_fwd with per-row encoder slices: row r attends over enc[row_utt[r], 0:row_len[r]] of enc
 * (U, T, H); alpha (R, Tp) is 0 from row_len[r] on.  Workspace: astk_attn_workspace_bytes(R, T, H). */
int astk_attn_step_fwd_rows(int R, int T, int H, const float* enc, const int32_t* row_utt, const int32_t* row_len, const float* q,
                            float* alpha, float* cv, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- normalisation layers of the optional encoder variants
 * L.LayerNormalization(units) behind an LSTM (rnn_config.ln; seq2seq.py:85-87, 200-202): rows x n, row strides ld*, per-row mean and
 * BIASED variance, y = (x - mu) / sqrt(var + eps) * gamma + beta (eps 1e-6, the link's default).  Backward recomputes the statistics
 * from x; dgamma / dbeta are ACCUMULATED (NULL: skipped), dx written (NULL: skipped). */
int astk_layernorm_fwd(int rows, int n, const float* x, long ldx, const float* gamma, const float* beta, float eps, float* y, long ldy,
                       void* stream);
int astk_layernorm_bwd(int rows, int n, const float* x, long ldx, const float* gamma, float eps, const float* dy, long lddy, float* dx,
                       long lddx, float* dgamma, float* dbeta, void* stream);
/* The projection between encoder layers of rnn_config.linear_proj (seq2seq.py:89-99, 280-286): out_t = relu(BN(z_t)) for every time
 * step t, z (T,B,C) = the Linear's output (a GEMM of the caller).  The reference calls its BatchNormalization link once per step on
 * a (B,C) matrix: batch statistics over the B rows OF THAT STEP, running averages advanced T times in step order (m = B samples).
 * stats (T,2,C) receives every step's mean and biased variance (read by the backward); train = 0 uses the running statistics. */
int astk_step_bn_relu_fwd(int T, int B, int C, const float* z, const float* gamma, const float* beta, float* avg_mean, float* avg_var,
                          float eps, float decay, int train, float* out, float* stats, void* stream);
/* dz written; dgamma / dbeta ACCUMULATED. */
int astk_step_bn_relu_bwd(int T, int B, int C, const float* z, const float* stats, const float* gamma, float eps, const float* out,
                          const float* d_out, float* dz, float* dgamma, float* dbeta, void* stream);

/* ---------------------------------------------------------------- softmax cross-entropy  (seq2seq.py:468-470)
 * rows = B: loss_rows[b] = -w[t_b] log_softmax(x_b)[t_b] / B ; dlogits = w[t_b](softmax - onehot)/B written in
 * place of logits; argmax (first maximum) written when non-NULL.  (Chainer-sem A6) */
int astk_softmax_ce_fwd(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride,
                        const float* class_weight, float inv_count, float* loss_rows, int32_t* argmax, void* stream);
/* ... with label smoothing eps (finite, 0 <= eps < 1; astk_decoder_desc.label_smoothing):
 * loss_rows[b] = w[t_b]/B ((1-eps)(LSE - x_t) + eps (LSE - mean_v x_v)); dlogits = w[t_b](softmax - (1-eps) onehot - eps/V)/B.
 * astk_softmax_ce_fwd is this call with eps = 0. */
int astk_softmax_ce_fwd_ex(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride,
                           const float* class_weight, float inv_count, float label_smoothing, float* loss_rows, int32_t* argmax,
                           void* stream);
/* ... with one weight per row: row_weight NULL or (B) float32, finite (not checked on the device), any sign; a factor on
 * class_weight[t_b], so on loss_rows[b] and on the row of dlogits alike; a zero weight gives an exactly-zero row of both.  argmax does
 * not depend on it.  astk_softmax_ce_fwd_ex is this call with row_weight = NULL. */
int astk_softmax_ce_fwd_w(int B, int V, long ld, float* logits_inout, const int32_t* targets, long t_stride,
                          const float* class_weight, const float* row_weight, float inv_count, float label_smoothing, float* loss_rows,
                          int32_t* argmax, void* stream);

/* ---------------------------------------------------------------- optimizer  (nn.py:81-119, Chainer-sem A7/A8)
 * One flat parameter / gradient buffer.  ONE norm launch at a time per process: astk_grad_sqnorm(_scaled) folds its per-block partial
 * sums through a process-wide scratch (no zeroing launch in front, a block-order sum whatever order the blocks finish in), so calls must
 * be ordered on one stream at a time -- which a train step's single optimizer is; astk_persist_status(.., reset = 1) also re-arms it.
 * sqnorm[0] = sum (g + l2*p)^2 in float64 (the clip norm of hook order
 * WeightDecay -> GradientClipping); the step applies decay, the clip rate min(1, clip/sqrt(sqnorm)) and
 * AMSGrad-Adam with lr_t = alpha*sqrt(1-b2^t)/(1-b1^t) computed by the caller; beta1 / beta2 are doubles because the kernel multiplies with
 * float32(1 - beta), the subtraction done in double (as a float, 0.999 has a complement 1.3e-5 off 0.001).  Both update kernels leave p (and the moments)
 * untouched while the persistent kernels' sticky status word is non-zero (a kernel of the step timed out: the gradients are
 * garbage, and the host only learns of it when it reads the loss back).  The word stays set until astk_persist_status(.., reset = 1):
 * a caller must read the status next to the loss at least once per step (the Python shim's loss.data / float(loss) do, and raise) --
 * one that never looks would silently drop every later update while its own step counter advances. */
int astk_grad_sqnorm(const float* g, const float* p, float l2, size_t n, double* sqnorm, void* stream);
int astk_decay_clip_amsgrad_step(float* p, const float* g, float* m, float* v, float* vhat, size_t n,
                                 float l2, float clip, const double* sqnorm, float lr_t, double beta1, double beta2,
                                 float eps, int amsgrad, void* stream);
int astk_decay_clip_sgd_step(float* p, const float* g, size_t n, float l2, float clip, const double* sqnorm,
                             float lr, void* stream);
/* The same three with the gradient read as grad_scale * g: under data parallelism g holds the SUM over the replicas after the
 * all-reduce and grad_scale = 1/world makes it the mean without a separate pass over the buffer (the product is rounded before
 * the decay term is added, exactly as a separate scaling pass would round it). */
int astk_grad_sqnorm_scaled(const float* g, const float* p, float grad_scale, float l2, size_t n, double* sqnorm, void* stream);
int astk_decay_clip_amsgrad_step_scaled(float* p, const float* g, float* m, float* v, float* vhat, size_t n, float grad_scale,
                                        float l2, float clip, const double* sqnorm, float lr_t, double beta1, double beta2,
                                        float eps, int amsgrad, void* stream);
int astk_decay_clip_sgd_step_scaled(float* p, const float* g, size_t n, float grad_scale, float l2, float clip,
                                    const double* sqnorm, float lr, void* stream);

/* ---------------------------------------------------------------- utilities
 * Dropout keep-masks (Chainer-sem A5): out[i] = (u_i >= ratio) / (1-ratio), u from a counter-based hash RNG. */
int astk_fill_dropout_mask(float* out, size_t n, float ratio, uint64_t seed, uint64_t offset, void* stream);
/* chainer.optimizer.GradientNoise behind the other two hooks (nn.py:108-110; hooks run in insertion order WeightDecay -> GradientClipping ->
 * GradientNoise, Chainer-sem A7): g <- clip(g * grad_scale + l2 * p) + sigma * N(0,1) in place, sigma^2 = eta / (1 + t)^0.55 (t = updates done before this one; the caller passes sigma).  The update
 * call that follows takes the finished gradient (grad_scale 1, l2 0, clip off).  Chainer draws from its unseeded global RNG (quirk Q7);
 * this is a counter-based stream (seed, offset) consuming n / 2 counters. */
int astk_decay_clip_noise(float* g, const float* p, size_t n, float grad_scale, float l2, float clip, const double* sqnorm, float sigma,
                          uint64_t seed, uint64_t offset, void* stream);
/* out[i] = 1 + sigma*N(0,1): the multiplicative speech noise of seq2seq.py:300-302, generated on device. */
int astk_fill_normal(float* out, size_t n, float mean, float sigma, uint64_t seed, uint64_t offset, void* stream);
/* Several fills of those two kinds in ONE launch (a train step's speech noise and dropout masks): every element gets exactly the value
 * astk_fill_normal / astk_fill_dropout_mask give it for the same (seed, offset).  kind ASTK_RAND_DROPOUT: a = ratio; ASTK_RAND_NORMAL:
 * a = mean, b = sigma.  Replaces the host-side np.random.normal of seq2seq.py:300 and Chainer's per-call F.dropout masks (A5). */
#define ASTK_RAND_SEG_MAX 8
#define ASTK_RAND_DROPOUT 0
#define ASTK_RAND_NORMAL 1
typedef struct {
  float* out;
  size_t n;
  int kind;
  float a, b;
  uint64_t seed, offset;
} astk_rand_seg;
int astk_fill_random(const astk_rand_seg* segs, int n_segs, void* stream);
/* ... and, in the same launch, n_words (<= ASTK_RAND_WORDS_MAX) HOST values written to the device array words_dst: the step's
 * teacher-forcing flags (seq2seq.py:431-436 draws them on the host) travel in the kernel arguments instead of a copy of their own.
 * n_segs may be 0. */
#define ASTK_RAND_WORDS_MAX 256
int astk_fill_random_ex(const astk_rand_seg* segs, int n_segs, const int32_t* words, int n_words, int32_t* words_dst, void* stream);
int astk_scale_f32(float* x, size_t n, float s, void* stream);
/* dst += src (n floats); dst[c] += sum_r src[r*lds + c] (bias gradients; the sum over time of the linear_proj encoder's reverse-stack
 * input gradient, whose input is one frame fed at every step).  The column sum loads 16-byte quads: src must be 16-byte aligned and
 * lds a multiple of 4 (the columns behind cols inside the last quad are read, never summed); any other layout is refused. */
int astk_add_f32(float* dst, const float* src, size_t n, void* stream);
int astk_colsum_add_f32(float* dst, const float* src, long lds, int rows, int cols, void* stream);
/* init_decoder_state (seq2seq.py:318-333) and its backward as ONE launch each: decoder layer k < n starts from [fwd_k ; rev_k] of the
 * encoder's final states.  enc_c / enc_h: (nd, nl_enc, B, h) as astk_lstm_stack_fwd leaves them; dec_c / dec_h: (>= n, B, nd*h).
 * to_decoder != 0: dec[k][b][d*h + u] = enc[d][k][b][u]; to_decoder == 0 (gradients): enc[d][k][b][u] = dec[k][b][d*h + u].
 * Layers >= n of either side are not touched. */
int astk_bridge_states(float* dec_c, float* dec_h, float* enc_c, float* enc_h, int nd, int nl_enc, int n, int B, int h, int to_decoder,
                       void* stream);
/* Frame zeroing of the training loader (dataloader.py:83-93, `zero_input`), on the padded device batch X (B,T,D): utterance b of true
 * length lengths[b] gets int(rate * lengths[b]) frames zeroed, drawn with replacement from [0, lengths[b]) like
 * np.random.choice(np.arange(T_b), size=n).  The reference's draw is unseeded (quirk Q7); this one is a counter-based stream
 * (seed, offset), consuming B*T counters per call. */
int astk_zero_frames(float* X, int B, int T, int D, const int32_t* lengths, double rate, uint64_t seed, uint64_t offset, void* stream);
/* The draws astk_zero_frames makes for the same (lengths, rate, seed, offset), written out instead of applied: counts[b] =
 * int(rate * lengths[b]) (double precision, as Python evaluates it), idx[b*max_draws + i] = the i-th frame drawn for utterance b.
 * Lets a test feed the device's stream to the oracle's _drop_frames (oracle/loader_ref.py) and compare whole batches bit for bit. */
int astk_zero_frames_draws(int B, int T, const int32_t* lengths, double rate, uint64_t seed, uint64_t offset, int32_t* idx, int max_draws,
                           int32_t* counts, void* stream);
/* SpecAugment of the training loader: contiguous frequency and time masks on the padded device batch X (B,T,D),
 * in place, one launch, stream-ordered, no allocation, no synchronisation.  Not in the reference: off unless a caller asks for it.
 * The masks are a contract, a pure function of (seed, presentation counter n of the utterance, D, len) that a host can restate
 * (ast_amd.spec_augment.spec_spans).  All integer arithmetic is uint64; mix64 is the splitmix64 finaliser quoted with the sampled
 * decode's noise contract above (Python: ast_amd.seq2seq.mix64).
 *   key(seed, n)      = mix64(seed ^ mix64(n))                      n = counter0 + b * counter_stride for row b of the call
 *   word(key,c,i,r)   = mix64(key ^ ((c << 32) | (i << 1) | r))     c: 0 frequency, 1 time; i: mask index; r: 0 width, 1 start
 *   frequency mask i  : cap = min(freq_width, D);  f = (word(key,0,i,0) >> 11) % (cap + 1);  f0 = (word(key,0,i,1) >> 11) % (D - f + 1)
 *                       masks bins [f0, f0 + f) of frames [0, len)
 *   time mask i       : cap = min(time_width, int(time_ratio * len)), the product in double, as Python evaluates it
 *                       t = (word(key,1,i,0) >> 11) % (cap + 1);  t0 = (word(key,1,i,1) >> 11) % (len - t + 1)
 *                       masks frames [t0, t0 + t), all D bins
 * len = lengths[b] clamped to [0, T]; a row with len == 0 is left alone, and the frames at and behind len (the padding) are never
 * written.  A width of 0 is a legal draw; an utterance may end up fully masked (freq_width >= D): that is the definition.  The modulo
 * of a 53-bit word over at most a few thousand values is biased by about 1e-12.  (key(2024, 0) = row_key(2024, 0) =
 * 0xEE8C6C05E85E6BD6; with D = 80, len = 800, two masks of each kind, freq_width 15, time_width 40, time_ratio 0.2 the (start, width)
 * spans of n = 0 are frequency (56,10) (51,11), time (680,34) (211,9).)
 * fill = ASTK_SPEC_FILL_ZERO: masked cells become +0.0f; X is not read.
 * fill = ASTK_SPEC_FILL_MEAN: a masked cell of bin d becomes the float32 mean over frames [0, len) of X[b, t, d] AS IT IS ON ENTRY to
 *   the call, before any mask of this call: overlapping masks are order-free, every masked cell of bin d of a row holds the same value.
 *   The sum is float32 in a fixed order that depends on (len, D) alone -- not on B, T or the row's position -- and is divided by
 *   (float)len: the same call twice gives the same bits, and so does the same utterance in another batch.
 * An utterance's masks depend on (seed, n, D, len) alone.  The loader gives row b of rank r the utterance's position in the epoch's
 * unsharded plan (counter0 = base + r, counter_stride = world size), so they do not depend on B, T, the shard or the world size.
 * Fails with a message that names the field, and launches nothing, for: a null X, lengths or descriptor; a wrong struct_size; B, T < 1
 * or D outside 1..ASTK_SPEC_MAX_BINS; n_freq or n_time outside 0..ASTK_SPEC_MAX_MASKS; a negative freq_width or time_width; a
 * time_ratio outside [0, 1] or not finite; an unknown fill.  With n_freq == n_time == 0 it returns 0 and launches nothing. */
#define ASTK_SPEC_FILL_ZERO 0
#define ASTK_SPEC_FILL_MEAN 1
#define ASTK_SPEC_MAX_MASKS 8
#define ASTK_SPEC_MAX_BINS 1024
typedef struct {
  uint32_t struct_size;  /* = sizeof(astk_spec_augment_desc) */
  int n_freq, freq_width, n_time, time_width;
  double time_ratio;
  int fill;
} astk_spec_augment_desc;
int astk_spec_augment(float* X, int B, int T, int D, const int32_t* lengths, const astk_spec_augment_desc* d, uint64_t seed,
                      uint64_t counter0, uint64_t counter_stride, void* stream);
/* ---------------------------------------------------------------- CTC loss on the encoder states
 * Joint CTC-attention training: standard CTC over logits (B, T, V) with row stride ldv >= V, the given blank id, float32 in the log
 * domain.  Not in the reference: off unless a caller asks for it.
 *   labels of row b     the entries of y[b][0 .. L) (int32, row stride ldy) with id >= first_label, in order (ids >= V are read as V - 1);
 *                       U of them, the extended sequence has S' = 2U + 1 states; U = 0 is allowed (only the all-blank path remains)
 *   input_len           (B) valid frames per row, clamped to [0, T]; NULL = T for every row
 *   row_nll[b]          -log p(labels_b | logits_b[0 : input_len[b]])
 *   dlogits             scale * d(sum of the feasible rows' nll) / d logits = scale * (softmax - posterior occupancy); every valid frame's
 *                       gradient sums to zero over v; frames at t >= input_len[b] and the columns V .. ldv of every frame are set to 0.
 *                       May alias logits.
 *   infeasible rows     input_len[b] < U + (number of adjacent equal labels): row_nll = +inf, nothing added to loss_acc, dlogits all
 *                       zero, counted in *n_infeasible (NULL or one int32, overwritten)
 *   loss_acc            NULL or one float: += scale * sum of the feasible rows' nll, by one thread in row order, in stream order behind
 *                       whatever wrote it before
 * No floating-point atomics: row_nll, loss_acc and dlogits are bit-identical from run to run.  Four launches, no allocation, no
 * synchronisation; ws of astk_ctc_workspace_bytes (16-byte aligned; alpha and the gathered emissions, 2 T (2L + 1) floats per row).
 * Refused from the descriptor alone, before any launch, with a message: a wrong struct_size; B, T, L < 1; V < 2; ldv < V; ldy < L; a
 * blank outside [0, V); first_label <= blank; L > ASTK_CTC_MAX_LABELS (a row holds at most L labels, and the rows' label counts are
 * device data: the bound on L is what keeps every U within ASTK_CTC_MAX_LABELS; the shipped max_pred is 175).
 * astk_ctc_greedy: best[b][t] = the argmax class of frame t (ties: the lowest index) for t < input_len[b], the blank behind it.
 * astk_ctc_head_fwd: the linear head, logits (rows, V; row stride ldv) = enc (rows, H) W^T + b, as ONE product under the forward ops'
 *   two-contributor rule (bit-identical from run to run) and the given arithmetic; astk_gemm_f32_ex otherwise.
 * astk_ctc_head_bwd: its backward under one arithmetic / deterministic setting, three launches:
 *   d_enc (rows, H) += dlogits W;  dW (V, H) += dlogits^T enc;  db (V) += column sums of dlogits.   (rows = B T; ldv, H multiples of 4) */
#define ASTK_CTC_MAX_LABELS 255
typedef struct {
  size_t struct_size;   /* = sizeof(astk_ctc_desc) */
  int B, T, V;
  long ldv;
  int L;
  long ldy;
  int first_label;
  int blank;
} astk_ctc_desc;
size_t astk_ctc_workspace_bytes(const astk_ctc_desc* d);      /* 0 for a descriptor the calls refuse (astk_last_error) */
int astk_ctc_loss(const astk_ctc_desc* d, const float* logits, const int32_t* y, const int32_t* input_len, float scale, float* row_nll,
                  float* loss_acc, float* dlogits, int32_t* n_infeasible, void* ws, size_t ws_bytes, void* stream);
int astk_ctc_greedy(const astk_ctc_desc* d, const float* logits, const int32_t* input_len, int32_t* best, void* stream);
int astk_ctc_head_fwd(int rows, int V, int H, const float* enc, const float* W, const float* b, float* logits, long ldv, int precision,
                      void* stream);
int astk_ctc_head_bwd(int rows, int V, int H, const float* dlogits, long ldv, const float* W, const float* enc, float* d_enc, float* dW,
                      float* db, int precision, int deterministic, void* stream);
/* ---------------------------------------------------------------- CTC forced alignment
 * The best monotonic path (Viterbi) of a row's labels through its frames, over the logits of the section-28 head.  Rows, labels, the
 * extended sequence z (S' = 2U + 1 states, blanks at the even positions), input_len (clamped to [0, T], NULL = T; n below) and L are
 * astk_ctc_loss's, through the same descriptor.  Float32:
 *   e[t][s]        = logits[t][z_s] - lse[t], lse the per-frame log-sum-exp with the maximum subtracted
 *   delta[0][0]    = e[0][0], delta[0][1] = e[0][1], the rest -inf
 *   delta[t][s]    = e[t][s] + max(delta[t-1][s], delta[t-1][s-1], [skip] delta[t-1][s-2]);  [skip]: z_s is a label and z_s != z_{s-2}
 *   tie rule       a predecessor replaces the current choice only if it is STRICTLY greater, tried in the order stay (s), s - 1, s - 2;
 *                  the final state is S' - 1 (the trailing blank) unless delta[n-1][S'-2] is strictly greater;
 *                  max(-inf, -inf) + e = -inf, never NaN
 *   frame_state    int32 (B, T): the state s of frame t on the best path for t < n, -1 behind n
 *   frame_class    int32 (B, T) or NULL: z_s of that state (the blank id on blank states), the blank behind n
 *   label_start /  int32 (B, L) or NULL: the frames [start, end) the path spends in label u's state 2u + 1; -1 for u >= U
 *   label_end
 *   label_logp     float32 (B, L) or NULL: the sum of e[t][2u+1] over those frames, in frame order; 0 for u >= U
 *   row_score      float32 (B): delta[n-1][final state], the best path's log-probability (0 for n = 0 and U = 0: the empty path)
 *   a row without a path (n < U + the number of adjacent equal labels): row_score = -inf, frame_state all -1, frame_class all blank,
 *                  spans -1, label_logp 0; such rows are counted in *n_infeasible (int32, or NULL)
 * logits is only read.  No atomics behind any output: bit-identical from run to run.  Two launches (three with n_infeasible), no
 * allocation, no synchronisation; ws of astk_ctc_align_workspace_bytes (16-byte aligned: the lse and 2 bits of back-pointer per frame and
 * state, T * ceil((2L + 1) / 64) * 16 bytes per row).  Refused before any launch: what astk_ctc_loss refuses from the descriptor, a
 * NULL logits / y / frame_state / row_score / ws, and a workspace below the query (which returns 0 for a refused descriptor). */
size_t astk_ctc_align_workspace_bytes(const astk_ctc_desc* d);
int astk_ctc_align(const astk_ctc_desc* d, const float* logits, const int32_t* y, const int32_t* input_len, int32_t* frame_state,
                   int32_t* frame_class, int32_t* label_start, int32_t* label_end, float* label_logp, float* row_score,
                   int32_t* n_infeasible, void* ws, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- CTC prefix beam search
 * N-best label strings from the head's logits alone (Hannun et al. 2014): the N most probable label prefixes are kept frame by frame,
 * all alignments of one prefix merged.  logits (B, T, ldv) float32, input_len clamped to [0, T] (NULL = T; n below); labels are the ids
 * >= first_label.  Float64 in the log domain; x[t][c] = logits[t][c] - lse[t], lse the float64 log-sum-exp over all V classes with the
 * maximum subtracted; logaddexp(-inf, -inf) = -inf, never NaN.
 *   proposals   per frame the C labels with the largest x[t][c]: higher first, equal ones lower id first; the same for every prefix
 *   state       at most N distinct prefixes with p_b, p_nb = the log-probability of their alignments over the frames 0..t that end in
 *               a blank / a non-blank; before frame 0 the empty prefix with p_b = 0, p_nb = -inf
 *   frame step  tot = logaddexp(p_b, p_nb); a prefix l with last label e gives
 *                 stay l:      p_b' = tot + x[t][blank], p_nb' = p_nb + x[t][e] (-inf for the empty prefix)
 *                 extend l.c:  for every proposal c, if l has fewer than max_labels labels: p_b' = -inf,
 *                              p_nb' = (c == e ? p_b : tot) + x[t][c]
 *               an extension that spells another member l' of the beam (exact equality of the label strings) is no candidate of its
 *               own: its p_nb' is added (logaddexp) to the stay candidate of l'
 *   selection   the N candidates with the largest logaddexp(p_b', p_nb'), none at -inf; equal scores: stay candidates before
 *               extensions, then the lower source slot, then the earlier proposal; the slots are in rank order after every frame
 *   tokens      int32 (B, N, max_labels): the labels of slot r, the blank id behind them and in unused slots
 *   n_labels    int32 (B, N): their count, -1 for an unused slot
 *   score       float64 (B, N): logaddexp(p_b, p_nb) after the row's n frames, -inf for an unused slot: a lower bound of
 *               log p_ctc(labels), equal to it where nothing was pruned.  n = 0: the empty string with score 0 in slot 0.
 * logits is only read.  No atomics: bit-identical from run to run.  Two launches, no allocation, no synchronisation; ws of
 * astk_ctc_beam_workspace_bytes (16-byte aligned: per frame the lse, the blank's and the proposals' log-probabilities and ids, per row a
 * trie of the prefixes as a hash table of 2^k >= 2 (T N + 1) 8-byte entries).  Refused before any launch: a wrong struct_size; B, T < 1;
 * T > ASTK_BEAM_CTC_MAX_T; V <= first_label; ldv < V; blank outside [0, V) or >= first_label; N or C outside 1..16; C > V - first_label;
 * max_labels outside 1..ASTK_CTC_MAX_LABELS; a NULL logits / tokens / n_labels / score / ws; a workspace below the query (which returns
 * 0 for a refused descriptor). */
typedef struct {
  size_t struct_size;   /* = sizeof(astk_ctc_beam_desc) */
  int B, T, V;
  long ldv;             /* row stride of logits, >= V */
  int N;                /* beam width */
  int C;                /* labels proposed per frame */
  int max_labels;       /* no prefix grows beyond it; the stride of tokens */
  int first_label;
  int blank;
} astk_ctc_beam_desc;
size_t astk_ctc_beam_workspace_bytes(const astk_ctc_beam_desc* d);
int astk_ctc_beam(const astk_ctc_beam_desc* d, const float* logits, const int32_t* input_len, int32_t* tokens, int32_t* n_labels,
                  double* score, void* ws, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- pair statistics of token strings
 * What minimum-Bayes-risk selection and error rates need of an n-best list, as integers: for every pair (a, b) = (hypothesis,
 * reference) of a pool of token strings the Levenshtein statistics and the clipped n-gram matches of BLEU.
 *   tokens  int32 (S, Lmax): the pool; any int32 value is an id; what lies behind a string's length is never read
 *   lens    int32 (S): each in 0..Lmax
 *   pairs   int32 (P, 2): rows (a, b) of indices into the pool; a == b and repeated rows are allowed
 *   stats   int32 (P, 8) = [dist, sub, del, ins, m1, m2, m3, m4]
 *   n_bad   int32, may be NULL: the number of bad rows
 * Edit statistics: D[0][0] = (0, 0, 0, 0) substitutions, deletions, insertions; D[i][0] = i insertions, D[0][j] = j deletions; for
 * i, j >= 1 the candidates are, in this order,
 *     diagonal   D[i-1][j-1], + 1 sub when a[i-1] != b[j-1]
 *     deletion   D[i][j-1] + 1 del (the reference token b[j-1] stays unmatched)
 *     insertion  D[i-1][j] + 1 ins
 * and the cell takes the one of least cost sub + del + ins, the earlier one among equals, with that candidate's three counts.  The
 * output is D[La][Lb]: dist = sub + del + ins is the Levenshtein distance, del - ins = Lb - La, and the forward rule makes the three
 * counts well defined without a back-pointer matrix.
 * Clipped matches: m_n = sum over the distinct n-grams g of min(count_a(g), count_b(g)), n = 1..4; 0 when either string has fewer
 * than n tokens; symmetric in (a, b) -- the numerator of BLEU's n-gram precision with one reference.
 * A row is bad when an index lies outside [0, S) or a named length outside [0, Lmax]: it gets eight -1, reads nothing out of bounds
 * and is counted in *n_bad.
 * tokens, lens and pairs are only read.  Integers throughout and no atomics: bit-identical from run to run, equal to a host model.
 * One launch (two with n_bad), no allocation, no synchronisation, no workspace.  Refused before any launch: a wrong struct_size;
 * S < 1; P < 1; Lmax outside 1..ASTK_PAIR_MAX_LEN; a NULL tokens / lens / pairs / stats. */
#define ASTK_PAIR_MAX_LEN 512
typedef struct {
  size_t struct_size;   /* = sizeof(astk_pair_stats_desc) */
  int S;                /* strings in the pool */
  int Lmax;             /* row stride of tokens, the longest string admitted */
  int P;                /* pairs */
} astk_pair_stats_desc;
int astk_pair_stats(const astk_pair_stats_desc* d, const int32_t* tokens, const int32_t* lens, const int32_t* pairs, int32_t* stats,
                    int32_t* n_bad, void* stream);
/* ---------------------------------------------------------------- risk weights for minimum-risk training
 * Turns the integers of astk_pair_stats and the candidates' sequence log-probabilities into the per-row weights of astk_decoder_fwd_w
 * under which the weighted cross-entropy's gradient is the gradient of the expected cost of each list (utterance):
 *     Q_i = exp(alpha (s_i - s_max)) / sum_j ..   Rbar = sum_i Q_i c_i   weight_i = risk_scale alpha Q_i (Rbar - c_i) + [flag bit 1] ref_weight
 * over the live rows of the list, in float64, each output rounded once to float32.
 *   first     int32 (U+1): row offsets of the lists, ascending, first[U] == R
 *   score     (R) sequence log-probabilities s_i
 *   stats     int32 (R, 8) of astk_pair_stats: row i is pair i of that call
 *   lens, pairs  the arrays that call read: hyp_len = lens[pairs[i][0]], ref_len = lens[pairs[i][1]]
 *   flags     int32 (R): bit 0 live (in the candidate set), bit 1 reference row
 *   weight    (R);  risk (U) the expected cost Rbar, may be NULL;  cost_out (R) c_i, may be NULL;  n_bad int32, may be NULL: bad lists
 * Cost: ASTK_RISK_COST_BLEU c = 1 - BLEU from (m1..m4, hyp_len, ref_len) -- method-2 smoothing ((m+1)/(t+1) for n >= 2), denominators
 * max(1, hyp_len - n + 1), the brevity penalty exp(1 - ref_len / hyp_len) (0 for an empty hypothesis), 0 when a match count is 0;
 * ASTK_RISK_COST_EDIT c = dist / max(1, ref_len).  A row is dead when bit 0 of its flag is clear or its stats row is the all -1 bad row:
 * Q = 0, cost_out = 0, only the reference term in its weight.  A list without live rows has risk 0.  A list is bad when it has more
 * than ASTK_RISK_MAX_LIST rows or its offsets do not ascend within [0, R] -- 0 <= first[u-1] <= first[u] <= first[u+1] <= R, so the
 * list behind a descent is bad too (it would share rows with an earlier one): its weights (its rows inside [0, R) and behind
 * first[u-1]), their cost_out and its risk are 0, nothing is read out of bounds, and it is counted in *n_bad.  score and flags must be finite / as described: they are not checked.
 * One wavefront per list, a lane per row, the three reductions as fixed-order shuffle trees: bit-identical from run to run.  One launch
 * (two with n_bad), no allocation, no synchronisation, no workspace, no atomics.  Refused before any launch: a wrong struct_size; U or
 * R < 1; cost outside {0, 1}; alpha negative or not finite; risk_scale or ref_weight not finite; a NULL first / score / stats / lens /
 * pairs / flags / weight. */
#define ASTK_RISK_MAX_LIST 64
enum { ASTK_RISK_COST_BLEU = 0, ASTK_RISK_COST_EDIT = 1 };
typedef struct {
  size_t struct_size;   /* = sizeof(astk_risk_desc) */
  int U;                /* lists (utterances) */
  int R;                /* rows = candidates over all lists */
  int cost;             /* ASTK_RISK_COST_* */
  float alpha;          /* sharpness of Q, finite, >= 0 */
  float risk_scale;     /* factor on the risk term, finite */
  float ref_weight;     /* added to the weight of a row whose flag has bit 1 set, finite */
} astk_risk_desc;
int astk_risk_weights(const astk_risk_desc* d, const int32_t* first, const float* score, const int32_t* stats, const int32_t* lens,
                      const int32_t* pairs, const int32_t* flags, float* weight, float* risk, float* cost_out, int32_t* n_bad,
                      void* stream);
/* ---------------------------------------------------------------- speech features from waveforms, and CMVN
 * MFCC / log mel filterbank features in the sense of Kaldi's compute-mfcc-feats / compute-fbank-feats (snip-edges=true only), written
 * from Kaldi's documented algorithm and option names; parity with Kaldi's binaries is NOT pinned (no Kaldi output exists to pin it
 * to): the contract is the float64 restatement tests/speech_features_model.py.
 *   wave       (B, Nmax) float32 or int16 (sample_type); sample values are used as they are (Kaldi's 16-bit scale, no division)
 *   n_samples  int32 (B); nothing behind a row's length is read
 *   feats      float32 (B, Fmax, D); D = num_mel_bins (fbank) or num_ceps (mfcc); frames t >= F_b are written as zeros
 *   n_frames   int32 (B): F_b, or -1 for a bad row
 *   n_bad      int32, may be NULL: the number of bad rows
 * Frames: F_b = 0 if n_b < frame_len, else 1 + (n_b - frame_len) / frame_shift (integer division); frame t covers the samples
 * t * frame_shift .. + frame_len.  N = the next power of two at or above frame_len.  Per frame, in this order:
 *   1. dither (dither != 0): x[n] += dither * z(seed, offset_b + n); z(seed, g) is element g of the unit-normal stream of
 *      astk_fill_normal at offset 0 (pair g >> 1: b = mix64(seed ^ mix64(g >> 1)), u1 / u2 = ((low / high half >> 8) + 1) 2^-24,
 *      sqrt(-2 ln u1) cos(2 pi u2) for even g, .. sin .. for odd g), evaluated in float64.  A function of the SAMPLE index: a sample
 *      carries the same dither in every frame that contains it (Kaldi draws per extracted frame).  offset_b = offsets[b], 0 if NULL.
 *   2. remove_dc_offset: subtract the frame's mean
 *   3. use_energy: raw log energy log(max(sum x^2, eps)) of the frame at this point; eps = 2^-23
 *   4. pre-emphasis: x[i] -= c x[i-1] for i = frame_len-1 .. 1, then x[0] -= c x[0]
 *   5. window: povey (0.5 - 0.5 cos(2 pi i / (frame_len - 1)))^0.85, hamming 0.54 - 0.46 cos(..), hanning 0.5 - 0.5 cos(..), rectangular
 *   6. zero-pad to N, real FFT, power spectrum |X_k|^2
 *   7. mel filterbank: mel(f) = 1127 ln(1 + f / 700); num_mel_bins triangles equally spaced in mel between low_freq and the resolved
 *      high_freq (high_freq <= 0: Nyquist + high_freq); with delta = (mel_high - mel_low) / (num_mel_bins + 1), filter j has left =
 *      mel_low + j delta, center = mel_low + (j + 1) delta, right = mel_low + (j + 2) delta.  FFT bin i in 0 .. N/2 - 1 lies at f = i sr / N and contributes to
 *      filter j when left < mel(f) < right, with weight (mel - left) / (center - left) when mel <= center, else (right - mel) /
 *      (right - center).  E_j = sum_i w_ji |X_i|^2 (ascending i); L_j = log(E_j) when E_j > eps, else log(eps).
 *   8. fbank: the row is L.  mfcc: c_k = sum_j (lift_k dct[k][j]) L_j (ascending j, each product rounded, then added), dct[0][j] =
 *      sqrt(1/M), dct[k][j] = sqrt(2/M) cos(pi/M (j + 0.5) k), lift_k = 1 + 0.5 Q sin(pi k / Q), Q = cepstral_lifter (0: no lifter);
 *      with use_energy c_0 is the raw log energy of step 3.
 * Float64 from step 1 to the last sum, rounded once to float32.  No atomics: two runs give identical bytes.
 * A bad row -- n_samples outside [0, Nmax], or F_b > Fmax -- gets n_frames = -1 and all-zero feature rows, reads nothing out of bounds
 * and is counted in *n_bad.
 *   astk_speech_features_workspace_bytes  bytes of the table workspace (0 for a refused descriptor)
 *   astk_speech_features_prepare          one small launch that fills the tables (window, twiddles, the filters' bin ranges and
 *                                         weights, lift * dct) on the device in float64 and a digest of the descriptor's table fields
 *                                         (sample_frequency, frame_len, window, num_mel_bins, num_ceps, low_freq, high_freq,
 *                                         cepstral_lifter, kind) in the workspace head.  B, Nmax, Fmax, sample_type, frame_shift and
 *                                         the per-frame options may differ between prepare and the calls that use the workspace.
 *   astk_speech_features                  one launch (two with n_bad)
 * All three only enqueue: no allocation, no copy, no synchronisation.  The library remembers the digest of every workspace address it
 * prepared (host side) and the kernel compares the digest in the workspace head again: a workspace that was overwritten since makes
 * every row a bad row.
 * Refused before any launch: a wrong struct_size; B, Nmax or Fmax < 1; frame_len outside 2..2048; frame_shift < 1; num_mel_bins
 * outside 3..128; num_ceps outside 1..num_mel_bins (mfcc); low_freq < 0, or a resolved high_freq at or below low_freq or above Nyquist;
 * an unknown kind / window / sample type; use_energy with fbank; NULL buffers; a workspace that is too small, was never prepared, or
 * was prepared for another descriptor. */
#define ASTK_FEAT_MFCC 0
#define ASTK_FEAT_FBANK 1
#define ASTK_FEAT_WINDOW_POVEY 0
#define ASTK_FEAT_WINDOW_HAMMING 1
#define ASTK_FEAT_WINDOW_HANNING 2
#define ASTK_FEAT_WINDOW_RECTANGULAR 3
#define ASTK_FEAT_SAMPLE_F32 0
#define ASTK_FEAT_SAMPLE_I16 1
#define ASTK_FEAT_MAX_FRAME_LEN 2048
#define ASTK_FEAT_MAX_MEL_BINS 128
typedef struct {
  size_t struct_size;      /* = sizeof(astk_speech_features_desc) */
  int B;                   /* rows of the batch */
  int Nmax;                /* row stride of wave, the longest waveform admitted */
  int Fmax;                /* frames per row of feats */
  int sample_type;         /* ASTK_FEAT_SAMPLE_* */
  int kind;                /* ASTK_FEAT_MFCC / ASTK_FEAT_FBANK */
  int window;              /* ASTK_FEAT_WINDOW_* */
  int frame_len;           /* samples */
  int frame_shift;         /* samples */
  int num_mel_bins;
  int num_ceps;            /* mfcc only */
  int remove_dc_offset;
  int use_energy;          /* mfcc only */
  double sample_frequency;
  double low_freq;
  double high_freq;
  double preemphasis;
  double cepstral_lifter;
  double dither;
  uint64_t seed;
  const int64_t* offsets;  /* device (B) dither stream offsets, or NULL for zeros */
} astk_speech_features_desc;
size_t astk_speech_features_workspace_bytes(const astk_speech_features_desc* d);
int astk_speech_features_prepare(const astk_speech_features_desc* d, void* ws, size_t ws_bytes, void* stream);
int astk_speech_features(const astk_speech_features_desc* d, const void* wave, const int32_t* n_samples, float* feats, int32_t* n_frames,
                         int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);
/* Cepstral mean and variance normalisation of float32 feature batches (B, Fmax, D) -- from astk_speech_features or from files.
 *   astk_cmvn_accumulate  adds the frames t < min(n_frames[b], Fmax) of the rows with n_frames[b] >= 0 to the float64 statistics
 *                         stats (G, 2, D + 1) of group[b], Kaldi's layout: [g][0][:D] sums, [g][0][D] the frame count, [g][1][:D] sums
 *                         of squares, [g][1][D] stays 0.  It ADDS to what is there (zero the buffer first; a speaker's statistics
 *                         may span calls).  A group id outside [0, G) skips the row and counts it in *n_bad (may be NULL).  No atomics,
 *                         a fixed summation order: two runs give identical bytes.
 *   astk_cmvn_apply       y = (x - mean_g) * s_g on the same frames, in place (feats_out == feats_in) or out of place; mean = sum /
 *                         count; s = 1 without norm_vars, else 1 / sqrt(max(sumsq / count - mean^2, 1e-20)); float64 arithmetic on
 *                         the float32 input, rounded once.  Rows of a group with count 0 or an id outside [0, G), rows with n_frames
 *                         < 0 and the frames at or behind n_frames[b] come out as they went in.
 * One launch each (two with n_bad).  Refused before any launch: a wrong struct_size; B, Fmax, D or G < 1; NULL buffers. */
typedef struct {
  size_t struct_size;      /* = sizeof(astk_cmvn_desc) */
  int B, Fmax, D;
  int G;                   /* groups (speakers) */
  int norm_vars;
} astk_cmvn_desc;
int astk_cmvn_accumulate(const astk_cmvn_desc* d, const float* feats, const int32_t* n_frames, const int32_t* group, double* stats,
                         int32_t* n_bad, void* stream);
int astk_cmvn_apply(const astk_cmvn_desc* d, const float* feats_in, float* feats_out, const int32_t* n_frames, const int32_t* group,
                    const double* stats, void* stream);
/* ---------------------------------------------------------------- resampling and speed perturbation of waveforms
 * Band-limited resampling by a rational ratio, out_rate / in_rate = q / p, with a Hann-windowed sinc: the operator in front of
 * astk_speech_features for files of another rate, and -- read at the ORIGINAL rate -- a speed change by the factor p / q (0.9 is p = 9,
 * q = 10: a longer, lower, slower copy).  Parity with sox / Kaldi is NOT pinned (Kaldi perturbs speed with sox, which does not exist
 * here): the contract is the float64 model tests/resample_model.py.
 *   wave       (B, Nmax) float32 or int16 (sample_type, ASTK_FEAT_SAMPLE_*); nothing behind a row's length is read
 *   n_samples  int32 (B)
 *   out        float32 (B, Mmax), zero at m >= n_out[b]
 *   n_out      int32 (B): ceil(n_samples[b] q / p), or -1 for a bad row
 *   n_bad      int32, may be NULL: the number of bad rows
 * p and q are reduced by their gcd inside.  With Z = num_zeros, c = rolloff * min(1, q / p) and K = ceil(Z / c):
 *   g(t) = c sinc(c t) cos^2(pi c t / (2 Z)) for |c t| < Z, else 0;  sinc(u) = sin(pi u) / (pi u), 1 at u = 0
 *   y[m] = sum over k = -K+1 .. K of x[n0 + k] g(phi / q - k),  n0 = (m p) div q,  phi = (m p) mod q  (64-bit integers)
 * x is 0 outside [0, n_samples[b]).  The sum runs in ascending k in float64 and is rounded once to float32.  No atomics: two runs give
 * identical bytes.  A bad row -- n_samples outside [0, Nmax], or an output count above Mmax -- gets n_out = -1 and an all-zero row,
 * reads nothing out of bounds and is counted in *n_bad.  Inputs are never written.
 *   astk_resample_workspace_bytes  bytes of the table workspace (0 for a refused descriptor)
 *   astk_resample_prepare          one small launch that fills the polyphase table (reduced q phases x 2K taps, float64, stored
 *                                  [tap][phase]) on the device and a digest of the descriptor's table fields (reduced p and q,
 *                                  num_zeros, rolloff) in the workspace head.  B, Nmax, Mmax and sample_type may differ between
 *                                  prepare and the calls that use the workspace.
 *   astk_resample                  one launch (two with n_bad)
 * All three only enqueue.  The library remembers the digest of every workspace address it prepared (host side) and the kernel compares
 * the digest in the workspace head again: a workspace that was overwritten since makes every row a bad row.
 * Refused before any launch: a wrong struct_size; B, Nmax or Mmax < 1; p or q < 1; a reduced q above ASTK_RESAMPLE_MAX_PHASES; K above
 * ASTK_RESAMPLE_MAX_HALF_TAPS; num_zeros < 1; rolloff outside (0, 1]; an unknown sample type; NULL buffers; a workspace that is too
 * small, was never prepared, or was prepared for other table fields. */
#define ASTK_RESAMPLE_MAX_PHASES 1024
#define ASTK_RESAMPLE_MAX_HALF_TAPS 256
#define ASTK_RESAMPLE_TILE 256     /* output samples per workgroup: tile t of a row covers m = 256 t .. 256 t + 255 */
typedef struct {
  size_t struct_size;      /* = sizeof(astk_resample_desc) */
  int B;                   /* rows of the batch */
  int Nmax;                /* row stride of wave, the longest waveform admitted */
  int Mmax;                /* row stride of out, the longest output admitted */
  int sample_type;         /* ASTK_FEAT_SAMPLE_* */
  int p;                   /* out_rate / in_rate = q / p */
  int q;
  int num_zeros;           /* Z: zero crossings of the sinc on each side (6) */
  double rolloff;          /* cut-off as a fraction of the narrower Nyquist (0.99) */
} astk_resample_desc;
size_t astk_resample_workspace_bytes(const astk_resample_desc* d);
int astk_resample_prepare(const astk_resample_desc* d, void* ws, size_t ws_bytes, void* stream);
int astk_resample(const astk_resample_desc* d, const void* wave, const int32_t* n_samples, float* out, int32_t* n_out, int32_t* n_bad,
                  const void* ws, size_t ws_bytes, void* stream);
/* One wavefront that keeps `stream` busy for `usec` microseconds (<= 100 000) and then increments *flag (may be NULL).  For probing
 * whether two streams really execute concurrently: HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
 * default), and two streams that share one are serialised whatever their events say (ast_amd/seq2seq.py:_cu_streams). */
int astk_spin(unsigned usec, unsigned* flag, void* stream);

/* Persistent-kernel health.  The encoder / decoder recurrences run as single launches whose workgroups hand activations to each
 * other (lstm_persist.hip, decoder_persist.hip); that needs the whole grid resident (one workgroup per CU), which the launchers
 * check against the device's CU count but cannot guarantee against other tenants of the GPU (RCCL kernels under data
 * parallelism, another process).  Every spin is bounded: a time-out drains the grid and sets a bit in a STICKY status word
 * (1 encoder fwd, 2 encoder bwd, 4 decoder fwd, 8 decoder bwd, 16 a peer rank reported one of these: astk_persist_status_merge); the
 * results of such a step are garbage.
 *   astk_persist_status_snapshot  enqueues a copy of the word (as a float) to *dst on `stream`: the Python shim places it next to
 *                                 the loss scalar, so the loss read-back of nn.py:189 sees it without an extra synchronisation;
 *   astk_persist_status           synchronises the device, returns the word in *mask_out (may be NULL) and clears it if `reset`.
 * astk_set_tuning("persist.spin_limit", polls) shrinks the spin bound; tests use it to force a time-out. */
int astk_persist_status_snapshot(float* dst, void* stream);
/* Data parallelism: `summed` = the SUM over all ranks of the words astk_persist_status_snapshot wrote (the Python shim appends the
 * word to the last gradient range, so the gradient all-reduce carries it: ast_amd/dist.py).  Non-zero: some rank's step is garbage --
 * bit 16 is set in THIS rank's sticky word, so that the update kernels enqueued behind it skip on every rank alike and every rank
 * raises at its next loss read-back instead of waiting in the next collective for a peer that has already failed. */
int astk_persist_status_merge(const float* summed, void* stream);
/* Which path a shape takes on the current device (so that a silent fall-back shows up in logs / bench.py's JSON line):
 *   astk_lstm_stack_path  1 = persistent wavefront kernels (all T steps of all cells in one launch; stacks with more cells than CUs: one launch
 *                         per group of layers), 2 = the hoisted form of the same kernels (h = 1024: one launch per layer, the input projection
 *                         and the gradient for the layer below as batched products between the launches), 0 = one fused-cell launch per step
 *   astk_decoder_path     0 = per-launch decoder loop; otherwise bit 0 = persistent loop, bit 1 = attention phase specialised for
 *                         H = 512 / chunk <= 32, bit 2 = the batch runs as TWO persistent launches over halves of its rows (more than
 *                         32 rows at the shipped width: the decoder couples no batch rows, the halves share nothing but the weights
 *                         and the loss's 1/B), bit 4 (alone) = the wide decoder of configs[4] (H = A = 1024, E = 128, one layer, up to 32 rows,
 *                         T'' <= 256 at 32 rows) on decoder_wide.hip's persistent loops, one launch for the forward and one for the backward
 *                         (with bit 2: two of each, over halves of more than 32 rows); bits 8.. = number of decoder layers fused into the persistent kernels */
int astk_lstm_stack_path(const astk_lstm_stack_desc* d);
/* CUs the persistent recurrence launches of this shape leave FREE on the current device (0: not the persistent path, or none): what a
 * caller may pass as `side_wgs` for work it runs on a second stream beside the recurrences (astk_decoder_desc.side_wgs). */
int astk_lstm_stack_free_cus(const astk_lstm_stack_desc* d);
/* Which recurrence kernels astk_lstm_stack_fwd / _bwd would launch for this descriptor on the current device -- `precision` and `side_stream`
 * as the calls would see them, under the tuning table in force.  Read-only.  *rows: the workgroup form, 16 = one 16-row batch tile per
 * workgroup, 32 = two tiles against one set of weight fragments ("lstm.rows32" 1), 33 = two virtual 16-row workgroups in one of 512 threads
 * ("lstm.rows32" 2, bf16x3 only).  *xs: the arithmetic of the recurrences' products, 0 = f32 MFMAs, 2 = fp16x2, 3 = bf16x3 with all three
 * planes of the weights in registers, 4 = bf16x3 with the weights' lowest plane in LDS (h >= 512, and the form 33).  On the per-step path
 * (astk_lstm_stack_path 0) no recurrence kernel runs and the values say what one would be.  Either pointer may be NULL.  Returns 0, or -1 for
 * a bad descriptor (astk_last_error). */
int astk_lstm_stack_form(const astk_lstm_stack_desc* d, int* rows, int* xs);
/* What astk_lstm_stack_fwd / _bwd (with an input gradient) would run beside the recurrences for this descriptor -- `side_stream`, `side_wgs`,
 * `precision` and `deterministic` as the calls would see them -- on the current device, under the tuning table in force: the loop steps of the
 * layer-0 input projection multiplied in line (T: all of them), the chunks of it on the side stream, and the chunks of the input gradient on
 * the side stream behind the backward recurrence.  (0, 0 chunks: everything in line.)  Any output pointer may be NULL.  Returns 0, or -1 for
 * a bad descriptor (astk_last_error). */
int astk_lstm_stack_side_plan(const astk_lstm_stack_desc* d, int* fwd_head_steps, int* fwd_chunks, int* bwd_chunks);
int astk_decoder_path(const astk_decoder_desc* d);
int astk_persist_status(unsigned* mask_out, int reset);
int astk_device_cu_count(void);

#ifdef ASTK_TEST_HOOKS
/* Test hooks (libastk_test.so only): the row-panel launchers of rowgemm.hip -- the per-launch decoder loop, the eval-mode decoder step, the
 * beam search steps, the LayerNorm / projection variants, the per-step encoder loop -- which no other entry point exposes by themselves.
 * The structs mirror the library's internal argument structs field by field (the meaning of each: RowGemmArgs, LstmCellFwdArgs,
 * LstmCellBwdArgs in csrc/common.h); ZERO-INITIALISE, set struct_size, then the fields used.  Every call runs the real launcher on `stream`
 * and writes the route that launcher took to route[4]: route[0] bit 0 = two 16-row tiles per workgroup, bit 1 = eight waves per
 * workgroup; route[1..3] = the grid's x, y, z.  Returns 0, or nonzero with a message (nothing launched, route zeroed). */
typedef struct {
  const float* A;  /* [rows][K], row stride lda */
  long lda;
  const float* W;  /* [cols][K], row stride ldw */
  long ldw;
  int K;           /* multiple of 4; 0 = pair unused (A, W may be NULL then) */
} astk_debug_row_pair;
typedef struct {
  size_t struct_size;
  astk_debug_row_pair p[2];
  int npairs;           /* 1 or 2: out = sum_p A_p W_p^T */
  int M, N;
  const float* bias;    /* [N] or NULL */
  const float* addend;  /* [M][N], row stride ld_add, or NULL */
  long ld_add;
  float* out;
  long ld_out;
  float* out2;          /* optional second copy, row stride ld_out2 */
  long ld_out2;
  int act;              /* 0 none, 1 tanh */
  float* carry;         /* optional: for n >= carry_col0, j = n - carry_col0: carry[r][j] = (out[r][n] + carry[r][j]) * (1 - carry_aux[r][j]^2) */
  long ld_carry;
  const float* carry_aux;
  long ld_carry_aux;
  int carry_col0;
} astk_debug_rowgemm_args;
typedef struct {
  size_t struct_size;
  astk_debug_row_pair p[2];  /* W_p: [4h][K_p], gate rows interleaved 4j + k, k = a, i, f, o */
  int npairs;                /* 0..2 */
  int B, h;
  const float* zx;           /* [B][4h], row stride ld_zx, or NULL */
  long ld_zx;
  const float* bias;         /* [4h] or NULL */
  const float* c_prev;       /* [B][h] or NULL (zeros) */
  float* gates;              /* [B][4h], row stride ld_g: the activated gates (may alias zx) */
  long ld_g;
  float* c_out;              /* [B][h] */
  float* h_out;              /* [B][h] */
  const float* mask;         /* [B][h] or NULL: applied to the dropped outputs only */
  float* hd_out;             /* optional, row stride ld_hd */
  long ld_hd;
  float* hd_out2;            /* optional, row stride ld_hd2 */
  long ld_hd2;
} astk_debug_cell_fwd_args;
typedef struct {
  size_t struct_size;
  astk_debug_row_pair p[2];  /* p[0] -> dh_rec (unmasked); p[1] -> joins dy, dy2 under the mask; W_p: [h][K_p] */
  int npairs;                /* 1 or 2 (K of p[0] may be 0: the last step) */
  int B, h;
  const float* dh_add;       /* [B][h] or NULL, unmasked */
  const float* dy;           /* row stride ld_dy, or NULL */
  long ld_dy;
  const float* dy2;          /* row stride ld_dy2, or NULL */
  long ld_dy2;
  const float* mask;         /* [B][h] or NULL */
  const float* dc_next;      /* [B][h] or NULL */
  const float* c_prev;       /* [B][h] or NULL (zeros) */
  const float* c_cur;        /* [B][h] */
  float* gates_dz;           /* [B][4h], row stride ld_g: in the activated gates, out dz */
  long ld_g;
  float* dc_prev;            /* [B][h] */
} astk_debug_cell_bwd_args;
int astk_debug_rowgemm(const astk_debug_rowgemm_args* args, int* route, void* stream);
int astk_debug_lstm_cell_fwd(const astk_debug_cell_fwd_args* cells, int ncells, int* route, void* stream);
int astk_debug_lstm_cell_bwd(const astk_debug_cell_bwd_args* cells, int ncells, int* route, void* stream);
/* The CTC prefix scorer alone (ctc_prefix.hip) behind an init: for every LIVE row r of st and k < K, psi[r][k] and new_state[r][k] (T, 2)
 * of the candidate cand_tok[r][k] (DEVICE (R, K) int32) from the slots' states in ctc; rows that are not live are left untouched.
 * form 0 = the shipped kernel (a wavefront per candidate), 1 = the plain one (a thread per candidate, serial over the frames), 2 = the
 * shipped kernel with the emissions read strided from ctc->logits instead of from the init's (U, V, T) copy. */
int astk_debug_ctc_prefix(const astk_beam_desc* b, const astk_beam_state* st, const astk_beam_ctc* ctc, const int32_t* cand_tok, int form,
                          double* psi, double* new_state, void* stream);
#endif

/* Optional per-kernel HIP-event timing on the launch stream (bench.py's roofline legs; off by default).
 * astk_prof_end: res[0..1] attention-scan fwd (ms, launches); [2..3] attention-scan bwd; [4..6] GEMMs (ms, launches, flops);
 * [7..8] fused LSTM cells (ms, launches); [9..11] attention-scan phase inside the persistent decoder forward measured with
 * in-kernel timestamps (mean us per step over workgroups, slowest workgroup's mean us, launches); [12..14] same for the
 * backward; [16..19] persistent decoder forward / backward kernels (ms, launches).  res must hold 24 doubles.  Synchronises the device. */
int astk_prof_begin(void);
int astk_prof_end(double* res);

#ifdef __cplusplus
}
#endif
#endif /* ASTK_H */
