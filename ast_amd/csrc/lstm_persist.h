// Persistent encoder LSTM loops: lstm_persist.hip, driven by lstm.hip.
#pragma once
#include "common.h"

namespace astk {

// one (direction, layer) cell of a launch, as lstm.hip's plan describes it; the launchers copy it into the kernels' PCellF / PCellB
struct PersistCellHost {
  const float *Wl, *Wu, *bias, *zx, *xin, *mask, *d_enc, *d_hT, *d_cT;
  float *gates, *C, *HR, *HD, *enc;
  float *PR, *PD;                 // backward, reduce-scatter path: partial-sum buffers of this cell
  const float* PD_up;
  int up_external;
  int reverse_pos, layer;
  unsigned long long* amax;       // backward: where max |dz| of the cell goes (16 sharded words, gemm_amax_reserve), null: not wanted
  float* db;                      // backward: bias gradient accumulated by the recurrence kernel itself (null: not wanted)
  long dy_sb, dy_st;              // backward: strides of d_enc (see PCellB)
  const unsigned* zx_flags; int zx_s0, zx_cs;      // forward, layer 0: chunk flags of the input projection (see PCellF)
  unsigned* prog; int prog_cs;                     // backward, layer 0: progress counter for side-stream consumers of dz (see PCellB)
  float* db_part;                                  // backward: deterministic bias-gradient scratch (see PCellB)
};

// Hoisted form (h = 1024): every layer is a launch of its own between batched GEMMs
bool lstm_persist_hoisted(int h);
bool lstm_persist_applicable(int T, int B, int h, int nl, int nd);
// Form of the recurrence workgroups (the `rows` argument of everything below): 16 = one 16-row batch tile per 256-thread workgroup;
// 33 = DUO: two 16-row tiles per 512-thread workgroup; 32 = MT 2: two tiles per 256-thread workgroup (lstm_persist.hip has the measurements)
constexpr int LSTM_ROWS_16 = 16, LSTM_ROWS_MT2 = 32, LSTM_ROWS_DUO = 33;
// Arithmetic of the recurrences' products (the kernels' template argument XS, so the values are fixed): f32 MFMAs; fp16x2 = two-term fp16
// splits; bf16x3 = three-term bf16 splits, resident weights in registers (h <= 256); bf16x3 with the weights' lo plane in LDS (h >= 512)
constexpr int LSTM_XS_F32 = 0, LSTM_XS_FP16X2 = 2, LSTM_XS_BF16X3 = 3, LSTM_XS_BF16X3_LDS = 4;
int lstm_persist_rows(int B, int h, int nl, int nd, bool side);
// The arithmetic (LSTM_XS_*) of the kernels a launch of form `rows` at width h runs under the mode and the knobs in force: what the
// launchers instantiate (the DUO form is bf16x3 with the lo plane in LDS at every width)
int lstm_persist_xs(int h, int rows);
// (Virtual) workgroup rows of a cell under form `rows`: 16-row batch tiles at 16; at 33 two virtual workgroups per 32 rows, so an EVEN number
// of 16-row tiles (what lstm.hip sizes the workspace for, whatever the form); at 32 one workgroup per 32 rows.  The grid has as many rows at 16
// and 32, half as many at 33.  Rows of the arrival counters (the abort word sits behind them), arrivals per unit slice on a progress counter,
// rows of the deterministic bias-gradient sums.
int lstm_persist_wg_rows(int B, int rows);
// Layers per launch: one workgroup per CU must hold a launch's whole grid.  0 = not applicable.
int lstm_persist_layers_per_launch(int B, int h, int nl, int nd, int rows);
// workgroups of one launch over `layers` layers of all directions
int lstm_persist_grid_wgs(int B, int h, int layers, int nd, int rows);
// floats of the reduce-scatter partial buffers of one cell (lstm.hip sizes the workspace with these)
size_t lstm_persist_pr_floats(int B, int h);
size_t lstm_persist_pd_floats(int T, int B, int h);
// the launchers return 0 on success
int lstm_persist_fwd_launch(const PersistCellHost* cells, int ncells, int nl, int T, int B, int h, int H, unsigned* counters, int rows, hipStream_t s);
int lstm_persist_bwd_launch(const PersistCellHost* cells, int ncells, int nl, int T, int B, int h, int H, unsigned* counters, unsigned amax_gen,
                            int rows, hipStream_t s);

}  // namespace astk
