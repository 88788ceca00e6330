// Resampling of waveforms by a rational ratio, and with it speed perturbation (include/astk.h astk_resample*):
// y[m] = sum over k = -K+1 .. K of x[n0 + k] g(phi / q - k), n0 = (m p) div q, phi = (m p) mod q, g a Hann-windowed sinc -- summed in
// ascending k in float64 and rounded once to float32, equal to tests/resample_model.py up to the contraction of a product and a sum
// into a fused multiply-add and the device's double sinpi / cospi.  wave, n_samples and the table are only read; no atomics anywhere.
//
// k_resample_prepare: fills the polyphase table of a descriptor into the caller's workspace -- Q = reduced q phases x 2K taps, stored
//   [tap][phase]: in tap j a wavefront's lanes read the doubles j Q + phi of ONE run of Q, whatever order the phases come in (phi
//   advances by p mod q from one output to the next), so up to 32 phases lie in 32 different LDS bank pairs and a larger table, read
//   through L2, is touched in one contiguous run per tap -- and then the digest of the table fields into the head.
// k_resample<TAB_LDS, SPAN_LDS>: one workgroup per (row, tile of ASTK_RESAMPLE_TILE output samples), one thread per output sample.
//   The input span of the tile, n0(first) - K + 1 .. n0(last) + K, is converted to float64 in LDS once (zeros outside the row's
//   length: what lies behind a length is never read, so a NaN there cannot surface) when it fits RS_SPAN_MAX doubles; a steeper
//   down-sampling reads its samples from global memory tap by tap.  The table is copied to LDS when it fits RS_TAB_MAX doubles (10
//   phases x 14 taps at 9/10: 1.1 KB) and is read through L2 otherwise.  Outputs at or behind a row's count, and every output of a
//   bad row, store zeros.
// k_resample_count_bad (only with n_bad): one workgroup re-validates every row and stores the count.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <mutex>
#include <unordered_map>

namespace astk {

namespace {

constexpr int RS_TILE = ASTK_RESAMPLE_TILE;                  // output samples, and threads, of one workgroup
constexpr int RS_TAB_MAX = 2048;                             // doubles of a table that is copied to LDS (16 KB)
constexpr int RS_SPAN_MAX = 4096;                            // doubles of an input span that is staged in LDS (32 KB)
constexpr int RS_COUNT_THREADS = 1024;
constexpr int RS_PREPARE_BLOCKS = 256;
constexpr unsigned long long RS_MAGIC = 0x726573616d706c65ull;

struct RsShape {
  long long P;                 // reduced p
  int Q, K, Z;                 // reduced q, half taps, num_zeros
  double c;                    // rolloff * min(1, q / p)
};

struct RsTables {
  unsigned long long* head;    // [0] digest of the table fields, [1] RS_MAGIC
  double* tab;                 // (2K, Q): g(phi / Q - (j - K + 1)) at [j][phi]
};

size_t rs_carve(void* base, const RsShape& s, RsTables& t) {
  Carver c(base);
  t.head = c.take<unsigned long long>(4);
  t.tab = c.take<double>((size_t)2 * s.K * s.Q);
  return c.total();
}

struct RsArgs {
  int B, Nmax, Mmax, i16, tiles;
  RsShape s;
  const void* wave;
  const int32_t* n_samples;
  float* out;
  int32_t* n_out;
  unsigned long long digest;
  RsTables t;
};

__global__ __launch_bounds__(256) void k_resample_prepare(RsShape s, RsTables t, unsigned long long digest) {
  const long total = 2l * s.K * s.Q;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int j = (int)(i / s.Q), phi = (int)(i % s.Q);
    const double tt = (double)phi / (double)s.Q - (double)(j - s.K + 1);
    const double u = s.c * tt;
    double g = 0.0;
    if (fabs(u) < (double)s.Z) {
      const double sinc = u == 0.0 ? 1.0 : sinpi(u) / (M_PI * u);
      const double cw = cospi(u / (2.0 * (double)s.Z));
      g = s.c * sinc * (cw * cw);
    }
    t.tab[i] = g;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    t.head[0] = digest;
    t.head[1] = RS_MAGIC;
  }
}

// output samples of a row of n samples, or -1 for a bad row (also: every row, when the workspace head does not hold this descriptor's
// digest).  The callers load n and the head side by side, not one behind the other's test.
__device__ __forceinline__ int rs_row_out(const RsArgs& a, int n, bool ws_ok) {
  if (!ws_ok || n < 0 || n > a.Nmax) return -1;
  const long long M = ((long long)n * a.s.Q + a.s.P - 1) / a.s.P;
  return M > a.Mmax ? -1 : (int)M;
}

__device__ __forceinline__ double rs_sample(const RsArgs& a, size_t row0, long long idx, int n) {      // x[idx] of the row, 0 outside [0, n)
  if (idx < 0 || idx >= n) return 0.0;
  return a.i16 ? (double)static_cast<const int16_t*>(a.wave)[row0 + (size_t)idx] : (double)static_cast<const float*>(a.wave)[row0 + (size_t)idx];
}

template <bool TAB_LDS, bool SPAN_LDS>
__global__ __launch_bounds__(RS_TILE) void k_resample(RsArgs a) {
  extern __shared__ double s_rs[];
  const RsShape& s = a.s;
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
  const int n = a.n_samples[b];
  const unsigned long long head0 = a.t.head[0], head1 = a.t.head[1];
  const int M = rs_row_out(a, n, head0 == a.digest && head1 == RS_MAGIC);
  if (tile == 0 && tid == 0) a.n_out[b] = M;
  const long long m0 = (long long)tile * RS_TILE, m = m0 + tid;
  float* out = a.out + (size_t)b * a.Mmax;
  if (m0 >= M) {                                             // (block-uniform) nothing of this tile is an output: a bad row too
    if (m < a.Mmax) out[m] = 0.f;
    return;
  }
  const int taps = 2 * s.K;
  double* s_tab = s_rs;
  double* s_x = s_rs + (TAB_LDS ? taps * s.Q : 0);
  if (TAB_LDS)
    for (int i = tid; i < taps * s.Q; i += RS_TILE) s_tab[i] = a.t.tab[i];
  const size_t row0 = (size_t)b * a.Nmax;                    // (0 <= n <= Nmax from here on: the row is a good one)
  const long long m_last = min(m0 + RS_TILE, (long long)M) - 1;
  const long long first = (m0 * s.P) / s.Q - s.K + 1;        // the span: first .. n0(m_last) + K, at most (TILE - 1) P / Q + 1 + 2K samples
  if (SPAN_LDS) {
    const int len = (int)((m_last * s.P) / s.Q + s.K - first + 1);
    for (int i = tid; i < len; i += RS_TILE) s_x[i] = rs_sample(a, row0, first + i, n);
  }
  __syncthreads();
  if (m >= M) {
    if (m < a.Mmax) out[m] = 0.f;
    return;
  }
  const long long mp = m * s.P;
  const long long n0 = mp / s.Q;
  const int phi = (int)(mp - n0 * s.Q);
  const double* tab = (TAB_LDS ? s_tab : a.t.tab) + phi;
  const long long x0 = n0 - s.K + 1;                         // the sample of tap 0
  const double* xs = s_x + (x0 - first);
  double acc = 0.0;
  for (int j = 0; j < taps; ++j) {
    const double x = SPAN_LDS ? xs[j] : rs_sample(a, row0, x0 + j, n);
    acc += x * tab[(size_t)j * s.Q];
  }
  out[m] = (float)acc;
}

__global__ __launch_bounds__(RS_COUNT_THREADS) void k_resample_count_bad(RsArgs a, int32_t* n_bad) {
  __shared__ int s_cnt[RS_COUNT_THREADS / 64];
  const bool ws_ok = a.t.head[0] == a.digest && a.t.head[1] == RS_MAGIC;
  int c = 0;
  for (int b = threadIdx.x; b < a.B; b += RS_COUNT_THREADS) c += rs_row_out(a, a.n_samples[b], ws_ok) < 0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < RS_COUNT_THREADS / 64; ++i) total += s_cnt[i];
    *n_bad = total;
  }
}

// ---- host side
std::mutex g_rs_mutex;
std::unordered_map<const void*, unsigned long long> g_rs_prepared;       // workspace address -> digest of the table enqueued into it

int rs_shape(const astk_resample_desc* d, RsShape& s, unsigned long long& digest) {
  ASTK_CHECK_DESC(d, astk_resample_desc);
  ASTK_CHECK(d->B >= 1, "resample: B = %d rows, there must be at least one", d->B);
  ASTK_CHECK(d->Nmax >= 1, "resample: Nmax = %d samples per row, there must be at least one", d->Nmax);
  ASTK_CHECK(d->Mmax >= 1, "resample: Mmax = %d output samples per row, there must be at least one", d->Mmax);
  ASTK_CHECK(d->p >= 1 && d->q >= 1, "resample: p = %d, q = %d: the ratio out / in = q / p needs both at least 1", d->p, d->q);
  ASTK_CHECK(d->sample_type == ASTK_FEAT_SAMPLE_F32 || d->sample_type == ASTK_FEAT_SAMPLE_I16,
             "resample: unknown sample_type %d (0 float32, 1 int16)", d->sample_type);
  ASTK_CHECK(d->num_zeros >= 1, "resample: num_zeros = %d, it must be at least 1", d->num_zeros);
  ASTK_CHECK(d->rolloff > 0.0 && d->rolloff <= 1.0, "resample: rolloff = %g lies outside (0, 1]", d->rolloff);
  int g = d->p, r = d->q;
  while (r) { const int t = g % r; g = r; r = t; }
  s.P = d->p / g;
  const int Q = d->q / g;
  ASTK_CHECK(Q <= ASTK_RESAMPLE_MAX_PHASES, "resample: q = %d reduces to %d phases, more than %d", d->q, Q, ASTK_RESAMPLE_MAX_PHASES);
  s.Q = Q;
  s.Z = d->num_zeros;
  s.c = d->rolloff * (s.Q < s.P ? (double)s.Q / (double)s.P : 1.0);
  const double half = std::ceil((double)s.Z / s.c);
  ASTK_CHECK(half <= (double)ASTK_RESAMPLE_MAX_HALF_TAPS, "resample: K = ceil(num_zeros / (rolloff min(1, q / p))) = %.0f half taps, more than %d",
             half, ASTK_RESAMPLE_MAX_HALF_TAPS);
  s.K = (int)half;
  const long tiles = ((long)d->Mmax + RS_TILE - 1) / RS_TILE;
  ASTK_CHECK(tiles * d->B <= 0x7fffffffl, "resample: B = %d rows of %ld tiles are more workgroups than one launch takes", d->B, tiles);
  unsigned long long rb;
  memcpy(&rb, &d->rolloff, sizeof(rb));
  unsigned long long h = RS_MAGIC;
  const unsigned long long words[] = {(unsigned long long)s.P, (unsigned long long)s.Q, (unsigned long long)s.Z, rb};
  for (unsigned long long w : words) h = mix64(h ^ w);
  digest = h;
  return 0;
}

template <bool TAB_LDS, bool SPAN_LDS>
void rs_launch(const RsArgs& a, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_resample<TAB_LDS, SPAN_LDS>), dim3((unsigned)((long)a.B * a.tiles)), dim3(RS_TILE), lds, s, a);
}

}  // namespace

}  // namespace astk

using namespace astk;

size_t astk_resample_workspace_bytes(const astk_resample_desc* d) {
  RsShape s;
  unsigned long long digest;
  if (rs_shape(d, s, digest) != 0) return 0;
  RsTables t;
  return rs_carve(nullptr, s, t);
}

int astk_resample_prepare(const astk_resample_desc* d, void* ws, size_t ws_bytes, void* stream) {
  RsShape s;
  unsigned long long digest;
  ASTK_TRY(rs_shape(d, s, digest));
  ASTK_CHECK(ws, "resample_prepare: the workspace must not be null");
  RsTables t;
  const size_t need = rs_carve(ws, s, t);
  ASTK_CHECK(ws_bytes >= need, "resample_prepare: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int blocks = (int)std::min<long>((2l * s.K * s.Q + 255) / 256, RS_PREPARE_BLOCKS);
  hipLaunchKernelGGL(k_resample_prepare, dim3(blocks), dim3(256), 0, (hipStream_t)stream, s, t, digest);
  ASTK_LAUNCH_CHECK();
  std::lock_guard<std::mutex> lock(g_rs_mutex);
  g_rs_prepared[ws] = digest;
  return 0;
}

int astk_resample(const astk_resample_desc* d, const void* wave, const int32_t* n_samples, float* out, int32_t* n_out, int32_t* n_bad,
                  const void* ws, size_t ws_bytes, void* stream) {
  RsArgs a;
  ASTK_TRY(rs_shape(d, a.s, a.digest));
  ASTK_CHECK(wave && n_samples && out && n_out && ws, "resample: wave, n_samples, out, n_out and the workspace must not be null");
  const size_t need = rs_carve(const_cast<void*>(ws), a.s, a.t);
  ASTK_CHECK(ws_bytes >= need, "resample: workspace of %zu bytes, %zu needed", ws_bytes, need);
  {
    std::lock_guard<std::mutex> lock(g_rs_mutex);
    const auto it = g_rs_prepared.find(ws);
    ASTK_CHECK(it != g_rs_prepared.end(), "resample: the workspace was never prepared (resample_prepare fills the table)");
    ASTK_CHECK(it->second == a.digest, "resample: the workspace was prepared for a different descriptor (its table fields differ)");
  }
  a.B = d->B; a.Nmax = d->Nmax; a.Mmax = d->Mmax;
  a.i16 = d->sample_type == ASTK_FEAT_SAMPLE_I16;
  a.tiles = (d->Mmax + RS_TILE - 1) / RS_TILE;
  a.wave = wave; a.n_samples = n_samples; a.out = out; a.n_out = n_out;
  hipStream_t s = (hipStream_t)stream;
  const long tab = 2l * a.s.K * a.s.Q;
  const long long span = ((long long)(RS_TILE - 1) * a.s.P) / a.s.Q + 1 + 2 * a.s.K;       // the longest span of a tile
  const bool tab_lds = tab <= RS_TAB_MAX, span_lds = span <= RS_SPAN_MAX;
  const size_t lds = ((tab_lds ? tab : 0) + (span_lds ? (long)span : 0)) * sizeof(double);
  if (tab_lds && span_lds) rs_launch<true, true>(a, lds, s);
  else if (tab_lds) rs_launch<true, false>(a, lds, s);
  else if (span_lds) rs_launch<false, true>(a, lds, s);
  else rs_launch<false, false>(a, lds, s);
  ASTK_LAUNCH_CHECK();
  if (n_bad) {
    hipLaunchKernelGGL(k_resample_count_bad, dim3(1), dim3(RS_COUNT_THREADS), 0, s, a, n_bad);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}
