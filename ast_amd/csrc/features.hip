// Speech features from waveforms and CMVN (include/astk.h astk_speech_features / astk_cmvn_*): MFCC or log mel
// filterbank rows in float64 arithmetic, rounded once to float32, equal to tests/speech_features_model.py up to the reordering of
// float64 sums and the device's double log / cos / pow.  wave, n_samples and the tables are only read; no atomics anywhere.
//
// k_feat_prepare: one workgroup fills the tables of a descriptor into the caller's workspace -- the window (zero behind frame_len up to
//   N), the twiddles exp(-2 pi i k / N) for k = 0 .. N/2, per mel filter its first FFT bin, its number of bins and the offset of its
//   weights in one packed array (a bin lies in at most two triangles: at most N weights), and lift_k dct[k][j] stored [j][k] -- and then
//   the digest of the descriptor's table fields into the head.  The cosine of the DCT and the sine of the lifter are evaluated by
//   feat_cospi below, a fixed sequence of IEEE operations (no fused multiply-add) that the host model repeats: the table is the model's
//   bit for bit, so frames whose mel energies sit on the floor (silence) come out equal to the model although their higher cepstra are
//   sums that cancel to rounding noise.
// k_speech_features: one wavefront per frame, FEAT_WAVES frames per workgroup, a grid-stride loop over the (row, frame) items of the
//   (B, Fmax) output; items at or behind a row's frame count (and every item of a bad row) store zeros.  The frame lives in the wave's
//   LDS slice of N doubles:
//     load        samples -> doubles (+ dither), the mean and the raw energy as wave reductions (butterfly shuffles: a fixed order)
//     pre-emphasis and window in passes of 64 samples from the top down, so a pass never reads what an earlier one wrote
//     FFT         the N real samples are N/2 complex ones as they lie; radix-2 decimation in frequency in place, one LDS exchange per
//                 stage, the result in bit-reversed order; the split step takes the bins k and N/2 - k together (both need Z[k] and
//                 Z[N/2 - k] and nothing else does) and leaves their powers where those two values lay
//     mel         one lane per filter (two rounds: up to 128 filters) over its bin range, ascending
//     DCT         the log energies go back to LDS; one lane per coefficient, ascending j, products and sums rounded separately
//   The waves of a workgroup work on different frames: every ordering point is wavefront-scope (feat_wave_sync).
// k_feat_count_bad / k_cmvn_count_bad (only with n_bad): one workgroup re-validates every row and stores the count.
// k_cmvn_accumulate: one workgroup per (group, 64 columns); wave w sums the frames t = w mod 4 of every row of the group in row order,
//   the four partial sums are added in wave order and then to the statistics.  k_cmvn_apply: one workgroup per (row, 64 frames).
#include "common.h"
#include <algorithm>
#include <mutex>
#include <unordered_map>

namespace astk {

namespace {

constexpr int FEAT_MAX_N = ASTK_FEAT_MAX_FRAME_LEN;          // frame_len <= 2048 = the largest FFT
constexpr int FEAT_MAX_MEL = ASTK_FEAT_MAX_MEL_BINS;
constexpr int FEAT_WAVES = 4;                                // frames in flight per workgroup: 4 * N * 8 bytes of LDS, 64 KiB at N = 2048
constexpr int FEAT_MAX_BLOCKS = 2048;                        // the grid: eight workgroups per CU; beyond it the loop strides
constexpr int FEAT_COUNT_THREADS = 1024;
constexpr double FEAT_EPS = 0x1p-23;                         // float32 epsilon: the floor of an energy
constexpr double FEAT_LOG_EPS = -15.942385152878742;         // ln(2^-23), the double next to it: what a floored energy's logarithm IS
constexpr unsigned long long FEAT_MAGIC = 0x7370656563686665ull;
constexpr int CMVN_FRAMES = 64;                              // frames of one row per workgroup of k_cmvn_apply
constexpr int CMVN_TILE = 1024;                              // columns whose mean / scale a workgroup keeps in LDS at a time

struct FeatTables {
  unsigned long long* head;    // [0] digest of the table fields
  double* window;              // (N)
  double2* tw;                 // (N/2 + 1)
  int* mel_start;              // (M)
  int* mel_count;              // (M)
  int* mel_off;                // (M)
  double* mel_w;               // (N)
  double* dct;                 // (M, num_ceps): lift_k dct[k][j] at [j][k]; mfcc only
};

struct FeatShape {
  int L, N, H, logH, M, ncep, window, mfcc;
  double sr, low, high, lifter;
};

size_t feat_carve(void* base, const FeatShape& s, FeatTables& t) {
  Carver c(base);
  t.head = c.take<unsigned long long>(4);
  t.window = c.take<double>(s.N);
  t.tw = c.take<double2>(s.H + 1);
  t.mel_start = c.take<int>(s.M);
  t.mel_count = c.take<int>(s.M);
  t.mel_off = c.take<int>(s.M);
  t.mel_w = c.take<double>(std::max(s.N, 2));
  t.dct = c.take<double>(s.mfcc ? (size_t)s.M * s.ncep : 1);
  return c.total();
}

struct FeatArgs {
  int B, Nmax, Fmax, D, shift, i16, dc, energy;
  FeatShape s;
  double preemph, dither;
  uint64_t seed;
  const int64_t* offsets;
  const void* wave;
  const int32_t* n_samples;
  float* feats;
  int32_t* n_frames;
  unsigned long long digest;
  FeatTables t;
};

// the lanes of one wavefront exchange data through their LDS slice: order the accesses on both sides (what __syncwarp() is made of)
__device__ __forceinline__ void feat_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double feat_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int feat_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sums and products the host model repeats bit for bit: rounded one by one, never contracted into a fused multiply-add
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double sub_rn(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- cos(pi t), t >= 0, as a fixed sequence of correctly rounded IEEE operations (tests/speech_features_model.py det_cospi repeats it)
__device__ double feat_poly(const double* c, int n, double x2) {
  double acc = c[n - 1];
  for (int i = n - 2; i >= 0; --i) acc = add_rn(mul_rn(acc, x2), c[i]);
  return acc;
}
__device__ double feat_cospi(double t) {
  // 1 / (2n)! and 1 / (2n + 1)! with alternating signs: the Taylor series to x^20 / x^21, 3e-21 at pi / 4
  const double cc[11] = {1.0, -1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
                         1.0 / 20922789888000.0, -1.0 / 6402373705728000.0, 1.0 / 2432902008176640000.0};
  const double sc[11] = {1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                         -1.0 / 1307674368000.0, 1.0 / 355687428096000.0, -1.0 / 121645100408832000.0, 1.0 / 51090942171709440000.0};
  double r = fmod(t, 2.0);
  double sign = 1.0;
  if (r > 1.0) r = sub_rn(2.0, r);
  if (r > 0.5) { r = sub_rn(1.0, r); sign = -1.0; }
  double v;
  if (r > 0.25) {
    const double x = mul_rn(M_PI, sub_rn(0.5, r));
    v = mul_rn(x, feat_poly(sc, 11, mul_rn(x, x)));
  } else {
    const double x = mul_rn(M_PI, r);
    v = feat_poly(cc, 11, mul_rn(x, x));
  }
  return mul_rn(sign, v);
}
__device__ double feat_sinpi(double t) { return feat_cospi(fabs(sub_rn(t, 0.5))); }

__device__ __forceinline__ double feat_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

__global__ __launch_bounds__(256) void k_feat_prepare(FeatShape s, FeatTables t, unsigned long long digest) {
  __shared__ int s_start[FEAT_MAX_MEL], s_count[FEAT_MAX_MEL], s_off[FEAT_MAX_MEL];
  const int tid = threadIdx.x;
  for (int i = tid; i < s.N; i += 256) {
    double w = 0.0;
    if (i < s.L) {
      const double c = cos(2.0 * M_PI * (double)i / (double)(s.L - 1));
      w = s.window == ASTK_FEAT_WINDOW_POVEY ? pow(0.5 - 0.5 * c, 0.85)
          : s.window == ASTK_FEAT_WINDOW_HAMMING ? 0.54 - 0.46 * c
          : s.window == ASTK_FEAT_WINDOW_HANNING ? 0.5 - 0.5 * c : 1.0;
    }
    t.window[i] = w;
  }
  for (int k = tid; k <= s.H; k += 256) {
    double sn, cs;
    sincospi(2.0 * (double)k / (double)s.N, &sn, &cs);
    t.tw[k] = make_double2(cs, -sn);
  }
  const double mel_low = feat_mel(s.low), mel_high = feat_mel(s.high);
  const double delta = (mel_high - mel_low) / (double)(s.M + 1);
  for (int j = tid; j < s.M; j += 256) {
    const double left = mel_low + j * delta, right = mel_low + (j + 2) * delta;
    int first = -1, n = 0;
    for (int i = 0; i < s.H; ++i) {
      const double m = feat_mel((double)i * s.sr / (double)s.N);
      if (m > left && m < right) {
        if (first < 0) first = i;
        ++n;
      }
    }
    s_start[j] = first < 0 ? 0 : first;
    s_count[j] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int off = 0;
    for (int j = 0; j < s.M; ++j) {
      s_off[j] = off;
      if (off + s_count[j] > s.N) s_count[j] = s.N - off;      // (cannot happen: a bin lies in at most two triangles)
      off += s_count[j];
    }
  }
  __syncthreads();
  for (int j = tid; j < s.M; j += 256) {
    const double left = mel_low + j * delta, center = mel_low + (j + 1) * delta, right = mel_low + (j + 2) * delta;
    t.mel_start[j] = s_start[j];
    t.mel_count[j] = s_count[j];
    t.mel_off[j] = s_off[j];
    for (int i = 0; i < s_count[j]; ++i) {
      const double m = feat_mel((double)(s_start[j] + i) * s.sr / (double)s.N);
      t.mel_w[s_off[j] + i] = m <= center ? (m - left) / (center - left) : (right - m) / (right - center);
    }
  }
  if (s.mfcc) {
    const double root1 = __dsqrt_rn(__ddiv_rn(1.0, (double)s.M)), root2 = __dsqrt_rn(__ddiv_rn(2.0, (double)s.M));
    for (int idx = tid; idx < s.ncep * s.M; idx += 256) {
      const int k = idx / s.M, j = idx % s.M;
      double lift = 1.0;
      if (s.lifter != 0.0) lift = add_rn(1.0, mul_rn(mul_rn(0.5, s.lifter), feat_sinpi(__ddiv_rn((double)k, s.lifter))));
      const double d = k == 0 ? root1 : mul_rn(root2, feat_cospi(__ddiv_rn(mul_rn((double)j + 0.5, (double)k), (double)s.M)));
      t.dct[(size_t)j * s.ncep + k] = mul_rn(lift, d);
    }
  }
  if (tid == 0) {
    t.head[0] = digest;
    t.head[1] = FEAT_MAGIC;
  }
}

// frames of row b, or -1 for a bad row (also: every row, when the workspace head does not hold this descriptor's digest)
__device__ __forceinline__ int feat_row_frames(const FeatArgs& a, int b, bool ws_ok) {
  const int n = a.n_samples[b];
  if (!ws_ok || n < 0 || n > a.Nmax) return -1;
  const int F = n < a.s.L ? 0 : 1 + (n - a.s.L) / a.shift;
  return F > a.Fmax ? -1 : F;
}

// element g of the unit-normal stream of util.hip's normal fill at offset 0, in float64 (tests/rng_model.unit_normals)
__device__ __forceinline__ double feat_dither(uint64_t seed, uint64_t g) {
  const uint64_t h = mix64(seed ^ mix64(g >> 1));
  const double u1 = (double)(((h & 0xffffffffull) >> 8) + 1) * 0x1p-24, u2 = (double)((h >> 40) + 1) * 0x1p-24;
  const double r = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
  return (g & 1) ? r * sin(ang) : r * cos(ang);
}

__device__ __forceinline__ double2 feat_cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__device__ __forceinline__ double feat_log_floor(double e) { return e > FEAT_EPS ? log(e) : FEAT_LOG_EPS; }

__global__ __launch_bounds__(FEAT_WAVES * 64) void k_speech_features(FeatArgs a) {
  extern __shared__ double s_feat[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const FeatShape& s = a.s;
  const int slice = max(s.N, FEAT_MAX_MEL);
  double* buf = s_feat + (size_t)wv * slice;
  double2* z = reinterpret_cast<double2*>(buf);
  const bool ws_ok = a.t.head[0] == a.digest && a.t.head[1] == FEAT_MAGIC;
  const long items = (long)a.B * a.Fmax;
  const int rev_shift = 32 - s.logH;                         // position of Z[k]: its logH bits reversed (H = 1: one point, at 0)
  auto rev = [&](int k) -> int { return s.logH ? (int)(__brev((unsigned)k) >> rev_shift) : 0; };
  for (long it = (long)blockIdx.x * FEAT_WAVES + wv; it < items; it += (long)gridDim.x * FEAT_WAVES) {      // (wave-uniform)
    const int b = (int)(it / a.Fmax), t = (int)(it % a.Fmax);
    const int F = feat_row_frames(a, b, ws_ok);
    float* out = a.feats + (size_t)it * a.D;
    if (t == 0 && lane == 0) a.n_frames[b] = F;
    if (t >= F) {
      for (int k = lane; k < a.D; k += 64) out[k] = 0.f;
      continue;
    }
    feat_wave_sync();                                        // the last frame's reads are behind us
    // ---- load (+ dither), mean, raw energy
    const size_t s0 = (size_t)b * a.Nmax + (size_t)t * a.shift;                          // s0 + L <= b Nmax + n_b: inside the row's length
    const uint64_t g0 = (uint64_t)(a.offsets ? a.offsets[b] : 0) + (uint64_t)t * (uint64_t)a.shift;
    double part = 0.0;
    for (int i = lane; i < s.L; i += 64) {
      double v = a.i16 ? (double)static_cast<const int16_t*>(a.wave)[s0 + i] : (double)static_cast<const float*>(a.wave)[s0 + i];
      if (a.dither != 0.0) v += a.dither * feat_dither(a.seed, g0 + (uint64_t)i);
      buf[i] = v;
      part += v;
    }
    const double mean = a.dc ? feat_wave_sum(part) / (double)s.L : 0.0;
    feat_wave_sync();
    double log_energy = 0.0;
    if (a.energy) {
      double e = 0.0;
      for (int i = lane; i < s.L; i += 64) {
        const double v = buf[i] - mean;
        e += v * v;
      }
      log_energy = feat_log_floor(feat_wave_sum(e));
    }
    // ---- pre-emphasis, window, zero padding: from the top down
    for (int i0 = s.N - 64; i0 > -64; i0 -= 64) {
      const int i = i0 + lane;
      double cur = 0.0, prev = 0.0;
      const bool on = i >= 0 && i < s.L;
      if (on) {
        cur = buf[i] - mean;
        prev = buf[i > 0 ? i - 1 : 0] - mean;
      }
      feat_wave_sync();                                      // lane l + 1 has read what lane l is about to write
      if (i >= 0 && i < s.N) buf[i] = on ? (cur - a.preemph * prev) * a.t.window[i] : 0.0;
    }
    feat_wave_sync();
    // ---- complex FFT of H = N / 2 points, decimation in frequency: Z[k] ends at position bitrev(k)
    for (int half = s.H >> 1, mult = 2; half >= 1; half >>= 1, mult <<= 1) {
      for (int q = lane; q < (s.H >> 1); q += 64) {
        const int k = q & (half - 1);
        const int i0 = ((q - k) << 1) + k, i1 = i0 + half;
        const double2 x0 = z[i0], x1 = z[i1];
        const double2 w = a.t.tw[k * mult];                  // exp(-2 pi i k / (2 half))
        z[i0] = make_double2(x0.x + x1.x, x0.y + x1.y);
        z[i1] = feat_cmul(make_double2(x0.x - x1.x, x0.y - x1.y), w);
      }
      feat_wave_sync();
    }
    // ---- split step and power spectrum: |X_k|^2 to z[bitrev(k)].x, k = 0 .. H - 1 (the Nyquist bin is not used)
    if (lane == 0) {
      const double x0 = z[0].x + z[0].y;
      z[0].x = x0 * x0;
    }
    for (int k = 1 + lane; k <= (s.H >> 1); k += 64) {
      const int p = rev(k), q = rev(s.H - k);
      const double2 zk = z[p], zq = z[q];
      const double2 xe = make_double2(0.5 * (zk.x + zq.x), 0.5 * (zk.y - zq.y));         // (Z_k + conj Z_{H-k}) / 2
      const double2 xo = make_double2(0.5 * (zk.y + zq.y), -0.5 * (zk.x - zq.x));        // (Z_k - conj Z_{H-k}) / 2i
      const double2 tt = feat_cmul(a.t.tw[k], xo);
      const double ar = xe.x + tt.x, ai = xe.y + tt.y, br = xe.x - tt.x, bi = xe.y - tt.y;
      z[p].x = ar * ar + ai * ai;
      z[q].x = br * br + bi * bi;                            // (k = H / 2: p == q and both are |Z_k|^2)
    }
    feat_wave_sync();
    // ---- mel energies: lane per filter
    double lg[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int j = lane + 64 * r;
      if (j < s.M) {
        const int st = a.t.mel_start[j], n = a.t.mel_count[j];
        const double* w = a.t.mel_w + a.t.mel_off[j];
        double e = 0.0;
        for (int i = 0; i < n; ++i) e += w[i] * z[rev(st + i)].x;
        lg[r] = feat_log_floor(e);
      }
    }
    if (!s.mfcc) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (lane + 64 * r < s.M) out[lane + 64 * r] = (float)lg[r];
      continue;
    }
    feat_wave_sync();                                        // every lane has read its powers
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (lane + 64 * r < s.M) buf[lane + 64 * r] = lg[r];
    feat_wave_sync();
    // ---- DCT and lifter: lane per coefficient
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int k = lane + 64 * r;
      if (k < s.ncep) {
        double acc = 0.0;
        for (int j = 0; j < s.M; ++j) acc = add_rn(acc, mul_rn(a.t.dct[(size_t)j * s.ncep + k], buf[j]));
        if (a.energy && k == 0) acc = log_energy;
        out[k] = (float)acc;
      }
    }
  }
}

__global__ __launch_bounds__(FEAT_COUNT_THREADS) void k_feat_count_bad(FeatArgs a, int32_t* n_bad) {
  __shared__ int s_cnt[FEAT_COUNT_THREADS / 64];
  const bool ws_ok = a.t.head[0] == a.digest && a.t.head[1] == FEAT_MAGIC;
  int c = 0;
  for (int b = threadIdx.x; b < a.B; b += FEAT_COUNT_THREADS) c += feat_row_frames(a, b, ws_ok) < 0 ? 1 : 0;
  c = feat_wave_sum_int(c);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < FEAT_COUNT_THREADS / 64; ++i) total += s_cnt[i];
    *n_bad = total;
  }
}

// ---- CMVN
struct CmvnArgs {
  int B, Fmax, D, G, norm_vars;
  const float* in;
  float* out;
  const int32_t* n_frames;
  const int32_t* group;
  double* stats;
};

__global__ __launch_bounds__(256) void k_cmvn_accumulate(CmvnArgs a) {
  __shared__ double s_sum[4][64], s_sq[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x, d = blockIdx.y * 64 + lane;
  double sum = 0.0, sq = 0.0;
  long count = 0;
  for (int b = 0; b < a.B; ++b) {
    if (a.group[b] != g || a.n_frames[b] < 0) continue;       // (block-uniform)
    const int nf = min(a.n_frames[b], a.Fmax);
    count += nf;
    if (d < a.D) {
      const float* x = a.in + (size_t)b * a.Fmax * a.D + d;
      for (int t = wv; t < nf; t += 4) {
        const double v = (double)x[(size_t)t * a.D];
        sum += v;
        sq += v * v;
      }
    }
  }
  s_sum[wv][lane] = sum;
  s_sq[wv][lane] = sq;
  __syncthreads();
  if (wv == 0) {
    double* st = a.stats + (size_t)g * 2 * (a.D + 1);
    if (d < a.D) {
      st[d] += ((s_sum[0][lane] + s_sum[1][lane]) + s_sum[2][lane]) + s_sum[3][lane];
      st[a.D + 1 + d] += ((s_sq[0][lane] + s_sq[1][lane]) + s_sq[2][lane]) + s_sq[3][lane];
    }
    if (blockIdx.y == 0 && lane == 0) st[a.D] += (double)count;
  }
}

__global__ __launch_bounds__(FEAT_COUNT_THREADS) void k_cmvn_count_bad(CmvnArgs a, int32_t* n_bad) {
  __shared__ int s_cnt[FEAT_COUNT_THREADS / 64];
  int c = 0;
  for (int b = threadIdx.x; b < a.B; b += FEAT_COUNT_THREADS) c += (a.group[b] < 0 || a.group[b] >= a.G) ? 1 : 0;
  c = feat_wave_sum_int(c);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < FEAT_COUNT_THREADS / 64; ++i) total += s_cnt[i];
    *n_bad = total;
  }
}

__global__ __launch_bounds__(256) void k_cmvn_apply(CmvnArgs a, const double* stats) {
  __shared__ double s_mean[CMVN_TILE], s_scale[CMVN_TILE];
  const int b = blockIdx.x, t0 = blockIdx.y * CMVN_FRAMES;
  const int nt = min(CMVN_FRAMES, a.Fmax - t0);
  const int g = a.group[b];
  const int nf = a.n_frames[b] < 0 ? 0 : min(a.n_frames[b], a.Fmax);
  const double* st = stats + (size_t)(g >= 0 && g < a.G ? g : 0) * 2 * (a.D + 1);
  const double count = (g >= 0 && g < a.G) ? st[a.D] : 0.0;
  const bool live = count > 0.0;                             // (block-uniform)
  const int nlive = live ? max(0, min(nt, nf - t0)) : 0;     // frames of this chunk that are normalised
  const size_t base = ((size_t)b * a.Fmax + t0) * a.D;
  for (int d0 = 0; d0 < a.D; d0 += CMVN_TILE) {
    const int dn = min(CMVN_TILE, a.D - d0);
    __syncthreads();
    if (nlive > 0) {
      for (int d = threadIdx.x; d < dn; d += 256) {
        const double mean = st[d0 + d] / count;
        double sc = 1.0;
        if (a.norm_vars) sc = 1.0 / sqrt(fmax(sub_rn(st[a.D + 1 + d0 + d] / count, mul_rn(mean, mean)), 1e-20));
        s_mean[d] = mean;
        s_scale[d] = sc;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nt * dn; e += 256) {
      const int tt = e / dn, dd = e % dn;
      const size_t idx = base + (size_t)tt * a.D + d0 + dd;
      if (tt < nlive) a.out[idx] = (float)mul_rn(sub_rn((double)a.in[idx], s_mean[dd]), s_scale[dd]);
      else if (a.out != a.in) a.out[idx] = a.in[idx];
    }
  }
}

// ---- host side
std::mutex g_feat_mutex;
std::unordered_map<const void*, unsigned long long> g_feat_prepared;     // workspace address -> digest of the tables enqueued into it

unsigned long long feat_bits(double v) {
  unsigned long long u;
  memcpy(&u, &v, sizeof(u));
  return u;
}

int feat_shape(const astk_speech_features_desc* d, FeatShape& s, unsigned long long& digest) {
  ASTK_CHECK_DESC(d, astk_speech_features_desc);
  ASTK_CHECK(d->B >= 1, "speech_features: B = %d rows, there must be at least one", d->B);
  ASTK_CHECK(d->Nmax >= 1, "speech_features: Nmax = %d samples per row, there must be at least one", d->Nmax);
  ASTK_CHECK(d->Fmax >= 1, "speech_features: Fmax = %d frames per row, there must be at least one", d->Fmax);
  ASTK_CHECK(d->frame_len >= 2 && d->frame_len <= FEAT_MAX_N, "speech_features: frame_len = %d lies outside 2..%d", d->frame_len, FEAT_MAX_N);
  ASTK_CHECK(d->frame_shift >= 1, "speech_features: frame_shift = %d, it must be at least 1", d->frame_shift);
  ASTK_CHECK(d->kind == ASTK_FEAT_MFCC || d->kind == ASTK_FEAT_FBANK, "speech_features: unknown kind %d (0 mfcc, 1 fbank)", d->kind);
  ASTK_CHECK(d->window >= ASTK_FEAT_WINDOW_POVEY && d->window <= ASTK_FEAT_WINDOW_RECTANGULAR,
             "speech_features: unknown window %d (0 povey, 1 hamming, 2 hanning, 3 rectangular)", d->window);
  ASTK_CHECK(d->sample_type == ASTK_FEAT_SAMPLE_F32 || d->sample_type == ASTK_FEAT_SAMPLE_I16,
             "speech_features: unknown sample_type %d (0 float32, 1 int16)", d->sample_type);
  ASTK_CHECK(d->num_mel_bins >= 3 && d->num_mel_bins <= FEAT_MAX_MEL, "speech_features: num_mel_bins = %d lies outside 3..%d", d->num_mel_bins,
             FEAT_MAX_MEL);
  if (d->kind == ASTK_FEAT_MFCC)
    ASTK_CHECK(d->num_ceps >= 1 && d->num_ceps <= d->num_mel_bins, "speech_features: num_ceps = %d lies outside 1..num_mel_bins = %d", d->num_ceps,
               d->num_mel_bins);
  ASTK_CHECK(!(d->use_energy && d->kind == ASTK_FEAT_FBANK), "speech_features: use_energy is an mfcc option, the kind is fbank");
  ASTK_CHECK(d->sample_frequency > 0.0, "speech_features: sample_frequency = %g, it must be positive", d->sample_frequency);
  const double nyquist = 0.5 * d->sample_frequency;
  const double high = d->high_freq > 0.0 ? d->high_freq : nyquist + d->high_freq;
  ASTK_CHECK(d->low_freq >= 0.0, "speech_features: low_freq = %g is negative", d->low_freq);
  ASTK_CHECK(high > d->low_freq && high <= nyquist, "speech_features: high_freq = %g resolves to %g, outside (low_freq = %g, Nyquist = %g]",
             d->high_freq, high, d->low_freq, nyquist);
  ASTK_CHECK(d->cepstral_lifter >= 0.0, "speech_features: cepstral_lifter = %g is negative", d->cepstral_lifter);
  s.L = d->frame_len;
  s.N = 2;
  while (s.N < s.L) s.N <<= 1;
  s.H = s.N >> 1;
  s.logH = 0;
  while ((1 << s.logH) < s.H) ++s.logH;
  s.M = d->num_mel_bins;
  s.mfcc = d->kind == ASTK_FEAT_MFCC;
  s.ncep = s.mfcc ? d->num_ceps : 0;
  s.window = d->window;
  s.sr = d->sample_frequency;
  s.low = d->low_freq;
  s.high = high;
  s.lifter = s.mfcc ? d->cepstral_lifter : 0.0;
  unsigned long long h = FEAT_MAGIC;
  const unsigned long long words[] = {(unsigned long long)s.L, (unsigned long long)s.M, (unsigned long long)s.ncep, (unsigned long long)s.window,
                                      (unsigned long long)s.mfcc, feat_bits(s.sr), feat_bits(s.low), feat_bits(s.high), feat_bits(s.lifter)};
  for (unsigned long long w : words) h = mix64(h ^ w);
  digest = h;
  return 0;
}

}  // namespace

}  // namespace astk

using namespace astk;

size_t astk_speech_features_workspace_bytes(const astk_speech_features_desc* d) {
  FeatShape s;
  unsigned long long digest;
  if (feat_shape(d, s, digest) != 0) return 0;
  FeatTables t;
  return feat_carve(nullptr, s, t);
}

int astk_speech_features_prepare(const astk_speech_features_desc* d, void* ws, size_t ws_bytes, void* stream) {
  FeatShape s;
  unsigned long long digest;
  ASTK_TRY(feat_shape(d, s, digest));
  ASTK_CHECK(ws, "speech_features_prepare: the workspace must not be null");
  FeatTables t;
  const size_t need = feat_carve(ws, s, t);
  ASTK_CHECK(ws_bytes >= need, "speech_features_prepare: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipLaunchKernelGGL(k_feat_prepare, dim3(1), dim3(256), 0, (hipStream_t)stream, s, t, digest);
  ASTK_LAUNCH_CHECK();
  std::lock_guard<std::mutex> lock(g_feat_mutex);
  g_feat_prepared[ws] = digest;
  return 0;
}

int astk_speech_features(const astk_speech_features_desc* d, const void* wave, const int32_t* n_samples, float* feats, int32_t* n_frames,
                         int32_t* n_bad, void* ws, size_t ws_bytes, void* stream) {
  FeatArgs a;
  ASTK_TRY(feat_shape(d, a.s, a.digest));
  ASTK_CHECK(wave && n_samples && feats && n_frames && ws, "speech_features: wave, n_samples, feats, n_frames and the workspace must not be null");
  const size_t need = feat_carve(ws, a.s, a.t);
  ASTK_CHECK(ws_bytes >= need, "speech_features: workspace of %zu bytes, %zu needed", ws_bytes, need);
  {
    std::lock_guard<std::mutex> lock(g_feat_mutex);
    const auto it = g_feat_prepared.find(ws);
    ASTK_CHECK(it != g_feat_prepared.end(), "speech_features: the workspace was never prepared (speech_features_prepare fills the tables)");
    ASTK_CHECK(it->second == a.digest, "speech_features: the workspace was prepared for a different descriptor (its table fields differ)");
  }
  a.B = d->B; a.Nmax = d->Nmax; a.Fmax = d->Fmax;
  a.D = a.s.mfcc ? a.s.ncep : a.s.M;
  a.shift = d->frame_shift;
  a.i16 = d->sample_type == ASTK_FEAT_SAMPLE_I16;
  a.dc = d->remove_dc_offset != 0;
  a.energy = d->use_energy != 0;
  a.preemph = d->preemphasis; a.dither = d->dither; a.seed = d->seed; a.offsets = d->offsets;
  a.wave = wave; a.n_samples = n_samples; a.feats = feats; a.n_frames = n_frames;
  hipStream_t s = (hipStream_t)stream;
  const long items = (long)d->B * d->Fmax;
  const int blocks = (int)std::min<long>((items + FEAT_WAVES - 1) / FEAT_WAVES, FEAT_MAX_BLOCKS);
  const size_t lds = (size_t)FEAT_WAVES * std::max(a.s.N, FEAT_MAX_MEL) * sizeof(double);
  hipLaunchKernelGGL(k_speech_features, dim3(blocks), dim3(FEAT_WAVES * 64), lds, s, a);
  ASTK_LAUNCH_CHECK();
  if (n_bad) {
    hipLaunchKernelGGL(k_feat_count_bad, dim3(1), dim3(FEAT_COUNT_THREADS), 0, s, a, n_bad);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

static int cmvn_args(const astk_cmvn_desc* d, CmvnArgs& a) {
  ASTK_CHECK_DESC(d, astk_cmvn_desc);
  ASTK_CHECK(d->B >= 1, "cmvn: B = %d rows, there must be at least one", d->B);
  ASTK_CHECK(d->Fmax >= 1, "cmvn: Fmax = %d frames per row, there must be at least one", d->Fmax);
  ASTK_CHECK(d->D >= 1, "cmvn: D = %d features, there must be at least one", d->D);
  ASTK_CHECK(d->G >= 1, "cmvn: G = %d groups, there must be at least one", d->G);
  ASTK_CHECK((d->Fmax + CMVN_FRAMES - 1) / CMVN_FRAMES <= 65535, "cmvn: Fmax = %d frames is more than %d", d->Fmax, 65535 * CMVN_FRAMES);
  ASTK_CHECK((d->D + 63) / 64 <= 65535, "cmvn: D = %d features is more than %d", d->D, 65535 * 64);
  a.B = d->B; a.Fmax = d->Fmax; a.D = d->D; a.G = d->G; a.norm_vars = d->norm_vars != 0;
  return 0;
}

int astk_cmvn_accumulate(const astk_cmvn_desc* d, const float* feats, const int32_t* n_frames, const int32_t* group, double* stats,
                         int32_t* n_bad, void* stream) {
  CmvnArgs a;
  ASTK_TRY(cmvn_args(d, a));
  ASTK_CHECK(feats && n_frames && group && stats, "cmvn_accumulate: feats, n_frames, group and stats must not be null");
  a.in = feats; a.out = nullptr; a.n_frames = n_frames; a.group = group; a.stats = stats;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cmvn_accumulate, dim3(a.G, (a.D + 63) / 64), dim3(256), 0, s, a);
  ASTK_LAUNCH_CHECK();
  if (n_bad) {
    hipLaunchKernelGGL(k_cmvn_count_bad, dim3(1), dim3(FEAT_COUNT_THREADS), 0, s, a, n_bad);
    ASTK_LAUNCH_CHECK();
  }
  return 0;
}

int astk_cmvn_apply(const astk_cmvn_desc* d, const float* feats_in, float* feats_out, const int32_t* n_frames, const int32_t* group,
                    const double* stats, void* stream) {
  CmvnArgs a;
  ASTK_TRY(cmvn_args(d, a));
  ASTK_CHECK(feats_in && feats_out && n_frames && group && stats, "cmvn_apply: feats_in, feats_out, n_frames, group and stats must not be null");
  a.in = feats_in; a.out = feats_out; a.n_frames = n_frames; a.group = group; a.stats = nullptr;
  hipLaunchKernelGGL(k_cmvn_apply, dim3(a.B, (a.Fmax + CMVN_FRAMES - 1) / CMVN_FRAMES), dim3(256), 0, (hipStream_t)stream, a, stats);
  ASTK_LAUNCH_CHECK();
  return 0;
}
