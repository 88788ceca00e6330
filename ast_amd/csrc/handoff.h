// The device side of the hand-off protocol between the workgroups of ONE persistent launch (lstm_persist.hip, decoder_persist.hip,
// decoder_wide.hip; attn.hip's in-launch combine uses the stores and loads).  DESIGN.md section 4 has the protocol and its measurements.
//
//   producer: written-through stores (st_sc1 / sti_sc1) -> publish(): every storing wave drains vmcnt, the workgroup barriers, ONE lane adds
//             to an arrival counter that lives on its own 256-byte line
//   consumer: one lane (wg_wait), or one lane per counter (wg_wait_multi, wg_wait_sh), polls with agent-scope loads; barrier; then sc1
//             loads (ld_sc1 / ldi_sc1 / ldb128_sc1): every such load goes to the memory side, never to a stale L2 line of this XCD
// Every spin is bounded: on time-out the waiter raises the launch's abort word (common.h AbortCtl), every poll loop checks it, the grid drains.
#pragma once
#include "common.h"

// In-kernel instrumentation (phase timers; the dawdling slice of the last-arrival regression test) exists only in the test-hook build
// (libastk_test.so, -DASTK_TEST_HOOKS): there ASTK_PERSIST_DBG is read at every launch; the product library's kernels see the constant 0
// and carry none of it.
#ifdef ASTK_TEST_HOOKS
static int persist_dbg_env() { const char* e = getenv("ASTK_PERSIST_DBG"); return e ? atoi(e) : 0; }
#define PERSIST_DBG(a) ((a).dbg)
#else
static int persist_dbg_env() { return 0; }
#define PERSIST_DBG(a) 0
#endif

namespace astk {

namespace {

constexpr int CTRS = 64;          // counter stride in words: arrival counters live 256 bytes apart, pollers of different counters never share a line

__device__ __forceinline__ unsigned ld_flag(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sti_sc1(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ldi_sc1(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// raw buffer descriptor over a hand-off buffer: lets the compiler track 16-byte sc1 loads / stores itself
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
// 16-byte sc1 load of handed-off activations at float offset float_off
__device__ __forceinline__ float4 ldb128_sc1(__amdgpu_buffer_rsrc_t r, long float_off) {
  const u32q v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(float_off * 4), 0, 16);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// Greedy decoding's stop (decoder_persist_fwd<.., GR = true>): `word` holds n_steps once every row has emitted EOS (stop_limit until
// then).  A wait made for decoder step `step` gives up, without raising the abort word, once step >= n_steps: its producer may have left.
// A wait for a step below n_steps never leaves on it -- every producer finishes all steps below n_steps before it leaves.  Every other
// kernel passes no word (the check folds away).  `recheck`: look once more after the counter is satisfied (the layer-0 cells' wait on
// their own tile's P6, which writes the word in front of that arrival).
struct StopCtl { const unsigned* word; int step; bool recheck; };
__device__ __forceinline__ bool stop_seen(const StopCtl& st) { return st.word && (unsigned)st.step >= ld_flag(st.word); }
// One lane waits until *ctr >= target (or the abort word is raised).  Returns false on abort / time-out.
__device__ __forceinline__ bool wait_ge(const unsigned* ctr, unsigned target, const AbortCtl& ab) {
  unsigned spins = 0;
  while (ld_flag(ctr) < target) {
    if (++spins > ab.limit) {   // ~seconds: something is wrong (grid not resident); drain instead of hanging
      abort_raise(ab);
      return false;
    }
    if ((spins & 63u) == 0 && abort_seen(ab)) return false;
  }
  return true;
}
// ... the same with the stop word in the slow path.  (A function of its own: with wait_ge written as wait_ge_stop with no word, four
// lstm_persist_bwd_rs instantiations came out with two instructions swapped and an fmac's operands commuted -- harmless, but not the same code.)
__device__ __forceinline__ bool wait_ge_stop(const unsigned* ctr, unsigned target, const AbortCtl& ab, const StopCtl& st) {
  unsigned spins = 0;
  while (ld_flag(ctr) < target) {
    if (++spins > ab.limit) {
      abort_raise(ab);
      return false;
    }
    if ((spins & 63u) == 0 && (abort_seen(ab) || stop_seen(st))) return false;
  }
  return true;
}
// workgroup-wide wait: lane 0 polls, everyone learns the outcome
__device__ __forceinline__ bool wg_wait(const unsigned* ctr, unsigned target, const AbortCtl& ab, int* s_flag,
                                        const StopCtl& st = StopCtl{nullptr, 0, false}) {
  if (threadIdx.x == 0) *s_flag = wait_ge_stop(ctr, target, ab, st) ? 1 : 0;
  __syncthreads();
  const bool ok = *s_flag != 0;
  __syncthreads();            // s_flag may be rewritten by the next wait
  return ok;
}
// workgroup-wide wait on `count` (<= 64) counters `stride` words apart: lane i of wave 0 polls counter i
__device__ __forceinline__ bool wg_wait_multi(const unsigned* base, int stride, int count, unsigned target, const AbortCtl& ab, int* s_flag,
                                              const StopCtl& st = StopCtl{nullptr, 0, false}) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    bool ok = true;
    unsigned spins = 0;
    for (;;) {
      const bool mine = lane < count ? ld_flag(base + (long)lane * stride) >= target : true;
      if (__all(mine)) break;
      if (++spins > ab.limit) { abort_raise(ab); ok = false; break; }
      if ((spins & 63u) == 0 && (abort_seen(ab) || stop_seen(st))) { ok = false; break; }
    }
    if (lane == 0) *s_flag = ok ? 1 : 0;
  }
  __syncthreads();
  const bool ok = *s_flag != 0;
  __syncthreads();
  return ok;
}
// Sharded phase counters: the items of a (phase, batch tile) bump one of NSH words (item % NSH), each on its own 256-byte line, and a
// waiter polls the NSH words with NSH lanes of one wave until `n_items` items have arrived `steps` times each.  Same-address atomics retire
// one after the other (~12 ns each in isolation, far more under load): with 32-128 arrivals per hand-off on ONE word the decoder kernels
// ran 1.00 / 1.00 ms; 4 / 8 / 16 / 32 / 64 words: 0.84/0.82, 0.80/0.78, 0.79/0.75, 0.78/0.73, 0.78/0.75 ms (forward / backward).
constexpr int NSH = 32;
__device__ __forceinline__ bool wg_wait_sh(const unsigned* base, int n_items, int steps, const AbortCtl& ab, int* s_flag,
                                           const StopCtl& st = StopCtl{nullptr, 0, false}) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned target = lane < NSH ? (unsigned)(((n_items - lane + NSH - 1) / NSH) * steps) : 0u;   // items with idx % NSH == lane
    bool ok = true;
    unsigned spins = 0;
    for (;;) {
      const bool mine = (lane < NSH && target > 0) ? ld_flag(base + lane * CTRS) >= target : true;
      if (__all(mine)) break;
      if (++spins > ab.limit) { abort_raise(ab); ok = false; break; }
      if ((spins & 63u) == 0 && (abort_seen(ab) || stop_seen(st))) { ok = false; break; }
    }
    if (ok && st.recheck && lane == 0 && stop_seen(st)) ok = false;
    if (lane == 0) *s_flag = ok ? 1 : 0;
  }
  __syncthreads();
  const bool ok = *s_flag != 0;
  __syncthreads();
  return ok;
}
// publish: every storing wave drains its stores (s_waitcnt vmcnt(0): the written-through stores it issued have completed), the workgroup
// barriers, one lane bumps the arrival counter.  That is ALL it drains: what a consumer reads behind the counter must have been stored
// written-through (sc1) by the waves that pass through here, and every one of them must pass through here.
// (tid: the caller's thread index inside its -- possibly virtual, see lstm_persist.hip's DUO -- workgroup)
__device__ __forceinline__ void publish(unsigned* ctr, int tid = threadIdx.x) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void publish_sh(unsigned* base, int item) { publish(base + (item & (NSH - 1)) * CTRS); }

// Gate activations of the persistent kernels' epilogues (on the recurrences' critical path): v_exp_f32 / v_rcp_f32 based,
// absolute error <= ~2e-7 (libdevice's tanhf/expf with full-precision division cost ~0.25 us more per step).
__device__ __forceinline__ float sigm_fast(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * x)) - 1.f; }

}  // namespace

}  // namespace astk
