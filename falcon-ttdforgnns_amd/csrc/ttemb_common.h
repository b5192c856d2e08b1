// Shared declarations for the libttemb_hip.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/ttemb.h"

namespace ttemb {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kMaxProbes = 3;      // reference MAX_PROBES, FBTT/tt_embeddings_cuda.cu:31
constexpr int64_t kEmptyKey = -1;  // reference UNUSED_KEY, FBTT/hashtbl_cuda_utils.cuh:100

// Device-side view of one table's factorisation (passed to kernels by value).
struct DevShape {
  int T;
  int p[TTEMB_MAX_CORES];
  int q[TTEMB_MAX_CORES];
  int R[TTEMB_MAX_CORES + 1];
  long long L[TTEMB_MAX_CORES];   // L[t] = prod(p[t+1:])
  int D;                          // prod(q)
  int row_len[TTEMB_MAX_CORES];   // floats per core row: R[t]*q[t]*R[t+1]
  int part_len[TTEMB_MAX_CORES];  // floats of the partial product after core t: q0..qt * R[t+1]
  int part_max;                   // max part_len over t < T-1 (and q0*R1)
};

struct CorePtrs {
  const float* c[TTEMB_MAX_CORES];
};
struct CorePtrsMut {
  float* c[TTEMB_MAX_CORES];
};

// host helpers (ttemb_api.hip)
int fail(int code, const char* fmt, ...);
int check_hip(hipError_t e, const char* what);
int make_dev_shape(const ttemb_shape_t* s, DevShape* out);
int current_path();
// measurement hook: bracket the main chain kernel with events when profiling is on
void profile_begin(int which, hipStream_t st);
void profile_end(int which, hipStream_t st);

// gfx950 has 160 KB of LDS per CU; a launch above the default 64 KB of dynamic LDS has to be allowed per kernel AND per
// device (hipFuncSetAttribute acts on the current device's function object; a process may drive several GPUs).  One gate
// per kernel: bit d = "allowed on device d"; devices past 63 ask the runtime every time.
constexpr size_t kLdsDefault = 64 * 1024, kCuLds = 160 * 1024;
struct LdsGate {
  std::atomic<uint64_t> devices{0};
};
int allow_big_lds(const void* kernel, size_t lds_bytes, LdsGate* gate, const char* what);
int device_cus();   // CUs of the current device (cached per device; 256 when it cannot be asked)

// generic kernels (ttemb_generic.hip)
int64_t generic_fwd_lds_bytes(const DevShape& s);
int64_t generic_bwd_lds_bytes(const DevShape& s);
int launch_forward_generic(const DevShape& s, const CorePtrs& cores, const int64_t* indices,
                           const int64_t* rowidx, const int64_t* offsets, int64_t B, int64_t nnz,
                           const int32_t* nnz_dev, float* output, hipStream_t st);
int launch_backward_generic(const DevShape& s, const CorePtrs& cores, const int64_t* indices,
                            const int64_t* rowidx, const int64_t* offsets, int64_t B, int64_t nnz,
                            const int32_t* nnz_dev, const float* d_output, const CorePtrsMut& d_cores, hipStream_t st);
// zero-fills the T gradient cores in one launch
int launch_zero_cores(const DevShape& s, const CorePtrsMut& d_cores, hipStream_t st);

// fast 3-core path (ttemb_fast3.hip)
bool fast3_supported(const DevShape& s);
bool fast3_pays(const DevShape& s, int64_t nnz);
bool fast3_prefix_in_chain(const DevShape& s, int64_t nnz, int64_t B);   // a whole forward of this size forms P inside its chain kernel
bool fast3_group_products_in_chain(const DevShape& s, int64_t nnz, int64_t B);   // a backward of this size forms the per-group products inside its chunk kernel
bool fast3_fits(const DevShape& s, int64_t nnz, int64_t B);   // the call fits one 32-bit row window / one grouping pass
bool fast3_fits_in_pieces(const DevShape& s, int64_t nnz, int64_t B);   // ... or runs as several pieces (needs `offsets`)
void fast3_set_piece_limits(int64_t rows, int64_t ids);                  // diagnostic: smaller pieces than the hardware's
int fast3_grouping_layout(const DevShape& s, int64_t nnz, int64_t* out);  // diagnostic: ttemb_grouping_layout
void fast3_set_spin_limit(int64_t tries);                                // diagnostic: tries of the grouping pass's bounded waits
void fast3_set_wide_slab_min_ids(int64_t ids);                           // diagnostic: call size from which the wide backward reduces dG2 in LDS
// The pinned host word a device-side wait that ran out reports to (ttemb_api.hip): its device address for the kernels
// (null until ttemb_init() / ttemb_status() has created it -- the lookups allocate nothing), and the host-side check every
// lookup entry point starts with -- TTEMB_E_HIP once per reported fault.
uint32_t* fault_word(hipStream_t st);
int fault_word_init();
int pending_device_fault();
int64_t fast3_workspace_bytes(const DevShape& s, int32_t op, int64_t nnz, int64_t B);
int64_t fast3_plan_bytes(const DevShape& s, int64_t nnz);
// phase: 0 = whole forward, 1 = id-only half (grouping into `plan`), 2 = lookup on a plan grouped by phase 1.
// rowidx may be null when offsets is given (rows are derived while grouping); zero_rows: clear the output rows
// of bags that do not hold exactly one id (needs offsets)
int launch_forward_fast3(const DevShape& s, const CorePtrs& cores, const int64_t* indices,
                         const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                         const int32_t* nnz_dev, int64_t B, float* output, bool zero_rows, void* ws,
                         int64_t ws_bytes, void* plan, int64_t plan_bytes, int phase, hipStream_t st, void* header);
// `header`: kFast3HeaderBytes at the start of the caller's workspace, the same address for every op on that workspace: the
// words of the grouping pass that outlive a call (its epoch, the pre-tagged range counters).  Any content is valid.
constexpr int64_t kFast3HeaderBytes = 40960;
// optimiser step folded into the last backward kernel (w == nullptr: none, gradients are written instead): the part the
// kernels take by value (FusedUpdate below adds what only the host reads)
struct FusedUpdateK {
  float* w[TTEMB_MAX_CORES];
  float* st[TTEMB_MAX_CORES];   // Adagrad state / Adam's first moment, or null for SGD
  float lr, eps;
  // The learning rate as a device word (null: the by-value `lr` above, the arithmetic unchanged).  Every stepping kernel reads
  // it once, at its top (a uniform load), and no kernel writes it: a captured backward holds the ADDRESS, so the rate of a
  // replay is whatever the word holds then (include/ttemb.h "Device-resident learning rate").  16-byte aligned.
  const float* lr_dev;
  // Adam (v[0] != null; st = the first moment m, v = the second): the step words (see AdamPrep) and the hyper-parameters
  float* v[TTEMB_MAX_CORES];
  uint32_t* step;
  float b1, omb1, b2, omb2;     // beta, 1 - beta (each rounded once from the double)
  float wd;                     // weight decay; decoupled != 0: w -= lr wd w (AdamW), else g += wd w (Adam)
  int32_t decoupled;
  // A word of the workspace header the finalize kernel sets to 1 when the plan it ran on is POISONED and the host hears of
  // it (fault word present), else to 0 (sticky = 1: a later piece of the same call only ever sets it): the optimiser step
  // that follows a gradient-writing route (padded ranks, merged pairs, calls in pieces) reads it and leaves the parameters
  // alone -- what the fused finalize kernel does by itself.  Written by every grouped backward, so any content is valid.
  uint32_t* poison_out;
  int32_t sticky;
};
// ... and the host's view of it: + the betas in double, which only the launch that carries an AdamPrep needs (adam_prep_of)
struct FusedUpdate : FusedUpdateK {
  double beta1, beta2;
};
// Adam's step count lives on the device, in four 32-bit words the caller owns: [0] t, the steps applied so far; [1] t + 1,
// [2] 1 / (1 - b1^(t+1)) and [3] 1 / sqrt(1 - b2^(t+1)) as float bits -- the PENDING step.  One lane of a kernel that runs
// before the stepping kernel of the same call forms words 1-3 from word 0 (adam_prepare); every workgroup of the stepping
// kernel reads words 2-3 only, and its first thread commits word 0 = word 1 unless the step is skipped.  No workgroup reads
// a word that another workgroup of the same launch writes, so t advances exactly once per applied step, and a skipped step
// (w, m, v and t as they were) can be repeated.
struct AdamPrep {
  uint32_t* step;   // null: not an Adam call
  double b1, b2;
};
__device__ __forceinline__ void adam_prepare(const AdamPrep& a) {
  const uint32_t t = a.step[0] + 1u;
  double p1 = 1.0, p2 = 1.0, x1 = a.b1, x2 = a.b2;   // beta^t by squaring, in double (1 - b2^t is ~1e-3 t: fp32 would lose four digits)
  for (uint32_t n = t; n != 0u; n >>= 1) {
    if (n & 1u) { p1 *= x1; p2 *= x2; }
    x1 *= x1; x2 *= x2;
  }
  a.step[1] = t;
  a.step[2] = __float_as_uint((float)(1.0 / (1.0 - p1)));
  a.step[3] = __float_as_uint((float)(1.0 / sqrt(1.0 - p2)));
}
// what the stepping kernel holds per workgroup: lr / (1 - b1^t) and 1 / sqrt(1 - b2^t)
struct AdamCoef {
  float step_size, inv_sqrt_bc2;
};
// the rate a stepping kernel applies: the device word when there is one, else the by-value argument
__device__ __forceinline__ float step_lr(const float* __restrict__ lr_dev, float lr_arg) { return lr_dev != nullptr ? *lr_dev : lr_arg; }
// One element of the Adam / AdamW step (torch.optim.Adam / AdamW without amsgrad).  A zero denominator (v = 0 and eps = 0: an
// element that has never seen a gradient) leaves w alone instead of dividing 0 by 0.
__device__ __forceinline__ void adam_element(float& w, float& m, float& v, float g, const AdamCoef& c, float lr, float eps, float b1,
                                             float omb1, float b2, float omb2, float wd, int decoupled) {
  if (decoupled) w -= lr * wd * w; else g += wd * w;
  m = b1 * m + omb1 * g;
  v = b2 * v + omb2 * (g * g);
  const float denom = sqrtf(v) * c.inv_sqrt_bc2 + eps;
  if (denom > 0.f) w -= c.step_size * m / denom;
}
inline AdamPrep adam_prep_of(const FusedUpdate& u) {
  AdamPrep a;
  a.step = u.v[0] != nullptr ? u.step : nullptr;
  a.b1 = u.beta1;
  a.b2 = u.beta2;
  return a;
}
// A FusedUpdate is the one description of an optimiser step on the host as well: v[0] != null is Adam, else st[0] != null is
// Adagrad, else SGD; lr_dev or lr gives the rate.  The two builders below (ttemb_api.hip) are the only code that fills one from
// an entry point's arguments, and they make every check of those arguments (TTEMB_E_BADARG).  They fill everything but `w`
// and the poison word, which the body that runs the step sets.  `T`: the arrays the step takes (the table's cores; 1 for a flat
// step; 0 when the call is empty or its shape will be refused, then no array is read).
// ... from arguments by value: `kind` a TTEMB_STEP_*, `state` / `state2` the Adagrad state or Adam's moments, `hp` / `adam_step`
// Adam's hyper-parameters (they carry its lr and eps) and step words
int step_from_values(int32_t kind, int T, float lr, float eps, float* const* state, float* const* state2, const ttemb_adam_t* hp,
                     int32_t* adam_step, FusedUpdate* upd);
// ... from a descriptor, whose rate is a device word.  `flat` (a flat step): the arrays are the call's own arguments, the
// descriptor's are not looked at
struct FlatArrays {
  float* state;
  float* state2;
  int32_t* adam_step;
};
int step_from_descriptor(const ttemb_step_t* step, int T, const FlatArrays* flat, FusedUpdate* upd);
int step_arrays(const ttemb_shape_t* shape);   // the T of a lookup's step: the table's cores, 0 for a shape no call accepts
// The step of `T` arrays (upd.w / st / v [t], gradients g[t], n[t] floats, all 16-byte aligned) from gradients in memory: for
// Adam a one-lane launch that forms the pending step words first, then one stepping launch (ttemb_api.hip).  grad_scale
// multiplies Adam's gradients; skip: null, or a device word that, non-zero, leaves everything as it was
int run_step_arrays(const FusedUpdate& upd, const float* const* g, const long long* n, int T, float grad_scale, const uint32_t* skip,
                    hipStream_t st);

// where that word sits in the header: behind the epoch words and the banks of range counters (16 + 8 * 512 * 8 bytes)
constexpr int64_t kHeaderPoisonOffset = 16 + 8 * 512 * 8;
static_assert(kHeaderPoisonOffset + 8 <= kFast3HeaderBytes, "the poison word lies inside the header");
static_assert(kHeaderPoisonOffset == TTEMB_HEADER_POISON_OFFSET, "include/ttemb.h names the same offset");
int launch_backward_fast3(const DevShape& s, const CorePtrs& cores, const int64_t* indices,
                          const int64_t* rowidx, const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev,
                          int64_t B, const float* d_output, const CorePtrsMut& d_cores, void* ws,
                          int64_t ws_bytes, const void* plan, int64_t plan_bytes, hipStream_t st,
                          const FusedUpdate* update, void* header);

// a window of a longer id list (one table of a table-batched call): bags [bag0, bag0 + B) of `offsets`, bounds read on the device
bool fast3_window_fits(const DevShape& s, int64_t nnz, int64_t bags_total, int64_t B);
int64_t fast3_window_workspace_bytes(const DevShape& s, bool bwd, int64_t nnz);
int launch_forward_window_fast3(const DevShape& s, const CorePtrs& cores, const int64_t* indices, const int64_t* offsets,
                                int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, float* output, void* ws, int64_t ws_bytes,
                                hipStream_t st, void* header);
int launch_backward_window_fast3(const DevShape& s, const CorePtrs& cores, const int64_t* indices, const int64_t* offsets,
                                 int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, const float* d_output,
                                 const CorePtrsMut& d_cores, void* ws, int64_t ws_bytes, hipStream_t st, const FusedUpdate* update,
                                 void* header);

// small batches of a 3-core table (ttemb_small3.inc): one wavefront per bag, MFMA per id, no grouping; `offsets` required.
// The backward ADDS into d_cores (zeroed by the caller) with float atomics.
bool small3_supported(const DevShape& s);   // (includes the run-time-shape kernels of ttemb_rt3.inc)
bool rt3_supported(const DevShape& s);
bool small3_templated_shape(const DevShape& s);   // a per-bag shape with an instantiated template
bool fast3_wide(const DevShape& s);               // a shape of the wide-rank grouped chain
bool small3_only(const DevShape& s);   // a rank-sweep shape only these kernels are instantiated for
int launch_forward_small3(const DevShape& s, const CorePtrs& cores, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                          const int32_t* nnz_dev, int64_t B, float* output, hipStream_t st);
int launch_backward_small3(const DevShape& s, const CorePtrs& cores, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                           const int32_t* nnz_dev, int64_t B, const float* d_output, const CorePtrsMut& d_cores, hipStream_t st);

// grid of a deterministic kernel over `items` workgroups' worth of work, capped by ttemb_set_exact_grid (ttemb_exact.hip;
// the bag kernels of ttemb_bag.hip use it too)
namespace exact {
unsigned ex_grid(int64_t items);
}

// zero `bytes` (a multiple of 4) at `p` with a kernel on `st`.  Used instead of hipMemsetAsync everywhere: inside a
// captured HIP graph (ROCm 7.2) a memset node was seen to race the kernel node that follows it.
int launch_zero(void* p, size_t bytes, hipStream_t st, const char* what);

// ---------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------
// does the bag of position n hold exactly one id?  With `offsets` the answer comes from the bag
// lengths of the original id list; otherwise from the neighbouring rows of the live range.
__device__ __forceinline__ bool bag_is_single(const int64_t* __restrict__ rowidx,
                                              const int64_t* __restrict__ offsets, int64_t n, int64_t cnt,
                                              int64_t row) {
  if (offsets != nullptr) return offsets[row + 1] - offsets[row] == 1;
  return (n == 0 || rowidx[n - 1] != row) && (n + 1 >= cnt || rowidx[n + 1] != row);
}

// bag of position n: the last b with offsets[b] <= n  (tt_embeddings_cuda.cu:1349-1365 expands the same map)
__device__ __forceinline__ int64_t bag_of_position(const int64_t* __restrict__ offsets, int64_t B, int64_t n) {
  if (n < B) {   // the usual case: every bag holds one id
    const int64_t o0 = offsets[n], o1 = offsets[n + 1];
    if (o0 <= n && n < o1) return n;
  }
  int64_t lo = 0, hi = B;  // invariant: offsets[lo] <= n < offsets[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= n) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t live_count(int64_t nnz, const int32_t* nnz_dev) {
  if (nnz_dev == nullptr) return nnz;
  int64_t c = *nnz_dev;
  return c < nnz ? (c < 0 ? 0 : c) : nnz;
}

// The rank core of the stable partitions (the cache's, ttemb_drop_padding's) and of the distinct-id pass (ttemb_unique.hip):
// the number of flagged positions before this thread's, in the whole call -- the counts of the tiles before `block` (blockcnt,
// summed by wave 0: a few hundred coalesced loads) plus a ballot rank inside the tile.  A tile is one workgroup of kRankTile
// threads.  No waits between workgroups.  `wave_cnt` / `wave_ball` / `before_lds` are the caller's LDS (wave_ball may be
// null); `before_block` and `total` (flagged positions of this tile) come back too.
constexpr int kRankTile = 256;
__device__ __forceinline__ int64_t partition_rank(const int32_t* __restrict__ blockcnt, int64_t block, bool f, int* wave_cnt,
                                                  unsigned long long* wave_ball, int64_t* before_lds, int64_t& before_block,
                                                  int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) {
    int64_t v = 0;
    for (int64_t b0 = 0; b0 < block; b0 += 8 * kWave) {   // eight loads per lane in flight, then the sums
      int32_t c[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t b = b0 + k * kWave + lane;
        c[k] = b < block ? blockcnt[b] : 0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) v += c[k];
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
      const uint32_t lo_w = __shfl_down((uint32_t)v, d, kWave), hi_w = __shfl_down((uint32_t)((uint64_t)v >> 32), d, kWave);
      v += (int64_t)((uint64_t)lo_w | ((uint64_t)hi_w << 32));
    }
    if (lane == 0) *before_lds = v;
  }
  const unsigned long long ball = __ballot(f);
  if (lane == 0) {
    wave_cnt[wave] = __popcll(ball);
    if (wave_ball != nullptr) wave_ball[wave] = ball;
  }
  __syncthreads();
  before_block = *before_lds;
  int64_t before = before_block + __popcll(ball & ((1ull << lane) - 1ull));
  total = 0;
  for (int w = 0; w < kRankTile / kWave; ++w) {
    if (w < wave) before += wave_cnt[w];
    total += wave_cnt[w];
  }
  return before;
}

// id -> per-core row numbers (reference: FBTT/tt_embeddings_cuda.cu:796-802).
__device__ __forceinline__ void split_index(const DevShape& s, int64_t idx, int (&i)[TTEMB_MAX_CORES]) {
  // an id outside the table is clamped as a whole (to the first / last row), the rule of every kernel family, so a bad
  // id gives the same row whichever kernels a batch size selects
  const int64_t rows = (int64_t)s.L[0] * s.p[0];
  idx = idx < 0 ? 0 : (idx >= rows ? rows - 1 : idx);
#pragma unroll
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) {
    if (t < s.T) {
      int64_t d = idx / s.L[t];
      idx -= d * s.L[t];
      // ids beyond prod(p) would index past core 0; clamp so a bad id cannot fault
      i[t] = (int)(d < s.p[t] ? (d < 0 ? 0 : d) : s.p[t] - 1);
    } else {
      i[t] = 0;
    }
  }
}

}  // namespace ttemb
