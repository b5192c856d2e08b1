// extern "C" entry points of libttemb_hip.so (declared in include/ttemb.h).
// Argument checking, workspace carving and kernel-family dispatch live here; the
// kernels are in ttemb_generic.hip / ttemb_fast3.hip / ttemb_cache.hip.
#include "ttemb_common.h"
#include "ttemb_cache.h"

#include <dlfcn.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ttemb {

static thread_local char g_err[512] = "";
// process-wide on purpose: autograd runs backward on its own thread
static std::atomic<int> g_path{TTEMB_PATH_AUTO};

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return TTEMB_OK;
  return fail(TTEMB_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

int allow_big_lds(const void* kernel, size_t lds_bytes, LdsGate* gate, const char* what) {
  if (lds_bytes <= kLdsDefault) return TTEMB_OK;
  if (lds_bytes > kCuLds)
    return fail(TTEMB_E_UNSUPPORTED, "%s needs %lld bytes of LDS per workgroup, the CU has %lld", what, (long long)lds_bytes, (long long)kCuLds);
  int dev = 0;
  int rc = check_hip(hipGetDevice(&dev), "hipGetDevice");
  if (rc) return rc;
  const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t(1) << dev) : 0;
  if (bit && (gate->devices.load(std::memory_order_acquire) & bit)) return TTEMB_OK;
  rc = check_hip(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCuLds), what);
  if (rc == TTEMB_OK && bit) gate->devices.fetch_or(bit, std::memory_order_release);
  return rc;
}

int device_cus() {
  static std::atomic<int> cus[64];   // zero-initialised: "not asked yet"
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool slot = dev >= 0 && dev < 64;
  if (slot && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (slot) cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

int current_path() { return g_path.load(); }

// ---- device-side faults (a bounded wait of the grouping pass that ran out: report_fault in ttemb_fast3.hip) ----
// One pinned, device-visible host word per process, allocated by ttemb_init() (or the first ttemb_status()) -- an explicit
// call the host makes outside any stream capture, never by a lookup (the lookups allocate nothing) -- and never freed (its
// address is baked into captured graphs).  The kernel that gives up stores its reason there; every lookup entry point looks
// at it first (one atomic exchange on a host word, no synchronisation), so the fault surfaces as TTEMB_E_HIP on the next
// call the host makes after the store has landed -- at the latest on the one after a synchronisation -- and is consumed by
// exactly one caller.  The error therefore names an EARLIER call: the call that reports it has not been started.  The
// results of the faulted call itself are NaN (poisoned plan), whether or not anyone asks.
static std::atomic<uint32_t*> g_fault_host{nullptr};
static std::atomic<uint32_t*> g_fault_dev{nullptr};
static std::atomic<int> g_fault_state{0};   // 0 = not tried, 1 = being set up, 2 = ready, 3 = not available

// the lookups' view: the word's device address when it exists, else null (that call reports through its NaN results only)
uint32_t* fault_word(hipStream_t) {
  return g_fault_state.load(std::memory_order_acquire) == 2 ? g_fault_dev.load(std::memory_order_relaxed) : nullptr;
}

// ttemb_init / ttemb_status: create the word (once per process; a call that loses the race goes without)
int fault_word_init() {
  int state = g_fault_state.load(std::memory_order_acquire);
  if (state == 2) return TTEMB_OK;
  if (state == 3) return fail(TTEMB_E_HIP, "no pinned host memory for the device-fault word: expired device-side waits are reported through NaN results only");
  int expect = 0;
  if (!g_fault_state.compare_exchange_strong(expect, 1)) return TTEMB_OK;   // another thread is setting it up
  void* host = nullptr;
  void* dev = nullptr;
  if (hipHostMalloc(&host, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess || host == nullptr ||
      hipHostGetDevicePointer(&dev, host, 0) != hipSuccess || dev == nullptr) {
    (void)hipGetLastError();
    g_fault_state.store(3, std::memory_order_release);
    return fail(TTEMB_E_HIP, "no pinned host memory for the device-fault word: expired device-side waits are reported through NaN results only");
  }
  memset(host, 0, 64);
  g_fault_host.store(reinterpret_cast<uint32_t*>(host), std::memory_order_relaxed);
  g_fault_dev.store(reinterpret_cast<uint32_t*>(dev), std::memory_order_relaxed);
  g_fault_state.store(2, std::memory_order_release);
  return TTEMB_OK;
}

int pending_device_fault() {
  if (g_fault_state.load(std::memory_order_acquire) != 2) return TTEMB_OK;
  uint32_t* w = g_fault_host.load(std::memory_order_relaxed);
  if (__atomic_load_n(w, __ATOMIC_RELAXED) == 0u) return TTEMB_OK;   // (the usual case: one plain read)
  const uint32_t code = __atomic_exchange_n(w, 0u, __ATOMIC_ACQ_REL);   // consumed by exactly one caller; a report landing now stays for the next
  if (code == 0u) return TTEMB_OK;
  return fail(TTEMB_E_HIP,
              "an EARLIER grouped lookup of this process gave up waiting on the device (%s): the rows / gradients of that call are "
              "NaN, not wrong numbers; a fused SGD / Adagrad backward on such a plan left the parameters and the optimizer state "
              "untouched (dense gradients are NaN).  The GPU is shared or throttled beyond what the grouping pass tolerates.  The "
              "call that returns this error was not started; discard the faulted step's outputs and run it again",
              code == 1u ? "range counter take-over in the decode step"
                         : (code == 3u ? "overflow area of the decode step exhausted" : "look-back of the place step"));
}

static std::atomic<bool> g_prof_on{false};
// slots: 0 forward chain kernel | 1 all backward chain kernels | 2 backward chunk kernel | 3 grouping pass (+ prefix products) |
//        4 cache probe pass (lookup, + LFU update when fused) | 5 partition scatter | 6 cached-row gather | 7 cached-row update |
//        8 group epilogue kernel | 9 finalize kernel
constexpr int kProfSlots = 10;
static hipEvent_t g_prof_ev[kProfSlots][2] = {};
static std::atomic<bool> g_prof_valid[kProfSlots] = {};

void profile_begin(int which, hipStream_t st) {
  if (!g_prof_on) return;
  for (int i = 0; i < 2; ++i)
    if (g_prof_ev[which][i] == nullptr && hipEventCreate(&g_prof_ev[which][i]) != hipSuccess) return;
  g_prof_valid[which] = hipEventRecord(g_prof_ev[which][0], st) == hipSuccess;
}

void profile_end(int which, hipStream_t st) {
  if (!g_prof_on || !g_prof_valid[which]) return;
  g_prof_valid[which] = hipEventRecord(g_prof_ev[which][1], st) == hipSuccess;
}

int make_dev_shape(const ttemb_shape_t* s, DevShape* out) {
  if (s == nullptr) return fail(TTEMB_E_BADARG, "shape is null");
  if (s->T < 2 || s->T > TTEMB_MAX_CORES)
    return fail(TTEMB_E_BADARG, "T=%d: the layer supports 2..4 cores", s->T);
  DevShape d;
  memset(&d, 0, sizeof(d));
  d.T = s->T;
  if (s->R[0] != 1 || s->R[s->T] != 1) return fail(TTEMB_E_BADARG, "R[0] and R[T] must be 1");
  long long D = 1;
  for (int t = 0; t < s->T; ++t) {
    if (s->p[t] <= 0 || s->q[t] <= 0 || s->R[t] <= 0 || s->R[t + 1] <= 0)
      return fail(TTEMB_E_BADARG, "non-positive factor at core %d", t);
    d.p[t] = s->p[t];
    d.q[t] = s->q[t];
    d.R[t] = s->R[t];
    D *= s->q[t];
    if (D > (1 << 20)) return fail(TTEMB_E_BADARG, "embedding_dim too large");
  }
  d.R[s->T] = 1;
  if (D % 4 != 0) return fail(TTEMB_E_BADARG, "embedding_dim %lld must be a multiple of 4", D);
  d.D = (int)D;
  long long L = 1;
  for (int t = s->T - 1; t >= 0; --t) {
    d.L[t] = L;
    if (L > (1ll << 62) / d.p[t]) return fail(TTEMB_E_BADARG, "prod(p) overflows");
    L *= d.p[t];
  }
  long long Q = 1;
  int pm = 0;
  for (int t = 0; t < s->T; ++t) {
    Q *= d.q[t];
    long long rl = (long long)d.R[t] * d.q[t] * d.R[t + 1];
    long long pl = Q * d.R[t + 1];
    if (rl > (1 << 24) || pl > (1 << 24)) return fail(TTEMB_E_BADARG, "core row too large");
    d.row_len[t] = (int)rl;
    d.part_len[t] = (int)pl;
    if (t + 1 < s->T && d.part_len[t] > pm) pm = d.part_len[t];
  }
  d.part_max = pm;
  *out = d;
  return TTEMB_OK;
}

static int64_t grad_scratch_bytes(const DevShape& s) {
  int64_t b = 0;
  for (int t = 0; t < s.T; ++t) b += align256((int64_t)s.p[t] * s.row_len[t] * 4);
  return b;
}

// have_offsets: the call carries its bag boundaries (size queries assume so) -- what a call past one 32-bit row window needs
// to run on the grouped path, piece by piece
static bool use_fast3(const DevShape& s, int64_t nnz, int64_t B, bool have_offsets = true) {
  const int path = current_path();
  if (path == TTEMB_PATH_GENERIC || path == TTEMB_PATH_PER_BAG || !fast3_supported(s)) return false;
  if (!fast3_fits(s, nnz, B) && !(have_offsets && fast3_fits_in_pieces(s, nnz, B))) return false;
  return path == TTEMB_PATH_FAST3 || fast3_pays(s, nnz);
}

// a 3-core shape (p, q, ranks r1 r2), through make_dev_shape; false when it has none (a core row too large)
static bool shape3(const int p[3], const int q[3], int r1, int r2, DevShape* out) {
  ttemb_shape_t t;
  memset(&t, 0, sizeof(t));
  t.T = 3;
  for (int k = 0; k < 3; ++k) { t.p[k] = p[k]; t.q[k] = q[k]; }
  t.R[0] = 1; t.R[1] = r1; t.R[2] = r2; t.R[3] = 1;
  return make_dev_shape(&t, out) == TTEMB_OK;
}

// ---------------------------------------------------------------------------------
// 4-core tables on the grouped path.  row = G0[i0].G1[i1].G2[i2].G3[i3] is a 3-core row over the table
// (p0 p1, p2, p3) with the VIRTUAL first core V[(i0, i1)] = G0[i0].G1[i1]  (q0 q1 x r2) -- or over (p0, p1, p2 p3)
// with the virtual last core V[(i2, i3)] = G2[i2].G3[i3]: the id digits are the same (i0 p1 + i1 is the leading,
// i2 p3 + i3 the trailing digit of the 3-core split), so the grouped kernels run unchanged on (V, G2, G3) /
// (G0, G1, V) when the merged (q, ranks) is one of their shapes.  V is rebuilt from the cores per call (a few
// thousand small GEMMs), its gradient is split back:  dA[ia] = sum_ib dV[ia,ib].B[ib]^T, dB[ib] = sum_ia A[ia]^T.dV[ia,ib]
// -- two tiny kernels around the 3-core path.
// ---------------------------------------------------------------------------------
struct Merged4 {
  bool on;
  bool per_bag;         // the 3-core view runs on the per-bag kernels (no grouped shape fits / the batch is small)
  int a;                // the merged pair: cores a and a + 1 (0: the first two, 2: the last two)
  DevShape s3;          // the 3-core view
  int64_t v_bytes;      // bytes of V (and of dV), 256-aligned
  // V[(ia, ib)] = A[ia] (rows x K) . Bm[ib] (K x n): the two cores as plain matrices
  int pa, pb, rows, K, n;
};

static bool view3(const DevShape& s, int a, DevShape* out) {   // the 3-core shape with cores a, a + 1 merged
  const long long pp = (long long)s.p[a] * s.p[a + 1], qq = (long long)s.q[a] * s.q[a + 1];
  if (pp > 0x7fffffffll || qq > 1024) return false;
  int p[3], q[3], R[3], k = 0;
  for (int t = 0; t < 4; ++t) {
    if (t == a + 1) continue;
    p[k] = t == a ? (int)pp : s.p[t];
    q[k] = t == a ? (int)qq : s.q[t];
    R[k] = s.R[t];
    ++k;
  }
  return shape3(p, q, R[1], R[2], out);
}

// first choice: merge the first two cores (small virtual core, the per-id operand stays the last core); else the
// last two (q = 5,5,2,2: the virtual last core has p2 p3 rows of r2 q2 q3 floats, its dG slabs grow with it)
// 2-core tables ride on the same 3-core kernels: row = G0[i0].G1[i1] = G0[i0].I.G1[i1] is a 3-core row over
// (p0, 1, p1) with q = (q0, 1, q1), ranks (r1, r1) and the r1 x r1 identity as the only row of a VIRTUAL middle core
// (a == -1 below).  The groups are the values of i0, the "prefix product" of a group is its G0 row, the gradient of
// the identity is computed and dropped.  (FBTT/tt_embeddings_cuda.cu:757-779, :81-117 are the reference's 2-core forms.)
static bool view_lifted2(const DevShape& s, DevShape* out) {
  const int p[3] = {s.p[0], 1, s.p[1]}, q[3] = {s.q[0], 1, s.q[1]};
  return shape3(p, q, s.R[1], s.R[1], out);
}

// per_bag_ok: the call could run on the per-bag kernels (ids + offsets, no row index; sizing queries pass true): a 2- or
// 4-core table whose 3-core view has no grouped shape, or whose batch is below the grouped path's crossover, then rides on
// the per-bag MFMA kernels (templated or run-time shape) through the same virtual core instead of the scalar kernels.
static Merged4 merge_first_two(const DevShape& s, int64_t nnz, int64_t B, bool per_bag_ok = false, bool have_offsets = true) {
  Merged4 m;
  memset(&m, 0, sizeof(m));
  const int path = current_path();
  if (path == TTEMB_PATH_GENERIC) return m;
  per_bag_ok = per_bag_ok && (path == TTEMB_PATH_AUTO || path == TTEMB_PATH_PER_BAG);
  if (s.T == 2) {
    DevShape d;
    if (!view_lifted2(s, &d)) return m;
    const bool f3 = use_fast3(d, nnz, B, have_offsets);
    if (f3 || (per_bag_ok && small3_supported(d))) {
      m.on = true;
      m.per_bag = !f3;
      m.a = -1;
      m.s3 = d;
      m.K = s.R[1];
      m.v_bytes = align256((long long)m.K * m.K * 4);
    }
    return m;
  }
  if (s.T != 4) return m;
  auto fill = [&](int a, const DevShape& d, bool per_bag) {
    m.on = true;
    m.per_bag = per_bag;
    m.a = a;
    m.s3 = d;
    m.pa = s.p[a]; m.pb = s.p[a + 1];
    m.rows = s.R[a] * s.q[a];          // A[ia] is (R_a q_a) x R_{a+1}
    m.K = s.R[a + 1];
    m.n = s.q[a + 1] * s.R[a + 2];     // Bm[ib] is R_{a+1} x (q_{a+1} R_{a+2})
    m.v_bytes = align256((long long)m.pa * m.pb * m.rows * m.n * 4);
  };
  for (int a = 0; a <= 2; a += 2) {
    DevShape d;
    if (!view3(s, a, &d) || !use_fast3(d, nnz, B, have_offsets)) continue;
    if (a == 2 && (long long)d.p[2] * d.row_len[2] * 4 > (4ll << 20)) continue;   // virtual last core: at most 4 MB (its slabs)
    fill(a, d, false);
    return m;
  }
  if (per_bag_ok) {   // first pair merged: the per-id operand stays the last core
    // The virtual core is REBUILT by every forward and split back (over all p0 p1 rows, gradients zero-filled) by every
    // backward, whatever nnz is: O(p0 p1 row) next to the scalar kernels' O(nnz).  The run scripts' 4-core tables have
    // 3 000-row virtual cores (0.4-1.5 MB: a few microseconds); a table with a large first pair takes this view only when
    // the batch amortises the rebuild -- at least one id per 16 rows of V -- or V is small anyway (<= 4 MB).  A conservative
    // gate, not a measured crossover (no script trains such a table).
    DevShape d;
    if (view3(s, 0, &d) && small3_supported(d)) {
      const long long v_rows = (long long)s.p[0] * s.p[1], v_bytes = v_rows * d.row_len[0] * 4;
      if (v_bytes <= (256ll << 20) && (v_bytes <= (4ll << 20) || nnz * 16 >= v_rows)) fill(0, d, true);
    }
  }
  return m;
}

// ---------------------------------------------------------------------------------
// Ranks off the instantiated list on the grouped path: zero-padded cores.
// A 3-core table with ranks (r1, r2) IS the table with ranks (R, R), R >= r1, r2, whose cores carry zeros in the added rank
// positions: every row is the same number for number (the added terms are products with zero), and the gradient with respect
// to an original entry is the same sum.  So any rank in [2, 256] -- tuning_SAGE.py:213 searches exactly that interval --
// rides on the grouped MFMA kernels of the next instantiated rank of its q shape (8 / 16 / 32; 64 / 128 / 256 for the wide
// chain): per call the cores are copied into padded form (a few hundred KB to a few MB: one small launch), the grouped
// kernels run on the padded table, and the backward keeps the original sub-block of the padded gradient.  The extra flops
// ((R / r)^2 on the first contraction) are small change next to what the per-bag kernels pay at large batches (no prefix
// reuse, float atomics per id): rank 12 at 65 536 ids -- 0.48 ms per-bag -- runs like rank 16.
// ---------------------------------------------------------------------------------
struct Padded3 {
  bool on;
  DevShape sp;               // the padded 3-core shape
  int64_t core_bytes[3];     // bytes of every padded core, 256-aligned
  int64_t cores_total;       // their sum
};

static Padded3 pad_ranks(const DevShape& s, int64_t nnz, int64_t B, bool have_offsets) {
  Padded3 pd;
  memset(&pd, 0, sizeof(pd));
  const int path = current_path();
  if (s.T != 3 || path == TTEMB_PATH_GENERIC || path == TTEMB_PATH_PER_BAG || fast3_supported(s)) return pd;
  const int need = s.R[1] > s.R[2] ? s.R[1] : s.R[2];
  for (int R : {8, 16, 32, 64, 128, 256}) {
    DevShape d;
    if (R < need || !shape3(s.p, s.q, R, R, &d) || !fast3_supported(d)) continue;
    if (!use_fast3(d, nnz, B, have_offsets)) return pd;   // (a larger rank of the list would pay even later)
    pd.on = true;
    pd.sp = d;
    for (int k = 0; k < 3; ++k) {
      pd.core_bytes[k] = align256((int64_t)d.p[k] * d.row_len[k] * 4);
      pd.cores_total += pd.core_bytes[k];
    }
    return pd;
  }
  return pd;
}

// ---------------------------------------------------------------------------------
// The route of a lookup: which kernels run, on which 3-core shape, decided once per call (and per size query) from the shape,
// the size, what the call carries and the forced path.  The kinds are disjoint by shape: GROUPED is a 3-core table of an
// instantiated grouped shape, PADDED one whose ranks are padded up to one, MERGED a 2- or 4-core table on a 3-core view;
// PER_BAG and SCALAR take what is left.
// ---------------------------------------------------------------------------------
enum RouteKind { kGrouped, kMerged, kPadded, kPerBag, kScalar };
struct Route {
  RouteKind kind;
  DevShape s3;     // the shape the 3-core call runs on: the table's own, the merged view (m4.s3) or the padded table (pd.sp)
  bool grouped;    // the 3-core call runs on the grouped kernels (else on the per-bag or the scalar ones)
  Merged4 m4;      // kMerged: the virtual core
  Padded3 pd;      // kPadded: the padded cores
};

// have_offsets: the ids come with their bag boundaries (what a call past one row window needs to run in pieces); per_bag_ok:
// ... and without a row index (what the per-bag kernels need); views_ok = false: neither the grouped kernels nor a view (an
// empty forward)
static Route route_of(const DevShape& ds, int64_t nnz, int64_t B, bool have_offsets, bool per_bag_ok, bool views_ok = true) {
  Route r;
  memset(&r, 0, sizeof(r));
  r.kind = kScalar;
  r.s3 = ds;
  const int path = current_path();
  if (views_ok && use_fast3(ds, nnz, B, have_offsets)) {
    r.kind = kGrouped;
    r.grouped = true;
  } else if (views_ok && (r.m4 = merge_first_two(ds, nnz, B, per_bag_ok, have_offsets)).on) {
    r.kind = kMerged;
    r.s3 = r.m4.s3;
    r.grouped = !r.m4.per_bag;
  } else if (views_ok && (r.pd = pad_ranks(ds, nnz, B, have_offsets)).on) {
    r.kind = kPadded;
    r.s3 = r.pd.sp;
    r.grouped = true;
  } else if (per_bag_ok && (path == TTEMB_PATH_AUTO || path == TTEMB_PATH_PER_BAG) && small3_supported(ds)) {
    r.kind = kPerBag;   // small batches: one wavefront per bag, MFMA per id (ttemb_small3.inc) instead of the scalar kernels
  }
  return r;
}

static const char* view_name(const Route& r) { return r.kind == kMerged ? "merged core" : "padded cores"; }

// what a view keeps in front of the grouped kernels' region: V / the padded cores, and (backward) their gradients behind them
static int64_t view_bytes(const Route& r, bool bwd) {
  const int64_t one = r.kind == kMerged ? r.m4.v_bytes : (r.kind == kPadded ? r.pd.cores_total : 0);
  return bwd ? 2 * one : one;
}

// a lookup's workspace: [header | gradient scratch (backward) | row slot | view_bytes | the grouped kernels' region]
static int64_t lookup_workspace_bytes(const Route& r, const DevShape& ds, int32_t op, int64_t nnz, int64_t B) {
  const bool bwd = op == TTEMB_OP_BACKWARD;
  return kFast3HeaderBytes + (bwd ? grad_scratch_bytes(ds) : 0) + align256(nnz * 8) + view_bytes(r, bwd) +
         (r.grouped ? fast3_workspace_bytes(r.s3, op, nnz, B) : 0);
}

// dst[row][a][j][b] (ranks Ra x Rb) = src[row][a][j][b] inside the original ranks (ra x rb), 0 outside -- and back
struct PadJob {
  const float* src[3];
  float* dst[3];
  int p[3], q[3], ra[3], rb[3], Ra[3], Rb[3];
};
__global__ __launch_bounds__(256) void pad_cores_kernel(PadJob j) {
  const int t = blockIdx.y;
  const long long n = (long long)j.p[t] * j.Ra[t] * j.q[t] * j.Rb[t];
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int b = (int)(e % j.Rb[t]);
    long long r = e / j.Rb[t];
    const int jj = (int)(r % j.q[t]);
    r /= j.q[t];
    const int a = (int)(r % j.Ra[t]);
    const long long row = r / j.Ra[t];
    j.dst[t][e] = (a < j.ra[t] && b < j.rb[t]) ? j.src[t][((row * j.ra[t] + a) * j.q[t] + jj) * j.rb[t] + b] : 0.f;
  }
}
// the original sub-block of a padded gradient: src is padded (Ra x Rb), dst original (ra x rb)
__global__ __launch_bounds__(256) void unpad_cores_kernel(PadJob j) {
  const int t = blockIdx.y;
  const long long n = (long long)j.p[t] * j.ra[t] * j.q[t] * j.rb[t];
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int b = (int)(e % j.rb[t]);
    long long r = e / j.rb[t];
    const int jj = (int)(r % j.q[t]);
    r /= j.q[t];
    const int a = (int)(r % j.ra[t]);
    const long long row = r / j.ra[t];
    j.dst[t][e] = j.src[t][((row * j.Ra[t] + a) * j.q[t] + jj) * j.Rb[t] + b];
  }
}
static PadJob pad_job(const DevShape& s, const Padded3& pd) {
  PadJob j;
  memset(&j, 0, sizeof(j));
  for (int t = 0; t < 3; ++t) {
    j.p[t] = s.p[t]; j.q[t] = s.q[t];
    j.ra[t] = s.R[t]; j.rb[t] = s.R[t + 1];
    j.Ra[t] = pd.sp.R[t]; j.Rb[t] = pd.sp.R[t + 1];
  }
  return j;
}
// padded copies of the cores at `buf` (pd.cores_total bytes); *cp3 receives their pointers
static int build_padded_cores(const DevShape& s, const Padded3& pd, const CorePtrs& cp, char* buf, CorePtrs* cp3, hipStream_t st) {
  PadJob j = pad_job(s, pd);
  memset(cp3, 0, sizeof(*cp3));
  int64_t off = 0, most = 0;
  for (int t = 0; t < 3; ++t) {
    j.src[t] = cp.c[t];
    j.dst[t] = reinterpret_cast<float*>(buf + off);
    cp3->c[t] = j.dst[t];
    off += pd.core_bytes[t];
    const int64_t n = (int64_t)pd.sp.p[t] * pd.sp.row_len[t];
    most = n > most ? n : most;
  }
  int64_t blocks = (most + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(pad_cores_kernel, dim3((unsigned)blocks, 3), dim3(256), 0, st, j);
  return check_hip(hipGetLastError(), "pad_cores_kernel");
}
static int unpad_grads(const DevShape& s, const Padded3& pd, const CorePtrsMut& padded, const CorePtrsMut& dst, hipStream_t st) {
  PadJob j = pad_job(s, pd);
  int64_t most = 0;
  for (int t = 0; t < 3; ++t) {
    j.src[t] = padded.c[t];
    j.dst[t] = dst.c[t];
    const int64_t n = (int64_t)s.p[t] * s.row_len[t];
    most = n > most ? n : most;
  }
  int64_t blocks = (most + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(unpad_cores_kernel, dim3((unsigned)blocks, 3), dim3(256), 0, st, j);
  return check_hip(hipGetLastError(), "unpad_cores_kernel");
}

// V[(ia, ib)] = A[ia] (rows x K) . Bm[ib] (K x n): one workgroup per pair
__global__ __launch_bounds__(256) void merge_pair_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int pb, int rows,
                                                         int K, int n, float* __restrict__ V) {
  const int pair = blockIdx.x, ia = pair / pb, ib = pair - ia * pb;
  const float* a = A + (size_t)ia * rows * K;
  const float* b = Bm + (size_t)ib * K * n;
  float* v = V + (size_t)pair * rows * n;
  for (int e = threadIdx.x; e < rows * n; e += 256) {
    const int r = e / n, c = e - r * n;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(a[r * K + k], b[k * n + c], acc);
    v[e] = acc;
  }
}

// `outs` (< 128) outputs of `terms` products each: 256 / (outs rounded up to a power of two) threads share an output
template <typename F>
__device__ __forceinline__ void sum_terms_few(int outs, int terms, float* dst, float* red, F term) {
  const int tid = threadIdx.x;
  int lanes = 256;
  for (int o2 = 1; o2 < outs; o2 <<= 1) lanes >>= 1;
  const int o = tid / lanes, l = tid - o * lanes;
  float acc = 0.f;
  if (o < outs)
    for (int k = l; k < terms; k += lanes) acc += term(o, k);
  red[tid] = acc;
  __syncthreads();
  for (int w = lanes >> 1; w > 0; w >>= 1) {
    if (l < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (l == 0 && o < outs) dst[o] = red[tid];
}

// grid (pa + pb, K): workgroup (ia, k) sums dA[ia][:, k] = sum over ib of dV[ia,ib] . Bm[ib][k, :]^T, workgroup (pa + ib, k)
// sums dBm[ib][k, :] = sum over ia of A[ia][:, k]^T . dV[ia,ib]   (one column / row of K per workgroup: the sums are short
// but there are only pa + pb of each kind, so they are spread over K times as many workgroups)
__global__ __launch_bounds__(256) void split_pair_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                         const float* __restrict__ dV, int pa, int pb, int rows, int K, int n,
                                                         float* __restrict__ dA, float* __restrict__ dBm) {
  __shared__ float red[256];
  __shared__ float outv[256];
  const int k = blockIdx.y;
  if ((int)blockIdx.x < pa) {
    const int ia = blockIdx.x;
    for (int r0 = 0; r0 < rows; r0 += 127) {   // outputs r, at most 127 per pass
      const int nr = rows - r0 < 127 ? rows - r0 : 127;
      sum_terms_few(nr, pb * n, outv, red, [&](int o, int t) {
        const int r = r0 + o, ib = t / n, c = t - ib * n;
        return dV[((size_t)ia * pb + ib) * rows * n + r * n + c] * Bm[((size_t)ib * K + k) * n + c];
      });
      __syncthreads();
      for (int o = threadIdx.x; o < nr; o += 256) dA[((size_t)ia * rows + r0 + o) * K + k] = outv[o];
      __syncthreads();
    }
  } else {
    const int ib = blockIdx.x - pa;
    for (int c0 = 0; c0 < n; c0 += 127) {
      const int nc = n - c0 < 127 ? n - c0 : 127;
      sum_terms_few(nc, pa * rows, outv, red, [&](int o, int t) {
        const int c = c0 + o, ia = t / rows, r = t - ia * rows;
        return A[((size_t)ia * rows + r) * K + k] * dV[((size_t)ia * pb + ib) * rows * n + r * n + c];
      });
      __syncthreads();
      for (int o = threadIdx.x; o < nc; o += 256) dBm[((size_t)ib * K + k) * n + c0 + o] = outv[o];
      __syncthreads();
    }
  }
}

__global__ void identity_core_kernel(float* __restrict__ V, int K) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < K * K) V[e] = (e / K == e % K) ? 1.f : 0.f;
}

static int build_merged_core(const Merged4& m, const CorePtrs& cp, float* V, hipStream_t st) {
  if (m.a < 0) {   // the lifted 2-core table: the virtual middle core is the identity
    hipLaunchKernelGGL(identity_core_kernel, dim3((unsigned)((m.K * m.K + 255) / 256)), dim3(256), 0, st, V, m.K);
    return check_hip(hipGetLastError(), "identity_core_kernel");
  }
  hipLaunchKernelGGL(merge_pair_kernel, dim3((unsigned)(m.pa * m.pb)), dim3(256), 0, st, cp.c[m.a], cp.c[m.a + 1], m.pb, m.rows,
                     m.K, m.n, V);
  return check_hip(hipGetLastError(), "merge_pair_kernel");
}

// the 3-core operand (or gradient) lists of a merged table: V (dV) in the place of the pair (the identity's gradient is dropped)
template <class Ptrs>
static void merged_cores(const Merged4& m, const Ptrs& cp, float* V, Ptrs* c3) {
  memset(c3, 0, sizeof(*c3));
  if (m.a < 0) { c3->c[0] = cp.c[0]; c3->c[1] = V; c3->c[2] = cp.c[1]; }
  else if (m.a == 0) { c3->c[0] = V; c3->c[1] = cp.c[2]; c3->c[2] = cp.c[3]; }
  else          { c3->c[0] = cp.c[0]; c3->c[1] = cp.c[1]; c3->c[2] = V; }
}

// the prologue of a route: V (the merged pair, or the lifted table's identity) / the padded cores at `buf`; *c3: the operands of
// the 3-core call.  build = false (the id-only half of a forward): the operands' places only, nothing launched
static int build_view(const Route& r, const DevShape& ds, const CorePtrs& cp, char* buf, bool build, CorePtrs* c3, hipStream_t st) {
  *c3 = cp;
  if (r.kind == kMerged) {
    merged_cores(r.m4, cp, reinterpret_cast<float*>(buf), c3);
    return build ? build_merged_core(r.m4, cp, reinterpret_cast<float*>(buf), st) : TTEMB_OK;
  }
  if (r.kind != kPadded) return TTEMB_OK;
  if (build) return build_padded_cores(ds, r.pd, cp, buf, c3, st);
  memset(c3, 0, sizeof(*c3));
  return TTEMB_OK;
}

__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n && (reinterpret_cast<uintptr_t>(p + i) & 15) == 0) {
      *reinterpret_cast<uint4*>(p + i) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (size_t j = i; j < n && j < i + 4; ++j) p[j] = 0u;
    }
  }
}

struct ZeroSegs {
  uint32_t* p[TTEMB_MAX_CORES];
  size_t n[TTEMB_MAX_CORES];   // words
};

__global__ void zero_segments_kernel(ZeroSegs z, int T) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int t = 0; t < T; ++t)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < z.n[t]; i += stride) z.p[t][i] = 0u;
}

int launch_zero_cores(const DevShape& s, const CorePtrsMut& d_cores, hipStream_t st) {
  ZeroSegs z;
  size_t most = 0;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) {
    z.p[t] = t < s.T ? reinterpret_cast<uint32_t*>(d_cores.c[t]) : nullptr;
    z.n[t] = t < s.T ? (size_t)s.p[t] * s.row_len[t] : 0;
    most = z.n[t] > most ? z.n[t] : most;
  }
  if (most == 0) return TTEMB_OK;
  const size_t blocks = (most + 255) / 256;
  hipLaunchKernelGGL(zero_segments_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, z, s.T);
  return check_hip(hipGetLastError(), "zero d_cores");
}

int launch_zero(void* p, size_t bytes, hipStream_t st, const char* what) {
  if (bytes == 0) return TTEMB_OK;
  const size_t n = bytes / 4;
  size_t blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint32_t*>(p), n);
  return check_hip(hipGetLastError(), what);
}

// rows whose bag length is not 1 must be zero before the lookups accumulate into them
__global__ void zero_rows_kernel(const int64_t* __restrict__ offsets, int64_t B, int D,
                                 float* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (offsets[b + 1] - offsets[b] == 1) return;
  float4* o = reinterpret_cast<float4*>(out + b * D);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c * 4 < D; ++c) o[c] = z;
}

__global__ void sgd_step_kernel(float* __restrict__ w, const float* __restrict__ g, int64_t n, float lr_arg, const float* __restrict__ lr_dev,
                                const float* __restrict__ skip) {
  // (ttemb_sgd_step_guarded: some rank's gradient came from a poisoned plan.  The word is tested BIT-wise: an all-reduced float
  //  count (k.0f) and the uint32 poison word of a workspace header (1) both read non-zero, +0.0f and 0u both zero)
  if (skip != nullptr && *reinterpret_cast<const uint32_t*>(skip) != 0u) return;
  const float lr = step_lr(lr_dev, lr_arg);
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    float4 wv = *reinterpret_cast<float4*>(w + i);
    const float4 gv = *reinterpret_cast<const float4*>(g + i);
    wv.x -= lr * gv.x; wv.y -= lr * gv.y; wv.z -= lr * gv.z; wv.w -= lr * gv.w;
    *reinterpret_cast<float4*>(w + i) = wv;
  } else {
    for (; i < n; ++i) w[i] -= lr * g[i];
  }
}

__global__ void adagrad_step_kernel(float* __restrict__ w, float* __restrict__ st,
                                    const float* __restrict__ g, int64_t n, float lr_arg, const float* __restrict__ lr_dev, float eps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float lr = step_lr(lr_dev, lr_arg);
  const float gv = g[i];
  const float s2 = st[i] + gv * gv;
  st[i] = s2;
  w[i] -= lr * gv / (sqrtf(s2) + eps);
}

struct Seg3 {
  float* w[TTEMB_MAX_CORES];
  float* st[TTEMB_MAX_CORES];
  const float* g[TTEMB_MAX_CORES];
  long long n[TTEMB_MAX_CORES];
};

// Adam's part of the step kernel's arguments (v[0] == null: not Adam; st of the Seg3 is the first moment)
struct AdamSeg {
  float* v[TTEMB_MAX_CORES];
  uint32_t* step;
  float b1, omb1, b2, omb2, wd, grad_scale;
  int32_t decoupled;
};

__global__ void adam_prepare_kernel(AdamPrep a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) adam_prepare(a);
}

// one launch for every core: blockIdx.y selects the core
// `skip`: the poison word a grouped backward of this call left in the workspace header (FusedUpdate::poison_out), or null
// `lr_dev`: the rate as a device word (null: `lr_arg`), read once per thread at the top
__global__ void fused_step_kernel(Seg3 seg, float lr_arg, const float* __restrict__ lr_dev, float eps, int adagrad,
                                  const uint32_t* __restrict__ skip, AdamSeg ad) {
  if (skip != nullptr && *skip != 0u) return;   // the gradients are NaN and the host hears of it: parameters stay as they are
  const float lr = step_lr(lr_dev, lr_arg);
  const int t = blockIdx.y;
  float* __restrict__ w = seg.w[t];
  const float* __restrict__ g = seg.g[t];
  const long long n = seg.n[t];
  if (ad.v[0] != nullptr) {   // Adam / AdamW on the pending step words (adam_prepare_kernel ran before); the first thread commits t
    AdamCoef ac;
    ac.step_size = lr * __uint_as_float(ad.step[2]);
    ac.inv_sqrt_bc2 = __uint_as_float(ad.step[3]);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ad.step[0] = ad.step[1];
    float* __restrict__ m = seg.st[t];
    float* __restrict__ v = ad.v[t];
    const float gs = ad.grad_scale;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
      if (i + 3 < n) {
        float4 wv = *reinterpret_cast<float4*>(w + i), mv = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
        const float4 gv = *reinterpret_cast<const float4*>(g + i);
        adam_element(wv.x, mv.x, vv.x, gv.x * gs, ac, lr, eps, ad.b1, ad.omb1, ad.b2, ad.omb2, ad.wd, ad.decoupled);
        adam_element(wv.y, mv.y, vv.y, gv.y * gs, ac, lr, eps, ad.b1, ad.omb1, ad.b2, ad.omb2, ad.wd, ad.decoupled);
        adam_element(wv.z, mv.z, vv.z, gv.z * gs, ac, lr, eps, ad.b1, ad.omb1, ad.b2, ad.omb2, ad.wd, ad.decoupled);
        adam_element(wv.w, mv.w, vv.w, gv.w * gs, ac, lr, eps, ad.b1, ad.omb1, ad.b2, ad.omb2, ad.wd, ad.decoupled);
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
        *reinterpret_cast<float4*>(w + i) = wv;
      } else {
        for (long long j = i; j < n; ++j)
          adam_element(w[j], m[j], v[j], g[j] * gs, ac, lr, eps, ad.b1, ad.omb1, ad.b2, ad.omb2, ad.wd, ad.decoupled);
      }
    }
    return;
  }
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
       i += (long long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      float4 wv = *reinterpret_cast<float4*>(w + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      if (adagrad) {
        float4 sv = *reinterpret_cast<float4*>(seg.st[t] + i);
        sv.x += gv.x * gv.x; sv.y += gv.y * gv.y; sv.z += gv.z * gv.z; sv.w += gv.w * gv.w;
        *reinterpret_cast<float4*>(seg.st[t] + i) = sv;
        wv.x -= lr * gv.x / (sqrtf(sv.x) + eps); wv.y -= lr * gv.y / (sqrtf(sv.y) + eps);
        wv.z -= lr * gv.z / (sqrtf(sv.z) + eps); wv.w -= lr * gv.w / (sqrtf(sv.w) + eps);
      } else {
        wv.x -= lr * gv.x; wv.y -= lr * gv.y; wv.z -= lr * gv.z; wv.w -= lr * gv.w;
      }
      *reinterpret_cast<float4*>(w + i) = wv;
    } else {
      for (long long j = i; j < n; ++j) {
        if (adagrad) {
          const float s2 = seg.st[t][j] + g[j] * g[j];
          seg.st[t][j] = s2;
          w[j] -= lr * g[j] / (sqrtf(s2) + eps);
        } else {
          w[j] -= lr * g[j];
        }
      }
    }
  }
}

static int run_sgd(const FusedUpdate& upd, float* w, const float* g, int64_t n, const float* skip, hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g)) & 15)
    return fail(TTEMB_E_BADARG, "sgd_step: buffers must be 16-byte aligned");
  const int threads = 256;
  const int64_t blocks = ((n + 3) / 4 + threads - 1) / threads;
  hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, w, g, n, upd.lr, upd.lr_dev, skip);
  return check_hip(hipGetLastError(), "sgd_step_kernel");
}

static int run_adagrad(const FusedUpdate& upd, float* w, const float* g, int64_t n, hipStream_t st) {
  const int threads = 256;
  const int64_t blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(adagrad_step_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, w, upd.st[0], g, n, upd.lr, upd.lr_dev, upd.eps);
  return check_hip(hipGetLastError(), "adagrad_step_kernel");
}

// a ttemb_adam_t into the lr, eps and Adam fields of a FusedUpdate; TTEMB_E_BADARG outside torch.optim.Adam's domain
static int adam_fill(const ttemb_adam_t* hp, int32_t* step, FusedUpdate* upd) {
  if (hp == nullptr || step == nullptr) return fail(TTEMB_E_BADARG, "adam: null hyper-parameters / step words");
  if (!(hp->beta1 >= 0.0 && hp->beta1 < 1.0) || !(hp->beta2 >= 0.0 && hp->beta2 < 1.0))
    return fail(TTEMB_E_BADARG, "adam: betas (%g, %g) outside [0, 1)", hp->beta1, hp->beta2);
  if (!(hp->lr >= 0.f) || !(hp->eps >= 0.f) || !(hp->weight_decay >= 0.f))
    return fail(TTEMB_E_BADARG, "adam: negative lr / eps / weight_decay");
  if (reinterpret_cast<uintptr_t>(step) & 15) return fail(TTEMB_E_BADARG, "adam: the step words must be 16-byte aligned");
  upd->lr = hp->lr;
  upd->eps = hp->eps;
  upd->step = reinterpret_cast<uint32_t*>(step);
  upd->b1 = (float)hp->beta1;
  upd->omb1 = (float)(1.0 - hp->beta1);
  upd->b2 = (float)hp->beta2;
  upd->omb2 = (float)(1.0 - hp->beta2);
  upd->wd = hp->weight_decay;
  upd->decoupled = hp->decoupled != 0 ? 1 : 0;
  upd->beta1 = hp->beta1;
  upd->beta2 = hp->beta2;
  return TTEMB_OK;
}

int step_arrays(const ttemb_shape_t* shape) { return shape != nullptr && shape->T >= 2 && shape->T <= TTEMB_MAX_CORES ? shape->T : 0; }

int step_from_values(int32_t kind, int T, float lr, float eps, float* const* state, float* const* state2, const ttemb_adam_t* hp,
                     int32_t* adam_step, FusedUpdate* upd) {
  memset(upd, 0, sizeof(*upd));
  const bool adam = kind == TTEMB_STEP_ADAM, adagrad = kind == TTEMB_STEP_ADAGRAD;
  if (adam) {
    if (state == nullptr || state2 == nullptr) return fail(TTEMB_E_BADARG, "exp_avg / exp_avg_sq is null");
    int rc = adam_fill(hp, adam_step, upd);
    if (rc) return rc;
  } else {
    if (adagrad && state == nullptr) return fail(TTEMB_E_BADARG, "opt_state is null");
    upd->lr = lr;
    upd->eps = adagrad ? eps : 0.f;
  }
  for (int t = 0; t < T && (adam || adagrad); ++t) {   // (the kind is read off st[0] / v[0] from here on: no null among them)
    if (state[t] == nullptr || (adam && state2[t] == nullptr)) return fail(TTEMB_E_BADARG, "null buffer");
    upd->st[t] = state[t];
    upd->v[t] = adam ? state2[t] : nullptr;
  }
  return TTEMB_OK;
}

int step_from_descriptor(const ttemb_step_t* step, int T, const FlatArrays* flat, FusedUpdate* upd) {
  if (step == nullptr) return fail(TTEMB_E_BADARG, "step: null descriptor");
  if (step->kind != TTEMB_STEP_SGD && step->kind != TTEMB_STEP_ADAGRAD && step->kind != TTEMB_STEP_ADAM)
    return fail(TTEMB_E_BADARG, "step: kind %d is none of TTEMB_STEP_SGD / _ADAGRAD / _ADAM", (int)step->kind);
  if (step->lr_dev == nullptr) return fail(TTEMB_E_BADARG, "step: lr_dev is null (the by-value calls take the rate on the host)");
  if (reinterpret_cast<uintptr_t>(step->lr_dev) & 15) return fail(TTEMB_E_BADARG, "step: lr_dev must be 16-byte aligned");
  float* const* state = flat != nullptr ? &flat->state : step->state;
  float* const* state2 = flat != nullptr ? &flat->state2 : step->state2;
  if (step->kind == TTEMB_STEP_ADAGRAD && state == nullptr) return fail(TTEMB_E_BADARG, "step: state is null (Adagrad)");
  ttemb_adam_t hp = {};   // (the descriptor's hyper-parameters with their lr ignored: 0 stands in for it, every kernel reads the word)
  if (step->kind == TTEMB_STEP_ADAM) {
    if (state == nullptr || state2 == nullptr) return fail(TTEMB_E_BADARG, "step: state / state2 is null (Adam's moments)");
    if (step->adam == nullptr) return fail(TTEMB_E_BADARG, "step: adam is null (the hyper-parameters)");
    hp = *step->adam;
    hp.lr = 0.f;
  }
  int rc = step_from_values(step->kind, T, 0.f, step->eps, state, state2, &hp, flat != nullptr ? flat->adam_step : step->adam_step, upd);
  if (rc) return rc;
  upd->lr_dev = step->lr_dev;
  return TTEMB_OK;
}

int run_step_arrays(const FusedUpdate& upd, const float* const* g, const long long* n, int T, float grad_scale, const uint32_t* skip,
                    hipStream_t st) {
  const bool adam = upd.v[0] != nullptr, adagrad = !adam && upd.st[0] != nullptr;
  Seg3 seg;
  AdamSeg ad;
  memset(&seg, 0, sizeof(seg));
  memset(&ad, 0, sizeof(ad));
  long long nmax = 0;
  for (int t = 0; t < T; ++t) {
    if (n[t] > 0 && (upd.w[t] == nullptr || g[t] == nullptr || ((adam || adagrad) && upd.st[t] == nullptr) || (adam && upd.v[t] == nullptr)))
      return fail(TTEMB_E_BADARG, "step: null buffer");
    if ((reinterpret_cast<uintptr_t>(upd.w[t]) | reinterpret_cast<uintptr_t>(upd.st[t]) | reinterpret_cast<uintptr_t>(upd.v[t]) |
         reinterpret_cast<uintptr_t>(g[t])) & 15)
      return fail(TTEMB_E_BADARG, "step: weights, optimizer state and gradients must be 16-byte aligned");
    seg.w[t] = upd.w[t];
    seg.st[t] = upd.st[t];
    seg.g[t] = g[t];
    seg.n[t] = n[t];
    ad.v[t] = upd.v[t];
    nmax = n[t] > nmax ? n[t] : nmax;
  }
  if (nmax == 0) return TTEMB_OK;
  if (adam) {
    ad.step = upd.step;
    ad.b1 = upd.b1; ad.omb1 = upd.omb1; ad.b2 = upd.b2; ad.omb2 = upd.omb2;
    ad.wd = upd.wd;
    ad.grad_scale = grad_scale;
    ad.decoupled = upd.decoupled;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(64), 0, st, adam_prep_of(upd));
    int rc = check_hip(hipGetLastError(), "adam_prepare_kernel");
    if (rc) return rc;
  }
  long long blocks = (nmax / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  hipLaunchKernelGGL(fused_step_kernel, dim3((unsigned)blocks, (unsigned)T), dim3(256), 0, st, seg, upd.lr, upd.lr_dev, upd.eps,
                     adagrad ? 1 : 0, skip, ad);
  return check_hip(hipGetLastError(), "fused_step_kernel");
}

static int check_lookup_args(const void* cores, const void* indices, int64_t nnz, int64_t B) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "negative size (nnz=%lld, B=%lld)", (long long)nnz, (long long)B);
  if (nnz > 0x7fffffffll) return fail(TTEMB_E_BADARG, "nnz=%lld exceeds int32 range", (long long)nnz);
  if (cores == nullptr) return fail(TTEMB_E_BADARG, "cores is null");
  if (nnz > 0 && indices == nullptr) return fail(TTEMB_E_BADARG, "indices is null");
  return TTEMB_OK;
}

// what every lookup entry point starts with: no pending device fault, a valid shape and sizes, the core pointers, and the
// workspace split into the header (the grouped path's persistent words: the first kFast3HeaderBytes of every lookup
// workspace; null when the workspace is smaller) and the rest
struct Entry {
  DevShape ds;
  CorePtrs cp;
  void* header;
  char* ws;
  int64_t ws_bytes;
  hipStream_t st;
};
static int enter(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices, int64_t nnz, int64_t B,
                 void* workspace, int64_t workspace_bytes, void* stream, Entry* e) {
  int rc = pending_device_fault();
  if (rc) return rc;
  rc = make_dev_shape(shape, &e->ds);
  if (rc) return rc;
  rc = check_lookup_args(cores, indices, nnz, B);
  if (rc) return rc;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) e->cp.c[t] = t < e->ds.T ? cores[t] : nullptr;
  const int64_t h = workspace != nullptr && workspace_bytes >= kFast3HeaderBytes ? kFast3HeaderBytes : 0;
  e->header = h ? workspace : nullptr;
  e->ws = reinterpret_cast<char*>(workspace) + h;
  e->ws_bytes = workspace_bytes - h;
  e->st = reinterpret_cast<hipStream_t>(stream);
  return TTEMB_OK;
}

// the row-index slot at the head of the workspace (part of the layout on every route; both kernel families derive the rows
// from `offsets` themselves when rowidx is null -- no expansion launch, no array); *ws / *ws_bytes are advanced past it
static int resolve_rowidx(const int64_t* rowidx, const int64_t* offsets, int64_t nnz, char** ws, int64_t* ws_bytes) {
  const int64_t need = align256(nnz * 8);
  if (*ws != nullptr && *ws_bytes >= need) {
    *ws += need;
    *ws_bytes -= need;
  } else if (rowidx == nullptr && nnz > 0) {
    return fail(TTEMB_E_WORKSPACE, "workspace too small for the row index (%lld bytes)", (long long)need);
  }
  if (rowidx == nullptr && offsets == nullptr && nnz > 0) return fail(TTEMB_E_BADARG, "rowidx and offsets are both null");
  return TTEMB_OK;
}

// shared body of the three backward entry points: gradient of the live ids into `dst` on route `r` -- prologue (V / the padded
// cores), one 3-core call, epilogue (dV back onto the pair / the original sub-block of the padded gradient).  `update`: the step
// the grouped backward's last kernel applies (only a GROUPED call of one piece is given one)
static int backward_into(const Route& r, const DevShape& ds, const CorePtrs& cp, const int64_t* indices, const int64_t* rowidx,
                         const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B, const float* d_output,
                         const CorePtrsMut& dst, char* ws, int64_t ws_bytes, const void* plan, int64_t plan_bytes, hipStream_t st,
                         void* header, const FusedUpdate* update = nullptr) {
  if (r.kind == kPadded && update != nullptr) return fail(TTEMB_E_BADARG, "internal: a padded table writes gradients, the step follows");
  const int64_t vb = view_bytes(r, true);   // [V | dV] / [padded cores | their gradients] in front of the grouped kernels' region
  if (vb > 0 && (ws == nullptr || ws_bytes < vb)) return fail(TTEMB_E_WORKSPACE, "backward needs room for the %s", view_name(r));
  CorePtrs c3;
  int rc = build_view(r, ds, cp, ws, true, &c3, st);
  if (rc) return rc;
  char* grads = ws + vb / 2;
  CorePtrsMut d3 = dst;
  if (r.kind == kMerged) merged_cores(r.m4, dst, reinterpret_cast<float*>(grads), &d3);
  int64_t off = 0;
  for (int t = 0; r.kind == kPadded && t < 3; off += r.pd.core_bytes[t++]) d3.c[t] = reinterpret_cast<float*>(grads + off);
  if (!r.grouped) {   // the per-bag and scalar kernels ADD into the gradients: clear them (the real cores, then dV)
    rc = launch_zero_cores(ds, dst, st);
    if (rc == TTEMB_OK && r.kind == kMerged) rc = launch_zero(grads, (size_t)r.m4.v_bytes, st, "zero dV");
    if (rc == TTEMB_OK)
      rc = r.kind == kScalar ? launch_backward_generic(ds, cp, indices, rowidx, offsets, B, nnz, nnz_dev, d_output, dst, st)
                             : launch_backward_small3(r.s3, c3, indices, offsets, nnz, nnz_dev, B, d_output, d3, st);
  } else {
    rc = launch_backward_fast3(r.s3, c3, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, d3, ws + vb, ws_bytes - vb, plan,
                               plan_bytes, st, r.kind == kGrouped ? update : nullptr, header);
  }
  if (rc) return rc;
  if (r.kind == kPadded) return unpad_grads(ds, r.pd, d3, dst, st);
  if (r.kind != kMerged || r.m4.a < 0) return TTEMB_OK;
  const Merged4& m4 = r.m4;
  hipLaunchKernelGGL(split_pair_kernel, dim3((unsigned)(m4.pa + m4.pb), (unsigned)m4.K), dim3(256), 0, st, cp.c[m4.a], cp.c[m4.a + 1],
                     reinterpret_cast<const float*>(grads), m4.pa, m4.pb, m4.rows, m4.K, m4.n, dst.c[m4.a], dst.c[m4.a + 1]);
  return check_hip(hipGetLastError(), "split_pair_kernel");
}

// ttemb_stage_call: one call of any size into the static buffers of a captured lookup.  Element i of the grid-stride loop is
// id i (widened from int32 when the caller's are) and offsets word i: the caller's, 0 .. B_live without offsets, n_live for
// every bag past the live ones.  indices_out past n_live is not touched.  No LDS; 8-byte stores, 512 contiguous bytes a wave.
__global__ __launch_bounds__(256) void stage_call_kernel(const void* __restrict__ indices_in, int ids_i32, long long n_live,
                                                         const void* __restrict__ offsets_in, int offs_i32, long long B_live,
                                                         int64_t* __restrict__ indices_out, int64_t* __restrict__ offsets_out,
                                                         long long B_cap, int32_t* __restrict__ nnz_dev_out) {
  const long long total = n_live > B_cap + 1 ? n_live : B_cap + 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) *nnz_dev_out = (int32_t)n_live;
  for (long long i = first; i < total; i += stride) {
    if (i < n_live)
      indices_out[i] = ids_i32 ? (int64_t) reinterpret_cast<const int32_t*>(indices_in)[i] : reinterpret_cast<const int64_t*>(indices_in)[i];
    if (i <= B_cap) {
      int64_t o = n_live;
      if (i <= B_live)
        o = offsets_in == nullptr ? (int64_t)i
                                  : (offs_i32 ? (int64_t) reinterpret_cast<const int32_t*>(offsets_in)[i] : reinterpret_cast<const int64_t*>(offsets_in)[i]);
      offsets_out[i] = o;
    }
  }
}

// ttemb_stage_bags: stage_call_kernel for a pooled call.  Element i is also weight i (copied for i < n_live; weights_out
// past n_live is not touched), and with fanout > 0 the offsets are generated here: i * fanout up to B_live, n_live past it.
__global__ __launch_bounds__(256) void stage_bags_kernel(const void* __restrict__ indices_in, int ids_i32, long long n_live,
                                                         const void* __restrict__ offsets_in, int offs_i32, long long B_live,
                                                         long long fanout, const float* __restrict__ weights_in,
                                                         int64_t* __restrict__ indices_out, int64_t* __restrict__ offsets_out,
                                                         long long B_cap, float* __restrict__ weights_out,
                                                         int32_t* __restrict__ nnz_dev_out) {
  const long long total = n_live > B_cap + 1 ? n_live : B_cap + 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) *nnz_dev_out = (int32_t)n_live;
  for (long long i = first; i < total; i += stride) {
    if (i < n_live) {
      indices_out[i] = ids_i32 ? (int64_t) reinterpret_cast<const int32_t*>(indices_in)[i] : reinterpret_cast<const int64_t*>(indices_in)[i];
      if (weights_in != nullptr) weights_out[i] = weights_in[i];
    }
    if (i <= B_cap) {
      int64_t o = n_live;
      if (i <= B_live) {
        if (fanout > 0)
          o = (int64_t)(i * fanout);
        else
          o = offsets_in == nullptr ? (int64_t)i
                                    : (offs_i32 ? (int64_t) reinterpret_cast<const int32_t*>(offsets_in)[i] : reinterpret_cast<const int64_t*>(offsets_in)[i]);
      }
      offsets_out[i] = o;
    }
  }
}

}  // namespace ttemb

using namespace ttemb;

// roctx ranges around the entry points (what the reference's drivers get from torch.profiler around the extension calls,
// sage_profiler.py): with TTEMB_ROCTX=1 in the environment every lookup / cache entry point is bracketed by
// roctxRangePush / roctxRangePop, so a rocprofv3 --marker-trace timeline shows the calls above their kernels.  The marker
// library is looked up at run time (librocprofiler-sdk-roctx.so, else libroctx64.so): no link dependency, and nothing
// but one relaxed load per call when the variable is not set.
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* e = getenv("TTEMB_ROCTX");
    if (e == nullptr || e[0] == '0' || e[0] == '\0') return;
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
      if (h == nullptr) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (push != nullptr && pop != nullptr) return;
      push = nullptr;
      pop = nullptr;
    }
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}
struct ApiRange {
  bool on;
  explicit ApiRange(const char* name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~ApiRange() {
    if (on) roctx().pop();
  }
  ApiRange(const ApiRange&) = delete;
  ApiRange& operator=(const ApiRange&) = delete;
};
}  // namespace

extern "C" {

int ttemb_abi_version(void) { return TTEMB_ABI_VERSION; }

const char* ttemb_last_error(void) { return g_err; }

int ttemb_set_path(int32_t path) {
  if (path < TTEMB_PATH_AUTO || path > TTEMB_PATH_PER_BAG) return fail(TTEMB_E_BADARG, "unknown path %d", path);
  g_path.store(path);
  return TTEMB_OK;
}

int ttemb_set_piece_limits(int64_t rows, int64_t ids) {
  fast3_set_piece_limits(rows, ids);
  return TTEMB_OK;
}

int ttemb_set_wide_slab_min_ids(int64_t ids) {
  fast3_set_wide_slab_min_ids(ids);
  return TTEMB_OK;
}

int ttemb_grouping_layout(const ttemb_shape_t* shape, int64_t nnz, int64_t* out) {
  if (shape == nullptr || out == nullptr || nnz < 0) return fail(TTEMB_E_BADARG, "grouping_layout: bad argument");
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  return fast3_grouping_layout(ds, nnz, out);
}

int ttemb_set_spin_limit(int64_t tries) {
  fast3_set_spin_limit(tries);
  return TTEMB_OK;
}

int ttemb_init(void) { return fault_word_init(); }

int ttemb_status(void) {
  if (g_fault_state.load(std::memory_order_acquire) == 0) (void)fault_word_init();   // (a caller that asks wants the word to exist)
  return pending_device_fault();
}

int ttemb_profile_enable(int32_t on) {
  if (on != 0)   // a read must never return a bracket recorded before this enable (by another leg, another kernel family)
    for (int i = 0; i < kProfSlots; ++i) g_prof_valid[i] = false;
  g_prof_on.store(on != 0);
  return TTEMB_OK;
}

int ttemb_profile_read(int32_t which, float* ms_host) {
  if (which < 0 || which >= kProfSlots || ms_host == nullptr) return fail(TTEMB_E_BADARG, "bad profile slot");
  if (!g_prof_valid[which]) return fail(TTEMB_E_BADARG, "no profiled launch recorded for slot %d", which);
  int rc = check_hip(hipEventSynchronize(g_prof_ev[which][1]), "hipEventSynchronize");
  if (rc) return rc;
  return check_hip(hipEventElapsedTime(ms_host, g_prof_ev[which][0], g_prof_ev[which][1]), "hipEventElapsedTime");
}

int64_t ttemb_workspace_bytes(const ttemb_shape_t* shape, int32_t op, int64_t nnz, int64_t B) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "negative size");
  // EVERY op leaves the first kFast3HeaderBytes of its workspace alone: the grouped lookup keeps its few persistent words
  // there, and callers reuse one workspace for all ops.  The grouped path's id buckets and their worst-case overflow area
  // (every id in overflow) fit the bytes its earlier three-launch grouping pass took: the buckets add 0 bytes, their slack
  // is what those bytes leave (1.9x the uniform fill at 409 600 ids on the products table; fast3.hip, grouping_layout)
  if (op == TTEMB_OP_PREPROCESS) return kFast3HeaderBytes + preprocess_workspace_bytes(nnz);
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  if (op == TTEMB_OP_CACHE_POPULATE) {   // the sort, and room for a grouped forward of the B rows
    const int64_t sort = populate_workspace_bytes(nnz);
    if (sort < 0) return fail(TTEMB_E_HIP, "rocprim size query failed");
    const bool grouped = route_of(ds, B, B, true, true).kind == kGrouped;
    return kFast3HeaderBytes + sort + (grouped ? fast3_workspace_bytes(ds, TTEMB_OP_FORWARD, B, B) : 0);
  }
  if (op != TTEMB_OP_FORWARD && op != TTEMB_OP_BACKWARD) return fail(TTEMB_E_BADARG, "unknown op %d", op);
  // (sized for ids with offsets and without a row index: the call may take any route)
  return lookup_workspace_bytes(route_of(ds, nnz, B, true, true), ds, op, nnz, B);
}

int ttemb_kernel_family(const ttemb_shape_t* shape, int64_t nnz, int64_t B, int32_t ids_with_offsets) {
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "negative size");
  // (without the bag boundaries a call past one row window cannot be cut into pieces)
  const Route r = route_of(ds, nnz, B, ids_with_offsets != 0, ids_with_offsets != 0);
  if (r.kind == kScalar) return TTEMB_FAMILY_SCALAR;
  const int view = r.kind == kMerged ? TTEMB_FAMILY_MERGED : (r.kind == kPadded ? TTEMB_FAMILY_PADDED : 0);
  if (!r.grouped) return view | (small3_templated_shape(r.s3) ? TTEMB_FAMILY_PER_BAG : TTEMB_FAMILY_PER_BAG_RT);
  if (fast3_wide(r.s3)) return view | TTEMB_FAMILY_GROUPED_WIDE;
  return view | TTEMB_FAMILY_GROUPED | (fast3_prefix_in_chain(r.s3, nnz, B) ? TTEMB_FAMILY_PREFIX_IN_CHAIN : 0) |
         (fast3_group_products_in_chain(r.s3, nnz, B) ? TTEMB_FAMILY_GROUP_PRODUCTS_IN_CHAIN : 0);
}

int64_t ttemb_plan_bytes(const ttemb_shape_t* shape, int64_t nnz) {
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  if (nnz < 0) return fail(TTEMB_E_BADARG, "negative size");
  // the plan of the 3-core call (a call that runs in pieces keeps none -- a plan describes one piece --; neither does a per-bag view)
  const Route r = route_of(ds, nnz, 0, true, false);
  return r.grouped && fast3_fits(r.s3, nnz, 0) ? fast3_plan_bytes(r.s3, nnz) : 0;
}

}  // extern "C"

// phase 0 = the whole forward; 1 = everything that depends only on the ids; 2 = the rest (reads the cores)
// prologue (V / the padded cores), one 3-core call; the workspace behind the header: [row slot | view_bytes | grouped region]
static int forward_phase(int phase, const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                         const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                         const int32_t* nnz_dev, int64_t B, float* output, void* workspace,
                         int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream) {
  Entry e;
  int rc = enter(shape, cores, indices, nnz, B, workspace, workspace_bytes, stream, &e);
  if (rc) return rc;
  if (B == 0) return TTEMB_OK;
  if (output == nullptr) return fail(TTEMB_E_BADARG, "output is null");
  if (B >= 0x7fffffffll) return fail(TTEMB_E_BADARG, "B exceeds int32 range");
  const DevShape& ds = e.ds;
  const Route r = route_of(ds, nnz, B, offsets != nullptr, rowidx == nullptr && offsets != nullptr, nnz > 0);
  if (phase == 1 && !r.grouped) return TTEMB_OK;   // the per-bag and scalar kernels have no id-only half: phase 2 is their whole forward
  if (phase == 2 && r.kind == kGrouped)   // (on the workspace as it is handed over: the row slot is the id-only half's business)
    return launch_forward_fast3(ds, e.cp, indices, rowidx, offsets, nnz, nnz_dev, B, output, offsets != nullptr, e.ws, e.ws_bytes,
                                plan, plan_bytes, 2, e.st, e.header);
  const int64_t vb = view_bytes(r, false);
  if (vb > 0 && (e.ws == nullptr || e.ws_bytes < align256(nnz * 8) + vb))
    return fail(TTEMB_E_WORKSPACE, "forward needs room for the %s", view_name(r));
  if (rowidx == nullptr && offsets == nullptr && nnz > 0) return fail(TTEMB_E_BADARG, "rowidx and offsets are both null");
  char* ws = e.ws;
  int64_t ws_bytes = e.ws_bytes;
  CorePtrs c3;
  rc = build_view(r, ds, e.cp, vb > 0 ? ws + align256(nnz * 8) : ws, phase != 1, &c3, e.st);   // (the id-only half does not read the cores)
  if (rc) return rc;
  if (!r.grouped && r.kind != kScalar)   // per-bag: one launch, every output row written once, zeros for an empty bag
    return launch_forward_small3(r.s3, c3, indices, offsets, nnz, nnz_dev, B, output, e.st);
  rc = resolve_rowidx(rowidx, offsets, nnz, &ws, &ws_bytes);
  if (rc) return rc;
  ws += vb;
  ws_bytes -= vb;
  // the rows the kernels add into: every row without offsets (the lookup half of a grouped forward finds them cleared by the id-only
  // half); with offsets those of bags that do not hold exactly one id -- the grouping pass clears them itself
  if (offsets == nullptr && !(phase == 2 && r.grouped)) {
    rc = launch_zero(output, (size_t)B * ds.D * 4, e.st, "zero output");
  } else if (offsets != nullptr && !r.grouped) {
    const int threads = 256;
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((B + threads - 1) / threads)), dim3(threads), 0,
                       e.st, offsets, B, ds.D, output);
    rc = check_hip(hipGetLastError(), "zero_rows_kernel");
  }
  if (rc || nnz == 0) return rc;
  if (r.grouped)
    return launch_forward_fast3(r.s3, c3, indices, rowidx, offsets, nnz, nnz_dev, B, output, offsets != nullptr, ws, ws_bytes, plan,
                                plan_bytes, phase, e.st, e.header);
  // (a forced TTEMB_PATH_FAST3 on a table the grouped kernels do not take -- another shape, or past a size limit of
  //  fits_shape / classify -- runs what ttemb_kernel_family and the size queries answer for it: the scalar kernels)
  return launch_forward_generic(ds, e.cp, indices, rowidx, offsets, B, nnz, nnz_dev, output, e.st);
}

extern "C" {

int ttemb_forward(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                  const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                  const int32_t* nnz_dev, int64_t B, float* output, void* workspace,
                  int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_forward");
  return forward_phase(0, shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, output, workspace, workspace_bytes, plan,
                       plan_bytes, stream);
}

int ttemb_forward_group(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                        const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                        const int32_t* nnz_dev, int64_t B, float* output, void* workspace,
                        int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_forward_group");
  return forward_phase(1, shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, output, workspace, workspace_bytes, plan,
                       plan_bytes, stream);
}

int ttemb_forward_lookup(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                         const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                         const int32_t* nnz_dev, int64_t B, float* output, void* workspace,
                         int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_forward_lookup");
  return forward_phase(2, shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, output, workspace, workspace_bytes, plan,
                       plan_bytes, stream);
}

int ttemb_backward_dense(const ttemb_shape_t* shape, const float* const* cores,
                         const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                         const int32_t* nnz_dev, int64_t B, const float* d_output,
                         float* const* d_cores, void* workspace, int64_t workspace_bytes,
                         const void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_dense");
  Entry e;
  int rc = enter(shape, cores, indices, nnz, B, workspace, workspace_bytes, stream, &e);
  if (rc) return rc;
  if (d_cores == nullptr) return fail(TTEMB_E_BADARG, "d_cores is null");
  if (nnz > 0 && d_output == nullptr) return fail(TTEMB_E_BADARG, "d_output is null");
  CorePtrsMut dp;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) dp.c[t] = t < e.ds.T ? d_cores[t] : nullptr;
  // the gradient scratch region behind the header is unused in dense mode
  const int64_t skip = grad_scratch_bytes(e.ds);
  char* ws = e.ws ? e.ws + skip : nullptr;
  int64_t rest = e.ws_bytes > skip ? e.ws_bytes - skip : 0;
  rc = resolve_rowidx(rowidx, offsets, nnz, &ws, &rest);
  if (rc) return rc;
  const Route r = route_of(e.ds, nnz, B, offsets != nullptr, rowidx == nullptr && offsets != nullptr);
  return backward_into(r, e.ds, e.cp, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, dp, ws, rest, plan, plan_bytes, e.st, e.header);
}

// body of the fused-step backward entry points.  `step`: the description a builder filled (every field but w)
static int fused_backward(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* rowidx,
                          const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B, const float* d_output,
                          const FusedUpdate& step, void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                          void* stream) {
  Entry e;
  int rc = enter(shape, cores, indices, nnz, B, workspace, workspace_bytes, stream, &e);
  if (rc) return rc;
  const DevShape& ds = e.ds;
  // zero gradient: SGD is a no-op, Adagrad adds 0 and divides 0; an Adam call without ids is defined as a no-op too (t stays)
  if (nnz == 0) return TTEMB_OK;
  if (d_output == nullptr) return fail(TTEMB_E_BADARG, "d_output is null");
  const int64_t need = kFast3HeaderBytes + grad_scratch_bytes(ds);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(TTEMB_E_WORKSPACE, "backward needs %lld workspace bytes, got %lld", (long long)need, (long long)workspace_bytes);
  CorePtrsMut gp;   // the gradient scratch behind the header
  const float* g[TTEMB_MAX_CORES];
  long long n[TTEMB_MAX_CORES];
  int64_t off = 0;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) {
    g[t] = gp.c[t] = t < ds.T ? reinterpret_cast<float*>(e.ws + off) : nullptr;
    n[t] = t < ds.T ? (long long)ds.p[t] * ds.row_len[t] : 0;
    off += align256(n[t] * 4);
  }
  char* rest_ws = e.ws + off;
  int64_t rest = e.ws_bytes - off;
  rc = resolve_rowidx(rowidx, offsets, nnz, &rest_ws, &rest);
  if (rc) return rc;
  const Route r = route_of(ds, nnz, B, offsets != nullptr, rowidx == nullptr && offsets != nullptr);
  // the grouped path of a one-piece call applies the step inside its last kernel; every other route writes gradients, then steps
  const bool fused = r.kind == kGrouped && fast3_fits(ds, nnz, B);
  FusedUpdate upd = step;
  for (int t = 0; t < ds.T; ++t)
    if ((upd.w[t] = cores[t]) == nullptr) return fail(TTEMB_E_BADARG, "null core / optimizer state");
  rc = backward_into(r, ds, e.cp, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, gp, rest_ws, rest, plan, plan_bytes, e.st,
                     e.header, fused ? &upd : nullptr);
  if (rc || fused) return rc;
  // (a grouped backward left its verdict in the header's poison word: a poisoned plan leaves the parameters alone)
  const uint32_t* header_skip =
      r.grouped ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(e.header) + kHeaderPoisonOffset) : nullptr;
  return run_step_arrays(upd, g, n, ds.T, 1.f, header_skip, e.st);
}

int ttemb_backward_adam(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                        int32_t* step, const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                        const int32_t* nnz_dev, int64_t B, const float* d_output, const ttemb_adam_t* hp,
                        void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_adam");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAM, step_arrays(shape), 0.f, 0.f, exp_avg, exp_avg_sq, hp, step, &upd);
  if (rc) return rc;
  return fused_backward(shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, upd, workspace, workspace_bytes, plan,
                        plan_bytes, stream);
}

int ttemb_backward_sgd(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices,
                       const int64_t* rowidx, const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B,
                       const float* d_output, float lr, void* workspace, int64_t workspace_bytes,
                       const void* plan, int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_sgd");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_SGD, step_arrays(shape), lr, 0.f, nullptr, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return fused_backward(shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, upd, workspace, workspace_bytes, plan,
                        plan_bytes, stream);
}

int ttemb_backward_adagrad(const ttemb_shape_t* shape, float* const* cores, float* const* opt_state,
                           const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                           const int32_t* nnz_dev, int64_t B, const float* d_output, float lr,
                           float eps, void* workspace, int64_t workspace_bytes, const void* plan,
                           int64_t plan_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_adagrad");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAGRAD, step_arrays(shape), lr, eps, opt_state, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return fused_backward(shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, upd, workspace, workspace_bytes, plan,
                        plan_bytes, stream);
}

// ---- a window of a longer id list: one table of a table-batched call (include/ttemb.h) ----
int64_t ttemb_window_workspace_bytes(const ttemb_shape_t* shape, int32_t op, int64_t nnz, int64_t bags_total, int64_t B) {
  if (nnz < 0 || B < 0 || bags_total < B) return fail(TTEMB_E_BADARG, "negative size, or more bags in the window than in the call");
  if (op != TTEMB_OP_FORWARD && op != TTEMB_OP_BACKWARD) return fail(TTEMB_E_BADARG, "a window is looked up (TTEMB_OP_FORWARD) or differentiated (TTEMB_OP_BACKWARD)");
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  if (nnz == 0 || B == 0) return kFast3HeaderBytes;
  if (current_path() == TTEMB_PATH_GENERIC || current_path() == TTEMB_PATH_PER_BAG || !fast3_window_fits(ds, nnz, bags_total, B))
    return fail(TTEMB_E_UNSUPPORTED, "the grouped kernels do not cover this window (shape, size or forced path)");
  return kFast3HeaderBytes + fast3_window_workspace_bytes(ds, op == TTEMB_OP_BACKWARD, nnz);
}

static int window_args(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices, const int64_t* offsets,
                       int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, void* workspace, int64_t workspace_bytes,
                       void* stream, Entry* e) {
  int rc = enter(shape, cores, indices, nnz, B, workspace, workspace_bytes, stream, e);
  if (rc) return rc;
  if (offsets == nullptr) return fail(TTEMB_E_BADARG, "a window needs the bag boundaries (offsets)");
  if (bag0 < 0 || B < 0 || bag0 + B > bags_total) return fail(TTEMB_E_BADARG, "the window [%lld, %lld) does not lie inside the call's %lld bags",
                                                                (long long)bag0, (long long)(bag0 + B), (long long)bags_total);
  if (current_path() == TTEMB_PATH_GENERIC || current_path() == TTEMB_PATH_PER_BAG)
    return fail(TTEMB_E_UNSUPPORTED, "a window is served by the grouped kernels (path forced elsewhere)");
  if (e->header == nullptr) return fail(TTEMB_E_WORKSPACE, "a window call needs ttemb_window_workspace_bytes() bytes");
  return TTEMB_OK;
}

int ttemb_forward_window(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices, const int64_t* offsets,
                         int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, float* output, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_forward_window");
  Entry e;
  int rc = window_args(shape, cores, indices, offsets, nnz, bags_total, bag0, B, workspace, workspace_bytes, stream, &e);
  if (rc || B == 0) return rc;
  if (output == nullptr) return fail(TTEMB_E_BADARG, "output is null");
  if (nnz == 0) return launch_zero(output + bag0 * e.ds.D, (size_t)B * e.ds.D * 4, e.st, "zero the window's rows");
  return launch_forward_window_fast3(e.ds, e.cp, indices, offsets, nnz, bags_total, bag0, B, output, e.ws, e.ws_bytes, e.st, e.header);
}

// body of the window backward entry points.  `step`: null for dense gradients into `d_cores`, else the description a builder filled
static int backward_window(const ttemb_shape_t* shape, float* const* cores, float* const* d_cores, const int64_t* indices,
                           const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, const float* d_output,
                           const FusedUpdate* step, void* workspace, int64_t workspace_bytes, void* stream) {
  Entry e;
  int rc = window_args(shape, cores, indices, offsets, nnz, bags_total, bag0, B, workspace, workspace_bytes, stream, &e);
  if (rc) return rc;
  const DevShape& ds = e.ds;
  CorePtrsMut dp;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) dp.c[t] = (step == nullptr && t < ds.T) ? d_cores[t] : nullptr;
  if (step == nullptr) {   // dense: every gradient is written whole
    for (int t = 0; t < ds.T; ++t)
      if (d_cores[t] == nullptr) return fail(TTEMB_E_BADARG, "d_cores[%d] is null", t);
    if (nnz == 0 || B == 0) return launch_zero_cores(ds, dp, e.st);
  } else if (nnz == 0 || B == 0) {
    return TTEMB_OK;   // zero gradient: SGD is a no-op, Adagrad adds 0 and divides 0
  }
  if (d_output == nullptr) return fail(TTEMB_E_BADARG, "d_output is null");
  FusedUpdate upd;
  if (step != nullptr) {
    upd = *step;
    for (int t = 0; t < ds.T; ++t)
      if ((upd.w[t] = cores[t]) == nullptr) return fail(TTEMB_E_BADARG, "null core / optimizer state");
  }
  return launch_backward_window_fast3(ds, e.cp, indices, offsets, nnz, bags_total, bag0, B, d_output, dp, e.ws, e.ws_bytes, e.st,
                                      step != nullptr ? &upd : nullptr, e.header);
}

int ttemb_backward_dense_window(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices, const int64_t* offsets,
                                int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, const float* d_output, float* const* d_cores,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_dense_window");
  if (d_cores == nullptr) return fail(TTEMB_E_BADARG, "d_cores is null");
  return backward_window(shape, const_cast<float* const*>(cores), d_cores, indices, offsets, nnz, bags_total, bag0, B, d_output, nullptr,
                         workspace, workspace_bytes, stream);
}

int ttemb_backward_sgd_window(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets,
                              int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, const float* d_output, float lr,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_sgd_window");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_SGD, step_arrays(shape), lr, 0.f, nullptr, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return backward_window(shape, cores, nullptr, indices, offsets, nnz, bags_total, bag0, B, d_output, &upd, workspace, workspace_bytes,
                         stream);
}

int ttemb_backward_adagrad_window(const ttemb_shape_t* shape, float* const* cores, float* const* opt_state, const int64_t* indices,
                                  const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B,
                                  const float* d_output, float lr, float eps, void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_adagrad_window");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAGRAD, step_arrays(shape), lr, eps, opt_state, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return backward_window(shape, cores, nullptr, indices, offsets, nnz, bags_total, bag0, B, d_output, &upd, workspace, workspace_bytes,
                         stream);
}

int ttemb_backward_adam_window(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                               int32_t* step, const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t bags_total,
                               int64_t bag0, int64_t B, const float* d_output, const ttemb_adam_t* hp, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_adam_window");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAM, step_arrays(shape), 0.f, 0.f, exp_avg, exp_avg_sq, hp, step, &upd);
  if (rc) return rc;
  return backward_window(shape, cores, nullptr, indices, offsets, nnz, bags_total, bag0, B, d_output, &upd, workspace, workspace_bytes,
                         stream);
}

int ttemb_stage_call(const void* indices_in, int32_t indices_are_i32, int64_t n_live, const void* offsets_in, int32_t offsets_are_i32,
                     int64_t B_live, int64_t* indices_out, int64_t nnz_cap, int64_t* offsets_out, int64_t B_cap, int32_t* nnz_dev_out,
                     void* stream) {
  ApiRange api_range("ttemb_stage_call");
  if (n_live < 0 || B_live < 0 || nnz_cap < 0 || B_cap < 0) return fail(TTEMB_E_BADARG, "ttemb_stage_call: negative size");
  if (n_live > nnz_cap)
    return fail(TTEMB_E_BADARG, "ttemb_stage_call: %lld ids exceed the capacity of %lld", (long long)n_live, (long long)nnz_cap);
  if (B_live > B_cap)
    return fail(TTEMB_E_BADARG, "ttemb_stage_call: %lld bags exceed the capacity of %lld", (long long)B_live, (long long)B_cap);
  if (nnz_cap > 0x7fffffffll) return fail(TTEMB_E_BADARG, "ttemb_stage_call: the id capacity exceeds int32 range (the count word is int32)");
  if (offsets_in == nullptr && B_live != n_live)
    return fail(TTEMB_E_BADARG, "ttemb_stage_call: without offsets every id is a bag of its own, but %lld ids came with %lld bags",
                (long long)n_live, (long long)B_live);
  if (offsets_out == nullptr || nnz_dev_out == nullptr || (n_live > 0 && (indices_in == nullptr || indices_out == nullptr)))
    return fail(TTEMB_E_BADARG, "ttemb_stage_call: null buffer");
  const int64_t total = n_live > B_cap + 1 ? n_live : B_cap + 1;
  int64_t blocks = (total + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks;   // (memory-bound: the grid is capped, the loop strides over the rest)
  hipLaunchKernelGGL(stage_call_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), indices_in,
                     indices_are_i32 != 0 ? 1 : 0, (long long)n_live, offsets_in, offsets_are_i32 != 0 ? 1 : 0, (long long)B_live, indices_out,
                     offsets_out, (long long)B_cap, nnz_dev_out);
  return check_hip(hipGetLastError(), "stage_call_kernel");
}

int ttemb_stage_bags(const void* indices_in, int32_t indices_are_i32, int64_t n_live, const void* offsets_in, int32_t offsets_are_i32,
                     int64_t B_live, int64_t fanout, const float* weights_in, int64_t* indices_out, int64_t nnz_cap,
                     int64_t* offsets_out, int64_t B_cap, float* weights_out, int32_t* nnz_dev_out, void* stream) {
  ApiRange api_range("ttemb_stage_bags");
  if (n_live < 0 || B_live < 0 || nnz_cap < 0 || B_cap < 0) return fail(TTEMB_E_BADARG, "ttemb_stage_bags: negative size");
  if (fanout < 0) return fail(TTEMB_E_BADARG, "ttemb_stage_bags: negative fanout");
  if (n_live > nnz_cap)
    return fail(TTEMB_E_BADARG, "ttemb_stage_bags: %lld ids exceed the capacity of %lld", (long long)n_live, (long long)nnz_cap);
  if (B_live > B_cap)
    return fail(TTEMB_E_BADARG, "ttemb_stage_bags: %lld bags exceed the capacity of %lld", (long long)B_live, (long long)B_cap);
  if (nnz_cap > 0x7fffffffll) return fail(TTEMB_E_BADARG, "ttemb_stage_bags: the id capacity exceeds int32 range (the count word is int32)");
  if (fanout > 0) {
    if (offsets_in != nullptr) return fail(TTEMB_E_BADARG, "ttemb_stage_bags: bags of a fixed fanout take no offsets");
    if (B_live > nnz_cap / fanout || n_live != B_live * fanout)   // (the division first: B_live * fanout cannot overflow)
      return fail(TTEMB_E_BADARG, "ttemb_stage_bags: %lld ids are not %lld bags of fanout %lld", (long long)n_live, (long long)B_live,
                  (long long)fanout);
  } else if (offsets_in == nullptr && B_live != n_live) {
    return fail(TTEMB_E_BADARG, "ttemb_stage_bags: without offsets every id is a bag of its own, but %lld ids came with %lld bags",
                (long long)n_live, (long long)B_live);
  }
  if ((weights_in == nullptr) != (weights_out == nullptr))
    return fail(TTEMB_E_BADARG, "ttemb_stage_bags: weights on one side only (weights_in and weights_out go together)");
  if (offsets_out == nullptr || nnz_dev_out == nullptr || (n_live > 0 && (indices_in == nullptr || indices_out == nullptr)))
    return fail(TTEMB_E_BADARG, "ttemb_stage_bags: null buffer");
  const int64_t total = n_live > B_cap + 1 ? n_live : B_cap + 1;
  int64_t blocks = (total + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks;   // (memory-bound: the grid is capped, the loop strides over the rest)
  hipLaunchKernelGGL(stage_bags_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), indices_in,
                     indices_are_i32 != 0 ? 1 : 0, (long long)n_live, offsets_in, offsets_are_i32 != 0 ? 1 : 0, (long long)B_live,
                     (long long)fanout, weights_in, indices_out, offsets_out, (long long)B_cap, weights_out, nnz_dev_out);
  return check_hip(hipGetLastError(), "stage_bags_kernel");
}

// body of the flat steps: `n` floats of one array.  sgd_step_kernel / adagrad_step_kernel for SGD / Adagrad (no gradient
// scale; Adagrad has no skip word), the array step for Adam
static int flat_step(const FusedUpdate& step, float* weights, const float* grads, int64_t n, float grad_scale, const float* skip,
                     void* stream) {
  if (n <= 0) return TTEMB_OK;
  if (weights == nullptr || grads == nullptr) return fail(TTEMB_E_BADARG, "null buffer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (step.v[0] != nullptr) {
    FusedUpdate upd = step;
    upd.w[0] = weights;
    const long long nn = n;
    return run_step_arrays(upd, &grads, &nn, 1, grad_scale, reinterpret_cast<const uint32_t*>(skip), st);
  }
  if (grad_scale != 1.f) return fail(TTEMB_E_BADARG, "flat step: grad_scale is Adam's (pass 1 for SGD / Adagrad)");
  if (step.st[0] == nullptr) return run_sgd(step, weights, grads, n, skip, st);
  if (skip != nullptr) return fail(TTEMB_E_BADARG, "flat step: the Adagrad step takes no skip word");
  return run_adagrad(step, weights, grads, n, st);
}

int ttemb_adam_step(float* weights, float* exp_avg, float* exp_avg_sq, int32_t* step, const float* grads, int64_t n,
                    float grad_scale, const ttemb_adam_t* hp, const float* skip, void* stream) {
  ApiRange api_range("ttemb_adam_step");
  if (n < 0) return fail(TTEMB_E_BADARG, "negative n");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAM, n > 0 ? 1 : 0, 0.f, 0.f, &exp_avg, &exp_avg_sq, hp, step, &upd);
  if (rc) return rc;
  return flat_step(upd, weights, grads, n, grad_scale, skip, stream);
}

int ttemb_sgd_step(float* weights, const float* grads, int64_t n, float lr, void* stream) {
  ApiRange api_range("ttemb_sgd_step");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_SGD, n > 0 ? 1 : 0, lr, 0.f, nullptr, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return flat_step(upd, weights, grads, n, 1.f, nullptr, stream);
}

int ttemb_sgd_step_guarded(float* weights, const float* grads, int64_t n, float lr, const float* skip, void* stream) {
  ApiRange api_range("ttemb_sgd_step_guarded");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_SGD, n > 0 ? 1 : 0, lr, 0.f, nullptr, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return flat_step(upd, weights, grads, n, 1.f, skip, stream);
}

int ttemb_adagrad_step(float* weights, float* state, const float* grads, int64_t n, float lr,
                       float eps, void* stream) {
  ApiRange api_range("ttemb_adagrad_step");
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAGRAD, n > 0 ? 1 : 0, lr, eps, &state, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return flat_step(upd, weights, grads, n, 1.f, nullptr, stream);
}

// ---- the step of a capturable caller: the learning rate is a device word (include/ttemb.h "Device-resident learning rate") ----
int ttemb_backward_step(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* rowidx,
                        const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B, const float* d_output,
                        const ttemb_step_t* step, void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                        void* stream) {
  ApiRange api_range("ttemb_backward_step");
  FusedUpdate upd;
  int rc = step_from_descriptor(step, step_arrays(shape), nullptr, &upd);
  if (rc) return rc;
  return fused_backward(shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, d_output, upd, workspace, workspace_bytes, plan,
                        plan_bytes, stream);
}

int ttemb_backward_step_window(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets,
                               int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B, const float* d_output,
                               const ttemb_step_t* step, void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_backward_step_window");
  FusedUpdate upd;
  int rc = step_from_descriptor(step, step_arrays(shape), nullptr, &upd);
  if (rc) return rc;
  return backward_window(shape, cores, nullptr, indices, offsets, nnz, bags_total, bag0, B, d_output, &upd, workspace, workspace_bytes,
                         stream);
}

int ttemb_flat_step(float* weights, float* state, float* state2, int32_t* adam_step, const float* grads, int64_t n, float grad_scale,
                    const ttemb_step_t* step, const float* skip, void* stream) {
  ApiRange api_range("ttemb_flat_step");
  if (n < 0) return fail(TTEMB_E_BADARG, "negative n");
  const FlatArrays flat = {state, state2, adam_step};
  FusedUpdate upd;
  int rc = step_from_descriptor(step, n > 0 ? 1 : 0, &flat, &upd);
  if (rc) return rc;
  return flat_step(upd, weights, grads, n, grad_scale, skip, stream);
}

static int cache_update(const int64_t* indices, int64_t nnz, int64_t* hashtbl, int64_t* cache_freq, int64_t H, bool one_sweep,
                        void* stream) {
  if (nnz < 0) return fail(TTEMB_E_BADARG, "negative nnz");
  if (nnz == 0) return TTEMB_OK;
  if (H <= 0 || H > 0x7fffffffll) return fail(TTEMB_E_BADARG, "hashtbl_size %lld out of range", (long long)H);
  if (!indices || !hashtbl || !cache_freq) return fail(TTEMB_E_BADARG, "null buffer");
  return launch_cache_update(indices, nnz, hashtbl, cache_freq, H, reinterpret_cast<hipStream_t>(stream), one_sweep);
}

int ttemb_cache_update(const int64_t* indices, int64_t nnz, int64_t* hashtbl, int64_t* cache_freq,
                       int64_t H, void* stream) {
  ApiRange api_range("ttemb_cache_update");
  return cache_update(indices, nnz, hashtbl, cache_freq, H, false, stream);
}

int ttemb_cache_update_one_sweep(const int64_t* indices, int64_t nnz, int64_t* hashtbl, int64_t* cache_freq,
                                 int64_t H, void* stream) {
  ApiRange api_range("ttemb_cache_update_one_sweep");
  return cache_update(indices, nnz, hashtbl, cache_freq, H, true, stream);
}

int ttemb_cache_populate(const ttemb_shape_t* shape, const float* const* cores, int64_t* hashtbl,
                         int64_t* cache_freq, int32_t* cache_state, int64_t H, float* cache_weight,
                         int64_t C, void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_cache_populate");
  DevShape ds;
  int rc = make_dev_shape(shape, &ds);
  if (rc) return rc;
  if (H <= 0 || H > 0x7fffffffll) return fail(TTEMB_E_BADARG, "hashtbl_size %lld out of range", (long long)H);
  if (C < 0 || C > H) return fail(TTEMB_E_BADARG, "cache rows %lld must be within [0, hashtbl_size]", (long long)C);
  if (!cores || !hashtbl || !cache_freq || !cache_state || (C > 0 && !cache_weight) || !workspace)
    return fail(TTEMB_E_BADARG, "null buffer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t* sorted_keys = nullptr;
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "cache_populate: workspace smaller than its header");
  workspace = reinterpret_cast<char*>(workspace) + kFast3HeaderBytes;   // (the lookups' persistent words)
  workspace_bytes -= kFast3HeaderBytes;
  rc = launch_cache_populate_rank(hashtbl, cache_freq, cache_state, H, C, workspace, workspace_bytes,
                                  &sorted_keys, st);
  if (rc || C == 0) return rc;
  CorePtrs cp;
  for (int t = 0; t < TTEMB_MAX_CORES; ++t) cp.c[t] = t < ds.T ? cores[t] : nullptr;
  // rows of the C hottest ids straight into cache_weight (reference: prefetch in chunks of 200)
  return launch_forward_generic(ds, cp, sorted_keys, nullptr, nullptr, C, C, nullptr, cache_weight, st);
}

static int preprocess_impl(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B, int32_t warmup,
                           int64_t* hashtbl, int64_t* cache_freq, const int32_t* cache_state, int64_t H,
                           int64_t* indices_out, int64_t* rowidx_out, int32_t* cache_loc_out, int32_t* nnz_tt_dev,
                           int32_t* dup_stamp, void* workspace, int64_t workspace_bytes, void* stream) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "negative size");
  if (nnz > 0x7fffffffll) return fail(TTEMB_E_BADARG, "nnz exceeds int32 range");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool passthrough = warmup != 0 || H == 0;
  if (nnz == 0) return nnz_tt_dev ? launch_set_count(nnz_tt_dev, 0, st) : TTEMB_OK;
  if (!indices || !offsets || !rowidx_out) return fail(TTEMB_E_BADARG, "null buffer");
  if (passthrough) {
    int rc = launch_rowidx(offsets, B, nnz, rowidx_out, st);
    if (rc) return rc;
    if (indices_out != nullptr && indices_out != indices) {
      rc = check_hip(hipMemcpyAsync(indices_out, indices, (size_t)nnz * 8, hipMemcpyDeviceToDevice, st), "copy indices");
      if (rc) return rc;
    }
    return nnz_tt_dev ? launch_set_count(nnz_tt_dev, (int32_t)nnz, st) : TTEMB_OK;
  }
  if (H > 0x7fffffffll) return fail(TTEMB_E_BADARG, "hashtbl_size out of range");
  if (!hashtbl || !cache_state || !indices_out || !cache_loc_out || !nnz_tt_dev || !workspace)
    return fail(TTEMB_E_BADARG, "null buffer");
  if (indices_out == indices) return fail(TTEMB_E_BADARG, "partition cannot run in place");
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "preprocess: workspace smaller than its header");
  return launch_partition(indices, offsets, nnz, B, hashtbl, cache_freq, cache_state, H, indices_out, rowidx_out,
                          cache_loc_out, nnz_tt_dev, dup_stamp, reinterpret_cast<char*>(workspace) + kFast3HeaderBytes,
                          workspace_bytes - kFast3HeaderBytes, st);
}

int ttemb_preprocess(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                     int32_t warmup, const int64_t* hashtbl, const int32_t* cache_state, int64_t H,
                     int64_t* indices_out, int64_t* rowidx_out, int32_t* cache_loc_out,
                     int32_t* nnz_tt_dev, int32_t* dup_stamp, int32_t epoch, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  ApiRange api_range("ttemb_preprocess");
  (void)epoch;   // ABI 1 took a per-call epoch for the stamps; position stamps need none
  return preprocess_impl(indices, offsets, nnz, B, warmup, const_cast<int64_t*>(hashtbl), nullptr, cache_state, H, indices_out,
                         rowidx_out, cache_loc_out, nnz_tt_dev, dup_stamp, workspace, workspace_bytes, stream);
}

int ttemb_preprocess_update(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B, int64_t* hashtbl,
                            int64_t* cache_freq, const int32_t* cache_state, int64_t H, int64_t* indices_out,
                            int64_t* rowidx_out, int32_t* cache_loc_out, int32_t* nnz_tt_dev, int32_t* dup_stamp,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_preprocess_update");
  if (H <= 0 || !hashtbl || !cache_freq) return fail(TTEMB_E_BADARG, "ttemb_preprocess_update needs the hash table and its counters");
  return preprocess_impl(indices, offsets, nnz, B, 0, hashtbl, cache_freq, cache_state, H, indices_out, rowidx_out,
                         cache_loc_out, nnz_tt_dev, dup_stamp, workspace, workspace_bytes, stream);
}

int64_t ttemb_drop_padding_workspace_bytes(int64_t nnz, int64_t B) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "ttemb_drop_padding_workspace_bytes: negative size");
  return kFast3HeaderBytes + drop_padding_workspace_bytes(nnz);
}

int ttemb_drop_padding(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B, int64_t pad,
                       int64_t* indices_out, int64_t* rowidx_out, int64_t* offsets_out, int32_t* nnz_kept_dev, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_drop_padding");
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "ttemb_drop_padding: negative size");
  if (nnz > 0x7fffffffll) return fail(TTEMB_E_BADARG, "ttemb_drop_padding: nnz exceeds int32 range");
  if (!offsets || !offsets_out || !nnz_kept_dev || !workspace || (nnz > 0 && (!indices || !indices_out || !rowidx_out)))
    return fail(TTEMB_E_BADARG, "ttemb_drop_padding: null buffer");
  if (nnz > 0 && indices_out == indices) return fail(TTEMB_E_BADARG, "ttemb_drop_padding: the partition cannot run in place");
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "ttemb_drop_padding: workspace smaller than its header");
  return launch_drop_padding(indices, offsets, nnz, B, pad, indices_out, rowidx_out, offsets_out, nnz_kept_dev,
                             reinterpret_cast<char*>(workspace) + kFast3HeaderBytes, workspace_bytes - kFast3HeaderBytes,
                             reinterpret_cast<hipStream_t>(stream));
}

int64_t ttemb_compact_bags_workspace_bytes(int64_t nnz) {
  if (nnz < 0) return fail(TTEMB_E_BADARG, "ttemb_compact_bags_workspace_bytes: negative size");
  return kFast3HeaderBytes + compact_bags_workspace_bytes(nnz);
}

int ttemb_compact_bags(const int64_t* indices, const int64_t* offsets, const float* weights, int64_t nnz, const int32_t* nnz_dev,
                       int64_t B, int64_t pad, int64_t* indices_out, int64_t* offsets_out, float* weights_out, int32_t* map_out,
                       int32_t* kept_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  ApiRange api_range("ttemb_compact_bags");
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "ttemb_compact_bags: negative size");
  if (nnz > 0x7fffffffll) return fail(TTEMB_E_BADARG, "ttemb_compact_bags: nnz exceeds int32 range");
  if (!offsets || !offsets_out || !kept_dev || !workspace || (nnz > 0 && (!indices || !indices_out)))
    return fail(TTEMB_E_BADARG, "ttemb_compact_bags: null buffer");
  if ((weights == nullptr) != (weights_out == nullptr))
    return fail(TTEMB_E_BADARG, "ttemb_compact_bags: weights and weights_out are both given or both NULL");
  if (nnz > 0 && indices_out == indices) return fail(TTEMB_E_BADARG, "ttemb_compact_bags: the partition cannot run in place");
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "ttemb_compact_bags: workspace smaller than its header");
  return launch_compact_bags(indices, offsets, weights, nnz, nnz_dev, B, pad, indices_out, offsets_out, weights_out, map_out,
                             kept_dev, reinterpret_cast<char*>(workspace) + kFast3HeaderBytes,
                             workspace_bytes - kFast3HeaderBytes, reinterpret_cast<hipStream_t>(stream));
}

int ttemb_expand_kept(const float* src, const int32_t* map, int64_t nnz, const int32_t* nnz_dev, float* out, void* stream) {
  ApiRange api_range("ttemb_expand_kept");
  if (nnz < 0) return fail(TTEMB_E_BADARG, "ttemb_expand_kept: negative size");
  if (nnz > 0x7fffffffll) return fail(TTEMB_E_BADARG, "ttemb_expand_kept: nnz exceeds int32 range");
  if (nnz > 0 && (!src || !map || !out)) return fail(TTEMB_E_BADARG, "ttemb_expand_kept: null buffer");
  if (nnz > 0 && out == src) return fail(TTEMB_E_BADARG, "ttemb_expand_kept: the gather cannot run in place");
  return launch_expand_kept(src, map, nnz, nnz_dev, out, reinterpret_cast<hipStream_t>(stream));
}

static int check_cache_args(const void* loc, const void* rowidx, int64_t start, int64_t nnz, int64_t D) {
  if (nnz < 0 || start < 0) return fail(TTEMB_E_BADARG, "negative size");
  if (D <= 0 || D % 4 != 0) return fail(TTEMB_E_BADARG, "embedding_dim %lld must be a positive multiple of 4", (long long)D);
  if (nnz > 0 && (!loc || !rowidx)) return fail(TTEMB_E_BADARG, "null buffer");
  return TTEMB_OK;
}

int ttemb_cache_forward(const int32_t* cache_loc, const int64_t* rowidx, const int64_t* offsets, int64_t start,
                        const int32_t* start_dev, int64_t nnz, const float* cache_weight, int64_t D,
                        float* output, void* stream) {
  ApiRange api_range("ttemb_cache_forward");
  int rc = check_cache_args(cache_loc, rowidx, start, nnz, D);
  if (rc) return rc;
  if (nnz > 0 && (!cache_weight || !output)) return fail(TTEMB_E_BADARG, "null buffer");
  return launch_cache_forward(cache_loc, rowidx, offsets, start, start_dev, nnz, cache_weight, D, output,
                              reinterpret_cast<hipStream_t>(stream));
}

int ttemb_cache_backward_sgd(const int32_t* cache_loc, const int64_t* rowidx, int64_t start,
                             const int32_t* start_dev, int64_t nnz, const float* d_output, int64_t D,
                             float lr, float* cache_weight, const int32_t* dup_dev, void* stream) {
  ApiRange api_range("ttemb_cache_backward_sgd");
  int rc = check_cache_args(cache_loc, rowidx, start, nnz, D);
  if (rc) return rc;
  if (nnz > 0 && (!cache_weight || !d_output)) return fail(TTEMB_E_BADARG, "null buffer");
  return launch_cache_scatter_add(cache_loc, rowidx, start, start_dev, nnz, d_output, D, -lr,
                                  cache_weight, dup_dev, reinterpret_cast<hipStream_t>(stream));
}

int ttemb_cache_backward_dense(const int32_t* cache_loc, const int64_t* rowidx, int64_t start,
                               const int32_t* start_dev, int64_t nnz, const float* d_output, int64_t D,
                               int64_t C, float* d_cache_weight, const int32_t* dup_dev, void* stream) {
  ApiRange api_range("ttemb_cache_backward_dense");
  int rc = check_cache_args(cache_loc, rowidx, start, nnz, D);
  if (rc) return rc;
  if (C < 0) return fail(TTEMB_E_BADARG, "negative cache rows");
  if (C > 0 && !d_cache_weight) return fail(TTEMB_E_BADARG, "null buffer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (C > 0) {
    rc = launch_zero(d_cache_weight, (size_t)C * D * 4, st, "zero d_cache_weight");
    if (rc) return rc;
  }
  if (nnz > 0 && !d_output) return fail(TTEMB_E_BADARG, "null buffer");
  return launch_cache_scatter_add(cache_loc, rowidx, start, start_dev, nnz, d_output, D, 1.0f,
                                  d_cache_weight, dup_dev, st);
}

int ttemb_cache_backward_rowwise_adagrad(const int32_t* cache_loc, const int64_t* rowidx, int64_t start,
                                         const int32_t* start_dev, int64_t nnz, const float* d_output,
                                         int64_t D, float lr, float eps, float* cache_state_sum,
                                         float* cache_weight, void* stream) {
  ApiRange api_range("ttemb_cache_backward_rowwise_adagrad");
  int rc = check_cache_args(cache_loc, rowidx, start, nnz, D);
  if (rc) return rc;
  if (nnz > 0 && (!cache_weight || !d_output || !cache_state_sum)) return fail(TTEMB_E_BADARG, "null buffer");
  return launch_cache_rowwise_adagrad(cache_loc, rowidx, start, start_dev, nnz, d_output, D, lr, eps,
                                      cache_state_sum, cache_weight, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
