// The distinct ids of a call, found on the device: the first step of the `dedup` route of the pooled lookups.  Two entry
// points over one pass: ttemb_unique_ids (include/ttemb_unique.h) takes the id count on the host;
// ttemb_unique_ids_n (include/ttemb_unique_n.h) takes the first n ids of a buffer of nnz_cap,
// n = live_count(nnz_cap, nnz_dev) read on the device -- nothing on the host depends on n, so one captured graph replays for
// every n.
//
//   sort      a stable radix sort of (id, position) pairs -- rocprim's, as launch_cache_populate_rank runs it: temporary
//             storage out of the workspace, size query at call time.  The positions come from a counting iterator, the sorted
//             positions ARE perm_out.
//               plain    the ids themselves as keys, on the key bits [0, bits), bits = bit_length(rows - 1).
//               counted  unique_keys_n_kernel writes key[p] = id & mask for p < n and 1 << bits for a dead position (mask =
//                        2^bits - 1): one bit above every live key.  Unsigned keys: with bits = 63 the dead key is the top
//                        bit.  All nnz_cap keys are sorted on bits + 1 bits: the dead positions end up behind the live ones,
//                        and the live part of the sorted positions is what the sort of n ids gives (both are stable on the
//                        same key bits).  Only the positions are used.
//   count     head flag of sorted place k: k == 0 or id(k) != id(k - 1) (the full 64-bit ids); every tile of 256 sorted
//             places leaves its number of heads.
//   scatter   the exclusive scan of the flags (partition_rank, ttemb_common.h: the counts of the tiles before, summed by wave
//             0, plus a ballot rank inside the tile) places every head: unique_out[j] = its id, seg_out[j] = k; every
//             position learns its run: inverse_out[perm[k]] = j.  The last tile writes U.
//
// count and scatter are written once (count_heads, scatter_heads) over an id list that says how many ids are live and which
// id stands at sorted place k: SortedIds (the count an argument, the sort's key output) for the plain call, PermIds (the count
// read on the device, indices[perm[k]]) for the counted one.  So ttemb_unique_ids_n with a null count gives what
// ttemb_unique_ids gives, word for word.
//
// The form of the ttemb_drop_padding kernels: integer work only, tiles of 256 in grid-stride loops (the grid honours
// ttemb_set_exact_grid and decides who computes a word, never what it is), no waits between workgroups, every workspace word
// that is read was written earlier in the same call.
#include "ttemb_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace ttemb {
namespace uniq {

constexpr int kTile = kRankTile;
constexpr int64_t kMaxIds = 0x7fffffff;   // positions are int32

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }
__host__ __device__ inline int64_t tiles_of(int64_t nnz) { return nnz > 0 ? (nnz + kTile - 1) / kTile : 1; }

// the key bits that tell the rows of the table apart (at least one: rocprim sorts a non-empty bit range)
inline int key_bits(int64_t rows) {
  int bits = 0;
  for (uint64_t v = (uint64_t)(rows - 1); v != 0; v >>= 1) ++bits;
  return bits > 0 ? bits : 1;
}

using PosIter = rocprim::counting_iterator<int32_t>;

// Key = int64_t: the plain call's ids on `bits` bits; Key = uint64_t: the counted call's keys on bits + 1
template <class Key>
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const Key* keys, Key* sorted, int32_t* perm, int64_t n, unsigned bits,
                      hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, sorted, PosIter(0), perm, (size_t)n, 0u, bits, st, false);
}

struct Layout {
  int64_t keys, sorted, tilecnt, tmp, tmp_bytes, total;   // byte offsets behind the header (keys: the counted call only)
};

// a function of n (the capacity of a counted call) and rows; `st` only names the device
int layout_of(int64_t n, int64_t rows, bool counted, hipStream_t st, Layout* L) {
  size_t tmp = 0;
  if (n > 0) {
    const int bits = key_bits(rows);
    hipError_t e = counted ? sort_pairs<uint64_t>(nullptr, tmp, nullptr, nullptr, nullptr, n, (unsigned)(bits + 1), st)
                           : sort_pairs<int64_t>(nullptr, tmp, nullptr, nullptr, nullptr, n, (unsigned)bits, st);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs(size)");
  }
  L->keys = 0;
  L->sorted = counted ? align256(n * 8) : 0;
  L->tilecnt = L->sorted + align256(n * 8);
  L->tmp = L->tilecnt + align256(tiles_of(n) * 4);
  L->tmp_bytes = (int64_t)tmp;
  L->total = L->tmp + align256((int64_t)tmp);
  return TTEMB_OK;
}

// ---- the id list of a call: how many ids are live, in how many tiles, and the id at sorted place k < count ----------------
struct SortedIds {
  const int64_t* __restrict__ sorted;
  int64_t nnz, ntiles;
  __device__ __forceinline__ int64_t count() const { return nnz; }
  __device__ __forceinline__ int64_t tiles(int64_t) const { return ntiles; }
  __device__ __forceinline__ int64_t id(int64_t k, int64_t) const { return sorted[k]; }
};

struct PermIds {
  const int64_t* __restrict__ indices;
  const int32_t* __restrict__ perm;
  int64_t nnz_cap;
  const int32_t* __restrict__ nnz_dev;
  __device__ __forceinline__ int64_t count() const { return live_count(nnz_cap, nnz_dev); }
  __device__ __forceinline__ int64_t tiles(int64_t n) const { return tiles_of(n); }
  // the position at sorted place k is a live one when the sort is what it says; clamped, so that no content can send a load astray
  __device__ __forceinline__ int64_t id(int64_t k, int64_t n) const {
    const int64_t p = perm[k];
    return indices[p < 0 ? 0 : (p >= n ? n - 1 : p)];
  }
};

template <class Ids>
__device__ __forceinline__ bool is_head(const Ids& ids, int64_t k, int64_t n) {
  return k < n && (k == 0 || ids.id(k, n) != ids.id(k - 1, n));
}

// `stride` is gridDim.x, read by the kernel: read here, next to __syncthreads_count (which reads the same word of the implicit
// kernel arguments for the workgroup's size), the two loads are merged before this body reaches the kernel, and the compiler
// then no longer folds "a full workgroup or the grid's remainder" -- two dependent vector loads in front of the loop.
template <class Ids>
__device__ __forceinline__ void count_heads(const Ids ids, int64_t stride, int32_t* __restrict__ tilecnt) {
  const int64_t nnz = ids.count(), tiles = ids.tiles(nnz);
  for (int64_t k = blockIdx.x; k < tiles; k += stride) {
    const int c = __syncthreads_count(is_head(ids, k * kTile + threadIdx.x, nnz));
    if (threadIdx.x == 0) tilecnt[k] = c;
  }
}

template <class Ids>
__device__ __forceinline__ void scatter_heads(const Ids ids, const int32_t* __restrict__ perm, const int32_t* __restrict__ tilecnt,
                                              int64_t* __restrict__ unique_out, int32_t* __restrict__ inverse_out,
                                              int64_t* __restrict__ seg_out, int32_t* __restrict__ count_dev) {
  __shared__ int wave_cnt[kTile / kWave];
  __shared__ int64_t before_lds;
  const int64_t nnz = ids.count(), tiles = ids.tiles(nnz);
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const int64_t n = k * kTile + threadIdx.x;
    int64_t id = 0;
    int32_t pos = 0;
    if (n < nnz) {   // independent of the counts: issued first
      id = ids.id(n, nnz);
      pos = perm[n];
    }
    const bool head = is_head(ids, n, nnz);
    int64_t before_tile;
    int total;
    const int64_t before = partition_rank(tilecnt, k, head, wave_cnt, nullptr, &before_lds, before_tile, total);   // heads before place n
    if (n < nnz) {
      // place n belongs to the run of the last head at or before it: run `before` for a head, `before - 1` otherwise
      // (place 0 is a head, so before >= 1 there: 0 <= j < U <= nnz).  0 <= pos < nnz when the sort permutes 0 .. nnz-1.
      const int64_t j = head ? before : before - 1;
      if (head) {
        unique_out[j] = id;
        seg_out[j] = n;
      }
      if (pos >= 0 && pos < nnz) inverse_out[pos] = (int32_t)j;
    }
    if (k == tiles - 1 && threadIdx.x == 0) {   // U <= nnz (no live id: the one tile has no head, U = 0)
      const int64_t U = before_tile + total;
      seg_out[U] = nnz;
      *count_dev = (int32_t)U;
    }
    __syncthreads();   // (this tile's LDS words are read above; the next tile rewrites them)
  }
}

__global__ __launch_bounds__(kTile) void unique_count_kernel(const int64_t* __restrict__ sorted, int64_t nnz, int64_t tiles,
                                                             int32_t* __restrict__ tilecnt) {
  count_heads(SortedIds{sorted, nnz, tiles}, gridDim.x, tilecnt);
}

__global__ __launch_bounds__(kTile) void unique_scatter_kernel(const int64_t* __restrict__ sorted, const int32_t* __restrict__ perm,
                                                               int64_t nnz, int64_t tiles, const int32_t* __restrict__ tilecnt,
                                                               int64_t* __restrict__ unique_out, int32_t* __restrict__ inverse_out,
                                                               int64_t* __restrict__ seg_out, int32_t* __restrict__ count_dev) {
  scatter_heads(SortedIds{sorted, nnz, tiles}, perm, tilecnt, unique_out, inverse_out, seg_out, count_dev);
}

__global__ __launch_bounds__(kTile) void unique_keys_n_kernel(const int64_t* __restrict__ indices, int64_t nnz_cap,
                                                              const int32_t* __restrict__ nnz_dev, int bits,
                                                              uint64_t* __restrict__ keys) {
  const int64_t n = live_count(nnz_cap, nnz_dev);
  const uint64_t dead = 1ull << bits, mask = dead - 1ull;
  for (int64_t p = (int64_t)blockIdx.x * kTile + threadIdx.x; p < nnz_cap; p += (int64_t)gridDim.x * kTile)
    keys[p] = p < n ? ((uint64_t)indices[p] & mask) : dead;   // (a dead id is not read)
}

__global__ __launch_bounds__(kTile) void unique_count_n_kernel(const int64_t* __restrict__ indices, const int32_t* __restrict__ perm,
                                                               int64_t nnz_cap, const int32_t* __restrict__ nnz_dev,
                                                               int32_t* __restrict__ tilecnt) {
  count_heads(PermIds{indices, perm, nnz_cap, nnz_dev}, gridDim.x, tilecnt);
}

__global__ __launch_bounds__(kTile) void unique_scatter_n_kernel(const int64_t* __restrict__ indices, const int32_t* __restrict__ perm,
                                                                 int64_t nnz_cap, const int32_t* __restrict__ nnz_dev,
                                                                 const int32_t* __restrict__ tilecnt,
                                                                 int64_t* __restrict__ unique_out, int32_t* __restrict__ inverse_out,
                                                                 int64_t* __restrict__ seg_out, int32_t* __restrict__ count_dev) {
  scatter_heads(PermIds{indices, perm, nnz_cap, nnz_dev}, perm, tilecnt, unique_out, inverse_out, seg_out, count_dev);
}

// ---- host: the checks of both entry points (`what`: the entry point, `nname`: what it calls its id count) ------------------
int check_sizes(const char* what, const char* nname, int64_t n, int64_t rows) {
  if (n < 0 || n > kMaxIds) return fail(TTEMB_E_BADARG, "%s: %s = %lld outside [0, 2^31)", what, nname, (long long)n);
  if (rows <= 0) return fail(TTEMB_E_BADARG, "%s: rows = %lld is not positive", what, (long long)rows);
  return TTEMB_OK;
}

int64_t workspace_bytes_of(const char* what, const char* nname, int64_t n, int64_t rows, bool counted) {
  int rc = check_sizes(what, nname, n, rows);
  if (rc) return rc;
  Layout L;
  if ((rc = layout_of(n, rows, counted, (hipStream_t)0, &L))) return rc;
  return kFast3HeaderBytes + L.total;
}

// ttemb_unique_ids (`nname` = "nnz", counted = false, nnz_dev unused) and ttemb_unique_ids_n (n = the capacity): the checks, the
// layout -- the capacity's, so the same in a capture and in every replay -- and the sort, the count and the scatter
int unique_call(const char* what, const char* nname, bool counted, const int64_t* indices, int64_t n, const int32_t* nnz_dev,
                int64_t rows, int64_t* unique_out, int32_t* inverse_out, int32_t* perm_out, int64_t* seg_out, int32_t* count_dev,
                void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(what, nname, n, rows);
  if (rc) return rc;
  if (seg_out == nullptr || count_dev == nullptr || workspace == nullptr ||
      (n > 0 && (indices == nullptr || unique_out == nullptr || inverse_out == nullptr || perm_out == nullptr)))
    return fail(TTEMB_E_BADARG, "%s: null buffer", what);
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "%s: workspace smaller than its header", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Layout L;
  if ((rc = layout_of(n, rows, counted, counted ? st : (hipStream_t)0, &L))) return rc;
  if (workspace_bytes < kFast3HeaderBytes + L.total)
    return fail(TTEMB_E_WORKSPACE, "%s: workspace of %lld bytes, need %lld", what, (long long)workspace_bytes,
                (long long)(kFast3HeaderBytes + L.total));
  char* base = reinterpret_cast<char*>(workspace) + kFast3HeaderBytes;
  int32_t* tilecnt = reinterpret_cast<int32_t*>(base + L.tilecnt);
  size_t tmp_bytes = (size_t)L.tmp_bytes;
  const int bits = key_bits(rows);
  const int64_t tiles = tiles_of(n);
  const dim3 grid(exact::ex_grid(tiles)), nt(kTile);
  if (!counted) {
    int64_t* sorted = reinterpret_cast<int64_t*>(base + L.sorted);
    if (n > 0) {
      hipError_t e = sort_pairs<int64_t>(base + L.tmp, tmp_bytes, indices, sorted, perm_out, n, (unsigned)bits, st);
      if (e != hipSuccess) return check_hip(e, "radix_sort_pairs");
    }
    hipLaunchKernelGGL(unique_count_kernel, grid, nt, 0, st, sorted, n, tiles, tilecnt);
    if ((rc = check_hip(hipGetLastError(), "unique_count_kernel"))) return rc;
    hipLaunchKernelGGL(unique_scatter_kernel, grid, nt, 0, st, sorted, perm_out, n, tiles, tilecnt, unique_out, inverse_out, seg_out,
                       count_dev);
    return check_hip(hipGetLastError(), "unique_scatter_kernel");
  }
  if (n > 0) {
    uint64_t* keys = reinterpret_cast<uint64_t*>(base + L.keys);
    hipLaunchKernelGGL(unique_keys_n_kernel, grid, nt, 0, st, indices, n, nnz_dev, bits, keys);
    if ((rc = check_hip(hipGetLastError(), "unique_keys_n_kernel"))) return rc;
    hipError_t e = sort_pairs<uint64_t>(base + L.tmp, tmp_bytes, keys, reinterpret_cast<uint64_t*>(base + L.sorted), perm_out, n,
                                        (unsigned)(bits + 1), st);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs");
  }
  hipLaunchKernelGGL(unique_count_n_kernel, grid, nt, 0, st, indices, perm_out, n, nnz_dev, tilecnt);
  if ((rc = check_hip(hipGetLastError(), "unique_count_n_kernel"))) return rc;
  hipLaunchKernelGGL(unique_scatter_n_kernel, grid, nt, 0, st, indices, perm_out, n, nnz_dev, tilecnt, unique_out, inverse_out,
                     seg_out, count_dev);
  return check_hip(hipGetLastError(), "unique_scatter_n_kernel");
}

}  // namespace uniq
}  // namespace ttemb

using namespace ttemb;
using namespace ttemb::uniq;

extern "C" {

int64_t ttemb_unique_ids_workspace_bytes(int64_t nnz, int64_t rows) {
  return workspace_bytes_of("ttemb_unique_ids_workspace_bytes", "nnz", nnz, rows, false);
}

int64_t ttemb_unique_ids_n_workspace_bytes(int64_t nnz_cap, int64_t rows) {
  return workspace_bytes_of("ttemb_unique_ids_n_workspace_bytes", "nnz_cap", nnz_cap, rows, true);
}

int ttemb_unique_ids(const int64_t* indices, int64_t nnz, int64_t rows, int64_t* unique_out, int32_t* inverse_out,
                     int32_t* perm_out, int64_t* seg_out, int32_t* count_dev, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  return unique_call("ttemb_unique_ids", "nnz", false, indices, nnz, nullptr, rows, unique_out, inverse_out, perm_out, seg_out,
                     count_dev, workspace, workspace_bytes, stream);
}

int ttemb_unique_ids_n(const int64_t* indices, int64_t nnz_cap, const int32_t* nnz_dev, int64_t rows, int64_t* unique_out,
                       int32_t* inverse_out, int32_t* perm_out, int64_t* seg_out, int32_t* count_dev, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return unique_call("ttemb_unique_ids_n", "nnz_cap", true, indices, nnz_cap, nnz_dev, rows, unique_out, inverse_out, perm_out,
                     seg_out, count_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
