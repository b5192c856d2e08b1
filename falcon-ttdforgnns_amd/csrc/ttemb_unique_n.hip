// The distinct ids of the first n ids of a buffer, n read on the device (ttemb_unique_ids_n, include/ttemb_unique_n.h;
// DESIGN.md §4.16): ttemb_unique_ids (ttemb_unique.hip) in the form a captured graph can hold.  n = live_count(nnz_cap,
// nnz_dev); nothing on the host depends on it, so one capture replays for every n.  A source of its own: ttemb_unique.hip and
// the kernels it compiles to stay what they are.
//
//   keys      key[p] = id & mask for p < n, 1 << bits for a dead position (bits = key_bits(rows), mask = 2^bits - 1): one
//             bit above every live key.  Unsigned keys: with bits = 63 the dead key is the top bit.
//   sort      the stable pair sort of ttemb_unique_ids over bits + 1 bits of all nnz_cap keys: the dead positions end up
//             behind the live ones, and the live part of the sorted positions is what the sort of n ids gives (both are
//             stable on the same key bits).  Only the positions are used: perm_out.
//   count / scatter   unique_count_kernel / unique_scatter_kernel with n for nnz and the id of sorted position k read as
//             indices[perm[k]] -- the full 64-bit ids, as there.
//
// The form of ttemb_unique.hip: integer work only, tiles of 256 in grid-stride loops (the grid honours ttemb_set_exact_grid
// and decides who computes a word, never what it is), no waits between workgroups, every workspace word that is read was
// written earlier in the same call.
#include "ttemb_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace ttemb {
namespace uniqn {

// (tile, limits and key bits: those of ttemb_unique.hip)
constexpr int kTile = 256;
constexpr int64_t kMaxIds = 0x7fffffff;   // positions are int32

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }
inline int64_t tiles_of(int64_t nnz) { return nnz > 0 ? (nnz + kTile - 1) / kTile : 1; }

inline int key_bits(int64_t rows) {
  int bits = 0;
  for (uint64_t v = (uint64_t)(rows - 1); v != 0; v >>= 1) ++bits;
  return bits > 0 ? bits : 1;
}

using PosIter = rocprim::counting_iterator<int32_t>;

hipError_t sort_pairs_n(void* tmp, size_t& tmp_bytes, const uint64_t* keys, uint64_t* sorted, int32_t* perm, int64_t nnz_cap,
                        int bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, sorted, PosIter(0), perm, (size_t)nnz_cap, 0u, (unsigned)(bits + 1), st,
                                   false);
}

struct LayoutN {
  int64_t keys, sorted, tilecnt, tmp, tmp_bytes, total;   // byte offsets behind the header
};

int layout_n_of(int64_t nnz_cap, int64_t rows, hipStream_t st, LayoutN* L) {
  size_t tmp = 0;
  if (nnz_cap > 0) {   // (a function of nnz_cap and rows; `st` only names the device)
    hipError_t e = sort_pairs_n(nullptr, tmp, nullptr, nullptr, nullptr, nnz_cap, key_bits(rows), st);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs(size)");
  }
  L->keys = 0;
  L->sorted = align256(nnz_cap * 8);
  L->tilecnt = L->sorted + align256(nnz_cap * 8);
  L->tmp = L->tilecnt + align256(tiles_of(nnz_cap) * 4);
  L->tmp_bytes = (int64_t)tmp;
  L->total = L->tmp + align256((int64_t)tmp);
  return TTEMB_OK;
}

__device__ __forceinline__ int64_t tiles_of_n(int64_t n) { return n > 0 ? (n + kTile - 1) / kTile : 1; }   // tiles_of, on the device

__global__ __launch_bounds__(kTile) void unique_keys_n_kernel(const int64_t* __restrict__ indices, int64_t nnz_cap,
                                                              const int32_t* __restrict__ nnz_dev, int bits,
                                                              uint64_t* __restrict__ keys) {
  const int64_t n = live_count(nnz_cap, nnz_dev);
  const uint64_t dead = 1ull << bits, mask = dead - 1ull;
  for (int64_t p = (int64_t)blockIdx.x * kTile + threadIdx.x; p < nnz_cap; p += (int64_t)gridDim.x * kTile)
    keys[p] = p < n ? ((uint64_t)indices[p] & mask) : dead;   // (a dead id is not read)
}

// the position at sorted place k < n: a live one when the sort is what it says; clamped, so that no content can send a load astray
__device__ __forceinline__ int64_t live_pos(const int32_t* __restrict__ perm, int64_t k, int64_t n) {
  const int64_t p = perm[k];
  return p < 0 ? 0 : (p >= n ? n - 1 : p);
}

__device__ __forceinline__ bool is_head_n(const int64_t* __restrict__ indices, const int32_t* __restrict__ perm, int64_t k,
                                          int64_t n) {
  return k < n && (k == 0 || indices[live_pos(perm, k, n)] != indices[live_pos(perm, k - 1, n)]);
}

__global__ __launch_bounds__(kTile) void unique_count_n_kernel(const int64_t* __restrict__ indices, const int32_t* __restrict__ perm,
                                                               int64_t nnz_cap, const int32_t* __restrict__ nnz_dev,
                                                               int32_t* __restrict__ tilecnt) {
  const int64_t n = live_count(nnz_cap, nnz_dev);
  const int64_t tiles = tiles_of_n(n);
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const int c = __syncthreads_count(is_head_n(indices, perm, k * kTile + threadIdx.x, n));
    if (threadIdx.x == 0) tilecnt[k] = c;
  }
}

__global__ __launch_bounds__(kTile) void unique_scatter_n_kernel(const int64_t* __restrict__ indices, const int32_t* __restrict__ perm,
                                                                 int64_t nnz_cap, const int32_t* __restrict__ nnz_dev,
                                                                 const int32_t* __restrict__ tilecnt,
                                                                 int64_t* __restrict__ unique_out, int32_t* __restrict__ inverse_out,
                                                                 int64_t* __restrict__ seg_out, int32_t* __restrict__ count_dev) {
  __shared__ int wave_cnt[kTile / kWave];
  __shared__ int64_t before_lds;
  const int64_t nnz = live_count(nnz_cap, nnz_dev);
  const int64_t tiles = tiles_of_n(nnz);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const int64_t n = k * kTile + threadIdx.x;
    int64_t id = 0;
    int32_t pos = 0;
    if (n < nnz) {
      pos = perm[n];
      id = indices[live_pos(perm, n, nnz)];
    }
    const bool head = is_head_n(indices, perm, n, nnz);
    if (wave == 0) {   // heads in the tiles before this one (unique_scatter_kernel's sum)
      int64_t v = 0;
      for (int64_t b0 = 0; b0 < k; b0 += 8 * kWave) {
        int32_t c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int64_t b = b0 + i * kWave + lane;
          c[i] = b < k ? tilecnt[b] : 0;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v += c[i];
      }
#pragma unroll
      for (int d = kWave / 2; d > 0; d >>= 1) v += (int64_t)__shfl_down((long long)v, d, kWave);
      if (lane == 0) before_lds = v;
    }
    const unsigned long long ball = __ballot(head);
    if (lane == 0) wave_cnt[wave] = __popcll(ball);
    __syncthreads();
    int64_t before = before_lds + __popcll(ball & ((1ull << lane) - 1ull));   // heads before position n
    int64_t total = before_lds;
    for (int w = 0; w < kTile / kWave; ++w) {
      if (w < wave) before += wave_cnt[w];
      total += wave_cnt[w];
    }
    if (n < nnz) {   // (position 0 is a head, so before >= 1 for every other one: 0 <= j < U <= nnz)
      const int64_t j = head ? before : before - 1;
      if (head) {
        unique_out[j] = id;
        seg_out[j] = n;
      }
      if (pos >= 0 && pos < nnz) inverse_out[pos] = (int32_t)j;
    }
    if (k == tiles - 1 && threadIdx.x == 0) {   // total = U <= nnz (no live id: the one tile has no head, U = 0)
      seg_out[total] = nnz;
      *count_dev = (int32_t)total;
    }
    __syncthreads();
  }
}

}  // namespace uniqn
}  // namespace ttemb

using namespace ttemb;
using namespace ttemb::uniqn;

extern "C" {

int64_t ttemb_unique_ids_n_workspace_bytes(int64_t nnz_cap, int64_t rows) {
  if (nnz_cap < 0 || nnz_cap > kMaxIds)
    return fail(TTEMB_E_BADARG, "ttemb_unique_ids_n_workspace_bytes: nnz_cap = %lld outside [0, 2^31)", (long long)nnz_cap);
  if (rows <= 0) return fail(TTEMB_E_BADARG, "ttemb_unique_ids_n_workspace_bytes: rows = %lld is not positive", (long long)rows);
  LayoutN L;
  int rc = layout_n_of(nnz_cap, rows, (hipStream_t)0, &L);
  if (rc) return rc;
  return kFast3HeaderBytes + L.total;
}

int ttemb_unique_ids_n(const int64_t* indices, int64_t nnz_cap, const int32_t* nnz_dev, int64_t rows, int64_t* unique_out,
                       int32_t* inverse_out, int32_t* perm_out, int64_t* seg_out, int32_t* count_dev, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  if (nnz_cap < 0 || nnz_cap > kMaxIds)
    return fail(TTEMB_E_BADARG, "ttemb_unique_ids_n: nnz_cap = %lld outside [0, 2^31)", (long long)nnz_cap);
  if (rows <= 0) return fail(TTEMB_E_BADARG, "ttemb_unique_ids_n: rows = %lld is not positive", (long long)rows);
  if (seg_out == nullptr || count_dev == nullptr || workspace == nullptr ||
      (nnz_cap > 0 && (indices == nullptr || unique_out == nullptr || inverse_out == nullptr || perm_out == nullptr)))
    return fail(TTEMB_E_BADARG, "ttemb_unique_ids_n: null buffer");
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "ttemb_unique_ids_n: workspace smaller than its header");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LayoutN L;
  int rc = layout_n_of(nnz_cap, rows, st, &L);   // (the capacity's: the same in the capture and in every replay)
  if (rc) return rc;
  if (workspace_bytes < kFast3HeaderBytes + L.total)
    return fail(TTEMB_E_WORKSPACE, "ttemb_unique_ids_n: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)(kFast3HeaderBytes + L.total));
  char* base = reinterpret_cast<char*>(workspace) + kFast3HeaderBytes;
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + L.keys);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(base + L.sorted);
  int32_t* tilecnt = reinterpret_cast<int32_t*>(base + L.tilecnt);
  const unsigned grid = exact::ex_grid(tiles_of(nnz_cap));
  if (nnz_cap > 0) {
    const int bits = key_bits(rows);
    hipLaunchKernelGGL(unique_keys_n_kernel, dim3(grid), dim3(kTile), 0, st, indices, nnz_cap, nnz_dev, bits, keys);
    if ((rc = check_hip(hipGetLastError(), "unique_keys_n_kernel"))) return rc;
    size_t tmp_bytes = (size_t)L.tmp_bytes;
    hipError_t e = sort_pairs_n(base + L.tmp, tmp_bytes, keys, sorted, perm_out, nnz_cap, bits, st);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs");
  }
  hipLaunchKernelGGL(unique_count_n_kernel, dim3(grid), dim3(kTile), 0, st, indices, perm_out, nnz_cap, nnz_dev, tilecnt);
  if ((rc = check_hip(hipGetLastError(), "unique_count_n_kernel"))) return rc;
  hipLaunchKernelGGL(unique_scatter_n_kernel, dim3(grid), dim3(kTile), 0, st, indices, perm_out, nnz_cap, nnz_dev, tilecnt,
                     unique_out, inverse_out, seg_out, count_dev);
  return check_hip(hipGetLastError(), "unique_scatter_n_kernel");
}

}  // extern "C"
