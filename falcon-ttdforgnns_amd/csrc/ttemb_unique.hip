// The distinct ids of a call, found on the device (ttemb_unique_ids, include/ttemb_unique.h): the first step
// of the `dedup` route of the pooled lookups.
//
//   sort      a stable radix sort of (id, position) pairs on the key bits [0, bit_length(rows - 1)) -- rocprim's, as
//             launch_cache_populate_rank runs it: temporary storage out of the workspace, size query at call time.  The
//             positions come from a counting iterator, the sorted positions ARE perm_out.
//   count     head flag of sorted position n: n == 0 or sorted[n] != sorted[n - 1] (the full 64-bit ids); every tile of 256
//             sorted positions leaves its number of heads.
//   scatter   the exclusive scan of the flags (the counts of the tiles before, summed by wave 0, plus a ballot rank inside
//             the tile: the rank core of the stable partitions of ttemb_cache.hip) places every head: unique_out[j] = its id,
//             seg_out[j] = n; every position learns its run: inverse_out[perm[n]] = j.  The last tile writes U.
//
// The form of the ttemb_drop_padding kernels: integer work only, tiles of 256 in grid-stride loops (the grid honours
// ttemb_set_exact_grid and decides who computes a word, never what it is), no waits between workgroups, every workspace word
// that is read was written earlier in the same call.
#include "ttemb_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace ttemb {
namespace uniq {

constexpr int kTile = 256;
constexpr int64_t kMaxIds = 0x7fffffff;   // positions are int32

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }
inline int64_t tiles_of(int64_t nnz) { return nnz > 0 ? (nnz + kTile - 1) / kTile : 1; }

// the key bits that tell the rows of the table apart (at least one: rocprim sorts a non-empty bit range)
inline int key_bits(int64_t rows) {
  int bits = 0;
  for (uint64_t v = (uint64_t)(rows - 1); v != 0; v >>= 1) ++bits;
  return bits > 0 ? bits : 1;
}

using PosIter = rocprim::counting_iterator<int32_t>;

hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const int64_t* keys, int64_t* sorted, int32_t* perm, int64_t nnz, int bits,
                      hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, sorted, PosIter(0), perm, (size_t)nnz, 0u, (unsigned)bits, st, false);
}

struct Layout {
  int64_t sorted, tilecnt, tmp, tmp_bytes, total;   // byte offsets behind the header
};

int layout_of(int64_t nnz, int64_t rows, Layout* L) {
  size_t tmp = 0;
  if (nnz > 0) {
    hipError_t e = sort_pairs(nullptr, tmp, nullptr, nullptr, nullptr, nnz, key_bits(rows), (hipStream_t)0);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs(size)");
  }
  L->sorted = 0;
  L->tilecnt = align256(nnz * 8);
  L->tmp = L->tilecnt + align256(tiles_of(nnz) * 4);
  L->tmp_bytes = (int64_t)tmp;
  L->total = L->tmp + align256((int64_t)tmp);
  return TTEMB_OK;
}

__device__ __forceinline__ bool is_head(const int64_t* __restrict__ sorted, int64_t n, int64_t nnz) {
  return n < nnz && (n == 0 || sorted[n] != sorted[n - 1]);
}

__global__ __launch_bounds__(kTile) void unique_count_kernel(const int64_t* __restrict__ sorted, int64_t nnz, int64_t tiles,
                                                             int32_t* __restrict__ tilecnt) {
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const int c = __syncthreads_count(is_head(sorted, k * kTile + threadIdx.x, nnz));
    if (threadIdx.x == 0) tilecnt[k] = c;
  }
}

__global__ __launch_bounds__(kTile) void unique_scatter_kernel(const int64_t* __restrict__ sorted, const int32_t* __restrict__ perm,
                                                               int64_t nnz, int64_t tiles, const int32_t* __restrict__ tilecnt,
                                                               int64_t* __restrict__ unique_out, int32_t* __restrict__ inverse_out,
                                                               int64_t* __restrict__ seg_out, int32_t* __restrict__ count_dev) {
  __shared__ int wave_cnt[kTile / kWave];
  __shared__ int64_t before_lds;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const int64_t n = k * kTile + threadIdx.x;
    int64_t id = 0;
    int32_t pos = 0;
    if (n < nnz) {   // independent of the counts: issued first
      id = sorted[n];
      pos = perm[n];
    }
    const bool head = is_head(sorted, n, nnz);
    if (wave == 0) {   // heads in the tiles before this one: eight loads per lane in flight, then the sums
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
      for (int d = kWave / 2; d > 0; d >>= 1) v += (int64_t)__shfl_down((long long)v, d, kWave);   // (< 2^31 heads in all)
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
    if (n < nnz) {
      // position n belongs to the run of the last head at or before it: run `before` for a head, `before - 1` otherwise
      // (position 0 is a head, so before >= 1 there).  0 <= pos < nnz: the sort permutes 0 .. nnz-1.
      const int64_t j = head ? before : before - 1;
      if (head) {
        unique_out[j] = id;
        seg_out[j] = n;
      }
      if (pos >= 0 && pos < nnz) inverse_out[pos] = (int32_t)j;
    }
    if (k == tiles - 1 && threadIdx.x == 0) {   // total = U <= nnz
      seg_out[total] = nnz;
      *count_dev = (int32_t)total;
    }
    __syncthreads();   // (this tile's LDS words are read above; the next tile rewrites them)
  }
}

}  // namespace uniq
}  // namespace ttemb

using namespace ttemb;
using namespace ttemb::uniq;

extern "C" {

int64_t ttemb_unique_ids_workspace_bytes(int64_t nnz, int64_t rows) {
  if (nnz < 0 || nnz > kMaxIds) return fail(TTEMB_E_BADARG, "ttemb_unique_ids_workspace_bytes: nnz = %lld outside [0, 2^31)", (long long)nnz);
  if (rows <= 0) return fail(TTEMB_E_BADARG, "ttemb_unique_ids_workspace_bytes: rows = %lld is not positive", (long long)rows);
  Layout L;
  int rc = layout_of(nnz, rows, &L);
  if (rc) return rc;
  return kFast3HeaderBytes + L.total;
}

int ttemb_unique_ids(const int64_t* indices, int64_t nnz, int64_t rows, int64_t* unique_out, int32_t* inverse_out,
                     int32_t* perm_out, int64_t* seg_out, int32_t* count_dev, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  if (nnz < 0 || nnz > kMaxIds) return fail(TTEMB_E_BADARG, "ttemb_unique_ids: nnz = %lld outside [0, 2^31)", (long long)nnz);
  if (rows <= 0) return fail(TTEMB_E_BADARG, "ttemb_unique_ids: rows = %lld is not positive", (long long)rows);
  if (seg_out == nullptr || count_dev == nullptr || workspace == nullptr ||
      (nnz > 0 && (indices == nullptr || unique_out == nullptr || inverse_out == nullptr || perm_out == nullptr)))
    return fail(TTEMB_E_BADARG, "ttemb_unique_ids: null buffer");
  if (workspace_bytes < kFast3HeaderBytes) return fail(TTEMB_E_WORKSPACE, "ttemb_unique_ids: workspace smaller than its header");
  Layout L;
  int rc = layout_of(nnz, rows, &L);
  if (rc) return rc;
  if (workspace_bytes < kFast3HeaderBytes + L.total)
    return fail(TTEMB_E_WORKSPACE, "ttemb_unique_ids: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)(kFast3HeaderBytes + L.total));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(workspace) + kFast3HeaderBytes;
  int64_t* sorted = reinterpret_cast<int64_t*>(base + L.sorted);
  int32_t* tilecnt = reinterpret_cast<int32_t*>(base + L.tilecnt);
  if (nnz > 0) {
    size_t tmp_bytes = (size_t)L.tmp_bytes;
    hipError_t e = sort_pairs(base + L.tmp, tmp_bytes, indices, sorted, perm_out, nnz, key_bits(rows), st);
    if (e != hipSuccess) return check_hip(e, "radix_sort_pairs");
  }
  const int64_t tiles = tiles_of(nnz);
  const unsigned grid = exact::ex_grid(tiles);
  hipLaunchKernelGGL(unique_count_kernel, dim3(grid), dim3(kTile), 0, st, sorted, nnz, tiles, tilecnt);
  if ((rc = check_hip(hipGetLastError(), "unique_count_kernel"))) return rc;
  hipLaunchKernelGGL(unique_scatter_kernel, dim3(grid), dim3(kTile), 0, st, sorted, perm_out, nnz, tiles, tilecnt, unique_out,
                     inverse_out, seg_out, count_dev);
  return check_hip(hipGetLastError(), "unique_scatter_kernel");
}

}  // extern "C"
