// Bag pooling around the lookups: per-sample weights (mode "sum") and mean pooling (include/ttemb.h, "Weighted and mean
// bags").  The TT kernels are not touched: a weighted call looks up one row per id (bags of one) and reduces those rows
// here; a mean call divides the bag sums of the plain lookup by the bag lengths.
//
//   reduce     out[b] = sum_{i in bag b} w[i] rows[i], ids in position order.  A bag of at most kBagChunk ids is summed
//              by one lane group; a longer bag is cut into the fixed chunks [k C, (k+1) C) of the position list
//              (bag_partial_kernel writes one partial per chunk it reaches) and its partials are added in chunk order.
//   backward   d_rows[i] = w[i] dOut[bag(i)] and d_w[i] = <dOut[bag(i)], rows[i]> in one pass, one lane group per id.
//   mean       dst[b] = src[b] / len(b), zeros for an empty bag.
//   max        out[b][d] = max_{i in bag b} rows[i][d] and argmax[b][d] = the FIRST position that holds it (-1 without one);
//              a NaN in a kept position wins over every number (the first NaN position).  Long bags go through the same
//              fixed chunks as the sums: per chunk the partial (value, position), combined in chunk order by the same
//              strict rule, so the first position still wins.  The backward sends dOut[b][d] to that position alone.
//   mapped     reduce over rows[map[i]] (one row per DISTINCT id: the dedup route, include/ttemb_unique.h) with the same
//              chunks; its backward sums, per distinct id, the gradients of its positions in position order.
//
// The three sums (reduce, mapped reduce, the mapped backward) are one chunked segment sum: chunk_partials / segment_sums
// below hold the chunks, the two slots per chunk and the chunk order once, and the kernels are wrappers that say what the
// segments and the terms are.  The max kernels have another combine rule and carry positions: they stand apart.
//
// Every kernel is deterministic by construction, in the sense of the exact-mode contract: no float atomics, no waits
// between workgroups, grid-stride loops over work items (the grid decides who computes a value, never how), summation
// orders set by `offsets` (and D) alone, and every workspace word that is read was written earlier in the same call.
// Their grids honour ttemb_set_exact_grid.
//
// The *_n entry points take a device id count (`nnz_dev`, nullable: the lookups' convention, live_count()): with
// c = min(nnz, *nnz_dev) every kernel uses c where it would use nnz -- bags are clamped to c, the loops over positions and
// over chunks stop at c, nothing at a position >= c is read or written -- while the launches and the workspace stay sized by
// nnz, the capacity.  Chunks are cut from position 0, so the live part is bit for bit what a call with nnz = c gives.  The
// entry points without the suffix are those calls with nnz_dev = NULL.
//
// Lane groups: a group of W lanes (W = the power of two >= D / 4, at most 64) owns one bag / chunk / id and walks its
// row in float4 columns, W at a time; a workgroup holds kBagNT / W groups.
#include "ttemb_common.h"

namespace ttemb {
namespace bag {

constexpr int kBagNT = 256;               // threads per workgroup
constexpr int64_t kBagChunk = 512;        // ids per chunk of a long bag
constexpr int64_t kBagHeader = kFast3HeaderBytes;   // the workspace header of the grouped lookups: never written here
constexpr int64_t kBagMaxIds = 0x7fffffff;   // max bags keep their winners as int32 positions

struct Groups {
  int shift;   // log2(W)
  int per_block;
};

Groups groups_of(int64_t D4) {
  int shift = 0;
  while ((int64_t(1) << shift) < D4 && shift < 6) ++shift;
  return Groups{shift, kBagNT >> shift};
}

__host__ __device__ inline int64_t chunks_of(int64_t nnz) { return (nnz + kBagChunk - 1) / kBagChunk; }

__device__ __forceinline__ float4 f4_scale(float w, float4 r) { return make_float4(w * r.x, w * r.y, w * r.z, w * r.w); }

__device__ __forceinline__ float4 f4_fma(float w, float4 r, float4 a) {
  return make_float4(fmaf(w, r.x, a.x), fmaf(w, r.y, a.y), fmaf(w, r.z, a.z), fmaf(w, r.w, a.w));
}

__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// [n0, n1) of bag b, clamped to the id list (a bag past the list is empty)
__device__ __forceinline__ void bag_range(const int64_t* __restrict__ offsets, int64_t nnz, int64_t b, int64_t& n0, int64_t& n1) {
  n0 = offsets[b];
  n1 = offsets[b + 1];
  n0 = n0 < 0 ? 0 : (n0 > nnz ? nnz : n0);
  n1 = n1 < n0 ? n0 : (n1 > nnz ? nnz : n1);
}

// ---- the chunked segment sum ---------------------------------------------------------------------------------------------------
// A position list cut into segments, one sum of terms per segment and column.  Written once, over two answers:
//   Segs    `end` positions in `count` segments; of(n) = the segment that holds position n, range(j) = [n0, n1) of segment j,
//           clamped to the list.  BagSegs: the id list in bags; SortedSegs: the sorted list in runs of one distinct id.
//   Terms   sum(D4, c, a, e) = the sum of the terms [a, e) of column c, in order (a < e): the first term a product (or a plain
//           load), every later term one fma (or one add).  RowTerms, MappedTerms, GradTerms below.
// The chunks, the two slots per chunk and the order in which partials are added are the same for every pair, so equal
// terms give equal bits whichever pair summed them.
struct BagSegs {
  const int64_t* __restrict__ offsets;
  int64_t count, end;   // B and the live id count
  __device__ __forceinline__ int64_t of(int64_t n) const { return bag_of_position(offsets, count, n); }
  __device__ __forceinline__ void range(int64_t b, int64_t& n0, int64_t& n1) const { bag_range(offsets, end, b, n0, n1); }
};

// terms w[i] rows[i][c]
struct RowTerms {
  const float4* __restrict__ rows;
  const float* __restrict__ w;
  __device__ __forceinline__ float4 sum(int64_t D4, int64_t c, int64_t a, int64_t e) const {
    float4 acc = f4_scale(w[a], rows[a * D4 + c]);
#pragma unroll 8
    for (int64_t i = a + 1; i < e; ++i) acc = f4_fma(w[i], rows[i * D4 + c], acc);
    return acc;
  }
};

// Chunk k = positions [k C, (k+1) C): the part of every LONG segment (more than C positions) that lies in it goes to one of
// the chunk's two slots -- slot 0 for the segment that began before the chunk, slot 1 for the segment that begins inside it (a
// long segment cannot lie wholly inside a chunk, so there are at most these two).  Short segments are summed by segment_sums.
template <class Segs, class Terms>
__device__ __forceinline__ void chunk_partials(const Segs segs, const Terms terms, int64_t D4, int shift,
                                               float4* __restrict__ partial) {
  const int64_t end = segs.end, nchunks = chunks_of(end);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  for (int64_t k = (int64_t)blockIdx.x * per_block + g; k < nchunks; k += (int64_t)gridDim.x * per_block) {
    const int64_t s = k * kBagChunk, e = s + kBagChunk < end ? s + kBagChunk : end;
    const int64_t js = segs.of(s), je = segs.of(e - 1);
    for (int which = 0; which < 2; ++which) {
      const int64_t j = which == 0 ? js : je;
      if (which == 1 && je == js) break;
      int64_t n0, n1;
      segs.range(j, n0, n1);
      const int64_t a = n0 > s ? n0 : s, z = n1 < e ? n1 : e;
      if (n1 - n0 <= kBagChunk || a >= z) continue;
      float4* dst = partial + (2 * k + (n0 < s ? 0 : 1)) * D4;
      for (int64_t c = lane; c < D4; c += W) dst[c] = terms.sum(D4, c, a, z);
    }
  }
}

// out[j], j < count: a short segment is one sum in position order (a segment of one term a scale and a store); a long one the
// sum of its chunk partials in chunk order (its first chunk's slot 1, then slot 0 of every later chunk it reaches); an empty
// one zeros.  One lane group per segment.
template <class Segs, class Terms>
__device__ __forceinline__ void segment_sums(const Segs segs, const Terms terms, int64_t D4, int shift,
                                             const float4* __restrict__ partial, float4* __restrict__ out) {
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  for (int64_t j = (int64_t)blockIdx.x * per_block + g; j < segs.count; j += (int64_t)gridDim.x * per_block) {
    int64_t n0, n1;
    segs.range(j, n0, n1);
    float4* dst = out + j * D4;
    if (n1 - n0 > kBagChunk) {
      const int64_t k0 = n0 / kBagChunk, k1 = (n1 - 1) / kBagChunk;
      for (int64_t c = lane; c < D4; c += W) {
        float4 acc = partial[(2 * k0 + 1) * D4 + c];
#pragma unroll 8
        for (int64_t k = k0 + 1; k <= k1; ++k) acc = f4_add(acc, partial[2 * k * D4 + c]);
        dst[c] = acc;
      }
    } else if (n1 > n0) {
      for (int64_t c = lane; c < D4; c += W) dst[c] = terms.sum(D4, c, n0, n1);
    } else {
      for (int64_t c = lane; c < D4; c += W) dst[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  }
}

// out[b] = sum_{i in bag b} w[i] rows[i]: the chunk partials of the long bags, then every bag
__global__ __launch_bounds__(kBagNT) void bag_partial_kernel(const float4* __restrict__ rows, const float* __restrict__ w,
                                                             const int64_t* __restrict__ offsets, int64_t nnz,
                                                             const int32_t* __restrict__ nnz_dev, int64_t B, int64_t D4,
                                                             int shift, float4* __restrict__ partial) {
  chunk_partials(BagSegs{offsets, B, live_count(nnz, nnz_dev)}, RowTerms{rows, w}, D4, shift, partial);
}

__global__ __launch_bounds__(kBagNT) void bag_reduce_kernel(const float4* __restrict__ rows, const float* __restrict__ w,
                                                            const int64_t* __restrict__ offsets, int64_t nnz,
                                                            const int32_t* __restrict__ nnz_dev, int64_t B, int64_t D4,
                                                            int shift, const float4* __restrict__ partial,
                                                            float4* __restrict__ out) {
  segment_sums(BagSegs{offsets, B, live_count(nnz, nnz_dev)}, RowTerms{rows, w}, D4, shift, partial, out);
}

// dot + <g, r>, x to w in order
__device__ __forceinline__ float dot4(float4 g, float4 r, float dot) {
  dot = fmaf(g.x, r.x, dot);
  dot = fmaf(g.y, r.y, dot);
  dot = fmaf(g.z, r.z, dot);
  return fmaf(g.w, r.w, dot);
}

// the sum of v over the W lanes of a group, on every lane: a butterfly, a fixed tree for a given W
__device__ __forceinline__ float group_sum(float v, int W) {
  for (int m = W >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, W);
  return v;
}

// d_rows[i] = w[i] dOut[bag(i)]; d_w[i] = <dOut[bag(i)], rows[i]> (each lane sums its columns in order, then a butterfly
// over the group's W lanes: a fixed tree for a given D).  An id outside every bag gets zeros.
__global__ __launch_bounds__(kBagNT) void bag_reduce_backward_kernel(const float4* __restrict__ d_out,
                                                                     const float* __restrict__ w,
                                                                     const float4* __restrict__ rows,
                                                                     const int64_t* __restrict__ offsets, int64_t nnz,
                                                                     const int32_t* __restrict__ nnz_dev, int64_t B,
                                                                     int64_t D4, int shift, float4* __restrict__ d_rows,
                                                                     float* __restrict__ d_w) {
  nnz = live_count(nnz, nnz_dev);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  const int64_t first = offsets[0], last = offsets[B];
  const int64_t passes = (D4 + W - 1) >> shift;
  for (int64_t i = (int64_t)blockIdx.x * per_block + g; i < nnz; i += (int64_t)gridDim.x * per_block) {
    const bool in_bag = i >= first && i < last;
    const int64_t b = in_bag ? bag_of_position(offsets, B, i) : 0;
    const float wi = w[i];
    float dot = 0.0f;
    for (int64_t k = 0; k < passes; ++k) {   // the same trip count on every lane of the group (the butterfly needs them all)
      const int64_t c = lane + (k << shift);
      if (c < D4) {
        const float4 gv = in_bag ? d_out[b * D4 + c] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        d_rows[i * D4 + c] = f4_scale(wi, gv);
        if (d_w != nullptr) dot = dot4(gv, rows[i * D4 + c], dot);
      }
    }
    if (d_w != nullptr) {
      dot = group_sum(dot, W);
      if (lane == 0) d_w[i] = dot;
    }
  }
}

// dst[b] = src[b] / len(b) (a division, as torch's mean bags); an empty bag gives zeros whatever src holds
__global__ __launch_bounds__(kBagNT) void bag_mean_kernel(const float4* src, float4* dst, const int64_t* __restrict__ offsets,
                                                          int64_t B, int64_t D4, int shift) {
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  for (int64_t b = (int64_t)blockIdx.x * per_block + g; b < B; b += (int64_t)gridDim.x * per_block) {
    const int64_t len = offsets[b + 1] - offsets[b];
    const float n = (float)len;
    for (int64_t c = lane; c < D4; c += W) {
      const float4 v = src[b * D4 + c];
      dst[b * D4 + c] = len > 0 ? make_float4(v.x / n, v.y / n, v.z / n, v.w / n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  }
}

// Masked rows of a padded call: w_out[i] = keep[i] (w[i] or 1) (mean ? 1 / len'(bag(i)) : 1), keep[i] = indices[i] != pad,
// len' = the kept ids of the bag.  One wavefront per bag (a count by ballots, then the stores); positions outside every bag
// get 0.  A bag of no kept id gets zeros whatever its weights.
__global__ __launch_bounds__(kBagNT) void pad_weights_kernel(const int64_t* __restrict__ indices, const int64_t* __restrict__ offsets,
                                                             const float* __restrict__ w, int64_t nnz,
                                                             const int32_t* __restrict__ nnz_dev, int64_t B, int64_t pad,
                                                             int mean, float* __restrict__ w_out) {
  nnz = live_count(nnz, nnz_dev);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t per_block = kBagNT / kWave;
  const int64_t stride = (int64_t)gridDim.x * per_block;
  for (int64_t b = (int64_t)blockIdx.x * per_block + (threadIdx.x / kWave); b < B; b += stride) {
    int64_t n0, n1;
    bag_range(offsets, nnz, b, n0, n1);
    float scale = 1.0f;
    if (mean) {
      int64_t kept = 0;
      for (int64_t i0 = n0; i0 < n1; i0 += kWave) {
        const int64_t i = i0 + lane;
        kept += __popcll(__ballot(i < n1 && indices[i] != pad));
      }
      scale = kept > 0 ? 1.0f / (float)kept : 0.0f;
    }
    for (int64_t i = n0 + lane; i < n1; i += kWave)
      w_out[i] = indices[i] != pad ? (w != nullptr ? w[i] * scale : scale) : 0.0f;
  }
  // positions before the first bag / after the last one
  int64_t first = offsets[0], last = offsets[B];
  first = first < 0 ? 0 : (first > nnz ? nnz : first);
  last = last < first ? first : (last > nnz ? nnz : last);
  const int64_t outside = first + (nnz - last);
  for (int64_t j = (int64_t)blockIdx.x * kBagNT + threadIdx.x; j < outside; j += (int64_t)gridDim.x * kBagNT)
    w_out[j < first ? j : last + (j - first)] = 0.0f;
}

// ---- max bags ------------------------------------------------------------------------------------------------------------
// The winner of a (bag, column) so far: its value and its position in the id list (p < 0: none yet).  `take` is the whole
// rule: the first kept position is taken, then only a strictly larger value, or the first NaN over a number.
struct Best4 {
  float4 v;
  int4 p;
};

__device__ __forceinline__ void max_take(float& best, int& pos, float v, int i) {
  const bool take = pos < 0 || v > best || (v != v && best == best);
  best = take ? v : best;
  pos = take ? i : pos;
}

__device__ __forceinline__ void max_take4(Best4& b, float4 v, int4 p) {
  if (p.x >= 0) max_take(b.v.x, b.p.x, v.x, p.x);
  if (p.y >= 0) max_take(b.v.y, b.p.y, v.y, p.y);
  if (p.z >= 0) max_take(b.v.z, b.p.z, v.z, p.z);
  if (p.w >= 0) max_take(b.v.w, b.p.w, v.w, p.w);
}

__device__ __forceinline__ Best4 best_none() { return Best4{make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_int4(-1, -1, -1, -1)}; }

// the winners of column c over positions [a, e) in position order; with `indices`, positions whose raw id is `pad` are skipped
__device__ __forceinline__ Best4 max_walk(const float4* __restrict__ rows, const int64_t* __restrict__ indices, int64_t pad,
                                          int64_t D4, int64_t c, int64_t a, int64_t e) {
  Best4 b = best_none();
#pragma unroll 4
  for (int64_t i = a; i < e; ++i) {
    if (indices != nullptr && indices[i] == pad) continue;
    const int n = (int)i;
    max_take4(b, rows[i * D4 + c], make_int4(n, n, n, n));
  }
  return b;
}

// As bag_partial_kernel: the part of every LONG bag that lies in chunk k goes to one of the chunk's two slots, here as the
// partial winners (values in pv, positions in pp; a part of pads only leaves positions of -1).
__global__ __launch_bounds__(kBagNT) void bag_max_partial_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ indices,
                                                                 int64_t pad, const int64_t* __restrict__ offsets, int64_t nnz,
                                                                 const int32_t* __restrict__ nnz_dev, int64_t B, int64_t D4,
                                                                 int shift, float4* __restrict__ pv, int4* __restrict__ pp) {
  nnz = live_count(nnz, nnz_dev);
  const int64_t nchunks = chunks_of(nnz);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  for (int64_t k = (int64_t)blockIdx.x * per_block + g; k < nchunks; k += (int64_t)gridDim.x * per_block) {
    const int64_t s = k * kBagChunk, e = s + kBagChunk < nnz ? s + kBagChunk : nnz;
    const int64_t bs = bag_of_position(offsets, B, s), be = bag_of_position(offsets, B, e - 1);
    for (int which = 0; which < 2; ++which) {
      const int64_t b = which == 0 ? bs : be;
      if (which == 1 && be == bs) break;
      int64_t n0, n1;
      bag_range(offsets, nnz, b, n0, n1);
      const int64_t a = n0 > s ? n0 : s, z = n1 < e ? n1 : e;
      if (n1 - n0 <= kBagChunk || a >= z) continue;
      const int64_t slot = (2 * k + (n0 < s ? 0 : 1)) * D4;
      for (int64_t c = lane; c < D4; c += W) {
        const Best4 w = max_walk(rows, indices, pad, D4, c, a, z);
        pv[slot + c] = w.v;
        pp[slot + c] = w.p;
      }
    }
  }
}

// out[b] and argmax[b]: a short bag is one walk in position order (a bag of one a copy); a long bag the combination of its
// chunk partials in chunk order (its first chunk's slot 1, then slot 0 of every later chunk it reaches); without a winner
// (an empty bag, a bag of pads only) zeros and -1.
__global__ __launch_bounds__(kBagNT) void bag_max_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ indices,
                                                         int64_t pad, const int64_t* __restrict__ offsets, int64_t nnz,
                                                         const int32_t* __restrict__ nnz_dev, int64_t B, int64_t D4, int shift,
                                                         const float4* __restrict__ pv, const int4* __restrict__ pp,
                                                         float4* __restrict__ out, int4* __restrict__ argmax) {
  nnz = live_count(nnz, nnz_dev);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  for (int64_t b = (int64_t)blockIdx.x * per_block + g; b < B; b += (int64_t)gridDim.x * per_block) {
    int64_t n0, n1;
    bag_range(offsets, nnz, b, n0, n1);
    const bool is_long = n1 - n0 > kBagChunk;
    const int64_t k0 = n0 / kBagChunk, k1 = is_long ? (n1 - 1) / kBagChunk : k0;
    for (int64_t c = lane; c < D4; c += W) {
      Best4 w;
      if (is_long) {
        w = Best4{pv[(2 * k0 + 1) * D4 + c], pp[(2 * k0 + 1) * D4 + c]};
        for (int64_t k = k0 + 1; k <= k1; ++k) max_take4(w, pv[2 * k * D4 + c], pp[2 * k * D4 + c]);
      } else {
        w = max_walk(rows, indices, pad, D4, c, n0, n1);
      }
      out[b * D4 + c] = make_float4(w.p.x < 0 ? 0.0f : w.v.x, w.p.y < 0 ? 0.0f : w.v.y, w.p.z < 0 ? 0.0f : w.v.z,
                                    w.p.w < 0 ? 0.0f : w.v.w);
      argmax[b * D4 + c] = w.p;
    }
  }
}

// d_rows[i][d] = dOut[bag(i)][d] where position i is the winner of (bag(i), d), else 0; every element is written (zeros for
// a position outside every bag).  One lane group per id.
__global__ __launch_bounds__(kBagNT) void bag_max_backward_kernel(const float4* __restrict__ d_out, const int4* __restrict__ argmax,
                                                                  const int64_t* __restrict__ offsets, int64_t nnz,
                                                                  const int32_t* __restrict__ nnz_dev, int64_t B, int64_t D4,
                                                                  int shift, float4* __restrict__ d_rows) {
  nnz = live_count(nnz, nnz_dev);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  const int64_t first = offsets[0], last = offsets[B];
  for (int64_t i = (int64_t)blockIdx.x * per_block + g; i < nnz; i += (int64_t)gridDim.x * per_block) {
    const bool in_bag = i >= first && i < last;
    const int64_t b = in_bag ? bag_of_position(offsets, B, i) : 0;
    const int n = (int)i;
    for (int64_t c = lane; c < D4; c += W) {
      float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (in_bag) {
        const int4 p = argmax[b * D4 + c];
        if (p.x == n || p.y == n || p.z == n || p.w == n) {
          const float4 gv = d_out[b * D4 + c];
          d = make_float4(p.x == n ? gv.x : 0.0f, p.y == n ? gv.y : 0.0f, p.z == n ? gv.z : 0.0f, p.w == n ? gv.w : 0.0f);
        }
      }
      d_rows[i * D4 + c] = d;
    }
  }
}

// ---- pooling through a map (the dedup route: include/ttemb_unique.h) ---------------------------------------
// The rows buffer holds one row per DISTINCT id ([cap][D]); position n of the id list reads rows[map[n]].  The forward is
// chunk_partials / segment_sums over the same bags with that indirection in the terms, so for equal row bits it gives the
// plain pool's bits on the expanded rows.  WEIGHTED = false is a weight of 1 without the loads: 1 * r and fma(1, r, a) round
// as r and r + a.  The five kernels take the device id count of the *_n convention above (include/ttemb_unique_n.h): every
// one uses c = live_count(nnz, nnz_dev) where it would use nnz.
__device__ __forceinline__ int64_t clamp_row(int32_t m, int64_t cap) { return m < 0 ? 0 : (m >= cap ? cap - 1 : (int64_t)m); }

// terms w[n] rows[map[n]][c]
template <bool WEIGHTED>
struct MappedTerms {
  const float4* __restrict__ rows;
  int64_t cap;
  const int32_t* __restrict__ map;
  const float* __restrict__ w;
  __device__ __forceinline__ float4 sum(int64_t D4, int64_t c, int64_t a, int64_t e) const {
    float4 acc = rows[clamp_row(map[a], cap) * D4 + c];
    if constexpr (WEIGHTED) acc = f4_scale(w[a], acc);
#pragma unroll 8
    for (int64_t n = a + 1; n < e; ++n) {
      const float4 r = rows[clamp_row(map[n], cap) * D4 + c];
      if constexpr (WEIGHTED) acc = f4_fma(w[n], r, acc); else acc = f4_add(r, acc);
    }
    return acc;
  }
};

template <bool WEIGHTED>
__global__ __launch_bounds__(kBagNT) void bag_partial_mapped_kernel(const float4* __restrict__ rows, int64_t cap,
                                                                    const int32_t* __restrict__ map, const float* __restrict__ w,
                                                                    const int64_t* __restrict__ offsets, int64_t nnz,
                                                                    const int32_t* __restrict__ nnz_dev, int64_t B,
                                                                    int64_t D4, int shift, float4* __restrict__ partial) {
  chunk_partials(BagSegs{offsets, B, live_count(nnz, nnz_dev)}, MappedTerms<WEIGHTED>{rows, cap, map, w}, D4, shift, partial);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kBagNT) void bag_reduce_mapped_kernel(const float4* __restrict__ rows, int64_t cap,
                                                                   const int32_t* __restrict__ map, const float* __restrict__ w,
                                                                   const int64_t* __restrict__ offsets, int64_t nnz,
                                                                   const int32_t* __restrict__ nnz_dev, int64_t B,
                                                                   int64_t D4, int shift, const float4* __restrict__ partial,
                                                                   float4* __restrict__ out) {
  segment_sums(BagSegs{offsets, B, live_count(nnz, nnz_dev)}, MappedTerms<WEIGHTED>{rows, cap, map, w}, D4, shift, partial, out);
}

// The backward sums, per distinct id j < U, the gradients of its positions: the sorted position list perm (positions by id,
// equal ids in position order) with the segments seg in the role of the id list with its offsets -- segment j is
// [seg[j], seg[j + 1]) and its term k is w[perm[k]] dOut[bag(perm[k])], zero for a position outside every bag.
__device__ __forceinline__ int64_t clamp_to(int64_t p, int64_t hi) { return p < 0 ? 0 : (p > hi ? hi : p); }

struct SortedSegs {
  const int64_t* __restrict__ seg;
  int64_t count, end;   // U and seg[U], the end of the sorted list
  // the segment of sorted position k: the last j < U with seg[j] <= k (seg[0] = 0 <= k)
  __device__ __forceinline__ int64_t of(int64_t k) const {
    int64_t lo = 0, hi = count;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (seg[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
  }
  // [s0, s1) of segment j, clamped to the sorted list like bag_range
  __device__ __forceinline__ void range(int64_t j, int64_t& s0, int64_t& s1) const {
    s0 = clamp_to(seg[j], end);
    s1 = clamp_to(seg[j + 1], end);
    s1 = s1 < s0 ? s0 : s1;
  }
};

// bagidx[n] = the bag of position n, -1 outside every bag: one thread per position, so the binary searches of bag_of_position
// run side by side ONCE per call instead of one after the other inside every segment sum (the sums then read one word per
// term).  A workspace array of the call: written here, read by the kernels launched behind it.
__global__ __launch_bounds__(kBagNT) void position_bags_kernel(const int64_t* __restrict__ offsets, int64_t nnz, int64_t B,
                                                               int32_t* __restrict__ bagidx) {
  const int64_t first = offsets[0], last = offsets[B];
  for (int64_t n = (int64_t)blockIdx.x * kBagNT + threadIdx.x; n < nnz; n += (int64_t)gridDim.x * kBagNT)
    bagidx[n] = n >= first && n < last ? (int32_t)bag_of_position(offsets, B, n) : -1;
}

// terms w[perm[k]] dOut[bag(perm[k])][c] of the sorted list
template <bool WEIGHTED>
struct GradTerms {
  const float4* __restrict__ d_out;
  const float* __restrict__ w;
  const int32_t* __restrict__ perm;
  const int32_t* __restrict__ bagidx;
  int64_t nnz;   // the live id count
  // term k, column c: the gradient row of its position's bag (zeros outside every bag) and, WEIGHTED, its weight
  __device__ __forceinline__ float4 term(int64_t D4, int64_t c, int64_t k, float& wk) const {
    const int64_t p = clamp_to(perm[k], nnz - 1);
    if constexpr (WEIGHTED) wk = w[p];
    const int64_t b = bagidx[p];   // (< B: position_bags_kernel wrote it in this call)
    if (b >= 0) return d_out[b * D4 + c];
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  __device__ __forceinline__ float4 sum(int64_t D4, int64_t c, int64_t a, int64_t e) const {
    float wk = 1.0f;
    float4 acc = term(D4, c, a, wk);
    if constexpr (WEIGHTED) acc = f4_scale(wk, acc);
#pragma unroll 4
    for (int64_t k = a + 1; k < e; ++k) {
      const float4 gv = term(D4, c, k, wk);
      if constexpr (WEIGHTED) acc = f4_fma(wk, gv, acc); else acc = f4_add(gv, acc);
    }
    return acc;
  }
};

// d_rows[j], j < U: the chunk partials of the long segments (chunks at or past seg[U] = the end of the list do not exist),
// then every segment.  One lane group per distinct id; the launches are sized by nnz, the loops stop at seg[U] and U.
template <bool WEIGHTED>
__global__ __launch_bounds__(kBagNT) void seg_partial_mapped_kernel(const float4* __restrict__ d_out, const float* __restrict__ w,
                                                                    const int32_t* __restrict__ perm,
                                                                    const int64_t* __restrict__ seg,
                                                                    const int32_t* __restrict__ count_dev,
                                                                    const int32_t* __restrict__ bagidx, int64_t nnz,
                                                                    const int32_t* __restrict__ nnz_dev, int64_t cap,
                                                                    int64_t D4, int shift, float4* __restrict__ partial) {
  nnz = live_count(nnz, nnz_dev);
  const int64_t U = live_count(nnz < cap ? nnz : cap, count_dev);   // the distinct ids of the live part
  if (U <= 0) return;
  chunk_partials(SortedSegs{seg, U, clamp_to(seg[U], nnz)}, GradTerms<WEIGHTED>{d_out, w, perm, bagidx, nnz}, D4, shift, partial);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kBagNT) void seg_reduce_mapped_kernel(const float4* __restrict__ d_out, const float* __restrict__ w,
                                                                   const int32_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ seg,
                                                                   const int32_t* __restrict__ count_dev,
                                                                   const int32_t* __restrict__ bagidx, int64_t nnz,
                                                                   const int32_t* __restrict__ nnz_dev, int64_t cap,
                                                                   int64_t D4, int shift, const float4* __restrict__ partial,
                                                                   float4* __restrict__ d_rows) {
  nnz = live_count(nnz, nnz_dev);
  const int64_t U = live_count(nnz < cap ? nnz : cap, count_dev);
  if (U <= 0) return;
  segment_sums(SortedSegs{seg, U, clamp_to(seg[U], nnz)}, GradTerms<WEIGHTED>{d_out, w, perm, bagidx, nnz}, D4, shift, partial, d_rows);
}

// d_w[n] = <dOut[bag(n)], rows[map[n]]>, 0 outside every bag: the dot product and lane butterfly of
// bag_reduce_backward_kernel, one lane group per position
__global__ __launch_bounds__(kBagNT) void mapped_weight_grad_kernel(const float4* __restrict__ d_out, const float4* __restrict__ rows,
                                                                    int64_t cap, const int32_t* __restrict__ map,
                                                                    const int32_t* __restrict__ bagidx, int64_t nnz,
                                                                    const int32_t* __restrict__ nnz_dev, int64_t D4, int shift,
                                                                    float* __restrict__ d_w) {
  nnz = live_count(nnz, nnz_dev);
  const int W = 1 << shift;
  const int g = threadIdx.x >> shift, lane = threadIdx.x & (W - 1);
  const int64_t per_block = kBagNT >> shift;
  const int64_t passes = (D4 + W - 1) >> shift;
  for (int64_t i = (int64_t)blockIdx.x * per_block + g; i < nnz; i += (int64_t)gridDim.x * per_block) {
    const int64_t b = bagidx[i];
    const bool in_bag = b >= 0;
    const int64_t m = clamp_row(map[i], cap);
    float dot = 0.0f;
    for (int64_t k = 0; k < passes; ++k) {   // the same trip count on every lane of the group (the butterfly needs them all)
      const int64_t c = lane + (k << shift);
      if (c < D4 && in_bag) dot = dot4(d_out[b * D4 + c], rows[m * D4 + c], dot);
    }
    dot = group_sum(dot, W);
    if (lane == 0) d_w[i] = dot;
  }
}

unsigned grid_of(int64_t items, const Groups& gr) { return exact::ex_grid((items + gr.per_block - 1) / gr.per_block); }

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int check_sizes(const char* what, int64_t nnz, int64_t B, int64_t D) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "%s: negative nnz / B", what);
  if (D <= 0 || D % 4 != 0) return fail(TTEMB_E_BADARG, "%s: D = %lld is not a positive multiple of 4", what, (long long)D);
  return TTEMB_OK;
}

}  // namespace bag
}  // namespace ttemb

using namespace ttemb;
using namespace ttemb::bag;

extern "C" {

int64_t ttemb_bag_workspace_bytes(int64_t nnz, int64_t B, int64_t D) {
  int rc = check_sizes("ttemb_bag_workspace_bytes", nnz, B, D);
  if (rc) return rc;
  return kBagHeader + 2 * chunks_of(nnz) * D * (int64_t)sizeof(float);
}

// ttemb_bag_reduce_n (`what`, mapped = false: one row per position, weights required) and ttemb_bag_reduce_mapped_n (mapped:
// rows[map[n]] of `cap` rows, weights may be null, nnz has to fit the int32 map): the same two launches over the same chunks
static int reduce_call(const char* what, bool mapped, const float* rows, int64_t cap, const int32_t* map, const float* weights,
                       const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B, int64_t D, float* output,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(what, nnz, B, D);
  if (rc) return rc;
  if (mapped && nnz > kBagMaxIds) return fail(TTEMB_E_BADARG, "%s: nnz = %lld does not fit the int32 map", what, (long long)nnz);
  if (B == 0) return TTEMB_OK;
  if (offsets == nullptr || output == nullptr) return fail(TTEMB_E_BADARG, "%s: offsets / output is null", what);
  if (nnz > 0 && mapped && (rows == nullptr || map == nullptr || cap < 1))
    return fail(TTEMB_E_BADARG, "%s: rows / map is null or cap < 1", what);
  if (nnz > 0 && !mapped && (rows == nullptr || weights == nullptr)) return fail(TTEMB_E_BADARG, "%s: rows / weights is null", what);
  if (misaligned(rows) || misaligned(output)) return fail(TTEMB_E_BADARG, "%s: rows / output not 16-byte aligned", what);
  const int64_t need = ttemb_bag_workspace_bytes(nnz, B, D);
  if (workspace_bytes < need || workspace == nullptr)
    return fail(TTEMB_E_WORKSPACE, "%s: workspace of %lld bytes, need %lld", what, (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t D4 = D / 4, nch = chunks_of(nnz);
  const Groups gr = groups_of(D4);
  float4* partial = reinterpret_cast<float4*>(reinterpret_cast<char*>(workspace) + kBagHeader);
  const float4* r4 = reinterpret_cast<const float4*>(rows);
  float4* o4 = reinterpret_cast<float4*>(output);
  const dim3 gp(grid_of(nch, gr)), gb(grid_of(B, gr)), nt(kBagNT);
  if (!mapped) {
    if (nch > 0) {
      hipLaunchKernelGGL(bag_partial_kernel, gp, nt, 0, st, r4, weights, offsets, nnz, nnz_dev, B, D4, gr.shift, partial);
      if ((rc = check_hip(hipGetLastError(), "bag_partial_kernel"))) return rc;
    }
    hipLaunchKernelGGL(bag_reduce_kernel, gb, nt, 0, st, r4, weights, offsets, nnz, nnz_dev, B, D4, gr.shift, partial, o4);
    return check_hip(hipGetLastError(), "bag_reduce_kernel");
  }
  const bool weighted = weights != nullptr;
  if (nch > 0) {
    hipLaunchKernelGGL((weighted ? bag_partial_mapped_kernel<true> : bag_partial_mapped_kernel<false>), gp, nt, 0, st, r4, cap, map,
                       weights, offsets, nnz, nnz_dev, B, D4, gr.shift, partial);
    if ((rc = check_hip(hipGetLastError(), "bag_partial_mapped_kernel"))) return rc;
  }
  hipLaunchKernelGGL((weighted ? bag_reduce_mapped_kernel<true> : bag_reduce_mapped_kernel<false>), gb, nt, 0, st, r4, cap, map,
                     weights, offsets, nnz, nnz_dev, B, D4, gr.shift, partial, o4);
  return check_hip(hipGetLastError(), "bag_reduce_mapped_kernel");
}

int ttemb_bag_reduce_n(const float* rows, const float* weights, const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev,
                       int64_t B, int64_t D, float* output, void* workspace, int64_t workspace_bytes, void* stream) {
  return reduce_call("ttemb_bag_reduce", false, rows, 0, nullptr, weights, offsets, nnz, nnz_dev, B, D, output, workspace,
                     workspace_bytes, stream);
}

int ttemb_bag_reduce(const float* rows, const float* weights, const int64_t* offsets, int64_t nnz, int64_t B, int64_t D,
                     float* output, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttemb_bag_reduce_n(rows, weights, offsets, nnz, nullptr, B, D, output, workspace, workspace_bytes, stream);
}

int ttemb_bag_reduce_backward_n(const float* d_output, const float* weights, const float* rows, const int64_t* offsets,
                                int64_t nnz, const int32_t* nnz_dev, int64_t B, int64_t D, float* d_rows, float* d_weights,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  int rc = check_sizes("ttemb_bag_reduce_backward", nnz, B, D);
  if (rc) return rc;
  if (nnz == 0) return TTEMB_OK;
  if (offsets == nullptr || weights == nullptr || d_rows == nullptr || (B > 0 && d_output == nullptr))
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_backward: offsets / weights / d_rows / d_output is null");
  if (d_weights != nullptr && rows == nullptr)
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_backward: the weight gradient needs the rows");
  if (misaligned(d_output) || misaligned(rows) || misaligned(d_rows))
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_backward: d_output / rows / d_rows not 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t D4 = D / 4;
  const Groups gr = groups_of(D4);
  hipLaunchKernelGGL(bag_reduce_backward_kernel, dim3(grid_of(nnz, gr)), dim3(kBagNT), 0, st,
                     reinterpret_cast<const float4*>(d_output), weights, reinterpret_cast<const float4*>(rows), offsets, nnz,
                     nnz_dev, B, D4, gr.shift, reinterpret_cast<float4*>(d_rows), d_weights);
  return check_hip(hipGetLastError(), "bag_reduce_backward_kernel");
}

int ttemb_bag_reduce_backward(const float* d_output, const float* weights, const float* rows, const int64_t* offsets,
                              int64_t nnz, int64_t B, int64_t D, float* d_rows, float* d_weights, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return ttemb_bag_reduce_backward_n(d_output, weights, rows, offsets, nnz, nullptr, B, D, d_rows, d_weights, workspace,
                                     workspace_bytes, stream);
}

int ttemb_bag_mean(const float* src, float* dst, const int64_t* offsets, int64_t B, int64_t D, void* stream) {
  int rc = check_sizes("ttemb_bag_mean", 0, B, D);
  if (rc) return rc;
  if (B == 0) return TTEMB_OK;
  if (src == nullptr || dst == nullptr || offsets == nullptr) return fail(TTEMB_E_BADARG, "ttemb_bag_mean: null pointer");
  if (misaligned(src) || misaligned(dst)) return fail(TTEMB_E_BADARG, "ttemb_bag_mean: src / dst not 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Groups gr = groups_of(D / 4);
  hipLaunchKernelGGL(bag_mean_kernel, dim3(grid_of(B, gr)), dim3(kBagNT), 0, st, reinterpret_cast<const float4*>(src),
                     reinterpret_cast<float4*>(dst), offsets, B, D / 4, gr.shift);
  return check_hip(hipGetLastError(), "bag_mean_kernel");
}

int64_t ttemb_bag_max_workspace_bytes(int64_t nnz, int64_t B, int64_t D) {
  int rc = check_sizes("ttemb_bag_max_workspace_bytes", nnz, B, D);
  if (rc) return rc;
  // per chunk two slots of D values and D positions
  return kBagHeader + 2 * chunks_of(nnz) * D * (int64_t)(sizeof(float) + sizeof(int32_t));
}

int ttemb_bag_max_n(const float* rows, const int64_t* indices, int64_t pad, const int64_t* offsets, int64_t nnz,
                    const int32_t* nnz_dev, int64_t B, int64_t D, float* output, int32_t* argmax, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  int rc = check_sizes("ttemb_bag_max", nnz, B, D);
  if (rc) return rc;
  if (nnz > kBagMaxIds) return fail(TTEMB_E_BADARG, "ttemb_bag_max: nnz = %lld does not fit the int32 positions", (long long)nnz);
  if (B == 0) return TTEMB_OK;
  if (offsets == nullptr || output == nullptr || argmax == nullptr)
    return fail(TTEMB_E_BADARG, "ttemb_bag_max: offsets / output / argmax is null");
  if (nnz > 0 && rows == nullptr) return fail(TTEMB_E_BADARG, "ttemb_bag_max: rows is null");
  if (misaligned(rows) || misaligned(output) || misaligned(argmax))
    return fail(TTEMB_E_BADARG, "ttemb_bag_max: rows / output / argmax not 16-byte aligned");
  const int64_t need = ttemb_bag_max_workspace_bytes(nnz, B, D);
  if (workspace_bytes < need || workspace == nullptr)
    return fail(TTEMB_E_WORKSPACE, "ttemb_bag_max: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t D4 = D / 4, nch = chunks_of(nnz);
  const Groups gr = groups_of(D4);
  float4* pv = reinterpret_cast<float4*>(reinterpret_cast<char*>(workspace) + kBagHeader);
  int4* pp = reinterpret_cast<int4*>(pv + 2 * nch * D4);
  const float4* r4 = reinterpret_cast<const float4*>(rows);
  if (nch > 0) {
    hipLaunchKernelGGL(bag_max_partial_kernel, dim3(grid_of(nch, gr)), dim3(kBagNT), 0, st, r4, indices, pad, offsets, nnz,
                       nnz_dev, B, D4, gr.shift, pv, pp);
    if ((rc = check_hip(hipGetLastError(), "bag_max_partial_kernel"))) return rc;
  }
  hipLaunchKernelGGL(bag_max_kernel, dim3(grid_of(B, gr)), dim3(kBagNT), 0, st, r4, indices, pad, offsets, nnz, nnz_dev, B, D4,
                     gr.shift, pv, pp, reinterpret_cast<float4*>(output), reinterpret_cast<int4*>(argmax));
  return check_hip(hipGetLastError(), "bag_max_kernel");
}

int ttemb_bag_max(const float* rows, const int64_t* indices, int64_t pad, const int64_t* offsets, int64_t nnz, int64_t B,
                  int64_t D, float* output, int32_t* argmax, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttemb_bag_max_n(rows, indices, pad, offsets, nnz, nullptr, B, D, output, argmax, workspace, workspace_bytes, stream);
}

int ttemb_bag_max_backward_n(const float* d_output, const int32_t* argmax, const int64_t* offsets, int64_t nnz,
                             const int32_t* nnz_dev, int64_t B, int64_t D, float* d_rows, void* stream) {
  int rc = check_sizes("ttemb_bag_max_backward", nnz, B, D);
  if (rc) return rc;
  if (nnz > kBagMaxIds)
    return fail(TTEMB_E_BADARG, "ttemb_bag_max_backward: nnz = %lld does not fit the int32 positions", (long long)nnz);
  if (nnz == 0) return TTEMB_OK;
  if (offsets == nullptr || d_rows == nullptr || (B > 0 && (d_output == nullptr || argmax == nullptr)))
    return fail(TTEMB_E_BADARG, "ttemb_bag_max_backward: offsets / d_rows / d_output / argmax is null");
  if (misaligned(d_output) || misaligned(argmax) || misaligned(d_rows))
    return fail(TTEMB_E_BADARG, "ttemb_bag_max_backward: d_output / argmax / d_rows not 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t D4 = D / 4;
  const Groups gr = groups_of(D4);
  hipLaunchKernelGGL(bag_max_backward_kernel, dim3(grid_of(nnz, gr)), dim3(kBagNT), 0, st,
                     reinterpret_cast<const float4*>(d_output), reinterpret_cast<const int4*>(argmax), offsets, nnz, nnz_dev, B,
                     D4, gr.shift, reinterpret_cast<float4*>(d_rows));
  return check_hip(hipGetLastError(), "bag_max_backward_kernel");
}

int ttemb_bag_max_backward(const float* d_output, const int32_t* argmax, const int64_t* offsets, int64_t nnz, int64_t B,
                           int64_t D, float* d_rows, void* stream) {
  return ttemb_bag_max_backward_n(d_output, argmax, offsets, nnz, nullptr, B, D, d_rows, stream);
}

int ttemb_pad_weights_n(const int64_t* indices, const int64_t* offsets, const float* weights, int64_t nnz,
                        const int32_t* nnz_dev, int64_t B, int64_t pad, int32_t mean, float* weights_out, void* stream) {
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "ttemb_pad_weights: negative nnz / B");
  if (nnz == 0) return TTEMB_OK;
  if (indices == nullptr || offsets == nullptr || weights_out == nullptr)
    return fail(TTEMB_E_BADARG, "ttemb_pad_weights: indices / offsets / weights_out is null");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t per_block = kBagNT / kWave;
  hipLaunchKernelGGL(pad_weights_kernel, dim3(exact::ex_grid((B + per_block - 1) / per_block)), dim3(kBagNT), 0, st, indices,
                     offsets, weights, nnz, nnz_dev, B, pad, mean != 0 ? 1 : 0, weights_out);
  return check_hip(hipGetLastError(), "pad_weights_kernel");
}

int ttemb_pad_weights(const int64_t* indices, const int64_t* offsets, const float* weights, int64_t nnz, int64_t B,
                      int64_t pad, int32_t mean, float* weights_out, void* stream) {
  return ttemb_pad_weights_n(indices, offsets, weights, nnz, nullptr, B, pad, mean, weights_out, stream);
}

int ttemb_bag_reduce_mapped_n(const float* rows, int64_t cap, const int32_t* map, const float* weights, const int64_t* offsets,
                              int64_t nnz, const int32_t* nnz_dev, int64_t B, int64_t D, float* output, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return reduce_call("ttemb_bag_reduce_mapped", true, rows, cap, map, weights, offsets, nnz, nnz_dev, B, D, output, workspace,
                     workspace_bytes, stream);
}

int ttemb_bag_reduce_mapped(const float* rows, int64_t cap, const int32_t* map, const float* weights, const int64_t* offsets,
                            int64_t nnz, int64_t B, int64_t D, float* output, void* workspace, int64_t workspace_bytes,
                            void* stream) {
  return ttemb_bag_reduce_mapped_n(rows, cap, map, weights, offsets, nnz, nullptr, B, D, output, workspace, workspace_bytes, stream);
}

int ttemb_bag_reduce_mapped_backward_n(const float* d_output, const float* weights, const float* rows, int64_t cap,
                                       const int32_t* map, const int32_t* perm, const int64_t* seg, const int32_t* count_dev,
                                       const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B, int64_t D,
                                       float* d_rows, float* d_weights, void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_sizes("ttemb_bag_reduce_mapped_backward", nnz, B, D);
  if (rc) return rc;
  if (nnz > kBagMaxIds)
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: nnz = %lld does not fit the int32 map", (long long)nnz);
  if (nnz == 0) return TTEMB_OK;
  if (offsets == nullptr || d_rows == nullptr || (B > 0 && d_output == nullptr))
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: offsets / d_rows / d_output is null");
  if (map == nullptr || perm == nullptr || seg == nullptr || count_dev == nullptr || cap < 1)
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: map / perm / seg / count_dev is null or cap < 1");
  if (d_weights != nullptr && rows == nullptr)
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: the weight gradient needs the rows");
  if (misaligned(d_output) || misaligned(rows) || misaligned(d_rows))
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: d_output / rows / d_rows not 16-byte aligned");
  if (B > kBagMaxIds)
    return fail(TTEMB_E_BADARG, "ttemb_bag_reduce_mapped_backward: B = %lld does not fit the int32 bag index", (long long)B);
  // behind the chunk partials of ttemb_bag_workspace_bytes: one int32 per position, its bag
  const int64_t partial_bytes = ttemb_bag_workspace_bytes(nnz, B, D);
  const int64_t need = partial_bytes + ((nnz * 4 + 255) & ~int64_t(255));
  if (workspace_bytes < need || workspace == nullptr)
    return fail(TTEMB_E_WORKSPACE, "ttemb_bag_reduce_mapped_backward: workspace of %lld bytes, need %lld",
                (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t D4 = D / 4, nch = chunks_of(nnz);
  const Groups gr = groups_of(D4);
  float4* partial = reinterpret_cast<float4*>(reinterpret_cast<char*>(workspace) + kBagHeader);
  const float4* g4 = reinterpret_cast<const float4*>(d_output);
  float4* dr4 = reinterpret_cast<float4*>(d_rows);
  int32_t* bagidx = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + partial_bytes);
  hipLaunchKernelGGL(position_bags_kernel, dim3(exact::ex_grid((nnz + kBagNT - 1) / kBagNT)), dim3(kBagNT), 0, st, offsets, nnz, B,
                     bagidx);
  if ((rc = check_hip(hipGetLastError(), "position_bags_kernel"))) return rc;
  const bool weighted = weights != nullptr;
  hipLaunchKernelGGL((weighted ? seg_partial_mapped_kernel<true> : seg_partial_mapped_kernel<false>), dim3(grid_of(nch, gr)),
                     dim3(kBagNT), 0, st, g4, weights, perm, seg, count_dev, bagidx, nnz, nnz_dev, cap, D4, gr.shift, partial);
  if ((rc = check_hip(hipGetLastError(), "seg_partial_mapped_kernel"))) return rc;
  hipLaunchKernelGGL((weighted ? seg_reduce_mapped_kernel<true> : seg_reduce_mapped_kernel<false>), dim3(grid_of(nnz, gr)),
                     dim3(kBagNT), 0, st, g4, weights, perm, seg, count_dev, bagidx, nnz, nnz_dev, cap, D4, gr.shift, partial, dr4);
  if ((rc = check_hip(hipGetLastError(), "seg_reduce_mapped_kernel"))) return rc;
  if (d_weights != nullptr) {
    hipLaunchKernelGGL(mapped_weight_grad_kernel, dim3(grid_of(nnz, gr)), dim3(kBagNT), 0, st, g4,
                       reinterpret_cast<const float4*>(rows), cap, map, bagidx, nnz, nnz_dev, D4, gr.shift, d_weights);
    rc = check_hip(hipGetLastError(), "mapped_weight_grad_kernel");
  }
  return rc;
}

int ttemb_bag_reduce_mapped_backward(const float* d_output, const float* weights, const float* rows, int64_t cap,
                                     const int32_t* map, const int32_t* perm, const int64_t* seg, const int32_t* count_dev,
                                     const int64_t* offsets, int64_t nnz, int64_t B, int64_t D, float* d_rows, float* d_weights,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  return ttemb_bag_reduce_mapped_backward_n(d_output, weights, rows, cap, map, perm, seg, count_dev, offsets, nnz, nullptr, B, D,
                                            d_rows, d_weights, workspace, workspace_bytes, stream);
}

}  // extern "C"
