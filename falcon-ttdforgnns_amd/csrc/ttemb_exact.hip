// Exact lookup: a forward and a backward whose results are a function of (shape, cores, indices, offsets, B, d_output,
// lr, eps) only, bit for bit (the contract is in include/ttemb.h, "Exact mode").  A kernel family of its own: nothing here
// is shared with the default kernels, whose device code is untouched by this file.
//
//   forward   one workgroup (one wave) per bag, ids in position order: the row of an id is P.G2[i2] with
//             P = G0[i0].G1[i1] formed in LDS, summed into the lane's registers in bag order, stored once.
//   backward  the ids' positions are sorted three times -- by i0, by i1, by i2 -- with a stable LSD radix sort
//             (per-tile digit histograms scanned tile-major, in-tile ranks in lane order), which gives every core row the
//             list of its ids in position order.  The sorted list is cut into fixed chunks (boundaries from the list
//             alone); a chunk sums each of its rows' contributions in list order, writes a row whose list lies wholly
//             inside it directly, and leaves a partial for a row whose list crosses a chunk edge; the fix-up kernel adds
//             those partials in chunk order.  The gradients of all three cores are complete before any core is updated
//             (each core's gradient reads the other two).
//
// No float atomics, no waits between workgroups, every loop over work items is grid-stride (the grid only decides who
// computes a value, never how), and every buffer that is read was written earlier in the same call.
#include "ttemb_common.h"

#include <atomic>
#include <cstdio>
#include <cstring>

namespace ttemb {
namespace exact {

constexpr int kExNT = 64;                   // threads of the lookup / reduction kernels: one wave per workgroup
constexpr int kExAcc = 16;                  // row entries per lane per slice
constexpr int kExSlice = kExNT * kExAcc;    // 1024 floats of a row per pass over a chunk
constexpr int kExChunk = 256;               // ids per chunk of a sorted list (times the number of slices of the row)
constexpr int kSortNT = 256;                // threads = elements per tile of the radix sort (4 waves)
constexpr int kScanSpan = 2048;             // ints per block of the scan (256 threads x 8)
constexpr int kPBuf = 64 * 32;              // q0 q1 <= 64, r2 <= 32: P or dP of one id
constexpr int kYBuf = 64 * 16;              // D = q0 q1 q2 <= 1024
constexpr int64_t kDefaultGrid = 1 << 20;

std::atomic<int> g_exact_grid{0};

// The 3-core view the exact kernels run on.  A 2-core table is lifted to (p0, 1, p1) with q = (q0, 1, q1), ranks
// (R1, R1) and the identity as the middle core (ident = 1: G1 is never read and has no gradient).  A 4-core table merges one
// adjacent pair (a, a + 1) into a virtual core V of pa pb rows, V[ia pb + ib] = Ga[ia] . Gb[ib] (contracted over their
// shared rank); the view's core `ma` is V, and the view's row index of an id is exactly ia pb + ib, so the ids decode as
// they are.  V's gradient is split back into dGa and dGb afterwards (exact_split_kernel).
struct ExShape {
  long long L0, L1, rows;   // decode strides p1 p2, p2; prod(p)
  int p[3];
  int q0, q1, q2, r1, r2;
  int D;
  int s[3];                 // floats per core row
  int ident;
  int ma;                   // 4-core tables: the merged pair's first core (the view's core ma is V); -1 otherwise
  int mpa, mpb, mRa, mqa, mRm, mqb, mRs;   // the pair: rows, and Ga row = [mRa][mqa][mRm], Gb row = [mRm][mqb][mRs]
};

__device__ __forceinline__ void decode(const ExShape& s, int64_t id, int& i0, int& i1, int& i2) {
  if (id < 0 || id >= s.rows) id = 0;   // an id outside the table reads row 0 instead of memory past the cores
  i0 = (int)(id / s.L0);
  const int64_t rem = id - (int64_t)i0 * s.L0;
  i1 = (int)(rem / s.L1);
  i2 = (int)(rem - (int64_t)i1 * s.L1);
}

// P[(x q1 + y) r2 + b] = sum_a G0[x][a] G1[a][y][b], a in order
__device__ __forceinline__ void form_p(const ExShape& s, const float* g0, const float* g1, float* P) {
  const int qr = s.q1 * s.r2, n = s.q0 * qr;
  for (int e = threadIdx.x; e < n; e += kExNT) {
    const int x = e / qr, rem = e - x * qr;
    float v;
    if (s.ident) {
      v = g0[x * s.r1 + rem];
    } else {
      v = 0.0f;
      for (int a = 0; a < s.r1; ++a) v = fmaf(g0[x * s.r1 + a], g1[a * qr + rem], v);
    }
    P[e] = v;
  }
}

// dP[(x q1 + y) r2 + b] = sum_z dY[(x q1 + y) q2 + z] G2[b][z], z in order (zeros for a position outside every bag)
__device__ __forceinline__ void form_dp(const ExShape& s, const float* dy, const float* g2, float* dP) {
  const int n = s.q0 * s.q1 * s.r2;
  for (int e = threadIdx.x; e < n; e += kExNT) {
    const int xy = e / s.r2, b = e - xy * s.r2;
    float v = 0.0f;
    if (dy != nullptr)
      for (int z = 0; z < s.q2; ++z) v = fmaf(dy[xy * s.q2 + z], g2[b * s.q2 + z], v);
    dP[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kExNT) void exact_forward_kernel(ExShape s, const float* __restrict__ G0,
                                                              const float* __restrict__ G1, const float* __restrict__ G2,
                                                              const int64_t* __restrict__ indices,
                                                              const int64_t* __restrict__ offsets, int64_t nnz, int64_t B,
                                                              float* __restrict__ out) {
  __shared__ float P[kPBuf];
  const int lane = threadIdx.x;
  const int nk = (s.D + kExNT - 1) / kExNT;
  for (int64_t bag = blockIdx.x; bag < B; bag += gridDim.x) {
    float acc[kExAcc];
#pragma unroll
    for (int k = 0; k < kExAcc; ++k) acc[k] = 0.0f;
    const int64_t n0 = offsets[bag] < 0 ? 0 : offsets[bag];
    const int64_t n1 = offsets[bag + 1] > nnz ? nnz : offsets[bag + 1];
    for (int64_t n = n0; n < n1; ++n) {
      int i0, i1, i2;
      decode(s, indices[n], i0, i1, i2);
      form_p(s, G0 + (int64_t)i0 * s.s[0], s.ident ? nullptr : G1 + (int64_t)i1 * s.s[1], P);
      __syncthreads();
      const float* g2 = G2 + (int64_t)i2 * s.s[2];   // [r2][q2]
#pragma unroll
      for (int k = 0; k < kExAcc; ++k) {
        const int d = lane + k * kExNT;
        if (k < nk && d < s.D) {
          const int xy = d / s.q2, z = d - xy * s.q2;
          float v = 0.0f;
          for (int b = 0; b < s.r2; ++b) v = fmaf(P[xy * s.r2 + b], g2[b * s.q2 + z], v);
          acc[k] += v;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kExAcc; ++k) {
      const int d = lane + k * kExNT;
      if (k < nk && d < s.D) out[bag * s.D + d] = acc[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// canonical order: decode, then a stable LSD radix sort of the positions by one core's row
// ---------------------------------------------------------------------------------------------------------------------
// keys[c][n] = i_c of position n; bagof[n] = the bag holding position n (-1: none)
__global__ __launch_bounds__(kSortNT) void exact_decode_kernel(ExShape s, const int64_t* __restrict__ indices,
                                                               const int64_t* __restrict__ offsets, int64_t B, int64_t n,
                                                               int32_t* __restrict__ k0, int32_t* __restrict__ k1,
                                                               int32_t* __restrict__ k2, int32_t* __restrict__ bagof) {
  for (int64_t i = (int64_t)blockIdx.x * kSortNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSortNT) {
    int i0, i1, i2;
    decode(s, indices[i], i0, i1, i2);
    k0[i] = i0;
    k1[i] = i1;
    k2[i] = i2;
    int64_t lo = 0, hi = B + 1;   // first b in [0, B] with offsets[b] > i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (offsets[mid] > i) hi = mid; else lo = mid + 1;
    }
    bagof[i] = (lo >= 1 && lo <= B) ? (int32_t)(lo - 1) : -1;
  }
}

// H[d * ntiles + t] = number of keys of tile t whose digit is d (integer counts: their order sets nothing)
__global__ __launch_bounds__(kSortNT) void exact_radix_hist_kernel(const int32_t* __restrict__ keys, int64_t n, int shift,
                                                                   int64_t ntiles, int32_t* __restrict__ H) {
  __shared__ int h[256];
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = t * kSortNT + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
    __syncthreads();
    H[threadIdx.x * ntiles + t] = h[threadIdx.x];
    __syncthreads();
  }
}

__device__ __forceinline__ int block_inclusive_scan(int v, int* tmp) {   // 256 threads
  tmp[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < kSortNT; o <<= 1) {
    const int add = threadIdx.x >= o ? tmp[threadIdx.x - o] : 0;
    __syncthreads();
    v += add;
    tmp[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

// exclusive scan of int32 a[0, m) in place: block sums, a one-block scan of them, then each block's own span
__global__ __launch_bounds__(kSortNT) void exact_scan_reduce_kernel(const int32_t* __restrict__ a, int64_t m,
                                                                    int64_t nblk, int32_t* __restrict__ sums) {
  __shared__ int tmp[kSortNT];
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int v = 0;
    const int64_t base = blk * kScanSpan + threadIdx.x * 8;
    for (int j = 0; j < 8; ++j)
      if (base + j < m) v += a[base + j];
    v = block_inclusive_scan(v, tmp);
    if (threadIdx.x == kSortNT - 1) sums[blk] = v;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSortNT) void exact_scan_top_kernel(int32_t* __restrict__ sums, int64_t nblk) {
  __shared__ int tmp[kSortNT];
  int carry = 0;
  for (int64_t base = 0; base < nblk; base += kSortNT) {
    const int64_t i = base + threadIdx.x;
    const int v = i < nblk ? sums[i] : 0;
    const int inc = block_inclusive_scan(v, tmp);
    if (i < nblk) sums[i] = carry + inc - v;
    carry += tmp[kSortNT - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSortNT) void exact_scan_down_kernel(int32_t* __restrict__ a, int64_t m, int64_t nblk,
                                                                  const int32_t* __restrict__ sums) {
  __shared__ int tmp[kSortNT];
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int v[8];
    int tot = 0;
    const int64_t base = blk * kScanSpan + threadIdx.x * 8;
    for (int j = 0; j < 8; ++j) {
      v[j] = base + j < m ? a[base + j] : 0;
      tot += v[j];
    }
    int run = sums[blk] + block_inclusive_scan(tot, tmp) - tot;
    for (int j = 0; j < 8; ++j) {
      if (base + j < m) a[base + j] = run;
      run += v[j];
    }
    __syncthreads();
  }
}

// stable scatter of one digit: destination = the scanned (digit, tile) offset + the keys of that digit in earlier waves of
// the tile + the lanes before this one in its wave with the same digit (8 ballots give the lanes of equal digit)
__global__ __launch_bounds__(kSortNT) void exact_radix_scatter_kernel(const int32_t* __restrict__ kin,
                                                                      const int32_t* __restrict__ vin, int64_t n, int shift,
                                                                      int64_t ntiles, const int32_t* __restrict__ H,
                                                                      int32_t* __restrict__ kout, int32_t* __restrict__ vout) {
  __shared__ int cnt[kSortNT / kWave][256];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    for (int i = threadIdx.x; i < (kSortNT / kWave) * 256; i += kSortNT) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const int64_t i = t * kSortNT + threadIdx.x;
    const bool valid = i < n;
    const int key = valid ? kin[i] : 0;
    const int val = valid ? (vin != nullptr ? vin[i] : (int)i) : 0;
    const int d = (key >> shift) & 255;
    unsigned long long m = __ballot(valid);
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long bb = __ballot((d >> bit) & 1);
      m &= ((d >> bit) & 1) ? bb : ~bb;
    }
    const int rank = __popcll(m & lt);
    if (valid && rank == 0) cnt[w][d] = __popcll(m);
    __syncthreads();
    if (valid) {
      int pre = 0;
      for (int v = 0; v < w; ++v) pre += cnt[v][d];
      const int64_t dst = (int64_t)H[d * ntiles + t] + pre + rank;
      kout[dst] = key;
      vout[dst] = val;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward: chunk sums over one core's sorted list, then the fix-up of rows whose list crosses a chunk edge
// ---------------------------------------------------------------------------------------------------------------------
// Contribution of one id to its row of core C:
//   C = 0: dG0[x][a]    = sum_{y, b} dP[x y][b] G1[a][y][b]
//   C = 1: dG1[a][y][b] = sum_x G0[x][a] dP[x y][b]
//   C = 2: dG2[b][z]    = sum_{x y} P[x y][b] dY[x y][z]
// with dP = dY.G2^T and P = G0.G1 of that id; every sum in a fixed order.
template <int C>
__global__ __launch_bounds__(kExNT) void exact_chunk_kernel(ExShape s, const float* __restrict__ G0,
                                                            const float* __restrict__ G1, const float* __restrict__ G2,
                                                            const int64_t* __restrict__ indices,
                                                            const int32_t* __restrict__ bagof,
                                                            const float* __restrict__ dY, const int32_t* __restrict__ skey,
                                                            const int32_t* __restrict__ spos, int64_t n, int64_t chunk,
                                                            int64_t nchunks, float* __restrict__ grad,
                                                            float* __restrict__ partial, uint8_t* __restrict__ touched) {
  __shared__ float buf[kPBuf];
  __shared__ float ybuf[C == 2 ? kYBuf : 1];
  const int S = s.s[C];
  const int lane = threadIdx.x;
  for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const int64_t c0 = k * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    for (int e0 = 0; e0 < S; e0 += kExSlice) {
      float acc[kExAcc];
#pragma unroll
      for (int j = 0; j < kExAcc; ++j) acc[j] = 0.0f;
      int64_t s0 = c0;
      for (int64_t j = c0; j < c1; ++j) {
        const int key = skey[j];
        const int pos = spos[j];
        int i0, i1, i2;
        decode(s, indices[pos], i0, i1, i2);
        const int bag = bagof[pos];
        const float* dy = bag >= 0 ? dY + (int64_t)bag * s.D : nullptr;
        const float* g0 = G0 + (int64_t)i0 * s.s[0];
        const float* g1 = s.ident ? nullptr : G1 + (int64_t)i1 * s.s[1];
        const float* g2 = G2 + (int64_t)i2 * s.s[2];
        if constexpr (C == 2) {
          form_p(s, g0, g1, buf);
          for (int e = lane; e < s.D; e += kExNT) ybuf[e] = dy != nullptr ? dy[e] : 0.0f;
        } else {
          form_dp(s, dy, g2, buf);
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < kExAcc; ++jj) {
          const int e = e0 + lane + jj * kExNT;
          if (e < S) {
            float v = 0.0f;
            if constexpr (C == 0) {
              const int x = e / s.r1, a = e - x * s.r1;
              const float* dp = buf + x * s.q1 * s.r2;
              if (s.ident) {
                v = dp[a];
              } else {
                for (int y = 0; y < s.q1; ++y)
                  for (int b = 0; b < s.r2; ++b) v = fmaf(dp[y * s.r2 + b], g1[(a * s.q1 + y) * s.r2 + b], v);
              }
            } else if constexpr (C == 1) {
              const int qr = s.q1 * s.r2, a = e / qr, yb = e - a * qr;
              for (int x = 0; x < s.q0; ++x) v = fmaf(g0[x * s.r1 + a], buf[x * qr + yb], v);
            } else {
              const int b = e / s.q2, z = e - b * s.q2;
              const int qq = s.q0 * s.q1;
              for (int xy = 0; xy < qq; ++xy) v = fmaf(buf[xy * s.r2 + b], ybuf[xy * s.q2 + z], v);
            }
            acc[jj] += v;
          }
        }
        __syncthreads();
        if (j + 1 == c1 || skey[j + 1] != key) {   // the piece [s0, j + 1) of row `key` ends here
          const bool starts = s0 == 0 || skey[s0 - 1] != key;
          const bool ends = j + 1 == n || skey[j + 1] != key;
          float* dst = (starts && ends) ? grad + (int64_t)key * S
                                        : partial + (2 * k + (s0 == c0 ? 0 : 1)) * (int64_t)S;
#pragma unroll
          for (int jj = 0; jj < kExAcc; ++jj) {
            const int e = e0 + lane + jj * kExNT;
            if (e < S) dst[e] = acc[jj];
            acc[jj] = 0.0f;
          }
          if (starts && ends && touched != nullptr && lane == 0 && e0 == 0) touched[key] = 1;
          s0 = j + 1;
        }
      }
    }
  }
}

// A row whose list starts in chunk k and runs past its end: its partials (the last piece of chunk k, then the first piece
// of every later chunk it reaches) are added in chunk order.  Exactly one chunk is the start of each such row.
__global__ __launch_bounds__(kExNT) void exact_fixup_kernel(const int32_t* __restrict__ skey, int64_t n, int64_t chunk,
                                                            int64_t nchunks, int S, const float* __restrict__ partial,
                                                            float* __restrict__ grad, uint8_t* __restrict__ touched) {
  for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const int64_t c0 = k * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    const int key = skey[c1 - 1];
    if (c1 >= n || skey[c1] != key) continue;           // the last row of the chunk ends inside it
    if (c0 > 0 && skey[c0 - 1] == key) continue;        // ... or began in an earlier chunk
    const int64_t first = 2 * k + (skey[c0] == key ? 0 : 1);
    for (int e = threadIdx.x; e < S; e += kExNT) {
      float v = partial[first * S + e];
      for (int64_t kk = k + 1;; ++kk) {
        v += partial[(2 * kk) * S + e];
        const int64_t end = (kk + 1) * chunk;
        if (!(end < n && skey[end] == key)) break;
      }
      grad[(int64_t)key * S + e] = v;
    }
    if (touched != nullptr && threadIdx.x == 0) touched[key] = 1;
  }
}

// the fused optimisers: touched rows only, every other row and its state stay as they are
__global__ __launch_bounds__(kExNT) void exact_sgd_kernel(float* __restrict__ W, const float* __restrict__ G,
                                                          const uint8_t* __restrict__ touched, int64_t rows, int S, float lr_arg,
                                                          const float* __restrict__ lr_dev) {
  const float lr = step_lr(lr_dev, lr_arg);
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    if (!touched[r]) continue;
    for (int e = threadIdx.x; e < S; e += kExNT) W[r * S + e] -= lr * G[r * S + e];
  }
}

__global__ __launch_bounds__(kExNT) void exact_adagrad_kernel(float* __restrict__ W, float* __restrict__ state,
                                                              const float* __restrict__ G, const uint8_t* __restrict__ touched,
                                                              int64_t rows, int S, float lr_arg, const float* __restrict__ lr_dev,
                                                              float eps) {
  const float lr = step_lr(lr_dev, lr_arg);
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    if (!touched[r]) continue;
    for (int e = threadIdx.x; e < S; e += kExNT) {
      const float g = G[r * S + e];
      const float st = state[r * S + e] + g * g;
      state[r * S + e] = st;
      W[r * S + e] -= lr * g / (sqrtf(st) + eps);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 4-core tables: the merged pair and the split of its gradient, every element a sum in a fixed order
// ---------------------------------------------------------------------------------------------------------------------
// V[ia pb + ib][r][xa qb + xb][t] = sum_m Ga[ia][r][xa][m] Gb[ib][m][xb][t]
__global__ __launch_bounds__(256) void exact_merge_kernel(ExShape s, const float* __restrict__ Ga, const float* __restrict__ Gb,
                                                          float* __restrict__ V) {
  const int qq = s.mqa * s.mqb, rowv = s.mRa * qq * s.mRs;
  const int64_t total = (int64_t)s.mpa * s.mpb * rowv;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / rowv;
    const int c = (int)(e - row * rowv);
    const int ia = (int)(row / s.mpb), ib = (int)(row - (int64_t)ia * s.mpb);
    const int r = c / (qq * s.mRs), x = (c / s.mRs) % qq, t = c % s.mRs;
    const int xa = x / s.mqb, xb = x - xa * s.mqb;
    const float* ga = Ga + (int64_t)ia * s.mRa * s.mqa * s.mRm + (r * s.mqa + xa) * s.mRm;
    const float* gb = Gb + (int64_t)ib * s.mRm * s.mqb * s.mRs + xb * s.mRs + t;
    float v = 0.0f;
    for (int m = 0; m < s.mRm; ++m) v = fmaf(ga[m], gb[m * s.mqb * s.mRs], v);
    V[e] = v;
  }
}

// dGa[ia][r][xa][m] = sum_ib sum_xb sum_t dV[ia pb + ib][r][xa qb + xb][t] Gb[ib][m][xb][t]            (elements of core a)
// dGb[ib][m][xb][t] = sum_ia sum_r sum_xa Ga[ia][r][xa][m] dV[ia pb + ib][r][xa qb + xb][t]            (then of core b)
// every loop in index order.  With `vt` (the fused optimisers): ta[ia] / tb[ib] = some V row of that ia / ib was touched.
__global__ __launch_bounds__(256) void exact_split_kernel(ExShape s, const float* __restrict__ dV, const float* __restrict__ Ga,
                                                          const float* __restrict__ Gb, float* __restrict__ dGa,
                                                          float* __restrict__ dGb, const uint8_t* __restrict__ vt,
                                                          uint8_t* __restrict__ ta, uint8_t* __restrict__ tb) {
  const int qq = s.mqa * s.mqb, rowv = s.mRa * qq * s.mRs;
  const int rowa = s.mRa * s.mqa * s.mRm, rowb = s.mRm * s.mqb * s.mRs;
  const int64_t na = (int64_t)s.mpa * rowa, total = na + (int64_t)s.mpb * rowb;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    float v = 0.0f;
    if (e < na) {
      const int ia = (int)(e / rowa), c = (int)(e - (int64_t)ia * rowa);
      const int r = c / (s.mqa * s.mRm), xa = (c / s.mRm) % s.mqa, m = c % s.mRm;
      bool any = false;
      for (int ib = 0; ib < s.mpb; ++ib) {
        const int64_t row = (int64_t)ia * s.mpb + ib;
        if (vt != nullptr && !vt[row]) continue;   // an untouched V row: its gradient holds zeros
        any = true;
        const float* dv = dV + row * rowv + (r * qq + xa * s.mqb) * s.mRs;
        const float* gb = Gb + (int64_t)ib * rowb + m * s.mqb * s.mRs;
        for (int xb = 0; xb < s.mqb; ++xb)
          for (int t = 0; t < s.mRs; ++t) v = fmaf(dv[xb * s.mRs + t], gb[xb * s.mRs + t], v);
      }
      dGa[e] = v;
      if (ta != nullptr && c == 0) ta[ia] = any ? 1 : 0;
    } else {
      const int64_t f = e - na;
      const int ib = (int)(f / rowb), c = (int)(f - (int64_t)ib * rowb);
      const int m = c / (s.mqb * s.mRs), xb = (c / s.mRs) % s.mqb, t = c % s.mRs;
      bool any = false;
      for (int ia = 0; ia < s.mpa; ++ia) {
        const int64_t row = (int64_t)ia * s.mpb + ib;
        if (vt != nullptr && !vt[row]) continue;
        any = true;
        const float* dv = dV + row * rowv + xb * s.mRs + t;
        const float* ga = Ga + (int64_t)ia * rowa + m;
        for (int r = 0; r < s.mRa; ++r)
          for (int xa = 0; xa < s.mqa; ++xa)
            v = fmaf(ga[(r * s.mqa + xa) * s.mRm], dv[(r * qq + xa * s.mqb) * s.mRs], v);
      }
      dGb[f] = v;
      if (tb != nullptr && c == 0) tb[ib] = any ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// whether the exact kernels cover the 3-core view (p3, q3, ranks); else false with the reason in `why`
bool view_fits(const int* p3, const int* q3, int r1, int r2, char* why, size_t n) {
  if (r1 > 32 || r2 > 32) {
    snprintf(why, n, "ranks (%d, %d) -- the exact kernels cover ranks <= 32", r1, r2);
    return false;
  }
  if (q3[0] > 16 || q3[2] > 16 || q3[0] * q3[1] > 64) {
    snprintf(why, n, "q = (%d, %d, %d) -- the exact kernels need q0, q2 <= 16 and q0 q1 <= 64", q3[0], q3[1], q3[2]);
    return false;
  }
  return true;
}

int exact_view(const ttemb_shape_t* shape, ExShape* out) {
  DevShape d;
  int rc = make_dev_shape(shape, &d);
  if (rc) return rc;
  ExShape s;
  memset(&s, 0, sizeof(s));
  s.ma = -1;
  char why[160] = "";
  long long p3[3];
  int q3[3], r1 = 0, r2 = 0;
  if (d.T == 3) {
    for (int c = 0; c < 3; ++c) p3[c] = d.p[c], q3[c] = d.q[c];
    r1 = d.R[1];
    r2 = d.R[2];
  } else if (d.T == 2) {
    p3[0] = d.p[0]; p3[1] = 1; p3[2] = d.p[1];
    q3[0] = d.q[0]; q3[1] = 1; q3[2] = d.q[1];
    r1 = r2 = d.R[1];
    s.ident = 1;
  } else {   // T == 4: merge the pair that fits the domain with the smallest virtual core
    long long best = -1;
    for (int a = 0; a < 3; ++a) {
      long long pp[3];
      int qv[3], rv[2], k = 0;
      for (int c = 0; c < 4; ++c) {
        if (c == a + 1) continue;
        pp[k] = c == a ? (long long)d.p[a] * d.p[a + 1] : d.p[c];
        qv[k] = c == a ? d.q[a] * d.q[a + 1] : d.q[c];
        ++k;
      }
      // the view's inner ranks: the 4-core ranks R1..R3 without the one the pair contracts over (R[a + 1])
      for (int c = 1, j = 0; c <= 3; ++c)
        if (c != a + 1) rv[j++] = d.R[c];
      int p32[3];
      bool ok = d.R[a + 1] <= 32;
      if (!ok) snprintf(why, sizeof(why), "rank %d inside a merged pair -- the exact kernels cover ranks <= 32", d.R[a + 1]);
      for (int c = 0; c < 3; ++c) {
        if (pp[c] >= (1ll << 31)) ok = false;
        p32[c] = (int)(pp[c] < (1ll << 31) ? pp[c] : 0);
      }
      if (ok && !view_fits(p32, qv, rv[0], rv[1], why, sizeof(why))) ok = false;
      if (!ok) continue;
      const long long size = pp[a] * (long long)d.R[a] * qv[a] * d.R[a + 2];
      if (best >= 0 && size >= best) continue;
      best = size;
      for (int c = 0; c < 3; ++c) p3[c] = pp[c], q3[c] = qv[c];
      r1 = rv[0];
      r2 = rv[1];
      s.ma = a;
      s.mpa = d.p[a]; s.mpb = d.p[a + 1];
      s.mRa = d.R[a]; s.mqa = d.q[a]; s.mRm = d.R[a + 1]; s.mqb = d.q[a + 1]; s.mRs = d.R[a + 2];
    }
    if (best < 0) return fail(TTEMB_E_UNSUPPORTED, "exact mode: 4-core table with no mergeable pair: %s", why);
  }
  int p32[3] = {(int)p3[0], (int)p3[1], (int)p3[2]};
  if (!view_fits(p32, q3, r1, r2, why, sizeof(why))) return fail(TTEMB_E_UNSUPPORTED, "exact mode: %s", why);
  for (int c = 0; c < 3; ++c) s.p[c] = p32[c];
  s.q0 = q3[0]; s.q1 = q3[1]; s.q2 = q3[2];
  s.r1 = r1; s.r2 = r2;
  s.L1 = s.p[2];
  s.L0 = (long long)s.p[1] * s.p[2];
  s.rows = s.L0 * s.p[0];
  s.D = s.q0 * s.q1 * s.q2;
  s.s[0] = s.q0 * s.r1;
  s.s[1] = s.r1 * s.q1 * s.r2;
  s.s[2] = s.r2 * s.q2;
  *out = s;
  return TTEMB_OK;
}

int64_t ex_align(int64_t b) { return (b + 255) & ~int64_t(255); }
int64_t ex_slices(int S) { return (S + kExSlice - 1) / kExSlice; }
int64_t ex_chunk(int S) { return kExChunk * ex_slices(S); }
int64_t ex_nchunks(int64_t n, int S) { return (n + ex_chunk(S) - 1) / ex_chunk(S); }

struct ExLayout {   // byte offsets into the workspace
  int64_t keys[3], bagof, kA, vA, kB, vB, hist, sums, touched, grads[3], partial;
  int64_t merged, mgrads[2], mtouched;   // 4-core tables: V, the pair's gradients and touched rows (fused optimisers)
  int64_t total;
};

ExLayout ex_layout(const ExShape& s, int64_t n) {
  ExLayout L;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { const int64_t at = o; o += ex_align(bytes); return at; };
  for (int c = 0; c < 3; ++c) L.keys[c] = take(4 * n);
  L.bagof = take(4 * n);
  L.kA = take(4 * n);
  L.vA = take(4 * n);
  L.kB = take(4 * n);
  L.vB = take(4 * n);
  const int64_t ntiles = (n + kSortNT - 1) / kSortNT;
  L.hist = take(4 * 256 * ntiles);
  L.sums = take(4 * ((256 * ntiles + kScanSpan - 1) / kScanSpan));
  L.touched = take((int64_t)s.p[0] + s.p[1] + s.p[2]);
  for (int c = 0; c < 3; ++c) L.grads[c] = take(4 * (int64_t)s.p[c] * s.s[c]);
  int64_t part = 0;
  for (int c = 0; c < 3; ++c) {
    const int64_t b = 4 * 2 * ex_nchunks(n, s.s[c]) * (int64_t)s.s[c];
    part = b > part ? b : part;
  }
  L.partial = take(part);
  L.merged = L.mgrads[0] = L.mgrads[1] = L.mtouched = 0;
  if (s.ma >= 0) {
    L.merged = take(4 * (int64_t)s.p[s.ma] * s.s[s.ma]);
    L.mgrads[0] = take(4 * (int64_t)s.mpa * s.mRa * s.mqa * s.mRm);
    L.mgrads[1] = take(4 * (int64_t)s.mpb * s.mRm * s.mqb * s.mRs);
    L.mtouched = take((int64_t)s.mpa + s.mpb);
  }
  L.total = o;
  return L;
}

unsigned ex_grid(int64_t items) {
  int64_t cap = g_exact_grid.load(std::memory_order_relaxed);
  if (cap <= 0) cap = kDefaultGrid;
  int64_t g = items < cap ? items : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

int ex_bits(int p) {
  int b = 0;
  while (b < 31 && (1ll << b) < p) ++b;
  return b;
}

// stable sort of positions 0..n-1 by keys (values < 2^bits); *k_out / *v_out: where the sorted keys / positions are
int ex_sort(const int32_t* keys, int64_t n, int bits, char* ws, const ExLayout& L, const int32_t** k_out,
            const int32_t** v_out, hipStream_t st) {
  const int64_t ntiles = (n + kSortNT - 1) / kSortNT, m = 256 * ntiles, nblk = (m + kScanSpan - 1) / kScanSpan;
  int32_t* H = reinterpret_cast<int32_t*>(ws + L.hist);
  int32_t* sums = reinterpret_cast<int32_t*>(ws + L.sums);
  int32_t* kbuf[2] = {reinterpret_cast<int32_t*>(ws + L.kA), reinterpret_cast<int32_t*>(ws + L.kB)};
  int32_t* vbuf[2] = {reinterpret_cast<int32_t*>(ws + L.vA), reinterpret_cast<int32_t*>(ws + L.vB)};
  const int passes = bits > 0 ? (bits + 7) / 8 : 1;
  const int32_t* kin = keys;
  const int32_t* vin = nullptr;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(exact_radix_hist_kernel, dim3(ex_grid(ntiles)), dim3(kSortNT), 0, st, kin, n, shift, ntiles, H);
    hipLaunchKernelGGL(exact_scan_reduce_kernel, dim3(ex_grid(nblk)), dim3(kSortNT), 0, st, H, m, nblk, sums);
    hipLaunchKernelGGL(exact_scan_top_kernel, dim3(1), dim3(kSortNT), 0, st, sums, nblk);
    hipLaunchKernelGGL(exact_scan_down_kernel, dim3(ex_grid(nblk)), dim3(kSortNT), 0, st, H, m, nblk, sums);
    hipLaunchKernelGGL(exact_radix_scatter_kernel, dim3(ex_grid(ntiles)), dim3(kSortNT), 0, st, kin, vin, n, shift, ntiles,
                       H, kbuf[pass & 1], vbuf[pass & 1]);
    kin = kbuf[pass & 1];
    vin = vbuf[pass & 1];
  }
  *k_out = kin;
  *v_out = vin;
  return check_hip(hipGetLastError(), "exact radix sort");
}

enum ExOp { kExDense = 0, kExSgd = 1, kExAdagrad = 2 };

// the table's core behind the view's core c: -1 = none (the 2-core table's identity), -2 = the merged pair's V
int view_core(const ExShape& s, int c) {
  if (s.ident) return c == 0 ? 0 : c == 1 ? -1 : 1;
  if (s.ma >= 0) return c < s.ma ? c : c == s.ma ? -2 : c + 1;
  return c;
}

// the view's operands; a 4-core table has its pair merged into V (workspace) first
int view_cores(const ExShape& s, const float* const* cores, char* ws, const ExLayout& L, const float** G, hipStream_t st) {
  float* V = s.ma >= 0 ? reinterpret_cast<float*>(ws + L.merged) : nullptr;
  for (int c = 0; c < 3; ++c) {
    const int t = view_core(s, c);
    G[c] = t >= 0 ? cores[t] : t == -2 ? V : cores[0];   // (the identity is never read: any valid pointer)
  }
  if (V == nullptr) return TTEMB_OK;
  const int64_t n = (int64_t)s.p[s.ma] * s.s[s.ma];
  hipLaunchKernelGGL(exact_merge_kernel, dim3(ex_grid((n + 255) / 256)), dim3(256), 0, st, s, cores[s.ma], cores[s.ma + 1], V);
  return check_hip(hipGetLastError(), "exact_merge_kernel");
}

int ex_check_common(const ttemb_shape_t* shape, ExShape* s, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                    int64_t B) {
  int rc = exact_view(shape, s);
  if (rc) return rc;
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "exact mode: negative nnz / B");
  if (nnz >= (int64_t(1) << 31) - kExChunk * 64)
    return fail(TTEMB_E_UNSUPPORTED, "exact mode: %lld ids in one call (positions are 32-bit)", (long long)nnz);
  if (B >= (int64_t(1) << 31)) return fail(TTEMB_E_UNSUPPORTED, "exact mode: %lld bags in one call", (long long)B);
  if (offsets == nullptr)
    return fail(TTEMB_E_UNSUPPORTED, "exact mode needs the bag offsets (a row index without offsets is not served)");
  if (nnz > 0 && indices == nullptr) return fail(TTEMB_E_BADARG, "exact mode: indices is null");
  return TTEMB_OK;
}

// `step`: null for dense gradients into `d_cores`, else the SGD / Adagrad description a builder filled (its state has no null)
int ex_backward(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                int64_t B, const float* d_output, float* const* d_cores, const FusedUpdate* step, void* workspace,
                int64_t workspace_bytes, void* stream) {
  ExShape s;
  int rc = ex_check_common(shape, &s, indices, offsets, nnz, B);
  if (rc) return rc;
  const int op = step == nullptr ? kExDense : step->st[0] != nullptr ? kExAdagrad : kExSgd;
  const int T = shape->T;
  for (int t = 0; t < T; ++t) {
    if (cores == nullptr || cores[t] == nullptr) return fail(TTEMB_E_BADARG, "exact mode: cores[%d] is null", t);
    if (op == kExDense && (d_cores == nullptr || d_cores[t] == nullptr))
      return fail(TTEMB_E_BADARG, "exact mode: d_cores[%d] is null", t);
  }
  if (nnz > 0 && B > 0 && d_output == nullptr) return fail(TTEMB_E_BADARG, "exact mode: d_output is null");
  const ExLayout L = ex_layout(s, nnz);
  if (workspace_bytes < L.total || (L.total > 0 && workspace == nullptr))
    return fail(TTEMB_E_WORKSPACE, "exact mode: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)L.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  // the view's core c -> the table's core (-1: the lifted 2-core table's identity, -2: a 4-core table's merged pair, whose
  // gradient lives in the workspace until it is split)
  int tcore[3];
  for (int c = 0; c < 3; ++c) tcore[c] = view_core(s, c);
  const float* G[3];
  if ((rc = view_cores(s, cores, ws, L, G, st))) return rc;
  float* grad[3];
  uint8_t* touched[3];
  int64_t toff = 0;
  for (int c = 0; c < 3; ++c) {
    touched[c] = op == kExDense ? nullptr : reinterpret_cast<uint8_t*>(ws + L.touched) + toff;
    toff += s.p[c];
    grad[c] = op == kExDense && tcore[c] != -2 ? (tcore[c] >= 0 ? d_cores[tcore[c]] : nullptr)
                                               : reinterpret_cast<float*>(ws + L.grads[c]);
  }
  float* mgrad[2] = {nullptr, nullptr};
  uint8_t* mtouched[2] = {nullptr, nullptr};
  if (s.ma >= 0) {
    for (int k = 0; k < 2; ++k)
      mgrad[k] = op == kExDense ? d_cores[s.ma + k] : reinterpret_cast<float*>(ws + L.mgrads[k]);
    if (op != kExDense) {
      mtouched[0] = reinterpret_cast<uint8_t*>(ws + L.mtouched);
      mtouched[1] = mtouched[0] + s.mpa;
    }
  }
  auto split = [&]() {   // dV -> dGa, dGb (every element written; with no ids dV is all zeros / no row is touched)
    if (s.ma < 0) return (int)TTEMB_OK;
    const int64_t n = (int64_t)s.mpa * s.mRa * s.mqa * s.mRm + (int64_t)s.mpb * s.mRm * s.mqb * s.mRs;
    hipLaunchKernelGGL(exact_split_kernel, dim3(ex_grid((n + 255) / 256)), dim3(256), 0, st, s, grad[s.ma], cores[s.ma],
                       cores[s.ma + 1], mgrad[0], mgrad[1], touched[s.ma], mtouched[0], mtouched[1]);
    return check_hip(hipGetLastError(), "exact_split_kernel");
  };
  if (op == kExDense) {
    for (int c = 0; c < 3; ++c)
      if (grad[c] != nullptr && (rc = check_hip(hipMemsetAsync(grad[c], 0, 4 * (size_t)s.p[c] * s.s[c], st), "hipMemsetAsync")))
        return rc;
  } else if ((rc = check_hip(hipMemsetAsync(ws + L.touched, 0, (size_t)s.p[0] + s.p[1] + s.p[2], st), "hipMemsetAsync"))) {
    return rc;
  }
  if (nnz == 0) return op == kExDense ? split() : TTEMB_OK;   // dense: zeros; fused: no row is touched

  int32_t* keys[3];
  for (int c = 0; c < 3; ++c) keys[c] = reinterpret_cast<int32_t*>(ws + L.keys[c]);
  int32_t* bagof = reinterpret_cast<int32_t*>(ws + L.bagof);
  hipLaunchKernelGGL(exact_decode_kernel, dim3(ex_grid((nnz + kSortNT - 1) / kSortNT)), dim3(kSortNT), 0, st, s, indices,
                     offsets, B, nnz, keys[0], keys[1], keys[2], bagof);
  if ((rc = check_hip(hipGetLastError(), "exact_decode_kernel"))) return rc;
  float* partial = reinterpret_cast<float*>(ws + L.partial);
  for (int c = 0; c < 3; ++c) {
    if (tcore[c] == -1) continue;   // the identity has no gradient; the merged pair's (-2) is split below
    const int32_t *skey = nullptr, *spos = nullptr;
    if ((rc = ex_sort(keys[c], nnz, ex_bits(s.p[c]), ws, L, &skey, &spos, st))) return rc;
    const int S = s.s[c];
    const int64_t chunk = ex_chunk(S), nch = ex_nchunks(nnz, S);
    const float* g1 = G[1];
    switch (c) {
      case 0:
        hipLaunchKernelGGL(exact_chunk_kernel<0>, dim3(ex_grid(nch)), dim3(kExNT), 0, st, s, G[0], g1, G[2], indices, bagof,
                           d_output, skey, spos, nnz, chunk, nch, grad[c], partial, touched[c]);
        break;
      case 1:
        hipLaunchKernelGGL(exact_chunk_kernel<1>, dim3(ex_grid(nch)), dim3(kExNT), 0, st, s, G[0], g1, G[2], indices, bagof,
                           d_output, skey, spos, nnz, chunk, nch, grad[c], partial, touched[c]);
        break;
      default:
        hipLaunchKernelGGL(exact_chunk_kernel<2>, dim3(ex_grid(nch)), dim3(kExNT), 0, st, s, G[0], g1, G[2], indices, bagof,
                           d_output, skey, spos, nnz, chunk, nch, grad[c], partial, touched[c]);
        break;
    }
    hipLaunchKernelGGL(exact_fixup_kernel, dim3(ex_grid(nch)), dim3(kExNT), 0, st, skey, nnz, chunk, nch, S, partial,
                       grad[c], touched[c]);
    if ((rc = check_hip(hipGetLastError(), "exact chunk / fix-up kernels"))) return rc;
  }
  if ((rc = split())) return rc;
  if (op == kExDense) return TTEMB_OK;
  for (int k = 0; s.ma >= 0 && k < 2; ++k) {   // every gradient is complete: now the cores may change
    const int t = s.ma + k;
    const int64_t rows = k == 0 ? s.mpa : s.mpb;
    const int S = k == 0 ? s.mRa * s.mqa * s.mRm : s.mRm * s.mqb * s.mRs;
    if (op == kExSgd)
      hipLaunchKernelGGL(exact_sgd_kernel, dim3(ex_grid(rows)), dim3(kExNT), 0, st, cores[t], mgrad[k], mtouched[k], rows, S, step->lr,
                         step->lr_dev);
    else
      hipLaunchKernelGGL(exact_adagrad_kernel, dim3(ex_grid(rows)), dim3(kExNT), 0, st, cores[t], step->st[t], mgrad[k],
                         mtouched[k], rows, S, step->lr, step->lr_dev, step->eps);
  }
  for (int c = 0; c < 3; ++c) {
    if (tcore[c] < 0) continue;
    float* W = cores[tcore[c]];
    if (op == kExSgd)
      hipLaunchKernelGGL(exact_sgd_kernel, dim3(ex_grid(s.p[c])), dim3(kExNT), 0, st, W, grad[c], touched[c],
                         (int64_t)s.p[c], s.s[c], step->lr, step->lr_dev);
    else
      hipLaunchKernelGGL(exact_adagrad_kernel, dim3(ex_grid(s.p[c])), dim3(kExNT), 0, st, W, step->st[tcore[c]], grad[c],
                         touched[c], (int64_t)s.p[c], s.s[c], step->lr, step->lr_dev, step->eps);
  }
  return check_hip(hipGetLastError(), "exact optimiser kernel");
}

}  // namespace exact
}  // namespace ttemb

using namespace ttemb;
using namespace ttemb::exact;

extern "C" {

int64_t ttemb_exact_workspace_bytes(const ttemb_shape_t* shape, int64_t nnz, int64_t B) {
  ExShape s;
  int rc = exact_view(shape, &s);
  if (rc) return rc;
  if (nnz < 0 || B < 0) return fail(TTEMB_E_BADARG, "exact mode: negative nnz / B");
  return ex_layout(s, nnz).total;
}

int64_t ttemb_exact_plan_bytes(const ttemb_shape_t* shape, int64_t nnz) {
  ExShape s;
  int rc = exact_view(shape, &s);
  if (rc) return rc;
  (void)nnz;
  return 0;
}

int ttemb_set_exact_grid(int32_t workgroups) {
  if (workgroups < 0) return fail(TTEMB_E_BADARG, "ttemb_set_exact_grid: negative grid");
  g_exact_grid.store(workgroups, std::memory_order_relaxed);
  return TTEMB_OK;
}

int ttemb_forward_exact(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                        const int64_t* offsets, int64_t nnz, int64_t B, float* output, void* workspace,
                        int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  ExShape s;
  int rc = ex_check_common(shape, &s, indices, offsets, nnz, B);
  if (rc) return rc;
  if (B == 0) return TTEMB_OK;
  if (output == nullptr) return fail(TTEMB_E_BADARG, "exact mode: output is null");
  for (int t = 0; t < shape->T; ++t)
    if (cores == nullptr || cores[t] == nullptr) return fail(TTEMB_E_BADARG, "exact mode: cores[%d] is null", t);
  const ExLayout L = ex_layout(s, nnz);
  const int64_t need = s.ma >= 0 ? L.total : 0;   // only a 4-core table's forward uses the workspace (its merged pair)
  if (workspace_bytes < need || (need > 0 && workspace == nullptr))
    return fail(TTEMB_E_WORKSPACE, "exact mode: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float* G[3];
  if ((rc = view_cores(s, cores, reinterpret_cast<char*>(workspace), L, G, st))) return rc;
  hipLaunchKernelGGL(exact_forward_kernel, dim3(ex_grid(B)), dim3(kExNT), 0, st, s, G[0], G[1], G[2], indices, offsets, nnz,
                     B, output);
  return check_hip(hipGetLastError(), "exact_forward_kernel");
}

int ttemb_backward_dense_exact(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                               const int64_t* offsets, int64_t nnz, int64_t B, const float* d_output, float* const* d_cores,
                               void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  return ex_backward(shape, const_cast<float* const*>(cores), indices, offsets, nnz, B, d_output, d_cores, nullptr, workspace,
                     workspace_bytes, stream);
}

// Adam: the dense exact gradient into scratch behind the exact workspace, then the elementwise step (it has no order)
static int adam_exact(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                      int64_t B, const float* d_output, const FusedUpdate& step, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  ExShape s;
  int rc = ex_check_common(shape, &s, indices, offsets, nnz, B);
  if (rc) return rc;
  if (cores == nullptr) return fail(TTEMB_E_BADARG, "exact mode: null cores / moments");
  if (nnz == 0) return TTEMB_OK;   // a call without ids is a no-op (t stays)
  const int64_t base = (ex_layout(s, nnz).total + 255) / 256 * 256;
  FusedUpdate upd = step;
  float* grads[TTEMB_MAX_CORES] = {nullptr, nullptr, nullptr, nullptr};
  const float* g[TTEMB_MAX_CORES];
  long long n[TTEMB_MAX_CORES];
  int64_t off = base;
  for (int t = 0; t < shape->T; ++t) {
    n[t] = (long long)shape->p[t] * shape->R[t] * shape->q[t] * shape->R[t + 1];
    g[t] = grads[t] = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + off);
    off += (n[t] * 4 + 255) / 256 * 256;
    upd.w[t] = cores[t];
  }
  if (workspace == nullptr || workspace_bytes < off)
    return fail(TTEMB_E_WORKSPACE, "exact Adam: workspace of %lld bytes, need %lld (the exact workspace and the gradient scratch)",
                (long long)workspace_bytes, (long long)off);
  rc = ex_backward(shape, cores, indices, offsets, nnz, B, d_output, grads, nullptr, workspace, base, stream);
  if (rc) return rc;
  return run_step_arrays(upd, g, n, shape->T, 1.f, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// body of the exact fused-step entry points: SGD and Adagrad step the rows the ids touch, Adam every row
static int exact_step(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets, int64_t nnz,
                      int64_t B, const float* d_output, const FusedUpdate& step, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  if (step.v[0] != nullptr) return adam_exact(shape, cores, indices, offsets, nnz, B, d_output, step, workspace, workspace_bytes, stream);
  return ex_backward(shape, cores, indices, offsets, nnz, B, d_output, nullptr, &step, workspace, workspace_bytes, stream);
}

int ttemb_backward_sgd_exact(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets,
                             int64_t nnz, int64_t B, const float* d_output, float lr, void* workspace, int64_t workspace_bytes,
                             const void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_SGD, step_arrays(shape), lr, 0.f, nullptr, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return exact_step(shape, cores, indices, offsets, nnz, B, d_output, upd, workspace, workspace_bytes, stream);
}

int ttemb_backward_adagrad_exact(const ttemb_shape_t* shape, float* const* cores, float* const* opt_state,
                                 const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                                 const float* d_output, float lr, float eps, void* workspace, int64_t workspace_bytes,
                                 const void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAGRAD, step_arrays(shape), lr, eps, opt_state, nullptr, nullptr, nullptr, &upd);
  if (rc) return rc;
  return exact_step(shape, cores, indices, offsets, nnz, B, d_output, upd, workspace, workspace_bytes, stream);
}

int ttemb_backward_adam_exact(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                              int32_t* step, const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                              const float* d_output, const ttemb_adam_t* hp, void* workspace, int64_t workspace_bytes,
                              const void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  FusedUpdate upd;
  int rc = step_from_values(TTEMB_STEP_ADAM, step_arrays(shape), 0.f, 0.f, exp_avg, exp_avg_sq, hp, step, &upd);
  if (rc) return rc;
  return exact_step(shape, cores, indices, offsets, nnz, B, d_output, upd, workspace, workspace_bytes, stream);
}

int ttemb_backward_step_exact(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices, const int64_t* offsets,
                              int64_t nnz, int64_t B, const float* d_output, const ttemb_step_t* step, void* workspace,
                              int64_t workspace_bytes, const void* plan, int64_t plan_bytes, void* stream) {
  (void)plan;
  (void)plan_bytes;
  FusedUpdate upd;
  int rc = step_from_descriptor(step, step_arrays(shape), nullptr, &upd);
  if (rc) return rc;
  return exact_step(shape, cores, indices, offsets, nnz, B, d_output, upd, workspace, workspace_bytes, stream);
}

}  // extern "C"
