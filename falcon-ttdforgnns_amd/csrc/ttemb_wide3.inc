// Grouped chain for WIDE ranks (r1, r2 multiples of 64: the upper half of the reference's rank sweep,
// run_script.sh:250-288 -- q = 5,5,4 and q = 4,4,8 at 64 / 128 / 256).  Included by ttemb_fast3.hip inside namespace
// ttemb; it shares the grouping pass, the plan and the finalize kernel with the register-resident chain above.
//
// At these ranks an operand of the chain no longer fits a wavefront's registers (P of one group is 25 x 256 floats,
// a G1 row 1.3 MB), and the arithmetic moves from the per-id products to the per-group ones:
//
//   prefix     P[i1]   (p0 q0 x q1 r2) = G0 (p0 q0 x r1) . G1[i1] (r1 x q1 r2)          one GEMM per i1
//   forward    out[id] (q0 q1 x q2)    = P[g] . G2[i2]                                  per chunk of <= 16 ids
//   backward   E[id]   (r2 x q2)       = P[g]^T . dOut[id],  dP[g] += dOut[id] . G2[i2]^T   per group
//              dG2                     = bucket sums of the E rows (fast3_dg2_reduce_kernel, a column slice per launch row)
//              dG1[i1] (r1 x q1 r2)    = G0^T . dP[i1]                                  one GEMM per i1, K = p0 q0
//              dG0     (p0 q0 x r1)    = sum over i1 of dP[i1] . G1[i1]^T               one GEMM per i1, summed by finalize
//
// Groups are numbered i1 * p0 + i0, so the P / dP of all groups of one i1 are ONE row-major (p0 q0) x (q1 r2)
// matrix and the three per-group products are plain GEMMs against the whole G0 table: no 16-row padding of q0, no
// per-group launch structure.  The GEMMs walk the rows of the groups that hold an id only (wide3_rows_kernel lists
// them per i1; a batch in which every group holds one runs without the indirection), and their tiles are dealt to
// the 8 XCDs so that the tiles that share an operand strip share an L2.
// Every product is fp32 MFMA 16x16x4 with operands loaded straight from L2 in MFMA
// layout -- 16 bytes per lane wherever the K index is the contiguous one (the K order inside a super-step of 16 is
// permuted to make it so: lane group `hi` owns k = 16 S + 4 hi + {0..3}), nothing staged in LDS, no barriers:
// wavefronts are independent, and the MFMA stream (which on gfx950 excludes every other instruction of the SIMD,
// DESIGN.md 4.0) is interrupted by ~1 load per 4-8 MFMAs.

template <int Q0, int Q1, int Q2, int R1, int R2>
struct WideCfg {
  static constexpr int M2 = Q0 * Q1;
  static constexpr int MT2 = (M2 + 15) / 16;
  static constexpr int N1 = Q1 * R2;
  static constexpr int ROW0 = Q0 * R1, ROW1 = R1 * N1, ROW2 = R2 * Q2;
  static constexpr int D = M2 * Q2;
  static constexpr int RT2 = R2 / 16;            // 16-wide tiles over r2
  static constexpr int TW = 4;                   // rank tiles one wavefront of the backward owns (its dP accumulators)
  static constexpr int TS = RT2 / TW;            // wavefronts per group in the backward
  static constexpr int KSE = (M2 + 3) / 4;       // k-steps of the E product (K = q0 q1)
  static constexpr int QV = Q2 / 4;              // 16-byte pieces of a run of q2 floats
  static_assert(R1 % 64 == 0 && R2 % 64 == 0, "wide ranks are multiples of 64");
  static_assert(Q2 % 4 == 0, "runs of q2 floats move as float4");
  static_assert(M2 <= 32, "two row tiles");
  static_assert((R2 / 16) % 2 == 0, "the forward takes super-steps of 16 two at a time");
};

__device__ __forceinline__ float f4c(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// ---------------------------------------------------------------------------------
// fp32 products on the bf16 matrix pipe (the GEMMs below; -DTTEMB_WIDE_F32 keeps them on v_mfma_f32_16x16x4_f32).
// On gfx950 the fp32 MFMA runs at the vector rate and holds the SIMD's vector issue (DESIGN.md 4.0); the bf16 forms take
// 16 cycles for 8x the products and other wavefronts' vector instructions issue under them.  An fp32 number is exactly xh + xm + xl, three
// bf16 numbers (the three bytes of its significand); of the nine partial products of x . y, xl . yl (< 2^-30 of the
// product) is dropped and the other eight -- each exact in the accumulator's fp32 -- are summed by FOUR
// v_mfma_f32_16x16x32_bf16 whose 32 K slots are 16 real k x 2 planes: a 32-bit operand register holds two planes of ONE
// element, (lo16, hi16), so the operand layout is that of the fp32 form (lane group hi: k = 4 hi + {0..3}), one dword per
// element:
//     (xh,xm).(yh,yh) + (xh,xm).(ym,ym) + (xh,xm).(yl,yl) + (xl,xl).(yh,ym)
// The split costs 6 vector instructions per element of X and 8 per element of Y; in a 64 x 64 tile every element feeds
// four tiles, so a K-step of 16 is 64 MFMAs (1 024 cycles) next to 232 splitting instructions (928 cycles), against 64 fp32
// MFMAs of 32 cycles that exclude everything else.  Measured (409 600 ids, products table; fp32 form -> this one): dG1 GEMM
// 158 -> 123 us at rank 128 and 535 -> 407 us at rank 256, prefix GEMM 174 -> 154 and 554 -> 464 us, dG0 GEMM unchanged,
// rank 64 unchanged: a super-step takes ~2 300 cycles of its SIMD, i.e. the splitting and the MFMAs of a wavefront mostly add
// up (in-order issue: only the OTHER wavefront of the SIMD -- two fit with 230 registers -- can fill an MFMA's cycles).
// The three-plane products are exact, so the results are those of the fp32 form (test_wide_rank_gemms_keep_fp32_accuracy).
// ---------------------------------------------------------------------------------
typedef __bf16 wide_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma_split(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wide_bf16x8, a), __builtin_bit_cast(wide_bf16x8, b), c, 0, 0, 0);
}
// truncating split of four elements: x = h + m + l exactly (8 + 8 + 8 significand bits)
__device__ __forceinline__ void split_pieces(const float (&x)[4], uint32_t (&u)[4], uint32_t (&r)[4], uint32_t (&s)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i] = __float_as_uint(x[i]);
    const float rf = x[i] - __uint_as_float(u[i] & 0xffff0000u);
    r[i] = __float_as_uint(rf);
    s[i] = __float_as_uint(rf - __uint_as_float(r[i] & 0xffff0000u));
  }
}
__device__ __forceinline__ void split_x(const float (&x)[4], u32x4& hm, u32x4& ll) {
  uint32_t u[4], r[4], s[4];
  split_pieces(x, u, r, s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hm[i] = __builtin_amdgcn_perm(r[i], u[i], 0x07060302u);   // low half = top of x (h), high half = top of the remainder (m)
    ll[i] = __builtin_amdgcn_perm(s[i], s[i], 0x03020302u);
  }
}
__device__ __forceinline__ void split_y(const float (&y)[4], u32x4& hh, u32x4& mm, u32x4& ll, u32x4& hm) {
  uint32_t u[4], r[4], s[4];
  split_pieces(y, u, r, s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hh[i] = __builtin_amdgcn_perm(u[i], u[i], 0x03020302u);
    mm[i] = __builtin_amdgcn_perm(r[i], r[i], 0x03020302u);
    ll[i] = __builtin_amdgcn_perm(s[i], s[i], 0x03020302u);
    hm[i] = __builtin_amdgcn_perm(r[i], u[i], 0x07060302u);
  }
}

// ---------------------------------------------------------------------------------
// Batched GEMM  C[b] (M x N) = A[b] . B[b], one wavefront per 64 x 64 tile of C, four tiles per workgroup.
// An operand is either K-CONTIGUOUS (A stored [m][k], B stored [n][k]: one 16-byte load per lane and 16-row tile
// feeds four k-steps) or K-STRIDED (A stored [k][m], B stored [k][n]: a dword per k-step, 64 contiguous bytes per
// row of lanes).  Rows / k past an operand fall off its buffer descriptor and read zeros; rows of C past M are dropped.
// Requires: N % 64 == 0; a K-contiguous operand has K % 32 == 0; a K-strided A has M % 64 == 0; k_chunk % 32 == 0.
// COMPACT = 1: the M dimension is the list g.rows of the batch (A K-contiguous: a lane's row comes from the list; rows
// of C likewise); COMPACT = 2: the K dimension is that list (both operands K-strided: the four rows of a lane group's
// super-step are one 16-byte load of the list, requested a super-step ahead of the operand loads that use it).
// Split K (gridDim.z layers, each its own C: the caller's next kernel adds them) is for products with few tiles and a
// long K -- dG1 at rank 64 is 700 tiles of K = p0 q0.
// ---------------------------------------------------------------------------------
struct WideGemm {
  const float* A;
  const float* B;
  float* C;
  uint32_t K;
  uint32_t lda, ldb, ldc;                 // floats
  uint32_t a_batch, b_batch, c_batch;     // floats between consecutive batches (0: shared)
  uint32_t a_bytes, b_bytes, c_bytes;     // extent of one batch's operand
  uint32_t tiles_m, tiles_n;
  uint32_t k_chunk, c_slice;              // split K: launch layer z takes k in [z k_chunk, (z + 1) k_chunk) and writes C + z c_slice
  const uint32_t* rows;                   // [batches][rows_stride] the rows of the compacted dimension that hold an id (padded with the
  const uint32_t* n_rows;                 // [batches] their number                                   first row PAST the operand)
  uint32_t rows_stride;
  uint32_t full;                          // the number of rows when every group holds an id
  uint32_t batches, splits;               // the grid: batches x K splits x tiles, dealt to the XCDs by the kernel
};

// The rows (i0, a) of every i1 whose group holds an id, in order: the compacted M of the prefix / dG0 GEMMs and the
// compacted K of the dG1 GEMM.  A frontier with locality (METIS-ordered ids, small batches) touches a fraction of the
// p0 p1 groups; the GEMMs then do that fraction of the work.  One workgroup per i1.
__global__ __launch_bounds__(256) void wide3_rows_kernel(GroupPlan plan, uint32_t p0, uint32_t q0, uint32_t stride, uint32_t* __restrict__ rows,
                                                         uint32_t* __restrict__ n_rows, AdamPrep adam) {
  __shared__ uint32_t wave_sums[4];
  if (adam.step != nullptr && blockIdx.x == 0 && threadIdx.x == 0) adam_prepare(adam);   // (a backward's: for its finalize kernel)
  const uint32_t i1 = blockIdx.x;
  uint32_t base = 0;
  for (uint32_t i0_0 = 0; i0_0 < p0; i0_0 += 256u) {
    const uint32_t i0 = i0_0 + threadIdx.x;
    const uint32_t live = (i0 < p0 && plan.counts[i1 * p0 + i0] != 0u) ? 1u : 0u;
    uint32_t total;
    const uint32_t k = base + block_exclusive<uint32_t, 256>(live, wave_sums, total);
    if (live)
      for (uint32_t a = 0; a < q0; ++a) rows[(size_t)i1 * stride + k * q0 + a] = i0 * q0 + a;
    base += total;
  }
  const uint32_t n = base * q0;
  for (uint32_t e = n + threadIdx.x; e < stride; e += 256u) rows[(size_t)i1 * stride + e] = p0 * q0;   // falls off every operand
  if (threadIdx.x == 0) n_rows[i1] = n;
}

// COMPACT: the form this instance computes; SPARSE: the form a plain instance hands a batch over to when it finds that
// not every group of the batch holds an id.
template <bool A_KC, bool B_KC, int COMPACT, int SPARSE>
__device__ __forceinline__ void wide3_gemm_tile(const WideGemm& g, uint32_t tm, uint32_t tn, uint32_t b, uint32_t z, int hi, int lo) {
  static_assert(COMPACT == 0 || (COMPACT == 1 && A_KC) || (COMPACT == 2 && !A_KC && !B_KC), "see above");
  // A wavefront starts in the plain form (COMPACT = 0, identity rows): right for a batch (a value of i1) in which every
  // group holds an id -- the common case of a large uniform frontier, where the list indirection costs 5-30 % (a lookup
  // round trip in front of a four-super-step K loop; a list load and eight multiplies per super-step in the K-compacted
  // form).  It requests its first operands BEFORE it looks at the batch's count, and starts over in the compacted form
  // when the count says that some group is empty.  (Two launches, one per form, left the few non-full batches of a
  // uniform frontier alone on the machine: +10-20 %.)
  const uint32_t n_live_raw = g.n_rows[b];
  const uint32_t* rows = g.rows + (size_t)b * g.rows_stride;
  const rsrc_t r_a = make_rsrc(g.A + (size_t)b * g.a_batch, g.a_bytes);
  const rsrc_t r_b = make_rsrc(g.B + (size_t)b * g.b_batch, g.b_bytes);
  const rsrc_t r_c = make_rsrc(g.C + (size_t)z * g.c_slice + (size_t)b * g.c_batch, g.c_bytes);
  const uint32_t k0 = z * g.k_chunk;
  const uint32_t n_live = COMPACT != 0 ? uniform(n_live_raw) : g.full;   // (the plain form looks at the count after its first loads)
  if (COMPACT == 1 && 64u * tm >= n_live) return;   // (rows of C that belong to no listed row are never read)
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    uint32_t m_row = 64u * tm + 16u * t + lo;
    if constexpr (COMPACT == 1) m_row = rows[m_row];
    a_off[t] = A_KC ? (m_row * g.lda + k0 + 4u * hi) * 4u : ((COMPACT == 2 ? 0u : (k0 + 4u * hi) * g.lda) + 64u * tm + 16u * t + lo) * 4u;
    b_off[t] = B_KC ? ((64u * tn + 16u * t + lo) * g.ldb + k0 + 4u * hi) * 4u : ((COMPACT == 2 ? 0u : (k0 + 4u * hi) * g.ldb) + 64u * tn + 16u * t + lo) * 4u;
  }
  // COMPACT = 2: the list entries k0 + 16 S + 4 hi + {0..3} of the next load() call
  const uint32_t* rlist = COMPACT == 2 ? rows + k0 + 4u * hi : nullptr;
  uint4 rl_next = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (COMPACT == 2) rl_next = *reinterpret_cast<const uint4*>(rlist);
  const uint32_t a_step = A_KC ? 64u : 64u * g.lda, b_step = B_KC ? 64u : 64u * g.ldb;   // bytes per super-step of 16 k
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto load_rows = [&](float (&a)[4][4], float (&bb)[4][4], const uint4& rl) {   // COMPACT = 2: the four rows of this lane group
    const uint32_t kr[4] = {rl.x, rl.y, rl.z, rl.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a[t][s] = __uint_as_float(buf_load1u(r_a, __umul24(kr[s], g.lda * 4u) + a_off[t]));   // rows < 2^24, row pitch < 2^24 bytes
        bb[t][s] = __uint_as_float(buf_load1u(r_b, __umul24(kr[s], g.ldb * 4u) + b_off[t]));
      }
  };
  auto load = [&](float (&a)[4][4], float (&bb)[4][4], uint32_t S) {
    if constexpr (COMPACT == 2) {
      const uint4 rl = rl_next;
      rl_next = *reinterpret_cast<const uint4*>(rlist + 16u * (S + 1u));   // (the list is padded by 64 entries past its stride)
      load_rows(a, bb, rl);
      return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if constexpr (A_KC) {
        const float4 v = buf_load4(r_a, a_off[t] + S * a_step);
        a[t][0] = v.x; a[t][1] = v.y; a[t][2] = v.z; a[t][3] = v.w;
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) a[t][s] = __uint_as_float(buf_load1u(r_a, a_off[t] + S * a_step + (uint32_t)s * g.lda * 4u));
      }
      if constexpr (B_KC) {
        const float4 v = buf_load4(r_b, b_off[t] + S * b_step);
        bb[t][0] = v.x; bb[t][1] = v.y; bb[t][2] = v.z; bb[t][3] = v.w;
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) bb[t][s] = __uint_as_float(buf_load1u(r_b, b_off[t] + S * b_step + (uint32_t)s * g.ldb * 4u));
      }
    }
  };
#ifdef TTEMB_WIDE_F32
  auto mma = [&](const float (&a)[4][4], const float (&bb)[4][4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], bb[j][s], acc[i][j], 0, 0, 0);
  };
#else
  auto mma = [&](const float (&a)[4][4], const float (&bb)[4][4]) {   // a[t][s], bb[t][s]: k = 4 hi + s of the super-step
    u32x4 yhh[4], ymm[4], yll[4], yhm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_y(bb[j], yhh[j], ymm[j], yll[j], yhm[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 xhm, xll;
      split_x(a[i], xhm, xll);
      // small terms first; the four column tiles' accumulation chains alternate
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, yll[j], acc[i][j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xll, yhm[j], acc[i][j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, ymm[j], acc[i][j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, yhh[j], acc[i][j]);
    }
  };
#endif
  float a0[4][4], b0[4][4], a1[4][4], b1[4][4];
  load(a0, b0, 0u);
  if constexpr (COMPACT == 0) {
    asm volatile("" ::: "memory");        // the requests above stay above the test below (the compiler otherwise sinks them
    __builtin_amdgcn_sched_barrier(0);    // behind the wait for the count)
    if constexpr (SPARSE != 0) {
      if (uniform(n_live_raw) < g.full) {   // some group of this batch is empty: the compacted form
        wide3_gemm_tile<A_KC, B_KC, SPARSE, 0>(g, tm, tn, b, z, hi, lo);
        return;
      }
    }
  }
  const uint32_t K_eff = COMPACT == 2 ? n_live : g.K;
  const uint32_t k_len = k0 >= K_eff ? 0u : (K_eff - k0 < g.k_chunk ? K_eff - k0 : g.k_chunk);
  const uint32_t NS = (k_len + 31u) / 32u * 2u;   // super-steps, an even number (a K-strided operand reads zeros past K)
#pragma unroll 1
  for (uint32_t S = 0; S < NS; S += 2) {
    load(a1, b1, S + 1u);
    __builtin_amdgcn_sched_barrier(0);   // the next super-step's operands are requested BEFORE this one's MFMAs (the
    mma(a0, b0);                         // scheduler otherwise sinks the loads to just before their use: exposed L2 latency)
    __builtin_amdgcn_sched_barrier(0);
    load(a0, b0, S + 2u);   // unconditional (the last one reads past K: values nobody uses, and a buffer load cannot fault) --
                            // a branch here joins two load histories and the compiler then waits for vmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
    mma(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uint32_t m_row = 64u * tm + 16u * i + 4u * hi + r;
        if constexpr (COMPACT == 1) m_row = rows[m_row];
        buf_store1(r_c, (m_row * g.ldc + 64u * tn + 16u * j + lo) * 4u, acc[i][j][r]);
      }
}

// XCD-aware order.  The hardware deals workgroups to the 8 XCDs round-robin by their linear id, and every XCD has its
// own L2: with tiles numbered plainly, the ~10 tiles that share a 64-column strip of G1[i1] (or a row block of dP[i1])
// land on 8 different L2s and the strip is fetched from HBM 4-10 times (PMC, rank 256: the dG0 GEMM fetched 3.35 GB for
// 0.6 GB of operands and ran at 5.9 TB/s of HBM traffic).  The 1-D grid is therefore re-read as 8 contiguous eighths --
// workgroup L works on virtual id (L % 8) * (n / 8) + L / 8 -- so that the tiles of one (split, batch) sit on one XCD.
template <bool A_KC, bool B_KC, int SPARSE>
__global__ __launch_bounds__(256) void wide3_gemm_kernel(WideGemm g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n_wg = gridDim.x;                              // a multiple of 8
  const uint32_t v = (blockIdx.x & 7u) * (n_wg >> 3) + (blockIdx.x >> 3);
  const uint32_t wgs_per_batch = (g.tiles_m * g.tiles_n + 3u) / 4u;
  const uint32_t zb = v / wgs_per_batch, x = v - zb * wgs_per_batch;   // (split z, batch b) in one number: z * batches + b
  const uint32_t z = zb / g.batches, b = zb - z * g.batches;
  if (z >= g.splits) return;
  const uint32_t unit = uniform(x * 4u + (uint32_t)wave);
  if (unit >= g.tiles_m * g.tiles_n) return;
  const uint32_t tm = unit / g.tiles_n;
  wide3_gemm_tile<A_KC, B_KC, 0, SPARSE>(g, tm, unit - tm * g.tiles_n, b, z, lane >> 4, lane & 15);
}

// ---------------------------------------------------------------------------------
// The same GEMM through LDS, for the product whose operands are BOTH K-contiguous (dG0 parts = dP[i1] . G1[i1]^T): loaded
// straight into MFMA layout, a load instruction of such an operand touches 16 rows x 64 bytes -- half of every 128-byte
// line per super-step, the other half fetched from L2 a second time a super-step later (with 128 KB of lines in flight per
// CU nothing survives in L1): 565 us at rank 256 whatever the MFMA form, 528 with every batch reading the first batch's
// operand (it is not the misses).  Here a four-wave workgroup owns a 128 x 128 block of C and walks K in stages of 32:
// every thread loads 16 bytes of four rows of each operand -- eight threads cover one row's 128 bytes, whole lines,
// coalesced, each read once per workgroup instead of once per wavefront -- into registers a stage ahead, then into one of
// two LDS buffers (rows padded by 16 bytes: the 16-byte MFMA-layout reads of eight consecutive rows fall on different bank
// groups); one barrier per stage.  The split-bf16 MFMAs co-issue with the other wavefronts' splitting and LDS traffic
// (DESIGN.md 4.0: what ruled LDS staging out for the fp32 MFMA form does not hold for this one).
// The M rows come from the list of rows whose group holds an id (identity rows when every group does).
// Requires K % 32 == 0 and N % 128 == 0 (ranks 128 / 256; rank 64 keeps the direct form).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void wide_mma_acc(f32x4 (&acc)[4][4], const float (&a)[4][4], const float (&bb)[4][4]) {
#ifdef TTEMB_WIDE_F32
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], bb[j][s], acc[i][j], 0, 0, 0);
#else
  u32x4 yhh[4], ymm[4], yll[4], yhm[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split_y(bb[j], yhh[j], ymm[j], yll[j], yhm[j]);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32x4 xhm, xll;
    split_x(a[i], xhm, xll);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, yll[j], acc[i][j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xll, yhm[j], acc[i][j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, ymm[j], acc[i][j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_split(xhm, yhh[j], acc[i][j]);
  }
#endif
}

constexpr int kLdsGemmBlock = 128, kLdsGemmK = 32, kLdsGemmLdk = kLdsGemmK + 4;
constexpr size_t kLdsGemmBytes = (size_t)4 * kLdsGemmBlock * kLdsGemmLdk * sizeof(float);   // two buffers of A and of B

__global__ __launch_bounds__(256, 2) void wide3_gemm_lds_kernel(WideGemm g) {
  constexpr int BM = kLdsGemmBlock, KT = kLdsGemmK, LDK = kLdsGemmLdk;
  extern __shared__ __attribute__((aligned(16))) float gemm_lds[];
  float* const sa = gemm_lds;                  // [2][BM][LDK]
  float* const sb = gemm_lds + 2 * BM * LDK;   // [2][BM][LDK]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, hi = lane >> 4, lo = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;     // the wavefront's 64 x 64 quarter of the block
  // XCD-aware order (see wide3_gemm_kernel): the blocks of one batch sit on one XCD
  const uint32_t n_wg = gridDim.x;             // a multiple of 8
  const uint32_t v = (blockIdx.x & 7u) * (n_wg >> 3) + (blockIdx.x >> 3);
  const uint32_t per_batch = g.tiles_m * g.tiles_n;   // (in 128 x 128 blocks)
  const uint32_t b = v / per_batch, x = v - b * per_batch;
  if (b >= g.batches) return;
  const uint32_t bm = x / g.tiles_n, bn = x - bm * g.tiles_n;
  const uint32_t n_live = g.n_rows[b];
  if ((uint32_t)BM * bm >= n_live) return;     // (the whole workgroup: no listed row in this block)
  const uint32_t* rows = g.rows + (size_t)b * g.rows_stride;
  const rsrc_t r_a = make_rsrc(g.A + (size_t)b * g.a_batch, g.a_bytes);
  const rsrc_t r_b = make_rsrc(g.B + (size_t)b * g.b_batch, g.b_bytes);
  const rsrc_t r_c = make_rsrc(g.C + (size_t)b * g.c_batch, g.c_bytes);
  // loader: thread t takes rows t / 8 + 32 j (j = 0..3) of the block, the 16-byte piece t % 8 of the stage's 128 bytes
  const int l_row = t >> 3, l_c = (t & 7) * 4;
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t m = (uint32_t)BM * bm + (uint32_t)(l_row + 32 * j);
    const uint32_t arow = rows[m];   // (the list is padded with the first row past the operand: such a row reads zeros)
    a_off[j] = (arow * g.lda + (uint32_t)l_c) * 4u;
    b_off[j] = (((uint32_t)BM * bn + (uint32_t)(l_row + 32 * j)) * g.ldb + (uint32_t)l_c) * 4u;
  }
  float4 pa[4], pb[4];
  auto gload = [&](uint32_t kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pa[j] = buf_load4(r_a, a_off[j] + kt * (uint32_t)(KT * 4));
      pb[j] = buf_load4(r_b, b_off[j] + kt * (uint32_t)(KT * 4));
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<float4*>(sa + (buf * BM + l_row + 32 * j) * LDK + l_c) = pa[j];
      *reinterpret_cast<float4*>(sb + (buf * BM + l_row + 32 * j) * LDK + l_c) = pb[j];
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const uint32_t NK = g.K / (uint32_t)KT;
  gload(0u);
  lstore(0);
  __syncthreads();
#pragma unroll 1
  for (uint32_t kt = 0; kt < NK; ++kt) {
    const int buf = (int)(kt & 1u);
    gload(kt + 1u);   // unconditional: past K it reads past the rows (the next row's data or zeros) that nobody multiplies
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int S = 0; S < KT / 16; ++S) {
      float a[4][4], bb[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 va = *reinterpret_cast<const float4*>(sa + (buf * BM + 64 * wm + 16 * i + lo) * LDK + 16 * S + 4 * hi);
        const float4 vb = *reinterpret_cast<const float4*>(sb + (buf * BM + 64 * wn + 16 * i + lo) * LDK + 16 * S + 4 * hi);
        a[i][0] = va.x; a[i][1] = va.y; a[i][2] = va.z; a[i][3] = va.w;
        bb[i][0] = vb.x; bb[i][1] = vb.y; bb[i][2] = vb.z; bb[i][3] = vb.w;
      }
      wide_mma_acc(acc, a, bb);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1u < NK) lstore(buf ^ 1);   // the other buffer: last read a stage ago, behind the barrier that closed that stage
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t m = (uint32_t)BM * bm + (uint32_t)(64 * wm + 16 * i + 4 * hi + r);
      const uint32_t crow = rows[m];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        buf_store1(r_c, (crow * g.ldc + (uint32_t)BM * bn + (uint32_t)(64 * wn + 16 * j + lo)) * 4u, acc[i][j][r]);
    }
  }
}

// ---------------------------------------------------------------------------------
// forward, LDS-free: one wavefront per chunk (<= 16 ids of one group), any rank that is a multiple of 8.  (The form the
// wide ranks run is the persistent chain below: same products, same mapping; this one remains as the reference point of
// the measurements quoted here and is selected by -DTTEMB_WIDE_FWD_SIMPLE / -DTTEMB_FWD_DIRECT.)
//     out[id][m][kk] = sum_c P[g][m][c] G2[i2][c][kk]
// MFMA column n is the ID (lane lo), one accumulator per (row tile mt, kk).  The K order is permuted so that every
// operand is a run of contiguous floats per lane: in a super-step of 4 CPL values of c, lane group `hi` owns
// c = SS S + CPL hi + {0 .. CPL-1}, so
//     A  = P[g][16 mt + lo][that run]                 -- CPL floats: one 16-byte load per row tile
//     B  = G2[i2_lo][that run][0 .. q2-1]             -- CPL q2 contiguous floats: the B operands of ALL q2 accumulators
// and the accumulators come out as out[id lo][m = 16 mt + 4 hi + {0..3}][0 .. q2-1]: 4 q2 contiguous floats of the
// id's row per lane -- stored straight from registers.  Per chunk of the products shape that is 7 loads, 40 MFMAs and
// 10 stores: no staging of G2 rows, no transposition of the output rows through LDS, no ds_read per operand.
// It is the forward of the wide ranks, where the products dominate.  For the narrow ranks (r2 <= 32) it does not beat
// the staged persistent kernel above (products shape, 409 600 ids; -DTTEMB_FWD_DIRECT selects it there): as is, 65 us
// against 44 -- its stores are 16-byte pieces 80 bytes apart (64 partial sectors per instruction instead of whole
// 400-byte rows: +24 us) and a wavefront per chunk pays three dependent round trips (descriptor, ids, operands).  As a
// persistent chain (operands of chunk c+1, ids of c+2, descriptor of c+3 in flight; rows transposed through LDS and
// stored whole) it took 43.3 us -- the staged kernel's time.  Its ablations say why (same box, one call): nothing but
// descriptors and ids 7.8 us; + operand loads 21.2; + MFMAs without loads 30.1; loads + MFMAs 32.2; + row transposition
// and stores 43.3.  The 40 MFMAs of a chunk alone hold the machine for 22 us (their nominal 20) and the ~60 LDS / store
// / address instructions of the output phase add their full issue time on top (DESIGN.md 4.0): the forward is bound by
// instruction issue on the MFMA-blocked SIMD, not by where its operands come from.
// ---------------------------------------------------------------------------------
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <int N>
__device__ __forceinline__ void load_run(rsrc_t r, uint32_t off, float (&dst)[N]) {   // N contiguous floats, 8-byte aligned at least
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int v = 0; v < N / 4; ++v) {
      const float4 x = buf_load4(r, off + 16u * v);
      dst[4 * v] = x.x; dst[4 * v + 1] = x.y; dst[4 * v + 2] = x.z; dst[4 * v + 3] = x.w;
    }
  } else {
    static_assert(N % 2 == 0, "runs are whole 8-byte pieces");
#pragma unroll
    for (int v = 0; v < N / 2; ++v) {
      const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(off + 8u * v), 0, 0);
      dst[2 * v] = __uint_as_float(x.x); dst[2 * v + 1] = __uint_as_float(x.y);
    }
  }
}

template <int Q0, int Q1, int Q2, int R1, int R2>
struct DirectCfg {
  static constexpr int M2 = Q0 * Q1, MT2 = (M2 + 15) / 16, D = M2 * Q2, ROW2 = R2 * Q2;
  static constexpr int CPL = R2 >= 16 ? 4 : R2 / 4;   // consecutive c a lane group owns per super-step
  static constexpr int SS = 4 * CPL;                  // c per super-step
  static constexpr int NS = R2 / SS;
  static constexpr int BF = CPL * Q2;                 // floats of the lane's G2 run per super-step
  static constexpr int OF = 4 * Q2;                   // floats of the lane's output run per row tile
  static constexpr bool ok = R2 % 8 == 0 && R2 % SS == 0 && (CPL == 4 || CPL == 2) && (M2 % 4 == 0 || Q2 % 4 == 0) && MT2 <= 2;
};

template <int Q0, int Q1, int Q2, int R1, int R2>
__global__ __launch_bounds__(256) void direct_forward_kernel(const float* __restrict__ G2, GroupPlan plan, uint32_t G, uint32_t p2,
                                                             float* __restrict__ out, uint32_t out_bytes) {
  using C = DirectCfg<Q0, Q1, Q2, R1, R2>;
  static_assert(C::ok, "shape outside the direct forward kernel");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hi = lane >> 4, lo = lane & 15;
  const uint32_t nchunks = (uint32_t)(plan.gpre[G] >> 32);
  const uint32_t c = uniform(blockIdx.x * 4u + (uint32_t)wave);
  if (plan_poisoned(plan, G)) {   // a bounded wait of the grouping pass ran out: NaN rows (see report_fault)
    poison_output(plan, out, out_bytes, (uint32_t)(Q0 * Q1 * Q2), c, gridDim.x * 4u, lane);
    return;
  }
  if (c >= nchunks) return;
  const uint4 d = plan.ctab[c];
  const uint32_t pos = uniform(d.x), grp = uniform(d.y), len = uniform(d.z) & 0xffu;
  const bool on = (uint32_t)lo < len;
  const uint32_t i2 = on ? plan.i2s[pos + lo] : 0u;
  const uint32_t val = on ? plan.vals[pos + lo] : 0u;
  const rsrc_t r_p = make_rsrc(plan.ptab + (size_t)grp * (C::M2 * R2), (uint32_t)(C::M2 * R2 * 4));
  const rsrc_t r_g2 = make_rsrc(G2, p2 * (uint32_t)(C::ROW2 * 4));
  if (plan.piece != nullptr) {   // a piece of a larger call: rows count from the piece's first bag
    out += plan.piece->rowbase * (long long)(Q0 * Q1 * Q2);
    out_bytes = (uint32_t)plan.piece->window_bytes;
  }
  const rsrc_t r_out = make_rsrc(out, out_bytes);
  uint32_t p_off[C::MT2];
#pragma unroll
  for (int mt = 0; mt < C::MT2; ++mt) p_off[mt] = (uint32_t)((16 * mt + lo) * R2 + C::CPL * hi) * 4u;   // rows >= q0 q1 fall off the group's slot
  const uint32_t g_off = (on && i2 < p2) ? i2 * (uint32_t)(C::ROW2 * 4) + (uint32_t)(C::CPL * hi * Q2 * 4) : kOobBase;
  f32x4 acc[C::MT2][Q2];
#pragma unroll
  for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
    for (int j = 0; j < Q2; ++j) acc[mt][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto load = [&](float (&a)[C::MT2][C::CPL], float (&bb)[C::BF], uint32_t S) {
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt) load_run<C::CPL>(r_p, p_off[mt] + (uint32_t)(C::SS * 4) * S, a[mt]);
    load_run<C::BF>(r_g2, g_off + (uint32_t)(C::SS * Q2 * 4) * S, bb);
  };
  auto mma = [&](const float (&a)[C::MT2][C::CPL], const float (&bb)[C::BF]) {
#pragma unroll
    for (int s = 0; s < C::CPL; ++s)
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
        for (int j = 0; j < Q2; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][s], bb[s * Q2 + j], acc[mt][j], 0, 0, 0);
  };
  float a0[C::MT2][C::CPL], b0[C::BF];
  load(a0, b0, 0u);
  if constexpr (C::NS == 1) {
    mma(a0, b0);
  } else {
    static_assert(C::NS == 1 || C::NS % 2 == 0, "super-steps are taken two at a time");
    float a1[C::MT2][C::CPL], b1[C::BF];
#pragma unroll 1
    for (uint32_t S = 0; S < (uint32_t)C::NS; S += 2) {
      load(a1, b1, S + 1u);
      __builtin_amdgcn_sched_barrier(0);   // the next super-step's operands are requested BEFORE this one's MFMAs
      mma(a0, b0);
      __builtin_amdgcn_sched_barrier(0);
      load(a0, b0, S + 2u);   // unconditional (past r2: values nobody uses; a buffer load cannot fault) -- a branch here
      __builtin_amdgcn_sched_barrier(0);   // joins two load histories and the compiler then waits for vmcnt(0)
      mma(a1, b1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // lane (hi, lo) holds out[id lo][m = 16 mt + 4 hi + r][kk]: a run of 4 q2 floats of the id's row per row tile
  const bool multi = (val & kMultiBit) != 0u;
  const uint32_t row_off = __umul24(val & 0x00ffffffu, (uint32_t)(C::D * 4));
  const bool some_multi = __ballot(on && multi) != 0ull;
#pragma unroll
  for (int mt = 0; mt < C::MT2; ++mt) {
    const int m0 = 16 * mt + 4 * hi;
    const int valid = (C::M2 - m0 > 4 ? 4 : (C::M2 - m0 < 0 ? 0 : C::M2 - m0)) * Q2;   // floats of the run that are rows < q0 q1 (a multiple of 4)
#pragma unroll
    for (int v = 0; v < C::OF / 4; ++v) {
      float4 x;
      x.x = acc[mt][(4 * v + 0) % Q2][(4 * v + 0) / Q2];
      x.y = acc[mt][(4 * v + 1) % Q2][(4 * v + 1) / Q2];
      x.z = acc[mt][(4 * v + 2) % Q2][(4 * v + 2) / Q2];
      x.w = acc[mt][(4 * v + 3) % Q2][(4 * v + 3) / Q2];
      const bool here = on && 4 * v < valid;
      buf_store4(r_out, here && !multi ? row_off + (uint32_t)(m0 * Q2 * 4 + 16 * v) : kOobBase, x);
      if (some_multi && here && multi) {   // a bag of several ids: its row was zeroed by the grouping pass, the ids add into it
        float* dst = out + (size_t)(val & 0x00ffffffu) * C::D + m0 * Q2 + 4 * v;
        atomicAdd(dst + 0, x.x);
        atomicAdd(dst + 1, x.y);
        atomicAdd(dst + 2, x.z);
        atomicAdd(dst + 3, x.w);
      }
    }
  }
}

// The same products as a persistent chain (wide ranks: two or more super-steps per chunk).  Every wavefront takes an equal
// contiguous share of the chunk table and never drains its load queue: the super-step after the last one of chunk c is
// the first one of chunk c + 1 (whose ids were requested a chunk earlier, and whose descriptor two chunks earlier -- after
// the instructions that read descriptor registers, because any use of a scalar register waits for every scalar load in
// flight).  A wavefront per chunk paid three dependent round trips (descriptor, ids, first operands) per 128 MFMAs at rank 64.
template <int Q0, int Q1, int Q2, int R1, int R2>
__global__ __launch_bounds__(256) void direct_forward_chain_kernel(const float* __restrict__ G2, GroupPlan plan, uint32_t G, uint32_t p2,
                                                                   float* __restrict__ out, uint32_t out_bytes) {
  using C = DirectCfg<Q0, Q1, Q2, R1, R2>;
  static_assert(C::ok && C::NS >= 2 && C::NS % 2 == 0, "super-steps are taken two at a time");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hi = lane >> 4, lo = lane & 15;
  const desc_ptr ctab = (desc_ptr)plan.ctab;
  const uint32_t nchunks = ((desc_ptr)plan.gpre)[2u * G + 1u];
  const uint32_t waves = gridDim.x * 4u, w = uniform(blockIdx.x * 4u + (uint32_t)wave);
  if (plan_poisoned(plan, G)) {   // a bounded wait of the grouping pass ran out: NaN rows (see report_fault)
    poison_output(plan, out, out_bytes, (uint32_t)(Q0 * Q1 * Q2), w, waves, lane);
    return;
  }
  const uint32_t per = (nchunks + waves - 1u) / waves;
  const uint32_t c0 = w * per < nchunks ? w * per : nchunks, c1 = c0 + per < nchunks ? c0 + per : nchunks;
  if (c0 >= c1) return;
  const rsrc_t r_g2 = make_rsrc(G2, p2 * (uint32_t)(C::ROW2 * 4));
  if (plan.piece != nullptr) {   // a piece of a larger call: rows count from the piece's first bag
    out += plan.piece->rowbase * (long long)(Q0 * Q1 * Q2);
    out_bytes = (uint32_t)plan.piece->window_bytes;
  }
  const rsrc_t r_out = make_rsrc(out, out_bytes);
  const uint32_t live = ((desc_ptr)plan.gpre)[2u * G];
  const rsrc_t r_i2 = make_rsrc(plan.i2s, live * 4u);
  const rsrc_t r_val = make_rsrc(plan.vals, live * 4u);
  struct Ids { uint32_t i2, val; };
  auto ids_of = [&](const uint4& d) {   // the id of slot lo of chunk d (zeros past the chunk)
    Ids x;
    const uint32_t off = (uint32_t)lo < (d.z & 0xffu) ? (d.x + (uint32_t)lo) * 4u : kOobBase;
    x.i2 = buf_load1u(r_i2, off);
    x.val = buf_load1u(r_val, off);
    return x;
  };
  uint32_t p_off[C::MT2];
#pragma unroll
  for (int mt = 0; mt < C::MT2; ++mt) p_off[mt] = (uint32_t)((16 * mt + lo) * R2 + C::CPL * hi) * 4u;
  // operands of super-step S of the chunk (d, id)
  auto load = [&](const uint4& d, const Ids& id, float (&a)[C::MT2][C::CPL], float (&bb)[C::BF], uint32_t S) {
    const bool on = (uint32_t)lo < (d.z & 0xffu);
    const rsrc_t r_p = make_rsrc(plan.ptab + (size_t)uniform(d.y) * (C::M2 * R2), (uint32_t)(C::M2 * R2 * 4));
    const uint32_t g_off = (on && id.i2 < p2) ? id.i2 * (uint32_t)(C::ROW2 * 4) + (uint32_t)(C::CPL * hi * Q2 * 4) : kOobBase;
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt) load_run<C::CPL>(r_p, p_off[mt] + (uint32_t)(C::SS * 4) * S, a[mt]);
    load_run<C::BF>(r_g2, g_off + (uint32_t)(C::SS * Q2 * 4) * S, bb);
  };
  f32x4 acc[C::MT2][Q2];
  auto mma = [&](const float (&a)[C::MT2][C::CPL], const float (&bb)[C::BF]) {
#pragma unroll
    for (int s = 0; s < C::CPL; ++s)
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
        for (int j = 0; j < Q2; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][s], bb[s * Q2 + j], acc[mt][j], 0, 0, 0);
  };
  auto store = [&](const uint4& d, const Ids& id) {   // lane (hi, lo) holds out[id lo][m = 16 mt + 4 hi + r][kk]
    const bool on = (uint32_t)lo < (d.z & 0xffu);
    const bool multi = (id.val & kMultiBit) != 0u;
    const uint32_t row_off = __umul24(id.val & 0x00ffffffu, (uint32_t)(C::D * 4));
    const bool some_multi = __ballot(on && multi) != 0ull;
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt) {
      const int m0 = 16 * mt + 4 * hi;
      const int valid = (C::M2 - m0 > 4 ? 4 : (C::M2 - m0 < 0 ? 0 : C::M2 - m0)) * Q2;
#pragma unroll
      for (int v = 0; v < C::OF / 4; ++v) {
        float4 x;
        x.x = acc[mt][(4 * v + 0) % Q2][(4 * v + 0) / Q2];
        x.y = acc[mt][(4 * v + 1) % Q2][(4 * v + 1) / Q2];
        x.z = acc[mt][(4 * v + 2) % Q2][(4 * v + 2) / Q2];
        x.w = acc[mt][(4 * v + 3) % Q2][(4 * v + 3) / Q2];
        buf_store4(r_out, on && 4 * v < valid && !multi ? row_off + (uint32_t)(m0 * Q2 * 4 + 16 * v) : kOobBase, x);
      }
    }
    if (some_multi) {   // rare: a bag of several ids -- its row was zeroed by the grouping pass, the ids add into it
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < Q2; ++j) {
            const int m = 16 * mt + 4 * hi + r;
            if (on && multi && m < C::M2) atomicAdd(out + (size_t)(id.val & 0x00ffffffu) * C::D + m * Q2 + j, acc[mt][j][r]);
          }
    }
  };
  uint4 d0 = load_desc(ctab, c0, c1), d1 = load_desc(ctab, c0 + 1u, c1), d2 = load_desc(ctab, c0 + 2u, c1);
  Ids i0 = ids_of(d0), i1 = ids_of(d1);
  float aA[C::MT2][C::CPL], bA[C::BF], aB[C::MT2][C::CPL], bB[C::BF];
  load(d0, i0, aA, bA, 0u);
#pragma unroll 1
  for (uint32_t c = c0; c < c1; ++c) {
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
      for (int j = 0; j < Q2; ++j) acc[mt][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Ids i2 = i1;
    uint4 d3 = d2;
#pragma unroll
    for (int S = 0; S < C::NS; S += 2) {
      load(d0, i0, aB, bB, (uint32_t)S + 1u);
      if (S == 0) {            // the ids of chunk c + 2 and the descriptor of c + 3, behind the uses of d0 above
        i2 = ids_of(d2);
        d3 = load_desc(ctab, c + 3u, c1);
      }
      __builtin_amdgcn_sched_barrier(0);
      mma(aA, bA);
      __builtin_amdgcn_sched_barrier(0);
      if (S + 2 < C::NS) load(d0, i0, aA, bA, (uint32_t)S + 2u);
      else load(d1, i1, aA, bA, 0u);   // the first super-step of the next chunk (an empty chunk past the share: zeros)
      __builtin_amdgcn_sched_barrier(0);
      mma(aB, bB);
      __builtin_amdgcn_sched_barrier(0);
    }
    store(d0, i0);
    __builtin_amdgcn_sched_barrier(0);
    d0 = d1; d1 = d2; d2 = d3;
    i0 = i1; i1 = i2;
  }
}

// ---------------------------------------------------------------------------------
// backward, per group: wavefront (g, ts) owns the rank tiles t = TW ts .. TW ts + TW - 1 of group g, walks the
// group's ids 16 at a time and keeps its tiles of dP[g] in accumulators until the group is done (plain stores, every
// non-empty group is written; the GEMMs that follow walk the non-empty groups only).  Per 16 ids it
// loads the d_output rows once, in the two register layouts the products want, and per rank tile
//     E[c][id][kk]  = sum_m  P[g][m][c] dOut[id][m][kk]            (K = q0 q1; E row of id: [kk][c], 16 bytes per lane)
//     dP[m][c]     += sum_(id,kk) dOut[id][m][kk] G2[i2_id][c][kk]  (K = 16 q2: lane group hi owns id = 4 S + hi)
// ---------------------------------------------------------------------------------
template <int Q0, int Q1, int Q2, int R1, int R2>
__global__ __launch_bounds__(256) void wide3_bwd_chunk_kernel(const float* __restrict__ G2, uint32_t G, uint32_t p2,
                                                              const float* __restrict__ d_out, uint32_t dout_bytes, GroupPlan plan) {
  using C = WideCfg<Q0, Q1, Q2, R1, R2>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hi = lane >> 4, lo = lane & 15;
  const uint32_t unit = uniform(blockIdx.x * 4u + (uint32_t)wave);
  const uint32_t grp = unit / C::TS, ts = unit - grp * C::TS;
  if (grp >= G || plan_poisoned(plan, G)) return;   // (a poisoned plan: the finalize kernel emits NaN gradients)
  const uint32_t cnt = uniform(plan.counts[grp]);
  if (cnt == 0u) return;   // no row of an empty group is read by the compacted GEMMs
  const uint32_t first = uniform((uint32_t)plan.gpre[grp]);
  const rsrc_t r_p = make_rsrc(plan.ptab + (size_t)grp * (C::M2 * R2), (uint32_t)(C::M2 * R2 * 4));
  const rsrc_t r_dp = make_rsrc(plan.dptab + (size_t)grp * (C::M2 * R2), (uint32_t)(C::M2 * R2 * 4));
  const rsrc_t r_g2 = make_rsrc(G2, p2 * (uint32_t)(C::ROW2 * 4));
  if (plan.piece != nullptr) {   // a piece of a larger call: rows count from the piece's first bag
    d_out += plan.piece->rowbase * (long long)(Q0 * Q1 * Q2);
    dout_bytes = (uint32_t)plan.piece->window_bytes;
  }
  const rsrc_t r_do = make_rsrc(d_out, dout_bytes);
  f32x4 dp[C::TW][C::MT2];
#pragma unroll
  for (int tl = 0; tl < C::TW; ++tl)
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt) dp[tl][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (uint32_t base = 0; base < cnt; base += 16u) {
    const uint32_t len = cnt - base < 16u ? cnt - base : 16u;
    const uint32_t pos = first + base;
    const bool on = (uint32_t)lo < len;
    const uint32_t i2_lo = on ? plan.i2s[pos + lo] : 0u;
    const uint32_t val_lo = on ? plan.vals[pos + lo] : 0u;
    const uint32_t row_lo = on ? __umul24(val_lo & 0x00ffffffu, (uint32_t)(C::D * 4)) : kOobBase;
    // d_output, E form: B[k = m = 4 s + hi][n = id lo], the q2 values of (id, m) in one lane
    float4 be[C::KSE][C::QV];
#pragma unroll
    for (int s = 0; s < C::KSE; ++s)
#pragma unroll
      for (int v = 0; v < C::QV; ++v)
        be[s][v] = buf_load4(r_do, (4 * s + hi < C::M2) ? row_lo + (uint32_t)((4 * s + hi) * Q2 * 4 + 16 * v) : kOobBase);
    // d_output, dP form: A[m = 16 mt + lo][k = (id = 4 S + hi, kk)]
    float4 ad[4][C::MT2][C::QV];
    uint32_t g2_S[4];
#pragma unroll
    for (int S = 0; S < 4; ++S) {
      const uint32_t row_S = __shfl(row_lo, 4 * S + hi, kWave);   // kOobBase for an id past the chunk
      const uint32_t i2_S = __shfl(i2_lo, 4 * S + hi, kWave);
      g2_S[S] = (row_S != kOobBase && i2_S < p2) ? i2_S * (uint32_t)(C::ROW2 * 4) : kOobBase;
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
        for (int v = 0; v < C::QV; ++v)
          ad[S][mt][v] = buf_load4(r_do, (16 * mt + lo < C::M2) ? row_S + (uint32_t)((16 * mt + lo) * Q2 * 4 + 16 * v) : kOobBase);
    }
    const rsrc_t r_e = make_rsrc(plan.etab + (size_t)pos * C::ROW2, 16u * (uint32_t)(C::ROW2 * 4));   // this chunk's 16 E rows
    // operands of rank tile t: P columns (A of the E product) and the G2 rows of the 16 ids (B of the dP product);
    // tile tl + 1 is requested before the MFMAs of tile tl (two register sets)
    float pa[2][C::KSE];
    float4 gb[2][4][C::QV];
    auto load_tile = [&](int buf, uint32_t t) {
#pragma unroll
      for (int s = 0; s < C::KSE; ++s) pa[buf][s] = __uint_as_float(buf_load1u(r_p, ((uint32_t)((4 * s + hi) * R2) + 16u * t + lo) * 4u));   // m >= q0 q1: zeros
#pragma unroll
      for (int S = 0; S < 4; ++S)
#pragma unroll
        for (int v = 0; v < C::QV; ++v) gb[buf][S][v] = buf_load4(r_g2, g2_S[S] + ((16u * t + lo) * Q2) * 4u + 16u * v);
    };
    load_tile(0, ts * C::TW);
#pragma unroll
    for (int tl = 0; tl < C::TW; ++tl) {
      const uint32_t t = ts * C::TW + tl;
      const int cur = tl & 1;
      if (tl + 1 < C::TW) load_tile(cur ^ 1, t + 1u);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 e[Q2];
#pragma unroll
      for (int j = 0; j < Q2; ++j) e[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < C::KSE; ++s)
#pragma unroll
        for (int j = 0; j < Q2; ++j) e[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[cur][s], f4c(be[s][j / 4], j % 4), e[j], 0, 0, 0);
#pragma unroll
      for (int S = 0; S < 4; ++S)   // (no skipping of the k-steps of a short chunk: a branch here makes the compiler sink the
#pragma unroll                      //  operand loads into it, behind a full wait)
        for (int kk = 0; kk < Q2; ++kk)
#pragma unroll
          for (int mt = 0; mt < C::MT2; ++mt)
            dp[tl][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(ad[S][mt][kk / 4], kk % 4), f4c(gb[cur][S][kk / 4], kk % 4), dp[tl][mt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // E row of id lo, layout [kk][c]: lane holds c = 16 t + 4 hi + {0..3} for every kk
#if defined(TTEMB_ABL) && (TTEMB_ABL & 2048)   // (ablation 2048: the E rows are not stored; timing only)
      if (G == 0xffffffffu)
#endif
#pragma unroll
      for (int j = 0; j < Q2; ++j)
        buf_store4(r_e, on ? (uint32_t)lo * (uint32_t)(C::ROW2 * 4) + ((uint32_t)(j * R2) + 16u * t + 4u * hi) * 4u : kOobBase,
                   make_float4(e[j][0], e[j][1], e[j][2], e[j][3]));
    }
  }
#pragma unroll
  for (int tl = 0; tl < C::TW; ++tl)
#pragma unroll
    for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)   // rows >= q0 q1 fall off the group's slot
        buf_store1(r_dp, ((uint32_t)((16 * mt + 4 * hi + r) * R2) + 16u * (ts * C::TW + tl) + lo) * 4u, dp[tl][mt][r]);
}

// ---------------------------------------------------------------------------------
// backward, per (chunk, rank tile), the dG2 reduction INSIDE the kernel: no E table (round 5).
//
// wide3_bwd_chunk_kernel writes one E row per id (r2 q2 floats: 4 KB at rank 256, q2 = 4; 8 KB at q2 = 8 -- 1.7 / 3.4 GB for
// 409 600 ids) and fast3_dg2_reduce_kernel reads the table back: a timing-only build without the stores and without the
// reduce launch takes 30 % (q = 5,5,4) / 49 % (q = 4,4,8) off the rank-256 backward (profiles/r05_wide_E_ablation.txt).
// Here a wavefront owns ONE rank tile t (16 values of c2) for the whole launch and keeps the tile's slice of dG2 --
// p2 rows of q2 x 16 floats -- in LDS: 38 KB at q2 = 4 (four wavefronts per CU), 75 KB at q2 = 8 (two).  It walks a contiguous
// share of the chunk table (the workgroup's wavefronts walk the SAME share with consecutive tiles: the d_output rows of a
// chunk come out of the CU's L1 for three of the four), forms the chunk's E tile in registers as before (MFMA column = id)
// and ADDS it into the slab rows of the ids' i2 with plain 16-byte LDS read-modify-writes: a lane owns its (id, 4 c2) quad,
// wavefronts own disjoint columns, and two ids of one chunk with the same i2 are told apart by an LDS tag (every id writes
// its slot number to tag[i2] and reads it back: the winner adds, the others go round again -- LDS operations of a wavefront
// are processed in order).  ds_add_f32 at ~160 cycles per wave-instruction was what made an LDS slab lose in round 2; these
// are 2 x q2 16-byte operations per chunk and tile.  dP accumulates over the chunks of a group as before (a wavefront owns the
// groups whose first chunk lies in its share) and is stored per (group, tile).  At the end every wavefront stores its slice of
// the share's slab: GS = CUs / (tiles per workgroup) slabs in all, summed by fast3_finalize_kernel.
// Software pipeline over the chunk table, two register sets: the operands of chunk c + 1 are requested before the MFMAs of
// chunk c, the ids of c + 2 and the descriptor of c + 3 behind them.
// ---------------------------------------------------------------------------------
// JS = 2 (q2 = 8): a tile's slice is SPLIT over two wavefronts by k2 halves -- each forms its half of the E tile (half the E
// MFMAs, half the slab: four wavefronts per CU instead of two) and BOTH accumulate the whole dP of the tile (the dP MFMAs are
// done twice; the wavefront of the first half stores it).  Two idle SIMDs per CU cost more than the repeated MFMAs.
template <int Q0, int Q1, int Q2, int R1, int R2, int JS>
__global__ __launch_bounds__(256) void wide3_bwd_slab_kernel(const float* __restrict__ G2, uint32_t G, uint32_t p2, const float* __restrict__ d_out,
                                                             uint32_t dout_bytes, GroupPlan plan, uint32_t wpb, uint32_t shares) {
  using C = WideCfg<Q0, Q1, Q2, R1, R2>;
  static_assert(JS == 1 || (JS == 2 && Q2 % 8 == 0), "k2 halves are whole 16-byte pieces of a d_output run");
  constexpr int QJ = Q2 / JS;        // k2 values this wavefront reduces
  constexpr int LDR = QJ * 16 + 4;   // slab row stride in floats: rows 16 bytes apart mod 128 -- ids of one chunk spread over the banks
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const int hi = lane >> 4, lo = lane & 15;
  if (wave >= wpb) return;   // (q2 = 8: two wavefronts per workgroup)
  float* const slab = smem + wave * (p2 * (uint32_t)(LDR + 1));
  uint32_t* const tag = reinterpret_cast<uint32_t*>(slab + p2 * (uint32_t)LDR);
  const uint32_t tgroups = (uint32_t)(C::RT2 * JS) / wpb;              // workgroups that cover the (rank tile, k2 half) units of one share
  const uint32_t unit = (blockIdx.x % tgroups) * wpb + wave;
  const uint32_t t = unit / JS;                                       // this wavefront's rank tile
  const int jh = (int)(unit % JS);                                    // ... and its k2 half (wave-uniform)
  const uint32_t share = blockIdx.x / tgroups;                        // < shares
  if (plan_poisoned(plan, G)) return;   // (the finalize kernel emits NaN gradients)
  for (uint32_t i = lane; i < p2 * (uint32_t)LDR; i += kWave) slab[i] = 0.f;
  const desc_ptr ctab = (desc_ptr)plan.ctab;
  const uint32_t nchunks = ((desc_ptr)plan.gpre)[2u * G + 1u];
  const uint32_t per = (nchunks + shares - 1u) / shares;
  const uint32_t c0 = share * per, c1 = c0 + per < nchunks ? c0 + per : nchunks;
  bool have = c0 < nchunks;
  uint32_t c = c0;
  if (have && !(ctab[4u * c0 + 2u] & kFirstBit)) {   // the share begins inside a group: that group belongs to the share before
    c = ctab[4u * c0 + 3u];
    have = c < c1;
  }
  const rsrc_t r_g2 = make_rsrc(G2, p2 * (uint32_t)(C::ROW2 * 4));
  if (plan.piece != nullptr) {   // a piece of a larger call: rows count from the piece's first bag
    d_out += plan.piece->rowbase * (long long)(Q0 * Q1 * Q2);
    dout_bytes = (uint32_t)plan.piece->window_bytes;
  }
  const rsrc_t r_do = make_rsrc(d_out, dout_bytes);
  const uint32_t live = ((desc_ptr)plan.gpre)[2u * G];
  const rsrc_t r_i2 = make_rsrc(plan.i2s, live * 4u);
  const rsrc_t r_val = make_rsrc(plan.vals, live * 4u);
  const uint4 none = make_uint4(0u, 0u, 0u, 0u);
  auto has_next = [&](uint32_t cc, const uint4& d) { return cc + 1u < nchunks && !((d.z & kLastBit) && cc + 1u >= c1); };
  struct Ids { uint32_t i2, row; };   // of slot lo: last index digit, byte offset of its d_output row (kOobBase past the chunk)
  auto ids_of = [&](const uint4& d) {
    Ids x;
    const bool on = (uint32_t)lo < (d.z & 0xffu);
    const uint32_t off = on ? (d.x + (uint32_t)lo) * 4u : kOobBase;
    x.i2 = buf_load1u(r_i2, off);
    x.row = buf_load1u(r_val, off);   // (the row word; turned into an offset when the operands are requested)
    return x;
  };
  struct Ops {   // operands of one chunk for this rank tile
    float4 be[C::KSE][C::QV / JS];  // d_output, E form: B[k = m = 4 s + hi][n = id lo], this wavefront's k2 values
    float4 ad[4][C::MT2][C::QV];    // d_output, dP form: A[m = 16 mt + lo][k = (id = 4 S + hi, kk)]
    float4 gb[4][C::QV];            // G2 rows of the ids 4 S + hi: B[k = (id, kk)][n = c2 = 16 t + lo]
    float pa[C::KSE];               // P columns of the tile: A[c2 = 16 t + lo][k = m = 4 s + hi]
    uint32_t i2;                    // of slot lo (p2 = "no id")
  };
  auto load = [&](const uint4& d, const Ids& id, Ops& o) {
    const bool on = (uint32_t)lo < (d.z & 0xffu);
    const uint32_t row_lo = on ? __umul24(id.row & 0x00ffffffu, (uint32_t)(C::D * 4)) : kOobBase;
    o.i2 = on && id.i2 < p2 ? id.i2 : p2;
#pragma unroll
    for (int s = 0; s < C::KSE; ++s)
#pragma unroll
      for (int v = 0; v < C::QV / JS; ++v)
        o.be[s][v] = buf_load4(r_do, (4 * s + hi < C::M2) ? row_lo + (uint32_t)((4 * s + hi) * Q2 * 4 + 16 * v) + (uint32_t)(jh * QJ * 4) : kOobBase);
#pragma unroll
    for (int S = 0; S < 4; ++S) {
      const uint32_t row_S = __shfl(row_lo, 4 * S + hi, kWave);   // kOobBase for an id past the chunk
      const uint32_t i2_S = __shfl(o.i2, 4 * S + hi, kWave);
      const uint32_t g2_S = (row_S != kOobBase && i2_S < p2) ? i2_S * (uint32_t)(C::ROW2 * 4) : kOobBase;
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt)
#pragma unroll
        for (int v = 0; v < C::QV; ++v)
          o.ad[S][mt][v] = buf_load4(r_do, (16 * mt + lo < C::M2) ? row_S + (uint32_t)((16 * mt + lo) * Q2 * 4 + 16 * v) : kOobBase);
#pragma unroll
      for (int v = 0; v < C::QV; ++v) o.gb[S][v] = buf_load4(r_g2, g2_S + ((16u * t + lo) * Q2) * 4u + 16u * v);
    }
    const rsrc_t r_p = make_rsrc(plan.ptab + (size_t)uniform(d.y) * (C::M2 * R2), uniform((d.z & 0xffu) != 0u ? (uint32_t)(C::M2 * R2 * 4) : 0u));
#pragma unroll
    for (int s = 0; s < C::KSE; ++s) o.pa[s] = __uint_as_float(buf_load1u(r_p, ((uint32_t)((4 * s + hi) * R2) + 16u * t + lo) * 4u));   // m >= q0 q1: zeros
  };
  f32x4 dp[C::MT2];
#pragma unroll
  for (int mt = 0; mt < C::MT2; ++mt) dp[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto compute = [&](const uint4& d, const Ops& o) {
    f32x4 e[QJ];   // k2 = jh QJ + j
#pragma unroll
    for (int j = 0; j < QJ; ++j) e[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < C::KSE; ++s)
#pragma unroll
      for (int j = 0; j < QJ; ++j) e[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.pa[s], f4c(o.be[s][j / 4], j % 4), e[j], 0, 0, 0);
#pragma unroll
    for (int S = 0; S < 4; ++S)
#pragma unroll
      for (int kk = 0; kk < Q2; ++kk)
#pragma unroll
        for (int mt = 0; mt < C::MT2; ++mt)
          dp[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(o.ad[S][mt][kk / 4], kk % 4), f4c(o.gb[S][kk / 4], kk % 4), dp[mt], 0, 0, 0);
    // E tile -> slab: lane (hi, lo) holds E[id lo][k2 = j][c2 = 16 t + 4 hi + {0..3}]; row of the id's i2, 16 bytes per (j, lane)
    bool todo = o.i2 < p2;
    float* const row = slab + (todo ? o.i2 : 0u) * (uint32_t)LDR + 4 * hi;
    uint32_t* const my_tag = tag + (todo ? o.i2 : 0u);
    while (__ballot(todo) != 0ull) {
      if (todo) *my_tag = (uint32_t)lo;   // (the four lane groups of an id store the same number)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const bool won = todo && *my_tag == (uint32_t)lo;
      if (won) {
#pragma unroll
        for (int j = 0; j < QJ; ++j) {
          f32x4* q = reinterpret_cast<f32x4*>(row + j * 16);
          *q = *q + e[j];
        }
      }
      todo = todo && !won;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();   // (a loser's next tag store must not overtake the winner's tag read)
    }
    if (d.z & kLastBit) {   // the group is complete: its dP columns of this tile (rows >= q0 q1 fall off the group's slot)
      const rsrc_t r_dp = make_rsrc(plan.dptab + (size_t)uniform(d.y) * (C::M2 * R2), jh == 0 ? (uint32_t)(C::M2 * R2 * 4) : 0u);   // (JS = 2: the first half's wavefront stores)
#pragma unroll
      for (int mt = 0; mt < C::MT2; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) buf_store1(r_dp, ((uint32_t)((16 * mt + 4 * hi + r) * R2) + 16u * t + lo) * 4u, dp[mt][r]);
        dp[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  if (have) {
    uint4 d0 = load_desc(ctab, c, nchunks);
    bool more1 = has_next(c, d0);
    uint4 d1 = more1 ? load_desc(ctab, c + 1u, nchunks) : none;
    bool more2 = more1 && has_next(c + 1u, d1);
    uint4 d2 = more2 ? load_desc(ctab, c + 2u, nchunks) : none;
    Ids i0 = ids_of(d0), i1 = ids_of(d1);
    Ops A, B;
    load(d0, i0, A);
    // one step: request chunk c + 1 into `nxt`, the ids of c + 2, the descriptor of c + 3; multiply chunk c out of `cur`
    auto step = [&](Ops& cur, Ops& nxt) {
      load(d1, i1, nxt);   // (an empty descriptor: every load falls off its buffer)
      const Ids i2n = ids_of(d2);
      const bool more3 = more2 && has_next(c + 2u, d2);
      const uint4 d3 = more3 ? load_desc(ctab, c + 3u, nchunks) : none;
      __builtin_amdgcn_sched_barrier(0);
      compute(d0, cur);
      __builtin_amdgcn_sched_barrier(0);
      const bool go = more1;
      ++c;
      d0 = d1; d1 = d2; d2 = d3;
      i0 = i1; i1 = i2n;
      more1 = more2; more2 = more3;
      return go;
    };
    for (;;) {
      if (!step(A, B)) break;
      if (!step(B, A)) break;
    }
  }
  // this wavefront's slice of the share's slab: [i2][kk = jh QJ ..][c2 = 16 t ..], every row written (zeros where no id came by)
  float* const out = plan.g2part + (size_t)share * p2 * C::ROW2 + 16u * t + (uint32_t)(jh * QJ * R2);
  for (uint32_t i2 = 0; i2 < p2; ++i2)
#pragma unroll
    for (int j0 = 0; j0 < QJ; j0 += 4) {
      const int j = j0 + hi;
      out[(size_t)i2 * C::ROW2 + (uint32_t)(j * R2) + lo] = slab[i2 * (uint32_t)LDR + j * 16 + lo];
    }
}

